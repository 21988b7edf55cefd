"""The on-disk shard format, version 1 (sparsifiedkmeans_amd/shardfile.py): the pure-host writer, reader and validator.
No GPU: scipy CSC matrices go through a directory and come back; every refusal of the reader names the file and the field;
a committed version-1 directory (tests/golden/shard_v1) must load with exact contents, so the format cannot drift."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

from sparsifiedkmeans_amd import shardfile as SF

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shard_v1")


def _meta(p, sketch="hadamard", **kw):
    m = dict(p=p, sketch=sketch, SparsityLevel=0.05, small_p=3, gamma=3 / p, sample_seed=2**62 + 5, first=0, n_total=0,
             ColumnSamples=False, FORCE_BUG=False)
    m.update(kw)
    return m


def _csc(p2, counts, seed):
    """p2 x len(counts) CSC with ascending rows and the given column lengths"""
    rng = np.random.default_rng(seed)
    ir = np.concatenate([np.sort(rng.choice(p2, c, replace=False)) for c in counts] + [np.zeros(0, np.int64)])
    x = rng.standard_normal(ir.size)
    jc = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return sp.csc_matrix((x, ir.astype(np.int64), jc), shape=(p2, len(counts)))


CASES = {
    "fixed_s3": (64, [3] * 7),
    "fixed_s1_n1": (64, [1]),
    "ragged": (64, [2, 0, 5, 1, 9, 3]),
    "ragged_empty_first_last": (64, [0, 4, 7, 0]),
    "n1_ragged_empty": (64, [0]),
    "nnz0": (64, [0, 0, 0]),
    "wide_ids_fixed": (131072, [4] * 5),
    "wide_ids_ragged": (131072, [0, 3, 6, 0]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_write_read_validate_round_trip(tmp_path, name):
    p2, counts = CASES[name]
    Y = _csc(p2, counts, seed=len(name))
    sign = np.where(np.arange(p2) % 3 == 0, -1.0, 1.0)
    SF.write_csc(str(tmp_path / name), Y, _meta(p2 - 1, n_total=len(counts)), sign)
    sf = SF.open_shard(str(tmp_path / name))
    m = sf.meta
    fixed = len(set(counts)) == 1 and sum(counts) > 0
    assert (m["p2"], m["n"], m["nnz"]) == (p2, len(counts), sum(counts))
    assert m["s"] == (counts[0] if fixed else 0) and sf.fixed == fixed
    assert m["ir_bits"] == (16 if p2 <= 65536 else 32) and sf.ir.dtype == (np.uint16 if p2 <= 65536 else np.uint32)
    assert (sf.jc is None) == fixed and os.path.exists(tmp_path / name / "jc.npy") == (not fixed)
    assert sf.x.dtype == np.float64 and np.array_equal(sf.x, Y.data) and np.array_equal(sf.ir, Y.indices)
    if not fixed:
        assert sf.jc.dtype == np.int64 and np.array_equal(sf.jc, Y.indptr)
    assert np.array_equal(sf.sign, sign) and m["sample_seed"] == 2**62 + 5 and m["byteorder"] == "little"
    Z = sf.to_csc()
    assert Z.shape == Y.shape and np.array_equal(Z.indptr, Y.indptr) and np.array_equal(Z.indices, Y.indices)
    assert np.array_equal(Z.data, Y.data)
    for c0, c1 in ((0, len(counts)), (len(counts) // 2, len(counts))):
        assert sf.column_bounds(c0, c1) == (int(Y.indptr[c0]), int(Y.indptr[c1]))
    if sum(counts):
        assert isinstance(sf.x, np.memmap) and isinstance(sf.ir, np.memmap)      # never resident at once


def test_no_sketch_has_no_sign_file(tmp_path):
    Y = _csc(64, [3, 3], seed=1)
    SF.write_csc(str(tmp_path / "a"), Y, _meta(64, sketch="none"))
    assert not os.path.exists(tmp_path / "a" / "sign.npy") and SF.open_shard(str(tmp_path / "a")).sign is None
    with pytest.raises(ValueError, match="sign"):
        SF.write_csc(str(tmp_path / "b"), Y, _meta(64, sketch="hadamard"))
    with pytest.raises(ValueError, match="sign"):
        SF.write_csc(str(tmp_path / "c"), Y, _meta(64, sketch="none"), np.ones(64))


def test_a_directory_without_meta_is_no_shard_and_meta_comes_last(tmp_path):
    w = SF.ShardWriter(str(tmp_path / "a"), dict(_meta(64, sketch="none"), p2=64, n=2, nnz=4, s=2, ir_bits=16))
    with pytest.raises(ValueError, match="meta.json"):
        SF.open_shard(str(tmp_path / "a"))
    w.x[:] = [1.0, 2.0, 3.0, 4.0]
    w.ir[:] = [0, 5, 1, 63]
    w.close()
    assert np.array_equal(SF.open_shard(str(tmp_path / "a")).ir, [0, 5, 1, 63])


def _edit_meta(d, **kw):
    fn = os.path.join(d, "meta.json")
    with open(fn) as f:
        m = json.load(f)
    m.update(kw)
    with open(fn, "w") as f:
        json.dump(m, f)


def test_every_refusal_names_the_file_and_the_field(tmp_path):
    Y = _csc(64, [2, 0, 5, 1], seed=3)

    def fresh(name, Yc=Y):
        d = str(tmp_path / name)
        SF.write_csc(d, Yc, _meta(64, sketch="none"))
        return d

    d = fresh("version")
    _edit_meta(d, version=2)
    with pytest.raises(ValueError, match=r"meta\.json: version = 2"):
        SF.open_shard(d)
    d = fresh("format")
    _edit_meta(d, format="something else")
    with pytest.raises(ValueError, match=r"meta\.json: format"):
        SF.open_shard(d)
    d = fresh("nnz")
    _edit_meta(d, nnz=9)
    with pytest.raises(ValueError, match=r"x\.npy: shape \(8,\), meta\.json says nnz = 9"):
        SF.open_shard(d)
    d = fresh("ir_len")
    np.save(os.path.join(d, "ir.npy"), np.zeros(7, np.uint16))
    with pytest.raises(ValueError, match=r"ir\.npy: shape \(7,\), meta\.json says nnz = 8"):
        SF.open_shard(d)
    d = fresh("n")
    _edit_meta(d, n=5)
    with pytest.raises(ValueError, match=r"jc\.npy: shape \(5,\), meta\.json says n \+ 1 = 6"):
        SF.open_shard(d)
    d = fresh("ir_type")
    np.save(os.path.join(d, "ir.npy"), np.zeros(8, np.uint32))
    with pytest.raises(ValueError, match=r"ir\.npy: dtype uint32"):
        SF.open_shard(d)
    d = fresh("jc_monotone")
    np.save(os.path.join(d, "jc.npy"), np.array([0, 2, 1, 7, 8], np.int64))
    with pytest.raises(ValueError, match=r"jc\.npy: jc is not monotone: jc\[1\] = 2 > jc\[2\] = 1"):
        SF.open_shard(d)
    assert SF.open_shard(d, check=False).meta["n"] == 4                 # (lengths only: the scans are validate()'s)
    d = fresh("jc_end")
    np.save(os.path.join(d, "jc.npy"), np.array([0, 2, 2, 7, 9], np.int64))
    with pytest.raises(ValueError, match=r"jc\.npy: jc\[n\] = 9, meta\.json says nnz = 8"):
        SF.open_shard(d)
    d = fresh("jc_start")
    np.save(os.path.join(d, "jc.npy"), np.array([1, 2, 2, 7, 8], np.int64))
    with pytest.raises(ValueError, match=r"jc\.npy: jc\[0\] = 1"):
        SF.open_shard(d)
    d = fresh("row_id")
    ir = np.array(Y.indices, np.uint16)
    ir[5] = 64
    np.save(os.path.join(d, "ir.npy"), ir)
    with pytest.raises(ValueError, match=r"ir\.npy: row id ir\[5\] = 64 is not below p2 = 64"):
        SF.open_shard(d)
    d = fresh("sign_missing")
    _edit_meta(d, sketch="dct")
    with pytest.raises(ValueError, match=r"sign\.npy: missing"):
        SF.open_shard(d)
    d = fresh("fixed_nnz", _csc(64, [3, 3], seed=4))
    _edit_meta(d, s=4)
    with pytest.raises(ValueError, match=r"meta\.json: nnz = 6 is not n \* s"):
        SF.open_shard(d)
    d = fresh("field")
    with open(os.path.join(d, "meta.json")) as f:
        m = json.load(f)
    del m["gamma"]
    with open(os.path.join(d, "meta.json"), "w") as f:
        json.dump(m, f)
    with pytest.raises(ValueError, match=r"meta\.json: field 'gamma' is missing"):
        SF.open_shard(d)
    d = fresh("bits")
    _edit_meta(d, ir_bits=8)
    with pytest.raises(ValueError, match=r"meta\.json: ir_bits = 8"):
        SF.open_shard(d)
    d = fresh("order")
    _edit_meta(d, byteorder="big")
    with pytest.raises(ValueError, match=r"meta\.json: byteorder"):
        SF.open_shard(d)


def test_the_committed_version_1_directory_loads_with_exact_contents():
    """tests/golden/shard_v1: a ragged 16-row shard of 5 points written by version 1 of the writer.  Its bytes are part of
    the repository; a reader that stops understanding them has changed the format."""
    assert sorted(os.listdir(GOLDEN)) == ["ir.npy", "jc.npy", "meta.json", "sign.npy", "x.npy"]
    assert sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN)) < 2048
    sf = SF.open_shard(GOLDEN)
    assert sf.meta == {"format": "spkm-shard", "version": 1, "byteorder": "little", "p": 13, "p2": 16, "n": 5, "nnz": 9, "s": 0,
                       "ir_bits": 16, "sketch": "hadamard", "SparsityLevel": 0.2, "small_p": 3, "gamma": 3 / 13,
                       "sample_seed": 6917529027641081861, "first": 40, "n_total": 100, "ColumnSamples": False,
                       "FORCE_BUG": False}
    assert sf.jc.dtype == np.dtype("<i8") and sf.jc.tolist() == [0, 0, 3, 5, 9, 9]
    assert sf.ir.dtype == np.dtype("<u2") and sf.ir.tolist() == [1, 7, 15, 0, 2, 3, 4, 8, 12]
    assert sf.x.dtype == np.dtype("<f8") and sf.x.tolist() == [0.5, -1.25, 3.0, 2.0 ** -40, -7.0, 1e300, -1e-300, 0.1, 1 / 3]
    assert sf.sign.tolist() == [1.0, -1.0] * 8
    # ... and the writer of today produces the same settings file and the same arrays
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        meta = {k: v for k, v in sf.meta.items() if k not in ("format", "version", "byteorder")}
        w = SF.ShardWriter(d, meta, np.array(sf.sign))
        w.x[:], w.ir[:], w.jc[:] = sf.x, sf.ir, sf.jc
        w.close()
        with open(os.path.join(GOLDEN, "meta.json"), "rb") as a, open(os.path.join(d, "meta.json"), "rb") as b:
            assert a.read() == b.read()
        for f in ("x.npy", "ir.npy", "jc.npy", "sign.npy"):
            a, b = np.load(os.path.join(GOLDEN, f)), np.load(os.path.join(d, f))
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f
