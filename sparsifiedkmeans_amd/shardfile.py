"""A sparsified shard on disk, format version 1: a directory that numpy alone can read.

    meta.json   settings only: format / version, p, p2, n, nnz, s (0 = ragged), ir_bits, the sketch kind, SparsityLevel as
                given, small_p, gamma, sample_seed, first, n_total, ColumnSamples, FORCE_BUG, byteorder ("little")
    sign.npy    float64 [p2]: the sketch's sign vector (absent for sketch "none")
    x.npy       float64 [nnz]: the stored values, column after column, in the order of the points
    ir.npy      uint16 (ir_bits 16) or uint32 (ir_bits 32) [nnz]: their row ids, each < p2
    jc.npy      int64 [n + 1]: column starts, jc[0] = 0, jc[n] = nnz -- RAGGED shards only (s = 0); a fixed-stride shard's
                column i is entries [i * s, (i + 1) * s)

Every array is little-endian and written through ``np.lib.format.open_memmap``, so that a shard larger than the host's
memory is written and read chunk by chunk; ``meta.json`` is written LAST, so a directory a writer did not finish does not
open.  This module is the pure-host half (reader, writer, validator): it imports neither torch nor the library, and the
device half (engine.save_shard / load_shard) streams through the arrays it hands out."""
from __future__ import annotations

import json
import os

import numpy as np

FORMAT = "spkm-shard"
VERSION = 1
META_FIELDS = ("p", "p2", "n", "nnz", "s", "ir_bits", "sketch", "SparsityLevel", "small_p", "gamma", "sample_seed", "first",
               "n_total", "ColumnSamples", "FORCE_BUG")
_INT_FIELDS = ("p", "p2", "n", "nnz", "s", "ir_bits", "small_p", "sample_seed", "first", "n_total")
SKETCHES = ("hadamard", "dct", "none")
_SCAN = 1 << 22     # entries per step of the validator's scans


def ir_dtype(ir_bits: int) -> np.dtype:
    if ir_bits not in (16, 32):
        raise ValueError(f"meta.json: ir_bits = {ir_bits!r}, expected 16 or 32")
    return np.dtype("<u2" if ir_bits == 16 else "<u4")


def _create(fn: str, dtype, count: int) -> np.ndarray:
    """a new .npy of ``count`` elements to be filled in place (an empty one cannot be mapped: it is written at once)"""
    if count == 0:
        np.save(fn, np.zeros(0, dtype))
        return np.zeros(0, dtype)
    return np.lib.format.open_memmap(fn, mode="w+", dtype=np.dtype(dtype), shape=(int(count),))


def _open(fn: str) -> np.ndarray:
    if not os.path.exists(fn):
        raise ValueError(f"{os.path.basename(fn)}: missing from {os.path.dirname(fn)}")
    try:
        return np.load(fn, mmap_mode="r", allow_pickle=False)
    except ValueError:
        return np.load(fn, allow_pickle=False)              # (an array of no elements)


def check_meta(meta: dict) -> dict:
    """``meta`` with every field of version 1 present and sane -- ValueError naming meta.json and the field otherwise"""
    if meta.get("format") != FORMAT:
        raise ValueError(f"meta.json: format = {meta.get('format')!r}, expected {FORMAT!r}")
    if meta.get("version") != VERSION:
        raise ValueError(f"meta.json: version = {meta.get('version')!r}; this reader knows version {VERSION}")
    for k in META_FIELDS:
        if k not in meta:
            raise ValueError(f"meta.json: field {k!r} is missing")
    for k in _INT_FIELDS:
        if isinstance(meta[k], bool) or not isinstance(meta[k], int) or meta[k] < 0:
            raise ValueError(f"meta.json: {k} = {meta[k]!r}, expected a non-negative integer")
    if meta.get("byteorder", "little") != "little":
        raise ValueError(f"meta.json: byteorder = {meta['byteorder']!r}; version 1 is little-endian")
    if meta["sketch"] not in SKETCHES:
        raise ValueError(f"meta.json: sketch = {meta['sketch']!r}, expected one of {SKETCHES}")
    ir_dtype(meta["ir_bits"])
    if meta["p"] < 1 or meta["p2"] < meta["p"]:
        raise ValueError(f"meta.json: p = {meta['p']}, p2 = {meta['p2']}: expected 1 <= p <= p2")
    if meta["ir_bits"] == 16 and meta["p2"] > 65536:
        raise ValueError(f"meta.json: ir_bits = 16 cannot name the rows of p2 = {meta['p2']}")
    if meta["s"] > 0 and meta["nnz"] != meta["n"] * meta["s"]:
        raise ValueError(f"meta.json: nnz = {meta['nnz']} is not n * s = {meta['n']} * {meta['s']}")
    return meta


class ShardFile:
    """An opened shard directory: ``meta`` (dict) and the arrays ``x``, ``ir``, ``jc`` (None: fixed stride), ``sign``
    (None: no sketch), memory-mapped read-only."""

    def __init__(self, path, meta, x, ir, jc, sign):
        self.path, self.meta, self.x, self.ir, self.jc, self.sign = path, meta, x, ir, jc, sign

    @property
    def fixed(self) -> bool:
        return self.meta["s"] > 0

    def column_bounds(self, c0: int, c1: int) -> tuple[int, int]:
        """entries [j0, j1) of columns [c0, c1)"""
        if self.fixed:
            return c0 * self.meta["s"], c1 * self.meta["s"]
        return int(self.jc[c0]), int(self.jc[c1])

    def to_csc(self):
        """the shard as a scipy CSC matrix p2 x n (small shards: tests, inspection)"""
        import scipy.sparse as sp

        m = self.meta
        jc = np.arange(m["n"] + 1, dtype=np.int64) * m["s"] if self.fixed else np.asarray(self.jc)
        return sp.csc_matrix((np.array(self.x), np.array(self.ir, dtype=np.int64), jc), shape=(m["p2"], m["n"]))


class ShardWriter:
    """Creates the directory and its arrays for a shard described by ``meta`` (every field of META_FIELDS); the caller fills
    ``x``, ``ir`` and, for a ragged shard (s = 0), ``jc`` in place -- chunk by chunk -- and calls close(), which flushes them
    and writes meta.json."""

    def __init__(self, path: str, meta: dict, sign=None):
        meta = dict(meta, format=FORMAT, version=VERSION, byteorder="little")
        self.meta = check_meta(meta)
        if (meta["sketch"] == "none") != (sign is None):
            raise ValueError("sign.npy: a sign vector belongs to the sketches 'hadamard' and 'dct', and to those alone")
        self.path = str(path)
        os.makedirs(self.path, exist_ok=True)
        stale = os.path.join(self.path, "meta.json")
        if os.path.exists(stale):
            os.remove(stale)                                    # (the directory is no shard until close())
        if sign is not None:
            sign = np.ascontiguousarray(sign, dtype="<f8").ravel()
            if sign.size != meta["p2"]:
                raise ValueError(f"sign.npy: {sign.size} elements, meta.json says p2 = {meta['p2']}")
            np.save(os.path.join(self.path, "sign.npy"), sign)
        elif os.path.exists(os.path.join(self.path, "sign.npy")):
            os.remove(os.path.join(self.path, "sign.npy"))
        self.x = _create(os.path.join(self.path, "x.npy"), "<f8", meta["nnz"])
        self.ir = _create(os.path.join(self.path, "ir.npy"), ir_dtype(meta["ir_bits"]), meta["nnz"])
        self.jc = None
        if meta["s"] == 0:
            self.jc = _create(os.path.join(self.path, "jc.npy"), "<i8", meta["n"] + 1)
        elif os.path.exists(os.path.join(self.path, "jc.npy")):
            os.remove(os.path.join(self.path, "jc.npy"))

    def close(self) -> None:
        for a in (self.x, self.ir, self.jc):
            if isinstance(a, np.memmap):
                a.flush()
        self.x = self.ir = self.jc = None
        tmp = os.path.join(self.path, "meta.json.tmp")
        with open(tmp, "w") as f:
            json.dump(self.meta, f, indent=1, sort_keys=True)
            f.write("\n")
        os.replace(tmp, os.path.join(self.path, "meta.json"))


def write_csc(path: str, Y, meta: dict, sign=None) -> None:
    """Write the scipy sparse matrix ``Y`` (p2 x n) as a shard.  ``meta`` supplies the settings; p2, n, nnz, s and -- unless
    given -- ir_bits are taken from Y: s = the common column length, 0 (ragged) if the columns differ or there are none."""
    Y = Y.tocsc()
    Y.sort_indices()
    p2, n = Y.shape
    cnt = np.diff(Y.indptr)
    s = int(cnt[0]) if n > 0 and Y.nnz > 0 and bool(np.all(cnt == cnt[0])) else 0
    meta = dict(meta, p2=int(p2), n=int(n), nnz=int(Y.nnz), s=s)
    meta.setdefault("ir_bits", 16 if p2 <= 65536 else 32)
    w = ShardWriter(path, meta, sign)
    w.x[:] = Y.data
    w.ir[:] = Y.indices
    if w.jc is not None:
        w.jc[:] = Y.indptr
    w.close()


def validate(sf: ShardFile) -> None:
    """Everything the arrays must satisfy beyond their lengths: jc starts at 0, never decreases and ends at nnz; every row
    id is below p2.  Scans in steps, so a memory-mapped shard is never resident.  ValueError names the file and the field."""
    m = sf.meta
    if sf.jc is not None:
        if int(sf.jc[0]) != 0:
            raise ValueError(f"jc.npy: jc[0] = {int(sf.jc[0])}, expected 0")
        if int(sf.jc[-1]) != m["nnz"]:
            raise ValueError(f"jc.npy: jc[n] = {int(sf.jc[-1])}, meta.json says nnz = {m['nnz']}")
        for a in range(0, m["n"], _SCAN):
            blk = np.asarray(sf.jc[a:a + _SCAN + 1])
            d = np.diff(blk)
            if d.size and d.min() < 0:
                bad = np.flatnonzero(d < 0)
                i = a + int(bad[0])
                raise ValueError(f"jc.npy: jc is not monotone: jc[{i}] = {int(blk[bad[0]])} > jc[{i + 1}] = {int(blk[bad[0] + 1])}")
    for a in range(0, m["nnz"], _SCAN):
        blk = np.asarray(sf.ir[a:a + _SCAN])
        if blk.max() >= m["p2"]:                       # (one reduction per step; the place is looked for only when there is one)
            bad = np.flatnonzero(blk >= m["p2"])
            raise ValueError(f"ir.npy: row id ir[{a + int(bad[0])}] = {int(blk[bad[0]])} is not below p2 = {m['p2']}")


def open_shard(path: str, check: bool = True) -> ShardFile:
    """Open a shard directory: meta.json checked, the arrays memory-mapped and their types and lengths held against
    meta.json; ``check`` also runs validate() (one scan of jc and ir)."""
    path = str(path)
    fn = os.path.join(path, "meta.json")
    if not os.path.exists(fn):
        raise ValueError(f"meta.json: missing from {path} (not a shard, or a writer did not finish)")
    with open(fn) as f:
        meta = check_meta(json.load(f))

    def arr(name, dtype, count, field):
        a = _open(os.path.join(path, name))
        if a.dtype != np.dtype(dtype):
            raise ValueError(f"{name}: dtype {a.dtype}, expected {np.dtype(dtype)} (ir_bits = {meta['ir_bits']}, little-endian)")
        if a.ndim != 1 or a.shape[0] != count:
            raise ValueError(f"{name}: shape {a.shape}, meta.json says {field} = {count}")
        return a

    x = arr("x.npy", "<f8", meta["nnz"], "nnz")
    ir = arr("ir.npy", ir_dtype(meta["ir_bits"]), meta["nnz"], "nnz")
    jc = arr("jc.npy", "<i8", meta["n"] + 1, "n + 1") if meta["s"] == 0 else None
    sign = arr("sign.npy", "<f8", meta["p2"], "p2") if meta["sketch"] != "none" else None
    sf = ShardFile(path, meta, x, ir, jc, sign)
    if check:
        validate(sf)
    return sf
