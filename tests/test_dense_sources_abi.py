"""The C ABI of the typed dense entries (spkm_dense_assign_src_dev / spkm_dense_accumulate_src_dev: the two-pass kernels
reading a chunk in its own element type), checked without a GPU: the declarations, the argument statuses and the engine's
signatures."""
import inspect
import re

import numpy as np
import pytest
import torch

from sparsifiedkmeans_amd import _lib

ENTRIES = ("spkm_dense_assign_src_dev", "spkm_dense_accumulate_src_dev")


def test_typed_dense_entries_are_declared():
    assert set(ENTRIES) <= set(_lib.declared_symbols())
    L = _lib.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == 9, name
    txt = open(_lib.HEADER).read()
    # src_kind sits in front of the chunk, as in the typed sparsifier entries
    for name in ENTRIES:
        assert re.search(rf"int {name}\(spkm_ctx \*ctx, uint64_t p, uint64_t n, int src_kind, const void \*d_X, uint64_t K,", txt)


@pytest.mark.parametrize("kind", [0, 5, 99])
def test_a_null_context_is_refused_before_the_kind_is_looked_at(kind):
    L = _lib.lib()
    assert L.spkm_dense_assign_src_dev(None, 16, 4, kind, None, 2, None, None, None) == _lib.ERR_NULL_ARG
    assert L.spkm_dense_accumulate_src_dev(None, 16, 4, kind, None, 2, None, None, None) == _lib.ERR_NULL_ARG


def test_engine_helpers_take_typed_chunks():
    from sparsifiedkmeans_amd import engine

    for fn, names in ((engine.dense_assign_device, ["ctx", "x", "centers", "src_kind"]),
                      (engine.dense_accumulate_device, ["ctx", "x", "assign", "sums", "counts", "src_kind"])):
        params = list(inspect.signature(fn).parameters.values())
        assert [q.name for q in params] == names               # the existing arguments unchanged, the new keyword last
        assert params[-1].default is None
    # the kind of a chunk: its dtype's, float64 on the old entries, uint16 as an int16 view named explicitly
    for dt, kind in engine._WIDEN_KIND.items():
        assert engine._dense_source(torch.zeros((2, 3), dtype=dt), None)[1] == kind
    assert engine._dense_source(torch.zeros((2, 3), dtype=torch.float64), None)[1] == 0
    x, kind = engine._dense_source(torch.zeros((2, 3), dtype=torch.int16), engine.SRC_U16)
    assert kind == 8 and x.dtype == torch.int16
    if getattr(torch, "uint16", None) is not None:
        x, kind = engine._dense_source(torch.zeros((2, 3), dtype=torch.uint16), None)
        assert kind == 8 and x.dtype == torch.int16
    with pytest.raises(ValueError):
        engine._dense_source(torch.zeros((2, 3), dtype=torch.uint8), engine.SRC_U16)      # a 2-byte kind on 1-byte elements
    with pytest.raises(TypeError):
        engine._dense_source(torch.zeros((2, 3), dtype=torch.int64), None)
    assert {k: engine._KIND_BYTES[k] for k in range(9)} == {0: 8, 1: 4, 2: 1, 3: 2, 4: 4, 5: 2, 6: 2, 7: 1, 8: 2}
    sig = inspect.signature(engine.SourceChunkStager.put)
    assert list(sig.parameters) == ["self", "chunk"]


def test_driver_names_the_resident_types():
    from sparsifiedkmeans_amd import kmeans

    assert set(kmeans._DENSE_RESIDENT_NP) == {np.float32, np.float16, np.uint8, np.int8, np.int16}
    assert set(kmeans._DENSE_RESIDENT_TORCH) == {torch.float32, torch.float16, torch.bfloat16, torch.uint8, torch.int8,
                                                 torch.int16}
    assert set(kmeans._DENSE_RESIDENT_NP) < set(kmeans._KEEP_NARROW_NP)                     # uint16 stays float64-resident
