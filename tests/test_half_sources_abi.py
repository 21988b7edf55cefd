"""The C ABI of the typed-source sparsifier (float16 / bfloat16 / int8 / uint16 sources, spkm_mix_sample_src_dev), checked
without a GPU: the source kinds, the declarations and the argument statuses."""
import inspect
import re

import torch

from sparsifiedkmeans_amd import _lib

KINDS = {"F64": 0, "F32": 1, "U8": 2, "I16": 3, "I32": 4, "F16": 5, "BF16": 6, "I8": 7, "U16": 8}


def test_header_names_the_source_kinds():
    txt = open(_lib.HEADER).read()
    for name, num in KINDS.items():
        assert re.search(rf"#define SPKM_SRC_{name} {num}\b", txt), name


def test_engine_maps_the_new_dtypes():
    from sparsifiedkmeans_amd import engine

    assert engine._WIDEN_KIND[torch.float16] == 5 and engine._WIDEN_KIND[torch.bfloat16] == 6
    assert engine._WIDEN_KIND[torch.int8] == 7
    assert {engine._WIDEN_KIND[t] for t in (torch.float32, torch.uint8, torch.int16, torch.int32)} == {1, 2, 3, 4}
    assert engine.SRC_U16 == 8 and getattr(torch, "uint16", None) not in engine._WIDEN_KIND
    # the existing signature is unchanged and the new keyword comes last, on by default
    params = list(inspect.signature(engine.StreamingSparsifier.__init__).parameters.values())
    assert [q.name for q in params] == ["self", "ctx", "p", "n_local", "s", "seed", "sign", "first", "sketch", "layout",
                                        "kind", "fused_source"]
    assert params[-1].default is True


def test_typed_entries_are_declared_and_refuse_a_null_context():
    assert {"spkm_mix_sample_src_dev", "spkm_mix_sample_rec_src_dev"} <= set(_lib.declared_symbols())
    L = _lib.lib()
    assert len(L.spkm_mix_sample_src_dev.argtypes) == 15 and len(L.spkm_mix_sample_rec_src_dev.argtypes) == 14
    for kind in (0, 5, 6, 99):
        assert L.spkm_mix_sample_src_dev(None, 100, 128, 1, kind, None, None, 1.0, 1.0, 5, 0, 0, None, 16,
                                         None) == _lib.ERR_NULL_ARG
        assert L.spkm_mix_sample_rec_src_dev(None, 100, 128, 1, kind, None, None, 1.0, 1.0, 5, 0, 0, 16,
                                             None) == _lib.ERR_NULL_ARG
    assert L.spkm_widen_f64_dev(None, 5, 0, None, None) == _lib.ERR_NULL_ARG
