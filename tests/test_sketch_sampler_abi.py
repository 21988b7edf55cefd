"""The C ABI of the DCT / no-sketch sparsifier, checked without a GPU: declarations, constants and argument statuses."""
import re

from sparsifiedkmeans_amd import _lib


def test_sketch_sampler_is_declared_with_its_kinds():
    txt = open(_lib.HEADER).read()
    assert re.search(r"#define SPKM_SKETCH_NONE 0\b", txt) and re.search(r"#define SPKM_SKETCH_DCT 1\b", txt)
    assert {"spkm_sketch_sample_dev", "spkm_sketch_sample_rec_dev"} <= set(_lib.declared_symbols())
    from sparsifiedkmeans_amd.engine import SKETCH_KIND

    assert SKETCH_KIND == {"none": 0, "dct": 1}


def test_sketch_sampler_null_arguments_without_gpu():
    L = _lib.lib()
    assert L.spkm_sketch_sample_dev(None, 1, 100, 1, None, None, 1.0, 5, 0, 0, None, 16, None) == _lib.ERR_NULL_ARG
    assert L.spkm_sketch_sample_rec_dev(None, 0, 100, 1, None, None, 1.0, 5, 0, 0, 16, None) == _lib.ERR_NULL_ARG
