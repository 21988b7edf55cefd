"""CPU: the compile-time check behind spkm_launch (sparsifiedkmeans_amd/csrc/launch.h) and the pointer types of the four
screen kernel families.  Compiling tests/native/launch_harness.cpp with g++ IS most of the test: its static_asserts hold
spkm_launch_ok to what it must accept (an exact match, nullptr for a pointer, a non-const pointer for a const one, int for
int) and reject (an argument too few or too many, float* for const int*, a pointer for an int, k_screen_quad's 22-entry
list against k_screen_tile's 12 parameters).  The harness then exports each pointer type's parameter count, which is
checked against the kernel definitions themselves, parsed from the sources."""
import ctypes as C
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "sparsifiedkmeans_amd", "csrc")
# family -> (index in the harness, the file that defines the kernel, its parameter count)
FAMILIES = {
    "k_screen_quad": (0, "screen_quad.hip", 22),
    "k_screen_tile": (1, "screen.hip", 12),
    "k_screen_wide": (2, "screen_wide.hip", 15),
    "k_screen_far": (3, "screen_far.hip", 13),
}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("launch") / "liblaunch.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(HERE, "native", "launch_harness.cpp"), "-o", so])
    return C.CDLL(so)


def defined_params(kernel, fname):
    """Parameters of the __global__ definition of `kernel`: the top-level commas of its parameter list, comments dropped."""
    src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, fname)).read())
    m = re.search(r"__global__[^\n;{]*\bvoid " + kernel + r"\(", src)
    assert m, f"{kernel}: no definition in {fname}"
    depth, commas, i = 1, 0, m.end()
    while depth:
        c = src[i]
        depth += (c == "(") - (c == ")")
        commas += c == "," and depth == 1
        i += 1
    assert src[i:].lstrip().startswith("{"), f"{kernel}: a declaration, not the definition"
    return commas + 1


@pytest.mark.parametrize("kernel", sorted(FAMILIES))
def test_pointer_type_has_the_kernels_parameter_count(harness, kernel):
    family, fname, count = FAMILIES[kernel]
    assert harness.launch_arity(family) == count
    assert defined_params(kernel, fname) == count


def test_unknown_family(harness):
    assert harness.launch_arity(4) == -1
