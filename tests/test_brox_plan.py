"""The host side of cv::cuda::BroxOpticalFlow, checked without a GPU: the plan (tests/cpp/brox_plan_test.cpp, a stand-alone program built
with -Wall -Werror, with and without the host sanitizers) and its constants as the GPU tests read them."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opencv_contrib_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import brox_numpy_ref as R  # noqa: E402


def plan_constants():
    """the enumerators of opencv_contrib_amd/csrc/brox_plan.h that are plain numbers: the GPU tests take their shapes from these"""
    txt = open(os.path.join(CSRC, "brox_plan.h")).read()
    return {n: int(v) for n, v in re.findall(r"\b(BROX_\w+) = (\d+)\b(?! \*| <<)", txt)}


SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module", params=["sanitized", "plain"])
def plan_exe(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("brox_plan") / ("brox_plan_test_" + request.param))
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off"] + (SANITIZE if request.param == "sanitized" else []) +
                       ["-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "brox_plan_test.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_plan_host_arithmetic(plan_exe):
    """validation, the level rule, the scratch layout and the launch list of both solver forms.  Plain C++ with its own main; nothing
    here is loaded into Python."""
    r = subprocess.run([plan_exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "brox_plan_test: ok" in r.stdout, r.stdout + r.stderr


def test_constants_read_from_the_header_are_the_compiled_ones(plan_exe):
    r = subprocess.run([plan_exe, "constants"], capture_output=True, text=True)
    k = plan_constants()
    got = [int(v) for v in r.stdout.split()]
    assert got[:3] == [k["BROX_SOR_TILE_X"], k["BROX_SOR_TILE_Y"], k["BROX_SOR_KMAX"]] and got[3] == 2 * k["BROX_SOR_KMAX"]
    assert got[4] == k["BROX_MIN_SIDE"] == 4 and got[5] == 22


def levels_of(exe, w, h, sf, outer):
    r = subprocess.run([exe, "levels", str(w), str(h), repr(sf), str(outer)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]


def test_level_sizes_equal_the_recorded_ones(plan_exe):
    """every class fixture holds the sizes the reference's host function gave its textures; among them a pyramid that outer_iterations
    cuts (0.95, 5 levels) and pyramids the 15-pixel rule ends"""
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "brox_refclass_*.npz")))
    assert len(files) == 8
    cut = ended = 0
    for path in files:
        z = np.load(path)
        rows, cols = z["I0"].shape
        sf, outer = float(z["fparams"][2]), int(z["iparams"][1])
        want = [tuple(int(v) for v in s) for s in z["levels"]]
        assert levels_of(plan_exe, cols, rows, sf, outer) == want, path
        cut += len(want) == outer and min(want[-1]) > 15
        ended += len(want) < outer
    assert cut >= 1 and ended >= 4


def test_a_pyramid_with_a_level_of_one_pixel_is_refused():
    """16 x 16 with scale_factor 0.05: the second level would be 1 x 1, where the derivative filter's two-step mirror leaves the plane.
    Through the host-only plan entry of the library, which needs no device; 0.15 gives 3 x 3 and is planned"""
    import ctypes as C
    from opencv_contrib_amd import capi, cuda
    with pytest.raises(capi.MiError) as e:
        cuda.brox_plan_info(16, 16, scale_factor=0.05)
    assert e.value.code == -1 and "side of 1" in str(e.value)
    for rows, cols in ((16, 400), (400, 16)):
        with pytest.raises(capi.MiError) as e:
            cuda.brox_plan_info(rows, cols, scale_factor=0.06)   # ceil(16 * 0.06) = 1 on the short side only
        assert e.value.code == -1
    assert cuda.brox_plan_info(16, 16, scale_factor=0.15, inner_iterations=2, solver_iterations=3) == (2, 1 + 1 + 2 * (3 + 2 * (2 + 6) + 1), 2 * 2 * 6)
    assert cuda.brox_plan_info(16, 16, 2, scale_factor=0.15, inner_iterations=2, solver_iterations=3)[2] == 2 * 2 * 2
    with pytest.raises(capi.MiError):
        cuda.brox_plan_info(3, 16)
    n = C.c_int()
    assert capi.lib().mi_brox_plan_info(None, 16, 16, 0, C.byref(n), C.byref(n), C.byref(n)) == -1


@pytest.mark.parametrize("sf", [0.5, 0.8, 0.95])
def test_level_sizes_equal_the_restatement(plan_exe, sf):
    """sizes x scale factors; the restatement's rule is pinned on the recorded sizes above"""
    for w, h in ((16, 16), (15, 90), (37, 70), (640, 480), (1920, 1080), (1380, 1000), (101, 77)):
        for outer in (1, 3, 150):
            assert levels_of(plan_exe, w, h, sf, outer) == R.level_sizes(w, h, sf, outer), (w, h, sf, outer)
