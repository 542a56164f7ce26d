"""The host side of cv::cuda::FastFeatureDetector, checked without a GPU: the plan (tests/cpp/fast_plan_test.cpp, a stand-alone program
under the host sanitizers), its constants as the GPU tests read them, and the validator through the C-ABI, which rejects before any
device call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opencv_contrib_amd", "csrc")


def plan_constants():
    """the constexpr ints of opencv_contrib_amd/csrc/fast_plan.h that are plain numbers: the GPU tests take their shapes from these"""
    txt = open(os.path.join(CSRC, "fast_plan.h")).read()
    return {k: int(v) for k, v in re.findall(r"constexpr int (FAST_\w+) = (\d+)\s*[;,]", txt)}


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fast_plan") / "fast_plan_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "fast_plan_test.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_plan_host_arithmetic(plan_exe):
    """geometry one below, at and above every tile and segment edge, the degenerate sizes, scratch bytes, the launch list of one frame
    and of a mixed batch, the validator.  Plain C++ with its own main; nothing here is loaded into Python."""
    r = subprocess.run([plan_exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fast_plan_test: ok" in r.stdout, r.stdout + r.stderr


def test_constants_read_from_the_header_are_the_compiled_ones(plan_exe):
    r = subprocess.run([plan_exe, "constants"], capture_output=True, text=True)
    k = plan_constants()
    assert [int(v) for v in r.stdout.split()] == [k["FAST_TILE_W"], k["FAST_TILE_H"], k["FAST_SEG"], 4, k["FAST_SCAN_THREADS"], 7]
    assert k["FAST_MAX_SIDE"] == 32767 and k["FAST_HALO"] == 3


# ------------------------------------------------------------------ the validator through the C-ABI, no device needed
def _mat(capi, rows, cols, type_=0, step=None, data=0x1000):
    """an mi_mat over memory that is never touched: every call here must return before it reads an image"""
    return capi.Mat(data, cols if step is None else step, rows, cols, type_)


def test_create_rejects_bad_parameters_before_it_looks_for_a_device():
    from opencv_contrib_amd import capi
    L = capi.lib()
    for th, nms, maxn in ((-1, 1, 5000), (10, 1, 0), (10, 0, -3)):
        h = C.c_void_p()
        p = capi.FastParams(th, nms, maxn)
        assert L.mi_fast_create(C.byref(p), C.byref(h)) == -1 and not h.value, (th, maxn)
        assert b"threshold" in L.mi_last_error() or b"max_npoints" in L.mi_last_error()
    h = C.c_void_p()
    assert L.mi_fast_create(C.byref(capi.FastParams(300, 1, 1)), None) == -1   # thresholds of 255 and above are legal: the null out is not


def test_defaults_equal_the_reference():
    """FastFeatureDetector::create, cudafeatures2d.hpp:434-437"""
    from opencv_contrib_amd import capi
    p = capi.FastParams()
    capi.lib().mi_fast_default_params(C.byref(p))
    assert (p.threshold, p.nonmax_suppression, p.max_npoints) == (10, 1, 5000)


BAD = [   # (what, image, mask, threshold, scores, expected status)
    ("negative threshold", (40, 140), None, -1, (40, 140, 4), -1),
    ("wrong image type", (40, 140, 5), None, 10, (40, 140, 4), -2),
    ("wrong mask type", (40, 140), (40, 140, 5), 10, (40, 140, 4), -2),
    ("mask size", (40, 140), (40, 139), 10, (40, 140, 4), -3),
    ("mask size", (40, 140), (39, 140), 10, (40, 140, 4), -3),
    ("rows above short2", (32768, 8), None, 10, (32768, 8, 4), -3),
    ("cols above short2", (8, 32768), None, 10, (8, 32768, 4), -3),
    ("scores type", (40, 140), None, 10, (40, 140, 5), -2),
    ("scores size", (40, 140), None, 10, (40, 141, 4), -3),
]


@pytest.mark.parametrize("what,img,mask,th,scores,want", BAD, ids=[f"{i}-{b[0].replace(' ', '_')}" for i, b in enumerate(BAD)])
def test_stage_entry_rejects_before_any_device_call(what, img, mask, th, scores, want):
    """mi_fast_score has no handle, so its validator runs on a machine without a GPU; the pointers are never read"""
    from opencv_contrib_amd import capi
    L = capi.lib()
    mi = _mat(capi, *img)
    mm = C.byref(_mat(capi, *mask)) if mask is not None else None
    ms = _mat(capi, scores[0], scores[1], scores[2], step=scores[1] * 4)
    assert L.mi_fast_score(C.byref(mi), mm, th, C.byref(ms), None) == want, (what, L.mi_last_error())


def test_python_mirror_rejects_before_the_library():
    from opencv_contrib_amd import capi, cuda
    with pytest.raises(capi.MiError) as e:
        cuda.FastFeatureDetector.create(type=cuda.FastFeatureDetector.TYPE_7_12)   # fast.cpp:213
    assert e.value.code == -1
    for kw in (dict(threshold=-1), dict(max_npoints=0)):
        with pytest.raises(capi.MiError) as e:
            cuda.FastFeatureDetector.create(**kw)
        assert e.value.code == -1, kw     # -1 also without a GPU: the validator runs first (a GPU-less machine would say -7 otherwise)


def test_convert_of_a_host_matrix():
    """convert accepts a host matrix, asserts 2 rows of 4-byte elements (fast.cpp:193-194) and gives size 7, angle -1"""
    import fast_numpy_ref as R
    from opencv_contrib_amd import capi, cuda
    loc = np.array([[5, 9], [300, 4], [32767, 32766]], np.int16)
    resp = np.array([11, 0, 254], np.float32)
    mat = R.pack(loc, resp)
    want = [(5.0, 9.0, 7.0, -1.0, 11.0), (300.0, 4.0, 7.0, -1.0, 0.0), (32767.0, 32766.0, 7.0, -1.0, 254.0)]
    assert cuda.FastFeatureDetector.convert(mat) == want == R.convert(mat)
    assert cuda.FastFeatureDetector.convert(mat.view(np.int32)) == want          # elemSize() == 4 is all the reference asks
    assert cuda.FastFeatureDetector.convert(np.zeros((2, 0), np.float32)) == []
    for bad in (np.zeros((3, 4), np.float32), np.zeros((2, 4), np.float64), np.zeros((2, 4), np.uint8)):
        with pytest.raises(capi.MiError):
            cuda.FastFeatureDetector.convert(bad)
