"""cv::cuda::ORB's C-ABI and its C++ and Python mirrors: exports, defaults, the validator (which rejects before any device call), the host
entries, and the drop-in header compiled against caller code.  Only the last test needs a GPU."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orb_numpy_ref as R  # noqa: E402

LIBDIR = os.path.join(ROOT, "opencv_contrib_amd")
EXPORTS = ["mi_orb_default_params", "mi_orb_create", "mi_orb_set_params", "mi_orb_get_params", "mi_orb_destroy", "mi_orb_scratch_bytes",
           "mi_orb_pattern_source", "mi_orb_reach", "mi_orb_make_pattern", "mi_orb_features_per_level", "mi_orb_u_max",
           "mi_orb_detect_and_compute", "mi_orb_pyramid_level", "mi_orb_cull", "mi_orb_harris", "mi_orb_angle", "mi_orb_blur", "mi_orb_descriptors"]


def test_exports_are_declared_and_present():
    from opencv_contrib_amd import capi
    L = C.CDLL(capi.LIB_PATH)
    declared = set(capi.declared_symbols())
    for s in EXPORTS:
        assert s in declared and hasattr(L, s), s
    assert hasattr(capi.lib(), "mi_orb_create")


def test_defaults_equal_the_reference():
    """cv::cuda::ORB::create, cudafeatures2d.hpp:463-472"""
    from opencv_contrib_amd import capi
    p = capi.OrbParams()
    capi.lib().mi_orb_default_params(C.byref(p))
    got = (p.nfeatures, p.scale_factor, p.nlevels, p.edge_threshold, p.first_level, p.wta_k, p.score_type, p.patch_size, p.fast_threshold,
           p.blur_for_descriptor)
    assert got == (500, float(np.float32(1.2)), 8, 31, 0, 2, 0, 31, 20, 0)
    d = R.DEFAULTS
    assert got == (d["nfeatures"], float(np.float32(d["scaleFactor"])), d["nlevels"], d["edgeThreshold"], d["firstLevel"], d["WTA_K"], d["scoreType"],
                   d["patchSize"], d["fastThreshold"], int(d["blurForDescriptor"]))


BAD = [dict(patch_size=1), dict(patch_size=60), dict(wta_k=5), dict(wta_k=1), dict(nlevels=0), dict(nlevels=33), dict(scale_factor=1.0),
       dict(nfeatures=-1), dict(score_type=2), dict(fast_threshold=-1), dict(edge_threshold=-1), dict(first_level=-1)]


@pytest.mark.parametrize("kw", BAD, ids=[f"{k}={v}" for b in BAD for k, v in b.items()])
def test_create_rejects_bad_parameters_before_it_looks_for_a_device(kw):
    from opencv_contrib_amd import capi
    p = capi.OrbParams()
    capi.lib().mi_orb_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    h = C.c_void_p()
    assert capi.lib().mi_orb_create(C.byref(p), None, C.byref(h)) == -1 and not h.value, capi.lib().mi_last_error()


def test_create_rejects_a_bad_pool_before_it_looks_for_a_device():
    from opencv_contrib_amd import capi
    L = capi.lib()
    pool = np.zeros((512, 2), np.int32)
    h = C.c_void_p()
    for rows, cols, type_, want in ((511, 2, capi.MI_32SC1, -3), (512, 3, capi.MI_32SC1, -3), (512, 2, capi.MI_32FC1, -2)):
        m = capi.Mat(pool.ctypes.data, 8, rows, cols, type_)
        assert L.mi_orb_create(None, C.byref(m), C.byref(h)) == want and not h.value
    assert L.mi_orb_create(None, C.byref(capi.Mat(None, 8, 512, 2, capi.MI_32SC1)), C.byref(h)) == -1
    assert L.mi_orb_create(None, None, None) == -1


def test_host_entries_equal_the_restatement():
    """mi_orb_make_pattern, mi_orb_features_per_level, mi_orb_u_max: host arithmetic, no device"""
    from opencv_contrib_amd import cuda
    pool = np.stack([np.arange(512) % 27 - 13, np.arange(512) % 23 - 11], 1).astype(np.int32)
    for wta in (2, 3, 4):
        for patch, p0 in ((31, None), (17, None), (31, pool)):
            np.testing.assert_array_equal(cuda.orb_make_pattern(patch, wta, p0), R.make_pattern(patch, wta, p0))
    np.testing.assert_array_equal(cuda.orb_make_pattern(31, 2, pool), pool.T)
    # ... and the reference's own: what its constructor uploads for patch 31, its quotas and u_max (tests/golden/orb_refhost.npz)
    import test_orb_ref as T
    for wta in (2, 3, 4):
        np.testing.assert_array_equal(cuda.orb_make_pattern(31, wta, T.POOL31), T.HOST[f"pattern_p31_wta{wta}"])
    assert cuda.orb_features_per_level(500, 1.2, 8) == T.HOST["quota_0"].tolist() and cuda.orb_features_per_level(1, 1.2, 2) == [1, 0]
    for patch in (2, 3, 9, 29, 31, 59):
        assert cuda.orb_u_max(patch) == T.HOST[f"u_max_{patch}"].tolist()
    for n, s, L in ((500, 1.2, 8), (4000, 1.2, 8), (1, 1.2, 2), (77, 1.7, 5)):
        assert cuda.orb_features_per_level(n, s, L) == R.features_per_level(n, s, L)
    for patch in (2, 9, 31, 59):
        assert cuda.orb_u_max(patch) == R.u_max(patch)
    with pytest.raises(cuda.MiError):
        cuda.orb_make_pattern(31, 5)
    with pytest.raises(cuda.MiError):
        cuda.orb_u_max(60)


def test_python_mirror_constants_and_convert():
    from opencv_contrib_amd import cuda
    O = cuda.ORB
    assert (O.X_ROW, O.Y_ROW, O.RESPONSE_ROW, O.ANGLE_ROW, O.OCTAVE_ROW, O.SIZE_ROW, O.ROWS_COUNT) == (0, 1, 2, 3, 4, 5, 6)
    assert (O.HARRIS_SCORE, O.FAST_SCORE, O.kBytes, O.NORM_HAMMING) == (0, 1, 32, cuda.NORM_HAMMING)
    k = np.array([[10.5, 3], [20, 4], [0.25, -1], [90, 359.5], [0, 2], [31, 44.64]], np.float32)
    assert O.convert(k) == [(10.5, 20.0, 31.0, 90.0, 0.25, 0), (3.0, 4.0, float(np.float32(44.64)), 359.5, -1.0, 2)]
    assert O.convert(np.zeros((6, 0), np.float32)) == []
    for bad in (np.zeros((5, 3), np.float32), np.zeros((6, 3), np.float64)):
        with pytest.raises(cuda.MiError):
            O.convert(bad)
    for kw in (dict(WTA_K=5), dict(patchSize=1), dict(nlevels=0)):
        with pytest.raises(cuda.MiError) as e:
            O.create(**kw)
        assert e.value.code == -1, kw   # -1 also without a GPU: the validator runs first


def build_shim(tmp_path):
    exe = str(tmp_path / "orb_shim")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "orb_shim.cpp"),
                        "-o", exe, "-L" + LIBDIR, "-lmiflow", "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_cpp_mirror_compiles_and_fails_loudly_without_gpu(tmp_path):
    """caller code against cudafeatures2d.hpp's ORB compiles (signatures and constants are static asserts in it); the reference's two
    constructor asserts need no device; creating the object without one throws"""
    import torch
    exe = build_shim(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 3 and "no CPU fallback" in r.stderr, (r.returncode, r.stderr)


@pytest.mark.gpu
def test_cpp_mirror_equals_the_restatement(tmp_path):
    from test_orb_gpu import corners_image
    img = corners_image(97, 131, 21)
    exe = build_shim(tmp_path)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("4i", 97, 131, 60, 2) + img.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = open(fout, "rb").read()
    n = struct.unpack("i", raw[:4])[0]
    want = R.detect_and_compute(img, nfeatures=60, nlevels=2)
    assert n == want["keypoints"].shape[1] > 0
    mat = np.frombuffer(raw, np.float32, 6 * n, 4).reshape(6, n)
    desc = np.frombuffer(raw, np.uint8, 32 * n, 4 + 24 * n).reshape(n, 32)
    conv = np.frombuffer(raw, np.float32, 6 * n, 4 + 56 * n).reshape(n, 6)
    np.testing.assert_array_equal(mat.view(np.uint32), want["keypoints"].view(np.uint32))
    np.testing.assert_array_equal(desc, want["descriptors"])
    np.testing.assert_array_equal(conv, want["keypoints"][[0, 1, 5, 3, 2, 4]].T)
