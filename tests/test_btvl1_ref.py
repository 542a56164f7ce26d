"""CPU tests of BTV-L1 super-resolution: hand-computed cases of every step of the NumPy restatement (tests/btvl1_numpy_ref.py, the
yardstick of tests/test_btvl1_gpu.py), the restatement of the reference's own acceptance test, the committed fixture that pins the
restatement, and the parts of the new interface that need no device (C-ABI defaults and refusal, headers, sample)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import btvl1_numpy_ref as R  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "btvl1_24x32.npz")


# ---------------------------------------------------------------------------------------------------------------- single steps
def test_btv_weight_table_in_the_references_enumeration_order():
    # btv_l1_cuda.cpp:180-184: m = 0 .. ksize, l = ksize down to -m (NOT down to -ksize)
    assert R.btv_weight_offsets(3) == [(0, 1), (0, 0), (1, 1), (1, 0), (1, -1)]
    a = float(F(0.7))
    w3 = R.btv_weights(3, 0.7)
    assert w3.dtype == F and np.array_equal(w3, np.array([a, 1.0, a * a, a, a * a], np.float64).astype(F))
    off7 = R.btv_weight_offsets(7)
    assert len(off7) == 4 + 5 + 6 + 7 and off7[:4] == [(0, 3), (0, 2), (0, 1), (0, 0)] and off7[-7:] == [(3, l) for l in range(3, -4, -1)]
    w7 = R.btv_weights(7, 0.7)
    assert w7[3] == 1 and w7[0] == F(a ** 3) and w7[-1] == F(a ** 6) and w7[-4] == F(a ** 3)
    assert len(R.btv_weight_offsets(1)) == 1 and len(R.btv_weight_offsets(2)) == 1 and len(R.btv_weight_offsets(16)) == 92


def test_btv_term_of_a_1x5_neighbourhood_by_hand():
    # btvKernelSize 5: only the centre of a 5 x 5 image is inside the border.  Every row but the middle one equals the centre value,
    # so only the m = 0 pairs count: l = 2: sign(2 - 9) - sign(3 - 2) = -2, l = 1: sign(2 - 5) - sign(1 - 2) = 0, l = 0: 0.
    img = np.full((5, 5), 2, F)
    img[2] = [3, 1, 2, 5, 9]
    w = R.btv_weights(5, 0.7)
    reg = R.btv_regularization(img, 5, w)
    want = np.zeros((5, 5), F)
    want[2, 2] = w[0] * F(-2)
    assert w[0] == F(float(F(0.7)) ** 2) and np.array_equal(reg, want)


def test_btv_term_of_a_3x3_neighbourhood_by_hand_and_its_fourth_channel():
    img = np.array([[9, 2, 3], [4, 5, 5], [7, 1, 0]], F)
    w = R.btv_weights(3, 0.7)
    # (0,1): sign(5-5) - sign(4-5) = 1; (0,0): 0; (1,1): sign(5-0) - sign(9-5) = 0; (1,0): sign(5-1) - sign(2-5) = 2; (1,-1): sign(5-7) - sign(3-5) = 0
    want = (F(0) + w[0] * F(1)) + w[3] * F(2)
    assert R.btv_regularization(img, 3, w)[1, 1] == want
    img4 = np.stack([img, img, img, img], -1)
    reg4 = R.btv_regularization(img4, 3, w)
    assert np.all(reg4[1, 1, :3] == want) and reg4[1, 1, 3] == 0          # btv_l1_gpu.cu:157-165
    assert np.count_nonzero(reg4) == 3                                     # the border of (3 - 1) / 2 pixels stays 0
    assert np.all(R.diff_sign(img4, img4.transpose(1, 0, 2))[..., 3] == R.diff_sign(img, img.T))   # the data term: all four alike


def test_borders_reflect101_and_replicate_at_both_ends():
    assert R.reflect101([-2, -1, 0, 4, 5, 6], 5).tolist() == [2, 1, 0, 4, 3, 2]
    assert R.replicate([-2, -1, 0, 4, 5, 6], 5).tolist() == [0, 0, 0, 4, 4, 4]
    assert R.reflect101([-1, 0, 1], 1).tolist() == [0, 0, 0]
    # taps 1/4 1/2 1/4 on one row: reflect-101 takes the neighbour's mirror image at either end, sums run tap 0 first
    out = R.gauss_separable(np.array([[1, 2, 4]], F), R.gaussian_kernel(3, 0))
    assert out.tolist() == [[1.5, 2.25, 3.0]]


def test_gaussian_kernel_tables_and_computed_sigma():
    assert R.gaussian_kernel(5, 0).tolist() == [0.0625, 0.25, 0.375, 0.25, 0.0625]
    assert R.gaussian_kernel(7, 0).tolist() == [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]
    k9 = R.gaussian_kernel(9, 0)     # sigma = 0.3 (4 - 1) + 0.8 = 1.7
    assert np.array_equal(k9, R.gaussian_kernel(9, 1.7)) and abs(float(k9.sum()) - 1) < 1e-6 and k9[4] == k9.max()
    assert not np.array_equal(R.gaussian_kernel(5, 1.2), R.gaussian_kernel(5, 0))


def test_remap_truncates_toward_zero_then_clamps():
    src = np.array([[10, 20, 30]], F)
    zero = np.zeros((1, 3), F)
    assert R.remap_nearest(src, np.array([[-0.7, 1.9, 2.999]], F), zero).tolist() == [[10, 20, 30]]   # -0.7 -> -0, not -1
    assert R.remap_nearest(src, np.array([[-1.5, 0.999, 3.7]], F), zero).tolist() == [[10, 10, 30]]
    col = np.array([[1], [2], [3]], F)
    assert R.remap_nearest(col, np.zeros((3, 1), F), np.array([[-5], [1.99], [7]], F)).tolist() == [[1], [2], [3]]


def test_forward_map_is_built_from_the_backward_motion():
    one = np.ones((2, 3), F)
    fmap, bmap = R.motion_maps((1 * one, 2 * one), (3 * one, 4 * one))
    assert fmap[0].tolist() == [[3, 4, 5], [3, 4, 5]] and fmap[1].tolist() == [[4, 4, 4], [5, 5, 5]]
    assert bmap[0].tolist() == [[1, 2, 3], [1, 2, 3]] and bmap[1].tolist() == [[2, 2, 2], [3, 3, 3]]


def test_relative_motions_are_running_sums_in_the_references_order():
    c = lambda v: (np.full((1, 1), v, F), np.full((1, 1), 10 * v, F))
    fwd = [c(1), c(2), c(4), None]
    bwd = [None, c(8), c(16), c(32)]
    rf, rb = R.relative_motions(fwd, bwd, 1, (1, 1))
    assert [float(m[0][0, 0]) for m in rf] == [1, 0, 16, 48] and [float(m[1][0, 0]) for m in rf] == [10, 0, 160, 480]
    assert [float(m[0][0, 0]) for m in rb] == [8, 0, 2, 6]


def test_resize_factors_and_cubic_at_integer_positions():
    assert R.resize_scale_factor(30, 10) == F(1.0 / 3.0) and R.resize_scale_factor(10, 30) == F(3) and R.resize_scale_factor(40, 10) == F(0.25)
    a = np.random.default_rng(0).uniform(0, 255, (6, 7)).astype(F)
    up = R.resize_cubic(a, 12, 14)
    assert np.array_equal(up[::2, ::2], a)            # the cubic weights at an integer position are 0 0 1 0 0
    assert np.array_equal(R.resize_nearest(up, 6, 7), a)
    assert np.array_equal(R.upscale(a, 3)[::3, ::3], a) and np.count_nonzero(R.upscale(a, 3)) == np.count_nonzero(a)
    assert R.add_weighted(F(3), 1.0, F(2), -1.3 * 0.03, 0.0) == F(3) + F(2) * F(-1.3 * 0.03)


def test_one_frame_needs_no_motions():
    a = np.random.default_rng(1).uniform(0, 255, (10, 12)).astype(F)
    kw = dict(scale=2, iterations=3, btv_kernel_size=3)
    out = R.process([a], [None], [None], 0, **kw)
    # by hand: identity maps, so the two remaps drop out
    taps, w = R.gaussian_kernel(5, 0), R.btv_weights(3, 0.7)
    X = R.resize_cubic(a, 20, 24)
    for _ in range(3):
        d = R.gauss_separable(R.upscale(R.diff_sign(a, R.gauss_separable(X, taps)[::2, ::2]), 2), taps)
        X = R.add_weighted(X, 1.0, R.btv_regularization(X, 3, w), -1.3 * 0.03, 0.0)
        X = R.add_weighted(X, 1.0, d, 1.3, 0.0)
    assert out.shape == (14, 18) and np.array_equal(out, X[3:-3, 3:-3])


# ---------------------------------------------------------------------------------------------------------------- acceptance
@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_meets_the_references_acceptance_criterion(seed):
    """superres/test/test_superres.cpp:223-274 restated on the synthetic sequence (five frames, base in the middle, analytic motions):
    scale 2, 100 iterations; MSSIM against the undegraded base frame >= 0.5 (the reference's threshold, :273) and better than the
    cubic upscale of the degraded base frame.
    Measured, restatement on the CPU: seed 0: 0.8746 (cubic 0.7115), seed 1: 0.8760 (cubic 0.7090).
    Measured on MI355X with the product's own Farneback flows over 12 frames (tests/test_btvl1_gpu.py): 0.8215 (cubic 0.7095)."""
    gold, low, offs = R.synthetic_sequence(seed)
    fwd, bwd = R.analytic_motions(offs, low[0].shape, 2)
    out = R.process([f.astype(F) for f in low], fwd, bwd, 2, scale=2, iterations=100)
    b = R.DEFAULTS["btv_kernel_size"]
    g = gold[2][b:-b, b:-b]
    sr = R.mssim(g, R.saturate_u8(out))
    cubic = R.mssim(g, R.saturate_u8(R.resize_cubic(low[2].astype(F), *gold[2].shape))[b:-b, b:-b])
    print(f"btvl1 restatement seed {seed}: MSSIM {sr:.4f}, cubic upscale {cubic:.4f}")
    assert sr >= 0.5
    assert sr > cubic


def test_ring_driver_yields_one_output_per_frame_then_none():
    _, low, offs = R.synthetic_sequence(3, n=7, hh=48, hw=64)
    calls = []

    def flow(a, b):
        calls.append(1)
        return np.zeros(a.shape, F), np.zeros(a.shape, F)

    sr = R.BTVL1(R.ListSource(low), flow, scale=2, iterations=1, temporal_area_radius=2)
    outs = []
    while (o := sr.nextFrame()) is not None:
        outs.append(o)
    assert len(outs) == 7 and len(calls) == 12 and outs[0].dtype == np.uint8 and outs[0].shape == (48 - 14, 64 - 14)
    assert sr.nextFrame() is None


# ---------------------------------------------------------------------------------------------------------------- fixture
def test_restatement_reproduces_the_committed_fixture():
    """tests/golden/btvl1_24x32.npz (tools/make_golden_btvl1.py): three 24 x 32 frames, motions, parameters and the restatement's output
    after 5 iterations.  An edit of the restatement that changes what it computes fails here, not silently in the GPU comparison."""
    z = np.load(GOLDEN)
    kw = json.loads(str(z["params"]))
    base = kw.pop("base_idx")
    n = z["frames"].shape[0]
    fwd = [(z["fwd"][i, 0], z["fwd"][i, 1]) if i < n - 1 else None for i in range(n)]
    bwd = [(z["bwd"][i, 0], z["bwd"][i, 1]) if i > 0 else None for i in range(n)]
    out = R.process(list(z["frames"]), fwd, bwd, base, **kw)
    assert out.dtype == F and np.array_equal(out.view(np.uint32), z["out"].view(np.uint32))
    assert os.path.getsize(GOLDEN) < 176 * 1024


# ---------------------------------------------------------------------------------------------------------------- interface
def test_c_abi_declares_exports_and_defaults():
    from opencv_contrib_amd import capi
    want = {"mi_btvl1_default_params", "mi_btvl1_create", "mi_btvl1_destroy", "mi_btvl1_process", "mi_btvl1_get_profile", "mi_btvl1_stage"}
    assert want <= set(capi.declared_symbols())
    L = capi.lib()
    assert hasattr(L, "miflow_selftest_btvl1_poison")
    p = capi.BTVL1Params()
    L.mi_btvl1_default_params(C.byref(p))
    # BTVL1_CUDA_Base::BTVL1_CUDA_Base, btv_l1_cuda.cpp:280-289
    assert (p.scale, p.iterations, p.tau, p.lambda_, p.alpha, p.btv_kernel_size, p.blur_kernel_size, p.blur_sigma) == (4, 180, 1.3, 0.03, 0.7, 7, 5, 0.0)
    assert R.DEFAULTS == dict(scale=4, iterations=180, tau=1.3, lambda_=0.03, alpha=0.7, btv_kernel_size=7, blur_kernel_size=5, blur_sigma=0.0,
                              temporal_area_radius=4)


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from opencv_contrib_amd import capi, superres
    h = C.c_void_p()
    assert capi.lib().mi_btvl1_create(None, C.byref(h)) == -7 and b"no CPU fallback" in capi.lib().mi_last_error()
    with pytest.raises(capi.MiError):
        superres.createSuperResolution_BTVL1_CUDA()
    src = superres.createFrameSource_List([1, 2])
    assert (src.nextFrame(), src.nextFrame(), src.nextFrame()) == (1, 2, None)
    src.reset()
    assert src.nextFrame() == 1 and superres.createFrameSource_Empty().nextFrame() is None


def test_superres_header_conformance_and_sample_compile(tmp_path):
    """tests/cpp/superres_conformance.cpp static_asserts the signatures of include/opencv2/superres.hpp against the reference's
    declarations (superres/include/opencv2/superres.hpp:60-203); samples/super_resolution.cpp compiles against the same headers."""
    for src in (os.path.join(ROOT, "tests", "cpp", "superres_conformance.cpp"), os.path.join(ROOT, "samples", "super_resolution.cpp")):
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
