"""PINNING, part 3: the NumPy restatement of BTV-L1 super-resolution (tests/btvl1_numpy_ref.py, the yardstick of tests/test_btvl1_gpu.py)
against the reference's OWN sources, executed here on the CPU.

oracle/_ref/libref_cu.so (oracle/Makefile.ref) holds, on the fiber shim: superres/src/cuda/btv_l1_gpu.cu whole; the separable filter
through cudafilters/src/cuda/{row,column}_filter.32fc{1,3,4}.cu whole (the cc >= 20 tiles, shared memory, __syncthreads, at_low /
at_high halos); of cudawarping/src/cuda/resize.cu and remap.cu the kernels resize_nearest / resize / remap with their launch wrappers;
the functors of cudaarithm's add_weighted.cu / mul_scalar.cu / add_mat.cu.  Compiled verbatim on the host side: superres/src/
btv_l1_cuda.cpp (calcRelativeMotions, upscaleMotions, calcBtvWeights, process, the BTVL1_CUDA ring driver), super_resolution.cpp,
frame_source.cpp, cudawarping/src/resize.cpp and remap.cpp, and the SeparableLinearFilter / createGaussianFilter part of cudafilters/
src/filtering.cpp.  Stand-ins remain for main-repo pieces only (getGaussianKernel, PointFilter / CubicFilter, the border index maps,
vec_math, GpuMat::convertTo / setTo): a reading shared by a stand-in and the restatement is NOT caught here.

Every comparison is on BITS (the uint32 view of the float32 arrays; +0 and -0 differ).  The skip rule is that of
tests/test_ref_pin_cuda.py, applied per test: the two tests of the committed btvl1_refclass_* fixtures' restatement side run everywhere.

Image sizes are chosen for the REFERENCE kernels' block structure, which the vectorised restatement does not have: row-filter blocks
cover 128 columns (1, 2 and >= 3 of them: the interior branch `blockIdx.x + 2 < gridDim.x`), column-filter blocks 64 rows, and no size
is a multiple of 32 / 8 / 16.
"""
import glob
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import btvl1_numpy_ref as R  # noqa: E402
from test_btvl1_gpu import BAD_PARAMS, CASES, make_case  # noqa: E402  (plain lists and a NumPy helper; nothing there touches a GPU at import)

from oracle import refcu, refocl  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_ref = pytest.mark.skipif(not (refcu.has_btvl1() or refocl.can_build()), reason="oracle/_ref not built (or built without BTV-L1) and /root/reference absent")


def same_bits(got, ref):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, ref.dtype, got.shape, ref.shape)
    view = np.uint32 if got.dtype == F else np.uint8
    ndiff = int((got.view(view) != ref.view(view)).sum())
    assert ndiff == 0, f"{ndiff} of {ref.size} values differ in their bits"


def image(rng, h, w, cn, levels=None):
    shape = (h, w) if cn == 1 else (h, w, cn)
    if levels:   # few distinct values: equal neighbours everywhere (the third branch of diffSign)
        return (rng.integers(0, levels, shape) * (255.0 / levels)).astype(F)
    return rng.uniform(0, 255, shape).astype(F)


def planes(rng, h, w, amp=3.0):
    return rng.uniform(-amp, amp, (h, w)).astype(F), rng.uniform(-amp, amp, (h, w)).astype(F)


# ------------------------------------------------------------------------------------------------------------------ btv_l1_gpu.cu
@needs_ref
@pytest.mark.parametrize("h,w", [(37, 53), (9, 11), (70, 301)])
def test_motion_maps_equal_build_motion_maps_kernel(h, w):
    """buildMotionMapsKernel (btv_l1_gpu.cu:73-95): which motion builds which map, and x + motion in f32."""
    rng = np.random.default_rng(h * w)
    f, b = planes(rng, h, w, 40.0), planes(rng, h, w, 40.0)
    rf, rb = refcu.btv_build_motion_maps(f, b)
    gf, gb = R.motion_maps(f, b)
    for got, ref in zip(gf + gb, rf + rb):
        same_bits(got, ref)
    assert not np.array_equal(rf[0], rb[0])


@needs_ref
@pytest.mark.parametrize("cn", [1, 3, 4])
@pytest.mark.parametrize("scale", [2, 3, 4])
def test_upscale_equals_upscale_kernel(cn, scale):
    """upscale (btv_l1_cuda.cpp:146-162 over upscaleKernel, btv_l1_gpu.cu:114-124): zeros but at (y scale, x scale)."""
    src = image(np.random.default_rng(cn * 10 + scale), 37, 53, cn) - F(100)
    same_bits(R.upscale(src, scale), refcu.btv_upscale(src, scale))


@needs_ref
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_diff_sign_equals_the_references_transform(cn):
    """diffSign of the data term (btv_l1_cuda.cpp:164-169: reshape(1), so all FOUR channels of a four-channel image alike; DiffSign,
    btv_l1_gpu.cu:145-148,167-173), with equal values, signed zeros and infinities among the operands."""
    rng = np.random.default_rng(cn)
    a, b = image(rng, 37, 53, cn, levels=4), image(rng, 37, 53, cn, levels=4)
    a.flat[:6] = [0.0, -0.0, np.inf, -np.inf, 1.0, np.inf]
    b.flat[:6] = [-0.0, 0.0, np.inf, np.inf, 1.0, 3.0]
    ref = refcu.btv_diff_sign(a, b)
    same_bits(R.diff_sign(a, b), ref)
    assert (ref == 0).any() and (ref == 1).any() and (ref == -1).any()
    if cn == 4:
        assert (ref[..., 3] != 0).any()   # unlike the regulariser's float4 diffSign, the data term keeps the fourth channel


@needs_ref
@pytest.mark.parametrize("cn", [1, 3, 4])
@pytest.mark.parametrize("bk", [1, 2, 3, 4, 7, 16])
def test_btv_regularization_equals_the_reference_kernel(cn, bk):
    """calcBtvRegularization (btv_l1_cuda.cpp:189-207 over calcBtvRegularizationKernel and its __constant__ table, btv_l1_gpu.cu:192-214)
    with the table calcBtvWeights loads: the enumeration order of the weights, the border of (btvKernelSize - 1) / 2 that stays +0, the
    fourth channel's +0."""
    rng = np.random.default_rng(100 * cn + bk)
    src = image(rng, 45, 70, cn, levels=6)
    wref = refcu.btv_weights(bk, 0.7)
    w = R.btv_weights(bk, 0.7)
    same_bits(w, wref[:len(w)])
    ref = refcu.btv_regularization(src, bk, wref)
    same_bits(R.btv_regularization(src, bk, w), ref)
    ks = (bk - 1) // 2
    inner = np.zeros(ref.shape[:2], bool)
    inner[ks:45 - ks, ks:70 - ks] = True
    assert not ref.view(np.uint32)[~inner].any()                       # the untouched border: +0 bits
    assert ks == 0 or np.abs(ref[inner]).max() > 0
    if cn == 4:
        assert not ref[..., 3].view(np.uint32).any()                   # the fourth channel: +0 bits everywhere


@needs_ref
@pytest.mark.parametrize("bk", range(1, 17))
def test_btv_weights_equal_calc_btv_weights(bk):
    """calcBtvWeights (btv_l1_cuda.cpp:171-187): pow(float(alpha), |m| + |l|) in the kernel's enumeration order; the rest of the
    btvKernelSize^2 vector stays 0."""
    for alpha in (0.7, 0.55, 1.0 / 3.0):
        ref = refcu.btv_weights(bk, alpha)
        got = R.btv_weights(bk, alpha)
        assert len(got) == len(R.btv_weight_offsets(bk)) <= ref.size
        same_bits(got, ref[:len(got)])
        assert not ref[len(got):].any()


# ------------------------------------------------------------------------------------------------------------- the separable blur
GAUSS_SHAPES = [(37, 100, 1), (100, 200, 3), (131, 420, 4), (150, 61, 1), (200, 300, 1), (8, 10, 1), (8, 10, 3), (5, 131, 4), (70, 3, 1)]


@needs_ref
@pytest.mark.parametrize("sigma", [0.0, 1.2])
@pytest.mark.parametrize("n", [1, 3, 5, 7, 9, 13, 31])
def test_gauss_separable_equals_the_references_filter(n, sigma):
    """cuda::createGaussianFilter(...)->apply (filtering.cpp:441-505,555-580 over linearRowFilter / linearColumnFilter): tap order,
    anchor, the f32 intermediate, reflect-101 at both ends of both axes.  Widths of 1, 2 and >= 3 row blocks, heights of 1, 2 and >= 3
    column blocks, and images shorter than the radius (the `% n` branch of BrdReflect101 is live for n = 31 on 8 x 10)."""
    rng = np.random.default_rng(31 * n + int(sigma * 10))
    k = R.gaussian_kernel(n, sigma)
    same_bits(k, refcu.cuda_gaussian_kernel(n, sigma))
    for h, w, cn in GAUSS_SHAPES:
        src = image(rng, h, w, cn) - F(64)
        same_bits(R.gauss_separable(src, k), refcu.cuda_gauss_filter(src, n, sigma))


@needs_ref
@pytest.mark.parametrize("n", range(1, 33))
def test_separable_filter_with_asymmetric_taps_equals_the_references(n):
    """The same filter class with taps that are NOT symmetric (a Gaussian hides a reversed tap order or a mirrored anchor from the
    values, leaving only the rounding order): every kernel length the reference instantiates, 1 .. 32, even ones included (anchor
    n >> 1), on an image of two row blocks and two column blocks and on one shorter than the kernel."""
    rng = np.random.default_rng(n)
    k = rng.uniform(-1, 1, n).astype(F)
    for h, w, cn in ((70, 140, 3), (9, 7, 1)):
        src = image(rng, h, w, cn) - F(100)
        same_bits(R.gauss_separable(src, k), refcu.cuda_separable_filter(src, k))


@needs_ref
def test_gauss_reference_is_self_consistent_across_its_block_structure():
    """The reference filter on a wide / tall image equals the reference filter on crops that put the same pixels into other blocks
    (interior, last-but-one, last), away from the borders: the block structure leaves no trace in the values."""
    rng = np.random.default_rng(7)
    src = image(rng, 210, 530, 1)
    full = refcu.cuda_gauss_filter(src, 13, 1.2)
    for y0, x0 in ((0, 0), (23, 57), (64, 128), (70, 250)):
        crop = refcu.cuda_gauss_filter(src[y0:, x0:], 13, 1.2)
        same_bits(crop[6:-6, 6:-6], full[y0 + 6:-6, x0 + 6:-6])


@needs_ref
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 13, 16, 21, 31, 32])
def test_gaussian_kernel_equals_the_stub_cores(n):
    """getGaussianKernel is main-repo code: libref_cu.so's is the C restatement of oracle/imgproc_ref.c.  Two statements of one reading,
    written apart (exp through libm there, math.exp here)."""
    for sigma in (0.0, 0.5, 1.2, 2.5):
        same_bits(R.gaussian_kernel(n, sigma), refcu.cuda_gaussian_kernel(n, sigma))


# ------------------------------------------------------------------------------------------------------------------- warping
@needs_ref
@pytest.mark.parametrize("cn", [1, 3, 4])
@pytest.mark.parametrize("scale", [2, 3, 4])
def test_resize_nearest_equals_the_reference_kernel(cn, scale):
    """cuda::resize(INTER_NEAREST) high-res -> low-res (resize.cpp:82-83,105 verbatim over resize_nearest, resize.cu:220-231): the
    f32 inverse factor and the truncation."""
    rng = np.random.default_rng(scale * 7 + cn)
    for lh, lw in ((37, 53), (9, 11), (64, 65)):
        src = image(rng, lh * scale, lw * scale, cn)
        same_bits(R.resize_nearest(src, lh, lw), refcu.cuda_resize_nearest(src, lh, lw))


@needs_ref
@pytest.mark.parametrize("cn", [1, 3, 4])
@pytest.mark.parametrize("scale", [2, 3, 4])
def test_resize_cubic_equals_the_reference_kernel(cn, scale):
    """cuda::resize(INTER_CUBIC) (the generic resize kernel, resize.cu:271-283, 369-383, over the CubicFilter / BrdReplicate stand-ins)."""
    rng = np.random.default_rng(scale * 11 + cn)
    for lh, lw in ((37, 53), (5, 4), (33, 70)):
        src = image(rng, lh, lw, cn) - F(30)
        same_bits(R.resize_cubic(src, lh * scale, lw * scale), refcu.cuda_resize_cubic(src, lh * scale, lw * scale))


@needs_ref
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_remap_nearest_equals_the_reference_kernel(cn):
    """cuda::remap(INTER_NEAREST, BORDER_REPLICATE, a stream) (remap.cpp verbatim, RemapDispatcherStream, remap.cu:57-69,85-104): maps
    that leave the image on all four sides, coordinates in (-1, 0) (truncation toward zero keeps them inside), exact integers, and
    just below an integer."""
    rng = np.random.default_rng(cn)
    h, w = 37, 53
    src = image(rng, h, w, cn)
    mx = rng.uniform(-9, w + 9, (41, 67)).astype(F)
    my = rng.uniform(-9, h + 9, (41, 67)).astype(F)
    mx[0, :8] = [-0.999, -0.5, -1e-7, -0.0, 0.0, 1.0, w - 1, w]
    my[0, :8] = [3.0, -0.25, -0.75, 5.0, -0.0, 2.0, h - 1, h]
    mx[1, :4] = np.nextafter(F([1, 7, w - 1, w]), F(-1000))
    my[1, :4] = np.nextafter(F([1, 7, h - 1, h]), F(-1000))
    mx[2] = np.round(mx[2])
    my[2] = np.round(my[2])
    assert mx.min() < -1 and mx.max() > w and my.min() < -1 and my.max() > h
    same_bits(R.remap_nearest(src, mx, my), refcu.cuda_remap_nearest_replicate(src, mx, my))


# ----------------------------------------------------------------------------------------------------------------- arithmetic
@needs_ref
@pytest.mark.parametrize("tau,lam", [(1.3, 0.03), (0.9, 0.1), (0.7, 0.2), (1.3, 1e-3)])
def test_add_weighted_equals_the_reference_functor(tau, lam):
    """cuda::addWeighted as process calls it (btv_l1_cuda.cpp:388,394): AddWeightedOp with float scalars -- the product -tau lambda is
    formed in double and rounded to f32 ONCE (not float(tau) * float(lambda))."""
    assert float(F(-tau * lam)) != -tau * lam                                       # not f32-representable
    rng = np.random.default_rng(int(tau * 100))
    a, b = image(rng, 37, 53, 3), image(rng, 37, 53, 3) - F(128)
    same_bits(R.add_weighted(a, 1.0, b, -tau * lam, 0.0), refcu.cuda_add_weighted(a, 1.0, b, -tau * lam, 0.0))
    same_bits(R.add_weighted(a, 1.0, b, tau, 0.0), refcu.cuda_add_weighted(a, 1.0, b, tau, 0.0))


@needs_ref
@pytest.mark.parametrize("scale", [2, 3, 4])
def test_upscale_motions_equal_the_references(scale):
    """upscaleMotions (btv_l1_cuda.cpp:117-129): cubic resize by (scale, scale) on the null stream, then MulScalarOp by float(scale)."""
    rng = np.random.default_rng(scale)
    motions = [planes(rng, 23, 31), planes(rng, 23, 31)]
    for got, ref in zip(R.upscale_motions(motions, scale), refcu.btv_upscale_motions(motions, scale)):
        same_bits(got[0], ref[0])
        same_bits(got[1], ref[1])
    same_bits(motions[0][0] * F(scale), refcu.cuda_multiply_scalar(motions[0][0], scale))


@needs_ref
@pytest.mark.parametrize("K,base", [(1, 0), (3, 0), (3, 1), (3, 2), (5, 0), (5, 2), (5, 4)])
def test_relative_motions_equal_calc_relative_motions(K, base):
    """calcRelativeMotions (btv_l1_cuda.cpp:80-115): the running sums outward from the base frame, and which of forward[i] /
    backward[i] each one reads (the entries the reference must not read are EMPTY matrices there: reading one throws)."""
    rng = np.random.default_rng(10 * K + base)
    fwd = [planes(rng, 19, 27) if i < K - 1 else None for i in range(K)]
    bwd = [planes(rng, 19, 27) if i > 0 else None for i in range(K)]
    gf, gb = R.relative_motions(fwd, bwd, base, (19, 27))
    rf, rb = refcu.btv_relative_motions(fwd, bwd, base, (19, 27))
    for got, ref in zip(gf + gb, rf + rb):
        same_bits(got[0], ref[0])
        same_bits(got[1], ref[1])


# ---------------------------------------------------------------------------------------------------------------- whole process
def case_id(c):
    return f"s{c[0]}_{c[1]}x{c[2]}x{c[3]}_K{c[4]}b{c[5]}_" + "_".join(f"{k}{v}" for k, v in c[7].items())


@needs_ref
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_process_equals_the_reference_class(case):
    """BTVL1_CUDA_Base::process (btv_l1_cuda.cpp:306-400, verbatim) over the reference's kernels, on the cases of
    tests/test_btvl1_gpu.py::test_process_bit_exact: 1 / 2 / 7 iterations, CN 1 / 3 / 4, scale 2 / 3 / 4, K 1 / 3 / 5 with the base first,
    in the middle and last, lambda 0 and > 0, every parameter corner.  Also btvWeights_ as the class leaves it."""
    seed, lh, lw, cn, K, base, _, kw = case
    frames, fwd, bwd = make_case(seed, lh, lw, cn, K)
    ref, wts = refcu.cuda_class_btvl1_process(frames, fwd, bwd, base, **kw)
    same_bits(R.process(frames, fwd, bwd, base, **kw), ref)
    p = dict(R.DEFAULTS, **kw)
    w = R.btv_weights(p["btv_kernel_size"], p["alpha"])
    same_bits(w, wts[:len(w)])


@needs_ref
def test_process_on_one_object_after_its_parameters_change():
    """The cache invalidation of btv_l1_cuda.cpp:320-335: one object, then a changed blur size, blur sigma, BTV size, alpha, frame count
    and channel count -- each result equals the restatement's (and a fresh object's)."""
    alg = refcu.BTVL1Class()
    steps = [(1, 3, dict(scale=2, iterations=3)),
             (1, 3, dict(scale=2, iterations=3, blur_kernel_size=9)),
             (1, 3, dict(scale=2, iterations=3, blur_kernel_size=9, blur_sigma=1.2)),
             (1, 3, dict(scale=2, iterations=3, blur_kernel_size=9, blur_sigma=1.2, btv_kernel_size=3)),
             (1, 3, dict(scale=2, iterations=3, blur_kernel_size=9, blur_sigma=1.2, btv_kernel_size=3, alpha=0.4)),
             (1, 5, dict(scale=2, iterations=3, blur_kernel_size=9, blur_sigma=1.2, btv_kernel_size=3, alpha=0.4)),
             (3, 5, dict(scale=3, iterations=2, blur_kernel_size=9, blur_sigma=1.2, btv_kernel_size=3, alpha=0.4)),
             (1, 3, dict(scale=2, iterations=3))]
    for n, (cn, K, kw) in enumerate(steps):
        frames, fwd, bwd = make_case(300 + n, 21, 29, cn, K)
        ref, wts = alg.process(frames, fwd, bwd, K // 2, **kw)
        same_bits(R.process(frames, fwd, bwd, K // 2, **kw), ref)
        same_bits(refcu.cuda_class_btvl1_process(frames, fwd, bwd, K // 2, **kw)[0], ref)
        w = R.btv_weights(dict(R.DEFAULTS, **kw)["btv_kernel_size"], dict(R.DEFAULTS, **kw)["alpha"])
        same_bits(w, wts[:len(w)])


GOOD_PARAMS = [dict(scale=2), dict(iterations=1), dict(tau=1e-6), dict(alpha=1e-6), dict(btv_kernel_size=1), dict(btv_kernel_size=16),
               dict(blur_kernel_size=1), dict(blur_kernel_size=31), dict(blur_sigma=0.0), dict(lambda_=0.0), dict(lambda_=-1.0)]


@needs_ref
def test_the_references_asserts_fire_where_check_params_rejects():
    """The CV_Asserts of process (btv_l1_cuda.cpp:310-316) and of the Gaussian / separable filter (filtering.cpp:441-442,568) against
    R.check_params: the reference throws for every parameter set tests/test_btvl1_gpu.py::test_argument_checks rejects (BAD_PARAMS), for
    none of their accepted neighbours, and R.check_params draws the same line."""
    frames, fwd, bwd = make_case(1, 16, 16, 1, 3)

    def ref_throws(kw):
        try:
            refcu.cuda_class_btvl1_process(frames, fwd, bwd, 1, **dict(dict(iterations=1), **kw))
        except ValueError:
            return True
        return False

    def r_rejects(kw):
        try:
            R.check_params(dict(R.DEFAULTS, **kw))
        except AssertionError:
            return True
        return False

    for kw, _ in BAD_PARAMS:
        assert ref_throws(kw) and r_rejects(kw), kw
    for kw in GOOD_PARAMS:
        assert not ref_throws(kw) and not r_rejects(kw), kw


# ------------------------------------------------------------------------------------------------------------------ ring driver
def run_restatement_sequence(frames, flows, **kw):
    """R.BTVL1 over the frames with a flow function that hands out `flows` in call order and records which frames it was asked about."""
    index = {f.tobytes(): i for i, f in enumerate(frames)}
    calls = []

    def flow(a, b):
        calls.append((index[np.ascontiguousarray(a).tobytes()], index[np.ascontiguousarray(b).tobytes()]))
        return flows[len(calls) - 1]

    sr = R.BTVL1(R.ListSource(frames), flow, **kw)
    outs = []
    while (o := sr.nextFrame()) is not None:
        outs.append(o)
    return outs, calls, sr.nextFrame() is None


@needs_ref
@pytest.mark.parametrize("radius,n,cn", [(1, 2, 1), (1, 3, 1), (1, 6, 3), (2, 3, 1), (2, 4, 4), (2, 5, 1), (2, 8, 1), (4, 5, 1), (4, 7, 1), (4, 9, 3)])
def test_ring_driver_equals_the_reference_class(radius, n, cn):
    """BTVL1_CUDA (btv_l1_cuda.cpp:426-583, with super_resolution.cpp's nextFrame) over a list of u8 frames and replayed flows: the number
    of outputs, the number and ORDER of the flow requests (which frame pair each asks about), every output byte, nothing after the last
    frame.  Sequences shorter than the window 2 r + 1, equal to it and longer (shortest: r + 1 frames -- initImpl processes frames
    0 .. r unconditionally, fewer is undefined behaviour in the reference)."""
    rng = np.random.default_rng(100 * radius + n)
    shape = (13, 17) if cn == 1 else (13, 17, cn)
    frames = [rng.integers(0, 256, shape).astype(np.uint8) for _ in range(n)]
    flows = [planes(rng, 13, 17, 2.0) for _ in range(2 * (n - 1))]
    kw = dict(scale=2, iterations=2, btv_kernel_size=3, blur_kernel_size=3, temporal_area_radius=radius)
    ref_outs, ref_calls, ref_ended = refcu.cuda_class_btvl1_sequence(frames, flows, **kw)
    outs, calls, ended = run_restatement_sequence(frames, flows, **kw)
    assert len(outs) == len(ref_outs) == n
    assert calls == ref_calls and len(calls) == 2 * (n - 1)
    for got, ref in zip(outs, ref_outs):
        same_bits(got, ref)
    assert ended and ref_ended


# -------------------------------------------------------------------------------------------------- the committed reference anchor
REFCLASS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "btvl1_refclass_*.npz")))


def load_refclass(path):
    z = np.load(path)
    kw = json.loads(str(z["params"]))
    base = kw.pop("base_idx")
    n = z["frames"].shape[0]
    fwd = [(z["fwd"][i, 0], z["fwd"][i, 1]) if i < n - 1 else None for i in range(n)]
    bwd = [(z["bwd"][i, 0], z["bwd"][i, 1]) if i > 0 else None for i in range(n)]
    return list(z["frames"]), fwd, bwd, base, kw, z["out"]


def test_refclass_fixtures_are_there():
    assert len(REFCLASS) >= 2 and all(os.path.getsize(p) < 176 * 1024 for p in REFCLASS)
    cns = {1 if np.load(p)["frames"].ndim == 3 else np.load(p)["frames"].shape[3] for p in REFCLASS}
    scales = {json.loads(str(np.load(p)["params"]))["scale"] for p in REFCLASS}
    assert {1, 4} <= cns and {2, 3} <= scales


@pytest.mark.parametrize("path", REFCLASS, ids=[os.path.basename(p) for p in REFCLASS])
def test_restatement_reproduces_the_reference_classes_recorded_output(path):
    """tests/golden/btvl1_refclass_*.npz (tools/make_golden_btvl1.py --refclass): inputs, motions, parameters and the output of the
    REFERENCE library's process -- data its programs wrote.  Runs everywhere, also where oracle/_ref is absent: the restatement stays
    tied to the reference class without the reference tree."""
    frames, fwd, bwd, base, kw, out = load_refclass(path)
    same_bits(R.process(frames, fwd, bwd, base, **kw), out)


@needs_ref
@pytest.mark.parametrize("path", REFCLASS, ids=[os.path.basename(p) for p in REFCLASS])
def test_reference_library_reproduces_its_recorded_output(path):
    """... and where the reference library is present, it still computes what was recorded from it."""
    frames, fwd, bwd, base, kw, out = load_refclass(path)
    same_bits(refcu.cuda_class_btvl1_process(frames, fwd, bwd, base, **kw)[0], out)
