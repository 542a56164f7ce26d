"""Farneback: oracle self-tests (CPU) and HIP-vs-oracle parity (GPU) for cv::cuda::FarnebackOpticalFlow.

Every comparison of a kernel or of a whole calc with the oracle is EQUALITY of every value (np.testing.assert_array_equal):
  * stage level: kernel and oracle/farneback_ref.c perform the same binary32 operations in the same order, both built with
    -ffp-contract=off; the division of the 2 x 2 solve is correctly rounded on both sides; the Gaussian taps and the inverse moment
    matrix are formed on the host by the same double formula.  Every launch form of every stage -- one-row, 256 x 4 and 64 x 4 tiles,
    two iterations per launch, the merged output, update 0 / 1, tiled and resize-sampling expansion, zero-flow and resize-fused matrix
    update, generic / tiled / in-place table blur -- is launched by name (cuda.farneback_*_form) at shapes that hold every tile edge
    and compared with the oracle and with the other forms.  Measured on an MI355X: 0 differing values in 3 188 comparisons.
  * whole calc (tests/fb_flow_check.py, shared with tests/test_golden.py and tests/test_ref_class_gpu.py): a calc is a fixed sequence
    of those stages, so the flow equals the oracle's at every pixel.  Measured GPU-versus-oracle maximum over the reference's parameter
    grid (12 cases, 388 x 584), config 1, the 24 configurations of the seeded sweep, fast pyramids, initial flow, the batches and the
    three golden files: 0 px, 0 differing values.  The mean-EPE <= 2e-3 px / |1 - CCORR| <= 1e-5 criterion these tests used before
    passed with 0.15 px added to a whole column of a 388 x 584 flow.
  * for scale, the reference algorithm's own sensitivity to rounding: the oracle as committed against the same sources compiled with
    -mfma -ffp-contract=fast, over the same configurations -- mean difference at most 2.4e-5 px, worst pixel typically 3e-6 .. 1e-4 px
    and 0.16 px at isolated pixels of one sweep configuration (floor() of the displaced position in the matrix update amplifies one
    ulp).  A bound derived from it would be orders looser than what holds; no bound is used.
  * the reference's own CUDA-vs-CPU acceptance is |1 - CCORR| <= 1e-4 (box) / 2e-2 (Gaussian), cudaoptflow/test/test_optflow.cpp:349.
"""
import os
import sys

import numpy as np
import pytest

from opencv_contrib_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fb_flow_check import assert_flow_equals as _assert_flow  # noqa: E402


def T(a, dev):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)   # (the shared stage inputs are read-only)


def N(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------ oracle (CPU)
def test_oracle_gaussian_kernel_tables_and_normalisation(oracle):
    np.testing.assert_array_equal(oracle.fb_gaussian_kernel(3, 0), np.array([0.25, 0.5, 0.25], np.float32))
    k = oracle.fb_gaussian_kernel(13, 13 // 2 * 0.3)
    assert abs(k.sum() - 1) < 1e-6 and np.allclose(k, k[::-1]) and k.argmax() == 6
    k = oracle.fb_gaussian_kernel(9, 0)      # sigma <= 0, n > 7: sigma = ((n-1)*0.5 - 1)*0.3 + 0.8
    s = ((9 - 1) * 0.5 - 1) * 0.3 + 0.8
    x = np.arange(9) - 4
    ref = np.exp(-x * x / (2 * s * s)); ref /= ref.sum()
    np.testing.assert_allclose(k, ref, rtol=1e-6)


def test_oracle_prepare_gaussian_inverts_moment_matrix(oracle):
    g, xg, xxg, ig = oracle.fb_prepare_gaussian(5, 1.1)
    full = np.concatenate([g[:0:-1], g])
    assert abs(full.sum() - 1) < 1e-6
    # ig11 = 1 / sum(g_y g_x x^2) (the x-moment block of G is diagonal)
    x = np.arange(-5, 6)
    m2 = (full[:, None] * full[None, :] * (x[None, :] ** 2)).sum()
    assert abs(ig[0] - 1 / m2) < 1e-5


def test_oracle_polyexp_recovers_quadratic(oracle):
    """f(x,y) = c + ax + by + (1/2)(r4 x^2... ): the expansion of an exact quadratic returns its coefficients
    in the layout [b_y?]: plane0 = d/dy, plane1 = d/dx, plane2 = yy/..., here checked via a pure linear ramp."""
    h, w = 40, 50
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = (3.0 + 0.5 * x - 0.25 * y).astype(np.float32)
    R = oracle.fb_poly_exp(img, 5, 1.1).reshape(5, h, w)
    c = (slice(8, -8), slice(8, -8))
    np.testing.assert_allclose(R[0][c], -0.25, atol=1e-4)   # b3*ig11: linear term in y
    np.testing.assert_allclose(R[1][c], 0.5, atol=1e-4)     # b2*ig11: linear term in x
    for k in (2, 3, 4):
        np.testing.assert_allclose(R[k][c], 0.0, atol=1e-4)


def test_oracle_pyr_down_constant_and_size(oracle):
    img = np.full((31, 45), 7.0, np.float32)
    d = oracle.fb_pyr_down(img)
    assert d.shape == (16, 23)
    np.testing.assert_allclose(d, 7.0, rtol=1e-6)


@pytest.mark.parametrize("flags", [0, 256])
def test_oracle_recovers_analytic_flow_config1(oracle, flags):
    """BASELINE configs[0]: 640x480 synthetic pair, class defaults."""
    I0, I1, gt = synth.flow_pair(480, 640, seed=1234, dtype="u8")
    f = oracle.fb_calc(I0, I1, oracle.fb_params(flags=flags))
    assert synth.epe(f[40:-40, 40:-40], gt[40:-40, 40:-40]) < 0.08


def test_oracle_initial_flow_and_fast_pyramids(oracle):
    I0, I1, gt = synth.flow_pair(240, 320, seed=5, dtype="u8")
    f = oracle.fb_calc(I0, I1, oracle.fb_params(fast_pyramids=1))
    assert synth.epe(f[30:-30, 30:-30], gt[30:-30, 30:-30]) < 0.12
    f2 = oracle.fb_calc(I0, I1, oracle.fb_params(flags=4, num_iters=3), init_flow=gt)
    assert synth.epe(f2[30:-30, 30:-30], gt[30:-30, 30:-30]) < 0.12


def test_oracle_blur_border_is_a_reflection_while_the_half_size_stays_below_the_plane(oracle):
    """BrdReflect101 as the oracle (and the kernels) state it, abs(abs(last - abs(last - i)) % n) % n, is the mirror image without the
    border pixel for |offset| <= n - 1; further out its modulo wraps (the reference's formula, not a second fold).  Checked through the
    blur against NumPy's 'reflect' padding with the taps summed in the same order: equal up to half size n - 1 of the smaller dimension."""
    rng = np.random.default_rng(0)
    for shape in ((5, 40), (37, 4)):
        img = rng.random(shape, dtype=np.float32)
        h, w = shape
        for kh in range(1, min(shape)):
            k = oracle.fb_gaussian_kernel(2 * kh + 1, 0.3 * kh + 0.8)
            p = np.pad(img, kh, mode="reflect")
            v = p[kh:kh + h] * k[kh]
            for j in range(1, kh + 1):
                v = v + (p[kh - j:kh - j + h] + p[kh + j:kh + j + h]) * k[kh + j]
            out = v[:, kh:kh + w] * k[kh]
            for j in range(1, kh + 1):
                out = out + (v[:, kh - j:kh - j + w] + v[:, kh + j:kh + j + w]) * k[kh + j]
            np.testing.assert_array_equal(oracle.fb_gaussian_blur(img, 2 * kh + 1, 0.3 * kh + 0.8), out, err_msg=f"{shape} half {kh}")


def test_oracle_argument_errors(oracle):
    I = np.zeros((64, 64), np.uint8)
    with pytest.raises(ValueError):
        oracle.fb_calc(I, I, oracle.fb_params(poly_n=6))              # CV_Assert(polyN == 5 || 7)  farneback.cpp:316
    with pytest.raises(ValueError):
        oracle.fb_calc(I, I, oracle.fb_params(fast_pyramids=1, pyr_scale=0.8))   # :317
    with pytest.raises(ValueError):
        oracle.fb_calc(I, I[:, :32])
    with pytest.raises(ValueError):
        oracle.fb_calc(I, I, oracle.fb_params(flags=4))               # initial flow missing


# ------------------------------------------------------------------ HIP vs oracle (GPU)
gpu_mark = pytest.mark.gpu


def _same(a, b, name):
    """Bit equality, with the figures printed first (run with -s to see them)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, name
    ne = a != b
    if ne.any():
        print(f"{name}: {int(ne.sum())} of {a.size} values differ, worst |a - b| {np.abs(a.astype(np.float64) - b)[ne].max():.3e} "
              f"at scale {np.abs(b).max():.3e}")
    np.testing.assert_array_equal(a, b, err_msg=name)


@gpu_mark
@pytest.mark.parametrize("shape", [(48, 70), (97, 531)])
@pytest.mark.parametrize("polyN,sigma", [(5, 1.1), (7, 1.5)])
def test_poly_exp_matches_oracle(gpu, oracle, shape, polyN, sigma):
    from opencv_contrib_amd import cuda
    img = np.random.default_rng(1).random(shape, dtype=np.float32) * 255
    ref = oracle.fb_poly_exp(img, polyN, sigma)
    _same(N(cuda.farneback_polyExp(T(img, gpu), polyN, sigma)), ref, "poly_exp")


def _fb_state(h, w, seed, amp=2.0):
    rng = np.random.default_rng(seed)
    I0 = synth.texture(h, w, seed, 2.0).astype(np.float32)
    I1 = synth.texture(h, w, seed + 1, 2.0).astype(np.float32)
    fx = ((rng.random((h, w), dtype=np.float32) - 0.5) * 2 * amp).astype(np.float32)
    fy = ((rng.random((h, w), dtype=np.float32) - 0.5) * 2 * amp).astype(np.float32)
    return I0, I1, fx, fy


@gpu_mark
@pytest.mark.parametrize("shape,amp", [((40, 64), 1.5), ((67, 300), 30.0)])
def test_update_matrices_matches_oracle(gpu, oracle, shape, amp):
    from opencv_contrib_amd import cuda
    I0, I1, fx, fy = _fb_state(*shape, seed=3, amp=amp)
    R0, R1 = oracle.fb_poly_exp(I0), oracle.fb_poly_exp(I1)
    ref = oracle.fb_update_matrices(fx, fy, R0, R1)
    out = cuda.farneback_updateMatrices(T(fx, gpu), T(fy, gpu), T(R0, gpu), T(R1, gpu))
    _same(N(out), ref, "update_matrices")


# ---- every launch form of a stage, one by one (cuda.farneback_*_form -> miflow_selftest_farneback_*): the level loop picks a form from
# the grid size and the tuning of the process, so a calc at a test's size runs a minority of them
# (7, 9): smaller than any tile and than 2 KH.  (61, 277): two 256- and five 64-column tiles, the last ragged in both directions, 16 row
# tiles.  (9, 513): a third 256-column tile of one column.  Tile grids of 2, 9 and 27 workgroups are no multiples of 8: the remainder
# branch of the XCD tile swizzle (the 32 and 80 workgroups of 61 x 277 take the other one).
_STAGE_SHAPES = [(7, 9), (61, 277), (9, 513)]
_TILED_WINDOWS = (9, 13, 15, 21)                # KH 4, 6, 7, 10: k_iterate_t; the first three also k_iterate2_t
_SENTINEL = np.float32(-12345.5)


_stage_cache = {}


def _stage_state(oracle, shape, seed, amp):
    """Random planes of one shape and their oracle expansions and matrices, computed once and read-only."""
    key = (shape, seed, amp)
    if key not in _stage_cache:
        I0, I1, fx, fy = _fb_state(*shape, seed=seed, amp=amp)
        R0, R1 = oracle.fb_poly_exp(I0), oracle.fb_poly_exp(I1)
        st = dict(I0=I0, I1=I1, fx=fx, fy=fy, R0=R0, R1=R1, M=oracle.fb_update_matrices(fx, fy, R0, R1))
        for v in st.values():
            v.setflags(write=False)
        _stage_cache[key] = st
    return _stage_cache[key]


def _oracle_iteration(oracle, M, R0, R1, ksize, gauss):
    """boxFilter5 / gaussianBlur5 -> updateFlow -> updateMatrices, the three launches one fused iteration stands for"""
    Mb = oracle.fb_blur5(M, ksize, float(ksize // 2 * np.float32(0.3)) if gauss else None)
    fx, fy = oracle.fb_update_flow(Mb)
    return fx, fy, oracle.fb_update_matrices(fx, fy, R0, R1)


def _check_updated_matrices(oracle, Mg, gfx, gfy, rfx, rfy, Mref, R0, R1, name):
    """The matrix update takes floor() of the displaced position: M' is held to the oracle's update of the GPU's OWN flow, and to the
    oracle chain wherever the flow bits agree -- a flow difference of one ulp cannot excuse a wrong M'."""
    _same(Mg, oracle.fb_update_matrices(gfx, gfy, R0, R1), name + " M' vs the oracle update of the GPU's flow")
    agree = np.tile((gfx == rfx) & (gfy == rfy), (5, 1))
    _same(Mg[agree], Mref[agree], name + " M' vs the oracle chain where the flows agree")


def _check_iterate_forms(gpu, oracle, shape, seed, amp, ksize, gauss):
    from opencv_contrib_amd import capi, cuda
    st = _stage_state(oracle, shape, seed, amp)
    h, w = shape
    M, R0, R1 = st["M"], st["R0"], st["R1"]
    tM, tR0, tR1 = T(M, gpu), T(R0, gpu), T(R1, gpu)
    rfx, rfy, M2 = _oracle_iteration(oracle, M, R0, R1, ksize, gauss)
    pattern = (np.arange(5 * h * w, dtype=np.float32).reshape(5 * h, w) * np.float32(0.25) + _SENTINEL)
    tiled = ksize in _TILED_WINDOWS
    forms = ["row"] + (["tile256", "tile64"] if tiled else [])
    tag = f"{shape} amp {amp} win {ksize} {'gauss' if gauss else 'box'}"
    out = {}
    for update in (True, False):
        for f in forms:
            fx, fy, Mo = cuda.farneback_iterate_form(f, tM, tR0, tR1, ksize, gauss, update, Mout=T(pattern, gpu))
            out[f, update] = N(fx), N(fy), N(Mo)
        gfx, gfy, gM = out["row", update]
        for f in forms[1:]:   # 1. the forms against each other
            for a, b, n in zip(out[f, update], out["row", update], ("flowx", "flowy", "Mout")):
                _same(a, b, f"{tag} update {update}: {f} vs row, {n}")
        _same(gfx, rfx, f"{tag} update {update}: flowx vs oracle")   # 2. against the oracle
        _same(gfy, rfy, f"{tag} update {update}: flowy vs oracle")
        if update:
            _check_updated_matrices(oracle, gM, gfx, gfy, rfx, rfy, M2, R0, R1, tag)
        else:
            _same(gM, pattern, f"{tag}: update = 0 must leave Mout alone")
    if not tiled:
        for f in ("tile256", "tile64", "pair"):
            with pytest.raises(capi.MiError):
                cuda.farneback_iterate_form(f, tM, tR0, tR1, ksize, gauss, True)
        return
    # 3. the merged CV_32FC2 output: a pitched matrix inside a buffer of sentinels
    import torch

    def merged_buf():
        buf = torch.full((h, w + 5, 2), float(_SENTINEL), dtype=torch.float32, device=gpu)
        return buf, buf[:, 2:2 + w]

    def check_merged(buf, fx, fy, name):
        b = N(buf)
        _same(b[:, 2:2 + w], np.stack([fx, fy], -1), name + ": merged flow vs the planes")
        assert (b[:, :2] == _SENTINEL).all() and (b[:, 2 + w:] == _SENTINEL).all(), name + ": padding of the merged matrix written"

    for f in forms[1:]:
        for update in (True, False):
            buf, view = merged_buf()
            fx, fy, Mo = cuda.farneback_iterate_form(f, tM, tR0, tR1, ksize, gauss, update, Mout=T(pattern, gpu), merged=view)
            for a, b, n in zip((N(fx), N(fy), N(Mo)), out[f, update], ("flowx", "flowy", "Mout")):
                _same(a, b, f"{tag} update {update}: {f} with the merged output, {n}")
            check_merged(buf, N(fx), N(fy), f"{tag} {f} update {update}")
    with pytest.raises(capi.MiError):
        cuda.farneback_iterate_form("row", tM, tR0, tR1, ksize, gauss, True, merged=merged_buf()[1])
    # two iterations per launch = two launches of a one-iteration form with M and Mout swapped in between, as the level loop swaps them
    if ksize == 21:
        with pytest.raises(capi.MiError):
            cuda.farneback_iterate_form("pair", tM, tR0, tR1, ksize, gauss, True)
        return
    tM1 = T(out["tile64", True][2], gpu)
    r2fx, r2fy, M3 = _oracle_iteration(oracle, M2, R0, R1, ksize, gauss)
    for update in (True, False):
        two = cuda.farneback_iterate_form("tile64", tM1, tR0, tR1, ksize, gauss, update, Mout=T(pattern, gpu))
        buf, view = merged_buf()
        pair = cuda.farneback_iterate_form("pair", tM, tR0, tR1, ksize, gauss, update, Mout=T(pattern, gpu), merged=view)
        bare = cuda.farneback_iterate_form("pair", tM, tR0, tR1, ksize, gauss, update, Mout=T(pattern, gpu))
        for a, b, c, n in zip(pair, bare, two, ("flowx", "flowy", "Mout")):
            _same(N(a), N(c), f"{tag} update {update}: pair vs two launches, {n}")
            _same(N(b), N(c), f"{tag} update {update}: pair without the merged output vs two launches, {n}")
        check_merged(buf, N(pair[0]), N(pair[1]), f"{tag} pair update {update}")
        pfx, pfy, pM = (N(t) for t in pair)
        if np.array_equal(out["tile64", True][2], M2):   # the first iteration equals the oracle's: so must the second
            _same(pfx, r2fx, f"{tag} update {update}: pair flowx vs two oracle iterations")
            _same(pfy, r2fy, f"{tag} update {update}: pair flowy vs two oracle iterations")
        if update:
            _check_updated_matrices(oracle, pM, pfx, pfy, r2fx, r2fy, M3, R0, R1, tag + " pair")
        else:
            _same(pM, pattern, f"{tag}: pair with update = 0 must leave Mout alone")


@gpu_mark
@pytest.mark.parametrize("ksize,gauss", [(13, False), (13, True), (5, False), (31, True)])
def test_blur5_update_flow_and_fused_iteration_match_oracle(gpu, oracle, ksize, gauss):
    """blur5 and updateFlow as separate launches, then the fused iteration in every form it has at this window size: the forms equal each
    other and the oracle's boxFilter5 / gaussianBlur5 -> updateFlow -> updateMatrices chain bit for bit (same binary32 operations in
    the same order on both sides, -ffp-contract=off, correctly rounded division; the Gaussian taps come from the same host formula)."""
    from opencv_contrib_amd import cuda
    h, w = 61, 277
    st = _stage_state(oracle, (h, w), 7, 2.0)
    M = st["M"]
    sig = (ksize // 2 * np.float32(0.3)) if gauss else None
    Mb = oracle.fb_blur5(M, ksize, float(sig) if gauss else None)
    _same(N(cuda.farneback_blur5(T(M, gpu), ksize, gauss)), Mb, "blur5")
    rfx, rfy = oracle.fb_update_flow(Mb)
    gfx, gfy = cuda.farneback_updateFlow(T(Mb, gpu))
    _same(N(gfx), rfx, "flowx"); _same(N(gfy), rfy, "flowy")
    # the entry calc()'s dispatch serves (whatever form it picks here) ...
    ifx, ify, iM = (N(t) for t in cuda.farneback_iterate(T(M, gpu), T(st["R0"], gpu), T(st["R1"], gpu), ksize, gauss, True))
    M2 = oracle.fb_update_matrices(rfx, rfy, st["R0"], st["R1"])
    _same(ifx, rfx, "iterate flowx"); _same(ify, rfy, "iterate flowy")
    _check_updated_matrices(oracle, iM, ifx, ify, rfx, rfy, M2, st["R0"], st["R1"], "iterate")
    # ... and every named form
    _check_iterate_forms(gpu, oracle, (h, w), 7, 2.0, ksize, gauss)


@gpu_mark
@pytest.mark.parametrize("ksize,gauss", [(k, g) for k in _TILED_WINDOWS for g in (False, True)] + [(11, False), (27, True)])
@pytest.mark.parametrize("amp", [1.5, 30.0])
@pytest.mark.parametrize("shape", _STAGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_iterate_form_matches_oracle_and_the_other_forms(gpu, oracle, shape, amp, ksize, gauss):
    """One-row k_iterate, k_iterate_t on 256 x 4 and on 64 x 4 tiles, k_iterate2_t (two iterations per launch; windows 9 / 13 / 15), box
    and Gaussian windows, update 0 / 1, with and without the merged CV_32FC2 output, on planes whose matrices come from flows of 1.5 and
    30 px (many displaced positions leave the image).  1. all forms give the same bytes; 2. they are the bytes of the oracle chain
    (M' against the oracle's update of the GPU's own flow as well); 3. the merged matrix holds the interleaved planes and its padding
    is untouched, update = 0 leaves Mout alone; a form without a kernel for the window is an error."""
    _check_iterate_forms(gpu, oracle, shape, 11, amp, ksize, gauss)


_POLY_SHAPES = {5: _STAGE_SHAPES + [(9, 246), (9, 247), (17, 484), (9, 485)],     # usable tile width 256 - 2 N: one / two tiles exactly, and
                7: _STAGE_SHAPES + [(9, 242), (9, 243), (17, 484), (9, 485)]}     # one column more; 9 and 17 rows: a ragged second / third row tile


@gpu_mark
@pytest.mark.parametrize("polyN,sigma,shape", [(n, s, shp) for n, s in ((5, 1.1), (7, 1.5)) for shp in _POLY_SHAPES[n]],
                         ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
def test_every_poly_exp_form_matches_oracle_and_the_other_forms(gpu, oracle, polyN, sigma, shape):
    """k_poly_exp (one row), k_poly_exp_t (8-row tiles; calc() runs it from 1024 workgroups on) and k_poly_exp<N, true>, which samples
    cuda::resize of a larger blurred plane on the fly (scale factors formed as poly_exp() forms them): equal to each other and to the
    oracle's fb_poly_exp (after resize_linear_cuda for the resized form) bit for bit."""
    from opencv_contrib_amd import capi, cuda
    h, w = shape
    img = np.random.default_rng(1).random(shape, dtype=np.float32) * 255
    ref = oracle.fb_poly_exp(img, polyN, sigma)
    row = N(cuda.farneback_polyExp_form("row", T(img, gpu), polyN, sigma))
    _same(N(cuda.farneback_polyExp_form("tiled", T(img, gpu), polyN, sigma)), row, "tiled vs row")
    _same(row, ref, "row vs oracle")
    for sshape in ((2 * h + 1, 2 * w - 1), (int(h / 0.8) + 1, int(w / 0.8))):   # about pyrScale 0.5 and 0.8
        big = np.random.default_rng(2).random(sshape, dtype=np.float32) * 255
        lvl = oracle.resize_linear_cuda(big, dsize=(w, h))
        _same(N(cuda.farneback_polyExp_form("resized", T(big, gpu), polyN, sigma, dsize=shape)), oracle.fb_poly_exp(lvl, polyN, sigma),
              f"resized from {sshape} vs oracle")
        _same(N(cuda.farneback_polyExp_form("row", T(lvl, gpu), polyN, sigma)), oracle.fb_poly_exp(lvl, polyN, sigma), "row on the resized plane")
    with pytest.raises(capi.MiError):
        cuda.farneback_polyExp_form("resized", T(img, gpu), polyN, sigma, dsize=shape)   # nothing to resize


@gpu_mark
@pytest.mark.parametrize("amp", [1.5, 30.0])
@pytest.mark.parametrize("shape", _STAGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_update_matrices_form_matches_oracle(gpu, oracle, shape, amp):
    """k_update_matrices with flow planes, with the zero flow of the coarsest level (null planes), and k_update_matrices_rs, which
    samples cuda::resize of the coarser level's flow, multiplies by 1 / pyrScale, stores the flow and updates in one launch."""
    from opencv_contrib_amd import cuda
    h, w = shape
    st = _stage_state(oracle, shape, 3, amp)
    fx, fy, R0, R1 = st["fx"], st["fy"], st["R0"], st["R1"]
    tR0, tR1 = T(R0, gpu), T(R1, gpu)
    M, _, _ = cuda.farneback_updateMatrices_form("plain", tR0, tR1, T(fx, gpu), T(fy, gpu))
    _same(N(M), st["M"], "plain vs oracle")
    _same(N(cuda.farneback_updateMatrices(T(fx, gpu), T(fy, gpu), tR0, tR1)), st["M"], "the stage entry vs oracle")
    M, _, _ = cuda.farneback_updateMatrices_form("zero", tR0, tR1)
    z = np.zeros(shape, np.float32)
    _same(N(M), oracle.fb_update_matrices(z, z, R0, R1), "zero flow vs oracle")
    for pshape, scale in (((max(h // 2, 2), max(w // 2, 2)), 0.5), ((max(int(h * 0.8), 2), max(int(w * 0.8), 2)), 0.8), (shape, 0.5)):
        _, _, px, py = _fb_state(*pshape, seed=5, amp=amp)
        alpha = np.float32(1.0 / scale)
        rx, ry = (oracle.resize_linear_cuda(p, dsize=(w, h)) * alpha for p in (px, py))
        if pshape == shape:
            continue   # (the level loop never fuses a zoom between equal sizes: cuda::resize is a copy there)
        M, gx, gy = (N(t) for t in cuda.farneback_updateMatrices_form("resized", tR0, tR1, prevx=T(px, gpu), prevy=T(py, gpu), alpha=alpha))
        _same(gx, rx, f"resized from {pshape}: flowx vs oracle"); _same(gy, ry, f"resized from {pshape}: flowy vs oracle")
        _check_updated_matrices(oracle, M, gx, gy, rx, ry, oracle.fb_update_matrices(rx, ry, R0, R1), R0, R1, f"resized from {pshape}")


# the stage shapes, a plane of five rows and one of four columns (kernel half size >= a plane dimension: REFLECT101 folds more than once)
_BLUR_SHAPES = _STAGE_SHAPES + [(5, 300), (53, 4)]


@gpu_mark
@pytest.mark.parametrize("border", [4, 1], ids=["reflect101", "replicate"])
@pytest.mark.parametrize("shape", _BLUR_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_gaussian_blur_form_matches_oracle_and_the_other_forms(gpu, oracle, shape, border):
    """The generic kernel with the one-fold border index (FAST) and with the reference's full BrdReflect101 formula, the tiled kernel
    (half sizes 1, 2, 3, 4, 9, 19), and the table kernels that read a pitched 8-bit / float pair of the caller's in place.  Half sizes
    up to 19 on planes down to 4 columns / 5 rows: where the half size reaches a plane dimension only the full formula may run (the
    one-fold forms must refuse).  Out there BrdReflect101's modulo wraps instead of folding a second time
    (test_oracle_blur_border_is_a_reflection_while_the_half_size_stays_below_the_plane); oracle and kernel state that same formula, so
    equality is asked for every half size."""
    import torch
    from opencv_contrib_amd import capi, cuda
    h, w = shape
    rng = np.random.default_rng(2)
    img = rng.random(shape, dtype=np.float32) * 255
    u8 = [rng.integers(0, 256, shape, dtype=np.uint8) for _ in range(2)]
    t = T(img, gpu)
    for kh in (1, 2, 3, 4, 5, 6, 8, 9, 19):
        ksize, sigma = 2 * kh + 1, 0.3 * kh + 0.8
        ref = oracle.fb_gaussian_blur(img, ksize, sigma, border)
        one_fold = kh < w and kh < h
        has_tile = one_fold and kh in (1, 2, 3, 4, 9, 19)
        tag = f"{shape} half {kh} border {border}"
        _same(N(cuda.farneback_gaussianBlur_form("generic_full", t, ksize, sigma, border)), ref, tag + ": generic, full border formula, vs oracle")
        _same(N(cuda.farneback_gaussianBlur(t, ksize, sigma, border)), ref, tag + ": the stage entry vs oracle")
        for form, ok in (("generic_fast", one_fold), ("tiled", has_tile)):
            if ok:
                _same(N(cuda.farneback_gaussianBlur_form(form, t, ksize, sigma, border)), ref, f"{tag}: {form} vs oracle")
            else:
                with pytest.raises(capi.MiError):
                    cuda.farneback_gaussianBlur_form(form, t, ksize, sigma, border)
        if border != 4:
            continue
        # table forms: pitched sources read in place, 8-bit converted on the fly; the oracle blurs the converted image
        b8 = [torch.full((h, w + 7), 77, dtype=torch.uint8, device=gpu) for _ in range(2)]
        bf = [torch.full((h, w + 5), 1e9, dtype=torch.float32, device=gpu) for _ in range(2)]
        for k in range(2):
            b8[k][:, 3:3 + w] = T(u8[k], gpu)
            bf[k][:, 1 + k:1 + k + w] = T(img if k == 0 else img[::-1, ::-1], gpu)
        srcs = {"8-bit": ([b8[0][:, 3:3 + w], b8[1][:, 3:3 + w]], [u8[0].astype(np.float32), u8[1].astype(np.float32)]),
                "float": ([bf[0][:, 1:1 + w], bf[1][:, 2:2 + w]], [img, np.ascontiguousarray(img[::-1, ::-1])])}
        for name, (views, hosts) in srcs.items():
            if has_tile:
                d0, d1 = cuda.farneback_gaussianBlur_form("table", views[0], ksize, sigma, border, src1=views[1])
                _same(N(d0), oracle.fb_gaussian_blur(hosts[0], ksize, sigma, border), f"{tag}: table form, {name} frame 0 vs oracle")
                _same(N(d1), oracle.fb_gaussian_blur(hosts[1], ksize, sigma, border), f"{tag}: table form, {name} frame 1 vs oracle")
            else:
                with pytest.raises(capi.MiError):
                    cuda.farneback_gaussianBlur_form("table", views[0], ksize, sigma, border, src1=views[1])


@gpu_mark
@pytest.mark.parametrize("border", [1, 4])
@pytest.mark.parametrize("ksize,sigma", [(3, 0.0), (9, 1.5), (39, 7.5)])
def test_gaussian_blur_and_pyr_down_match_oracle(gpu, oracle, border, ksize, sigma):
    from opencv_contrib_amd import cuda
    img = np.random.default_rng(2).random((53, 300), dtype=np.float32) * 255
    _same(N(cuda.farneback_gaussianBlur(T(img, gpu), ksize, sigma, border)), oracle.fb_gaussian_blur(img, ksize, sigma, border), "gaussian_blur")
    if border == 4 and ksize == 3:
        for shp in ((53, 300), (32, 33), (7, 9)):
            im = np.random.default_rng(3).random(shp, dtype=np.float32)
            np.testing.assert_array_equal(N(cuda.pyrDown(T(im, gpu))), oracle.fb_pyr_down(im))


def _assert_flow_equal(flow, ref, what=""):
    _assert_flow(flow, ref, what)   # tests/fb_flow_check.py: the one whole-calc criterion, shared with test_golden.py and test_ref_class_gpu.py


@gpu_mark
@pytest.mark.parametrize("pyrScale", [0.3, 0.5, 0.8])
@pytest.mark.parametrize("polyN,sigma", [(5, 1.1), (7, 1.5)])
@pytest.mark.parametrize("flags", [0, 256])
def test_calc_matches_oracle_reference_test_parameters(gpu, oracle, pyrScale, polyN, sigma, flags):
    """Parameter grid of cudaoptflow/test/test_optflow.cpp:307-356 (pyrScale x polyN x flags), RubberWhale-size
    synthetic pair (584x388)."""
    from opencv_contrib_amd import cuda
    I0, I1, _ = synth.flow_pair(388, 584, seed=31, dtype="u8")
    p = oracle.fb_params(pyr_scale=pyrScale, poly_n=polyN, poly_sigma=sigma, flags=flags)
    ref = oracle.fb_calc(I0, I1, p)
    alg = cuda.FarnebackOpticalFlow.create(pyrScale=pyrScale, polyN=polyN, polySigma=sigma, flags=flags)
    flow = N(alg.calc(T(I0, gpu), T(I1, gpu)))
    _assert_flow_equal(flow, ref)


@gpu_mark
def test_calc_config1_defaults_640x480(gpu, oracle):
    """BASELINE configs[0] workload on the GPU path vs the oracle, plus accuracy against the analytic flow."""
    from opencv_contrib_amd import cuda
    I0, I1, gt = synth.flow_pair(480, 640, seed=1234, dtype="u8")
    ref = oracle.fb_calc(I0, I1)
    alg = cuda.FarnebackOpticalFlow.create()
    assert alg.getDefaultName() == "DenseOpticalFlow.FarnebackOpticalFlow" and alg.getWinSize() == 13
    flow = N(alg.calc(T(I0, gpu), T(I1, gpu)))
    _assert_flow_equal(flow, ref)
    assert synth.epe(flow[40:-40, 40:-40], gt[40:-40, 40:-40]) < 0.08


@gpu_mark
def test_calc_initial_flow_fast_pyramids_f32_and_pitched(gpu, oracle):
    import torch
    from opencv_contrib_amd import cuda
    I0, I1, gt = synth.flow_pair(240, 320, seed=5, dtype="u8")
    # fastPyramids
    ref = oracle.fb_calc(I0, I1, oracle.fb_params(fast_pyramids=1))
    alg = cuda.FarnebackOpticalFlow.create(fastPyramids=True)
    _assert_flow_equal(N(alg.calc(T(I0, gpu), T(I1, gpu))), ref)
    # initial flow (flags = USE_INITIAL_FLOW), pitched float frames and pitched flow
    F0, F1 = I0.astype(np.float32), I1.astype(np.float32)
    ref = oracle.fb_calc(F0, F1, oracle.fb_params(flags=4, num_iters=3, num_levels=3), init_flow=gt)
    buf0 = torch.zeros((240, 384), dtype=torch.float32, device=gpu); buf1 = torch.zeros((240, 352), dtype=torch.float32, device=gpu)
    fbuf = torch.zeros((240, 330, 2), dtype=torch.float32, device=gpu)
    buf0[:, 5:325] = T(F0, gpu); buf1[:, 1:321] = T(F1, gpu); fbuf[:, 3:323] = T(gt, gpu)
    alg = cuda.FarnebackOpticalFlow.create(numLevels=3, numIters=3, flags=cuda.OPTFLOW_USE_INITIAL_FLOW)
    out = alg.calc(buf0[:, 5:325], buf1[:, 1:321], fbuf[:, 3:323])
    _assert_flow_equal(N(out), ref)


@gpu_mark
def test_calc_argument_errors_and_determinism(gpu):
    import torch
    from opencv_contrib_amd import cuda, capi
    a = torch.zeros((64, 80), dtype=torch.uint8, device=gpu)
    with pytest.raises(capi.MiError):
        cuda.FarnebackOpticalFlow.create(polyN=6).calc(a, a)
    with pytest.raises(capi.MiError):
        cuda.FarnebackOpticalFlow.create(fastPyramids=True, pyrScale=0.8).calc(a, a)
    with pytest.raises(capi.MiError):
        cuda.FarnebackOpticalFlow.create().calc(a, a[:, :40])
    I0, I1, _ = synth.flow_pair(200, 300, seed=9, dtype="u8")
    alg = cuda.FarnebackOpticalFlow.create()
    f1 = N(alg.calc(T(I0, gpu), T(I1, gpu)))
    f2 = N(cuda.FarnebackOpticalFlow.create().calc(T(I0, gpu), T(I1, gpu)))
    np.testing.assert_array_equal(f1, f2)


@gpu_mark
@pytest.mark.parametrize("kw", [dict(), dict(fastPyramids=True), dict(flags=256, winSize=9), dict(flags=4)],
                         ids=["defaults", "fast_pyramids", "gaussian", "initial_flow"])
def test_calc_batch_equals_single_calcs(gpu, oracle, kw):
    """mi_farneback_calc_batch (blockIdx.z = pair in every kernel of the level loop): every pair of a batch of distinct
    pairs equals, bit for bit, the single calc() of that pair -- and with it the oracle -- for the default path, fast pyramids,
    the Gaussian window and a caller-supplied initial flow."""
    import torch
    from opencv_contrib_amd import cuda
    pairs = [synth.flow_pair(240, 320, seed=60 + k, dtype="u8")[:2] for k in range(5)]
    I0s, I1s = [T(p[0], gpu) for p in pairs], [T(p[1], gpu) for p in pairs]
    alg, one = cuda.FarnebackOpticalFlow.create(**kw), cuda.FarnebackOpticalFlow.create(**kw)
    flows = None
    if kw.get("flags", 0) & 4:   # OPTFLOW_USE_INITIAL_FLOW: flows carry the initial guess in, the result out
        rng = np.random.default_rng(3)
        init = [torch.from_numpy((rng.standard_normal((240, 320, 2)) * 0.5).astype(np.float32)).to(gpu) for _ in range(5)]
        flows = torch.stack(init).clone()
        singles = [one.calc(I0s[k], I1s[k], init[k].clone()) for k in range(5)]
    else:
        singles = [one.calc(I0s[k], I1s[k]).clone() for k in range(5)]
    out = alg.calc_batch(I0s, I1s, flows)
    torch.cuda.synchronize()
    for k in range(5):
        assert torch.equal(out[k], singles[k]), f"pair {k}"
    assert not torch.equal(out[0], out[1])
    if not kw.get("flags", 0) & 4:
        p = oracle.fb_params(fast_pyramids=int(kw.get("fastPyramids", False)), flags=kw.get("flags", 0), win_size=kw.get("winSize", 13))
        _assert_flow_equal(N(out[3]), oracle.fb_calc(pairs[3][0], pairs[3][1], p))
    # a smaller batch through the same handle afterwards (capacity is kept), and a larger one (arena regrown)
    again = alg.calc_batch(I0s[:2], I1s[:2], None if flows is None else torch.stack(init[:2]).clone())
    assert torch.equal(again[1], singles[1])


@gpu_mark
@pytest.mark.parametrize("kw", [dict(), dict(flags=4, fastPyramids=True)], ids=["defaults", "initial_flow_fast_pyramids"])
def test_large_batch_runs_in_cache_sized_groups_and_equals_single_calcs(gpu, kw):
    """Round 5: a large batch walks the level loop in groups of pairs whose planes fit the last-level cache (MIFLOW_FB_GROUP_MB,
    farneback_api.cpp calc) and converts / merges 64 pairs per launch.  70 pairs of 240 x 320 are three groups with a ragged last one
    and two convert launches with a ragged second one: every pair still equals its single calc() bit for bit."""
    import torch
    from opencv_contrib_amd import cuda
    pairs = [synth.flow_pair(240, 320, seed=80 + k, dtype="u8")[:2] for k in range(5)]
    I0s, I1s = [T(p[0], gpu) for p in pairs], [T(p[1], gpu) for p in pairs]
    alg, one = cuda.FarnebackOpticalFlow.create(**kw), cuda.FarnebackOpticalFlow.create(**kw)
    B, flows = 70, None
    if kw.get("flags", 0) & 4:
        rng = np.random.default_rng(5)
        init = [torch.from_numpy((rng.standard_normal((240, 320, 2)) * 0.5).astype(np.float32)).to(gpu) for _ in range(5)]
        flows = torch.stack([init[k % 5] for k in range(B)]).clone()
        singles = [one.calc(I0s[k], I1s[k], init[k].clone()).clone() for k in range(5)]
    else:
        singles = [one.calc(I0s[k], I1s[k]).clone() for k in range(5)]
    out = alg.calc_batch([I0s[k % 5] for k in range(B)], [I1s[k % 5] for k in range(B)], flows)
    torch.cuda.synchronize()
    for k in range(B):
        assert torch.equal(out[k], singles[k % 5]), f"pair {k}"


def test_call_plan_host_arithmetic(tmp_path):
    """tests/cpp/fb_plan_test.cpp: the plan of a mi_farneback_calc_batch call (csrc/fb_plan.h, round 6 -- the level crop and geometry of
    cudaoptflow/src/farneback.cpp:330-395, how each level's flow starts, fused / plain zoom, pair groups, two iterations per launch) for
    the class defaults, the bench's batch, the initial-flow and zero-iteration cases, fast pyramids, forced switches, and its invariants
    over a sweep of shapes; the form rules against a table, the scratch layout, and the ordered launch list: exact for four calls, and over
    the sweep no plane read before an entry wrote it, every launch kind covering the batch once, chains inside fork / join, M and bufM
    alternating.  mi_farneback_calc_batch only executes the list.  Plain C++, no device."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "fb_plan_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(root, "opencv_contrib_amd", "csrc"),
                        os.path.join(root, "tests", "cpp", "fb_plan_test.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "fb_plan_test: ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(), dict(winSize=9), dict(winSize=15), dict(winSize=21), dict(winSize=11), dict(winSize=5, numIters=1),
                                dict(flags=256), dict(polyN=7, polySigma=1.5), dict(fastPyramids=True), dict(numLevels=1), dict(pyrScale=0.8, numLevels=8)],
                         ids=["defaults_win13", "win9", "win15", "win21", "win11_generic", "win5_one_iteration", "gaussian", "poly7", "fast_pyramids",
                              "one_level", "scale0.8"])
@pytest.mark.parametrize("shape,B", [((120, 160), 1), ((97, 203), 3), ((480, 640), 1), ((240, 320), 40)])
def test_no_plane_is_read_before_it_is_written(gpu, kw, shape, B):
    """the coarsest level's flow planes are never cleared -- the first matrix update takes the flow as zero and every iterate
    variant (tiled, narrow 64 x 4 tiles, two iterations per launch, the generic window sizes, Gaussian windows, pair groups on two
    streams) must write all w x h pixels of both planes before anything reads them.  A calc whose scratch arena was filled with NaNs
    (miflow_selftest_farneback_poison) must give the bytes of the calc before it: a stale read would turn up as NaNs or as a changed flow."""
    import torch
    from opencv_contrib_amd import capi, cuda
    pairs = [synth.flow_pair(*shape, seed=600 + k, dtype="u8")[:2] for k in range(min(B, 4))]
    I0s = [torch.from_numpy(pairs[k % len(pairs)][0]).to(gpu) for k in range(B)]
    I1s = [torch.from_numpy(pairs[k % len(pairs)][1]).to(gpu) for k in range(B)]
    alg = cuda.FarnebackOpticalFlow.create(**kw)
    run = (lambda: alg.calc(I0s[0], I1s[0]).clone()) if B == 1 else (lambda: alg.calc_batch(I0s, I1s).clone())
    a = run()
    torch.cuda.synchronize()
    capi.check(capi.lib().miflow_selftest_farneback_poison(alg._h, capi.current_stream_ptr()))
    b = run()
    torch.cuda.synchronize()
    assert torch.isfinite(b).all()
    assert torch.equal(a, b)


def test_pair_group_plan_host_arithmetic(tmp_path):
    """tests/cpp/fb_groups_test.cpp: the plan of the batched level loop (csrc/fb_groups.h -- pairs per launch group, one or two chains)
    for the bench's shape, the sizes where no groups are formed, and its invariants over a sweep (groups cover the batch, the groups in
    flight stay inside the cache budget).  Plain C++, no device."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "fb_groups_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(root, "opencv_contrib_amd", "csrc"),
                        os.path.join(root, "tests", "cpp", "fb_groups_test.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "fb_groups_test: ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_pair_group_budget_never_changes_a_flow(gpu):
    """MIFLOW_FB_GROUP_MB (read once per process, hence the subprocesses) only decides how many pairs a launch of a large level covers
    and on which of the handle's two streams a group's chain runs: whole-batch launches (0), the default and a budget that leaves one
    pair per group give the same bytes for a 12-pair 640 x 480 batch."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    digests = {}
    for mb in ("0", None, "30"):
        env = dict(os.environ)
        env.pop("MIFLOW_FB_GROUP_MB", None)
        if mb is not None:
            env["MIFLOW_FB_GROUP_MB"] = mb
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "fb_batch.py"), "12", "1", "640", "480"], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        digests[mb] = re.search(r"digest ([0-9a-f]+)", r.stdout).group(1)
    assert len(set(digests.values())) == 1, digests


@pytest.mark.gpu
@pytest.mark.parametrize("mb", ["6", "20"])
def test_random_batches_in_many_small_pair_groups_equal_single_calcs(gpu, mb):
    """tools/fb_stress.py under a pair-group budget of a few MB (every level of every call is cut into many groups on two streams): random
    sizes, 2..40 pairs, 8-bit / float frames, pitched ROI inputs (the pre-blur reads them in place), window sizes, pyramid parameters, the fast
    pyramid -- each batch equals the single calc()s of its pairs bit for bit."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fb_stress.py"), "8", mb], capture_output=True, text=True,
                       env=dict(os.environ, MIFLOW_FB_GROUP_MB=mb), timeout=900)
    assert r.returncode == 0 and "fb_stress: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@gpu_mark
@pytest.mark.parametrize("batch", [1, 12], ids=["one_pair", "batch_in_groups"])
def test_calc_captured_into_a_graph_by_the_caller_replays_the_same_flow(gpu, batch):
    """A caller may capture calc() / calc_batch() into a HIP graph (torch.cuda.CUDAGraph here) and replay it: no call of the level loop
    synchronises or allocates once the handle has its arena, and a batch whose levels run in pair groups stays ONE chain while its
    stream is being captured (the second chain lives on a stream of the handle's own, which a capture must not touch).  The replay
    writes the bytes of the plain call."""
    import torch
    from opencv_contrib_amd import cuda
    pairs = [synth.flow_pair(480, 640, seed=300 + k, dtype="u8")[:2] for k in range(min(batch, 3))]
    I0 = [T(pairs[i % len(pairs)][0], gpu) for i in range(batch)]
    I1 = [T(pairs[i % len(pairs)][1], gpu) for i in range(batch)]
    alg = cuda.FarnebackOpticalFlow.create()
    run = (lambda out: alg.calc(I0[0], I1[0], out)) if batch == 1 else (lambda out: alg.calc_batch(I0, I1, out))
    out = run(None)
    torch.cuda.synchronize()
    ref = out.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(out)                      # the handle's arena and streams exist before the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run(out)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref)


def _random_fb_configs():
    rng = np.random.default_rng(int(os.environ.get("MIFLOW_SWEEP_SEED", "7702")))
    out = []
    for k in range(int(os.environ.get("MIFLOW_SWEEP_N", "24"))):
        out.append(dict(shape=(int(rng.integers(40, 300)), int(rng.integers(40, 420))), seed=int(rng.integers(1, 10 ** 6)),
                        winSize=int((9, 13, 15, 21, 11, 5, 27)[int(rng.integers(7))]),   # 9 / 13 / 15 / 21: tiled kernel; others: one-row kernel
                        flags=int((0, 256)[int(rng.integers(2))]), numLevels=int(rng.integers(1, 6)), numIters=int(rng.integers(1, 7)),
                        pyrScale=float((0.5, 0.7, 0.35)[int(rng.integers(3))]), fastPyramids=bool(rng.integers(2)),
                        batch=int((1, 1, 3)[int(rng.integers(3))])))
    return out


@gpu_mark
@pytest.mark.parametrize("cfg", _random_fb_configs(), ids=lambda c: f"{c['shape'][0]}x{c['shape'][1]}-w{c['winSize']}-f{c['flags']}-l{c['numLevels']}"
                                                                   f"-i{c['numIters']}-b{c['batch']}")
def test_random_configuration_matches_oracle(gpu, oracle, cfg):
    """Seeded sweep over frame sizes that are multiples of nothing (row / column tile edges of the tiled iteration kernel, its
    XCD-contiguous tile order, the mirror-step border indices of the pyramid blur), window sizes of the tiled and of the one-row
    kernel, box and Gaussian windows, pyramid depth and scale, fast pyramids, and batches."""
    from opencv_contrib_amd import cuda
    if cfg["fastPyramids"]:
        cfg = dict(cfg, pyrScale=0.5)   # CV_Assert(!fastPyramids || std::abs(pyrScale - 0.5) < 1e-6), farneback.cpp:317
    kw = dict(numLevels=cfg["numLevels"], pyrScale=cfg["pyrScale"], fastPyramids=cfg["fastPyramids"], winSize=cfg["winSize"],
              numIters=cfg["numIters"], flags=cfg["flags"])
    okw = dict(num_levels=cfg["numLevels"], pyr_scale=cfg["pyrScale"], fast_pyramids=int(cfg["fastPyramids"]), win_size=cfg["winSize"],
               num_iters=cfg["numIters"], flags=cfg["flags"])
    pairs = [synth.flow_pair(*cfg["shape"], seed=cfg["seed"] + b, dtype="u8") for b in range(cfg["batch"])]
    alg = cuda.FarnebackOpticalFlow.create(**kw)
    if cfg["batch"] == 1:
        flows = [alg.calc(T(pairs[0][0], gpu), T(pairs[0][1], gpu))]
    else:
        flows = list(alg.calc_batch([T(p[0], gpu) for p in pairs], [T(p[1], gpu) for p in pairs]))
    for b, p in enumerate(pairs):
        _assert_flow_equal(N(flows[b]), oracle.fb_calc(p[0], p[1], oracle.fb_params(**okw)))


@pytest.mark.gpu
def test_few_launch_forms_of_a_single_pair_are_bit_identical(gpu):
    """Round 4: a single pair is a chain of launch latencies, so small calls run forms with fewer / shorter
    launches -- 64 x 4 tiles (MIFLOW_FB_NARROW), the resize sampled inside poly_exp and the first matrix update + the merge written by
    the last iteration (MIFLOW_FB_FUSE), two iterations per launch on the coarse levels (MIFLOW_FB_PAIR).  Every one of them performs the same operations in the same order: the flow
    of a whole calc must not change by a bit.  The switches are read once per process, hence the subprocesses."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    digests = {}
    for name, env in (("plain", {"MIFLOW_FB_NARROW": "0", "MIFLOW_FB_FUSE": "0", "MIFLOW_FB_PAIR": "0"}), ("default", {}),
                      ("all_on", {"MIFLOW_FB_NARROW": "1", "MIFLOW_FB_FUSE": "1", "MIFLOW_FB_PAIR": "1"})):
        for (w, h) in ((640, 480), (333, 217)):
            r = subprocess.run([sys.executable, os.path.join(root, "tools", "fb_single.py"), str(w), str(h), "3"], capture_output=True, text=True,
                               env=dict(os.environ, **env), timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            digests[(name, w)] = [l.split("digest")[1].strip() for l in r.stdout.splitlines() if "digest" in l][0]
    for w in (640, 333):
        assert digests[("plain", w)] == digests[("default", w)] == digests[("all_on", w)], digests
