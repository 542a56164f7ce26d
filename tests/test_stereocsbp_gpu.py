"""cv::cuda::StereoConstantSpaceBP on the GPU: the HIP class and each of its kernels against the reference's recorded outputs
(tests/golden/stereocsbp_ref*.npz) and against the NumPy restatement (tests/stereocsbp_numpy_ref.py).  Equality throughout: every
operation is a correctly rounded f32 one or an integer one."""
import functools
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import stereocsbp_numpy_ref as R  # noqa: E402
import make_golden_stereocsbp as G  # noqa: E402
import test_stereocsbp_ref as T  # noqa: E402  (the fixtures' loaders and the restatement's stage wrappers)

pytestmark = pytest.mark.gpu
GOLDEN = T.GOLDEN
MSG = T.MSG
eq = np.testing.assert_array_equal
SETTERS = dict(max_data_term="setMaxDataTerm", data_weight="setDataWeight", max_disc_term="setMaxDiscTerm", disc_single_jump="setDiscSingleJump",
               min_disp="setMinDisparity", local="setUseLocalInitDataCost")


def _dev(a, gpu, pitched=False):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    if not pitched:
        return t
    big = torch.zeros((a.shape[0], a.shape[1] + 5) + a.shape[2:], dtype=t.dtype, device=gpu)
    big[:, :a.shape[1]] = t
    return big[:, :a.shape[1]]


def _csbp(cuda, kw):
    bp = cuda.createStereoConstantSpaceBP(kw["ndisp"], kw["iters"], kw["levels"], kw["nr_plane"], kw["msg_type"])
    for k, name in SETTERS.items():
        if k in kw:
            getattr(bp, name)(kw[k])
    return bp


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(h, w, cn, seed, items):
    """a pair and the restatement's (disparity, levels) for it, computed once"""
    left, right = R.synth_pair(h, w, cn, seed)
    disp, levels = R.compute(left, right, **dict(items))
    disp.setflags(write=False)
    return left, right, disp, levels


def _kw(msg, **kw):
    return tuple(sorted(dict(dict(ndisp=16, iters=3, levels=3, nr_plane=2), msg_type=MSG[msg], **kw).items()))


# ------------------------------------------------------------------ the class
def test_fixtures_present():
    assert len(T.CLASS_FILES) == 2 * len(G.CLASS_CASES) and len(T.STAGE_FILES) == 8


@pytest.mark.parametrize("path", T.CLASS_FILES, ids=T._ids(T.CLASS_FILES))
def test_compute_equals_reference_class(gpu, path):
    """the default path, 3 and 4 channels, global selection, min_disp, the level clamp (and getNumLevels afterwards), ndisp 2, more planes
    than disparities, a fractional max_disc_term, 16-bit saturation and the deep pyramid, for both message types"""
    from opencv_contrib_amd import cuda
    z = np.load(path)
    left, right, kw = T.class_inputs(z)
    bp = _csbp(cuda, kw)
    out = _np(bp.compute(_dev(left, gpu), _dev(right, gpu)))
    eq(out, z["disp"])
    assert bp.getNumLevels() == int(z["levels_after"])
    want, levels = T.class_restated(path)
    eq(out, want)
    assert levels == bp.getNumLevels()
    if "clamp" in path:
        assert kw["levels"] == 4 and bp.getNumLevels() == 2


@pytest.mark.parametrize("msg", ["f32", "s16"])
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_compute_pitched(gpu, cn, msg):
    from opencv_contrib_amd import cuda
    import torch
    items = _kw(msg, min_disp=1)
    left, right, want, _ = _case(29, 37, cn, 40 + cn, items)
    out = torch.full((29, 37 + 7), -5, dtype=torch.int16, device=gpu)
    _csbp(cuda, dict(items)).compute(_dev(left, gpu, True), _dev(right, gpu, True), out[:, :37])
    eq(_np(out)[:, :37], want)
    assert (_np(out)[:, 37:] == -5).all()


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int32, np.float32])
def test_compute_output_types(gpu, dtype):
    import torch
    from opencv_contrib_amd import cuda
    items = _kw("f32")
    left, right, want, _ = _case(29, 37, 1, 41, items)
    out = torch.zeros((29, 37), dtype=getattr(torch, np.dtype(dtype).name), device=gpu)
    res = _csbp(cuda, dict(items)).compute(_dev(left, gpu), _dev(right, gpu), out)
    assert res.dtype == out.dtype
    eq(_np(res), R.convert_disp(want, dtype))


def test_handle_reuse_across_sizes_and_params(gpu):
    """one handle, other sizes, channels, message types and parameters in turn, then the first again: stale scratch (the sets are zeroed
    by every compute) changes nothing"""
    from opencv_contrib_amd import cuda
    seq = [((29, 37, 1, 50), _kw("f32")), ((21, 23, 3, 51), _kw("s16", levels=2, nr_plane=3, local=False)),
           ((45, 67, 4, 52), _kw("f32", ndisp=32, levels=4, nr_plane=1)), ((29, 37, 1, 50), _kw("f32"))]
    bp = cuda.createStereoConstantSpaceBP(16, 3, 3, 2)
    for shape, items in seq:
        kw = dict(items)
        bp.setNumDisparities(kw["ndisp"]); bp.setNumIters(kw["iters"]); bp.setNumLevels(kw["levels"]); bp.setNrPlane(kw["nr_plane"])
        bp.setMsgType(kw["msg_type"]); bp.setUseLocalInitDataCost(kw.get("local", True))
        left, right, want, _ = _case(*shape, items)
        eq(_np(bp.compute(_dev(left, gpu), _dev(right, gpu))), want)
    assert (bp.getNumDisparities(), bp.getNumIters(), bp.getNumLevels(), bp.getNrPlane(), bp.getMsgType()) == (16, 3, 3, 2, R.CV_32F)
    assert (bp.getBlockSize(), bp.getSpeckleWindowSize(), bp.getSpeckleRange(), bp.getDisp12MaxDiff()) == (0,) * 4
    with pytest.raises(NotImplementedError):
        bp.compute_data(None)


def test_two_handles_on_two_streams(gpu):
    """parameters travel as kernel arguments: two handles with different weights, interleaved on two streams, give their own results"""
    import torch
    from opencv_contrib_amd import cuda
    ia, ib = _kw("f32"), _kw("s16", data_weight=0.5, disc_single_jump=4.5, max_data_term=20.0, max_disc_term=33.7, min_disp=2)
    left, right, wa, _ = _case(29, 37, 1, 60, ia)
    wb = _case(29, 37, 1, 60, ib)[2]
    a, b = _csbp(cuda, dict(ia)), _csbp(cuda, dict(ib))
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    L, Rt = _dev(left, gpu), _dev(right, gpu)
    torch.cuda.synchronize()
    outs = [(a.compute(L, Rt, stream=sa), b.compute(L, Rt, stream=sb)) for _ in range(3)]
    for oa, ob in outs:
        eq(_np(oa), wa)
        eq(_np(ob), wb)


def test_pipeline_with_disparity_bilateral_filter(gpu, oracle):
    """the pipeline the filter exists for: constant-space belief propagation refined by the joint bilateral filter"""
    from opencv_contrib_amd import cuda
    items = _kw("s16", iters=4)
    left, right, want, _ = _case(48, 64, 1, 42, items)
    L = _dev(left, gpu)
    disp = _csbp(cuda, dict(items)).compute(L, _dev(right, gpu))
    out = cuda.createDisparityBilateralFilter(16, 3, 2).apply(disp, L)
    eq(_np(disp), want)
    eq(_np(out), oracle.dbf_apply(np.array(want), left, oracle.dbf_params(ndisp=16, radius=3, iters=2)))


# ------------------------------------------------------------------ the stage entries
@pytest.mark.parametrize("msg", ["f32", "s16"])
@pytest.mark.parametrize("level", range(8))
def test_stage_init_data_cost(gpu, level, msg):
    """every level 0-7 (the plain form and every reduce width) on the smallest image with a 3 x 3 level, 1 / 3 / 4 channels, local and
    global selection; ndisp 5, and 70 where winsz <= 32"""
    from opencv_contrib_amd import cuda
    z = np.load(os.path.join(GOLDEN, f"stereocsbp_refstage_init_{msg}.npz"))
    n = 0
    for key, lv, cn, local, ndisp, min_disp in T.init_stage_cases():
        if lv != level:
            continue
        left, right = T.init_stage_images(level, cn)
        cost, disp = cuda.stereocsbp_init_data_cost(_dev(left, gpu), _dev(right, gpu), level, 4, ndisp, MSG[msg], local, min_disp=min_disp)
        eq(_np(cost), z[key + "_cost"], err_msg=key)
        eq(_np(disp), z[key + "_disp"], err_msg=key)
        n += 1
    assert n == (12 if level <= 5 else 6)


@pytest.mark.parametrize("msg", ["f32", "s16"])
@pytest.mark.parametrize("local", [True, False])
@pytest.mark.parametrize("ndisp", [63, 64, 65, 4096, 4097])
def test_stage_first_k_forms(gpu, ndisp, local, msg):
    """the selection kernel at its lane-count edges and on both sides of the threshold between the wave-per-pixel form (ndisp <= 4096)
    and the lane-per-pixel form, against the restatement; 7 x 9 pixels at level 0, more planes asked for than local minima exist"""
    from opencv_contrib_amd import cuda
    left, right = R.synth_pair(7, 9, 1, 300 + ndisp)
    cost, disp = cuda.stereocsbp_init_data_cost(_dev(left, gpu), _dev(right, gpu), 0, 40, ndisp, MSG[msg], local, data_weight=3.0)
    want_cost, want_disp = R.init_data_cost(left, right, 0, 40, ndisp, MSG[msg], local, data_weight=3.0)
    eq(_np(cost), T.planar(want_cost))
    eq(_np(disp), T.planar(want_disp))


@pytest.mark.parametrize("msg,cn", [("f32", 1), ("f32", 3), ("s16", 1), ("s16", 3)])
def test_stage_compute_data_cost_and_init_message(gpu, msg, cn):
    """compute_data_cost at levels 0, 1, 2, 5 and 6 with random parent candidates (below min_disp and beyond x included); init_message with
    nr_plane 1, 2, 4 and 16 and frequent ties"""
    from opencv_contrib_amd import cuda
    z = np.load(os.path.join(GOLDEN, f"stereocsbp_refstage_chain_{msg}_c{cn}.npz"))
    for level, rows, cols in G.DATA_COST_CASES:
        left, right = R.synth_pair(rows, cols, cn, 200 + level)
        out = cuda.stereocsbp_compute_data_cost(_dev(left, gpu), _dev(right, gpu), level, _dev(z[f"dc{level}_parent"], gpu), 6, min_disp=2)
        eq(_np(out), z[f"dc{level}_out"], err_msg=f"level {level}")
    for n in G.INIT_MESSAGE_PLANES:
        new, sel = cuda.stereocsbp_init_message([_dev(a, gpu) for a in z[f"im{n}_cur"]], _dev(z[f"im{n}_dc"], gpu), n, 2 * n)
        eq(np.stack([_np(a) for a in new]), z[f"im{n}_new"], err_msg=f"nr_plane {n}")
        eq(_np(sel), z[f"im{n}_sel"], err_msg=f"nr_plane {n}")


@functools.lru_cache(maxsize=None)
def _iter_inputs(msg, h, w, n):
    dt = R.msg_dtype(MSG[msg])
    rng = np.random.default_rng(1000 * h + 10 * n + (msg == "s16"))
    msgs = G.rand_msgs(rng, dt, (4, n * h, w))
    if msg == "s16":
        msgs[rng.random(msgs.shape) < 0.03] = 32000   # sums of shorts that wrap
    return msgs, rng.integers(0, 40, (n * h, w)).astype(dt), G.rand_msgs(rng, dt, (n * h, w), 0, 200)


@functools.lru_cache(maxsize=None)
def _iter_want(msg, h, w, n, t0, n_iters):
    msgs, sel_disp, sel_cost = _iter_inputs(msg, h, w, n)
    return T.restate_iterations(msgs, sel_disp, sel_cost, n, t0, n_iters, 25.9, 1.5)


ITER_RUNS = [(0, 1), (1, 1), (0, 3), (1, 3)]
REG_PLANES = [4, 3, 8, 7, 16, 15, 32, 31, 64, 63]   # every register capacity, full and one short


def _iterate(cuda, gpu, msg, h, w, n, t0, n_iters, form):
    msgs, sel_disp, sel_cost = _iter_inputs(msg, h, w, n)
    out = cuda.stereocsbp_iterate([_dev(a, gpu) for a in msgs], _dev(sel_disp, gpu), _dev(sel_cost, gpu), n, t0, n_iters, form,
                                  max_disc_term=25.9, disc_single_jump=1.5)
    return np.stack([_np(a) for a in out])


@pytest.mark.parametrize("msg", ["f32", "s16"])
@pytest.mark.parametrize("h,w", [(9, 11), (8, 70)])
@pytest.mark.parametrize("n", REG_PLANES)
def test_stage_iterate_register_form(gpu, n, h, w, msg):
    """the register form at nr_plane = capacity and capacity - 1, both parities, one and three half-sweeps: equal to the restatement and
    to the general form; max_disc_term 25.9 travels as 25"""
    from opencv_contrib_amd import capi, cuda
    for t0, n_iters in ITER_RUNS:
        reg = _iterate(cuda, gpu, msg, h, w, n, t0, n_iters, capi.MI_STEREOCSBP_FORM_REG)
        eq(reg, _iter_want(msg, h, w, n, t0, n_iters), err_msg=str((t0, n_iters)))
        eq(reg, _iterate(cuda, gpu, msg, h, w, n, t0, n_iters, capi.MI_STEREOCSBP_FORM_GEN), err_msg=str((t0, n_iters)))
        eq(reg, _iterate(cuda, gpu, msg, h, w, n, t0, n_iters, capi.MI_STEREOCSBP_FORM_AUTO), err_msg=str((t0, n_iters)))


@pytest.mark.parametrize("msg", ["f32", "s16"])
@pytest.mark.parametrize("h,w", [(9, 11), (8, 70)])
@pytest.mark.parametrize("n", [3, 65])
def test_stage_iterate_general_form(gpu, n, h, w, msg):
    from opencv_contrib_amd import capi, cuda
    for t0, n_iters in ITER_RUNS:
        eq(_iterate(cuda, gpu, msg, h, w, n, t0, n_iters, capi.MI_STEREOCSBP_FORM_GEN), _iter_want(msg, h, w, n, t0, n_iters), err_msg=str((t0, n_iters)))


@pytest.mark.parametrize("msg", ["f32", "s16"])
def test_stage_iterate_and_disp_equal_reference_kernels(gpu, msg):
    from opencv_contrib_amd import capi, cuda
    z = np.load(os.path.join(GOLDEN, f"stereocsbp_refstage_iter_{msg}.npz"))
    for h, w, n in G.ITER_CASES:
        key = f"it{h}x{w}_{n}"
        args = ([_dev(a, gpu) for a in z[key + "_msgs"]], _dev(z[key + "_disp"], gpu), _dev(z[key + "_cost"], gpu), n)
        for iters in ((1, 3) if n <= 4 else (3,)):
            for form in (capi.MI_STEREOCSBP_FORM_GEN,) + ((capi.MI_STEREOCSBP_FORM_REG,) if n <= 64 else ()):
                out = cuda.stereocsbp_iterate(*args, 0, iters, form, max_disc_term=25.0, disc_single_jump=1.5)
                eq(np.stack([_np(a) for a in out]), z[f"{key}_out{iters}"], err_msg=f"{key} form {form}")
    key = "it9x11_4"
    sel_disp, sel_cost = _dev(z[key + "_disp"], gpu), _dev(z[key + "_cost"], gpu)
    eq(_np(cuda.stereocsbp_compute_disp([_dev(a, gpu) for a in z[key + "_out3"]], sel_disp, sel_cost, 4)), z["cd_disp"])
    # border 0, ties to the first candidate
    tie = _dev(np.full_like(z[key + "_cost"], 7), gpu)
    zero = [_dev(np.zeros_like(a), gpu) for a in z[key + "_msgs"]]
    out = _np(cuda.stereocsbp_compute_disp(zero, sel_disp, tie, 4))
    eq(out, z["cd_tie_disp"])
    eq(out[1:-1, 1:-1], z[key + "_disp"][:9][1:-1, 1:-1].astype(np.int16))
    assert not out[0].any() and not out[-1].any() and not out[:, 0].any() and not out[:, -1].any()
    import torch
    for dtype in (np.uint8, np.int32, np.float32):
        res = cuda.stereocsbp_compute_disp(zero, sel_disp, tie, 4, dtype=getattr(torch, np.dtype(dtype).name))
        eq(_np(res), R.convert_disp(z["cd_tie_disp"], dtype))


def test_stage_iterate_rejects_register_form_beyond_its_capacity(gpu):
    from opencv_contrib_amd import capi, cuda
    msgs, sel_disp, sel_cost = _iter_inputs("f32", 9, 11, 65)
    with pytest.raises(capi.MiError) as e:
        cuda.stereocsbp_iterate([_dev(a, gpu) for a in msgs], _dev(sel_disp, gpu), _dev(sel_cost, gpu), 65, 0, 1, capi.MI_STEREOCSBP_FORM_REG)
    assert e.value.code == -1 and "register form" in str(e.value)


def test_stage_entries_take_pitched_matrices(gpu):
    """one step for the matrices of a level, wider than the level"""
    import ctypes as C
    import torch
    from opencv_contrib_amd import capi, cuda
    msgs, sel_disp, sel_cost = _iter_inputs("s16", 9, 11, 4)
    temp = _dev(np.zeros_like(sel_cost), gpu, True)
    p = cuda._csbp_params(R.CV_16S, max_disc_term=25.9, disc_single_jump=1.5)
    for form in (capi.MI_STEREOCSBP_FORM_REG, capi.MI_STEREOCSBP_FORM_GEN):
        out = [_dev(a, gpu, True) for a in msgs]
        sd, sc = _dev(sel_disp, gpu, True), _dev(sel_cost, gpu, True)   # named: they must outlive the launch
        capi.check(capi.lib().mi_stereocsbp_iterate(C.byref(p), cuda._mats(out), C.byref(cuda._m(sd)), C.byref(cuda._m(sc)),
                                                    C.byref(cuda._m(temp)), 4, 0, 3, form, capi.current_stream_ptr()))
        torch.cuda.synchronize()
        eq(np.stack([_np(a) for a in out]), _iter_want("s16", 9, 11, 4, 0, 3))


# ------------------------------------------------------------------ argument checks
def test_argument_checks(gpu):
    """the reference's asserts as error codes with the asserted condition as text, in the reference's order"""
    import torch
    from opencv_contrib_amd import cuda
    from opencv_contrib_amd.capi import MiError
    img = torch.zeros((24, 32), dtype=torch.uint8, device=gpu)

    def fails(code, text, fn):
        with pytest.raises(MiError) as e:
            fn()
        assert e.value.code == code and text in str(e.value), str(e.value)

    make = cuda.createStereoConstantSpaceBP
    for args in ((0, 2, 2, 2), (16, 0, 2, 2), (16, 2, 0, 2), (16, 2, 2, 0), (1024, 2, 9, 2)):
        fails(-1, "0 < ndisp_ && 0 < iters_ && 0 < levels_ && 0 < nr_plane_ && levels_ <= 8", lambda: make(*args).compute(img, img))
    fails(-1, "msg_type_ == CV_32F || msg_type_ == CV_16S", lambda: make(0, 2, 2, 2, 0).compute(img, img))   # the message type first
    fails(-1, "undefined in the reference", lambda: make(1, 2, 2, 2).compute(img, img))
    fails(-3, "undefined in the reference", lambda: make(256, 2, 6, 2).compute(img, img))                      # 24 >> 5 == 0
    ok = make(16, 2, 2, 2)
    ok.compute(img, img)
    fails(-1, "0 < ndisp_", lambda: make(0, 2, 2, 2).compute(img, img[:, :31]))                                # the counts before the images
    fails(-3, "left.size() == right.size()", lambda: ok.compute(img, img[:, :31]))
    fails(-3, "left.size() == right.size()", lambda: ok.compute(img, torch.zeros((24, 32, 3), dtype=torch.uint8, device=gpu)))
    fails(-2, "left.type() == CV_8UC1", lambda: ok.compute(img.to(torch.float32), img.to(torch.float32)))
    fails(-2, "disparity", lambda: ok.compute(img, img, torch.zeros((24, 32, 2), dtype=torch.float32, device=gpu)))
    fails(-3, "disparity", lambda: ok.compute(img, img, torch.zeros((24, 31), dtype=torch.int16, device=gpu)))
    # the stage entries: a level with odd sizes has pixels without a parent
    odd = torch.zeros((25, 32), dtype=torch.uint8, device=gpu)
    fails(-3, "even rows and cols", lambda: cuda.stereocsbp_compute_data_cost(odd, odd, 0, torch.zeros((2 * 12, 16), dtype=torch.float32, device=gpu), 2))


def test_argument_checks_allocate_nothing(gpu):
    """a rejected call leaves the handle's scratch as it was: empty on a fresh handle, unchanged on a used one"""
    import torch
    from opencv_contrib_amd import cuda
    from opencv_contrib_amd.capi import MiError
    img = torch.zeros((24, 32), dtype=torch.uint8, device=gpu)
    make = cuda.createStereoConstantSpaceBP
    bad = [make(0, 2, 2, 2), make(16, 2, 9, 2), make(16, 2, 2, 2, 1), make(1, 2, 2, 2), make(16, 2, 2, 2)]
    for bp in bad[:4]:
        with pytest.raises(MiError):
            bp.compute(img, img)
    with pytest.raises(MiError):
        bad[4].compute(img, img[:, :30])
    with pytest.raises(MiError):
        bad[4].compute(img, img, torch.zeros((24, 31), dtype=torch.int16, device=gpu))
    assert [bp.scratchBytes() for bp in bad] == [0] * 5
    bad[4].compute(img, img)
    used = bad[4].scratchBytes()
    assert used > 0
    bad[4].setNumLevels(9)
    with pytest.raises(MiError):
        bad[4].compute(img, img)
    assert bad[4].scratchBytes() == used
