"""cv::cuda::StereoBeliefPropagation on the GPU: the HIP class and each of its kernels against the reference's recorded outputs
(tests/golden/stereobp_ref*.npz) and against the NumPy restatement (tests/stereobp_numpy_ref.py).  Equality throughout: every
operation is a correctly rounded f32 one or an integer one."""
import functools
import glob
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stereobp_numpy_ref as R  # noqa: E402
from opencv_contrib_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden")
CLASS_FILES = sorted(glob.glob(os.path.join(GOLDEN, "stereobp_refclass_*.npz")))
STAGE_FILES = sorted(glob.glob(os.path.join(GOLDEN, "stereobp_refstage_*.npz")))
MSG = {"f32": R.CV_32F, "s16": R.CV_16S}
eq = np.testing.assert_array_equal


def _images(h, w, cn, seed, kind="random"):
    rng = np.random.default_rng(seed)
    if kind == "const":
        shape = (h, w) if cn == 1 else (h, w, cn)
        return np.full(shape, 77, np.uint8), np.full(shape, 77, np.uint8)
    if kind == "synth":
        left, right, _ = synth.stereo_pair(h, w, seed=seed, max_disp=12)
        if cn > 1:
            left = np.stack([np.roll(left, k, 1) for k in range(cn)], -1)
            right = np.stack([np.roll(right, k, 1) for k in range(cn)], -1)
        return np.ascontiguousarray(left), np.ascontiguousarray(right)
    shape = (h, w) if cn == 1 else (h, w, cn)
    left = rng.integers(0, 256, shape, dtype=np.uint8)
    right = np.roll(left, -2, 1) if seed & 1 else rng.integers(0, 256, shape, dtype=np.uint8)
    return left, np.ascontiguousarray(right)


@functools.lru_cache(maxsize=None)
def _ref_compute(h, w, cn, seed, kind, ndisp, iters, levels, msg, weights=()):
    left, right = _images(h, w, cn, seed, kind)
    out = R.compute(left, right, ndisp, iters, levels, MSG[msg], **dict(weights))
    out.setflags(write=False)
    return out


def _dev(a, gpu, pitched=False):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    if not pitched:
        return t
    big = torch.zeros((a.shape[0], a.shape[1] + 5) + a.shape[2:], dtype=t.dtype, device=gpu)
    big[:, :a.shape[1]] = t
    return big[:, :a.shape[1]]


def _bp(cuda, ndisp, iters, levels, msg, weights=()):
    bp = cuda.createStereoBeliefPropagation(ndisp, iters, levels, MSG[msg])
    w = dict(weights)
    if w:
        bp.setMaxDataTerm(w.get("max_data_term", 10.0)); bp.setDataWeight(w.get("data_weight", 0.07))
        bp.setMaxDiscTerm(w.get("max_disc_term", 1.7)); bp.setDiscSingleJump(w.get("disc_single_jump", 1.0))
    return bp


def _run(gpu, h, w, cn, seed, kind, ndisp, iters, levels, msg, weights=(), pitched=False, out_dtype=None):
    import torch
    from opencv_contrib_amd import cuda
    left, right = _images(h, w, cn, seed, kind)
    bp = _bp(cuda, ndisp, iters, levels, msg, weights)
    disp = None
    if out_dtype is not None or pitched:
        disp = _dev(np.full((h, w), 99, out_dtype or np.int16), gpu, pitched)
    out = bp.compute(_dev(left, gpu, pitched), _dev(right, gpu, pitched), disp)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ------------------------------------------------------------------ whole compute: the reference's own outputs
def test_fixtures_present():
    assert len(CLASS_FILES) >= 6 and len(STAGE_FILES) >= 2


@pytest.mark.parametrize("path", CLASS_FILES, ids=[os.path.basename(p)[:-4] for p in CLASS_FILES])
def test_compute_equals_reference_class(gpu, path):
    import torch
    from opencv_contrib_amd import cuda
    z = np.load(path)
    p = json.loads(str(z["params"]))
    bp = _bp(cuda, p["ndisp"], p["iters"], p["levels"], p["msg"], tuple(sorted(p["weights"].items())))
    if "data" in z.files:
        out = bp.compute_data(_dev(z["data"], gpu))
    else:
        out = bp.compute(_dev(z["left"], gpu), _dev(z["right"], gpu))
    torch.cuda.synchronize()
    eq(out.cpu().numpy(), z["disp"])


# ------------------------------------------------------------------ whole compute: the restatement
SHAPES = [(3, 3, 1), (4, 7, 1), (13, 11, 2), (37, 29, 3), (67, 41, 4), (9, 131, 1), (9, 129, 1)]


@pytest.mark.parametrize("msg", ["f32", "s16"])
@pytest.mark.parametrize("cn", [1, 3, 4])
@pytest.mark.parametrize("h,w,levels", SHAPES)
def test_compute_shapes(gpu, h, w, levels, cn, msg):
    """one interior pixel; no multiple of anything; every level count; a row of updated pixels that ends one past / exactly at a wave.
    ndisp = 16 exceeds the width of the small shapes: the x - disp < 1 branch."""
    args = (h, w, cn, 10 * h + cn, "random", 16, 3, levels, msg)
    eq(_run(gpu, *args), _ref_compute(*args))


# below, at and above each capacity of the register form (16, 32, 64), the smallest values, and the general form far beyond
@pytest.mark.parametrize("msg", ["f32", "s16"])
@pytest.mark.parametrize("ndisp", [1, 2, 7, 15, 16, 17, 31, 32, 33, 63, 64, 65])
def test_compute_ndisp(gpu, ndisp, msg):
    args = (21, 19, 1, ndisp, "random", ndisp, 2, 2, msg)
    eq(_run(gpu, *args), _ref_compute(*args))


@pytest.mark.parametrize("msg", ["f32", "s16"])
def test_compute_ndisp_200(gpu, msg):
    args = (30, 40, 3, 5, "random", 200, 2, 2, msg)
    eq(_run(gpu, *args), _ref_compute(*args))


@pytest.mark.parametrize("msg", ["f32", "s16"])
@pytest.mark.parametrize("iters", [1, 2, 5])
def test_compute_iters_on_a_stereo_pair(gpu, iters, msg):
    args = (48, 64, 1, 42, "synth", 16, iters, 3, msg)
    ref = _ref_compute(*args)
    assert len(np.unique(ref[1:-1, 1:-1])) > 3          # the case does find a disparity field
    eq(_run(gpu, *args), ref)


@pytest.mark.parametrize("msg", ["f32", "s16"])
def test_compute_weights_and_colour_pair(gpu, msg):
    w = (("data_weight", 0.11), ("disc_single_jump", 0.65), ("max_data_term", 14.5), ("max_disc_term", 2.3))
    args = (33, 47, 3, 7, "synth", 24, 3, 2, msg, w)
    eq(_run(gpu, *args), _ref_compute(*args))


@pytest.mark.parametrize("msg", ["f32", "s16"])
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_compute_pitched(gpu, cn, msg):
    args = (37, 29, cn, 370 + cn, "random", 16, 3, 3, msg)
    eq(_run(gpu, *args, pitched=True), _ref_compute(*args))


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int32, np.float32])
def test_compute_output_types(gpu, dtype):
    """convertTo's saturate_cast: 300 disparities clamp at 255 in CV_8U"""
    args = (12, 330, 1, 4, "random", 300, 1, 1, "f32")
    ref = _ref_compute(*args)
    assert ref.max() > 255
    want = np.clip(ref, 0, 255).astype(np.uint8) if dtype == np.uint8 else ref.astype(dtype)
    eq(_run(gpu, *args, out_dtype=dtype), want)


@pytest.mark.parametrize("msg", ["f32", "s16"])
@pytest.mark.parametrize("cn", [1, 3])
def test_constant_images_first_minimum(gpu, cn, msg):
    """every cost ties: the first strict minimum wins"""
    args = (13, 11, cn, 0, "const", 16, 2, 2, msg)
    ref = _ref_compute(*args)
    eq(_run(gpu, *args), ref)
    assert ref.max() <= 1     # ties resolve to the first of the tied disparities


# ------------------------------------------------------------------ compute(data)
def _volume(msg, nd, h, w, seed):
    rng = np.random.default_rng(seed)
    if msg == "f32":
        return rng.uniform(0, 20, (nd * h, w)).astype(np.float32)
    v = rng.integers(0, 300, (nd * h, w)).astype(np.int16)
    edge = rng.random((nd * h, w))
    v[edge < 0.08] = 32767 - rng.integers(0, 40)      # near the range limit: saturating stores, and the truncating subtraction wraps
    v[edge > 0.94] = -32768 + rng.integers(0, 40)
    return v


@pytest.mark.parametrize("msg", ["f32", "s16"])
@pytest.mark.parametrize("nd,levels", [(8, 2), (20, 1)])
def test_compute_data(gpu, msg, nd, levels):
    import torch
    from opencv_contrib_amd import cuda
    h, w = 17, 23
    vol = _volume(msg, nd, h, w, nd)
    ref = R.compute_data(vol, nd, 3, levels, MSG[msg])
    bp = _bp(cuda, nd, 3, levels, msg)
    out = bp.compute_data(_dev(vol, gpu))
    out_p = bp.compute_data(_dev(vol, gpu, pitched=True))
    torch.cuda.synchronize()
    eq(out.cpu().numpy(), ref)
    eq(out_p.cpu().numpy(), ref)


# ------------------------------------------------------------------ stage entries
def _stage_case(msg, cn, nd=8, h=9, w=11, seed=5):
    """inputs of every stage, the way tools/make_golden_stereobp.py chains them"""
    rng = np.random.default_rng(seed)
    left, right = _images(h, w, cn, seed)
    T = R.msg_dtype(MSG[msg])
    ch, cw = (h + 1) // 2, (w + 1) // 2
    lo, hi = (-3.0, 9.0) if msg == "f32" else (-40, 90)
    coarse = [rng.uniform(lo, hi, (nd, ch, cw)).astype(T) for _ in range(4)]
    return left, right, coarse


def _planar_dev(vols, gpu):
    return [_dev(R.planar(v), gpu) for v in vols]


@pytest.mark.parametrize("msg", ["f32", "s16"])
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_stage_comp_data_keeps_the_border(gpu, msg, cn):
    from opencv_contrib_amd import cuda
    nd, h, w = 8, 9, 11
    left, right, _ = _stage_case(msg, cn)
    T = R.msg_dtype(MSG[msg])
    sentinel = np.full((nd, h, w), 123, T)
    wts = dict(max_data_term=9.0, data_weight=0.09)
    ref = R.comp_data(left, right, R.consts(nd, MSG[msg], **wts), MSG[msg], sentinel.copy())
    out = cuda.stereobp_comp_data(_dev(left, gpu), _dev(right, gpu), nd, MSG[msg], data=_dev(R.planar(sentinel), gpu), **wts)
    out = R.unplanar(out.cpu().numpy(), nd)
    eq(out, ref)
    assert (out[:, 0] == 123).all() and (out[:, -1] == 123).all() and (out[:, :, 0] == 123).all() and (out[:, :, -1] == 123).all()
    assert (out[:, 1:-1, 1:-1] != 123).any()


@pytest.mark.parametrize("msg", ["f32", "s16"])
@pytest.mark.parametrize("h,w", [(9, 11), (8, 70), (5, 129)])
def test_stage_step_down_and_level_up(gpu, msg, h, w):
    from opencv_contrib_amd import cuda
    nd = 5
    rng = np.random.default_rng(h * w)
    T = R.msg_dtype(MSG[msg])
    src = (rng.uniform(0, 30, (nd, h, w)) if msg == "f32" else rng.integers(0, 20000, (nd, h, w))).astype(T)   # short sums saturate
    down = cuda.stereobp_data_step_down(_dev(R.planar(src), gpu), nd).cpu().numpy()
    ref = R.data_step_down(src)
    eq(R.unplanar(down, nd), ref)
    coarse = [np.roll(ref, k, 2) for k in range(4)]
    up = cuda.stereobp_level_up(_planar_dev(coarse, gpu), nd, h, w)
    for k in range(4):
        eq(R.unplanar(up[k].cpu().numpy(), nd), R.level_up(coarse[k], h, w))


FORMS = {"reg": 1, "gen": 2}


@pytest.mark.parametrize("msg", ["f32", "s16"])
@pytest.mark.parametrize("form", ["reg", "gen"])
@pytest.mark.parametrize("nd", [8, 16, 17, 32, 33, 64])
@pytest.mark.parametrize("t0,n_iters", [(0, 1), (1, 1), (0, 3), (1, 3)])
def test_stage_iterate_forms(gpu, msg, form, nd, t0, n_iters):
    """both kernel forms by name (every capacity of the register form), either starting parity, one and three half-sweeps"""
    from opencv_contrib_amd import cuda
    h, w = 7, 133
    rng = np.random.default_rng(nd + t0)
    T = R.msg_dtype(MSG[msg])
    lo, hi = (-3.0, 9.0) if msg == "f32" else (-40, 90)
    msgs = [rng.uniform(lo, hi, (nd, h, w)).astype(T) for _ in range(4)]
    data = rng.uniform(0, hi, (nd, h, w)).astype(T)
    wts = dict(max_disc_term=1.9, disc_single_jump=0.7)
    ref = [m.copy() for m in msgs]
    R.calc_all_iterations(*ref, data, n_iters, R.consts(nd, MSG[msg], **wts), t0=t0)
    out = cuda.stereobp_iterate(_planar_dev(msgs, gpu), _dev(R.planar(data), gpu), nd, t0, n_iters, FORMS[form], **wts)
    for k in range(4):
        eq(R.unplanar(out[k].cpu().numpy(), nd), ref[k])


@pytest.mark.parametrize("msg", ["f32", "s16"])
def test_stage_forms_agree(gpu, msg):
    """the register form and the general form on a shape both accept, chained through all stages"""
    from opencv_contrib_amd import cuda
    nd, h, w = 8, 9, 11
    left, right, coarse = _stage_case(msg, 3)
    data = cuda.stereobp_comp_data(_dev(left, gpu), _dev(right, gpu), nd, MSG[msg])
    up = cuda.stereobp_level_up(_planar_dev(coarse, gpu), nd, h, w)
    a = cuda.stereobp_iterate(up, data, nd, 0, 4, FORMS["reg"])
    b = cuda.stereobp_iterate(up, data, nd, 0, 4, FORMS["gen"])
    for k in range(4):
        eq(a[k].cpu().numpy(), b[k].cpu().numpy())
    c = R.consts(nd, MSG[msg])
    rdata = R.comp_data(left, right, c, MSG[msg])
    ref = [R.level_up(m, h, w) for m in coarse]
    R.calc_all_iterations(*ref, rdata, 4, c)
    eq(cuda.stereobp_output(a, data, nd).cpu().numpy(), R.output(*ref, rdata))


def test_stage_iterate_rejects_register_form_beyond_its_capacity(gpu):
    import torch
    from opencv_contrib_amd import cuda
    from opencv_contrib_amd.capi import MiError
    msgs = [torch.zeros((65 * 5, 6), dtype=torch.float32, device=gpu) for _ in range(5)]
    with pytest.raises(MiError, match="register form"):
        cuda.stereobp_iterate(msgs[:4], msgs[4], 65, 0, 1, FORMS["reg"])


@pytest.mark.parametrize("path", STAGE_FILES, ids=[os.path.basename(p)[:-4] for p in STAGE_FILES])
def test_stages_equal_reference_kernels(gpu, path):
    """every kernel wrapper of the reference on its own, from its recorded inputs to its recorded outputs; both forms"""
    from opencv_contrib_amd import cuda
    z = np.load(path)
    p = json.loads(str(z["params"]))
    nd, mt, w = p["ndisp"], MSG[p["msg"]], p["weights"]
    h, wd = z["left"].shape[:2]
    data = cuda.stereobp_comp_data(_dev(z["left"], gpu), _dev(z["right"], gpu), nd, mt, **w)
    eq(data.cpu().numpy(), z["data"])
    eq(cuda.stereobp_data_step_down(_dev(z["data"], gpu), nd).cpu().numpy(), z["data_down"])
    up = cuda.stereobp_level_up([_dev(m, gpu) for m in z["coarse"]], nd, h, wd)
    for k in range(4):
        eq(up[k].cpu().numpy(), z["up"][k])
    for form in FORMS.values():
        for n, key in ((1, "iter1"), (2, "iter2")):
            out = cuda.stereobp_iterate([_dev(m, gpu) for m in z["up"]], _dev(z["data"], gpu), nd, 0, n, form, **w)
            for k in range(4):
                eq(out[k].cpu().numpy(), z[key][k])
    eq(cuda.stereobp_output([_dev(m, gpu) for m in z["iter2"]], _dev(z["data"], gpu), nd).cpu().numpy(), z["disp"])


# ------------------------------------------------------------------ handles
def test_two_handles_on_two_streams(gpu):
    """parameters travel as kernel arguments: two handles with different weights, interleaved on two streams, give their own results"""
    import torch
    from opencv_contrib_amd import cuda
    wa = ()
    wb = (("data_weight", 0.2), ("disc_single_jump", 0.5), ("max_data_term", 20.0), ("max_disc_term", 3.1))
    args = (37, 29, 1, 371, "random", 16, 3, 3)
    left, right = _images(*args[:5])
    a, b = _bp(cuda, 16, 3, 3, "f32", wa), _bp(cuda, 16, 3, 3, "s16", wb)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    L, Rt = _dev(left, gpu), _dev(right, gpu)
    torch.cuda.synchronize()
    outs = []
    for _ in range(3):
        outs.append((a.compute(L, Rt, stream=sa), b.compute(L, Rt, stream=sb)))
    torch.cuda.synchronize()
    for oa, ob in outs:
        eq(oa.cpu().numpy(), _ref_compute(*args, "f32", wa))
        eq(ob.cpu().numpy(), _ref_compute(*args, "s16", wb))


def test_handle_reuse_across_sizes_and_params(gpu):
    import torch
    from opencv_contrib_amd import cuda
    bp = cuda.createStereoBeliefPropagation(16, 3, 3, R.CV_32F)
    seq = [((37, 29, 1, 371, "random", 16, 3, 3, "f32"), None), ((13, 11, 3, 133, "random", 16, 3, 2, "s16"), None),
           ((67, 41, 4, 674, "random", 16, 3, 4, "f32"), None), ((37, 29, 1, 371, "random", 16, 3, 3, "f32"), None)]
    for args, _ in seq:
        h, w, cn, seed, kind, nd, iters, levels, msg = args
        bp.setNumDisparities(nd); bp.setNumIters(iters); bp.setNumLevels(levels); bp.setMsgType(MSG[msg])
        left, right = _images(h, w, cn, seed, kind)
        out = bp.compute(_dev(left, gpu), _dev(right, gpu))
        torch.cuda.synchronize()
        eq(out.cpu().numpy(), _ref_compute(*args))
    assert (bp.getNumDisparities(), bp.getNumIters(), bp.getNumLevels(), bp.getMsgType()) == (16, 3, 3, R.CV_32F)
    assert (bp.getMinDisparity(), bp.getBlockSize(), bp.getSpeckleWindowSize(), bp.getSpeckleRange(), bp.getDisp12MaxDiff()) == (0,) * 5


def test_pipeline_with_disparity_bilateral_filter(gpu, oracle):
    """the pipeline the filter exists for: belief propagation refined by the joint bilateral filter = restatement refined by the oracle"""
    import torch
    from opencv_contrib_amd import cuda
    args = (48, 64, 1, 42, "synth", 16, 5, 3, "s16")
    left, right = _images(*args[:5])
    L = _dev(left, gpu)
    disp = _bp(cuda, 16, 5, 3, "s16").compute(L, _dev(right, gpu))
    out = cuda.createDisparityBilateralFilter(16, 3, 2).apply(disp, L)
    torch.cuda.synchronize()
    ref_disp = _ref_compute(*args)
    ref = oracle.dbf_apply(np.array(ref_disp), left, oracle.dbf_params(ndisp=16, radius=3, iters=2))
    eq(disp.cpu().numpy(), ref_disp)
    eq(out.cpu().numpy(), ref)


# ------------------------------------------------------------------ argument checks
def test_argument_checks(gpu):
    """the reference's asserts as error codes with the asserted condition as text; nothing is allocated on the way"""
    import torch
    from opencv_contrib_amd import cuda
    from opencv_contrib_amd.capi import MiError
    img = torch.zeros((24, 32), dtype=torch.uint8, device=gpu)

    def fails(code, text, fn):
        with pytest.raises(MiError) as e:
            fn()
        assert e.value.code == code and text in str(e.value), str(e.value)

    for kw in (dict(ndisp=0), dict(iters=0), dict(levels=0)):
        a = dict(dict(ndisp=16, iters=2, levels=2), **kw)
        fails(-1, "0 < ndisp_ && 0 < iters_ && 0 < levels_", lambda: cuda.createStereoBeliefPropagation(a["ndisp"], a["iters"], a["levels"]).compute(img, img))
    fails(-1, "msg_type_ == CV_32F || msg_type_ == CV_16S", lambda: cuda.createStereoBeliefPropagation(16, 2, 2, 0).compute(img, img))
    bp = cuda.createStereoBeliefPropagation(16, 2, 3, R.CV_16S)
    bp.setMaxDataTerm(819.2)     # 4 * 10 * 819.2 = 32768 >= 32767
    fails(-1, "std::numeric_limits<short>::max()", lambda: bp.compute(img, img))
    bp.setMaxDataTerm(819.0)     # 32760 < 32767
    bp.compute(img, img)
    ok = cuda.createStereoBeliefPropagation(16, 2, 4)                  # 24 >> 3 = 3 > 2 holds; with 5 levels it is 1
    ok.compute(img, img)
    fails(-3, "min_image_dim_size", lambda: cuda.createStereoBeliefPropagation(16, 2, 5).compute(img, img))
    fails(-3, "left.size() == right.size()", lambda: ok.compute(img, img[:, :31]))
    fails(-3, "left.size() == right.size()", lambda: ok.compute(img, torch.zeros((24, 32, 3), dtype=torch.uint8, device=gpu)))
    fails(-2, "left.type() == CV_8UC1", lambda: ok.compute(img.to(torch.float32), img.to(torch.float32)))
    fails(-1, "data.rows % ndisp_ == 0", lambda: ok.compute_data(torch.zeros((16 * 24 + 1, 32), dtype=torch.float32, device=gpu)))
    fails(-1, "data.type() == msg_type_", lambda: ok.compute_data(torch.zeros((16 * 24, 32), dtype=torch.int16, device=gpu)))
    fails(-2, "disparity", lambda: ok.compute(img, img, torch.zeros((24, 32, 2), dtype=torch.float32, device=gpu)))
    fails(-3, "disparity", lambda: ok.compute(img, img, torch.zeros((24, 31), dtype=torch.int16, device=gpu)))


def test_argument_checks_allocate_nothing(gpu):
    """a rejected call leaves the handle's scratch as it was: empty on a fresh handle, unchanged on a used one"""
    import torch
    from opencv_contrib_amd import cuda
    from opencv_contrib_amd.capi import MiError
    img = torch.zeros((24, 32), dtype=torch.uint8, device=gpu)
    bad = [cuda.createStereoBeliefPropagation(0, 2, 2), cuda.createStereoBeliefPropagation(16, 2, 9), cuda.createStereoBeliefPropagation(16, 2, 2, 1),
           cuda.createStereoBeliefPropagation(16, 2, 2)]
    for bp in bad[:3]:
        with pytest.raises(MiError):
            bp.compute(img, img)
    with pytest.raises(MiError):
        bad[3].compute(img, img[:, :30])
    with pytest.raises(MiError):
        bad[3].compute(img, img, torch.zeros((24, 31), dtype=torch.int16, device=gpu))
    assert [bp.scratchBytes() for bp in bad] == [0, 0, 0, 0]
    bad[3].compute(img, img)
    used = bad[3].scratchBytes()
    assert used > 0
    bad[3].setNumLevels(9)
    with pytest.raises(MiError):
        bad[3].compute(img, img)
    assert bad[3].scratchBytes() == used
