"""cv::cuda::CornernessCriteria and cv::cuda::CornersDetector on the GPU: every stage and the classes equal the NumPy restatement
(tests/gftt_numpy_ref.py) in every bit and in order.  Shapes at the plan's tile edges and the block sizes at which the launch form
changes come from the plan's constants (opencv_contrib_amd/csrc/gftt_plan.h)."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gftt_numpy_ref as R  # noqa: E402
from test_gftt_plan import fused_lds, plan_constants  # noqa: E402

pytestmark = pytest.mark.gpu
K = plan_constants()
TW, TH, SORT_TILE, LDS_LIMIT = K["GFTT_TILE_W"], K["GFTT_TILE_H"], K["GFTT_SORT_TILE"], K["GFTT_LDS_LIMIT"]
FUSED, PLANES = K["GFTT_FORM_FUSED"], K["GFTT_FORM_PLANES"]
MAX_FUSED_BS = max(b for b in range(1, 200) if fused_lds(b) <= LDS_LIMIT)
SIZES = [(3, 3), (5, 7), (23, 71), (40, 140)]
NAMES = {R.BORDER_REFLECT101: "reflect101", R.BORDER_REFLECT: "reflect", R.BORDER_REPLICATE: "replicate"}


def cuda():
    from opencv_contrib_amd import cuda as c
    return c


def dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def eq_bits(got, want):
    """equal in every bit: -0 is not +0 and a NaN is only itself"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(bits(got), bits(want))


def type_of(img):
    from opencv_contrib_amd import capi
    return capi.MI_8UC1 if img.dtype == np.uint8 else capi.MI_32FC1


@functools.lru_cache(maxsize=None)
def image(rows, cols, kind, dt):
    return R.synth_image(rows, cols, rows * 1000 + cols, kind, np.uint8 if dt == "u8" else np.float32)


@functools.lru_cache(maxsize=None)
def want_response(rows, cols, kind, dt, bs, border, harris):
    return R.response(image(rows, cols, kind, dt), bs, border, harris, 0.04)


# ------------------------------------------------------------------ response planes
@pytest.mark.parametrize("bs", [1, 2, 3, 4, 5, 7])
@pytest.mark.parametrize("border", R.BORDERS, ids=[NAMES[b] for b in R.BORDERS])
@pytest.mark.parametrize("dt", ["u8", "f32"])
@pytest.mark.parametrize("harris", [False, True], ids=["mineig", "harris"])
def test_criteria_classes_equal_restatement(gpu, harris, dt, border, bs):
    c = cuda()
    for rows, cols in SIZES:
        img = image(rows, cols, "noise", dt)
        crit = c.createHarrisCorner(type_of(img), bs, 3, 0.04, border) if harris else c.createMinEigenValCorner(type_of(img), bs, 3, border)
        eq_bits(crit.compute(dev(img, gpu)).cpu().numpy(), want_response(rows, cols, "noise", dt, bs, border, harris))


EDGES = [(h, w) for h in (TH - 1, TH, TH + 1) for w in (TW - 1, TW, TW + 1)] + [(2 * TH + 1, 2 * TW + 1)]


@pytest.mark.parametrize("form", [FUSED, PLANES], ids=["fused", "planes"])
@pytest.mark.parametrize("dt", ["u8", "f32"])
def test_each_launch_form_at_the_tile_edges(gpu, dt, form):
    for rows, cols in EDGES:
        img = image(rows, cols, "noise", dt)
        for bs, border, harris in ((3, R.BORDER_REFLECT101, False), (6, R.BORDER_REFLECT, True), (5, R.BORDER_REPLICATE, False)):
            d, s = R.taps(img.dtype, bs)
            got = cuda().gftt_response(dev(img, gpu), d, s, bs, border, harris, 0.04, form).cpu().numpy()
            eq_bits(got, want_response(rows, cols, "noise", dt, bs, border, harris))


@pytest.mark.parametrize("border", R.BORDERS, ids=[NAMES[b] for b in R.BORDERS])
def test_launch_forms_equal_each_other_up_to_the_largest_fused_window(gpu, border):
    """the largest blockSize whose tile fits the LDS, on images of one and of two tile rows that are smaller than the window, where the
    border map wraps; and the restatement"""
    for bs in (MAX_FUSED_BS, MAX_FUSED_BS - 1, 16):
        for rows, cols in ((TH + 1, TW + 6), (TH + 4, 9), (7, TW + 1)):
            img = image(rows, cols, "noise", "u8")
            d, s = R.taps(img.dtype, bs)
            a = cuda().gftt_response(dev(img, gpu), d, s, bs, border, False, 0.0, FUSED).cpu().numpy()
            b = cuda().gftt_response(dev(img, gpu), d, s, bs, border, False, 0.0, PLANES).cpu().numpy()
            eq_bits(a, b)
            eq_bits(a, want_response(rows, cols, "noise", "u8", bs, border, False))


def test_window_above_the_fused_limit_takes_the_planes_form(gpu):
    from opencv_contrib_amd import capi
    bs = MAX_FUSED_BS + 1
    img = image(TH + 3, TW + 2, "noise", "f32")
    d, s = R.taps(img.dtype, bs)
    with pytest.raises(capi.MiError):
        cuda().gftt_response(dev(img, gpu), d, s, bs, R.BORDER_REFLECT101, False, 0.0, FUSED)
    want = want_response(TH + 3, TW + 2, "noise", "f32", bs, R.BORDER_REFLECT101, False)
    eq_bits(cuda().gftt_response(dev(img, gpu), d, s, bs, R.BORDER_REFLECT101, False, 0.0, 0).cpu().numpy(), want)
    eq_bits(cuda().createMinEigenValCorner(type_of(img), bs, 3).compute(dev(img, gpu)).cpu().numpy(), want)


@pytest.mark.parametrize("form", [FUSED, PLANES], ids=["fused", "planes"])
@pytest.mark.parametrize("dt", ["u8", "f32"])
def test_pitched_views_inside_a_sentinel_frame(gpu, dt, form):
    """source and destination are ROIs of larger allocations at odd offsets: the frame of the destination stays as it was, and the frame
    of a float source is NaN, which any read would carry into the result"""
    import torch
    rows, cols, bs = TH + 3, TW + 5, 5
    img = image(rows, cols, "noise", dt)
    big = torch.full((rows + 7, cols + 13), 255 if dt == "u8" else float("nan"), dtype=torch.uint8 if dt == "u8" else torch.float32, device=gpu)
    big[3:3 + rows, 5:5 + cols] = dev(img, gpu)
    out = torch.full((rows + 4, cols + 9), -7.5, dtype=torch.float32, device=gpu)
    d, s = R.taps(img.dtype, bs)
    cuda().gftt_response(big[3:3 + rows, 5:5 + cols], d, s, bs, R.BORDER_REFLECT, False, 0.0, form, dst=out[2:2 + rows, 3:3 + cols])
    o = out.cpu().numpy()
    eq_bits(o[2:2 + rows, 3:3 + cols], want_response(rows, cols, "noise", dt, bs, R.BORDER_REFLECT, False))
    o[2:2 + rows, 3:3 + cols] = -7.5
    assert (o == -7.5).all()


@pytest.mark.parametrize("q", [1e-6, 0.01, 0.5, 1.0])
def test_device_threshold(gpu, q):
    for rows, cols, harris in ((23, 71, False), (2 * TH + 1, 2 * TW + 1, True)):
        img = image(rows, cols, "noise", "u8")
        d, s = R.taps(img.dtype, 3)
        plane, thr = cuda().gftt_response(dev(img, gpu), d, s, 3, R.BORDER_REFLECT101, harris, 0.04, 0, qualityLevel=q)
        want = want_response(rows, cols, "noise", "u8", 3, R.BORDER_REFLECT101, harris)
        eq_bits(plane.cpu().numpy(), want)
        eq_bits(np.float32(thr), R.threshold(want, q))


# ------------------------------------------------------------------ findCorners
def find(gpu, resp, thr, mask=None, max_count=4000):
    return cuda().gftt_find_corners(dev(resp, gpu), thr, dev(mask, gpu) if mask is not None else None, max_count).cpu().numpy().reshape(-1, 2)


def test_find_corners_masks(gpu):
    rows, cols = 2 * TH + 1, 2 * TW + 3
    resp = want_response(rows, cols, "noise", "u8", 3, R.BORDER_REFLECT101, False)
    thr = R.threshold(resp, 0.01)
    plain, found = R.find_corners(resp, thr)
    assert found > 100
    eq_bits(find(gpu, resp, thr), plain)
    irregular = R.synth_mask(rows, cols, 5)
    want, n = R.find_corners(resp, thr, irregular)
    assert 0 < n < found
    eq_bits(find(gpu, resp, thr, irregular), want)
    assert find(gpu, resp, thr, np.zeros((rows, cols), np.uint8)).shape == (0, 2)
    x, y = plain[len(plain) // 2].astype(int)
    one = np.zeros((rows, cols), np.uint8)
    one[y, x] = 1
    eq_bits(find(gpu, resp, thr, one), np.array([[x, y]], np.float32))


def test_find_corners_plateau_and_borders(gpu):
    """equal 3 x 3 neighbours all emit (val == maxVal); the outermost rows and columns never do, whatever they hold"""
    resp = np.zeros((TH + 2, TW + 9), np.float32)
    resp[4:9, 60:70] = 1.0      # a plateau across a segment edge
    resp[0, :] = 9.0
    resp[:, -1] = 9.0
    resp[12, 3] = 0.5
    want, found = R.find_corners(resp, 0.25)
    assert found == 5 * 10 + 1
    eq_bits(find(gpu, resp, 0.25), want)
    for rows, cols in ((1, 5), (2, 2), (3, 2), (2, 3)):   # no interior pixel
        assert find(gpu, np.ones((rows, cols), np.float32), 0.0).shape == (0, 2)


def test_find_corners_capacity_cut_is_row_major(gpu):
    resp = R.response(image(128, 128, "noise", "u8"), 3)
    thr = R.threshold(resp, 1e-6)
    every, found = R.find_corners(resp, thr)
    assert found > 1000
    eq_bits(find(gpu, resp, thr, None, 1000), every[:1000])
    eq_bits(find(gpu, resp, thr, None, found), every)
    eq_bits(find(gpu, resp, thr, None, found + 1), every)


# ------------------------------------------------------------------ sort
def sort_case(n, seed, quantum=None):
    rows, cols = 100, 173
    rng = np.random.default_rng(seed)
    resp = rng.standard_normal((rows, cols)).astype(np.float32)
    if quantum:
        resp = (np.round(resp / quantum) * quantum).astype(np.float32)
        resp[resp == 0] = np.where(rng.random(int((resp == 0).sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
    at = rng.permutation(rows * cols)[:n]
    pts = np.stack([at % cols, at // cols], 1).astype(np.float32)
    return resp, pts


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 1024, 1025, SORT_TILE, SORT_TILE + 1, 2 * SORT_TILE + 5, 4 * SORT_TILE - 1])
def test_sort_counts(gpu, n):
    """one count above a single workgroup's LDS tile and counts that need one and two levels of global steps"""
    resp, pts = sort_case(n, n)
    eq_bits(cuda().gftt_sort(dev(resp, gpu), dev(pts[None], gpu)).cpu().numpy()[0], R.sort_corners(resp, pts))


@pytest.mark.parametrize("n", [65, 3000, SORT_TILE + 77])
def test_sort_ties_negative_values_and_signed_zeros(gpu, n):
    resp, pts = sort_case(n, 1000 + n, quantum=0.5)
    r = resp[pts[:, 1].astype(int), pts[:, 0].astype(int)]
    assert len(np.unique(r)) < n / 4 and (r < 0).any() and (np.signbit(r) & (r == 0)).any() and (~np.signbit(r) & (r == 0)).any()
    want = R.sort_corners(resp, pts)
    eq_bits(cuda().gftt_sort(dev(resp, gpu), dev(pts[None], gpu)).cpu().numpy()[0], want)
    w = resp[want[:, 1].astype(int), want[:, 0].astype(int)]
    idx = want[:, 1] * resp.shape[1] + want[:, 0]
    assert ((w[:-1] > w[1:]) | ((w[:-1] == w[1:]) & (idx[:-1] < idx[1:]))).all()


# ------------------------------------------------------------------ class
CASES = {   # name: (image kind, rows, cols, dtype, masked, kwargs)
    "flat": ("flat", 23, 71, "u8", False, {}),
    "blocks_ties": ("blocks", 40, 140, "u8", False, dict(max_corners=0)),
    "noise23x71_u8": ("noise", 23, 71, "u8", False, {}),
    "noise23x71_f32": ("noise", 23, 71, "f32", False, {}),
    "noise40x140_u8": ("noise", 40, 140, "u8", False, {}),
    "noise40x140_f32": ("noise", 40, 140, "f32", False, {}),
    "masked": ("noise", 40, 140, "u8", True, {}),
    "harris": ("noise", 40, 140, "u8", False, dict(harris=True)),
    "harris_f32_bs5": ("noise", 40, 140, "f32", False, dict(harris=True, block_size=5, k=0.06)),
    "bs2": ("noise", 40, 140, "u8", False, dict(block_size=2)),
    "bs5": ("noise", 40, 140, "u8", False, dict(block_size=5)),
    "bs7": ("noise", 23, 71, "u8", False, dict(block_size=7)),
    "bs7_above_the_side": ("noise", 5, 140, "u8", False, dict(block_size=7)),
    "md3": ("noise", 40, 140, "u8", False, dict(min_dist=3.0)),
    "md7.5": ("noise", 40, 140, "u8", False, dict(min_dist=7.5)),
    "md3_max10": ("noise", 40, 140, "u8", False, dict(min_dist=3.0, max_corners=10)),
    "md7.5_all": ("noise", 40, 140, "f32", False, dict(min_dist=7.5, max_corners=0)),
    "max10": ("noise", 40, 140, "u8", False, dict(max_corners=10)),
    "all": ("noise", 40, 140, "u8", False, dict(max_corners=0)),
    "blocks_md3": ("blocks", 40, 140, "u8", True, dict(min_dist=3.0, max_corners=0)),
    "smallest": ("noise", 3, 3, "u8", False, dict(quality_level=1e-6)),
}


def detector(img, max_corners=1000, quality_level=0.01, min_dist=0.0, block_size=3, harris=False, k=0.04):
    return cuda().createGoodFeaturesToTrackDetector(type_of(img), max_corners, quality_level, min_dist, block_size, harris, k)


def check_detect(gpu, img, mask=None, det=None, **kw):
    import torch
    det = det or detector(img, **kw)
    got = det.detect(dev(img, gpu), dev(mask, gpu) if mask is not None else None)
    assert got.dtype == torch.float32 and got.dim() == 3 and got.shape[0] == 1 and got.shape[2] == 2 and got.is_contiguous()
    want = R.detect(img, mask, **kw)
    eq_bits(got.cpu().numpy()[0], want)
    return want


@pytest.mark.parametrize("name", sorted(CASES))
def test_class_equals_restatement(gpu, name):
    kind, rows, cols, dt, masked, kw = CASES[name]
    img = image(rows, cols, kind, dt)
    want = check_detect(gpu, img, R.synth_mask(rows, cols, 3) if masked else None, **kw)
    assert len(want) == 0 if name == "flat" else len(want) > 0 or name == "smallest"


def test_class_capacity_cut_and_a_sort_beyond_one_tile(gpu):
    """312 x 320: capacity 4992 needs two sort tiles; quality 1e-6 finds more local maxima than that"""
    img = image(312, 320, "noise", "u8")
    st = {}
    R.detect(img, None, 0, 1e-6, 0.0, stages=st)
    assert st["found"] > R.capacity(312, 320) > SORT_TILE
    assert len(check_detect(gpu, img, max_corners=0, quality_level=1e-6)) == R.capacity(312, 320)
    check_detect(gpu, img, max_corners=5000, quality_level=0.05, min_dist=4.0)


def test_one_handle_setters_empty_results_and_changing_sizes(gpu):
    a, b, flat = image(40, 140, "noise", "u8"), image(2 * TH + 1, 2 * TW + 1, "noise", "u8"), image(23, 71, "flat", "u8")
    det = detector(a)
    check_detect(gpu, a, det=det)
    det.setMaxCorners(10)
    assert len(check_detect(gpu, a, det=det, max_corners=10)) == 10
    det.setMinDistance(7.5)
    check_detect(gpu, a, det=det, max_corners=10, min_dist=7.5)
    det.setMaxCorners(0)
    check_detect(gpu, b, det=det, max_corners=0, min_dist=7.5)
    assert det.detect(dev(flat, gpu)).shape == (1, 0, 2)        # empty ...
    check_detect(gpu, a, det=det, max_corners=0, min_dist=7.5)   # ... then not, on the same handle
    det.setMinDistance(0.0)
    assert det.detect(dev(flat, gpu)).shape == (1, 0, 2)
    check_detect(gpu, b, det=det, max_corners=0)
    assert det.scratchBytes() > 0


def test_non_default_stream(gpu):
    import torch
    img = image(40, 140, "noise", "u8")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = dev(img, gpu)
        for kw in (dict(), dict(min_dist=3.0)):
            eq_bits(detector(img, **kw).detect(t).cpu().numpy()[0], R.detect(img, **kw))
    s.synchronize()


def test_rejections_with_a_device(gpu):
    from opencv_contrib_amd import capi
    det = detector(image(23, 71, "noise", "u8"))
    with pytest.raises(capi.MiError):
        det.detect(dev(image(23, 71, "noise", "f32"), gpu))               # src.type() == srcType
    with pytest.raises(capi.MiError):
        det.detect(dev(image(23, 71, "noise", "u8"), gpu), dev(np.ones((23, 70), np.uint8), gpu))   # mask.size() == image.size()
    for bad in (dict(setMaxCorners=-1), dict(setMinDistance=-0.5)):
        for name, v in bad.items():
            with pytest.raises(capi.MiError):
                getattr(det, name)(v)


def test_corners_feed_the_sparse_tracker_unchanged(gpu):
    """GFTT -> SparsePyrLK as videostab/src/global_motion.cpp:796-806 chains them: detect's tensor goes in as prevPts as it is, and the
    tracker gives what it gives for the same points uploaded from NumPy"""
    from opencv_contrib_amd import synth
    A0, A1, _ = synth.flow_pair(120, 160, seed=5, dtype="u8")
    t0, t1 = dev(A0, gpu), dev(A1, gpu)
    pts = detector(A0, 200, 0.01, 5.0).detect(t0)
    want = R.detect(A0, None, 200, 0.01, 5.0)
    assert pts.shape[1] == len(want) >= 32
    lk = cuda().SparsePyrLKOpticalFlow.create()
    n1, s1, e1 = lk.calc(t0, t1, pts)
    n2, s2, e2 = lk.calc(t0, t1, dev(want[None], gpu))
    eq_bits(n1.cpu().numpy(), n2.cpu().numpy())
    np.testing.assert_array_equal(s1.cpu().numpy(), s2.cpu().numpy())
    found = s1.cpu().numpy() != 0   # where the flow was not found the error is not defined (cudaoptflow.hpp:100-101)
    eq_bits(e1.cpu().numpy()[found], e2.cpu().numpy()[found])
    assert found.mean() > 0.5


@pytest.mark.parametrize("dt,masked,harris", [("u8", 0, 0), ("f32", 1, 1)], ids=["u8", "f32_masked_harris"])
def test_cpp_shim_equals_restatement(gpu, tmp_path, dt, masked, harris):
    """tests/cpp/gftt_shim.cpp: the reference's classes from C++ on a stream of their own, the setters between two calls on one object"""
    import struct
    import subprocess
    from test_gftt_ref import build_shim
    exe = build_shim(tmp_path)
    rows, cols, bs, q, k = 37, 131, 3 + 2 * harris, 0.02, 0.05
    img, mask = image(rows, cols, "noise", dt), R.synth_mask(rows, cols, 8)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("=7i3d", rows, cols, dt == "f32", masked, 300, bs, harris, q, 0.0, k) + img.tobytes() + (mask.tobytes() if masked else b""))
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = fout.read_bytes()
    at = 0
    for kw in (dict(max_corners=300, min_dist=0.0), dict(max_corners=5, min_dist=4.0)):
        n = struct.unpack_from("i", raw, at)[0]
        got = np.frombuffer(raw, np.float32, 2 * n, at + 4).reshape(n, 2)
        at += 4 + 8 * n
        want = R.detect(img, mask if masked else None, quality_level=q, block_size=bs, harris=bool(harris), k=k, **kw)
        assert n == len(want) > 0
        eq_bits(got, want)
    eq_bits(np.frombuffer(raw, np.float32, rows * cols, at).reshape(rows, cols), R.response(img, bs, R.BORDER_REFLECT101, bool(harris), k))
    assert at + 4 * rows * cols == len(raw)


# ------------------------------------------------------------------ what the reference's own code recorded (tests/golden/gftt_ref*.npz)
import test_gftt_ref as T  # noqa: E402


@pytest.mark.parametrize("path", T.CLASS_FILES, ids=T._ids(T.CLASS_FILES))
def test_class_equals_reference_fixture(gpu, path):
    """every class fixture end to end: the detector's output, and the stage entries on the fixture's own planes"""
    z = np.load(path)
    img, mask, kw = T.class_inputs(z)
    got = detector(img, **kw).detect(dev(img, gpu), dev(mask, gpu) if mask is not None else None).cpu().numpy()[0]
    T.check_class_fixture(z, os.path.basename(path)[:-4], got)
    crit = (cuda().createHarrisCorner(type_of(img), kw["block_size"], 3, kw["k"]) if kw["harris"] else
            cuda().createMinEigenValCorner(type_of(img), kw["block_size"], 3))
    eq_bits(crit.compute(dev(img, gpu)).cpu().numpy(), z["response"])
    cand = find(gpu, z["response"], float(z["threshold"]), mask, int(z["capacity"]))
    eq_bits(cand, z["candidates"])
    if len(cand) and not path.endswith("blocks_ties.npz"):
        eq_bits(cuda().gftt_sort(dev(z["response"], gpu), dev(cand[None], gpu)).cpu().numpy()[0], z["sorted"])


@pytest.mark.parametrize("path", T.STAGE_FILES, ids=T._ids(T.STAGE_FILES))
def test_response_equals_reference_stage_fixture(gpu, path):
    z = np.load(path)
    border = int(z["border"])
    for tag in T.STAGE_SIZES:
        img = z[f"img_{tag}"]
        for bs in T.STAGE_BS:
            for form in (FUSED, PLANES):
                for harris, name in ((False, "mineig"), (True, "harris")):
                    got = cuda().gftt_response(dev(img, gpu), z[f"deriv_bs{bs}"], z[f"smooth_bs{bs}"], bs, border, harris, float(z["harris_k"]), form)
                    eq_bits(got.cpu().numpy(), z[f"{name}_{tag}_bs{bs}"])
