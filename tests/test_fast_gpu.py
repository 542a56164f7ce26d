"""cv::cuda::FastFeatureDetector on the GPU: equality everywhere, against what the reference's own kernels and class recorded
(tests/golden/fast_ref*.npz) and against the NumPy restatement (tests/fast_numpy_ref.py), in row-major order.  Shapes at the plan's tile
and segment edges come from the plan's constants."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fast_numpy_ref as R  # noqa: E402
import test_fast_ref as T  # noqa: E402
from test_fast_plan import plan_constants  # noqa: E402

pytestmark = pytest.mark.gpu
eq = np.testing.assert_array_equal
K = plan_constants()
TW, TH, SEG, SCAN = K["FAST_TILE_W"], K["FAST_TILE_H"], K["FAST_SEG"], K["FAST_SCAN_THREADS"]


def cuda():
    from opencv_contrib_amd import cuda as c
    return c


def dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def got(kp):
    """a (2, n) device matrix -> (loc (n, 2) int16, resp (n,) float32)"""
    k = kp.cpu().numpy()
    assert k.shape[0] == 2 and k.dtype == np.float32
    return R.unpack(k) if k.shape[1] else (np.zeros((0, 2), np.int16), np.zeros(0, np.float32))


def check(gpu, img, th=10, nms=True, maxn=5000, mask=None, timg=None, tmask=None, det=None):
    """detectAsync of the image (or of the given device tensors that hold it) equals the restatement, bit for bit and in order"""
    det = det or cuda().FastFeatureDetector.create(th, nms, max_npoints=maxn)
    loc, resp = got(det.detectAsync(dev(img, gpu) if timg is None else timg, (dev(mask, gpu) if mask is not None else None) if tmask is None else tmask))
    wl, wr, count = R.detect(img, th, nms, maxn, mask)
    eq(loc, wl)
    eq(resp, wr)
    return loc, resp, count


# ------------------------------------------------------------------ class cases and stage entries
@pytest.mark.parametrize("path", T.CLASS_FILES, ids=T._ids(T.CLASS_FILES))
def test_class_equals_reference_class_and_restatement(gpu, path):
    z = np.load(path)
    img, mask, th, maxn = T.case_inputs(z)
    loc, resp, count = check(gpu, img, th, bool(int(z["nonmax_suppression"])), maxn, mask)
    assert count == int(z["count"])
    T.check_against_class_fixture(z, T.stage_of(path), loc, resp)
    kp = cuda().FastFeatureDetector.create(th, bool(int(z["nonmax_suppression"])), max_npoints=maxn)
    conv = np.array(kp.detect(dev(img, gpu), dev(mask, gpu) if mask is not None else None), np.float32).reshape(-1, 5)
    eq(conv[:, :2], loc.astype(np.float32))
    eq(conv[:, 4], resp)
    if int(z["count"]) <= maxn:
        o = np.lexsort((z["converted"][:, 0], z["converted"][:, 1]))
        eq(conv, z["converted"][o])


@pytest.mark.parametrize("path", T.STAGE_FILES, ids=T._ids(T.STAGE_FILES))
def test_score_stage_equals_reference_plane(gpu, path):
    z = np.load(path)
    img, mask, th, _ = T.case_inputs(z)
    s = cuda().fast_score(dev(img, gpu), dev(mask, gpu) if mask is not None else None, th).cpu().numpy()
    assert s.dtype == np.int32
    eq(s, z["score"])


# ------------------------------------------------------------------ shapes
EDGE_W = sorted({TW - 1, TW, TW + 1, TW + 3, TW + 4, 2 * TW - 1, 2 * TW, 2 * TW + 1})
EDGE_H = sorted({TH - 1, TH, TH + 1, TH + 3, TH + 4, 2 * TH - 1, 2 * TH, 2 * TH + 1})
SHAPES = [(7, 7), (7, 40), (40, 7), (8, 8)] + [(TH + 5, w) for w in EDGE_W] + [(h, TW + 9) for h in EDGE_H] + \
         [(TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 1, 2 * TW + 1)]


@pytest.mark.parametrize("rows,cols", SHAPES, ids=[f"{r}x{c}" for r, c in SHAPES])
def test_shape_sweep(gpu, rows, cols):
    img = R.synth_image(rows, cols, rows * 1000 + cols, "noise")
    if rows == 7 or cols == 7:   # one tested row or column: plant corners so that it is not empty by chance
        img[3, 3] = 255 if img[3, 3] < 128 else 0
    loc, _, count = check(gpu, img, 10, True)
    check(gpu, img, 10, False)
    eq(cuda().fast_score(dev(img, gpu), None, 10).cpu().numpy(), R.score_plane(img, 10)[1])
    if rows > 12 and cols > 12:
        assert count > 0 and 0 < len(loc) < count


def test_segment_counts_at_the_scan_and_block_edges(gpu):
    """one column of segments: rows = segments; one below, at and above the scan's thread count (a thread's run of segments goes from
    1 to 2) with candidates in the last rows"""
    for rows in (SCAN - 1, SCAN, SCAN + 1, 2 * SCAN + 3):
        img = R.synth_image(rows, 20, rows, "flat")
        img[-9:] = R.synth_image(9, 20, rows, "noise")
        img[:9] = R.synth_image(9, 20, rows + 1, "noise")
        loc, _, count = check(gpu, img, 10, True)
        assert count > 0 and loc[:, 1].max() >= rows - 6 and loc[:, 1].min() <= 5


@pytest.mark.parametrize("rows,cols", [(6, 100), (100, 6), (6, 6), (0, 0), (3, 0), (0, 9)])
def test_below_a_ring_gives_zero_keypoints_and_no_error(gpu, rows, cols):
    import torch
    det = cuda().FastFeatureDetector.create()
    img = torch.zeros((rows, cols), dtype=torch.uint8, device=gpu)
    kp = det.detectAsync(img)
    assert tuple(kp.shape) == (2, 0) and det.detect(img) == [] and det.scratchBytes() == 0   # nothing was launched or allocated
    s = cuda().fast_score(img, None, 10)
    assert tuple(s.shape) == (rows, cols) and not s.any()


# ------------------------------------------------------------------ addressing
def test_pitched_image_and_mask(gpu):
    import torch
    img, mask = R.synth_image(37, 131, 1, "noise"), R.synth_mask(37, 131, 1)
    big = torch.full((50, 333), 255, dtype=torch.uint8, device=gpu)
    bigm = torch.full((50, 407), 255, dtype=torch.uint8, device=gpu)
    big[5:42, 11:142] = dev(img, gpu)
    bigm[2:39, 7:138] = dev(mask, gpu)
    timg, tmask = big[5:42, 11:142], bigm[2:39, 7:138]
    assert timg.stride(0) == 333 and tmask.stride(0) == 407
    check(gpu, img, 10, True, mask=mask, timg=timg, tmask=tmask)
    check(gpu, img, 0, False, timg=timg)
    # columns that are not dense (a transposed view) are copied by the mirror
    check(gpu, np.ascontiguousarray(img.T), 10, True, timg=timg.t())


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("step", [TW + 11, 2 * TW + 7])   # odd steps: every row has another alignment
def test_roi_with_misaligned_base_and_odd_step(gpu, offset, step):
    import torch
    assert step % 2 == 1
    rows, cols = TH + 6, step - 5
    img = R.synth_image(rows, cols, offset * 100 + step, "noise")
    buf = torch.full((offset + rows * step + 8,), 255, dtype=torch.uint8, device=gpu)
    view = torch.as_strided(buf, (rows, cols), (step, 1), offset)
    view.copy_(dev(img, gpu))
    assert view.data_ptr() % 4 == (buf.data_ptr() + offset) % 4 and view.stride(0) == step
    check(gpu, img, 10, True, timg=view)
    eq(cuda().fast_score(view, None, 10).cpu().numpy(), R.score_plane(img, 10)[1])


def test_image_in_the_last_bytes_of_its_allocation(gpu):
    """The narrowest shape at which a wide staged load over-reads: the image's last byte is the allocation's last byte, its base and
    step are odd.  Through the C-ABI on memory of the library's own allocator."""
    import torch
    from opencv_contrib_amd import capi
    L = capi.lib()
    rows, cols, step, lead = 9, TW + 3, TW + 5, 3
    total = lead + (rows - 1) * step + cols
    img = R.synth_image(rows, cols, 77, "noise")
    host = np.full(total, 255, np.uint8)
    for y in range(rows):
        host[lead + y * step: lead + y * step + cols] = img[y]
    p = C.c_void_p()
    capi.check(L.mi_malloc(C.byref(p), total))
    try:
        capi.check(L.mi_memcpy_h2d(p, total, host.ctypes.data_as(C.c_void_p), total, total, 1, None))
        capi.check(L.mi_stream_synchronize(None))
        kp = torch.empty((2, 5000), dtype=torch.float32, device=gpu)
        h = C.c_void_p()
        capi.check(L.mi_fast_create(C.byref(capi.FastParams(10, 1, 5000)), C.byref(h)))
        n = C.c_int(-1)
        mi = capi.Mat(p.value + lead, step, rows, cols, capi.MI_8UC1)
        capi.check(L.mi_fast_detect(h, C.byref(mi), None, C.byref(capi.mat_from_tensor(kp)), C.byref(n), None))
        L.mi_fast_destroy(h)
        loc, resp = got(kp[:, : n.value])
        wl, wr, _ = R.detect(img, 10, True)
        eq(loc, wl)
        eq(resp, wr)
        assert n.value > 0
    finally:
        L.mi_free(p)


# ------------------------------------------------------------------ masks, thresholds, suppression
def test_masks(gpu):
    img = R.synth_image(40, 140, 9, "noise")
    y, x = np.mgrid[0:40, 0:140]
    loc, _, _ = check(gpu, img, 10, True, mask=np.zeros_like(img))
    assert len(loc) == 0
    a = check(gpu, img, 10, True, mask=np.full_like(img, 255))
    b = check(gpu, img, 10, True)
    eq(a[0], b[0]); eq(a[1], b[1])
    checker = (((y + x) & 1) * 255).astype(np.uint8)
    loc, _, count = check(gpu, img, 10, True, mask=checker)
    assert 0 < count and ((loc[:, 0] + loc[:, 1]) & 1).all()
    one255 = np.where((y // 3 + x // 5) % 3 == 0, 1, np.where((y + x) % 3 == 1, 255, 0)).astype(np.uint8)
    assert set(np.unique(one255)) == {0, 1, 255}
    check(gpu, img, 10, True, mask=one255)
    check(gpu, img, 10, False, mask=one255)
    eq(cuda().fast_score(dev(img, gpu), dev(one255, gpu), 10).cpu().numpy(), R.score_plane(img, 10, one255)[1])


@pytest.mark.parametrize("th", [0, 1, 10, 254, 255, 300])
def test_thresholds(gpu, th):
    img = R.synth_image(23, 71, 3, "noise")
    img[10, 10] = 0
    for dy, dx in R.RING:
        img[10 + dy, 10 + dx] = 255   # the one pixel that is still a corner at 254
    for nms in (True, False):
        loc, resp, count = check(gpu, img, th, nms)
        if th >= 255:
            assert count == 0 and len(loc) == 0
        if th == 254:
            assert count == 1 and loc.tolist() == [[10, 10]] and resp.tolist() == [254.0 if nms else 0.0]
    eq(cuda().fast_score(dev(img, gpu), None, th).cpu().numpy(), R.score_plane(img, th)[1])


def test_threshold_zero_candidate_of_score_zero_never_survives(gpu):
    flat = R.synth_image(23, 71, 0, "flat").astype(np.int32)
    for dy, dx in R.RING[:9]:
        flat[10 + dy, 30 + dx] += 1
    img = flat.astype(np.uint8)
    cand, score = R.score_plane(img, 0)
    assert cand[10, 30] and score[10, 30] == 0
    loc, _, count = check(gpu, img, 0, True)
    assert count > 0 and (30, 10) not in {(int(x), int(y)) for x, y in loc}
    raw, _, _ = check(gpu, img, 0, False)
    assert (30, 10) in {(int(x), int(y)) for x, y in raw}


def test_suppression_off_is_row_major_with_zero_responses_and_blocks_tie(gpu):
    img = R.synth_image(40, 140, T.G.case_seed("blocks"), "blocks")
    loc, resp, count = check(gpu, img, 10, False)
    assert len(loc) == count >= 100 and not resp.any()
    eq(loc, T.row_major(loc))
    nl, nr, _ = check(gpu, img, 10, True)
    assert R.tie_count(img, 10) >= 100 and len(nl) < count // 10   # equal neighbouring scores suppress each other


def test_truncation(gpu):
    """the first max_npoints candidates in row-major order keep a slot; the ones cut still suppress their neighbours"""
    img = R.synth_image(40, 140, 21, "noise")
    count = R.detect(img, 10, False)[2]
    full = R.detect(img, 10, True, count)[0]
    for maxn in (1, count - 1, count, count + 1):
        for nms in (True, False):
            loc, resp, c = check(gpu, img, 10, nms, maxn)
            assert c == count and len(loc) <= maxn
            if not nms:
                assert len(loc) == min(count, maxn)
    cut = check(gpu, img, 10, True, count // 2)[0]
    assert {tuple(v) for v in cut.tolist()} < {tuple(v) for v in full.tolist()}


# ------------------------------------------------------------------ every ring pattern
_allmasks = {}


def allmasks(pol):
    if pol not in _allmasks:
        img = R.all_masks_image(pol)
        _allmasks[pol] = (img,) + R.score_plane(img, 10)
    return _allmasks[pol]


@pytest.mark.parametrize("name,pol", [("bright", 1), ("dark", -1)])
def test_every_ring_pattern(gpu, name, pol):
    img, cand, score = allmasks(pol)
    t = dev(img, gpu)
    s = cuda().fast_score(t, None, 10).cpu().numpy()
    eq(s, score)
    eq(R.centre_bitmap(s > 0), np.load(T.ALLMASKS)[name])
    n = int(cand.sum())
    loc, resp = got(cuda().FastFeatureDetector.create(10, False, max_npoints=n + 5).detectAsync(t))
    ys, xs = np.nonzero(cand)
    eq(loc, np.stack([xs, ys], 1).astype(np.int16))
    assert not resp.any()
    nl, nr = got(cuda().FastFeatureDetector.create(10, True, max_npoints=n).detectAsync(t))
    assert len(nl) == 0 or (nr == 10).all()   # every candidate scores 10 here: only isolated ones survive
    wl, wr = R.detect_from(cand, score, True, n)
    eq(nl, wl)
    eq(nr, wr)


# ------------------------------------------------------------------ the handle
def test_handle_reuse_parameter_change_and_stream(gpu):
    import torch
    big, small = R.synth_image(200, 300, 1, "noise"), R.synth_image(9, 12, 2, "noise")
    det = cuda().FastFeatureDetector.create(10, True)
    check(gpu, big, 10, True, det=det)
    b = det.scratchBytes()
    assert b > 200 * 300
    check(gpu, small, 10, True, det=det)
    assert det.scratchBytes() == b     # grows, never shrinks
    check(gpu, big, 10, True, det=det)
    det.setThreshold(40)
    check(gpu, big, 40, True, det=det)
    det.setNonmaxSuppression(False)
    check(gpu, big, 40, False, det=det)
    det.setMaxNumPoints(17)
    check(gpu, big, 40, False, 17, det=det)
    assert (det.getThreshold(), det.getNonmaxSuppression(), det.getMaxNumPoints(), det.getType()) == (40, False, 17, 2)
    from opencv_contrib_amd import capi
    with pytest.raises(capi.MiError):
        det.setThreshold(-5)
    with pytest.raises(capi.MiError):
        det.setMaxNumPoints(0)
    with pytest.raises(capi.MiError):
        det.setType(0)
    assert (det.getThreshold(), det.getMaxNumPoints()) == (40, 17)   # a rejected value leaves the object as it was
    det.setNonmaxSuppression(True); det.setMaxNumPoints(5000)
    st = torch.cuda.Stream()
    t = dev(big, gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        loc, resp = got(det.detectAsync(t))
    wl, wr, _ = R.detect(big, 40, True)
    eq(loc, wl)
    eq(resp, wr)
    loc, resp = got(det.detectAsync(t, stream=st.cuda_stream))
    eq(loc, wl)


def test_entry_points_reject_with_a_handle(gpu):
    import torch
    from opencv_contrib_amd import capi
    det = cuda().FastFeatureDetector.create(10, True, max_npoints=100)
    img = torch.zeros((20, 30), dtype=torch.uint8, device=gpu)
    for bad_mask, code in ((torch.zeros((20, 31), dtype=torch.uint8, device=gpu), -3), (torch.zeros((20, 30), dtype=torch.float32, device=gpu), -2)):
        with pytest.raises(capi.MiError) as e:
            det.detectAsync(img, bad_mask)
        assert e.value.code == code
    with pytest.raises(capi.MiError) as e:
        det.detectAsync(img.to(torch.float32))
    assert e.value.code == -2
    n = C.c_int()
    for kp, code in ((torch.empty((2, 99), device=gpu), -3), (torch.empty((3, 100), device=gpu), -3), (torch.empty((2, 100), dtype=torch.int32, device=gpu), -2)):
        rc = capi.lib().mi_fast_detect(det._h, C.byref(capi.mat_from_tensor(img)), None, C.byref(capi.mat_from_tensor(kp)), C.byref(n), None)
        assert rc == code, (rc, code)


def test_batch_equals_single_calls(gpu):
    frames = [R.synth_image(40, 140, 1, "noise"), np.zeros((6, 50), np.uint8), R.synth_image(23, 71, 0, "flat"), R.synth_image(TH + 1, 2 * TW + 1, 2, "noise"),
              R.synth_image(130, 70, 3, "blocks"), R.synth_image(7, 7, 4, "noise")]
    masks = [R.synth_mask(40, 140, 5), None, None, None, R.synth_mask(130, 70, 6), None]
    for nms in (True, False):
        det = cuda().FastFeatureDetector.create(10, nms, max_npoints=300)
        singles = [det.detectAsync(dev(f, gpu), dev(m, gpu) if m is not None else None).cpu().numpy() for f, m in zip(frames, masks)]
        batch = det.detect_batch([dev(f, gpu) for f in frames], [dev(m, gpu) if m is not None else None for m in masks])
        assert len(batch) == len(frames)
        for i, (s, b) in enumerate(zip(singles, batch)):
            assert s.tobytes() == b.cpu().numpy().tobytes() and s.shape == tuple(b.shape), i
            wl, wr, _ = R.detect(frames[i], 10, nms, 300, masks[i])
            eq(got(b)[0], wl)
            eq(got(b)[1], wr)
        assert batch[1].shape[1] == 0 and batch[2].shape[1] == 0 and batch[0].shape[1] > 0 and batch[3].shape[1] > 0
        nomask = det.detect_batch([dev(f, gpu) for f in frames])
        for i, b in enumerate(nomask):
            eq(got(b)[0], R.detect(frames[i], 10, nms, 300)[0])


def test_locations_to_points(gpu):
    img = R.synth_image(40, 140, 1, "noise")
    det = cuda().FastFeatureDetector.create()
    kp = det.detectAsync(dev(img, gpu))
    pts = cuda().fast_locations_to_points(kp)
    loc, _ = got(kp)
    assert tuple(pts.shape) == (1, len(loc), 2) and len(loc) > 50
    eq(pts.cpu().numpy()[0], loc.astype(np.float32))
    eq(pts.cpu().numpy()[0], np.array([k[:2] for k in det.convert(kp)], np.float32))
    assert tuple(cuda().fast_locations_to_points(kp[:, :0]).shape) == (1, 0, 2)
    # ... which is what the sparse tracker takes, without leaving the device
    nxt, status, _ = cuda().SparsePyrLKOpticalFlow.create().calc(dev(img, gpu), dev(img, gpu), pts)
    assert tuple(nxt.shape) == tuple(pts.shape) and status.any()


# ------------------------------------------------------------------ the C++ mirror
@pytest.mark.parametrize("nms,masked", [(1, 0), (0, 1)])
def test_cpp_mirror_equals_python_mirror(gpu, tmp_path, nms, masked):
    exe = T.build_shim(tmp_path)
    rows, cols, th, maxn = 37, 131, 12, 200
    img, mask = R.synth_image(rows, cols, 8, "noise"), R.synth_mask(rows, cols, 8)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("6i", rows, cols, th, nms, maxn, masked) + img.tobytes() + (mask.tobytes() if masked else b""))
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = fout.read_bytes()
    n = struct.unpack("i", raw[:4])[0]
    kp = cuda().FastFeatureDetector.create(th, bool(nms), max_npoints=maxn).detectAsync(dev(img, gpu), dev(mask, gpu) if masked else None)
    assert n == kp.shape[1] > 0
    assert raw[4:4 + 8 * n] == kp.cpu().numpy().tobytes()
    conv = np.frombuffer(raw[4 + 8 * n:], np.float32).reshape(n, 5)
    eq(conv, np.array(cuda().FastFeatureDetector.convert(kp), np.float32))
