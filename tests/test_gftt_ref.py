"""The NumPy restatement of CornernessCriteria / CornersDetector (tests/gftt_numpy_ref.py) held to what can be said about it without
the library: the border index formulas against a mirror walk, the filter against a plain Sobel in exact arithmetic, the window sums
against a direct per-pixel loop in the reference's order, findCorners, the order rule, the capacity rule and the minDistance loop
against direct statements of each."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gftt_numpy_ref as R  # noqa: E402

f32 = np.float32


# ------------------------------------------------------------------ border index formulas
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 16, 23])
def test_border_formulas_against_a_mirror_walk(n):
    """offsets up to three image lengths on either side.  Every result lies inside the axis.  Where the formulas are a reflection they
    equal the mirror walk: at_low and at_high up to one image length outside, which is all the 3-tap filter and a window no larger than
    the image need.  Further out they wrap with % n instead of reflecting again -- that is what the reference computes, so it is what the
    restatement computes."""
    i = np.arange(-3 * n, 4 * n)
    for border in R.BORDERS:
        for f, use in ((R.brd_low, i < n), (R.brd_high, i >= 0), (R.brd_window, i == i), (R.brd_filter, i == i)):
            v = f(i, n, border)[use]   # at_low serves positions left of the image's end, at_high right of its start
            assert v.min() >= 0 and v.max() <= n - 1, (f.__name__, border)
        walk = np.array([R.reflect_brute(int(k), n, border) for k in i])
        inside = (i >= 0) & (i < n)
        np.testing.assert_array_equal(R.brd_filter(i, n, border)[inside], i[inside])
        np.testing.assert_array_equal(R.brd_window(i, n, border)[inside], i[inside])
        near_low = (i < 0) & (i > -n) if border != R.BORDER_REFLECT else (i < 0) & (i >= -n)
        near_high = (i >= n) & (i < 2 * n - 1) if border != R.BORDER_REFLECT else (i >= n) & (i < 2 * n)
        if border == R.BORDER_REPLICATE:
            near_low, near_high = i < 0, i >= n
        np.testing.assert_array_equal(R.brd_low(i, n, border)[near_low], walk[near_low])
        np.testing.assert_array_equal(R.brd_high(i, n, border)[near_high], walk[near_high])
        np.testing.assert_array_equal(R.brd_filter(i, n, border)[near_low | near_high], walk[near_low | near_high])
        # the window's map is idx_low(idx_high(i)): right of the image it is at_high
        np.testing.assert_array_equal(R.brd_window(i, n, border)[near_high], walk[near_high])
    # ... and left of it idx_high comes first, which for BORDER_REFLECT gives BORDER_REFLECT101's position, not the mirror's:
    # BrdRowReflect::idx_col(-1) is 1 where at_low(-1) is 0.  Replicate and Reflect101 are the walk on both sides.
    lo = i[(i < 0) & (i > -n)]
    np.testing.assert_array_equal(R.brd_window(lo, n, R.BORDER_REFLECT), np.abs(lo) % n)
    for border in (R.BORDER_REFLECT101, R.BORDER_REPLICATE):
        np.testing.assert_array_equal(R.brd_window(lo, n, border), [R.reflect_brute(int(k), n, border) for k in lo])
    if n >= 3:
        assert R.brd_window(-1, n, R.BORDER_REFLECT) == 1 and R.brd_low(-1, n, R.BORDER_REFLECT) == 0


# ------------------------------------------------------------------ filter
def test_taps():
    d, s = R.taps(np.uint8, 3)
    assert d.tolist() == [-1, 0, 1] and s.dtype == f32
    assert s[0] == f32(1.0 / (4 * 3 * 255.0)) and s[1] == f32(2.0 / (4 * 3 * 255.0)) and s[0] == s[2]
    d, s = R.taps(np.float32, 7)
    assert s[0] == f32(1.0 / 28) and s[1] == f32(2.0 / 28)
    # +-1 and 2 are exact: scaling the float tap and rounding equals rounding the scaled double, whichever way it is read
    for bs in range(1, 64):
        for dt in (np.uint8, np.float32):
            _, s = R.taps(dt, bs)
            scale = 1.0 / (4.0 * bs * (255.0 if dt == np.uint8 else 1.0))
            assert s[1] == f32(np.float64(f32(2)) * scale) == f32(2 * scale) and s[0] == f32(scale)
            assert float(s[1]) == 2 * float(s[0])


@pytest.mark.parametrize("border", R.BORDERS)
def test_sobel_with_unit_taps_is_the_integer_sobel(border):
    """with smooth = [1 2 1] every product and sum of an 8-bit image is an exact integer in float32, so Dx and Dy must equal the Sobel
    of the image extended by the filter's border rule, in any order of evaluation"""
    img = R.synth_image(9, 13, 3, "noise")
    dx, dy = R.sobel(img, [-1, 0, 1], [1, 2, 1], border)
    rows, cols = img.shape
    ys = np.array([R.brd_filter(y, rows, border) for y in range(-1, rows + 1)])
    xs = np.array([R.brd_filter(x, cols, border) for x in range(-1, cols + 1)])
    e = img[np.ix_(ys, xs)].astype(np.int64)
    wx = (e[:-2, 2:] - e[:-2, :-2]) + 2 * (e[1:-1, 2:] - e[1:-1, :-2]) + (e[2:, 2:] - e[2:, :-2])
    wy = (e[2:, :-2] - e[:-2, :-2]) + 2 * (e[2:, 1:-1] - e[:-2, 1:-1]) + (e[2:, 2:] - e[:-2, 2:])
    np.testing.assert_array_equal(dx, wx.astype(f32))
    np.testing.assert_array_equal(dy, wy.astype(f32))


# ------------------------------------------------------------------ window sums, a pixel at a time in the reference's order
def _pixel(dx, dy, y, x, bs, border, harris, k):
    rows, cols = dx.shape
    a = b = c = f32(0)
    ibegin, jbegin = y - bs // 2, x - bs // 2
    for i in range(ibegin, ibegin + bs):
        yy = int(R.brd_window(i, rows, border))
        for j in range(jbegin, jbegin + bs):
            xx = int(R.brd_window(j, cols, border))
            vx, vy = dx[yy, xx], dy[yy, xx]
            a = f32(a + f32(vx * vx))
            b = f32(b + f32(vx * vy))
            c = f32(c + f32(vy * vy))
    if harris:
        return f32(f32(f32(a * c) - f32(b * b)) - f32(f32(f32(k) * f32(a + c)) * f32(a + c)))
    a, c = f32(a * f32(0.5)), f32(c * f32(0.5))
    return f32(f32(a + c) - f32(np.sqrt(np.float64(f32(f32(f32(a - c) * f32(a - c)) + f32(b * b))))))   # binary64 root, rounded once


@pytest.mark.parametrize("bs", [1, 2, 3, 4, 7])
@pytest.mark.parametrize("border", R.BORDERS)
def test_response_against_a_per_pixel_loop(border, bs):
    for dt, rows, cols in ((np.uint8, 6, 9), (np.float32, 5, 4)):
        img = R.synth_image(rows, cols, 17, "noise", dt)
        d, s = R.taps(dt, bs)
        dx, dy = R.sobel(img, d, s, border)
        for harris in (False, True):
            got = R.response_from(dx, dy, bs, border, harris, 0.04)
            want = np.array([[_pixel(dx, dy, y, x, bs, border, harris, 0.04) for x in range(cols)] for y in range(rows)], f32)
            np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def test_flat_image_has_a_zero_plane_and_no_corner():
    for dt in (np.uint8, np.float32):
        img = R.synth_image(23, 71, 1, "flat", dt) if dt == np.uint8 else np.zeros((23, 71), f32)
        assert not R.response(img, 3).any() and R.threshold(R.response(img, 3), 0.01) == 0
        assert R.detect(img).shape == (0, 2)


# ------------------------------------------------------------------ findCorners, order, capacity, minDistance
def test_find_corners_against_a_direct_loop():
    resp = R.response(R.synth_image(23, 71, 2, "noise"), 3)
    mask = R.synth_mask(23, 71, 2)
    thr = R.threshold(resp, 0.01)
    want = []
    for i in range(23):
        for j in range(71):
            if 0 < i < 22 and 0 < j < 70 and mask[i, j]:
                v = resp[i, j]
                if v > thr and v == resp[i - 1:i + 2, j - 1:j + 2].max():
                    want.append((j, i))
    got, found = R.find_corners(resp, thr, mask)
    assert found == len(want) > 20
    np.testing.assert_array_equal(got, np.array(want, f32))
    np.testing.assert_array_equal(R.find_corners(resp, thr, mask, 7)[0], np.array(want[:7], f32))   # the first in row-major order
    assert R.find_corners(resp, thr, mask, 7)[1] == found


def test_threshold_is_rounded_once_from_the_double_product():
    resp = np.array([[0.1, 0.7], [0.3, -2.0]], f32)
    assert R.threshold(resp, 0.01) == f32(float(f32(0.7)) * 0.01)
    assert R.threshold(resp, 1.0) == f32(0.7) and R.threshold(-resp, 0.5) == f32(1.0)
    assert R.capacity(100, 200) == 1000 and R.capacity(100, 201) == 1005 and R.capacity(1080, 1920) == 103680


def test_order_rule_and_blocks_ties():
    img = R.synth_image(40, 140, 1, "blocks")
    st = {}
    out = R.detect(img, None, 0, 0.01, 0.0, stages=st)
    r = st["response"][out[:, 1].astype(int), out[:, 0].astype(int)]
    idx = out[:, 1] * 140 + out[:, 0]
    assert ((r[:-1] > r[1:]) | ((r[:-1] == r[1:]) & (idx[:-1] < idx[1:]))).all()
    runs = np.diff(np.flatnonzero(np.concatenate([[True], r[1:] != r[:-1], [True]])))
    assert runs.max() >= 8          # a run of equal responses: the order among them is this library's rule, not the reference's
    assert {tuple(p) for p in out} == {tuple(p) for p in st["candidates"]}
    resp = np.array([[0, 0, 0, 0], [0, -0.0, 0.0, 0], [0, 1, -1, 0]], f32)
    pts = np.array([[2, 1], [1, 1], [2, 2], [1, 2]], f32)
    np.testing.assert_array_equal(R.sort_corners(resp, pts), np.array([[1, 2], [1, 1], [2, 1], [2, 2]], f32))   # -0 ties with +0


def test_strict_cases_have_unique_order_and_stay_below_capacity():
    for rows, cols, dt in ((23, 71, np.uint8), (40, 140, np.uint8), (23, 71, np.float32), (40, 140, np.float32)):
        st = {}
        out = R.detect(R.synth_image(rows, cols, rows * 1000 + cols, "noise", dt), None, 0, 0.01, 0.0, stages=st)
        r = st["response"][out[:, 1].astype(int), out[:, 0].astype(int)]
        assert len(out) >= 32 and len(np.unique(r)) == len(r) and st["found"] < R.capacity(rows, cols)


def test_min_distance_against_the_definition():
    """every survivor is at least minDistance from every earlier survivor, every dropped point is nearer than that to one of them"""
    st = {}
    R.detect(R.synth_image(40, 140, 11, "noise"), None, 0, 0.001, 0.0, stages=st)
    srt = st["sorted"].astype(np.float64)
    for md in (1.0, 3.0, 7.5):
        kept = []
        for p in srt:
            if all((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 >= md * md for q in kept):
                kept.append(p)
        np.testing.assert_array_equal(R.min_distance(st["sorted"], 40, 140, md, 0), np.array(kept, f32))
        np.testing.assert_array_equal(R.min_distance(st["sorted"], 40, 140, md, 10), np.array(kept[:10], f32))


# ------------------------------------------------------------------ the C++ mirror
LIBDIR = os.path.join(ROOT, "opencv_contrib_amd")


def build_shim(tmp_path):
    import subprocess
    exe = str(tmp_path / "gftt_shim")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "gftt_shim.cpp"),
                        "-o", exe, "-L" + LIBDIR, "-lmiflow", "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_cpp_mirror_compiles_and_fails_loudly_without_gpu(tmp_path):
    """caller code against cudaimgproc.hpp's corner classes compiles with the reference's signatures and defaults (static_asserts in
    tests/cpp/gftt_shim.cpp); ksize, borderType and the constructor's asserts need no device; creating the detector without one throws"""
    import subprocess
    import torch
    exe = build_shim(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 3 and "no CPU fallback" in r.stderr, (r.returncode, r.stderr)


# ------------------------------------------------------------------ what the reference's own code recorded (tools/make_golden_gftt.py)
import glob  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
STAGE_FILES = sorted(glob.glob(os.path.join(GOLDEN, "gftt_refstage_*.npz")))
CLASS_FILES = sorted(glob.glob(os.path.join(GOLDEN, "gftt_refclass_*.npz")))
STAGE_SIZES, STAGE_BS = ("13x31", "5x31", "3x3"), (2, 3, 5, 7)


def _ids(paths):
    return [os.path.basename(p)[len("gftt_"):-len(".npz")] for p in paths]


def eq_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == f32 and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def class_inputs(z):
    """-> image, mask, and the keyword arguments of gftt_numpy_ref.detect"""
    bs, harris, maxc = (int(v) for v in z["params"])
    k, q, md = (float(v) for v in z["fparams"])
    return z["img"], (z["mask"] if "mask" in z.files else None), dict(max_corners=maxc, quality_level=q, min_dist=md, block_size=bs,
                                                                      harris=bool(harris), k=k)


def check_class_fixture(z, name, corners, stages=None):
    """corners (and, where given, the stages on the way) against a class fixture: every bit and in order; `blocks_ties` as a set"""
    if stages is not None:
        eq_bits(stages["response"], z["response"])
        eq_bits(np.asarray(stages["threshold"], f32), z["threshold"])
        assert stages["found"] == int(z["total"]) < int(z["capacity"])
        eq_bits(stages["candidates"], z["candidates"])
    if name.endswith("blocks_ties"):
        assert len(corners) == len(z["corners"]) and {tuple(p) for p in corners} == {tuple(p) for p in z["corners"]}
        if stages is not None:
            assert {tuple(p) for p in stages["sorted"]} == {tuple(p) for p in z["sorted"]}
        return
    if stages is not None:
        eq_bits(stages["sorted"], z["sorted"])
    eq_bits(corners, z["corners"])


def test_fixtures_are_all_here():
    assert len(STAGE_FILES) == 6 and len(CLASS_FILES) == 15
    assert max(os.path.getsize(p) for p in STAGE_FILES + CLASS_FILES) < 96 * 1024


@pytest.mark.parametrize("path", STAGE_FILES, ids=_ids(STAGE_FILES))
def test_restatement_equals_reference_stages(path):
    """taps, Dx, Dy and both criteria's planes for every size and blockSize of one type and border mode"""
    z = np.load(path)
    border = int(z["border"])
    for tag in STAGE_SIZES:
        img = z[f"img_{tag}"]
        for bs in STAGE_BS:
            d, s = R.taps(img.dtype, bs)
            eq_bits(d, z[f"deriv_bs{bs}"])
            eq_bits(s, z[f"smooth_bs{bs}"])
            dx, dy = R.sobel(img, d, s, border)
            eq_bits(dx, z[f"dx_{tag}_bs{bs}"])
            eq_bits(dy, z[f"dy_{tag}_bs{bs}"])
            eq_bits(R.response_from(dx, dy, bs, border, False), z[f"mineig_{tag}_bs{bs}"])
            eq_bits(R.response_from(dx, dy, bs, border, True, float(z["harris_k"])), z[f"harris_{tag}_bs{bs}"])


@pytest.mark.parametrize("path", CLASS_FILES, ids=_ids(CLASS_FILES))
def test_restatement_equals_reference_class(path):
    z = np.load(path)
    img, mask, kw = class_inputs(z)
    st = {}
    out = R.detect(img, mask, stages=st, **kw)
    check_class_fixture(z, os.path.basename(path)[:-4], out, st)
    # the host loop on the reference's own sorted list
    if kw["min_dist"] >= 1 and len(z["sorted"]):
        eq_bits(R.min_distance(z["sorted"], *img.shape, kw["min_dist"], kw["max_corners"]), z["corners"])


def test_recording_again_gives_the_same_bytes(tmp_path):
    """tools/make_golden_gftt.py on the reference tree: skipped where the tree is absent"""
    import subprocess
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden_gftt as M
    if not M.have_reference():
        pytest.skip("the reference tree is not on this machine")
    env = dict(os.environ, GFTT_GOLDEN_DIR=str(tmp_path))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_gftt.py")], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for p in STAGE_FILES + CLASS_FILES:
        assert open(p, "rb").read() == open(os.path.join(str(tmp_path), os.path.basename(p)), "rb").read(), p


def test_sample_builds_against_the_headers(tmp_path):
    """samples/track_corners.cpp: the GFTT -> SparsePyrLK chain with nothing but the drop-in headers and the library"""
    import subprocess
    exe = str(tmp_path / "track_corners")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "samples", "track_corners.cpp"),
                        "-o", exe, "-L" + LIBDIR, "-lmiflow", "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
