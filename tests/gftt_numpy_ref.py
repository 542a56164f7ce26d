"""NumPy restatement of cv::cuda::CornernessCriteria and cv::cuda::CornersDetector -- TEST INFRASTRUCTURE.

Written from the reference's definitions (modules/cudafilters/src/filtering.cpp:458-545 with cuda/row_filter.hpp and column_filter.hpp,
modules/cudaimgproc/src/corners.cpp:83-176 with cuda/corners.cu:62-269, src/gftt.cpp:107-214 with cuda/gftt.cu:55-136), not from the HIP
kernels: Dx and Dy are whole planes here, the window sums read them at border-mapped coordinates, every float32 operation is rounded on
its own in the reference's order.  tests/test_gftt_ref.py holds it to its own invariants; tests/test_gftt_gpu.py holds the HIP stages
and classes to it.

Where the reference leaves the result open this restatement, like the library, has one rule each:
  - order among equal responses (the atomic append and thrust's unstable sort leave it open): response descending, then (y, x) ascending;
  - which candidates survive a capacity overflow (the atomic order decides): the first `capacity` in row-major order, then the sort.
"""
import numpy as np

f32 = np.float32
BORDER_REPLICATE, BORDER_REFLECT, BORDER_REFLECT101 = 1, 2, 4   # cv::BorderTypes, main repository
BORDERS = (BORDER_REFLECT101, BORDER_REFLECT, BORDER_REPLICATE)
MIN_CAPACITY = 1000   # gftt.cpp:122


# ---------------------------------------------------------------- inputs (integer arithmetic only: the same on every NumPy)
def _hash(y, x, s):
    v = y.astype(np.uint64) * np.uint64(7919) + x.astype(np.uint64) * np.uint64(104729) + np.uint64(s * 15485863 + 12345)
    v = (v ^ (v >> np.uint64(13))) * np.uint64(2654435761) & np.uint64(0xFFFFFFFF)
    v = (v ^ (v >> np.uint64(16))) * np.uint64(2246822519) & np.uint64(0xFFFFFFFF)
    return (v >> np.uint64(11)).astype(np.int64)


def synth_image(rows, cols, seed, kind, dtype=np.uint8):
    """noise: uniform bytes; blocks: constant rectangles on a flat ground (runs of exactly equal responses); flat: all zero.
    float32 images are the bytes / 255 plus a 1 / 4096 dither, so that they are not the 8-bit case again."""
    y, x = np.mgrid[0:rows, 0:cols]
    if kind == "noise":
        img = _hash(y, x, seed) & 255
    elif kind == "flat":
        img = np.zeros((rows, cols), np.int64)
    else:
        assert kind == "blocks", kind
        img = np.full((rows, cols), 60, np.int64)
        for by in range(2, rows - 6, 9):
            for bx in range(2, cols - 6, 11):
                img[by:by + 5, bx:bx + 6] = 180
    if dtype == np.uint8:
        return img.astype(np.uint8)
    assert dtype == np.float32
    return (img.astype(f32) / f32(255) + (_hash(y, x, seed + 7) & 15).astype(f32) / f32(4096)).astype(f32)


def synth_mask(rows, cols, seed):
    """random 0 / 1 / 255"""
    y, x = np.mgrid[0:rows, 0:cols]
    return np.array([0, 1, 255, 255], np.uint8)[_hash(y, x, seed + 99) % 4]


# ---------------------------------------------------------------- border_interpolate.hpp (main repository) as the kernels use it
def brd_low(i, n, border):
    i = np.asarray(i, np.int64)
    if border == BORDER_REPLICATE:
        return np.maximum(i, 0)
    if border == BORDER_REFLECT101:
        return np.abs(i) % n
    assert border == BORDER_REFLECT, border
    return (np.abs(i) - (i < 0)) % n


def brd_high(i, n, border):
    i = np.asarray(i, np.int64)
    if border == BORDER_REPLICATE:
        return np.minimum(i, n - 1)
    if border == BORDER_REFLECT101:
        return np.abs((n - 1) - np.abs((n - 1) - i)) % n
    assert border == BORDER_REFLECT, border
    return np.abs((n - 1) - np.abs((n - 1) - i) + (i > n - 1)) % n


def brd_window(i, n, border):
    """BrdRow* / BrdCol*::idx_col / idx_row = idx_low(idx_high(i)) (corners.cu:114-118); the texture's clamp for BORDER_REPLICATE (:150)"""
    return brd_low(brd_high(i, n, border), n, border)


def brd_filter(i, n, border):
    """what the separable filter reads for position i in [-1, n]: at_low left of the image, at_high right of it (row_filter.hpp:83-121)"""
    i = np.asarray(i, np.int64)
    return np.where(i < 0, brd_low(i, n, border), np.where(i >= n, brd_high(i, n, border), i))


def reflect_brute(i, n, border):
    """the position a mirror walk reaches: what the formulas stand for while |offset| stays below one image length"""
    period = 2 * n - 2 if border == BORDER_REFLECT101 else 2 * n
    if border == BORDER_REPLICATE:
        return min(max(i, 0), n - 1)
    if n == 1:
        return 0
    m = i % period
    if border == BORDER_REFLECT101:
        return m if m < n else period - m
    return m if m < n else period - 1 - m


# ---------------------------------------------------------------- corners.cpp:93-113 and filtering.cpp:524-545 for ksize == 3
def taps(dtype, block_size):
    """-> deriv [-1 0 1], smooth [1 2 1] * scale as float32; the scale and the products in double (Mat *= double)"""
    scale = float(1 << (3 - 1)) * block_size
    if np.dtype(dtype) == np.uint8:
        scale *= 255.0
    scale = 1.0 / scale
    return np.array([-1, 0, 1], f32), np.array([1.0 * scale, 2.0 * scale, 1.0 * scale], np.float64).astype(f32)


def _taps3(v0, v1, v2, k):
    s = np.zeros_like(v0)
    s = s + v0 * k[0]
    s = s + v1 * k[1]
    s = s + v2 * k[2]
    return s


def sobel(img, deriv, smooth, border):
    """linearRow<T, float> into a CV_32F buffer, then linearColumn<float, float>: -> Dx, Dy"""
    rows, cols = img.shape
    s = img.astype(f32)   # saturate_cast<float>
    deriv, smooth = np.asarray(deriv, f32), np.asarray(smooth, f32)
    x, y = np.arange(cols), np.arange(rows)
    xs = [brd_filter(x - 1, cols, border), x, brd_filter(x + 1, cols, border)]
    ys = [brd_filter(y - 1, rows, border), y, brd_filter(y + 1, rows, border)]
    row_d = _taps3(s[:, xs[0]], s[:, xs[1]], s[:, xs[2]], deriv)
    row_s = _taps3(s[:, xs[0]], s[:, xs[1]], s[:, xs[2]], smooth)
    dx = _taps3(row_d[ys[0]], row_d[ys[1]], row_d[ys[2]], smooth)
    dy = _taps3(row_s[ys[0]], row_s[ys[1]], row_s[ys[2]], deriv)
    return dx, dy


def response_from(dx, dy, block_size, border, harris, k=0.04):
    """cornerHarris_kernel / cornerMinEigenVal_kernel, corners.cu:62-131,164-240"""
    rows, cols = dx.shape
    a, b, c = (np.zeros((rows, cols), f32) for _ in range(3))
    y, x = np.arange(rows), np.arange(cols)
    lo = block_size // 2
    for i in range(block_size):
        ym = brd_window(y - lo + i, rows, border)
        for j in range(block_size):
            xm = brd_window(x - lo + j, cols, border)
            vx, vy = dx[np.ix_(ym, xm)], dy[np.ix_(ym, xm)]
            a = a + vx * vx
            b = b + vx * vy
            c = c + vy * vy
    if harris:
        k = f32(k)
        return a * c - b * b - k * (a + c) * (a + c)
    a = a * f32(0.5)
    c = c * f32(0.5)
    return (a + c) - np.sqrt((a - c) * (a - c) + b * b)


def response(img, block_size, border=BORDER_REFLECT101, harris=False, k=0.04, deriv=None, smooth=None):
    d, s = taps(img.dtype, block_size)
    dx, dy = sobel(img, d if deriv is None else deriv, s if smooth is None else smooth, border)
    return response_from(dx, dy, block_size, border, harris, k)


# ---------------------------------------------------------------- gftt.cpp:107-214
def threshold(resp, quality_level):
    """static_cast<float>(maxVal * qualityLevel_), the product in double (gftt.cpp:124)"""
    return f32(np.float64(resp.max()) * np.float64(quality_level))


def capacity(rows, cols):
    return max(MIN_CAPACITY, int(np.float64(rows * cols) * np.float64(0.05)))


def find_corners(resp, thr, mask=None, max_count=None):
    """findCorners, gftt.cu:55-88 -> (n, 2) float32 {x, y} in row-major order, cut at max_count; and the number found"""
    rows, cols = resp.shape
    if rows < 3 or cols < 3:
        return np.zeros((0, 2), f32), 0
    c = resp[1:-1, 1:-1]
    m = c.copy()
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                m = np.fmax(resp[dy:dy + rows - 2, dx:dx + cols - 2], m)
    ok = (c > f32(thr)) & (c == m)
    if mask is not None:
        ok &= mask[1:-1, 1:-1] != 0
    ys, xs = np.nonzero(ok)   # row-major
    pts = np.stack([xs + 1, ys + 1], 1).astype(f32)
    found = len(pts)
    return (pts if max_count is None else pts[:max_count]), found


def sort_corners(resp, pts):
    """sortCorners_gpu, gftt.cu:114-136, with the order rule: response descending ( -0 == +0, EigGreater uses > ), then (y, x) ascending"""
    pts = np.asarray(pts, f32).reshape(-1, 2)
    x, y = pts[:, 0].astype(np.int64), pts[:, 1].astype(np.int64)
    r = resp[y, x]
    order = np.lexsort((x, y, -(r + f32(0))))
    return pts[order]


def cv_round(v):
    return int(np.rint(v))   # to nearest, ties to even


def min_distance(pts, rows, cols, min_dist, max_corners):
    """the grid loop of gftt.cpp:140-207"""
    pts = np.asarray(pts, f32).reshape(-1, 2)
    cell = cv_round(min_dist)
    gw, gh = (cols + cell - 1) // cell, (rows + cell - 1) // cell
    grid = {}
    out = []
    lim = np.float64(min_dist) * np.float64(min_dist)
    for p in pts:
        xc, yc = int(p[0] / f32(cell)), int(p[1] / f32(cell))
        good = True
        for yy in range(max(0, yc - 1), min(gh - 1, yc + 1) + 1):
            for xx in range(max(0, xc - 1), min(gw - 1, xc + 1) + 1):
                for q in grid.get((yy, xx), ()):
                    dx, dy = f32(p[0] - q[0]), f32(p[1] - q[1])
                    if np.float64(f32(f32(dx * dx) + f32(dy * dy))) < lim:
                        good = False
                        break
                if not good:
                    break
            if not good:
                break
        if good:
            grid.setdefault((yc, xc), []).append(p)
            out.append(p)
            if max_corners > 0 and len(out) == max_corners:
                break
    return np.array(out, f32).reshape(-1, 2)


def detect(img, mask=None, max_corners=1000, quality_level=0.01, min_dist=0.0, block_size=3, harris=False, k=0.04, stages=None):
    """GoodFeaturesToTrackDetector::detect -> (n, 2) float32 {x, y}; stages (a dict): what was computed on the way"""
    rows, cols = img.shape
    resp = response(img, block_size, BORDER_REFLECT101, harris, k)
    thr = threshold(resp, quality_level)
    cand, found = find_corners(resp, thr, mask, capacity(rows, cols))
    srt = sort_corners(resp, cand)
    if stages is not None:
        stages.update(response=resp, threshold=thr, candidates=cand, found=found, sorted=srt)
    if len(srt) == 0:
        return srt
    if min_dist < 1:
        return srt[:max_corners] if max_corners > 0 else srt
    return min_distance(srt, rows, cols, min_dist, max_corners)
