"""NumPy restatement of cv::cuda::FastFeatureDetector (modules/cudafeatures2d/src/cuda/fast.cu, src/fast.cpp) -- TEST INFRASTRUCTURE.

Written from the reference's definitions, not from the HIP kernels: the ring test is the literal comparison of the sixteen ring pixels,
the score the literal search for the largest threshold at which the pixel still is a candidate.  tests/test_fast_ref.py holds it to what
the reference's own kernels recorded (tests/golden/fast_ref*.npz); tests/test_fast_gpu.py holds the HIP class to it.

Order: the reference appends in the arrival order of its atomics; this library's order, and the restatement's, is row-major (y, then x).
"""
import numpy as np

# ring pixel k as (dy, dx): bit k of the reference's masks (fast.cu:223-252, calcMask :67-183)
RING = [(3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3), (0, -3), (1, -3), (2, -2),
        (3, -1)]
FEATURE_SIZE, ROWS_COUNT, LOCATION_ROW, RESPONSE_ROW = 7, 2, 0, 1   # cudafeatures2d.hpp:429-432
TYPE_9_16 = 2   # cv::FastFeatureDetector::TYPE_9_16, main repository features2d.hpp


# ---------------------------------------------------------------- inputs (integer arithmetic only: the same on every NumPy)
def _hash(y, x, s):
    v = y.astype(np.uint64) * np.uint64(7919) + x.astype(np.uint64) * np.uint64(104729) + np.uint64(s * 15485863 + 12345)
    v = (v ^ (v >> np.uint64(13))) * np.uint64(2654435761) & np.uint64(0xFFFFFFFF)
    v = (v ^ (v >> np.uint64(16))) * np.uint64(2246822519) & np.uint64(0xFFFFFFFF)
    return (v >> np.uint64(11)).astype(np.int64)


def synth_image(rows, cols, seed, kind):
    """noise: uniform bytes; blocks: random constant rectangles on a flat ground (many exact score ties); flat: one value"""
    y, x = np.mgrid[0:rows, 0:cols]
    if kind == "noise":
        return (_hash(y, x, seed) & 255).astype(np.uint8)
    if kind == "flat":
        return np.full((rows, cols), 97, np.uint8)
    assert kind == "blocks", kind
    img = np.full((rows, cols), 60, np.int64)
    k = np.arange(max(4, rows * cols // 120))
    z = np.zeros_like(k)
    y0, x0 = _hash(k, z, seed) % rows, _hash(k, z + 1, seed) % cols
    hh, ww = 2 + _hash(k, z + 2, seed) % 7, 2 + _hash(k, z + 3, seed) % 9
    val = 20 + 40 * (_hash(k, z + 4, seed) % 6)
    for i in range(len(k)):
        img[y0[i]:y0[i] + hh[i], x0[i]:x0[i] + ww[i]] = val[i]
    return img.astype(np.uint8)


def synth_mask(rows, cols, seed):
    """random 0 / 1 / 255"""
    y, x = np.mgrid[0:rows, 0:cols]
    return np.array([0, 1, 255, 255], np.uint8)[_hash(y, x, seed + 99) % 4]


def all_masks_image(polarity):
    """1792 x 1792: 256 x 256 patches of 7 x 7; patch m (row m >> 8, column m & 255) has centre 128 and ring pixel k at 128 + polarity * 11
    iff bit k of m, 128 elsewhere.  Every 16-bit ring pattern occurs at a patch centre."""
    assert polarity in (-1, 1)
    img = np.full((1792, 1792), 128, np.uint8)
    m = np.arange(65536)
    cy, cx = (m >> 8) * 7 + 3, (m & 255) * 7 + 3
    for k, (dy, dx) in enumerate(RING):
        on = (m >> k) & 1 == 1
        img[cy[on] + dy, cx[on] + dx] = 128 + polarity * 11
    return img


def centre_bitmap(cand):
    """the 65 536 patch centres of an all_masks_image's candidate map, packed to 8 KB (bit m & 7 of byte m >> 3, little bit order)"""
    return np.packbits(cand[3::7, 3::7].reshape(-1).astype(np.uint8), bitorder="little")


# ---------------------------------------------------------------- the ring test
def run_of_nine(m):
    """isKeyPoint's table test (fast.cu:187-191) as what the table holds: bits k .. k + 8 (mod 16) all set for some k"""
    m = np.asarray(m, np.uint64)
    d = m | (m << np.uint64(16))
    ok = np.zeros(m.shape, bool)
    for k in range(16):
        ok |= ((d >> np.uint64(k)) & np.uint64(0x1FF)) == np.uint64(0x1FF)
    return ok


def _ring_diffs(img, ys, xs):
    """ring - centre for the pixels (ys, xs): (n, 16) int32"""
    v = img[ys, xs].astype(np.int32)
    return np.stack([img[ys + dy, xs + dx].astype(np.int32) - v for dy, dx in RING], 1)


def _is_candidate(diffs, th):
    w = (np.uint64(1) << np.arange(16, dtype=np.uint64))[None, :]
    m1 = ((diffs < -th) * w).sum(1, dtype=np.uint64)
    m2 = ((diffs > th) * w).sum(1, dtype=np.uint64)
    return run_of_nine(m1) | run_of_nine(m2)


def tested_pixels(img, mask=None):
    rows, cols = img.shape
    t = np.zeros((rows, cols), bool)
    if rows >= 7 and cols >= 7:
        t[3:rows - 3, 3:cols - 3] = True
    if mask is not None:
        t &= mask != 0
    return t


def score_plane(img, threshold, mask=None):
    """-> (candidate map, the reference's CV_32SC1 plane: cornerScore at candidates, 0 elsewhere).  cornerScore (fast.cu:193-214) is the
    largest t in [threshold, 255] at which the pixel still is a candidate, found here by trying every t upwards."""
    rows, cols = img.shape
    cand = np.zeros((rows, cols), bool)
    score = np.zeros((rows, cols), np.int32)
    ys, xs = np.nonzero(tested_pixels(img, mask))
    if len(ys) == 0:
        return cand, score
    diffs = _ring_diffs(img, ys, xs)
    live = _is_candidate(diffs, threshold)
    ys, xs, diffs = ys[live], xs[live], diffs[live]
    cand[ys, xs] = True
    s = np.full(len(ys), threshold, np.int32)
    idx = np.arange(len(ys))
    t = threshold + 1
    while len(idx) and t <= 255:
        still = _is_candidate(diffs[idx], t)
        idx = idx[still]
        s[idx] = t
        t += 1
    score[ys, xs] = s
    return cand, score


def detect_from(cand, score, nonmax_suppression=True, max_npoints=5000):
    """detect() from a candidate map and its score plane -> (loc (n, 2) int16 {x, y}, response (n,) float32), row-major"""
    ys, xs = np.nonzero(cand)   # row-major
    ys, xs = ys[:max_npoints], xs[:max_npoints]
    if nonmax_suppression:
        s = score[ys, xs]
        keep = np.ones(len(ys), bool)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dy or dx:
                    keep &= s > score[ys + dy, xs + dx]
        ys, xs = ys[keep], xs[keep]
        resp = score[ys, xs].astype(np.float32)
    else:
        resp = np.zeros(len(ys), np.float32)
    return np.stack([xs, ys], 1).astype(np.int16).reshape(-1, 2), resp


def detect(img, threshold=10, nonmax_suppression=True, max_npoints=5000, mask=None):
    """-> (loc (n, 2) int16 {x, y}, response (n,) float32, number of candidates), row-major.  fast.cpp:122-173: the first max_npoints
    candidates keep a slot, ALL candidates write their score; suppression runs over the kept ones against the full plane."""
    cand, score = score_plane(img, threshold, mask)
    loc, resp = detect_from(cand, score, nonmax_suppression, max_npoints)
    return loc, resp, int(cand.sum())


def pack(loc, resp):
    """the 2 x n CV_32FC1 matrix of detectAsync: row 0 short2 {x, y} in an element's 4 bytes, row 1 the response"""
    out = np.zeros((ROWS_COUNT, len(resp)), np.float32)
    out[LOCATION_ROW] = np.ascontiguousarray(loc, np.int16).reshape(-1).view(np.float32)
    out[RESPONSE_ROW] = resp
    return out


def unpack(mat):
    mat = np.ascontiguousarray(mat)
    assert mat.shape[0] == ROWS_COUNT and mat.itemsize == 4   # fast.cpp:193-194
    return mat[LOCATION_ROW].view(np.int16).reshape(-1, 2), mat[RESPONSE_ROW].view(np.float32)


def convert(mat):
    """FAST_Impl::convert, fast.cpp:175-208 -> [(x, y, size, angle, response)]"""
    if mat is None or mat.size == 0:
        return []
    loc, resp = unpack(mat)
    return [(float(x), float(y), float(FEATURE_SIZE), -1.0, float(r)) for (x, y), r in zip(loc, resp)]


def tie_count(img, threshold, mask=None):
    """candidates with an eight-neighbour of the same score that is a candidate too"""
    cand, score = score_plane(img, threshold, mask)
    ys, xs = np.nonzero(cand)
    tie = np.zeros(len(ys), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                tie |= cand[ys + dy, xs + dx] & (score[ys + dy, xs + dx] == score[ys, xs])
    return int(tie.sum())
