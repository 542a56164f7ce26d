"""NumPy restatement of cv::cuda::ORB (modules/cudafeatures2d/src/orb.cpp, src/cuda/orb.cu) and of what it calls (the resize_linear kernel
of cudawarping/src/cuda/resize.cu:234-269, THRESH_TOZERO, the 7 x 7 Gaussian of cudafilters) -- TEST INFRASTRUCTURE.

Written from the reference's definitions, not from the HIP kernels: every integer and f32 operation in the reference's order, one NumPy
float32 operation per C operation (NumPy never contracts).  The three transcendental places follow this library's definition (DESIGN.md
4.11): angle = f32(atan2(f64 m_01, f64 m_10)), sina / cosa = f32(sin / cos(f64 ar)), evaluated with the C library through `math`.
The cull is the total order (response descending, index ascending) with -0 == +0, i.e. a STABLE descending sort of FAST's row-major order.
cv::RNG (main repository) is restated here as well; no fixture pins it.
"""
import math

import numpy as np

import fast_numpy_ref as FR

F = np.float32
X_ROW, Y_ROW, RESPONSE_ROW, ANGLE_ROW, OCTAVE_ROW, SIZE_ROW, ROWS_COUNT = range(7)   # cudafeatures2d.hpp:455-461
HARRIS_SCORE, FAST_SCORE = 0, 1
NPOINTS, KBYTES = 512, 32
PI_F = F(3.14159265)      # CV_PI_F
HARRIS_K = F(0.04)
DEFAULTS = dict(nfeatures=500, scaleFactor=1.2, nlevels=8, edgeThreshold=31, firstLevel=0, WTA_K=2, scoreType=HARRIS_SCORE, patchSize=31,
                fastThreshold=20, blurForDescriptor=False)   # cudafeatures2d.hpp:463-472


def cv_round(v):
    """cvRound: to nearest, ties to even"""
    return int(np.rint(np.float64(v)))


# ---------------------------------------------------------------- cv::RNG and the patterns (orb.cpp:431-477,538-568)
class RNG:
    def __init__(self, state):
        self.state = state if state else 0xFFFFFFFF

    def next(self):
        self.state = ((self.state & 0xFFFFFFFF) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.state & 0xFFFFFFFF

    def uniform(self, a, b):
        if a == b:
            return a
        v = (self.next() % (b - a) + a) & 0xFFFFFFFF   # unsigned arithmetic, then (int)
        return v - (1 << 32) if v >= (1 << 31) else v


def c_div(a, b):
    """C's integer division (towards zero)"""
    return int(a / b) if a * b < 0 else a // b


def random_pool(patch_size):
    """makeRandomPattern -> (512, 2) int32 {x, y}"""
    rng = RNG(0x34985739)
    lo, hi = c_div(-patch_size, 2), patch_size // 2 + 1
    out = np.zeros((NPOINTS, 2), np.int32)
    for i in range(NPOINTS):
        out[i, 0] = rng.uniform(lo, hi)
        out[i, 1] = rng.uniform(lo, hi)
    return out


def make_pattern(patch_size, wta_k, pool0=None):
    """the 2 x N matrix ORB_Impl uploads; pool0: (512, 2) {x, y} or None (the random pool, for every patch size)"""
    pool = random_pool(patch_size) if pool0 is None else np.asarray(pool0, np.int32).reshape(NPOINTS, 2)
    if wta_k == 2:
        return np.ascontiguousarray(pool.T)
    rng = RNG(0x12345678)
    ntuples = KBYTES * 4
    pat = np.zeros((2, ntuples * wta_k), np.int32)
    for i in range(ntuples):
        for k in range(wta_k):
            while True:
                x, y = pool[rng.uniform(0, NPOINTS)]
                if not any(pat[0, wta_k * i + k1] == x and pat[1, wta_k * i + k1] == y for k1 in range(k)):
                    pat[0, wta_k * i + k], pat[1, wta_k * i + k] = x, y
                    break
    return pat


def pattern_reach(pat):
    h = np.sqrt(pat[0].astype(np.float64) ** 2 + pat[1].astype(np.float64) ** 2)
    return int(np.floor(h * 1.00001 + 0.5).max())


# ---------------------------------------------------------------- host tables (orb.cpp:506-534,573-576)
def get_scale(scale_factor, first_level, level):
    return F(math.pow(float(F(scale_factor)), float(level - first_level)))


def features_per_level(nfeatures, scale_factor, nlevels):
    factor = F(1) / F(scale_factor)
    num = F(nfeatures) * (F(1) - factor)   # int * float
    n_desired = F(float(num) / (1.0 - math.pow(float(factor), float(nlevels))))
    out, total = [], 0
    for _ in range(nlevels - 1):
        out.append(cv_round(n_desired))
        total += out[-1]
        n_desired = n_desired * factor
    out.append(nfeatures - total)
    return out


def u_max(patch_size):
    half = patch_size // 2
    u = [0] * (half + 2)
    lim = F(half) * np.sqrt(F(2)) / F(2)
    v = 0
    while v <= lim + F(1):
        u[v] = cv_round(np.sqrt(F(half * half - v * v)))
        v += 1
    v, v0 = half, 0
    while v >= lim:
        while u[v0] == u[v0 + 1]:
            v0 += 1
        u[v] = v0
        v0 += 1
        v -= 1
    return u


def reach(p, pat_reach, detect=True):
    r = pat_reach
    if detect:
        r = max(r, p["patchSize"] // 2)
        if p["scoreType"] == HARRIS_SCORE:
            r = max(r, 4)
    return r


def level_geometry(rows, cols, p, nlevels=None):
    """-> per level dict(rows, cols, scale, loc_scale, size, src, mask_mode)"""
    out = []
    for l in range(p["nlevels"] if nlevels is None else nlevels):
        sc = get_scale(p["scaleFactor"], p["firstLevel"], l)
        inv = F(1) / sc
        out.append(dict(rows=cv_round(F(rows) * inv), cols=cv_round(F(cols) * inv), scale=sc, loc_scale=sc if l != p["firstLevel"] else F(1),
                        size=F(p["patchSize"]) * sc, src=-1 if l <= p["firstLevel"] else l - 1,
                        mask_mode=0 if l == p["firstLevel"] else 1 if l < p["firstLevel"] else 2))
    return out


# ---------------------------------------------------------------- pyramid (resize.cu:234-269, resize.cpp:82-105, orb.cpp:672-718)
def sat_u8(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def resize_linear(src, drows, dcols):
    srows, scols = src.shape
    fx, fy = F(1.0 / (dcols / scols)), F(1.0 / (drows / srows))
    dx, dy = np.arange(dcols, dtype=F)[None, :], np.arange(drows, dtype=F)[:, None]
    sx, sy = dx * fx, dy * fy
    x1, y1 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    x2, y2 = x1 + 1, y1 + 1
    x1r, y1r = np.clip(x1, 0, scols - 1), np.clip(y1, 0, srows - 1)
    x2r, y2r = np.minimum(x2, scols - 1), np.minimum(y2, srows - 1)
    s = src.astype(F)
    wx2, wx1 = x2.astype(F) - sx, sx - x1.astype(F)
    wy2, wy1 = y2.astype(F) - sy, sy - y1.astype(F)
    out = np.zeros((drows, dcols), F)
    out = out + s[y1r, x1r] * (wx2 * wy2)
    out = out + s[y1r, x2r] * (wx1 * wy2)
    out = out + s[y2r, x1r] * (wx2 * wy1)
    out = out + s[y2r, x2r] * (wx1 * wy1)
    return sat_u8(out)


def pyramid_level(src, drows, dcols, src_mask=None, mask_mode=0, edge=31):
    """-> (image, mask): one level as this library computes it (the global kernel's arithmetic at every level)"""
    img = resize_linear(src, drows, dcols)
    m = np.full((drows, dcols), 255, np.uint8)
    if src_mask is not None:
        if mask_mode == 0:
            m = src_mask.copy()
        else:
            m = resize_linear(src_mask, drows, dcols)
            if mask_mode == 2:
                m = np.where(m > 254, m, 0).astype(np.uint8)
    frame = np.zeros((drows, dcols), bool)
    if dcols - 2 * edge > 0 and drows - 2 * edge > 0:
        frame[edge:drows - edge, edge:dcols - edge] = True
    return img, np.where(frame, m, 0).astype(np.uint8)


# ---------------------------------------------------------------- cull, Harris, angle (orb.cpp:722-737, orb.cu:94-228)
def cull(loc, resp, n_points):
    """-> (loc, resp) kept.  count <= n: unchanged; n == 0: none; else the first n of a stable descending sort"""
    if len(resp) <= n_points:
        return loc, resp
    if n_points == 0:
        return loc[:0], resp[:0]
    order = np.argsort(-resp.astype(np.float64), kind="stable")[:n_points]
    return loc[order], resp[order]


def harris(img, loc, block=7):
    I = img.astype(np.int64)
    r = block // 2
    x, y = loc[:, 0].astype(np.int64), loc[:, 1].astype(np.int64)
    a = np.zeros(len(loc), np.int64)
    b, c = a.copy(), a.copy()
    for i in range(block):
        for j in range(block):
            yy, xx = y - r + i, x - r + j
            Ix = (I[yy, xx + 1] - I[yy, xx - 1]) * 2 + (I[yy - 1, xx + 1] - I[yy - 1, xx - 1]) + (I[yy + 1, xx + 1] - I[yy + 1, xx - 1])
            Iy = (I[yy + 1, xx] - I[yy - 1, xx]) * 2 + (I[yy + 1, xx - 1] - I[yy - 1, xx - 1]) + (I[yy + 1, xx + 1] - I[yy - 1, xx + 1])
            a += Ix * Ix
            b += Iy * Iy
            c += Ix * Iy
    af, bf, cf = a.astype(F), b.astype(F), c.astype(F)
    scale = F(1) / (F(4 * block) * F(255))
    ssss = scale * scale * scale * scale
    return ((af * bf - cf * cf) - (HARRIS_K * (af + bf)) * (af + bf)) * ssss


def moments(img, loc, patch_size):
    """-> (m_01, m_10) int64"""
    I = img.astype(np.int64)
    half, um = patch_size // 2, u_max(patch_size)
    x, y = loc[:, 0].astype(np.int64), loc[:, 1].astype(np.int64)
    m01, m10 = np.zeros(len(loc), np.int64), np.zeros(len(loc), np.int64)
    for u in range(-half, half + 1):
        m10 += u * I[y, x + u]
    for v in range(1, half + 1):
        for u in range(-um[v], um[v] + 1):
            p, m = I[y + v, x + u], I[y - v, x + u]
            m01 += v * (p - m)
            m10 += u * (p + m)
    return m01, m10


def angle_from_moments(m01, m10):
    a = np.array([math.atan2(float(p), float(q)) for p, q in zip(m01, m10)], np.float64).astype(F)
    a = a + (a < 0).astype(F) * (F(2) * PI_F)
    return a * (F(180) / PI_F)


# ---------------------------------------------------------------- blur and descriptors (orb.cpp:570,815, orb.cu:250-381)
def gaussian_taps():
    t = [math.exp(-0.5 / 4.0 * (i - 3.0) * (i - 3.0)) for i in range(7)]
    s = 0.0
    for v in t:
        s += v
    inv = 1.0 / s
    return np.array([v * inv for v in t], np.float64).astype(F)


def reflect101(i, n):
    i = np.asarray(i).copy()
    if n == 1:
        return np.zeros_like(i)
    while ((i < 0) | (i >= n)).any():
        i = np.where(i < 0, -i, i)
        i = np.where(i >= n, 2 * n - 2 - i, i)
    return i


def blur(img):
    k = gaussian_taps()
    H, W = img.shape
    s = img.astype(F)
    buf = np.zeros((H, W), F)
    xs, ys = np.arange(W), np.arange(H)
    for j in range(7):
        buf = buf + s[:, reflect101(xs - 3 + j, W)] * k[j]
    dst = np.zeros((H, W), F)
    for j in range(7):
        dst = dst + buf[reflect101(ys - 3 + j, H)] * k[j]
    return sat_u8(dst)


def sincos(angle):
    ar = np.asarray(angle, F) * (PI_F / F(180))
    sina = np.array([math.sin(float(v)) for v in ar], np.float64).astype(F)
    cosa = np.array([math.cos(float(v)) for v in ar], np.float64).astype(F)
    return sina, cosa


def sample_coords(pat, sina, cosa):
    """-> (dy, dx) int64 of shape (n, N): the rounded rotated test points"""
    px, py = pat[0].astype(F)[None, :], pat[1].astype(F)[None, :]
    s, c = sina[:, None], cosa[:, None]
    dy = np.rint(px * s + py * c).astype(np.int64)
    dx = np.rint(px * c - py * s).astype(np.int64)
    return dy, dx


def descriptors_from(img, loc, sina, cosa, pat, wta_k):
    n = len(loc)
    if n == 0:
        return np.zeros((0, KBYTES), np.uint8)
    dy, dx = sample_coords(pat, sina, cosa)
    v = img[loc[:, 1].astype(np.int64)[:, None] + dy, loc[:, 0].astype(np.int64)[:, None] + dx].astype(np.int64)   # (n, N)
    out = np.zeros((n, KBYTES), np.int64)
    if wta_k == 2:
        t = v.reshape(n, KBYTES, 8, 2)
        for g in range(8):
            out |= (t[:, :, g, 0] < t[:, :, g, 1]).astype(np.int64) << g
    elif wta_k == 3:
        t = v.reshape(n, KBYTES, 4, 3)
        for g in range(4):
            t0, t1, t2 = t[:, :, g, 0], t[:, :, g, 1], t[:, :, g, 2]
            out |= np.where(t2 > t1, np.where(t2 > t0, 2, 0), (t1 > t0).astype(np.int64)) << (2 * g)
    else:
        t = v.reshape(n, KBYTES, 4, 4)
        for g in range(4):
            t0, t1, t2, t3 = t[:, :, g, 0], t[:, :, g, 1], t[:, :, g, 2], t[:, :, g, 3]
            a, m0 = (t1 > t0).astype(np.int64), np.maximum(t0, t1)
            b, m2 = np.where(t3 > t2, 3, 2), np.maximum(t2, t3)
            out |= np.where(m0 > m2, a, b) << (2 * g)
    return out.astype(np.uint8)


def descriptors(img, loc, angle, pat, wta_k):
    sina, cosa = sincos(angle)
    return descriptors_from(img, loc, sina, cosa, pat, wta_k)


def tie_sensitive_bits(loc, angle, pat, wta_k):
    """(n, 32, 8) bool: descriptor bits one of whose rounded sample coordinates changes when sina or cosa moves by one f32 ulp either way"""
    sina, cosa = sincos(angle)
    dy0, dx0 = sample_coords(pat, sina, cosa)
    moved = np.zeros(dy0.shape, bool)
    for s in (np.nextafter(sina, F(-2)), sina, np.nextafter(sina, F(2))):
        for c in (np.nextafter(cosa, F(-2)), cosa, np.nextafter(cosa, F(2))):
            dy, dx = sample_coords(pat, s.astype(F), c.astype(F))
            moved |= (dy != dy0) | (dx != dx0)
    n = len(loc)
    if wta_k == 2:
        return moved.reshape(n, KBYTES, 8, 2).any(3)
    g = moved.reshape(n, KBYTES, 4, wta_k).any(3)   # two bits per group
    return np.repeat(g, 2, axis=2)


# ---------------------------------------------------------------- the class (orb.cpp:578-866)
def detect_and_compute(img, mask=None, pool0=None, want_descriptors=True, **kw):
    """-> dict(keypoints (6, n) f32, descriptors (n, 32) u8 or None, levels=[per-level stages])"""
    p = dict(DEFAULTS, **kw)
    pat = make_pattern(p["patchSize"], p["WTA_K"], pool0)
    rows, cols = img.shape
    geo = level_geometry(rows, cols, p)
    quota = features_per_level(p["nfeatures"], p["scaleFactor"], p["nlevels"])
    edge = p["edgeThreshold"]
    assert edge >= reach(p, pattern_reach(pat) if want_descriptors else 0)
    levels, cols_out, desc_out = [], [], []
    for l, g in enumerate(geo):
        assert g["cols"] - 2 * edge > 0 and g["rows"] - 2 * edge > 0, "empty inner rectangle"
        src = img if g["src"] < 0 else levels[g["src"]]["img"]
        msrc = None if mask is None else (mask if g["src"] < 0 else levels[g["src"]]["mask"])
        limg, lmask = pyramid_level(src, g["rows"], g["cols"], msrc, g["mask_mode"], edge)
        st = dict(img=limg, mask=lmask, quota=quota[l])
        fast_max = int(0.05 * (g["rows"] * g["cols"]))
        loc, resp, ncand = FR.detect(limg, p["fastThreshold"], True, fast_max, lmask)
        st.update(fast_loc=loc, fast_resp=resp, fast_candidates=ncand)
        if p["scoreType"] == HARRIS_SCORE:
            loc, resp = cull(loc, resp, 2 * quota[l])
            st.update(cull1_loc=loc, cull1_resp=resp)
            resp = harris(limg, loc) if len(loc) else resp
            st.update(harris=resp)
        loc, resp = cull(loc, resp, quota[l])
        m01, m10 = moments(limg, loc, p["patchSize"])
        ang = angle_from_moments(m01, m10)
        st.update(loc=loc, resp=resp, m01=m01, m10=m10, angle=ang)
        if want_descriptors:
            dimg = blur(limg) if p["blurForDescriptor"] else limg
            st.update(dimg=dimg, desc=descriptors(dimg, loc, ang, pat, p["WTA_K"]))
            desc_out.append(st["desc"])
        k = np.zeros((6, len(loc)), F)
        k[0], k[1] = loc[:, 0].astype(F) * g["loc_scale"], loc[:, 1].astype(F) * g["loc_scale"]
        k[2], k[3], k[4], k[5] = resp, ang, F(l), g["size"]
        cols_out.append(k)
        levels.append(st)
    return dict(keypoints=np.concatenate(cols_out, 1), descriptors=np.concatenate(desc_out, 0) if want_descriptors else None, levels=levels,
                pattern=pat)


def compute_provided(img, keypoints, pool0=None, **kw):
    """useProvidedKeypoints (orb.cpp:581-635) -> (keypoints regrouped by octave, descriptors)"""
    p = dict(DEFAULTS, **kw)
    pat = make_pattern(p["patchSize"], p["WTA_K"], pool0)
    kp = np.asarray(keypoints, F)
    octave = kp[4].astype(np.int64)
    order = np.argsort(octave, kind="stable")
    kp = kp[:, order]
    nlevels = int(octave.max()) + 1
    geo = level_geometry(img.shape[0], img.shape[1], p, nlevels)
    imgs, desc = [], []
    for l, g in enumerate(geo):
        imgs.append(resize_linear(img if g["src"] < 0 else imgs[g["src"]], g["rows"], g["cols"]))
        k = kp[:, kp[4].astype(np.int64) == l]
        if k.shape[1] == 0:
            continue
        scale = F(1) / g["loc_scale"]
        loc = np.stack([np.rint((k[0] * scale).astype(np.float64)), np.rint((k[1] * scale).astype(np.float64))], 1).astype(np.int16)
        dimg = blur(imgs[l]) if p["blurForDescriptor"] else imgs[l]
        desc.append(descriptors(dimg, loc, k[3], pat, p["WTA_K"]))
    return kp, np.concatenate(desc, 0)


def pack_level(loc, resp, angle=None):
    """a keyPointsPyr_-style matrix: row 0 short2 {x, y}, row 1 the response, row 2 the angle"""
    out = np.zeros((3, len(resp)), F)
    out[0] = np.ascontiguousarray(loc, np.int16).reshape(-1).view(F)
    out[1] = resp
    if angle is not None:
        out[2] = angle
    return out
