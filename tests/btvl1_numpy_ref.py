"""NumPy float32 restatement of the reference's BTV-L1 super-resolution (class BTVL1_CUDA, superres/src/btv_l1_cuda.cpp and
superres/src/cuda/btv_l1_gpu.cu): the yardstick of tests/test_btvl1_gpu.py.  A plain helper module, not a conftest.

One function per reference step, deliberately UNFUSED (every intermediate plane of the reference exists here), so that it is an
independent statement of what the fused HIP kernels must produce.  Every intermediate is np.float32, every sum runs in the
reference's order, and no operation is contracted into an fma (the library is compiled with -ffp-contract=off).
Frames are (H, W) or (H, W, CN) arrays, CN in {3, 4}; motions and maps are pairs (x plane, y plane).

THE PIN: tests/test_ref_pin_btvl1.py holds every function here, process() and the BTVL1 ring driver BIT FOR BIT to the reference's own
kernels and host class executed on the CPU (oracle/_ref/libref_cu.so: btv_l1_gpu.cu, row_filter.hpp / column_filter.hpp, the resize /
remap kernels, the cudaarithm functors, btv_l1_cuda.cpp verbatim), and tests/golden/btvl1_refclass_*.npz keep that library's output of
process where the reference tree is absent.  Main-repo pieces (getGaussianKernel, PointFilter / CubicFilter, the border index maps)
are stand-ins there as well: DESIGN.md 2.
"""
from __future__ import annotations

import math

import numpy as np

F = np.float32

DEFAULTS = dict(scale=4, iterations=180, tau=1.3, lambda_=0.03, alpha=0.7, btv_kernel_size=7, blur_kernel_size=5, blur_sigma=0.0,
                temporal_area_radius=4)   # btv_l1_cuda.cpp:280-304,459-462


# ---------------------------------------------------------------------------------------------------------------- host tables
_SMALL_GAUSSIAN = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
                   7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}


def gaussian_kernel(n: int, sigma: float) -> np.ndarray:
    """getGaussianKernel(n, sigma, CV_32F) (main repo imgproc, called from cudafilters/src/filtering.cpp:573): the fixed tables for
    sigma <= 0 and odd n <= 7, else sigma = 0.3 ((n - 1) / 2 - 1) + 0.8; exp and the normalisation in double, stored as f32."""
    if sigma <= 0 and n % 2 == 1 and n <= 7:
        return np.array(_SMALL_GAUSSIAN[n], F)
    s = sigma if sigma > 0 else ((n - 1) * 0.5 - 1) * 0.3 + 0.8
    scale2x = -0.5 / (s * s)
    t = [math.exp(scale2x * (i - (n - 1) * 0.5) * (i - (n - 1) * 0.5)) for i in range(n)]
    inv = 1.0 / _sum_in_order(t)
    return np.array([v * inv for v in t], np.float64).astype(F)


def _sum_in_order(vals):
    s = 0.0
    for v in vals:
        s += v
    return s


def btv_weight_offsets(btv_kernel_size: int):
    """The (m, l) pairs in the enumeration order of calcBtvWeights / calcBtvRegularizationKernel (btv_l1_cuda.cpp:180-184,
    btv_l1_gpu.cu:207-211): m = 0 .. ksize, l = ksize down to -m."""
    ksize = (btv_kernel_size - 1) // 2
    return [(m, l) for m in range(ksize + 1) for l in range(ksize, -m - 1, -1)]


def btv_weights(btv_kernel_size: int, alpha: float) -> np.ndarray:
    """calcBtvWeights (btv_l1_cuda.cpp:171-187): pow(float(alpha), |m| + |l|) is std::pow(float, int), evaluated in double, stored f32."""
    a = float(F(alpha))
    return np.array([math.pow(a, abs(m) + abs(l)) for m, l in btv_weight_offsets(btv_kernel_size)], np.float64).astype(F)


# ---------------------------------------------------------------------------------------------------------------- borders
def reflect101(i, n):
    """BrdReflect101::idx_col (main repo core/cuda/border_interpolate.hpp, as used by row_filter.hpp:95,115):
    idx_low(idx_high(i)) with idx_low(i) = |i| % n and idx_high(i) = |last - |last - i|| % n."""
    i = np.asarray(i, np.int64)
    last = n - 1
    hi = np.abs(last - np.abs(last - i)) % n
    return np.abs(hi) % n


def replicate(i, n):
    """BrdReplicate::idx_col: clamp to 0 .. n - 1."""
    return np.clip(np.asarray(i, np.int64), 0, n - 1)


# ---------------------------------------------------------------------------------------------------------------- steps
def relative_motions(forward, backward, base_idx: int, size):
    """calcRelativeMotions (btv_l1_cuda.cpp:80-115).  forward[i] is used for i < n - 1, backward[i] for i > 0."""
    n = len(forward)
    z = np.zeros(size, F)
    rel_f, rel_b = [None] * n, [None] * n
    rel_f[base_idx], rel_b[base_idx] = (z.copy(), z.copy()), (z.copy(), z.copy())
    for i in range(base_idx - 1, -1, -1):
        rel_f[i] = (rel_f[i + 1][0] + forward[i][0], rel_f[i + 1][1] + forward[i][1])
        rel_b[i] = (rel_b[i + 1][0] + backward[i + 1][0], rel_b[i + 1][1] + backward[i + 1][1])
    for i in range(base_idx + 1, n):
        rel_f[i] = (rel_f[i - 1][0] + backward[i][0], rel_f[i - 1][1] + backward[i][1])
        rel_b[i] = (rel_b[i - 1][0] + forward[i - 1][0], rel_b[i - 1][1] + forward[i - 1][1])
    return rel_f, rel_b


def bicubic_coeff(x):
    """CubicFilter::bicubicCoeff == tvl1flow.cu:89-104 (Keys, a = -0.5)."""
    x = np.abs(np.asarray(x, F))
    near = x * x * (F(1.5) * x - F(2.5)) + F(1.0)
    far = x * (x * (F(-0.5) * x + F(2.5)) - F(4.0)) + F(2.0)
    return np.where(x <= F(1), near, np.where(x < F(2), far, F(0))).astype(F)


def resize_scale_factor(dsize: int, ssize: int) -> np.float32:
    """cudawarping/src/resize.cpp:82-83,105: the kernels receive float(1.0 / (double(dsize) / src))."""
    return F(1.0 / (float(dsize) / float(ssize)))


def resize_cubic(src, dh: int, dw: int):
    """cuda::resize(..., INTER_CUBIC) on f32: resize.cu:271-283 with CubicFilter<BrdReplicate> (main repo core/cuda/filters.hpp,
    the gather spelled out in-tree at tvl1flow.cu:118-148): taps cx = ceil(x - 2) .. floor(x + 2), w = c(x - cx) c(y - cy),
    sum += w src(clamped tap), wsum += w, result sum / wsum (0 where wsum == 0)."""
    src = np.asarray(src, F)
    H, W = src.shape[:2]
    fy, fx = resize_scale_factor(dh, H), resize_scale_factor(dw, W)
    sx = np.arange(dw, dtype=F) * fx
    sy = np.arange(dh, dtype=F) * fy
    xmin, xmax = np.ceil(sx - F(2)), np.floor(sx + F(2))
    ymin, ymax = np.ceil(sy - F(2)), np.floor(sy + F(2))
    shape = (dh, dw) + src.shape[2:]
    ex = (slice(None), slice(None)) + (None,) * (src.ndim - 2)
    acc = np.zeros(shape, F)
    wsum = np.zeros((dh, dw), F)
    for j in range(5):
        cy = ymin + F(j)
        wy = bicubic_coeff(sy - cy)
        oky = cy <= ymax
        iy = replicate(np.floor(cy), H)
        for i in range(5):
            cx = xmin + F(i)
            wx = bicubic_coeff(sx - cx)
            okx = cx <= xmax
            ix = replicate(np.floor(cx), W)
            w = (wx[None, :] * wy[:, None]).astype(F)
            ok = oky[:, None] & okx[None, :]
            v = src[iy[:, None], ix[None, :]]
            acc = np.where(ok[ex], acc + w[ex] * v, acc)
            wsum = np.where(ok, wsum + w, wsum)
    with np.errstate(divide="ignore", invalid="ignore"):
        res = np.where((wsum == 0)[ex], F(0), acc / wsum[ex])
    return res.astype(F)


def upscale_motions(motions, scale: int):
    """upscaleMotions (btv_l1_cuda.cpp:117-129): cubic resize by (scale, scale), then multiply by scale."""
    out = []
    for mx, my in motions:
        h, w = mx.shape
        out.append((resize_cubic(mx, h * scale, w * scale) * F(scale), resize_cubic(my, h * scale, w * scale) * F(scale)))
    return out


def motion_maps(forward_motion, backward_motion):
    """buildMotionMapsKernel (btv_l1_gpu.cu:73-95): forwardMap = pixel + BACKWARD motion, backwardMap = pixel + FORWARD motion."""
    h, w = forward_motion[0].shape
    x = np.arange(w, dtype=F)[None, :]
    y = np.arange(h, dtype=F)[:, None]
    forward_map = (x + backward_motion[0], y + backward_motion[1])
    backward_map = (x + forward_motion[0], y + forward_motion[1])
    return forward_map, backward_map


def remap_nearest(src, mapx, mapy):
    """cuda::remap(INTER_NEAREST, BORDER_REPLICATE): PointFilter truncates the coordinate toward zero (__float2int_rz), BrdReplicate
    clamps it (cudawarping/src/cuda/remap.cu:57-69,256-260)."""
    H, W = src.shape[:2]
    ix = np.clip(np.trunc(mapx), 0, W - 1).astype(np.int64)
    iy = np.clip(np.trunc(mapy), 0, H - 1).astype(np.int64)
    return src[iy, ix]


def gauss_separable(src, k):
    """SeparableLinearFilter of createGaussianFilter (cudafilters/src/filtering.cpp:441-442,555-580): row pass (along x) into an f32
    buffer, then column pass, each sum = sum + v * kernel[j] for j ascending from 0 (row_filter.hpp:132-136, column_filter.hpp),
    anchor ksize / 2, BORDER_REFLECT101 both ways."""
    src = np.asarray(src, F)
    k = np.asarray(k, F)
    n, a = len(k), len(k) // 2
    H, W = src.shape[:2]
    buf = np.zeros_like(src)
    xs = np.arange(W)
    for j in range(n):
        buf = buf + src[:, reflect101(xs - a + j, W)] * k[j]
    dst = np.zeros_like(src)
    ys = np.arange(H)
    for j in range(n):
        dst = dst + buf[reflect101(ys - a + j, H)] * k[j]
    return dst


def resize_nearest(src, dh: int, dw: int):
    """cuda::resize(..., INTER_NEAREST): src(trunc(y fy), trunc(x fx)), resize.cu:220-231."""
    H, W = src.shape[:2]
    fy, fx = resize_scale_factor(dh, H), resize_scale_factor(dw, W)
    iy = np.trunc(np.arange(dh, dtype=F) * fy).astype(np.int64)
    ix = np.trunc(np.arange(dw, dtype=F) * fx).astype(np.int64)
    return src[iy[:, None], ix[None, :]]


def diff_sign(a, b):
    """diffSign of the data term (btv_l1_gpu.cu:145-148,187-190): on reshape(1), i.e. every channel alike (btv_l1_cuda.cpp:168)."""
    return np.where(a > b, F(1), np.where(a < b, F(-1), F(0))).astype(F)


def upscale(src, scale: int):
    """upscale (btv_l1_cuda.cpp:146-162, btv_l1_gpu.cu:114-124): zero-stuffing, dst(y scale, x scale) = src(y, x)."""
    H, W = src.shape[:2]
    dst = np.zeros((H * scale, W * scale) + src.shape[2:], F)
    dst[::scale, ::scale] = src
    return dst


def btv_regularization(src, btv_kernel_size: int, weights):
    """calcBtvRegularization (btv_l1_cuda.cpp:189-207, btv_l1_gpu.cu:194-214): a border of (btvKernelSize - 1) / 2 stays 0; the
    four-channel diffSign writes 0 into the fourth channel (btv_l1_gpu.cu:157-165)."""
    src = np.asarray(src, F)
    H, W = src.shape[:2]
    ks = (btv_kernel_size - 1) // 2
    dst = np.zeros_like(src)
    if H - 2 * ks <= 0 or W - 2 * ks <= 0:
        return dst
    c = src[ks:H - ks, ks:W - ks]
    acc = np.zeros_like(c)
    for count, (m, l) in enumerate(btv_weight_offsets(btv_kernel_size)):
        p = src[ks + m:H - ks + m, ks + l:W - ks + l]
        q = src[ks - m:H - ks - m, ks - l:W - ks - l]
        d = diff_sign(c, p) - diff_sign(q, c)
        if src.ndim == 3 and src.shape[2] == 4:
            d[..., 3] = F(0)
        acc = acc + F(weights[count]) * d
    dst[ks:H - ks, ks:W - ks] = acc
    return dst


def add_weighted(a, alpha: float, b, beta: float, gamma: float):
    """cuda::addWeighted on f32: a * alpha + b * beta + gamma with the scalars cast to f32 (cudaarithm/src/cuda/add_weighted.cu:61-93)."""
    return (a * F(alpha) + b * F(beta)) + F(gamma)


# ---------------------------------------------------------------------------------------------------------------- process
def check_params(p):
    """The CV_Asserts of BTVL1_CUDA_Base::process (btv_l1_cuda.cpp:310-316) and of createGaussianFilter / the linear filters
    (filtering.cpp:568, kernel length <= 32)."""
    assert p["scale"] > 1 and p["iterations"] > 0 and p["tau"] > 0.0 and p["alpha"] > 0.0
    assert 0 < p["btv_kernel_size"] <= 16
    assert p["blur_kernel_size"] > 0 and p["blur_kernel_size"] % 2 == 1 and p["blur_kernel_size"] <= 31
    assert p["blur_sigma"] >= 0.0


def stage(frames, forward, backward, base_idx: int, params):
    """Everything before the iterations (btv_l1_cuda.cpp:339-354): returns (forward maps, backward maps, initial estimate)."""
    s = params["scale"]
    size = frames[0].shape[:2]
    rel_f, rel_b = relative_motions(forward, backward, base_idx, size)
    hi_f, hi_b = upscale_motions(rel_f, s), upscale_motions(rel_b, s)
    fmaps, bmaps = [], []
    for f, b in zip(hi_f, hi_b):
        fm, bm = motion_maps(f, b)
        fmaps.append(fm)
        bmaps.append(bm)
    init = resize_cubic(np.asarray(frames[base_idx], F), size[0] * s, size[1] * s)
    return fmaps, bmaps, init


def process(frames, forward, backward, base_idx: int, **kw):
    """BTVL1_CUDA_Base::process (btv_l1_cuda.cpp:306-400).  frames: n arrays (H, W[, CN]) f32; forward / backward: n entries, each a
    pair of (H, W) f32 planes or None where the reference does not read it."""
    p = dict(DEFAULTS, **kw)
    check_params(p)
    s, bk = p["scale"], p["btv_kernel_size"]
    frames = [np.asarray(f, F) for f in frames]
    lh, lw = frames[0].shape[:2]
    taps = gaussian_kernel(p["blur_kernel_size"], p["blur_sigma"])
    weights = btv_weights(bk, p["alpha"])
    fmaps, bmaps, X = stage(frames, forward, backward, base_idx, p)
    for _ in range(p["iterations"]):
        terms = []
        for k, src in enumerate(frames):
            a = remap_nearest(X, *bmaps[k])
            b = gauss_separable(a, taps)
            c = resize_nearest(b, lh, lw)
            c = diff_sign(src, c)
            a = upscale(c, s)
            b = gauss_separable(a, taps)
            terms.append(remap_nearest(b, *fmaps[k]))
        if p["lambda_"] > 0:
            reg = btv_regularization(X, bk, weights)
            X = add_weighted(X, 1.0, reg, -p["tau"] * p["lambda_"], 0.0)
        for t in terms:
            X = add_weighted(X, 1.0, t, p["tau"], 0.0)
    H, W = X.shape[:2]
    return np.ascontiguousarray(X[bk:H - bk, bk:W - bk])


# ---------------------------------------------------------------------------------------------------------------- the class
def saturate_u8(a):
    """convertTo(CV_8U) of an f32 matrix: round to nearest even, saturate."""
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


class BTVL1:
    """BTVL1_CUDA (btv_l1_cuda.cpp:426-583) around process(): the ring of 2 r + 1 frames, two flows per new frame, the window and
    baseIdx selection of processFrame, nextFrame returning convertTo(CV_8U).  `flow(prev, cur)` returns the (x, y) planes of
    opticalFlow_->calc(prev, cur); `source` has nextFrame() -> array or None and reset()."""

    def __init__(self, source, flow, **kw):
        self.p = dict(DEFAULTS, **kw)
        self.source, self.flow = source, flow
        self.first = True

    def _at(self, i, items):
        return ((i % len(items)) + len(items)) % len(items)

    def _read_next(self):
        cur = self.source.nextFrame()
        if cur is None:
            return
        self.store += 1
        self.frames[self._at(self.store, self.frames)] = np.asarray(cur).astype(F)
        if self.store > 0:
            self.fwd[self._at(self.store - 1, self.fwd)] = self.flow(self.prev, cur)
            self.bwd[self._at(self.store, self.bwd)] = self.flow(cur, self.prev)
        self.prev = cur.copy()

    def _process_frame(self, idx):
        r = self.p["temporal_area_radius"]
        start = max(idx - r, 0)
        end = min(start + 2 * r, self.store)
        fr, fw, bw, base = [], [], [], -1
        for i in range(start, end + 1):
            if i == idx:
                base = len(fr)
            fr.append(self.frames[self._at(i, self.frames)])
            fw.append(self.fwd[self._at(i, self.fwd)] if i < end else None)
            bw.append(self.bwd[self._at(i, self.bwd)] if i > start else None)
        kw = {k: v for k, v in self.p.items() if k != "temporal_area_radius"}
        self.outputs[self._at(idx, self.outputs)] = process(fr, fw, bw, base, **kw)

    def _init(self):
        r = self.p["temporal_area_radius"]
        n = 2 * r + 1
        self.frames, self.fwd, self.bwd, self.outputs = [None] * n, [None] * n, [None] * n, [None] * n
        self.store, self.prev = -1, None
        for _ in range(-r, r + 1):
            self._read_next()
        for i in range(r + 1):
            self._process_frame(i)
        self.proc, self.out = r, -1

    def nextFrame(self):
        if self.first:
            self._init()
            self.first = False
        if self.out >= self.store:
            return None
        self._read_next()
        if self.proc < self.store:
            self.proc += 1
            self._process_frame(self.proc)
        self.out += 1
        return saturate_u8(self.outputs[self._at(self.out, self.outputs)])

    def reset(self):
        self.source.reset()
        self.first = True


class ListSource:
    def __init__(self, frames):
        self.frames, self.pos = list(frames), 0

    def nextFrame(self):
        if self.pos >= len(self.frames):
            return None
        self.pos += 1
        return self.frames[self.pos - 1]

    def reset(self):
        self.pos = 0


# ---------------------------------------------------------------------------------------------------------------- acceptance
def mssim(i1, i2) -> float:
    """MSSIM of the reference's acceptance test (superres/test/test_superres.cpp:155-214), single channel; the 11 x 11, sigma 1.5
    blur is cv::GaussianBlur's (reflect-101 border)."""
    C1, C2 = 6.5025, 58.5225
    k = gaussian_kernel(11, 1.5)
    I1, I2 = np.asarray(i1).astype(F), np.asarray(i2).astype(F)
    blur = lambda a: gauss_separable(a, k)
    mu1, mu2 = blur(I1), blur(I2)
    s1 = blur(I1 * I1) - mu1 * mu1
    s2 = blur(I2 * I2) - mu2 * mu2
    s12 = blur(I1 * I2) - mu1 * mu2
    num = (2 * mu1 * mu2 + F(C1)) * (2 * s12 + F(C2))
    den = (mu1 * mu1 + mu2 * mu2 + F(C1)) * (s1 + s2 + F(C2))
    return float(np.mean((num / den).astype(np.float64)))


def synthetic_sequence(seed: int, n: int = 5, hh: int = 192, hw: int = 256, scale: int = 2, max_shift: int = 3):
    """The acceptance sequence (no video file is in the tree): a high-res scene of smooth seeded noise plus ~25 flat rectangles, n
    frames shifted by integer high-res offsets in -max_shift .. max_shift, degraded as DegradeFrameSource does
    (test_superres.cpp:137-148: 5 x 5 Gaussian, nearest decimation, Gaussian noise sigma = 10, one pixel in 500 set to 255).
    Returns (gold u8 frames, degraded u8 frames, offsets (ox, oy) per frame)."""
    rng = np.random.default_rng(seed)
    m = max_shift
    ch, cw = hh + 2 * m, hw + 2 * m
    coarse = rng.uniform(40, 215, (ch // 16 + 3, cw // 16 + 3)).astype(F)
    scene = resize_cubic(coarse, coarse.shape[0] * 16, coarse.shape[1] * 16)[:ch, :cw].copy()
    for _ in range(25):
        y0, x0 = int(rng.integers(0, ch - 8)), int(rng.integers(0, cw - 8))
        h, w = int(rng.integers(6, 48)), int(rng.integers(6, 48))
        scene[y0:y0 + h, x0:x0 + w] = F(rng.uniform(0, 255))
    scene = np.clip(scene, 0, 255)
    offs = [(int(rng.integers(-m, m + 1)), int(rng.integers(-m, m + 1))) for _ in range(n)]
    k5 = gaussian_kernel(5, 0.0)
    gold, low = [], []
    for ox, oy in offs:
        g = saturate_u8(scene[m + oy:m + oy + hh, m + ox:m + ox + hw])
        gold.append(g)
        d = gauss_separable(g.astype(F), k5)
        d = saturate_u8(d)[::scale, ::scale].astype(F)
        d = d + rng.normal(0.0, 10.0, d.shape).astype(F)
        d = saturate_u8(d)
        d[rng.integers(0, 500, d.shape) < 1] = 255
        low.append(d)
    return gold, low, offs


def analytic_motions(offs, shape, scale: int):
    """forward[i] = flow of frame i -> i + 1, backward[i] = flow of frame i -> i - 1, in low-res pixels: a scene point at p in frame
    a lies at p + (o_a - o_b) in frame b."""
    n = len(offs)
    plane = lambda v: np.full(shape, v, F)
    fwd = [(plane((offs[i][0] - offs[i + 1][0]) / scale), plane((offs[i][1] - offs[i + 1][1]) / scale)) if i < n - 1 else None
           for i in range(n)]
    bwd = [(plane((offs[i][0] - offs[i - 1][0]) / scale), plane((offs[i][1] - offs[i - 1][1]) / scale)) if i > 0 else None
           for i in range(n)]
    return fwd, bwd
