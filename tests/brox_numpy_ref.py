"""cv::cuda::BroxOpticalFlow restated in NumPy binary32, operation by operation: the yardstick of the GPU tests (the GPU machine has no
reference tree).  It is itself pinned, bit for bit, on tests/golden/brox_ref*.npz, which tools/make_golden_brox.py records from the
reference's own kernels run on the host (tests/test_brox_ref.py).

Two reads of the reference are DEFINITIONS, not measurements of NVIDIA hardware, because its source does not define them (the header
of oracle/pyrlk_ref.c is the precedent; DESIGN.md 4.13 states them too):

  * the nine normalised, linearly filtered, mirror-addressed texture reads of prepare_sor_stage_1_tex (NCVBroxOpticalFlow.cu:372-379)
    follow the CUDA programming guide's rule as oracle/refshim/cudashim/opencv2/cudev/ptr2d/texture.hpp states it, extended to
    normalised coordinates and the mirror: xb = xn * W - 0.5f, i = floor(xb), a = floor((xb - i) * 256 + 0.5) / 256 (1.8 fixed point),
    the same in y; taps i, i + 1, j, j + 1 each mapped by m = k mod 2N, m < N ? m : 2N - 1 - m; value
    (1-a)(1-b) T00 + a(1-b) T10 + (1-a)b T01 + ab T11 in that order, every operation rounded to binary32.  The normalised
    point-filtered read of resizeBicubic (NPP_staging.cu:2226) is texel floor(xn * W) with the same mirror.
  * rsqrtf(x) (NCVBroxOpticalFlow.cu:385) is 1.0f / sqrtf(x), both correctly rounded; the device intrinsic is within 2 ulp of that.

Everything else is the reference's text: NCVBroxOpticalFlow.cu (cited as B:line) and NPP_staging.cu (N:line) of modules/cudalegacy/src/cuda.
No FMA contraction anywhere: the yardstick is the kernels compiled with -ffp-contract=off.
"""
import numpy as np

F = np.float32
EPS2 = F(1e-6)      # B:78
OMEGA = F(1.99)     # B:914
DEFAULTS = dict(alpha=0.197, gamma=50.0, scale_factor=0.8, inner_iterations=5, outer_iterations=150, solver_iterations=10)   # cudaoptflow.hpp:179-185
SUPERRES = dict(alpha=0.197, gamma=50.0, scale_factor=0.8, inner_iterations=10, outer_iterations=77, solver_iterations=10)   # superres/src/optical_flow.cpp:542
IMAGE_NAMES = ("I0", "I1", "Ix", "Ixx", "Ix0", "Iy", "Iyy", "Iy0", "Ixy")                       # B:340
COEFF_NAMES = ("diffusivity_x", "diffusivity_y", "inv_denominator_u", "inv_denominator_v", "numerator_dudv", "numerator_u", "numerator_v")
DERIV_NAMES = ("Ix0", "Iy0", "Ix", "Iy", "Ixx", "Iyy", "Ixy")                                   # B:842-868, in the order computed


def synth_pair(rows, cols, seed):
    """two frames in [0, 1]: box-smoothed noise, and the same texture moved by a fraction of a pixel (sums and constant weights: no libm)"""
    big = np.random.RandomState(seed).rand(rows + 8, cols + 8)
    k = np.zeros_like(big)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            k += np.roll(np.roll(big, dy, 0), dx, 1)
    k /= 9.0
    a = k[4:4 + rows, 4:4 + cols]
    b = 0.5 * k[4:4 + rows, 4:4 + cols] + 0.3 * k[4:4 + rows, 3:3 + cols] + 0.2 * k[5:5 + rows, 4:4 + cols]
    return np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)


def synth_plane(rows, cols, seed, lo=-1.0, hi=1.0):
    return np.ascontiguousarray(lo + (hi - lo) * np.random.RandomState(seed).rand(rows, cols), F)


def level_sizes(w, h, scale_factor, outer_iterations):
    """B:698-785 -> [(w, h)], level 0 first"""
    sf = F(scale_factor)
    out = [(w, h)]
    scale = F(1.0) * sf
    pw, ph = w, h
    while pw > 15 and ph > 15 and len(out) < outer_iterations:
        lw, lh = int(np.ceil(F(w) * scale)), int(np.ceil(F(h) * scale))
        out.append((lw, lh))
        scale = scale * sf
        pw, ph = lw, lh
    return out


def _line_ranges(n_dst, n_src, scale):
    x = scale * np.arange(n_dst, dtype=F)
    b = np.maximum(x - scale, F(0))
    e = np.minimum(x + scale, F(n_src) - F(1))
    fb, ce = np.floor(b), np.ceil(e)
    return b, e, fb, ce, fb.astype(np.int64), ce.astype(np.int64)


def resize_down(src, dw, dh, scale_factor):
    """resizeSuperSample_32f, N:2073-2149, as nppiStResize_32f_C1R launches it (N:2265): scale = 1 / scale_factor"""
    sh, sw = src.shape
    scale = F(1.0) / F(scale_factor)
    xb, xe, fxb, cxe, ib, ie = _line_ranges(dw, sw, scale)
    yb, ye, fyb, cye, jb, je = _line_ranges(dh, sh, scale)
    # processLine for every source row and every destination column
    w0 = F(1.0) - xb + fxb
    wsum = np.broadcast_to(w0, (sh, dw)).copy()
    s = src[:, ib] * w0
    for n in range(1, int((ie - ib).max()) + 1):
        m = ib + n < ie
        idx = np.where(m, ib + n, 0)
        s = np.where(m, s + src[:, idx], s)
        wsum = np.where(m, wsum + F(1.0), wsum)
    last = np.maximum(ie, ib + 1)
    s = s + src[:, last] * (cxe - xe)
    wsum = wsum + (cxe - xe)
    line = s / wsum
    # the rows
    w0 = (F(1.0) - yb + fyb)[:, None]
    wsum = np.broadcast_to(w0, (dh, dw)).copy()
    s = line[jb] * w0
    for n in range(1, int((je - jb).max()) + 1):
        m = (jb + n < je)[:, None]
        idx = np.where(m[:, 0], jb + n, 0)
        s = np.where(m, s + line[idx], s)
        wsum = np.where(m, wsum + F(1.0), wsum)
    last = np.maximum(je, jb + 1)
    s = s + line[last] * (cye - ye)[:, None]
    wsum = wsum + (cye - ye)[:, None]
    return (s / wsum).astype(F)


def mirror_periodic(k, n):
    m = np.mod(k, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def _bicubic_coeff(x_):
    x = np.abs(x_)
    a = x * x * (F(1.5) * x - F(2.5)) + F(1.0)
    b = x * (x * (F(-0.5) * x + F(2.5)) - F(4.0)) + F(2.0)
    return np.where(x <= F(1.0), a, np.where(x < F(2.0), b, F(0.0))).astype(F)


def resize_up(src, dw, dh, scale_factor):
    """resizeBicubic, N:2152-2231, launched with 1 / (1 / scale_factor) (B:952-953, N:2272), then ScaleVector by 1 / scale_factor (B:955)"""
    sh, sw = src.shape
    x_factor = F(1.0) / F(scale_factor)
    scale = F(1.0) / x_factor
    mul = F(1.0) / F(scale_factor)
    dx, dy = F(1.0) / F(sw), F(1.0) / F(sh)
    rw, rh = F(sw), F(sh)
    x = (scale * np.arange(dw, dtype=F))[None, :]
    y = (scale * np.arange(dh, dtype=F))[:, None]
    xmin, xmax = np.maximum(np.ceil(x - F(2.0)), F(0.0)), np.minimum(np.floor(x + F(2.0)), rw - F(1.0))
    ymin, ymax = np.maximum(np.ceil(y - F(2.0)), F(0.0)), np.minimum(np.floor(y + F(2.0)), rh - F(1.0))
    x, y = x + F(0.5), y + F(0.5)
    xmin, xmax, ymin, ymax = xmin + F(0.5), xmax + F(0.5), ymin + F(0.5), ymax + F(0.5)
    s = np.zeros((dh, dw), F)
    wsum = np.zeros((dh, dw), F)
    for ny in range(5):
        cy = ymin + F(ny)
        wy = _bicubic_coeff(y - cy)
        ty = mirror_periodic(np.floor(cy * dy * rh).astype(np.int64), sh)
        for nx in range(5):
            cx = xmin + F(nx)
            m = (cy <= ymax) & (cx <= xmax)
            wx = _bicubic_coeff(x - cx) * wy
            tx = mirror_periodic(np.floor(cx * dx * rw).astype(np.int64), sw)
            t = src[np.broadcast_to(ty, (dh, dw)), np.broadcast_to(tx, (dh, dw))]
            s = np.where(m, s + wx * t, s)
            wsum = np.where(m, wsum + wx, wsum)
    with np.errstate(all="ignore"):
        r = np.where(wsum == 0, F(0.0), s / wsum)
    return (r * mul).astype(F)


TAPS = (F(1.0), F(-8.0), F(0.0), F(8.0), F(-1.0))   # B:689


def derivative(src, column):
    """FilterRowBorderMirror_32f_C1R / FilterColumnBorderMirror_32f_C1R, N:1433-1501: the mirror is asymmetric (-1 -> 2, -2 -> 3)"""
    n = src.shape[0] if column else src.shape[1]
    c = np.arange(n)
    s = np.zeros(src.shape, F)
    for m in range(5):
        i = c + m - 2
        i = np.where(i < 0, 1 - i, i)
        i = np.where(i >= n, n + n - i - 1, i)
        s = s + (src[i, :] if column else src[:, i]) * TAPS[m]
    return (s * (F(1.0) / F(12.0))).astype(F)


def derivatives(i0, i1):
    """B:842-868 -> dict of the seven planes"""
    d = {"Ix0": derivative(i0, False), "Iy0": derivative(i0, True), "Ix": derivative(i1, False), "Iy": derivative(i1, True)}
    d["Ixx"] = derivative(d["Ix"], False)
    d["Iyy"] = derivative(d["Iy"], True)
    d["Ixy"] = derivative(d["Iy"], False)
    return d


def tex_linear(t, yn, xn):
    """the definition at the head of this file"""
    h, w = t.shape
    xb, yb = xn * F(w) - F(0.5), yn * F(h) - F(0.5)
    fi, fj = np.floor(xb), np.floor(yb)
    a = np.floor((xb - fi) * F(256.0) + F(0.5)) / F(256.0)
    b = np.floor((yb - fj) * F(256.0) + F(0.5)) / F(256.0)
    i, j = fi.astype(np.int64), fj.astype(np.int64)
    i0, i1, j0, j1 = mirror_periodic(i, w), mirror_periodic(i + 1, w), mirror_periodic(j, h), mirror_periodic(j + 1, h)
    one = F(1.0)
    return ((one - a) * (one - b) * t[j0, i0] + a * (one - b) * t[j0, i1] + (one - a) * b * t[j1, i0] + a * b * t[j1, i1]).astype(F)


def _mirror_sym(i, n):
    i = np.maximum(i, -i - 1)      # B:243-246
    return np.minimum(i, n - i + n - 1)


def prepare_stage1(u, v, du, dv, im, alpha, gamma):
    """prepare_sor_stage_1_tex, B:340-406 (diffusivities B:188-227) -> dict of the seven planes before stage 2"""
    h, w = u.shape
    alpha, gamma = F(alpha), F(gamma)
    jj, ii = np.arange(h)[:, None], np.arange(w)[None, :]
    xl, xr, yd, yu = _mirror_sym(ii - 1, w), _mirror_sym(ii + 1, w), _mirror_sym(jj - 1, h), _mirror_sym(jj + 1, h)
    x = (ii.astype(F) + F(0.5)) + np.zeros((h, 1), F)
    y = (jj.astype(F) + F(0.5)) + np.zeros((1, w), F)
    wx, wy = (x + u) / F(w), (y + v) / F(h)
    x, y = x / F(w), y / F(h)
    Iz = tex_linear(im["I1"], wy, wx) - tex_linear(im["I0"], y, x)
    Ix = tex_linear(im["Ix"], wy, wx)
    Ixz = Ix - tex_linear(im["Ix0"], y, x)
    Ixy = tex_linear(im["Ixy"], wy, wx)
    Ixx = tex_linear(im["Ixx"], wy, wx)
    Iy = tex_linear(im["Iy"], wy, wx)
    Iyz = Iy - tex_linear(im["Iy0"], y, x)
    Iyy = tex_linear(im["Iyy"], wy, wx)
    q0 = Iz + Ix * du + Iy * dv
    q1 = Ixz + Ixx * du + Ixy * dv
    q2 = Iyz + Ixy * du + Iyy * dv
    data = F(0.5) * (F(1.0) / np.sqrt(q0 * q0 + gamma * (q1 * q1 + q2 * q2) + EPS2))
    data = data / alpha
    g = lambda p, yy, xx: p[np.broadcast_to(yy, (h, w)), np.broadcast_to(xx, (h, w))]
    # diffusivity_along_x, B:188-202
    u_x = u + du - g(u, jj, xl) - g(du, jj, xl)
    v_x = v + dv - g(v, jj, xl) - g(dv, jj, xl)
    u_y = F(0.25) * (g(u, yu, ii) + g(du, yu, ii) + g(u, yu, xl) + g(du, yu, xl) - g(u, yd, ii) - g(du, yd, ii) - g(u, yd, xl) - g(du, yd, xl))
    v_y = F(0.25) * (g(v, yu, ii) + g(dv, yu, ii) + g(v, yu, xl) + g(dv, yu, xl) - g(v, yd, ii) - g(dv, yd, ii) - g(v, yd, xl) - g(dv, yd, xl))
    sx = F(0.5) / np.sqrt(u_x * u_x + v_x * v_x + u_y * u_y + v_y * v_y + EPS2)
    # diffusivity_along_y, B:213-227
    u_y = u + du - g(u, yd, ii) - g(du, yd, ii)
    v_y = v + dv - g(v, yd, ii) - g(dv, yd, ii)
    u_x = F(0.25) * (g(u, jj, xr) + g(u, yd, xr) + g(du, jj, xr) + g(du, yd, xr) - g(u, jj, xl) - g(u, yd, xl) - g(du, jj, xl) - g(du, yd, xl))
    v_x = F(0.25) * (g(v, jj, xr) + g(v, yd, xr) + g(dv, jj, xr) + g(dv, yd, xr) - g(v, jj, xl) - g(v, yd, xl) - g(dv, jj, xl) - g(dv, yd, xl))
    sy = F(0.5) / np.sqrt(u_x * u_x + v_x * v_x + u_y * u_y + v_y * v_y + EPS2)
    sx = sx.copy(); sy = sy.copy()
    sx[:, 0] = 0
    sy[0, :] = 0
    out = {"numerator_dudv": data * (Ix * Iy + gamma * Ixy * (Ixx + Iyy)),
           "numerator_u": data * (Ix * Iz + gamma * (Ixx * Ixz + Ixy * Iyz)),
           "numerator_v": data * (Iy * Iz + gamma * (Iyy * Iyz + Ixy * Ixz)),
           "denominator_u": data * (Ix * Ix + gamma * (Ixy * Ixy + Ixx * Ixx)),
           "denominator_v": data * (Iy * Iy + gamma * (Ixy * Ixy + Iyy * Iyy)),
           "diffusivity_x": sx, "diffusivity_y": sy}
    return {k: np.ascontiguousarray(a, F) for k, a in out.items()}


def prepare_stage2(c):
    """prepare_sor_stage_2, B:416-473: the denominators become their inverses"""
    sx, sy = c["diffusivity_x"], c["diffusivity_y"]
    sx_r = np.zeros_like(sx); sx_r[:, :-1] = sx[:, 1:]
    sy_u = np.zeros_like(sy); sy_u[:-1, :] = sy[1:, :]
    dsum = sx + sx_r + sy + sy_u
    out = {k: c[k] for k in ("diffusivity_x", "diffusivity_y", "numerator_dudv", "numerator_u", "numerator_v")}
    out["inv_denominator_u"] = (F(1.0) / (c["denominator_u"] + dsum)).astype(F)
    out["inv_denominator_v"] = (F(1.0) / (c["denominator_v"] + dsum)).astype(F)
    return out


def prepare(u, v, du, dv, im, alpha, gamma):
    return prepare_stage2(prepare_stage1(u, v, du, dv, im, alpha, gamma))


def sor_pass(colour, u, v, du, dv, c):
    """sor_pass<colour>, B:479-554 -> (new_du, new_dv)"""
    h, w = u.shape
    jj, ii = np.arange(h)[:, None], np.arange(w)[None, :]
    ir, il = np.minimum(ii + 1, w - 1), np.maximum(ii - 1, 0)
    ju, jd = np.minimum(jj + 1, h - 1), np.maximum(jj - 1, 0)
    g = lambda p, yy, xx: p[np.broadcast_to(yy, (h, w)), np.broadcast_to(xx, (h, w))]
    sx, sy = c["diffusivity_x"], c["diffusivity_y"]
    s_left, s_down = sx, sy
    s_right = np.where(ii < w - 1, g(sx, jj, ir), F(0.0)).astype(F)
    s_up = np.where(jj < h - 1, g(sy, ju, ii), F(0.0)).astype(F)
    ssum = s_left + s_right + s_up + s_down
    ndudv = c["numerator_dudv"]
    num_u = (s_left * (g(u, jj, il) + g(du, jj, il)) + s_up * (g(u, ju, ii) + g(du, ju, ii)) + s_right * (g(u, jj, ir) + g(du, jj, ir))
             + s_down * (g(u, jd, ii) + g(du, jd, ii)) - u * ssum - c["numerator_u"] - ndudv * dv)
    ndu = (F(1.0) - OMEGA) * du + OMEGA * c["inv_denominator_u"] * num_u
    num_v = (s_left * (g(v, jj, il) + g(dv, jj, il)) + s_up * (g(v, ju, ii) + g(dv, ju, ii)) + s_right * (g(v, jj, ir) + g(dv, jj, ir))
             + s_down * (g(v, jd, ii) + g(dv, jd, ii)) - v * ssum - c["numerator_v"] - ndudv * ndu)
    ndv = (F(1.0) - OMEGA) * dv + OMEGA * c["inv_denominator_v"] * num_v
    m = (ii + jj) % 2 == colour
    return np.where(m, ndu, du).astype(F), np.where(m, ndv, dv).astype(F)


def sor(u, v, du, dv, c, solver_iterations):
    """the solver loop, B:912-925"""
    for _ in range(solver_iterations):
        du2, dv2 = sor_pass(0, u, v, du, dv, c)
        du, dv = sor_pass(1, u, v, du2, dv2, c)
    return du, dv


def calc(i0, i1, alpha=0.197, gamma=50.0, scale_factor=0.8, inner_iterations=5, outer_iterations=150, solver_iterations=10):
    """NCVBroxOpticalFlow, B:598-985 -> (flow rows x cols x 2, level sizes)"""
    h, w = i0.shape
    sizes = level_sizes(w, h, scale_factor, outer_iterations)
    pyr = [(i0, i1)]
    if min(min(s) for s in sizes) < 2:   # the derivative filter's mirror leaves a level with a side of 1 (and NumPy would wrap round silently)
        raise ValueError("scale_factor gives a pyramid level with a side of 1")
    for lw, lh in sizes[1:]:
        a, b = pyr[-1]
        pyr.append((resize_down(a, lw, lh, scale_factor), resize_down(b, lw, lh, scale_factor)))
    lw, lh = sizes[-1]
    u, v = np.zeros((lh, lw), F), np.zeros((lh, lw), F)
    for l in range(len(sizes) - 1, -1, -1):
        a, b = pyr[l]
        du, dv = np.zeros_like(u), np.zeros_like(u)
        im = derivatives(a, b)
        im["I0"], im["I1"] = a, b
        for _ in range(inner_iterations):
            c = prepare(u, v, du, dv, im, alpha, gamma)
            du, dv = sor(u, v, du, dv, c, solver_iterations)
        u, v = u + du, v + dv                                   # B:929-931
        if l > 0:
            nw, nh = sizes[l - 1]
            u, v = resize_up(u, nw, nh, scale_factor), resize_up(v, nw, nh, scale_factor)
    return np.ascontiguousarray(np.stack([u, v], axis=2), F), sizes
