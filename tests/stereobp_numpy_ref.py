"""NumPy restatement of cv::cuda::StereoBeliefPropagation: modules/cudastereo/src/stereobp.cpp (host class) over
modules/cudastereo/src/cuda/stereobp.cu (kernels).  The yardstick of the HIP class; pinned itself on tests/golden/stereobp_ref*.npz,
which the reference's own code wrote (tools/make_golden_stereobp.py).

Vectorised over pixels, loops over disparities.  Every operation is a separately rounded f32 one in the reference's order; for
16-bit messages every store through short is applied where the reference stores.  Planar volumes are arrays (ndisp, rows, cols) of the
message type: element [k, y, x] is row k * rows + y, column x of the reference's matrix (`planar` / `unplanar` convert).
"""
import math

import numpy as np

F = np.float32
CV_16S, CV_32F = 3, 5
FLT_MAX = np.finfo(np.float32).max
DEFAULTS = dict(max_data_term=10.0, data_weight=0.07, max_disc_term=1.7, disc_single_jump=1.0)   # stereobp.cpp:147-150


def msg_dtype(msg_type):
    return np.float32 if msg_type == CV_32F else np.int16


def planar(vol):
    """(ndisp, rows, cols) -> the reference's (ndisp * rows, cols) matrix"""
    return np.ascontiguousarray(vol).reshape(-1, vol.shape[2])


def unplanar(mat, ndisp):
    return mat.reshape(ndisp, mat.shape[0] // ndisp, mat.shape[1])


def sat(dtype, v):
    """saturate_cast<T>(float): short = round to nearest even, clamp; float = the value"""
    v = np.asarray(v, F)
    if dtype == np.float32:
        return v
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def consts(ndisp, msg_type, max_data_term=10.0, data_weight=0.07, max_disc_term=1.7, disc_single_jump=1.0):
    """what init() hands load_constants, stereobp.cpp:176,271: the members are floats (:111-121), the products f32"""
    scale = F(1.0) if msg_type == CV_32F else F(10.0)
    return dict(ndisp=int(ndisp), max_data_term=F(max_data_term), data_weight=scale * F(data_weight),
                max_disc_term=scale * F(max_disc_term), disc_single_jump=scale * F(disc_single_jump))


def check_params(ndisp, iters, levels, msg_type, max_data_term=10.0, left=None, right=None, data=None):
    """The CV_Asserts of compute(left, right) stereobp.cpp:178-195 and compute(data) :210-225, in their order; ValueError carries the
    asserted condition.  Returns (rows, cols)."""
    if not (0 < ndisp and 0 < iters and 0 < levels):
        raise ValueError("0 < ndisp_ && 0 < iters_ && 0 < levels_")
    if msg_type not in (CV_32F, CV_16S):
        raise ValueError("msg_type_ == CV_32F || msg_type_ == CV_16S")
    if msg_type == CV_16S and not (levels <= 31 and F(1 << (levels - 1)) * F(10.0) * F(max_data_term) < F(32767)):
        raise ValueError("msg_type_ == CV_32F || (1 << (levels_ - 1)) * scale_ * max_data_term_ < std::numeric_limits<short>::max()")
    if data is not None:
        if not (data.dtype == msg_dtype(msg_type) and data.ndim == 2 and data.shape[0] % ndisp == 0):
            raise ValueError("(data.type() == msg_type_) && (data.rows % ndisp_ == 0)")
        rows, cols = data.shape[0] // ndisp, data.shape[1]
    else:
        cn = 1 if left.ndim == 2 else left.shape[2]
        if not (left.dtype == np.uint8 and cn in (1, 3, 4)):
            raise ValueError("left.type() == CV_8UC1 || left.type() == CV_8UC3 || left.type() == CV_8UC4")
        if not (left.shape == right.shape and left.dtype == right.dtype):
            raise ValueError("left.size() == right.size() && left.type() == right.type()")
        rows, cols = left.shape[:2]
    lowest = 0 if levels - 1 >= 31 else min(cols, rows) >> (levels - 1)   # cols / (int) pow(2.f, levels - 1)
    if not lowest > 2:
        raise ValueError("std::min(lowest_cols, lowest_rows) > min_image_dim_size")
    return rows, cols


def comp_data(left, right, c, msg_type, data=None):
    """comp_data<cn, D>, stereobp.cu:76-161.  Writes interior pixels of `data` (made of zeros when not given) and returns it."""
    T = msg_dtype(msg_type)
    rows, cols = left.shape[:2]
    nd = c["ndisp"]
    if data is None:
        data = np.zeros((nd, rows, cols), T)
    if rows < 3 or cols < 3:
        return data
    L = left.reshape(rows, cols, -1).astype(np.int32)
    R = right.reshape(rows, cols, -1).astype(np.int32)
    cn = L.shape[2]
    w, cap = c["data_weight"], c["data_weight"] * c["max_data_term"]
    xs = np.arange(1, cols - 1)
    for disp in range(nd):
        ok = xs - disp >= 1                                   # :149
        xr = np.where(ok, xs - disp, xs)
        diff = np.abs(L[1:-1, 1:-1] - R[1:-1][:, xr]).astype(F)   # PixDiff :76-130
        if cn == 1:
            val = diff[..., 0]
        else:
            val = F(0.114) * diff[..., 0]
            val = val + F(0.587) * diff[..., 1]
            val = val + F(0.299) * diff[..., 2]
        v = np.where(ok[None, :], np.minimum(w * val, cap), cap).astype(F)   # :153 / :157
        data[disp, 1:-1, 1:-1] = sat(T, v)
    return data


def data_step_down(src):
    """data_step_down<T>, stereobp.cu:257-280: ((y0x0 + y1x0) + y0x1) + y1x1, right / bottom index clamped"""
    nd, srows, scols = src.shape
    drows, dcols = (srows + 1) // 2, (scols + 1) // 2
    y0, x0 = 2 * np.arange(drows), 2 * np.arange(dcols)
    y1, x1 = np.minimum(y0 + 1, srows - 1), np.minimum(x0 + 1, scols - 1)
    s = src.astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        v = s[:, y0][:, :, x0]
        v = v + s[:, y1][:, :, x0]
        v = v + s[:, y0][:, :, x1]
        v = v + s[:, y1][:, :, x1]
        return _sat_any(src.dtype, v)


def _sat_any(dtype, v):
    """sat() that tolerates NaN / inf in elements no result depends on (poisoned borders)"""
    if dtype == np.float32:
        return v.astype(F)
    with np.errstate(invalid="ignore"):
        return np.clip(np.rint(np.nan_to_num(v, nan=0.0, posinf=32767, neginf=-32768)), -32768, 32767).astype(np.int16)


def level_up(src, rows, cols):
    """level_up_message<T>, stereobp.cu:305-322: every pixel of the finer level, borders included, from (y / 2, x / 2)"""
    return src[:, np.arange(rows) // 2][:, :, np.arange(cols) // 2].copy()


def message(m1, m2, m3, data, c, T):
    """message(), stereobp.cu:389-426 with calc_min_linear_penalty :358-387.  Arguments (ndisp, n) of T; returns dst (ndisp, n) of T."""
    nd = c["ndisp"]
    jump, disc = c["disc_single_jump"], c["max_disc_term"]
    short = T == np.int16
    thru = (lambda v: sat(T, v).astype(F)) if short else (lambda v: v)
    with np.errstate(invalid="ignore", over="ignore"):
        s = m1.astype(F) + m2.astype(F)
        s = s + m3.astype(F)
        s = s + data.astype(F)
        minimum = np.full(s.shape[1], FLT_MAX, F)
        for i in range(nd):
            minimum = np.where(s[i] < minimum, s[i], minimum)   # of the unstored sums :401
        dst = thru(s)                                            # :404
        prev = dst[0].copy()
        for i in range(1, nd):                                   # :363-373
            prev = prev + jump
            cur = dst[i]
            rep = prev < cur
            dst[i] = np.where(rep, thru(prev), cur)
            prev = np.where(rep, prev, cur)
        prev = dst[nd - 1].copy()
        for i in range(nd - 2, -1, -1):                          # :375-386
            prev = prev + jump
            cur = dst[i]
            rep = prev < cur
            dst[i] = np.where(rep, thru(prev), cur)
            prev = np.where(rep, prev, cur)
        minimum = minimum + disc                                 # :409
        total = np.zeros(s.shape[1], F)
        for i in range(nd):                                      # :411-421
            v = dst[i]
            rep = v > minimum
            dst[i] = np.where(rep, thru(minimum), v)
            total = total + np.where(rep, minimum, v)
        total = total / F(nd)                                    # :422
        out = dst - total[None, :]                               # :425
        if not short:
            return out.astype(F)
        # short -= float: the difference converts to short by truncation toward zero (through int, wrapping)
        return np.trunc(np.nan_to_num(out)).astype(np.int64).astype(np.int32).astype(np.int16)


def one_iteration(u, d, l, r, data, t, c):
    """one_iteration<T>, stereobp.cu:429-450, in place: pixels x = 2 i + ((y + t) & 1), interior only; u, d, r, l in that order"""
    T = u.dtype.type
    nd, rows, cols = u.shape
    ys, xs = np.meshgrid(np.arange(1, rows - 1), np.arange(1, cols - 1), indexing="ij")
    sel = (xs & 1) == ((ys + t) & 1)
    ys, xs = ys[sel], xs[sel]
    if ys.size == 0:
        return
    dt = data[:, ys, xs]
    u[:, ys, xs] = message(u[:, ys + 1, xs], l[:, ys, xs + 1], r[:, ys, xs - 1], dt, c, T)   # :445
    d[:, ys, xs] = message(d[:, ys - 1, xs], l[:, ys, xs + 1], r[:, ys, xs - 1], dt, c, T)   # :446
    r[:, ys, xs] = message(u[:, ys + 1, xs], d[:, ys - 1, xs], r[:, ys, xs - 1], dt, c, T)   # :447
    l[:, ys, xs] = message(u[:, ys + 1, xs], d[:, ys - 1, xs], l[:, ys, xs + 1], dt, c, T)   # :448


def calc_all_iterations(u, d, l, r, data, iters, c, t0=0):
    """calc_all_iterations_gpu, stereobp.cu:452-472 (t0: the first parity; the reference starts every level at 0)"""
    for t in range(t0, t0 + iters):
        one_iteration(u, d, l, r, data, t, c)


def output(u, d, l, r, data, out_dtype=np.int16):
    """output<T>, stereobp.cu:481-517, into a zeroed map (stereobp.cpp:353) and convertTo's saturate_cast (:357-358)"""
    nd, rows, cols = u.shape
    disp = np.zeros((rows, cols), np.int16)
    if rows >= 3 and cols >= 3:
        best = np.zeros((rows - 2, cols - 2), np.int32)
        best_val = np.full((rows - 2, cols - 2), FLT_MAX, F)
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(nd):
                v = u[k, 2:, 1:-1].astype(F) + d[k, :-2, 1:-1].astype(F)
                v = v + l[k, 1:-1, 2:].astype(F)
                v = v + r[k, 1:-1, :-2].astype(F)
                v = v + data[k, 1:-1, 1:-1].astype(F)
                win = v < best_val                        # the first strict minimum wins :508
                best_val = np.where(win, v, best_val)
                best = np.where(win, k, best)
        disp[1:-1, 1:-1] = np.minimum(best, 32767).astype(np.int16)
    if out_dtype == np.uint8:
        return np.clip(disp, 0, 255).astype(np.uint8)
    return disp.astype(out_dtype)


def level_sizes(rows, cols, levels):
    sizes = [(rows, cols)]
    for _ in range(1, levels):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))   # stereobp.cpp:316-317
    return sizes


def _level_view(buf, nd, rows, cols):
    """the level's planes inside a message buffer of a larger size: plane k at row k * rows, the buffer's own step"""
    return buf[:nd * rows].reshape(nd, rows, buf.shape[1])[:, :, :cols]


def calc_bp(data0, iters, levels, c, out_dtype=np.int16, msg_fill=None, trace=None):
    """init + calcBP, stereobp.cpp:234-359, on the level-0 cost volume (ndisp, rows, cols).  The messages live in the reference's two
    alternating buffer sets (full size and half size).  msg_fill None: the set of the coarsest level is zeroed as a whole (:243-268)
    and the other starts from zeros as well; otherwise both sets start filled with msg_fill (NaN, say) and ONLY the planes of the
    coarsest level are zeroed -- which gives the same map if every element that is read has been written."""
    nd, rows, cols = data0.shape
    T = data0.dtype
    sizes = level_sizes(rows, cols, levels)
    datas = [data0]
    for i in range(1, levels):
        datas.append(data_step_down(datas[-1]))
    shapes = [(nd * rows, cols), (nd * ((rows + 1) // 2), (cols + 1) // 2)]
    sets = []
    for s in range(2):
        if msg_fill is None:
            sets.append([np.zeros(shapes[s], T) for _ in range(4)])
        else:
            sets.append([np.full(shapes[s], msg_fill, T) for _ in range(4)])
    mem_idx = 0 if levels & 1 else 1                                   # :329
    if msg_fill is not None:
        for m in sets[mem_idx]:
            _level_view(m, nd, *sizes[levels - 1])[...] = 0
    for i in range(levels - 1, -1, -1):                               # :331-340
        lr, lc = sizes[i]
        cur = [_level_view(m, nd, lr, lc) for m in sets[mem_idx]]
        if i != levels - 1:
            src = [_level_view(m, nd, *sizes[i + 1]) for m in sets[(mem_idx + 1) & 1]]
            for k in range(4):
                cur[k][...] = level_up(src[k], lr, lc)
        calc_all_iterations(cur[0], cur[1], cur[2], cur[3], datas[i], iters, c)
        if trace is not None:
            trace.append([m.copy() for m in cur])
        mem_idx = (mem_idx + 1) & 1
    top = [_level_view(m, nd, rows, cols) for m in sets[0]]           # u_, d_, l_, r_ :355
    return output(top[0], top[1], top[2], top[3], datas[0], out_dtype)


def compute(left, right, ndisp=64, iters=5, levels=5, msg_type=CV_32F, out_dtype=np.int16, border_fill=None, msg_fill=None, **weights):
    """compute(left, right, disparity), stereobp.cpp:165-204.  border_fill: what the never-written border elements of the level-0
    data hold (zeros when None)."""
    w = dict(DEFAULTS, **weights)
    check_params(ndisp, iters, levels, msg_type, w["max_data_term"], left=left, right=right)
    c = consts(ndisp, msg_type, **w)
    T = msg_dtype(msg_type)
    rows, cols = left.shape[:2]
    data = np.zeros((ndisp, rows, cols), T) if border_fill is None else np.full((ndisp, rows, cols), border_fill, T)
    comp_data(left, right, c, msg_type, data)
    return calc_bp(data, iters, levels, c, out_dtype, msg_fill)


def compute_data(data, ndisp=64, iters=5, levels=5, msg_type=CV_32F, out_dtype=np.int16, **weights):
    """compute(data, disparity, stream), stereobp.cpp:206-232; data: the (ndisp * rows, cols) matrix"""
    w = dict(DEFAULTS, **weights)
    check_params(ndisp, iters, levels, msg_type, w["max_data_term"], data=data)
    c = consts(ndisp, msg_type, **w)
    return calc_bp(unplanar(data, ndisp).copy(), iters, levels, c, out_dtype)


def estimate_recommended_params(width, height):
    """estimateRecommendedParams, stereobp.cpp:367-378 -> (ndisp, iters, levels)"""
    ndisp = width // 4
    if ndisp & 1:
        ndisp += 1
    mm = max(width, height)
    iters = mm // 100 + 2
    levels = int(math.log(float(mm)) + 1) * 4 // 5
    if levels == 0:
        levels += 1
    return ndisp, iters, levels
