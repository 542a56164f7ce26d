"""NumPy restatement of cv::cuda::StereoConstantSpaceBP: modules/cudastereo/src/stereocsbp.cpp (host class) over
modules/cudastereo/src/cuda/stereocsbp.cu (kernels).  The yardstick of the HIP class; pinned itself on tests/golden/stereocsbp_ref*.npz,
which the reference's own code wrote (tools/make_golden_stereocsbp.py).

Vectorised over pixels, loops over planes.  Every operation is a separately rounded f32 one in the reference's order; 16-bit messages are
summed in int and wrap when narrowed, and every store through short is applied where the reference stores.  A planar matrix is the
reference's: (planes * h, cols) of the message type, plane k of pixel (y, x) of an h x w level at row k * h + y.  The class keeps the
reference's buffers ((rows * nr_plane) x cols each, zero-initialised): at a level with an odd number of rows or columns the reference
reads one row / column past the parent level, which lands in the next plane or in what lies behind the level's planes, and these
buffers make that read what it reads there.
"""
import math

import numpy as np

F = np.float32
CV_16S, CV_32F = 3, 5
FLT_MAX = np.finfo(np.float32).max
DEFAULTS = dict(max_data_term=30.0, data_weight=1.0, max_disc_term=160.0, disc_single_jump=10.0, min_disp=0, local=True)   # stereocsbp.cpp:132-143


def msg_dtype(msg_type):
    return np.float32 if msg_type == CV_32F else np.int16


def t_max(dtype):
    return FLT_MAX if dtype == np.float32 else np.int16(32767)


def sat(dtype, v):
    """saturate_cast<T>(float): short = round to nearest even, clamp; float = the value"""
    v = np.asarray(v, F)
    if dtype == np.float32:
        return v
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def tsum(dtype, *terms):
    """T v = a + b + ...: f32 adds left to right; shorts are promoted to int and the sum wraps when it is narrowed to short"""
    if dtype == np.float32:
        acc = terms[0].astype(F)
        for t in terms[1:]:
            acc = acc + t
        return acc
    acc = terms[0].astype(np.int32)
    for t in terms[1:]:
        acc = acc + t.astype(np.int32)
    return acc.astype(np.int16)


def clamp_levels(ndisp, levels):
    """stereocsbp.cpp:171"""
    return min(levels, int(math.log(float(ndisp)) / math.log(2.0)))


def check_params(ndisp, iters, levels, nr_plane, msg_type, left=None, right=None):
    """The CV_Asserts of compute, stereocsbp.cpp:154-161, in their order, then the clamp of :171; ValueError carries the asserted
    condition.  Returns the clamped level count.  What is undefined in the reference after the clamp is rejected."""
    if msg_type not in (CV_32F, CV_16S):
        raise ValueError("msg_type_ == CV_32F || msg_type_ == CV_16S")
    if not (0 < ndisp and 0 < iters and 0 < levels and 0 < nr_plane and levels <= 8):
        raise ValueError("0 < ndisp_ && 0 < iters_ && 0 < levels_ && 0 < nr_plane_ && levels_ <= 8")
    if left is not None:
        if not (left.dtype == np.uint8 and (left.ndim == 2 or (left.ndim == 3 and left.shape[2] in (1, 3, 4)))):
            raise ValueError("left.type() == CV_8UC1 || left.type() == CV_8UC3 || left.type() == CV_8UC4")
        if not (left.shape == right.shape and left.dtype == right.dtype):
            raise ValueError("left.size() == right.size() && left.type() == right.type()")
    levels = clamp_levels(ndisp, levels)
    if levels < 1:
        raise ValueError("ndisp == 1: levels_ = min(levels_, int(log(ndisp_) / log(2.0))) is 0, which is undefined in the reference")
    if left is not None and ((left.shape[0] >> (levels - 1)) < 1 or (left.shape[1] >> (levels - 1)) < 1):
        raise ValueError("the coarsest level is empty: an empty launch, which is undefined in the reference")
    return levels


def estimate_recommended_params(width, height):
    """StereoConstantSpaceBP::estimateRecommendedParams, stereocsbp.cpp:342-355 -> (ndisp, iters, levels, nr_plane)"""
    ndisp = int(F(width) / F(3.14))
    if ndisp & 1:
        ndisp += 1
    mm = max(width, height)
    iters = mm // 100 + (-4 if mm > 1200 else 4)
    levels = int(math.log(float(mm))) * 2 // 3
    if levels == 0:
        levels += 1
    nr_plane = int(float(F(ndisp)) / math.pow(2.0, levels + 1))
    return ndisp, iters, levels, nr_plane


def level_sizes(rows, cols, nr_plane, levels):
    """stereocsbp.cpp:179-188 -> [(rows, cols, planes)] per level"""
    out = [(rows, cols, nr_plane)]
    for _ in range(1, levels):
        r, c, n = out[-1]
        out.append((r // 2, c // 2, n * 2))
    return out


def synth_pair(rows, cols, cn, seed):
    """A stereo pair from integer arithmetic alone (the same on every NumPy): a smoothed hash texture, the right image the left one
    shifted by 1 .. 4 px by region plus a little hash noise.  Fixtures of large images record (rows, cols, cn, seed) instead of pixels."""
    def h(y, x, c, s):
        v = (y.astype(np.uint64) * np.uint64(7919) + x.astype(np.uint64) * np.uint64(104729) + np.uint64(c * 1299709 + s * 15485863 + 12345))
        v = (v ^ (v >> np.uint64(13))) * np.uint64(2654435761) & np.uint64(0xFFFFFFFF)
        v = (v ^ (v >> np.uint64(16))) * np.uint64(2246822519) & np.uint64(0xFFFFFFFF)
        return ((v >> np.uint64(11)) & np.uint64(255)).astype(np.int64)
    y, x = np.mgrid[0:rows, 0:cols]
    tex = lambda yy, xx, c: (h(yy, xx, c, seed) + h(yy, xx + 1, c, seed) + h(yy + 1, xx, c, seed) + h(yy // 3, xx // 3, c, seed + 1)) // 4
    d = 1 + (y // 5 + x // 7) % 4
    left = np.stack([tex(y, x + 8, c) for c in range(cn)], -1)
    right = np.stack([np.clip(tex(y, x + 8 + d, c) + h(y, x, c, seed + 2) % 5 - 2, 0, 255) for c in range(cn)], -1)
    left, right = left.astype(np.uint8), right.astype(np.uint8)
    return (left[..., 0], right[..., 0]) if cn == 1 else (left, right)


# ---------------------------------------------------------------- pixeldiff, stereocsbp.cu:61-84
def pixeldiff(l, r, max_data_term):
    """l, r: uint8 arrays (..., cn)"""
    a = np.abs(l.astype(np.int32) - r.astype(np.int32)).astype(F)
    if l.shape[-1] == 1:
        return np.minimum(a[..., 0], F(max_data_term))
    tb, tg, tr = F(0.114) * a[..., 0], F(0.587) * a[..., 1], F(0.299) * a[..., 2]
    return np.minimum((tr + tg) + tb, F(max_data_term))


def _img3(img):
    return img[:, :, None] if img.ndim == 2 else img


def _tree(v):
    """reduce<W>(smem, val, tid, plus) of core/cuda/reduce.hpp over the last axis (W = 4 .. 128) -> lane 0's total
    (restated in oracle/refshim/cudashim/opencv2/core/cuda/reduce.hpp:5-9)"""
    w = v.shape[-1]
    if w <= 32:
        d = w // 2
        while d >= 1:
            v = v[..., :d] + v[..., d:2 * d]
            d //= 2
        return v[..., 0]
    g = np.stack([_tree(v[..., k * 32:(k + 1) * 32]) for k in range(w // 32)], -1)   # the tree of 32 in every warp
    return _tree(g)                                                                  # then the tree of width W / 32 over the totals


def data_cost(left, right, level, cand, max_data_term=30.0, data_weight=1.0, min_disp=0, **_):
    """init_data_cost / compute_data_cost and their reduce forms, stereocsbp.cu:178-267, :356-447, before the saturate_cast.
    cand: int (n, h, w), the disparity of candidate k at level pixel (y, x) -> f32 (n, h, w)"""
    left, right = _img3(left), _img3(right)
    rows, cols = left.shape[:2]
    n, h, w = cand.shape
    dw, mdt = F(data_weight), F(max_data_term)
    win = 1 << level
    ys, xs = np.arange(h)[None, :, None] * win, np.arange(w)[None, None, :] * win
    if level <= 1:   # one running sum, rows outer and columns inner (:196-216)
        val = np.zeros((n, h, w), F)
        for dy in range(win):
            for dx in range(win):
                yi, xi = np.broadcast_to(ys + dy, cand.shape), np.broadcast_to(xs + dx, cand.shape)
                xr = xi - cand
                out = (cand < min_disp) | (xr < 0)
                diff = pixeldiff(left[yi, xi], right[yi, np.clip(xr, 0, cols - 1)], mdt)
                val = val + np.where(out, dw * mdt, dw * diff)
        return val
    # column tid sums its len rows, then the tree (:220-267)
    tid = np.arange(win)[None, None, None, :]
    xi = np.broadcast_to(xs[..., None] + tid, (n, h, w, win))
    c4 = cand[..., None]
    xr = xi - c4
    length = np.minimum(ys + win, rows) - ys                     # (1, h, 1)
    inside = xi < cols
    out = (xr < 0) | (c4 < min_disp)
    val = np.zeros((n, h, w, win), F)
    xic, xrc = np.clip(xi, 0, cols - 1), np.clip(xr, 0, cols - 1)
    for y in range(win):
        yi = np.broadcast_to((ys + y)[..., None], xi.shape)
        live = np.broadcast_to((y < length)[..., None], xi.shape)
        diff = pixeldiff(left[np.clip(yi, 0, rows - 1), xic], right[np.clip(yi, 0, rows - 1), xrc], mdt)
        val = np.where(live, val + dw * diff, val)
    val = np.where(out, (dw * mdt) * length[..., None].astype(F), val)
    val = np.where(inside, val, F(0))
    return _tree(val)


def planes_of(mat, n, h, w):
    """the (n, h, w) view of the level's planes in a planar matrix (rows k * h + y, columns < w)"""
    return mat[:n * h].reshape(n, h, mat.shape[1])[:, :, :w]


# ---------------------------------------------------------------- get_first_k_initial_local / _global, stereocsbp.cu:86-176
def first_k(cost, nr_plane, local):
    """cost: (ndisp, h, w) of T, consumed -> (sel_cost, sel_disp), (nr_plane, h, w) of T"""
    ndisp, h, w = cost.shape
    T = cost.dtype
    mx = t_max(T)
    sel_cost, sel_disp = np.zeros((nr_plane, h, w), T), np.zeros((nr_plane, h, w), T)
    found = np.zeros((h, w), np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    if local and ndisp > 2:   # with ndisp == 2 the loop of :140 never runs (plane 2 is read and not used)
        prev, cur, nxt = cost[0].copy(), cost[1].copy(), cost[2].copy()
        for d in range(1, ndisp - 1):
            hit = (found < nr_plane) & (cur < prev) & (cur < nxt)
            slot = np.minimum(found, nr_plane - 1)
            sel_cost[slot[hit], yy[hit], xx[hit]] = cur[hit]
            sel_disp[slot[hit], yy[hit], xx[hit]] = d
            cost[d][hit] = mx
            found = found + hit
            prev, cur = cur, nxt
            nxt = cost[d + 1].copy()
    for i in range(nr_plane):
        todo = found <= i
        idx = np.argmin(cost, 0)   # strict <: the lowest index of the minimum; all spent: (max, 0)
        minimum = np.take_along_axis(cost, idx[None], 0)[0]
        sel_cost[i][todo] = minimum[todo]
        sel_disp[i][todo] = idx[todo]
        cost[idx[todo], yy[todo], xx[todo]] = mx
    return sel_cost, sel_disp


def init_data_cost(left, right, level, nr_plane, ndisp, msg_type, local=True, **w):
    """init_data_cost<T>, stereocsbp.cu:307-344 -> (data_cost_selected, disp_selected) as (nr_plane, h, w)"""
    T = msg_dtype(msg_type)
    h, wd = left.shape[0] >> level, left.shape[1] >> level
    cand = np.broadcast_to(np.arange(ndisp)[:, None, None], (ndisp, h, wd))
    cost = sat(T, data_cost(left, right, level, cand, **w)).copy()
    return first_k(cost, nr_plane, local)


# ---------------------------------------------------------------- the class's buffers and the kernels that read past a level
class Buffers:
    """mbuf_ of stereocsbp.cpp:190-212 as separate zero-initialised matrices"""

    def __init__(self, rows, cols, nr_plane, T, scratch_fill=0):
        z = lambda k=1: np.zeros((rows * nr_plane * k, cols), T)
        self.set = [dict(u=z(), d=z(), l=z(), r=z(), disp=z()) for _ in range(2)]
        # what the class zeroes (:235-236) but no kernel reads before writing it; scratch_fill proves that
        self.data_cost = np.full((rows * nr_plane * 2, cols), scratch_fill, T)
        self.sel_cost = np.full((rows * nr_plane, cols), scratch_fill, T)


def _parent(mat, k, h2, y, x):
    """mat[(k * h2 + y) , x] for index arrays y (may be == h2: the next plane, or past the level's planes) and x"""
    return mat[k * h2 + y, x]


def compute_data_cost(left, right, level, disp_parent, h, w, h2, n2, T, **wts):
    """compute_data_cost<T>, stereocsbp.cu:356-447: disp_parent a planar matrix -> (n2, h, w) of T"""
    yy, xx = np.mgrid[0:h, 0:w]
    cand = np.stack([_parent(disp_parent, k, h2, yy // 2, xx // 2) for k in range(n2)]).astype(np.int64)
    return sat(T, data_cost(left, right, level, cand, **wts))


def init_message(cur, new, data_cost_mat, sel_cost_mat, h, w, n, h2, w2, n2):
    """init_message<T>, stereocsbp.cu:558-607, on planar matrices: cur / new dicts of u, d, l, r, disp"""
    T = data_cost_mat.dtype
    yy, xx = np.mgrid[0:h, 0:w]
    y2, x2 = yy // 2, xx // 2
    dc = planes_of(data_cost_mat, n2, h, w)
    total = np.stack([tsum(T, dc[k], _parent(cur["u"], k, h2, np.minimum(h2 - 1, y2 + 1), x2),
                           _parent(cur["d"], k, h2, np.maximum(0, y2 - 1), x2),
                           _parent(cur["l"], k, h2, y2, np.minimum(w2 - 1, x2 + 1)),
                           _parent(cur["r"], k, h2, y2, np.maximum(0, x2 - 1))) for k in range(n2)])
    mx = t_max(T)
    for i in range(n):   # get_first_k_element_increase (:525-556): selected on the summed cost, stored is the unsummed one
        idx = np.argmin(total, 0)
        planes_of(sel_cost_mat, n, h, w)[i] = np.take_along_axis(dc, idx[None], 0)[0]
        for name in ("disp", "u", "d", "l", "r"):
            planes_of(new[name], n, h, w)[i] = cur[name][idx * h2 + y2, x2]
        total[idx, yy, xx] = mx


# ---------------------------------------------------------------- compute_message, stereocsbp.cu:656-716
def iterate(msgs, disp_mat, sel_cost_mat, h, w, n, t, max_disc_term, disc_single_jump):
    """one half-sweep (parity t & 1), in place; msgs a dict of planar matrices u, d, l, r.  max_disc_term: the float the class holds;
    calc_all_iterations takes it as int (stereocsbp.cu:720), truncated toward zero at the call (stereocsbp.cpp:266-268)."""
    T = sel_cost_mat.dtype
    mdisc, jump = int(max_disc_term), F(disc_single_jump)
    if h < 3 or w < 3:
        return   # no interior pixel
    ys, xs = np.mgrid[1:h - 1, 1:w - 1]
    keep = ((xs + ys + t) & 1) == 0   # x = 2 i + ((y + t) & 1)
    y, x = ys[keep], xs[keep]
    if y.size == 0:
        return
    at = lambda mat, dy=0, dx=0: np.stack([mat[k * h + y + dy, x + dx] for k in range(n)])
    data, dst_disp = at(sel_cost_mat), at(disp_mat).astype(F)
    ports = (("u", (("r", 0, -1), ("u", 1, 0), ("l", 0, 1)), (-1, 0)), ("d", (("d", -1, 0), ("r", 0, -1), ("l", 0, 1)), (1, 0)),
             ("l", (("u", 1, 0), ("d", -1, 0), ("l", 0, 1)), (0, -1)), ("r", (("u", 1, 0), ("d", -1, 0), ("r", 0, -1)), (0, 1)))
    for name, ins, (sy, sx) in ports:   # one after the other, in this order (:711-714)
        val = tsum(T, data, *[at(msgs[m], dy, dx) for m, dy, dx in ins])
        minimum = val.min(0)
        ceiling = minimum + F(mdisc) if T == np.float32 else (minimum.astype(np.int32) + mdisc).astype(F)
        src_disp = at(disp_mat, sy, sx).astype(F)
        valf = val.astype(F)
        temp = np.zeros_like(val)
        total = np.zeros(y.shape, F)
        for d in range(n):
            cost_min = np.minimum(ceiling, (valf + jump * np.abs(dst_disp - src_disp[d][None])).min(0))
            temp[d] = sat(T, cost_min)
            total = total + cost_min   # the unrounded one
        total = total / F(n)
        out = sat(T, temp.astype(F) - total[None])
        for k in range(n):
            msgs[name][k * h + y, x] = out[k]


def compute_disp(msgs, disp_mat, sel_cost_mat, rows, cols, n):
    """compute_disp<T>, stereocsbp.cu:752-785, on a zeroed map (stereocsbp.cpp:314) -> int16 (rows, cols)"""
    T = sel_cost_mat.dtype
    out = np.zeros((rows, cols), np.int16)
    if rows < 3 or cols < 3:
        return out
    y, x = np.mgrid[1:rows - 1, 1:cols - 1]
    at = lambda mat, dy=0, dx=0: np.stack([mat[k * rows + y + dy, x + dx] for k in range(n)])
    val = tsum(T, at(sel_cost_mat), at(msgs["u"], 1, 0), at(msgs["d"], -1, 0), at(msgs["l"], 0, 1), at(msgs["r"], 0, -1))
    idx = np.argmin(val, 0)   # strict <: the first candidate of the minimum
    best = np.take_along_axis(at(disp_mat), idx[None], 0)[0]
    best = np.where(np.take_along_axis(val, idx[None], 0)[0] < t_max(T), sat(np.int16, best), 0)   # nothing below max: best stays 0
    out[1:-1, 1:-1] = best
    return out


def convert_disp(disp16, dtype):
    """GpuMat::convertTo of the CV_16SC1 map (stereocsbp.cpp:327-328): saturate_cast<D>(short)"""
    if dtype == np.uint8:
        return np.clip(disp16, 0, 255).astype(np.uint8)
    return disp16.astype(dtype)


# ---------------------------------------------------------------- the class, stereocsbp.cpp:150-329
def compute(left, right, ndisp=128, iters=8, levels=4, nr_plane=4, msg_type=CV_32F, max_data_term=30.0, data_weight=1.0, max_disc_term=160.0,
            disc_single_jump=10.0, min_disp=0, local=True, scratch_fill=0, trace=None):
    """-> (disparity int16, clamped levels).  trace: a dict that receives the four messages of every level after its iterations."""
    levels = check_params(ndisp, iters, levels, nr_plane, msg_type, left, right)
    T = msg_dtype(msg_type)
    rows, cols = left.shape[:2]
    wts = dict(max_data_term=F(max_data_term), data_weight=F(data_weight), min_disp=min_disp)
    sizes = level_sizes(rows, cols, nr_plane, levels)
    B = Buffers(rows, cols, nr_plane, T, scratch_fill)
    cur = 0
    for i in range(levels - 1, -1, -1):
        h, w, n = sizes[i]
        if i == levels - 1:
            sc, sd = init_data_cost(left, right, i, n, ndisp, msg_type, local, **wts)
            planes_of(B.sel_cost, n, h, w)[:] = sc
            planes_of(B.set[cur]["disp"], n, h, w)[:] = sd
        else:
            h2, w2, n2 = sizes[i + 1]
            planes_of(B.data_cost, n2, h, w)[:] = compute_data_cost(left, right, i, B.set[cur]["disp"], h, w, h2, n2, T, **wts)
            new = (cur + 1) & 1
            init_message(B.set[cur], B.set[new], B.data_cost, B.sel_cost, h, w, n, h2, w2, n2)
            cur = new
        if trace is not None:
            trace[(i, "init")] = {k: planes_of(v, n, h, w).copy() for k, v in B.set[cur].items()}
        for t in range(iters):
            iterate(B.set[cur], B.set[cur]["disp"], B.sel_cost, h, w, n, t, F(max_disc_term), F(disc_single_jump))
        if trace is not None:
            trace[i] = {k: planes_of(v, n, h, w).copy() for k, v in B.set[cur].items()}
    return compute_disp(B.set[cur], B.set[cur]["disp"], B.sel_cost, rows, cols, nr_plane), levels
