"""HIP integer-descriptor matcher against the oracle: exact integer distances, identical lists.  The kernel logic is checked bit for
bit on the CPU (tests/test_bfmatch_int.py, the same source compiled for the host); what only the device shows -- barriers, the grid,
the strides from mi_mat into the kernels, 8/16-bit loads at odd byte offsets, __popc, the unsigned wrap of the L1 sum -- is checked here
on the edge table of that module.  (Collected last.)"""
import ctypes as C

import numpy as np
import pytest

from test_bfmatch_int import CASES, EDGE_IDS, EDGE_SHAPES, FLT_MAX, check_radius_is_strict, edge_data, edge_runs, occurring_radius

pytestmark = pytest.mark.gpu

NORM_L1, NORM_HAMMING = 2, 6


def _torch_dtype_ok(dt):
    import torch
    return hasattr(torch, dt)


@pytest.mark.parametrize("dt,norm,hi", CASES)
def test_hip_integer_matcher_equals_the_oracle(gpu, oracle, dt, norm, hi):
    import torch
    from opencv_contrib_amd import cuda
    if not _torch_dtype_ok(dt):
        pytest.skip(f"torch has no {dt}")
    rng = np.random.default_rng(9)
    lo = -hi if dt in ("int16", "int32") else 0
    nq, nts, d = 150, (333, 5, 64), 32
    q = rng.integers(lo, hi, (nq, d)).astype(dt)
    trains = [rng.integers(lo, hi, (n, d)).astype(dt) for n in nts]
    trains[0][3] = trains[0][1]
    masks = [(rng.random((nq, n)) < 0.7).astype(np.uint8) for n in nts]
    masks[1] = None
    T = lambda a: None if a is None else torch.from_numpy(a).to(gpu)
    m = cuda.createBFMatcher(norm)
    m.add([T(t) for t in trains])
    for ms in (None, masks):
        tm = None if ms is None else [T(x) for x in ms]
        for k in (1, 2, 7, 16):
            r = oracle.bf_knn_match(q, trains, k, norm, ms)
            idx, img, dist = m.knnMatchDevice(T(q), None, k=k, masks=tm)
            np.testing.assert_array_equal(idx.cpu().numpy(), r[0])
            np.testing.assert_array_equal(img.cpu().numpy(), r[1])
            np.testing.assert_array_equal(dist.cpu().numpy(), r[2])
        full = oracle.bf_knn_match(q, trains, 16, norm, ms)
        radius = float(np.percentile(full[2][:, -1], 60)) + 1
        rr = oracle.bf_radius_match(q, trains, radius, nq, norm, ms)
        i2, m2, d2, n2 = m.radiusMatchDevice(T(q), None, radius, masks=tm)
        np.testing.assert_array_equal(n2.cpu().numpy(), rr[3])
        np.testing.assert_array_equal(i2.cpu().numpy(), rr[0])
        np.testing.assert_array_equal(m2.cpu().numpy(), rr[1])
        np.testing.assert_array_equal(d2.cpu().numpy(), rr[2])
    # single train set through the host-list forms
    ms1 = m.match(T(q), T(trains[0]))
    r1 = oracle.bf_knn_match(q, trains[0], 1, norm)
    assert [x.trainIdx for x in ms1] == r1[0][:, 0].tolist()


def _equal(got, want):
    """device tensors against the oracle's arrays, in order"""
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g.cpu().numpy(), w)


@pytest.mark.parametrize("dt,norm,hi", CASES)
@pytest.mark.parametrize("d,nq,nts,k", EDGE_SHAPES, ids=EDGE_IDS)
def test_hip_integer_matcher_edge_shapes(gpu, oracle, dt, norm, hi, d, nq, nts, k):
    """Values over the whole range of the dtype (int32 L1 at d = 128 wraps the 32-bit sum; uint16 beyond 2^15), the shapes of
    EDGE_SHAPES with their masks, and for 65 queries once more with image 0 masked completely (the continuation launches find empty
    lists).  k-nearest lists; a radius match at a radius equal to an occurring distance; a radius match at 0; for the 200-row train
    set a single-set radius match of one query, whose two columns overflow."""
    import torch
    from opencv_contrib_amd import cuda
    if not _torch_dtype_ok(dt):
        pytest.skip(f"torch has no {dt}")
    T = lambda a: None if a is None else torch.from_numpy(a).to(gpu)
    for mask_first in edge_runs((d, nq, nts, k)):
        q, trains, masks = edge_data(dt, d, nq, nts, mask_first)
        tm = None if masks is None else [T(x) for x in masks]
        m = cuda.createBFMatcher(norm)
        m.add([T(t) for t in trains])
        r = oracle.bf_knn_match(q, trains, k, norm, masks)
        if d == 1:
            assert r[0].tolist() == [[0] + [-1] * 15] and (r[2][0, 1:] == FLT_MAX).all()
        if mask_first:
            assert (r[1] != 0).all()
        _equal(m.knnMatchDevice(T(q), None, k=k, masks=tm), r)
        radius = occurring_radius(r)
        rr = oracle.bf_radius_match(q, trains, radius, nq, norm, masks)
        check_radius_is_strict(r, rr, radius)
        _equal(m.radiusMatchDevice(T(q), None, radius, masks=tm), rr)
        r0 = oracle.bf_radius_match(q, trains, 0.0, nq, norm, masks)
        assert (r0[3] == 0).all() and (r0[0] == -1).all() and (r0[1] == -1).all() and (r0[2] == 0).all()
        _equal(m.radiusMatchDevice(T(q), None, 0.0, masks=tm), r0)
        if nts == (200,):
            # one query against one train set: cols = max(200 // 100, 1) = 2, and more hits than columns
            qi = int(np.argmax(rr[3]))
            q1, m1 = q[qi:qi + 1], masks[0][qi:qi + 1]
            r1 = oracle.bf_radius_match(q1, trains[0], radius, 2, norm, m1)
            assert r1[3][0] > 2
            got = m.radiusMatchDevice(T(q1), T(trains[0]), radius, mask=T(m1))
            assert got[0].shape == (1, 2)
            _equal(got, r1)


SENTINEL = -77


def _slice_of_wider(gpu, a, left, right, rng):
    """`a` as a column slice of a wider device tensor whose other columns hold random values -> (whole tensor, view)"""
    import torch
    info = np.iinfo(a.dtype)
    wide = rng.integers(info.min, info.max, (a.shape[0], left + a.shape[1] + right), dtype=np.int64, endpoint=True).astype(a.dtype)
    wide[:, left:left + a.shape[1]] = a
    w = torch.from_numpy(wide).to(gpu)
    return w, w[:, left:left + a.shape[1]]


def _sentinel_slice(gpu, rows, cols, dtype, left, right, prefill=None):
    """A rows x cols column slice of a wider tensor filled with SENTINEL (the slice itself with `prefill` if given)"""
    import torch
    w = torch.full((rows, left + cols + right), SENTINEL, dtype=dtype, device=gpu)
    v = w[:, left:left + cols]
    if prefill is not None:
        v.fill_(prefill)
    return w, v


def _sentinels_survive(w, left, cols):
    g = w.cpu().numpy()
    assert (g[:, :left] == SENTINEL).all() and (g[:, left + cols:] == SENTINEL).all()


@pytest.mark.parametrize("dt,norm,hi", CASES)
@pytest.mark.parametrize("d,nq,nts,k", [EDGE_SHAPES[1], EDGE_SHAPES[3]], ids=[EDGE_IDS[1], EDGE_IDS[3]])
def test_hip_integer_matcher_pitched_inputs_and_outputs(gpu, oracle, dt, norm, hi, d, nq, nts, k):
    """mi_bf_knn_match and mi_bf_radius_match called directly: query, trains and masks are column slices of wider tensors (uint8: at
    odd byte offsets), the outputs column slices of wider sentinel-filled tensors.  Results equal the oracle's and every element
    outside the slices keeps its sentinel."""
    import torch
    from opencv_contrib_amd import capi, cuda
    if not _torch_dtype_ok(dt):
        pytest.skip(f"torch has no {dt}")
    _m = capi.mat_from_tensor
    rng = np.random.default_rng(d)
    q, trains, masks = edge_data(dt, d, nq, nts)
    keep = []                                                     # the wide tensors: alive until the calls have run
    def view(a, left, right):
        if a is None:
            return None
        w, v = _slice_of_wider(gpu, a, left, right, rng)
        keep.append(w)
        assert (a.shape[0] == 1 or not v.is_contiguous()) and (v.data_ptr() - w.data_ptr()) == left * a.dtype.itemsize
        return v
    qv = view(q, 3, 2)
    tv = [view(t, 1 + 2 * j, 4) for j, t in enumerate(trains)]
    mv = [view(x, 5, 3 + j) for j, x in enumerate(masks)]
    m = cuda.createBFMatcher(norm)
    mats = cuda.BFMatcher._mats
    r = oracle.bf_knn_match(q, trains, k, norm, masks)
    wi, vi = _sentinel_slice(gpu, nq, k, torch.int32, 2, 3)
    wm, vm = _sentinel_slice(gpu, nq, k, torch.int32, 1, 5)
    wd, vd = _sentinel_slice(gpu, nq, k, torch.float32, 4, 1)
    capi.check(capi.lib().mi_bf_knn_match(m._h, C.byref(_m(qv)), mats(tv), mats(mv), len(tv), k, C.byref(_m(vi)), C.byref(_m(vm)), C.byref(_m(vd)),
                                          capi.current_stream_ptr()))
    _equal((vi, vm, vd), r)
    _sentinels_survive(wi, 2, k); _sentinels_survive(wm, 1, k); _sentinels_survive(wd, 4, k)
    radius = occurring_radius(r)
    cols = max(1, int(np.median(oracle.bf_radius_match(q, trains, radius, 1, norm, masks)[3])))   # some rows overflow, some stay short
    rr = oracle.bf_radius_match(q, trains, radius, cols, norm, masks)
    assert (rr[3] > cols).any() and (rr[3] < cols).any()
    wi, vi = _sentinel_slice(gpu, nq, cols, torch.int32, 3, 2, -1)
    wm, vm = _sentinel_slice(gpu, nq, cols, torch.int32, 5, 1, -1)
    wd, vd = _sentinel_slice(gpu, nq, cols, torch.float32, 1, 4, 0)
    wn, vn = _sentinel_slice(gpu, 1, nq, torch.int32, 3, 3)
    capi.check(capi.lib().mi_bf_radius_match(m._h, C.byref(_m(qv)), mats(tv), mats(mv), len(tv), radius, C.byref(_m(vi)), C.byref(_m(vm)),
                                             C.byref(_m(vd)), C.byref(_m(vn)), capi.current_stream_ptr()))
    _equal((vi, vm, vd, vn[0]), rr)
    _sentinels_survive(wi, 3, cols); _sentinels_survive(wm, 5, cols); _sentinels_survive(wd, 1, cols); _sentinels_survive(wn, 3, nq)


@pytest.mark.parametrize("dt,norm", [("uint8", NORM_HAMMING), ("int32", NORM_L1)])
@pytest.mark.parametrize("d,nq,nts,k", [EDGE_SHAPES[1], EDGE_SHAPES[3]], ids=[EDGE_IDS[1], EDGE_IDS[3]])
def test_hip_integer_matcher_fixed_shape_entry_points(gpu, oracle, dt, norm, d, nq, nts, k):
    """mi_bf_match and mi_bf_knn_match2 with integer descriptors: the outputs are 1 x nq rows whose element packs a query's k
    entries, so the kernels' per-query stride is k.  Equal to the oracle's k = 1 and k = 2 on the first train set, masked."""
    import torch
    from opencv_contrib_amd import capi, cuda
    _m = capi.mat_from_tensor
    q, trains, masks = edge_data(dt, d, nq, nts)
    t, mask = trains[0], masks[0]
    T = lambda a: torch.from_numpy(a).to(gpu)
    tq, tt, tm = T(q), T(t), T(mask)
    m = cuda.createBFMatcher(norm)
    r1 = oracle.bf_knn_match(q, t, 1, norm, mask)
    r2 = oracle.bf_knn_match(q, t, 2, norm, mask)
    assert r1[0][-1, 0] == -1 and (r2[0] >= 0).any()                 # the last query is masked completely
    i1 = torch.full((1, nq), SENTINEL, dtype=torch.int32, device=gpu); d1 = torch.full((1, nq), SENTINEL, dtype=torch.float32, device=gpu)
    capi.check(capi.lib().mi_bf_match(m._h, C.byref(_m(tq)), C.byref(_m(tt)), C.byref(_m(tm)), C.byref(_m(i1)), C.byref(_m(d1)),
                                      capi.current_stream_ptr()))
    ik = torch.full((1, nq, 2), SENTINEL, dtype=torch.int32, device=gpu); dk = torch.full((1, nq, 2), SENTINEL, dtype=torch.float32, device=gpu)
    capi.check(capi.lib().mi_bf_knn_match2(m._h, C.byref(_m(tq)), C.byref(_m(tt)), C.byref(_m(tm)), C.byref(_m(ik)), C.byref(_m(dk)),
                                           capi.current_stream_ptr()))
    _equal((i1[0], d1[0]), (r1[0][:, 0], r1[2][:, 0]))
    _equal((ik[0], dk[0]), (r2[0], r2[2]))


def test_hip_reference_binding_test_and_type_table(gpu):
    """cudafeatures2d/misc/python/test/test_cudafeatures2d.py:46-54 on random 32-byte descriptors + the (depth, norm) table's errors."""
    import torch
    from opencv_contrib_amd import capi, cuda
    rng = np.random.default_rng(4)
    d1 = rng.integers(0, 256, (500, 32)).astype(np.uint8)
    d2 = d1.copy()
    d2[::3] ^= rng.integers(0, 4, d2[::3].shape).astype(np.uint8)
    t1, t2 = torch.from_numpy(d1).to(gpu), torch.from_numpy(d2).to(gpu)
    bf = cuda.DescriptorMatcher.createBFMatcher(cuda.NORM_HAMMING)
    assert len(bf.match(t1, t2)) == 500
    assert len(bf.knnMatch(t1, t2, 2)) == 500
    assert sum(len(r) for r in bf.radiusMatch(t1, t2, 0.1)) >= 300
    with pytest.raises(capi.MiError):
        cuda.createBFMatcher(cuda.NORM_L2).matchDevice(t1, t2)                      # L2 on CV_8U: unsupported combination
    with pytest.raises(capi.MiError):
        cuda.createBFMatcher(cuda.NORM_HAMMING).matchDevice(t1.to(torch.int16), t2.to(torch.int16))   # Hamming on CV_16S
    with pytest.raises(capi.MiError):
        bf.knnMatchDevice(t1, t2, k=17)                                             # integer path: k <= 16
    with pytest.raises(capi.MiError):
        bf.matchDevice(torch.zeros((4, 200), dtype=torch.uint8, device=gpu), torch.zeros((4, 200), dtype=torch.uint8, device=gpu))   # > 128 elements
