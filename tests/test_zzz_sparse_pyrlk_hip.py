"""HIP SparsePyrLKOpticalFlow against the oracle.  The kernel logic is checked bit for bit on the CPU (tests/test_sparse_pyrlk.py, the same
source compiled for the host) and uses only correctly rounded binary32 operations; on MI355X status, next point and error equal the oracle bit
for bit at every point of every case below (random, border and single points), so equality is what is asserted."""
import numpy as np
import pytest

from opencv_contrib_amd import synth
from test_sparse_pyrlk import EDGE_CASES, EDGE_IDS, edge_frames, edge_points

pytestmark = pytest.mark.gpu


def _border_points(cols, rows):
    """Points exactly on x = 0, y = 0, x = cols - 1 and y = rows - 1 (the four corners included), then a few inside."""
    xs = np.linspace(0, cols - 1, 9).round()
    ys = np.linspace(0, rows - 1, 7).round()
    p = [(x, 0) for x in xs] + [(x, rows - 1) for x in xs] + [(0, y) for y in ys] + [(cols - 1, y) for y in ys] + [(40.5, 50.25), (160, 100)]
    return np.array(p, np.float32)


def _run(gpu, oracle, I0, I1, pts, win, max_level, iters, use_init):
    import torch
    from opencv_contrib_amd import cuda
    init = (pts + np.float32(1.5)).astype(np.float32) if use_init else None
    rn, rs, re_ = oracle.pyrlk_sparse(I0, I1, pts, win, max_level, iters, init)
    alg = cuda.SparsePyrLKOpticalFlow.create(win, max_level, iters, use_init)
    assert alg.getWinSize() == win and alg.getMaxLevel() == max_level and alg.getDefaultName() == "SparseOpticalFlow.SparsePyrLKOpticalFlow"
    t = lambda a: torch.from_numpy(a).to(gpu)
    nxt, st, err = alg.calc(t(I0), t(I1), t(pts), t(init) if use_init else None)
    return (nxt.cpu().numpy()[0], st.cpu().numpy()[0], err.cpu().numpy()[0]), (rn, rs, re_)


@pytest.fixture(scope="module")
def frames():
    I0, I1, _ = synth.flow_pair(203, 317, seed=11, dtype="u8")
    return I0, I1


OLD_CASES = [((21, 21), 3, 30, False), ((13, 9), 2, 10, False), ((31, 31), 4, 30, True)]
NEW_WINDOWS = [((3, 3), 0, 5, False), ((32, 32), 1, 8, False)]      # the smallest window and the largest one built (1024 pixels)


def _random_points():
    rng = np.random.default_rng(3)
    return np.stack([rng.uniform(-12, 329, 500), rng.uniform(-12, 215, 500)], 1).astype(np.float32)


def _check(gpu, oracle, frames, pts, win, max_level, iters, use_init):
    (nxt, st, err), (rn, rs, re_) = _run(gpu, oracle, frames[0], frames[1], pts, win, max_level, iters, use_init)
    assert (rs > 0).any()
    np.testing.assert_array_equal(st, rs)
    np.testing.assert_array_equal(nxt, rn)                         # every point: an untracked one keeps its prepared start value
    np.testing.assert_array_equal(err[rs > 0], re_[rs > 0])        # err is written where the track completes at level 0


@pytest.mark.parametrize("win,max_level,iters,use_init", OLD_CASES)
def test_hip_sparse_pyrlk_matches_the_oracle(gpu, oracle, frames, win, max_level, iters, use_init):
    _check(gpu, oracle, frames, _random_points(), win, max_level, iters, use_init)


@pytest.mark.parametrize("win,max_level,iters,use_init", NEW_WINDOWS)
def test_hip_sparse_pyrlk_smallest_and_largest_window(gpu, oracle, frames, win, max_level, iters, use_init):
    _check(gpu, oracle, frames, _random_points(), win, max_level, iters, use_init)


@pytest.mark.parametrize("win,max_level,iters,use_init", OLD_CASES + NEW_WINDOWS)
def test_hip_sparse_pyrlk_one_point(gpu, oracle, frames, win, max_level, iters, use_init):
    _check(gpu, oracle, frames, np.array([[151.25, 97.5]], np.float32), win, max_level, iters, use_init)


@pytest.mark.parametrize("win,max_level,iters,use_init", OLD_CASES + NEW_WINDOWS)
def test_hip_sparse_pyrlk_points_on_the_image_border(gpu, oracle, frames, win, max_level, iters, use_init):
    """x = 0, y = 0, x = cols - 1, y = rows - 1: inside [0, cols) x [0, rows), so tracked, with half the window clamped."""
    _check(gpu, oracle, frames, _border_points(317, 203), win, max_level, iters, use_init)


def test_hip_sparse_pyrlk_arguments(gpu):
    import torch
    from opencv_contrib_amd import capi, cuda
    I0, I1, _ = synth.flow_pair(64, 80, seed=1, dtype="u8")
    t = lambda a: torch.from_numpy(a).to(gpu)
    alg = cuda.SparsePyrLKOpticalFlow.create()
    nxt, st, err = alg.calc(t(I0), t(I1), torch.empty((0, 2), device=gpu))
    assert nxt.shape == (1, 0, 2) and st.shape == (1, 0)
    pts = t(np.array([[20.0, 20.0]], np.float32))
    with pytest.raises(capi.MiError):
        alg.calc(t(I0), t(I1[:60]), pts)                                   # prevImg.size() == nextImg.size()
    with pytest.raises(capi.MiError):
        alg.calc(t(I0.astype(np.float32)), t(I1.astype(np.float32)), pts)  # CV_8UC1 only
    with pytest.raises(capi.MiError):
        cuda.SparsePyrLKOpticalFlow.create((2, 21))                        # winSize > 2
    with pytest.raises(capi.MiError):
        cuda.SparsePyrLKOpticalFlow.create((40, 40))                       # more than 1024 window pixels: not built
    with pytest.raises(capi.MiError):
        cuda.SparsePyrLKOpticalFlow.create(useInitialFlow=True).calc(t(I0), t(I1), pts)   # nextPts required


# ---- edge shapes: the table of tests/test_sparse_pyrlk.py (there through the host build), here through the product
def _calc(gpu, I0, I1, pts, init, win, max_level, iters, use_init, want_err=True):
    """I0, I1: device tensors (dense or pitched) -> host (nextPts, status, err or None)"""
    import torch
    from opencv_contrib_amd import cuda
    alg = cuda.SparsePyrLKOpticalFlow.create(win, max_level, iters, use_init)
    t = lambda a: torch.from_numpy(a).to(gpu)
    nxt, st, err = alg.calc(I0, I1, t(pts), t(init) if use_init else None, wantErr=want_err)
    return nxt.cpu().numpy()[0], st.cpu().numpy()[0], (err.cpu().numpy()[0] if want_err else None)


def _same(got, want):
    (nxt, st, err), (rn, rs, re_) = got, want
    np.testing.assert_array_equal(st, rs)
    np.testing.assert_array_equal(nxt, rn)
    if err is not None:
        np.testing.assert_array_equal(err[rs > 0], re_[rs > 0])


@pytest.mark.parametrize("rows,cols,win,max_level,iters,use_init", EDGE_CASES, ids=EDGE_IDS)
def test_hip_sparse_pyrlk_edge_shapes(gpu, oracle, rows, cols, win, max_level, iters, use_init):
    """Frames of a few pixels, a window larger than the frame, wide and tall windows, sixteen levels that collapse to 1 x 1, no Newton
    step, pyramid levels on and one past a k_pyr_down_u8 workgroup edge; points outside, on the corners, at -0.0 and far away."""
    import torch
    I0, I1 = edge_frames(rows, cols)
    pts, init = edge_points(rows, cols)
    want = oracle.pyrlk_sparse(I0, I1, pts, win, max_level, iters, init if use_init else None)
    assert 0 < want[1].sum() < len(pts)
    _same(_calc(gpu, torch.from_numpy(I0).to(gpu), torch.from_numpy(I1).to(gpu), pts, init, win, max_level, iters, use_init), want)


def _pitched(gpu, frame, pitch, offset):
    """The frame as a column slice at byte `offset` of a buffer with rows of `pitch` bytes (one more row above and below); the
    surroundings hold the value farthest from the frame's median."""
    import torch
    rows, cols = frame.shape
    buf = np.full((rows + 2, pitch), 0 if np.median(frame) > 127 else 255, np.uint8)
    buf[1:rows + 1, offset:offset + cols] = frame
    view = torch.from_numpy(buf).to(gpu)[1:rows + 1, offset:offset + cols]
    assert view.stride(0) == pitch and not view.is_contiguous()
    return view


@pytest.mark.parametrize("rows,cols,win,max_level,iters,use_init", [c for c in EDGE_CASES if c[:2] == (33, 65)],
                         ids=[i for c, i in zip(EDGE_CASES, EDGE_IDS) if c[:2] == (33, 65)])
def test_hip_sparse_pyrlk_pitched_frames(gpu, oracle, rows, cols, win, max_level, iters, use_init):
    """prevImg at byte offset 7 of 96-byte rows, nextImg at byte offset 3 of 160-byte rows (the smaller pitch belongs to prevImg: nextImg
    read with prevImg's step would return wrong pixels from inside its own allocation): equal to the oracle on the dense frames."""
    I0, I1 = edge_frames(rows, cols)
    pts, init = edge_points(rows, cols)
    want = oracle.pyrlk_sparse(I0, I1, pts, win, max_level, iters, init if use_init else None)
    assert 0 < want[1].sum() < len(pts)
    _same(_calc(gpu, _pitched(gpu, I0, 96, 7), _pitched(gpu, I1, 160, 3), pts, init, win, max_level, iters, use_init), want)


@pytest.mark.parametrize("rows,cols,win,max_level,iters,use_init", [EDGE_CASES[2], EDGE_CASES[4], EDGE_CASES[5]],
                         ids=[EDGE_IDS[2], EDGE_IDS[4], EDGE_IDS[5]])
def test_hip_sparse_pyrlk_without_err(gpu, oracle, rows, cols, win, max_level, iters, use_init):
    """err == NULL: next points and status are those of a call with err, and the oracle's."""
    import torch
    I0, I1 = edge_frames(rows, cols)
    pts, init = edge_points(rows, cols)
    want = oracle.pyrlk_sparse(I0, I1, pts, win, max_level, iters, init if use_init else None)
    t0, t1 = torch.from_numpy(I0).to(gpu), torch.from_numpy(I1).to(gpu)
    with_err = _calc(gpu, t0, t1, pts, init, win, max_level, iters, use_init)
    without = _calc(gpu, t0, t1, pts, init, win, max_level, iters, use_init, want_err=False)
    assert without[2] is None
    _same(with_err, want)
    _same(without, want)
    np.testing.assert_array_equal(without[0], with_err[0])
    np.testing.assert_array_equal(without[1], with_err[1])


@pytest.mark.parametrize("use_init", [False, True])
@pytest.mark.parametrize("n", [255, 256, 257])
def test_hip_sparse_pyrlk_point_counts_around_a_prepare_workgroup(gpu, oracle, n, use_init):
    """k_prepare runs 256 points per workgroup: one short of it, exactly it, one over."""
    import torch
    I0, I1 = edge_frames(33, 65)
    pts, init = edge_points(33, 65, n)
    want = oracle.pyrlk_sparse(I0, I1, pts, (9, 9), 2, 10, init if use_init else None)
    assert 0 < want[1].sum() < n
    _same(_calc(gpu, torch.from_numpy(I0).to(gpu), torch.from_numpy(I1).to(gpu), pts, init, (9, 9), 2, 10, use_init), want)
