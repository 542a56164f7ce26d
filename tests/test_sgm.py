"""cv::cuda::StereoSGM.  The stage tests restate the reference's own unit tests (cudastereo/test/test_sgm_funcs.cpp):
random census / cost volumes through each device stage against the CPU twin the reference ships for it, bit-exact
(EXPECT_MAT_NEAR(gold, dst, 0)); the oracle's census, path aggregation and left winner-takes-all ARE those twins
(oracle/sgm_ref.c), so these stages are pinned on the reference's own tests."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opencv_contrib_amd import synth  # noqa: E402

DIRS = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1)]   # test_sgm_funcs.cpp:301-339


# ------------------------------------------------------------------ oracle (CPU)
def test_oracle_census_bit_order_and_border(oracle):
    """A single bright pixel: bit b of the census of a pixel is set iff the b-th compared neighbour (row-major over the upper
    half window, test_sgm_funcs.cpp:139-147) is brighter than its point reflection; the 4 / 3 pixel border stays 0."""
    img = np.zeros((15, 21), np.uint8)
    img[7, 10] = 255
    c = oracle.sgm_census(img)
    assert (c[:3] == 0).all() and (c[-3:] == 0).all() and (c[:, :4] == 0).all() and (c[:, -4:] == 0).all()
    # centre pixel (7, 10): no compared pair contains it (pairs are point reflections about the centre) -> 0
    assert c[7, 10] == 0
    # pixel (8, 10): its neighbour (dy, dx) = (-1, 0) is the bright pixel = comparison index 9 + 9 + 4 = 22 of 31 -> bit 30 - 22
    assert c[8, 10] == 1 << (30 - 22)
    # pixel (6, 10): the bright pixel is its (+1, 0) neighbour = the reflected operand b of that same comparison -> a > b false
    assert c[6, 10] == 0


def test_oracle_path_first_pixel_and_saturation(oracle):
    rng = np.random.default_rng(0)
    l = rng.integers(0, 2 ** 31 - 1, (5, 9), dtype=np.int64).astype(np.int32)
    r = rng.integers(0, 2 ** 31 - 1, (5, 9), dtype=np.int64).astype(np.int32)
    out = oracle.sgm_path(l, r, 64, 0, 10, 120, 1, 0).reshape(5, 9, 64)
    # first pixel of a left-to-right path: no predecessor, cost = hamming(l, 0) for every disparity > 0 (k > j -> r = 0)
    assert out[2, 0, 5] == bin(int(l[2, 0]) & 0xffffffff).count("1")
    assert out[2, 0, 0] == bin((int(l[2, 0]) ^ int(r[2, 0])) & 0xffffffff).count("1")
    big = oracle.sgm_path(l, r, 64, 0, 10, 250, 1, 0)      # P2 + popcount can exceed 255: static_cast<uint8_t> wraps
    assert big.dtype == np.uint8


def test_oracle_compute_rejects_unsupported(oracle):
    img = np.zeros((32, 64), np.uint8)
    with pytest.raises(ValueError):
        oracle.sgm_compute(img, img, oracle.sgm_params(num_disparities=96))      # stereosgm.cpp:138 "Unsupported num of disparities"
    with pytest.raises(ValueError):
        oracle.sgm_compute(img, img, oracle.sgm_params(mode=0))                  # stereosgm.cpp:102-105 "Unsupported mode"


def test_oracle_recovers_synthetic_disparity(oracle):
    left, right, gt = synth.stereo_pair(96, 224, seed=42, max_disp=30)
    d = oracle.sgm_compute(left, right, oracle.sgm_params(num_disparities=64)).astype(np.float64) / 16
    ys, xs = np.mgrid[0:96, 0:224]
    valid = d > 0
    xr = np.clip(np.round(xs - d).astype(int), 0, 223)
    assert valid.mean() > 0.7 and np.median(np.abs(d - gt[ys, xr])[valid]) < 1.0


# ------------------------------------------------------------------ stages, HIP vs the reference's CPU twins (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("shape", [(128, 128), (113, 131), (8, 12), (6, 30)])
def test_census_random(gpu, oracle, dtype, shape):
    """StereoSGM_CensusTransformRandom, test_sgm_funcs.cpp:190-206."""
    import torch
    from opencv_contrib_amd import cuda
    rng = np.random.default_rng(shape[0])
    img = rng.integers(0, 256 if dtype == np.uint8 else 65536, shape).astype(dtype)
    out = cuda.sgm_census(torch.from_numpy(img).to(gpu)).cpu().numpy()
    np.testing.assert_array_equal(out, oracle.sgm_census(img))


@pytest.mark.gpu
@pytest.mark.parametrize("dxdy", DIRS)
@pytest.mark.parametrize("min_disp", [0, 1, 10])
def test_path_aggregation_random(gpu, oracle, dxdy, min_disp):
    """StereoSGM_PathAggregation.Random*, test_sgm_funcs.cpp:262-345: DISPARITY 128, P1 10, P2 120, random 31-bit census values."""
    import torch
    from opencv_contrib_amd import cuda
    rng = np.random.default_rng(7 + min_disp)
    h, w = 67, 113
    l = rng.integers(0, 2 ** 31 - 1, (h, w), dtype=np.int64).astype(np.int32)
    r = rng.integers(0, 2 ** 31 - 1, (h, w), dtype=np.int64).astype(np.int32)
    out = cuda.sgm_aggregate_path(torch.from_numpy(l).to(gpu), torch.from_numpy(r).to(gpu), 128, min_disp, 10, 120, *dxdy).cpu().numpy()
    np.testing.assert_array_equal(out.reshape(-1), oracle.sgm_path(l, r, 128, min_disp, 10, 120, *dxdy))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [64, 256])
def test_path_aggregation_other_disparity_counts(gpu, oracle, D):
    import torch
    from opencv_contrib_amd import cuda
    rng = np.random.default_rng(D)
    l = rng.integers(0, 2 ** 31 - 1, (21, 300), dtype=np.int64).astype(np.int32)
    r = rng.integers(0, 2 ** 31 - 1, (21, 300), dtype=np.int64).astype(np.int32)
    for dxdy in [(1, 0), (0, -1), (-1, 1)]:
        out = cuda.sgm_aggregate_path(torch.from_numpy(l).to(gpu), torch.from_numpy(r).to(gpu), D, 2, 7, 200, *dxdy).cpu().numpy()
        np.testing.assert_array_equal(out.reshape(-1), oracle.sgm_path(l, r, D, 2, 7, 200, *dxdy))


@pytest.mark.gpu
@pytest.mark.parametrize("subpixel", [False, True])
@pytest.mark.parametrize("npaths", [4, 8])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_winner_takes_all_random(gpu, oracle, subpixel, npaths, D):
    """StereoSGM_WinnerTakesAll.RandomLeft, test_sgm_funcs.cpp:405-441 (costs 0..32, uniqueness 0.95) -- and the right map."""
    import torch
    from opencv_contrib_amd import cuda
    rng = np.random.default_rng(D + npaths)
    h, w = 19, 141
    agg = rng.integers(0, 32, (1, w * h * D * npaths)).astype(np.uint8)
    left, right = cuda.sgm_winner_takes_all(torch.from_numpy(agg).to(gpu), w, h, D, npaths, 0.95, subpixel)
    rl, rr = oracle.sgm_wta(agg, w, h, D, npaths, 0.95, subpixel)
    np.testing.assert_array_equal(left.cpu().numpy(), rl)
    np.testing.assert_array_equal(right.cpu().numpy(), rr)


@pytest.mark.gpu
@pytest.mark.parametrize("D,w", [(64, 600), (128, 777), (256, 1100)])
def test_winner_takes_all_wide_rows_are_segmented(gpu, oracle, D, w):
    """Rows wider than one segment (256 / 512 px): segments walk D - 1 pixels past their end for the right minima."""
    import torch
    from opencv_contrib_amd import cuda
    rng = np.random.default_rng(D + w)
    h = 5
    agg = rng.integers(0, 32, (1, w * h * D * 4)).astype(np.uint8)
    left, right = cuda.sgm_winner_takes_all(torch.from_numpy(agg).to(gpu), w, h, D, 4, 0.95, True)
    rl, rr = oracle.sgm_wta(agg, w, h, D, 4, 0.95, True)
    np.testing.assert_array_equal(left.cpu().numpy(), rl)
    np.testing.assert_array_equal(right.cpu().numpy(), rr)


def _census_pair(rng, shape):
    l = rng.integers(0, 2 ** 31 - 1, shape, dtype=np.int64).astype(np.int32)
    r = rng.integers(0, 2 ** 31 - 1, shape, dtype=np.int64).astype(np.int32)
    return l, r


def _hip_path(gpu, l, r, D, min_disp, p1, p2, dxdy):
    import torch
    from opencv_contrib_amd import cuda
    return cuda.sgm_aggregate_path(torch.from_numpy(l).to(gpu), torch.from_numpy(r).to(gpu), D, min_disp, p1, p2, *dxdy).cpu().numpy().reshape(-1)


@pytest.fixture(scope="module")
def shifted_census():
    """right random, left = right shifted by 7: disparity 7 costs 0 all along a line while the others cost ~15.5 bits, so their path
    costs climb to the P2 cap above the minimum and cap + popcount passes 255."""
    r = _census_pair(np.random.default_rng(250), (40, 150))[1]
    return np.roll(r, 7, axis=1), r


@pytest.mark.gpu
@pytest.mark.parametrize("dxdy", DIRS)
@pytest.mark.parametrize("D", [64, 128, 256])
def test_path_aggregation_cost_cast_wraps(gpu, oracle, shifted_census, dxdy, D):
    """min(.., P2 = 250) + popcount > 255: static_cast<uint8_t> wraps modulo 256, it does not saturate.  With P2 = 224 (224 + 31 = 255)
    nothing wraps; the outputs of the two must differ or the case does not reach the cast."""
    l, r = shifted_census
    ref = oracle.sgm_path(l, r, D, 0, 10, 250, *dxdy)
    assert (ref != oracle.sgm_path(l, r, D, 0, 10, 224, *dxdy)).any()
    np.testing.assert_array_equal(_hip_path(gpu, l, r, D, 0, 10, 250, dxdy), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("min_disp", [-1, -5, -70])
@pytest.mark.parametrize("D", [64, 128])
def test_path_aggregation_negative_min_disparity(gpu, oracle, min_disp, D):
    """j - k - minDisparity can pass the right end of the row (cost against census 0 there); at -70 on 70 columns it always does."""
    l, r = _census_pair(np.random.default_rng(D - min_disp), (9, 70))
    for dxdy in [(1, 0), (0, -1), (-1, 1)]:
        np.testing.assert_array_equal(_hip_path(gpu, l, r, D, min_disp, 10, 120, dxdy), oracle.sgm_path(l, r, D, min_disp, 10, 120, *dxdy))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 70), (70, 1), (3, 3), (2, 130)])
def test_path_aggregation_lines_shorter_than_the_prefetch(gpu, oracle, shape):
    """Scan lines of 1 .. 3 pixels: the 4-deep census prefetch starts outside the image."""
    l, r = _census_pair(np.random.default_rng(shape[0] * 1000 + shape[1]), shape)
    for dxdy in DIRS:
        np.testing.assert_array_equal(_hip_path(gpu, l, r, 128, 1, 10, 120, dxdy), oracle.sgm_path(l, r, 128, 1, 10, 120, *dxdy))


def _wta_widths(D):
    return [1, 63, D - 1, D, D + 1] + ([256, 257] if D <= 128 else [512, 513])


@pytest.fixture(scope="module")
def wta_oracle(oracle):
    """Oracle results of the winner-takes-all sweep, computed once per (values, D)."""
    cache = {}

    def get(values, D):
        if (values, D) not in cache:
            rng = np.random.default_rng(D + values)
            cases = []
            for w in _wta_widths(D):
                for h in (1, 5):
                    agg = rng.integers(0, values, (1, w * h * D * 8)).astype(np.uint8)
                    for uniq in (0.0, 0.95, 1.0):
                        for sub in (False, True):
                            cases.append((w, h, agg, uniq, sub, oracle.sgm_wta(agg, w, h, D, 8, uniq, sub)))
            cache[(values, D)] = cases
        return cache[(values, D)]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("values", [256, 2])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_winner_takes_all_at_its_ends(gpu, wta_oracle, values, D):
    """Costs over all of 0 .. 255 on 8 paths (sums to 2040), and costs from {0, 1}: many equal sums, so the first minimum (lowest
    disparity) rule decides both maps (it also keeps the sub-pixel denominator l - 2 best + r positive: the left neighbour of a
    first minimum costs strictly more).  Widths below, at and above D
    and one segment / one segment and a pixel; uniqueness 0 (only a zero best cost survives), 0.95, 1 (nothing is rejected)."""
    import torch
    from opencv_contrib_amd import cuda
    for w, h, agg, uniq, sub, (rl, rr) in wta_oracle(values, D):
        left, right = cuda.sgm_winner_takes_all(torch.from_numpy(agg).to(gpu), w, h, D, 8, uniq, sub)
        np.testing.assert_array_equal(left.cpu().numpy(), rl, err_msg=f"left w={w} h={h} uniq={uniq} subpixel={sub}")
        np.testing.assert_array_equal(right.cpu().numpy(), rr, err_msg=f"right w={w} h={h} uniq={uniq} subpixel={sub}")


# ------------------------------------------------------------------ full pipeline
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("D,min_disp", [(64, 0), (128, 3)])
@pytest.mark.parametrize("quirks", [True, False])
def test_compute_bit_exact(gpu, oracle, mode, D, min_disp, quirks):
    import torch
    from opencv_contrib_amd import cuda
    left, right, _ = synth.stereo_pair(101, 237, seed=11, max_disp=40)      # not multiples of 16: the consistency-check quirk matters
    sgm = cuda.createStereoSGM(min_disp, D, 10, 120, 5, mode, emulateCudaQuirks=quirks)
    assert (sgm.getMinDisparity(), sgm.getNumDisparities(), sgm.getP1(), sgm.getP2(), sgm.getUniquenessRatio(), sgm.getMode()) == \
        (min_disp, D, 10, 120, 5, mode)
    assert (sgm.getBlockSize(), sgm.getDisp12MaxDiff(), sgm.getPreFilterCap()) == (-1, 1, -1)       # stereosgm.cpp:38-72
    out = sgm.compute(torch.from_numpy(left).to(gpu), torch.from_numpy(right).to(gpu)).cpu().numpy()
    ref = oracle.sgm_compute(left, right, oracle.sgm_params(min_disp, D, 10, 120, 5, mode, int(quirks)))
    np.testing.assert_array_equal(out, ref)
    assert (out >= (min_disp - 1) * 16).all() and (out > 0).mean() > 0.5


@pytest.mark.gpu
def test_compute_16bit_images_pitched_and_errors(gpu, oracle):
    import torch
    from opencv_contrib_amd import capi, cuda
    left, right, _ = synth.stereo_pair(64, 160, seed=12, max_disp=30)
    l16, r16 = (left.astype(np.uint16) * 257), (right.astype(np.uint16) * 257)
    sgm = cuda.createStereoSGM(0, 64)
    bigl = torch.zeros((70, 200), dtype=torch.uint16, device=gpu); bigr = torch.zeros_like(bigl)
    bigl[3:67, 20:180] = torch.from_numpy(l16).to(gpu); bigr[3:67, 20:180] = torch.from_numpy(r16).to(gpu)
    out = sgm.compute(bigl[3:67, 20:180], bigr[3:67, 20:180]).cpu().numpy()        # pitched ROI views
    np.testing.assert_array_equal(out, oracle.sgm_compute(l16, r16, oracle.sgm_params(num_disparities=64)))
    tl = torch.from_numpy(left).to(gpu)
    sgm.setNumDisparities(96)
    with pytest.raises(capi.MiError):
        sgm.compute(tl, tl)                                    # "Unsupported num of disparities"
    sgm.setNumDisparities(64); sgm.setMode(0)
    with pytest.raises(capi.MiError):
        sgm.compute(tl, tl)                                    # "Unsupported mode"
    sgm.setMode(3)
    with pytest.raises(capi.MiError):
        sgm.compute(tl, torch.from_numpy(right[:, :100].copy()).to(gpu))           # size mismatch


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(13, 15), (16, 16), (32, 48), (17, 33)])
@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("quirks", [True, False])
def test_compute_small_sizes_negative_min_disparity(gpu, oracle, shape, mode, quirks):
    """Sizes around the 16 x 16 blocks of the reference's consistency check (13 x 15 with quirks: no pixel is checked), minDisparity -8,
    P2 250 (the cost cast wraps), uniquenessRatio 0 and 100."""
    import torch
    from opencv_contrib_amd import cuda
    left, right, _ = synth.stereo_pair(shape[0], shape[1], seed=13, max_disp=10)
    tl, tr = torch.from_numpy(left).to(gpu), torch.from_numpy(right).to(gpu)
    for ur in (0, 100):
        sgm = cuda.createStereoSGM(-8, 64, 10, 250, ur, mode, emulateCudaQuirks=quirks)
        ref = oracle.sgm_compute(left, right, oracle.sgm_params(-8, 64, 10, 250, ur, mode, int(quirks)))
        np.testing.assert_array_equal(sgm.compute(tl, tr).cpu().numpy(), ref, err_msg=f"uniquenessRatio={ur}")


@pytest.mark.gpu
def test_compute_handle_reuse_across_sizes(gpu, oracle):
    import torch
    from opencv_contrib_amd import cuda
    sgm = cuda.createStereoSGM(-8, 64, 10, 250, 5, 1)
    p = oracle.sgm_params(-8, 64, 10, 250, 5, 1, 1)
    big = synth.stereo_pair(64, 160, seed=12, max_disp=30)[:2]
    small = synth.stereo_pair(13, 15, seed=13, max_disp=10)[:2]
    ref = {id(big): oracle.sgm_compute(*big, p), id(small): oracle.sgm_compute(*small, p)}
    for pair in (big, small, big):
        out = sgm.compute(torch.from_numpy(pair[0]).to(gpu), torch.from_numpy(pair[1]).to(gpu)).cpu().numpy()
        np.testing.assert_array_equal(out, ref[id(pair)])
