"""cv::cuda::DisparityBilateralFilter (first part): HIP vs the CPU restatement, bit-exact (integer output; the
float costs are accumulated in the same order with separately rounded operations on both sides)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opencv_contrib_amd import synth  # noqa: E402


def _case(oracle, h=96, w=160, nd=32, bs=9, seed=3):
    left, right, _ = synth.stereo_pair(h, w, seed=seed, max_disp=nd - 8)
    disp = oracle.sbm_compute(left, right, oracle.sbm_params(num_disparities=nd, block_size=bs))
    return left, disp


# ------------------------------------------------------------------ oracle (CPU)
def test_oracle_flat_map_is_a_fixed_point(oracle):
    """No discontinuity >= edge_disc anywhere: nothing is refined (disparity_bilateral_filter.cu:96)."""
    img = np.random.default_rng(0).integers(0, 256, (40, 50), dtype=np.uint8)
    disp = np.full((40, 50), 17, np.uint8)
    disp[:, 25:] = 18                               # step of 1 < edge_disc = max(1, short(64 * 0.1 + 0.5)) = 6
    np.testing.assert_array_equal(oracle.dbf_apply(disp, img), disp)


def test_oracle_snaps_outlier_to_the_guided_side(oracle):
    """A disparity step that does not coincide with the image edge: pixels between the two are pulled to the side whose
    image intensity they share (the purpose of the joint filter); border rows/cols are never touched (cu:88)."""
    h, w = 21, 40
    img = np.zeros((h, w), np.uint8); img[:, 22:] = 200        # image edge at x = 22
    disp = np.full((h, w), 10, np.uint8); disp[:, 18:] = 40    # disparity edge at x = 18 (4 px too early)
    out = oracle.dbf_apply(disp, img, oracle.dbf_params(ndisp=64, radius=5, iters=4))
    assert (out[5:-5, 18:22] == 10).mean() > 0.5               # mostly pulled back to the left surface
    np.testing.assert_array_equal(out[0], disp[0]); np.testing.assert_array_equal(out[:, 0], disp[:, 0])
    np.testing.assert_array_equal(out[-1], disp[-1]); np.testing.assert_array_equal(out[:, -1], disp[:, -1])


def test_oracle_rejects_bad_arguments(oracle):
    img = np.zeros((8, 8), np.uint8)
    with pytest.raises(ValueError):
        oracle.dbf_apply(np.zeros((8, 8), np.uint8), img, oracle.dbf_params(radius=0))     # CV_Assert 0 < radius_
    with pytest.raises(ValueError):
        oracle.dbf_apply(np.zeros((8, 8), np.float32), img)                                  # disp type
    with pytest.raises(ValueError):
        oracle.dbf_apply(np.zeros((8, 9), np.uint8), img)                                    # size mismatch


# ------------------------------------------------------------------ HIP vs oracle (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.int16])
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("radius,iters", [(3, 1), (5, 2)])
def test_apply_bit_exact(gpu, oracle, dtype, cn, radius, iters):
    import torch
    from opencv_contrib_amd import cuda
    left, disp = _case(oracle)
    disp = disp.astype(dtype)
    if dtype == np.int16:
        disp = (disp.astype(np.int16) * 16)          # fixed-point disparities as StereoSGM / CPU StereoBM produce them
    img = left if cn == 1 else np.stack([left, np.roll(left, 1, 1), np.roll(left, 1, 0)], -1)
    nd = 32 if dtype == np.uint8 else 32 * 16
    f = cuda.createDisparityBilateralFilter(nd, radius, iters)
    assert (f.getNumDisparities(), f.getRadius(), f.getNumIters()) == (nd, radius, iters)
    assert f.getEdgeThreshold() == pytest.approx(0.1) and f.getMaxDiscThreshold() == pytest.approx(0.2) and f.getSigmaRange() == 10.0
    out = f.apply(torch.from_numpy(disp).to(gpu), torch.from_numpy(np.ascontiguousarray(img)).to(gpu)).cpu().numpy()
    ref = oracle.dbf_apply(disp, img, oracle.dbf_params(ndisp=nd, radius=radius, iters=iters))
    assert (ref != disp).sum() > 50                  # the case does exercise the refinement
    np.testing.assert_array_equal(out, ref)


@pytest.mark.gpu
def test_setters_inplace_roi_and_edge_sizes(gpu, oracle):
    import torch
    from opencv_contrib_amd import cuda
    left, disp = _case(oracle, h=67, w=131, seed=9)
    f = cuda.createDisparityBilateralFilter(32, 3, 1)
    f.setSigmaRange(25.0); f.setRadius(4); f.setEdgeThreshold(0.05); f.setMaxDiscThreshold(0.3); f.setNumIters(3)
    p = oracle.dbf_params(ndisp=32, radius=4, iters=3, edge_threshold=0.05, max_disc_threshold=0.3, sigma_range=25.0)
    # pitched ROI views + in-place (dst is disp)
    big_d = torch.zeros((80, 200), dtype=torch.uint8, device=gpu); big_i = torch.zeros((80, 200), dtype=torch.uint8, device=gpu)
    d = big_d[5:72, 30:161]; i = big_i[5:72, 30:161]
    d.copy_(torch.from_numpy(disp)); i.copy_(torch.from_numpy(left))
    out = f.apply(d, i, dst=d)
    np.testing.assert_array_equal(out.cpu().numpy(), oracle.dbf_apply(disp, left, p))
    assert int(big_d[:5].sum()) == 0 and int(big_d[:, :30].sum()) == 0      # nothing written outside the ROI
    # images too small to have interior pixels, and a window larger than the image
    for shape in [(2, 9), (9, 2), (1, 1), (5, 5)]:
        rng = np.random.default_rng(shape[0] * 10 + shape[1])
        dd = rng.integers(0, 32, shape).astype(np.uint8); ii = rng.integers(0, 256, shape).astype(np.uint8)
        o = f.apply(torch.from_numpy(dd).to(gpu), torch.from_numpy(ii).to(gpu)).cpu().numpy()
        np.testing.assert_array_equal(o, oracle.dbf_apply(dd, ii, p))


def _hip_dbf(gpu, disp, img, p):
    import torch
    from opencv_contrib_amd import cuda
    f = cuda.createDisparityBilateralFilter(p.ndisp, p.radius, p.iters)
    f.setEdgeThreshold(p.edge_threshold); f.setMaxDiscThreshold(p.max_disc_threshold); f.setSigmaRange(p.sigma_range)
    return f.apply(torch.from_numpy(disp).to(gpu), torch.from_numpy(np.ascontiguousarray(img)).to(gpu)).cpu().numpy()


def _blocks_case(h=48, w=64, seed=5):
    """Guide: 3 x 3 blocks of 0 / 255; disparity: two surfaces (10 | 40) with a jagged edge (+-3 px per row) and 3 % outliers."""
    rng = np.random.default_rng(seed)
    img = np.kron(rng.integers(0, 2, ((h + 2) // 3, (w + 2) // 3)), np.ones((3, 3), np.int64))[:h, :w].astype(np.uint8) * 255
    edge = w // 2 + rng.integers(-3, 4, h)
    disp = np.where(np.arange(w)[None, :] < edge[:, None], 10, 40).astype(np.uint8)
    out = rng.random((h, w)) < 0.03
    disp[out] = rng.integers(0, 64, (h, w))[out].astype(np.uint8)
    return img, disp, edge


def _edge_pixels_with_distance_255(img, disp, radius=4, edge_disc=6):
    """Interior pixels the first pass may refine (a 4-neighbour differs by >= edge_disc = short(64 * 0.1 + 0.5)) whose
    (2 radius + 1)^2 window holds a guide pixel at colour distance 255 -> (those pixels, those with the distance)."""
    d = disp.astype(int)
    c = d[1:-1, 1:-1]
    is_edge = np.zeros(d.shape, bool)
    is_edge[1:-1, 1:-1] = (np.abs(d[:-2, 1:-1] - c) >= edge_disc) | (np.abs(d[2:, 1:-1] - c) >= edge_disc) | \
                          (np.abs(d[1:-1, :-2] - c) >= edge_disc) | (np.abs(d[1:-1, 2:] - c) >= edge_disc)
    hit = 0
    for y, x in zip(*np.nonzero(is_edge)):
        win = img[max(0, y - radius):y + radius + 1, max(0, x - radius):x + radius + 1].astype(int)
        hit += int(np.abs(win - int(img[y, x])).max() == 255)
    return int(is_edge.sum()), hit


def test_blocks_case_reaches_colour_distance_255():
    img, disp, _ = _blocks_case()
    n, hit = _edge_pixels_with_distance_255(img, disp)
    assert hit >= 100, (n, hit)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.int16])
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("sigma", [10.0, 150.0])
def test_colour_distance_255_bit_exact(gpu, oracle, dtype, cn, sigma):
    """DistRgbMax of a 0 and a 255 pixel is 255; the reference's colour table has 255 entries (it reads one past it: undefined).
    Here the table has 256, entry 255 = exp(-255^2 / (2 sigma^2)): ~0 at sigma 10, 0.236 at sigma 150 -- against the space weight
    stab[0] = 1.0 that a 255-entry table in front of the space table would return."""
    img, disp, _ = _blocks_case()
    assert _edge_pixels_with_distance_255(img, disp)[1] >= 100   # (channel 0 alone; DistRgbMax of three channels is no smaller)
    scale = 1 if dtype == np.uint8 else 16
    disp = (disp.astype(np.int16) * scale).astype(dtype)
    if cn == 3:
        img = np.stack([img, np.roll(img, 3, 1), np.roll(img, 3, 0)], -1)
    p = oracle.dbf_params(ndisp=64 * scale, radius=4, iters=2, sigma_range=sigma)
    ref = oracle.dbf_apply(disp, img, p)
    assert (ref != disp).sum() >= 50
    np.testing.assert_array_equal(_hip_dbf(gpu, disp, img, p), ref)


@pytest.mark.gpu
def test_negative_16bit_disparities_from_sgm(gpu, oracle):
    """StereoSGM with minDisparity -8 marks invalid pixels (-8 - 1) * 16 = -144: the filter's differences are taken on signed values."""
    import torch
    from opencv_contrib_amd import cuda
    left, right, _ = synth.stereo_pair(48, 80, seed=1, max_disp=20)
    ref_d = oracle.sgm_compute(left, right, oracle.sgm_params(min_disparity=-8, num_disparities=64))
    assert (ref_d == -144).any() and (ref_d > 0).any()
    d = cuda.createStereoSGM(-8, 64).compute(torch.from_numpy(left).to(gpu), torch.from_numpy(right).to(gpu))
    np.testing.assert_array_equal(d.cpu().numpy(), ref_d)
    p = oracle.dbf_params(ndisp=1024, radius=3, iters=2)
    f = cuda.createDisparityBilateralFilter(1024, 3, 2)
    out = f.apply(d, torch.from_numpy(left).to(gpu)).cpu().numpy()
    ref = oracle.dbf_apply(ref_d, left, p)
    assert (ref != ref_d).any()
    np.testing.assert_array_equal(out, ref)


@pytest.mark.gpu
def test_thresholds_at_their_ends(gpu, oracle):
    left, disp = _case(oracle, h=40, w=64, seed=4)
    # max_disc_threshold 0: every cost is 0, the first candidate (the pixel itself) wins the strict minimum -> identity
    p = oracle.dbf_params(ndisp=32, radius=3, iters=2, max_disc_threshold=0.0)
    ref = oracle.dbf_apply(disp, left, p)
    np.testing.assert_array_equal(ref, disp)
    np.testing.assert_array_equal(_hip_dbf(gpu, disp, left, p), ref)
    # edge_threshold 0: edge_disc = short(0.5) = 0 is clamped to 1 -> only pixels with a differing 4-neighbour are refined
    p = oracle.dbf_params(ndisp=32, radius=3, iters=2, edge_threshold=0.0)
    ref = oracle.dbf_apply(disp, left, p)
    assert (ref != disp).sum() > 50
    np.testing.assert_array_equal(_hip_dbf(gpu, disp, left, p), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,radius", [((3, 129), 3), ((4, 2), 3), ((12, 20), 1), ((12, 20), 8)])
def test_pair_lane_edge_and_radius_ends(gpu, oracle, shape, radius):
    """A lane owns the pixel pair (2k, 2k + 1) and a workgroup 128 columns: 129 columns leave a pair with one pixel in a second
    workgroup, 2 columns one pair without interior; radius 1 (3 x 3 window) and a window (17 x 17) larger than the 12-row image."""
    rng = np.random.default_rng(shape[1] * 10 + radius)
    disp = np.where(rng.random(shape) < 0.5, 5, 25).astype(np.uint8)
    img = rng.integers(0, 256, shape).astype(np.uint8)
    p = oracle.dbf_params(ndisp=32, radius=radius, iters=2)
    ref = oracle.dbf_apply(disp, img, p)
    if shape[0] > 2 and shape[1] > 2:
        assert (ref != disp).any()
    np.testing.assert_array_equal(_hip_dbf(gpu, disp, img, p), ref)


@pytest.mark.gpu
def test_argument_checks(gpu):
    import torch
    from opencv_contrib_amd import capi, cuda
    f = cuda.createDisparityBilateralFilter(64, 3, 1)
    d = torch.zeros((8, 8), dtype=torch.uint8, device=gpu)
    with pytest.raises(capi.MiError):
        f.apply(d, torch.zeros((8, 9), dtype=torch.uint8, device=gpu))               # disp.size() == img.size()
    with pytest.raises(capi.MiError):
        f.apply(torch.zeros((8, 8), dtype=torch.float32, device=gpu), d)             # disp type
    f.setNumIters(0)
    with pytest.raises(capi.MiError):
        f.apply(d, d)                                                                # 0 < iters_
