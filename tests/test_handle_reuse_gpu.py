"""One handle through a sequence of calls that grow, shrink and switch what it needs of its device scratch, against a FRESH handle with
the same parameters on the same inputs at every step: bit for bit, no tolerance, no oracle.  The scratch of every handle is a set of
grow-only owners (csrc/mi_buf.h) that each call ensures before it uses them; a buffer that arrives late (StereoBM's prefilter planes,
SURF's mask integral), a re-grow between two layouts (the batch stride of StereoBM, BFMatcher's knn / radius partials) or a handle that
goes back to a small frame after a large one must give what a handle that never saw anything else gives.  A TV-L1 handle owns more than
buffers -- per lane an internal stream, events and an arena out of the process-wide cache (csrc/mi_own.h) -- and has the same test over
the calls that create each of them.  StereoSGM and DensePyrLK have
the same test next to their others (test_compute_handle_reuse_across_sizes, test_calc_handle_reuse_across_sizes_and_kernel_templates).
Inputs: the seeded generators of opencv_contrib_amd.synth and seeded random descriptors / points."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opencv_contrib_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu


def T(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def same_bits(a, b, what):
    """Tensors (or tuples of them) equal byte for byte, shapes included."""
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for k, (x, y) in enumerate(zip(a, b)):
            same_bits(x, y, f"{what} [{k}]")
        return
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    x, y = a.contiguous().cpu().numpy(), b.contiguous().cpu().numpy()
    np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=what)


@pytest.mark.parametrize("uniqueness", [0, 10])
def test_stereobm_scratch_follows_size_prefilter_and_batch(gpu, uniqueness):
    """64 x 48 without prefilter; the same with PREFILTER_XSOBEL (lebuf / ribuf arrive late); 128 x 80 with
    PREFILTER_NORMALIZED_RESPONSE; batches of 3 at 64 x 48 and of 5 at 128 x 80 (the per-pair stride changes twice); a single 64 x 48
    again.  uniquenessRatio 10 reads minssd, 0 does not store it."""
    from opencv_contrib_amd import cuda
    small = [synth.stereo_pair(48, 64, seed=100 + k, max_disp=14)[:2] for k in range(3)]
    large = [synth.stereo_pair(80, 128, seed=200 + k, max_disp=14)[:2] for k in range(5)]
    NONE, XSOBEL, NORM = -1, cuda.StereoBM.PREFILTER_XSOBEL, cuda.StereoBM.PREFILTER_NORMALIZED_RESPONSE
    steps = [("64x48", NONE, small[:1]), ("64x48 xsobel", XSOBEL, small[:1]), ("128x80 norm", NORM, large[:1]),
             ("3 x 64x48", NORM, small), ("5 x 128x80", NORM, large), ("64x48 again", NORM, small[:1])]

    def make(prefilter):
        bm = cuda.createStereoBM(16, 5)
        bm.setUniquenessRatio(uniqueness)
        bm.setPreFilterType(prefilter)
        return bm

    def run(bm, pairs):
        ls, rs = [T(p[0], gpu) for p in pairs], [T(p[1], gpu) for p in pairs]
        return bm.compute(ls[0], rs[0]) if len(pairs) == 1 else bm.compute_batch(ls, rs)

    reused = make(NONE)
    for name, prefilter, pairs in steps:
        reused.setPreFilterType(prefilter)
        out = run(reused, pairs)
        assert int((out > 0).sum()) > out.numel() // 20, name   # disparities were found: not an all-zero map on both sides
        same_bits(out, run(make(prefilter), pairs), f"StereoBM uniqueness {uniqueness}, step {name}")


def test_surf_replans_keeps_and_releases_its_scratch(gpu):
    """98 x 124 (the smallest frame test_surf.py detects on, 2 octaves x 2 layers) and 196 x 248: small, large, small; nOctaveLayers
    2 -> 1 (a full re-plan); a lower keypointsRatio (the candidate lists are large enough: scratch kept); a mask (its integral image
    arrives late); releaseMemory() and a detect.  Keypoints and descriptors at every step."""
    from opencv_contrib_amd import cuda
    img_s, img_l = synth.blob_image(98, 124, seed=41), synth.blob_image(196, 248, seed=42)
    mask = np.ones_like(img_s)
    mask[:, :40] = 0

    def make(layers=2, ratio=0.05):
        return cuda.SURF_CUDA.create(20.0, 2, layers, False, ratio, False)

    def run(alg, img, m=None):
        kp, desc = alg.detectWithDescriptors(T(img, gpu), None if m is None else T(m, gpu))
        assert kp.shape[1] >= 1   # (a comparison of two empty sets would say nothing)
        return kp.clone(), desc.clone()

    reused = make()
    for name, img in (("small", img_s), ("large", img_l), ("small again", img_s)):
        same_bits(run(reused, img), run(make(), img), f"SURF {name}")
    reused.nOctaveLayers = 1
    same_bits(run(reused, img_s), run(make(layers=1), img_s), "SURF nOctaveLayers 2 -> 1")
    reused.keypointsRatio = 0.02
    same_bits(run(reused, img_s), run(make(layers=1, ratio=0.02), img_s), "SURF lower keypointsRatio")
    unmasked = run(reused, img_s)[0].shape[1]
    out = run(reused, img_s, mask)
    assert out[0].shape[1] < unmasked   # the mask did exclude keypoints
    same_bits(out, run(make(layers=1, ratio=0.02), img_s, mask), "SURF with a mask")
    reused.releaseMemory()
    same_bits(run(reused, img_s), run(make(layers=1, ratio=0.02), img_s), "SURF after releaseMemory")


def test_farneback_arena_follows_size_and_batch(gpu):
    """Default parameters.  64 x 48, 96 x 64, 64 x 48 (another size: the arena is re-made and carved again); batches of 2, 4 and 1
    pair (it is re-made when the batch grows and kept when it shrinks)."""
    from opencv_contrib_amd import cuda

    def pairs(h, w, n, seed):
        return [tuple(T(a, gpu) for a in synth.flow_pair(h, w, seed=seed + k, dtype="u8")[:2]) for k in range(n)]

    def run(alg, ps):
        if len(ps) == 1:
            return alg.calc(ps[0][0], ps[0][1])
        return alg.calc_batch([p[0] for p in ps], [p[1] for p in ps])

    small, large, batch = pairs(48, 64, 1, 300), pairs(64, 96, 1, 310), pairs(48, 64, 4, 320)
    reused = cuda.FarnebackOpticalFlow.create()
    for name, ps in (("64x48", small), ("96x64", large), ("64x48 again", small), ("batch of 2", batch[:2]), ("batch of 4", batch),
                     ("batch of 1", batch[:1])):
        out = run(reused, ps)
        assert float(out.abs().max()) > 0.1, name
        same_bits(out, run(cuda.FarnebackOpticalFlow.create(), ps), f"Farneback {name}")


def test_tvl1_lanes_events_and_cached_arena_follow_the_calls(gpu):
    """96 x 80 and 160 x 120 (five pyramid levels above the 16-px cut each), 20 iterations.  One handle through: a single pair; a batch
    of 4 (two lanes: the internal stream, the fork and the done event); epsilon 0.01 with host_feedback 1 set through the params struct,
    on the batch of 4 and on a single pair (one lane: the feedback flags in pinned memory and the feedback event); the same two with
    profiling on (the pool of timing events, read through getProfile); the other frame size, single and batch (each lane's arena goes
    back to the cache and another is acquired).  Then the handle is destroyed with its last calc still in flight and a new handle runs
    the batch of 4 of the first geometry -- on the blocks, with their idle events, that the cache just took -- and
    release_cached_memory() returns."""
    from opencv_contrib_amd import cuda

    def pairs(h, w, n, seed):
        return [tuple(T(a, gpu) for a in synth.flow_pair(h, w, seed=seed + k)[:2]) for k in range(n)]

    def make(epsilon=0.0, fb=0):
        return cuda.OpticalFlowDual_TVL1.create(iterations=20, epsilon=epsilon, hostFeedback=fb)

    def run(alg, ps):
        if len(ps) == 1:
            return alg.calc(ps[0][0], ps[0][1])
        return alg.calc_batch([p[0] for p in ps], [p[1] for p in ps])

    small, large = pairs(80, 96, 4, 800), pairs(120, 160, 4, 810)
    reused = make()
    first_batch = None
    for name, eps, fb, prof, ps in (("96x80", 0.0, 0, False, small[:1]), ("4 x 96x80", 0.0, 0, False, small),
                                    ("4 x 96x80, epsilon", 0.01, 1, False, small), ("96x80, epsilon + host feedback", 0.01, 1, False, small[:1]),
                                    ("4 x 96x80, profiling", 0.01, 1, True, small), ("96x80, profiling", 0.01, 1, True, small[:1]),
                                    ("160x120", 0.01, 1, True, large[:1]), ("4 x 160x120", 0.01, 1, True, large)):
        reused._set(epsilon=eps, host_feedback=fb)
        reused.setProfiling(prof)
        out = run(reused, ps)
        assert float(out.abs().max()) > 0.1, name
        fresh = run(make(eps, fb), ps)
        same_bits(out, fresh, f"TV-L1 {name}")
        if prof:
            ms, launches, _ = reused.getProfile()
            assert ms > 0.0 and launches > 0, name
        if first_batch is None and len(ps) == 4:
            first_batch = fresh.clone()
    reused.__del__()   # mi_tvl1_destroy, behind the 160 x 120 batch it has just enqueued
    again = make()
    same_bits(run(again, small), first_batch, "TV-L1 4 x 96x80 on a new handle after the destroy")
    again.__del__()
    cuda.release_cached_memory()


def test_bfmatcher_partials_follow_size_and_layout(gpu):
    """L2, d = 64: knnMatch k = 2 of 70 x 100 descriptors, of 300 x 900, a radiusMatch (the same buffer as [segment][query] counts), the
    first again."""
    from opencv_contrib_amd import cuda
    rng = np.random.default_rng(400)
    q1, t1 = (T(rng.standard_normal((n, 64)).astype(np.float32), gpu) for n in (70, 100))
    q2, t2 = (T(rng.standard_normal((n, 64)).astype(np.float32), gpu) for n in (300, 900))
    radius = 10.5   # a little under the typical distance of two such descriptors (sqrt(2 * 64) = 11.3): some hits, far from all

    def knn(m, q, t):
        return m.knnMatchDevice(q, t, k=2)

    def rad(m, q, t):
        return m.radiusMatchDevice(q, t, radius)

    reused = cuda.createBFMatcher(cuda.BFMatcher.NORM_L2)
    for name, fn, q, t in (("knn 70 x 100", knn, q1, t1), ("knn 300 x 900", knn, q2, t2), ("radius 300 x 900", rad, q2, t2),
                           ("radius 70 x 100", rad, q1, t1), ("knn 70 x 100 again", knn, q1, t1)):
        out = fn(reused, q, t)
        if fn is rad:
            n = out[3].cpu().numpy()
            assert n.max() > 0 and n.min() < t.shape[0], name
        same_bits(out, fn(cuda.createBFMatcher(cuda.BFMatcher.NORM_L2), q, t), f"BFMatcher {name}")


def test_sparse_pyrlk_pyramid_scratch_appears_and_goes_unused(gpu):
    """maxLevel 0 (no scratch at all: the handle's buffer stays empty), maxLevel 3 at 96 x 64 and at 160 x 120, maxLevel 0 again."""
    from opencv_contrib_amd import cuda
    rng = np.random.default_rng(500)

    def case(h, w, seed):
        I0, I1, _ = synth.flow_pair(h, w, seed=seed, dtype="u8")
        pts = np.stack([rng.uniform(8, w - 8, 40), rng.uniform(8, h - 8, 40)], -1).astype(np.float32)
        return T(I0, gpu), T(I1, gpu), T(pts, gpu)

    small, large = case(64, 96, 501), case(120, 160, 502)
    reused = cuda.SparsePyrLKOpticalFlow.create(maxLevel=0)
    for name, level, c in (("level 0", 0, small), ("level 3, 96x64", 3, small), ("level 3, 160x120", 3, large), ("level 0 again", 0, small)):
        reused.setMaxLevel(level)
        out = reused.calc(*c)
        assert int(out[1].sum()) > 10, name   # most points tracked
        same_bits(out, cuda.SparsePyrLKOpticalFlow.create(maxLevel=level).calc(*c), f"SparsePyrLK {name}")


def test_btvl1_arena_follows_the_frame_size(gpu):
    """Scale 2, one channel, 3 frames: 16 x 12, 24 x 16, 16 x 12."""
    from test_btvl1_gpu import gpu_motions, make_alg, make_case, to_gpu

    def args(seed, lh, lw):
        frames, fwd, bwd = make_case(seed, lh, lw, 1, 3, amp=2.0)
        return [to_gpu(gpu, f) for f in frames], gpu_motions(gpu, fwd), gpu_motions(gpu, bwd), 1

    small, large = args(600, 12, 16), args(601, 16, 24)
    reused = make_alg(scale=2)
    for name, a in (("16x12", small), ("24x16", large), ("16x12 again", small)):
        out = reused.process(*a).clone()
        assert bool(out.isfinite().all()) and float(out.std()) > 1.0, name
        same_bits(out, make_alg(scale=2).process(*a), f"BTV-L1 {name}")


def test_dbf_table_follows_radius_and_sigma(gpu):
    """8-bit disparity at 64 x 48: radius 2 -> 5 -> 2 with a sigmaRange change in between (the table is rebuilt on every change and
    only then)."""
    from opencv_contrib_amd import cuda
    left, right, _ = synth.stereo_pair(48, 64, seed=700, max_disp=30)
    disp = cuda.createStereoBM(32, 7).compute(T(left, gpu), T(right, gpu))
    img = T(left, gpu)

    def make(radius, sigma):
        f = cuda.createDisparityBilateralFilter(32, radius, 2)
        f.setSigmaRange(sigma)
        return f

    reused = make(2, 10.0)
    changed = 0
    for radius, sigma in ((2, 10.0), (5, 10.0), (5, 40.0), (2, 40.0), (2, 10.0)):
        reused.setRadius(radius)
        reused.setSigmaRange(sigma)
        out = reused.apply(disp, img)
        changed += int((out != disp).sum())
        same_bits(out, make(radius, sigma).apply(disp, img), f"DBF radius {radius} sigma {sigma}")
    assert changed > 50   # the filter did refine the map
