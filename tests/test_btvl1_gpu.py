"""BTV-L1 super-resolution on the GPU (mi_btvl1_*, opencv_contrib_amd.superres.BTVL1_CUDA) against the NumPy float32 restatement of
the reference (tests/btvl1_numpy_ref.py), BIT FOR BIT: every value is a fixed sequence of separately rounded f32 operations (the
only nonlinearity is a comparison), so there is no tolerance anywhere in this file.  Comparisons are on VALUES (a != b counts the
differing elements, so +0 equals -0: the fused update skips taps that add a signed zero, see csrc/btvl1_kernels.hip); a real
mismatch flips a sign sample and shows up as a difference of order tau, never of an ulp.

The restatement is itself pinned, bit for bit, on the reference's own kernels and class executed on the host
(tests/test_ref_pin_btvl1.py, which imports CASES and BAD_PARAMS from here), and tests/test_ref_class_gpu.py compares the product with
that reference class directly.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import btvl1_numpy_ref as R  # noqa: E402

F = np.float32


def make_case(seed, lh, lw, cn, K, amp=6.0):
    """Random frames in 0 .. 255 and motions = a constant per frame + an expansion about the centre + noise: with `amp` low-res pixels
    per frame step the accumulated maps leave the image on every side."""
    rng = np.random.default_rng(seed)
    shape = (lh, lw) if cn == 1 else (lh, lw, cn)
    frames = [rng.uniform(0, 255, shape).astype(F) for _ in range(K)]
    yy, xx = np.mgrid[0:lh, 0:lw].astype(F)

    def motion():
        cx, cy = rng.uniform(-amp, amp, 2)
        e = rng.uniform(-0.4, 0.4)
        mx = cx + e * (xx - lw / 2) + rng.uniform(-1.5, 1.5, (lh, lw))
        my = cy + e * (yy - lh / 2) + rng.uniform(-1.5, 1.5, (lh, lw))
        return mx.astype(F), my.astype(F)

    fwd = [motion() if i < K - 1 else None for i in range(K)]
    bwd = [motion() if i > 0 else None for i in range(K)]
    return frames, fwd, bwd


def to_gpu(gpu, a, pitched=False):
    """CUDA tensor of array a; pitched: a view into a wider buffer (step > cols * elemSize) whose padding is NaN."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    if not pitched:
        return t
    pad = (t.shape[0], t.shape[1] + 5) + tuple(t.shape[2:])
    buf = torch.full(pad, float("nan"), dtype=t.dtype, device=gpu)
    view = buf[:, :t.shape[1]]
    view.copy_(t)
    return view


def gpu_motions(gpu, motions, pitched=False):
    return [None if m is None else (to_gpu(gpu, m[0], pitched), to_gpu(gpu, m[1], pitched)) for m in motions]


def make_alg(**kw):
    from opencv_contrib_amd import superres
    alg = superres.createSuperResolution_BTVL1_CUDA()
    names = dict(scale="Scale", iterations="Iterations", tau="Tau", lambda_="Lambda", alpha="Alpha", btv_kernel_size="KernelSize",
                 blur_kernel_size="BlurKernelSize", blur_sigma="BlurSigma")
    for k, v in kw.items():
        getattr(alg, "set" + names[k])(v)
    return alg


def run_both(gpu, seed, lh, lw, cn, K, base, pitched=False, amp=6.0, **kw):
    import torch
    frames, fwd, bwd = make_case(seed, lh, lw, cn, K, amp)
    ref = R.process(frames, fwd, bwd, base, **kw)
    alg = make_alg(**kw)
    out = alg.process([to_gpu(gpu, f, pitched) for f in frames], gpu_motions(gpu, fwd, pitched), gpu_motions(gpu, bwd, pitched), base)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert out.shape == ref.shape and np.isfinite(out).all()
    ndiff = int((out != ref).sum())
    print(f"btvl1 seed {seed} {lh}x{lw}x{cn} K {K} base {base} {kw}: {ndiff} of {ref.size} values differ, max |d| "
          f"{float(np.abs(out - ref).max()):.3g}")
    return ndiff


@pytest.mark.gpu
@pytest.mark.parametrize("cn,scale,K,base", [(1, 2, 3, 1), (3, 3, 5, 0), (4, 4, 5, 4), (1, 3, 1, 0), (1, 4, 3, 2)])
def test_stage_maps_initial_estimate_and_tables(gpu, cn, scale, K, base):
    """mi_btvl1_stage: relative motions -> the four high-res map planes of every frame, the cubic initial estimate, and the blur taps /
    BTV weights the handle hands to its kernels (host exp / pow), each equal to the restatement."""
    import torch
    frames, fwd, bwd = make_case(100 + cn + scale, 37, 53, cn, K)
    kw = dict(scale=scale, blur_kernel_size=9, blur_sigma=1.2, btv_kernel_size=7, alpha=0.7)
    alg = make_alg(**kw)
    maps, init, taps, weights = alg.stage([to_gpu(gpu, f) for f in frames], gpu_motions(gpu, fwd), gpu_motions(gpu, bwd), base)
    torch.cuda.synchronize()
    fmaps, bmaps, rinit = R.stage(frames, fwd, bwd, base, dict(R.DEFAULTS, **kw))
    for k in range(K):
        got = [m.cpu().numpy() for m in maps[k]]
        want = [fmaps[k][0], fmaps[k][1], bmaps[k][0], bmaps[k][1]]
        for name, g, w in zip(("forwardMap x", "forwardMap y", "backwardMap x", "backwardMap y"), got, want):
            assert int((g != w).sum()) == 0, (k, name, int((g != w).sum()), float(np.abs(g - w).max()))
    # the maps of the five-frame cases leave the image on every side (they exercise the replicate clamp)
    allx = np.stack([bmaps[k][0] for k in range(K)] + [fmaps[k][0] for k in range(K)])
    ally = np.stack([bmaps[k][1] for k in range(K)] + [fmaps[k][1] for k in range(K)])
    if K == 5:
        assert allx.min() < -1 and allx.max() > 53 * scale and ally.min() < -1 and ally.max() > 37 * scale
    gi = init.cpu().numpy()
    assert int((gi != rinit).sum()) == 0, (int((gi != rinit).sum()), float(np.abs(gi - rinit).max()))
    rt, rw = R.gaussian_kernel(9, 1.2), R.btv_weights(7, 0.7)
    assert np.array_equal(np.array(taps[:9], F), rt) and not any(taps[9:])
    assert np.array_equal(np.array(weights[:len(rw)], F), rw) and not any(weights[len(rw):])
    # the fixed small tables (sigma 0, odd size <= 7) and the computed sigma of a larger kernel
    for n, sigma in ((5, 0.0), (9, 0.0), (3, 1.2)):
        alg.setBlurKernelSize(n)
        alg.setBlurSigma(sigma)
        taps = alg.stage([to_gpu(gpu, f) for f in frames], gpu_motions(gpu, fwd), gpu_motions(gpu, bwd), base)[2]
        assert np.array_equal(np.array(taps[:n], F), R.gaussian_kernel(n, sigma)), (n, sigma)


CASES = [
    # seed, lh, lw, cn, K, base, pitched, parameters
    (1, 37, 53, 1, 3, 1, False, dict(scale=2, iterations=1)),
    (2, 37, 53, 1, 3, 1, False, dict(scale=2, iterations=2)),
    (3, 37, 53, 1, 3, 1, False, dict(scale=2, iterations=7)),
    (4, 37, 53, 3, 5, 0, False, dict(scale=3, iterations=7)),
    (5, 37, 53, 4, 5, 4, False, dict(scale=4, iterations=7)),
    (6, 37, 53, 1, 5, 2, True, dict(scale=4, iterations=7)),
    (7, 37, 53, 3, 3, 2, True, dict(scale=2, iterations=7)),
    (8, 37, 53, 1, 1, 0, False, dict(scale=3, iterations=7)),
    (9, 37, 53, 4, 1, 0, True, dict(scale=2, iterations=7)),
    (10, 37, 53, 1, 3, 0, False, dict(scale=4, iterations=7, lambda_=0.0)),
    (11, 37, 53, 3, 3, 1, False, dict(scale=3, iterations=7, btv_kernel_size=1)),
    (12, 37, 53, 1, 5, 3, False, dict(scale=2, iterations=7, btv_kernel_size=3)),
    (13, 37, 53, 4, 3, 1, False, dict(scale=4, iterations=7, btv_kernel_size=7, blur_kernel_size=3)),
    (14, 37, 53, 1, 3, 2, False, dict(scale=3, iterations=7, blur_kernel_size=9)),
    (15, 37, 53, 1, 3, 0, False, dict(scale=2, iterations=7, blur_kernel_size=9, blur_sigma=1.2)),
    (16, 37, 53, 3, 5, 2, False, dict(scale=4, iterations=7, blur_kernel_size=3, blur_sigma=1.2)),
    (17, 37, 53, 1, 5, 4, False, dict(scale=3, iterations=7, blur_kernel_size=5, blur_sigma=1.2)),
    (18, 24, 32, 1, 3, 1, False, dict(scale=2, iterations=7, btv_kernel_size=16, blur_kernel_size=31, blur_sigma=0.0)),
    (19, 64, 96, 1, 5, 2, False, dict(scale=4, iterations=7, tau=0.9, alpha=0.55, lambda_=0.1)),
    (20, 9, 11, 1, 3, 1, False, dict(scale=2, iterations=2, btv_kernel_size=2, blur_kernel_size=31)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[f"s{c[0]}_{c[1]}x{c[2]}x{c[3]}_K{c[4]}b{c[5]}{'_pitched' if c[6] else ''}_"
                                              + "_".join(f"{k}{v}" for k, v in c[7].items()) for c in CASES])
def test_process_bit_exact(gpu, case):
    """process after 1, 2 and 7 iterations; CN 1 / 3 / 4; scale 2 / 3 / 4; K 1 / 3 / 5 with the base first, in the middle and last;
    sizes that are no multiple of any tile; pitched inputs; lambda = 0; btvKernelSize 1 / 3 / 7 (and 2, 16); blurKernelSize 3 / 5 /
    9 (and 31) with blurSigma 0 and 1.2; motions that take the maps out of the image on every side.  0 differing values."""
    seed, lh, lw, cn, K, base, pitched, kw = case
    assert run_both(gpu, seed, lh, lw, cn, K, base, pitched, **kw) == 0


@pytest.mark.gpu
def test_random_sweep_bit_exact(gpu):
    """24 seeded random configurations over the same ranges."""
    rng = np.random.default_rng(2024)
    total = 0
    for n in range(24):
        cn = int(rng.choice([1, 3, 4]))
        K = int(rng.choice([1, 2, 3, 5]))
        kw = dict(scale=int(rng.choice([2, 3, 4])), iterations=int(rng.choice([1, 2, 3, 7])), lambda_=float(rng.choice([0.0, 0.03, 0.2])),
                  tau=float(rng.choice([0.7, 1.3])), alpha=float(rng.choice([0.7, 0.4])),
                  btv_kernel_size=int(rng.choice([1, 3, 4, 7, 9])), blur_kernel_size=int(rng.choice([1, 3, 5, 9, 13])),
                  blur_sigma=float(rng.choice([0.0, 1.2, 2.5])))
        lh, lw = int(rng.integers(12, 60)), int(rng.integers(12, 70))
        total += run_both(gpu, 5000 + n, lh, lw, cn, K, int(rng.integers(0, K)), bool(rng.integers(0, 2)), amp=float(rng.choice([0.5, 6.0])), **kw)
    assert total == 0


@pytest.mark.gpu
def test_no_scratch_plane_is_read_before_it_is_written(gpu):
    """The handle's arena filled with NaNs (miflow_selftest_btvl1_poison) between two process calls of the same geometry, and between
    calls of different geometries (a smaller one inside the larger arena, then growth): the same bytes out."""
    import torch
    from opencv_contrib_amd import capi
    alg = make_alg(scale=2, iterations=5)

    def run(seed, lh, lw, cn, K, base):
        frames, fwd, bwd = make_case(seed, lh, lw, cn, K)
        out = alg.process([to_gpu(gpu, f) for f in frames], gpu_motions(gpu, fwd), gpu_motions(gpu, bwd), base)
        torch.cuda.synchronize()
        return out.clone()

    def poison():
        capi.check(capi.lib().miflow_selftest_btvl1_poison(alg._h, capi.current_stream_ptr()))

    geos = [(1, 37, 53, 3, 5, 2), (2, 20, 31, 1, 3, 0), (3, 48, 70, 4, 5, 4)]
    first = [run(*g) for g in geos]
    for g, a in zip(geos + geos[::-1], first + first[::-1]):
        poison()
        b = run(*g)
        assert torch.isfinite(b).all()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), g


@pytest.mark.gpu
def test_two_handles_on_two_streams_share_no_state(gpu):
    """Two handles with different parameters (blur taps, BTV weights, geometry) enqueued on two streams at the same time give the bytes of
    their sequential runs: the tables travel in the kernel arguments, there is no __constant__ or global state."""
    import torch
    cfg = [(dict(scale=2, iterations=40, blur_kernel_size=5, alpha=0.7, btv_kernel_size=7), (21, 60, 80, 1, 5, 2)),
           (dict(scale=3, iterations=40, blur_kernel_size=9, blur_sigma=1.2, alpha=0.4, btv_kernel_size=3), (22, 45, 64, 3, 3, 0))]
    algs = [make_alg(**kw) for kw, _ in cfg]
    args = []
    for _, (seed, lh, lw, cn, K, base) in cfg:
        frames, fwd, bwd = make_case(seed, lh, lw, cn, K)
        args.append(([to_gpu(gpu, f) for f in frames], gpu_motions(gpu, fwd), gpu_motions(gpu, bwd), base))
    seq = [alg.process(*a).clone() for alg, a in zip(algs, args)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)]
    for rep in range(3):
        outs = []
        for alg, a, st in zip(algs, args, streams):
            with torch.cuda.stream(st):
                outs.append(alg.process(*a))
        torch.cuda.synchronize()
        for s, o in zip(seq, outs):
            assert torch.equal(s.view(torch.int32), o.view(torch.int32)), rep


@pytest.mark.gpu
def test_two_launches_per_iteration_whatever_the_window(gpu):
    """mi_btvl1_get_profile: 2 * iterations + 3 launches per process (relative motions, maps, initial estimate) for K = 1, 3 and 9."""
    counts = {}
    for K in (1, 3, 9):
        for it in (4, 11):
            frames, fwd, bwd = make_case(30 + K, 24, 40, 1, K, amp=1.0)
            alg = make_alg(scale=2, iterations=it)
            alg.process([to_gpu(gpu, f) for f in frames], gpu_motions(gpu, fwd), gpu_motions(gpu, bwd), K // 2)
            ms, launches = alg.getProfile()
            assert ms > 0
            counts[(K, it)] = launches - 2 * it
    print("btvl1 launches beyond 2 * iterations:", counts)
    assert set(counts.values()) == {3}, counts


# the parameter sets the reference's CV_Asserts reject, with the status code each maps to (tests/test_ref_pin_btvl1.py holds the
# reference class itself to this list)
BAD_PARAMS = ((dict(scale=1), -1), (dict(iterations=0), -1), (dict(tau=0.0), -1), (dict(alpha=0.0), -1), (dict(btv_kernel_size=0), -1),
              (dict(btv_kernel_size=17), -1), (dict(blur_kernel_size=4), -1), (dict(blur_kernel_size=33), -1), (dict(blur_sigma=-1.0), -1))


@pytest.mark.gpu
def test_argument_checks(gpu):
    """The reference's CV_Asserts (btv_l1_cuda.cpp:310-316, filtering.cpp:441,568) as status codes, before any launch."""
    from opencv_contrib_amd import capi
    frames, fwd, bwd = make_case(1, 16, 16, 1, 3)
    gf, gw, gb = [to_gpu(gpu, f) for f in frames], gpu_motions(gpu, fwd), gpu_motions(gpu, bwd)
    for kw, code in BAD_PARAMS:
        with pytest.raises(capi.MiError) as ei:
            make_alg(**kw).process(gf, gw, gb, 1)
        assert ei.value.code == code, kw
    with pytest.raises(capi.MiError) as ei:
        make_alg().process(gf, gw, gb, 3)
    assert ei.value.code == -1
    with pytest.raises(capi.MiError) as ei:
        make_alg().process([gf[0], gf[1][:8], gf[2]], gw, gb, 1)
    assert ei.value.code == -3
    with pytest.raises(capi.MiError) as ei:
        make_alg().process([g.to(dtype=__import__("torch").uint8) for g in gf], gw, gb, 1)
    assert ei.value.code == -2


# ---------------------------------------------------------------------------------------------------------------- the full class
class RecordingFlow:
    """Wraps a flow adapter and keeps every (u, v) it returns, in call order."""

    def __init__(self, inner):
        self.inner, self.log = inner, []

    def calc(self, a, b):
        u, v = self.inner.calc(a, b)
        self.log.append((u.cpu().numpy().copy(), v.cpu().numpy().copy()))
        return u, v

    def collectGarbage(self):
        self.inner.collectGarbage()


@pytest.mark.gpu
def test_class_equals_restatement_on_its_own_flows_and_ends_after_12_frames(gpu):
    """The whole class over a list-backed source of 12 frames, radius 2, Farneback flow: (a) every output equals the restatement's ring
    driver fed the SAME GPU flows, bit for bit; (b) the 13th nextFrame returns None, and again after reset()."""
    import torch
    from opencv_contrib_amd import superres
    _, low, _ = R.synthetic_sequence(7, n=12, hh=96, hw=128, scale=2)
    alg = make_alg(scale=2, iterations=6)
    alg.setTemporalAreaRadius(2)
    rec = RecordingFlow(superres.createOptFlow_Farneback_CUDA())
    alg.setOpticalFlow(rec)
    alg.setInput(superres.createFrameSource_List([torch.from_numpy(f).to(gpu) for f in low]))
    outs = []
    while True:
        o = alg.nextFrame()
        if o is None:
            break
        assert o.dtype == torch.uint8 and o.is_cuda
        outs.append(o.cpu().numpy())
        assert len(outs) <= 12
    assert len(outs) == 12 and alg.nextFrame() is None
    log = list(rec.log)
    assert len(log) == 22
    ref = R.BTVL1(R.ListSource(low), lambda a, b: log.pop(0), scale=2, iterations=6, temporal_area_radius=2)
    for i in range(12):
        r = ref.nextFrame()
        assert r is not None and int((r != outs[i]).sum()) == 0, (i, int((r != outs[i]).sum()))
    assert ref.nextFrame() is None
    alg.reset()
    again = [alg.nextFrame() for _ in range(13)]
    assert again[12] is None and all(np.array_equal(a.cpu().numpy(), o) for a, o in zip(again[:12], outs))
    # an empty source yields nothing
    alg.setInput(superres.createFrameSource_Empty())
    assert alg.nextFrame() is None


@pytest.mark.gpu
def test_acceptance_criterion_with_the_products_own_flows(gpu):
    """The reference's acceptance test (superres/test/test_superres.cpp:223-274) on the synthetic sequence: scale 2, 100 iterations,
    radius 2, Farneback flows computed by the product on the degraded frames.  Mean MSSIM against the undegraded frames >= 0.5 (the
    reference's threshold, :273) and better than the cubic upscale of the degraded frames.
    Measured on MI355X: mean MSSIM 0.8215 (minimum over the 12 frames 0.8162), cubic upscale 0.7095; the values of the analytic-motion
    restatement are in tests/test_btvl1_ref.py."""
    import torch
    from opencv_contrib_amd import superres
    gold, low, _ = R.synthetic_sequence(0, n=12)
    alg = superres.createSuperResolution_BTVL1_CUDA()
    alg.setScale(2)
    alg.setIterations(100)
    alg.setTemporalAreaRadius(2)
    alg.setInput(superres.createFrameSource_List([torch.from_numpy(f).to(gpu) for f in low]))
    b = alg.getKernelSize()
    sr, cub = [], []
    for i in range(12):
        o = alg.nextFrame()
        assert o is not None
        g = gold[i][b:-b, b:-b]
        sr.append(R.mssim(g, o.cpu().numpy()))
        cub.append(R.mssim(g, R.saturate_u8(R.resize_cubic(low[i].astype(F), *gold[i].shape))[b:-b, b:-b]))
    print(f"btvl1 acceptance, Farneback flows: mean MSSIM {np.mean(sr):.4f} (min {min(sr):.4f}), cubic upscale {np.mean(cub):.4f}")
    assert np.mean(sr) >= 0.5
    assert np.mean(sr) > np.mean(cub)


@pytest.mark.gpu
def test_cpp_shim_matches_python_mirror(gpu, tmp_path):
    """include/opencv2/superres.hpp and opencv_contrib_amd.superres bind the same C-ABI: the same sequence through both (Farneback
    flows, radius 2) gives the same bytes, frame by frame, and both stop after the last frame."""
    import struct
    import subprocess
    import torch
    from opencv_contrib_amd import superres
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "opencv_contrib_amd")
    exe = str(tmp_path / "superres_shim")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "superres_shim.cpp"),
                        "-o", exe, "-L" + libdir, "-lmiflow", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    _, low, _ = R.synthetic_sequence(5, n=7, hh=96, hw=128, scale=2)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("6i", 7, 48, 64, 2, 9, 2))
        for a in low:
            f.write(a.tobytes())
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = open(fout, "rb").read()
    count, orows, ocols = struct.unpack("3i", raw[:12])
    assert (count, orows, ocols) == (7, 96 - 14, 128 - 14)
    got = np.frombuffer(raw[12:], np.uint8).reshape(count, orows, ocols)
    alg = make_alg(scale=2, iterations=9)
    alg.setTemporalAreaRadius(2)
    alg.setInput(superres.createFrameSource_List([torch.from_numpy(a).to(gpu) for a in low]))
    for i in range(7):
        np.testing.assert_array_equal(alg.nextFrame().cpu().numpy(), got[i])
    assert alg.nextFrame() is None
