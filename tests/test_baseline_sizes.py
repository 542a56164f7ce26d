"""Parity at the sizes BASELINE.json quotes: HIP through the C-ABI against the oracle on the same seeded inputs.

  configs[1]  TV-L1 1920x1080, CV_32FC1 and CV_8UC1, iterations = 10 (the reference's accuracy-test setting,
              cudaoptflow/test/test_optflow.cpp:450): what a default-constructed object runs (fast math, fused iterations)
              and exact math against oracle.tvl1_calc; tolerance stated per test (the reference's own is |1 - CCORR| <= 4e-3,
              test_optflow.cpp:465);
  configs[2]  StereoBM 1920x1080, 128 disparities, block 15: bit-exact;
  configs[3]  SURF 3840x2160, threshold 400: keypoint count, keypoints, >= 99 % of orientations / descriptors;
  configs[4]  a 64-pair calc_batch (one GPU's share of the 512 pairs) equals 64 single calcs bit for bit.
Also here: the kernels a default calc() is made of that round 2 added (fused-gradient warp, two-lane batches).
"""
import numpy as np
import os

import pytest

from opencv_contrib_amd import synth

pytestmark = pytest.mark.gpu


def T(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def N(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ TV-L1, configs[1]
@pytest.fixture(scope="module")
def pair1080(oracle):
    out = {}
    for dt in ("f32", "u8"):
        I0, I1, gt = synth.flow_pair(1080, 1920, seed=1234, dtype=dt)
        ref = oracle.tvl1_calc(I0, I1, oracle.tvl1_params(iterations=10, epsilon=0.0))
        out[dt] = (I0, I1, gt, ref)
    return out


def test_default_object_runs_cpu_class_arithmetic_in_fast_math(gpu):
    from opencv_contrib_amd import capi, cuda
    alg = cuda.OpticalFlowDual_TVL1.create()
    assert (alg._p.semantics, alg._p.exact_math, alg._p.time_block, alg._p.lanes) == (capi.MI_SEM_CPU_REF, 0, 0, 0)
    assert (alg.getNumIterations(), alg.getEpsilon(), alg.getNumScales(), alg.getNumWarps()) == (300, 0.01, 5, 5)


@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("exact", [False, True], ids=["default_fast_fused", "exact_math"])
def test_tvl1_1080p_against_oracle(gpu, pair1080, dtype, exact):
    from opencv_contrib_amd import cuda
    I0, I1, gt, ref = pair1080[dtype]
    alg = cuda.OpticalFlowDual_TVL1.create(iterations=10, epsilon=0.0, exactMath=exact)
    flow = N(alg.calc(T(I0, gpu), T(I1, gpu)))
    assert np.isfinite(flow).all()
    d = np.sqrt(((flow - ref) ** 2).sum(-1))
    # exact math: the same separately rounded operations as the oracle (order of the error-free parts only);
    # default: v_rcp / v_sqrt / fma and 10 iterations per HBM pass
    assert d.mean() <= (2e-3 if exact else 5e-3), d.mean()
    assert synth.ccorr_dissimilarity(flow, ref) <= 1e-4       # the reference accepts 4e-3 (test_optflow.cpp:465)
    assert (d <= 0.02).mean() >= 0.99
    assert synth.epe(flow, gt) < 0.15                          # and it is a flow: analytic field of the generator


def test_tvl1_1080p_cuda_semantics_against_its_oracle(gpu, oracle):
    """MI_SEM_CUDA_COMPAT at the BASELINE size against the oracle of the same semantics -- the one pinned bit for bit on
    the reference's own OpenCL kernels (tests/test_ref_pin.py)."""
    from opencv_contrib_amd import cuda
    I0, I1, gt = synth.flow_pair(1080, 1920, seed=1234)
    ref = oracle.tvl1_calc(I0, I1, oracle.tvl1_params(iterations=10, epsilon=0.0, semantics=1))
    flow = N(cuda.OpticalFlowDual_TVL1.create(iterations=10, epsilon=0.0, semantics=1).calc(T(I0, gpu), T(I1, gpu)))
    d = np.sqrt(((flow - ref) ** 2).sum(-1))
    assert d.mean() <= 5e-3, d.mean()
    assert synth.ccorr_dissimilarity(flow, ref) <= 1e-4


@pytest.mark.parametrize("sem", [0, 1], ids=["cpu_class", "cuda_class"])
def test_tvl1_1080p_gamma1_against_oracle(gpu, oracle, sem):
    """The other half of the reference's TV-L1 test matrix -- Gamma(1.0), cudaoptflow/test/test_optflow.cpp:451,530-532 -- at the
    BASELINE size on the path a default-constructed object runs since round 6: the blocked kernel with the illumination channel
    (k_iterate_tbr GAM; tvl1flow.cu:209-288 u3 terms, :313-348 p31 / p32).  A brightness change between the frames exercises u3."""
    from opencv_contrib_amd import cuda
    I0, I1, gt = synth.flow_pair(1080, 1920, seed=1234)
    I1 = np.clip(I1 * 1.05 + 0.02, 0, 1).astype(np.float32)
    ref = oracle.tvl1_calc(I0, I1, oracle.tvl1_params(iterations=10, epsilon=0.0, gamma=1.0, semantics=sem))
    ref0 = oracle.tvl1_calc(I0, I1, oracle.tvl1_params(iterations=10, epsilon=0.0, gamma=0.0, semantics=sem))
    assert np.sqrt(((ref - ref0) ** 2).sum(-1)).mean() > 1e-2, "gamma has no effect on this input"
    flow = N(cuda.OpticalFlowDual_TVL1.create(iterations=10, epsilon=0.0, gamma=1.0, semantics=sem).calc(T(I0, gpu), T(I1, gpu)))
    assert np.isfinite(flow).all()
    d = np.sqrt(((flow - ref) ** 2).sum(-1))
    assert d.mean() <= 5e-3, d.mean()
    assert synth.ccorr_dissimilarity(flow, ref) <= 1e-4       # the reference accepts 4e-3 (test_optflow.cpp:465)
    assert (d <= 0.02).mean() >= 0.985
    # gamma = 1 with the illumination change modelled recovers the analytic field better than gamma = 0 does on the same frames
    assert synth.epe(flow, gt) < synth.epe(ref0, gt) + 0.02


def test_tvl1_batch_of_64_equals_64_single_calcs(gpu):
    """configs[4]: one GPU's share of the 512-pair batch.  64 distinct 1080p pairs (4 generated pairs under flips and rolls)
    through ONE calc_batch (two internal lanes of 32) against 64 calc() calls of another object: bit-identical flows."""
    import torch
    from opencv_contrib_amd import cuda
    base = [synth.flow_pair(1080, 1920, seed=1000 + k)[:2] for k in range(4)]
    I0s, I1s = [], []
    for k in range(64):
        a, b = (T(x, gpu) for x in base[k % 4])
        v = k // 4
        if v & 1: a, b = a.flip(0), b.flip(0)
        if v & 2: a, b = a.flip(1), b.flip(1)
        s = (v >> 2) * 37
        I0s.append(torch.roll(a, s, 1).contiguous()); I1s.append(torch.roll(b, s, 1).contiguous())
    alg = cuda.OpticalFlowDual_TVL1.create(iterations=10, epsilon=0.0)
    flows = alg.calc_batch(I0s, I1s)
    torch.cuda.synchronize()
    single = cuda.OpticalFlowDual_TVL1.create(iterations=10, epsilon=0.0)
    for k in range(64):
        f = single.calc(I0s[k], I1s[k])
        assert torch.equal(f, flows[k]), f"pair {k}"
    assert not torch.equal(flows[0], flows[4])


@pytest.mark.parametrize("nlanes", [2, 3, 4])
@pytest.mark.parametrize("eps,iters", [(0.0, 10), (0.01, 60)])
def test_two_lanes_equal_one_lane(gpu, eps, iters, nlanes):
    """A batch split over several lanes (the caller's stream + internal streams; 2 is the default from 4 pairs on) is
    bit-identical to the same batch on the caller's stream alone (lanes = 1), for fixed work and for the device-decided
    convergence path, whose per-pair iteration counts must come back from the right lane."""
    import torch
    from opencv_contrib_amd import cuda
    pairs = [synth.flow_pair(150, 210, seed=40 + k)[:2] for k in range(5)]
    I0s, I1s = [T(p[0], gpu) for p in pairs], [T(p[1], gpu) for p in pairs]
    a1 = cuda.OpticalFlowDual_TVL1.create(iterations=iters, epsilon=eps, lanes=1)
    a2 = cuda.OpticalFlowDual_TVL1.create(iterations=iters, epsilon=eps, lanes=nlanes)
    f1, f2 = a1.calc_batch(I0s, I1s), a2.calc_batch(I0s, I1s)
    torch.cuda.synchronize()
    assert torch.equal(f1, f2)
    for k in range(5):
        assert a1.lastIterations(k) == a2.lastIterations(k)
    if eps > 0:
        assert a1.lastIterations(0) != a1.lastIterations(3) or a1.lastIterations(1) != a1.lastIterations(4)
    # ... and to five single calcs: the stopping decisions use integer error sums, so they do not depend on the batch either
    single = cuda.OpticalFlowDual_TVL1.create(iterations=iters, epsilon=eps)
    for k in range(5):
        assert torch.equal(single.calc(I0s[k], I1s[k]), f1[k]), f"pair {k}"
        assert single.lastIterations(0) == a1.lastIterations(k)


# ------------------------------------------------------------------------------------------------ TV-L1 at 4K, class defaults at 1080p,
# the reference test's literal setting
@pytest.fixture(scope="module")
def pair4k(oracle):
    # the motion of the 1080p pairs in pixels (flow_scale 3, texture sigma 6): five 0.8-scales cover it at either size -- the
    # generator's default scales the motion with the width, 21 px at 4K, which no 5-scale pyramid recovers (oracle included)
    I0, I1, gt = synth.flow_pair(2160, 3840, seed=1234, flow_scale=3.0, sigma=6.0)
    return I0, I1, gt, oracle.tvl1_calc(I0, I1, oracle.tvl1_params(iterations=10, epsilon=0.0))


@pytest.mark.parametrize("exact", [False, True], ids=["default_fast_fused", "exact_math"])
def test_tvl1_4k_against_oracle(gpu, pair4k, exact):
    """north_star "synthetic 1080p/4K pairs": 3840 x 2160 CV_32FC1, iterations = 10, against oracle.tvl1_calc with the 1080p bounds
    (reference call path cudaoptflow/src/tvl1flow.cpp:185-302; the plane offsets of a 4K batch are where the 32-bit guard of
    c3a8dde sits)."""
    from opencv_contrib_amd import cuda
    I0, I1, gt, ref = pair4k
    alg = cuda.OpticalFlowDual_TVL1.create(iterations=10, epsilon=0.0, exactMath=exact)
    flow = N(alg.calc(T(I0, gpu), T(I1, gpu)))
    assert np.isfinite(flow).all()
    d = np.sqrt(((flow - ref) ** 2).sum(-1))
    assert d.mean() <= (2e-3 if exact else 5e-3), d.mean()
    assert synth.ccorr_dissimilarity(flow, ref) <= 1e-4
    assert (d <= 0.02).mean() >= 0.99
    assert synth.epe(flow, gt) < 0.15


def test_tvl1_4k_batch_equals_single_calcs(gpu, pair4k):
    """A 4K batch (two lanes, 5 pairs: 1.6 GB of planes per lane) is bit-identical to single calcs."""
    import torch
    from opencv_contrib_amd import cuda
    I0, I1, _, _ = pair4k
    a, b = T(I0, gpu), T(I1, gpu)
    I0s = [torch.roll(a, 11 * k, 1).contiguous() for k in range(5)]
    I1s = [torch.roll(b, 11 * k, 1).contiguous() for k in range(5)]
    alg = cuda.OpticalFlowDual_TVL1.create(iterations=10, epsilon=0.0)
    fb = alg.calc_batch(I0s, I1s)
    torch.cuda.synchronize()
    single = cuda.OpticalFlowDual_TVL1.create(iterations=10, epsilon=0.0)
    for k in (0, 2, 4):
        assert torch.equal(single.calc(I0s[k], I1s[k]), fb[k]), f"pair {k}"


@pytest.mark.parametrize("sem", [0, 1], ids=["cpu_class_rule", "cv_cuda_schedule"])
def test_class_defaults_at_1080p(gpu, oracle, sem):
    """The class defaults (300 iterations, epsilon 0.01: cudaoptflow.hpp:382) at the BASELINE size, the configuration bench.py's
    `class_defaults_300_eps0.01` variant publishes: device-decided stop, iteration counts within 2 of the oracle's per (scale,
    warp), flow within the change of the last converged iterations, deterministic."""
    from opencv_contrib_amd import cuda
    I0, I1, gt = synth.flow_pair(1080, 1920, seed=1234)
    ref, st = oracle.tvl1_calc(I0, I1, oracle.tvl1_params(iterations=300, semantics=sem), return_stats=True)
    alg = cuda.OpticalFlowDual_TVL1.create(semantics=sem)
    flow = N(alg.calc(T(I0, gpu), T(I1, gpu)))
    it = np.array(alg.lastIterations())
    rit = np.array(st["iters"])[:it.shape[0], :it.shape[1]]
    assert it.shape == rit.shape == (5, 5)
    assert it.min() >= 1 and (it < 300).any()
    assert np.abs(it - rit).max() <= 2, (it.tolist(), rit.tolist())
    d = np.sqrt(((flow - ref) ** 2).sum(-1))
    assert d.mean() <= 2e-2, d.mean()
    assert synth.ccorr_dissimilarity(flow, ref) <= 4e-3
    assert synth.epe(flow, gt) < 0.15
    np.testing.assert_array_equal(flow, N(alg.calc(T(I0, gpu), T(I1, gpu))))


@pytest.mark.parametrize("sem", [0, 1], ids=["cpu_class_rule", "cv_cuda_schedule"])
@pytest.mark.parametrize("shape,seed,dtype", [((388, 584), 78, "u8"), ((480, 640), 5, "f32"), ((1080, 1920), 1234, "f32")])
def test_reference_accuracy_test_literal_setting(gpu, oracle, sem, shape, seed, dtype):
    """cudaoptflow/test/test_optflow.cpp:440-466 LITERALLY: `OpticalFlowDual_TVL1::create(); setNumIterations(10);` -- nothing else,
    so epsilon stays 0.01 and "N = 10" is the convergence-checked loop with at most 10 iterations per warp, not fixed work
    (the CPU twin there: medianFiltering 1, innerIterations 1, outerIterations = the CUDA object's iterations).  Counts within 2 of
    the oracle's and never above 10, flow inside the reference's own acceptance |1 - CCORR| <= 4e-3 by a wide margin."""
    from opencv_contrib_amd import cuda
    I0, I1, _ = synth.flow_pair(*shape, seed=seed, dtype=dtype)
    alg = cuda.OpticalFlowDual_TVL1.create(semantics=sem)
    alg.setNumIterations(10)
    assert (alg.getNumIterations(), alg.getEpsilon()) == (10, 0.01)
    ref, st = oracle.tvl1_calc(I0, I1, oracle.tvl1_params(iterations=10, semantics=sem), return_stats=True)
    flow = N(alg.calc(T(I0, gpu), T(I1, gpu)))
    it = np.array(alg.lastIterations())
    rit = np.array(st["iters"])[:it.shape[0], :it.shape[1]]
    assert it.shape == rit.shape
    assert it.min() >= 1 and it.max() <= 10
    assert np.abs(it - rit).max() <= 2, (it.tolist(), rit.tolist())
    d = np.sqrt(((flow - ref) ** 2).sum(-1))
    assert d.mean() <= 2e-2, d.mean()
    assert synth.ccorr_dissimilarity(flow, ref) <= 1e-3       # test_optflow.cpp:465 accepts 4e-3


def test_sixteen_handles_sixteen_streams_one_calc_each(gpu, oracle):
    """cudaoptflow/test/test_optflow.cpp:468-527 (the reference's async test): 16 objects, 16 streams, one calc() each, all in
    flight together; every flow must equal the flow of a lone calc on the default stream bit for bit (handles share nothing)."""
    import torch
    from opencv_contrib_amd import cuda
    pairs = [synth.flow_pair(388, 584, seed=300 + k)[:2] for k in range(16)]
    I0s, I1s = [T(p[0], gpu) for p in pairs], [T(p[1], gpu) for p in pairs]
    algs = [cuda.OpticalFlowDual_TVL1.create() for _ in range(16)]
    for a in algs:
        a.setNumIterations(10)
    streams = [torch.cuda.Stream(device=gpu) for _ in range(16)]
    torch.cuda.synchronize()
    # outputs allocated up front (a tensor freed while another stream still writes it could be handed out again)
    outs = [[torch.empty((388, 584, 2), dtype=torch.float32, device=gpu) for _ in range(16)] for _ in range(2)]
    torch.cuda.synchronize()
    for rep in range(2):   # the second round re-uses warm handles while the first may still be running
        for k in range(16):
            algs[k].calc(I0s[k], I1s[k], flow=outs[rep][k], stream=streams[k].cuda_stream)
    flows = outs[1]
    for s in streams:
        s.synchronize()
    lone = cuda.OpticalFlowDual_TVL1.create()
    lone.setNumIterations(10)
    for k in range(16):
        assert torch.equal(lone.calc(I0s[k], I1s[k]), flows[k]), f"handle {k}"
    ref = oracle.tvl1_calc(pairs[3][0], pairs[3][1], oracle.tvl1_params(iterations=10))
    assert np.sqrt(((N(flows[3]) - ref) ** 2).sum(-1)).mean() <= 2e-2


@pytest.mark.parametrize("devices,chunk", [([0], 4), ([0, 0], 2), ([0, 0, 0], 16)])
def test_multi_device_host_entry_equals_calc_batch(gpu, devices, chunk):
    """mi_tvl1_multi_calc_batch (host threads, one per device; peer-to-peer staging in double-buffered chunks): on the one-GPU
    test box the worker list names device 0 several times, which runs every code path -- the in-place root worker, the staged
    workers with their copy / compute streams, the chunking with a ragged last chunk -- and must give, pair for pair, the bytes
    of mi_tvl1_calc_batch.  Inputs include pitched (ROI) matrices."""
    import torch
    from opencv_contrib_amd import cuda
    n = 11
    pairs = [synth.flow_pair(96, 160, seed=80 + k)[:2] for k in range(4)]
    big0 = torch.zeros((n, 96, 200), dtype=torch.float32, device=gpu)
    I0s, I1s = [], []
    for k in range(n):
        a, b = T(pairs[k % 4][0], gpu), T(pairs[k % 4][1], gpu)
        a, b = torch.roll(a, 5 * (k // 4), 1), torch.roll(b, 5 * (k // 4), 1)
        big0[k, :, 20:180] = a
        I0s.append(big0[k, :, 20:180])          # pitched view: step = 800 bytes, 640 used
        I1s.append(b.contiguous())
    alg = cuda.OpticalFlowDual_TVL1.create(iterations=10, epsilon=0.0)
    ref = alg.calc_batch(I0s, I1s)
    torch.cuda.synchronize()
    multi = cuda.TVL1MultiDevice(alg, devices=devices, chunk=chunk)
    assert multi.deviceCount() == len(devices)
    out = multi.calc_batch(I0s, I1s)
    assert torch.equal(out, ref)
    out2 = multi.calc_batch(I0s[:3], I1s[:3])   # fewer pairs than workers x chunk: some workers idle
    assert torch.equal(out2, ref[:3])


def test_rccl_binding_of_the_multi_device_entry_on_one_gpu(gpu):
    """Round 5: the C++ multi-GPU entry moves its shards as RCCL point-to-point messages (grouped ncclSend /
    ncclRecv, librccl bound at run time).  A one-GPU box cannot open a two-rank communicator on two devices, but it can run the same
    entry points with the same argument orders and constants: a one-rank communicator, a grouped send to self / receive from self.
    Workers that share the root's GPU keep their peer copies (transport() says so) and still give the bytes of calc_batch."""
    import ctypes as C
    import torch
    from opencv_contrib_amd import capi, cuda
    torch.cuda.set_device(gpu)
    src = bytes(np.random.default_rng(5).integers(0, 256, size=1 << 20, dtype=np.uint8))
    dst = C.create_string_buffer(len(src))
    avail = C.c_int(-1)
    capi.check(capi.lib().miflow_selftest_rccl_self_copy(src, dst, len(src), C.byref(avail)))
    assert avail.value == 1, "librccl.so of the ROCm installation was not found"
    assert dst.raw == src
    multi = cuda.TVL1MultiDevice(cuda.OpticalFlowDual_TVL1.create(iterations=10, epsilon=0.0), devices=[0, 0, 0], chunk=2)
    assert multi.transport() == (0, 2)


def test_multi_device_host_entry_over_distinct_devices(gpu):
    """The same entry over DIFFERENT GPUs: real peer enable, per-device arena caches, xGMI
    peer copies, one worker thread per device.  Needs a node with at least two visible devices; the one-GPU test box skips it
    (the driver's multi-GPU node, if any, runs it).  Every pair's flow must be the bytes mi_tvl1_calc_batch produces on the
    root device -- the kernels are deterministic and identical on every device."""
    import torch
    from opencv_contrib_amd import cuda
    nd = torch.cuda.device_count()
    if nd < 2:
        pytest.skip("needs >= 2 visible GPUs")
    n = 13
    pairs = [synth.flow_pair(120, 200, seed=300 + k)[:2] for k in range(n)]
    I0s, I1s = [T(p[0], gpu) for p in pairs], [T(p[1], gpu) for p in pairs]
    alg = cuda.OpticalFlowDual_TVL1.create(iterations=10, epsilon=0.0)
    ref = alg.calc_batch(I0s, I1s)
    torch.cuda.synchronize()
    for devices, chunk in ((list(range(nd)), 2), ([nd - 1, 0], 16), ([0, 1, 1, 0], 3)):
        multi = cuda.TVL1MultiDevice(alg, devices=devices, chunk=chunk)
        assert multi.deviceCount() == len(devices)
        assert multi.transport() == (sum(1 for d in devices[1:] if d != devices[0]), sum(1 for d in devices[1:] if d == devices[0]))   # RCCL between distinct GPUs
        for _ in range(2):    # the second call re-uses the workers' warm handles and staging slots
            out = multi.calc_batch(I0s, I1s)
            assert torch.equal(out, ref), (devices, chunk)
        del multi
    torch.cuda.set_device(gpu)


def test_bench_two_ranks_over_rccl_when_two_gpus_are_visible(gpu):
    """`python bench.py --gpus 2` on a node with two GPUs: two ranks on two distinct devices over RCCL, the scatter / gather leg
    included, flows gathered on rank 0 identical to rank 0's own computation of every shard.  Skips on the one-GPU box."""
    import json
    import subprocess
    import sys
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 visible GPUs")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update({"MIFLOW_BENCH_EXCHANGE_PAIRS": "8", "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "8"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["n_gpus"] == 2 and out["rccl_ranks"]["distinct_devices"] == 2 and len(out["per_rank_pairs_per_s"]) == 2
    assert out["gathered_flows_identical"] is True, out.get("with_scatter_gather")


def test_fused_warp_pass_is_bit_identical(gpu, exp_env):
    """(Experiments build: the fused form lost its A/B, profiles/r14, and is not in the release library since round 6.)  Round 5: `MIFLOW_TB_FW=1` runs a warp whose iterations are one pass of the T = 10 kernel INSIDE that pass --
    four producer waves per workgroup compute I1wx, I1wy, rho_c with the warp kernel's own per-pixel routines (tvl1_warp_px.h) and
    hand them to the joined consumer waves through LDS; the three planes never reach HBM.  Same operations in the same order: the flows
    of fixed-work calcs (both arithmetics, f32 and u8 frames, odd sizes, 8..64 pairs, one and two passes per warp) must not change by
    a bit (tools/fw_check.py runs each setting in its own process: the switch is read once)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fw_check.py")], capture_output=True, text=True, timeout=1200, env=exp_env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    assert r.stdout.count("IDENTICAL") == 8 and "DIFFERENT" not in r.stdout, r.stdout[-3000:]
    assert "fused warp" in r.stdout   # the fused kernel really ran in the MIFLOW_TB_FW=1 process (MIFLOW_TB_VERBOSE lines)


def test_scheduling_switches_of_the_release_library_do_not_change_results(gpu):
    """The release switches that only move WORK AROUND -- `MIFLOW_LANES` (internal streams of a batch), `MIFLOW_TB_HIST` (block lengths
    of the convergence-checked path from the handle's previous calc) -- must leave the flows of a fixed-work batch and of a
    class-default batch bit-identical (each setting in its own process: the switches are read once).  Where the experiments build is in
    the tree, its `MIFLOW_TB_JW=0` (independent instead of joined waves) and `MIFLOW_TB_FW=1` (warp inside the pass) must give the
    release library's digests as well -- two other formulations of the same arithmetic."""
    import re
    import subprocess
    import sys
    from conftest import experiments_lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dig = {}
    settings = [("default", {}), ("lanes1", {"MIFLOW_LANES": "1"}), ("lanes3", {"MIFLOW_LANES": "3"}), ("nohist", {"MIFLOW_TB_HIST": "0"})]
    if experiments_lib():
        settings += [("exp", {"MIFLOW_LIB": experiments_lib()}), ("exp_jw0", {"MIFLOW_LIB": experiments_lib(), "MIFLOW_TB_JW": "0"}),
                     ("exp_fw1", {"MIFLOW_LIB": experiments_lib(), "MIFLOW_TB_FW": "1"})]
    for tag, env in settings:
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "defaults_digest.py"), "6", "both"], capture_output=True, text=True,
                           env=dict(os.environ, **env), timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        dig[tag] = re.findall(r"digest ([0-9a-f]{16})", r.stdout)
        assert len(dig[tag]) == 2, r.stdout
    assert all(v == dig["default"] for v in dig.values()), dig


def test_result_changing_switches_are_not_read_by_the_release_library(gpu):
    """Round 5: `MIFLOW_TB_P16=1` (dual variable as 16-bit fixed point between passes: changes results) and
    `MIFLOW_X_SKIP` (skips launches: wrong results) exist in the experiments build only.  With either set, the shipped library computes
    exactly what it computes without them (fixed-work headline setting and class defaults)."""
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dig = {}
    base_env = {k: v for k, v in os.environ.items() if k != "MIFLOW_LIB"}   # the RELEASE library, whatever library this suite runs under
    for tag, env in (("default", {}), ("p16", {"MIFLOW_TB_P16": "1"}), ("skip1", {"MIFLOW_X_SKIP": "1"}), ("skip2", {"MIFLOW_X_SKIP": "2"})):
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "defaults_digest.py"), "4", "both"], capture_output=True, text=True,
                           env=dict(base_env, **env), timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        dig[tag] = re.findall(r"digest ([0-9a-f]{16})", r.stdout)
        assert len(dig[tag]) == 2, r.stdout
    assert dig["default"] == dig["p16"] == dig["skip1"] == dig["skip2"], dig


@pytest.mark.parametrize("sem", [0, 1], ids=["cpu_class_rule", "cv_cuda_schedule"])
@pytest.mark.parametrize("shape,seed", [((120, 160), 11), ((388, 584), 78)])
def test_class_defaults_speculative_convergence(gpu, oracle, sem, shape, seed):
    """Class defaults (300 iterations, epsilon 0.01) in fast math: blocks of 10 iterations run speculatively with their
    per-iteration error sums recorded, the stopping rule of the reference (CPU class: after every iteration,
    optflow/src/tvl1flow.cpp:1376-1390; cv::cuda: odd iterations while prevError < scaledEpsilon,
    cudaoptflow/src/tvl1flow.cpp:357-377) is applied on the device and a block the loop stops in is replayed with exactly
    that many iterations.  Iteration counts per (scale, warp) within 2 of the oracle's (fast-math error sums), flow within
    the change of the last converged iterations."""
    from opencv_contrib_amd import cuda
    I0, I1, _ = synth.flow_pair(*shape, seed=seed)
    ref, st = oracle.tvl1_calc(I0, I1, oracle.tvl1_params(iterations=300, semantics=sem), return_stats=True)
    alg = cuda.OpticalFlowDual_TVL1.create(semantics=sem)
    flow = N(alg.calc(T(I0, gpu), T(I1, gpu)))
    it = np.array(alg.lastIterations())
    rit = np.array(st["iters"])[:it.shape[0], :it.shape[1]]
    assert it.min() >= 1 and it.max() <= 300
    assert (it < 300).any(), "nothing converged: the stopping rule never fired"
    assert np.abs(it - rit).max() <= 2, (it.tolist(), rit.tolist())
    d = np.sqrt(((flow - ref) ** 2).sum(-1))
    assert d.mean() <= 2e-2, d.mean()
    assert synth.ccorr_dissimilarity(flow, ref) <= 4e-3
    # the same object, same inputs: deterministic (fixed-point error sums), and a batch gives every pair its own counts
    flow2 = N(alg.calc(T(I0, gpu), T(I1, gpu)))
    np.testing.assert_array_equal(flow, flow2)


@pytest.mark.parametrize("iters,eps", [(300, 0.01), (10, 0.01), (23, 0.05)])
def test_host_feedback_never_changes_a_flow(gpu, iters, eps):
    """mi_tvl1_params.host_feedback (round 3): a convergence-checked calc of one or two pairs reads the converged flags back between
    launches and stops enqueuing for a warp that has stopped (the host waits inside calc() about once per warp, as the reference's
    class does at each of its checks, cudaoptflow/src/tvl1flow.cpp:362-368).  Which launches were enqueued must not show: flows and
    per-(scale, warp) iteration counts with feedback off (-1), automatic (0) and forced (1, also for a 3-pair single-lane batch) are
    identical, singles equal the batch, and repeated calls of one handle (warm predictions) reproduce."""
    import torch
    from opencv_contrib_amd import cuda
    pairs = [synth.flow_pair(240, 320, seed=90 + k)[:2] for k in range(3)]
    I0s, I1s = [T(p[0], gpu) for p in pairs], [T(p[1], gpu) for p in pairs]
    algs = {fb: cuda.OpticalFlowDual_TVL1.create(iterations=iters, epsilon=eps, hostFeedback=fb, lanes=1) for fb in (-1, 0, 1)}
    ref = algs[-1].calc_batch(I0s, I1s)
    torch.cuda.synchronize()
    counts = [algs[-1].lastIterations(k) for k in range(3)]
    f1 = algs[1].calc_batch(I0s, I1s)                      # forced: three pairs, one lane
    assert torch.equal(f1, ref) and [algs[1].lastIterations(k) for k in range(3)] == counts
    for rep in range(2):
        for k in range(3):
            for fb in (0, 1, -1):
                f = algs[fb].calc(I0s[k], I1s[k])
                assert torch.equal(f, ref[k]), (rep, k, fb)
                assert algs[fb].lastIterations(0) == counts[k]
    f2 = algs[0].calc_batch(I0s[:2], I1s[:2])              # automatic: two pairs
    assert torch.equal(f2, ref[:2])
    assert np.array(counts).max() <= iters and (iters < 300 or np.array(counts).max() < 300)


@pytest.mark.parametrize("sem", [0, 1], ids=["cpu_class_rule", "cv_cuda_schedule"])
def test_block_lengths_from_the_previous_calc_never_change_a_flow(gpu, sem):
    """Round 4: the first block of a warp's speculative steps is as long as THIS warp of THIS pair slot needed in the handle's previous
    calc (SpecK::h_in, tvl1_tb_dev.h spec_settle) -- on video the best estimate there is, and like every estimate only a matter of how
    many passes run.  A handle whose history is exact (same pair again), misleading (another pair, a permuted batch, another size
    in between) or absent (fresh handle) returns the same flows and the same per-(scale, warp) counts."""
    import torch
    from opencv_contrib_amd import cuda
    pairs = [synth.flow_pair(200, 264, seed=140 + k)[:2] for k in range(4)]
    I0s, I1s = [T(p[0], gpu) for p in pairs], [T(p[1], gpu) for p in pairs]
    small = synth.flow_pair(96, 128, seed=150)[:2]

    def fresh(idx):
        a = cuda.OpticalFlowDual_TVL1.create(semantics=sem, lanes=1)
        f = a.calc_batch([I0s[i] for i in idx], [I1s[i] for i in idx])
        torch.cuda.synchronize()
        return f.clone(), [a.lastIterations(k) for k in range(len(idx))]

    alg = cuda.OpticalFlowDual_TVL1.create(semantics=sem, lanes=1)
    for idx in ([0, 1, 2, 3], [0, 1, 2, 3], [3, 2, 1, 0], [1, 1, 1, 1], [2, 0, 3, 1]):
        want, counts = fresh(idx)
        got = alg.calc_batch([I0s[i] for i in idx], [I1s[i] for i in idx])
        torch.cuda.synchronize()
        assert torch.equal(got, want), idx
        assert [alg.lastIterations(k) for k in range(4)] == counts, idx
    alg.calc(T(small[0], gpu), T(small[1], gpu))              # another geometry in between: the counts are dropped, not misread
    for k in (0, 0, 2):
        want, counts = fresh([k])
        assert torch.equal(alg.calc(I0s[k], I1s[k]), want[0]), k
        assert alg.lastIterations(0) == counts[0]
    assert (np.array(counts) < 300).any()


@pytest.mark.parametrize("shape", [(480, 640), (1080, 1920)], ids=["perf_test_640x480", "1080p"])
def test_single_calcs_at_baseline_sizes_with_and_without_history(gpu, shape):
    """The reference's own calling pattern at its perf test's size (cudaoptflow/perf/perf_optflow.cpp:283-311) and at 1080p: one pair per
    calc(), class defaults, three scenes in turn through ONE handle (its block-length history, host-seen counts, tile margins and the
    warp kernels enqueued ahead are then wrong as often as right) against a fresh handle per calc -- flows and counts identical, twice
    round the scenes."""
    import torch
    from opencv_contrib_amd import cuda
    h, w = shape
    pairs = [synth.flow_pair(h, w, seed=1234 + k)[:2] for k in range(3)]
    I0s, I1s = [T(p[0], gpu) for p in pairs], [T(p[1], gpu) for p in pairs]
    want = []
    for k in range(3):
        a = cuda.OpticalFlowDual_TVL1.create()
        want.append((a.calc(I0s[k], I1s[k]).clone(), a.lastIterations(0)))
        torch.cuda.synchronize()
    alg = cuda.OpticalFlowDual_TVL1.create()
    for rep in range(2):
        for k in (0, 0, 1, 2, 2, 1):
            f = alg.calc(I0s[k], I1s[k])
            assert torch.equal(f, want[k][0]), (rep, k)
            assert alg.lastIterations(0) == want[k][1], (rep, k)
    assert (np.array(want[0][1]) < 300).any()


@pytest.mark.parametrize("iters", [1, 2, 3, 5, 7, 12, 23])
@pytest.mark.parametrize("shape", [(16, 16), (21, 37), (64, 9), (5, 300), (97, 131)])
def test_speculative_steps_iteration_limits_and_small_images(gpu, oracle, shape, iters):
    """The convergence-checked fast path on the sizes and iteration limits where its plan degenerates: limits below, at and
    between the kernels' block sizes (5, 10), images narrower than a wave's strip or with fewer rows than a band, levels dropped
    by the 16-px rule.  Counts never exceed the limit, stay within 2 of the oracle's, and the flow stays within the change of the
    last iterations; with an unreachable threshold the count equals the limit exactly."""
    from opencv_contrib_amd import cuda
    I0, I1, _ = synth.flow_pair(*shape, seed=shape[0] * 7 + iters)
    ref, st = oracle.tvl1_calc(I0, I1, oracle.tvl1_params(iterations=iters, epsilon=0.05), return_stats=True)
    alg = cuda.OpticalFlowDual_TVL1.create(iterations=iters, epsilon=0.05)
    flow = N(alg.calc(T(I0, gpu), T(I1, gpu)))
    it = np.array(alg.lastIterations())
    rit = np.array(st["iters"])[:it.shape[0], :it.shape[1]]
    assert it.shape == rit.shape
    assert it.min() >= 1 and it.max() <= iters
    assert np.abs(it - rit).max() <= 2, (it.tolist(), rit.tolist())
    assert np.isfinite(flow).all()
    assert np.sqrt(((flow - ref) ** 2).sum(-1)).mean() <= 5e-2
    full = cuda.OpticalFlowDual_TVL1.create(iterations=iters, epsilon=1e-12)
    full.calc(T(I0, gpu), T(I1, gpu))
    assert np.array(full.lastIterations()).min() == iters and np.array(full.lastIterations()).max() == iters


@pytest.mark.parametrize("eps,iters", [(0.0, 10), (0.01, 300), (0.05, 23)])
def test_flows_do_not_depend_on_which_iteration_kernel_a_level_runs_on(gpu, eps, iters):
    """A level of at most 2.3 M pixels x pairs per lane iterates on the register-tile kernel, a larger one on the streaming kernel
    (tvl1_tile_kernels.hip): the same 150 x 210 pairs alone (tile kernel, also for the speculative steps of the convergence path)
    and inside a batch of 160 (streaming kernel on the two finest levels) must give bit-identical flows and iteration counts --
    identical per-pixel arithmetic, integer error sums."""
    import torch
    from opencv_contrib_amd import cuda
    pairs = [synth.flow_pair(150, 210, seed=70 + k)[:2] for k in range(4)]
    I0s = [T(pairs[k % 4][0], gpu) for k in range(160)]
    I1s = [T(pairs[k % 4][1], gpu) for k in range(160)]
    big = cuda.OpticalFlowDual_TVL1.create(iterations=iters, epsilon=eps)
    fb = big.calc_batch(I0s, I1s)
    torch.cuda.synchronize()
    single = cuda.OpticalFlowDual_TVL1.create(iterations=iters, epsilon=eps)
    for k in (0, 1, 2, 3, 157):
        assert torch.equal(single.calc(I0s[k], I1s[k]), fb[k]), f"pair {k}"
        assert single.lastIterations(0) == big.lastIterations(k)


def test_stop_slack_runs_at_most_a_few_more_iterations(gpu, oracle):
    """mi_tvl1_params.stop_slack = 1 (miflow extension, off by default): a speculative block is kept when the reference's test
    first passed one iteration before its end.  Counts stay within the slack (+ the knock-on of a slightly different start of
    the following warps) of the exact run, the flow within the change of one converged iteration."""
    from opencv_contrib_amd import cuda
    I0, I1, _ = synth.flow_pair(388, 584, seed=78)
    ref = oracle.tvl1_calc(I0, I1, oracle.tvl1_params(iterations=300))
    exact = cuda.OpticalFlowDual_TVL1.create()
    loose = cuda.OpticalFlowDual_TVL1.create(stopSlack=1)
    f0, f1 = N(exact.calc(T(I0, gpu), T(I1, gpu))), N(loose.calc(T(I0, gpu), T(I1, gpu)))
    i0, i1 = np.array(exact.lastIterations()), np.array(loose.lastIterations())
    assert np.abs(i1 - i0).max() <= 2, (i0.tolist(), i1.tolist())
    assert i1.sum() >= i0.sum() - 2
    assert np.sqrt(((f1 - f0) ** 2).sum(-1)).mean() <= 1.5e-2
    assert np.sqrt(((f1 - ref) ** 2).sum(-1)).mean() <= 2e-2
    np.testing.assert_array_equal(f1, N(loose.calc(T(I0, gpu), T(I1, gpu))))


def test_speculative_equals_fixed_work_when_nothing_converges(gpu):
    """With an unreachable threshold every speculative block is accepted: the result must be bit-identical to the fixed-work
    run of the same iteration count (same kernels, MODE 1 vs MODE 0), for a count that is not a multiple of the block size."""
    import torch
    from opencv_contrib_amd import cuda
    I0, I1, _ = synth.flow_pair(150, 210, seed=5)
    a = cuda.OpticalFlowDual_TVL1.create(iterations=27, epsilon=1e-9)
    b = cuda.OpticalFlowDual_TVL1.create(iterations=27, epsilon=0.0, timeBlock=0)
    fa, fb = a.calc(T(I0, gpu), T(I1, gpu)), b.calc(T(I0, gpu), T(I1, gpu))
    assert np.array(a.lastIterations()).min() == 27
    # the fixed-work plan fuses 27 = 10 + 10 + 5 + 2 differently (cost model): compare with a tolerance of rounding only
    assert float((fa - fb).abs().max()) <= 1e-4


# ------------------------------------------------------------------------------------------------ fused-gradient warp
@pytest.mark.parametrize("amp", [0.0, 1.5, 8.0, 400.0])
@pytest.mark.parametrize("shape", [(77, 101), (6, 9), (5, 300), (211, 467)])
def test_fused_warp_bit_exact_against_oracle_cpu_semantics(gpu, oracle, shape, amp):
    """k_warp6<CPU_REF> (gradient of I1 formed in the kernel from a 6 x 6 window) against oracle.tvl1_warp: bit for bit,
    interior and border lanes, flows up to far outside the image, images too small for any interior window."""
    from opencv_contrib_amd import capi, cuda
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    I0 = (rng.random((h, w)) * 255).astype(np.float32)
    I1 = (rng.random((h, w)) * 255).astype(np.float32)
    u1 = (rng.standard_normal((h, w)) * amp).astype(np.float32)
    u2 = (rng.standard_normal((h, w)) * amp).astype(np.float32)
    if amp == 0.0:
        u1[::3, ::5] = 0.5; u2[1::4, ::2] = -1.0; u1[::2, 1::3] = 1.0 / 64   # phase ties of the 1/32-px quantisation
    ox, oy = oracle.tvl1_centered_gradient(I1)
    ref = oracle.tvl1_warp(0, I0, I1, ox, oy, u1, u2)
    got = cuda.tvl1_warpBackward(capi.MI_SEM_CPU_REF, T(I0, gpu), T(I1, gpu), None, None, T(u1, gpu), T(u2, gpu))
    for name, r, g in zip(("I1w", "I1wx", "I1wy", "grad", "rho_c"), ref, got):
        np.testing.assert_array_equal(N(g), r, err_msg=name)


@pytest.mark.parametrize("sem", [0, 1])
@pytest.mark.parametrize("amp", [0.0, 2.5, 400.0])
def test_fused_warp_equals_gather_warp(gpu, oracle, sem, amp):
    """The fused-gradient kernel and the packed-plane gather kernel (the round-1 kernel, still the stage-level path for
    caller-supplied derivative planes) are two implementations of one function: bit-identical for both semantics."""
    from opencv_contrib_amd import cuda
    h, w = 130, 203
    rng = np.random.default_rng(sem * 7 + int(amp))
    I0 = (rng.random((h, w)) * 255).astype(np.float32)
    I1 = (rng.random((h, w)) * 255).astype(np.float32)
    u1 = (rng.standard_normal((h, w)) * amp).astype(np.float32)
    u2 = (rng.standard_normal((h, w)) * amp).astype(np.float32)
    if amp == 0.0:
        u1[::3, ::5] = 1.0; u2[1::4, ::2] = -2.0   # integer positions: the 5-tap windows of the reference's loop bounds
    ox, oy = oracle.tvl1_centered_gradient(I1)
    a = cuda.tvl1_warpBackward(sem, T(I0, gpu), T(I1, gpu), T(ox, gpu), T(oy, gpu), T(u1, gpu), T(u2, gpu))
    b = cuda.tvl1_warpBackward(sem, T(I0, gpu), T(I1, gpu), None, None, T(u1, gpu), T(u2, gpu))
    for name, x, y in zip(("I1w", "I1wx", "I1wy", "grad", "rho_c"), a, b):
        np.testing.assert_array_equal(N(x), N(y), err_msg=name)


from conftest import loaded_library_is_experiments_build  # noqa: E402


# (collected where the loaded library is the experiments build: tests/test_tvl1_gpu.py::test_experiment_only_kernels_under_the_experiments_build)
LDS_WARP_CASES = [(sem, amp, shape) for sem in (0, 1) for amp in (0.0, 2.5, 12.0, 400.0) for shape in ((130, 203), (6, 9), (97, 640))] \
    if loaded_library_is_experiments_build() else []


@pytest.mark.parametrize("sem,amp,shape", LDS_WARP_CASES)
def test_fused_warp_lds_staged_equals_gather(gpu, sem, amp, shape):
    """(Experiments build only since round 6: the LDS-staged warp lost its A/B under the two-lane overlap, r02z3.)  k_warp_lds (windows read from an LDS-staged region of I1 found from the tile's own flows; fallback to the global path
    for border windows and for tiles whose flow spreads the windows beyond the buffer: amp 12 and 400) and k_warp6 (global
    gather) are bit-identical, in exact and in fast (separable sums) form."""
    from opencv_contrib_amd import cuda
    h, w = shape
    rng = np.random.default_rng(sem * 7 + int(amp) + h)
    I0 = (rng.random((h, w)) * 255).astype(np.float32)
    I1 = (rng.random((h, w)) * 255).astype(np.float32)
    u1 = (rng.standard_normal((h, w)) * amp).astype(np.float32) + np.float32(3.3)
    u2 = (rng.standard_normal((h, w)) * amp).astype(np.float32) - np.float32(1.7)
    for fast in (0, 0x100):
        a = cuda.tvl1_warpBackward(sem | fast | 0x400, T(I0, gpu), T(I1, gpu), None, None, T(u1, gpu), T(u2, gpu))
        b = cuda.tvl1_warpBackward(sem | fast | 0x200, T(I0, gpu), T(I1, gpu), None, None, T(u1, gpu), T(u2, gpu))
        for name, x, y in zip(("I1w", "I1wx", "I1wy", "grad", "rho_c"), a, b):
            np.testing.assert_array_equal(N(x), N(y), err_msg=f"{name} fast={fast}")


@pytest.mark.parametrize("sem", [0, 1])
@pytest.mark.parametrize("amp", [0.0, 2.5, 400.0])
def test_fused_warp_fast_math_is_the_exact_warp_up_to_rounding(gpu, sem, amp):
    """Fast device math forms the three bicubic sums separably (68 instead of 173 operations per pixel): same taps, same
    weights, another association -- rounding-level differences only (images in 0..255: 1e-3 absolute on the warped planes)."""
    from opencv_contrib_amd import cuda
    h, w = 211, 467
    rng = np.random.default_rng(sem * 11 + int(amp))
    I0 = (rng.random((h, w)) * 255).astype(np.float32)
    I1 = (rng.random((h, w)) * 255).astype(np.float32)
    u1 = (rng.standard_normal((h, w)) * amp).astype(np.float32)
    u2 = (rng.standard_normal((h, w)) * amp).astype(np.float32)
    a = cuda.tvl1_warpBackward(sem, T(I0, gpu), T(I1, gpu), None, None, T(u1, gpu), T(u2, gpu))
    b = cuda.tvl1_warpBackward(sem | 0x100, T(I0, gpu), T(I1, gpu), None, None, T(u1, gpu), T(u2, gpu))
    for name, x, y in zip(("I1w", "I1wx", "I1wy"), a[:3], b[:3]):
        np.testing.assert_allclose(N(y), N(x), rtol=0, atol=1e-3, err_msg=name)
    np.testing.assert_allclose(N(b[3]), N(a[3]), rtol=1e-4, atol=1e-2, err_msg="grad")
    scale = 1.0 + np.abs(u1) + np.abs(u2)          # rho_c = I1w - I1wx u1 - I1wy u2 - I0
    assert np.all(np.abs(N(b[4]) - N(a[4])) <= 2e-3 * scale)


# ------------------------------------------------------------------------------------------------ StereoBM, configs[2]
def test_stereobm_1080p_128_15_bit_exact(gpu, oracle):
    from opencv_contrib_amd import cuda
    left, right, _ = synth.stereo_pair(1080, 1920, seed=42, max_disp=70)
    ref = oracle.sbm_compute(left, right, oracle.sbm_params(num_disparities=128, block_size=15))
    got = N(cuda.createStereoBM(128, 15).compute(T(left, gpu), T(right, gpu)))
    np.testing.assert_array_equal(got, ref)
    assert (ref > 0).mean() > 0.5   # a real disparity map, not the all-rejected corner case


# ------------------------------------------------------------------------------------------------ SURF, configs[3]
def test_surf_4k_threshold_400_against_oracle(gpu, oracle):
    """3840 x 2160, hessianThreshold 400, 4 octaves x 2 layers, keypointsRatio 0.01: maxFeatures clamps at 65 535 and the
    u32 integral image runs close to 2^31.  Every feature through tests/surf_check.py: detector rows bit for bit, angles against
    the libm-exact candidates, descriptors bit for bit at the HIP angles (computed once, in rounded mode).
    MI355X: 12 564 features, every angle matches the candidate with no rounding flipped (at most 2^-15 degrees away), 10 865 bit-equal,
    289 features with undecided samples (2.3 %, none above 3), no descriptor differs in any bit, 1 hard direction."""
    from opencv_contrib_amd import cuda
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from surf_check import assert_surf_equals
    img = synth.blob_image(2160, 3840, seed=7)
    ref = oracle.surf_detect_describe(img, oracle.surf_params(hessian_threshold=400.0), want_desc=False)
    assert ref["n"] > 2000
    np.testing.assert_array_equal(N(cuda.surf_integral(T(img, gpu))).view(np.uint32), oracle.surf_integral(img))
    alg = cuda.SURF_CUDA.create(400.0)
    kpg, desc = alg.detectWithDescriptors(T(img, gpu))
    kp = cuda.SURF_CUDA.downloadKeypoints(kpg)
    assert_surf_equals(oracle, img, kp, N(desc), ref, extended=False, upright=False, what="4K")
