"""Times cv::cuda::StereoConstantSpaceBP on the GPU and writes profiles/stereocsbp/stereocsbp.json (one JSON document; also printed).

Scenario: the parameters of the reference's perf test (cudastereo/perf/perf_stereo.cpp:166-199, createStereoConstantSpaceBP(128): ndisp
128, iters 8, levels 4, nr_plane 4) on a synthetic colour pair of 640 x 480 and of 1280 x 720; both message types.  Per scenario:

  compute        whole compute(left, right) calls, each bracketed by device events after warm-up calls (median, min, max ms);
  stereobp       cv::cuda::StereoBeliefPropagation of this library (ndisp 128, iters 8, levels 4) on the same pair, for orientation;
  init_data_cost the coarsest level's data cost and first-k selection through the stage entry (level 3, 128 disparities -> 32 planes);
  data_cost      compute_data_cost of every finer level through the stage entry (2 x planes candidates);
  iteration      ONE half-sweep of compute_message per level through the stage entry, in the register form and in the general form:
                 events around a block of alternating-parity launches, ms per launch.

Bytes are derived from the code, not measured.  Data cost of n candidates at an h x w level: both images once plus n h w sizeof(T)
written (plus the parents' n candidates read).  A half-sweep updates half the pixels, and an updated pixel reads four neighbour messages,
its data cost, its candidates and four neighbours' candidates and writes four messages: 14 n sizeof(T), so 7 n sizeof(T) per pixel of
the level.  The share of peak is of the 8.0 TB/s HBM3E specification.  There is no CPU fallback: without a device this fails.

    python tools/perf_stereocsbp.py [--reps 20] [--warmup 3] [--out profiles/stereocsbp/stereocsbp.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
CV_16S, CV_32F = 3, 5
NDISP, ITERS, LEVELS, NR_PLANE, CN = 128, 8, 4, 4, 3
SCENARIOS = {"vga": (480, 640), "hd720": (720, 1280)}   # name: rows, cols


def _events(fn, reps):
    import torch
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return times


def _stat(t, nbytes=None):
    med = float(np.median(t))
    rec = dict(ms=dict(median=med, min=float(np.min(t)), max=float(np.max(t))))
    if nbytes is not None:
        rec.update(bytes=nbytes, bytes_per_s=nbytes / (med * 1e-3), share_of_hbm_peak=nbytes / (med * 1e-3) / HBM_PEAK)
    return rec


def run(name, msg, reps, warmup):
    import torch
    from opencv_contrib_amd import capi, cuda
    rows, cols = SCENARIOS[name]
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    left = rng.integers(0, 256, (rows, cols, CN), dtype=np.uint8)
    left = ((left.astype(np.int32) + np.roll(left, 1, 1) + np.roll(left, 1, 0)) // 3).astype(np.uint8)
    right = np.roll(left, -7, 1)
    L, Rt = torch.from_numpy(left).to(dev), torch.from_numpy(np.ascontiguousarray(right)).to(dev)
    msg_type = CV_32F if msg == "f32" else CV_16S
    elem = 4 if msg == "f32" else 2
    T = torch.float32 if msg == "f32" else torch.int16
    disp = torch.empty((rows, cols), dtype=torch.int16, device=dev)
    timed = lambda fn: (([fn() for _ in range(warmup)], torch.cuda.synchronize(), _events(fn, reps))[2])

    bp = cuda.createStereoConstantSpaceBP(NDISP, ITERS, LEVELS, NR_PLANE, msg_type)
    rec = dict(scenario=name, msg=msg, rows=rows, cols=cols, channels=CN, ndisp=NDISP, iters=ITERS, levels=LEVELS, nr_plane=NR_PLANE,
               compute=_stat(timed(lambda: bp.compute(L, Rt, disp))), scratch_bytes=bp.scratchBytes())
    del bp
    sbp = cuda.createStereoBeliefPropagation(NDISP, ITERS, LEVELS, msg_type)
    rec["stereobp"] = dict(_stat(timed(lambda: sbp.compute(L, Rt, disp))), scratch_bytes=sbp.scratchBytes())
    del sbp
    torch.cuda.empty_cache()

    lib, st = capi.lib(), capi.current_stream_ptr
    p = cuda._csbp_params(msg_type, ndisp=NDISP)
    m = lambda t: C.byref(capi.mat_from_tensor(t))
    mk = lambda n, h, w, hi=8: (torch.rand((n * h, w), device=dev) * hi).to(T)
    image_bytes = 2 * rows * cols * CN
    # the coarsest level
    lv = LEVELS - 1
    h, w, n = rows >> lv, cols >> lv, NR_PLANE << lv
    temp, sel_cost, sel_disp = mk(NDISP, h, w), mk(n, h, w), mk(n, h, w)
    call = lambda: capi.check(lib.mi_stereocsbp_init_data_cost(C.byref(p), m(L), m(Rt), lv, n, m(temp), m(sel_cost), m(sel_disp), st()))
    rec["init_data_cost"] = dict(_stat(timed(call), image_bytes + NDISP * h * w * elem), level=lv, candidates=NDISP, planes=n)
    rec["data_cost"], rec["iteration"] = [], []
    n_launch = 10
    for lv in range(LEVELS - 1, -1, -1):
        h, w, n = rows >> lv, cols >> lv, NR_PLANE << lv
        if lv < LEVELS - 1:
            n2 = 2 * n
            parent, cost = mk(n2, h // 2, w // 2, 100), mk(n2, h, w)
            call = lambda: capi.check(lib.mi_stereocsbp_compute_data_cost(C.byref(p), m(L), m(Rt), lv, n2, m(parent), m(cost), st()))
            rec["data_cost"].append(dict(_stat(timed(call), image_bytes + n2 * (h * w + (h // 2) * (w // 2)) * elem), level=lv, candidates=n2))
            del parent, cost
        msgs = [mk(n, h, w) for _ in range(4)]
        mats = (capi.Mat * 4)(*[capi.mat_from_tensor(t) for t in msgs])
        sel_disp, sel_cost, temp = mk(n, h, w, 100), mk(n, h, w, 200), mk(n, h, w)
        one = 7.0 * n * elem * h * w
        entry = dict(level=lv, rows=h, cols=w, planes=n)
        for fname, form in (("reg", capi.MI_STEREOCSBP_FORM_REG), ("gen", capi.MI_STEREOCSBP_FORM_GEN)):
            call = lambda: capi.check(lib.mi_stereocsbp_iterate(C.byref(p), mats, m(sel_disp), m(sel_cost), m(temp), n, 0, n_launch, form, st()))
            t = np.array(timed(call)) / n_launch
            entry[fname] = _stat(t, one)
        rec["iteration"].append(entry)
        del msgs, mats, sel_disp, sel_cost, temp
        torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenarios", default=",".join(SCENARIOS))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stereocsbp", "stereocsbp.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("perf_stereocsbp: no GPU (there is no CPU fallback)")
    out = dict(device=torch.cuda.get_device_name(0), hbm_peak_bytes_per_s=HBM_PEAK, reps=a.reps, warmup=a.warmup, results=[])
    for name in a.scenarios.split(","):
        for msg in ("f32", "s16"):
            out["results"].append(run(name, msg, a.reps, a.warmup))
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
