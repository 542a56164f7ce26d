"""Times cv::cuda::StereoBeliefPropagation on the GPU and writes profiles/stereobp/stereobp.json (one JSON document; also printed).

Scenarios: the reference's perf test size (cudastereo/perf/perf_stereo.cpp StereoBeliefPropagation: a 640 x 480 colour pair, class
defaults ndisp 64, iters 5, levels 5) and 1920 x 1080 with ndisp 128; both message types.  Per scenario:

  compute      whole compute(left, right) calls, each bracketed by device events after warm-up calls (median, min, max ms);
  iteration    ONE level-0 half-sweep of the iteration kernel through the stage entry, in every form that takes the ndisp (register
               form for ndisp <= 64, general form always): events around a block of alternating-parity launches, ms per launch.

Bytes are derived from the code, not measured: a half-sweep updates half the pixels, and an updated pixel moves 9 ndisp sizeof(T) bytes
(four neighbour messages and the data cost read, four messages written), so 4.5 ndisp sizeof(T) per pixel of the level.  Over a whole
compute the iterations of all levels move  iters * sum_l 4.5 ndisp sizeof(T) rows_l cols_l.  The share of peak is of the 8.0 TB/s HBM3E
specification; it is a bandwidth bound (the kernel does ~15 f32 operations per 36 bytes).  There is no CPU fallback: without a device this fails.

    python tools/perf_stereobp.py [--reps 20] [--warmup 3] [--out profiles/stereobp/stereobp.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
CV_16S, CV_32F = 3, 5
SCENARIOS = {   # name: rows, cols, channels, ndisp, iters, levels
    "vga_defaults": (480, 640, 3, 64, 5, 5),
    "hd_nd128": (1080, 1920, 3, 128, 5, 5),
}


def iteration_bytes(rows, cols, ndisp, elem):
    """bytes one half-sweep of a rows x cols level moves: 9 ndisp sizeof(T) per updated pixel, half the pixels updated"""
    return 4.5 * ndisp * elem * rows * cols


def compute_iteration_bytes(rows, cols, ndisp, elem, iters, levels):
    total = 0.0
    for _ in range(levels):
        total += iters * iteration_bytes(rows, cols, ndisp, elem)
        rows, cols = (rows + 1) // 2, (cols + 1) // 2
    return total


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


def run(name, msg, reps, warmup):
    import torch
    from opencv_contrib_amd import cuda, capi
    rows, cols, cn, ndisp, iters, levels = SCENARIOS[name]
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    left = rng.integers(0, 256, (rows, cols, cn), dtype=np.uint8)
    right = np.roll(left, -7, 1)
    L, Rt = torch.from_numpy(left).to(dev), torch.from_numpy(np.ascontiguousarray(right)).to(dev)
    msg_type = CV_32F if msg == "f32" else CV_16S
    elem = 4 if msg == "f32" else 2
    bp = cuda.createStereoBeliefPropagation(ndisp, iters, levels, msg_type)
    disp = torch.empty((rows, cols), dtype=torch.int16, device=dev)
    for _ in range(warmup):
        bp.compute(L, Rt, disp)
    torch.cuda.synchronize()
    t = _events(lambda: bp.compute(L, Rt, disp), reps)
    it_bytes = compute_iteration_bytes(rows, cols, ndisp, elem, iters, levels)
    rec = dict(scenario=name, msg=msg, rows=rows, cols=cols, channels=cn, ndisp=ndisp, iters=iters, levels=levels,
               compute_ms=dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t))),
               compute_iteration_bytes=it_bytes, scratch_bytes=bp.scratchBytes(),
               compute_iteration_bytes_per_s=it_bytes / (float(np.median(t)) * 1e-3), iteration={})
    rec["compute_share_of_hbm_peak"] = rec["compute_iteration_bytes_per_s"] / HBM_PEAK
    del bp
    # one level-0 half-sweep per form, on messages and data of the level's size
    T = torch.float32 if msg == "f32" else torch.int16
    shape = (ndisp * rows, cols)
    mk = (lambda: (torch.rand(shape, device=dev) * 8).to(T))
    msgs, data = [mk() for _ in range(4)], mk()
    mats = (capi.Mat * 4)(*[capi.mat_from_tensor(m) for m in msgs])
    dmat = capi.mat_from_tensor(data)
    import ctypes as C
    p = capi.StereoBPParams()
    capi.lib().mi_stereobp_default_params(C.byref(p))
    p.ndisp, p.msg_type = ndisp, msg_type
    n_launch = 10
    forms = [("reg", capi.MI_STEREOBP_FORM_REG)] if ndisp <= 64 else []
    forms.append(("gen", capi.MI_STEREOBP_FORM_GEN))
    one = iteration_bytes(rows, cols, ndisp, elem)
    for fname, form in forms:
        call = lambda: capi.check(capi.lib().mi_stereobp_iterate(C.byref(p), mats, C.byref(dmat), 0, n_launch, form, capi.current_stream_ptr()))
        for _ in range(warmup):
            call()
        torch.cuda.synchronize()
        t = np.array(_events(call, reps)) / n_launch
        rec["iteration"][fname] = dict(ms_per_half_sweep=dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t))),
                                       bytes=one, bytes_per_s=one / (float(np.median(t)) * 1e-3),
                                       share_of_hbm_peak=one / (float(np.median(t)) * 1e-3) / HBM_PEAK)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenarios", default=",".join(SCENARIOS))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stereobp", "stereobp.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("perf_stereobp: no GPU (there is no CPU fallback)")
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
