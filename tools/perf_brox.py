"""Times cv::cuda::BroxOpticalFlow on the GPU and writes profiles/brox/brox.json (one JSON document; also printed).

Per size (640 x 480 and 1920 x 1080, a pair of synth.flow_pair as CV_32FC1), with the class defaults (0.197, 50, 0.8, 5, 150, 10) and
with the superres adapter's parameters (0.197, 50, 0.8, 10, 77, 10), in the plain and in the blocked form of the solver, the two
forms alternating call by call:

  calc            whole calc calls: host clock around a call followed by the stream wait (median, min, max ms over --reps calls after
                  --warmup calls);
  launch_floor    a chain of as many launches of a one-element kernel as the plan lists for that calc, then the stream wait: what the
                  call costs when the kernels do nothing;
  sor_iteration   ms per solver iteration of the finest level in each form: the stage entry (which allocates, launches and waits) with
                  60 and with 20 iterations, the difference over 40 (median of --reps differences), so its fixed costs cancel;
  bytes           the algorithmic bytes of a solver iteration: the eleven planes a pixel's update reads (u, v, du, dv, two diffusivities,
                  two inverse denominators, three numerators) and the two it writes, once per iteration = 52 bytes a pixel, over the
                  measured time, beside the HBM peak.  The plain form moves twice that (every plane once per half-pass).

The number of launches is the plan's own (mi_brox_plan_info; opencv_contrib_amd/csrc/brox_plan.h).  There is no CPU fallback: without
a device this fails.  With --trace-only it runs 1 warm-up and 3 timed calcs per case and writes nothing: the form a kernel trace is taken of, in a run of its own.

    python tools/perf_brox.py [--reps 10] [--warmup 3] [--out profiles/brox/brox.json] [--trace-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = {"vga": (480, 640), "hd1080": (1080, 1920)}
PARAMS = {"defaults": dict(alpha=0.197, gamma=50.0, scale_factor=0.8, inner_iterations=5, outer_iterations=150, solver_iterations=10),
          "superres": dict(alpha=0.197, gamma=50.0, scale_factor=0.8, inner_iterations=10, outer_iterations=77, solver_iterations=10)}
FORMS = {"plain": 1, "blocked": 2}
HBM_PEAK_BYTES_PER_S = 8.0e12   # MI355X: 8 HBM3E stacks, 8 TB/s
SOR_BYTES_PER_PIXEL = 13 * 4


def plan_launches(rows, cols, p, form):
    """the library's own plan (mi_brox_plan_info, host only) -> (launches, levels)"""
    from opencv_contrib_amd import cuda
    levels, launches, _ = cuda.brox_plan_info(rows, cols, FORMS[form], **p)
    return launches, levels


def _stat(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "brox", "brox.json"))
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    import torch
    from opencv_contrib_amd import cuda, synth
    assert torch.cuda.is_available(), "no GPU: nothing is measured without one"
    dev = torch.device("cuda:0")
    if a.trace_only:
        a.reps, a.warmup = 3, 1
    one = torch.zeros(1, dtype=torch.int32, device=dev)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    doc = dict(device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, hbm_peak_bytes_per_s=HBM_PEAK_BYTES_PER_S,
               sor_bytes_per_pixel_per_iteration=SOR_BYTES_PER_PIXEL, sizes={})
    for name, (rows, cols) in SIZES.items():
        i0, i1, _ = synth.flow_pair(rows, cols, seed=11)
        t0, t1 = torch.from_numpy(np.ascontiguousarray(i0)).to(dev), torch.from_numpy(np.ascontiguousarray(i1)).to(dev)
        flow = torch.empty((rows, cols, 2), dtype=torch.float32, device=dev)
        rec = dict(rows=rows, cols=cols)
        for pname, p in PARAMS.items():
            algs = {}
            for fname, form in FORMS.items():
                algs[fname] = cuda.BroxOpticalFlow.create(**p)
                algs[fname].setSolverForm(form)
            for _ in range(a.warmup):
                for alg in algs.values():
                    alg.calc(t0, t1, flow)
            torch.cuda.synchronize()
            ms = {f: [] for f in FORMS}
            outs = {}
            for _ in range(a.reps):
                for f, alg in algs.items():   # alternating: both forms see the same machine
                    ms[f].append(timed(lambda: alg.calc(t0, t1, flow)))
                    outs[f] = flow.clone()
            assert torch.equal(outs["plain"].view(torch.int32), outs["blocked"].view(torch.int32)), "the two forms differ"
            prec = dict(params=p, finite=bool(torch.isfinite(outs["plain"]).all()))
            for f in FORMS:
                launches, levels = plan_launches(rows, cols, p, f)
                d = dict(calc_ms=_stat(ms[f]), launches=launches, levels=levels, scratch_bytes=algs[f].scratchBytes())
                if not a.trace_only:
                    def floor():
                        for _ in range(launches):
                            one.add_(1)   # one element: the launch is the cost
                    for _ in range(2):
                        floor()
                    torch.cuda.synchronize()
                    d["launch_floor_ms"] = _stat([timed(floor) for _ in range(max(3, a.reps // 2))])
                prec[f] = d
            rec[pname] = prec
        if not a.trace_only:
            # the solver alone on the finest level: coefficients of the first inner iteration of a zero flow
            z = torch.zeros((rows, cols), dtype=torch.float32, device=dev)
            d = cuda.brox_derivatives(t0, t1)
            images = [t0, t1, d[2], d[4], d[0], d[3], d[5], d[1], d[6]]   # I0, I1, Ix, Ixx, Ix0, Iy, Iyy, Iy0, Ixy
            co = cuda.brox_prepare(z, z, z, z, images, 0.197, 50.0)
            srec = {}
            for f, form in FORMS.items():
                du, dv = torch.zeros_like(z), torch.zeros_like(z)
                run = lambda n: timed(lambda: cuda.brox_sor(z, z, du, dv, co, n, form))
                for _ in range(a.warmup):
                    run(20), run(60)
                per = [(run(60) - run(20)) / 40.0 for _ in range(a.reps)]
                m = float(np.median(per))
                bps = SOR_BYTES_PER_PIXEL * rows * cols / (m * 1e-3)
                srec[f] = dict(ms_per_iteration=_stat(per), algorithmic_bytes_per_s=bps, share_of_hbm_peak=bps / HBM_PEAK_BYTES_PER_S)
            rec["sor_iteration"] = srec
        doc["sizes"][name] = rec
    if a.trace_only:
        return
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
