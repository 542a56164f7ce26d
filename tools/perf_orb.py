"""Times cv::cuda::ORB on the GPU and writes profiles/orb/orb.json (one JSON document; also printed).

Per size (640 x 480 and 1920 x 1080, the first frame of synth.flow_pair as CV_8UC1) and setting -- `defaults`: the class defaults with blur
(500 features, 8 levels, Harris score, blurForDescriptor), `perf4000`: the reference's perf case of 4 000 features (perf_features2d.cpp) --

  detect_and_compute  whole detectAndComputeAsync calls, read-back of the per-level counts included: host clock around a call that ends
                      in the stream wait (median, min, max us over --reps calls after --warmup calls);
  launch_floor        a chain of as many eager torch launches of a one-element kernel as the call enqueues (memset and copies counted as
                      one each), then a read-back through pinned memory and the stream wait.  Python-dispatch bound (about 6 us per
                      launch), so NOT a lower bound of a call whose launches come from one C++ loop: a yardstick of the same length only;
  fast_floor          the sum over the levels of FastFeatureDetector.detectAsync (threshold 20, suppression, max_npoints = 5 % of the
                      area) on an image of the level's size: the existing stage ORB runs at every level.  Each of these calls has a wait of
                      its own, which ORB's levels have not, and runs on a synthesised frame of the level's size, not on the resized level, so
                      candidate counts differ and the sum OVERSTATES FAST's share of an ORB call.
  --single            one call per setting at 1920 x 1080 and nothing else: the run a kernel trace is taken of.

The stages are not timed alone here; profiles/orb/README.md has the kernel trace.  There is no CPU fallback: without a device this fails.

    python tools/perf_orb.py [--reps 100] [--warmup 10] [--out profiles/orb/orb.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = {"vga": (480, 640), "hd1080": (1080, 1920)}
SETTINGS = {"defaults": dict(nfeatures=500, blurForDescriptor=True), "perf4000": dict(nfeatures=4000)}


def _stat(us):
    return dict(median=float(np.median(us)), min=float(np.min(us)), max=float(np.max(us)))


def _host_timed(fn, reps, warmup):
    """fn ends in a stream wait: the host clock around it is the call's time"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        us.append((time.perf_counter() - t0) * 1e6)
    return us


def launches_of(levels, harris, blur):
    """what orb_plan.h lists for a call whose levels all hold keypoints: clear + table copy, a level kernel and FAST's four per level, five
    per cull, Harris, angle, a blur per level, descriptors, merge, the read-back's copy"""
    ncull = 2 if harris else 1
    return 2 + levels * (1 + 4) + 5 * ncull + (1 if harris else 0) + 1 + (levels if blur else 0) + 1 + 1 + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--single", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orb", "orb.json"))
    a = ap.parse_args()
    import torch
    import orb_numpy_ref as R
    from opencv_contrib_amd import cuda, synth
    assert torch.cuda.is_available(), "no GPU: nothing is measured without one"
    dev = torch.device("cuda:0")
    if a.single:
        t = torch.from_numpy(np.ascontiguousarray(synth.flow_pair(1080, 1920, seed=11, dtype="u8")[0])).to(dev)
        for kw in SETTINGS.values():
            kp, _ = cuda.ORB.create(**kw).detectAndComputeAsync(t)
            print(kw, int(kp.shape[1]))
        return
    one = torch.zeros(1, dtype=torch.int32, device=dev)
    cnt = torch.zeros(128, dtype=torch.int32, device=dev)
    pinned = torch.zeros(128, dtype=torch.int32).pin_memory()
    stream = torch.cuda.current_stream()

    def launch_floor(launches):
        def f():
            for _ in range(launches):
                one.add_(1)                        # one element: the launch is the cost
            pinned.copy_(cnt, non_blocking=True)   # the counts' read-back
            stream.synchronize()
        return f

    doc = dict(device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, sizes={})
    for name, (rows, cols) in SIZES.items():
        img = np.ascontiguousarray(synth.flow_pair(rows, cols, seed=11, dtype="u8")[0])
        t = torch.from_numpy(img).to(dev)
        geo = R.level_geometry(rows, cols, R.DEFAULTS)
        fast_us, fast_kp = 0.0, []
        for g in geo:
            lt = torch.from_numpy(np.ascontiguousarray(synth.flow_pair(g["rows"], g["cols"], seed=11, dtype="u8")[0])).to(dev)
            det = cuda.FastFeatureDetector.create(20, True, max_npoints=int(0.05 * g["rows"] * g["cols"]))
            fast_kp.append(int(det.detectAsync(lt).shape[1]))
            fast_us += float(np.median(_host_timed(lambda: det.detectAsync(lt), a.reps, a.warmup)))
        rec = dict(rows=rows, cols=cols, levels=[(g["rows"], g["cols"]) for g in geo], fast_floor_us=fast_us, fast_keypoints=fast_kp)
        for sname, kw in SETTINGS.items():
            orb = cuda.ORB.create(**kw)
            kp, desc = orb.detectAndComputeAsync(t)
            us = _stat(_host_timed(lambda: orb.detectAndComputeAsync(t), a.reps, a.warmup))
            n = launches_of(len(geo), True, bool(kw.get("blurForDescriptor")))
            lf = _stat(_host_timed(launch_floor(n), a.reps, a.warmup))
            per_level = np.bincount(kp[4].cpu().numpy().astype(np.int64), minlength=len(geo)).tolist()
            rec[sname] = dict(params=kw, keypoints=int(kp.shape[1]), keypoints_per_level=per_level, launches=n, detect_and_compute_us=us,
                              launch_floor_us=lf, over_launch_floor=us["median"] / lf["median"], over_fast_floor=us["median"] / fast_us,
                              scratch_bytes=orb.scratchBytes())
        doc["sizes"][name] = rec
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
