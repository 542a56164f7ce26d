"""Times cv::cuda::CornersDetector (goodFeaturesToTrack) on the GPU and writes profiles/gftt/gftt.json (one JSON document; also printed).

Per size (640 x 480, 1920 x 1080, 3840 x 2160, the first frame of synth.flow_pair as CV_8UC1), MinEigenVal and Harris, minDistance 0 and 3,
at the factory's defaults otherwise (maxCorners 1000, qualityLevel 0.01, blockSize 3):

  detect        whole detect calls, read-back included: host clock around a call that ends in the stream wait (median, min, max us over
                --reps calls after --warmup calls).  With minDistance 3 the sorted points come to the host, the grid loop runs there and
                the survivors go back, inside the call;
  launch_floor  a chain of as many launches of a one-element kernel as the plan lists for a detect at that size (the sort is launched for
                the capacity, so the count grows with the image), then a read-back of eight ints through pinned memory and the stream
                wait: what the call costs when the kernels do nothing;
  copy_floor    a device-to-device copy of the bytes the response kernel moves (1 read and 4 written per pixel), device events around
                --reps copies;
  response      the criterion's compute alone (one launch), device events around --reps calls: us, and the bytes above per second beside
                the HBM peak;
  host_loop     the minDistance grid loop alone on the host (mi_gftt_min_distance) on the candidates the frame gives, for minDistance 3.

Both floors are taken in the same process on the same device as the times they are compared with.  There is no CPU fallback: without
a device this fails.  With --trace-only it runs 5 warm-up and 20 timed detects per case and writes nothing: the form a kernel trace is
taken of, in a run of its own.

    python tools/perf_gftt.py [--reps 200] [--warmup 20] [--out profiles/gftt/gftt.json] [--trace-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = {"vga": (480, 640), "hd1080": (1080, 1920), "uhd2160": (2160, 3840)}
HBM_PEAK_BYTES_PER_S = 8.0e12   # MI355X: 8 HBM3E stacks, 8 TB/s
SORT_TILE = 4096                # GFTT_SORT_TILE of opencv_contrib_amd/csrc/gftt_plan.h


def plan_launches(rows, cols):
    """the launch list of gftt_make_plan at blockSize 3: response, threshold, find, scan, emit, the sort for the capacity, points"""
    cap = max(1000, int(rows * cols * 0.05))
    sort_cap = SORT_TILE
    while sort_cap < cap:
        sort_cap *= 2
    levels = (sort_cap // SORT_TILE).bit_length() - 1
    return 5 + (1 + levels + levels * (levels + 1) // 2) + 1, cap


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


def _event_timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gftt", "gftt.json"))
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    import torch
    from opencv_contrib_amd import capi, cuda, synth
    assert torch.cuda.is_available(), "no GPU: nothing is measured without one"
    dev = torch.device("cuda:0")
    if a.trace_only:
        a.reps, a.warmup = 20, 5
    one = torch.zeros(1, dtype=torch.int32, device=dev)
    eight = torch.zeros(8, dtype=torch.int32, device=dev)
    pinned = torch.zeros(8, dtype=torch.int32).pin_memory()
    stream = torch.cuda.current_stream()

    def launch_floor(launches):
        def f():
            for _ in range(launches):
                one.add_(1)                          # one element: the launch is the cost
            pinned.copy_(eight, non_blocking=True)   # the control block's read-back
            stream.synchronize()
        return f

    doc = dict(device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, max_corners=1000, quality_level=0.01, block_size=3,
               hbm_peak_bytes_per_s=HBM_PEAK_BYTES_PER_S, sizes={})
    for name, (rows, cols) in SIZES.items():
        img = np.ascontiguousarray(synth.flow_pair(rows, cols, seed=11, dtype="u8")[0])
        t = torch.from_numpy(img).to(dev)
        launches, cap = plan_launches(rows, cols)
        rec = dict(rows=rows, cols=cols, capacity=cap, launches=launches)
        if not a.trace_only:
            rec["launch_floor_us"] = _stat(_host_timed(launch_floor(launches), a.reps, a.warmup))
            nbytes = 5 * rows * cols
            src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            rec["copy_floor_us"] = _event_timed(lambda: dst.copy_(src), a.reps, a.warmup)
            rec["response_bytes"] = nbytes
        for harris in (False, True):
            crit = cuda.createHarrisCorner(capi.MI_8UC1, 3, 3, 0.04) if harris else cuda.createMinEigenValCorner(capi.MI_8UC1, 3, 3)
            plane = torch.empty((rows, cols), dtype=torch.float32, device=dev)
            r_us = _event_timed(lambda: crit.compute(t, plane), a.reps, a.warmup)
            crec = dict(response_us=r_us, response_bytes_per_s=5 * rows * cols / (r_us * 1e-6),
                        response_share_of_hbm_peak=5 * rows * cols / (r_us * 1e-6) / HBM_PEAK_BYTES_PER_S)
            every = cuda.createGoodFeaturesToTrackDetector(capi.MI_8UC1, 0, 0.01, 0.0, 3, harris).detect(t)
            crec["candidates"] = int(every.shape[1])
            for md in (0.0, 3.0):
                det = cuda.createGoodFeaturesToTrackDetector(capi.MI_8UC1, 1000, 0.01, md, 3, harris)
                n = int(det.detect(t).shape[1])
                us = _stat(_host_timed(lambda: det.detect(t), a.reps, a.warmup))
                d = dict(corners=n, detect_us=us, scratch_bytes=det.scratchBytes())
                if not a.trace_only:
                    d["over_launch_floor"] = us["median"] / rec["launch_floor_us"]["median"]
                if md >= 1:
                    pts = every.cpu().numpy()[0]
                    d["host_loop_us"] = _stat(_host_timed(lambda: cuda.gftt_min_distance(pts, rows, cols, md, 1000), max(10, a.reps // 4), 3))
                crec[f"min_distance_{md:g}"] = d
            rec["harris" if harris else "min_eigen_val"] = crec
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
