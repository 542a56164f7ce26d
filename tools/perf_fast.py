"""Times cv::cuda::FastFeatureDetector on the GPU and writes profiles/fast/fast.json (one JSON document; also printed).

Per size (640 x 480, 1920 x 1080, 3840 x 2160, the first frame of synth.flow_pair as CV_8UC1), with suppression and without, at the class
defaults (threshold 10, max_npoints 5000):

  detect        whole detectAsync calls, read-back of the count included: host clock around a call that ends in the stream wait
                (median, min, max us over --reps calls after --warmup calls);
  detect_batch  16 frames of 1920 x 1080 in one call, one read-back: us per call and per frame;
  launch_floor  a chain of as many launches of a one-element kernel as the plan lists for a detect (4 with suppression, 3 without), then the
                same read-back of two ints through pinned memory and the stream wait: what the call costs when the kernels do nothing;
  copy_floor    a device-to-device copy of 3 bytes per pixel (the bytes a detect moves: image read, byte plane written and read again),
                device events around --reps copies.

Both floors are taken in the same process on the same device as the times they are compared with.  `sits_on` names the larger floor.
There is no CPU fallback: without a device this fails.

    python tools/perf_fast.py [--reps 200] [--warmup 20] [--out profiles/fast/fast.json]
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
BATCH = 16


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fast", "fast.json"))
    a = ap.parse_args()
    import torch
    from opencv_contrib_amd import cuda, synth
    assert torch.cuda.is_available(), "no GPU: nothing is measured without one"
    dev = torch.device("cuda:0")
    one = torch.zeros(1, dtype=torch.int32, device=dev)
    two = torch.zeros(2, dtype=torch.int32, device=dev)
    pinned = torch.zeros(2, dtype=torch.int32).pin_memory()
    stream = torch.cuda.current_stream()

    def launch_floor(launches):
        def f():
            for _ in range(launches):
                one.add_(1)                        # one element: the launch is the cost
            pinned.copy_(two, non_blocking=True)   # the count's read-back
            stream.synchronize()
        return f

    floors = {n: _stat(_host_timed(launch_floor(n), a.reps, a.warmup)) for n in (3, 4)}
    doc = dict(device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, threshold=10, max_npoints=5000,
               launch_floor_us={str(n): floors[n] for n in floors}, sizes={})
    frames = {}
    for name, (rows, cols) in SIZES.items():
        img = np.ascontiguousarray(synth.flow_pair(rows, cols, seed=11, dtype="u8")[0])
        t = torch.from_numpy(img).to(dev)
        frames[name] = t
        src = torch.empty(3 * rows * cols, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        for _ in range(a.warmup):
            dst.copy_(src)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            dst.copy_(src)
        e1.record()
        e1.synchronize()
        copy_us = e0.elapsed_time(e1) * 1e3 / a.reps
        rec = dict(rows=rows, cols=cols, copy_floor_us=copy_us, copy_bytes=3 * rows * cols)
        for nms in (True, False):
            det = cuda.FastFeatureDetector.create(10, nms)
            kp = det.detectAsync(t)
            us = _stat(_host_timed(lambda: det.detectAsync(t), a.reps, a.warmup))
            lf = floors[4 if nms else 3]["median"]
            rec["nms" if nms else "raw"] = dict(keypoints=int(kp.shape[1]), launches=4 if nms else 3, detect_us=us, launch_floor_us=lf,
                                                sits_on="launch_floor" if lf >= copy_us else "copy_floor",
                                                over_larger_floor=us["median"] / max(lf, copy_us), scratch_bytes=det.scratchBytes())
        doc["sizes"][name] = rec
    batch = [frames["hd1080"]] * BATCH
    rec = {}
    for nms in (True, False):
        det = cuda.FastFeatureDetector.create(10, nms)
        us = _stat(_host_timed(lambda: det.detect_batch(batch), max(10, a.reps // 10), 3))
        rec["nms" if nms else "raw"] = dict(frames=BATCH, launches=BATCH * (4 if nms else 3), call_us=us, per_frame_us=us["median"] / BATCH)
    doc["detect_batch_hd1080"] = rec
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
