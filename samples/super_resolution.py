"""BTV-L1 super-resolution through the Python mirror, in the calling pattern of the reference's own test
(superres/test/test_superres.cpp:223-274): configure, setInput, then nextFrame until the source is exhausted.

    python samples/super_resolution.py [frames=8] [scale=2] [iterations=100] [farneback|tvl1]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_frame(rows, cols, scale, ox, oy):
    y, x = np.mgrid[0:rows, 0:cols]
    X, Y = x * scale + ox, y * scale + oy
    v = 128 + 60 * np.sin(X * 0.05) * np.cos(Y * 0.04) + 30 * np.sin((X + Y) * 0.11)
    flat = ((X // 24) + (Y // 18)) % 3 == 0
    v = np.where(flat, 40 + 15 * ((X // 24) % 5), v)
    return np.clip(v, 0, 255).astype(np.uint8)


def main():
    import torch
    from opencv_contrib_amd import superres
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    scale = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    iterations = int(sys.argv[3]) if len(sys.argv) > 3 else 100
    dev = torch.device("cuda:0")
    frames = [torch.from_numpy(make_frame(120, 160, scale, (i * 3) % 5 - 2, (i * 2) % 5 - 2)).to(dev) for i in range(count)]

    sr = superres.createSuperResolution_BTVL1_CUDA()
    sr.setScale(scale)
    sr.setIterations(iterations)
    sr.setTemporalAreaRadius(2)
    if len(sys.argv) > 4 and sys.argv[4] == "tvl1":
        sr.setOpticalFlow(superres.createOptFlow_DualTVL1_CUDA())
    sr.setInput(superres.createFrameSource_List(frames))
    i = 0
    while (out := sr.nextFrame()) is not None:
        print(f"frame {i}: {out.shape[1]} x {out.shape[0]}, mean {out.float().mean().item():.2f}")
        i += 1


if __name__ == "__main__":
    main()
