"""Python twin of samples/track_corners.cpp: goodFeaturesToTrack in front of the sparse tracker.  detect's (1, N, 2) tensor goes to
SparsePyrLKOpticalFlow.calc as prevPts unchanged.  Needs an MI355X (there is no CPU fallback):  python samples/track_corners.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opencv_contrib_amd import capi, cuda, synth  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    I0, I1, gt = synth.flow_pair(240, 320, seed=1234, dtype="u8")
    t0, t1 = torch.from_numpy(I0).to(dev), torch.from_numpy(I1).to(dev)
    corners = cuda.createGoodFeaturesToTrackDetector(capi.MI_8UC1, maxCorners=200, qualityLevel=0.01, minDistance=8.0).detect(t0)
    nxt, status, _ = cuda.SparsePyrLKOpticalFlow.create().calc(t0, t1, corners)
    p = corners.cpu().numpy()[0]
    d = nxt.cpu().numpy()[0] - p
    g = gt[p[:, 1].astype(int), p[:, 0].astype(int)]
    ok = status.cpu().numpy()[0] > 0
    print(f"{len(p)} corners, strongest at {tuple(p[0])}; {int(ok.sum())} tracked, median error {np.median(np.hypot(*(d - g)[ok].T)):.3f} px")


if __name__ == "__main__":
    main()
