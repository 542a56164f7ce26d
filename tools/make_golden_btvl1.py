"""Writes tests/golden/btvl1_24x32.npz: the fixture that pins the NumPy restatement of BTV-L1 super-resolution
(tests/btvl1_numpy_ref.py).  Three 24 x 32 low-res frames (a shifted, degraded synthetic scene), their motions, the parameters and the
restatement's output after 5 iterations; tests/test_btvl1_ref.py checks that the restatement still reproduces it bit for bit.

    python tools/make_golden_btvl1.py        # rewrites the fixture: only when the restatement is MEANT to change
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import btvl1_numpy_ref as R  # noqa: E402

F = np.float32


def main():
    _, low, offs = R.synthetic_sequence(11, n=3, hh=48, hw=64, scale=2)
    frames = np.stack([f.astype(F) for f in low])
    rng = np.random.default_rng(12)
    fwd_a, bwd_a = R.analytic_motions(offs, low[0].shape, 2)
    wobble = lambda m: None if m is None else tuple((p + rng.uniform(-0.3, 0.3, p.shape)).astype(F) for p in m)   # not constant planes
    fwd_a, bwd_a = [wobble(m) for m in fwd_a], [wobble(m) for m in bwd_a]
    zero = np.zeros((2,) + low[0].shape, F)
    fwd = np.stack([zero if m is None else np.stack(m) for m in fwd_a])
    bwd = np.stack([zero if m is None else np.stack(m) for m in bwd_a])
    params = dict(scale=2, iterations=5, tau=1.3, lambda_=0.03, alpha=0.7, btv_kernel_size=7, blur_kernel_size=5, blur_sigma=0.0, base_idx=1)
    kw = dict(params)
    base = kw.pop("base_idx")
    out = R.process(list(frames), fwd_a, bwd_a, base, **kw)
    path = os.path.join(ROOT, "tests", "golden", "btvl1_24x32.npz")
    np.savez_compressed(path, frames=frames, fwd=fwd, bwd=bwd, params=np.array(json.dumps(params)), out=out)
    print(path, os.path.getsize(path), "bytes; output", out.shape)


if __name__ == "__main__":
    main()
