"""Writes tests/golden/btvl1_24x32.npz: the fixture that pins the NumPy restatement of BTV-L1 super-resolution
(tests/btvl1_numpy_ref.py).  Three 24 x 32 low-res frames (a shifted, degraded synthetic scene), their motions, the parameters and the
restatement's output after 5 iterations; tests/test_btvl1_ref.py checks that the restatement still reproduces it bit for bit.

    python tools/make_golden_btvl1.py        # rewrites the fixture: only when the restatement is MEANT to change

    python tools/make_golden_btvl1.py --refclass
writes tests/golden/btvl1_refclass_*.npz instead: small cases whose `out` is what the REFERENCE's own class computed -- BTVL1_CUDA_Base::
process of superres/src/btv_l1_cuda.cpp over the reference's kernels, executed on the host from oracle/_ref/libref_cu.so (oracle/Makefile.ref;
needs the reference tree).  Data the reference's programs wrote: tests/test_ref_pin_btvl1.py holds the restatement to it everywhere, and
the reference library where it is present.
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


REFCLASS_CASES = [   # name, seed, low-res h x w, channels, frames, base, parameters
    ("c1_s2", 21, 20, 28, 1, 3, 1, dict(scale=2, iterations=5, tau=1.3, lambda_=0.03, alpha=0.7, btv_kernel_size=7, blur_kernel_size=5, blur_sigma=0.0)),
    ("c4_s3", 22, 14, 18, 4, 3, 2, dict(scale=3, iterations=4, tau=1.3, lambda_=0.03, alpha=0.7, btv_kernel_size=7, blur_kernel_size=5, blur_sigma=0.0)),
    ("c3_s4", 23, 12, 15, 3, 2, 0, dict(scale=4, iterations=3, tau=0.9, lambda_=0.1, alpha=0.55, btv_kernel_size=3, blur_kernel_size=9, blur_sigma=1.2)),
]


def refclass():
    sys.path.insert(0, ROOT)
    from oracle import refcu
    from test_btvl1_gpu import make_case
    for name, seed, lh, lw, cn, K, base, kw in REFCLASS_CASES:
        frames, fwd_a, bwd_a = make_case(seed, lh, lw, cn, K, amp=3.0)
        out, _ = refcu.cuda_class_btvl1_process(frames, fwd_a, bwd_a, base, **kw)
        zero = np.zeros((2, lh, lw), F)
        fwd = np.stack([zero if m is None else np.stack(m) for m in fwd_a])
        bwd = np.stack([zero if m is None else np.stack(m) for m in bwd_a])
        path = os.path.join(ROOT, "tests", "golden", f"btvl1_refclass_{name}.npz")
        np.savez_compressed(path, frames=np.stack(frames), fwd=fwd, bwd=bwd, params=np.array(json.dumps(dict(kw, base_idx=base))), out=out)
        print(path, os.path.getsize(path), "bytes; output", out.shape)


if __name__ == "__main__":
    refclass() if "--refclass" in sys.argv[1:] else main()
