"""Writes tests/golden/stereobp_refclass_*.npz and stereobp_refstage_*.npz: what the REFERENCE's own StereoBeliefPropagation computed.

The reference's kernels (modules/cudastereo/src/cuda/stereobp.cu, rewritten only at their launch sites by oracle/refshim/cu2host.py and run
on the host through oracle/refshim/cudashim) and its host class (modules/cudastereo/src/stereobp.cpp, compiled as it lies against the stub
core of oracle/refshim/cudahost) are built from the reference tree into a temporary directory; tools/stereobp_ref/ holds the C entry
points and the three pieces the stubs lack.  Only the recorded inputs and outputs are kept.

    python tools/make_golden_stereobp.py            # needs the reference tree (REF, default /root/reference)

  refclass: inputs, parameters and the disparity of the class (compute(left, right) and compute(data)).
  refstage: inputs and outputs of every kernel wrapper on its own, chained: comp_data -> data_step_down; level_up of random coarse
            messages; calc_all_iterations for 1 and 2 iterations (both parities); output.
tests/test_stereobp_ref.py holds the NumPy restatement to these files everywhere and rebuilds them where the reference tree is present;
tests/test_stereobp_gpu.py holds the HIP class and its stage entries to them.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REF", "/root/reference")
SHIM = os.path.join(ROOT, "oracle", "refshim")
HERE = os.path.join(ROOT, "tools", "stereobp_ref")
GOLDEN = os.path.join(ROOT, "tests", "golden")
F = np.float32
CV_16S, CV_32F = 3, 5
MSG = {"f32": CV_32F, "s16": CV_16S}
DEFAULT_W = dict(max_data_term=10.0, data_weight=0.07, max_disc_term=1.7, disc_single_jump=1.0)
OTHER_W = dict(max_data_term=14.5, data_weight=0.11, max_disc_term=2.3, disc_single_jump=0.65)


def have_reference():
    return os.path.exists(os.path.join(REF, "modules", "cudastereo", "src", "cuda", "stereobp.cu"))


def build(outdir):
    """Compiles the reference's stereobp.cu and stereobp.cpp for the host into `outdir` (outside the repository) -> the library's path."""
    out = lambda n: os.path.join(outdir, n)
    cs = os.path.join(REF, "modules", "cudastereo")
    common = ["-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-w"]
    cu = common + ["-I" + os.path.join(HERE, "cu"), "-I" + os.path.join(SHIM, "cudashim"), "-include", os.path.join(SHIM, "cudashim", "cudashim.h")]
    ch = common + ["-fno-gnu-unique", "-I" + HERE, "-I" + os.path.join(SHIM, "cudahost"), "-I" + os.path.join(SHIM, "cudashim"),
                   "-I" + os.path.join(cs, "include")]
    steps = [
        [sys.executable, os.path.join(SHIM, "cu2host.py"), os.path.join(cs, "src", "cuda", "stereobp.cu"), out("stereobp.gen.cpp")],
        ["g++"] + cu + ["-c", out("stereobp.gen.cpp"), "-o", out("stereobp.gen.o")],
        ["g++"] + cu + ["-c", os.path.join(HERE, "sbp_ref_stage.cpp"), "-o", out("sbp_ref_stage.o")],
        ["g++"] + cu + ["-c", os.path.join(SHIM, "cudashim", "cudashim.cpp"), "-o", out("cudashim.o")],
        ["g++"] + ch + ["-c", os.path.join(cs, "src", "stereobp.cpp"), "-o", out("stereobp_host.o")],
        ["g++"] + ch + ["-c", os.path.join(HERE, "sbp_ref_class.cpp"), "-o", out("sbp_ref_class.o")],
        ["gcc", "-O2", "-fPIC", "-fopenmp", "-ffp-contract=off", "-c", os.path.join(SHIM, "oclrt.c"), "-o", out("oclrt.o")],
        ["g++", "-shared", "-fopenmp", "-o", out("libsbp_ref.so"), out("stereobp.gen.o"), out("sbp_ref_stage.o"), out("cudashim.o"),
         out("stereobp_host.o"), out("sbp_ref_class.o"), out("oclrt.o"), "-lm", "-Wl,--no-undefined"],
    ]
    for cmd in steps:
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(" ".join(cmd) + "\n" + r.stdout + r.stderr)
    return out("libsbp_ref.so")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Ref:
    """ctypes binding of the library build() makes"""

    def __init__(self, path):
        self.L = C.CDLL(path)

    @staticmethod
    def _w(weights):
        w = dict(DEFAULT_W, **weights)
        return (C.c_float * 4)(w["max_data_term"], w["data_weight"], w["max_disc_term"], w["disc_single_jump"])

    def compute(self, left, right, ndisp, iters, levels, msg_type, weights, out_dtype=np.int16):
        """-> the class's disparity, or None if it threw"""
        left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
        rows, cols = left.shape[:2]
        cn = 1 if left.ndim == 2 else left.shape[2]
        if right.shape != left.shape:
            rcn = 1 if right.ndim == 2 else right.shape[2]
            rc = self.L.sbp_ref_compute_mismatched(rows, cols, cn, right.shape[0], right.shape[1], rcn, ndisp, iters, levels, msg_type)
            assert rc == 1
            return None
        out_type = {np.uint8: 0, np.int16: 3, np.int32: 4, np.float32: 5}[out_dtype]
        disp = np.empty((rows, cols), out_dtype)
        rc = self.L.sbp_ref_compute(_p(left), _p(right), rows, cols, cn, ndisp, iters, levels, msg_type, self._w(weights), out_type, _p(disp))
        assert rc in (0, 1), rc
        return disp if rc == 0 else None

    def compute_data(self, data, ndisp, iters, levels, msg_type, weights):
        data = np.ascontiguousarray(data)
        data_type = {np.dtype(np.int16): 3, np.dtype(np.float32): 5, np.dtype(np.uint8): 0}[data.dtype]
        disp = np.empty((data.shape[0] // max(ndisp, 1), data.shape[1]), np.int16)
        rc = self.L.sbp_ref_compute_data(_p(data), data.shape[0], data.shape[1], data_type, ndisp, iters, levels, msg_type, self._w(weights), _p(disp))
        assert rc in (0, 1), rc
        return disp if rc == 0 else None

    def estimate(self, width, height):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self.L.sbp_ref_estimate(width, height, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    # ---- the kernel wrappers; planar matrices (ndisp * rows, cols)
    def load_constants(self, ndisp, msg_type, weights):
        w = dict(DEFAULT_W, **weights)
        scale = F(1.0) if msg_type == CV_32F else F(10.0)   # stereobp.cpp:176,271
        self.L.sbp_ref_load_constants(ndisp, C.c_float(w["max_data_term"]), C.c_float(scale * F(w["data_weight"])),
                                      C.c_float(scale * F(w["max_disc_term"])), C.c_float(scale * F(w["disc_single_jump"])))

    def comp_data(self, left, right, ndisp, msg_type):
        rows, cols = left.shape[:2]
        cn = 1 if left.ndim == 2 else left.shape[2]
        data = np.zeros((ndisp * rows, cols), np.float32 if msg_type == CV_32F else np.int16)
        assert self.L.sbp_ref_comp_data(_p(np.ascontiguousarray(left)), _p(np.ascontiguousarray(right)), rows, cols, cn, int(msg_type == CV_32F), ndisp, _p(data)) == 0
        return data

    def step_down(self, src, ndisp):
        rows, cols = src.shape[0] // ndisp, src.shape[1]
        dst = np.zeros((ndisp * ((rows + 1) // 2), (cols + 1) // 2), src.dtype)
        self.L.sbp_ref_step_down(int(src.dtype == np.float32), ndisp, _p(src), rows, cols, _p(dst), (rows + 1) // 2, (cols + 1) // 2)
        return dst

    def level_up(self, coarse, ndisp, rows, cols):
        coarse = np.ascontiguousarray(coarse)
        dst = np.zeros((4, ndisp * rows, cols), coarse.dtype)
        self.L.sbp_ref_level_up(int(coarse.dtype == np.float32), ndisp, _p(coarse), coarse.shape[1] // ndisp, coarse.shape[2], _p(dst), rows, cols)
        return dst

    def iterations(self, msgs, data, ndisp, iters):
        out = np.ascontiguousarray(msgs).copy()
        self.L.sbp_ref_iterations(int(out.dtype == np.float32), ndisp, _p(out), _p(np.ascontiguousarray(data)), data.shape[0] // ndisp, data.shape[1], iters)
        return out

    def output(self, msgs, data, ndisp):
        disp = np.full((data.shape[0] // ndisp, data.shape[1]), 0, np.int16)   # the class zeroes the map first (stereobp.cpp:353)
        self.L.sbp_ref_output(int(data.dtype == np.float32), ndisp, _p(np.ascontiguousarray(msgs)), _p(np.ascontiguousarray(data)), disp.shape[0], disp.shape[1], _p(disp))
        return disp


def pair(rows, cols, cn, seed):
    """a left image of smooth random texture and the right image it gives under a disparity of 1..4 px that varies by region, plus noise"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (rows, cols + 8, cn)).astype(np.float64)
    base = (base + np.roll(base, 1, 1) + np.roll(base, 1, 0)) / 3.0
    left = base[:, 4:4 + cols]
    d = 1 + (np.arange(rows)[:, None] // 5 + np.arange(cols)[None, :] // 7) % 4
    xs = np.arange(cols)[None, :] + d + 4
    right = base[np.arange(rows)[:, None], xs] + rng.normal(0, 2.0, (rows, cols, cn))
    to8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    left, right = to8(left), to8(right)
    return (left[..., 0], right[..., 0]) if cn == 1 else (left, right)


def volume(msg, ndisp, rows, cols, seed):
    rng = np.random.default_rng(seed)
    if msg == "f32":
        return rng.uniform(0, 20, (ndisp * rows, cols)).astype(np.float32)
    v = rng.integers(0, 300, (ndisp * rows, cols)).astype(np.int16)
    edge = rng.random(v.shape)
    v[edge < 0.08] = 32760    # near the range limit: the saturating stores and the truncating subtraction show
    v[edge > 0.94] = -32760
    return v


# name, rows, cols, channels (0: compute(data)), ndisp, iters, levels, msg, weights
CLASS_CASES = [
    ("f32_c1_l3", 21, 27, 1, 12, 3, 3, "f32", {}),
    ("s16_c3_l2", 15, 19, 3, 10, 3, 2, "s16", {}),
    ("f32_c4_l1", 9, 13, 4, 9, 4, 1, "f32", {}),
    ("s16_c1_l4", 33, 41, 1, 8, 2, 4, "s16", {}),
    ("f32_c3_w", 17, 23, 3, 20, 3, 2, "f32", OTHER_W),
    ("s16_c4_w", 25, 29, 4, 7, 5, 3, "s16", OTHER_W),
    ("data_f32", 11, 15, 0, 8, 3, 2, "f32", {}),
    ("data_s16", 13, 11, 0, 6, 3, 2, "s16", {}),
]
STAGE_CASES = [("f32_c1", 9, 11, 1, 8, "f32", {}), ("s16_c3", 9, 11, 3, 8, "s16", OTHER_W), ("f32_c4", 7, 12, 4, 5, "f32", OTHER_W),
               ("s16_c1", 10, 9, 1, 16, "s16", {})]


def run_class_case(ref, case):
    name, rows, cols, cn, ndisp, iters, levels, msg, w = case
    params = np.array(json.dumps(dict(ndisp=ndisp, iters=iters, levels=levels, msg=msg, weights=dict(DEFAULT_W, **w))))
    seed = sum(map(ord, name))
    if cn == 0:
        data = volume(msg, ndisp, rows, cols, seed)
        return dict(data=data, params=params, disp=ref.compute_data(data, ndisp, iters, levels, MSG[msg], w))
    left, right = pair(rows, cols, cn, seed)
    return dict(left=left, right=right, params=params, disp=ref.compute(left, right, ndisp, iters, levels, MSG[msg], w))


def run_stage_case(ref, case):
    name, rows, cols, cn, ndisp, msg, w = case
    seed = sum(map(ord, name))
    rng = np.random.default_rng(seed)
    left, right = pair(rows, cols, cn, seed)
    T = np.float32 if msg == "f32" else np.int16
    lo, hi = (-3.0, 9.0) if msg == "f32" else (-40, 90)
    ch, cw = (rows + 1) // 2, (cols + 1) // 2
    coarse = rng.uniform(lo, hi, (4, ndisp * ch, cw)).astype(T)
    ref.load_constants(ndisp, MSG[msg], w)
    data = ref.comp_data(left, right, ndisp, MSG[msg])
    up = ref.level_up(coarse, ndisp, rows, cols)
    iter2 = ref.iterations(up, data, ndisp, 2)
    return dict(left=left, right=right, params=np.array(json.dumps(dict(ndisp=ndisp, msg=msg, weights=dict(DEFAULT_W, **w)))),
                data=data, data_down=ref.step_down(data, ndisp), coarse=coarse, up=up, iter1=ref.iterations(up, data, ndisp, 1),
                iter2=iter2, disp=ref.output(iter2, data, ndisp))


def main():
    if not have_reference():
        sys.exit("the reference tree is not at " + REF)
    with tempfile.TemporaryDirectory(prefix="sbp_ref_") as tmp:
        ref = Ref(build(tmp))
        for kind, cases, run in (("refclass", CLASS_CASES, run_class_case), ("refstage", STAGE_CASES, run_stage_case)):
            for case in cases:
                rec = run(ref, case)
                assert rec["disp"] is not None, case
                path = os.path.join(GOLDEN, f"stereobp_{kind}_{case[0]}.npz")
                np.savez_compressed(path, **rec)
                print(path, os.path.getsize(path), "bytes; distinct disparities", len(np.unique(rec["disp"])))
                assert os.path.getsize(path) < 176 * 1024


if __name__ == "__main__":
    main()
