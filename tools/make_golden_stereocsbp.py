"""Writes tests/golden/stereocsbp_refclass_*.npz and stereocsbp_refstage_*.npz: what the REFERENCE's own StereoConstantSpaceBP computed.

The reference's kernels (modules/cudastereo/src/cuda/stereocsbp.cu, rewritten only at their launch sites by oracle/refshim/cu2host.py and
run on the host through oracle/refshim/cudashim) and its host class (modules/cudastereo/src/stereocsbp.cpp, compiled as it lies against
the stub core of oracle/refshim/cudahost) are built from the reference tree into a temporary directory; tools/stereocsbp_ref/ holds the C
entry points and the pieces the stubs lack.  Only the recorded inputs, parameters and outputs are kept.

    python tools/make_golden_stereocsbp.py            # needs the reference tree (REF, default /root/reference)

  refclass: inputs (or, for large images, the arguments of stereocsbp_numpy_ref.synth_pair), parameters, the disparity of the class and
            getNumLevels() after compute.
  refstage: inputs and outputs of every kernel wrapper on its own: init_data_cost at every level (init), compute_data_cost with random
            parents and init_message (chain), calc_all_iterations and compute_disp (iter).
tests/test_stereocsbp_ref.py holds the NumPy restatement to these files everywhere and rebuilds them where the reference tree is present;
tests/test_stereocsbp_gpu.py holds the HIP class and its stage entries to them.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from stereocsbp_numpy_ref import synth_pair  # noqa: E402  (integer arithmetic only: the inputs' generator, nothing of the algorithm)

REF = os.environ.get("REF", "/root/reference")
SHIM = os.path.join(ROOT, "oracle", "refshim")
HERE = os.path.join(ROOT, "tools", "stereocsbp_ref")
GOLDEN = os.path.join(ROOT, "tests", "golden")
CV_16S, CV_32F = 3, 5
MSG = {"f32": CV_32F, "s16": CV_16S}
DEFAULTS = dict(ndisp=16, iters=3, levels=3, nr_plane=2, min_disp=0, local=True, max_data_term=30.0, data_weight=1.0, max_disc_term=160.0,
                disc_single_jump=10.0)
STORE_PIXELS_UP_TO = 8192   # larger inputs are recorded as synth_pair's arguments


def have_reference():
    return os.path.exists(os.path.join(REF, "modules", "cudastereo", "src", "cuda", "stereocsbp.cu"))


def build(outdir):
    """Compiles the reference's stereocsbp.cu and stereocsbp.cpp for the host into `outdir` (outside the repository) -> the library's path."""
    out = lambda n: os.path.join(outdir, n)
    cs = os.path.join(REF, "modules", "cudastereo")
    common = ["-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-w"]
    cu = common + ["-I" + os.path.join(HERE, "cu"), "-I" + os.path.join(SHIM, "cudashim"), "-I" + os.path.join(cs, "src"),
                   "-include", os.path.join(SHIM, "cudashim", "cudashim.h")]
    ch = common + ["-fno-gnu-unique", "-I" + HERE, "-I" + os.path.join(SHIM, "cudahost"), "-I" + os.path.join(SHIM, "cudashim"),
                   "-I" + os.path.join(cs, "include")]
    steps = [
        [sys.executable, os.path.join(SHIM, "cu2host.py"), os.path.join(cs, "src", "cuda", "stereocsbp.cu"), out("stereocsbp.gen.cpp")],
        ["g++"] + cu + ["-I" + os.path.join(cs, "src", "cuda"), "-c", out("stereocsbp.gen.cpp"), "-o", out("stereocsbp.gen.o")],
        ["g++"] + cu + ["-c", os.path.join(HERE, "csbp_ref_stage.cpp"), "-o", out("csbp_ref_stage.o")],
        ["g++"] + cu + ["-c", os.path.join(SHIM, "cudashim", "cudashim.cpp"), "-o", out("cudashim.o")],
        ["g++"] + ch + ["-c", os.path.join(cs, "src", "stereocsbp.cpp"), "-o", out("stereocsbp_host.o")],
        ["g++"] + ch + ["-c", os.path.join(HERE, "csbp_ref_class.cpp"), "-o", out("csbp_ref_class.o")],
        ["gcc", "-O2", "-fPIC", "-fopenmp", "-ffp-contract=off", "-c", os.path.join(SHIM, "oclrt.c"), "-o", out("oclrt.o")],
        ["g++", "-shared", "-fopenmp", "-o", out("libcsbp_ref.so"), out("stereocsbp.gen.o"), out("csbp_ref_stage.o"), out("cudashim.o"),
         out("stereocsbp_host.o"), out("csbp_ref_class.o"), out("oclrt.o"), "-lm", "-Wl,--no-undefined"],
    ]
    for cmd in steps:
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(" ".join(cmd) + "\n" + r.stdout + r.stderr)
    return out("libcsbp_ref.so")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _cn(img):
    return 1 if img.ndim == 2 else img.shape[2]


class Ref:
    """ctypes binding of the library build() makes.  Planar matrices are dense (planes * h, w) arrays."""

    def __init__(self, path):
        self.L = C.CDLL(path)

    def compute(self, left, right, msg_type, out_dtype=np.int16, **kw):
        """-> (the class's disparity, getNumLevels() afterwards), or (None, None) if it threw.  left / right may be shapes (tuples)."""
        p = dict(DEFAULTS, **kw)
        shape = lambda a: tuple(a) if isinstance(a, tuple) else (a.shape[0], a.shape[1], _cn(a))
        (rows, cols, cn), (rr, rc, rcn) = shape(left), shape(right)
        ptr = lambda a: None if isinstance(a, tuple) else _p(np.ascontiguousarray(a))
        ip = (C.c_int * 7)(p["ndisp"], p["iters"], p["levels"], p["nr_plane"], msg_type, p["min_disp"], int(p["local"]))
        w = (C.c_float * 4)(p["max_data_term"], p["data_weight"], p["max_disc_term"], p["disc_single_jump"])
        out_type = {np.uint8: 0, np.int16: 3, np.int32: 4, np.float32: 5}[out_dtype]
        disp = np.empty((rows, cols), out_dtype)
        lv = C.c_int(-1)
        rc_ = self.L.csbp_ref_compute(ptr(left), ptr(right), rows, cols, cn, rr, rc, rcn, ip, w, out_type, _p(disp), C.byref(lv))
        assert rc_ in (0, 1), rc_
        return (disp, lv.value) if rc_ == 0 else (None, None)

    def estimate(self, width, height):
        v = [C.c_int() for _ in range(4)]
        self.L.csbp_ref_estimate(width, height, *[C.byref(x) for x in v])
        return tuple(x.value for x in v)

    @staticmethod
    def _w(kw):
        p = dict(DEFAULTS, **kw)
        return (C.c_float * 2)(p["max_data_term"], p["data_weight"]), p["min_disp"]

    def init_data_cost(self, left, right, level, nr_plane, ndisp, msg_type, local=True, **kw):
        T = np.float32 if msg_type == CV_32F else np.int16
        h, w = left.shape[0] >> level, left.shape[1] >> level
        cost, disp = np.zeros((nr_plane * h, w), T), np.zeros((nr_plane * h, w), T)
        wt, md = self._w(kw)
        self.L.csbp_ref_init_data_cost(int(msg_type == CV_32F), _p(np.ascontiguousarray(left)), _p(np.ascontiguousarray(right)), left.shape[0],
                                       left.shape[1], _cn(left), level, nr_plane, ndisp, wt, md, int(local), _p(cost), _p(disp))
        return cost, disp

    def compute_data_cost(self, left, right, level, disp_parent, n2, **kw):
        h, w = left.shape[0] >> level, left.shape[1] >> level
        out = np.zeros((n2 * h, w), disp_parent.dtype)
        wt, md = self._w(kw)
        self.L.csbp_ref_compute_data_cost(int(out.dtype == np.float32), _p(np.ascontiguousarray(left)), _p(np.ascontiguousarray(right)), left.shape[0],
                                          left.shape[1], _cn(left), level, n2, wt, md, _p(np.ascontiguousarray(disp_parent)), _p(out))
        return out

    def init_message(self, cur, data_cost, n, n2):
        """cur: (5, n2 * h2, w2) -> ((5, n * h, w), data_cost_selected)"""
        h, w = data_cost.shape[0] // n2, data_cost.shape[1]
        new, sel = np.zeros((5, n * h, w), data_cost.dtype), np.zeros((n * h, w), data_cost.dtype)
        self.L.csbp_ref_init_message(int(sel.dtype == np.float32), _p(np.ascontiguousarray(cur)), _p(new), _p(np.ascontiguousarray(data_cost)), _p(sel), h, w, n, n2)
        return new, sel

    def iterations(self, msgs, sel_disp, sel_cost, n, iters, max_disc_term, disc_single_jump):
        out = np.ascontiguousarray(msgs).copy()
        self.L.csbp_ref_iterations(int(out.dtype == np.float32), _p(out), _p(np.ascontiguousarray(sel_disp)), _p(np.ascontiguousarray(sel_cost)),
                                   sel_cost.shape[0] // n, sel_cost.shape[1], n, iters, int(max_disc_term), C.c_float(disc_single_jump))
        return out

    def compute_disp(self, msgs, sel_disp, sel_cost, n):
        disp = np.zeros((sel_cost.shape[0] // n, sel_cost.shape[1]), np.int16)
        self.L.csbp_ref_compute_disp(int(sel_cost.dtype == np.float32), _p(np.ascontiguousarray(msgs)), _p(np.ascontiguousarray(sel_disp)),
                                     _p(np.ascontiguousarray(sel_cost)), disp.shape[0], disp.shape[1], n, _p(disp))
        return disp


# name, rows, cols, channels, parameters other than DEFAULTS; every case is recorded for both message types
CLASS_CASES = [
    ("default", 29, 37, 1, {}),
    ("c3", 29, 37, 3, {}),
    ("c4", 27, 35, 4, {}),
    ("global", 29, 37, 1, dict(local=False)),
    ("mindisp", 29, 37, 1, dict(min_disp=3)),
    ("clamp", 29, 37, 1, dict(ndisp=5, levels=4)),                      # levels 4 -> 2
    ("ndisp2", 21, 23, 1, dict(ndisp=2, levels=3)),                     # levels -> 1; the local form's loop never runs
    ("fill", 29, 37, 1, dict(ndisp=8, nr_plane=4, levels=3)),           # 16 planes of 8 disparities at level 2: the (max, 0) fill
    ("disc27", 29, 37, 1, dict(max_disc_term=2.7, disc_single_jump=0.9)),   # the int truncation of max_disc_term
    ("sat", 29, 37, 1, dict(data_weight=100.0)),                        # 16 px x 30 x 100 > 32767 at level 2
    ("deep", 130, 260, 1, dict(ndisp=256, levels=8, nr_plane=1, iters=2, data_weight=0.02)),   # winsz 64 and 128 in the whole
    # pipeline; the weight keeps the 128 x 128 window's cost inside 16 bits
]


def case_seed(name):
    return sum(map(ord, name))


def run_class_case(ref, case, msg):
    name, rows, cols, cn, kw = case
    left, right = synth_pair(rows, cols, cn, case_seed(name))
    disp, lv = ref.compute(left, right, MSG[msg], **kw)
    rec = dict(params=np.array(json.dumps(dict(DEFAULTS, **kw, msg=msg))), synth=np.array([rows, cols, cn, case_seed(name)]), disp=disp,
               levels_after=np.array(lv))
    if rows * cols * cn <= STORE_PIXELS_UP_TO:
        rec.update(left=left, right=right)
    return rec


INIT_NDISP = (5, 70)


def run_stage_init(ref, msg):
    """init_data_cost at every level 0-7 on the smallest image that gives a 3 x 3 level, c1 / c3 / c4, local and global; ndisp 5, and 70
    where winsz <= 32 (x0 + tid - d < 0 then occurs inside a window)"""
    rec = {}
    for level in range(8):
        side = 3 << level
        for cn in (1, 3, 4):
            left, right = synth_pair(side, side, cn, 100 + level * 5 + cn)
            for local in (True, False):
                for ndisp in INIT_NDISP:
                    if ndisp == 70 and level > 5:
                        continue
                    cost, disp = ref.init_data_cost(left, right, level, 4, ndisp, MSG[msg], local, min_disp=1 if cn == 3 else 0)
                    key = f"L{level}_c{cn}_{'local' if local else 'global'}_n{ndisp}"
                    rec[key + "_cost"], rec[key + "_disp"] = cost, disp
    return rec


def rand_msgs(rng, T, shape, lo=-40, hi=90):
    return rng.integers(lo, hi, shape).astype(T) if T == np.int16 else (rng.integers(lo * 4, hi * 4, shape) / 4.0).astype(T)


DATA_COST_CASES = [(0, 24, 32), (1, 24, 32), (2, 24, 32), (5, 128, 128), (6, 128, 128)]   # level, image rows, cols: even levels
INIT_MESSAGE_PLANES = (1, 2, 4, 16)
ITER_CASES = [(9, 11, 3), (9, 11, 4), (5, 7, 16), (8, 70, 2), (4, 5, 65)]   # h, w, nr_plane


def run_stage_chain(ref, msg, cn):
    T = np.float32 if msg == "f32" else np.int16
    rng = np.random.default_rng(case_seed(msg) + cn)
    rec = {}
    for level, rows, cols in DATA_COST_CASES:
        left, right = synth_pair(rows, cols, cn, 200 + level)
        h, w = rows >> level, cols >> level
        n2 = 6
        parent = rng.integers(0, max(4, cols // 2), (n2 * (h // 2), w // 2)).astype(T)   # below min_disp = 2 and beyond x included
        rec[f"dc{level}_parent"] = parent
        rec[f"dc{level}_out"] = ref.compute_data_cost(left, right, level, parent, n2, min_disp=2)
    for n in INIT_MESSAGE_PLANES:
        h, w, n2 = 6, 8, 2 * n
        cur = rand_msgs(rng, T, (5, n2 * (h // 2), w // 2), 0, 6)     # a small range: equal summed costs (ties) are frequent
        dc = rand_msgs(rng, T, (n2 * h, w), 0, 4)
        new, sel = ref.init_message(cur, dc, n, n2)
        rec.update({f"im{n}_cur": cur, f"im{n}_dc": dc, f"im{n}_new": new, f"im{n}_sel": sel})
    return rec


def run_stage_iter(ref, msg):
    T = np.float32 if msg == "f32" else np.int16
    rng = np.random.default_rng(case_seed(msg) + 77)
    rec = {}
    for h, w, n in ITER_CASES:
        msgs = rand_msgs(rng, T, (4, n * h, w))
        sel_disp = rng.integers(0, 40, (n * h, w)).astype(T)
        sel_cost = rand_msgs(rng, T, (n * h, w), 0, 200)
        if msg == "s16":
            msgs[rng.random(msgs.shape) < 0.03] = 32000   # sums of shorts that wrap
        key = f"it{h}x{w}_{n}"
        rec.update({key + "_msgs": msgs, key + "_disp": sel_disp, key + "_cost": sel_cost})
        for iters in ((1, 3) if n <= 4 else (3,)):
            rec[f"{key}_out{iters}"] = ref.iterations(msgs, sel_disp, sel_cost, n, iters, 25, 1.5)
        if (h, w, n) == (9, 11, 4):
            tie = sel_cost.copy()
            tie[:] = 7   # every candidate equal: the first one wins
            rec["cd_disp"] = ref.compute_disp(rec[key + "_out3"], sel_disp, sel_cost, n)
            rec["cd_tie_disp"] = ref.compute_disp(np.zeros_like(msgs), sel_disp, tie, n)
    return rec


def save_npz(path, rec):
    """np.savez_compressed with a fixed time stamp on every member: the same arrays give the same bytes"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(rec):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(rec[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    if not have_reference():
        sys.exit("the reference tree is not at " + REF)
    with tempfile.TemporaryDirectory(prefix="csbp_ref_") as tmp:
        ref = Ref(build(tmp))
        jobs = []
        for msg in ("f32", "s16"):
            jobs += [(f"refclass_{case[0]}_{msg}", (lambda c=case, m=msg: run_class_case(ref, c, m))) for case in CLASS_CASES]
            jobs.append((f"refstage_init_{msg}", (lambda m=msg: run_stage_init(ref, m))))
            jobs += [(f"refstage_chain_{msg}_c{cn}", (lambda m=msg, c=cn: run_stage_chain(ref, m, c))) for cn in (1, 3)]
            jobs.append((f"refstage_iter_{msg}", (lambda m=msg: run_stage_iter(ref, m))))
        for name, run in jobs:
            rec = run()
            assert all(v is not None for v in rec.values()), name
            path = os.path.join(GOLDEN, f"stereocsbp_{name}.npz")
            save_npz(path, rec)
            extra = f"; distinct disparities {len(np.unique(rec['disp']))}" if "disp" in rec else ""
            print(path, os.path.getsize(path), "bytes" + extra)
            assert os.path.getsize(path) < 176 * 1024


if __name__ == "__main__":
    main()
