"""Writes tests/golden/sgm_refstage_*.npz and sgm_refclass_*.npz: what the REFERENCE's own StereoSGM computed.

The reference's kernels (modules/cudastereo/src/cuda/stereosgm.cu, rewritten only at their launch sites by oracle/refshim/cu2host.py and
run on the host through oracle/refshim/cudashim, whose warp shuffles are collectives over the lanes of a 32-lane warp) and its host class
(modules/cudastereo/src/stereosgm.cpp, compiled as it lies against the stub core of oracle/refshim/cudahost, rows pitched to 512 bytes as
a device allocation's are) are built from the reference tree into a temporary directory; tools/sgm_ref/ holds the C entry points and the
headers the stubs lack.  The three CPU twins of the reference's own tests (test/test_sgm_funcs.cpp) are cut out of the reference tree into
the same library, and the kernels are held to them with zero difference before anything is recorded.  Only recorded inputs, parameters
and outputs are kept.

    python tools/make_golden_sgm.py            # needs the reference tree (REF, default /root/reference)

Everything is run twice, every stub allocation filled with 0x00 and then with 0xFF: where the two results differ the reference never
wrote (or computed from what it never wrote).  Those pixels are the fixture's `undef` masks; the values stored are those of the 0x00 run.

  refstage: inputs and outputs of every kernel wrapper on its own.  Cost volumes of the path kernels are stored whole for the smallest
            cases and otherwise as per-row check sums (path_checksum) with the SHA-256 of the volume, which is exact and stays small.
  refclass: inputs, parameters, the disparity of the class, the four maps around the median (left / right, before / after), the
            source pitch the median chose its kernel by and the kernel's name.
tests/test_sgm_ref.py holds oracle/sgm_ref.c to these files everywhere and rebuilds them where the reference tree is present;
tests/test_sgm.py holds the HIP kernels and the HIP class to them.
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opencv_contrib_amd import synth  # noqa: E402  (the stereo pairs tests/test_sgm.py uses; class fixtures store them whole)

REF = os.environ.get("REF", "/root/reference")
SHIM = os.path.join(ROOT, "oracle", "refshim")
HERE = os.path.join(ROOT, "tools", "sgm_ref")
GOLDEN = os.path.join(ROOT, "tests", "golden")
MODE_HH, MODE_HH4 = 1, 3
# PathAggregation::operator() fills its buffers in this order; (dx, dy) as the reference's tests name the directions
DIRS = [(0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, 1), (-1, -1), (1, -1)]
MAX_FILE = 176108   # the largest fixture before these


def have_reference():
    return os.path.exists(os.path.join(REF, "modules", "cudastereo", "src", "cuda", "stereosgm.cu"))


def build(outdir):
    """Compiles the reference's stereosgm.cu, stereosgm.cpp and the CPU twins of its tests for the host into `outdir` (outside the
    repository) -> the library's path."""
    out = lambda n: os.path.join(outdir, n)
    cs = os.path.join(REF, "modules", "cudastereo")
    common = ["-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-strict-aliasing", "-fno-gnu-unique", "-w",
              "-DCUDAHOST_PITCH_ALIGN=512", "-DCUDASHIM_COUNTED_BARRIERS", "-I" + os.path.join(HERE, "cu"), "-I" + os.path.join(SHIM, "cudahost"),
              "-I" + os.path.join(SHIM, "cudashim"), "-I" + os.path.join(cs, "include"), "-I" + os.path.join(cs, "src")]
    cu = common + ["-D__CUDA_ARCH__=700", "-include", os.path.join(SHIM, "cudashim", "cudashim.h"), "-I" + os.path.join(cs, "src", "cuda")]
    steps = [
        [sys.executable, os.path.join(SHIM, "cu2host.py"), os.path.join(cs, "src", "cuda", "stereosgm.cu"), out("stereosgm.gen.cpp")],
        [sys.executable, os.path.join(SHIM, "cu2host.py"), os.path.join(cs, "test", "test_sgm_funcs.cpp"), out("twins.gen.inc"), "--extract",
         "fn:census_transform,fn:path_aggregation,fn:winner_takes_all_left"],
        ["g++"] + cu + ["-c", out("stereosgm.gen.cpp"), "-o", out("stereosgm.gen.o")],
        ["g++"] + cu + ["-c", os.path.join(HERE, "sgm_ref_stage.cpp"), "-o", out("sgm_ref_stage.o")],
        ["g++"] + cu + ["-c", os.path.join(SHIM, "cudashim", "cudashim.cpp"), "-o", out("cudashim.o")],
        # the class as it lies; its calls of medianFilter and censusTransform are led through tools/sgm_ref/sgm_ref_class.cpp (see there)
        ["g++"] + common + ["-Dmedian_filter=median_filter_seen", "-Dcensus_transform=census_transform_seen", "-c",
                            os.path.join(cs, "src", "stereosgm.cpp"), "-o", out("stereosgm_host.o")],
        ["g++"] + common + ["-c", os.path.join(HERE, "sgm_ref_class.cpp"), "-o", out("sgm_ref_class.o")],
        ["g++", "-std=c++17", "-O2", "-fPIC", "-w", "-DSGM_REF_TWINS_INC=\"" + out("twins.gen.inc") + "\"", "-c",
         os.path.join(HERE, "sgm_ref_twins.cpp"), "-o", out("sgm_ref_twins.o")],
        ["gcc", "-O2", "-fPIC", "-fopenmp", "-ffp-contract=off", "-c", os.path.join(SHIM, "oclrt.c"), "-o", out("oclrt.o")],
        ["g++", "-shared", "-fopenmp", "-o", out("libsgm_ref.so"), out("stereosgm.gen.o"), out("sgm_ref_stage.o"), out("cudashim.o"),
         out("stereosgm_host.o"), out("sgm_ref_class.o"), out("sgm_ref_twins.o"), out("oclrt.o"), "-lm", "-Wl,--no-undefined"],
    ]
    for cmd in steps:
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(" ".join(cmd) + "\n" + r.stdout + r.stderr)
    return out("libsgm_ref.so")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _c(a, dtype=None):
    return np.ascontiguousarray(a, dtype)


class Threw(Exception):
    """the reference rejected its arguments"""


class Ref:
    """ctypes binding of the library build() makes.  Every method runs the reference once with the current fill byte."""

    def __init__(self, path):
        self.L = C.CDLL(path)

    def fill(self, byte):
        self.L.sgm_ref_set_fill(int(byte))

    def zero_census_border(self, on):
        self.L.sgm_ref_zero_census_border(int(on))

    @staticmethod
    def _ok(rc):
        if rc == 1:
            raise Threw()
        assert rc == 0, rc

    def census(self, img):
        out = np.empty(img.shape, np.int32)
        self._ok(self.L.sgm_ref_census(_p(_c(img)), img.shape[0], img.shape[1], int(img.dtype == np.uint16), _p(out)))
        return out

    def path(self, left, right, ndisp, direction, p1, p2, min_disp):
        """direction: index into DIRS -> (rows * cols * ndisp,) uint8"""
        h, w = left.shape
        out = np.empty(h * w * ndisp, np.uint8)
        self._ok(self.L.sgm_ref_path(_p(_c(left, np.int32)), _p(_c(right, np.int32)), h, w, ndisp, direction, p1, p2, min_disp, _p(out)))
        return out

    def wta(self, cost, h, w, ndisp, paths, uniqueness, subpixel):
        left, right = np.empty((h, w), np.uint16), np.empty((h, w), np.uint16)
        mode = {4: MODE_HH4, 8: MODE_HH}[paths]
        self._ok(self.L.sgm_ref_wta(_p(_c(cost, np.uint8)), h, w, ndisp, mode, C.c_float(uniqueness), int(subpixel), _p(left), _p(right)))
        return left, right

    def median(self, src):
        """-> (filtered, the source's pitch in bytes)"""
        out, pitch = np.empty(src.shape, np.uint16), C.c_int()
        self._ok(self.L.sgm_ref_median(_p(_c(src, np.uint16)), src.shape[0], src.shape[1], _p(out), C.byref(pitch)))
        return out, pitch.value

    def check(self, left_disp, right_disp, src_left, subpixel=True):
        out = _c(left_disp, np.uint16).copy()
        self._ok(self.L.sgm_ref_check(_p(out), _p(_c(right_disp, np.uint16)), _p(_c(src_left)), int(src_left.dtype == np.uint16), out.shape[0],
                                      out.shape[1], int(subpixel)))
        return out

    def range(self, disp, subpixel, min_disp):
        out = _c(disp, np.uint16).copy()
        self._ok(self.L.sgm_ref_range(_p(out), out.shape[0], out.shape[1], int(subpixel), min_disp))
        return out

    def compute(self, left, right, min_disp=0, ndisp=128, p1=10, p2=120, uniq=5, mode=MODE_HH4):
        """-> (disparity int16, maps (4, h, w) uint16: left before / after the median, right before / after, median source pitch)"""
        h, w = left.shape
        disp, maps, pitch = np.empty((h, w), np.int16), np.empty((4, h, w), np.uint16), C.c_int()
        ip = (C.c_int * 6)(min_disp, ndisp, p1, p2, uniq, mode)
        self._ok(self.L.sgm_ref_compute(_p(_c(left)), _p(_c(right)), h, w, right.shape[0], right.shape[1], int(left.dtype == np.uint16), ip,
                                        _p(disp), _p(maps), C.byref(pitch)))
        return disp, maps, pitch.value

    # the CPU twins of the reference's tests
    def twin_census(self, img):
        out = np.empty(img.shape, np.int32)
        self.L.sgm_twin_census(_p(_c(img, np.uint8)), img.shape[0], img.shape[1], _p(out))
        return out

    def twin_path(self, left, right, ndisp, min_disp, p1, p2, dx, dy):
        h, w = left.shape
        out = np.empty(h * w * ndisp, np.uint8)
        self.L.sgm_twin_path(_p(_c(left, np.int32)), _p(_c(right, np.int32)), h, w, ndisp, min_disp, p1, p2, dx, dy, _p(out))
        return out

    def twin_wta_left(self, cost, h, w, ndisp, paths, uniqueness, subpixel):
        out = np.empty((h, w), np.uint16)
        self.L.sgm_twin_wta_left(_p(_c(cost, np.uint8)), h, w, ndisp, paths, C.c_float(uniqueness), int(subpixel), _p(out))
        return out


def twice(ref, run):
    """run() with every allocation filled with 0x00 and then 0xFF -> (the 0x00 results, per result the mask of what differs)"""
    ref.fill(0x00)
    a = run()
    ref.fill(0xFF)
    b = run()
    ref.fill(0x00)
    a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
    return a, tuple(x != y for x, y in zip(a, b))


def noise(seed, shape, mod):
    """Integers in [0, mod): a counter through the splitmix64 finaliser.  Integer arithmetic only, the same on every machine: the
    inputs' generator, nothing of the algorithm."""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        z = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64((seed * 0xD1B54A32D192ED03) & (2 ** 64 - 1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(20)) % np.uint64(mod)).astype(np.int64).reshape(shape)


def census_pair(seed, shape):
    """two images of random 31-bit census values, as the reference's path tests draw them"""
    return noise(seed, shape, 2 ** 31 - 1).astype(np.int32), noise(seed + 1, shape, 2 ** 31 - 1).astype(np.int32)


def path_checksum(volume, h, w, ndisp):
    """(h,) uint32: per image row, the sum over its pixels and disparities k of (2k + 1) * cost[k]; says in which rows two volumes differ
    when their SHA-256 does"""
    v = volume.reshape(h, w, ndisp).astype(np.uint32)
    return (v * (2 * np.arange(ndisp, dtype=np.uint32) + 1)).sum(axis=(1, 2), dtype=np.uint32)


def sha(volume):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(volume).tobytes()).digest(), np.uint8)


# ------------------------------------------------------------------ the kernels against the reference's own CPU twins
TWIN_PATH_CASES = [(64, (21, 37), 0), (128, (19, 45), 1), (128, (9, 40), 10), (256, (7, 35), 2)]   # ndisp, shape, min_disp (>= 0: the twin's range)
TWIN_WTA_CASES = [(64, 9, 70), (128, 10, 141), (256, 5, 300)]                                       # ndisp, rows, cols


def check_against_twins(ref):
    """What the reference's own tests assert (EXPECT_MAT_NEAR(gold, dst, 0)), here of its kernels on the shim: census on random 8-bit
    images, every path direction on random census values (P1 10, P2 120 and 7 / 200), the left winner-takes-all map on costs 0 .. 31,
    4 and 8 paths, with and without sub-pixel.  -> the number of comparisons made"""
    n = 0
    for i, shape in enumerate([(128, 128), (113, 131), (8, 12), (6, 30), (7, 9)]):
        img = noise(900 + i, shape, 256).astype(np.uint8)
        np.testing.assert_array_equal(ref.census(img), ref.twin_census(img))
        n += 1
    for ndisp, shape, min_disp in TWIN_PATH_CASES:
        left, right = census_pair(ndisp + min_disp, shape)
        for d, (dx, dy) in enumerate(DIRS):
            for p1, p2 in ((10, 120), (7, 200)):
                np.testing.assert_array_equal(ref.path(left, right, ndisp, d, p1, p2, min_disp), ref.twin_path(left, right, ndisp, min_disp, p1, p2, dx, dy),
                                              err_msg=f"D={ndisp} {shape} direction {dx},{dy}")
                n += 1
    for ndisp, h, w in TWIN_WTA_CASES:
        for paths in (4, 8):
            cost = noise(ndisp + paths, (paths * h * w * ndisp,), 32).astype(np.uint8)
            for sub in (False, True):
                np.testing.assert_array_equal(ref.wta(cost, h, w, ndisp, paths, 0.95, sub)[0], ref.twin_wta_left(cost, h, w, ndisp, paths, 0.95, sub))
                n += 1
    return n


# ------------------------------------------------------------------ stage cases
CENSUS_SHAPES = [(7, 9), (6, 20), (9, 8), (8, 10), (17, 131), (35, 13)]   # one interior pixel; below the window (rows, then columns); 2 x 2
#                                                                          interior; two blocks across (120 columns each); three down (16 rows)


def run_stage_census(ref):
    rec = {}
    for dt, mod in ((np.uint8, 256), (np.uint16, 65536)):
        for i, shape in enumerate(CENSUS_SHAPES):
            src = noise(300 + i + mod, shape, mod).astype(dt)
            (out,), (undef,) = twice(ref, lambda: ref.census(src))
            key = f"{np.dtype(dt).name}_{shape[0]}x{shape[1]}"
            rec.update({key + "_src": src, key + "_out": out, key + "_undef": undef})
    return rec


# per number of disparities: (name, (rows, cols), min_disp, P2, whole volumes stored, left = right rolled by 7)
# Tiling of the reference's kernels: the horizontal ones take 16 / 8 / 4 rows a block and 4 / 2 / 1 a warp (D = 64 / 128 / 256), the
# vertical ones 64 / 32 / 16 columns a block and 8 / 4 / 2 a warp, the oblique ones the same number of diagonals.
PATH_CASES = {
    64: [("whole", (6, 20), 0, 120, True, False), ("whole_m1", (6, 20), -1, 120, True, False),
         ("t15x63", (15, 63), 0, 120, False, False), ("t16x64", (16, 64), 0, 120, False, False), ("t17x65", (17, 65), 0, 120, False, False),
         ("t3x7", (3, 7), 0, 120, False, False), ("t4x8", (4, 8), 0, 120, False, False), ("t5x9", (5, 9), 0, 120, False, False),
         ("md3", (9, 70), 3, 120, False, False), ("md_1", (9, 70), -1, 120, False, False), ("md_70", (9, 70), -70, 120, False, False),
         ("md_70w", (5, 90), -70, 120, False, False), ("wrap", (12, 40), 0, 250, False, True),
         ("l1x9", (1, 9), 1, 120, False, False), ("l9x1", (9, 1), 1, 120, False, False), ("l2x9", (2, 9), 1, 120, False, False),
         ("l9x2", (9, 2), 1, 120, False, False), ("l3x3", (3, 3), 1, 120, False, False), ("l1x1", (1, 1), 0, 120, False, False)],
    128: [("whole", (3, 10), 0, 120, True, False),
          ("t7x31", (7, 31), 0, 120, False, False), ("t8x32", (8, 32), 0, 120, False, False), ("t9x33", (9, 33), 0, 120, False, False),
          ("t1x3", (1, 3), 0, 120, False, False), ("t2x4", (2, 4), 0, 120, False, False), ("t3x5", (3, 5), 0, 120, False, False),
          ("md3", (5, 140), 3, 120, False, False), ("md_1", (5, 140), -1, 120, False, False), ("md_70", (5, 140), -70, 120, False, False),
          ("md_130", (5, 140), -130, 120, False, False), ("wrap", (8, 40), 0, 250, False, True),
          ("l1x9", (1, 9), 1, 120, False, False), ("l9x1", (9, 1), 1, 120, False, False), ("l3x3", (3, 3), 1, 120, False, False)],
    256: [("whole", (2, 6), 0, 120, True, False),
          ("t3x15", (3, 15), 0, 120, False, False), ("t4x16", (4, 16), 0, 120, False, False), ("t5x17", (5, 17), 0, 120, False, False),
          ("t1x1", (1, 1), 0, 120, False, False), ("t2x2", (2, 2), 0, 120, False, False), ("t2x3", (2, 3), 0, 120, False, False),
          ("md3", (3, 270), 3, 120, False, False), ("md_1", (3, 270), -1, 120, False, False), ("md_70", (3, 270), -70, 120, False, False),
          ("md_260", (3, 270), -260, 120, False, False), ("wrap", (6, 40), 0, 250, False, True),
          ("l1x9", (1, 9), 1, 120, False, False), ("l9x1", (9, 1), 1, 120, False, False)],
}
PATH_P1 = 10


def path_inputs(ndisp, case):
    name, shape, min_disp, p2, whole, rolled = case
    left, right = census_pair(ndisp * 1000 + sum(map(ord, name)), shape)
    if rolled:   # disparity 7 costs 0 all along a line while the others climb to the P2 cap: cap + popcount passes 255
        left = np.roll(right, 7, axis=1)
    return left, right


def run_stage_paths(ref, ndisp):
    rec = {}
    for case in PATH_CASES[ndisp]:
        name, (h, w), min_disp, p2, whole, rolled = case
        left, right = path_inputs(ndisp, case)
        rec[name + "_in_sha"] = sha(np.stack([left, right]))
        for q in range(8):
            (vol,), (undef,) = twice(ref, lambda: ref.path(left, right, ndisp, q, PATH_P1, p2, min_disp))
            assert not undef.any(), (ndisp, name, q)   # the path kernels write every cost
            rec[f"{name}_d{q}_sum"] = path_checksum(vol, h, w, ndisp)
            rec[f"{name}_d{q}_sha"] = sha(vol)
            if whole:
                rec[f"{name}_d{q}_vol"] = vol
        if rolled:   # the case must reach the cast: with P2 = 224 (224 + 31 = 255) nothing wraps
            assert (ref.path(left, right, ndisp, 2, PATH_P1, 250, 0) != ref.path(left, right, ndisp, 2, PATH_P1, 224, 0)).any()
    return rec


WTA_SHAPES = {64: (3, 70), 128: (2, 133), 256: (2, 261)}   # wider than D: right pixels whose candidates start beyond one window
WTA_VALUES = (2, 32, 256)                                   # {0, 1}: ties everywhere; the reference's tests' range; all of a byte
WTA_UNIQ = (0.0, 0.95, 1.0)


def wta_cost(ndisp, values, paths):
    h, w = WTA_SHAPES[ndisp]
    return noise(ndisp + values + paths, (paths * h * w * ndisp,), values).astype(np.uint8)


def run_stage_wta(ref):
    rec = {}
    for ndisp, (h, w) in WTA_SHAPES.items():
        for values in WTA_VALUES:
            for paths in (4, 8):
                cost = wta_cost(ndisp, values, paths)
                rec[f"D{ndisp}_v{values}_p{paths}_in_sha"] = sha(cost)
                for ui, uniq in enumerate(WTA_UNIQ):
                    for sub in (0, 1):
                        (left, right), (ul, ur) = twice(ref, lambda: ref.wta(cost, h, w, ndisp, paths, uniq, sub))
                        assert not ul.any() and not ur.any()   # both maps are written everywhere
                        key = f"D{ndisp}_v{values}_p{paths}_u{ui}_s{sub}"
                        rec[key + "_left"], rec[key + "_right"] = left, right
    return rec


MEDIAN_SHAPES = [(6, 4), (6, 5), (5, 15), (5, 16), (7, 17), (3, 40), (20, 33)]


def median_kernel_name(pitch):
    """median_filter<uint16_t> takes its two-pixel kernel when the pitch holds an even number of pixels (stereosgm.cu:1922)"""
    return "median_kernel_3x3_16u_v2" if (pitch // 2) % 2 == 0 else "median_kernel_3x3_16u"


def median_source(i, shape, big):
    src = noise(500 + i + big, shape, 0x1400 if big else 200).astype(np.uint16)
    if big:
        src[noise(600 + i, shape, 7) == 0] = 0xFFFF
    return src


def run_stage_median(ref):
    rec = {}
    for i, shape in enumerate(MEDIAN_SHAPES):
        for big in (0, 1):   # values below 256, and values above 255 with 0xFFFF among them
            src = median_source(i, shape, big)
            (out, pitch), (undef, _) = twice(ref, lambda: ref.median(src))
            key = f"{shape[0]}x{shape[1]}_{'big' if big else 'small'}"
            rec.update({key + "_src": src, key + "_out": out, key + "_undef": undef, key + "_pitch": np.array(pitch),
                        key + "_kernel": np.array(median_kernel_name(pitch))})
    return rec


CHECK_SHAPES = [(16, 16), (32, 48), (17, 33), (13, 15), (33, 50), (16, 15), (15, 16)]


def check_inputs(i, shape, dt):
    src = noise(700 + i, shape, 256 if dt == np.uint8 else 65536).astype(dt)
    src[noise(701 + i, shape, 9) == 0] = 0
    left = noise(702 + i, shape, 40 * 16).astype(np.uint16)
    left[noise(703 + i, shape, 11) == 0] = 0xFFFF
    right = noise(704 + i, shape, 40).astype(np.uint16)
    return left, right, src


def run_stage_check(ref):
    rec = {}
    for i, shape in enumerate(CHECK_SHAPES):
        for dt in (np.uint8, np.uint16):
            left, right, src = check_inputs(i, shape, dt)
            for sub in (0, 1):
                (out,), (undef,) = twice(ref, lambda: ref.check(left, right, src, sub))
                assert not undef.any()
                key = f"{shape[0]}x{shape[1]}_{np.dtype(dt).name}_s{sub}"
                rec.update({key + "_left": left, key + "_right": right, key + "_src": src, key + "_out": out})
    return rec


RANGE_MIN_DISP = (-8, 0, 3, 300)


def run_stage_range(ref):
    rec = {}
    disp = noise(800, (17, 19), 64 * 16).astype(np.uint16)
    disp[noise(801, disp.shape, 5) == 0] = 0xFFFF
    rec["disp"] = disp
    for md in RANGE_MIN_DISP:
        for sub in (0, 1):
            (out,), (undef,) = twice(ref, lambda: ref.range(disp, sub, md))
            assert not undef.any()
            rec[f"m{md}_s{sub}_out"] = out
    return rec


# ------------------------------------------------------------------ class cases
# name, (rows, cols), (seed, max_disp) of synth.stereo_pair, 16-bit input, keyword arguments of Ref.compute
def _small():
    out = []
    for shape in ((13, 15), (16, 16), (17, 33), (32, 48)):
        for mode in (MODE_HH, MODE_HH4):
            for uniq in (0, 100):
                out.append((f"{shape[0]}x{shape[1]}_m{mode}_u{uniq}", shape, (13, 10), False,
                            dict(min_disp=-8, ndisp=64, p1=10, p2=250, uniq=uniq, mode=mode)))
    return out


CLASS_CASES = _small() + [
    ("64x160_reuse", (64, 160), (12, 30), False, dict(min_disp=-8, ndisp=64, p1=10, p2=250, uniq=5, mode=MODE_HH)),
    ("13x15_reuse", (13, 15), (13, 10), False, dict(min_disp=-8, ndisp=64, p1=10, p2=250, uniq=5, mode=MODE_HH)),
    ("64x160_u16", (64, 160), (12, 30), True, dict(min_disp=0, ndisp=64, p1=10, p2=120, uniq=5, mode=MODE_HH4)),
    ("64x160_D128", (64, 160), (12, 30), False, dict(min_disp=3, ndisp=128, p1=10, p2=120, uniq=5, mode=MODE_HH4)),
    ("32x48_D128_hh", (32, 48), (13, 10), False, dict(min_disp=3, ndisp=128, p1=10, p2=120, uniq=5, mode=MODE_HH)),
    ("32x48_D256_u16", (32, 48), (13, 10), True, dict(min_disp=0, ndisp=256, p1=10, p2=120, uniq=100, mode=MODE_HH)),
    ("17x33_D256", (17, 33), (13, 10), False, dict(min_disp=3, ndisp=256, p1=10, p2=250, uniq=0, mode=MODE_HH4)),
]
REJECTED = [("mode", dict(mode=0), None), ("ndisp96", dict(ndisp=96), None), ("size", dict(), (32, 40))]   # name, arguments, right image's shape


def class_pair(shape, synth_args, is16):
    left, right, _ = synth.stereo_pair(shape[0], shape[1], seed=synth_args[0], max_disp=synth_args[1])
    return (left.astype(np.uint16) * 257, right.astype(np.uint16) * 257) if is16 else (left, right)


def run_class_case(ref, case):
    name, shape, synth_args, is16, kw = case
    left, right = class_pair(shape, synth_args, is16)
    ref.zero_census_border(1)
    (disp, maps, pitch), (undef, maps_undef, _) = twice(ref, lambda: ref.compute(left, right, **kw))
    # the same with the census border left as the allocation's fill (0x00 gives the run above again, so only 0xFF is run): what hangs on
    # memory the class never clears (see sgm_ref_class.cpp)
    ref.zero_census_border(0)
    ref.fill(0xFF)
    undef_census = ref.compute(left, right, **kw)[0] != disp
    ref.fill(0x00)
    ref.zero_census_border(1)
    return dict(left=left, right=right, params=np.array(json.dumps(kw)), disp=disp, undef=undef, maps=maps, maps_undef=maps_undef,
                pitch=np.array(pitch), median_kernel=np.array(median_kernel_name(pitch)), undef_census_border=undef_census)


def run_rejected(ref):
    rec = {}
    left, right = class_pair((32, 48), (13, 10), False)
    for name, kw, rshape in REJECTED:
        try:
            ref.compute(left, right if rshape is None else right[:rshape[0], :rshape[1]], **dict(dict(ndisp=64), **kw))
            threw = 0
        except Threw:
            threw = 1
        rec[name + "_threw"] = np.array(threw)
    rec["accepted_threw"] = np.array(0)
    ref.compute(left, right, ndisp=64)   # the same call with nothing wrong: does not throw
    return rec


def depends_on_unwritten(left_after_median, quirks=True):
    """The pixels of the class's result that are computed from memory the reference never writes: the one-pixel frame neither median
    writes, and the pixels whose left-right check reads the right map in that frame (rows 0 and h - 1 are frame themselves, so: in
    column 0 or w - 1), within the blocks the check covers.  left_after_median: the class's left map after the median (its own frame
    does not matter).  The `undef` mask of a class fixture, measured by running the class on allocations filled with 0x00 and with 0xFF,
    lies inside this set; it can be smaller, where both fills happen to decide a check the same way."""
    h, w = left_after_median.shape
    dep = np.ones((h, w), bool)
    dep[1:-1, 1:-1] = False
    k = np.arange(w)[None, :] - (left_after_median.astype(np.uint16).astype(np.int32) >> 4)
    reads = (k == 0) | (k == w - 1)
    if quirks:
        reads[h // 16 * 16:, :] = False
        reads[:, w // 16 * 16:] = False
    return dep | reads


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


def jobs(ref):
    """(fixture name, function that records it)"""
    out = [("refstage_census", lambda: run_stage_census(ref))]
    out += [(f"refstage_paths_D{d}", (lambda d=d: run_stage_paths(ref, d))) for d in PATH_CASES]
    out += [("refstage_wta", lambda: run_stage_wta(ref)), ("refstage_median", lambda: run_stage_median(ref)),
            ("refstage_check", lambda: run_stage_check(ref)), ("refstage_range", lambda: run_stage_range(ref))]
    out += [("refclass_" + case[0], (lambda c=case: run_class_case(ref, c))) for case in CLASS_CASES]
    out.append(("refclass_rejected", lambda: run_rejected(ref)))
    return out


def fixture_names():
    return [f"sgm_refstage_{n}" for n in ["census"] + [f"paths_D{d}" for d in PATH_CASES] + ["wta", "median", "check", "range"]] + \
           ["sgm_refclass_" + c[0] for c in CLASS_CASES] + ["sgm_refclass_rejected"]


def main():
    if not have_reference():
        sys.exit("the reference tree is not at " + REF)
    with tempfile.TemporaryDirectory(prefix="sgm_ref_") as tmp:
        ref = Ref(build(tmp))
        print("kernels on the shim against the reference's CPU twins:", check_against_twins(ref), "comparisons, zero difference")
        total = 0
        for name, run in jobs(ref):
            rec = run()
            path = os.path.join(GOLDEN, f"sgm_{name}.npz")
            save_npz(path, rec)
            size = os.path.getsize(path)
            total += size
            extra = f"; undefined {int(rec['undef'].sum())} of {rec['undef'].size} pixels, median {rec['median_kernel']}" if "undef" in rec else ""
            print(path, size, "bytes" + extra)
            assert size <= MAX_FILE
        print("all:", total, "bytes")
        assert total < 1000000


if __name__ == "__main__":
    main()
