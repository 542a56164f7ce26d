"""Writes tests/golden/gftt_ref*.npz: what the REFERENCE's own code computed for cv::cuda::CornernessCriteria and CornersDetector.

Built from the reference tree into a temporary directory outside the repository, with the flags of tools/make_golden_orb.py
(tools/gftt_ref/ holds the C entry points and the stand-ins the stubs lack):
  kernels, rewritten only at their launch sites by oracle/refshim/cu2host.py and run on the host through oracle/refshim/cudashim and
  cudavec, which are used as they are:
    cudaimgproc/src/cuda/corners.cu and gftt.cu (whole files), cudafilters/src/cuda/row_filter.8uc1.cu, row_filter.32fc1.cu and
    column_filter.32fc1.cu with row_filter.hpp / column_filter.hpp.  The texture stand-in is oracle/refshim/cudashim's; thrust::sort with
    an execution policy, the allocator, the mask functors, atomicAdd and the border names are tools/gftt_ref/cu/.
  host code as SLICES of its text (cu2host.py --slice), #included by tools/gftt_ref/gftt_ref_stage.cpp:
    corners.cpp:93-101 (the scale), gftt.cpp:122-124 (the capacity, the threshold and the call of findCorners_gpu) and gftt.cpp:147-207
    (the grid loop of minDistance).
corners.cpp and gftt.cpp as wholes are NOT compiled: they need cuda::createSobelFilter / createScharrFilter (filtering.cpp, which needs
NPP and getDerivKernels), cuda::minMax (a cudaarithm kernel), GpuMat::colRange / copyTo / download / upload, ensureSizeIsEnough and
Stream::waitForCompletion of a core that oracle/refshim/cudahost does not have, and nothing under oracle/ is edited.  So the class
fixtures come from the reference's kernels and slices run in the reference's order by the glue; written by the glue and not by the
reference are: the maximum of the plane (a plain loop for cuda::minMax), the branch on minDistance < 1 with the copy of the head
(gftt.cpp:134-137), cvRound (lrint), and the taps: [-1 0 1] and [1 2 1] * scale with the product in double (getDerivKernels and
Mat *= double are main-repository code; for ksize 3 every reading gives these bits).

    python tools/make_golden_gftt.py            # needs the reference tree (REF, default /root/reference)

  gftt_refstage_<type>_<border>   images of 13 x 31, 5 x 31 (blockSize 7 above the side) and 3 x 3, the taps, and per blockSize in
                                  {2, 3, 5, 7}: Dx, Dy and both criteria's planes, for one border mode.
  gftt_refclass_<case>            image, mask, parameters (inputs); the response plane, threshold, capacity, findCorners' set (sorted
                                  row-major: the reference's order is the order its blocks ran in), the sorted list and the class output.
The smallest image: 3 x 3 is the first size tried and it is defined.  Every index the filter kernels form goes through % length
(border_interpolate.hpp), so no size reads outside its source; recorded here by running each stage image a second time as a view
inside a frame of NaN (float) or 255 (bytes) with a larger step and asserting the same bits.

Asserted on the reference's outputs while recording: every strict case has at least 32 corners and no two equal responses among its
candidates, so the order is unique; no strict case reaches capacity; `blocks_ties` has a run of at least 8 equal responses (it is
compared as a set); `flat` is empty.  A re-run gives the same bytes (save_npz of tools/make_golden_stereocsbp.py).
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gftt_numpy_ref as R  # noqa: E402
from make_golden_stereocsbp import save_npz  # noqa: E402  (fixed time stamps: the same arrays give the same bytes)

REF = os.environ.get("REF", "/root/reference")
SHIM = os.path.join(ROOT, "oracle", "refshim")
HERE = os.path.join(ROOT, "tools", "gftt_ref")
GOLDEN = os.environ.get("GFTT_GOLDEN_DIR", os.path.join(ROOT, "tests", "golden"))   # the tests re-record into a temporary directory
F = np.float32
BORDER_NAMES = {R.BORDER_REFLECT101: "reflect101", R.BORDER_REFLECT: "reflect", R.BORDER_REPLICATE: "replicate"}


def have_reference():
    return os.path.exists(os.path.join(REF, "modules", "cudaimgproc", "src", "cuda", "gftt.cu"))


def build(outdir):
    """Compiles the reference's kernels and the slices for the host into `outdir` (outside the repository) -> the library's path."""
    out = lambda n: os.path.join(outdir, n)
    mod = lambda *a: os.path.join(REF, "modules", *a)
    c2h = [sys.executable, os.path.join(SHIM, "cu2host.py")]
    common = ["-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-w"]
    cu = common + ["-D__CUDA_ARCH__=700", "-I" + outdir, "-I" + os.path.join(HERE, "cu"), "-I" + os.path.join(SHIM, "cudavec"),
                   "-I" + os.path.join(SHIM, "cudashim"), "-include", os.path.join(SHIM, "cudashim", "cudashim.h")]
    flt = mod("cudafilters", "src", "cuda")
    img = mod("cudaimgproc", "src")
    units = ["corners", "gftt", "row_filter.8uc1", "row_filter.32fc1", "column_filter.32fc1"]
    steps = [
        c2h + [os.path.join(img, "corners.cpp"), out("corners_scale.gen.inc"), "--slice", "double scale = static_cast<double>(1 <<", "if (ksize_ > 0)"],
        c2h + [os.path.join(img, "gftt.cpp"), out("gftt_capacity.gen.inc"), "--slice", "ensureSizeIsEnough(1, std::max(1000", "if (total == 0)"],
        c2h + [os.path.join(img, "gftt.cpp"), out("gftt_grid.gen.inc"), "--slice", "const int cell_size = cvRound(minDistance_);",
               "_corners.create(1, static_cast<int>(tmp2.size())"],
        c2h + [os.path.join(flt, "row_filter.hpp"), out("row_filter.hpp")],
        c2h + [os.path.join(flt, "column_filter.hpp"), out("column_filter.hpp")],
        c2h + [os.path.join(img, "cuda", "corners.cu"), out("corners.gen.cpp")],
        c2h + [os.path.join(img, "cuda", "gftt.cu"), out("gftt.gen.cpp")],
    ]
    steps += [c2h + [os.path.join(flt, n + ".cu"), out(n + ".gen.cpp")] for n in units[2:]]
    steps += [["g++"] + cu + ["-c", out(n + ".gen.cpp"), "-o", out(n + ".gen.o")] for n in units]
    steps += [
        ["g++"] + cu + ["-c", os.path.join(HERE, "gftt_ref_stage.cpp"), "-o", out("gftt_ref_stage.o")],
        ["g++"] + cu + ["-c", os.path.join(SHIM, "cudashim", "cudashim.cpp"), "-o", out("cudashim.o")],
        ["gcc", "-O2", "-fPIC", "-fopenmp", "-ffp-contract=off", "-c", os.path.join(SHIM, "oclrt.c"), "-o", out("oclrt.o")],
        ["g++", "-shared", "-fopenmp", "-o", out("libgftt_ref.so")] + [out(n + ".gen.o") for n in units] +
        [out("gftt_ref_stage.o"), out("cudashim.o"), out("oclrt.o"), "-lm", "-Wl,--no-undefined"],
    ]
    for cmd in steps:
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(" ".join(cmd) + "\n" + r.stdout + r.stderr)
    return out("libgftt_ref.so")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Ref:
    """ctypes binding of the library build() makes"""

    def __init__(self, path):
        self.L = C.CDLL(path)
        self.L.gftt_ref_scale.restype = C.c_double

    def taps(self, dtype, block_size):
        """the scale is the reference's (corners.cpp:93-101); the product with [1 2 1] in double is the glue's"""
        scale = self.L.gftt_ref_scale(3, block_size, int(np.dtype(dtype) == np.uint8))
        return np.array([-1, 0, 1], F), (np.array([1.0, 2.0, 1.0]) * scale).astype(F)

    def sobel(self, img, deriv, smooth, border, framed=False):
        """createSobelFilter(1, 0) and (0, 1): -> Dx, Dy.  framed: the image is a view inside a larger array of NaN / 255"""
        rows, cols = img.shape
        src, view = np.ascontiguousarray(img), None
        if framed:
            src = np.full((rows + 6, cols + 11), np.nan if img.dtype == F else 255, img.dtype)
            src[3:3 + rows, 4:4 + cols] = img
            view = src[3:3 + rows, 4:4 + cols]
        ptr = C.c_void_p((view if framed else src).ctypes.data)
        out = []
        for rk, ck in ((deriv, smooth), (smooth, deriv)):
            buf, dst = np.zeros((rows, cols), F), np.zeros((rows, cols), F)
            self.L.gftt_ref_sobel(ptr, C.c_size_t(src.strides[0]), rows, cols, int(img.dtype == F), _p(np.ascontiguousarray(rk, F)),
                                  _p(np.ascontiguousarray(ck, F)), border, _p(buf), _p(dst))
            out.append(dst)
        return out

    def corner(self, dx, dy, block_size, border, harris, k):
        dst = np.zeros(dx.shape, F)
        self.L.gftt_ref_corner(_p(dx), _p(dy), dx.shape[0], dx.shape[1], block_size, border, int(harris), C.c_float(k), _p(dst))
        return dst

    def detect_tail(self, resp, mask, quality, min_dist, max_corners):
        rows, cols = resp.shape
        cap = R.capacity(rows, cols)
        cand, srt, out = (np.zeros((cap, 2), F) for _ in range(3))
        thr, capacity, total = C.c_float(), C.c_int(), C.c_int()
        m = None if mask is None else np.ascontiguousarray(mask)
        n = self.L.gftt_ref_detect_tail(_p(resp), rows, cols, _p(m), C.c_double(quality), C.c_double(min_dist), max_corners, C.byref(thr),
                                        C.byref(capacity), _p(cand), C.byref(total), _p(srt), _p(out))
        assert capacity.value == cap, (capacity.value, cap)
        t = total.value
        return dict(threshold=np.array(thr.value, F), capacity=np.array(cap), total=np.array(t), candidates=cand[:t].copy(),
                    sorted=srt[:t].copy(), corners=out[:n].copy())


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def run_stage(ref, dtype, border):
    rec = {"border": np.array(border)}
    for rows, cols in ((13, 31), (5, 31), (3, 3)):
        img = R.synth_image(rows, cols, rows * 1000 + cols, "noise", dtype)
        tag = f"{rows}x{cols}"
        rec[f"img_{tag}"] = img
        for bs in (2, 3, 5, 7):
            d, s = ref.taps(dtype, bs)
            dx, dy = ref.sobel(img, d, s, border)
            fx, fy = ref.sobel(img, d, s, border, framed=True)
            assert bits_equal(dx, fx) and bits_equal(dy, fy), ("a filter kernel read outside its source", tag, bs)
            rec.update({f"deriv_bs{bs}": d, f"smooth_bs{bs}": s, f"dx_{tag}_bs{bs}": dx, f"dy_{tag}_bs{bs}": dy,
                        f"mineig_{tag}_bs{bs}": ref.corner(dx, dy, bs, border, False, 0.0),
                        f"harris_{tag}_bs{bs}": ref.corner(dx, dy, bs, border, True, 0.04)})
    rec["harris_k"] = np.array(0.04, F)
    return rec


# name: (kind, rows, cols, dtype, masked, block_size, harris, k, quality, min_distance, max_corners)
CLASS_CASES = {
    "flat": ("flat", 23, 71, np.uint8, False, 3, False, 0.04, 0.01, 0.0, 1000),
    "blocks_ties": ("blocks", 40, 140, np.uint8, False, 3, False, 0.04, 0.01, 0.0, 0),
    "noise23x71_u8": ("noise", 23, 71, np.uint8, False, 3, False, 0.04, 0.01, 0.0, 1000),
    "noise23x71_f32": ("noise", 23, 71, np.float32, False, 3, False, 0.04, 0.01, 0.0, 1000),
    "noise40x140_u8": ("noise", 40, 140, np.uint8, False, 3, False, 0.04, 0.01, 0.0, 1000),
    "noise40x140_f32": ("noise", 40, 140, np.float32, False, 3, False, 0.04, 0.01, 3.0, 0),
    "masked": ("noise", 40, 140, np.uint8, True, 3, False, 0.04, 0.01, 0.0, 1000),
    "harris": ("noise", 40, 140, np.uint8, False, 3, True, 0.04, 0.01, 0.0, 1000),
    "harris_f32_bs5": ("noise", 40, 140, np.float32, False, 5, True, 0.06, 0.01, 7.5, 1000),
    "bs2": ("noise", 40, 140, np.uint8, False, 2, False, 0.04, 0.01, 0.0, 10),
    "bs5_md3": ("noise", 40, 140, np.uint8, True, 5, False, 0.04, 0.01, 3.0, 1000),
    "bs7": ("noise", 40, 140, np.uint8, False, 7, False, 0.04, 0.001, 0.0, 0),
    "bs7_above_the_side": ("noise", 5, 140, np.uint8, False, 7, False, 0.04, 0.001, 0.0, 0),
    "md3_max10": ("noise", 40, 140, np.uint8, False, 3, False, 0.04, 0.01, 3.0, 10),
    "md7.5": ("noise", 40, 140, np.uint8, False, 3, False, 0.04, 0.01, 7.5, 0),
}
LOOSE = ("flat", "blocks_ties", "bs7_above_the_side")   # not strict: empty, ties on purpose, three interior rows


def run_class(ref, name):
    kind, rows, cols, dtype, masked, bs, harris, k, q, md, maxc = CLASS_CASES[name]
    img = R.synth_image(rows, cols, rows * 1000 + cols, kind, dtype)
    mask = R.synth_mask(rows, cols, 3) if masked else None
    d, s = ref.taps(dtype, bs)
    dx, dy = ref.sobel(img, d, s, R.BORDER_REFLECT101)
    resp = ref.corner(dx, dy, bs, R.BORDER_REFLECT101, harris, k)
    rec = ref.detect_tail(resp, mask, q, md, maxc)
    cand = rec["candidates"]
    rec["candidates"] = cand[np.lexsort((cand[:, 0], cand[:, 1]))]   # as a set: row-major
    r = resp[cand[:, 1].astype(int), cand[:, 0].astype(int)]
    total = int(rec["total"])
    if name == "flat":
        assert total == 0 and len(rec["corners"]) == 0
    elif name == "blocks_ties":
        runs = np.diff(np.flatnonzero(np.concatenate([[True], np.sort(r)[1:] != np.sort(r)[:-1], [True]])))
        assert runs.max() >= 8 and md == 0 and maxc == 0, runs.max()
    elif name not in LOOSE:
        assert total >= 32 and len(np.unique(r)) == total, (name, total, len(np.unique(r)))
    assert total < int(rec["capacity"]), name
    print(f"{name}: {total} candidates (capacity {int(rec['capacity'])}), {len(rec['corners'])} corners, threshold {float(rec['threshold']):.6g}")
    rec.update(img=img, deriv=d, smooth=s, response=resp,
               params=np.array([bs, int(harris), maxc], np.int32), fparams=np.array([k, q, md], np.float64))
    if mask is not None:
        rec["mask"] = mask
    return rec


def main():
    if not have_reference():
        sys.exit("the reference tree is not at " + REF)
    with tempfile.TemporaryDirectory(prefix="gftt_ref_") as tmp:
        ref = Ref(build(tmp))
        recs = {}
        for dtype, tname in ((np.uint8, "u8"), (np.float32, "f32")):
            for border in R.BORDERS:
                recs[f"refstage_{tname}_{BORDER_NAMES[border]}"] = run_stage(ref, dtype, border)
        for name in CLASS_CASES:
            recs[f"refclass_{name}"] = run_class(ref, name)
        for name in sorted(recs):
            path = os.path.join(GOLDEN, f"gftt_{name}.npz")
            save_npz(path, recs[name])
            print(path, os.path.getsize(path), "bytes")
            assert os.path.getsize(path) < 96 * 1024


if __name__ == "__main__":
    main()
