"""Writes tests/golden/brox_ref*.npz: what the REFERENCE's own code computed for cv::cuda::BroxOpticalFlow.

Built from the reference tree into a temporary directory outside the repository, with the flags of tools/make_golden_gftt.py
(-O2 -ffp-contract=off -fno-fast-math):
  kernels AND host code, rewritten only at their launch sites by oracle/refshim/cu2host.py and run on the host through
  oracle/refshim/cudashim, which is used as it is:
    cudalegacy/src/cuda/NCVBroxOpticalFlow.cu, the whole file: NCVBroxOpticalFlow() compiles whole, so the class fixtures are what the
      reference's host function returned;
    cudalegacy/src/cuda/NPP_staging.cu as two slices (cu2host.py --slice, then the launch rewrite): the mirror filters with
      nppiStFilterRowBorder_32f_C1R / nppiStFilterColumnBorder_32f_C1R (:1433-1633) and processLine .. nppiStResize_32f_C1R
      (:2073-2282).  The rest of that file (integral images, compaction, frame interpolation) needs NCV's allocators and is not Brox's.
  the builder's own text, tools/brox_ref/cu/ (first on the include path, so it shadows two shim headers without editing oracle/):
    opencv2/cudev/ptr2d/texture.hpp  the two constructor forms Brox uses and the DEFINITIONS of its texture reads
                                     (tests/brox_numpy_ref.py states them);
    brox_ncv_standin.hpp             the NCV scalar types, size / rectangle, status codes, assertion macros, allocator, vector (host
                                     memory filled with NaN) and matrix, the runtime calls as memcpy / memset, and rsqrtf(x) = 1.0f / sqrtf(x);
    opencv2/core/cuda/utility.hpp    cv::cuda::device::swap.
  tools/brox_ref/brox_ref.cpp: the C entry points.  For the STAGE fixtures it runs SLICES of the host function's text (cu2host.py --slice,
  then the launch rewrite; generated, never committed): the supersample call (NCVBroxOpticalFlow.cu:763-764), the prolongation with its
  scaling (:952-955), the seven filter calls (:842-868), the grids (:889-893), the launches of the two prepare stages (:901-902, :906)
  and the solver loop (:912-924).  Written by the glue and not by the reference: the objects those slices name (planes with a ptr(),
  sizes, rectangles, strides, the five taps as data) and the closing brace of the solver loop.  The level sizes of a class fixture are
  read off the linearly filtered textures the host function makes (nine per level).

    python tools/make_golden_brox.py            # needs the reference tree (REF, default /root/reference)

  brox_refstage_filter      the seven derivative planes at 4 x 4, 5 x 37 and 13 x 16
  brox_refstage_resize      supersample 16 x 16 -> 13 x 13, 23 x 37 -> 19 x 30, 4 x 4 -> 4 x 4, 5 x 37 -> 4 x 30; bicubic prolongation with the
                            1 / scale_factor scaling 4 x 4 -> 5 x 5, 4 x 30 -> 5 x 37, 13 x 16 -> 16 x 20 (rows x cols)
  brox_refstage_prepare_*   u, v, du, dv, the nine images, the seven planes after stage 1 and the two inverse denominators after stage 2,
                            at 9 x 37 (two reference tiles each way): generic; warped positions on texel centres; on the 1/512
                            boundaries of the weight; more than a frame width outside on each side; gamma = 0
  brox_refstage_sor_*       u, v, du, dv, the coefficients, and du, dv after 1, 2, 3 and 5 solver iterations at 4 x 4, 7 x 33 and 17 x 65
  brox_refclass_*           frames, parameters, level sizes and the flow of NCVBroxOpticalFlow(); sf0.15_16x16 has a level of 3 x 3, the
                            smallest kind the plan lets through (a side of 1 leaves the plane in the reference's filter and is refused)
The smallest frame: the filter's mirror sends -2 to 3, so 4 is the smallest side that reads inside the plane.  Recorded here by
running the 4 x 4 derivative stage and the 4 x 4 class case a second time as views inside frames of NaN with a larger step and
asserting the same bits.  A re-run gives the same bytes (save_npz of tools/make_golden_stereocsbp.py).
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
import brox_numpy_ref as R  # noqa: E402
from make_golden_stereocsbp import save_npz  # noqa: E402  (fixed time stamps: the same arrays give the same bytes)

REF = os.environ.get("REF", "/root/reference")
SHIM = os.path.join(ROOT, "oracle", "refshim")
HERE = os.path.join(ROOT, "tools", "brox_ref")
GOLDEN = os.environ.get("BROX_GOLDEN_DIR", os.path.join(ROOT, "tests", "golden"))   # the tests re-record into a temporary directory
F = np.float32
NCV = os.path.join(REF, "modules", "cudalegacy", "src", "cuda", "NCVBroxOpticalFlow.cu")
NPP = os.path.join(REF, "modules", "cudalegacy", "src", "cuda", "NPP_staging.cu")


def have_reference():
    return os.path.exists(NCV) and os.path.exists(NPP)


def build(outdir):
    """Compiles the reference's kernels and host function for the host into `outdir` (outside the repository) -> the library's path."""
    out = lambda n: os.path.join(outdir, n)
    c2h = [sys.executable, os.path.join(SHIM, "cu2host.py")]
    common = ["-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-w"]
    cu = common + ["-D__CUDA_ARCH__=700", "-I" + outdir, "-I" + os.path.join(HERE, "cu"), "-I" + os.path.join(SHIM, "cudashim"),
                   "-include", os.path.join(SHIM, "cudashim", "cudashim.h")]
    steps = [
        c2h + [NPP, out("brox_npp.slice.cpp"), "--slice", "float getValueMirrorRow(", "// FrameInterpolate.cu",
               "float processLine(", "#endif /* CUDA_DISABLER */"],
        c2h + [out("brox_npp.slice.cpp"), out("brox_npp.gen.cpp")],
        c2h + [NCV, out("brox_ncv.gen.cpp")],
    ]
    # slices of the host function for the stage fixtures: cut, then the launch rewrite
    for name, start, end in (("down", "nppiStResize_32f_C1R (I0->ptr(), srcSize, prev_level_pitch", "// frame 1"),
                             ("up", "nppiStResize_32f_C1R (ptrU->ptr(), inner_srcSize", "ncvAssertCUDALastErrorReturn"),
                             ("filters", "// Ix0", "Texture texIx(kLevelHeight"),
                             ("grids", "dim3 psor_blocks(iDivUp(kLevelWidth", "// inner loop"),
                             ("stage1", "prepare_sor_stage_1_tex<<<", "ncvAssertCUDALastErrorReturn"),
                             ("stage2", "prepare_sor_stage_2<<<", "ncvAssertCUDALastErrorReturn"),
                             ("solver", "for (Ncv32u solver_iteration = 0", "}//end of solver loop")):
        steps += [c2h + [NCV, out(f"brox_s_{name}.slice.inc"), "--slice", start, end],
                  c2h + [out(f"brox_s_{name}.slice.inc"), out(f"brox_s_{name}.gen.inc")]]
    steps += [
        ["g++"] + cu + ["-c", os.path.join(HERE, "brox_ref.cpp"), "-o", out("brox_ref.o")],
        ["g++"] + cu + ["-c", os.path.join(SHIM, "cudashim", "cudashim.cpp"), "-o", out("cudashim.o")],
        ["gcc", "-O2", "-fPIC", "-fopenmp", "-ffp-contract=off", "-c", os.path.join(SHIM, "oclrt.c"), "-o", out("oclrt.o")],
        ["g++", "-shared", "-fopenmp", "-o", out("libbrox_ref.so"), out("brox_ref.o"), out("cudashim.o"), out("oclrt.o"), "-lm", "-Wl,--no-undefined"],
    ]
    for cmd in steps:
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(" ".join(cmd) + "\n" + r.stdout + r.stderr)
    return out("libbrox_ref.so")


def _pp(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


class Ref:
    """ctypes binding of the library build() makes; every plane is C-contiguous float32, rows x cols, stride = cols unless framed"""

    def __init__(self, path):
        self.L = C.CDLL(path)

    def resize(self, src, dh, dw, scale_factor, up):
        src = np.ascontiguousarray(src, F)
        dst = np.full((dh, dw), np.nan, F)
        fn = self.L.brox_ref_resize_up if up else self.L.brox_ref_resize_down
        st = fn(C.c_void_p(src.ctypes.data), src.shape[1], src.shape[0], src.shape[1], C.c_void_p(dst.ctypes.data), dw, dh, dw, C.c_float(scale_factor))
        assert st == 0, st
        return dst

    def derivatives(self, i0, i1, framed=False):
        rows, cols = i0.shape
        stride = cols + 5 if framed else cols
        def frame(a):
            f = np.full((rows + 4, stride), np.nan, F)
            f[2:2 + rows, 3:3 + cols] = a
            return f
        if framed:
            fa, fb = frame(i0), frame(i1)
            a, b = fa[2:, 3:], fb[2:, 3:]
            outs = [np.full((rows + 4, stride), np.nan, F) for _ in range(7)]
            views = [o[2:, 3:] for o in outs]
        else:
            a, b = np.ascontiguousarray(i0, F), np.ascontiguousarray(i1, F)
            outs = [np.full((rows, cols), np.nan, F) for _ in range(7)]
            views = outs
        ptrs = (C.c_void_p * 7)(*[v.ctypes.data for v in views])
        st = self.L.brox_ref_derivatives(C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), cols, rows, stride, ptrs)
        assert st == 0, st
        if framed:
            for o in outs:   # nothing outside the view was written
                m = np.ones(o.shape, bool); m[2:2 + rows, 3:3 + cols] = False
                assert np.isnan(o[m]).all()
        return {n: np.ascontiguousarray(v[:rows, :cols]) for n, v in zip(R.DERIV_NAMES, views)}

    def prepare(self, u, v, du, dv, im, alpha, gamma):
        rows, cols = u.shape
        flows = [np.ascontiguousarray(a, F) for a in (u, v, du, dv)]
        images = [np.ascontiguousarray(im[n], F) for n in R.IMAGE_NAMES]
        co = [np.full((rows, cols), np.nan, F) for _ in range(7)]
        assert 0 == self.L.brox_ref_prepare(1, _pp(flows), _pp(images), _pp(co), cols, rows, cols, C.c_float(alpha), C.c_float(gamma))
        names1 = ("diffusivity_x", "diffusivity_y", "denominator_u", "denominator_v", "numerator_dudv", "numerator_u", "numerator_v")
        stage1 = {n: a.copy() for n, a in zip(names1, co)}
        assert 0 == self.L.brox_ref_prepare(2, _pp(flows), _pp(images), _pp(co), cols, rows, cols, C.c_float(alpha), C.c_float(gamma))
        stage2 = {n: a.copy() for n, a in zip(R.COEFF_NAMES, co)}
        return stage1, stage2

    def sor(self, u, v, du, dv, c, iterations):
        rows, cols = u.shape
        flows = [np.ascontiguousarray(a, F).copy() for a in (u, v, du, dv)]
        tmp = [np.full((rows, cols), np.nan, F) for _ in range(2)]
        co = [np.ascontiguousarray(c[n], F) for n in R.COEFF_NAMES]
        assert 0 == self.L.brox_ref_sor(_pp(flows), _pp(tmp), _pp(co), cols, rows, cols, iterations)
        return flows[2], flows[3]

    def calc(self, i0, i1, p, framed=False):
        rows, cols = i0.shape
        if framed:
            fa, fb = (np.full((rows + 4, cols + 7), np.nan, F) for _ in range(2))
            fa[2:2 + rows, 3:3 + cols] = i0
            fb[2:2 + rows, 3:3 + cols] = i1
            a, b, pitch = fa[2:, 3:], fb[2:, 3:], (cols + 7) * 4
        else:
            a, b, pitch = np.ascontiguousarray(i0, F), np.ascontiguousarray(i1, F), cols * 4
        u, v = np.full((rows, cols), np.nan, F), np.full((rows, cols), np.nan, F)
        levels = np.zeros((256, 2), np.int32)
        n = C.c_int()
        st = self.L.brox_ref_calc(C.c_float(p["alpha"]), C.c_float(p["gamma"]), C.c_float(p["scale_factor"]), p["inner_iterations"], p["outer_iterations"],
                                  p["solver_iterations"], C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), cols, rows, pitch,
                                  C.c_void_p(u.ctypes.data), C.c_void_p(v.ctypes.data), cols * 4, 32, C.c_void_p(levels.ctypes.data), 256, C.byref(n))
        assert st == 0, st
        lv = levels[:n.value][::-1]   # finest first, (w, h) like level_sizes
        return np.ascontiguousarray(np.stack([u, v], axis=2)), np.ascontiguousarray(lv[:, ::-1])


FILTER_SIZES = ((4, 4), (5, 37), (13, 16))
DOWN_CASES = ((16, 16, 0.8), (23, 37, 0.8), (4, 4, 0.8), (5, 37, 0.8), (17, 21, 0.5), (17, 21, 0.95))   # rows, cols, scale_factor; dst by the pyramid's rule
UP_CASES = ((4, 4, 5, 5, 0.8), (4, 30, 5, 37, 0.8), (13, 16, 16, 20, 0.8), (9, 11, 17, 21, 0.5))   # src rows, cols, dst rows, cols, scale_factor


def run_filter(ref):
    rec = {}
    for rows, cols in FILTER_SIZES:
        i0, i1 = R.synth_pair(rows, cols, rows * 1000 + cols)
        d = ref.derivatives(i0, i1)
        tag = f"{rows}x{cols}"
        rec[f"I0_{tag}"], rec[f"I1_{tag}"] = i0, i1
        rec.update({f"{n}_{tag}": a for n, a in d.items()})
        if (rows, cols) == (4, 4):
            f = ref.derivatives(i0, i1, framed=True)
            assert all(bits_equal(d[n], f[n]) and np.isfinite(f[n]).all() for n in d), "a filter kernel read outside its 4 x 4 source"
    return rec


def down_size(rows, cols, sf):
    return int(np.ceil(F(rows) * F(sf))), int(np.ceil(F(cols) * F(sf)))   # the first level of the pyramid's rule


def run_resize(ref):
    rec = {}
    for rows, cols, sf in DOWN_CASES:
        src, _ = R.synth_pair(rows, cols, rows * 1000 + cols + 7)
        dh, dw = down_size(rows, cols, sf)
        tag = f"down_{rows}x{cols}_sf{sf}"
        rec[f"src_{tag}"], rec[f"dst_{tag}"] = src, ref.resize(src, dh, dw, sf, False)
    for rows, cols, dh, dw, sf in UP_CASES:
        src = R.synth_plane(rows, cols, rows * 1000 + cols + 9, -2.0, 2.0)
        tag = f"up_{rows}x{cols}_to_{dh}x{dw}_sf{sf}"
        rec[f"src_{tag}"], rec[f"dst_{tag}"] = src, ref.resize(src, dh, dw, sf, True)
    return rec


PREPARE_SHAPE = (9, 37)
PREPARE_CASES = ("generic", "centres", "boundaries", "outside", "gamma0")


def prepare_inputs(case):
    """-> u, v, du, dv, images, alpha, gamma"""
    rows, cols = PREPARE_SHAPE
    i0, i1 = R.synth_pair(rows, cols, 4242)
    im = R.derivatives(i0, i1)
    im["I0"], im["I1"] = i0, i1
    rs = np.random.RandomState(PREPARE_CASES.index(case) + 77)
    if case == "centres":        # whole pixels: the warped position falls on texel centres
        u, v = rs.randint(-3, 4, (rows, cols)).astype(F), rs.randint(-3, 4, (rows, cols)).astype(F)
    elif case == "boundaries":   # odd multiples of 1/512: the 1.8 fixed-point weight is at a rounding boundary
        u = ((2 * rs.randint(-600, 600, (rows, cols)) + 1) / 512.0).astype(F)
        v = ((2 * rs.randint(-600, 600, (rows, cols)) + 1) / 512.0).astype(F)
    elif case == "outside":      # more than one frame width / height outside, on each side: the periodic mirror
        sign = np.where(rs.rand(rows, cols) < 0.5, -1.0, 1.0)
        u = (sign * (cols + rs.rand(rows, cols) * 2.5 * cols)).astype(F)
        v = (np.where(rs.rand(rows, cols) < 0.5, -1.0, 1.0) * (rows + rs.rand(rows, cols) * 2.5 * rows)).astype(F)
    else:
        u, v = (rs.rand(rows, cols) * 3 - 1.5).astype(F), (rs.rand(rows, cols) * 3 - 1.5).astype(F)
    du, dv = (rs.rand(rows, cols) * 0.5 - 0.25).astype(F), (rs.rand(rows, cols) * 0.5 - 0.25).astype(F)
    return u, v, du, dv, im, 0.197, (0.0 if case == "gamma0" else 50.0)


def run_prepare(ref, case):
    u, v, du, dv, im, alpha, gamma = prepare_inputs(case)
    s1, s2 = ref.prepare(u, v, du, dv, im, alpha, gamma)
    rec = dict(u=u, v=v, du=du, dv=dv, alpha=np.array(alpha, F), gamma=np.array(gamma, F))
    rec.update({n: im[n] for n in R.IMAGE_NAMES})
    rec.update({"stage1_" + n: a for n, a in s1.items()})
    rec.update({"stage2_" + n: s2[n] for n in ("inv_denominator_u", "inv_denominator_v")})
    assert all(np.isfinite(a).all() for a in rec.values()), case
    if case == "outside":
        assert (np.abs(u) > PREPARE_SHAPE[1]).all() and (u < 0).any() and (u > 0).any() and (v < 0).any() and (v > 0).any()
    return rec


SOR_SHAPES = ((4, 4), (7, 33), (17, 65))
SOR_ITERATIONS = (1, 2, 3, 5)


def sor_inputs(rows, cols):
    i0, i1 = R.synth_pair(rows, cols, rows * 100 + cols)
    im = R.derivatives(i0, i1)
    im["I0"], im["I1"] = i0, i1
    rs = np.random.RandomState(rows * 100 + cols + 1)
    u, v = (rs.rand(rows, cols) - 0.5).astype(F), (rs.rand(rows, cols) - 0.5).astype(F)
    du, dv = (rs.rand(rows, cols) * 0.2 - 0.1).astype(F), (rs.rand(rows, cols) * 0.2 - 0.1).astype(F)
    return u, v, du, dv, im


def run_sor(ref, rows, cols):
    u, v, du, dv, im = sor_inputs(rows, cols)
    _, c = ref.prepare(u, v, du, dv, im, 0.197, 50.0)
    rec = dict(u=u, v=v, du=du, dv=dv)
    rec.update(c)
    for it in SOR_ITERATIONS:
        rec[f"du_it{it}"], rec[f"dv_it{it}"] = ref.sor(u, v, du, dv, c, it)
    assert all(np.isfinite(a).all() for a in rec.values()), (rows, cols)
    return rec


# name: (rows, cols, parameters)
CLASS_CASES = {
    "4x4": (4, 4, R.DEFAULTS),
    "16x16": (16, 16, R.DEFAULTS),
    "37x70": (37, 70, dict(R.DEFAULTS, inner_iterations=2, solver_iterations=3)),
    "70x37": (70, 37, dict(R.DEFAULTS, inner_iterations=2, solver_iterations=3)),
    "superres_48x64": (48, 64, R.SUPERRES),
    "sf0.5_40x50": (40, 50, dict(R.DEFAULTS, scale_factor=0.5, inner_iterations=2, solver_iterations=4)),
    "sf0.15_16x16": (16, 16, dict(R.DEFAULTS, scale_factor=0.15, inner_iterations=2, solver_iterations=3)),   # a 3 x 3 level: the mirror's second step
    "sf0.95_outer5_24x31": (24, 31, dict(R.DEFAULTS, scale_factor=0.95, outer_iterations=5, inner_iterations=2, solver_iterations=3)),
}
MIN_LEVELS = {"4x4": 1, "16x16": 2, "37x70": 3, "70x37": 3}


def run_class(ref, name):
    rows, cols, p = CLASS_CASES[name]
    i0, i1 = R.synth_pair(rows, cols, rows * 1000 + cols + 3)
    flow, levels = ref.calc(i0, i1, p)
    assert np.isfinite(flow).all(), name
    if name in MIN_LEVELS:
        assert len(levels) >= MIN_LEVELS[name] and (name not in ("4x4", "16x16") or len(levels) == MIN_LEVELS[name]), (name, levels)
    if name == "4x4":
        f2, _ = ref.calc(i0, i1, p, framed=True)
        assert bits_equal(flow, f2), "a 4 x 4 calc read outside its frames"
    print(f"{name}: {len(levels)} levels, coarsest {levels[-1][0]} x {levels[-1][1]}, max |flow| {np.abs(flow).max():.4g}")
    return dict(I0=i0, I1=i1, flow=flow, levels=levels.astype(np.int32),
                fparams=np.array([p["alpha"], p["gamma"], p["scale_factor"]], F),
                iparams=np.array([p["inner_iterations"], p["outer_iterations"], p["solver_iterations"]], np.int32))


def record(ref):
    recs = {"refstage_filter": run_filter(ref), "refstage_resize": run_resize(ref)}
    for case in PREPARE_CASES:
        recs[f"refstage_prepare_{case}"] = run_prepare(ref, case)
    for rows, cols in SOR_SHAPES:
        recs[f"refstage_sor_{rows}x{cols}"] = run_sor(ref, rows, cols)
    for name in CLASS_CASES:
        recs[f"refclass_{name}"] = run_class(ref, name)
    return recs


def main():
    if not have_reference():
        sys.exit("the reference tree is not at " + REF)
    with tempfile.TemporaryDirectory(prefix="brox_ref_") as tmp:
        ref = Ref(build(tmp))
        recs = record(ref)
        for name in sorted(recs):
            path = os.path.join(GOLDEN, f"brox_{name}.npz")
            save_npz(path, recs[name])
            print(path, os.path.getsize(path), "bytes")
            assert os.path.getsize(path) < 96 * 1024


if __name__ == "__main__":
    main()
