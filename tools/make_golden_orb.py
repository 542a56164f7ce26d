"""Writes tests/golden/orb_ref*.npz and orb_pattern31.npz: what the REFERENCE's own code computed for cv::cuda::ORB.

Built from the reference tree into a temporary directory, with the flags of tools/make_golden_fast.py (tools/orb_ref/ holds the C entry
points and the pieces the stubs lack):
  kernels, rewritten only at their launch sites by oracle/refshim/cu2host.py and run on the host through oracle/refshim/cudashim:
    cudafeatures2d/src/cuda/orb.cu (all five wrappers), fast.cu (through tools/fast_ref's entry points), the resize_linear kernel of
    cudawarping/src/cuda/resize.cu (oracle/refshim/cudashim/warping_cu_host.cpp instantiates it for uchar), and the 8uc1 row and
    32f -> 8u column filters of cudafilters/src/cuda;
  host arithmetic of cudafeatures2d/src/orb.cpp as SLICES of its text (cu2host.py --slice): the learned table of patch 31, both pattern
    generators and the constructor's "Calc pattern" statements, its quota and u_max statements, getScale and the level-size statements.
orb.cpp as a whole is NOT compiled: against oracle/refshim/cudahost it stops with 21 errors on members the stub core lacks (cv::RNG,
Mat::setTo / rowRange / the (rows, cols, type) constructor, Range, GpuMat::rowRange / setTo(Scalar) / operator()(Range, Range),
ensureSizeIsEnough(Size, ...), OutputArray::needed, cuda::threshold, cuda::bitwise_and, THRESH_TOZERO, NORM_HAMMING), and nothing under
oracle/ is edited.  So there are no class fixtures; the orchestration (which stage runs when) is restated in tests/orb_numpy_ref.py.
Also written by the glue or by this tool, not by the reference: cv::RNG (main repository; NO fixture pins it), the Gaussian's taps
(getGaussianKernel is main-repository), the factors of resize.cpp:82-83,105, THRESH_TOZERO, bitwise_and and the frame (cudaarithm kernels
that are not built here; one comparison and one AND per pixel).

    python tools/make_golden_orb.py            # needs the reference tree (REF, default /root/reference)

  orb_pattern31.npz       the learned pool of patch 31 as (512, 2) points: data the reference's class uploads.  Tests load it; nothing else.
  orb_refhost.npz         quotas, u_max, scales, level sizes and the uploaded pattern matrices (patch 31: WTA_K 2, 3, 4 from the learned
                          pool; patches 29 and 9 from the glue's RNG).
  orb_refstage_<case>     image, keypoint locations, u_max and the pattern (inputs), and per kernel wrapper on its own: Harris responses,
                          cull_gpu's sorted head of them, IC_Angle's angles (glibc atan2f), descriptors on those angles (glibc sincosf),
                          mergeLocation's coordinates, and the blurred image of the two filter kernels.
  orb_refstage_pyramid    three levels with firstLevel 1 and a mask: every level's image and mask, and FAST's keypoints on every level.
  orb_refstage_cullfast   cull_gpu on FAST scores at a cut no tie straddles.
  orb_refstage_ties       the `blocks` image: cull_gpu on FAST scores at a cut INSIDE a run of equal scores; compared as a multiset.

Asserted on the reference's outputs while recording: every stage case has at least 64 keypoints; no tie straddles the cut of a strict
fixture; in `ties` (at least 64 keypoints) the cut falls inside a run of at least 16 equal scores; every level's FAST candidate count is at most int(0.05 area) and at least two levels have keypoints; the
largest distance between the restatement's angles and the reference's is at most 4 ulp (recorded as `angle_max_ulp`); the descriptor bits
that differ from the restatement's all are tie-sensitive, and the tie-sensitive share is at most 0.5 % (recorded).
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
import fast_numpy_ref as FR  # noqa: E402
import orb_numpy_ref as R  # noqa: E402
from make_golden_stereocsbp import save_npz  # noqa: E402  (fixed time stamps: the same arrays give the same bytes)

REF = os.environ.get("REF", "/root/reference")
SHIM = os.path.join(ROOT, "oracle", "refshim")
HERE = os.path.join(ROOT, "tools", "orb_ref")
FAST_HERE = os.path.join(ROOT, "tools", "fast_ref")
GOLDEN = os.path.join(ROOT, "tests", "golden")
F = np.float32


def have_reference():
    return os.path.exists(os.path.join(REF, "modules", "cudafeatures2d", "src", "cuda", "orb.cu"))


def build(outdir):
    """Compiles the reference's kernels and the slices of orb.cpp for the host into `outdir` (outside the repository) -> the library's path."""
    out = lambda n: os.path.join(outdir, n)
    mod = lambda *a: os.path.join(REF, "modules", *a)
    c2h = [sys.executable, os.path.join(SHIM, "cu2host.py")]
    common = ["-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-w"]
    shim = ["-I" + os.path.join(SHIM, "cudashim"), "-include", os.path.join(SHIM, "cudashim", "cudashim.h")]
    cu = common + ["-D__CUDA_ARCH__=700", "-I" + os.path.join(HERE, "cu")] + shim
    cufast = common + ["-D__CUDA_ARCH__=700", "-I" + os.path.join(FAST_HERE, "cu")] + shim
    cuvec = common + ["-D__CUDA_ARCH__=700", "-I" + outdir, "-I" + os.path.join(HERE, "cu"), "-I" + os.path.join(SHIM, "cudavec")] + shim
    orb_cpp = mod("cudafeatures2d", "src", "orb.cpp")
    flt = mod("cudafilters", "src", "cuda")
    slices = [("orb_table", "const int bit_pattern_31_[256 * 4]", "class ORB_Impl : public"),
              ("orb_pattern", "static void initializeOrbPattern", "ORB_Impl::ORB_Impl(int nFeatures"),
              ("orb_ctor", "// fill the extractors and descriptors", "cv::cuda::device::orb::loadUMax"),
              ("orb_calc", "// Calc pattern", "pattern_.upload(h_pattern)"),
              ("orb_scale", "static float getScale", "void ORB_Impl::detectAndCompute("),
              ("orb_size", "float scale = 1.0f / getScale", "ensureSizeIsEnough(sz, image.type()")]
    steps = [c2h + [orb_cpp, out(n + ".gen.inc"), "--slice", a, b] for n, a, b in slices]
    steps += [
        ["g++"] + common + ["-I" + outdir, "-c", os.path.join(HERE, "orb_ref_host.cpp"), "-o", out("orb_ref_host.o")],
        c2h + [mod("cudafeatures2d", "src", "cuda", "orb.cu"), out("orb.gen.cpp")],
        ["g++"] + cu + ["-c", out("orb.gen.cpp"), "-o", out("orb.gen.o")],
        ["g++"] + cu + ["-c", os.path.join(HERE, "orb_ref_stage.cpp"), "-o", out("orb_ref_stage.o")],
        c2h + [mod("cudafeatures2d", "src", "cuda", "fast.cu"), out("fast.gen.cpp")],
        ["g++"] + cufast + ["-c", out("fast.gen.cpp"), "-o", out("fast.gen.o")],
        ["g++"] + cufast + ["-c", os.path.join(FAST_HERE, "fast_ref_stage.cpp"), "-o", out("fast_ref_stage.o")],
        c2h + [mod("cudawarping", "src", "cuda", "resize.cu"), out("resize.gen.inc"), "--extract", "resize_linear"],
        c2h + [mod("cudawarping", "src", "cuda", "pyr_down.cu"), out("pyrdown.gen.inc"), "--extract", "pyrDown"],
        [sys.executable, "-c", "import sys; open(sys.argv[3], 'w').write(open(sys.argv[1]).read() + open(sys.argv[2]).read())", out("resize.gen.inc"),
         out("pyrdown.gen.inc"), out("warping.gen.inc")],
        ["g++"] + common + ["-I" + outdir] + shim + ["-c", os.path.join(SHIM, "cudashim", "warping_cu_host.cpp"), "-o", out("warping_cu_host.o")],
        c2h + [os.path.join(flt, "row_filter.hpp"), out("row_filter.hpp")],
        c2h + [os.path.join(flt, "column_filter.hpp"), out("column_filter.hpp")],
        c2h + [os.path.join(flt, "row_filter.8uc1.cu"), out("row_filter.8uc1.gen.cpp")],
        c2h + [os.path.join(flt, "column_filter.8uc1.cu"), out("column_filter.8uc1.gen.cpp")],
        ["g++"] + cuvec + ["-c", out("row_filter.8uc1.gen.cpp"), "-o", out("row_filter.8uc1.gen.o")],
        ["g++"] + cuvec + ["-c", out("column_filter.8uc1.gen.cpp"), "-o", out("column_filter.8uc1.gen.o")],
        ["g++"] + cuvec + ["-c", os.path.join(HERE, "orb_ref_filters.cpp"), "-o", out("orb_ref_filters.o")],
        ["g++"] + cu + ["-c", os.path.join(SHIM, "cudashim", "cudashim.cpp"), "-o", out("cudashim.o")],
        ["gcc", "-O2", "-fPIC", "-fopenmp", "-ffp-contract=off", "-c", os.path.join(SHIM, "oclrt.c"), "-o", out("oclrt.o")],
        ["g++", "-shared", "-fopenmp", "-o", out("liborb_ref.so")] + [out(n) for n in (
            "orb_ref_host.o", "orb.gen.o", "orb_ref_stage.o", "fast.gen.o", "fast_ref_stage.o", "warping_cu_host.o", "row_filter.8uc1.gen.o",
            "column_filter.8uc1.gen.o", "orb_ref_filters.o", "cudashim.o", "oclrt.o")] + ["-lm", "-Wl,--no-undefined"],
    ]
    for cmd in steps:
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(" ".join(cmd) + "\n" + r.stdout + r.stderr)
    return out("liborb_ref.so")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Ref:
    """ctypes binding of the library build() makes.  The orb.cu wrappers want npoints as a multiple of 8 (tools/orb_ref/orb_ref_stage.cpp)."""

    def __init__(self, path):
        self.L = C.CDLL(path)
        self.L.orb_ref_scale.restype = C.c_float

    # ---- orb.cu
    def harris(self, img, loc):
        resp = np.zeros(len(loc), F)
        self.L.orb_ref_harris(_p(img), img.shape[0], img.shape[1], _p(loc), _p(resp), len(loc))
        return resp

    def angle(self, img, loc, u_max, half_k):
        ang = np.zeros(len(loc), F)
        um = np.array(u_max, np.int32)
        self.L.orb_ref_angle(_p(img), img.shape[0], img.shape[1], _p(loc), _p(ang), len(loc), _p(um), len(um), half_k)
        return ang

    def descriptors(self, img, loc, ang, pat, wta_k):
        desc = np.zeros((len(loc), 32), np.uint8)
        pat = np.ascontiguousarray(pat, np.int32)
        self.L.orb_ref_descriptors(_p(img), img.shape[0], img.shape[1], _p(loc), _p(ang), len(loc), _p(pat), pat.shape[1], wta_k, _p(desc))
        return desc

    def cull(self, loc, resp, n):
        l, r = np.ascontiguousarray(loc).copy(), resp.copy()
        kept = self.L.orb_ref_cull(_p(l), _p(r), len(r), n)
        return l[:kept], r[:kept]

    def merge(self, loc, scale):
        x, y = np.zeros(len(loc), F), np.zeros(len(loc), F)
        self.L.orb_ref_merge(_p(loc), _p(x), _p(y), len(loc), C.c_float(scale))
        return x, y

    # ---- fast.cu, resize.cu, the filters
    def fast(self, img, mask, threshold, max_npoints):
        """FAST_Impl::detectAsync's two wrappers with suppression -> (candidates, loc (n, 2) int16, response (n,) f32)"""
        img = np.ascontiguousarray(img)
        mask = None if mask is None else np.ascontiguousarray(mask)
        score = np.zeros(img.shape, np.int32)
        kp = np.zeros((max_npoints, 2), np.int16)
        count = self.L.fast_ref_calc_keypoints(_p(img), _p(mask), img.shape[0], img.shape[1], threshold, max_npoints, _p(score), _p(kp))
        kp = np.ascontiguousarray(kp[:min(count, max_npoints)])
        loc, resp = np.zeros((max(len(kp), 1), 2), np.int16), np.zeros(max(len(kp), 1), F)
        m = self.L.fast_ref_nonmax_suppression(_p(kp), len(kp), _p(score), img.shape[0], img.shape[1], _p(loc), _p(resp)) if len(kp) else 0
        return count, loc[:m].copy(), resp[:m].copy()

    def resize(self, src, drows, dcols):
        """the kernel with the factors of resize.cpp:82-83,105"""
        src = np.ascontiguousarray(src)
        dst = np.zeros((drows, dcols), np.uint8)
        fx, fy = F(1.0 / (dcols / src.shape[1])), F(1.0 / (drows / src.shape[0]))
        self.L.ref_cu_resize_linear_u8(_p(src), src.shape[0], src.shape[1], _p(dst), drows, dcols, C.c_float(fy), C.c_float(fx))
        return dst

    def blur(self, img, taps):
        img = np.ascontiguousarray(img)
        dst, buf = np.zeros(img.shape, np.uint8), np.zeros(img.shape, F)
        self.L.orb_ref_blur(_p(img), img.shape[0], img.shape[1], _p(np.ascontiguousarray(taps, F)), len(taps), _p(dst), _p(buf))
        return dst

    # ---- slices of orb.cpp
    def table31(self):
        t = np.zeros((512, 2), np.int32)
        self.L.orb_ref_table31(_p(t))
        return t

    def ctor(self, nfeatures, scale_factor, nlevels, patch):
        q, um, n = np.zeros(nlevels, np.int32), np.zeros(64, np.int32), C.c_int()
        assert self.L.orb_ref_ctor(nfeatures, C.c_float(scale_factor), nlevels, patch, _p(q), _p(um), C.byref(n)) == 0
        return q, um[:n.value].copy()

    def pattern(self, patch, wta):
        out, n = np.zeros(1024, np.int32), C.c_int()
        assert self.L.orb_ref_pattern(patch, wta, _p(out), C.byref(n)) == 0
        return out[:2 * n.value].reshape(2, n.value).copy()

    def scale(self, scale_factor, first, level):
        return F(self.L.orb_ref_scale(C.c_float(scale_factor), first, level))

    def level_size(self, rows, cols, scale_factor, first, level):
        r, c = C.c_int(), C.c_int()
        self.L.orb_ref_level_size(rows, cols, C.c_float(scale_factor), first, level, C.byref(r), C.byref(c))
        return r.value, c.value


def corners_image(rows, cols, seed):
    """noise smoothed once (integer arithmetic only)"""
    n = FR.synth_image(rows + 2, cols + 2, seed, "noise").astype(np.int64)
    s = n[:-2, :-2] + n[:-2, 2:] + n[2:, :-2] + n[2:, 2:] + 2 * (n[1:-1, :-2] + n[1:-1, 2:] + n[:-2, 1:-1] + n[2:, 1:-1]) + 4 * n[1:-1, 1:-1]
    return ((s - s.min()) * 255 // max(1, s.max() - s.min())).astype(np.uint8)


def ulps(a, b):
    """distance in f32 ulps between two arrays of non-negative finite floats"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# name -> (rows, cols, seed, patch, wta_k)
CASES = [("p31_wta2", 120, 203, 31, 31, 2), ("p31_wta3", 97, 131, 32, 31, 3), ("p9_wta4", 97, 131, 33, 9, 4), ("p29_wta2", 120, 203, 34, 29, 2)]


def run_case(ref, name, rows, cols, seed, patch, wta):
    """patch 31 runs on the LEARNED pool, as the reference's class does"""
    img = corners_image(rows, cols, seed)
    pat = ref.pattern(patch, wta)
    _, um = ref.ctor(500, 1.2, 8, patch)
    margin = max(R.pattern_reach(pat), patch // 2, 4)
    mask = np.zeros((rows, cols), np.uint8)
    mask[margin:rows - margin, margin:cols - margin] = 255
    _, loc, fast_resp = ref.fast(img, mask, 20, int(0.05 * rows * cols))
    o = np.lexsort((loc[:, 0], loc[:, 1]))   # the reference appends in the order its blocks ran: row-major here
    loc = loc[o]
    n = len(loc) // 8 * 8
    assert n >= 64, (name, len(loc))
    loc = np.ascontiguousarray(loc[:n])
    harris = ref.harris(img, loc)
    ang = ref.angle(img, loc, um, patch // 2)
    desc = ref.descriptors(img, loc, ang, pat, wta)
    x, y = ref.merge(loc, 1.44)
    # a cut no tie straddles, searched downwards from a third of the keypoints
    order = np.sort(harris)[::-1]
    ncut = next(k for k in range(n // 3, 0, -1) if order[k - 1] != order[k])
    cull_loc, cull_resp = ref.cull(loc.view(np.int32).reshape(-1), harris, ncut)
    assert len(cull_resp) == ncut and cull_resp[-1] > order[ncut]
    # the conditions of the yardstick, on the reference's outputs
    m01, m10 = R.moments(img, loc, patch)
    max_ulp = int(ulps(R.angle_from_moments(m01, m10), ang).max())
    assert max_ulp <= 4, (name, max_ulp)
    tie = R.tie_sensitive_bits(loc, ang, pat, wta)
    diff = np.unpackbits(R.descriptors(img, loc, ang, pat, wta) ^ desc, axis=1, bitorder="little").reshape(n, 32, 8).astype(bool)
    assert not (diff & ~tie).any(), (name, int((diff & ~tie).sum()))
    share = float(tie.mean())
    assert share <= 0.005, (name, share)
    print(f"{name}: {n} keypoints, cut at {ncut}, angle max {max_ulp} ulp, tie-sensitive share {share:.2e}, differing bits {int(diff.sum())}")
    return dict(img=img, loc=loc, patch_size=np.array(patch), wta_k=np.array(wta), u_max=um, pattern=pat, harris=harris,
                angle=ang, descriptors=desc, merge_x=x, merge_y=y, merge_scale=np.array(1.44, F), cull_n=np.array(ncut),
                cull_loc=cull_loc.view(np.int16).reshape(-1, 2), cull_resp=cull_resp, angle_max_ulp=np.array(max_ulp),
                tie_sensitive_share=np.array(share), blur=ref.blur(img, R.gaussian_taps()))


def run_host(ref):
    rec = {}
    for i, (n, s, L) in enumerate(((500, 1.2, 8), (4000, 1.2, 8), (60, 1.2, 2), (7, 1.5, 3), (1, 1.2, 2), (1000, 2.0, 1))):
        q, _ = ref.ctor(n, s, L, 31)
        rec[f"quota_{i}_args"], rec[f"quota_{i}"] = np.array([n, s, L], np.float64), q
    for patch in (2, 3, 9, 29, 31, 59):
        rec[f"u_max_{patch}"] = ref.ctor(500, 1.2, 8, patch)[1]
    rec["scales_1.2_first1"] = np.array([ref.scale(1.2, 1, l) for l in range(8)], F)
    rec["scales_1.2_first0"] = np.array([ref.scale(1.2, 0, l) for l in range(8)], F)
    for rows, cols, first in ((480, 640, 0), (97, 131, 1), (1080, 1920, 0), (75, 131, 0)):
        rec[f"sizes_{rows}x{cols}_first{first}"] = np.array([ref.level_size(rows, cols, 1.2, first, l) for l in range(8)], np.int32)
    for patch, wta in ((31, 2), (31, 3), (31, 4), (29, 2), (29, 3), (9, 4)):
        rec[f"pattern_p{patch}_wta{wta}"] = ref.pattern(patch, wta)
    return rec


def run_pyramid(ref):
    """buildScalePyramids (orb.cpp:661-719) level by level with the reference's resize kernel, then FAST as computeKeyPointsPyramid runs it"""
    for th in range(20, 200, 10):   # the first threshold at which no level has more candidates than FAST keeps
        try:
            return _pyramid(ref, th)
        except OverflowError:
            pass
    raise AssertionError("no threshold keeps every level's candidates within 5 % of its area")


def _pyramid(ref, th):
    rows, cols, first, edge, nlevels, sf = 97, 131, 1, 9, 3, 1.2
    img = corners_image(rows, cols, 41)
    mask = FR.synth_mask(rows, cols, 41)
    mask[10:80, 15:110] = 255
    rec = dict(img=img, mask=mask, params=np.array([first, edge, nlevels, th], np.int32), scale_factor=np.array(sf, F))
    imgs, masks, with_kp = [], [], 0
    for l in range(nlevels):
        r, c = ref.level_size(rows, cols, sf, first, l)
        if l == first:
            li, lm = img.copy(), mask.copy()
        elif l < first:
            li, lm = ref.resize(img, r, c), ref.resize(mask, r, c)
        else:
            li, lm = ref.resize(imgs[l - 1], r, c), ref.resize(masks[l - 1], r, c)
            lm = np.where(lm > 254, lm, 0).astype(np.uint8)          # THRESH_TOZERO at 254
        frame = np.zeros((r, c), np.uint8)
        frame[edge:r - edge, edge:c - edge] = 255
        lm = lm & frame
        imgs.append(li)
        masks.append(lm)
        cap = int(0.05 * r * c)
        count, loc, resp = ref.fast(li, lm, th, cap)
        if count > cap:   # the reference's set would depend on the order its blocks ran
            raise OverflowError
        o = np.lexsort((loc[:, 0], loc[:, 1]))
        with_kp += len(loc) > 0
        rec.update({f"img_{l}": li, f"mask_{l}": lm, f"fast_count_{l}": np.array(count), f"fast_loc_{l}": loc[o], f"fast_resp_{l}": resp[o]})
        print(f"pyramid level {l}: {r} x {c}, {count} candidates (cap {cap}), {len(loc)} keypoints")
    assert with_kp >= 2
    return rec


def run_cull_fast(ref):
    """cull_gpu on FAST scores: a strict cut on smoothed noise, and a cut inside a run of equal scores on the `blocks` image"""
    out = {}
    for name, img, th in (("cullfast", corners_image(120, 203, 51), 20), ("ties", FR.synth_image(400, 640, FR_SEED_BLOCKS, "blocks"), 10)):
        # `blocks` has more candidates than 5 % of its area: FAST keeps them all here, so that its set does not depend on the order the
        # reference's blocks ran in (the cull is what this fixture is about)
        _, loc, resp = ref.fast(img, None, th, img.size if name == "ties" else int(0.05 * img.size))
        o = np.lexsort((loc[:, 0], loc[:, 1]))
        loc, resp = np.ascontiguousarray(loc[o]), np.ascontiguousarray(resp[o])
        order = np.sort(resp)[::-1]
        n = len(resp)
        if name == "ties":
            ncut = next(k for k in range(n // 2, 0, -1) if order[k - 1] == order[k])
            assert order[ncut - 1] == order[ncut] and n >= 64 and int((resp == order[ncut]).sum()) >= 16, (n, ncut)
            assert 0 < int((order[:ncut] == order[ncut]).sum()) < int((resp == order[ncut]).sum())   # some of the run kept, some cut
        else:
            ncut = next(k for k in range(n // 3, 0, -1) if order[k - 1] != order[k])
            assert order[ncut - 1] > order[ncut] and len(np.unique(order[:ncut])) < ncut   # ties INSIDE the kept set, none across the cut
        cl, cr = ref.cull(loc.view(np.int32).reshape(-1), resp, ncut)
        assert len(cr) == ncut
        print(f"{name}: {n} FAST keypoints, cut at {ncut}, {int((resp == order[ncut - 1]).sum())} equal to the last kept")
        out[f"refstage_{name}"] = dict(img=img, threshold=np.array(th), loc=loc, resp=resp, cull_n=np.array(ncut),
                                       cull_loc=cl.view(np.int16).reshape(-1, 2), cull_resp=cr)
    return out


FR_SEED_BLOCKS = sum(map(ord, "blocks"))   # the seed of tools/make_golden_fast.py's blocks case


def main():
    if not have_reference():
        sys.exit("the reference tree is not at " + REF)
    with tempfile.TemporaryDirectory(prefix="orb_ref_") as tmp:
        ref = Ref(build(tmp))
        recs = {"pattern31": dict(pattern0=ref.table31()), "refhost": run_host(ref), "refstage_pyramid": run_pyramid(ref)}
        assert recs["pattern31"]["pattern0"].shape == (512, 2) and np.abs(recs["pattern31"]["pattern0"]).max() <= 15
        for case in CASES:
            recs[f"refstage_{case[0]}"] = run_case(ref, *case)
        recs.update(run_cull_fast(ref))
        for name in sorted(recs):
            path = os.path.join(GOLDEN, f"orb_{name}.npz")
            save_npz(path, recs[name])
            print(path, os.path.getsize(path), "bytes")
            assert os.path.getsize(path) < 176 * 1024


if __name__ == "__main__":
    main()
