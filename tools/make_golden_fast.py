"""Writes tests/golden/fast_refclass_*.npz and fast_refstage_*.npz: what the REFERENCE's own FastFeatureDetector computed.

The reference's kernels (modules/cudafeatures2d/src/cuda/fast.cu, rewritten only at their launch sites by oracle/refshim/cu2host.py and run on
the host through oracle/refshim/cudashim) and its host class (modules/cudafeatures2d/src/fast.cpp and feature2d_async.cpp, compiled as they
lie against the stub core of oracle/refshim/cudahost) are built from the reference tree into a temporary directory; tools/fast_ref/ holds
the C entry points and the pieces the stubs lack.  Only the recorded inputs, parameters and outputs are kept.

    python tools/make_golden_fast.py            # needs the reference tree (REF, default /root/reference)

  refclass: image, mask, parameters, the 2 x n matrix of detectAsync and the keypoints of convert, with suppression and without.
  refstage: for the same inputs the two kernel wrappers on their own: calcKeypoints_gpu's counter, its kpLoc and its CV_32SC1 score plane,
            nonmaxSuppression_gpu's locations and responses; and the candidate bits at the 65 536 patch centres of both
            fast_numpy_ref.all_masks_image polarities at threshold 10.
The reference's ORDER is the arrival order of its atomics (here: the order the shim runs the blocks in); consumers compare as sets.

Asserted on the reference's outputs, so that no fixture is vacuous: every noise / blocks class case has at least 50 candidates and every
one of them, the masked and the truncated one loses at least one candidate to suppression (the flat image has no candidate and the 7 x 7 one
a single corner: nothing to suppress); blocks has at least 100 candidates with an equal-score neighbour, noise 23 x 71 at threshold 10 at
least one; both all-masks images have 1 025 candidate centres.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fast_numpy_ref import all_masks_image, centre_bitmap, synth_image, synth_mask  # noqa: E402  (inputs and packing, nothing of the algorithm)
from make_golden_stereocsbp import save_npz  # noqa: E402  (fixed time stamps: the same arrays give the same bytes)

REF = os.environ.get("REF", "/root/reference")
SHIM = os.path.join(ROOT, "oracle", "refshim")
HERE = os.path.join(ROOT, "tools", "fast_ref")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def have_reference():
    return os.path.exists(os.path.join(REF, "modules", "cudafeatures2d", "src", "cuda", "fast.cu"))


def build(outdir):
    """Compiles the reference's fast.cu, fast.cpp and feature2d_async.cpp for the host into `outdir` (outside the repository) -> the
    library's path."""
    out = lambda n: os.path.join(outdir, n)
    cf = os.path.join(REF, "modules", "cudafeatures2d")
    common = ["-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-w"]
    # __CUDA_ARCH__: the kernels' bodies are inside #if __CUDA_ARCH__ >= 110 (fast.cu:214,314)
    cu = common + ["-D__CUDA_ARCH__=700", "-I" + os.path.join(HERE, "cu"), "-I" + os.path.join(SHIM, "cudashim"), "-include",
                   os.path.join(SHIM, "cudashim", "cudashim.h")]
    ch = common + ["-fno-gnu-unique", "-I" + HERE, "-I" + os.path.join(SHIM, "cudahost"), "-I" + os.path.join(SHIM, "cudashim"),
                   "-I" + os.path.join(cf, "include"), "-I" + os.path.join(cf, "src")]
    steps = [
        [sys.executable, os.path.join(SHIM, "cu2host.py"), os.path.join(cf, "src", "cuda", "fast.cu"), out("fast.gen.cpp")],
        ["g++"] + cu + ["-c", out("fast.gen.cpp"), "-o", out("fast.gen.o")],
        ["g++"] + cu + ["-c", os.path.join(HERE, "fast_ref_stage.cpp"), "-o", out("fast_ref_stage.o")],
        ["g++"] + cu + ["-c", os.path.join(SHIM, "cudashim", "cudashim.cpp"), "-o", out("cudashim.o")],
        ["g++"] + ch + ["-c", os.path.join(cf, "src", "fast.cpp"), "-o", out("fast_host.o")],
        ["g++"] + ch + ["-c", os.path.join(cf, "src", "feature2d_async.cpp"), "-o", out("feature2d_async.o")],
        ["g++"] + ch + ["-c", os.path.join(HERE, "fast_ref_class.cpp"), "-o", out("fast_ref_class.o")],
        ["gcc", "-O2", "-fPIC", "-fopenmp", "-ffp-contract=off", "-c", os.path.join(SHIM, "oclrt.c"), "-o", out("oclrt.o")],
        ["g++", "-shared", "-fopenmp", "-o", out("libfast_ref.so"), out("fast.gen.o"), out("fast_ref_stage.o"), out("cudashim.o"), out("fast_host.o"),
         out("feature2d_async.o"), out("fast_ref_class.o"), out("oclrt.o"), "-lm", "-Wl,--no-undefined"],
    ]
    for cmd in steps:
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(" ".join(cmd) + "\n" + r.stdout + r.stderr)
    return out("libfast_ref.so")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Ref:
    """ctypes binding of the library build() makes"""

    def __init__(self, path):
        self.L = C.CDLL(path)

    def detect(self, img, mask, threshold, nms, max_npoints):
        """-> (the 2 x n float32 matrix of detectAsync, (n, 5) keypoints of convert, getMaxNumPoints())"""
        img = np.ascontiguousarray(img)
        mask = None if mask is None else np.ascontiguousarray(mask)
        out = np.zeros(2 * max_npoints, np.float32)
        kp = np.zeros((max_npoints, 5), np.float32)
        after = C.c_int(-1)
        n = self.L.fast_ref_detect(_p(img), _p(mask), img.shape[0], img.shape[1], threshold, int(nms), max_npoints, _p(out), _p(kp), C.byref(after))
        assert n >= 0, n
        return out[:2 * n].reshape(2, n).copy(), kp[:n].copy(), after.value

    def create_accepts_type(self, t):
        return bool(self.L.fast_ref_create_accepts_type(t))

    def calc_keypoints(self, img, mask, threshold, max_keypoints, with_score=True):
        """-> (the counter, kpLoc[:min(counter, max_keypoints)] as (n, 2) int16 {x, y}, the score plane or None)"""
        img = np.ascontiguousarray(img)
        mask = None if mask is None else np.ascontiguousarray(mask)
        score = np.full(img.shape, -1, np.int32) if with_score else None
        loc = np.zeros((max_keypoints, 2), np.int16)
        count = self.L.fast_ref_calc_keypoints(_p(img), _p(mask), img.shape[0], img.shape[1], threshold, max_keypoints, _p(score), _p(loc))
        return count, loc[:min(count, max_keypoints)].copy(), score

    def nonmax_suppression(self, kp_loc, score):
        n = len(kp_loc)
        loc, resp = np.zeros((max(n, 1), 2), np.int16), np.zeros(max(n, 1), np.float32)
        m = self.L.fast_ref_nonmax_suppression(_p(np.ascontiguousarray(kp_loc)), n, _p(np.ascontiguousarray(score)), score.shape[0], score.shape[1],
                                               _p(loc), _p(resp))
        return loc[:m].copy(), resp[:m].copy()


def corner7():
    """7 x 7 with one hand-made corner: eleven ring pixels 60 above the centre"""
    img = np.full((7, 7), 50, np.uint8)
    for dy, dx in [(3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2)]:
        img[3 + dy, 3 + dx] = 110
    return img


def case_seed(name):
    return sum(map(ord, name))


# name -> (image, mask or None, threshold, max_npoints, kind); every case is recorded with suppression (nms) and without (raw)
def cases():
    out = []
    for rows, cols in ((23, 71), (40, 140)):
        for th in (0, 10, 60):
            name = f"noise{rows}x{cols}_t{th}"
            out.append((name, synth_image(rows, cols, case_seed(name), "noise"), None, th, 5000, "noise"))
    out.append(("blocks", synth_image(40, 140, case_seed("blocks"), "blocks"), None, 10, 5000, "blocks"))
    out.append(("masked", synth_image(40, 140, case_seed("masked"), "noise"), synth_mask(40, 140, case_seed("masked")), 10, 5000, "masked"))
    out.append(("flat", synth_image(23, 71, 0, "flat"), None, 10, 5000, "flat"))
    out.append(("corner7", corner7(), None, 10, 5000, "corner"))
    out.append(("truncated", synth_image(40, 140, case_seed("truncated"), "noise"), None, 10, 100, "truncated"))
    return out


def ties(score, loc):
    """candidates with an equal-score candidate neighbour, from the reference's plane and candidate set"""
    cand = np.zeros(score.shape, bool)
    cand[loc[:, 1], loc[:, 0]] = True
    y, x = loc[:, 1].astype(int), loc[:, 0].astype(int)
    t = np.zeros(len(loc), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                t |= cand[y + dy, x + dx] & (score[y + dy, x + dx] == score[y, x])
    return int(t.sum())


def run_case(ref, case):
    """-> {file suffix: record}"""
    name, img, mask, th, maxn, kind = case
    recs = {}
    base = dict(img=img, threshold=np.array(th), max_npoints=np.array(maxn))
    if mask is not None:
        base["mask"] = mask
    # the stage: every candidate (a kpLoc as large as the image), then the class's own cut
    count, all_loc, score = ref.calc_keypoints(img, mask, th, img.size)
    count_cut, cut_loc, score_cut = ref.calc_keypoints(img, mask, th, maxn)
    assert count_cut == count and np.array_equal(score, score_cut)
    count_raw, raw_loc, none = ref.calc_keypoints(img, mask, th, img.size, with_score=False)
    assert count_raw == count and none is None and np.array_equal(raw_loc, all_loc)
    nms_loc, nms_resp = ref.nonmax_suppression(all_loc, score)
    cut_nms_loc, cut_nms_resp = ref.nonmax_suppression(cut_loc, score)
    recs[f"refstage_{name}"] = dict(base, count=np.array(count), kp_loc=all_loc, score=score, nms_loc=nms_loc, nms_resp=nms_resp, cut_loc=cut_loc,
                                    cut_nms_loc=cut_nms_loc, cut_nms_resp=cut_nms_resp)
    if kind in ("noise", "blocks"):
        assert count >= 50, (name, count)
    if kind in ("noise", "blocks", "masked", "truncated"):
        assert len(nms_loc) < count and len(cut_nms_loc) < len(cut_loc), name
    if kind == "blocks":
        assert ties(score, all_loc) >= 100, ties(score, all_loc)
    if name == "noise23x71_t10":
        assert ties(score, all_loc) >= 1
    if kind == "truncated":
        assert count > maxn
    for nms in (True, False):
        mat, kp, after = ref.detect(img, mask, th, nms, maxn)
        assert after == maxn
        # the class is its two wrappers (fast.cpp:143-172)
        want = (cut_nms_loc, cut_nms_resp) if nms else (cut_loc, np.zeros(len(cut_loc), np.float32))
        assert np.array_equal(mat[0].view(np.int16).reshape(-1, 2), want[0]) and np.array_equal(mat[1], want[1]), name
        recs[f"refclass_{name}_{'nms' if nms else 'raw'}"] = dict(base, nonmax_suppression=np.array(int(nms)), keypoints=mat, converted=kp,
                                                                 count=np.array(count))
    return recs


def run_all_masks(ref):
    rec = {}
    for name, pol in (("bright", 1), ("dark", -1)):
        img = all_masks_image(pol)
        count, loc, _ = ref.calc_keypoints(img, None, 10, img.size, with_score=False)
        cand = np.zeros(img.shape, bool)
        cand[loc[:, 1], loc[:, 0]] = True
        assert int(cand.sum()) == count
        rec[name] = centre_bitmap(cand)
        assert rec[name].size == 8192 and int(np.unpackbits(rec[name]).sum()) == 1025, name
    return {"refstage_allmasks_t10": rec}


def main():
    if not have_reference():
        sys.exit("the reference tree is not at " + REF)
    with tempfile.TemporaryDirectory(prefix="fast_ref_") as tmp:
        ref = Ref(build(tmp))
        assert ref.create_accepts_type(2) and not ref.create_accepts_type(0) and not ref.create_accepts_type(1)   # fast.cpp:213
        recs = {}
        for case in cases():
            recs.update(run_case(ref, case))
        recs.update(run_all_masks(ref))
        for name in sorted(recs):
            path = os.path.join(GOLDEN, f"fast_{name}.npz")
            save_npz(path, recs[name])
            print(path, os.path.getsize(path), "bytes")
            assert os.path.getsize(path) < 176 * 1024


if __name__ == "__main__":
    main()
