"""The yardstick of cv::cuda::FastFeatureDetector, checked without a GPU: the NumPy restatement (tests/fast_numpy_ref.py) reproduces what
the reference's own kernels and host class recorded (tests/golden/fast_ref*.npz); where the reference tree is present the fixtures are
rebuilt from it byte for byte; the run-of-nine test equals the reference's table for all 65 536 masks; the ABI; the C++ mirror."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fast_numpy_ref as R  # noqa: E402
import make_golden_fast as G  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CLASS_FILES = sorted(glob.glob(os.path.join(GOLDEN, "fast_refclass_*.npz")))
STAGE_FILES = sorted(p for p in glob.glob(os.path.join(GOLDEN, "fast_refstage_*.npz")) if "allmasks" not in p)
ALLMASKS = os.path.join(GOLDEN, "fast_refstage_allmasks_t10.npz")
LIBDIR = os.path.join(ROOT, "opencv_contrib_amd")
eq = np.testing.assert_array_equal
_ids = lambda files: [os.path.basename(p)[:-4] for p in files]


# ------------------------------------------------------------------ helpers shared with tests/test_fast_gpu.py
def row_major(loc, resp=None):
    """the reference's arbitrary order -> row-major (y, then x)"""
    o = np.lexsort((loc[:, 0], loc[:, 1]))
    return loc[o] if resp is None else (loc[o], resp[o])


def case_inputs(z):
    """(image, mask or None, threshold, max_npoints) of a fixture"""
    return z["img"], (z["mask"] if "mask" in z.files else None), int(z["threshold"]), int(z["max_npoints"])


def stage_of(class_path):
    """the stage fixture of a class fixture's inputs"""
    name = os.path.basename(class_path)[len("fast_refclass_"):-len("_nms.npz")]
    return np.load(os.path.join(GOLDEN, f"fast_refstage_{name}.npz"))


def check_against_class_fixture(z, zs, loc, resp):
    """(loc, resp): a row-major detection of the fixture's inputs.  Untruncated: equal to the reference's as sets.  Truncated: the
    reference kept the candidates whose atomics arrived first, so only the count (without suppression) and membership in the
    reference's untruncated result are held."""
    nms = bool(int(z["nonmax_suppression"]))
    rl, rr = R.unpack(z["keypoints"])
    count, maxn = int(z["count"]), int(z["max_npoints"])
    if count <= maxn:
        rl, rr = row_major(rl, rr)
        eq(loc, rl)
        eq(resp, rr)
        return
    full = {(int(x), int(y)): float(s) for (x, y), s in zip(zs["nms_loc"], zs["nms_resp"])} if nms else \
           {(int(x), int(y)): 0.0 for x, y in zs["kp_loc"]}
    if not nms:
        assert len(loc) == len(rl) == maxn
    assert len(loc) <= maxn
    for (x, y), s in zip(loc, resp):
        assert full.get((int(x), int(y))) == float(s), (x, y, s)
    eq(row_major(loc), loc)


def test_fixtures_cover_the_cases():
    names = {os.path.basename(p)[len("fast_refclass_"):-4] for p in CLASS_FILES}
    want = {f"noise{s}_t{t}" for s in ("23x71", "40x140") for t in (0, 10, 60)} | {"blocks", "masked", "flat", "corner7", "truncated"}
    assert names == {f"{n}_{m}" for n in want for m in ("nms", "raw")}
    assert {os.path.basename(p)[len("fast_refstage_"):-4] for p in STAGE_FILES} == want and os.path.exists(ALLMASKS)
    for p in CLASS_FILES + STAGE_FILES + [ALLMASKS]:
        assert os.path.getsize(p) < 176 * 1024, p
    # not vacuous (the tool asserts the same on a fresh build of the reference)
    z = np.load(os.path.join(GOLDEN, "fast_refstage_blocks.npz"))
    assert int(z["count"]) >= 100 and len(z["nms_loc"]) < int(z["count"]) and G.ties(z["score"], z["kp_loc"]) >= 100
    z = np.load(os.path.join(GOLDEN, "fast_refstage_noise23x71_t10.npz"))
    assert int(z["count"]) >= 50 and G.ties(z["score"], z["kp_loc"]) >= 1
    z = np.load(os.path.join(GOLDEN, "fast_refstage_truncated.npz"))
    assert int(z["count"]) > int(z["max_npoints"]) == len(z["cut_loc"])
    z = np.load(os.path.join(GOLDEN, "fast_refstage_masked.npz"))
    assert set(np.unique(z["mask"])) == {0, 1, 255}
    z = np.load(os.path.join(GOLDEN, "fast_refstage_flat.npz"))
    assert int(z["count"]) == 0
    z = np.load(os.path.join(GOLDEN, "fast_refstage_corner7.npz"))
    assert int(z["count"]) == 1 and z["img"].shape == (7, 7) and z["kp_loc"].tolist() == [[3, 3]]


@pytest.mark.parametrize("path", STAGE_FILES, ids=_ids(STAGE_FILES))
def test_restatement_reproduces_reference_kernels(path):
    z = np.load(path)
    img, mask, th, maxn = case_inputs(z)
    cand, score = R.score_plane(img, th, mask)
    eq(score, z["score"])   # calcKeypoints<true>'s plane over the cleared matrix
    assert int(cand.sum()) == int(z["count"])
    ys, xs = np.nonzero(cand)
    eq(np.stack([xs, ys], 1).reshape(-1, 2), row_major(z["kp_loc"]).reshape(-1, 2))
    assert (score[cand] >= th).all() and (score <= 254).all()
    loc, resp, count = R.detect(img, th, True, img.size, mask)   # nonmaxSuppression over every candidate
    rl, rr = row_major(z["nms_loc"], z["nms_resp"])
    eq(loc, rl)
    eq(resp, rr)
    assert R.tie_count(img, th, mask) == G.ties(z["score"], z["kp_loc"])


@pytest.mark.parametrize("path", CLASS_FILES, ids=_ids(CLASS_FILES))
def test_restatement_reproduces_reference_class(path):
    z = np.load(path)
    img, mask, th, maxn = case_inputs(z)
    nms = bool(int(z["nonmax_suppression"]))
    loc, resp, count = R.detect(img, th, nms, maxn, mask)
    assert count == int(z["count"])
    check_against_class_fixture(z, stage_of(path), loc, resp)
    # convert: FEATURE_SIZE, angle -1, the response (fast.cpp:205)
    conv = np.array(R.convert(z["keypoints"]), np.float32).reshape(-1, 5)
    eq(conv, z["converted"])
    if len(conv):
        assert (conv[:, 2] == 7).all() and (conv[:, 3] == -1).all()
        if not nms:
            assert not conv[:, 4].any()   # fast.cpp:171


def test_truncation_cuts_row_major_and_cut_candidates_still_suppress():
    z = np.load(os.path.join(GOLDEN, "fast_refstage_truncated.npz"))
    img, mask, th, maxn = case_inputs(z)
    all_loc, all_resp, count = R.detect(img, th, True, img.size)
    raw, _, _ = R.detect(img, th, False, maxn)
    eq(raw, row_major(z["kp_loc"])[:maxn])
    loc, resp, _ = R.detect(img, th, True, maxn)
    kept = {(int(x), int(y)) for x, y in raw}
    want = [(int(x), int(y)) for x, y in all_loc if (int(x), int(y)) in kept]
    assert [(int(x), int(y)) for x, y in loc] == want and 0 < len(want) < len(all_loc)


def test_run_of_nine_equals_the_reference_table_for_every_mask():
    """the reference's popc > 8 && c_table[...] (fast.cu:187-191), recorded at the 65 536 patch centres of both all-masks images, equals
    'a circular run of at least nine set bits'; so does the restatement's candidate map on those images"""
    z = np.load(ALLMASKS)
    run = np.packbits(R.run_of_nine(np.arange(65536)).astype(np.uint8), bitorder="little")
    assert int(R.run_of_nine(np.arange(65536)).sum()) == 1025
    for name, pol in (("bright", 1), ("dark", -1)):
        eq(z[name], run)
        cand, score = R.score_plane(R.all_masks_image(pol), 10)
        eq(R.centre_bitmap(cand), z[name])
        assert set(np.unique(score[cand])) == {10}   # ring pixels differ by 11: candidates at 10, not at 11
    # the doubling form the kernels use
    m = np.arange(65536, dtype=np.uint64)
    d = m | (m << np.uint64(16))
    a = d & (d >> np.uint64(1))
    b = a & (a >> np.uint64(2))
    c = b & (b >> np.uint64(4))
    eq(((c & (d >> np.uint64(8))) & np.uint64(0xFFFF)) != 0, R.run_of_nine(m))


def test_score_is_the_best_arc_minimum_minus_one():
    """the kernels' closed form of cornerScore: max over both polarities and the 16 arcs of nine of the arc's smallest difference, - 1"""
    img = R.synth_image(40, 140, 5, "noise")
    cand, score = R.score_plane(img, 0)
    ys, xs = np.nonzero(cand)
    d = R._ring_diffs(img, ys, xs)
    best = np.full(len(ys), -256)
    for sign in (1, -1):
        for k in range(16):
            best = np.maximum(best, np.min(sign * d[:, [(k + j) % 16 for j in range(9)]], 1))
    eq(best - 1, score[ys, xs])


def test_threshold_edges():
    img = R.synth_image(23, 71, 3, "noise")
    img[10, 10] = 0
    for dy, dx in R.RING:
        img[10 + dy, 10 + dx] = 255
    for th, n in ((254, 1), (255, 0), (300, 0)):
        assert R.detect(img, th, False)[2] == n, th
    assert R.score_plane(img, 254)[1][10, 10] == 254
    flat = R.synth_image(23, 71, 0, "flat")
    assert R.detect(flat, 0)[2] == 0   # equal pixels are no corner at threshold 0
    # threshold 0: a candidate of score 0 never survives (its non-candidate neighbours score 0 too)
    one = flat.copy().astype(np.int32)
    for dy, dx in R.RING[:9]:
        one[10 + dy, 30 + dx] += 1
    one = one.astype(np.uint8)
    cand, score = R.score_plane(one, 0)
    assert cand[10, 30] and score[10, 30] == 0
    loc, _, _ = R.detect(one, 0, True)
    assert (30, 10) not in {(int(x), int(y)) for x, y in loc}


# ------------------------------------------------------------------ against a fresh build of the reference
@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    if not G.have_reference():
        pytest.skip("the reference tree is not on this machine")
    return G.Ref(G.build(str(tmp_path_factory.mktemp("fast_ref"))))


def test_fixtures_equal_a_fresh_build_of_the_reference_byte_for_byte(ref, tmp_path):
    recs = {}
    for case in G.cases():
        recs.update(G.run_case(ref, case))
    recs.update(G.run_all_masks(ref))
    assert len(recs) == len(CLASS_FILES) + len(STAGE_FILES) + 1
    for name, rec in recs.items():
        p = str(tmp_path / f"fast_{name}.npz")
        G.save_npz(p, rec)
        assert open(p, "rb").read() == open(os.path.join(GOLDEN, f"fast_{name}.npz"), "rb").read(), name


def test_reference_accepts_type_9_16_only(ref):
    assert ref.create_accepts_type(R.TYPE_9_16) and not ref.create_accepts_type(0) and not ref.create_accepts_type(1)


# ------------------------------------------------------------------ the ABI
SYMBOLS = ["mi_fast_default_params", "mi_fast_create", "mi_fast_set_params", "mi_fast_get_params", "mi_fast_destroy", "mi_fast_scratch_bytes",
           "mi_fast_detect", "mi_fast_detect_batch", "mi_fast_score", "mi_fast_locations_to_points"]


def test_symbols_declared_exported_and_bound():
    from opencv_contrib_amd import capi
    declared = capi.declared_symbols()
    L = C.CDLL(capi.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared and hasattr(L, s), s
        assert getattr(capi.lib(), s).argtypes is not None, s
    assert sorted(s for s in declared if s.startswith("mi_fast_")) == sorted(SYMBOLS)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from opencv_contrib_amd import capi, cuda
    with pytest.raises(capi.MiError) as e:
        cuda.FastFeatureDetector.create()
    assert e.value.code == -7


def test_mirror_constants():
    from opencv_contrib_amd import cuda
    F = cuda.FastFeatureDetector
    assert (F.LOCATION_ROW, F.RESPONSE_ROW, F.ROWS_COUNT, F.FEATURE_SIZE, F.TYPE_9_16) == \
           (R.LOCATION_ROW, R.RESPONSE_ROW, R.ROWS_COUNT, R.FEATURE_SIZE, R.TYPE_9_16) == (0, 1, 2, 7, 2)


# ------------------------------------------------------------------ the C++ mirror
def build_shim(tmp_path):
    exe = str(tmp_path / "fast_shim")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "fast_shim.cpp"),
                        "-o", exe, "-L" + LIBDIR, "-lmiflow", "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_cpp_mirror_compiles_and_fails_loudly_without_gpu(tmp_path):
    """caller code against cudafeatures2d.hpp's FastFeatureDetector compiles next to xfeatures2d/cuda.hpp (one cv::KeyPoint); the type
    assert needs no device; creating the object without one throws"""
    import torch
    exe = build_shim(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 3 and "no CPU fallback" in r.stderr, (r.returncode, r.stderr)


def test_public_signatures_match_the_reference_header():
    """tests/cpp/fast_conformance.cpp: member-function pointer types, the factory's defaults and the constants, at compile time"""
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "fast_conformance.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
