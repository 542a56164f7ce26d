"""The yardstick of cv::cuda::StereoBeliefPropagation, checked without a GPU: the NumPy restatement (tests/stereobp_numpy_ref.py)
reproduces what the reference's own code recorded (tests/golden/stereobp_ref*.npz); where the reference tree is present the fixtures
are rebuilt from it; the two facts the class's internal layout rests on; the validator; the host plan; the ABI; the C++ mirror."""
import ctypes as C
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import stereobp_numpy_ref as R  # noqa: E402
import make_golden_stereobp as G  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CLASS_FILES = sorted(glob.glob(os.path.join(GOLDEN, "stereobp_refclass_*.npz")))
STAGE_FILES = sorted(glob.glob(os.path.join(GOLDEN, "stereobp_refstage_*.npz")))
MSG = {"f32": R.CV_32F, "s16": R.CV_16S}
LIBDIR = os.path.join(ROOT, "opencv_contrib_amd")
eq = np.testing.assert_array_equal
_ids = lambda files: [os.path.basename(p)[:-4] for p in files]


# ------------------------------------------------------------------ the restatement against the reference's recorded outputs
def test_fixtures_cover_the_cases():
    """both message types; 1, 3 and 4 channels; levels 1, 2, 3 and 4; odd sizes on both axes; non-default weights with a fractional
    single jump; compute(data); every file small"""
    assert len(CLASS_FILES) == len(G.CLASS_CASES) and len(STAGE_FILES) == len(G.STAGE_CASES)
    seen = set()
    for p in CLASS_FILES + STAGE_FILES:
        assert os.path.getsize(p) < 176 * 1024
    for p in CLASS_FILES:
        z = np.load(p)
        q = json.loads(str(z["params"]))
        cn = 0 if "data" in z.files else (1 if z["left"].ndim == 2 else z["left"].shape[2])
        rows, cols = z["disp"].shape
        seen |= {("msg", q["msg"]), ("cn", cn), ("levels", q["levels"]), ("msg_cn", q["msg"], cn > 0)}
        if rows % 2 and cols % 2:
            seen.add("odd")
        if q["weights"] != G.DEFAULT_W and q["weights"]["disc_single_jump"] % 1:
            seen.add("weights")
    want = {("msg", "f32"), ("msg", "s16"), ("cn", 0), ("cn", 1), ("cn", 3), ("cn", 4), ("levels", 1), ("levels", 2), ("levels", 3),
            ("levels", 4), "odd", "weights", ("msg_cn", "f32", False), ("msg_cn", "s16", False)}
    assert want <= seen, want - seen
    for p in STAGE_FILES:
        assert json.loads(str(np.load(p)["params"]))["ndisp"] <= 16


def _class_out(z):
    q = json.loads(str(z["params"]))
    args = (q["ndisp"], q["iters"], q["levels"], MSG[q["msg"]])
    if "data" in z.files:
        return R.compute_data(z["data"], *args, **q["weights"])
    return R.compute(z["left"], z["right"], *args, **q["weights"])


@pytest.mark.parametrize("path", CLASS_FILES, ids=_ids(CLASS_FILES))
def test_restatement_reproduces_reference_class(path):
    z = np.load(path)
    assert len(np.unique(z["disp"])) > 2
    eq(_class_out(z), z["disp"])


def _stage_outs(z):
    """every stage of the restatement from the fixture's recorded INPUT of that stage"""
    q = json.loads(str(z["params"]))
    nd, mt = q["ndisp"], MSG[q["msg"]]
    c = R.consts(nd, mt, **q["weights"])
    h, w = z["left"].shape[:2]
    data = R.unplanar(z["data"], nd)
    up = [R.unplanar(m, nd) for m in z["up"]]
    out = dict(data=R.planar(R.comp_data(z["left"], z["right"], c, mt)), data_down=R.planar(R.data_step_down(data)),
               up=np.stack([R.planar(R.level_up(R.unplanar(m, nd), h, w)) for m in z["coarse"]]))
    for n, key in ((1, "iter1"), (2, "iter2")):
        m = [u.copy() for u in up]
        R.calc_all_iterations(*m, data, n, c)
        out[key] = np.stack([R.planar(x) for x in m])
    out["disp"] = R.output(*[R.unplanar(m, nd) for m in z["iter2"]], data)
    return out


@pytest.mark.parametrize("path", STAGE_FILES, ids=_ids(STAGE_FILES))
def test_restatement_reproduces_reference_kernels(path):
    z = np.load(path)
    out = _stage_outs(z)
    for key, val in out.items():
        eq(val, z[key], err_msg=key)
    assert (z["iter1"] != z["up"]).any() and (z["iter2"] != z["iter1"]).any()     # both parities did update


# ------------------------------------------------------------------ the reference itself, where its tree is present
@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    if not G.have_reference():
        pytest.skip("the reference tree is not on this machine")
    return G.Ref(G.build(str(tmp_path_factory.mktemp("sbp_ref"))))


def test_tool_reproduces_the_committed_fixtures(ref):
    for kind, cases, run in (("refclass", G.CLASS_CASES, G.run_class_case), ("refstage", G.STAGE_CASES, G.run_stage_case)):
        for case in cases:
            z = np.load(os.path.join(GOLDEN, f"stereobp_{kind}_{case[0]}.npz"))
            rec = run(ref, case)
            assert sorted(rec) == sorted(z.files)
            for key in z.files:
                eq(rec[key], z[key], err_msg=f"{case[0]}:{key}")


def test_reference_output_types_and_estimate(ref):
    left, right = G.pair(12, 40, 1, 9)
    base = ref.compute(left, right, 30, 2, 1, R.CV_32F, {})
    for dt in (np.uint8, np.int32, np.float32):
        eq(ref.compute(left, right, 30, 2, 1, R.CV_32F, {}, out_dtype=dt), R.compute(left, right, 30, 2, 1, R.CV_32F, out_dtype=dt))
        eq(ref.compute(left, right, 30, 2, 1, R.CV_32F, {}, out_dtype=dt), base.astype(dt))
    for w, h in SIZES:
        assert ref.estimate(w, h) == R.estimate_recommended_params(w, h)


# ------------------------------------------------------------------ the two facts
@pytest.mark.parametrize("msg", ["f32", "s16"])
@pytest.mark.parametrize("h,w,levels", [(12, 16, 2), (13, 15, 2), (25, 27, 3), (24, 26, 3), (41, 33, 4)])
def test_fact_1_the_level0_data_border_reaches_no_disparity(msg, h, w, levels):
    """comp_data never writes the border of the level-0 data; data_step_down reads it, but only into border pixels of coarser levels,
    which neither one_iteration nor output reads: any fill gives the same map, for even and odd sizes"""
    left, right = G.pair(h, w, 1, h * w)
    kw = dict(ndisp=6, iters=2, levels=levels, msg_type=MSG[msg])
    base = R.compute(left, right, **kw)
    fills = (np.nan, np.inf, -1e30) if msg == "f32" else (32767, -32768, 12345)
    for fill in fills:
        eq(R.compute(left, right, border_fill=fill, **kw), base)


@pytest.mark.parametrize("msg", ["f32", "s16"])
@pytest.mark.parametrize("h,w,levels", [(9, 11, 1), (12, 16, 2), (13, 15, 2), (25, 27, 3), (41, 33, 4)])
def test_fact_2_every_message_element_read_was_written(msg, h, w, levels):
    """message buffers that start filled with NaN (f32) or a huge value (16-bit), of which only the coarsest level's planes are zeroed,
    give the map that all-zero buffers give: everything read comes from that zeroing, from level_up or from an iteration"""
    left, right = G.pair(h, w, 3, h + w)
    kw = dict(ndisp=5, iters=2, levels=levels, msg_type=MSG[msg])
    base = R.compute(left, right, **kw)
    eq(R.compute(left, right, msg_fill=np.nan if msg == "f32" else 31000, **kw), base)
    assert len(np.unique(base)) > 2


# ------------------------------------------------------------------ the validator
IMG = np.zeros((24, 32), np.uint8)
BAD = [   # what the asserts of stereobp.cpp:178-195 / :210-225 reject: (text, arguments of check_params)
    ("0 < ndisp_", dict(ndisp=0, iters=2, levels=2, msg_type=R.CV_32F, left=IMG, right=IMG)),
    ("0 < ndisp_", dict(ndisp=8, iters=0, levels=2, msg_type=R.CV_32F, left=IMG, right=IMG)),
    ("0 < ndisp_", dict(ndisp=8, iters=2, levels=0, msg_type=R.CV_32F, left=IMG, right=IMG)),
    ("msg_type_ == CV_32F", dict(ndisp=8, iters=2, levels=2, msg_type=0, left=IMG, right=IMG)),
    ("numeric_limits<short>::max()", dict(ndisp=8, iters=2, levels=3, msg_type=R.CV_16S, max_data_term=819.2, left=IMG, right=IMG)),   # 4 * 10 * 819.2 = 32768
    ("min_image_dim_size", dict(ndisp=8, iters=2, levels=5, msg_type=R.CV_32F, left=IMG, right=IMG)),                                 # 24 >> 4 = 1
    ("min_image_dim_size", dict(ndisp=8, iters=2, levels=1, msg_type=R.CV_32F, left=IMG[:2], right=IMG[:2])),
    ("left.size() == right.size()", dict(ndisp=8, iters=2, levels=2, msg_type=R.CV_32F, left=IMG, right=IMG[:, :31])),
    ("left.size() == right.size()", dict(ndisp=8, iters=2, levels=2, msg_type=R.CV_32F, left=IMG, right=np.zeros((24, 32, 3), np.uint8))),
    ("left.type() == CV_8UC1", dict(ndisp=8, iters=2, levels=2, msg_type=R.CV_32F, left=np.zeros((24, 32, 2), np.uint8), right=np.zeros((24, 32, 2), np.uint8))),
    ("data.rows % ndisp_ == 0", dict(ndisp=8, iters=2, levels=2, msg_type=R.CV_32F, data=np.zeros((8 * 24 + 1, 32), np.float32))),
    ("data.type() == msg_type_", dict(ndisp=8, iters=2, levels=2, msg_type=R.CV_32F, data=np.zeros((8 * 24, 32), np.int16))),
]
GOOD = [dict(ndisp=8, iters=2, levels=3, msg_type=R.CV_16S, max_data_term=819.0, left=IMG, right=IMG),     # 32760 < 32767
        dict(ndisp=8, iters=2, levels=3, msg_type=R.CV_32F, max_data_term=819.2, left=IMG, right=IMG),     # binds 16-bit messages only
        dict(ndisp=8, iters=2, levels=4, msg_type=R.CV_32F, left=IMG, right=IMG),                          # 24 >> 3 = 3 > 2
        dict(ndisp=8, iters=2, levels=2, msg_type=R.CV_16S, data=np.zeros((8 * 24, 32), np.int16))]


@pytest.mark.parametrize("text,kw", BAD, ids=[f"{i}-{t[:12]}" for i, (t, _) in enumerate(BAD)])
def test_check_params_rejects(text, kw):
    with pytest.raises(ValueError, match=text.replace("(", r"\(").replace(")", r"\)").replace("|", r"\|")):
        R.check_params(**kw)


def test_check_params_accepts():
    for kw in GOOD:
        R.check_params(**kw)


def _ref_throws(ref, kw):
    w = dict(max_data_term=kw.get("max_data_term", 10.0))
    if "data" in kw:
        return ref.compute_data(kw["data"], kw["ndisp"], kw["iters"], kw["levels"], kw["msg_type"], w) is None
    if kw["left"].ndim == 3 and kw["left"].shape[2] == 2:
        return True    # a 2-channel image: the entry points of the tool upload 1, 3 or 4 channels only
    return ref.compute(kw["left"], kw["right"], kw["ndisp"], kw["iters"], kw["levels"], kw["msg_type"], w) is None


def test_reference_throws_for_the_same_sets(ref):
    for text, kw in BAD:
        assert _ref_throws(ref, kw), text
    for kw in GOOD:
        assert not _ref_throws(ref, kw)


# ------------------------------------------------------------------ the host plan
def test_plan_host_arithmetic(tmp_path):
    """tests/cpp/sbp_plan_test.cpp: level sizes, buffer alternation, the zeroed set for odd and even levels, launch order, the form at
    every ndisp boundary of the register form, one rejected case per assert.  Plain C++ with its own main, built with the address and
    undefined-behaviour sanitizers (host code only; nothing here is loaded into Python)."""
    exe = str(tmp_path / "sbp_plan_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "opencv_contrib_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "sbp_plan_test.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "sbp_plan_test: ok" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------ the ABI
SYMBOLS = ["mi_stereobp_default_params", "mi_stereobp_create", "mi_stereobp_set_params", "mi_stereobp_get_params", "mi_stereobp_destroy",
           "mi_stereobp_compute", "mi_stereobp_compute_data", "mi_stereobp_estimate_recommended_params", "mi_stereobp_comp_data",
           "mi_stereobp_data_step_down", "mi_stereobp_level_up", "mi_stereobp_iterate", "mi_stereobp_output", "mi_stereobp_scratch_bytes"]
SIZES = [(w, h) for w in (1, 2, 3, 7, 8, 100, 320, 640, 1280, 1920, 4096) for h in (1, 2, 240, 480, 1080, 2161, 5000)]


def test_symbols_declared_exported_and_bound():
    from opencv_contrib_amd import capi
    declared = capi.declared_symbols()
    L = C.CDLL(capi.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared and hasattr(L, s), s
        assert getattr(capi.lib(), s).argtypes is not None, s


def test_defaults_equal_the_reference():
    """stereobp.cpp:147-158, cudastereo.hpp:189"""
    from opencv_contrib_amd import capi
    p = capi.StereoBPParams()
    capi.lib().mi_stereobp_default_params(C.byref(p))
    assert (p.ndisp, p.iters, p.levels, p.msg_type) == (64, 5, 5, R.CV_32F)
    f = np.float32
    assert (p.max_data_term, p.data_weight, p.max_disc_term, p.disc_single_jump) == (10.0, float(f(0.07)), float(f(1.7)), 1.0)


def test_estimate_recommended_params_equals_the_restatement():
    from opencv_contrib_amd import cuda
    for w, h in SIZES:
        assert cuda.StereoBeliefPropagation.estimateRecommendedParams(w, h) == R.estimate_recommended_params(w, h), (w, h)
    assert cuda.StereoBeliefPropagation.estimateRecommendedParams(640, 480) == (160, 8, 5)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from opencv_contrib_amd import capi, cuda
    with pytest.raises(capi.MiError) as e:
        cuda.createStereoBeliefPropagation()
    assert e.value.code == -7


# ------------------------------------------------------------------ the C++ mirror
def _build_shim(tmp_path):
    exe = str(tmp_path / "stereobp_shim")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "stereobp_shim.cpp"), "-o", exe, "-L" + LIBDIR, "-lmiflow",
                        "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_cpp_mirror_compiles_and_fails_loudly_without_gpu(tmp_path):
    """caller code against cudastereo.hpp's StereoBeliefPropagation compiles (signatures checked at compile time in the program);
    estimateRecommendedParams is host arithmetic; creating the object without a device throws"""
    import torch
    exe = _build_shim(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 3 and "no CPU fallback" in r.stderr, (r.returncode, r.stderr)


@pytest.mark.gpu
def test_cpp_mirror_matches_the_restatement(gpu, tmp_path):
    import struct
    exe = _build_shim(tmp_path)
    h, w = 20, 30
    left, right = G.pair(h, w, 1, 77)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("ii", h, w) + left.tobytes() + right.tobytes())
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = np.frombuffer(fout.read_bytes(), np.int16).reshape(2, h, w)
    wts = dict(max_data_term=12.0, data_weight=0.1, max_disc_term=2.0, disc_single_jump=0.75)
    eq(out[0], R.compute(left, right, 16, 3, 2, R.CV_16S, **wts))
    l, rr = left.astype(np.int64).ravel(), right.astype(np.int64).ravel()
    vol = np.stack([(l * (k + 1) + rr * (16 - k)) % 97 for k in range(16)]).astype(np.int16).reshape(16 * h, w)
    eq(out[1], R.compute_data(vol, 16, 3, 2, R.CV_16S, **wts))
