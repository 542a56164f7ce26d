"""The yardstick of cv::cuda::StereoConstantSpaceBP, checked without a GPU: the NumPy restatement (tests/stereocsbp_numpy_ref.py)
reproduces what the reference's own code recorded (tests/golden/stereocsbp_ref*.npz); where the reference tree is present the fixtures
are rebuilt from it and the validator and estimateRecommendedParams are held to the reference; the two facts the class's scratch rests
on; the host plan; the ABI; the C++ mirror."""
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
import stereocsbp_numpy_ref as R  # noqa: E402
import make_golden_stereocsbp as G  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CLASS_FILES = sorted(glob.glob(os.path.join(GOLDEN, "stereocsbp_refclass_*.npz")))
STAGE_FILES = sorted(glob.glob(os.path.join(GOLDEN, "stereocsbp_refstage_*.npz")))
MSG = {"f32": R.CV_32F, "s16": R.CV_16S}
LIBDIR = os.path.join(ROOT, "opencv_contrib_amd")
eq = np.testing.assert_array_equal
_ids = lambda files: [os.path.basename(p)[:-4] for p in files]


# ------------------------------------------------------------------ helpers shared with tests/test_stereocsbp_gpu.py
def class_inputs(z):
    """(left, right, keyword arguments of R.compute) of a class fixture"""
    q = json.loads(str(z["params"]))
    if "left" in z.files:
        left, right = z["left"], z["right"]
    else:
        left, right = R.synth_pair(*[int(v) for v in z["synth"]])
    kw = {k: q[k] for k in ("ndisp", "iters", "levels", "nr_plane", "max_data_term", "data_weight", "max_disc_term", "disc_single_jump",
                            "min_disp", "local")}
    kw["msg_type"] = MSG[q["msg"]]
    return left, right, kw


_class_cache = {}


def class_restated(path):
    """the restatement's (disparity, levels) of a class fixture, computed once per session"""
    if path not in _class_cache:
        left, right, kw = class_inputs(np.load(path))
        _class_cache[path] = R.compute(left, right, **kw)
    return _class_cache[path]


def init_stage_cases():
    """(key, level, cn, local, ndisp, min_disp) of the init_data_cost fixtures, as tools/make_golden_stereocsbp.py ran them"""
    for level in range(8):
        for cn in (1, 3, 4):
            for local in (True, False):
                for ndisp in G.INIT_NDISP:
                    if ndisp == 70 and level > 5:
                        continue
                    yield f"L{level}_c{cn}_{'local' if local else 'global'}_n{ndisp}", level, cn, local, ndisp, (1 if cn == 3 else 0)


def init_stage_images(level, cn):
    return R.synth_pair(3 << level, 3 << level, cn, 100 + level * 5 + cn)


def planar(vol):
    return np.ascontiguousarray(vol).reshape(-1, vol.shape[2])


# ------------------------------------------------------------------ the restatement against the reference's recorded outputs
def test_fixtures_cover_the_cases():
    assert len(CLASS_FILES) == 2 * len(G.CLASS_CASES) and len(STAGE_FILES) == 8
    for p in CLASS_FILES + STAGE_FILES:
        assert os.path.getsize(p) < 176 * 1024
    seen = set()
    for p in CLASS_FILES:
        z = np.load(p)
        q = json.loads(str(z["params"]))
        rows, cols = z["disp"].shape
        seen |= {("msg", q["msg"]), ("cn", int(z["synth"][2])), ("local", q["local"]), ("levels_after", int(z["levels_after"]))}
        if rows % 2 and cols % 2:
            seen.add("odd")
        if q["levels"] != int(z["levels_after"]):
            seen.add("clamped")
        if q["nr_plane"] << (int(z["levels_after"]) - 1) > q["ndisp"]:
            seen.add("fill")
        if q["max_disc_term"] % 1:
            seen.add("fractional disc term")
    want = {("msg", "f32"), ("msg", "s16"), ("cn", 1), ("cn", 3), ("cn", 4), ("local", True), ("local", False), ("levels_after", 1),
            ("levels_after", 2), ("levels_after", 3), ("levels_after", 8), "odd", "clamped", "fill", "fractional disc term"}
    assert want <= seen, want - seen


@pytest.mark.parametrize("path", CLASS_FILES, ids=_ids(CLASS_FILES))
def test_restatement_reproduces_reference_class(path):
    z = np.load(path)
    assert len(np.unique(z["disp"])) >= 2
    disp, levels = class_restated(path)
    assert levels == int(z["levels_after"])
    eq(disp, z["disp"])


@pytest.mark.parametrize("msg", ["f32", "s16"])
def test_restatement_reproduces_reference_init_data_cost(msg):
    """every level 0-7 (the plain form, every reduce width 4 .. 128), 1 / 3 / 4 channels, local and global selection, ndisp 5 and 70"""
    z = np.load(os.path.join(GOLDEN, f"stereocsbp_refstage_init_{msg}.npz"))
    n = 0
    for key, level, cn, local, ndisp, min_disp in init_stage_cases():
        left, right = init_stage_images(level, cn)
        cost, disp = R.init_data_cost(left, right, level, 4, ndisp, MSG[msg], local, min_disp=min_disp)
        eq(planar(cost), z[key + "_cost"], err_msg=key)
        eq(planar(disp), z[key + "_disp"], err_msg=key)
        n += 1
    assert 2 * n == len(z.files)


def restate_chain(z, msg, cn):
    """-> {key: array} for every output the chain fixture records, from the fixture's recorded input of that stage"""
    T = R.msg_dtype(MSG[msg])
    out = {}
    for level, rows, cols in G.DATA_COST_CASES:
        left, right = R.synth_pair(rows, cols, cn, 200 + level)
        h, w = rows >> level, cols >> level
        out[f"dc{level}_out"] = planar(R.compute_data_cost(left, right, level, z[f"dc{level}_parent"], h, w, h // 2, 6, T, min_disp=2))
    for n in G.INIT_MESSAGE_PLANES:
        h, w, n2 = 6, 8, 2 * n
        cur = dict(zip(("u", "d", "l", "r", "disp"), z[f"im{n}_cur"]))
        new = {k: np.zeros((n * h, w), T) for k in cur}
        sel = np.zeros((n * h, w), T)
        R.init_message(cur, new, z[f"im{n}_dc"], sel, h, w, n, h // 2, w // 2, n2)
        out[f"im{n}_new"] = np.stack([new[k] for k in ("u", "d", "l", "r", "disp")])
        out[f"im{n}_sel"] = sel
    return out


def restate_iterations(msgs, sel_disp, sel_cost, n, t0, n_iters, max_disc_term=25.0, disc_single_jump=1.5):
    h, w = sel_cost.shape[0] // n, sel_cost.shape[1]
    m = dict(zip("udlr", [a.copy() for a in msgs]))
    for t in range(t0, t0 + n_iters):
        R.iterate(m, sel_disp, sel_cost, h, w, n, t, max_disc_term, disc_single_jump)
    return np.stack([m[k] for k in "udlr"])


@pytest.mark.parametrize("msg,cn", [("f32", 1), ("f32", 3), ("s16", 1), ("s16", 3)])
def test_restatement_reproduces_reference_data_cost_and_init_message(msg, cn):
    z = np.load(os.path.join(GOLDEN, f"stereocsbp_refstage_chain_{msg}_c{cn}.npz"))
    out = restate_chain(z, msg, cn)
    assert len(out) == len(G.DATA_COST_CASES) + 2 * len(G.INIT_MESSAGE_PLANES)
    for k, v in out.items():
        eq(v, z[k], err_msg=k)
    # the fixtures hold what they are meant to: candidates below min_disp and beyond x, and tied summed costs
    assert (z["dc0_parent"] < 2).any() and (z["dc0_parent"] >= 12).any()


@pytest.mark.parametrize("msg", ["f32", "s16"])
def test_restatement_reproduces_reference_iterations_and_disp(msg):
    z = np.load(os.path.join(GOLDEN, f"stereocsbp_refstage_iter_{msg}.npz"))
    for h, w, n in G.ITER_CASES:
        key = f"it{h}x{w}_{n}"
        for iters in ((1, 3) if n <= 4 else (3,)):
            eq(restate_iterations(z[key + "_msgs"], z[key + "_disp"], z[key + "_cost"], n, 0, iters), z[f"{key}_out{iters}"], err_msg=key)
    key = "it9x11_4"
    m = dict(zip("udlr", z[key + "_out3"]))
    eq(R.compute_disp(m, z[key + "_disp"], z[key + "_cost"], 9, 11, 4), z["cd_disp"])
    assert len(np.unique(z["cd_disp"])) > 3
    tie = np.full_like(z[key + "_cost"], 7)
    zero = dict(zip("udlr", np.zeros_like(z[key + "_msgs"])))
    eq(R.compute_disp(zero, z[key + "_disp"], tie, 9, 11, 4), z["cd_tie_disp"])
    eq(z["cd_tie_disp"][1:-1, 1:-1], z[key + "_disp"][:9][1:-1, 1:-1].astype(np.int16))   # ties go to the first candidate
    assert not z["cd_tie_disp"][0].any() and not z["cd_tie_disp"][:, 0].any()              # the border is 0


# ------------------------------------------------------------------ against a fresh build of the reference
@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    if not G.have_reference():
        pytest.skip("the reference tree is not on this machine")
    return G.Ref(G.build(str(tmp_path_factory.mktemp("csbp_ref"))))


def test_fixtures_equal_a_fresh_build_of_the_reference(ref):
    jobs = []
    for msg in ("f32", "s16"):
        jobs += [(f"refclass_{c[0]}_{msg}", (lambda c=c, m=msg: G.run_class_case(ref, c, m))) for c in G.CLASS_CASES]
        jobs.append((f"refstage_init_{msg}", (lambda m=msg: G.run_stage_init(ref, m))))
        jobs += [(f"refstage_chain_{msg}_c{cn}", (lambda m=msg, c=cn: G.run_stage_chain(ref, m, c))) for cn in (1, 3)]
        jobs.append((f"refstage_iter_{msg}", (lambda m=msg: G.run_stage_iter(ref, m))))
    assert len(jobs) == len(CLASS_FILES) + len(STAGE_FILES)
    for name, run in jobs:
        rec, z = run(), np.load(os.path.join(GOLDEN, f"stereocsbp_{name}.npz"))
        assert sorted(rec) == sorted(z.files), name
        for k in rec:
            eq(np.asarray(rec[k]), z[k], err_msg=f"{name}:{k}")


# ------------------------------------------------------------------ the validator and estimateRecommendedParams
IMG = np.zeros((24, 32), np.uint8)
OK = dict(ndisp=16, iters=2, levels=2, nr_plane=2, msg_type=R.CV_32F, left=IMG, right=IMG)
BAD = [   # what the asserts of stereocsbp.cpp:154-161 reject, in their order: (text, arguments of check_params)
    ("msg_type_ == CV_32F", dict(OK, msg_type=0)),
    ("msg_type_ == CV_32F", dict(OK, msg_type=0, ndisp=0)),          # the message type is asserted first
    ("0 < ndisp_", dict(OK, ndisp=0)),
    ("0 < ndisp_", dict(OK, iters=0)),
    ("0 < ndisp_", dict(OK, levels=0)),
    ("0 < ndisp_", dict(OK, nr_plane=0)),
    ("levels_ <= 8", dict(OK, levels=9, ndisp=1024)),
    ("0 < ndisp_", dict(OK, ndisp=0, right=IMG[:, :31])),              # the counts before the images
    ("left.type() == CV_8UC1", dict(OK, left=np.zeros((24, 32, 2), np.uint8), right=np.zeros((24, 32, 2), np.uint8))),
    ("left.size() == right.size()", dict(OK, right=IMG[:, :31])),
    ("left.size() == right.size()", dict(OK, right=np.zeros((24, 32, 3), np.uint8))),
]
UNDEFINED = [   # accepted by the reference's asserts, undefined behind them, rejected here
    ("ndisp == 1", dict(OK, ndisp=1)),
    ("coarsest level is empty", dict(OK, ndisp=256, levels=6)),       # 24 >> 5 == 0
]
GOOD = [(dict(OK), 2), (dict(OK, msg_type=R.CV_16S, levels=8), 4), (dict(OK, ndisp=5, levels=4), 2), (dict(OK, ndisp=2, levels=3), 1),
        (dict(OK, ndisp=3, levels=3), 1), (dict(OK, ndisp=8, levels=8), 3), (dict(OK, ndisp=7, levels=3), 2), (dict(OK, ndisp=64, levels=5), 5),
        (dict(OK, ndisp=63, levels=8, left=np.zeros((40, 40, 3), np.uint8), right=np.zeros((40, 40, 3), np.uint8)), 5)]


@pytest.mark.parametrize("text,kw", BAD + UNDEFINED, ids=[f"{i}-{t[:12]}" for i, (t, _) in enumerate(BAD + UNDEFINED)])
def test_check_params_rejects(text, kw):
    with pytest.raises(ValueError, match=text.replace("(", r"\(").replace(")", r"\)").replace("|", r"\|")):
        R.check_params(**kw)


def test_check_params_accepts_and_clamps():
    for kw, levels in GOOD:
        assert R.check_params(**kw) == levels, kw
    for ndisp in list(range(2, 70)) + [127, 128, 129, 255, 256, 257, 1000, 4096]:
        assert R.clamp_levels(ndisp, 8) == min(8, ndisp.bit_length() - 1), ndisp   # int(log(n) / log(2.0)) is floor(log2 n) for these


def test_reference_throws_and_clamps_for_the_same_sets(ref):
    def run(kw):
        if kw["left"].ndim == 3 and kw["left"].shape[2] == 2:
            return None, None    # a 2-channel image: the entry points of the tool upload 1, 3 or 4 channels only
        cn = lambda a: 1 if a.ndim == 2 else a.shape[2]
        shape = lambda a: (a.shape[0], a.shape[1], cn(a))
        return ref.compute(shape(kw["left"]), shape(kw["right"]), kw["msg_type"], ndisp=kw["ndisp"], iters=kw["iters"], levels=kw["levels"],
                           nr_plane=kw["nr_plane"])
    for text, kw in BAD:
        assert run(kw)[0] is None, text
    for kw, levels in GOOD:
        disp, after = run(kw)
        assert disp is not None and after == levels, kw


SIZES = [(w, h) for w in (1, 2, 3, 7, 8, 100, 320, 640, 1280, 1920, 4096) for h in (1, 2, 240, 480, 1080, 2161, 5000)]


def test_estimate_recommended_params_equals_the_reference(ref):
    for w, h in SIZES:
        assert R.estimate_recommended_params(w, h) == ref.estimate(w, h), (w, h)


def test_estimate_recommended_params_equals_the_restatement():
    from opencv_contrib_amd import cuda
    for w, h in SIZES:
        assert cuda.StereoConstantSpaceBP.estimateRecommendedParams(w, h) == R.estimate_recommended_params(w, h), (w, h)
    assert cuda.StereoConstantSpaceBP.estimateRecommendedParams(640, 480) == (204, 10, 4, 6)


# ------------------------------------------------------------------ two facts the implementation relies on
FACT_CASE = dict(ndisp=16, iters=3, levels=3, nr_plane=2)


@pytest.mark.parametrize("msg", ["f32", "s16"])
def test_unwritten_scratch_reaches_no_output(msg):
    """The class zeroes data_cost and data_cost_selected (stereocsbp.cpp:235-236) and allocates temp_ unzeroed; the handle zeroes none of
    the three.  Every element of them that any kernel reads was written before by the same level.  (The two message / disparity sets are
    another matter: a level with odd sizes reads past its parent, so the handle zeroes them whole, as the class's buffers are here.)"""
    left, right = R.synth_pair(29, 37, 1, 5)
    a = R.compute(left, right, msg_type=MSG[msg], **FACT_CASE)[0]
    b = R.compute(left, right, msg_type=MSG[msg], scratch_fill=123, **FACT_CASE)[0]
    eq(a, b)
    assert len(np.unique(a)) > 2


@pytest.mark.parametrize("msg", ["f32", "s16"])
def test_border_messages_stay_as_initialised(msg):
    """compute_message updates interior pixels only (stereocsbp.cu:698): after a level's iterations the border rows and columns of its
    four messages are what the level started from (zeros at the coarsest level, init_message's copies below), while the interior moved"""
    left, right = R.synth_pair(29, 37, 1, 6)
    trace = {}
    R.compute(left, right, msg_type=MSG[msg], trace=trace, **FACT_CASE)
    for i in range(3):
        for k in "udlr":
            a, b = trace[(i, "init")][k], trace[i][k]
            for sl in ((slice(None), 0), (slice(None), -1), (slice(None), slice(None), 0), (slice(None), slice(None), -1)):
                eq(a[sl], b[sl])
            assert (a != b).any()
        eq(trace[(i, "init")]["disp"], trace[i]["disp"])
    assert not any(trace[(2, "init")][k].any() for k in "udlr")


# ------------------------------------------------------------------ the host plan
def test_plan_host_arithmetic(tmp_path):
    """tests/cpp/scsbp_plan_test.cpp: level sizes, planes, set alternation, the clamp, forms and capacities at their boundaries, scratch
    sizes, launch order, one rejected case per assert.  Plain C++ with its own main, built with the address and undefined-behaviour
    sanitizers (host code only; nothing here is loaded into Python)."""
    exe = str(tmp_path / "scsbp_plan_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "opencv_contrib_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "scsbp_plan_test.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "scsbp_plan_test: ok" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------ the ABI
SYMBOLS = ["mi_stereocsbp_default_params", "mi_stereocsbp_create", "mi_stereocsbp_set_params", "mi_stereocsbp_get_params", "mi_stereocsbp_destroy",
           "mi_stereocsbp_compute", "mi_stereocsbp_scratch_bytes", "mi_stereocsbp_estimate_recommended_params", "mi_stereocsbp_init_data_cost",
           "mi_stereocsbp_compute_data_cost", "mi_stereocsbp_init_message", "mi_stereocsbp_iterate", "mi_stereocsbp_compute_disp"]


def test_symbols_declared_exported_and_bound():
    from opencv_contrib_amd import capi
    declared = capi.declared_symbols()
    L = C.CDLL(capi.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared and hasattr(L, s), s
        assert getattr(capi.lib(), s).argtypes is not None, s
    assert sorted(s for s in declared if s.startswith("mi_stereocsbp_")) == sorted(SYMBOLS)


def test_defaults_equal_the_reference():
    """stereocsbp.cpp:132-143, cudastereo.hpp:241-242"""
    from opencv_contrib_amd import capi
    p = capi.StereoCSBPParams()
    capi.lib().mi_stereocsbp_default_params(C.byref(p))
    assert (p.ndisp, p.iters, p.levels, p.nr_plane, p.msg_type, p.min_disp_th, p.use_local_init_data_cost) == (128, 8, 4, 4, R.CV_32F, 0, 1)
    assert (p.max_data_term, p.data_weight, p.max_disc_term, p.disc_single_jump) == (30.0, 1.0, 160.0, 10.0)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from opencv_contrib_amd import capi, cuda
    with pytest.raises(capi.MiError) as e:
        cuda.createStereoConstantSpaceBP()
    assert e.value.code == -7


# ------------------------------------------------------------------ the C++ mirror
def _build_shim(tmp_path):
    exe = str(tmp_path / "stereocsbp_shim")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "stereocsbp_shim.cpp"), "-o", exe, "-L" + LIBDIR, "-lmiflow",
                        "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_cpp_mirror_compiles_and_fails_loudly_without_gpu(tmp_path):
    """caller code against cudastereo.hpp's StereoConstantSpaceBP compiles (signatures checked at compile time in the program);
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
    h, w = 21, 30
    left, right = R.synth_pair(h, w, 1, 77)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("ii", h, w) + left.tobytes() + right.tobytes())
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = np.frombuffer(fout.read_bytes(), np.int16)
    want, levels = R.compute(left, right, ndisp=12, iters=3, levels=5, nr_plane=3, msg_type=R.CV_16S, min_disp=1, local=False, max_data_term=25.0,
                             data_weight=0.8, max_disc_term=90.5, disc_single_jump=7.5)
    assert out[-1] == levels == 3
    eq(out[:-1].reshape(h, w), want)
