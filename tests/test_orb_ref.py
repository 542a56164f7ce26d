"""The NumPy restatement of cv::cuda::ORB (tests/orb_numpy_ref.py) against what the reference's own kernels recorded
(tests/golden/orb_ref*.npz, tools/make_golden_orb.py: orb.cu, fast.cu, the resize_linear kernel and the 8-bit row and column filters run on
the host, and the host arithmetic of orb.cpp run from slices of its text).  No GPU.  orb.cpp as a whole does not compile against the stub
core (the recorder's docstring lists what is missing), so there are no class fixtures: the orchestration is restated.

Integer and f32 stages -- Harris responses, the cull's kept set and order (fixtures without a tie at the cut), merged coordinates -- bit
for bit.  The angle within the largest distance measured while recording plus one ulp (the restatement rounds a double atan2 once, the
fixture holds glibc's atan2f).  Descriptors on the fixture's own (loc, angle), so that only sincosf differs: equal in every bit that is
not tie-sensitive, and the tie-sensitive share is at most 0.5 %."""
import glob
import os

import numpy as np
import pytest

import orb_numpy_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STAGE_FILES = sorted(glob.glob(os.path.join(GOLDEN, "orb_refstage_p*_wta*.npz")))
eq = np.testing.assert_array_equal


POOL31 = np.load(os.path.join(GOLDEN, "orb_pattern31.npz"))["pattern0"]   # the learned pool: loaded by tests only
HOST = dict(np.load(os.path.join(GOLDEN, "orb_refhost.npz")))


def _ids(paths):
    return [os.path.basename(p)[len("orb_refstage_"):-4] for p in paths]


def test_the_fixtures_are_there():
    assert _ids(STAGE_FILES) == ["p29_wta2", "p31_wta2", "p31_wta3", "p9_wta4"]
    for n in ("orb_pattern31", "orb_refhost", "orb_refstage_pyramid", "orb_refstage_cullfast", "orb_refstage_ties"):
        assert os.path.exists(os.path.join(GOLDEN, n + ".npz")), n


def ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.fixture(scope="module", params=STAGE_FILES, ids=_ids(STAGE_FILES))
def z(request):
    return dict(np.load(request.param))


def test_inputs_are_the_reference_host_tables(z):
    """u_max and the pattern of a stage fixture come from the slices of orb.cpp (patch 31: the learned pool); the restatement gives the
    same, and the keypoints keep clear of the border"""
    patch, wta = int(z["patch_size"]), int(z["wta_k"])
    assert z["u_max"].tolist() == R.u_max(patch)
    eq(z["pattern"], R.make_pattern(patch, wta, POOL31 if patch == 31 else None))
    n = len(z["loc"])
    assert n >= 64 and n % 8 == 0
    r = max(R.pattern_reach(z["pattern"]), patch // 2, 4)
    rows, cols = z["img"].shape
    assert (z["loc"][:, 0] >= r).all() and (z["loc"][:, 0] < cols - r).all() and (z["loc"][:, 1] >= r).all() and (z["loc"][:, 1] < rows - r).all()


def test_harris_equals_reference_kernel(z):
    got = R.harris(z["img"], z["loc"])
    eq(got.view(np.uint32), z["harris"].view(np.uint32))
    assert len(np.unique(z["harris"])) > len(z["harris"]) // 2


def test_cull_equals_reference_sort(z):
    """the fixture's cut has no tie across it, asserted here on the reference's output; inside the kept set equal responses keep their
    order in both (std::stable_sort in the recording glue)"""
    n = int(z["cull_n"])
    order = np.sort(z["harris"])[::-1]
    assert order[n - 1] > order[n] and len(z["cull_resp"]) == n
    loc, resp = R.cull(z["loc"], z["harris"], n)
    eq(loc, z["cull_loc"])
    eq(resp.view(np.uint32), z["cull_resp"].view(np.uint32))


def test_angle_within_the_measured_tolerance(z):
    """max over the fixture of |restatement - glibc atan2f path| in ulps, as measured at recording time, plus one; above 4 the restatement
    would be wrong, not the tolerance.  Measured: 2, 2, 2, 1 ulp (p29_wta2, p31_wta2, p31_wta3, p9_wta4)."""
    m01, m10 = R.moments(z["img"], z["loc"], int(z["patch_size"]))
    d = ulps(R.angle_from_moments(m01, m10), z["angle"])
    print("angle: max", int(d.max()), "ulp; recorded", int(z["angle_max_ulp"]))
    assert int(z["angle_max_ulp"]) <= 4
    assert d.max() <= int(z["angle_max_ulp"]) + 1
    assert (z["angle"] >= 0).all() and (z["angle"] < 360.001).all() and np.ptp(z["angle"]) > 180


def test_descriptors_equal_outside_tie_sensitive_bits(z):
    patch, wta = int(z["patch_size"]), int(z["wta_k"])
    got = R.descriptors(z["img"], z["loc"], z["angle"], z["pattern"], wta)
    tie = R.tie_sensitive_bits(z["loc"], z["angle"], z["pattern"], wta)
    share = float(tie.mean())
    print("tie-sensitive share", share, "recorded", float(z["tie_sensitive_share"]))
    assert share <= 0.005 and share == float(z["tie_sensitive_share"])
    diff = np.unpackbits(got ^ z["descriptors"], axis=1, bitorder="little").reshape(len(got), 32, 8).astype(bool)
    assert not (diff & ~tie).any()
    assert len(np.unique(z["descriptors"], axis=0)) > len(got) // 2


def test_blur_equals_reference_filter_kernels(z):
    """linearRow<uchar, float> then linearColumn<float, uchar>: the 8-bit saturating store included"""
    eq(R.blur(z["img"]), z["blur"])
    assert (z["blur"] != z["img"]).mean() > 0.5


def test_merged_coordinates_equal_reference_kernel(z):
    s = z["merge_scale"]
    eq((z["loc"][:, 0].astype(np.float32) * s).view(np.uint32), z["merge_x"].view(np.uint32))
    eq((z["loc"][:, 1].astype(np.float32) * s).view(np.uint32), z["merge_y"].view(np.uint32))


# ------------------------------------------------------------------ the host arithmetic of orb.cpp, run from its own text
def test_quotas_equal_reference_constructor():
    n = 0
    while f"quota_{n}" in HOST:
        nf, sf, L = HOST[f"quota_{n}_args"]
        assert R.features_per_level(int(nf), float(sf), int(L)) == HOST[f"quota_{n}"].tolist(), (nf, sf, L)
        n += 1
    assert n == 6 and HOST["quota_0"].tolist()[0] == 109 and HOST["quota_4"].tolist() == [1, 0]


@pytest.mark.parametrize("patch", [2, 3, 9, 29, 31, 59])
def test_u_max_equals_reference_constructor(patch):
    assert R.u_max(patch) == HOST[f"u_max_{patch}"].tolist()


def test_scales_and_level_sizes_equal_reference():
    for first in (0, 1):
        got = np.array([R.get_scale(1.2, first, l) for l in range(8)], np.float32)
        eq(got.view(np.uint32), HOST[f"scales_1.2_first{first}"].view(np.uint32))
    for key in ("sizes_480x640_first0", "sizes_97x131_first1", "sizes_1080x1920_first0", "sizes_75x131_first0"):
        rows, cols = (int(v) for v in key.split("_")[1].split("x"))
        first = int(key[-1])
        g = R.level_geometry(rows, cols, dict(R.DEFAULTS, firstLevel=first))
        assert [[v["rows"], v["cols"]] for v in g] == HOST[key].tolist(), key
    assert HOST["sizes_75x131_first0"][1].tolist() == [62, 109]   # cvRound(62.5) = 62: the empty inner rectangle of the plan test


@pytest.mark.parametrize("wta", [2, 3, 4])
def test_pattern31_equals_the_uploaded_matrices(wta):
    """initializeOrbPattern / the WTA_K 2 copy on the learned pool against the matrix the reference's constructor uploads.  For WTA_K 3 and
    4 the draw order comes from cv::RNG, which the recording glue supplies: a wrong restatement of the generator would show as a
    mismatch only if the two restatements differed, so the RNG itself stays unpinned."""
    assert POOL31.shape == (512, 2)
    eq(R.make_pattern(31, wta, POOL31), HOST[f"pattern_p31_wta{wta}"])
    if wta == 2:
        eq(HOST["pattern_p31_wta2"], POOL31.T)


@pytest.mark.parametrize("key", ["pattern_p29_wta2", "pattern_p29_wta3", "pattern_p9_wta4"])
def test_random_patterns_equal_the_uploaded_matrices(key):
    patch, wta = int(key.split("_")[1][1:]), int(key[-1])
    eq(R.make_pattern(patch, wta), HOST[key])


# ------------------------------------------------------------------ pyramid, mask, FAST inside ORB
PYR = dict(np.load(os.path.join(GOLDEN, "orb_refstage_pyramid.npz")))


def test_pyramid_and_masks_equal_reference_resize_kernel():
    first, edge, nlevels, th = (int(v) for v in PYR["params"])
    p = dict(R.DEFAULTS, firstLevel=first, nlevels=nlevels, scaleFactor=float(PYR["scale_factor"]))
    imgs, masks = [], []
    for l, g in enumerate(R.level_geometry(*PYR["img"].shape, p)):
        src = PYR["img"] if g["src"] < 0 else imgs[g["src"]]
        msrc = PYR["mask"] if g["src"] < 0 else masks[g["src"]]
        li, lm = R.pyramid_level(src, g["rows"], g["cols"], msrc, g["mask_mode"], edge)
        eq(li, PYR[f"img_{l}"])
        eq(lm, PYR[f"mask_{l}"])
        imgs.append(li)
        masks.append(lm)
    assert PYR["img_0"].shape > PYR["img_1"].shape > PYR["img_2"].shape and PYR["mask_2"].any() and (PYR["mask_2"] == 0).any()


def test_fast_on_every_level_equals_reference_kernels():
    import fast_numpy_ref as FR
    th = int(PYR["params"][3])
    with_kp = 0
    for l in range(int(PYR["params"][2])):
        img, mask = PYR[f"img_{l}"], PYR[f"mask_{l}"]
        cap = int(0.05 * img.size)
        loc, resp, count = FR.detect(img, th, True, cap, mask)
        assert count == int(PYR[f"fast_count_{l}"]) <= cap
        eq(loc, PYR[f"fast_loc_{l}"])
        eq(resp, PYR[f"fast_resp_{l}"])
        with_kp += len(loc) > 0
    assert with_kp >= 2


# ------------------------------------------------------------------ the culls on FAST scores
def test_cull_on_fast_scores_equals_reference_sort():
    z = np.load(os.path.join(GOLDEN, "orb_refstage_cullfast.npz"))
    n = int(z["cull_n"])
    order = np.sort(z["resp"])[::-1]
    assert order[n - 1] > order[n] and len(np.unique(order[:n])) < n   # ties inside the kept set, none across the cut
    loc, resp = R.cull(z["loc"], z["resp"], n)
    eq(loc, z["cull_loc"])
    eq(resp.view(np.uint32), z["cull_resp"].view(np.uint32))


def test_ties_at_the_cut_keep_the_reference_multiset():
    """the `blocks` image: the cut falls inside a run of equal FAST scores, so which of them the reference keeps is its sort's business;
    the kept RESPONSES are the same multiset, and ours are the first of the run in row-major order"""
    z = np.load(os.path.join(GOLDEN, "orb_refstage_ties.npz"))
    n = int(z["cull_n"])
    order = np.sort(z["resp"])[::-1]
    assert order[n - 1] == order[n]
    loc, resp = R.cull(z["loc"], z["resp"], n)
    eq(np.sort(resp), np.sort(z["cull_resp"]))
    run = np.nonzero(z["resp"] == order[n - 1])[0]
    kept_of_run = int((resp == order[n - 1]).sum())
    eq(loc[resp == order[n - 1]], z["loc"][run[:kept_of_run]])


def test_tie_sensitive_exclusion_on_provided_keypoints_at_30_degrees():
    """provided keypoints at angle 30 on a fixture's image, described by the reference's kernel at recording time is not available for
    this angle; what is checked here: the mask marks bits at 30 degrees (sin next to 1/2 puts sample points next to half-integers), marks
    none at 0, and a descriptor computed with sina / cosa moved by one ulp differs from the restatement's ONLY inside the mask"""
    z = dict(np.load(STAGE_FILES[1]))
    loc = z["loc"][:64]
    pat = z["pattern"]
    wta = int(z["wta_k"])
    a30 = np.full(len(loc), 30.0, np.float32)
    tie = R.tie_sensitive_bits(loc, a30, pat, wta)
    assert tie.any() and not R.tie_sensitive_bits(loc, np.zeros(len(loc), np.float32), pat, wta).any()
    base = R.descriptors(z["img"], loc, a30, pat, wta)
    sina, cosa = R.sincos(a30)
    seen = 0
    for s in (np.nextafter(sina, np.float32(-2)), np.nextafter(sina, np.float32(2))):
        for c in (np.nextafter(cosa, np.float32(-2)), np.nextafter(cosa, np.float32(2))):
            d = R.descriptors_from(z["img"], loc, s.astype(np.float32), c.astype(np.float32), pat, wta)
            diff = np.unpackbits(d ^ base, axis=1, bitorder="little").reshape(len(loc), 32, 8).astype(bool)
            assert not (diff & ~tie).any()
            seen += int(diff.sum())
    assert seen > 0, "one ulp of sina / cosa changed no bit: the exclusion rule is not exercised"
