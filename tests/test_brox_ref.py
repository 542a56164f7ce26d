"""The NumPy restatement of cv::cuda::BroxOpticalFlow (tests/brox_numpy_ref.py) against what the reference's own kernels and host
function computed (tests/golden/brox_ref*.npz, recorded by tools/make_golden_brox.py): every bit of every pixel.  CPU only."""
import glob
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import brox_numpy_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
STAGE_FILES = sorted(glob.glob(os.path.join(GOLDEN, "brox_refstage_*.npz")))
CLASS_FILES = sorted(glob.glob(os.path.join(GOLDEN, "brox_refclass_*.npz")))
f32 = np.float32


def _ids(paths):
    return [os.path.basename(p)[len("brox_"):-4] for p in paths]


def eq_bits(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype == f32, (what, a.shape, b.shape, a.dtype, b.dtype)
    bad = a.view(np.uint32) != b.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {tuple(np.argwhere(bad)[0])}: {a[bad][0]!r} vs {b[bad][0]!r}"


def class_params(z):
    a, g, s = (float(x) for x in z["fparams"])
    i, o, n = (int(x) for x in z["iparams"])
    return dict(alpha=a, gamma=g, scale_factor=s, inner_iterations=i, outer_iterations=o, solver_iterations=n)


def resize_cases(z):
    """-> [(tag, up, src, dst, scale_factor)] of the resize fixture"""
    out = []
    for k in z.files:
        if k.startswith("src_"):
            tag = k[4:]
            out.append((tag, tag.startswith("up_"), z[k], z["dst_" + tag], float(tag.rsplit("_sf", 1)[1])))
    return sorted(out, key=lambda c: c[0])


def test_fixtures_are_all_here():
    assert len(STAGE_FILES) == 10 and len(CLASS_FILES) == 8
    assert max(os.path.getsize(p) for p in STAGE_FILES + CLASS_FILES) < 96 * 1024


def test_restatement_equals_reference_filter():
    z = np.load(os.path.join(GOLDEN, "brox_refstage_filter.npz"))
    tags = sorted({k.split("_", 1)[1] for k in z.files})
    assert tags == ["13x16", "4x4", "5x37"]
    for tag in tags:
        d = R.derivatives(z["I0_" + tag], z["I1_" + tag])
        for n in R.DERIV_NAMES:
            eq_bits(d[n], z[f"{n}_{tag}"], f"{n} {tag}")


def test_the_filter_mirror_is_the_asymmetric_one():
    """-1 -> 2 and -2 -> 3 (NPP_staging.cu:1435): on a ramp the first column's derivative differs from the symmetric mirror's"""
    ramp = np.tile(np.arange(6, dtype=f32) ** 2, (4, 1))
    d = R.derivative(ramp, False)
    want0 = (ramp[0, 3] * 1 + ramp[0, 2] * -8 + 0 + ramp[0, 1] * 8 + ramp[0, 2] * -1) / 12
    assert d[0, 0] == f32(want0)


def test_restatement_equals_reference_resize():
    z = np.load(os.path.join(GOLDEN, "brox_refstage_resize.npz"))
    cases = resize_cases(z)
    assert sum(1 for c in cases if c[1]) == 4 and sum(1 for c in cases if not c[1]) == 6
    for tag, up, src, dst, sf in cases:
        got = (R.resize_up if up else R.resize_down)(src, dst.shape[1], dst.shape[0], sf)
        eq_bits(got, dst, tag)


@pytest.mark.parametrize("path", [p for p in STAGE_FILES if "_prepare_" in p], ids=lambda p: os.path.basename(p)[len("brox_refstage_"):-4])
def test_restatement_equals_reference_prepare(path):
    z = np.load(path)
    im = {n: z[n] for n in R.IMAGE_NAMES}
    s1 = R.prepare_stage1(z["u"], z["v"], z["du"], z["dv"], im, float(z["alpha"]), float(z["gamma"]))
    for n, a in s1.items():
        eq_bits(a, z["stage1_" + n], n)
    s2 = R.prepare_stage2({n: z["stage1_" + n] for n in s1})
    for n in ("inv_denominator_u", "inv_denominator_v"):
        eq_bits(s2[n], z["stage2_" + n], n)


@pytest.mark.parametrize("path", [p for p in STAGE_FILES if "_sor_" in p], ids=lambda p: os.path.basename(p)[len("brox_refstage_"):-4])
def test_restatement_equals_reference_sor(path):
    z = np.load(path)
    c = {n: z[n] for n in R.COEFF_NAMES}
    its = sorted(int(k[5:]) for k in z.files if k.startswith("du_it"))
    assert its == [1, 2, 3, 5]
    for it in its:
        du, dv = R.sor(z["u"], z["v"], z["du"], z["dv"], c, it)
        eq_bits(du, z[f"du_it{it}"], f"du after {it}")
        eq_bits(dv, z[f"dv_it{it}"], f"dv after {it}")


@pytest.mark.parametrize("path", CLASS_FILES, ids=_ids(CLASS_FILES))
def test_restatement_equals_reference_class(path):
    z = np.load(path)
    p = class_params(z)
    flow, sizes = R.calc(z["I0"], z["I1"], **p)
    assert [tuple(s) for s in sizes] == [tuple(int(x) for x in s) for s in z["levels"]]
    eq_bits(flow, z["flow"], "flow")


def test_a_level_with_a_side_of_one_is_refused_and_three_is_not():
    """16 x 16 at scale_factor 0.05 would get a 1 x 1 level, where the filter's mirror maps -2 -> 3 -> -2 (NumPy would wrap round silently):
    refused, as the plan refuses it; at 0.15 the level is 3 x 3 and the reference's own run is the fixture sf0.15_16x16"""
    assert R.level_sizes(16, 16, 0.05, 150) == [(16, 16), (1, 1)] and R.level_sizes(16, 16, 0.15, 150) == [(16, 16), (3, 3)]
    z = np.zeros((16, 16), f32)
    with pytest.raises(ValueError):
        R.calc(z, z, scale_factor=0.05)


def test_recording_again_gives_the_same_bytes(tmp_path):
    """tools/make_golden_brox.py on the reference tree: skipped where the tree is absent"""
    import subprocess
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden_brox as M
    if not M.have_reference():
        pytest.skip("the reference tree is not on this machine")
    env = dict(os.environ, BROX_GOLDEN_DIR=str(tmp_path))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_brox.py")], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for p in STAGE_FILES + CLASS_FILES:
        assert open(p, "rb").read() == open(os.path.join(str(tmp_path), os.path.basename(p)), "rb").read(), p
