"""cv::cuda::BroxOpticalFlow on the GPU: every stage and the whole calc equal, in every bit of every pixel, the fixtures recorded from
the reference's own kernels (tests/golden/brox_ref*.npz) and, at shapes the fixtures do not hold, the NumPy restatement that is pinned
on them (tests/brox_numpy_ref.py, tests/test_brox_ref.py).  No tolerance, no pixel left out.  The tile of the blocked solver comes
from the plan's constants (opencv_contrib_amd/csrc/brox_plan.h)."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import brox_numpy_ref as R  # noqa: E402
from test_brox_plan import plan_constants  # noqa: E402
from test_brox_ref import CLASS_FILES, GOLDEN, class_params, resize_cases  # noqa: E402

pytestmark = pytest.mark.gpu
K = plan_constants()
TILE_X, TILE_Y, KMAX, HALO = K["BROX_SOR_TILE_X"], K["BROX_SOR_TILE_Y"], K["BROX_SOR_KMAX"], 2 * K["BROX_SOR_KMAX"]
PLAIN, BLOCKED = 1, 2
FORMS = pytest.mark.parametrize("form", [PLAIN, BLOCKED], ids=["plain", "blocked"])


def cuda():
    from opencv_contrib_amd import cuda as c
    return c


def dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def eq_bits(got, want, what=""):
    """equal in every bit: -0 is not +0 and a NaN is only itself"""
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {tuple(np.argwhere(bad)[0])}: {got[bad][0]!r} vs {want[bad][0]!r}"


def stage(name):
    return np.load(os.path.join(GOLDEN, f"brox_refstage_{name}.npz"))


# ------------------------------------------------------------------ derivative filter and the two resizes
@pytest.mark.parametrize("tag", ["4x4", "5x37", "13x16"])
def test_derivatives_equal_reference(gpu, tag):
    z = stage("filter")
    planes = cuda().brox_derivatives(dev(z["I0_" + tag], gpu), dev(z["I1_" + tag], gpu))
    for n, p in zip(R.DERIV_NAMES, planes):
        eq_bits(p, z[f"{n}_{tag}"], f"{n} {tag}")


def test_resizes_equal_reference(gpu):
    """supersample at 16 x 16 -> 13 x 13, a non-square odd size, 4 x 4, 5 x 37 and scale factors 0.5 / 0.95; prolongation at 4 x 4,
    5 x 37 and 13 x 16 -> 16 x 20"""
    c = cuda()
    cases = resize_cases(stage("resize"))
    assert {"down_16x16_sf0.8", "down_23x37_sf0.8", "up_13x16_to_16x20_sf0.8", "up_4x4_to_5x5_sf0.8"} <= {t[0] for t in cases}
    for tag, up, src, dst, sf in cases:
        got = (c.brox_resize_up if up else c.brox_resize_down)(dev(src, gpu), dst.shape[0], dst.shape[1], sf)
        eq_bits(got, dst, tag)


def test_resize_down_rejects_a_window_outside_the_source(gpu):
    from opencv_contrib_amd.capi import MiError
    with pytest.raises(MiError):
        cuda().brox_resize_down(dev(np.zeros((8, 8), np.float32), gpu), 8, 8, 0.5)


# ------------------------------------------------------------------ prepare (stage 1 + stage 2)
@pytest.mark.parametrize("case", ["generic", "centres", "boundaries", "outside", "gamma0"])
def test_prepare_equals_reference(gpu, case):
    """warped positions on texel centres, on the 1/512 boundaries of the weight, beyond one frame width outside on each side; gamma 0"""
    z = stage("prepare_" + case)
    if case == "gamma0":
        assert float(z["gamma"]) == 0.0
    images = [dev(z[n], gpu) for n in R.IMAGE_NAMES]
    co = cuda().brox_prepare(dev(z["u"], gpu), dev(z["v"], gpu), dev(z["du"], gpu), dev(z["dv"], gpu), images, float(z["alpha"]), float(z["gamma"]))
    for n, p in zip(R.COEFF_NAMES, co):
        eq_bits(p, z[("stage2_" if n.startswith("inv_") else "stage1_") + n], f"{n} {case}")


# ------------------------------------------------------------------ the solver, both forms
def run_sor(gpu, z, iterations, form):
    co = [dev(z[n], gpu) for n in R.COEFF_NAMES]
    return cuda().brox_sor(dev(z["u"], gpu), dev(z["v"], gpu), dev(z["du"], gpu), dev(z["dv"], gpu), co, iterations, form)


@FORMS
@pytest.mark.parametrize("iterations", [1, 2, 3, 5])
@pytest.mark.parametrize("shape", ["4x4", "7x33", "17x65"])
def test_sor_equals_reference(gpu, shape, iterations, form):
    """4 x 4 (smaller than the blocked form's halo), 7 x 33 (odd width: the colour of a row's first pixel alternates), one tile plus one
    pixel each way; 1, 3 and 5 iterations are no multiple of the blocked form's K"""
    assert (TILE_Y + 1, TILE_X + 1) == (17, 65) and KMAX == 2 and 4 <= HALO
    z = stage("sor_" + shape)
    du, dv = run_sor(gpu, z, iterations, form)
    eq_bits(du, z[f"du_it{iterations}"], "du")
    eq_bits(dv, z[f"dv_it{iterations}"], "dv")


@functools.lru_cache(maxsize=None)
def interior_tile_case():
    """three tiles each way: the middle tile has a halo on all four sides"""
    rows, cols = 2 * TILE_Y + 5, 2 * TILE_X + 9
    i0, i1 = R.synth_pair(rows, cols, 99)
    im = R.derivatives(i0, i1)
    im["I0"], im["I1"] = i0, i1
    rs = np.random.RandomState(5)
    u, v, du, dv = ((rs.rand(rows, cols) * 0.4 - 0.2).astype(np.float32) for _ in range(4))
    c = R.prepare(u, v, du, dv, im, 0.197, 50.0)
    z = dict(u=u, v=v, du=du, dv=dv, **c)
    z["du_it5"], z["dv_it5"] = R.sor(u, v, du, dv, c, 5)
    return z


@FORMS
def test_sor_with_interior_tiles_equals_restatement(gpu, form):
    z = interior_tile_case()
    du, dv = run_sor(gpu, z, 5, form)
    eq_bits(du, z["du_it5"], "du")
    eq_bits(dv, z["dv_it5"], "dv")


# ------------------------------------------------------------------ the whole calc
def calc(gpu, i0, i1, p, form=0, flow=None, stream=None):
    alg = cuda().BroxOpticalFlow.create(**p)
    alg.setSolverForm(form)
    return alg.calc(dev(i0, gpu), dev(i1, gpu), flow, stream)


@FORMS
@pytest.mark.parametrize("path", CLASS_FILES, ids=[os.path.basename(p)[len("brox_refclass_"):-4] for p in CLASS_FILES])
def test_calc_equals_reference(gpu, path, form):
    """4 x 4 (one level), 16 x 16 (two), 37 x 70 and 70 x 37 (six), the superres adapter's parameters at 48 x 64, scale factors 0.5 and
    0.95 with outer_iterations cutting the pyramid; in the plain and in the blocked form"""
    z = np.load(path)
    eq_bits(calc(gpu, z["I0"], z["I1"], class_params(z), form), z["flow"], "flow")


def test_default_form_is_the_plans_rule(gpu):
    z = np.load(os.path.join(GOLDEN, "brox_refclass_37x70.npz"))
    eq_bits(calc(gpu, z["I0"], z["I1"], class_params(z)), z["flow"], "flow")


def test_pitched_and_framed_matrices(gpu):
    """frames and flow as views inside larger allocations filled with NaN: the same bits, and nothing outside the flow is written"""
    import torch
    z = np.load(os.path.join(GOLDEN, "brox_refclass_37x70.npz"))
    rows, cols = z["I0"].shape
    big = [torch.full((rows + 5, cols + 9), float("nan"), device=gpu) for _ in range(2)]
    views = []
    for b, a in zip(big, (z["I0"], z["I1"])):
        b[2:2 + rows, 3:3 + cols] = dev(a, gpu)
        views.append(b[2:2 + rows, 3:3 + cols])
    out = torch.full((rows + 4, cols + 6, 2), float("nan"), device=gpu)
    alg = cuda().BroxOpticalFlow.create(**class_params(z))
    alg.calc(views[0], views[1], out[1:1 + rows, 2:2 + cols])
    eq_bits(out[1:1 + rows, 2:2 + cols].contiguous(), z["flow"], "flow")
    outside = torch.ones(out.shape, dtype=torch.bool, device=gpu)
    outside[1:1 + rows, 2:2 + cols] = False
    assert bool(torch.isnan(out[outside]).all())


def test_second_calc_with_another_size_and_back(gpu):
    """one handle, 70 x 37, then 16 x 16, then 70 x 37 again: each the bits of a fresh handle (the fixture's)"""
    a, b = (np.load(os.path.join(GOLDEN, f"brox_refclass_{n}.npz")) for n in ("70x37", "16x16"))
    alg = cuda().BroxOpticalFlow.create(**class_params(b))
    for z in (a, b, a):
        for k, val in class_params(z).items():
            if k.endswith("iterations"):
                getattr(alg, "set" + "".join(w.capitalize() for w in k.split("_")))(val)
        eq_bits(alg.calc(dev(z["I0"], gpu), dev(z["I1"], gpu)), z["flow"], "flow")
    assert alg.scratchBytes() > 0


def test_non_default_stream_and_a_flow_that_held_nan(gpu):
    import torch
    z = np.load(os.path.join(GOLDEN, "brox_refclass_16x16.npz"))
    i0, i1 = dev(z["I0"], gpu), dev(z["I1"], gpu)
    flow = torch.full((16, 16, 2), float("nan"), device=gpu)
    s = torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize()
    alg = cuda().BroxOpticalFlow.create(**class_params(z))
    alg.calc(i0, i1, flow, s.cuda_stream)
    s.synchronize()
    eq_bits(flow, z["flow"], "flow")


def test_forms_agree_on_a_frame_of_many_tiles(gpu):
    """150 x 200: levels of several tiles each way, plain against blocked"""
    i0, i1 = R.synth_pair(150, 200, 11)
    p = dict(R.DEFAULTS, inner_iterations=2, solver_iterations=5)
    a, b = calc(gpu, i0, i1, p, PLAIN), calc(gpu, i0, i1, p, BLOCKED)
    eq_bits(a, b.cpu().numpy(), "plain against blocked")
    assert np.isfinite(a.cpu().numpy()).all()


def test_output_is_finite_with_the_reference_nan_test_parameters(gpu):
    """BroxOpticalFlow.OpticalFlowNan (cudaoptflow/test/test_optflow.cpp:130-161): 0.197, 50, 0.8, 10, 77, 10; here at 320 x 240 on a synthetic pair"""
    from opencv_contrib_amd import synth
    i0, i1, _ = synth.flow_pair(240, 320, seed=7)
    flow = calc(gpu, i0, i1, dict(alpha=0.197, gamma=50.0, scale_factor=0.8, inner_iterations=10, outer_iterations=77, solver_iterations=10))
    assert flow.shape == (240, 320, 2) and bool(np.isfinite(flow.cpu().numpy()).all())


def test_a_pyramid_with_a_level_of_one_pixel_is_rejected_before_any_launch(gpu):
    from opencv_contrib_amd.capi import MiError
    z = dev(np.zeros((16, 16), np.float32), gpu)
    with pytest.raises(MiError) as e:
        cuda().BroxOpticalFlow.create(scale_factor=0.05).calc(z, z)
    assert e.value.code == -1


def test_a_side_of_three_is_rejected(gpu):
    from opencv_contrib_amd.capi import MiError
    alg = cuda().BroxOpticalFlow.create()
    for shape in ((3, 8), (8, 3)):
        with pytest.raises(MiError) as e:
            alg.calc(dev(np.zeros(shape, np.float32), gpu), dev(np.zeros(shape, np.float32), gpu))
        assert e.value.code == -1
