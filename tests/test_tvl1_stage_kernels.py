"""Stage-level tests of the TV-L1 iteration kernels in the forms calc() runs them (mi_tvl1_iterate_stage).

mi_tvl1_iterate reaches close relatives of the product's kernels (always a stored |grad|^2 plane, no illumination channel, no speculative
steps).  Here every form goes through the same inputs:
  a. NG: the default blocked kernel forming |grad|^2 itself == the same kernel reading the plane == independent waves, bit for bit;
  b. gamma != 0, exact math, one launch per iteration: nine planes against the oracle, error sums against the oracle's;
  c. gamma != 0, fast blocked: every decomposition into blocks of 10 / 5 (joined waves) and 2 / 1 (independent waves) and the register
     tiles bit-identical, and close to (b) on all nine planes;
  d. p_zero: the first pass's p = 0 kernels == explicit zero planes (the hook fills the unread p planes with NaN);
  e. the speculative steps (MODE 1): planes == fixed work, and every iteration's integer error sum == oracle.tvl1_err_fix of the
     fixed-work planes, exactly -- saturated terms included.
Shapes: one to four active waves of a joined group, strip seams (246 | 247, 482 | 483 columns), ragged last groups, several bands; forced
band heights of 8, 13 and 37 rows; batches of 3 pairs, each pair equal to its single run.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L_T, THETA, TAUT = float(np.float32(0.15 * 0.3)), float(np.float32(0.3)), float(np.float32(0.25 / 0.3))
GAMMA = 0.5
SHAPES = [(37, 64), (70, 65), (16, 192), (135, 246), (53, 247), (40, 482), (97, 483), (30, 1000), (24, 1920)]
U_NAMES, P_NAMES = ["u1", "u2", "u3"], ["p11", "p12", "p21", "p22", "p31", "p32"]


def _pair(h, w, seed, gam=False, spikes=False):
    """One pair's planes: I1wx, I1wy with 5 % textureless pixels, grad = f32(ix*ix) + f32(iy*iy) (the warp's own expression), rho_c,
    u, p.  spikes: a few large p11 values (strip seams included), so that u moves by more than 16 px there in the first iterations."""
    rng = np.random.default_rng(seed)
    f = lambda s: (rng.standard_normal((h, w)) * s).astype(np.float32)
    ix, iy = f(8), f(8)
    flat = rng.random((h, w)) < 0.05
    ix[flat] = 0
    iy[flat] = 0
    grad = (ix * ix) + (iy * iy)
    rho = f(5)
    u = [f(1), f(1)] + ([f(1)] if gam else [])
    p = [f(0.3) for _ in range(6 if gam else 4)]
    if spikes:
        ys = rng.integers(0, h, 6)
        xs = np.concatenate([rng.integers(0, w, 3), np.clip([63, 245, 246], 0, w - 1)])
        p[0][ys, xs] = np.float32(200.0) * np.sign(rng.standard_normal(6)).astype(np.float32)
    return dict(ix=ix, iy=iy, grad=grad, rho=rho, u=u, p=p)


def _branch_fractions(x, gam):
    """Fractions of the pixels in the three branches of the threshold test (rho < -l_t g, rho > l_t g, in between) for the inputs."""
    rho = x["rho"].astype(np.float64) + x["ix"] * x["u"][0].astype(np.float64) + x["iy"] * x["u"][1].astype(np.float64)
    if gam:
        rho = rho + GAMMA * x["u"][2].astype(np.float64)
    ltg = L_T * x["grad"].astype(np.float64)
    lo, hi = rho < -ltg, rho > ltg
    return lo.mean(), hi.mean(), (~lo & ~hi).mean()


def _inputs(h, w, seed, gam=False, B=1, spikes=False):
    pairs = [_pair(h, w, seed + 101 * b, gam, spikes) for b in range(B)]
    for x in pairs:
        assert min(_branch_fractions(x, gam)) >= 0.10, _branch_fractions(x, gam)
        assert (x["grad"] == 0).mean() >= 0.02   # textureless pixels: the grad <= eps branch
    if B == 1:
        return pairs[0]
    st = lambda k: np.stack([x[k] for x in pairs])
    return dict(ix=st("ix"), iy=st("iy"), grad=st("grad"), rho=st("rho"),
                u=[np.stack([x["u"][i] for x in pairs]) for i in range(len(pairs[0]["u"]))],
                p=[np.stack([x["p"][i] for x in pairs]) for i in range(len(pairs[0]["p"]))])


def _pair_of(x, b):
    return dict(ix=x["ix"][b], iy=x["iy"][b], grad=x["grad"][b], rho=x["rho"][b], u=[a[b] for a in x["u"]], p=[a[b] for a in x["p"]])


def _run(gpu, form, x, niter, nograd=False, zero_p=False, **kw):
    """-> (planes [u..., p...] as numpy arrays, error sums or None)."""
    import torch
    from opencv_contrib_amd import cuda
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    gam = kw.get("gamma", 0.0) != 0.0
    p = None if kw.get("p_zero") else [T(np.zeros_like(a) if zero_p else a) for a in x["p"]]
    u, po, err = cuda.tvl1_iterate_stage(form, T(x["ix"]), T(x["iy"]), None if nograd else T(x["grad"]), T(x["rho"]),
                                         [T(a) for a in x["u"][:3 if gam else 2]], p, L_T, THETA, TAUT, niter, **kw)
    return [t.cpu().numpy() for t in u + po], err


def _names(gam):
    return U_NAMES[:3] + P_NAMES if gam else U_NAMES[:2] + P_NAMES[:4]


def _assert_same(a, b, gam, what):
    for nm, x, y in zip(_names(gam), a, b):
        np.testing.assert_array_equal(x, y, err_msg=f"{nm}: {what}")


# ------------------------------------------------------------------ the hook refuses what no kernel runs
def test_stage_hook_refuses_unsupported_combinations(gpu):
    import torch
    from opencv_contrib_amd import capi
    x = _inputs(40, 70, seed=1, gam=True)
    G = dict(gamma=GAMMA)
    bad = [("exact_blocked", 10, G), ("blocked", 7, dict(blocks=[7])), ("blocked", 10, dict(rows_per_band=7)),
           ("tile", 10, dict(rows_per_band=8)), ("tile", 10, dict(variant=9)), ("tile", 10, dict(variant=2, **G)),
           ("spec", 10, dict(time_block=8)), ("spec", 10, dict(time_block=10, p_zero=True)), ("indep", 5, dict(blocks=[5], **G)),
           ("blocked", 9, dict(blocks=[5, 4], **G)), ("blocked", 11, dict(blocks=[10])), ("exact_blocked", 10, dict(blocks=[6, 4])),
           ("one", 2, dict(nograd=True)), ("indep", 10, dict(nograd=True)), ("blocked", 10, dict(nograd=True, blocks=[5, 5])),
           ("tile", 10, dict(nograd=True)), ("blocked", 10, dict(want_err=True)), ("spec_tile", 10, dict(time_block=11))]
    for form, niter, kw in bad:
        kw = dict(kw)
        nograd = kw.pop("nograd", False)
        with pytest.raises(capi.MiError) as ei:
            _run(gpu, form, x, niter, nograd=nograd, **kw)
        assert ei.value.code in (-1, -3), (form, kw, ei.value)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ a. NG: |grad|^2 formed inside the pass
@pytest.mark.parametrize("shape", SHAPES + [(8, 247), (300, 483)])
def test_ng_kernel_equals_grad_plane_and_independent_waves(gpu, shape):
    """The headline kernel (k_iterate_tbr<10, .., NG = true>, what calc() runs on the streaming levels) forms |grad|^2 from I1wx, I1wy
    with the warp's expression; against the joined-wave kernel reading the plane and the independent-wave kernel: all six planes
    bit-identical after 10, 20 and 30 iterations, and whatever the band height."""
    x = _inputs(*shape, seed=3)
    for niter in (10, 20, 30):
        ng, _ = _run(gpu, "blocked", x, niter, nograd=True, time_block=10)
        jw, _ = _run(gpu, "blocked", x, niter, time_block=10)
        iw, _ = _run(gpu, "indep", x, niter, time_block=10)
        _assert_same(ng, jw, False, f"NG vs grad plane niter={niter}")
        _assert_same(ng, iw, False, f"NG vs independent waves niter={niter}")
    planner, _ = _run(gpu, "blocked", x, 20, nograd=True, time_block=10)
    for rows in (8, 13, 37):
        a, _ = _run(gpu, "blocked", x, 20, nograd=True, time_block=10, rows_per_band=rows)
        _assert_same(a, planner, False, f"NG rows_per_band={rows}")


@pytest.mark.parametrize("shape", [(45, 247), (33, 483)])
def test_ng_kernel_batch_equals_single_runs(gpu, shape):
    x = _inputs(*shape, seed=5, B=3)
    for rows in (0, 13):
        bt, _ = _run(gpu, "blocked", x, 20, nograd=True, time_block=10, rows_per_band=rows)
        for b in range(3):
            s, _ = _run(gpu, "blocked", _pair_of(x, b), 20, nograd=True, time_block=10, rows_per_band=rows)
            _assert_same([a[b] for a in bt], s, False, f"pair {b} rows={rows}")


# ------------------------------------------------------------------ b. gamma != 0, exact math vs the oracle
@pytest.mark.parametrize("shape", [(37, 64), (70, 65), (53, 247), (40, 483), (24, 1920)])
@pytest.mark.parametrize("err_u3", [0, 1])
def test_gamma_exact_one_iteration_matches_oracle(gpu, oracle, shape, err_u3):
    """k_iterate<EXACT, .., GAMMA> (the checked launch) against oracle.tvl1_iteration(gamma) on all nine planes, at the bound of the
    gamma = 0 stage test; its error sums (quantised per workgroup, so not exact) against the oracle's fixed-point sums."""
    x = _inputs(*shape, seed=7, gam=True)
    niter = 3
    ru, rp, want = [a.copy() for a in x["u"]], [a.copy() for a in x["p"]], []
    for _ in range(niter):
        prev = [a.copy() for a in ru]
        out = oracle.tvl1_iteration(0, x["ix"], x["iy"], x["grad"], x["rho"], ru[0], ru[1], *rp[:4], L_T, THETA, TAUT,
                                    gamma=GAMMA, u3=ru[2], p31=rp[4], p32=rp[5])
        ru = [out[1], out[2], out[7]]
        rp = [out[3], out[4], out[5], out[6], out[8], out[9]]
        want.append(oracle.tvl1_err_fix(prev, ru, eu3=err_u3))
    got, err = _run(gpu, "one", x, niter, exact=True, gamma=GAMMA, err_u3=err_u3, want_err=True)
    for nm, a, b in zip(_names(True), got, ru + rp):
        np.testing.assert_allclose(a, b, rtol=0, atol=2e-6 * niter, err_msg=nm)
    np.testing.assert_allclose(np.array(err[0], np.float64), np.array(want, np.float64), rtol=2e-5)


# ------------------------------------------------------------------ c. gamma != 0, fast blocked: every form the same bits
def _decompositions(n):
    """Greedy blocks of at most 10, 5, 2 and 1, and a mix of all four lengths in two orders."""
    out = [_greedy(n, [10, 5, 2, 1]), _greedy(n, [5, 2, 1]), _greedy(n, [2, 1]), [1] * n]
    mix = [1, 2, 5, 10, 5, 2, 1, 10]
    m, left = [], n
    for v in mix * 4:
        if v <= left:
            m.append(v)
            left -= v
    m += [1] * left
    out.append(m)
    out.append(list(reversed(m)))
    return out


def _greedy(n, sup):
    blocks = []
    while n > 0:
        t = max(v for v in sup if v <= n)
        blocks.append(t)
        n -= t
    return blocks


@pytest.mark.parametrize("shape", SHAPES)
def test_gamma_fast_blocked_forms_bit_identical_and_close_to_exact(gpu, shape):
    """k_iterate_tbr<.., GAM>: blocks of 10 and 5 run as joined waves (seam values, u3 included, handed over through LDS), blocks of 2
    and 1 as independent waves, and the register tile with the channel (variants 0 and 1).  Any mix gives the same nine planes bit for
    bit -- a wrong u3 / p31 hand-over at a seam cannot hide behind an error both forms share -- and they stay within 2e-5 per
    iteration of the exact one-iteration kernel, borders included."""
    x = _inputs(*shape, seed=11, gam=True)
    for niter in (10, 20, 23):
        ref = None
        for blocks in _decompositions(niter):
            got, _ = _run(gpu, "blocked", x, niter, blocks=blocks, gamma=GAMMA, err_u3=1)
            if ref is None:
                ref = got
            else:
                _assert_same(got, ref, True, f"blocks {blocks}")
        iw, _ = _run(gpu, "indep", x, niter, blocks=_greedy(niter, [2, 1]), gamma=GAMMA)
        _assert_same(iw, ref, True, f"independent waves niter={niter}")
        for variant in (0, 1):
            tb = _greedy(niter, [10, 7, 3])
            tl, _ = _run(gpu, "tile", x, niter, blocks=tb, variant=variant, gamma=GAMMA)
            _assert_same(tl, ref, True, f"tile variant {variant} blocks {tb}")
        ex, _ = _run(gpu, "one", x, niter, exact=True, gamma=GAMMA)
        for nm, a, b in zip(_names(True), ref, ex):
            np.testing.assert_allclose(a, b, rtol=0, atol=2e-5 * niter, err_msg=f"{nm} niter={niter} fast blocked vs exact")
    for rows in (8, 13, 37):
        got, _ = _run(gpu, "blocked", x, 23, blocks=[10, 5, 5, 2, 1], rows_per_band=rows, gamma=GAMMA)
        _assert_same(got, _run(gpu, "blocked", x, 23, gamma=GAMMA)[0], True, f"rows_per_band={rows}")


def test_gamma_fast_blocked_batch_equals_single_runs(gpu):
    x = _inputs(41, 483, seed=13, gam=True, B=3)
    for form, kw in (("blocked", dict(blocks=[10, 5, 2, 1])), ("tile", dict(blocks=[10, 8], variant=1))):
        bt, _ = _run(gpu, form, x, 18, gamma=GAMMA, **kw)
        for b in range(3):
            s, _ = _run(gpu, form, _pair_of(x, b), 18, gamma=GAMMA, **kw)
            _assert_same([a[b] for a in bt], s, True, f"{form} pair {b}")


# ------------------------------------------------------------------ d. the first pass of a scale: p = 0 without reading p
@pytest.mark.parametrize("shape", SHAPES)
def test_p_zero_kernels_equal_explicit_zero_planes(gpu, shape):
    """The PZ instantiations (the first pass of every scale) against the same forms fed explicit zero p planes (the hook fills the p
    planes it does not read with NaN): NG and gamma blocked, the register tile with and without the channel, the exact blocks."""
    x = _inputs(*shape, seed=17, gam=True)
    x2 = dict(x, u=x["u"][:2], p=x["p"][:4])
    cases = [("blocked", x2, False, dict(blocks=[10, 10], nograd=True)), ("blocked", x, True, dict(blocks=[10, 5, 2, 1])),
             ("blocked", x, True, dict(blocks=[2, 10])), ("blocked", x, True, dict(blocks=[1, 1])),
             ("tile", x2, False, dict(blocks=[7, 10], variant=0)), ("tile", x, True, dict(blocks=[10, 3], variant=1)),
             ("exact_blocked", x2, False, dict(blocks=[5, 3])), ("exact_blocked", x2, False, dict(blocks=[1, 2]))]
    for form, xx, gam, kw in cases:
        kw = dict(kw)
        nograd = kw.pop("nograd", False)
        n = sum(kw["blocks"])
        g = dict(gamma=GAMMA) if gam else {}
        a, _ = _run(gpu, form, xx, n, nograd=nograd, p_zero=True, **g, **kw)
        b, _ = _run(gpu, form, xx, n, nograd=nograd, zero_p=True, **g, **kw)
        assert all(np.isfinite(v).all() for v in a), (form, kw)
        _assert_same(a, b, gam, f"{form} {kw} p_zero vs zero planes")


# ------------------------------------------------------------------ e. the speculative steps (MODE 1)
def _mode0_trajectory(gpu, x, niter, gam):
    """The fixed-work planes after 0, 1, .., niter iterations (blocked kernel; any decomposition gives the same bits)."""
    g = dict(gamma=GAMMA) if gam else {}
    traj = [list(x["u"][:3 if gam else 2]) + list(x["p"][:6 if gam else 4])]
    for t in range(1, niter + 1):
        traj.append(_run(gpu, "blocked", x, t, **g)[0])
    return traj


def _check_spec(gpu, oracle, x, niter, traj, gam, eu3, what, **kw):
    g = dict(gamma=GAMMA, err_u3=eu3) if gam else {}
    got, err = _run(gpu, kw.pop("form"), x, niter, want_err=True, **g, **kw)
    _assert_same(got, traj[niter], gam, f"{what}: planes vs fixed work")
    nu = 3 if gam else 2
    want = [oracle.tvl1_err_fix(traj[t][:nu], traj[t + 1][:nu], eu3=eu3 if gam else 0) for t in range(niter)]
    assert err[0] == want, f"{what}: error sums {err[0]} != {want}"
    return want


@pytest.mark.parametrize("shape", SHAPES)
def test_speculative_steps_equal_fixed_work_and_exact_error_sums(gpu, oracle, shape):
    """MODE 1 as run_spec runs it (blocks of T, then the settling launch), with a threshold no iteration passes: NG streaming (T = 10,
    5), gamma streaming (10, 5) with and without (du3)^2, and the register tiles (blocks <= 4, <= 7, 10 on tiles of that margin;
    gamma 0 and != 0).  Planes bit-identical to fixed work; every iteration's integer error sum equal to the oracle's fixed-point sum
    of the fixed-work planes, exactly -- halo rows, seams and tile margins counted once, nothing dropped."""
    x = _inputs(*shape, seed=19, gam=True)
    x2 = dict(x, u=x["u"][:2], p=x["p"][:4])
    n = 12
    t0, t3 = _mode0_trajectory(gpu, x2, n, False), _mode0_trajectory(gpu, x, n, True)
    for T in (10, 5):
        _check_spec(gpu, oracle, x2, n, t0, False, 0, f"NG T={T}", form="spec", time_block=T, nograd=True)
        for eu3 in (0, 1):
            _check_spec(gpu, oracle, x, n, t3, True, eu3, f"gamma T={T} eu3={eu3}", form="spec", time_block=T)
    _check_spec(gpu, oracle, x2, n, t0, False, 0, "NG T=10 rows 13", form="spec", time_block=10, nograd=True, rows_per_band=13)
    _check_spec(gpu, oracle, x, n, t3, True, 1, "gamma T=5 rows 8", form="spec", time_block=5, rows_per_band=8)
    for T in (4, 7, 10):
        for variant in (0, 1):
            _check_spec(gpu, oracle, x2, n, t0, False, 0, f"tile T={T} v{variant}", form="spec_tile", time_block=T, variant=variant)
        _check_spec(gpu, oracle, x, n, t3, True, T % 2, f"tile gamma T={T}", form="spec_tile", time_block=T, variant=T % 2)


def test_speculative_steps_count_saturated_terms(gpu, oracle):
    """A few pixels move by more than 16 px (et >= 256 px^2): their terms saturate at 2^32 - 1 on the device and in the oracle alike."""
    x = _inputs(60, 483, seed=23, gam=True, spikes=True)
    x2 = dict(x, u=x["u"][:2], p=x["p"][:4])
    n = 7
    t0, t3 = _mode0_trajectory(gpu, x2, n, False), _mode0_trajectory(gpu, x, n, True)
    e1 = t0[1][0] - t0[0][0]
    e2 = t0[1][1] - t0[0][1]
    assert ((e1.astype(np.float64) ** 2 + e2.astype(np.float64) ** 2) >= 256).sum() >= 3, "no saturated term in the first iteration"
    _check_spec(gpu, oracle, x2, n, t0, False, 0, "NG T=5", form="spec", time_block=5, nograd=True)
    _check_spec(gpu, oracle, x2, n, t0, False, 0, "tile T=7", form="spec_tile", time_block=7, variant=0)
    _check_spec(gpu, oracle, x, n, t3, True, 1, "gamma T=10", form="spec", time_block=10)


def test_speculative_steps_batch_equals_single_runs(gpu):
    x = _inputs(33, 247, seed=29, gam=True, B=3)
    x2 = dict(x, u=x["u"][:2], p=x["p"][:4])
    for form, xx, kw in (("spec", x2, dict(time_block=10, nograd=True)), ("spec", x, dict(time_block=5, gamma=GAMMA, err_u3=1)),
                         ("spec_tile", x2, dict(time_block=7, variant=1))):
        kw = dict(kw)
        nograd = kw.pop("nograd", False)
        bt, be = _run(gpu, form, xx, 12, nograd=nograd, want_err=True, **kw)
        gam = "gamma" in kw
        for b in range(3):
            s, se = _run(gpu, form, _pair_of(xx, b), 12, nograd=nograd, want_err=True, **kw)
            _assert_same([a[b] for a in bt], s, gam, f"{form} pair {b}")
            assert be[b] == se[0], (form, b)


# ------------------------------------------------------------------ the checked one-iteration launch's sums are raw integers too
def test_checked_one_iteration_sums_are_fixed_point_integers(gpu, oracle):
    """The error-checked one-iteration launch quantises each workgroup's float sum: not exact, but within rtol 2e-5 of the oracle's
    fixed-point sum of its own planes (fast math) -- and its planes equal the unchecked launch's."""
    x = _inputs(70, 300, seed=31)
    n = 4
    traj = [list(x["u"])]
    for t in range(1, n + 1):
        traj.append(_run(gpu, "one", x, t)[0][:2])
    got, err = _run(gpu, "one", x, n, want_err=True)
    plain, _ = _run(gpu, "one", x, n)
    _assert_same(got, plain, False, "checked vs unchecked")
    want = [oracle.tvl1_err_fix(traj[t], traj[t + 1]) for t in range(n)]
    np.testing.assert_allclose(np.array(err[0], np.float64), np.array(want, np.float64), rtol=2e-5)
