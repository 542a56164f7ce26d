"""SURF: oracle self-tests (CPU) and HIP-vs-oracle parity (GPU) for cv::cuda::SURF_CUDA.

What is held to what (every whole-class comparison goes through tests/surf_check.py::assert_surf_equals, every feature of it):
  * integral image, det / trace planes, candidate set, and the x / y / laplacian / octave / size / hessian rows: EQUAL IN EVERY BIT --
    the same double / float operations in the same order on both sides (box_div is the correctly rounded quotient, solve3x3 the
    reference's double reciprocal, no contraction);
  * angle: within 2^-13 degrees (circular) of a direction the oracle admits for that feature when every atan2 is correctly rounded
    and every sample whose angle lies within 2^-13 degrees of a half-integer may round either way (the device's atan2f is within 2 ulp
    of the correctly rounded value: test_device_atan2f_is_within_two_ulp; the derivation of 2^-13 is in tests/surf_check.py);
  * descriptors: equal in every bit to the oracle's descriptor AT THE HIP ANGLE with the sine and cosine of the direction correctly
    rounded, which the kernels' sincos_rounded is (test_sincos_rounded_is_correctly_rounded).
The reference's own CUDA-vs-CPU acceptance is far looser (matched-keypoint ratio > 0.95, descriptor match ratio > 0.6,
xfeatures2d/test/test_surf.cuda.cpp:102-107,166-173).
"""
import os
import sys

import numpy as np
import pytest

from opencv_contrib_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import surf_check as S  # noqa: E402
from surf_check import TILE_EDGE_CASES, assert_surf_equals  # noqa: E402


def T(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------ oracle (CPU)
def test_oracle_tables_match_reference_literals(oracle):
    """Generated tables vs literal entries of the reference's constant tables (xfeatures2d/src/cuda/surf.cu:520-522,
    685-707): c_aptX[0..8], c_aptY[0..8], c_aptW[0], c_aptW[56] (centre), c_DW[0], c_DW[21], c_DW[210]."""
    ax, ay, aw, dw = oracle.surf_tables()
    np.testing.assert_array_equal(ax[:9], [-6, -5, -5, -5, -5, -5, -5, -5, -4])
    np.testing.assert_array_equal(ay[:9], [0, -3, -2, -1, 0, 1, 2, 3, -4])
    assert ax[-1] == 6 and ay[-1] == 0 and len(ax) == 113
    # bit for bit (round 3: the generator reproduces the literals' own rounding; all 113 + 400 entries are compared against the parsed
    # reference file in tests/test_ref_pin_cuda.py::test_surf_weight_tables_equal_the_literals_of_surf_cu)
    np.testing.assert_array_equal([aw[0], aw[56]], np.array([0.001455130288377404, 0.02592208795249462], np.float32))
    np.testing.assert_array_equal([dw[0], dw[21], dw[210]], np.array([3.695352233989979e-06, 1.929736572492402e-05, 0.01435048412531614], np.float32))


def test_oracle_integral(oracle):
    img = np.random.default_rng(0).integers(0, 256, size=(37, 53)).astype(np.uint8)
    s = oracle.surf_integral(img)
    ref = np.zeros((38, 54), np.uint64)
    ref[1:, 1:] = img.astype(np.uint64).cumsum(0).cumsum(1)
    np.testing.assert_array_equal(s, ref.astype(np.uint32))


def test_oracle_cross_fixture(oracle):
    """A self-contained SURF fixture of the reference (xfeatures2d/test/test_rotation_and_scale_invariance.cpp:259-285; the one
    with known answers, the Java tests' cross, is in tests/test_zz_surf_cpu_class.py:
    100x100 white image, two 3-px dark bars, SURF(8000, 3, 4, extended, upright=false)).  The CPU class reports 5
    keypoints there; under the CUDA class's strict 26-neighbour maximum the centre is a plateau (det = 15376 on a 3x3
    patch of layer 1) and only the 4 symmetric keypoints survive -- with equal responses, as that test requires."""
    img = synth.cross_image()
    r = oracle.surf_detect_describe(img, oracle.surf_params(hessian_threshold=8000, n_octaves=3, n_octave_layers=4, extended=1,
                                                            keypoints_ratio=0.05))
    assert r["n"] == 4
    assert np.ptp(r["hessian"]) <= 1e-6 * r["hessian"][0]
    c = np.stack([r["x"], r["y"]], 1)
    np.testing.assert_allclose(np.abs(c - 50.0), np.abs(c[0] - 50.0)[None].repeat(4, 0), rtol=1e-6)   # 4-fold symmetric about (50,50)
    assert set(map(tuple, np.sign(c - 50.0).astype(int))) == {(-1, -1), (1, -1), (-1, 1), (1, 1)}


def test_oracle_blobs_scale_and_descriptor_norm(oracle):
    img = synth.blob_image(240, 320, seed=7)
    r = oracle.surf_detect_describe(img, oracle.surf_params(hessian_threshold=400))
    assert r["n"] > 50 and len(np.unique(r["octave"])) >= 2
    np.testing.assert_allclose(np.linalg.norm(r["descriptors"], axis=1), 1.0, atol=1e-5)
    assert ((r["angle"] >= 0) & (r["angle"] < 360)).all()
    r2 = oracle.surf_detect_describe(img, oracle.surf_params(hessian_threshold=400, upright=1, extended=1))
    assert (r2["angle"] == 270).all() and r2["descriptors"].shape[1] == 128 and r2["n"] == r["n"]


def test_oracle_mask_and_errors(oracle):
    img = synth.blob_image(200, 260, seed=3)
    full = oracle.surf_detect_describe(img, oracle.surf_params(hessian_threshold=300), want_desc=False)
    mask = np.zeros_like(img); mask[:, :130] = 255
    half = oracle.surf_detect_describe(img, oracle.surf_params(hessian_threshold=300), mask=mask, want_desc=False)
    assert 0 < half["n"] < full["n"] and half["x"].max() < 140
    with pytest.raises(ValueError):
        oracle.surf_detect_describe(img[:60, :60], oracle.surf_params())          # too small for 4 octaves (surf.cuda.cpp:144-151)
    with pytest.raises(ValueError):
        oracle.surf_detect_describe(img, oracle.surf_params(n_octaves=0))


# ------------------------------------------------------------------ HIP vs oracle (GPU)
gpu_mark = pytest.mark.gpu


@gpu_mark
def test_wave_scan_semantics(gpu):
    import ctypes as C
    from opencv_contrib_amd import capi
    v = np.random.default_rng(1).integers(0, 1000, size=64).astype(np.uint32)
    inp = (C.c_uint * 64)(*[int(x) for x in v]); out = (C.c_uint * 64)()
    capi.check(capi.lib().miflow_selftest_wave_scan(inp, out))
    np.testing.assert_array_equal(np.array(out[:], np.uint64), np.cumsum(v.astype(np.uint64)))


@gpu_mark
@pytest.mark.parametrize("shape", [(37, 53), (100, 64), (481, 1283)])
def test_integral_bit_exact(gpu, oracle, shape):
    from opencv_contrib_amd import cuda
    img = np.random.default_rng(2).integers(0, 256, size=shape).astype(np.uint8)
    np.testing.assert_array_equal(N(cuda.surf_integral(T(img, gpu))).view(np.uint32), oracle.surf_integral(img))
    m = (img > 100).astype(np.uint8) * 255
    np.testing.assert_array_equal(N(cuda.surf_integral(T(m, gpu), True)).view(np.uint32), oracle.surf_integral(np.minimum(m, 1)))


@gpu_mark
@pytest.mark.parametrize("octave", [0, 1, 2, 3, 4])
def test_det_trace_matches_oracle(gpu, oracle, octave):
    """k_det_trace against the oracle with nOctaveLayers 1, 2 and 4, on the frames at the tile edges and 200 x 264: every det and trace
    value equal in its bits (the cells no sample reaches hold +0.0 on both sides).  An image too small for an octave by the class's
    own limits (surf.cuda.cpp:144-151: octave 3 on the tile-edge frames, octave 4 everywhere) is rejected by both sides.
    MI355X: no differing value in any of the 75 plane pairs."""
    from opencv_contrib_amd import capi, cuda
    ran = 0
    for shape in [sh for sh, _, _ in TILE_EDGE_CASES] + [(200, 264)]:
        Sum = oracle.surf_integral(synth.blob_image(*shape, seed=5))
        St = T(Sum.view(np.int32), gpu)
        for layers in (1, 2, 4):
            try:
                rd, rt = oracle.surf_det_trace(Sum, octave, layers)
            except ValueError:
                with pytest.raises(capi.MiError):
                    cuda.surf_detTrace(St, octave, layers)
                continue
            gd, gt = cuda.surf_detTrace(St, octave, layers)
            lc = shape[1] >> octave
            ran += 1
            np.testing.assert_array_equal(S.bits(N(gd)[:, :lc]), S.bits(rd[:, :lc]), err_msg=f"det, {shape}, {layers} layers")
            np.testing.assert_array_equal(S.bits(N(gt)[:, :lc]), S.bits(rt[:, :lc]), err_msg=f"trace, {shape}, {layers} layers")
    assert ran == {0: 24, 1: 24, 2: 24, 3: 3, 4: 0}[octave]


def _run(gpu, oracle, img, what, thr, octaves, layers, extended=False, ratio=0.05, upright=False, mask=None):
    """detectWithDescriptors against the oracle's detection through assert_surf_equals -> (the oracle's result, the checker's counts)"""
    from opencv_contrib_amd import cuda
    ref = oracle.surf_detect_describe(img, oracle.surf_params(hessian_threshold=thr, n_octaves=octaves, n_octave_layers=layers, extended=int(extended),
                                                              upright=int(upright), keypoints_ratio=ratio), mask=mask, want_desc=False)
    alg = cuda.SURF_CUDA.create(thr, octaves, layers, extended, ratio, upright)
    kpg, desc = alg.detectWithDescriptors(T(img, gpu), None if mask is None else T(mask, gpu))
    assert desc.shape == (ref["n"], alg.descriptorSize())
    return ref, assert_surf_equals(oracle, img, cuda.SURF_CUDA.downloadKeypoints(kpg), N(desc), ref, extended=extended, upright=upright, what=what)


@gpu_mark
@pytest.mark.parametrize("thr,octaves,layers,extended,upright", S.GRID)
def test_detect_and_describe_match_oracle(gpu, oracle, thr, octaves, layers, extended, upright):
    """Parameter grid after xfeatures2d/test/test_surf.cuda.cpp:176-187, keypointsRatio 0.05 as there (:92)."""
    from opencv_contrib_amd import cuda
    ref, _ = _run(gpu, oracle, synth.blob_image(300, 400, seed=11), "grid", thr, octaves, layers, extended, 0.05, upright)
    assert ref["n"] > 20 and cuda.SURF_CUDA.create(thr).defaultNorm() == 4


@gpu_mark
@pytest.mark.parametrize("octaves,layers", S.PLANS)
def test_detect_per_octave_and_all_octave_launch_plans_agree_with_the_oracle(gpu, oracle, octaves, layers):
    """Round 3: one launch per detector stage covers all octaves where the kernel arguments hold them (<= 6 octaves, nOctaveLayers + 2
    <= 6 layers: every default); otherwise the octaves run one after the other through one set of planes (the round-2 plan).
    (3, 5) takes the per-octave plan, (4, 4) and (2, 1) the all-octave plan at its layer limit / smallest size; one handle re-used
    across a change of the plan must re-size its scratch."""
    from opencv_contrib_amd import cuda
    img = synth.blob_image(300, 400, seed=21)
    for (o, l) in ((octaves, layers), (2, 2)):
        ref = oracle.surf_detect_describe(img, oracle.surf_params(hessian_threshold=100.0, n_octaves=o, n_octave_layers=l, keypoints_ratio=0.05), want_desc=False)
        alg = cuda.SURF_CUDA.create(100.0, o, l, False, 0.05, False)
        kpg, desc = alg.detectWithDescriptors(T(img, gpu))
        assert ref["n"] > 20
        assert_surf_equals(oracle, img, cuda.SURF_CUDA.downloadKeypoints(kpg), N(desc), ref, extended=False, upright=False, what=f"plan {o}/{l}")


@gpu_mark
@pytest.mark.parametrize("shape,thr,extended", [((300, 400), 100.0, False), ((1080, 1920), 400.0, False), ((720, 1283), 50.0, True)])
def test_detect_and_compute_with_the_count_on_the_device_is_bit_identical(gpu, shape, thr, extended):
    """Round 5: `mi_surf_detect_and_compute` leaves the feature count on the device between detectKeypoints and
    computeDescriptors (the reference reads keypoints.cols back in between, surf.cuda.cpp:205-209) -- the descriptor kernels read it
    themselves and a fixed grid walks the features.  Keypoints and descriptors must equal, bit for bit, detect() followed by
    compute_descriptors with the host-known count (one workgroup per feature); overflow (tiny keypointsRatio) and a mask included."""
    from opencv_contrib_amd import cuda
    img = synth.blob_image(*shape, seed=31)
    t = T(img, gpu)
    for ratio, mask in ((0.05 if shape[0] < 1000 else 0.01, None), (0.0005, None), (0.05 if shape[0] < 1000 else 0.01, "m")):
        m = None
        if mask:
            mm = np.zeros_like(img); mm[shape[0] // 8: shape[0] // 2, shape[1] // 6: shape[1] - 40] = 1
            m = T(mm, gpu)
        alg = cuda.SURF_CUDA.create(thr, 4, 2, extended, ratio, False)
        kp1, d1 = alg.detectWithDescriptors(t, m)
        kp0 = alg.detect(t, m)
        assert kp0.shape == kp1.shape and kp0.shape[1] > 5
        np.testing.assert_array_equal(N(kp0), N(kp1))
        _, d0 = alg.detectWithDescriptors(t, None, kp0.clone(), True)   # provided keypoints: host-known count, one workgroup per feature
        assert d0.shape == d1.shape == (kp0.shape[1], alg.descriptorSize())
        np.testing.assert_array_equal(N(d0), N(d1))


@gpu_mark
def test_maxima_flagged_inside_the_det_kernel_are_bit_identical(gpu):
    """Round 5: octave 0's det / trace values stay in the LDS tile of the kernel that computes them, the 26
    comparisons run there and only the flag words (+ the sign of the trace at each maximum) leave it; the sub-pixel refinement
    evaluates its 27 values from the integral image (MIFLOW_SURF_NMS0=1: an opt-in -- measured slower than the plane form, see
    surf_api.cpp).  Keypoints (order included) and descriptors must not change by a bit against the default plane form -- 4K at the BASELINE setting, small and odd sizes, one
    layer, a mask, the overflow of the candidate list, and the small frames at the tile edges (TILE_EDGE_CASES).  The switch is read once
    per process, hence the subprocesses."""
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for tag, env in (("fused", {"MIFLOW_SURF_NMS0": "1"}), ("planes", {}), ("strided", {"MIFLOW_SURF_POLY": "0"})):
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "surf_digest.py")], capture_output=True, text=True,
                           env=dict(os.environ, **env), timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        out[tag] = re.findall(r"n=(\d+) digest ([0-9a-f]{16})", r.stdout)
        assert len(out[tag]) == 5 + len(TILE_EDGE_CASES) and all(int(n) > 5 for n, _ in out[tag]), r.stdout
    # ... and the polyphase planes of the integral image (octaves >= 1 read consecutive words, the default since round 5) against the
    # strided gathers (MIFLOW_SURF_POLY=0): the same integers, the same det / trace values
    assert out["fused"] == out["planes"] == out["strided"], out


# TILE_EDGE_CASES: tests/surf_check.py
@gpu_mark
def test_detect_at_the_tile_edges_matches_the_oracle(gpu, oracle):
    """The default launch forms on TILE_EDGE_CASES against the oracle (threshold 50, keypointsRatio 0.05): a wrong region offset or
    tile count of the detect plan (csrc/surf_plan.h) shows where a frame ends just before, at and just after a tile."""
    for shape, octaves, layers in TILE_EDGE_CASES:
        ref, _ = _run(gpu, oracle, synth.blob_image(*shape, seed=41), f"tile edge {shape}", 50.0, octaves, layers)
        assert ref["n"] > 5, (shape, ref["n"])


@gpu_mark
def test_detect_mask_overflow_and_provided_keypoints(gpu, oracle):
    from opencv_contrib_amd import cuda
    img = synth.blob_image(260, 330, seed=13)
    mask = np.zeros_like(img); mask[40:200, 30:220] = 7
    p = oracle.surf_params(hessian_threshold=200, keypoints_ratio=0.05)
    ref = oracle.surf_detect_describe(img, p, mask=mask, want_desc=False)
    alg = cuda.SURF_CUDA.create(200, _keypointsRatio=0.05)
    kpg = alg.detect(T(img, gpu), T(mask, gpu))
    assert 20 < ref["n"]
    assert_surf_equals(oracle, img, cuda.SURF_CUDA.downloadKeypoints(kpg), None, ref, extended=False, upright=False, what="rectangular mask, detect()")
    # overflow: tiny keypointsRatio -> deterministic prefix of the scan-ordered feature list
    full = oracle.surf_detect_describe(img, oracle.surf_params(hessian_threshold=50, keypoints_ratio=0.05), want_desc=False)
    few = oracle.surf_detect_describe(img, oracle.surf_params(hessian_threshold=50, keypoints_ratio=0.0004), want_desc=False)
    assert few["n"] == int(np.float32(260 * 330) * np.float32(0.0004)) < full["n"]
    kpf, df = cuda.SURF_CUDA.create(50, _keypointsRatio=0.0004).detectWithDescriptors(T(img, gpu))
    assert_surf_equals(oracle, img, cuda.SURF_CUDA.downloadKeypoints(kpf), N(df), few, extended=False, upright=False, what="feature-list overflow")
    # useProvidedKeypoints: orientation + descriptors recomputed for the given keypoints
    ref2 = oracle.surf_detect_describe(img, oracle.surf_params(hessian_threshold=200, keypoints_ratio=0.05), want_desc=False)
    kpg2 = alg.detect(T(img, gpu))
    kpg2c = kpg2.clone(); kpg2c[5] = 0
    kpo, desc = alg.detectWithDescriptors(T(img, gpu), None, kpg2c, True)
    assert_surf_equals(oracle, img, cuda.SURF_CUDA.downloadKeypoints(kpo), N(desc), ref2, extended=False, upright=False, provided_angle=0.0,
                       what="provided after detect")


@gpu_mark
def test_cross_fixture_and_errors(gpu, oracle):
    import torch
    from opencv_contrib_amd import cuda, capi
    img = synth.cross_image()
    alg = cuda.SURF_CUDA.create(8000, 3, 4, True, 0.05, False)
    kp = cuda.SURF_CUDA.downloadKeypoints(alg.detect(T(img, gpu)))
    assert kp["x"].shape[0] == 4 and np.ptp(kp["hessian"]) <= 1e-6 * kp["hessian"][0]
    with pytest.raises(capi.MiError):
        cuda.SURF_CUDA.create(100).detect(T(img[:60, :60], gpu))                  # too small for 4 octaves
    with pytest.raises(capi.MiError):
        cuda.SURF_CUDA.create(100).detect(T(img.astype(np.float32), gpu))         # CV_8UC1 only (surf.cuda.cpp:139)
    with pytest.raises(capi.MiError):
        cuda.SURF_CUDA.create(100).detect(T(img, gpu), T(img[:50], gpu))          # mask size (:140)
    # determinism: two runs, identical bytes
    b = synth.blob_image(300, 400, seed=4)
    a1, alg2 = cuda.SURF_CUDA.create(100), cuda.SURF_CUDA.create(100)
    k1, d1 = a1.detectWithDescriptors(T(b, gpu)); k2, d2 = alg2.detectWithDescriptors(T(b, gpu))
    # compare bit patterns: the LAPLACIAN row stores int -1 = 0xFFFFFFFF, a NaN when read as float
    assert torch.equal(k1.view(torch.int32), k2.view(torch.int32)) and torch.equal(d1, d2)


_random_surf_configs = S.random_surf_configs


@gpu_mark
@pytest.mark.parametrize("cfg", _random_surf_configs(), ids=lambda c: f"{c['shape'][0]}x{c['shape'][1]}-t{int(c['thr'])}-o{c['octaves']}l{c['layers']}"
                                                                     f"-e{int(c['extended'])}u{int(c['upright'])}")
def test_random_configuration_matches_oracle(gpu, oracle, cfg):
    """Seeded sweep over image sizes (band / chunk edges of the integral, NMS rows, octave sub-sampling remainders), thresholds,
    octave and layer counts, 64 / 128-element descriptors, oriented and upright: every row, angle and descriptor of every feature
    through assert_surf_equals."""
    from opencv_contrib_amd import cuda
    from opencv_contrib_amd import capi
    img = synth.blob_image(*cfg["shape"], seed=cfg["seed"])
    alg = cuda.SURF_CUDA.create(cfg["thr"], cfg["octaves"], cfg["layers"], cfg["extended"], 0.05, cfg["upright"])
    try:
        ref = oracle.surf_detect_describe(img, oracle.surf_params(hessian_threshold=cfg["thr"], n_octaves=cfg["octaves"], n_octave_layers=cfg["layers"],
                                                                  extended=int(cfg["extended"]), upright=int(cfg["upright"]), keypoints_ratio=0.05),
                                          want_desc=False)
    except ValueError:
        # the image is too small for the last octave's filters: CV_Assert(layer_rows - 2 * min_margin > 0), surf.cuda.cpp:154-156
        with pytest.raises(capi.MiError):
            alg.detect(T(img, gpu))
        return
    if ref["n"] == 0:
        kpg = alg.detect(T(img, gpu))
        assert cuda.SURF_CUDA.downloadKeypoints(kpg)["x"].shape[0] == 0
        return
    kpg, desc = alg.detectWithDescriptors(T(img, gpu))
    assert_surf_equals(oracle, img, cuda.SURF_CUDA.downloadKeypoints(kpg), N(desc), ref, extended=cfg["extended"], upright=cfg["upright"], what="sweep")


def test_box_division_by_reciprocal_is_exact(tmp_path):
    """k_det_trace (round 3) divides a box sum by its area as q = a y, q += fma(-q, b, a) y with y = RN(1 / b) instead of a / b.  For
    the integers that occur -- |a| = box sum x weight < 2^35, b = box area < 2^24 -- this must BE the correctly rounded quotient,
    or det / trace would stop being bit-identical to the reference's double-precision division (surf.cu:148): every area of every
    filter size of 5 octaves x 6 layers against 20 000 dividends each (incl. near multiples), and 2e7 random (a, b)."""
    import subprocess
    src = tmp_path / "divtest.c"
    src.write_text(r'''
#include <math.h>
#include <stdio.h>
#include <stdint.h>
static uint64_t s = 88172645463325252ull;
static inline uint64_t rnd(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
static long check(double a, double b)
{
    const double y = 1.0 / b, q = a * y;
    return fma(fma(-q, b, a), y, q) != a / b;
}
int main(void)
{
    long bad = 0, n = 0;
    for (int octave = 0; octave < 5; ++octave)
        for (int layer = 0; layer < 6; ++layer) {
            const int size = (9 + 6 * layer) << octave;
            const float ratio = (float)size / 9;
            int e[10];
            for (int k = 0; k < 10; ++k) e[k] = (int)rintf(ratio * (float)k);
            const int areas[6] = {(e[3] - e[0]) * (e[7] - e[2]), (e[6] - e[3]) * (e[7] - e[2]), (e[9] - e[6]) * (e[7] - e[2]),
                                  (e[4] - e[1]) * (e[4] - e[1]), (e[8] - e[5]) * (e[4] - e[1]), (e[8] - e[5]) * (e[8] - e[5])};
            for (int ai = 0; ai < 6; ++ai)
                for (int t = 0; t < 20000; ++t) {
                    int64_t a = (int64_t)(rnd() % (1ull << 35)) - (1ll << 34);
                    if (t < 200) a = (int64_t)areas[ai] * (t - 100) * 977 + (t % 3) - 1;
                    bad += check((double)a, (double)areas[ai]); ++n;
                }
        }
    for (long t = 0; t < 20000000; ++t) {
        const int64_t a = (int64_t)(rnd() % (1ull << 35)) - (1ll << 34);
        bad += check((double)a, (double)(1 + rnd() % (1u << 24))); ++n;
    }
    printf("%ld %ld\n", n, bad);
    return bad != 0;
}
''')
    exe = str(tmp_path / "divtest")
    r = subprocess.run(["gcc", "-O2", "-mfma", "-ffp-contract=off", str(src), "-o", exe, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    n, bad = (int(x) for x in r.stdout.split())
    assert r.returncode == 0 and n > 2.3e7 and bad == 0, r.stdout


@gpu_mark
def test_staged_descriptor_kernel_is_bit_identical_to_the_global_memory_kernel(gpu):
    """Round 3: features with a cell side s >= 5 build their 21 x 21 patch in `k_descriptors_staged` -- the texels of a strip of patch rows
    staged through LDS by lanes arranged as 8 x 8 blocks of the rotated window lattice, then accumulated per sample in the reference's
    order -- instead of every thread walking its own cell through global memory.  Same texel per (dy, dx), same order of the float
    adds: the descriptors must be identical to the last bit.  tools/surf_stage_check.py prints digests of the 64- and 128-float
    descriptors of the 4K blob frame and of 300 provided keypoints of sizes 4 .. 700 px (cells from below the threshold to larger than a
    tile holds, which stay on the global path); MIFLOW_SURF_STAGE_S is read once per process, hence two subprocesses."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for stage in ("0", "5"):
        env = dict(os.environ, MIFLOW_SURF_STAGE_S=stage)
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "surf_stage_check.py")], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append([l for l in r.stdout.splitlines() if l.startswith(("4K blob", "provided sizes"))])
    assert len(outs[0]) == 4 and all(l.endswith("True") for l in outs[0][2:])
    assert outs[0] == outs[1]


# ------------------------------------------------------------------ the three libm calls, by themselves
def _ordered(a):
    """float32 -> int64 that counts floats in order (-0.0 and +0.0 coincide): |difference| is the distance in ulps"""
    i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _ulp_distance(a, b):
    return np.abs(_ordered(a) - _ordered(b))


def _surf_libm(a, b):
    from opencv_contrib_amd import capi
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape and a.ndim == 1 and 0 < a.size <= 1 << 22
    out = [np.empty_like(a) for _ in range(3)]
    capi.check(capi.lib().miflow_selftest_surf_libm(a.ctypes.data, b.ctypes.data, a.size, *(o.ctypes.data for o in out)))
    return out


def _round_once(v):
    """long double -> (float32, hard): hard where v lies within 2^-16 of a float ulp of the midpoint of two floats"""
    with np.errstate(invalid="ignore", over="ignore"):
        f = v.astype(np.float32)
        other = np.nextafter(f, np.where(v >= f, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        fl, ol = f.astype(np.longdouble), other.astype(np.longdouble)
        hard = np.abs(v - (fl + ol) / 2) < np.abs(ol - fl) / 65536
    return f, hard & np.isfinite(v)


@gpu_mark
def test_device_atan2f_is_within_two_ulp(gpu, oracle):
    """atan2f as k_orientation compiles it (miflow_selftest_surf_libm) against the long-double atan2 rounded once to float, in ulps: on
    the 113 (Y, X) sample pairs of every feature of the `global` keypoint group and of the 300 x 400 blob frame, on 2^20 seeded pairs
    with magnitudes 2^-20 .. 2^20 in both components and every sign, on the axes, the signed zeros in every combination, |Y| == |X|
    and denormals.  Everything tests/surf_check.py bounds -- delta_deg = 2^-13 for the undecided samples and the 2^-13 degrees of the
    final angle -- rests on this distance being at most 2 ulp.
    MI355X: max 2 ulp on the samples of the global group (27 120 pairs), of the blob frame (22 035) and on the 2^20 seeded pairs, 1 ulp
    on the axes / zeros / denormals and on |Y| == |X|; 63 .. 71 % of the results are correctly rounded (95 and 89 % in the last two
    sets); no zero of the wrong sign."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_surf_provided as P
    sets = {}
    x, y, size = P.group("global")
    yx = oracle.surf_orientation_candidates(P.image(), x, y, size)["yx"].reshape(-1, 2)
    sets["samples of the global group"] = (yx[:, 0], yx[:, 1])
    img = synth.blob_image(300, 400, seed=11)
    r = oracle.surf_detect_describe(img, oracle.surf_params(keypoints_ratio=0.05), want_desc=False)
    yx = oracle.surf_orientation_candidates(img, r["x"], r["y"], r["size"])["yx"].reshape(-1, 2)
    sets["samples of the blob frame"] = (yx[:, 0], yx[:, 1])
    rng = np.random.default_rng(4242)
    n = 1 << 20
    mag = lambda: (np.exp2(rng.uniform(-20, 20, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    sets["2^20 seeded pairs"] = (mag(), mag())
    v = np.float32([0.0, -0.0, 1.0, -1.0, 3.5e-4, -7.25, 2.0 ** 20, -2.0 ** -20, 1e-45, -1e-45, 3e-39, -3e-39, 1.1754944e-38, 3.0e38])
    sets["axes, signed zeros, denormals"] = tuple(g.reshape(-1).astype(np.float32) for g in np.meshgrid(v, v, indexing="ij"))
    d = mag()
    sets["|Y| == |X|"] = (d, d * rng.choice([-1.0, 1.0], n).astype(np.float32))
    worst = 0
    for name, (Y, X) in sets.items():
        got = _surf_libm(Y, X)[0]
        want = np.arctan2(Y.astype(np.longdouble), X.astype(np.longdouble)).astype(np.float32)
        u = _ulp_distance(got, want)
        k = int(np.argmax(u))
        print(f"[surf libm] atan2f, {name}: {len(u)} pairs, max {int(u.max())} ulp (at Y = {Y[k]!r}, X = {X[k]!r}: {got[k]!r} vs {want[k]!r}), "
              f"{float((u == 0).mean()):.4f} correctly rounded, sign of zero differs at {int((np.signbit(got) != np.signbit(want)).sum())}")
        worst = max(worst, int(u.max()))
    assert worst <= 2, worst


def _ddir(angle):
    """the descriptor's direction in radians from the ANGLE row, in the kernel's float operations (surf.cu:757-760)"""
    d = np.float32(360.0) - np.float32(angle)
    if abs(d - np.float32(360.0)) < np.finfo(np.float32).eps:
        d = np.float32(0.0)
    return np.float32(d * (np.float32(3.14159265) / np.float32(180.0)))


@gpu_mark
def test_sincos_rounded_is_correctly_rounded(gpu):
    """sincos_rounded (csrc/surf_kernels.hip) decides which texels a window of 800 texels reads.  Against sinl / cosl rounded once:
    every 256th float from 1.4e-36 up to 2 pi (every 256th float of [0, 2 pi] is 4.25 million values, more than one launch of 2^22
    holds; below 1.4e-36 the sine is its argument and the cosine 1, and a few such values and denormals are in the list), +-64 ulps
    around each multiple of pi / 2 up to 1024, both sides of the |x| < 1024 switch, -0.0, +-inf, NaN, and the exact directions of the
    angles 0, 90, 180, 270 and of the last float below 360.  For |x| < 1024 sine and cosine equal the correctly rounded value in every
    bit (zeros compared by value), `hard` arguments -- within 2^-16 ulp of a rounding boundary -- excepted and counted; beyond, the
    device's sincosf is within 2 ulp; NaN and inf give NaN.
    MI355X: of 4 194 292 arguments below 1024 none off the correctly rounded sine or cosine; 19 hard sines and 17 hard cosines, all
    rounded as the long double rounds; sin(-0.0) is +0.0 (the one zero of another sign); beyond 1024 at most 1 ulp."""
    two_pi_bits = int(np.float32(2 * np.pi).view(np.int32))
    kk = np.arange(1, int(1024 / (np.pi / 2)) + 1)
    centres = (kk * (np.pi / 2)).astype(np.float32).view(np.int32).astype(np.int64)
    near = (centres[:, None] + np.arange(-64, 65)[None]).reshape(-1).astype(np.int32).view(np.float32)
    special = np.float32([-0.0, 0.0, 1e-45, -1e-45, 3e-39, 1e-38, 1e-37, -1e-37, np.nextafter(np.float32(1024), np.float32(0)), 1024.0,
                          np.nextafter(np.float32(1024), np.float32(2048)), -np.nextafter(np.float32(1024), np.float32(0)), -1024.0, 1500.5, -4097.0,
                          1e6, 1e10, 1e30, -3e38, np.inf, -np.inf, np.nan] + [_ddir(a) for a in (0.0, 90.0, 180.0, 270.0, np.nextafter(np.float32(360), np.float32(0)))])
    rest = (1 << 22) - near.size * 2 - special.size
    sweep = np.arange(two_pi_bits - 256 * (rest - 1), two_pi_bits + 1, 256, dtype=np.int64).astype(np.int32).view(np.float32)
    x = np.concatenate([sweep, near, -near, special])
    assert x.size == 1 << 22 and sweep[0] > 0 and sweep[0] < 2e-36 and sweep[-1] == np.float32(2 * np.pi)
    _, sn, cs = _surf_libm(x, x)
    xl = x.astype(np.longdouble)
    fin = np.isfinite(x)
    small = fin & (np.abs(x) < 1024)
    n_hard = 0
    with np.errstate(invalid="ignore"):
        for name, got, v in (("sine", sn, np.sin(xl)), ("cosine", cs, np.cos(xl))):
            want, hard = _round_once(v)
            assert np.isnan(got[~fin]).all(), name
            eq = (got.view(np.int32) == want.view(np.int32)) | ((got == 0) & (want == 0))
            bad = small & ~eq & ~hard
            u = _ulp_distance(got[fin & ~small], want[fin & ~small])
            n_hard += int((hard & small).sum())
            print(f"[surf libm] {name}: {int(small.sum())} arguments below 1024, {int((small & ~eq).sum())} not correctly rounded, {int((hard & small).sum())} hard, "
                  f"sign of a zero differs at {int((small & (np.signbit(got) != np.signbit(want)) & (want == 0)).sum())}; beyond 1024: {u.size} arguments, max {int(u.max())} ulp")
            assert not bad.any(), (name, x[bad][:8], got[bad][:8], want[bad][:8], int(bad.sum()))
            assert (_ulp_distance(got[small & hard], want[small & hard]) <= 1).all()
            assert u.max() <= 2, (name, int(u.max()))
    print(f"[surf libm] hard sine / cosine arguments: {n_hard} of {2 * int(small.sum())}")


# ------------------------------------------------------------------ small inputs the exact checker makes worth having
@gpu_mark
def test_irregular_masks(gpu, oracle):
    """Every other mask of the suite is a rectangle, and mask_check reads a 9-cell box of the mask integral per candidate: a seeded blob
    region with the values 0, 1, 7 and 255; single-pixel holes on and beside the strongest maxima (nothing may be lost); a mask that
    leaves octave 0 without a candidate (the compaction's running count crosses an empty octave).  128 x 192, 3 octaves."""
    small = S.small_frame()
    n = {}
    for tag, mask in (("blob", S.blob_mask()), ("holes", S.holes_mask(oracle)), ("octave 0 emptied", S.octave0_emptying_mask(oracle))):
        ref, _ = _run(gpu, oracle, small, f"mask: {tag}", 50.0, 3, 2, mask=mask)
        n[tag] = ref["n"]
        assert ref["n"] >= 5 and (tag != "octave 0 emptied" or (ref["octave"] >= 1).all())
    full, _ = _run(gpu, oracle, small, "no mask", 50.0, 3, 2)
    assert n["blob"] < n["holes"] == full["n"]


@gpu_mark
def test_an_octave_without_candidates_before_one_with(gpu, oracle):
    """Five Gaussian blobs: octave 0 yields no candidate, octave 1 the features -- the candidate and feature counts the octaves share
    must carry over an octave that adds nothing.  Sigma 5 with 2 layers (all-octave plan), sigma 8.5 with 5 layers (per-octave plan);
    tests/test_surf_exact_ref.py asserts the candidate counts per octave on the oracle."""
    kw = S.LARGE_BLOB_PARAMS
    for sigma, layers in S.LARGE_BLOB_CASES:
        ref, _ = _run(gpu, oracle, S.large_blob_frame(sigma), f"large blobs, sigma {sigma}, {layers} layers", kw["hessian_threshold"], kw["n_octaves"], layers)
        assert ref["n"] >= 4 and (ref["octave"] >= 1).all()


@gpu_mark
@pytest.mark.parametrize("shape,octaves,layers,ratio", S.OVERFLOW_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_candidate_list_and_feature_list_overflow_in_one_call(gpu, oracle, shape, octaves, layers, ratio):
    """A tiny keypointsRatio on a busy texture: octaves 0 and 1 each find more maxima than maxCandidates = 1.5 maxFeatures holds and
    the survivors more than maxFeatures (tests/test_surf_exact_ref.py asserts both on the oracle): the lists keep the first entries in
    scan order, on the all-octave plan (4 octaves x 2 layers) and on the per-octave plan (3 x 5)."""
    ref, _ = _run(gpu, oracle, S.busy_frame(*shape), f"both overflows {octaves}/{layers}", 20.0, octaves, layers, ratio=ratio)
    assert ref["n"] == int(np.float32(shape[0] * shape[1]) * np.float32(ratio)) >= 19


@gpu_mark
@pytest.mark.parametrize("count", S.GRID_WALK_COUNTS)
def test_grid_walk_tails_with_provided_keypoints(gpu, oracle, count):
    """Provided keypoints, so the count is exact: 1, 3, 4 and 5 features are one wave short of, exactly and one over the orientation
    kernel's 4-wave workgroup; 4099 is no multiple of 4 and more than the 4096 workgroups of the fixed descriptor grid.  Sizes from both
    sides of the staged-kernel switch (s = 5 at size 37.5)."""
    import torch
    from opencv_contrib_amd import cuda
    img = S.texture_200x260()
    x, y, size = S.grid_walk_keypoints(count)
    rows = S.kp_rows(x, y, size, 123.0)
    kp = np.zeros((7, count), np.float32)
    kp[0], kp[1], kp[4], kp[5] = x, y, size, 123.0
    kp.view(np.int32)[2] = 1
    for extended in (False, True):
        k2, d = cuda.SURF_CUDA.create(100.0, 4, 2, extended, 0.05, False).detectWithDescriptors(T(img, gpu), None, torch.from_numpy(kp.copy()).to(gpu), True)
        st = assert_surf_equals(oracle, img, S.kp_dict(N(k2)), N(d), rows, extended=extended, upright=False, provided_angle=123.0, what=f"{count} provided")
        assert st["sampled"] == count


@gpu_mark
def test_descriptor_grid_walk_with_the_count_on_the_device(gpu, oracle):
    """600 x 900 texture, threshold 20: between 4096 and 8192 features, no multiple of 4096 or 4 -- with the count on the device the
    descriptor kernels walk the features with a fixed grid of 4096 workgroups (16 per CU) and the last sweep is partial."""
    kw = S.GRID_WALK_PARAMS
    ref, _ = _run(gpu, oracle, S.busy_frame(*S.GRID_WALK_SHAPE), "descriptor grid walk", kw["hessian_threshold"], kw["n_octaves"], 2, ratio=kw["keypoints_ratio"])
    assert 4096 < ref["n"] < 8192
