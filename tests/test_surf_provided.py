"""SURF_CUDA with PROVIDED keypoints (operator()(img, mask, keypoints, descriptors, useProvidedKeypoints = true), surf.cuda.cpp:380-397):
the HIP orientation and descriptor kernels against the oracle, which tests/test_ref_pin_cuda.py pins bit for bit on the reference's own
kernels for provided keypoints.  tests/test_surf.py compares HIP with the oracle only on keypoints the detector produced (size >= 9,
a filter margin inside the frame, angles of the same run); a caller's keypoints reach code no detected keypoint does:

  * LinearFilter (s = size * 1.2 / 9 <= 1) and the `s > 1` switch at s == 1.0f exactly (size 7.5);
  * win_get's clamp for windows partly or wholly outside the image, the per-sample bounds test of the orientation;
  * the orientation's early return (2 * rn(2 s) > rows + 1 or cols + 1: the caller's ANGLE survives);
  * the 360-degree fold of the descriptor's direction;
  * both edges of the staged-kernel predicate (s >= 5; one patch row inside the 48 KB tile: s < 46.7);
  * pitched images, masks and keypoint matrices; one handle across shapes and keypointsRatio; mi_surf_detect_batch.

What is held to what (tests/surf_check.py has the reasoning), every feature of every group:
  * descriptors at ANY angle: EQUAL IN EVERY BIT to the oracle's descriptors with the sine and cosine of the direction correctly
    rounded (oracle.surf_descriptors(rounded=True); the kernels' sincos_rounded is correctly rounded, the host's sinf / cosf are an ulp
    off at 2.6 % of the directions -- at ANGLE 0 / 360 the two modes of the oracle coincide);
  * orientation: within 2^-13 degrees (circular) of a candidate direction of oracle.surf_orientation_candidates; bit-exact where the
    kernel must not write (123.0 survives) and where every sample lies outside the image (+0.0); the descriptors of the same call
    bit-equal to the rounded-mode oracle AT THE HIP ANGLE.

Measured on the MI355X: see the docstrings of the tests.  The oracle's results are computed once per group.
"""
import functools
import os
import sys

import numpy as np
import pytest

from opencv_contrib_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import surf_check as S  # noqa: E402

ROWS, COLS = 96, 131          # small, odd width
N_KP = 240                    # keypoints per group
GROUPS = ("linear", "switch", "global", "stage_edge", "tile_edge", "border", "outside")
SIZE_NEXT_7_5 = float(np.nextafter(np.float32(7.5), np.float32(8.0)))
GROUP_SIZES = {
    "linear": (4, 5, 6, 7, 7.5),                          # s <= 1: LinearFilter
    "switch": (7.5, SIZE_NEXT_7_5, 7.6, 9),               # s == 1.0f, the next s above it, ...
    "global": None,                                       # uniform in [9, 37.4): 1 < s < 5, the global-memory patch kernel
    "stage_edge": (37.4, 37.5, 37.6, 60, 133),            # s == 5.0f at 37.5: the staged kernel from there on
    "tile_edge": (337.5, 345, 350, 352.5, 400, 700),      # s = 45, 46, 46.67 (staged) | 47, 53.3, 93.3 (beyond the 48 KB tile: global)
    "border": (4, 7.5, 15, 30, 60),
    "outside": (4, 12, 30),
}
SPECIAL_ANGLES = (90.0, 180.0, 270.0, float(np.nextafter(np.float32(360), np.float32(0))))


def T(a, dev):
    import torch
    return torch.from_numpy(np.array(a)).to(dev)   # (a copy: the shared inputs are read-only)


def N(t):
    return t.detach().cpu().numpy()


def cell_side(size):
    """s of surf.cu:545,748 in its own float arithmetic."""
    return np.asarray(size, np.float32) * np.float32(1.2) / np.float32(9.0)


@functools.lru_cache(maxsize=None)
def image():
    img = np.rint(synth.texture(ROWS, COLS, 11, 2.0)).astype(np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def group(name):
    """-> (x, y, size) float32, N_KP keypoints, seeded per group; every size of the group occurs in both halves of the list."""
    rng = np.random.default_rng(1000 + GROUPS.index(name))
    n = N_KP
    x, y = rng.uniform(1, COLS - 2, n), rng.uniform(1, ROWS - 2, n)
    sizes = GROUP_SIZES[name]
    size = rng.uniform(9, 37.4, n) if sizes is None else np.array([sizes[i % len(sizes)] for i in range(n)], np.float64)
    if name in ("border", "outside"):
        # which edge or corner: (-1 | 0 | +1) per axis = near the low edge | anywhere along it | near the high edge, never (0, 0)
        sides = [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1) if (a, b) != (0, 0)]
        for i in range(n):
            a, b = sides[i % 8]
            for axis, side, last in ((x, a, COLS - 1), (y, b, ROWS - 1)):
                if name == "border":      # within 2 px of the edge, either side of it
                    if side:
                        axis[i] = (0 if side < 0 else last) + rng.uniform(-2, 2)
                else:                     # up to 40 px beyond it
                    if side:
                        axis[i] = -rng.uniform(0, 40) if side < 0 else last + rng.uniform(0, 40)
        if name == "border":
            exact = [(0, 0), (COLS - 1, 0), (0, ROWS - 1), (COLS - 1, ROWS - 1), (0, 40.25), (60.5, 0), (COLS - 1, 47.75), (70.5, ROWS - 1),
                     (0.5, 0.5), (COLS - 1.5, ROWS - 0.5), (-0.25, 33), (77, ROWS - 0.75)]
            for k, (ex, ey) in enumerate(exact * 5):      # 60 keypoints: every exact position at every size of the group
                x[k], y[k] = ex, ey
                size[k] = sizes[(k // len(exact)) % len(sizes)]
        else:
            for k in range(3):                            # far outside: every texel read clamps to the corner pixel
                x[k], y[k], size[k] = -500, -500, sizes[k]
    out = tuple(np.asarray(v, np.float32) for v in (x, y, size))
    for v in out:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def angles(name, mode):
    """mode "fold": 0 for one half of the group, 360 for the other (both fold to direction 0); "any": uniform in [0, 360) with
    the multiples of 90 and the last float below 360 among them."""
    if mode == "fold":
        a = np.where(np.arange(N_KP) < N_KP // 2, 0.0, 360.0)
    else:
        a = np.random.default_rng(2000 + GROUPS.index(name)).uniform(0, 360, N_KP)
        a[N_KP - 2 * len(SPECIAL_ANGLES):] = SPECIAL_ANGLES * 2
    a = a.astype(np.float32)
    a.setflags(write=False)
    return a


def kp_matrix(x, y, size, angle):
    """The 7 x n keypoint matrix a caller uploads (uploadKeypoints, surf.cuda.cpp:297-317): LAPLACIAN int 1, OCTAVE and HESSIAN 0."""
    kp = np.zeros((7, len(x)), np.float32)
    kp[0], kp[1], kp[4], kp[5] = x, y, size, angle
    kp.view(np.int32)[2] = 1
    return kp


# the oracle's results are computed once per (group, angles, extended) and shared (read-only) by the tests below
@functools.lru_cache(maxsize=None)
def ref_descriptors(oracle, name, mode, extended):
    x, y, size = group(name)
    d = oracle.surf_descriptors(image(), x, y, size, angles(name, mode), extended)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def ref_descriptors_rounded(oracle, name, mode, extended):
    """-> (descriptors, hard, alternatives) with the sine / cosine correctly rounded"""
    x, y, size = group(name)
    out = oracle.surf_descriptors(image(), x, y, size, angles(name, mode), extended, rounded=True)
    out[0].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ref_orientation(oracle, name):
    """-> (angle, samples inside, descriptors at that angle) for ANGLE = 123 provided."""
    x, y, size = group(name)
    a = oracle.surf_orientation(image(), x, y, size, 123.0)
    out = (a, oracle.surf_orientation_samples(ROWS, COLS, x, y, size), oracle.surf_descriptors(image(), x, y, size, a, False))
    for v in out:
        v.setflags(write=False)
    return out


def feature_diff(a, b):
    """max |a - b| per feature; a NaN on both sides (0 / 0 of a constant patch) agrees, a NaN on one side is infinitely far."""
    both = np.isnan(a) & np.isnan(b)
    d = np.where(both, 0.0, np.abs(a.astype(np.float64) - b))
    return np.where(np.isnan(d), np.inf, d).max(1)


def circ(a, b):
    d = np.abs(a.astype(np.float64) - b)
    return np.minimum(d, 360.0 - d)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ------------------------------------------------------------------ oracle wrappers (CPU)
def test_groups_sit_where_their_names_say():
    """The float facts the groups rely on: size 7.5 gives s == 1.0f and the next float32 above it s > 1; 37.5 gives s == 5.0f;
    sizes >= 182 make grad_wav_size exceed rows + 1 = 97; the staged predicate of csrc/surf_kernels.hip flips between 350 and 352.5."""
    s = cell_side
    assert s(7.5) == 1.0 and s(SIZE_NEXT_7_5) > 1.0 and s(7.6) > 1.0
    assert (s(group("linear")[2]) <= 1).all() and (s(group("global")[2]) > 1).all() and (s(group("global")[2]) < 5).all()
    assert s(37.4) < 5.0 and s(37.5) == 5.0 and s(37.6) > 5.0
    fits = lambda z: (np.ceil(s(z)) + 3) * (np.floor(np.float32(20) * s(z) + s(z)) + 2) <= 48 * 1024
    assert [bool(fits(z)) for z in GROUP_SIZES["tile_edge"]] == [True, True, True, False, False, False]
    gws = lambda z: 2 * int(np.rint(np.float32(2) * s(z)))
    assert gws(181) <= ROWS + 1 < gws(182) and gws(133) <= ROWS + 1 and all(gws(z) > ROWS + 1 for z in GROUP_SIZES["tile_edge"])
    for name in GROUPS:
        x, y, size = group(name)
        assert len(x) == N_KP >= 200 and size.min() >= 4
        if GROUP_SIZES[name]:
            for half in (size[: N_KP // 2], size[N_KP // 2:]):
                assert set(np.float32(GROUP_SIZES[name])) == set(half)
        inside = (x >= 0) & (x <= COLS - 1) & (y >= 0) & (y <= ROWS - 1)
        assert inside.all() == (name not in ("border", "outside")) and (name != "outside" or not inside.any())
    bx, by, _ = group("border")
    assert (np.minimum(np.minimum(np.abs(bx), np.abs(bx - (COLS - 1))), np.minimum(np.abs(by), np.abs(by - (ROWS - 1)))) <= 2).all()
    assert {0.0, COLS - 1.0} <= set(bx) and {0.0, ROWS - 1.0} <= set(by) and (bx != np.rint(bx)).any()
    ox, oy, _ = group("outside")
    assert ox.min() == -500 and ox[3:].min() >= -40 and ox.max() <= COLS + 39 and oy[3:].min() >= -40 and oy.max() <= ROWS + 39


def test_wrappers_reproduce_the_pipeline_oracle(oracle):
    """surf_orientation / surf_descriptors fed the keypoints of surf_detect_describe give that call's angles and descriptors: the
    wrappers are pinned on the pipeline oracle, which tests/test_ref_pin_cuda.py pins on the reference."""
    img = synth.blob_image(240, 320, 7)
    r = oracle.surf_detect_describe(img)
    assert r["n"] > 50
    a = oracle.surf_orientation(img, r["x"], r["y"], r["size"], 0.0)
    assert a.dtype == np.float32
    np.testing.assert_array_equal(a, r["angle"])
    d = oracle.surf_descriptors(img, r["x"], r["y"], r["size"], r["angle"], False)
    assert d.shape == (r["n"], 64) and d.dtype == np.float32
    np.testing.assert_array_equal(d, r["descriptors"])
    r2 = oracle.surf_detect_describe(img, oracle.surf_params(extended=1))
    np.testing.assert_array_equal(oracle.surf_descriptors(img, r2["x"], r2["y"], r2["size"], r2["angle"], True), r2["descriptors"])


def test_orientation_wrapper_models_the_early_return_and_the_all_outside_case(oracle):
    """size 200 on the 96 x 131 image: grad_wav_size = 106 > rows + 1 = 97, the kernel returns without writing -> angle_in survives
    (the C function returns 0).  (-30, -30), size 12: all 113 samples outside -> 360 - atan2f(0, 0) folds to 0.0."""
    img = image()
    assert 2 * int(np.rint(np.float32(2) * cell_side(200))) == 106
    a = oracle.surf_orientation(img, [40.0, 60.0], [50.0, 30.0], [200.0, 200.0], [123.0, 77.5])
    np.testing.assert_array_equal(a, np.float32([123.0, 77.5]))
    np.testing.assert_array_equal(oracle.surf_orientation_samples(ROWS, COLS, [40.0, 60.0, 60.0], [50.0, 30.0, 50.0], [200.0, 200.0, 15.0]), [-1, -1, 113])
    assert oracle.surf_orientation_samples(ROWS, COLS, [-30.0], [-30.0], [12.0])[0] == 0
    b = oracle.surf_orientation(img, [-30.0], [-30.0], [12.0], 123.0)
    assert b[0] == 0.0 and not np.signbit(b[0])
    c = oracle.surf_orientation(img, [60.0], [50.0], [15.0], 123.0)     # an ordinary keypoint is computed, not passed through
    assert c[0] != 123.0 and 0 <= c[0] < 360


# ------------------------------------------------------------------ HIP vs oracle (GPU)
gpu_mark = pytest.mark.gpu


def hip_provided(gpu, kp, extended, upright, img_t=None):
    """detectWithDescriptors(..., keypoints, True) on a fresh handle (2 octaves: the image is too small for more)."""
    from opencv_contrib_amd import cuda
    alg = cuda.SURF_CUDA.create(100.0, 2, 2, extended, 0.01, upright)
    k2, d = alg.detectWithDescriptors(T(image(), gpu) if img_t is None else img_t, None, kp, True)
    return k2, d


@gpu_mark
@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("name", GROUPS)
def test_descriptors_at_direction_zero_are_bit_exact(gpu, oracle, name, extended):
    """ANGLE = 0 (first half) and 360 (second half), upright: the direction folds to 0, sincosf(0) = (0, 1) on both sides, and every
    remaining operation is the same binary32 operation in the same order -- any difference is a kernel defect.  Upright with provided
    keypoints writes nothing into the keypoint matrix.  MI355X: all 14 cases exact."""
    x, y, size = group(name)
    kp = kp_matrix(x, y, size, angles(name, "fold"))
    k2, d = hip_provided(gpu, T(kp, gpu), extended, True)
    np.testing.assert_array_equal(N(d), ref_descriptors(oracle, name, "fold", extended))
    np.testing.assert_array_equal(bits(N(k2)), bits(kp))


@gpu_mark
@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("name", GROUPS)
def test_descriptors_at_any_direction(gpu, oracle, name, extended):
    """ANGLE uniform in [0, 360) plus 90, 180, 270 and the last float below 360; upright.  Every feature's descriptor equals the oracle's
    in every bit, the oracle's sine and cosine being correctly rounded as the kernels' are (a `hard` direction admits its neighbouring
    rounding; NaN on both sides, 0 / 0 of a constant patch, agrees).
    MI355X: every feature of all 14 cases bit-equal, no hard direction.  (With the device's sincosf, which the kernels used first and
    which is an ulp off the host's at a third of the directions: 1 of 240 in stage_edge outside 1e-4, max |diff| 3.6e-4.)"""
    x, y, size = group(name)
    kp = kp_matrix(x, y, size, angles(name, "any"))
    k2, d = hip_provided(gpu, T(kp, gpu), extended, True)
    d = N(d)
    rd, hard, alts = ref_descriptors_rounded(oracle, name, "any", extended)
    ok = S.rows_equal(d, rd)
    for k in np.flatnonzero(~ok & hard):
        ok[k] = bool(S.rows_equal(np.broadcast_to(d[k], alts[int(k)].shape), alts[int(k)]).any())
    dd = feature_diff(d, rd)
    print(f"[surf provided] any direction, {name}, extended {extended}: {int((~ok).sum())} of {len(dd)} features not bit-equal, "
          f"{int(hard.sum())} hard directions, max |diff| {dd.max():.3g}")
    np.testing.assert_array_equal(bits(N(k2)), bits(kp))
    assert ok.all(), (name, np.flatnonzero(~ok)[:8], float(dd.max()))


@gpu_mark
@pytest.mark.parametrize("name", GROUPS)
def test_orientation_of_provided_keypoints(gpu, oracle, name):
    """upright = False, ANGLE = 123 provided, through tests/surf_check.py.  Where grad_wav_size exceeds rows + 1 or cols + 1 (sizes >= 182
    here: all of tile_edge) the kernel must not write: 123.0 survives bit for bit.  Where all 113 samples lie outside the image the
    result is +0.0.  Elsewhere every angle lies within 2^-13 degrees (circular) of a candidate direction of the libm-exact oracle, and
    every descriptor of the same call equals the rounded-mode oracle AT THE HIP ANGLE in every bit.  Every other row comes back
    bit-identical.
    MI355X: every angle matches the candidate with no rounding flipped, at most 2^-15 degrees away; bit-equal 209, 211, 208, 204, 218 of 240
    in linear, switch, global, stage_edge, border and 22 of the 24 sampled ones in outside (216 all outside, tile_edge 240 unwritten);
    features with undecided samples: 4 in global, 5 in stage_edge; no descriptor differs in any bit, no hard direction.
    tile_edge is the case that made the kernels round their sine and cosine correctly (sincos_rounded, csrc/surf_kernels.hip): all 240
    keypoints keep the one direction 123, their windows span 790 .. 1630 texels, and the device's sincosf gives the sine of 237 degrees
    an ulp below the host's -- every window read some other texels."""
    x, y, size = group(name)
    kp = kp_matrix(x, y, size, 123.0)
    _, samples, _ = ref_orientation(oracle, name)
    k2, d = hip_provided(gpu, T(kp, gpu), False, False)
    k2, d = N(k2), N(d)
    early, allout, rest = samples == -1, samples == 0, samples > 0
    if name == "tile_edge":
        assert early.all()
    if name == "outside":
        assert allout[:3].all() and allout.sum() > 10 and rest.sum() > 10
    st = S.assert_surf_equals(oracle, image(), S.kp_dict(k2), d, S.kp_rows(x, y, size), extended=False, upright=False, provided_angle=123.0,
                              what=f"provided, {name}")
    assert (st["early"], st["all_outside"], st["sampled"]) == (int(early.sum()), int(allout.sum()), int(rest.sum()))


@gpu_mark
@pytest.mark.parametrize("name", ["switch", "border"])
def test_pitched_image_and_keypoint_matrix(gpu, oracle, name):
    """The image as a ROI of a wider device buffer (step 160 > cols 131, an odd byte offset), the keypoint matrix as a column slice of
    a wider tensor whose other columns hold a canary: descriptors and keypoints equal the contiguous call bit for bit -- and with it the
    oracle (direction 0) -- and no canary is touched; the same with the orientation writing its row."""
    import torch
    x, y, size = group(name)
    n = len(x)
    buf = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (110, 160)).astype(np.uint8)).to(gpu)
    buf[3:99, 5:136] = T(image(), gpu)
    roi = buf[3:99, 5:136]
    assert roi.stride(0) == 160 and not roi.is_contiguous()
    for upright, ang in ((True, angles(name, "fold")), (False, np.full(n, 123.0, np.float32))):
        kp = kp_matrix(x, y, size, ang)
        wide = torch.full((7, n + 19), -777.25, dtype=torch.float32, device=gpu)
        wide[:, 7:7 + n] = T(kp, gpu)
        for extended in (False, True):
            kc, dc = hip_provided(gpu, T(kp, gpu), extended, upright)
            kpv = wide.clone()
            k2, d = hip_provided(gpu, kpv[:, 7:7 + n], extended, upright, roi)
            np.testing.assert_array_equal(N(d), N(dc))
            np.testing.assert_array_equal(bits(N(k2)), bits(N(kc)))
            assert k2.data_ptr() == kpv[:, 7:7 + n].data_ptr()
            assert bool((kpv[:, :7] == -777.25).all()) and bool((kpv[:, 7 + n:] == -777.25).all())
            if upright:
                np.testing.assert_array_equal(N(d), ref_descriptors(oracle, name, "fold", extended))
                np.testing.assert_array_equal(bits(N(k2)), bits(kp))
            else:
                assert (N(k2)[5] != 123.0).sum() > n // 2


def kp_equal(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@gpu_mark
def test_detector_on_pitched_image_and_mask(gpu):
    """detect / detectWithDescriptors on a 130 x 170 ROI of a wider buffer with a mask that is a ROI of another: bit-identical to the
    contiguous call (compared as int32: the LAPLACIAN row holds int bit patterns)."""
    import torch
    from opencv_contrib_amd import cuda
    img = synth.blob_image(130, 170, seed=17)
    mask = np.zeros_like(img); mask[10:120, 20:160] = 255; mask[50:70, 60:90] = 0
    rng = np.random.default_rng(8)
    ibuf = torch.from_numpy(rng.integers(0, 256, (141, 203)).astype(np.uint8)).to(gpu)
    mbuf = torch.from_numpy(rng.integers(0, 2, (150, 181)).astype(np.uint8) * 255).to(gpu)
    ibuf[4:134, 7:177] = T(img, gpu)
    mbuf[9:139, 3:173] = T(mask, gpu)
    iv, mv = ibuf[4:134, 7:177], mbuf[9:139, 3:173]
    mk = lambda: cuda.SURF_CUDA.create(50.0, 3, 2, False, 0.05, False)
    for m_c, m_v in ((None, None), (T(mask, gpu), mv)):
        k0 = mk().detect(T(img, gpu), m_c)
        assert k0.shape[1] > 10
        assert kp_equal(mk().detect(iv, m_v), k0)
        k1, d1 = mk().detectWithDescriptors(T(img, gpu), m_c)
        k2, d2 = mk().detectWithDescriptors(iv, m_v)
        assert kp_equal(k1, k0) and kp_equal(k2, k0) and torch.equal(d1, d2)
    assert mk().detect(T(img, gpu), T(mask, gpu)).shape[1] < mk().detect(T(img, gpu)).shape[1]


@gpu_mark
def test_one_handle_across_shapes_ratios_masks_and_layers(gpu):
    """The branches of ensure() (csrc/surf_api.cpp) that keep, re-plan or free a handle's scratch: a sequence of detectWithDescriptors
    calls on ONE handle -- another image size and back, keypointsRatio lowered (lists kept, re-planned), raised back (kept) and raised
    beyond what was allocated (re-allocated), a mask after calls without one, nOctaveLayers 2 -> 4 -> 2, releaseMemory() in the middle --
    each call bit-identical to the same call on a fresh handle."""
    import torch
    from opencv_contrib_amd import cuda
    A, B = T(synth.blob_image(300, 400, seed=23), gpu), T(synth.blob_image(130, 170, seed=29), gpu)
    mm = np.zeros((300, 400), np.uint8); mm[30:250, 50:380] = 1
    M = T(mm, gpu)
    P = dict(ratio=0.05, layers=2)
    alg = cuda.SURF_CUDA.create(100.0, 3, 2, False, 0.05, False)
    steps = [("A", A, None, {}), ("B", B, None, {}), ("A again", A, None, {}),
             ("ratio 0.01", A, None, dict(ratio=0.01)), ("ratio 0.05", A, None, dict(ratio=0.05)), ("ratio 0.08", A, None, dict(ratio=0.08)),
             ("ratio back", A, None, dict(ratio=0.05)), ("mask", A, M, {}), ("no mask", A, None, {}),
             ("layers 4", A, None, dict(layers=4)), ("layers 2", A, None, dict(layers=2)),
             ("release", A, None, dict(release=True)), ("mask after release", A, M, {}), ("B after all", B, None, {})]
    counts = {}
    for tag, img, mask, change in steps:
        if change.pop("release", False):
            alg.releaseMemory()
        P.update(change)
        alg.keypointsRatio, alg.nOctaveLayers = P["ratio"], P["layers"]
        fresh = cuda.SURF_CUDA.create(100.0, 3, P["layers"], False, P["ratio"], False)
        k0, d0 = fresh.detectWithDescriptors(img, mask)
        k1, d1 = alg.detectWithDescriptors(img, mask)
        assert k0.shape[1] > 20, tag
        assert kp_equal(k1, k0) and torch.equal(d1, d0), tag
        counts[tag] = k0.shape[1]
    assert counts["ratio 0.01"] <= 1200 and counts["mask"] < counts["A"]
    assert counts["A"] == counts["A again"] == counts["ratio back"] == counts["no mask"] == counts["layers 2"] == counts["release"]


@gpu_mark
def test_detect_batch_equals_detect_per_frame(gpu):
    """SURF_CUDA.detect_batch (mi_surf_detect_batch): three frames of different sizes through one handle, the second with a mask, the
    others with None -- each result and feature count equals detect() of that frame on a fresh handle.  A batch whose second frame is
    too small for four octaves raises MiError, and the handle still serves the next batch correctly."""
    from opencv_contrib_amd import cuda, capi
    shapes = ((300, 400), (130, 170), (200, 260))
    imgs = [T(synth.blob_image(r, c, seed=50 + i), gpu) for i, (r, c) in enumerate(shapes)]
    mm = np.zeros(shapes[1], np.uint8); mm[20:110, 15:150] = 255
    masks = [None, T(mm, gpu), None]
    mk = lambda octaves: cuda.SURF_CUDA.create(100.0, octaves, 2, False, 0.05, False)
    alg = mk(3)
    out = alg.detect_batch(imgs, masks)
    assert len(out) == 3
    for im, m, kp in zip(imgs, masks, out):
        k0 = mk(3).detect(im, m)
        assert k0.shape[1] > 10 and kp_equal(kp, k0)
    assert out[1].shape[1] < mk(3).detect(imgs[1]).shape[1]          # the mask was that of frame 1, and it was applied
    for kp, k0 in zip(alg.detect_batch(imgs), (mk(3).detect(im) for im in imgs)):   # masks = None
        assert kp_equal(kp, k0)
    with pytest.raises(capi.MiError):
        alg.detect_batch(imgs, masks[:2])
    alg4 = mk(4)
    small = T(synth.blob_image(60, 60, seed=5), gpu)
    with pytest.raises(capi.MiError):
        alg4.detect_batch([imgs[0], small, imgs[2]])
    for kp, im in zip(alg4.detect_batch([imgs[0], imgs[2]]), (imgs[0], imgs[2])):
        assert kp_equal(kp, mk(4).detect(im))
