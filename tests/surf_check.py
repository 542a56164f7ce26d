"""The one criterion every whole-class SURF comparison goes through (tests/test_surf.py, test_surf_provided.py, test_golden.py,
test_ref_class_gpu.py, test_baseline_sizes.py), and the inputs those tests send through it.

The HIP kernels and the oracle perform the same binary32 / binary64 operations in the same order (the library is built without
contraction and fast math) but for three libm calls: atan2f in the orientation (113 samples and the final direction) and the sine /
cosine of the descriptor's direction.  So everything is compared bit for bit against an oracle that is exact about those calls
(oracle.surf_orientation_candidates, oracle.surf_descriptors(rounded=True)):

  * x, y, laplacian, octave, size, hessian: equal int32 bit patterns, in order;
  * angle: within ANGLE_BOUND_DEG = 2^-13 degrees (circular) of one of the feature's candidate directions.  The bound is what an atan2f
    within 2 ulp of the correctly rounded value (measured: tests/test_surf.py::test_device_atan2f_is_within_two_ulp) leaves of the final
    direction -- 2 ulp of a value in [4, 8) rad = 1.8 * 2^-15 deg, the + 2 pi add 0.46 * 2^-15, the degree multiply 0.5 * 2^-15, the
    360 - angle subtraction and the candidate's own roundings up to 2^-15 more: < 4 * 2^-15.  The candidates are the directions the
    window search gives under both roundings of every sample whose angle lies within that bound of a half-integer (at most 3 such
    samples per feature; the share of such features per input is capped by tests/test_surf_exact_ref.py);
  * descriptors: the rounded-mode oracle evaluated AT THE HIP ANGLE equals the HIP descriptor in every bit (NaN on both sides, 0 / 0 of
    a constant patch, agrees).  A `hard` sine / cosine (within 2^-16 ulp of a rounding boundary) admits its neighbouring rounding.

MI355X: in every comparison of the suite every angle matched the candidate with no rounding flipped (0 matched by a flipped one), at most
2^-15 degrees away, 83 .. 91 % of them bit-equal; no descriptor differed; 1 hard direction (600 x 900 texture, 5517 features), rounded as
the long double rounds.
"""
import functools
import glob
import json
import os

import numpy as np

from opencv_contrib_amd import synth

ANGLE_BOUND_DEG = 2.0 ** -13
DETECTOR_ROWS = ("x", "y", "laplacian", "octave", "size", "hessian")


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def circ(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return np.minimum(d, 360.0 - d)


def rows_equal(a, b):
    """per row: every value equal in its bits, or NaN on both sides"""
    return ((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all(1)


def assert_surf_equals(oracle, img, kp_hip, desc_hip, ref, *, extended, upright, provided_angle=None, what=""):
    """kp_hip: the dict of SURF_CUDA.downloadKeypoints; desc_hip: (n, 64 | 128) float32, or None after a bare detect(); ref: the dict
    of oracle.surf_detect_describe (only its detector rows are read), or the caller's own rows for provided keypoints.
    provided_angle: the ANGLE row a caller provided (it survives where the kernel must not write); None after a detection, whose
    matrix starts zeroed.  Returns the printed counts."""
    n = len(ref["x"])
    assert kp_hip["x"].shape[0] == n, (what, kp_hip["x"].shape[0], n)
    for k in DETECTOR_ROWS:
        np.testing.assert_array_equal(bits(kp_hip[k]), bits(np.asarray(ref[k], kp_hip[k].dtype)), err_msg=f"{what}: row {k}")
    x, y, size, ang = kp_hip["x"], kp_hip["y"], kp_hip["size"], np.ascontiguousarray(kp_hip["angle"], np.float32)
    kept = np.zeros(n, np.float32) if provided_angle is None else np.broadcast_to(np.asarray(provided_angle, np.float32), (n,))
    stats = {"n": n, "early": 0, "all_outside": 0, "flipped": 0, "angle_bit_equal": n, "hard": 0, "hard_alt": 0}
    if upright:
        # detectKeypoints' upright fill (360 - 90); with provided keypoints the upright path writes nothing
        want = kept if provided_angle is not None else np.full(n, 270.0, np.float32)
        np.testing.assert_array_equal(bits(ang), bits(want), err_msg=f"{what}: upright angle")
    else:
        c = oracle.surf_orientation_candidates(img, x, y, size, ANGLE_BOUND_DEG, want_yx=False)
        st, cand, nc, und = c["status"], c["candidates"], c["n_candidates"], c["undecided"]
        early, allout, rest = st == -1, st == 0, st > 0
        np.testing.assert_array_equal(bits(ang[early]), bits(kept[early]), err_msg=f"{what}: angle where the kernel must not write")
        np.testing.assert_array_equal(bits(ang[allout]), bits(np.zeros(int(allout.sum()), np.float32)), err_msg=f"{what}: all samples outside")
        assert int((und > oracle.SURF_MAX_UNDECIDED).sum()) == 0, (what, "features with too many undecided samples", np.flatnonzero(und > 3))
        with np.errstate(invalid="ignore"):
            d = np.where(np.isnan(cand), np.inf, circ(ang[:, None], cand))          # (n, 8)
        near = d <= ANGLE_BOUND_DEG
        bad = np.flatnonzero(rest & ~near.any(1))
        flipped = rest & ~near[:, 0] & near.any(1)
        biteq = rest & (bits(ang)[:, None] == bits(cand)).any(1)
        stats.update(early=int(early.sum()), all_outside=int(allout.sum()), flipped=int(flipped.sum()), angle_bit_equal=int(biteq.sum()),
                     sampled=int(rest.sum()), undecided_features=int((und[rest] > 0).sum()))
        print(f"[surf check] {what}: {n} features, {stats['early']} unwritten, {stats['all_outside']} all outside; of {stats['sampled']} angles "
              f"{int((rest & near[:, 0]).sum())} match the no-flip candidate, {stats['flipped']} a flipped one, {stats['angle_bit_equal']} bit-equal; "
              f"{stats['undecided_features']} features with undecided samples; worst {float(d.min(1)[rest].max()) if rest.any() else 0.0:.3g} deg")
        assert bad.size == 0, (what, [dict(feature=int(k), x=float(x[k]), y=float(y[k]), size=float(size[k]), hip=float(ang[k]),
                                           candidates=cand[k, :nc[k]].tolist(), undecided=int(und[k])) for k in bad[:8]], int(bad.size))
    if desc_hip is not None:
        desc_hip = np.ascontiguousarray(desc_hip, np.float32)
        rd, hard, alts = oracle.surf_descriptors(img, x, y, size, ang, extended, rounded=True)
        assert desc_hip.shape == rd.shape, (what, desc_hip.shape, rd.shape)
        ok = rows_equal(desc_hip, rd)
        for k in np.flatnonzero(~ok & hard):
            if rows_equal(np.broadcast_to(desc_hip[k], alts[int(k)].shape), alts[int(k)]).any():
                ok[k] = True
                stats["hard_alt"] += 1
        stats["hard"] = int(hard.sum())
        with np.errstate(invalid="ignore"):
            dd = np.nan_to_num(np.abs(desc_hip.astype(np.float64) - rd), nan=0.0).max(1) if n else np.zeros(0)
        print(f"[surf check] {what}: descriptors at the HIP angles: {int((~ok).sum())} of {n} features differ (max |diff| "
              f"{float(dd.max()) if n else 0.0:.3g}), {stats['hard']} hard directions, {stats['hard_alt']} matched by a neighbouring rounding")
        bad = np.flatnonzero(~ok)
        assert bad.size == 0, (what, [dict(feature=int(k), x=float(x[k]), y=float(y[k]), size=float(size[k]), angle=float(ang[k]),
                                           max_diff=float(dd[k])) for k in bad[:8]], int(bad.size))
    return stats


def kp_rows(x, y, size, angle=0.0):
    """the rows of provided keypoints as assert_surf_equals reads them (uploadKeypoints: LAPLACIAN int 1, OCTAVE and HESSIAN 0)"""
    n = len(x)
    return {"n": n, "x": np.asarray(x, np.float32), "y": np.asarray(y, np.float32), "laplacian": np.ones(n, np.int32), "octave": np.zeros(n, np.int32),
            "size": np.asarray(size, np.float32), "angle": np.broadcast_to(np.asarray(angle, np.float32), (n,)).copy(), "hessian": np.zeros(n, np.float32)}


def kp_dict(k):
    """a 7 x n keypoint matrix (host) as the dict of SURF_CUDA.downloadKeypoints"""
    k = np.ascontiguousarray(k, np.float32)
    ki = k.view(np.int32)
    return {"x": k[0].copy(), "y": k[1].copy(), "laplacian": ki[2].copy(), "octave": ki[3].copy(), "size": k[4].copy(), "angle": k[5].copy(),
            "hessian": k[6].copy()}


# ------------------------------------------------------------------ the inputs of the GPU tests that go through assert_surf_equals
# (tests/test_surf_exact_ref.py holds the share of their features with undecided samples under a cap, on the CPU)
GRID = [(100, 4, 2, False, False), (500, 3, 3, True, False), (1000, 4, 2, False, True), (100, 3, 2, True, True)]   # thr, octaves, layers, extended, upright
PLANS = [(3, 5), (4, 4), (2, 1)]
# Small frames at the edges of octave 0's tiles (the last lines of tools/surf_digest.py): widths one sample either side of two / three
# 62-column tiles (maxima flagged in the det kernel) and 64-column tiles, heights around the 14- / 16-row tiles, rows of the polyphase
# planes that cross a 64-word alignment; (3, 4) has too many layers for the LDS tiles.  (rows, cols), octaves, layers
TILE_EDGE_CASES = (((98, 124), 2, 2), ((112, 127), 2, 2), ((113, 128), 3, 2), ((114, 129), 2, 3), ((127, 187), 2, 2), ((128, 192), 3, 4),
                   ((129, 193), 3, 2))
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def random_surf_configs():
    rng = np.random.default_rng(int(os.environ.get("MIFLOW_SWEEP_SEED", "90210")))
    out = []
    for k in range(int(os.environ.get("MIFLOW_SWEEP_N", "12"))):
        out.append(dict(shape=(int(rng.integers(120, 520)), int(rng.integers(160, 700))), seed=int(rng.integers(1, 10 ** 6)),
                        thr=float((50.0, 100.0, 400.0, 1500.0)[int(rng.integers(4))]), octaves=int(rng.integers(2, 5)), layers=int(rng.integers(1, 4)),
                        extended=bool(rng.integers(2)), upright=bool(rng.integers(2))))
    return out


def rect_mask(shape, r0, r1, c0, c1, value):
    m = np.zeros(shape, np.uint8)
    m[r0:r1, c0:c1] = value
    return m


@functools.lru_cache(maxsize=None)
def texture_200x260():
    return np.rint(synth.texture(200, 260, 11, 2.0)).astype(np.uint8)


# ---- small inputs the exact checker makes worth having (tests/test_surf.py, "irregular masks" ... "both overflows")
SMALL = (128, 192)


@functools.lru_cache(maxsize=None)
def small_frame():
    return synth.blob_image(*SMALL, seed=65)


@functools.lru_cache(maxsize=None)
def blob_mask():
    """an irregular region (a thresholded smooth field) with the values 1, 7 and 255 inside, 0 outside: cuda::min(mask, 1) must treat
    every non-zero value alike, and mask_check's 9-cell box crosses its boundary at every slope"""
    rng = np.random.default_rng(62)
    f = synth.texture(SMALL[0], SMALL[1], 63, 12.0)
    inside = f > np.median(f)
    return np.where(inside, rng.choice(np.array([1, 7, 255], np.uint8), SMALL), 0).astype(np.uint8)


def holes_mask(oracle):
    """all ones but single-pixel holes on and beside the strongest maxima: a hole moves no box mean below 0.5, nothing may be lost"""
    r = oracle.surf_detect_describe(small_frame(), oracle.surf_params(hessian_threshold=50.0, n_octaves=3, keypoints_ratio=0.05), want_desc=False)
    m = np.full(SMALL, 255, np.uint8)
    for k in np.argsort(-r["hessian"])[:12]:
        yy, xx = int(round(float(r["y"][k]))), int(round(float(r["x"][k])))
        for dy, dx in ((0, 0), (0, 2), (-2, -1)):
            m[min(max(yy + dy, 0), SMALL[0] - 1), min(max(xx + dx, 0), SMALL[1] - 1)] = 0
    return m


def octave0_emptying_mask(oracle):
    """zero boxes over every octave-0 feature, repeated until the oracle finds none there: octave 0 contributes nothing, octave 1 does"""
    p = oracle.surf_params(hessian_threshold=50.0, n_octaves=3, keypoints_ratio=0.05)
    m = np.full(SMALL, 255, np.uint8)
    for _ in range(20):
        r = oracle.surf_detect_describe(small_frame(), p, mask=m, want_desc=False)
        sel = np.flatnonzero(r["octave"] == 0)
        if sel.size == 0:
            break
        for k in sel:
            h = int(r["size"][k]) // 2 + 3          # the feature's whole filter box: its mean falls below 0.5
            yy, xx = int(r["y"][k]), int(r["x"][k])
            m[max(yy - h, 0): yy + h + 1, max(xx - h, 0): xx + h + 1] = 0
    return m


@functools.lru_cache(maxsize=None)
def large_blob_frame(sigma=5.0):
    """five Gaussian blobs of sigma about 5: their response grows up to the 27 / 39 px filters, so octave 0 with 2 layers (9 .. 27 px, maxima
    in its 15 and 21 px layers only) has no candidate at all and octave 1 has five; sigma 8.5 does the same to octave 0 with 5 layers
    (9 .. 45 px) -- the per-octave plan"""
    yy, xx = np.mgrid[0:SMALL[0], 0:SMALL[1]].astype(np.float64)
    f = np.zeros(SMALL)
    for cy, cx, ds, amp in ((40, 50, 0.0, 200), (84, 120, 0.7, -150), (50, 150, -0.4, 180), (95, 40, 0.3, 160), (30, 100, 0.0, -170)):
        sg = sigma + ds
        f += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sg * sg))
    return np.clip(np.rint(90 + f), 0, 255).astype(np.uint8)


LARGE_BLOB_PARAMS = dict(hessian_threshold=500.0, n_octaves=3, n_octave_layers=2, keypoints_ratio=0.05)
LARGE_BLOB_CASES = ((5.0, 2), (8.5, 5))     # sigma, nOctaveLayers


@functools.lru_cache(maxsize=None)
def busy_frame(rows, cols):
    return np.rint(synth.texture(rows, cols, 72, 2.0)).astype(np.uint8)


# (rows, cols), octaves, layers, keypointsRatio: the all-octave and the per-octave plan, both lists overflowing in one call
OVERFLOW_CASES = (((192, 256), 4, 2, 0.0005), ((128, 192), 3, 5, 0.0008))


# more features than the 4096 workgroups of the descriptor launch's fixed grid on the MI355X (16 per CU), and no multiple of it
GRID_WALK_SHAPE = (600, 900)
GRID_WALK_PARAMS = dict(hessian_threshold=20.0, n_octaves=3, keypoints_ratio=0.05)


GRID_WALK_COUNTS = (1, 3, 4, 5, 4099)


def grid_walk_keypoints(count):
    """-> (x, y, size) of `count` provided keypoints on texture_200x260(), sizes from both sides of the staged-kernel switch (s = 5 at 37.5)"""
    rng = np.random.default_rng(550 + count)   # (a seed at which the oracle alone finds no undecided sample among the 1 .. 5 keypoints)
    x, y = rng.uniform(20, 240, count).astype(np.float32), rng.uniform(20, 180, count).astype(np.float32)
    return x, y, rng.choice(np.float32([9, 15.5, 24, 37.4, 37.5, 48, 60]), count).astype(np.float32)


def candidates_per_octave(oracle, img, n_octaves, n_octave_layers, thr, mask=None):
    """the number of maxima icvFindMaximaInLayer finds per octave, uncapped (oracle.lib().orc_surf_find_maxima)"""
    S = oracle.surf_integral(img)
    M = oracle.surf_integral(np.minimum(mask, 1)) if mask is not None else None
    rows, cols = img.shape
    cand = np.zeros(4 * rows * cols, np.int32)
    out = []
    for o in range(n_octaves):
        det, tr = oracle.surf_det_trace(S, o, n_octave_layers)
        out.append(int(oracle.lib().orc_surf_find_maxima(det.reshape(-1), tr.reshape(-1), M.ctypes.data if M is not None else None, rows, cols, o,
                                                          n_octave_layers, thr, rows * cols, cand)))
    return out


def helper_inputs(oracle):
    """-> [(tag, image, surf_params keywords, mask | None)]: every committed oriented (not upright) detector input the GPU tests send
    through assert_surf_equals, the 4K frame of tests/test_baseline_sizes.py excepted for its time.  tag = "test case" or
    "test case|frame" where one test case walks several frames."""
    out = []
    for thr, o, l, e, u in GRID:
        if not u:
            out.append((f"grid {thr}/{o}/{l}", synth.blob_image(300, 400, seed=11), dict(hessian_threshold=thr, n_octaves=o, n_octave_layers=l, keypoints_ratio=0.05), None))
    for o, l in PLANS + [(2, 2)]:
        out.append((f"plan {o}/{l}", synth.blob_image(300, 400, seed=21), dict(hessian_threshold=100.0, n_octaves=o, n_octave_layers=l, keypoints_ratio=0.05), None))
    for shape, o, l in TILE_EDGE_CASES:
        out.append((f"tile edge|{shape}", synth.blob_image(*shape, seed=41), dict(hessian_threshold=50.0, n_octaves=o, n_octave_layers=l, keypoints_ratio=0.05), None))
    img13 = synth.blob_image(260, 330, seed=13)
    out.append(("mask rect", img13, dict(hessian_threshold=200, keypoints_ratio=0.05), rect_mask(img13.shape, 40, 200, 30, 220, 7)))
    out.append(("overflow 0.0004", img13, dict(hessian_threshold=50, keypoints_ratio=0.0004), None))
    out.append(("provided after detect", img13, dict(hessian_threshold=200, keypoints_ratio=0.05), None))
    for c in random_surf_configs():
        if not c["upright"]:
            out.append((f"sweep {c['shape']} seed {c['seed']}", synth.blob_image(*c["shape"], seed=c["seed"]),
                        dict(hessian_threshold=c["thr"], n_octaves=c["octaves"], n_octave_layers=c["layers"], keypoints_ratio=0.05), None))
    for path in sorted(glob.glob(os.path.join(GOLDEN_DIR, "surf_*.npz"))):
        z = np.load(path)
        kw = json.loads(str(z["params"]))
        if not kw.get("upright", 0):
            out.append((os.path.basename(path), z["img"], {k: v for k, v in kw.items() if k not in ("extended", "upright")}, None))
    out.append(("texture 200x260", texture_200x260(), dict(hessian_threshold=50.0), None))
    p3 = dict(hessian_threshold=50.0, n_octaves=3, keypoints_ratio=0.05)
    out.append(("irregular masks|blob", small_frame(), p3, blob_mask()))
    out.append(("irregular masks|holes", small_frame(), p3, holes_mask(oracle)))
    out.append(("irregular masks|octave 0 emptied", small_frame(), p3, octave0_emptying_mask(oracle)))
    for sigma, l in LARGE_BLOB_CASES:
        out.append((f"large blobs|{sigma}", large_blob_frame(sigma), dict(LARGE_BLOB_PARAMS, n_octave_layers=l), None))
    for shape, o, l, ratio in OVERFLOW_CASES:
        out.append((f"both overflows {o}/{l}", busy_frame(*shape), dict(hessian_threshold=20.0, n_octaves=o, n_octave_layers=l, keypoints_ratio=ratio), None))
    out.append(("descriptor grid walk", busy_frame(*GRID_WALK_SHAPE), GRID_WALK_PARAMS, None))
    return out
