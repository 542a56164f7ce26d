"""The host side of cv::cuda::ORB, checked without a GPU: the plan (tests/cpp/orb_plan_test.cpp, a stand-alone program under the host
sanitizers) and its host tables -- cv::RNG and the patterns, the quotas, u_max -- against the NumPy restatement."""
import os
import subprocess

import numpy as np
import pytest

import orb_numpy_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opencv_contrib_amd", "csrc")


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("orb_plan") / "orb_plan_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "orb_plan_test.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _ints(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return [int(v) for v in r.stdout.split()]


def test_plan_host_arithmetic(plan_exe):
    """validator edges, the empty inner rectangle, R, capacities, the scratch layout, the launch list and its single read-back, for
    detection and for provided keypoints.  Plain C++ with its own main; nothing here is loaded into Python."""
    r = subprocess.run([plan_exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "orb_plan_test: ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("patch,wta", [(31, 2), (31, 3), (31, 4), (29, 2), (9, 3), (2, 4)])
def test_generated_pattern_equals_the_restatement(plan_exe, patch, wta):
    """makeRandomPattern and initializeOrbPattern over cv::RNG, orb.cpp:431-477"""
    want = R.make_pattern(patch, wta)
    assert want.shape == (2, 512 if wta == 2 else 128 * wta)
    assert _ints(plan_exe, "pattern", patch, wta) == want.reshape(-1).tolist()


@pytest.mark.parametrize("n,s,L", [(500, 1.2, 8), (4000, 1.2, 8), (60, 1.2, 2), (7, 1.5, 3), (0, 1.2, 3), (1000, 2.0, 1)])
def test_quotas_equal_the_restatement(plan_exe, n, s, L):
    q = R.features_per_level(n, s, L)
    assert sum(q) == n and _ints(plan_exe, "quota", n, s, L) == q


@pytest.mark.parametrize("patch", [2, 3, 9, 29, 31, 59])
def test_u_max_equals_the_restatement(plan_exe, patch):
    assert _ints(plan_exe, "umax", patch) == R.u_max(patch)


def test_u_max_31_is_the_known_disc():
    """the table every ORB implementation derives for a 31-pixel patch"""
    assert R.u_max(31) == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3, 0]


def test_restated_cull_is_the_total_order():
    """response descending, index ascending among equals, -0 == +0, the stored bits kept"""
    resp = np.array([1.0, 3.0, -0.0, 3.0, 0.0, 2.0, 3.0, -1.0], np.float32)
    loc = np.arange(16, dtype=np.int16).reshape(8, 2)
    l, r = R.cull(loc, resp, 5)
    assert l[:, 0].tolist() == [2, 6, 12, 10, 0] and r.tolist() == [3, 3, 3, 2, 1]
    l, r = R.cull(loc, resp, 7)
    assert l[:, 0].tolist() == [2, 6, 12, 10, 0, 4, 8] and np.signbit(r[5]) and not np.signbit(r[6])
    assert R.cull(loc, resp, 8)[0] is loc and len(R.cull(loc, resp, 0)[1]) == 0


def test_tie_sensitive_bits_at_30_degrees():
    """sin(30 deg) rounds to an f32 next to 1/2: products such as 2 * sina + ... land next to a half-integer for some test points, and only
    the bits that read such a point are marked; at 0 degrees sina = 0 and cosa = 1 leave integer sums and one ulp moves no coordinate
    across a half"""
    pat = R.make_pattern(31, 2)
    loc = np.array([[40, 40]], np.int16)
    m30 = R.tie_sensitive_bits(loc, np.array([30.0], np.float32), pat, 2)
    m0 = R.tie_sensitive_bits(loc, np.array([0.0], np.float32), pat, 2)
    assert m30.shape == m0.shape == (1, 32, 8)
    assert not m0.any()
    assert 0 < m30.sum() <= 0.25 * m30.size
    # a marked bit really has a sample point within one ulp's reach of a half-integer
    sina, cosa = R.sincos(np.array([30.0], np.float32))
    px, py = pat[0].astype(np.float64), pat[1].astype(np.float64)
    fy, fx = px * float(sina[0]) + py * float(cosa[0]), px * float(cosa[0]) - py * float(sina[0])
    near = (np.abs(fy - np.floor(fy) - 0.5) < 1e-4) | (np.abs(fx - np.floor(fx) - 0.5) < 1e-4)
    assert (near.reshape(32, 8, 2).any(2) >= m30[0]).all()


def test_restated_blur_equals_the_pinned_gaussian_filter():
    """the 7 x 7 sigma 2 Gaussian against the BTV-L1 restatement's separable filter, which is held to the reference's own row and column
    kernels: the same taps, the same f32 intermediate, then ORB's saturating round to 8 bits"""
    import btvl1_numpy_ref as B
    import fast_numpy_ref as FR
    np.testing.assert_array_equal(R.gaussian_taps(), B.gaussian_kernel(7, 2.0))
    for rows, cols in ((40, 57), (7, 9)):
        img = FR.synth_image(rows, cols, 5, "noise")
        want = np.clip(np.rint(B.gauss_separable(img.astype(np.float32), B.gaussian_kernel(7, 2.0))), 0, 255).astype(np.uint8)
        np.testing.assert_array_equal(R.blur(img), want)
