"""HIP kernels of the CPU-class SURF stages (csrc/surfcpu_kernels.hip) against the pinned oracle and the reference's golden vectors.
The kernel logic itself is checked bit for bit on the CPU (tests/test_surfcpu_emulation.py, the same source compiled for the host);
what can differ on the device is sinf / cosf of the rotated window (1 ulp), so the tolerances are: the upright path (no libm call)
exact, orientation exact for >= 99 % of the keypoints, descriptors within 1e-4 for >= 99 %, the golden vectors within the Java tests'
EPS 1e-3.  The hand-placed tables of tests/test_surfcpu_emulation.py (there through the host build) run here through the product.
(File name: collected last.)"""
import ctypes as C

import numpy as np
import pytest

from opencv_contrib_amd import synth
from test_surfcpu_emulation import CHUNK_EDGES, HAND_PLACED, hand_frame, keypoint_rows, large_window_keypoints

pytestmark = pytest.mark.gpu


def _kp_matrix(kp):
    """oracle rows {x, y, size, angle, response, octave, class_id} -> SURF_CUDA 7 x n matrix (cuda.hpp:89-99)"""
    k = np.zeros((7, len(kp)), np.float32)
    k[0], k[1], k[4], k[5], k[6] = kp[:, 0], kp[:, 1], kp[:, 2], kp[:, 3], kp[:, 4]
    k.view(np.int32)[2] = kp[:, 6].astype(np.int32)
    k.view(np.int32)[3] = kp[:, 5].astype(np.int32)
    return k


@pytest.mark.parametrize("extended,upright", [(False, False), (True, False), (True, True)])
def test_hip_cpu_class_stages_match_the_oracle(gpu, oracle, extended, upright):
    import torch
    from opencv_contrib_amd import cuda
    img = synth.blob_image(360, 480, seed=21)
    kp = oracle.surfcpu_detect(img, 200.0, 4, 3)
    k_ref, d_ref = oracle.surfcpu_compute(img, kp, extended, upright)
    alg = cuda.SURF_CUDA.create(200.0, 4, 3, extended, 0.05, upright)
    kg, dg = alg.detectAndComputeCpuClass(torch.from_numpy(img).to(gpu), None, torch.from_numpy(_kp_matrix(kp)).to(gpu), True)
    kg, dg = kg.cpu().numpy(), dg.cpu().numpy()
    assert kg.shape[1] == len(k_ref) and dg.shape == d_ref.shape
    np.testing.assert_array_equal(kg[0], k_ref[:, 0]); np.testing.assert_array_equal(kg[4], k_ref[:, 2])
    if upright:                                                    # no libm call on this path
        np.testing.assert_array_equal(kg[5], k_ref[:, 3])
        np.testing.assert_array_equal(dg, d_ref)
        return
    assert (kg[5] == k_ref[:, 3]).mean() >= 0.99 and np.abs(kg[5] - k_ref[:, 3]).max() < 360
    ok = np.abs(dg - d_ref).max(1) <= 1e-4
    assert ok.mean() >= 0.99, (float(np.abs(dg - d_ref).max()), int((~ok).sum()))


def _product(gpu, img, kp, extended, upright):
    """The product on the oracle's keypoint rows -> host (keypoints (7, n), descriptors) of the survivors"""
    import torch
    from opencv_contrib_amd import cuda
    alg = cuda.SURF_CUDA.create(200.0, 4, 3, extended, 0.05, upright)
    kg, dg = alg.detectAndComputeCpuClass(torch.from_numpy(img).to(gpu), None, torch.from_numpy(_kp_matrix(kp)).to(gpu), True)
    return kg.cpu().numpy(), dg.cpu().numpy()


@pytest.mark.parametrize("extended", [False, True])
def test_hip_upright_is_bit_exact_on_the_hand_placed_tables(gpu, oracle, extended):
    """Upright: neither stage calls libm and the library is built without contraction, so every surviving keypoint of HAND_PLACED,
    CHUNK_EDGES (windows of exactly 256, 257, 512, 513, 768, 769 and 1024 rows: one to four chunks of the descriptor kernel's 256
    threads) and the 200 keypoints of two to four chunks equals the oracle's bit for bit: x, y, size, angle = 270, every descriptor
    float."""
    img = hand_frame()
    kp = keypoint_rows(HAND_PLACED + CHUNK_EDGES + large_window_keypoints())
    k_ref, d_ref = oracle.surfcpu_compute(img, kp, extended, True)
    assert len(k_ref) == len(kp) and (k_ref[:, 3] == 270).all()      # the upright pass erases nothing here
    kg, dg = _product(gpu, img, kp, extended, True)
    assert kg.shape[1] == len(k_ref) and dg.shape == d_ref.shape
    for row, col in ((0, 0), (1, 1), (4, 2), (5, 3)):
        np.testing.assert_array_equal(kg[row], k_ref[:, col])
    np.testing.assert_array_equal(dg, d_ref)


def test_hip_orientation_is_exact_on_the_hand_placed_tables(gpu, oracle):
    """The angle of every surviving keypoint of the three tables: fast_atan2 and the window sums call no libm function, so equality
    is expected.  Unequal angles on MI355X at the first run: 0 of 227."""
    img = hand_frame()
    kp = keypoint_rows(HAND_PLACED + CHUNK_EDGES + large_window_keypoints())
    k_ref, _ = oracle.surfcpu_compute(img, kp, False, False, want_desc=False)
    kg, _ = _product(gpu, img, kp, False, False)
    assert kg.shape[1] == len(k_ref)
    for row, col in ((0, 0), (1, 1), (4, 2)):
        np.testing.assert_array_equal(kg[row], k_ref[:, col])
    unequal = int((kg[5] != k_ref[:, 3]).sum())
    print(f"oriented: {unequal} of {len(k_ref)} angles differ from the oracle's")
    assert unequal == 0


@pytest.mark.parametrize("extended", [False, True])
def test_hip_oriented_descriptors_of_two_to_four_chunk_windows(gpu, oracle, extended):
    """200 keypoints whose windows all exceed one chunk of 256 rows, a third each in two, three and four chunks, plus CHUNK_EDGES,
    described at the ORACLE's angles (so only the descriptor kernel is under test).  The file's rule: max |diff| <= 1e-4 for
    >= 99 % of the keypoints; only a sinf / cosf ulp may explain an exception.  Observed on MI355X: 0 exceptions of 214 keypoints
    (2 keypoints not bit-equal, max |diff| 7.0e-5 for 64 floats and 4.9e-5 for 128)."""
    import torch
    from opencv_contrib_amd import cuda
    img = hand_frame()
    kp = keypoint_rows(large_window_keypoints() + CHUNK_EDGES)
    k_ref, d_ref = oracle.surfcpu_compute(img, kp, extended, False)
    assert len(k_ref) > 150
    alg = cuda.SURF_CUDA.create(200.0, 4, 3, extended, 0.05, False)
    dg = alg.cpuClassDescriptors(torch.from_numpy(img).to(gpu), torch.from_numpy(_kp_matrix(k_ref)).to(gpu)).cpu().numpy()
    diff = np.abs(dg - d_ref).max(1)
    ok = diff <= 1e-4
    print(f"oriented descriptors (extended={extended}): {int((~ok).sum())} of {len(ok)} keypoints beyond 1e-4, "
          f"{int((diff > 0).sum())} not bit-equal, max |diff| {float(diff.max()):.3e}")
    assert ok.mean() >= 0.99, (float(diff.max()), int((~ok).sum()))


SENTINEL = -12345.0


def test_hip_cpu_class_strides_through_the_c_abi(gpu, oracle):
    """mi_surfcpu_orientation on a keypoint matrix of more columns than n (kstep != n): the columns from n on keep their sentinels.
    mi_surfcpu_descriptors (upright: exact) with the image a column slice at an odd byte offset of a wider buffer and the descriptors
    written into a column slice of a wider sentinel-filled tensor (dstep != 64): survivors equal the oracle's, an erased keypoint
    (size <= 0) gets a zero row, the sentinels survive."""
    import torch
    from opencv_contrib_amd import capi, cuda
    _m = capi.mat_from_tensor
    img = hand_frame()
    pts = HAND_PLACED + CHUNK_EDGES
    kp, n = keypoint_rows(pts), len(pts)
    k_ref, _ = oracle.surfcpu_compute(img, kp, False, False, want_desc=False)
    assert len(k_ref) < n
    km = np.full((7, n + 5), SENTINEL, np.float32)
    km[:, :n] = _kp_matrix(kp)
    tk = torch.from_numpy(km).to(gpu)
    timg = torch.from_numpy(img).to(gpu)
    capi.check(capi.lib().mi_surfcpu_orientation(C.byref(_m(cuda.surf_integral(timg))), C.byref(_m(tk)), n, 0, capi.current_stream_ptr()))
    kg = tk.cpu().numpy()
    assert (kg[:, n:] == SENTINEL).all()
    keep = kg[4, :n] > 0
    assert keep.sum() == len(k_ref)
    for row, col in ((0, 0), (1, 1), (4, 2), (5, 3)):
        np.testing.assert_array_equal(kg[row, :n][keep], k_ref[:, col])
    np.testing.assert_array_equal(kg[6, :n], kp[:, 4])                # the rows the kernel does not own
    # descriptors, upright, from the matrix the orientation left (sizes of the erased keypoints are -1)
    wide = np.full((img.shape[0] + 2, img.shape[1] + 24), 0 if np.median(img) > 127 else 255, np.uint8)
    wide[1:-1, 7:7 + img.shape[1]] = img
    vimg = torch.from_numpy(wide).to(gpu)[1:-1, 7:7 + img.shape[1]]
    assert not vimg.is_contiguous()
    wd = torch.full((n + 3, 3 + 64 + 6), SENTINEL, dtype=torch.float32, device=gpu)
    vd = wd[1:n + 1, 3:3 + 64]
    capi.check(capi.lib().mi_surfcpu_descriptors(C.byref(_m(vimg)), C.byref(_m(tk)), n, 0, 1, C.byref(_m(vd)), capi.current_stream_ptr()))
    dg = vd.cpu().numpy()
    k_up, d_up = oracle.surfcpu_compute(img, kp[keep], False, True)  # the upright pass erases none of them
    assert len(k_up) == keep.sum()
    np.testing.assert_array_equal(dg[keep], d_up)
    assert (dg[~keep] == 0).all() and (~keep).any()
    g = wd.cpu().numpy()
    g[1:n + 1, 3:3 + 64] = SENTINEL
    assert (g == SENTINEL).all()


def test_hip_reproduces_the_reference_golden_vectors(gpu, oracle):
    """The Java tests' known answers (see tests/test_zz_surf_cpu_class.py) through the product: this class's detector, then the CPU
    class's orientation and descriptor."""
    import torch
    from opencv_contrib_amd import cuda
    from test_zz_surf_cpu_class import EPS, JAVA_DESCRIPTOR, JAVA_TRUTH, java_cross
    img = torch.from_numpy(java_cross()).to(gpu)
    alg = cuda.SURF_CUDA.create(8000, 3, 4, True, 0.05, False)
    kg, _ = alg.detectAndComputeCpuClass(img)
    k = cuda.SURF_CUDA.downloadKeypoints(kg)
    order = np.argsort(k["angle"])
    got = np.stack([k["x"], k["y"], k["size"], k["angle"], k["hessian"]], 1)[order]
    assert got.shape == (4, 5)
    np.testing.assert_allclose(got[:, :4], JAVA_TRUTH[:, :4], rtol=0, atol=EPS)
    np.testing.assert_allclose(got[:, 4], JAVA_TRUTH[:, 4], rtol=0, atol=5e-3)     # response: 8617.86 in binary32 has 1e-3 resolution
    assert (k["octave"] == 0).all() and (k["laplacian"] == -1).all()
    # SURFDescriptorExtractorTest: SURF(100, 2, 4, extended, not upright).compute on the given keypoint
    kp = np.array([[55.775577545166016, 44.224422454833984, 16, 9.754629, 8617.863, 1, -1]], np.float32)
    k1 = np.zeros((7, 1), np.float32)
    k1[0], k1[1], k1[4], k1[5], k1[6] = kp[:, 0], kp[:, 1], kp[:, 2], kp[:, 3], kp[:, 4]
    alg2 = cuda.SURF_CUDA.create(100, 2, 4, True, 0.05, False)
    k2, d2 = alg2.detectAndComputeCpuClass(img, None, torch.from_numpy(k1).to(gpu), True)
    assert abs(float(k2[5, 0]) - 350.24573) < EPS
    np.testing.assert_allclose(d2.cpu().numpy()[0], JAVA_DESCRIPTOR, rtol=0, atol=EPS)
