"""The HIP kernels of the CPU-class SURF stages (csrc/surfcpu_dev.h) compiled for the HOST: every phase of a workgroup runs as a loop
over the thread index (tests/cpp/surfcpu_emul.cpp), so the kernel logic -- phases, shared-memory hand-offs, the chunked area resize,
the sequential position accumulation -- is checked BIT FOR BIT against the pinned oracle (oracle/surfcpu_ref.c) without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from opencv_contrib_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emul") / "libsurfcpu_emul.so")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
           "-I" + os.path.join(ROOT, "opencv_contrib_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "surfcpu_emul.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = C.CDLL(out)
    L.emul_orientation.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    L.emul_descriptors.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return L


def _integral(img):
    s = np.zeros((img.shape[0] + 1, img.shape[1] + 1), np.int32)
    s[1:, 1:] = img.astype(np.int64).cumsum(0).cumsum(1)
    return s


def _run(L, oracle, img, kp, extended, upright):
    img = np.ascontiguousarray(img)
    k_ref, d_ref = oracle.surfcpu_compute(img, kp, extended, upright)
    s = _integral(img)
    k = np.ascontiguousarray(kp, np.float32).copy()
    L.emul_orientation(s.ctypes.data, img.shape[0], img.shape[1], k.ctypes.data, len(k), int(upright))
    d = np.zeros((len(k), 128 if extended else 64), np.float32)
    bad = L.emul_descriptors(img.ctypes.data, img.shape[0], img.shape[1], k.ctypes.data, len(k), int(extended), int(upright), d.ctypes.data)
    keep = k[:, 2] > 0
    assert bad == 0
    np.testing.assert_array_equal(k[keep], k_ref)
    np.testing.assert_array_equal(d[keep], d_ref)
    return int(keep.sum())


@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("upright", [False, True])
def test_emulated_kernels_equal_the_oracle_on_detected_keypoints(emul, oracle, extended, upright):
    img = synth.blob_image(360, 480, seed=21)
    kp = oracle.surfcpu_detect(img, 200.0, 4, 3)
    assert _run(emul, oracle, img, kp, extended, upright) > 100


def test_emulated_kernels_equal_the_oracle_on_the_golden_cross(emul, oracle):
    cross = np.full((100, 100), 255, np.uint8)
    cross[49:52, 20:80] = 100
    cross[20:80, 49:52] = 100
    kp = oracle.surfcpu_detect(cross, 8000.0, 3, 4)
    assert _run(emul, oracle, cross, kp, True, False) == 4


def win_rows(size):
    """Rows (= columns) of a keypoint's descriptor window: the kernel's own binary32 expression (int)(21 * (size * 1.2f / 9.0f))"""
    s = np.float32(np.float32(size) * np.float32(1.2)) / np.float32(9.0)
    return int(np.float32(21) * s)


def size_for_rows(win):
    """A keypoint size in the middle of those whose window has `win` rows"""
    size = float(np.float32((win + 0.5) * 9.0 / (21 * 1.2)))
    assert win_rows(size) == win
    return size


# Hand-placed keypoints (x, y, size) on the 300 x 400 frame hand_frame(): windows larger than one chunk of 256 rows (size 120 -> 336
# rows, size 300 -> 840 rows), keypoints on and outside the image border (clamped window reads; no orientation sample inside the image ->
# erased), the smallest filter size, 7.7: a 21-row window, resized by copy ...
HAND_PLACED = [(200, 150, 120), (10, 10, 120), (390, 290, 300), (200, 150, 300), (0.5, 0.5, 9), (399.2, 299.7, 9), (200.3, 1.2, 20),
               (1.7, 150.1, 33), (-40, -40, 12), (460, 340, 15), (200, 150, 9), (123.4, 77.7, 8), (50, 250, 51), (350, 40, 27), (100, 100, 7.7)]
# ... and windows of exactly one to four chunks of the descriptor kernel's 256 threads, each chunk count at its edge, at the frame
# centre and near a corner.  (Windows of fewer than 21 or more than 1024 rows get a zero row by design: the oracle has no counterpart.)
CHUNK_EDGE_ROWS = [256, 257, 512, 513, 768, 769, 1024]
CHUNK_EDGES = [(x, y, size_for_rows(w)) for w in CHUNK_EDGE_ROWS for x, y in ((200, 150), (12.3, 9.6))]


def hand_frame():
    return synth.blob_image(300, 400, seed=5)


def keypoint_rows(pts):
    """(x, y, size) -> the oracle's rows {x, y, size, angle = -1, response, octave, class_id}"""
    kp = np.zeros((len(pts), 7), np.float32)
    for i, (x, y, s) in enumerate(pts):
        kp[i, :3] = (x, y, s)
        kp[i, 3] = -1
        kp[i, 4] = 1000 - i
    return kp


def large_window_keypoints(n=200):
    """n keypoints at random positions of hand_frame() whose windows all have more than 256 rows: a third each in two, three and
    four chunks of 256 rows"""
    rng = np.random.default_rng(77)
    pts = []
    for i in range(n):
        lo, hi = [(257, 512), (513, 768), (769, 1024)][i % 3]
        size = size_for_rows(int(rng.integers(lo, hi, endpoint=True)))
        pts.append((float(rng.uniform(0, 400)), float(rng.uniform(0, 300)), size))
    chunks = np.array([(win_rows(s) + 255) // 256 for _, _, s in pts])
    assert chunks.min() == 2 and all(abs(int((chunks == c).sum()) - n / 3) <= 1 for c in (2, 3, 4))
    return pts


def test_window_rows_of_the_hand_placed_tables():
    assert [win_rows(s) for _, _, s in HAND_PLACED[:4]] == [336, 336, 840, 840] and win_rows(7.7) == 21 and win_rows(8) == 22
    assert [win_rows(s) for _, _, s in CHUNK_EDGES] == [w for w in CHUNK_EDGE_ROWS for _ in range(2)]
    assert all(21 <= win_rows(s) <= 1024 for _, _, s in HAND_PLACED + CHUNK_EDGES + large_window_keypoints())


def test_emulated_kernels_borders_large_windows_and_erased_keypoints(emul, oracle):
    """HAND_PLACED and CHUNK_EDGES: the oriented pass erases some of the former (the upright pass has no samples to miss), every one
    of the latter survives."""
    img = hand_frame()
    kp = keypoint_rows(HAND_PLACED + CHUNK_EDGES)
    for extended in (False, True):
        for upright in (False, True):
            n = _run(emul, oracle, img, kp, extended, upright)
            assert n == len(kp) if upright else 8 <= n - len(CHUNK_EDGES) < len(HAND_PLACED)
    k_ref, _ = oracle.surfcpu_compute(img, kp[len(HAND_PLACED):], False, False)
    assert len(k_ref) == len(CHUNK_EDGES)


@pytest.mark.parametrize("upright", [False, True])
def test_emulated_kernels_equal_the_oracle_on_two_to_four_chunk_windows(emul, oracle, upright):
    assert _run(emul, oracle, hand_frame(), keypoint_rows(large_window_keypoints()), True, upright) > 150
