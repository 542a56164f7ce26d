"""The band-height rule of the streaming TV-L1 kernels (csrc/tvl1_plan.h tb_band_rows), checked on the host."""
import os
import subprocess


def test_band_height_rule_host_arithmetic(tmp_path):
    """tests/cpp/tvl1_band_test.cpp: over heights 16 .. 2200, waves per band row, capacities and T in {1, 2, 3, 4, 5, 6, 8, 10} the band
    count equals the round-3 rule's, the summed executed steps of the bands never exceed the equal cut's and equal the brute-force
    minimum over the admissible heights (at least 8 rows, the same band count, no band longer than the tallest band of the equal
    cut), and the headline's levels cut as stated: 553 rows 3 x 148 + 109, 442 rows 5 x 82 + 32.  Plain C++, no device."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "tvl1_band_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(root, "opencv_contrib_amd", "csrc"),
                        "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "tvl1_band_test.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "tvl1_band_test: ok" in r.stdout, r.stdout + r.stderr
