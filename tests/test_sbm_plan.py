"""The plan of StereoBM's launches (csrc/sbm_plan.h), checked on the host."""
import os
import subprocess


def test_block_match_plan_host_arithmetic(tmp_path):
    """tests/cpp/sbm_plan_test.cpp: sbm_make_plan / bm_lds / texf_lds / bm_band_rows / sbm_check against the expressions they replaced
    (Cfg<R>'s widths, the LDS sizes of k_block_match / launch_bm and k_textureness_fused / textureness_fused(), the band rule, grid and
    block of block_match_impl, textureness_scratch_dims, check_bm_params), field by field, over every radius 1..25 x 6 disparity ranges
    x 5 batch sizes x widths and heights from the smallest image the validator admits (1, TW and TW + 1 valid columns) up to 1080p x
    the 8 settings of the switches x uniqueness on / off (rejected shapes are skipped, the compared count is asserted exactly); the
    layouts' invariants (regions in order and disjoint, the transposition buffer on a 16-byte boundary, per-wave slices disjoint, the
    total = the end of the last region and below 64 KiB, a lane's reads inside its row); coverage of the grid; the band rule's bounds and
    its two known heights; the kernel's typed form of the layout against the host's; one rejected case per requirement of the validator.
    Plain C++, no device; compiled as the release build and as the experiments build see the header."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "sbm_plan_test")
    for flags in ([], ["-DMIFLOW_EXPERIMENTS"]):
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I" + os.path.join(root, "opencv_contrib_amd", "csrc"),
                            "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "sbm_plan_test.cpp"), "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "sbm_plan_test: ok" in r.stdout, r.stdout + r.stderr
