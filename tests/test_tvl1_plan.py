"""The plan of one lane's TV-L1 calc (csrc/tvl1_plan.h), checked on the host."""
import os
import subprocess


def test_calc_plan_host_arithmetic(tmp_path):
    """tests/cpp/tvl1_plan_test.cpp: the plan lane_calc executes -- level sizes and the 16 px cut (cudaoptflow/src/tvl1flow.cpp:238-266),
    the arena layout, the iteration form and blocks of every warp for the headline, the class defaults, gamma, exact math, time_block 1
    and the median filter, and a worst-case run of the speculative launch loop that never leaves the control slots it was sized for;
    the table of the streaming kernels and tb_select against the tables and dispatch rules they replaced, in the release build's and
    in the experiments build's form.  Plain C++, no device."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "tvl1_plan_test")
    for flags in ([], ["-DMIFLOW_EXPERIMENTS"]):
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I" + os.path.join(root, "opencv_contrib_amd", "csrc"),
                            "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "tvl1_plan_test.cpp"), "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "tvl1_plan_test: ok" in r.stdout, r.stdout + r.stderr
