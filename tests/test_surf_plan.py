"""The plan of a SURF detect call (csrc/surf_plan.h), checked on the host."""
import os
import subprocess


def test_detect_plan_host_arithmetic(tmp_path):
    """tests/cpp/surf_plan_test.cpp: surf_make_plan against the expressions it replaced (make_octset, fused_sizes, fused_supported, the
    sizes and the launch-form mask of ensure(), the downgrade rules of detect_fused), field by field, over widths 40..300 + {640, 1283,
    1920, 3840} x heights 40..130 + {480, 1080, 2160} x 1..7 octaves x 1..5 layers x the 16 settings of the four switches (shapes the
    constructor's limits reject are skipped: 32.7 % of the sweep is compared, the count is asserted exactly); the layout's invariants
    (no region of an octave reaches into the next one's, the last ends at the allocated count, workgroup ranges in multiples of 8 and
    non-decreasing, sizes independent of the octave-0 form); the geometry table byte for byte with and without the polyphase planes;
    the compile-time geometry of the LDS tiles against haar_geo.  Plain C++, no device; compiled as the release build and as the
    experiments build see the header."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "surf_plan_test")
    for flags in ([], ["-DMIFLOW_EXPERIMENTS"]):
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I" + os.path.join(root, "opencv_contrib_amd", "csrc"),
                            "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "surf_plan_test.cpp"), "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "surf_plan_test: ok" in r.stdout, r.stdout + r.stderr
