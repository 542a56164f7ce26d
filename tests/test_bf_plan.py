"""The plan of the brute-force matcher's calls (csrc/bf_plan.h), checked on the host."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = {"plain": [], "sanitized": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]}


def _compile(flags, src, exe):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags,
                           "-I" + os.path.join(ROOT, "opencv_contrib_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), src, "-o", exe],
                          capture_output=True, text=True)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_matcher_plan_host_arithmetic(tmp_path, variant):
    """tests/cpp/bf_plan_test.cpp: bf_make_plan against the rules it replaced, restated there in the form they had (knn_shape,
    radius_shape, the split arithmetic, the two scratch formulas, the loops of run_knn / mi_bf_radius_match / bfint::knn / bfint::radius
    as launch lists, and the validation of the four entry points with bf::plan and bfint::check in their order, codes and texts).
    Sweep, field by field: 8 query counts x 9 descriptor lengths x 7 train sizes around the tile height x both float norms x one and
    four train sets x MIFLOW_BF_W 4 / 1 x (8 values of k + a radius match), the two fixed-shape calls, and the seven integer
    (depth, norm) rows x 4 lengths (k > 16 rejected); the compared counts are asserted exactly.  Invariants of every plan: the splits
    cover the train rows once, in whole tiles, none empty; seg0 and t_base are the prefix sums; the passes' columns tile [0, k) once and
    each merge follows the passes of its columns; assign-image entries only with img_idx, once per train set, descending, last; radius is
    count per set, one scan, write per set; grid.x = ceil(n_q / 64); the kernel's static_assert for every table row.  Four exact launch
    lists (150 queries x 700 / 33 / 1 / 260 rows with k = 13 and as a radius match, 12 564^2 with k = 2, uint8 Hamming k = 16 over two
    sets).  One rejected input per requirement with code and text, the pairs of faults whose winner depends on the order, the 32-bit
    bounds (INT_MAX train rows, n_q x cols, n_q x k), and every (depth, norm) pair against the reference's table.
    Plain C++, no device, its own process: once plain and once under -fsanitize=address,undefined (skipped only where a trivial program
    does not build with those flags)."""
    flags = VARIANTS[variant]
    if flags:
        trivial = tmp_path / "trivial.cpp"
        trivial.write_text("int main() { return 0; }\n")
        if _compile(flags, str(trivial), str(tmp_path / "trivial")).returncode != 0:
            pytest.skip("no address / undefined-behaviour sanitizer runtime for g++ on this machine")
    exe = str(tmp_path / "bf_plan_test")
    r = _compile(flags, os.path.join(ROOT, "tests", "cpp", "bf_plan_test.cpp"), exe)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bf_plan_test: ok" in r.stdout, r.stdout + r.stderr
