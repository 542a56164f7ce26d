"""cv::cuda::BroxOpticalFlow and cv::superres::createOptFlow_Brox_CUDA() from C++ (tests/cpp/brox_shim.cpp) and the Python superres
adapter: the bits of the C-ABI, which tests/test_brox_gpu.py holds to the reference's own kernels, on one class fixture."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_brox_ref import GOLDEN, class_params  # noqa: E402

LIBDIR = os.path.join(ROOT, "opencv_contrib_amd")
FIXTURE = os.path.join(GOLDEN, "brox_refclass_37x70.npz")


def build_shim(tmp_path):
    exe = str(tmp_path / "brox_shim")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "brox_shim.cpp"),
                        "-o", exe, "-L" + LIBDIR, "-lmiflow", "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def eq_bits(got, want, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), what


def test_cpp_mirror_compiles_and_fails_loudly_without_gpu(tmp_path):
    """the reference's signatures and defaults (static_asserts), the rejections that need no device; creating the class without a device
    throws.  CPU test: with a device the same program passes its no-argument checks."""
    import torch
    r = subprocess.run([build_shim(tmp_path)], capture_output=True, text=True)
    if torch.cuda.is_available():
        assert r.returncode == 0, (r.returncode, r.stderr)
    else:
        assert r.returncode == 3 and "device" in r.stderr.lower(), (r.returncode, r.stderr)


@pytest.mark.gpu
def test_cpp_class_and_adapter_equal_the_c_abi(gpu, tmp_path):
    import torch
    from opencv_contrib_amd import cuda
    z = np.load(FIXTURE)
    p = class_params(z)
    rows, cols = z["I0"].shape
    want = cuda.BroxOpticalFlow.create(**p).calc(torch.from_numpy(z["I0"]).to(gpu), torch.from_numpy(z["I1"]).to(gpu)).cpu().numpy()
    eq_bits(want, z["flow"], "the C-ABI against the fixture")
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("=5i3d", rows, cols, p["inner_iterations"], p["outer_iterations"], p["solver_iterations"], p["alpha"], p["gamma"],
                                p["scale_factor"]) + z["I0"].tobytes() + z["I1"].tobytes())
    r = subprocess.run([build_shim(tmp_path), str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.frombuffer(fout.read_bytes(), np.float32)
    n = rows * cols
    assert raw.size == 4 * n
    eq_bits(raw[:2 * n].reshape(rows, cols, 2), want, "cuda::BroxOpticalFlow")
    eq_bits(raw[2 * n:3 * n].reshape(rows, cols), np.ascontiguousarray(want[..., 0]), "createOptFlow_Brox_CUDA u")
    eq_bits(raw[3 * n:].reshape(rows, cols), np.ascontiguousarray(want[..., 1]), "createOptFlow_Brox_CUDA v")


@pytest.mark.gpu
def test_python_superres_adapter_equals_the_c_abi(gpu):
    import torch
    from opencv_contrib_amd import superres
    from opencv_contrib_amd.capi import MiError
    z = np.load(FIXTURE)
    p = class_params(z)
    ext = superres.createOptFlow_Brox_CUDA()
    assert (ext.getInnerIterations(), ext.getOuterIterations(), ext.getSolverIterations()) == (10, 77, 10)   # optical_flow.cpp:542
    assert (ext.getAlpha(), ext.getGamma(), ext.getScaleFactor()) == (float(np.float32(0.197)), 50.0, float(np.float32(0.8)))
    ext.setAlpha(p["alpha"]); ext.setGamma(p["gamma"]); ext.setScaleFactor(p["scale_factor"])
    ext.setInnerIterations(p["inner_iterations"]); ext.setOuterIterations(p["outer_iterations"]); ext.setSolverIterations(p["solver_iterations"])
    f0, f1 = torch.from_numpy(z["I0"]).to(gpu), torch.from_numpy(z["I1"]).to(gpu)
    for _ in range(2):
        u, v = ext.calc(f0, f1)
        eq_bits(u.cpu().numpy(), np.ascontiguousarray(z["flow"][..., 0]), "u")
        eq_bits(v.cpu().numpy(), np.ascontiguousarray(z["flow"][..., 1]), "v")
        eq_bits(ext.calc(f0, f1, want_flow2=False).cpu().numpy(), z["flow"], "merged")
        ext.collectGarbage()
    with pytest.raises(MiError):
        ext.calc(f0.to(torch.uint8), f1.to(torch.uint8))


@pytest.mark.gpu
def test_a_rejected_setter_leaves_the_object_as_it_was(gpu):
    from opencv_contrib_amd import cuda
    from opencv_contrib_amd.capi import MiError
    alg = cuda.BroxOpticalFlow.create()
    before = [getattr(alg, g)() for g in ("getFlowSmoothness", "getGradientConstancyImportance", "getPyramidScaleFactor", "getInnerIterations",
                                          "getOuterIterations", "getSolverIterations")]
    for setter, bad in (("setFlowSmoothness", 0.0), ("setGradientConstancyImportance", -1.0), ("setPyramidScaleFactor", 1.0),
                        ("setPyramidScaleFactor", 0.0), ("setInnerIterations", 0), ("setOuterIterations", -2), ("setSolverIterations", 0)):
        with pytest.raises(MiError) as e:
            getattr(alg, setter)(bad)
        assert e.value.code == -1
        assert [getattr(alg, g)() for g in ("getFlowSmoothness", "getGradientConstancyImportance", "getPyramidScaleFactor", "getInnerIterations",
                                            "getOuterIterations", "getSolverIterations")] == before
    with pytest.raises(MiError):
        alg.setSolverForm(3)
    alg.setSolverIterations(3)
    assert alg.getSolverIterations() == 3
