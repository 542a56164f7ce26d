"""The one criterion every whole-calc Farneback comparison goes through (tests/test_farneback.py, tests/test_golden.py,
tests/test_ref_class_gpu.py).  The reasoning behind it and the measured figures are in the module docstring of tests/test_farneback.py."""
import numpy as np


def assert_flow_equals(flow, ref, what=""):
    """Every stage of a calc is held to the oracle bit for bit, form by form (tests/test_farneback.py, stage tests), and a calc is a fixed
    sequence of those stages: the whole flow equals the reference's, every pixel of it.  The worst pixel and the number of differing
    values are printed first, so that a failure says how far off the flow is and not only that it is."""
    flow, ref = np.asarray(flow), np.asarray(ref)
    assert flow.shape == ref.shape and np.isfinite(flow).all(), what
    d = np.sqrt(((flow.astype(np.float64) - ref) ** 2).sum(-1))
    print(f"farneback flow {what}: worst pixel {d.max():.3e} px, mean {d.mean():.3e} px, {int((flow != ref).sum())} of {flow.size} values differ")
    np.testing.assert_array_equal(flow, ref, err_msg=what)
