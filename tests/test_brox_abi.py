"""The C boundary of cv::cuda::BroxOpticalFlow without a GPU: the exports, the reference's defaults, and every rejection happening before
the device is looked for (a machine without one would answer MI_ERR_NO_DEVICE otherwise)."""
import ctypes as C

import pytest

OK, BAD_ARG, BAD_TYPE, BAD_SIZE, NO_DEVICE = 0, -1, -2, -3, -7
F32C1, F32C2 = 5, 13
ENTRIES = ["mi_brox_default_params", "mi_brox_create", "mi_brox_set_params", "mi_brox_get_params", "mi_brox_set_form", "mi_brox_scratch_bytes", "mi_brox_plan_info",
           "mi_brox_calc", "mi_brox_destroy", "mi_brox_resize_down", "mi_brox_resize_up", "mi_brox_derivatives", "mi_brox_prepare", "mi_brox_sor"]


def lib():
    from opencv_contrib_amd import capi
    return capi, capi.lib()


def _mat(capi, rows, cols, type_=F32C1, step=None, data=0x1000):
    """an mi_mat over memory that is never touched: every call here must return before it reads an image"""
    es = 8 if type_ == F32C2 else 4
    return capi.Mat(data, cols * es if step is None else step, rows, cols, type_)


def _mats(capi, n, rows, cols):
    return (capi.Mat * n)(*[_mat(capi, rows, cols) for _ in range(n)])


def test_exports_and_header_agree():
    capi, L = lib()
    declared = [s for s in capi.declared_symbols() if s.startswith("mi_brox_")]
    assert sorted(declared) == sorted(ENTRIES)
    for name in ENTRIES:
        assert getattr(L, name).argtypes is not None, name


def test_defaults_equal_the_reference():
    """BroxOpticalFlow::create, cudaoptflow.hpp:179-185"""
    capi, L = lib()
    p = capi.BroxParams()
    L.mi_brox_default_params(C.byref(p))
    f = C.c_float
    assert (p.alpha, p.gamma, p.scale_factor) == (f(0.197).value, 50.0, f(0.8).value)
    assert (p.inner_iterations, p.outer_iterations, p.solver_iterations) == (5, 150, 10)
    L.mi_brox_default_params(None)   # tolerated


BAD = [("alpha 0", "alpha", 0.0), ("alpha -1", "alpha", -1.0), ("alpha nan", "alpha", float("nan")), ("gamma -0.5", "gamma", -0.5),
       ("gamma nan", "gamma", float("nan")), ("scale_factor 0", "scale_factor", 0.0), ("scale_factor 1", "scale_factor", 1.0),
       ("scale_factor 1.5", "scale_factor", 1.5), ("scale_factor -0.8", "scale_factor", -0.8), ("scale_factor nan", "scale_factor", float("nan")),
       ("inner 0", "inner_iterations", 0), ("inner -1", "inner_iterations", -1), ("outer 0", "outer_iterations", 0),
       ("solver 0", "solver_iterations", 0), ("solver -5", "solver_iterations", -5)]


@pytest.mark.parametrize("what,field,value", BAD, ids=[b[0].replace(" ", "_") for b in BAD])
def test_create_rejects_before_it_looks_for_a_device(what, field, value):
    """NCVBroxOpticalFlow.cu:606-610 and 0 < scale_factor < 1"""
    capi, L = lib()
    p = capi.BroxParams()
    L.mi_brox_default_params(C.byref(p))
    setattr(p, field, value)
    h = C.c_void_p()
    assert L.mi_brox_create(C.byref(p), C.byref(h)) == BAD_ARG and not h.value, L.mi_last_error()
    assert L.mi_last_error()
    from opencv_contrib_amd import cuda
    kw = {f: getattr(p, f) for f, _ in capi.BroxParams._fields_}
    with pytest.raises(capi.MiError) as e:
        cuda.BroxOpticalFlow.create(**kw)
    assert e.value.code == BAD_ARG


def test_gamma_zero_is_accepted_and_the_device_is_looked_for_last():
    """with legal parameters the answer is the device's: MI_ERR_NO_DEVICE without one, a handle with one"""
    capi, L = lib()
    p = capi.BroxParams()
    L.mi_brox_default_params(C.byref(p))
    p.gamma = 0.0
    h = C.c_void_p()
    rc = L.mi_brox_create(C.byref(p), C.byref(h))
    if L.mi_device_count() <= 0:
        assert rc == NO_DEVICE and not h.value and L.mi_last_error()
    else:
        assert rc == OK and h.value
        L.mi_brox_destroy(h)
    assert L.mi_brox_create(C.byref(p), None) == BAD_ARG
    L.mi_brox_destroy(None)   # tolerated


def test_null_handles_and_arguments():
    capi, L = lib()
    p, n = capi.BroxParams(), C.c_size_t()
    m = _mat(capi, 8, 8)
    assert L.mi_brox_set_params(None, C.byref(p)) == BAD_ARG and L.mi_brox_get_params(None, C.byref(p)) == BAD_ARG
    assert L.mi_brox_set_form(None, 1) == BAD_ARG and L.mi_brox_scratch_bytes(None, C.byref(n)) == BAD_ARG
    assert L.mi_brox_calc(None, C.byref(m), C.byref(m), C.byref(_mat(capi, 8, 8, F32C2)), None) == BAD_ARG


def test_stage_entries_reject_a_side_of_three_and_bad_matrices_before_any_device_call():
    capi, L = lib()
    ok, ok7, ok9 = _mat(capi, 8, 8), _mats(capi, 7, 8, 8), _mats(capi, 9, 8, 8)
    for rows, cols in ((3, 8), (8, 3), (1, 1)):
        small, small7, small9 = _mat(capi, rows, cols), _mats(capi, 7, rows, cols), _mats(capi, 9, rows, cols)
        assert L.mi_brox_derivatives(C.byref(small), C.byref(small), small7, None) == BAD_ARG, L.mi_last_error()
        assert L.mi_brox_prepare(C.byref(small), C.byref(small), C.byref(small), C.byref(small), small9, 0.197, 50.0, small7, None) == BAD_ARG
        assert L.mi_brox_sor(C.byref(small), C.byref(small), C.byref(small), C.byref(small), small7, 1, 1, None) == BAD_ARG
        assert L.mi_brox_resize_down(C.byref(small), C.byref(ok), 0.8, None) == BAD_ARG
    assert L.mi_brox_derivatives(C.byref(_mat(capi, 32768, 8)), C.byref(ok), ok7, None) == BAD_SIZE
    assert L.mi_brox_derivatives(C.byref(ok), C.byref(_mat(capi, 8, 9)), ok7, None) == BAD_SIZE
    assert L.mi_brox_derivatives(C.byref(ok), C.byref(_mat(capi, 8, 8, 0)), ok7, None) == BAD_TYPE
    assert L.mi_brox_derivatives(C.byref(ok), C.byref(_mat(capi, 8, 8, step=30)), ok7, None) == BAD_ARG      # step below the row
    assert L.mi_brox_derivatives(C.byref(ok), C.byref(_mat(capi, 8, 8, step=34)), ok7, None) == BAD_ARG      # step no multiple of 4
    assert L.mi_brox_derivatives(C.byref(ok), C.byref(_mat(capi, 8, 8, data=0x1002)), ok7, None) == BAD_ARG  # data not float-aligned
    assert L.mi_brox_derivatives(C.byref(ok), C.byref(_mat(capi, 8, 8, data=None)), ok7, None) == BAD_ARG
    assert L.mi_brox_prepare(C.byref(ok), C.byref(ok), C.byref(ok), C.byref(ok), ok9, 0.0, 50.0, ok7, None) == BAD_ARG    # alpha
    assert L.mi_brox_prepare(C.byref(ok), C.byref(ok), C.byref(ok), C.byref(ok), ok9, 0.197, -1.0, ok7, None) == BAD_ARG  # gamma
    assert L.mi_brox_sor(C.byref(ok), C.byref(ok), C.byref(ok), C.byref(ok), ok7, 3, 1, None) == BAD_ARG                  # form
    assert L.mi_brox_sor(C.byref(ok), C.byref(ok), C.byref(ok), C.byref(ok), ok7, 1, 0, None) == BAD_ARG                  # iterations
    for sf in (0.0, 1.0, -0.5, float("nan")):
        assert L.mi_brox_resize_down(C.byref(ok), C.byref(ok), sf, None) == BAD_ARG
        assert L.mi_brox_resize_up(C.byref(ok), C.byref(ok), sf, None) == BAD_ARG
    # a destination whose last supersample window would leave the source
    assert L.mi_brox_resize_down(C.byref(ok), C.byref(ok), 0.5, None) == BAD_SIZE and b"window" in L.mi_last_error()
    assert L.mi_brox_resize_up(C.byref(ok), C.byref(_mat(capi, 0, 8)), 0.8, None) == BAD_SIZE


def test_legal_stage_calls_answer_no_device_without_one():
    capi, L = lib()
    if L.mi_device_count() > 0:
        return   # with a device these calls would run, on memory that does not exist; tests/test_brox_gpu.py runs them on real planes
    ok, ok7 = _mat(capi, 8, 8), _mats(capi, 7, 8, 8)
    assert L.mi_brox_derivatives(C.byref(ok), C.byref(ok), ok7, None) == NO_DEVICE
    assert L.mi_brox_sor(C.byref(ok), C.byref(ok), C.byref(ok), C.byref(ok), ok7, 2, 3, None) == NO_DEVICE
    assert L.mi_brox_resize_up(C.byref(ok), C.byref(_mat(capi, 10, 10)), 0.8, None) == NO_DEVICE
    assert L.mi_brox_resize_down(C.byref(ok), C.byref(_mat(capi, 7, 7)), 0.8, None) == NO_DEVICE
