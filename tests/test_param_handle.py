"""The one owner of (handle, parameters) in each wrapper layer, checked on the host: cv::cuda::miflow_detail::ParamHandle of the C++
drop-in headers over a fake C library, and cuda._Handle of the Python mirror over a fake capi.lib()."""
import ctypes as C
import os
import subprocess

import pytest

from opencv_contrib_amd import capi, cuda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = {"plain": [], "sanitized": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]}


def _compile(flags, src, exe):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "include"), src, "-o", exe],
                          capture_output=True, text=True)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_param_handle_host_semantics(tmp_path, variant):
    """tests/cpp/param_handle_test.cpp: a create that fails throws and destroys nothing; an accepted set commits; a rejected set leaves
    params() bit-identical and the library's copy untouched, and a valid set after it succeeds; refresh overwrites the kept struct;
    a create with a further argument goes through the callable overload; every handle is destroyed exactly once (the handles are
    malloc'd, so a leak or a second destroy fails the sanitized build).  Plain C++, no device, its own process: once plain and once
    under -fsanitize=address,undefined (skipped only where a trivial program does not build with those flags)."""
    flags = VARIANTS[variant]
    if flags:
        trivial = tmp_path / "trivial.cpp"
        trivial.write_text("int main() { return 0; }\n")
        if _compile(flags, str(trivial), str(tmp_path / "trivial")).returncode != 0:
            pytest.skip("no address / undefined-behaviour sanitizer runtime for g++ on this machine")
    exe = str(tmp_path / "param_handle_test")
    r = _compile(flags, os.path.join(ROOT, "tests", "cpp", "param_handle_test.cpp"), exe)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "param_handle_test: ok" in r.stdout, r.stdout + r.stderr


class FakeLib:
    """mi_fast_create / _set_params / _destroy as the base calls them: records every call, hands out handles 0x1000, 0x1001, ...;
    rejects a negative threshold like a validating set_params, and every create while `fail_create` is set."""

    def __init__(self):
        self.calls, self.live, self.fail_create, self.next, self.made = [], set(), False, 0x1000, []

    def mi_last_error(self):
        return b"fake: rejected"

    def mi_fast_create(self, p, out):
        self.calls.append(("create", bytes(p._obj)))
        if self.fail_create or p._obj.threshold < 0:
            return -1
        out._obj.value = self.next
        self.live.add(self.next)
        self.next += 1
        return 0

    def mi_fast_set_params(self, h, p):
        self.calls.append(("set_params", h.value, bytes(p._obj)))
        return -1 if p._obj.threshold < 0 else 0

    def mi_fast_destroy(self, h):
        self.calls.append(("destroy", h.value))
        self.live.remove(h.value)   # a second destroy of a handle raises here, and __del__ would swallow it: the call log shows it

    def keep(self, obj):
        """An object made over this fake: the fixture disarms it before the real library is back, whatever the test did."""
        self.made.append(obj)
        return obj

    def count(self, kind):
        return sum(1 for c in self.calls if c[0] == kind)


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(capi, "lib", lambda: lib)
    yield lib
    for obj in lib.made:   # a fake handle must never reach the real mi_fast_destroy when the object is collected later
        obj._h = None


def test_python_failed_create_leaves_no_handle(fake):
    fake.fail_create = True
    obj = cuda._Handle()
    with pytest.raises(capi.MiError) as e:
        obj._open("fast", capi.FastParams(10, 1, 5000))
    assert e.value.code == -1
    assert obj._h is None and not hasattr(obj, "_p")
    obj.__del__()
    obj.__del__()
    assert fake.count("create") == 1 and fake.count("destroy") == 0
    # through a class: the constructor raises, and collecting the half-built object is silent and destroys nothing
    with pytest.raises(capi.MiError):
        cuda.FastFeatureDetector(threshold=10)
    half = cuda.FastFeatureDetector.__new__(cuda.FastFeatureDetector)   # __init__ never ran: no _h at all
    half.__del__()
    assert fake.count("destroy") == 0


def test_python_set_commits_on_acceptance_only(fake):
    alg = fake.keep(cuda.FastFeatureDetector(threshold=10, nonmaxSuppression=True, max_npoints=5000))
    p, kind = alg._p, type(alg._p)
    assert isinstance(alg._h, C.c_void_p) and alg._h.value == 0x1000 and kind is capi.FastParams

    alg.setThreshold(25)   # accepted: the same _p object now holds it, and the library was sent the edited copy
    assert alg._p is p and type(alg._p) is kind and alg.getThreshold() == 25 and p.threshold == 25
    assert fake.calls[-1] == ("set_params", 0x1000, bytes(capi.FastParams(25, 1, 5000)))

    before = bytes(alg._p)
    with pytest.raises(capi.MiError) as e:
        alg.setThreshold(-3)   # rejected
    assert e.value.code == -1 and "fake: rejected" in str(e.value)
    assert fake.calls[-1] == ("set_params", 0x1000, bytes(capi.FastParams(-3, 1, 5000)))   # the library was asked
    assert alg._p is p and bytes(alg._p) == before and alg.getThreshold() == 25

    alg.setMaxNumPoints(100)   # the object is not stuck: a valid setter after the rejected one succeeds
    assert alg._p is p and bytes(alg._p) == bytes(capi.FastParams(25, 1, 100))
    assert fake.calls[-1] == ("set_params", 0x1000, bytes(capi.FastParams(25, 1, 100)))


def test_python_destroy_runs_once(fake):
    alg = fake.keep(cuda.FastFeatureDetector())
    h = alg._h.value
    alg.__del__()
    assert alg._h is None
    alg.__del__()
    assert [c for c in fake.calls if c[0] == "destroy"] == [("destroy", h)] and not fake.live


def test_python_del_tolerates_a_missing_library(monkeypatch, fake):
    alg = fake.keep(cuda.FastFeatureDetector())

    def gone():
        raise OSError("libmiflow.so: cannot open shared object file")
    monkeypatch.setattr(capi, "lib", gone)
    alg.__del__()   # never raises
    assert alg._h is None


def test_stream_and_array_helpers(monkeypatch):
    """_stream_ptr: the caller's stream, else the current one; _mats: one mi_mat per tensor, a NULL-data one for None."""
    monkeypatch.setattr(capi, "current_stream_ptr", lambda: C.c_void_p(0x77))
    assert cuda._stream_ptr(0x1234).value == 0x1234 and cuda._stream_ptr(None).value == 0x77
    monkeypatch.setattr(capi, "mat_from_tensor", lambda t: capi.Mat(t, 8, 2, 2, capi.MI_32FC1))
    arr = cuda._mats([0x10, None, 0x30])
    assert len(arr) == 3 and [m.data for m in arr] == [0x10, None, 0x30] and (arr[1].rows, arr[1].cols, arr[1].step) == (0, 0, 0)
    assert len(cuda._mats([])) == 0
