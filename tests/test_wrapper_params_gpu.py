"""The Python mirror's classes over the real library: a value mi_*_set_params refuses leaves the object as it was, and every settable
field of every class goes to the library and comes back through its getter."""
import numpy as np
import pytest

from opencv_contrib_amd import capi, cuda, synth


@pytest.fixture(scope="module")
def pair(gpu):
    import torch
    a, b, _ = synth.flow_pair(64, 64, seed=5, dtype="u8")
    return torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)


def _rejected(setter, value):
    with pytest.raises(capi.MiError) as e:
        setter(value)
    assert e.value.code == -1


@pytest.mark.gpu
def test_tvl1_rejected_setter_leaves_the_object_as_it_was(gpu, pair):
    """setNumScales(0) raises MiError -1 (validate_params); getNumScales() still answers 3; setNumWarps(3), a valid value, then succeeds
    (before, every later setter re-sent the rejected nscales and failed too); the flow of a 64 x 64 pair then equals, bit for bit, the
    flow of a new object made with the same final parameters."""
    import torch
    kw = dict(nscales=3, warps=2, iterations=20)
    alg = cuda.OpticalFlowDual_TVL1.create(**kw)
    p = alg._p
    before = bytes(p)
    _rejected(alg.setNumScales, 0)
    assert alg.getNumScales() == 3 and alg._p is p and bytes(p) == before
    alg.setNumWarps(3)
    assert alg.getNumWarps() == 3 and alg.getNumScales() == 3
    flow = alg.calc(*pair)
    fresh = cuda.OpticalFlowDual_TVL1.create(**dict(kw, warps=3)).calc(*pair)
    torch.cuda.synchronize()
    assert flow.shape == (64, 64, 2) and torch.isfinite(flow).all() and (flow != 0).any()
    assert torch.equal(flow.view(torch.int32), fresh.view(torch.int32))


@pytest.mark.gpu
def test_sparse_pyrlk_rejected_setter_leaves_the_object_as_it_was(gpu, pair):
    """setMaxLevel(16) raises MiError -1 (validate: maxLevel < 16); getMaxLevel() still answers 2; setNumIters(7) then succeeds; the
    tracks of 33 points on a 64 x 64 pair equal, bit for bit, those of a new object made with the same final parameters."""
    import torch
    rng = np.random.default_rng(5)
    pts = torch.from_numpy(np.stack([rng.uniform(4, 60, 33), rng.uniform(4, 60, 33)], 1).astype(np.float32)).to(gpu)
    alg = cuda.SparsePyrLKOpticalFlow((9, 9), 2, 10)
    p = alg._p
    before = bytes(p)
    _rejected(alg.setMaxLevel, 16)
    assert alg.getMaxLevel() == 2 and alg._p is p and bytes(p) == before
    alg.setNumIters(7)
    assert alg.getNumIters() == 7 and alg.getMaxLevel() == 2
    got = alg.calc(*pair, pts)
    want = cuda.SparsePyrLKOpticalFlow((9, 9), 2, 7).calc(*pair, pts)
    torch.cuda.synchronize()
    ok = got[1][0] > 0
    assert ok.sum() > 0 and torch.equal(got[1], want[1])
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
    assert torch.equal(got[2][0][ok].view(torch.int32), want[2][0][ok].view(torch.int32))   # err is defined where the track completed


def _acc(name):
    """(set, get) through the reference's accessor pair setName / getName"""
    return (lambda o, v: getattr(o, "set" + name)(v)), (lambda o: getattr(o, "get" + name)())


def _field(name):
    """(set, get) through a public field of the reference class, a property here"""
    return (lambda o, v: setattr(o, name, v)), (lambda o: getattr(o, name))


# class -> (constructor, [(set, get, a second valid value)]); float values are exact in binary32, the width of most struct fields
CLASSES = {
    "StereoBM": (lambda: cuda.createStereoBM(64, 19), [(*_acc(n), v) for n, v in [
        ("NumDisparities", 128), ("BlockSize", 15), ("PreFilterType", 0), ("PreFilterSize", 11), ("PreFilterCap", 20), ("TextureThreshold", 5),
        ("UniquenessRatio", 10)]]),
    "DensePyrLKOpticalFlow": (lambda: cuda.DensePyrLKOpticalFlow.create(), [(*_acc(n), v) for n, v in [
        ("WinSize", (21, 21)), ("MaxLevel", 2), ("NumIters", 10), ("UseInitialFlow", True)]]),
    "StereoSGM": (lambda: cuda.createStereoSGM(), [(*_acc(n), v) for n, v in [
        ("MinDisparity", 3), ("NumDisparities", 64), ("P1", 8), ("P2", 100), ("UniquenessRatio", 10), ("Mode", 1)]]),
    "DisparityBilateralFilter": (lambda: cuda.createDisparityBilateralFilter(), [(*_acc(n), v) for n, v in [
        ("NumDisparities", 32), ("Radius", 5), ("NumIters", 2), ("EdgeThreshold", 0.25), ("MaxDiscThreshold", 0.5), ("SigmaRange", 16.0)]]),
    "StereoBeliefPropagation": (lambda: cuda.createStereoBeliefPropagation(), [(*_acc(n), v) for n, v in [
        ("NumDisparities", 32), ("NumIters", 3), ("NumLevels", 3), ("MaxDataTerm", 8.0), ("DataWeight", 0.125), ("MaxDiscTerm", 2.0),
        ("DiscSingleJump", 0.5), ("MsgType", cuda.CV_16S)]]),
    "StereoConstantSpaceBP": (lambda: cuda.createStereoConstantSpaceBP(), [(*_acc(n), v) for n, v in [
        ("NumDisparities", 64), ("NumIters", 3), ("NumLevels", 3), ("MaxDataTerm", 8.0), ("DataWeight", 0.125), ("MaxDiscTerm", 2.0),
        ("DiscSingleJump", 0.5), ("MsgType", cuda.CV_16S), ("MinDisparity", 2), ("NrPlane", 2), ("UseLocalInitDataCost", False)]]),
    "FarnebackOpticalFlow": (lambda: cuda.FarnebackOpticalFlow.create(), [(*_acc(n), v) for n, v in [
        ("NumLevels", 3), ("PyrScale", 0.75), ("FastPyramids", True), ("WinSize", 9), ("NumIters", 4), ("PolyN", 7), ("PolySigma", 1.5),
        ("Flags", cuda.OPTFLOW_FARNEBACK_GAUSSIAN)]]),
    "SURF_CUDA": (lambda: cuda.SURF_CUDA(), [(*_field(n), v) for n, v in [
        ("hessianThreshold", 400.0), ("nOctaves", 3), ("nOctaveLayers", 3), ("extended", False), ("upright", True), ("keypointsRatio", 0.125)]]),
    "FastFeatureDetector": (lambda: cuda.FastFeatureDetector.create(), [(*_acc(n), v) for n, v in [
        ("Threshold", 25), ("NonmaxSuppression", False), ("MaxNumPoints", 1000)]]),
    # the reference class has setters only; the getter side reads the kept struct
    "CornersDetector": (lambda: cuda.createGoodFeaturesToTrackDetector(capi.MI_8UC1), [
        (lambda o, v: o.setMaxCorners(v), lambda o: o._p.max_corners, 50), (lambda o, v: o.setMinDistance(v), lambda o: o._p.min_distance, 3.0)]),
    "ORB": (lambda: cuda.ORB.create(), [(*_acc(n), v) for n, v in [
        ("MaxFeatures", 300), ("ScaleFactor", 1.5), ("NLevels", 4), ("EdgeThreshold", 20), ("FirstLevel", 1), ("WTA_K", 3),
        ("ScoreType", cuda.ORB.FAST_SCORE), ("PatchSize", 21), ("FastThreshold", 10), ("BlurForDescriptor", True)]]),
    # create and destroy only: no parameter struct, or no setter
    "BFMatcher": (lambda: cuda.createBFMatcher(cuda.NORM_L2), []),
    "CornernessCriteria": (lambda: cuda.createHarrisCorner(capi.MI_8UC1, 3, 3, 0.04), []),
    "TVL1MultiDevice": (lambda: cuda.TVL1MultiDevice(cuda.OpticalFlowDual_TVL1.create(), devices=[0]), []),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CLASSES))
def test_every_settable_field_goes_through_the_library(gpu, name):
    """Construct; set each settable field to a second valid value and read it back through the getter, with every field set before it
    still in place; the kept struct keeps its identity and equals what the library holds (mi_*_get_params where the class has it);
    destroy once."""
    import ctypes as C
    make, fields = CLASSES[name]
    alg = make()
    assert isinstance(alg._h, C.c_void_p) and alg._h.value
    p = getattr(alg, "_p", None)
    done = []
    for setter, getter, value in fields:
        assert getter(alg) != value, "a second value, not the default"
        setter(alg, value)
        done.append((getter, value))
        for g, v in done:
            assert g(alg) == v
        assert alg._p is p
        get_params = getattr(capi.lib(), "mi_%s_get_params" % alg._prefix)
        held = type(p)()
        capi.check(get_params(alg._h, C.byref(held)))
        assert [getattr(held, f[0]) for f in held._fields_] == [getattr(p, f[0]) for f in p._fields_]
    alg.__del__()
    assert alg._h is None
    alg.__del__()
