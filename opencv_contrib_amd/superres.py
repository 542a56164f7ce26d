"""Mirror of the reference's superres GPU classes: the optical-flow adapters, the one in-tree CALLER of the hot
path, and BTV-L1 super-resolution (`createSuperResolution_BTVL1_CUDA`, superres/src/btv_l1_cuda.cpp), their one in-tree consumer.

`cv::superres::createOptFlow_DualTVL1_CUDA()` / `createOptFlow_Farneback_CUDA()` (superres/src/optical_flow.cpp:665-845) wrap
the `cv::cuda` flow classes behind `DenseOpticalFlowExt::calc(frame0, frame1, flow1, flow2)`: frames of any supported
depth/channel count are converted to CV_8UC1 (`convertToType`, input_array_utility.cpp:291-314), the class runs, and the
CV_32FC2 result is split into two CV_32FC1 planes (or returned merged when flow2 is not requested, optical_flow.cpp:475-493).
Frames are torch CUDA tensors here where the reference takes GpuMat; everything runs through the C-ABI (no CPU fallback).
"""
from __future__ import annotations

import ctypes as C

from . import capi, cuda


def _m(t):
    return capi.mat_from_tensor(t)


def convertToGray8(frame):
    """convertToType(frame, CV_8UC1): BGR/BGRA -> gray, then depth -> 8U with scale 255 / maxVal(depth)."""
    import torch
    if frame.dtype == torch.uint8 and frame.dim() == 2:
        return frame   # input_array_utility.cpp:293-294: same type, no copy
    dst = torch.empty(frame.shape[:2], dtype=torch.uint8, device=frame.device)
    capi.check(capi.lib().mi_superres_to_gray8(C.byref(_m(frame)), C.byref(_m(dst)), capi.current_stream_ptr()))
    return dst


def splitFlow(flow):
    """cuda::split(flow, flows): CV_32FC2 -> two CV_32FC1 planes."""
    import torch
    u = torch.empty(flow.shape[:2], dtype=torch.float32, device=flow.device)
    v = torch.empty_like(u)
    capi.check(capi.lib().mi_split_flow(C.byref(_m(flow)), C.byref(_m(u)), C.byref(_m(v)), capi.current_stream_ptr()))
    return u, v


class _GpuOpticalFlow:
    """cv::superres GpuOpticalFlow (optical_flow.cpp:436-505), work type CV_8UC1."""

    def calc(self, frame0, frame1, want_flow2: bool = True):
        """Returns (flow1, flow2) = (u, v) planes, or the merged CV_32FC2 flow when want_flow2 is False
        (`_flow2.needed()` in the reference)."""
        if frame0.dtype != frame1.dtype or frame0.shape != frame1.shape:
            raise capi.MiError(-3, "frame1.type() == frame0.type() && frame1.size() == frame0.size()")   # optical_flow.cpp:466-467
        in0, in1 = convertToGray8(frame0), convertToGray8(frame1)
        flow = self._impl(in0, in1)
        return splitFlow(flow) if want_flow2 else flow

    def collectGarbage(self):
        self._alg = self._create()


class DualTVL1_CUDA(_GpuOpticalFlow):
    """cv::superres::createOptFlow_DualTVL1_CUDA() (optical_flow.cpp:757-845): getters/setters of
    cv::superres::DualTVL1OpticalFlow, parameters pushed into the cuda class at every calc (:817-826)."""

    def __init__(self):
        self._alg = self._create()
        a = self._alg
        self._p = dict(Tau=a.getTau(), Lambda=a.getLambda(), Theta=a.getTheta(), ScalesNumber=a.getNumScales(),
                       WarpingsNumber=a.getNumWarps(), Epsilon=a.getEpsilon(), Iterations=a.getNumIterations(),
                       UseInitialFlow=a.getUseInitialFlow())

    @staticmethod
    def _create():
        return cuda.OpticalFlowDual_TVL1.create()

    def _impl(self, in0, in1):
        a, p = self._alg, self._p
        a.setTau(p["Tau"]); a.setLambda(p["Lambda"]); a.setTheta(p["Theta"]); a.setNumScales(p["ScalesNumber"])
        a.setNumWarps(p["WarpingsNumber"]); a.setEpsilon(p["Epsilon"]); a.setNumIterations(p["Iterations"])
        a.setUseInitialFlow(p["UseInitialFlow"])
        return a.calc(in0, in1)


class Farneback_CUDA(_GpuOpticalFlow):
    """cv::superres::createOptFlow_Farneback_CUDA() (optical_flow.cpp:665-750)."""

    def __init__(self):
        self._alg = self._create()
        a = self._alg
        self._p = dict(PyrScale=a.getPyrScale(), LevelsNumber=a.getNumLevels(), WindowSize=a.getWinSize(),
                       Iterations=a.getNumIters(), PolyN=a.getPolyN(), PolySigma=a.getPolySigma(), Flags=a.getFlags())

    @staticmethod
    def _create():
        return cuda.FarnebackOpticalFlow.create()

    def _impl(self, in0, in1):
        a, p = self._alg, self._p
        a.setPyrScale(p["PyrScale"]); a.setNumLevels(p["LevelsNumber"]); a.setWinSize(p["WindowSize"])
        a.setNumIters(p["Iterations"]); a.setPolyN(p["PolyN"]); a.setPolySigma(p["PolySigma"]); a.setFlags(p["Flags"])
        return a.calc(in0, in1)


class Brox_CUDA(_GpuOpticalFlow):
    """cv::superres::createOptFlow_Brox_CUDA() (optical_flow.cpp:502-586): defaults 0.197, 50, 0.8, 10, 77, 10, parameters pushed into
    the cuda class at every calc (:561-566).  The work type is CV_32FC1 (:540); frames of another type are rejected here (the
    conversion this module has goes to CV_8UC1 only)."""

    def __init__(self):
        self._alg = cuda.BroxOpticalFlow.create(0.197, 50.0, 0.8, 10, 77, 10)
        a = self._alg
        self._p = dict(Alpha=a.getFlowSmoothness(), Gamma=a.getGradientConstancyImportance(), ScaleFactor=a.getPyramidScaleFactor(),
                       InnerIterations=a.getInnerIterations(), OuterIterations=a.getOuterIterations(), SolverIterations=a.getSolverIterations())

    def _create(self):
        p = self._p   # collectGarbage re-creates with the cached parameters, optical_flow.cpp:576-580
        return cuda.BroxOpticalFlow.create(p["Alpha"], p["Gamma"], p["ScaleFactor"], p["InnerIterations"], p["OuterIterations"], p["SolverIterations"])

    def calc(self, frame0, frame1, want_flow2: bool = True):
        import torch
        if frame0.dtype != frame1.dtype or frame0.shape != frame1.shape:
            raise capi.MiError(-3, "frame1.type() == frame0.type() && frame1.size() == frame0.size()")   # optical_flow.cpp:466-467
        if frame0.dtype != torch.float32 or frame0.dim() != 2:
            raise capi.MiError(-2, "Brox_CUDA takes CV_32FC1 frames")
        flow = self._impl(frame0, frame1)
        return splitFlow(flow) if want_flow2 else flow

    def _impl(self, in0, in1):
        a, p = self._alg, self._p
        a.setFlowSmoothness(p["Alpha"]); a.setGradientConstancyImportance(p["Gamma"]); a.setPyramidScaleFactor(p["ScaleFactor"])
        a.setInnerIterations(p["InnerIterations"]); a.setOuterIterations(p["OuterIterations"]); a.setSolverIterations(p["SolverIterations"])
        return a.calc(in0, in1)


def _add_accessors(cls, names):
    for n in names:
        setattr(cls, "get" + n, (lambda n: lambda self: self._p[n])(n))
        setattr(cls, "set" + n, (lambda n: lambda self, val: self._p.__setitem__(n, val))(n))


_add_accessors(DualTVL1_CUDA, ["Tau", "Lambda", "Theta", "ScalesNumber", "WarpingsNumber", "Epsilon", "Iterations", "UseInitialFlow"])
_add_accessors(Brox_CUDA, ["Alpha", "Gamma", "ScaleFactor", "InnerIterations", "OuterIterations", "SolverIterations"])
_add_accessors(Farneback_CUDA, ["PyrScale", "LevelsNumber", "WindowSize", "Iterations", "PolyN", "PolySigma", "Flags"])


def createOptFlow_DualTVL1_CUDA():
    return DualTVL1_CUDA()


def createOptFlow_Brox_CUDA():
    return Brox_CUDA()


def createOptFlow_Farneback_CUDA():
    return Farneback_CUDA()


# ------------------------------------------------------------------------------------------------ BTV-L1 super-resolution
class _EmptyFrameSource:
    """cv::superres::createFrameSource_Empty() (superres/src/frame_source.cpp): nextFrame yields an empty frame."""

    def nextFrame(self):
        return None

    def reset(self):
        pass


class ListFrameSource:
    """A frame source over a sequence of CUDA tensors (the tree has no videoio: video / camera sources are out of scope)."""

    def __init__(self, frames):
        self._frames, self._pos = list(frames), 0

    def nextFrame(self):
        if self._pos >= len(self._frames):
            return None
        self._pos += 1
        return self._frames[self._pos - 1]

    def reset(self):
        self._pos = 0


def createFrameSource_Empty():
    return _EmptyFrameSource()


def createFrameSource_List(frames):
    return ListFrameSource(frames)


def _mats(tensors):
    """list of tensors (None where the reference does not read the entry) -> ctypes array of mi_mat"""
    arr = (capi.Mat * max(len(tensors), 1))()
    for i, t in enumerate(tensors):
        if t is not None:
            arr[i] = _m(t)
    return arr


class BTVL1_CUDA(cuda._Handle):
    """cv::superres::createSuperResolution_BTVL1_CUDA() (btv_l1_cuda.cpp:209-588): BTVL1_CUDA_Base::process behind the C-ABI
    (mi_btvl1_process), the frame ring of BTVL1_CUDA and SuperResolution::nextFrame (super_resolution.cpp) in Python."""

    def __init__(self):
        p = capi.BTVL1Params()
        capi.lib().mi_btvl1_default_params(C.byref(p))
        self._open("btvl1", p)
        self._p = dict(Scale=p.scale, Iterations=p.iterations, Tau=p.tau, Lambda=p.lambda_, Alpha=p.alpha, KernelSize=p.btv_kernel_size,
                       BlurKernelSize=p.blur_kernel_size, BlurSigma=p.blur_sigma, TemporalAreaRadius=4,   # btv_l1_cuda.cpp:461
                       OpticalFlow=createOptFlow_Farneback_CUDA())                                           # btv_l1_cuda.cpp:292
        self._source = createFrameSource_Empty()
        self._first = True

    # ---- BTVL1_CUDA_Base
    def _push_params(self):
        q = self._p
        p = capi.BTVL1Params(q["Scale"], q["Iterations"], q["Tau"], q["Lambda"], q["Alpha"], q["KernelSize"], q["BlurKernelSize"], q["BlurSigma"])
        capi.check(capi.lib().mi_btvl1_set_params(self._h, C.byref(p)))

    @staticmethod
    def _planes(motions, k):
        return [None if m is None else m[k] for m in motions]

    def _args(self, frames, forward, backward):
        n = len(frames)
        forward = list(forward) if forward is not None else [None] * n
        backward = list(backward) if backward is not None else [None] * n
        if n < 1 or len(forward) != n or len(backward) != n:
            raise capi.MiError(-1, "frames, forward and backward motions must have one entry per frame")
        keep = [frames, forward, backward]   # the tensors behind the mi_mat views
        return keep, (_mats(frames), _mats(self._planes(forward, 0)), _mats(self._planes(forward, 1)),
                      _mats(self._planes(backward, 0)), _mats(self._planes(backward, 1)))

    def process(self, frames, forward, backward, baseIdx):
        """BTVL1_CUDA_Base::process (btv_l1_cuda.cpp:306-400).  frames: n float32 CUDA tensors (H, W) or (H, W, 3 | 4); forward /
        backward: n entries (x, y) of float32 (H, W) planes, forward[i] read for i < n - 1 and backward[i] for i > 0 (None elsewhere).
        Returns the high-res frame without its border of KernelSize pixels."""
        import torch
        self._push_params()
        keep, (fr, fx, fy, bx, by) = self._args(frames, forward, backward)
        s, b = self._p["Scale"], self._p["KernelSize"]
        f0 = frames[0]
        shape = (f0.shape[0] * s - 2 * b, f0.shape[1] * s - 2 * b) + tuple(f0.shape[2:])
        if shape[0] <= 0 or shape[1] <= 0:
            raise capi.MiError(-3, "high-res frame not larger than the cropped border of KernelSize pixels")
        dst = torch.empty(shape, dtype=torch.float32, device=f0.device)
        md = _m(dst)
        capi.check(capi.lib().mi_btvl1_process(self._h, len(frames), fr, fx, fy, bx, by, baseIdx, C.byref(md), capi.current_stream_ptr()))
        del keep
        return dst

    def stage(self, frames, forward, backward, baseIdx):
        """mi_btvl1_stage (test hook): ([(forwardMap x, y, backwardMap x, y) per frame], initial estimate, blur taps, BTV weights)."""
        import torch
        self._push_params()
        keep, (fr, fx, fy, bx, by) = self._args(frames, forward, backward)
        s, n, f0 = self._p["Scale"], len(frames), frames[0]
        hh, hw = f0.shape[0] * s, f0.shape[1] * s
        maps = [torch.empty((hh, hw), dtype=torch.float32, device=f0.device) for _ in range(4 * n)]
        init = torch.empty((hh, hw) + tuple(f0.shape[2:]), dtype=torch.float32, device=f0.device)
        taps, weights = (C.c_float * 32)(), (C.c_float * 256)()
        mi = _m(init)
        capi.check(capi.lib().mi_btvl1_stage(self._h, n, fr, fx, fy, bx, by, baseIdx, _mats(maps), C.byref(mi), taps, weights,
                                             capi.current_stream_ptr()))
        del keep
        return [tuple(maps[4 * k:4 * k + 4]) for k in range(n)], init, list(taps), list(weights)

    def getProfile(self):
        """(device milliseconds, kernel launches) of the last process (mi_btvl1_get_profile); waits for it."""
        ms, n = C.c_double(), C.c_longlong()
        capi.check(capi.lib().mi_btvl1_get_profile(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # ---- SuperResolution (superres/src/super_resolution.cpp)
    def setInput(self, source):
        self._source = source
        self._first = True

    def nextFrame(self):
        """uint8 CUDA tensor, or None at the end of the source (the reference's empty frame)."""
        if self._first:
            self._init_impl()
            self._first = False
        return self._process_impl()

    def reset(self):
        self._source.reset()
        self._first = True

    def collectGarbage(self):
        # BTVL1_CUDA::collectGarbage (btv_l1_cuda.cpp:464-481): the ring and the scratch memory go, the parameters stay
        self._frames = self._fwd = self._bwd = self._outputs = None
        self._cur = self._prev = None
        self._p["OpticalFlow"].collectGarbage()
        self._close()
        self._open("btvl1", None, None)   # NULL: the library's defaults; _push_params sends this object's before every process

    # ---- BTVL1_CUDA (btv_l1_cuda.cpp:483-582)
    @staticmethod
    def _at(index, items):
        n = len(items)
        return ((index % n) + n) % n

    def _init_impl(self):
        r = self._p["TemporalAreaRadius"]
        n = 2 * r + 1
        self._frames, self._fwd, self._bwd, self._outputs = [None] * n, [None] * n, [None] * n, [None] * n
        self._store, self._prev = -1, None
        for _ in range(-r, r + 1):
            self._read_next_frame()
        # the reference runs processFrame(0 .. r) whatever the source held and indexes an empty window where it held fewer than
        # r + 1 frames; here only the frames that exist are processed (an empty source then yields no frame at all)
        for i in range(min(r, self._store) + 1):
            self._process_frame(i)
        self._proc, self._out = r, -1

    def _process_impl(self):
        import torch
        if self._out >= self._store:
            return None
        self._read_next_frame()
        if self._proc < self._store:
            self._proc += 1
            self._process_frame(self._proc)
        self._out += 1
        cur = self._outputs[self._at(self._out, self._outputs)]
        return torch.round(cur).clamp_(0, 255).to(torch.uint8)   # convertTo(CV_8U): round to nearest even, saturate

    def _read_next_frame(self):
        import torch
        cur = self._source.nextFrame()
        if cur is None:
            return
        self._store += 1
        self._frames[self._at(self._store, self._frames)] = cur.to(torch.float32).contiguous()   # convertTo(CV_32F)
        if self._store > 0:
            flow = self._p["OpticalFlow"]
            self._fwd[self._at(self._store - 1, self._fwd)] = flow.calc(self._prev, cur)
            self._bwd[self._at(self._store, self._bwd)] = flow.calc(cur, self._prev)
        self._prev = cur.clone()

    def _process_frame(self, idx):
        r = self._p["TemporalAreaRadius"]
        start = max(idx - r, 0)
        end = min(start + 2 * r, self._store)
        frames, fwd, bwd, base = [], [], [], -1
        for i in range(start, end + 1):
            if i == idx:
                base = len(frames)
            frames.append(self._frames[self._at(i, self._frames)])
            fwd.append(self._fwd[self._at(i, self._fwd)] if i < end else None)
            bwd.append(self._bwd[self._at(i, self._bwd)] if i > start else None)
        self._outputs[self._at(idx, self._outputs)] = self.process(frames, fwd, bwd, base)


_add_accessors(BTVL1_CUDA, ["Scale", "Iterations", "Tau", "Lambda", "Alpha", "KernelSize", "BlurKernelSize", "BlurSigma",
                            "TemporalAreaRadius", "OpticalFlow"])


def createSuperResolution_BTVL1_CUDA():
    return BTVL1_CUDA()
