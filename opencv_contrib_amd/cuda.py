"""Python mirror of the reference's `cv2.cuda` classes for the hot path, over the miflow C-ABI.

Names, argument meaning and error behaviour follow the reference headers
(modules/cudaoptflow/include/opencv2/cudaoptflow.hpp:305-386 for OpticalFlowDual_TVL1); device
images are torch CUDA tensors standing in for cv::cuda::GpuMat (pitched row-major; see
capi.mat_from_tensor).  torch is plumbing only: allocation, streams, distributed.
"""
from __future__ import annotations

import ctypes as C

from . import capi
from .capi import MiError


class _Handle:
    """The one owner of a C-ABI handle `_h` and of the parameter struct `_p` the library last accepted, the base of every class here.
    One rule for a setter: copy the struct, ask the library, commit on acceptance; a rejected value leaves the object as it was."""

    def _open(self, prefix, params, *extra):
        """mi_<prefix>_create(&params, *extra, &h); params None: the create takes no struct (its arguments are all in `extra`)."""
        self._h = None
        self._prefix = prefix
        h = C.c_void_p()
        head = () if params is None else (C.byref(params),)
        capi.check(getattr(capi.lib(), f"mi_{prefix}_create")(*head, *extra, C.byref(h)))
        self._h = h
        if params is not None:
            self._p = params

    def _set(self, **kw):
        q = type(self._p).from_buffer_copy(self._p)
        for k, v in kw.items():
            setattr(q, k, v)
        capi.check(getattr(capi.lib(), f"mi_{self._prefix}_set_params")(self._h, C.byref(q)))
        C.memmove(C.byref(self._p), C.byref(q), C.sizeof(q))   # _p keeps its identity: callers hold references to it

    def _close(self):
        """Never raises (interpreter shutdown, failed __init__, library gone); a second call does nothing."""
        try:
            h, self._h = getattr(self, "_h", None), None
            if h:
                getattr(capi.lib(), f"mi_{self._prefix}_destroy")(h)
        except Exception:
            pass

    __del__ = _close


def _stream_ptr(stream):
    return C.c_void_p(stream) if stream is not None else capi.current_stream_ptr()


def _m(t):
    return capi.mat_from_tensor(t)


def _mats(tensors):
    """sequence of tensors (None: an mi_mat with a NULL data pointer) -> ctypes array of mi_mat"""
    return (capi.Mat * len(tensors))(*[_m(t) if t is not None else capi.Mat() for t in tensors])


def release_cached_memory():
    """miflow extension: hand the scratch blocks that destroyed handles left in libmiflow's process-wide cache (up to
    MIFLOW_CACHE_GB, default 24) back to the driver, e.g. before torch's allocator needs the memory."""
    capi.check(capi.lib().mi_release_cached_memory())


class OpticalFlowDual_TVL1(_Handle):
    """cv::cuda::OpticalFlowDual_TVL1 (cudaoptflow.hpp:305-386).

    Extra, non-reference knobs (C-ABI extensions): `semantics` (0 = arithmetic of the CPU class
    cv::optflow::DualTVL1OpticalFlow, the acceptance reference and the DEFAULT; 1 = arithmetic of cv::cuda's kernels),
    `exactMath` (default False: fast device math, fused iterations), `innerIterations`/`medianFiltering` (CPU-class
    parameters), `lanes` (internal streams a batch is split over).
    """

    def __init__(self, params: capi.TVL1Params):
        self._open("tvl1", params)

    # -- factory with the reference's signature and defaults (cudaoptflow.hpp:375-385)
    @staticmethod
    def create(tau=0.25, lambda_=0.15, theta=0.3, nscales=5, warps=5, epsilon=0.01, iterations=300,
               scaleStep=0.8, gamma=0.0, useInitialFlow=False, *, semantics=None, exactMath=None, innerIterations=1,
               medianFiltering=1, timeBlock=0, lanes=0, stopSlack=0, hostFeedback=0) -> "OpticalFlowDual_TVL1":
        """The keyword-only arguments are miflow extensions; None = the library default (mi_tvl1_default_params):
        semantics MI_SEM_CPU_REF (the arithmetic of the CPU class, the acceptance reference; MI_SEM_CUDA_COMPAT = cv::cuda's
        own kernels, ~0.1 px mean EPE away, mostly at borders), fast device math (exactMath=True: IEEE operations in the
        reference's order -- fused in blocks of up to 5 iterations when the work is fixed, bit-identical to one launch per iteration); stopSlack > 0 lets the convergence-checked loop run up to that many
        iterations past the reference's stopping point (mi_tvl1_params.stop_slack)."""
        p = capi.TVL1Params()
        capi.lib().mi_tvl1_default_params(C.byref(p))
        p.tau, p.lambda_, p.theta, p.nscales, p.warps = tau, lambda_, theta, nscales, warps
        p.epsilon, p.iterations, p.scale_step, p.gamma = epsilon, iterations, scaleStep, gamma
        p.use_initial_flow = int(bool(useInitialFlow))
        if semantics is not None:
            p.semantics = semantics
        if exactMath is not None:
            p.exact_math = int(bool(exactMath))
        p.inner_iterations, p.median_filtering, p.time_block, p.lanes = innerIterations, medianFiltering, timeBlock, lanes
        p.stop_slack = stopSlack
        p.host_feedback = hostFeedback   # 0 automatic (a call of <= 2 pairs reads the converged flags back between launches), -1 never, 1 every single-lane call
        return OpticalFlowDual_TVL1(p)

    def getDefaultName(self) -> str:  # cudaoptflow/src/tvl1flow.cpp:122
        return "DenseOpticalFlow.OpticalFlowDual_TVL1"

    # getters / setters, cudaoptflow/src/tvl1flow.cpp:90-118
    def getTau(self): return self._p.tau
    def setTau(self, v): self._set(tau=v)
    def getLambda(self): return self._p.lambda_
    def setLambda(self, v): self._set(lambda_=v)
    def getGamma(self): return self._p.gamma
    def setGamma(self, v): self._set(gamma=v)
    def getTheta(self): return self._p.theta
    def setTheta(self, v): self._set(theta=v)
    def getNumScales(self): return self._p.nscales
    def setNumScales(self, v): self._set(nscales=v)
    def getNumWarps(self): return self._p.warps
    def setNumWarps(self, v): self._set(warps=v)
    def getEpsilon(self): return self._p.epsilon
    def setEpsilon(self, v): self._set(epsilon=v)
    def getNumIterations(self): return self._p.iterations
    def setNumIterations(self, v): self._set(iterations=v)
    def getScaleStep(self): return self._p.scale_step
    def setScaleStep(self, v): self._set(scale_step=v)
    def getUseInitialFlow(self): return bool(self._p.use_initial_flow)
    def setUseInitialFlow(self, v): self._set(use_initial_flow=int(bool(v)))

    def calc(self, I0, I1, flow=None, stream=None):
        """DenseOpticalFlow::calc(I0, I1, flow, stream) (cudaoptflow.hpp:80).  Returns flow (H,W,2) f32."""
        import torch
        if flow is None:
            if self._p.use_initial_flow:
                raise MiError(-1, "useInitialFlow requires a flow argument")
            flow = torch.empty((I0.shape[0], I0.shape[1], 2), dtype=torch.float32, device=I0.device)
        m0, m1, mf = capi.mat_from_tensor(I0), capi.mat_from_tensor(I1), capi.mat_from_tensor(flow)
        sp = _stream_ptr(stream)
        capi.check(capi.lib().mi_tvl1_calc(self._h, C.byref(m0), C.byref(m1), C.byref(mf), sp))
        capi.check(capi.lib().mi_tvl1_get_params(self._h, C.byref(self._p)))   # nscales shrinks like the reference's nscales_
        return flow

    def calc_batch(self, I0s, I1s, flows=None, stream=None):
        """n independent pairs in one pass (batched-frames mode).  I0s/I1s: sequences of tensors, or
        one (N,H,W) tensor each; flows: list or (N,H,W,2)."""
        import torch
        n = len(I0s)
        if flows is None:
            flows = torch.empty((n, I0s[0].shape[0], I0s[0].shape[1], 2), dtype=torch.float32, device=I0s[0].device)
        A0 = _mats(I0s)
        A1 = _mats(I1s)
        AF = _mats(flows)
        sp = _stream_ptr(stream)
        capi.check(capi.lib().mi_tvl1_calc_batch(self._h, n, A0, A1, AF, sp))
        capi.check(capi.lib().mi_tvl1_get_params(self._h, C.byref(self._p)))
        return flows

    def setProfiling(self, on=True):
        capi.check(capi.lib().mi_tvl1_set_profiling(self._h, int(bool(on))))

    def getProfile(self, kind=0, level=-1):
        """(ms inside the iteration-launch regions [kind 0] or the warp launches [kind 1], launches, algorithmic bytes) of the
        last calc; level >= 0 restricts it to one pyramid level (0 = finest)."""
        ms, n, by = C.c_double(), C.c_longlong(), C.c_double()
        capi.check(capi.lib().mi_tvl1_get_profile_level(self._h, kind, level, C.byref(ms), C.byref(n), C.byref(by)))
        return ms.value, n.value, by.value

    def lastIterations(self, pair=0):
        """Executed inner iterations [scale][warp] of the last calc (epsilon > 0: device-decided)."""
        ns = C.c_int()
        cap = 32 * 64
        buf = (C.c_int * cap)()
        capi.check(capi.lib().mi_tvl1_last_iterations(self._h, pair, C.byref(ns), buf, cap, capi.current_stream_ptr()))
        nw = self._p.warps
        return [[buf[s * nw + w] for w in range(nw)] for s in range(ns.value)]


BROX_FORM_AUTO, BROX_FORM_PLAIN, BROX_FORM_BLOCKED = 0, 1, 2


class BroxOpticalFlow(_Handle):
    """cv::cuda::BroxOpticalFlow (cudaoptflow.hpp:155-186; cudaoptflow/src/brox.cpp, cudalegacy/src/cuda/NCVBroxOpticalFlow.cu).
    CV_32FC1 frames, each side at least 4; every result is the reference's kernels' bit for bit."""

    def __init__(self, alpha=0.197, gamma=50.0, scale_factor=0.8, inner_iterations=5, outer_iterations=150, solver_iterations=10):
        self._open("brox", capi.BroxParams(float(alpha), float(gamma), float(scale_factor), int(inner_iterations), int(outer_iterations),
                                           int(solver_iterations)))

    @staticmethod
    def create(alpha=0.197, gamma=50.0, scale_factor=0.8, inner_iterations=5, outer_iterations=150, solver_iterations=10):
        return BroxOpticalFlow(alpha, gamma, scale_factor, inner_iterations, outer_iterations, solver_iterations)

    def getDefaultName(self) -> str:
        return "DenseOpticalFlow.BroxOpticalFlow"   # cudaoptflow/src/brox.cpp:67

    def getFlowSmoothness(self): return float(self._p.alpha)
    def setFlowSmoothness(self, v): self._set(alpha=float(v))
    def getGradientConstancyImportance(self): return float(self._p.gamma)
    def setGradientConstancyImportance(self, v): self._set(gamma=float(v))
    def getPyramidScaleFactor(self): return float(self._p.scale_factor)
    def setPyramidScaleFactor(self, v): self._set(scale_factor=float(v))
    def getInnerIterations(self): return self._p.inner_iterations
    def setInnerIterations(self, v): self._set(inner_iterations=int(v))
    def getOuterIterations(self): return self._p.outer_iterations
    def setOuterIterations(self, v): self._set(outer_iterations=int(v))
    def getSolverIterations(self): return self._p.solver_iterations
    def setSolverIterations(self, v): self._set(solver_iterations=int(v))

    def setSolverForm(self, form):
        """miflow extension: BROX_FORM_AUTO (the plan's rule), BROX_FORM_PLAIN or BROX_FORM_BLOCKED; the bits do not depend on it"""
        capi.check(capi.lib().mi_brox_set_form(self._h, int(form)))

    def scratchBytes(self):
        b = C.c_size_t()
        capi.check(capi.lib().mi_brox_scratch_bytes(self._h, C.byref(b)))
        return b.value

    def calc(self, I0, I1, flow=None, stream=None):
        """DenseOpticalFlow::calc(I0, I1, flow, stream) (cudaoptflow.hpp:80).  Returns flow (H,W,2) f32; what `flow` held is ignored."""
        import torch
        if flow is None:
            flow = torch.empty((I0.shape[0], I0.shape[1], 2), dtype=torch.float32, device=I0.device)
        capi.check(capi.lib().mi_brox_calc(self._h, C.byref(_m(I0)), C.byref(_m(I1)), C.byref(_m(flow)), _stream_ptr(stream)))
        return flow


def brox_plan_info(rows, cols, form=BROX_FORM_AUTO, **params):
    """miflow extension, host only: (levels, launches, solver launches) of a calc at rows x cols; raises what calc would"""
    p = capi.BroxParams()
    capi.lib().mi_brox_default_params(C.byref(p))
    for k, v in params.items():
        setattr(p, k, v)
    n = [C.c_int() for _ in range(3)]
    capi.check(capi.lib().mi_brox_plan_info(C.byref(p), int(rows), int(cols), int(form), *[C.byref(x) for x in n]))
    return tuple(x.value for x in n)


def _like(t, rows=None, cols=None):
    import torch
    return torch.empty((t.shape[0] if rows is None else rows, t.shape[1] if cols is None else cols), dtype=torch.float32, device=t.device)


def brox_resize_down(src, rows, cols, scale_factor, dst=None):
    """Stage entry: the pyramid's supersample resize to rows x cols with factor scale_factor"""
    dst = _like(src, rows, cols) if dst is None else dst
    capi.check(capi.lib().mi_brox_resize_down(C.byref(_m(src)), C.byref(_m(dst)), float(scale_factor), capi.current_stream_ptr()))
    return dst


def brox_resize_up(src, rows, cols, scale_factor, dst=None):
    """Stage entry: the bicubic prolongation to rows x cols, times 1 / scale_factor"""
    dst = _like(src, rows, cols) if dst is None else dst
    capi.check(capi.lib().mi_brox_resize_up(C.byref(_m(src)), C.byref(_m(dst)), float(scale_factor), capi.current_stream_ptr()))
    return dst


def brox_derivatives(i0, i1, planes=None):
    """Stage entry -> [Ix0, Iy0, Ix, Iy, Ixx, Iyy, Ixy]"""
    planes = [_like(i0) for _ in range(7)] if planes is None else planes
    capi.check(capi.lib().mi_brox_derivatives(C.byref(_m(i0)), C.byref(_m(i1)), _mats(planes), capi.current_stream_ptr()))
    return planes


def brox_prepare(u, v, du, dv, images, alpha, gamma, coeffs=None):
    """Stage entry.  images: [I0, I1, Ix, Ixx, Ix0, Iy, Iyy, Iy0, Ixy] -> [diffusivity_x, diffusivity_y, inv_denominator_u,
    inv_denominator_v, numerator_dudv, numerator_u, numerator_v] after stage 2"""
    coeffs = [_like(u) for _ in range(7)] if coeffs is None else coeffs
    capi.check(capi.lib().mi_brox_prepare(C.byref(_m(u)), C.byref(_m(v)), C.byref(_m(du)), C.byref(_m(dv)), _mats(images), float(alpha),
                                          float(gamma), _mats(coeffs), capi.current_stream_ptr()))
    return coeffs


def brox_sor(u, v, du, dv, coeffs, solver_iterations, form=BROX_FORM_AUTO):
    """Stage entry: du, dv are overwritten with the result of solver_iterations red-black SOR iterations -> (du, dv)"""
    capi.check(capi.lib().mi_brox_sor(C.byref(_m(u)), C.byref(_m(v)), C.byref(_m(du)), C.byref(_m(dv)), _mats(coeffs), int(form),
                                      int(solver_iterations), capi.current_stream_ptr()))
    return du, dv


class TVL1MultiDevice(_Handle):
    """Batched-frames mode over the GPUs of one node through the C-ABI (mi_tvl1_multi_*): contiguous shards of independent pairs,
    one host thread + handle + stream pair per device, staging from / to the ROOT device (devices[0]) over RCCL point-to-point
    messages (where librccl is present and the worker sits on another GPU) or peer-to-peer copies; no reduction.
    `alg` is an OpticalFlowDual_TVL1 whose parameters are used (create it with the reference's factory arguments).
    The same device id may appear several times (several workers on one GPU)."""

    def __init__(self, alg: "OpticalFlowDual_TVL1", devices=None, chunk=16):
        ids = None if devices is None else (C.c_int * len(devices))(*devices)
        self._open("tvl1_multi", None, C.byref(alg._p), 0 if devices is None else len(devices), ids)   # alg keeps its parameters: no _p here
        capi.check(capi.lib().mi_tvl1_multi_set_chunk(self._h, chunk))

    def deviceCount(self):
        return capi.lib().mi_tvl1_multi_device_count(self._h)

    def transport(self):
        """(workers linked to the root over RCCL, workers using peer copies)."""
        a, b = C.c_int(), C.c_int()
        capi.check(capi.lib().mi_tvl1_multi_transport(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    @staticmethod
    def transportWhy():
        """Why the most recent link of this process fell back to peer copies ("" if none did)."""
        return (capi.lib().mi_tvl1_multi_transport_why() or b"").decode()

    def calc_batch(self, I0s, I1s, flows=None):
        """All tensors on the root device.  Synchronous: earlier work on the inputs must be complete (synchronised here)."""
        import torch
        n = len(I0s)
        if flows is None:
            flows = torch.empty((n, I0s[0].shape[0], I0s[0].shape[1], 2), dtype=torch.float32, device=I0s[0].device)
        torch.cuda.synchronize()
        A0 = _mats(I0s)
        A1 = _mats(I1s)
        AF = _mats(flows)
        capi.check(capi.lib().mi_tvl1_multi_calc_batch(self._h, n, A0, A1, AF))
        return flows


# ---------------------------------------------------------------------------------------------
# stage-level functions (the reference's internal device-layer boundary), used by parity tests
def tvl1_centeredGradient(src):
    import torch
    dx, dy = torch.empty_like(src), torch.empty_like(src)
    capi.check(capi.lib().mi_tvl1_centered_gradient(C.byref(_m(src)), C.byref(_m(dx)), C.byref(_m(dy)), capi.current_stream_ptr()))
    return dx, dy


def tvl1_warpBackward(semantics, I0, I1, I1x, I1y, u1, u2):
    """I1x = I1y = None: the derivative planes are formed from I1 inside the kernel (the kernel calc() runs)."""
    import torch
    torch.cuda.synchronize()
    outs = [torch.empty_like(I0) for _ in range(5)]
    args = [C.byref(_m(t)) if t is not None else None for t in (I0, I1, I1x, I1y, u1, u2, *outs)]
    capi.check(capi.lib().mi_tvl1_warp_backward(semantics, *args))
    return tuple(outs)


def tvl1_iterate(I1wx, I1wy, grad, rho_c, u, p, l_t, theta, taut, niter=1, exact=True, time_block=0, want_err=True):
    """u: [u1,u2], p: [p11,p12,p21,p22] -> (u_out, p_out, err[niter])."""
    import torch
    u_out = [torch.empty_like(t) for t in u]
    p_out = [torch.empty_like(t) for t in p]
    U = (capi.Mat * 2)(*[_m(t) for t in u]); P = (capi.Mat * 4)(*[_m(t) for t in p])
    UO = (capi.Mat * 2)(*[_m(t) for t in u_out]); PO = (capi.Mat * 4)(*[_m(t) for t in p_out])
    err = (C.c_double * niter)()
    capi.check(capi.lib().mi_tvl1_iterate(int(exact), time_block, niter, C.byref(_m(I1wx)), C.byref(_m(I1wy)),
                                          C.byref(_m(grad)), C.byref(_m(rho_c)), U, P, UO, PO, l_t, theta, taut,
                                          err if want_err else None, capi.current_stream_ptr()))
    torch.cuda.synchronize()
    return u_out, p_out, list(err)


_STAGE_FORMS = {"one": capi.MI_TVL1_STAGE_ONE, "blocked": capi.MI_TVL1_STAGE_BLOCKED, "indep": capi.MI_TVL1_STAGE_INDEP,
                "tile": capi.MI_TVL1_STAGE_TILE, "exact_blocked": capi.MI_TVL1_STAGE_EXACT_BLOCKED, "spec": capi.MI_TVL1_STAGE_SPEC,
                "spec_tile": capi.MI_TVL1_STAGE_SPEC_TILE}


def tvl1_iterate_stage(form, I1wx, I1wy, grad, rho_c, u, p, l_t, theta, taut, niter=1, *, exact=False, time_block=0, blocks=None,
                       rows_per_band=0, variant=0, p_zero=False, gamma=0.0, err_u3=0, want_err=False):
    """The iterations in one of the forms calc() runs them (mi_tvl1_iterate_stage).  form: 'one' | 'blocked' | 'indep' | 'tile' |
    'exact_blocked' | 'spec' | 'spec_tile'.  Planes are (h, w) or (B, h, w) float32 CUDA tensors (B pairs in one launch); grad may
    be None (the pass forms |grad|^2); u = [u1, u2(, u3)], p = [p11, p12, p21, p22(, p31, p32)] (p may be None with p_zero).
    Returns (u_out, p_out, err) -- err: per pair the per-iteration error sums as 2^-24 fixed-point ints (want_err), else None."""
    import torch
    B = I1wx.shape[0] if I1wx.dim() == 3 else 1
    flat = lambda t: t.reshape(-1, t.shape[-1]) if t is not None else None   # (B, h, w) -> (B*h, w): the pairs stacked
    gam = gamma != 0.0
    nu, np_ = (3, 6) if gam else (2, 4)
    u_out = [torch.empty_like(t) for t in u[:nu]]
    p_out = [torch.empty_like(u[0]) for _ in range(np_)]
    ms = lambda ts, n: (capi.Mat * 6)(*[_m(flat(t)) for t in ts[:n]])
    U, UO, PO = ms(u, nu), ms(u_out, nu), ms(p_out, np_)
    P = ms(p, np_) if p is not None else None
    stat = [_m(flat(t)) if t is not None else None for t in (I1wx, I1wy, grad, rho_c)]
    d = capi.TVL1StageDesc()
    d.form, d.exact_math, d.niter, d.time_block = _STAGE_FORMS[form], int(exact), niter, time_block
    blk = (C.c_int * len(blocks))(*blocks) if blocks else None
    if blk is not None:
        d.blocks, d.nblocks = C.cast(blk, C.POINTER(C.c_int)), len(blocks)
    d.rows_per_band, d.variant, d.p_zero, d.batch = rows_per_band, variant, int(bool(p_zero)), B
    d.l_t, d.theta, d.taut, d.gamma, d.err_u3 = l_t, theta, taut, gamma, int(err_u3)
    ref = lambda m: C.pointer(m) if m is not None else None
    d.I1wx, d.I1wy, d.grad, d.rho_c = (ref(m) for m in stat)
    d.u_in, d.u_out, d.p_out = C.cast(U, C.POINTER(capi.Mat)), C.cast(UO, C.POINTER(capi.Mat)), C.cast(PO, C.POINTER(capi.Mat))
    d.p_in = C.cast(P, C.POINTER(capi.Mat)) if P is not None else None
    err = (C.c_ulonglong * (niter * B))() if want_err else None
    if err is not None:
        d.err_fix = C.cast(err, C.POINTER(C.c_ulonglong))
    capi.check(capi.lib().mi_tvl1_iterate_stage(C.byref(d), capi.current_stream_ptr()))
    torch.cuda.synchronize()
    errs = [[int(v) for v in err[b * niter:(b + 1) * niter]] for b in range(B)] if want_err else None
    return u_out, p_out, errs


def resize_linear(src, dsize=None, fx=0.0, fy=0.0, semantics=capi.MI_SEM_CPU_REF, post_scale=1.0):
    """cv::resize / cv::cuda::resize (INTER_LINEAR, CV_32FC1).  dsize = (width, height)."""
    import torch
    h, w = src.shape
    if dsize is None:
        dw, dh = int(round_half_even(w * fx)), int(round_half_even(h * fy))
        explicit = 0
    else:
        dw, dh = dsize
        explicit = 1
    dst = torch.empty((dh, dw), dtype=torch.float32, device=src.device)
    capi.check(capi.lib().mi_resize_linear(semantics, C.byref(_m(src)), C.byref(_m(dst)), fx, fy, explicit,
                                           post_scale, capi.current_stream_ptr()))
    return dst


def round_half_even(v: float) -> int:
    import numpy as np
    return int(np.rint(v))


# =============================================================================================
class StereoBM(_Handle):
    """cv::cuda::StereoBM (cudastereo.hpp:72-90; StereoBMImpl cudastereo/src/stereobm.cpp:67-132).

    Setters that are no-ops in the reference (minDisparity, speckle*, disp12MaxDiff, smallerBlockSize,
    ROI1/2: stereobm.cpp:78-115) are no-ops here and their getters return the same constants."""

    PREFILTER_NORMALIZED_RESPONSE, PREFILTER_XSOBEL = 0, 1  # cv::StereoBM (main repo calib3d.hpp)

    def __init__(self, numDisparities=64, blockSize=19, *, emulateCudaEdge=True):
        p = capi.StereoBMParams()
        capi.lib().mi_stereobm_default_params(C.byref(p))
        p.num_disparities, p.block_size, p.emulate_cuda_edge = numDisparities, blockSize, int(bool(emulateCudaEdge))
        self._open("stereobm", p)

    def getMinDisparity(self): return 0
    def setMinDisparity(self, v): pass
    def getNumDisparities(self): return self._p.num_disparities
    def setNumDisparities(self, v): self._set(num_disparities=v)
    def getBlockSize(self): return self._p.block_size
    def setBlockSize(self, v): self._set(block_size=v)
    def getSpeckleWindowSize(self): return 0
    def setSpeckleWindowSize(self, v): pass
    def getSpeckleRange(self): return 0
    def setSpeckleRange(self, v): pass
    def getDisp12MaxDiff(self): return 0
    def setDisp12MaxDiff(self, v): pass
    def getPreFilterType(self): return self._p.prefilter_type
    def setPreFilterType(self, v): self._set(prefilter_type=v)
    def getPreFilterSize(self): return self._p.prefilter_size
    def setPreFilterSize(self, v): self._set(prefilter_size=v)
    def getPreFilterCap(self): return self._p.prefilter_cap
    def setPreFilterCap(self, v): self._set(prefilter_cap=v)
    def getTextureThreshold(self): return int(self._p.texture_threshold)
    def setTextureThreshold(self, v): self._set(texture_threshold=float(v))
    def getUniquenessRatio(self): return self._p.uniqueness_ratio
    def setUniquenessRatio(self, v): self._set(uniqueness_ratio=v)
    def getSmallerBlockSize(self): return 0
    def setSmallerBlockSize(self, v): pass

    def compute(self, left, right, disparity=None, stream=None):
        """compute(left, right, disparity[, stream]) (cudastereo.hpp:80-82).  Returns CV_8UC1 disparity."""
        import torch
        if disparity is None:  # _disparity.create(left.size(), CV_8UC1)  stereobm.cpp:154
            disparity = torch.empty((left.shape[0], left.shape[1]), dtype=torch.uint8, device=left.device)
        ml, mr, md = capi.mat_from_tensor(left), capi.mat_from_tensor(right), capi.mat_from_tensor(disparity)
        sp = _stream_ptr(stream)
        capi.check(capi.lib().mi_stereobm_compute(self._h, C.byref(ml), C.byref(mr), C.byref(md), sp))
        return disparity

    def compute_batch(self, lefts, rights, disparities=None, stream=None):
        """n stereo pairs through one handle (miflow extension): sequences of tensors or (N,H,W) tensors."""
        import torch
        n = len(lefts)
        if disparities is None:
            disparities = torch.empty((n, lefts[0].shape[0], lefts[0].shape[1]), dtype=torch.uint8, device=lefts[0].device)
        AL = _mats(lefts)
        AR = _mats(rights)
        AD = _mats(disparities)
        sp = _stream_ptr(stream)
        capi.check(capi.lib().mi_stereobm_compute_batch(self._h, n, AL, AR, AD, sp))
        return disparities


def createStereoBM(numDisparities=64, blockSize=19, **kw) -> StereoBM:
    """cv::cuda::createStereoBM (cudastereo.hpp:90)."""
    return StereoBM(numDisparities, blockSize, **kw)


class DensePyrLKOpticalFlow(_Handle):
    """cv::cuda::DensePyrLKOpticalFlow (cudaoptflow.hpp; cudaoptflow/src/pyrlk.cpp:238-299,354-406)."""

    def __init__(self, winSize=(13, 13), maxLevel=3, iters=30, useInitialFlow=False):
        p = capi.DensePyrLKParams()
        capi.lib().mi_densepyrlk_default_params(C.byref(p))
        p.win_width, p.win_height, p.max_level, p.iters = winSize[0], winSize[1], maxLevel, iters
        p.use_initial_flow = int(bool(useInitialFlow))
        self._open("densepyrlk", p)

    @classmethod
    def create(cls, winSize=(13, 13), maxLevel=3, iters=30, useInitialFlow=False):
        return cls(winSize, maxLevel, iters, useInitialFlow)

    def getDefaultName(self): return "DenseOpticalFlow.DensePyrLKOpticalFlow"   # pyrlk.cpp:394
    def getWinSize(self): return (self._p.win_width, self._p.win_height)
    def setWinSize(self, v): self._set(win_width=v[0], win_height=v[1])
    def getMaxLevel(self): return self._p.max_level
    def setMaxLevel(self, v): self._set(max_level=v)
    def getNumIters(self): return self._p.iters
    def setNumIters(self, v): self._set(iters=v)
    def getUseInitialFlow(self): return bool(self._p.use_initial_flow)
    def setUseInitialFlow(self, v): self._set(use_initial_flow=int(bool(v)))

    def calc(self, prevImg, nextImg, flow=None):
        import torch
        if flow is None:
            flow = torch.empty((prevImg.shape[0], prevImg.shape[1], 2), dtype=torch.float32, device=prevImg.device)
        capi.check(capi.lib().mi_densepyrlk_calc(self._h, C.byref(_m(prevImg)), C.byref(_m(nextImg)), C.byref(_m(flow)),
                                                 capi.current_stream_ptr()))
        return flow


class SparsePyrLKOpticalFlow(_Handle):
    """cv::cuda::SparsePyrLKOpticalFlow for CV_8UC1 frames (cudaoptflow.hpp:85-104,203-223; cudaoptflow/src/pyrlk.cpp:149-231,308-352).
    calc(prevImg, nextImg, prevPts (1, N, 2) or (N, 2) float32[, nextPts]) -> (nextPts (1, N, 2), status (1, N) uint8, err (1, N))."""

    def __init__(self, winSize=(21, 21), maxLevel=3, iters=30, useInitialFlow=False):
        p = capi.SparsePyrLKParams()
        capi.lib().mi_sparsepyrlk_default_params(C.byref(p))
        p.win_width, p.win_height, p.max_level, p.iters = winSize[0], winSize[1], maxLevel, iters
        p.use_initial_flow = int(bool(useInitialFlow))
        self._open("sparsepyrlk", p)

    @classmethod
    def create(cls, winSize=(21, 21), maxLevel=3, iters=30, useInitialFlow=False):
        return cls(winSize, maxLevel, iters, useInitialFlow)

    def getDefaultName(self): return "SparseOpticalFlow.SparsePyrLKOpticalFlow"   # pyrlk.cpp:350
    def getWinSize(self): return (self._p.win_width, self._p.win_height)
    def setWinSize(self, v): self._set(win_width=v[0], win_height=v[1])
    def getMaxLevel(self): return self._p.max_level
    def setMaxLevel(self, v): self._set(max_level=v)
    def getNumIters(self): return self._p.iters
    def setNumIters(self, v): self._set(iters=v)
    def getUseInitialFlow(self): return bool(self._p.use_initial_flow)
    def setUseInitialFlow(self, v): self._set(use_initial_flow=int(bool(v)))

    def calc(self, prevImg, nextImg, prevPts, nextPts=None, wantErr=True):
        import torch
        pp = prevPts.reshape(1, -1, 2).contiguous()
        n = pp.shape[1]
        if n == 0:      # pyrlk.cpp:209-215: empty input releases the outputs
            e = torch.empty((1, 0), device=prevImg.device)
            return torch.empty((1, 0, 2), device=prevImg.device), e.to(torch.uint8), (e if wantErr else None)
        if self._p.use_initial_flow:
            if nextPts is None or nextPts.numel() != pp.numel():
                raise capi.MiError(-1, "nextPts.size() == prevPts.size() (useInitialFlow)")   # :160
            npts = nextPts.reshape(1, -1, 2).contiguous().clone()
        else:
            npts = torch.empty_like(pp)
        status = torch.empty((1, n), dtype=torch.uint8, device=prevImg.device)
        err = torch.empty((1, n), dtype=torch.float32, device=prevImg.device) if wantErr else None
        capi.check(capi.lib().mi_sparsepyrlk_calc(self._h, C.byref(_m(prevImg)), C.byref(_m(nextImg)), C.byref(_m(pp)), C.byref(_m(npts)),
                                                  C.byref(_m(status)), C.byref(_m(err)) if wantErr else None, capi.current_stream_ptr()))
        return npts, status, err


class StereoSGM(_Handle):
    """cv::cuda::StereoSGM (cudastereo.hpp; cudastereo/src/stereosgm.cpp:20-153): semi-global matching on census costs,
    4 (MODE_HH4) or 8 (MODE_HH) paths, CV_16SC1 output with 4 fractional bits."""

    MODE_HH, MODE_HH4 = 1, 3

    def __init__(self, minDisparity=0, numDisparities=128, P1=10, P2=120, uniquenessRatio=5, mode=3, emulateCudaQuirks=True):
        p = capi.StereoSGMParams()
        capi.lib().mi_stereosgm_default_params(C.byref(p))
        p.min_disparity, p.num_disparities, p.P1, p.P2 = minDisparity, numDisparities, P1, P2
        p.uniqueness_ratio, p.mode, p.emulate_cuda_quirks = uniquenessRatio, mode, int(bool(emulateCudaQuirks))
        self._open("stereosgm", p)

    # stereosgm.cpp:38-72 (the fixed getters of the reference included)
    def getBlockSize(self): return -1
    def setBlockSize(self, v): pass
    def getDisp12MaxDiff(self): return 1
    def setDisp12MaxDiff(self, v): pass
    def getMinDisparity(self): return self._p.min_disparity
    def setMinDisparity(self, v): self._set(min_disparity=v)
    def getNumDisparities(self): return self._p.num_disparities
    def setNumDisparities(self, v): self._set(num_disparities=v)
    def getSpeckleWindowSize(self): return 0
    def setSpeckleWindowSize(self, v): pass
    def getSpeckleRange(self): return 0
    def setSpeckleRange(self, v): pass
    def getP1(self): return self._p.P1
    def setP1(self, v): self._set(P1=v)
    def getP2(self): return self._p.P2
    def setP2(self, v): self._set(P2=v)
    def getUniquenessRatio(self): return self._p.uniqueness_ratio
    def setUniquenessRatio(self, v): self._set(uniqueness_ratio=v)
    def getMode(self): return self._p.mode
    def setMode(self, v): self._set(mode=v)
    def getPreFilterCap(self): return -1
    def setPreFilterCap(self, v): pass

    def compute(self, left, right, disparity=None):
        import torch
        if disparity is None:
            disparity = torch.empty(left.shape[:2], dtype=torch.int16, device=left.device)
        capi.check(capi.lib().mi_stereosgm_compute(self._h, C.byref(_m(left)), C.byref(_m(right)), C.byref(_m(disparity)),
                                                   capi.current_stream_ptr()))
        return disparity


def createStereoSGM(minDisparity=0, numDisparities=128, P1=10, P2=120, uniquenessRatio=5, mode=3, **kw) -> StereoSGM:
    """cv::cuda::createStereoSGM (cudastereo.hpp)."""
    return StereoSGM(minDisparity, numDisparities, P1, P2, uniquenessRatio, mode, **kw)


def sgm_census(img):
    import torch
    out = torch.empty(img.shape, dtype=torch.int32, device=img.device)
    capi.check(capi.lib().mi_sgm_census(C.byref(_m(img)), C.byref(_m(out)), capi.current_stream_ptr()))
    return out


def sgm_aggregate_path(left_census, right_census, num_disparities, min_disparity, p1, p2, dx, dy):
    import torch
    h, w = left_census.shape
    out = torch.empty((1, h * w * num_disparities), dtype=torch.uint8, device=left_census.device)
    capi.check(capi.lib().mi_sgm_aggregate_path(C.byref(_m(left_census)), C.byref(_m(right_census)), C.byref(_m(out)), num_disparities,
                                                min_disparity, p1, p2, dx, dy, capi.current_stream_ptr()))
    return out


def sgm_winner_takes_all(aggregated, width, height, num_disparities, num_paths, uniqueness, subpixel):
    import torch
    left = torch.empty((height, width), dtype=torch.int16, device=aggregated.device)
    right = torch.empty_like(left)
    capi.check(capi.lib().mi_sgm_winner_takes_all(C.byref(_m(aggregated)), C.byref(_m(left)), C.byref(_m(right)), num_disparities, num_paths,
                                                  C.c_float(uniqueness), int(subpixel), capi.current_stream_ptr()))
    return left, right


class DMatch:
    """cv::DMatch (queryIdx, trainIdx, imgIdx, distance); ordered by distance like the reference's operator<."""
    __slots__ = ("queryIdx", "trainIdx", "imgIdx", "distance")

    def __init__(self, queryIdx=-1, trainIdx=-1, imgIdx=-1, distance=float("inf")):
        self.queryIdx, self.trainIdx, self.imgIdx, self.distance = int(queryIdx), int(trainIdx), int(imgIdx), float(distance)

    def __lt__(self, other):
        return self.distance < other.distance

    def __repr__(self):
        return f"DMatch(queryIdx={self.queryIdx}, trainIdx={self.trainIdx}, imgIdx={self.imgIdx}, distance={self.distance:.6g})"


def _nonempty(tensors):
    """an empty tensor of a train or mask collection goes to the library like a missing one"""
    return [t if t is not None and t.numel() else None for t in tensors]


class BFMatcher(_Handle):
    """cv::cuda::DescriptorMatcher::createBFMatcher(NORM_L1 | NORM_L2 | NORM_HAMMING): float descriptors (L1 / L2) and integer ones
    (L1 / Hamming: the reference's (depth, norm) table) (cudafeatures2d.hpp;
    cudafeatures2d/src/brute_force_matcher.cpp:143-1070; kernels cuda/bf_match.cu, bf_knnmatch.cu, bf_radius_match.cu).

    Three forms of every query, like the reference: `match / knnMatch / radiusMatch` return DMatch lists (host),
    `*Async` return the reference's packed device matrix and `*Convert` unpack it; `*Device` return the separate device tensors
    the C-ABI fills (no host transfer).  With `trainDescriptors=None` the collection added with add() is searched."""

    NORM_L1 = 2
    NORM_L2 = 4
    NORM_HAMMING = 6      # integer descriptors (uint8 / uint16 / int32); NORM_L1 also takes uint8 / uint16 / int16 / int32
    _mats = staticmethod(_mats)   # the module's array builder under the name callers of the C-ABI know (tests reach it as BFMatcher._mats)

    def __init__(self, normType=4):
        self._open("bf", None, int(normType))   # the norm type is its only parameter, fixed at create
        self._train = []

    # ---- train collection (brute_force_matcher.cpp:187-211)
    def isMaskSupported(self): return True
    def add(self, descriptors): self._train.extend(descriptors)
    def getTrainDescriptors(self): return self._train
    def clear(self): self._train = []
    def empty(self): return not self._train
    def train(self): pass

    def _collection(self, train, mask, masks):
        """-> (trains list, masks list or None, is_collection)"""
        if train is not None:
            return [train], ([mask] if mask is not None else None), False
        if masks is not None and len(masks) and len(masks) != len(self._train):
            raise capi.MiError(-1, "masks.size() == trainDescCollection.size()")          # makeGpuCollection, :156
        return list(self._train), (list(masks) if masks else None), True

    # ---- device forms
    def knnMatchDevice(self, queryDescriptors, trainDescriptors=None, k=2, mask=None, masks=None):
        """-> (trainIdx (nq, k) int32, imgIdx (nq, k) int32, distance (nq, k) float32); entries past the candidates -1 / -1 / FLT_MAX."""
        import torch
        trains, ms, _ = self._collection(trainDescriptors, mask, masks)
        q = queryDescriptors
        if q.numel() == 0 or not trains:
            e = torch.empty((0, k), dtype=torch.int32, device=q.device)
            return e, e.clone(), torch.empty((0, k), dtype=torch.float32, device=q.device)
        nq = q.shape[0]
        idx = torch.empty((nq, k), dtype=torch.int32, device=q.device)
        img = torch.empty((nq, k), dtype=torch.int32, device=q.device)
        dist = torch.empty((nq, k), dtype=torch.float32, device=q.device)
        capi.check(capi.lib().mi_bf_knn_match(self._h, C.byref(_m(q)), _mats(_nonempty(trains)), _mats(_nonempty(ms)) if ms else None, len(trains), int(k),
                                              C.byref(_m(idx)), C.byref(_m(img)), C.byref(_m(dist)), capi.current_stream_ptr()))
        return idx, img, dist

    def matchDevice(self, queryDescriptors, trainDescriptors=None, mask=None, masks=None):
        """-> (trainIdx (nq,), imgIdx (nq,), distance (nq,))"""
        idx, img, dist = self.knnMatchDevice(queryDescriptors, trainDescriptors, 1, mask, masks)
        return idx[:, 0], img[:, 0], dist[:, 0]

    def radiusMatchDevice(self, queryDescriptors, trainDescriptors=None, maxDistance=0.0, mask=None, masks=None):
        """-> (trainIdx, imgIdx, distance) (nq, cols) and nMatches (nq,); cols as the reference sizes it (max(nTrain / 100, nQuery),
        nQuery for a collection: brute_force_matcher.cpp:897,969).  Row q holds its first min(nMatches[q], cols) hits in ascending
        (image, train) order."""
        import torch
        trains, ms, coll = self._collection(trainDescriptors, mask, masks)
        q = queryDescriptors
        if q.numel() == 0 or not trains:
            e = torch.empty((0, 0), dtype=torch.int32, device=q.device)
            return e, e.clone(), torch.empty((0, 0), dtype=torch.float32, device=q.device), torch.empty((0,), dtype=torch.int32, device=q.device)
        nq = q.shape[0]
        cols = nq if coll else max(trains[0].shape[0] // 100, nq)
        idx = torch.full((nq, cols), -1, dtype=torch.int32, device=q.device)
        img = torch.full((nq, cols), -1, dtype=torch.int32, device=q.device)
        dist = torch.zeros((nq, cols), dtype=torch.float32, device=q.device)
        n = torch.empty((1, nq), dtype=torch.int32, device=q.device)
        capi.check(capi.lib().mi_bf_radius_match(self._h, C.byref(_m(q)), _mats(_nonempty(trains)), _mats(_nonempty(ms)) if ms else None, len(trains),
                                                 float(maxDistance), C.byref(_m(idx)), C.byref(_m(img)), C.byref(_m(dist)), C.byref(_m(n)),
                                                 capi.current_stream_ptr()))
        return idx, img, dist, n[0]

    # ---- the reference's packed device matrices (matchAsync / knnMatchAsync / radiusMatchAsync)
    def matchAsync(self, queryDescriptors, trainDescriptors=None, mask=None, masks=None):
        """CV_32SC1 2 x nq {trainIdx; distance bits} (:367-374), 3 x nq {trainIdx; imgIdx; distance bits} for the collection (:429-437)."""
        import torch
        idx, img, dist = self.matchDevice(queryDescriptors, trainDescriptors, mask, masks)
        rows = [idx, dist.view(torch.int32)] if trainDescriptors is not None else [idx, img, dist.view(torch.int32)]
        return torch.stack(rows, 0)

    @staticmethod
    def matchConvert(gpu_matches):
        """brute_force_matcher.cpp:440-495: unmatched queries (trainIdx -1) are dropped."""
        import numpy as np
        g = gpu_matches.cpu().numpy()
        if g.size == 0:
            return []
        assert g.dtype == np.int32 and g.shape[0] in (2, 3)
        idx, dist = g[0], g[-1].view(np.float32)
        img = g[1] if g.shape[0] == 3 else np.zeros_like(idx)
        return [DMatch(q, idx[q], img[q], dist[q]) for q in range(g.shape[1]) if idx[q] != -1]

    def match(self, queryDescriptors, trainDescriptors=None, mask=None, masks=None):
        return self.matchConvert(self.matchAsync(queryDescriptors, trainDescriptors, mask, masks))

    def knnMatchAsync(self, queryDescriptors, trainDescriptors=None, k=2, mask=None, masks=None):
        """k = 2: CV_32SC2 2 x nq (3 x nq with imgIdx for the collection); other k (single train set only, like the reference:
        :662-665): CV_32SC1 2 nq x k, trainIdx rows then distance rows (:634-642)."""
        import torch
        if trainDescriptors is None and k != 2:
            raise capi.MiError(-1, "only k=2 mode is supported for now (knnMatchAsync over the collection); use knnMatch")
        idx, img, dist = self.knnMatchDevice(queryDescriptors, trainDescriptors, k, mask, masks)
        bits = dist.view(torch.int32)
        if k == 2:
            return torch.stack([idx, bits] if trainDescriptors is not None else [idx, img, bits], 0)
        return torch.cat([idx, bits], 0)

    @staticmethod
    def knnMatchConvert(gpu_matches, compactResult=False):
        """brute_force_matcher.cpp:727-812"""
        import numpy as np
        g = gpu_matches.cpu().numpy()
        if g.size == 0:
            return []
        if g.ndim == 3:
            idx, dist = g[0], g[-1].view(np.float32)
            img = g[1] if g.shape[0] == 3 else np.zeros_like(idx)
        else:
            nq = g.shape[0] // 2
            idx, dist = g[:nq], g[nq:].view(np.float32)
            img = np.zeros_like(idx)
        out = []
        for q in range(idx.shape[0]):
            cur = [DMatch(q, idx[q, j], img[q, j], dist[q, j]) for j in range(idx.shape[1]) if idx[q, j] != -1]
            if cur or not compactResult:
                out.append(cur)
        return out

    def knnMatch(self, queryDescriptors, trainDescriptors=None, k=2, mask=None, masks=None, compactResult=False):
        """The reference merges per-image k-lists on the host for k != 2 over a collection (:512-571); here one device pass."""
        import numpy as np
        if trainDescriptors is not None or k == 2:
            return self.knnMatchConvert(self.knnMatchAsync(queryDescriptors, trainDescriptors, k, mask, masks), compactResult)
        idx, img, dist = (t.cpu().numpy() for t in self.knnMatchDevice(queryDescriptors, None, k, None, masks))
        out = []
        for q in range(idx.shape[0]):
            cur = [DMatch(q, idx[q, j], img[q, j], dist[q, j]) for j in range(k) if idx[q, j] != -1]
            if cur or not compactResult:
                out.append(cur)
        return out

    def radiusMatchAsync(self, queryDescriptors, trainDescriptors=None, maxDistance=0.0, mask=None, masks=None):
        """CV_32SC1 (2 nq + 1) x cols {trainIdx rows; distance rows; nMatches} (:897-905); collection: (3 nq + 1) x nq with imgIdx rows
        (the reference types that one CV_32FC1, :969-975; the bits are the same)."""
        import torch
        idx, img, dist, n = self.radiusMatchDevice(queryDescriptors, trainDescriptors, maxDistance, mask, masks)
        if idx.numel() == 0:
            return idx
        last = torch.zeros((1, idx.shape[1]), dtype=torch.int32, device=idx.device)
        last[0, :n.shape[0]] = n
        parts = [idx, dist.view(torch.int32), last] if trainDescriptors is not None else [idx, img, dist.view(torch.int32), last]
        return torch.cat(parts, 0)

    @staticmethod
    def radiusMatchConvert(gpu_matches, compactResult=False, collection=False):
        """brute_force_matcher.cpp:982-1063: min(nMatches, cols) entries per query, sorted by distance (stable here: ties keep the
        ascending (image, train) order)."""
        import numpy as np
        g = gpu_matches.cpu().numpy()
        if g.size == 0:
            return []
        per = 3 if collection else 2
        nq = (g.shape[0] - 1) // per
        idx, dist, n = g[:nq], g[(per - 1) * nq:per * nq].view(np.float32), g[per * nq]
        img = g[nq:2 * nq] if collection else np.zeros_like(idx)
        out = []
        for q in range(nq):
            m = min(int(n[q]), g.shape[1])
            if m == 0:
                if not compactResult:
                    out.append([])
                continue
            cur = [DMatch(q, idx[q, j], img[q, j], dist[q, j]) for j in range(m)]
            cur.sort(key=lambda d: d.distance)
            out.append(cur)
        return out

    def radiusMatch(self, queryDescriptors, trainDescriptors=None, maxDistance=0.0, mask=None, masks=None, compactResult=False):
        g = self.radiusMatchAsync(queryDescriptors, trainDescriptors, maxDistance, mask, masks)
        return self.radiusMatchConvert(g, compactResult, collection=trainDescriptors is None)


def createBFMatcher(normType=4) -> BFMatcher:
    """cv::cuda::DescriptorMatcher::createBFMatcher (cudafeatures2d.hpp)."""
    return BFMatcher(normType)


class DescriptorMatcher:
    """Name parity with cv2.cuda_DescriptorMatcher: `cuda.DescriptorMatcher.createBFMatcher(cuda.NORM_L2)`."""
    createBFMatcher = staticmethod(createBFMatcher)


NORM_L1, NORM_L2, NORM_HAMMING = 2, 4, 6


class DisparityBilateralFilter(_Handle):
    """cv::cuda::DisparityBilateralFilter (cudastereo.hpp:298-330; cudastereo/src/disparity_bilateral_filter.cpp:58-190):
    joint bilateral refinement of a disparity map at its discontinuities, guided by the image."""

    def __init__(self, ndisp=64, radius=3, iters=1):
        p = capi.DispBilateralParams()
        capi.lib().mi_disp_bilateral_default_params(C.byref(p))
        p.ndisp, p.radius, p.iters = ndisp, radius, iters
        self._open("disp_bilateral", p)

    def getNumDisparities(self): return self._p.ndisp
    def setNumDisparities(self, v): self._set(ndisp=v)
    def getRadius(self): return self._p.radius
    def setRadius(self, v): self._set(radius=v)
    def getNumIters(self): return self._p.iters
    def setNumIters(self, v): self._set(iters=v)
    def getEdgeThreshold(self): return float(self._p.edge_threshold)
    def setEdgeThreshold(self, v): self._set(edge_threshold=float(v))
    def getMaxDiscThreshold(self): return float(self._p.max_disc_threshold)
    def setMaxDiscThreshold(self, v): self._set(max_disc_threshold=float(v))
    def getSigmaRange(self): return float(self._p.sigma_range)
    def setSigmaRange(self, v): self._set(sigma_range=float(v))

    def apply(self, disparity, image, dst=None):
        """disparity: uint8 or int16 (H, W); image: uint8 (H, W) or (H, W, 3); returns dst (same type as disparity)."""
        import torch
        if dst is None:
            dst = torch.empty_like(disparity)
        capi.check(capi.lib().mi_disp_bilateral_apply(self._h, C.byref(_m(disparity)), C.byref(_m(image)), C.byref(_m(dst)),
                                                      capi.current_stream_ptr()))
        return dst


def createDisparityBilateralFilter(ndisp=64, radius=3, iters=1) -> DisparityBilateralFilter:
    """cv::cuda::createDisparityBilateralFilter (cudastereo.hpp:338-339)."""
    return DisparityBilateralFilter(ndisp, radius, iters)


CV_16S, CV_32F = 3, 5   # the depth codes StereoBeliefPropagation's msg_type takes


def _bp_dtype(msg_type):
    import torch
    return torch.float32 if msg_type == CV_32F else torch.int16


class StereoBeliefPropagation(_Handle):
    """cv::cuda::StereoBeliefPropagation (cudastereo.hpp:128-189; cudastereo/src/stereobp.cpp:78-378): hierarchical belief propagation
    on a checkerboard schedule, 16-bit or f32 messages, bit-exact to the reference."""

    def __init__(self, ndisp=64, iters=5, levels=5, msg_type=CV_32F):
        p = capi.StereoBPParams()
        capi.lib().mi_stereobp_default_params(C.byref(p))
        p.ndisp, p.iters, p.levels, p.msg_type = ndisp, iters, levels, msg_type
        self._open("stereobp", p)

    def getMinDisparity(self): return 0
    def setMinDisparity(self, v): pass
    def getNumDisparities(self): return self._p.ndisp
    def setNumDisparities(self, v): self._set(ndisp=v)
    def getBlockSize(self): return 0
    def setBlockSize(self, v): pass
    def getSpeckleWindowSize(self): return 0
    def setSpeckleWindowSize(self, v): pass
    def getSpeckleRange(self): return 0
    def setSpeckleRange(self, v): pass
    def getDisp12MaxDiff(self): return 0
    def setDisp12MaxDiff(self, v): pass
    def getNumIters(self): return self._p.iters
    def setNumIters(self, v): self._set(iters=v)
    def getNumLevels(self): return self._p.levels
    def setNumLevels(self, v): self._set(levels=v)
    def getMaxDataTerm(self): return float(self._p.max_data_term)
    def setMaxDataTerm(self, v): self._set(max_data_term=float(v))
    def getDataWeight(self): return float(self._p.data_weight)
    def setDataWeight(self, v): self._set(data_weight=float(v))
    def getMaxDiscTerm(self): return float(self._p.max_disc_term)
    def setMaxDiscTerm(self, v): self._set(max_disc_term=float(v))
    def getDiscSingleJump(self): return float(self._p.disc_single_jump)
    def setDiscSingleJump(self, v): self._set(disc_single_jump=float(v))
    def getMsgType(self): return self._p.msg_type
    def setMsgType(self, v): self._set(msg_type=v)

    def compute(self, left, right, disparity=None, stream=None):
        """left, right: uint8 (H, W), (H, W, 3) or (H, W, 4); returns the disparity, int16 (H, W) unless `disparity` (uint8, int16,
        int32 or float32) is given (stereobp.cpp:342)."""
        import torch
        if disparity is None:
            disparity = torch.empty(left.shape[:2], dtype=torch.int16, device=left.device)
        s = capi.current_stream_ptr() if stream is None else C.c_void_p(stream.cuda_stream)
        capi.check(capi.lib().mi_stereobp_compute(self._h, C.byref(_m(left)), C.byref(_m(right)), C.byref(_m(disparity)), s))
        return disparity

    def compute_data(self, data, disparity=None, stream=None):
        """compute(data, disparity, stream), stereobp.cpp:206-232: data is the caller's cost volume (ndisp * H, W) of the message type."""
        import torch
        if disparity is None:
            nd = max(int(self._p.ndisp), 1)
            disparity = torch.empty((data.shape[0] // nd, data.shape[1]), dtype=torch.int16, device=data.device)
        s = capi.current_stream_ptr() if stream is None else C.c_void_p(stream.cuda_stream)
        capi.check(capi.lib().mi_stereobp_compute_data(self._h, C.byref(_m(data)), C.byref(_m(disparity)), s))
        return disparity

    def scratchBytes(self):
        """miflow extension: bytes of device scratch the handle holds."""
        n = C.c_size_t()
        capi.check(capi.lib().mi_stereobp_scratch_bytes(self._h, C.byref(n)))
        return n.value

    @staticmethod
    def estimateRecommendedParams(width, height):
        """-> (ndisp, iters, levels), stereobp.cpp:367-378."""
        nd, it, lv = C.c_int(), C.c_int(), C.c_int()
        capi.check(capi.lib().mi_stereobp_estimate_recommended_params(width, height, C.byref(nd), C.byref(it), C.byref(lv)))
        return nd.value, it.value, lv.value


def createStereoBeliefPropagation(ndisp=64, iters=5, levels=5, msg_type=CV_32F) -> StereoBeliefPropagation:
    """cv::cuda::createStereoBeliefPropagation (cudastereo.hpp:189)."""
    return StereoBeliefPropagation(ndisp, iters, levels, msg_type)


def _bp_params(ndisp, msg_type, max_data_term=10.0, data_weight=0.07, max_disc_term=1.7, disc_single_jump=1.0):
    p = capi.StereoBPParams()
    capi.lib().mi_stereobp_default_params(C.byref(p))
    p.ndisp, p.msg_type = ndisp, msg_type
    p.max_data_term, p.data_weight, p.max_disc_term, p.disc_single_jump = max_data_term, data_weight, max_disc_term, disc_single_jump
    return p


def stereobp_comp_data(left, right, ndisp, msg_type=CV_32F, data=None, **weights):
    """comp_data_gpu (stereobp.cu:132-251) -> data (ndisp * H, W); border elements keep what `data` held (zeros if it is made here)."""
    import torch
    if data is None:
        data = torch.zeros((ndisp * left.shape[0], left.shape[1]), dtype=_bp_dtype(msg_type), device=left.device)
    p = _bp_params(ndisp, msg_type, **weights)
    capi.check(capi.lib().mi_stereobp_comp_data(C.byref(p), C.byref(_m(left)), C.byref(_m(right)), C.byref(_m(data)), capi.current_stream_ptr()))
    return data


def stereobp_data_step_down(src, ndisp):
    """data_step_down_gpu (stereobp.cu:257-299)."""
    import torch
    rows = src.shape[0] // ndisp
    dst = torch.empty((ndisp * ((rows + 1) // 2), (src.shape[1] + 1) // 2), dtype=src.dtype, device=src.device)
    capi.check(capi.lib().mi_stereobp_data_step_down(C.byref(_m(src)), C.byref(_m(dst)), ndisp, capi.current_stream_ptr()))
    return dst


def stereobp_level_up(msgs, ndisp, rows, cols):
    """level_up_messages_gpu (stereobp.cu:305-352): msgs = (u, d, l, r) of the coarser level -> the four of the rows x cols level."""
    import torch
    out = [torch.empty((ndisp * rows, cols), dtype=msgs[0].dtype, device=msgs[0].device) for _ in range(4)]
    capi.check(capi.lib().mi_stereobp_level_up(_mats(msgs), _mats(out), ndisp, capi.current_stream_ptr()))
    return out


def stereobp_iterate(msgs, data, ndisp, t0=0, n_iters=1, form=capi.MI_STEREOBP_FORM_AUTO, **weights):
    """calc_all_iterations_gpu (stereobp.cu:358-475) for t = t0 .. t0 + n_iters - 1 on copies of msgs = (u, d, l, r)."""
    import torch
    out = [m.clone() for m in msgs]
    p = _bp_params(ndisp, CV_32F if data.dtype == torch.float32 else CV_16S, **weights)
    capi.check(capi.lib().mi_stereobp_iterate(C.byref(p), _mats(out), C.byref(_m(data)), t0, n_iters, form, capi.current_stream_ptr()))
    return out


def stereobp_output(msgs, data, ndisp, dtype=None):
    """output_gpu (stereobp.cu:481-539) with the zero border and the conversion of calcBP (stereobp.cpp:342-358)."""
    import torch
    disp = torch.empty((data.shape[0] // ndisp, data.shape[1]), dtype=dtype or torch.int16, device=data.device)
    capi.check(capi.lib().mi_stereobp_output(_mats(msgs), C.byref(_m(data)), ndisp, C.byref(_m(disp)), capi.current_stream_ptr()))
    return disp


class StereoConstantSpaceBP(StereoBeliefPropagation):
    """cv::cuda::StereoConstantSpaceBP (cudastereo.hpp; cudastereo/src/stereocsbp.cpp:60-355): belief propagation over nr_plane << level
    candidate disparities per pixel instead of all ndisp, 16-bit or f32 messages, bit-exact to the reference."""

    def __init__(self, ndisp=128, iters=8, levels=4, nr_plane=4, msg_type=CV_32F):
        p = capi.StereoCSBPParams()
        capi.lib().mi_stereocsbp_default_params(C.byref(p))
        p.ndisp, p.iters, p.levels, p.nr_plane, p.msg_type = ndisp, iters, levels, nr_plane, msg_type
        self._open("stereocsbp", p)

    def getMinDisparity(self): return self._p.min_disp_th
    def setMinDisparity(self, v): self._set(min_disp_th=v)
    def getNrPlane(self): return self._p.nr_plane
    def setNrPlane(self, v): self._set(nr_plane=v)
    def getUseLocalInitDataCost(self): return bool(self._p.use_local_init_data_cost)
    def setUseLocalInitDataCost(self, v): self._set(use_local_init_data_cost=int(bool(v)))

    def compute(self, left, right, disparity=None, stream=None):
        """left, right: uint8 (H, W), (H, W, 3) or (H, W, 4); returns the disparity, int16 (H, W) unless `disparity` (uint8, int16,
        int32 or float32) is given (stereocsbp.cpp:303).  getNumLevels() returns the clamped level count afterwards (:171)."""
        import torch
        if disparity is None:
            disparity = torch.empty(left.shape[:2], dtype=torch.int16, device=left.device)
        s = capi.current_stream_ptr() if stream is None else C.c_void_p(stream.cuda_stream)
        capi.check(capi.lib().mi_stereocsbp_compute(self._h, C.byref(_m(left)), C.byref(_m(right)), C.byref(_m(disparity)), s))
        capi.check(capi.lib().mi_stereocsbp_get_params(self._h, C.byref(self._p)))
        return disparity

    def compute_data(self, data, disparity=None, stream=None):
        """compute(data, disparity, stream), stereocsbp.cpp:331-334."""
        raise NotImplementedError("Not implemented")

    def scratchBytes(self):
        """miflow extension: bytes of device scratch the handle holds."""
        n = C.c_size_t()
        capi.check(capi.lib().mi_stereocsbp_scratch_bytes(self._h, C.byref(n)))
        return n.value

    @staticmethod
    def estimateRecommendedParams(width, height):
        """-> (ndisp, iters, levels, nr_plane), stereocsbp.cpp:342-355."""
        nd, it, lv, nr = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        capi.check(capi.lib().mi_stereocsbp_estimate_recommended_params(width, height, C.byref(nd), C.byref(it), C.byref(lv), C.byref(nr)))
        return nd.value, it.value, lv.value, nr.value


def createStereoConstantSpaceBP(ndisp=128, iters=8, levels=4, nr_plane=4, msg_type=CV_32F) -> StereoConstantSpaceBP:
    """cv::cuda::createStereoConstantSpaceBP (cudastereo.hpp)."""
    return StereoConstantSpaceBP(ndisp, iters, levels, nr_plane, msg_type)


def _csbp_params(msg_type, ndisp=128, min_disp=0, local=True, max_data_term=30.0, data_weight=1.0, max_disc_term=160.0, disc_single_jump=10.0):
    p = capi.StereoCSBPParams()
    capi.lib().mi_stereocsbp_default_params(C.byref(p))
    p.ndisp, p.msg_type, p.min_disp_th, p.use_local_init_data_cost = ndisp, msg_type, min_disp, int(bool(local))
    p.max_data_term, p.data_weight, p.max_disc_term, p.disc_single_jump = max_data_term, data_weight, max_disc_term, disc_single_jump
    return p


def _csbp_msg_type(t):
    import torch
    return CV_32F if t.dtype == torch.float32 else CV_16S


def stereocsbp_init_data_cost(left, right, level, nr_plane, ndisp, msg_type=CV_32F, local=True, **kw):
    """init_data_cost (stereocsbp.cu:86-350) at `level` -> (data_cost_selected, disp_selected), nr_plane planes of the level each."""
    import torch
    h, w = left.shape[0] >> level, left.shape[1] >> level
    mk = lambda n: torch.zeros((n * h, w), dtype=_bp_dtype(msg_type), device=left.device)
    temp, sel_cost, sel_disp = mk(ndisp), mk(nr_plane), mk(nr_plane)
    p = _csbp_params(msg_type, ndisp=ndisp, local=local, **kw)
    capi.check(capi.lib().mi_stereocsbp_init_data_cost(C.byref(p), C.byref(_m(left)), C.byref(_m(right)), level, nr_plane, C.byref(_m(temp)),
                                                       C.byref(_m(sel_cost)), C.byref(_m(sel_disp)), capi.current_stream_ptr()))
    return sel_cost, sel_disp


def stereocsbp_compute_data_cost(left, right, level, disp_selected_parent, nr_plane2, **kw):
    """compute_data_cost (stereocsbp.cu:356-517): the costs of the parents' nr_plane2 candidates at the pixels of `level`."""
    import torch
    h, w = left.shape[0] >> level, left.shape[1] >> level
    data_cost = torch.zeros((nr_plane2 * h, w), dtype=disp_selected_parent.dtype, device=left.device)
    p = _csbp_params(_csbp_msg_type(disp_selected_parent), **kw)
    capi.check(capi.lib().mi_stereocsbp_compute_data_cost(C.byref(p), C.byref(_m(left)), C.byref(_m(right)), level, nr_plane2,
                                                          C.byref(_m(disp_selected_parent)), C.byref(_m(data_cost)), capi.current_stream_ptr()))
    return data_cost


def stereocsbp_init_message(cur, data_cost, nr_plane, nr_plane2):
    """init_message (stereocsbp.cu:525-650): cur = (u, d, l, r, disp_selected) of the coarser level -> (the five of the level,
    data_cost_selected)."""
    import torch
    h, w = data_cost.shape[0] // nr_plane2, data_cost.shape[1]
    mk = lambda n: torch.zeros((n * h, w), dtype=data_cost.dtype, device=data_cost.device)
    new = [mk(nr_plane) for _ in range(5)]
    sel_cost, temp = mk(nr_plane), mk(nr_plane2)
    capi.check(capi.lib().mi_stereocsbp_init_message(_mats(cur), _mats(new), C.byref(_m(data_cost)), C.byref(_m(sel_cost)), C.byref(_m(temp)),
                                                     nr_plane, nr_plane2, capi.current_stream_ptr()))
    return new, sel_cost


def stereocsbp_iterate(msgs, disp_selected, data_cost_selected, nr_plane, t0=0, n_iters=1, form=capi.MI_STEREOCSBP_FORM_AUTO, **kw):
    """calc_all_iterations (stereocsbp.cu:656-744) for t = t0 .. t0 + n_iters - 1 on copies of msgs = (u, d, l, r)."""
    import torch
    out = [m.clone() for m in msgs]
    temp = torch.zeros_like(data_cost_selected)
    p = _csbp_params(_csbp_msg_type(data_cost_selected), **kw)
    capi.check(capi.lib().mi_stereocsbp_iterate(C.byref(p), _mats(out), C.byref(_m(disp_selected)), C.byref(_m(data_cost_selected)),
                                                C.byref(_m(temp)), nr_plane, t0, n_iters, form, capi.current_stream_ptr()))
    return out


def stereocsbp_compute_disp(msgs, disp_selected, data_cost_selected, nr_plane, dtype=None):
    """compute_disp (stereocsbp.cu:752-810) with the zero border and the conversion of stereocsbp.cpp:303-328."""
    import torch
    disp = torch.empty((data_cost_selected.shape[0] // nr_plane, data_cost_selected.shape[1]), dtype=dtype or torch.int16,
                       device=data_cost_selected.device)
    capi.check(capi.lib().mi_stereocsbp_compute_disp(_mats(msgs), C.byref(_m(disp_selected)), C.byref(_m(data_cost_selected)), nr_plane,
                                                     C.byref(_m(disp)), capi.current_stream_ptr()))
    return disp


def stereobm_prefilter_xsobel(img, cap=31):
    import torch
    out = torch.empty_like(img)
    capi.check(capi.lib().mi_stereobm_prefilter_xsobel(C.byref(_m(img)), C.byref(_m(out)), cap, capi.current_stream_ptr()))
    return out


def stereobm_prefilter_norm(img, cap=31, winsize=9):
    import torch
    out = torch.empty_like(img)
    capi.check(capi.lib().mi_stereobm_prefilter_norm(C.byref(_m(img)), C.byref(_m(out)), cap, winsize, capi.current_stream_ptr()))
    return out


def stereobm_block_match(left, right, ndisp=64, winsz=19, uniqueness_ratio=0, emulate_cuda_edge=True):
    """-> (disp CV_8UC1, minSSD CV_32SC1 holding uint32 bit patterns)."""
    import torch
    disp = torch.empty_like(left)
    ssd = torch.empty(left.shape, dtype=torch.int32, device=left.device)
    capi.check(capi.lib().mi_stereobm_block_match(C.byref(_m(left)), C.byref(_m(right)), C.byref(_m(disp)), C.byref(_m(ssd)),
                                                  ndisp, winsz, uniqueness_ratio, int(bool(emulate_cuda_edge)),
                                                  capi.current_stream_ptr()))
    return disp, ssd


def stereobm_textureness(img, disp, winsz=19, avg_threshold=3.0):
    out = disp.clone()
    capi.check(capi.lib().mi_stereobm_textureness(C.byref(_m(img)), C.byref(_m(out)), winsz, avg_threshold,
                                                  capi.current_stream_ptr()))
    return out


# =============================================================================================
OPTFLOW_USE_INITIAL_FLOW, OPTFLOW_FARNEBACK_GAUSSIAN = 4, 256   # cv::OPTFLOW_* (main repo video/tracking.hpp)


class FarnebackOpticalFlow(_Handle):
    """cv::cuda::FarnebackOpticalFlow (cudaoptflow.hpp:258-294; impl cudaoptflow/src/farneback.cpp:96-165)."""

    def __init__(self, params: capi.FarnebackParams):
        self._open("farneback", params)

    @staticmethod
    def create(numLevels=5, pyrScale=0.5, fastPyramids=False, winSize=13, numIters=10, polyN=5, polySigma=1.1,
               flags=0) -> "FarnebackOpticalFlow":
        p = capi.FarnebackParams()
        capi.lib().mi_farneback_default_params(C.byref(p))
        p.num_levels, p.pyr_scale, p.fast_pyramids, p.win_size = numLevels, pyrScale, int(bool(fastPyramids)), winSize
        p.num_iters, p.poly_n, p.poly_sigma, p.flags = numIters, polyN, polySigma, flags
        return FarnebackOpticalFlow(p)

    def getDefaultName(self) -> str:  # farneback.cpp:132
        return "DenseOpticalFlow.FarnebackOpticalFlow"

    # getters / setters, farneback.cpp:106-128
    def getNumLevels(self): return self._p.num_levels
    def setNumLevels(self, v): self._set(num_levels=v)
    def getPyrScale(self): return self._p.pyr_scale
    def setPyrScale(self, v): self._set(pyr_scale=v)
    def getFastPyramids(self): return bool(self._p.fast_pyramids)
    def setFastPyramids(self, v): self._set(fast_pyramids=int(bool(v)))
    def getWinSize(self): return self._p.win_size
    def setWinSize(self, v): self._set(win_size=v)
    def getNumIters(self): return self._p.num_iters
    def setNumIters(self, v): self._set(num_iters=v)
    def getPolyN(self): return self._p.poly_n
    def setPolyN(self, v): self._set(poly_n=v)
    def getPolySigma(self): return self._p.poly_sigma
    def setPolySigma(self, v): self._set(poly_sigma=v)
    def getFlags(self): return self._p.flags
    def setFlags(self, v): self._set(flags=v)

    def calc(self, I0, I1, flow=None, stream=None):
        """DenseOpticalFlow::calc(I0, I1, flow, stream) (cudaoptflow.hpp:80).  Returns flow (H,W,2) f32."""
        import torch
        if flow is None:
            if self._p.flags & OPTFLOW_USE_INITIAL_FLOW:
                raise MiError(-1, "OPTFLOW_USE_INITIAL_FLOW requires a flow argument")
            flow = torch.empty((I0.shape[0], I0.shape[1], 2), dtype=torch.float32, device=I0.device)
        m0, m1, mf = capi.mat_from_tensor(I0), capi.mat_from_tensor(I1), capi.mat_from_tensor(flow)
        sp = _stream_ptr(stream)
        capi.check(capi.lib().mi_farneback_calc(self._h, C.byref(m0), C.byref(m1), C.byref(mf), sp))
        return flow

    def calc_batch(self, I0s, I1s, flows=None, stream=None):
        """n independent pairs of one size and type in one pass (miflow extension; blockIdx.z = pair in every kernel)."""
        import torch
        n = len(I0s)
        if flows is None:
            if self._p.flags & OPTFLOW_USE_INITIAL_FLOW:
                raise MiError(-1, "OPTFLOW_USE_INITIAL_FLOW requires the flows argument")
            flows = torch.empty((n, I0s[0].shape[0], I0s[0].shape[1], 2), dtype=torch.float32, device=I0s[0].device)
        A0 = _mats(I0s)
        A1 = _mats(I1s)
        AF = _mats(flows)
        sp = _stream_ptr(stream)
        capi.check(capi.lib().mi_farneback_calc_batch(self._h, n, A0, A1, AF, sp))
        return flows


def farneback_polyExp(src, polyN=5, polySigma=1.1):
    import torch
    dst = torch.empty((5 * src.shape[0], src.shape[1]), dtype=torch.float32, device=src.device)
    capi.check(capi.lib().mi_farneback_poly_exp(C.byref(_m(src)), C.byref(_m(dst)), polyN, polySigma, capi.current_stream_ptr()))
    return dst


def farneback_updateMatrices(flowx, flowy, R0, R1):
    import torch
    M = torch.empty_like(R0)
    capi.check(capi.lib().mi_farneback_update_matrices(C.byref(_m(flowx)), C.byref(_m(flowy)), C.byref(_m(R0)), C.byref(_m(R1)),
                                                       C.byref(_m(M)), capi.current_stream_ptr()))
    return M


def farneback_blur5(M, ksize, gaussian=False):
    import torch
    out = torch.empty_like(M)
    capi.check(capi.lib().mi_farneback_blur5(C.byref(_m(M)), C.byref(_m(out)), ksize, int(bool(gaussian)), capi.current_stream_ptr()))
    return out


def farneback_updateFlow(M):
    import torch
    h = M.shape[0] // 5
    fx = torch.empty((h, M.shape[1]), dtype=torch.float32, device=M.device)
    fy = torch.empty_like(fx)
    capi.check(capi.lib().mi_farneback_update_flow(C.byref(_m(M)), C.byref(_m(fx)), C.byref(_m(fy)), capi.current_stream_ptr()))
    return fx, fy


def farneback_iterate(M, R0, R1, ksize, gaussian=False, update=True):
    """One fused inner iteration -> (flowx, flowy, M')."""
    import torch
    h = M.shape[0] // 5
    fx = torch.empty((h, M.shape[1]), dtype=torch.float32, device=M.device)
    fy = torch.empty_like(fx)
    Mo = torch.empty_like(M)
    capi.check(capi.lib().mi_farneback_iterate(C.byref(_m(M)), C.byref(_m(R0)), C.byref(_m(R1)), C.byref(_m(fx)), C.byref(_m(fy)),
                                               C.byref(_m(Mo)), ksize, int(bool(gaussian)), int(bool(update)),
                                               capi.current_stream_ptr()))
    return fx, fy, Mo


# ---- one named launch form per call (miflow_selftest_farneback_*, csrc/mi_selftest.h): the level loop picks a form from the grid size
# and the process-wide tuning; these let one test process run every form on the same planes.  A form that has no kernel for the
# request raises MiError and launches nothing.
FB_ITERATE_FORMS = {"row": 1, "tile256": 2, "tile64": 3, "pair": 4}
FB_POLY_FORMS = {"row": 1, "tiled": 2, "resized": 3}
FB_UPDATE_FORMS = {"plain": 1, "zero": 2, "resized": 3}
FB_BLUR_FORMS = {"generic_fast": 1, "generic_full": 2, "tiled": 3, "table": 4}


def _ref(t):
    return C.byref(_m(t)) if t is not None else None


def farneback_iterate_form(form, M, R0, R1, ksize, gaussian=False, update=True, Mout=None, merged=None):
    """One launch of the named iteration form -> (flowx, flowy, Mout).  'pair' runs two iterations (k_iterate2_t).  Mout: a 5h x w
    tensor whose contents update=False must keep (default: zeros); merged: a (h, w, 2) view, rows possibly pitched, written in place."""
    import torch
    h = M.shape[0] // 5
    fx = torch.empty((h, M.shape[1]), dtype=torch.float32, device=M.device)
    fy = torch.empty_like(fx)
    Mo = torch.zeros_like(M) if Mout is None else Mout
    capi.check(capi.lib().miflow_selftest_farneback_iterate(FB_ITERATE_FORMS[form], _ref(M), _ref(R0), _ref(R1), _ref(fx), _ref(fy), _ref(Mo),
                                                            _ref(merged), ksize, int(bool(gaussian)), int(bool(update)), capi.current_stream_ptr()))
    return fx, fy, Mo


def farneback_polyExp_form(form, src, polyN=5, polySigma=1.1, dsize=None):
    """form 'resized': src is the plane the level image is resized FROM and dsize = (h, w) of the level."""
    import torch
    h, w = dsize if form == "resized" else src.shape
    dst = torch.empty((5 * h, w), dtype=torch.float32, device=src.device)
    capi.check(capi.lib().miflow_selftest_farneback_poly_exp(FB_POLY_FORMS[form], _ref(src), _ref(dst), polyN, polySigma, capi.current_stream_ptr()))
    return dst


def farneback_updateMatrices_form(form, R0, R1, flowx=None, flowy=None, prevx=None, prevy=None, alpha=1.0):
    """'plain': M(flowx, flowy); 'zero': M of the zero flow, no flow planes; 'resized': flow = resize(prev) * alpha and M(flow) in one
    launch.  -> (M, flowx, flowy)."""
    import torch
    M = torch.empty_like(R0)
    if form == "resized":
        flowx = torch.empty((R0.shape[0] // 5, R0.shape[1]), dtype=torch.float32, device=R0.device)
        flowy = torch.empty_like(flowx)
    capi.check(capi.lib().miflow_selftest_farneback_update_matrices(FB_UPDATE_FORMS[form], _ref(prevx), _ref(prevy), float(alpha), _ref(flowx), _ref(flowy),
                                                                    _ref(R0), _ref(R1), _ref(M), capi.current_stream_ptr()))
    return M, flowx, flowy


def farneback_gaussianBlur_form(form, src, ksize, sigma, border=4, src1=None):
    """'table': src and src1 are pitched uint8 or float32 views, read in place -> (dst0, dst1); the other forms -> dst."""
    import torch
    dst = torch.empty(tuple(src.shape), dtype=torch.float32, device=src.device)
    dst1 = torch.empty_like(dst) if form == "table" else None
    capi.check(capi.lib().miflow_selftest_farneback_gaussian_blur(FB_BLUR_FORMS[form], _ref(src), _ref(src1), _ref(dst), _ref(dst1), ksize, float(sigma),
                                                                  border, capi.current_stream_ptr()))
    return (dst, dst1) if form == "table" else dst


def farneback_gaussianBlur(src, ksize, sigma, border=4):
    import torch
    dst = torch.empty_like(src)
    capi.check(capi.lib().mi_farneback_gaussian_blur(C.byref(_m(src)), C.byref(_m(dst)), ksize, float(sigma), border,
                                                     capi.current_stream_ptr()))
    return dst


def pyrDown(src):
    """cv::cuda::pyrDown on CV_32FC1 (cudawarping/src/pyramids.cpp:66-94)."""
    import torch
    dst = torch.empty(((src.shape[0] + 1) // 2, (src.shape[1] + 1) // 2), dtype=torch.float32, device=src.device)
    capi.check(capi.lib().mi_pyr_down(C.byref(_m(src)), C.byref(_m(dst)), capi.current_stream_ptr()))
    return dst


# =============================================================================================
class SURF_CUDA(_Handle):
    """cv::cuda::SURF_CUDA (xfeatures2d/cuda.hpp:86-196).  Keypoints live in a 7 x N CV_32FC1 device matrix
    (rows X, Y, LAPLACIAN, OCTAVE, SIZE, ANGLE, HESSIAN; LAPLACIAN/OCTAVE hold int bit patterns)."""

    X_ROW, Y_ROW, LAPLACIAN_ROW, OCTAVE_ROW, SIZE_ROW, ANGLE_ROW, HESSIAN_ROW, ROWS_COUNT = range(8)

    def __init__(self, _hessianThreshold=100.0, _nOctaves=4, _nOctaveLayers=2, _extended=True, _keypointsRatio=0.01,
                 _upright=False):
        # defaults of the default constructor (surf.cuda.cpp:257-265): extended = true
        p = capi.SURFParams()
        p.hessian_threshold, p.n_octaves, p.n_octave_layers = _hessianThreshold, _nOctaves, _nOctaveLayers
        p.extended, p.keypoints_ratio, p.upright = int(bool(_extended)), _keypointsRatio, int(bool(_upright))
        self._open("surf", p)

    @staticmethod
    def create(_hessianThreshold, _nOctaves=4, _nOctaveLayers=2, _extended=False, _keypointsRatio=0.01, _upright=False):
        """cuda.hpp:117-118 (extended defaults to false here)."""
        return SURF_CUDA(_hessianThreshold, _nOctaves, _nOctaveLayers, _extended, _keypointsRatio, _upright)

    # public fields of the reference class
    hessianThreshold = property(lambda s: s._p.hessian_threshold, lambda s, v: s._set(hessian_threshold=v))
    nOctaves = property(lambda s: s._p.n_octaves, lambda s, v: s._set(n_octaves=v))
    nOctaveLayers = property(lambda s: s._p.n_octave_layers, lambda s, v: s._set(n_octave_layers=v))
    extended = property(lambda s: bool(s._p.extended), lambda s, v: s._set(extended=int(bool(v))))
    upright = property(lambda s: bool(s._p.upright), lambda s, v: s._set(upright=int(bool(v))))
    keypointsRatio = property(lambda s: s._p.keypoints_ratio, lambda s, v: s._set(keypoints_ratio=v))

    def descriptorSize(self): return 128 if self._p.extended else 64   # surf.cuda.cpp:277-280
    def defaultNorm(self): return 4                                    # NORM_L2, surf.cuda.cpp:282-285
    def releaseMemory(self): capi.lib().mi_surf_release_memory(self._h)

    def detect(self, img, mask=None, stream=None):
        """operator()(img, mask, keypoints) -> keypoints (7, nFeatures) float32 device tensor."""
        import torch
        mf = C.c_int()
        capi.check(capi.lib().mi_surf_max_features(self._h, img.shape[0], img.shape[1], C.byref(mf)))
        kp = torch.empty((7, mf.value), dtype=torch.float32, device=img.device)   # ensureSizeIsEnough(ROWS_COUNT, maxFeatures)
        n = C.c_int()
        sp = _stream_ptr(stream)
        mm = C.byref(capi.mat_from_tensor(mask)) if mask is not None else None
        mk = capi.mat_from_tensor(kp)
        capi.check(capi.lib().mi_surf_detect(self._h, C.byref(capi.mat_from_tensor(img)), mm, C.byref(mk), C.byref(n), sp))
        return kp[:, : n.value]   # keypoints.cols = featureCounter (surf.cuda.cpp:209)

    def detect_batch(self, imgs, masks=None, stream=None):
        """detect() of every frame of `imgs` through this handle in one call (mi_surf_detect_batch); frames may differ in size.
        masks: None, or one entry per frame (a tensor or None).  -> list of (7, nFeatures) keypoint tensors, one per frame."""
        import torch
        n = len(imgs)
        if masks is not None and len(masks) != n:
            raise capi.MiError(-3, "masks: one entry (a tensor or None) per frame")
        kps = []
        for im in imgs:
            # a frame the limits reject gets no matrix here: the batch call runs the frames before it and returns that frame's error
            mf = C.c_int()
            ok = capi.lib().mi_surf_max_features(self._h, im.shape[0], im.shape[1], C.byref(mf)) == 0
            kps.append(torch.empty((7, mf.value), dtype=torch.float32, device=im.device) if ok else None)
        mi = _mats(imgs)
        mk = _mats(kps)
        mm = None
        if masks is not None:   # a frame without a mask: an mi_mat with a NULL data pointer
            mm = _mats(masks)
        nf = (C.c_int * n)()
        sp = _stream_ptr(stream)
        capi.check(capi.lib().mi_surf_detect_batch(self._h, n, mi, mm, mk, nf, sp))
        return [kp[:, : nf[i]] for i, kp in enumerate(kps)]

    def detectWithDescriptors(self, img, mask=None, keypoints=None, useProvidedKeypoints=False, stream=None):
        """operator()(img, mask, keypoints, descriptors, useProvidedKeypoints) (surf.cuda.cpp:380-397)."""
        import torch
        sp = _stream_ptr(stream)
        if not useProvidedKeypoints:
            # one enqueue for the frame: the descriptor kernels read the feature count on the device (mi_surf_detect_and_compute)
            mf = C.c_int()
            capi.check(capi.lib().mi_surf_max_features(self._h, img.shape[0], img.shape[1], C.byref(mf)))
            kp = torch.empty((7, mf.value), dtype=torch.float32, device=img.device)
            desc = torch.empty((mf.value, self.descriptorSize()), dtype=torch.float32, device=img.device)
            n = C.c_int()
            mm = C.byref(capi.mat_from_tensor(mask)) if mask is not None else None
            mk, md = capi.mat_from_tensor(kp), capi.mat_from_tensor(desc)
            capi.check(capi.lib().mi_surf_detect_and_compute(self._h, C.byref(capi.mat_from_tensor(img)), mm, C.byref(mk), C.byref(md), C.byref(n), sp))
            return kp[:, : n.value], desc[: n.value]
        elif not self._p.upright:
            capi.check(capi.lib().mi_surf_compute_orientation(self._h, C.byref(capi.mat_from_tensor(img)),
                                                              C.byref(capi.mat_from_tensor(keypoints)), keypoints.shape[1], sp))
        n = keypoints.shape[1]
        desc = torch.empty((n, self.descriptorSize()), dtype=torch.float32, device=img.device)
        if n:
            capi.check(capi.lib().mi_surf_compute_descriptors(self._h, C.byref(capi.mat_from_tensor(img)),
                                                              C.byref(capi.mat_from_tensor(keypoints)), n,
                                                              C.byref(capi.mat_from_tensor(desc)), sp))
        return keypoints, desc

    # ---- the CPU class's orientation / descriptor arithmetic (xfeatures2d::SURF_Impl, surf.cpp:568-866) on the same keypoint matrix
    def cpuClassOrientation(self, img, keypoints, stream=None):
        """Writes the ANGLE row of `keypoints` (7, n) in place as SURFInvoker does (270 when upright) and sets SIZE to -1 for the
        keypoints the CPU class erases."""
        sp = _stream_ptr(stream)
        if keypoints.shape[1] == 0:
            return keypoints
        s = surf_integral(img)
        capi.check(capi.lib().mi_surfcpu_orientation(C.byref(capi.mat_from_tensor(s)), C.byref(capi.mat_from_tensor(keypoints)),
                                                     keypoints.shape[1], int(self._p.upright), sp))
        return keypoints

    def cpuClassDescriptors(self, img, keypoints, stream=None):
        import torch
        sp = _stream_ptr(stream)
        n = keypoints.shape[1]
        desc = torch.empty((n, self.descriptorSize()), dtype=torch.float32, device=img.device)
        if n:
            capi.check(capi.lib().mi_surfcpu_descriptors(C.byref(capi.mat_from_tensor(img)), C.byref(capi.mat_from_tensor(keypoints)), n,
                                                         int(self._p.extended), int(self._p.upright), C.byref(capi.mat_from_tensor(desc)), sp))
        return desc

    def detectAndComputeCpuClass(self, img, mask=None, keypoints=None, useProvidedKeypoints=False):
        """cv::xfeatures2d::SURF::detectAndCompute (surf.cpp:881-1015) on the GPU: this class's detector (the same fast-Hessian
        responses: tests/test_zz_surf_cpu_class.py), then the CPU class's orientation and descriptor; keypoints it erases are
        removed.  -> (keypoints (7, n), descriptors (n, 64 | 128))."""
        if not useProvidedKeypoints:
            keypoints = self.detect(img, mask)
        keypoints = keypoints.contiguous().clone()
        self.cpuClassOrientation(img, keypoints)
        desc = self.cpuClassDescriptors(img, keypoints)
        keep = keypoints[4] > 0
        return keypoints[:, keep], desc[keep]

    @staticmethod
    def downloadKeypoints(keypointsGPU):
        """-> dict of host arrays (the fields of cv::KeyPoint the reference fills, surf.cuda.cpp:319-356)."""
        import numpy as np
        k = keypointsGPU.detach().cpu().numpy()
        ki = k.view(np.int32)
        return {"x": k[0].copy(), "y": k[1].copy(), "laplacian": ki[2].copy(), "octave": ki[3].copy(), "size": k[4].copy(),
                "angle": k[5].copy(), "hessian": k[6].copy()}


def surf_integral(img, clamp_to_one=False):
    import torch
    alg = SURF_CUDA(100)
    s = torch.empty((img.shape[0] + 1, img.shape[1] + 1), dtype=torch.int32, device=img.device)
    capi.check(capi.lib().mi_surf_integral(alg._h, C.byref(_m(img)), int(bool(clamp_to_one)), C.byref(_m(s)), capi.current_stream_ptr()))
    return s


def surf_detTrace(sum_, octave, nOctaveLayers=2):
    import torch
    alg = SURF_CUDA(100)
    rows, cols = sum_.shape[0] - 1, sum_.shape[1] - 1
    det = torch.empty(((nOctaveLayers + 2) * (rows >> octave), cols), dtype=torch.float32, device=sum_.device)
    tr = torch.empty_like(det)
    capi.check(capi.lib().mi_surf_det_trace(alg._h, C.byref(_m(sum_)), octave, nOctaveLayers, C.byref(_m(det)), C.byref(_m(tr)),
                                            capi.current_stream_ptr()))
    torch.cuda.synchronize()
    return det, tr


# ---------------------------------------------------------------- FastFeatureDetector (cudafeatures2d.hpp:426-442, src/fast.cpp)
def _u8(t):
    """a uint8 device tensor as the kernels take it: rows of any pitch, dense within a row (anything else is copied)"""
    return t if t.dim() != 2 or t.stride(1) == 1 or t.shape[1] <= 1 else t.contiguous()


class FastFeatureDetector(_Handle):
    """cv::cuda::FastFeatureDetector.  Images and masks are uint8 device tensors; keypoints are the reference's 2 x n CV_32FC1 matrix
    (row 0: short2 {x, y} in an element's 4 bytes, row 1: the response), here in row-major order of the image."""
    LOCATION_ROW, RESPONSE_ROW, ROWS_COUNT, FEATURE_SIZE = 0, 1, 2, 7   # cudafeatures2d.hpp:429-432
    TYPE_5_8, TYPE_7_12, TYPE_9_16 = 0, 1, 2                            # cv::FastFeatureDetector (main repository, features2d.hpp)

    def __init__(self, threshold=10, nonmaxSuppression=True, type=2, max_npoints=5000):
        if type != self.TYPE_9_16:
            raise MiError(-1, "type == cv::FastFeatureDetector::TYPE_9_16")   # fast.cpp:213
        self._open("fast", capi.FastParams(int(threshold), int(bool(nonmaxSuppression)), int(max_npoints)))

    @staticmethod
    def create(threshold=10, nonmaxSuppression=True, type=2, max_npoints=5000) -> "FastFeatureDetector":
        return FastFeatureDetector(threshold, nonmaxSuppression, type, max_npoints)

    def setThreshold(self, threshold): self._set(threshold=int(threshold))
    def getThreshold(self): return self._p.threshold
    def setNonmaxSuppression(self, f): self._set(nonmax_suppression=int(bool(f)))
    def getNonmaxSuppression(self): return bool(self._p.nonmax_suppression)
    def setMaxNumPoints(self, max_npoints): self._set(max_npoints=int(max_npoints))
    def getMaxNumPoints(self): return self._p.max_npoints

    def setType(self, type):
        if type != self.TYPE_9_16:
            raise MiError(-1, "type == cv::FastFeatureDetector::TYPE_9_16")   # fast.cpp:85

    def getType(self): return self.TYPE_9_16

    def scratchBytes(self):
        b = C.c_size_t()
        capi.check(capi.lib().mi_fast_scratch_bytes(self._h, C.byref(b)))
        return b.value

    def detectAsync(self, image, mask=None, stream=None):
        """-> the (2, n) float32 keypoint matrix on the device; (2, 0) where the reference releases it (fast.cpp:146-150,158-161)"""
        import torch
        image = _u8(image)
        kp = torch.empty((self.ROWS_COUNT, self._p.max_npoints), dtype=torch.float32, device=image.device)
        n = C.c_int()
        sp = _stream_ptr(stream)
        mm = C.byref(capi.mat_from_tensor(_u8(mask))) if mask is not None else None
        capi.check(capi.lib().mi_fast_detect(self._h, C.byref(capi.mat_from_tensor(image)), mm, C.byref(capi.mat_from_tensor(kp)), C.byref(n), sp))
        return kp[:, : n.value]

    def detect(self, image, mask=None):
        """-> the keypoints as convert() gives them"""
        return self.convert(self.detectAsync(image, mask))

    def detect_batch(self, images, masks=None, stream=None):
        """detectAsync of every frame through this handle in one call, with one read-back for all counts; frames may differ in size.
        masks: None, or one entry per frame (a tensor or None).  -> list of (2, n) keypoint matrices."""
        import torch
        n = len(images)
        if masks is not None and len(masks) != n:
            raise MiError(-3, "masks: one entry (a tensor or None) per frame")
        images = [_u8(t) for t in images]
        kps = [torch.empty((self.ROWS_COUNT, self._p.max_npoints), dtype=torch.float32, device=t.device) for t in images]
        mi = _mats(images)
        mk = _mats(kps)
        mm = None
        if masks is not None:
            keep = [_u8(m) if m is not None else None for m in masks]
            mm = _mats(keep)
        ns = (C.c_int * n)()
        sp = _stream_ptr(stream)
        capi.check(capi.lib().mi_fast_detect_batch(self._h, n, mi, mm, mk, ns, sp))
        return [kp[:, : ns[i]] for i, kp in enumerate(kps)]

    @staticmethod
    def convert(gpu_keypoints):
        """FAST_Impl::convert (fast.cpp:175-208): a device or host matrix -> [(x, y, size, angle, response)]"""
        import numpy as np
        k = gpu_keypoints.detach().cpu().numpy() if hasattr(gpu_keypoints, "detach") else np.asarray(gpu_keypoints)
        if k.size == 0:
            return []
        if k.shape[0] != FastFeatureDetector.ROWS_COUNT or k.itemsize != 4:
            raise MiError(-1, "h_keypoints.rows == ROWS_COUNT && h_keypoints.elemSize() == 4")
        k = np.ascontiguousarray(k)
        loc = k[0].view(np.int16).reshape(-1, 2)
        resp = k[1].view(np.float32)
        return [(float(x), float(y), float(FastFeatureDetector.FEATURE_SIZE), -1.0, float(r)) for (x, y), r in zip(loc, resp)]


def fast_score(image, mask=None, threshold=10):
    """The reference's CV_32SC1 score plane (score.setTo(0) + calcKeypoints<true>, fast.cpp:139-143): cornerScore at candidates, 0 elsewhere"""
    import torch
    image = _u8(image)
    scores = torch.empty(image.shape, dtype=torch.int32, device=image.device)
    if scores.numel() == 0:
        return scores
    mm = C.byref(capi.mat_from_tensor(_u8(mask))) if mask is not None else None
    capi.check(capi.lib().mi_fast_score(C.byref(capi.mat_from_tensor(image)), mm, int(threshold), C.byref(capi.mat_from_tensor(scores)),
                                        capi.current_stream_ptr()))
    return scores


def fast_locations_to_points(gpu_keypoints):
    """(2, n) keypoint matrix -> (1, n, 2) float32 points on the device, the form SparsePyrLKOpticalFlow.calc takes"""
    import torch
    n = gpu_keypoints.shape[1]
    pts = torch.empty((1, n, 2), dtype=torch.float32, device=gpu_keypoints.device)
    if n:
        capi.check(capi.lib().mi_fast_locations_to_points(C.byref(capi.mat_from_tensor(gpu_keypoints)), n, C.byref(capi.mat_from_tensor(pts)),
                                                          capi.current_stream_ptr()))
    return pts


BORDER_REPLICATE, BORDER_REFLECT, BORDER_REFLECT101 = 1, 2, 4   # cv::BorderTypes (main repository)


def _src_type(t):
    import torch
    types = {torch.uint8: capi.MI_8UC1, torch.float32: capi.MI_32FC1}
    if t.dim() != 2 or t.dtype not in types:
        raise MiError(-2, "a 2-D uint8 or float32 image")
    return types[t.dtype]


class CornernessCriteria(_Handle):
    """cv::cuda::CornernessCriteria (cudaimgproc.hpp:538-549): compute(src) -> the float32 response plane on the device.  Made by
    createHarrisCorner / createMinEigenValCorner; srcType is capi.MI_8UC1 or capi.MI_32FC1 (the OpenCV codes)."""

    def __init__(self, srcType, blockSize, ksize, borderType, harris, k=0.0):
        self._open("corner", capi.CornerParams(int(srcType), int(blockSize), int(ksize), int(borderType), int(bool(harris)), float(k)))   # no setter

    def compute(self, src, dst=None, stream=None):
        import torch
        src = _u8(src)
        if _src_type(src) != self._p.type:
            raise MiError(-2, "src.type() == srcType")   # corners.cpp:117
        if dst is None:
            dst = torch.empty(src.shape, dtype=torch.float32, device=src.device)
        sp = _stream_ptr(stream)
        capi.check(capi.lib().mi_corner_compute(self._h, C.byref(capi.mat_from_tensor(src)), C.byref(capi.mat_from_tensor(dst)), sp))
        return dst


def createHarrisCorner(srcType, blockSize, ksize, k, borderType=BORDER_REFLECT101) -> CornernessCriteria:
    """cv::cuda::createHarrisCorner, cudaimgproc.hpp:562"""
    return CornernessCriteria(srcType, blockSize, ksize, borderType, True, k)


def createMinEigenValCorner(srcType, blockSize, ksize, borderType=BORDER_REFLECT101) -> CornernessCriteria:
    """cv::cuda::createMinEigenValCorner, cudaimgproc.hpp:575"""
    return CornernessCriteria(srcType, blockSize, ksize, borderType, False)


class CornersDetector(_Handle):
    """cv::cuda::CornersDetector (cudaimgproc.hpp:581-597), made by createGoodFeaturesToTrackDetector.  detect(image[, mask]) -> the
    corners as a (1, N, 2) float32 device tensor {x, y}, strongest first, which SparsePyrLKOpticalFlow.calc takes as prevPts unchanged;
    (1, 0, 2) where the reference releases the output."""

    def __init__(self, srcType, maxCorners=1000, qualityLevel=0.01, minDistance=0.0, blockSize=3, useHarrisDetector=False, harrisK=0.04):
        self._open("gftt", capi.GfttParams(int(srcType), int(maxCorners), float(qualityLevel), float(minDistance), int(blockSize),
                                           int(bool(useHarrisDetector)), float(harrisK)))

    def setMaxCorners(self, maxCorners): self._set(max_corners=int(maxCorners))
    def setMinDistance(self, minDistance): self._set(min_distance=float(minDistance))

    def scratchBytes(self):
        b = C.c_size_t()
        capi.check(capi.lib().mi_gftt_scratch_bytes(self._h, C.byref(b)))
        return b.value

    def detect(self, image, mask=None, stream=None):
        import torch
        image = _u8(image)
        if _src_type(image) != self._p.type:
            raise MiError(-2, "image.type() == srcType")
        rows, cols = image.shape
        cap = max(1000, int(rows * cols * 0.05))   # gftt.cpp:122
        need = min(self._p.max_corners, cap) if self._p.max_corners > 0 else cap
        out = torch.empty((1, need, 2), dtype=torch.float32, device=image.device)
        n = C.c_int()
        sp = _stream_ptr(stream)
        mm = C.byref(capi.mat_from_tensor(_u8(mask))) if mask is not None else None
        capi.check(capi.lib().mi_gftt_detect(self._h, C.byref(capi.mat_from_tensor(image)), mm, C.byref(capi.mat_from_tensor(out)), C.byref(n), sp))
        return out[:, : n.value]


def createGoodFeaturesToTrackDetector(srcType, maxCorners=1000, qualityLevel=0.01, minDistance=0.0, blockSize=3, useHarrisDetector=False,
                                      harrisK=0.04) -> CornersDetector:
    """cv::cuda::createGoodFeaturesToTrackDetector, cudaimgproc.hpp:617-618"""
    return CornersDetector(srcType, maxCorners, qualityLevel, minDistance, blockSize, useHarrisDetector, harrisK)


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def gftt_response(src, deriv, smooth, blockSize, borderType=BORDER_REFLECT101, harris=False, k=0.04, form=0, dst=None, qualityLevel=None):
    """Stage entry: the response plane from explicit 3-tap kernels; form 0 / 1 / 2: the plan's choice / one launch / two launches.
    -> the plane, or (plane, threshold) with qualityLevel: (float)((double)max * qualityLevel) as the device computes it"""
    import torch
    src = _u8(src)
    if dst is None:
        dst = torch.empty(src.shape, dtype=torch.float32, device=src.device)
    thr = C.c_float()
    capi.check(capi.lib().mi_gftt_response(C.byref(capi.mat_from_tensor(src)), _f3(deriv), _f3(smooth), int(blockSize), int(borderType),
                                           int(bool(harris)), float(k), int(form), C.byref(capi.mat_from_tensor(dst)),
                                           float(qualityLevel or 0.0), C.byref(thr) if qualityLevel is not None else None,
                                           capi.current_stream_ptr()))
    return dst if qualityLevel is None else (dst, thr.value)


def gftt_find_corners(response, threshold, mask=None, max_count=1000):
    """Stage entry: findCorners -> (1, n, 2) float32 {x, y}, the first max_count in row-major order"""
    import torch
    out = torch.empty((1, int(max_count), 2), dtype=torch.float32, device=response.device)
    n = C.c_int()
    mm = C.byref(capi.mat_from_tensor(_u8(mask))) if mask is not None else None
    capi.check(capi.lib().mi_gftt_find_corners(C.byref(capi.mat_from_tensor(response)), float(threshold), mm, C.byref(capi.mat_from_tensor(out)),
                                               C.byref(n), capi.current_stream_ptr()))
    return out[:, : n.value]


def gftt_sort(response, corners):
    """Stage entry: corners (1, n, 2) by response descending, then (y, x) ascending"""
    import torch
    corners = corners.reshape(1, -1, 2).contiguous()
    n = corners.shape[1]
    out = torch.empty_like(corners)
    if n:
        capi.check(capi.lib().mi_gftt_sort(C.byref(capi.mat_from_tensor(response)), C.byref(capi.mat_from_tensor(corners)), n,
                                           C.byref(capi.mat_from_tensor(out)), capi.current_stream_ptr()))
    return out


def gftt_min_distance(points, rows, cols, minDistance, maxCorners):
    """Stage entry, host only: the grid loop of gftt.cpp:140-207 on an (n, 2) float32 NumPy array -> the survivors"""
    import numpy as np
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
    out = np.empty_like(p) if len(p) else np.empty((1, 2), np.float32)
    src = p if len(p) else np.zeros((1, 2), np.float32)
    n = C.c_int()
    fp = C.POINTER(C.c_float)
    capi.check(capi.lib().mi_gftt_min_distance(src.ctypes.data_as(fp), len(p), int(rows), int(cols), float(minDistance), int(maxCorners),
                                               out.ctypes.data_as(fp), C.byref(n)))
    return out[: n.value].copy()


def _host_mat(a):
    """a C-contiguous 2-D int32 / float32 / uint8 NumPy array as a HOST mi_mat (the array must outlive the call)"""
    import numpy as np
    types = {np.dtype(np.uint8): capi.MI_8UC1, np.dtype(np.int32): capi.MI_32SC1, np.dtype(np.float32): capi.MI_32FC1}
    assert a.ndim == 2 and a.flags.c_contiguous and a.dtype in types
    return capi.Mat(a.ctypes.data, a.strides[0], a.shape[0], a.shape[1], types[a.dtype])


def _orb_pool(pattern0):
    """pattern0 (None, or 512 points {x, y}) -> (the int32 (512, 2) array to keep alive or None, the argument for the C call)"""
    import numpy as np
    if pattern0 is None:
        return None, None
    pool = np.ascontiguousarray(np.asarray(pattern0).reshape(-1, 2), dtype=np.int32)
    return pool, C.byref(_host_mat(pool))


class ORB(_Handle):
    """cv::cuda::ORB (cudafeatures2d.hpp:452-505).  Images and masks are uint8 device tensors; keypoints are the reference's 6 x n
    CV_32FC1 matrix (rows X, Y, RESPONSE, ANGLE, OCTAVE, SIZE), descriptors n x 32 uint8.  pattern0: the pool of 512 test points the
    reference reads from its learned table when patchSize == 31 (an OpenCV binding passes its own), None: makeRandomPattern."""
    X_ROW, Y_ROW, RESPONSE_ROW, ANGLE_ROW, OCTAVE_ROW, SIZE_ROW, ROWS_COUNT = 0, 1, 2, 3, 4, 5, 6   # cudafeatures2d.hpp:455-461
    HARRIS_SCORE, FAST_SCORE = 0, 1     # cv::ORB (main repository, features2d.hpp)
    kBytes = 32
    NORM_HAMMING = 6                    # cv::NORM_HAMMING (main repository, core/base.hpp)
    PATTERN_RANDOM, PATTERN_PROVIDED = 0, 1

    def __init__(self, nfeatures=500, scaleFactor=1.2, nlevels=8, edgeThreshold=31, firstLevel=0, WTA_K=2, scoreType=0, patchSize=31,
                 fastThreshold=20, blurForDescriptor=False, pattern0=None):
        self._pool, pm = _orb_pool(pattern0)
        self._open("orb", capi.OrbParams(int(nfeatures), float(scaleFactor), int(nlevels), int(edgeThreshold), int(firstLevel), int(WTA_K),
                                         int(scoreType), int(patchSize), int(fastThreshold), int(bool(blurForDescriptor))), pm)

    @staticmethod
    def create(nfeatures=500, scaleFactor=1.2, nlevels=8, edgeThreshold=31, firstLevel=0, WTA_K=2, scoreType=0, patchSize=31, fastThreshold=20,
               blurForDescriptor=False, pattern0=None) -> "ORB":
        return ORB(nfeatures, scaleFactor, nlevels, edgeThreshold, firstLevel, WTA_K, scoreType, patchSize, fastThreshold, blurForDescriptor, pattern0)

    def _sync(self):
        capi.check(capi.lib().mi_orb_get_params(self._h, C.byref(self._p)))

    def setMaxFeatures(self, v): self._set(nfeatures=int(v))
    def getMaxFeatures(self): return self._p.nfeatures
    def setScaleFactor(self, v): self._set(scale_factor=float(v))
    def getScaleFactor(self): return float(self._p.scale_factor)
    def setNLevels(self, v): self._set(nlevels=int(v))
    def getNLevels(self): return self._p.nlevels
    def setEdgeThreshold(self, v): self._set(edge_threshold=int(v))
    def getEdgeThreshold(self): return self._p.edge_threshold
    def setFirstLevel(self, v): self._set(first_level=int(v))
    def getFirstLevel(self): return self._p.first_level
    def setWTA_K(self, v): self._set(wta_k=int(v))              # orb.cpp:376 asserts 2, 3 or 4: the library does
    def getWTA_K(self): return self._p.wta_k
    def setScoreType(self, v): self._set(score_type=int(v))
    def getScoreType(self): return self._p.score_type
    def setPatchSize(self, v): self._set(patch_size=int(v))    # orb.cpp:382 asserts >= 2: the library does
    def getPatchSize(self): return self._p.patch_size
    def setFastThreshold(self, v): self._set(fast_threshold=int(v))
    def getFastThreshold(self): return self._p.fast_threshold
    def setBlurForDescriptor(self, v): self._set(blur_for_descriptor=int(bool(v)))
    def getBlurForDescriptor(self): return bool(self._p.blur_for_descriptor)

    def descriptorSize(self): return self.kBytes
    def descriptorType(self): return 0   # CV_8U
    def defaultNorm(self): return self.NORM_HAMMING

    def getPatternSource(self):
        """PATTERN_RANDOM (generated by makeRandomPattern) or PATTERN_PROVIDED (the caller's pattern0)"""
        s = C.c_int()
        capi.check(capi.lib().mi_orb_pattern_source(self._h, C.byref(s)))
        return s.value

    def getReach(self):
        """R: edgeThreshold must be at least this for detection"""
        r = C.c_int()
        capi.check(capi.lib().mi_orb_reach(self._h, C.byref(r)))
        return r.value

    def scratchBytes(self):
        b = C.c_size_t()
        capi.check(capi.lib().mi_orb_scratch_bytes(self._h, C.byref(b)))
        return b.value

    def detectAndComputeAsync(self, image, mask=None, keypoints=None, useProvidedKeypoints=False, stream=None, computeDescriptors=True):
        """-> (keypoints, descriptors).  Detection: the (6, n) float32 keypoint matrix and the (n, 32) uint8 descriptors (None unless
        wanted) on the device.  useProvidedKeypoints: `keypoints` is a host (6, n) matrix; it comes back regrouped by octave (stable), the
        order of the descriptor rows (orb.cpp:595-600), and nlevels becomes the largest octave + 1."""
        import numpy as np
        import torch
        image = _u8(image)
        sp = _stream_ptr(stream)
        n = C.c_int()
        if useProvidedKeypoints:
            kp = np.array(keypoints.detach().cpu().numpy() if hasattr(keypoints, "detach") else keypoints, dtype=np.float32, order="C")
            if kp.ndim != 2 or kp.shape[0] != self.ROWS_COUNT:
                raise MiError(-3, "h_keypoints.rows == ROWS_COUNT")
            n.value = kp.shape[1]
            desc = torch.empty((kp.shape[1], self.kBytes), dtype=torch.uint8, device=image.device)
            km = _host_mat(kp) if kp.shape[1] else capi.Mat(kp.ctypes.data, 4, 6, 0, capi.MI_32FC1)
            dm = C.byref(capi.mat_from_tensor(desc)) if kp.shape[1] else None
            try:
                capi.check(capi.lib().mi_orb_detect_and_compute(self._h, C.byref(capi.mat_from_tensor(image)), None, C.byref(km), dm, C.byref(n), 1, sp))
            finally:
                self._sync()
            return kp, desc
        cap = max(self._p.nfeatures, 1)
        kp = torch.empty((self.ROWS_COUNT, cap), dtype=torch.float32, device=image.device)
        desc = torch.empty((cap, self.kBytes), dtype=torch.uint8, device=image.device) if computeDescriptors else None
        mask = _u8(mask) if mask is not None else None   # held in a local: a copy made here must outlive the call
        mm = C.byref(capi.mat_from_tensor(mask)) if mask is not None else None
        dm = C.byref(capi.mat_from_tensor(desc)) if desc is not None else None
        capi.check(capi.lib().mi_orb_detect_and_compute(self._h, C.byref(capi.mat_from_tensor(image)), mm, C.byref(capi.mat_from_tensor(kp)), dm,
                                                        C.byref(n), 0, sp))
        return kp[:, : n.value], (desc[: n.value] if desc is not None else None)

    def detectAndCompute(self, image, mask=None, keypoints=None, useProvidedKeypoints=False):
        """-> (keypoints as convert() gives them, descriptors on the device)"""
        kp, desc = self.detectAndComputeAsync(image, mask, keypoints, useProvidedKeypoints)
        return self.convert(kp), desc

    def detectAsync(self, image, mask=None, stream=None):
        return self.detectAndComputeAsync(image, mask, stream=stream, computeDescriptors=False)[0]

    def detect(self, image, mask=None):
        return self.convert(self.detectAsync(image, mask))

    @staticmethod
    def convert(gpu_keypoints):
        """ORB_Impl::convert (orb.cpp:868-913): a device or host matrix -> [(x, y, size, angle, response, octave)]"""
        import numpy as np
        k = gpu_keypoints.detach().cpu().numpy() if hasattr(gpu_keypoints, "detach") else np.asarray(gpu_keypoints)
        if k.size == 0:
            return []
        if k.shape[0] != ORB.ROWS_COUNT or k.dtype != np.float32:
            raise MiError(-1, "h_keypoints.rows == ROWS_COUNT && h_keypoints.type() == CV_32FC1")
        return [(float(k[0, i]), float(k[1, i]), float(k[5, i]), float(k[3, i]), float(k[2, i]), int(k[4, i])) for i in range(k.shape[1])]


def orb_make_pattern(patchSize=31, WTA_K=2, pattern0=None):
    """The 2 x N int32 matrix the reference uploads (orb.cpp:538-568), on the host"""
    import numpy as np
    out = np.zeros((2, 512 if WTA_K == 2 else 128 * WTA_K), np.int32)
    pool, pm = _orb_pool(pattern0)
    capi.check(capi.lib().mi_orb_make_pattern(int(patchSize), int(WTA_K), pm, C.byref(_host_mat(out))))
    return out


def orb_features_per_level(nfeatures=500, scaleFactor=1.2, nlevels=8):
    """n_features_per_level, orb.cpp:506-517"""
    p = capi.OrbParams()
    capi.lib().mi_orb_default_params(C.byref(p))
    p.nfeatures, p.scale_factor, p.nlevels = int(nfeatures), float(scaleFactor), int(nlevels)
    q = (C.c_int * 32)()
    capi.check(capi.lib().mi_orb_features_per_level(C.byref(p), q))
    return list(q[: p.nlevels])


def orb_u_max(patchSize=31):
    """u_max, orb.cpp:519-534"""
    u, n = (C.c_int * 32)(), C.c_int()
    capi.check(capi.lib().mi_orb_u_max(int(patchSize), u, C.byref(n)))
    return list(u[: n.value])


def _mat_or_none(t):
    return C.byref(capi.mat_from_tensor(t)) if t is not None else None


def orb_pyramid_level(src, dsize, src_mask=None, mask_mode=0, edgeThreshold=31, want_mask=True):
    """One level of buildScalePyramids (orb.cpp:672-718) -> (image, mask) of dsize = (rows, cols)"""
    import torch
    src = _u8(src)
    img = torch.empty(dsize, dtype=torch.uint8, device=src.device)
    mask = torch.empty(dsize, dtype=torch.uint8, device=src.device) if want_mask else None
    src_mask = _u8(src_mask) if src_mask is not None else None   # held in a local: a copy made here must outlive the call
    capi.check(capi.lib().mi_orb_pyramid_level(C.byref(capi.mat_from_tensor(src)), _mat_or_none(src_mask),
                                               int(mask_mode), int(edgeThreshold), C.byref(capi.mat_from_tensor(img)), _mat_or_none(mask),
                                               capi.current_stream_ptr()))
    return img, mask


def orb_cull(keypoints, n_points, out=None):
    """cull (orb.cpp:722-737) of a (2 or 3, count) keypoint matrix -> (2, kept): response descending, index ascending among equals"""
    import torch
    count = keypoints.shape[1]
    kept = count if count <= n_points else n_points
    if out is None:
        out = torch.empty((2, max(kept, 1)), dtype=torch.float32, device=keypoints.device)
    n = C.c_int()
    if count == 0:
        return out[:, :0]
    capi.check(capi.lib().mi_orb_cull(C.byref(capi.mat_from_tensor(keypoints)), count, int(n_points), C.byref(capi.mat_from_tensor(out)), C.byref(n),
                                      capi.current_stream_ptr()))
    return out[:, : n.value]


def orb_harris(image, keypoints):
    """HarrisResponses_gpu (orb.cu:94-161): writes row 1 of the (>= 2, n) keypoint matrix from row 0, in place"""
    if keypoints.shape[1] == 0:
        return keypoints
    capi.check(capi.lib().mi_orb_harris(C.byref(capi.mat_from_tensor(_u8(image))), C.byref(capi.mat_from_tensor(keypoints)), keypoints.shape[1],
                                        capi.current_stream_ptr()))
    return keypoints


def orb_angle(image, keypoints, patchSize=31):
    """IC_Angle_gpu (orb.cu:173-243): writes row 2 of the (3, n) keypoint matrix from row 0, in place -> (m_01, m_10) int32"""
    import torch
    n = keypoints.shape[1]
    m01 = torch.zeros((1, max(n, 1)), dtype=torch.int32, device=keypoints.device)
    m10 = torch.zeros_like(m01)
    if n == 0:
        return m01[0, :0], m10[0, :0]
    capi.check(capi.lib().mi_orb_angle(C.byref(capi.mat_from_tensor(_u8(image))), C.byref(capi.mat_from_tensor(keypoints)), n, int(patchSize),
                                       C.byref(capi.mat_from_tensor(m01)), C.byref(capi.mat_from_tensor(m10)), capi.current_stream_ptr()))
    return m01[0, :n], m10[0, :n]


def orb_blur(image, out=None):
    """createGaussianFilter(CV_8UC1, -1, 7 x 7, sigma 2, BORDER_REFLECT_101) (orb.cpp:570,815)"""
    import torch
    image = _u8(image)
    if out is None:
        out = torch.empty(tuple(image.shape), dtype=torch.uint8, device=image.device)
    capi.check(capi.lib().mi_orb_blur(C.byref(capi.mat_from_tensor(image)), C.byref(capi.mat_from_tensor(out)), capi.current_stream_ptr()))
    return out


def orb_descriptors(image, keypoints, pattern, WTA_K=2, out=None):
    """computeOrbDescriptor_gpu (orb.cu:250-411) from rows 0 and 2 of the (3, n) keypoint matrix; pattern: host 2 x N int32 -> (n, 32)"""
    import numpy as np
    import torch
    n = keypoints.shape[1]
    if out is None:
        out = torch.empty((max(n, 1), ORB.kBytes), dtype=torch.uint8, device=keypoints.device)
    pat = np.ascontiguousarray(pattern, dtype=np.int32)
    if n == 0:
        return out[:0]
    capi.check(capi.lib().mi_orb_descriptors(C.byref(capi.mat_from_tensor(_u8(image))), C.byref(capi.mat_from_tensor(keypoints)), n,
                                             C.byref(_host_mat(pat)), int(WTA_K), C.byref(capi.mat_from_tensor(out)), capi.current_stream_ptr()))
    return out[:n]
