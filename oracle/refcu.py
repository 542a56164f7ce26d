"""ctypes front-end of oracle/_ref/libref_cu.so -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The reference's own CUDA kernel sources -- cudastereo/src/cuda/stereobm.cu, cudaoptflow/src/cuda/farneback.cu,
cudaoptflow/src/cuda/tvl1flow.cu, cudastereo/src/cuda/disparity_bilateral_filter.cu -- compiled for the HOST: oracle/Makefile.ref
rewrites only their launch sites (oracle/refshim/cu2host.py) into oracle/_ref/ and compiles the result against
oracle/refshim/cudashim (thread blocks as cooperatively scheduled contexts, __shared__ as static storage, the few main-repo device
headers stubbed).  Every line of kernel arithmetic that runs is the reference's.  Built where /root/reference exists; the .so
travels with the tree.  tests/test_ref_pin_cuda.py holds the restated oracles to it; tests/test_ref_pin_btvl1.py the NumPy restatement of
BTV-L1 super-resolution (superres/src/cuda/btv_l1_gpu.cu, the separable filter of cudafilters, the resize / remap kernels of cudawarping,
the cudaarithm functors, and superres/src/btv_l1_cuda.cpp itself: the section at the end of this file).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import refocl

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(_HERE, "_ref", "libref_cu.so")
_lib = None
_f32 = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
_u8 = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")


def available() -> bool:
    return os.path.exists(LIB)


def has_btvl1() -> bool:
    """True if the library on disk holds the BTV-L1 entry points (one built before they existed does not: it is rebuilt where the
    reference tree is present, and the BTV-L1 pins skip where it is not)."""
    if not available():
        return False
    with open(LIB, "rb") as f:
        return b"ref_cuhost_btvl1_process" in f.read()


def lib():
    global _lib
    if _lib is None:
        if not available():
            refocl.build()
        elif not has_btvl1() and refocl.can_build():
            refocl.build(force=True)
        L = C.CDLL(LIB)
        i, f, vp = C.c_int, C.c_float, C.c_void_p
        L.ref_cu_sbm_block_match.argtypes = [_u8, _u8, i, i, i, i, i, _u8, vp]
        L.ref_cu_sbm_prefilter_xsobel.argtypes = [_u8, i, i, i, _u8]
        L.ref_cu_sbm_prefilter_norm.argtypes = [_u8, i, i, i, i, _u8]
        L.ref_cu_sbm_textureness.argtypes = [_u8, i, i, i, f, _u8]
        L.ref_cu_fb_poly_exp.argtypes = [_f32, i, i, i, _f32, _f32, _f32, f, f, f, f, _f32]
        L.ref_cu_fb_update_matrices.argtypes = [_f32, _f32, _f32, _f32, i, i, _f32]
        L.ref_cu_fb_update_flow.argtypes = [_f32, i, i, _f32, _f32]
        L.ref_cu_fb_box5.argtypes = [_f32, i, i, i, _f32]
        L.ref_cu_fb_gaussian_blur.argtypes = [_f32, i, i, _f32, i, i, _f32]
        L.ref_cu_fb_gaussian_blur5.argtypes = [_f32, i, i, _f32, i, i, _f32]
        L.ref_cu_tvl1_centered_gradient.argtypes = [_f32, i, i, _f32, _f32]
        L.ref_cu_tvl1_warp.argtypes = [_f32] * 6 + [i, i] + [_f32] * 5
        L.ref_cu_tvl1_estimate_u.argtypes = [_f32] * 4 + [vp] * 10 + [i, i, f, f, f, i]
        L.ref_cu_tvl1_estimate_dual.argtypes = [vp] * 9 + [i, i, f, f]
        L.ref_cu_dbf_apply.restype = i
        L.ref_cu_dbf_apply.argtypes = [vp, i, _u8, i, i, i, i, i, i, f, f, f]
        L.ref_cu_resize_linear_f32.argtypes = [_f32, i, i, _f32, i, i, f, f]
        L.ref_cu_resize_linear_u8.argtypes = [_u8, i, i, _u8, i, i, f, f]
        L.ref_cu_pyr_down_f32.argtypes = [_f32, i, i, _f32, i, i]
        L.ref_cu_pyr_down_u8.argtypes = [_u8, i, i, _u8, i, i]
        d = C.c_double
        L.ref_cuhost_tvl1_calc.restype = i
        L.ref_cuhost_tvl1_calc.argtypes = [d, d, d, i, i, d, i, d, d, i, vp, vp, i, i, i, _f32, C.POINTER(i)]
        _lib = L
    return _lib


def _c(a, dt=np.float32):
    return np.ascontiguousarray(a, dtype=dt)


# ---------------------------------------------------------------------------------------------------------- StereoBM
def sbm_block_match(left, right, ndisp=64, winsz=19, uniqueness_ratio=0):
    left, right = _c(left, np.uint8), _c(right, np.uint8)
    d = np.zeros_like(left)
    ssd = np.zeros(left.shape, np.uint32)
    rc = lib().ref_cu_sbm_block_match(left, right, left.shape[0], left.shape[1], ndisp, winsz, uniqueness_ratio, d, ssd.ctypes.data)
    if rc:
        raise ValueError("stereoBM_CUDA threw")
    return d, ssd


def sbm_prefilter_xsobel(img, cap=31):
    img = _c(img, np.uint8)
    out = np.zeros_like(img)
    lib().ref_cu_sbm_prefilter_xsobel(img, img.shape[0], img.shape[1], cap, out)
    return out


def sbm_prefilter_norm(img, cap=31, winsize=9):
    img = _c(img, np.uint8)
    out = np.zeros_like(img)
    lib().ref_cu_sbm_prefilter_norm(img, img.shape[0], img.shape[1], cap, winsize, out)
    return out


def sbm_textureness(img, disp, winsz=19, avg_threshold=3.0):
    img, d = _c(img, np.uint8), _c(disp, np.uint8).copy()
    lib().ref_cu_sbm_textureness(img, img.shape[0], img.shape[1], winsz, avg_threshold, d)
    return d


# --------------------------------------------------------------------------------------------------------- Farneback
def fb_poly_exp(src, poly_n, g, xg, xxg, ig):
    src = _c(src)
    h, w = src.shape
    pad = lambda a: np.ascontiguousarray(np.concatenate([a, np.zeros(8 - len(a), np.float32)]))
    dst = np.zeros((5 * h, w), np.float32)
    lib().ref_cu_fb_poly_exp(src, h, w, poly_n, pad(g), pad(xg), pad(xxg), ig[0], ig[1], ig[2], ig[3], dst)
    return dst


def fb_update_matrices(flowx, flowy, R0, R1):
    flowx, flowy, R0, R1 = map(_c, (flowx, flowy, R0, R1))
    h, w = flowx.shape
    M = np.zeros((5 * h, w), np.float32)
    lib().ref_cu_fb_update_matrices(flowx, flowy, R0, R1, h, w, M)
    return M


def fb_update_flow(M):
    M = _c(M)
    h, w = M.shape[0] // 5, M.shape[1]
    fx, fy = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
    lib().ref_cu_fb_update_flow(M, h, w, fx, fy)
    return fx, fy


def fb_box5(M, ksize):
    M = _c(M)
    out = np.zeros_like(M)
    lib().ref_cu_fb_box5(M, M.shape[0] // 5, M.shape[1], ksize // 2, out)
    return out


def fb_gaussian_blur(src, half_kernel, border):
    src, k = _c(src), _c(half_kernel)
    out = np.zeros_like(src)
    lib().ref_cu_fb_gaussian_blur(src, src.shape[0], src.shape[1], k, len(k) - 1, border, out)
    return out


def fb_gaussian_blur5(M, half_kernel, border=1):
    M, k = _c(M), _c(half_kernel)
    out = np.zeros_like(M)
    lib().ref_cu_fb_gaussian_blur5(M, M.shape[0] // 5, M.shape[1], k, len(k) - 1, border, out)
    return out


# ------------------------------------------------------------------------------------------------ TV-L1 (cv::cuda kernels)
def tvl1_centered_gradient(src):
    src = _c(src)
    dx, dy = np.zeros_like(src), np.zeros_like(src)
    lib().ref_cu_tvl1_centered_gradient(src, src.shape[0], src.shape[1], dx, dy)
    return dx, dy


def tvl1_warp(I0, I1, I1x, I1y, u1, u2):
    a = [_c(x) for x in (I0, I1, I1x, I1y, u1, u2)]
    h, w = a[0].shape
    out = [np.zeros((h, w), np.float32) for _ in range(5)]
    lib().ref_cu_tvl1_warp(*a, h, w, *out)
    return tuple(out)


def tvl1_iteration(I1wx, I1wy, grad, rho_c, u1, u2, p11, p12, p21, p22, l_t, theta, taut, gamma=0.0, u3=None, p31=None, p32=None):
    """estimateU (error plane on) then estimateDualVariables, on copies.  -> (error plane, u1, u2, p11..p22[, u3, p31, p32])."""
    st = [_c(x) for x in (I1wx, I1wy, grad, rho_c)]
    h, w = st[0].shape
    u = [_c(x).copy() for x in (u1, u2)]
    p = [_c(x).copy() for x in (p11, p12, p21, p22)]
    g3 = [_c(x).copy() if x is not None else np.zeros((h, w), np.float32) for x in (u3, p31, p32)]
    err = np.zeros((h, w), np.float32)
    ptr = lambda a: a.ctypes.data
    L = lib()
    L.ref_cu_tvl1_estimate_u(*st, ptr(p[0]), ptr(p[1]), ptr(p[2]), ptr(p[3]), ptr(g3[1]), ptr(g3[2]), ptr(u[0]), ptr(u[1]), ptr(g3[0]), ptr(err),
                             h, w, l_t, theta, gamma, 1)
    L.ref_cu_tvl1_estimate_dual(ptr(u[0]), ptr(u[1]), ptr(g3[0]), ptr(p[0]), ptr(p[1]), ptr(p[2]), ptr(p[3]), ptr(g3[1]), ptr(g3[2]), h, w, taut, gamma)
    out = (err, u[0], u[1], *p)
    return out + tuple(g3) if u3 is not None else out


# ------------------------------------------------------------------------------------------ DisparityBilateralFilter
def dbf_apply(disp, img, ndisp=64, radius=3, iters=1, edge_threshold=0.1, max_disc_threshold=0.2, sigma_range=10.0):
    disp = np.ascontiguousarray(disp).copy()
    img = np.ascontiguousarray(img, np.uint8)
    assert disp.dtype in (np.uint8, np.int16)
    ch = 1 if img.ndim == 2 else img.shape[2]
    rc = lib().ref_cu_dbf_apply(disp.ctypes.data, 0 if disp.dtype == np.uint8 else 3, img.reshape(-1), ch, disp.shape[0], disp.shape[1], ndisp, radius,
                                iters, edge_threshold, max_disc_threshold, sigma_range)
    if rc:
        raise ValueError("unsupported disparity type")
    return disp


def resize_linear(src, dsize):
    """cuda::resize(src, dst, dsize, 0, 0, INTER_LINEAR) for CV_32FC1 / CV_8UC1: the host arithmetic of cudawarping/src/resize.cpp:83-107
    (fx = dsize.width / cols in double, the kernel gets float(1 / fx)) around the reference's resize_linear kernel."""
    src = np.ascontiguousarray(src)
    sh, sw = src.shape
    dw, dh = dsize
    if (dw, dh) == (sw, sh):
        return src.copy()
    fx, fy = dw / sw, dh / sh
    dst = np.empty((dh, dw), src.dtype)
    fn = lib().ref_cu_resize_linear_f32 if src.dtype == np.float32 else lib().ref_cu_resize_linear_u8
    fn(src, sh, sw, dst, dh, dw, np.float32(1.0 / fy), np.float32(1.0 / fx))
    return dst


def pyr_down(src):
    """cuda::pyrDown (dst size (cols + 1) / 2 x (rows + 1) / 2, cudawarping/src/pyramids.cpp:66-94) on the reference's pyrDown kernel."""
    src = np.ascontiguousarray(src)
    sh, sw = src.shape
    dst = np.empty(((sh + 1) // 2, (sw + 1) // 2), src.dtype)
    fn = lib().ref_cu_pyr_down_f32 if src.dtype == np.float32 else lib().ref_cu_pyr_down_u8
    fn(src, sh, sw, dst, dst.shape[0], dst.shape[1])
    return dst


def cuda_class_tvl1_calc(I0, I1, tau=0.25, lambda_=0.15, theta=0.3, nscales=5, warps=5, epsilon=0.01, iterations=300, scale_step=0.8,
                         gamma=0.0, init_flow=None):
    """cv::cuda::OpticalFlowDual_TVL1::create(...)->calc(I0, I1, flow): the reference's HOST class (modules/cudaoptflow/src/tvl1flow.cpp,
    compiled verbatim) over the reference's kernels (tvl1flow.cu, resize.cu).  Returns (flow, nscales after the call)."""
    I0, I1 = np.ascontiguousarray(I0), np.ascontiguousarray(I1)
    assert I0.dtype == I1.dtype and I0.dtype in (np.uint8, np.float32) and I0.shape == I1.shape
    h, w = I0.shape
    flow = np.zeros((h, w, 2), np.float32)
    if init_flow is not None:
        flow[...] = init_flow
    ns = C.c_int(0)
    rc = lib().ref_cuhost_tvl1_calc(tau, lambda_, theta, nscales, warps, epsilon, iterations, scale_step, gamma, int(init_flow is not None),
                                    I0.ctypes.data, I1.ctypes.data, 0 if I0.dtype == np.uint8 else 1, w, h, flow.reshape(-1), C.byref(ns))
    if rc:
        raise ValueError("the reference class threw")
    return flow, ns.value


def cuda_class_farneback_calc(I0, I1, num_levels=5, pyr_scale=0.5, fast_pyramids=False, win_size=13, num_iters=10, poly_n=5, poly_sigma=1.1,
                              flags=0, init_flow=None):
    """cv::cuda::FarnebackOpticalFlow::create(...)->calc(I0, I1, flow): the reference's HOST class (modules/cudaoptflow/src/farneback.cpp,
    compiled verbatim) over the reference's kernels (farneback.cu, resize.cu, pyr_down.cu)."""
    I0, I1 = np.ascontiguousarray(I0), np.ascontiguousarray(I1)
    assert I0.dtype == I1.dtype and I0.dtype in (np.uint8, np.float32) and I0.shape == I1.shape
    h, w = I0.shape
    flow = np.zeros((h, w, 2), np.float32)
    if init_flow is not None:
        flow[...] = init_flow
    L = lib()
    L.ref_cuhost_farneback_calc.restype = C.c_int
    L.ref_cuhost_farneback_calc.argtypes = [C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_int, C.c_int, C.c_int, _f32]
    rc = L.ref_cuhost_farneback_calc(num_levels, pyr_scale, int(fast_pyramids), win_size, num_iters, poly_n, poly_sigma, flags,
                                     I0.ctypes.data, I1.ctypes.data, 0 if I0.dtype == np.uint8 else 1, w, h, flow.reshape(-1))
    if rc:
        raise ValueError("the reference class threw")
    return flow


def cuda_class_stereobm_compute(left, right, ndisp=64, block=19, prefilter_type=-1, prefilter_size=-1, prefilter_cap=-1, texture_threshold=-1,
                                uniqueness_ratio=-1):
    """cv::cuda::createStereoBM(ndisp, block)->compute(left, right, disp): the reference's HOST class (modules/cudastereo/src/stereobm.cpp,
    compiled verbatim) over the reference's kernels (stereobm.cu).  -1 = leave the constructor's value (no prefilter, cap 31, size 9,
    texture threshold 3, uniqueness 0)."""
    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    assert left.dtype == np.uint8 and right.dtype == np.uint8 and left.shape == right.shape
    h, w = left.shape
    disp = np.zeros((h, w), np.uint8)
    L = lib()
    L.ref_cuhost_stereobm_compute.restype = C.c_int
    L.ref_cuhost_stereobm_compute.argtypes = [C.c_int] * 7 + [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    rc = L.ref_cuhost_stereobm_compute(ndisp, block, prefilter_type, prefilter_size, prefilter_cap, texture_threshold, uniqueness_ratio,
                                       left.ctypes.data, right.ctypes.data, w, h, disp.ctypes.data)
    if rc:
        raise ValueError("the reference class threw")
    return disp


def cuda_class_surf(img, hessian_threshold=100.0, n_octaves=4, n_octave_layers=2, extended=False, keypoints_ratio=0.01, upright=False, mask=None,
                    want_desc=True, provided=None):
    """cv::cuda::SURF_CUDA::create(...) then operator(): the reference's HOST class (modules/xfeatures2d/src/surf.cuda.cpp, compiled
    verbatim) over the reference's kernels (xfeatures2d/src/cuda/surf.cu on the fiber shim).  -> the dict of oracle.surf_detect_describe,
    sorted by (octave, y, x, size) -- the class appends through atomicInc, its own order is arbitrary.  provided = dict of keypoint
    rows (x, y, octave, size, angle) for useProvidedKeypoints."""
    img = np.ascontiguousarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    rows, cols = img.shape
    cap = 65536
    kp = np.zeros((7, cap), np.uint32)
    dsz = 128 if extended else 64
    n_in = 0
    if provided is not None:
        n_in = len(provided["x"])
        kf = kp.view(np.float32)
        ki = kp.view(np.int32)
        kf[0, :n_in] = provided["x"]; kf[1, :n_in] = provided["y"]; ki[2, :n_in] = 1; ki[3, :n_in] = provided["octave"]
        kf[4, :n_in] = provided["size"]; kf[5, :n_in] = provided["angle"]; kf[6, :n_in] = provided.get("hessian", 0.0)
    desc = np.zeros((cap if provided is None else max(n_in, 1), dsz), np.float32) if want_desc else None
    m = np.ascontiguousarray(mask) if mask is not None else None
    L = lib()
    L.ref_cuhost_surf.restype = C.c_int
    L.ref_cuhost_surf.argtypes = [C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_void_p, C.c_int, C.c_void_p]
    n = L.ref_cuhost_surf(hessian_threshold, n_octaves, n_octave_layers, int(extended), keypoints_ratio, int(upright), img.ctypes.data,
                          m.ctypes.data if m is not None else None, cols, rows, int(provided is not None), n_in, kp.ctypes.data, cap,
                          desc.ctypes.data if want_desc else None)
    if n < 0:
        raise ValueError("the reference class threw" if n == -1 else "keypoint capacity")
    kf, ki = kp.view(np.float32), kp.view(np.int32)
    out = {"n": n, "x": kf[0, :n].copy(), "y": kf[1, :n].copy(), "laplacian": ki[2, :n].copy(), "octave": ki[3, :n].copy(),
           "size": kf[4, :n].copy(), "angle": kf[5, :n].copy(), "hessian": kf[6, :n].copy(),
           "descriptors": desc[:n].copy() if want_desc else None}
    if provided is None:
        order = np.lexsort((out["size"], out["x"], out["y"], out["octave"]))
        for k in ("x", "y", "laplacian", "octave", "size", "angle", "hessian"):
            out[k] = out[k][order]
        if want_desc:
            out["descriptors"] = out["descriptors"][order]
    return out


def cuda_class_dbf_apply(disp, img, ndisp=64, radius=3, iters=1, edge_threshold=-1.0, max_disc_threshold=-1.0, sigma_range=-1.0):
    """cv::cuda::createDisparityBilateralFilter(ndisp, radius, iters)->apply(disp, img, dst): the reference's HOST class
    (modules/cudastereo/src/disparity_bilateral_filter.cpp, compiled verbatim: weight tables, edge_disc / max_disc, type dispatch) over the
    reference kernel.  Negative thresholds keep the constructor's defaults (0.1, 0.2, 10)."""
    disp = np.ascontiguousarray(disp).copy()
    img = np.ascontiguousarray(img, np.uint8)
    assert disp.dtype in (np.uint8, np.int16) and img.shape[:2] == disp.shape
    ch = 1 if img.ndim == 2 else img.shape[2]
    L = lib()
    L.ref_cuhost_dbf_apply.restype = C.c_int
    L.ref_cuhost_dbf_apply.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]
    rc = L.ref_cuhost_dbf_apply(ndisp, radius, iters, edge_threshold, max_disc_threshold, sigma_range, disp.ctypes.data,
                                0 if disp.dtype == np.uint8 else 3, img.ctypes.data, ch, disp.shape[1], disp.shape[0])
    if rc:
        raise ValueError("the reference class threw")
    return disp


# ----------------------------------------------------------------------------------------------- BTV-L1 super-resolution (superres)
# superres/src/cuda/btv_l1_gpu.cu and the cudafilters / cudawarping / cudaarithm kernels BTVL1_CUDA runs, on the fiber shim; the host side
# is the reference's superres/src/btv_l1_cuda.cpp, cudawarping/src/resize.cpp and remap.cpp (verbatim) and the separable-filter slice of
# cudafilters/src/filtering.cpp.  Images are (H, W) or (H, W, CN) float32, CN in {3, 4}; a raised ValueError = the reference threw.
BTV_DEFAULTS = dict(scale=4, iterations=180, tau=1.3, lambda_=0.03, alpha=0.7, btv_kernel_size=7, blur_kernel_size=5, blur_sigma=0.0)


def _img(a):
    a = _c(a)
    assert a.ndim in (2, 3)
    return a, a.shape[0], a.shape[1], (1 if a.ndim == 2 else a.shape[2])


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _ok(rc):
    if rc:
        raise ValueError("the reference threw" if rc == 1 else "the reference returned an unexpected size or type")


def btv_build_motion_maps(forward_motion, backward_motion):
    """buildMotionMaps (btv_l1_cuda.cpp:131-144 over buildMotionMapsKernel).  -> ((forward map x, y), (backward map x, y))."""
    fx, fy, bx, by = (_c(a) for a in (*forward_motion, *backward_motion))
    out = [np.empty_like(fx) for _ in range(4)]
    _ok(lib().ref_cuhost_btv_motion_maps(_p(fx), _p(fy), _p(bx), _p(by), fx.shape[0], fx.shape[1], *(_p(o) for o in out)))
    return (out[0], out[1]), (out[2], out[3])


def btv_upscale(src, scale):
    """upscale (btv_l1_cuda.cpp:146-162: dst zeroed, then upscaleKernel)."""
    s, h, w, cn = _img(src)
    dst = np.empty((h * scale, w * scale) + s.shape[2:], np.float32)
    _ok(lib().ref_cuhost_btv_upscale(_p(s), h, w, cn, scale, _p(dst)))
    return dst


def btv_diff_sign(a, b):
    """diffSign (btv_l1_cuda.cpp:164-169: both reshaped to one channel, DiffSign through device::transform)."""
    a, h, w, cn = _img(a)
    b = _c(b)
    dst = np.empty_like(a)
    _ok(lib().ref_cuhost_btv_diff_sign(_p(a), _p(b), h, w, cn, _p(dst)))
    return dst


def btv_regularization(src, btv_kernel_size, weights):
    """loadBtvWeights(weights) then calcBtvRegularization (btv_l1_cuda.cpp:189-207 over calcBtvRegularizationKernel)."""
    s, h, w, cn = _img(src)
    wts = _c(weights)
    assert wts.size <= 256
    dst = np.empty_like(s)
    _ok(lib().ref_cuhost_btv_regularization(_p(s), h, w, cn, btv_kernel_size, _p(wts), wts.size, _p(dst)))
    return dst


def btv_weights(btv_kernel_size, alpha):
    """calcBtvWeights (btv_l1_cuda.cpp:171-187): the whole vector of btvKernelSize^2 floats (only the enumerated entries are set)."""
    out = np.zeros(btv_kernel_size * btv_kernel_size, np.float32)
    _ok(lib().ref_cuhost_btv_weights(btv_kernel_size, C.c_double(alpha), _p(out)))
    return out


def _pack_motions(motions, shape):
    present = np.array([m is not None for m in motions], np.int32)
    planes = np.zeros((len(motions), 2) + tuple(shape), np.float32)
    for i, m in enumerate(motions):
        if m is not None:
            planes[i, 0], planes[i, 1] = m
    return planes, present


def btv_upscale_motions(motions, scale):
    """upscaleMotions (btv_l1_cuda.cpp:117-129): cuda::resize(INTER_CUBIC, null stream) then cuda::multiply by Scalar::all(scale)."""
    h, w = motions[0][0].shape
    planes, _ = _pack_motions(motions, (h, w))
    out = np.empty((len(motions), 2, h * scale, w * scale), np.float32)
    _ok(lib().ref_cuhost_btv_upscale_motions(_p(planes), len(motions), h, w, scale, _p(out)))
    return [(o[0].copy(), o[1].copy()) for o in out]


def btv_relative_motions(forward, backward, base_idx, size):
    """calcRelativeMotions (btv_l1_cuda.cpp:80-115, cuda::add = the reference's AddOp1).  None entries stay empty GpuMats."""
    f, fp = _pack_motions(forward, size)
    b, bp = _pack_motions(backward, size)
    of, ob = np.empty_like(f), np.empty_like(b)
    _ok(lib().ref_cuhost_btv_relative_motions(_p(f), _p(fp), _p(b), _p(bp), len(forward), size[0], size[1], base_idx, _p(of), _p(ob)))
    return [(o[0].copy(), o[1].copy()) for o in of], [(o[0].copy(), o[1].copy()) for o in ob]


def cuda_gaussian_kernel(n, sigma):
    """getGaussianKernel(n, sigma, CV_32F) as the stub core forwards it (oracle/imgproc_ref.c: a main-repo stand-in, not reference text)."""
    out = np.empty(n, np.float32)
    _ok(lib().ref_cuhost_gaussian_kernel(n, C.c_double(sigma), _p(out)))
    return out


def cuda_gauss_filter(src, ksize, sigma):
    """cuda::createGaussianFilter(type, -1, Size(ksize, ksize), sigma)->apply(src, dst, a stream): filtering.cpp's createGaussianFilter and
    SeparableLinearFilter over linearRowFilter / linearColumnFilter with the cc >= 20 geometry."""
    s, h, w, cn = _img(src)
    dst = np.empty_like(s)
    _ok(lib().ref_cuhost_gauss_filter(_p(s), h, w, cn, ksize, C.c_double(sigma), _p(dst)))
    return dst


def cuda_separable_filter(src, kernel):
    """cuda::createSeparableLinearFilter(type, -1, kernel, kernel)->apply: the filter createGaussianFilter builds, with any taps (1 .. 32)."""
    s, h, w, cn = _img(src)
    k = _c(kernel)
    dst = np.empty_like(s)
    _ok(lib().ref_cuhost_separable_filter(_p(s), h, w, cn, _p(k), k.size, _p(dst)))
    return dst


def _cuda_resize(src, dh, dw, interpolation, own_stream):
    s, h, w, cn = _img(src)
    dst = np.empty((dh, dw) + s.shape[2:], np.float32)
    _ok(lib().ref_cuhost_resize(_p(s), h, w, cn, dh, dw, interpolation, int(own_stream), _p(dst)))
    return dst


def cuda_resize_nearest(src, dh, dw):
    """cuda::resize(src, dst, Size(dw, dh), 0, 0, INTER_NEAREST, a stream) (resize.cpp verbatim over resize_nearest), as btv_l1_cuda.cpp:373."""
    return _cuda_resize(src, dh, dw, 0, True)


def cuda_resize_cubic(src, dh, dw):
    """cuda::resize(..., INTER_CUBIC) on the null stream (resize.cpp verbatim over the generic resize kernel with CubicFilter), as
    btv_l1_cuda.cpp:123-124,354."""
    return _cuda_resize(src, dh, dw, 2, False)


def cuda_remap_nearest_replicate(src, mapx, mapy):
    """cuda::remap(src, dst, mapx, mapy, INTER_NEAREST, BORDER_REPLICATE, Scalar(), a stream) (remap.cpp verbatim over RemapDispatcherStream)."""
    s, h, w, cn = _img(src)
    mx, my = _c(mapx), _c(mapy)
    dst = np.empty(mx.shape + s.shape[2:], np.float32)
    _ok(lib().ref_cuhost_remap_nearest_replicate(_p(s), h, w, cn, _p(mx), _p(my), mx.shape[0], mx.shape[1], _p(dst)))
    return dst


def cuda_add_weighted(a, alpha, b, beta, gamma):
    """cuda::addWeighted on CV_32F: AddWeightedOp<float, float, float, float> (add_weighted.cu:61-93) over every element."""
    a, b = _c(a), _c(b)
    dst = np.empty_like(a)
    L = lib()
    L.ref_cu_add_weighted_f32.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_size_t]
    L.ref_cu_add_weighted_f32(_p(a), alpha, _p(b), beta, gamma, _p(dst), a.size)
    return dst


def cuda_multiply_scalar(a, val):
    """cuda::multiply(src, Scalar::all(val), dst) on CV_32F: MulScalarOp<float, float, float> (mul_scalar.cu:61-69,151)."""
    a = _c(a)
    dst = np.empty_like(a)
    L = lib()
    L.ref_cu_mul_scalar_f32.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_size_t]
    L.ref_cu_mul_scalar_f32(_p(a), val, _p(dst), a.size)
    return dst


class BTVL1Class:
    """One object of the reference's BTVL1_CUDA kept across process() calls (its filter and weight caches, btv_l1_cuda.cpp:320-335)."""

    def __init__(self):
        L = lib()
        L.ref_cuhost_btvl1_new.restype = C.c_void_p
        L.ref_cuhost_btvl1_delete.argtypes = [C.c_void_p]
        self._h = C.c_void_p(L.ref_cuhost_btvl1_new())
        assert self._h

    def __del__(self):
        if getattr(self, "_h", None):
            lib().ref_cuhost_btvl1_delete(self._h)
            self._h = None

    def process(self, frames, forward, backward, base_idx, **params):
        """-> (result, btvWeights_ after the call)."""
        p = dict(BTV_DEFAULTS, **params)
        fr = np.ascontiguousarray(np.stack([_c(f) for f in frames]))
        n, h, w = fr.shape[:3]
        cn = 1 if fr.ndim == 3 else fr.shape[3]
        f, fp = _pack_motions(forward, (h, w))
        b, bp = _pack_motions(backward, (h, w))
        s, bk = p["scale"], p["btv_kernel_size"]
        out = np.empty((max(h * s - 2 * bk, 0), max(w * s - 2 * bk, 0)) + fr.shape[3:], np.float32)
        wts = np.zeros(max(bk, 1) ** 2, np.float32)
        L = lib()
        L.ref_cuhost_btvl1_process.argtypes = [C.c_void_p] * 2 + [C.c_int] * 4 + [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_double] * 3 + [C.c_int] * 2 + \
            [C.c_double, C.c_void_p, C.c_void_p]
        _ok(L.ref_cuhost_btvl1_process(self._h, _p(fr), n, h, w, cn, _p(f), _p(fp), _p(b), _p(bp), base_idx, s, p["iterations"], p["tau"], p["lambda_"],
                                       p["alpha"], bk, p["blur_kernel_size"], p["blur_sigma"], _p(out), _p(wts)))
        return out, wts


def cuda_class_btvl1_process(frames, fwd, bwd, base, **params):
    """BTVL1_CUDA_Base::process (btv_l1_cuda.cpp:306-400) on a fresh object of the reference's class.  -> (result, btvWeights_).  The filter
    taps live inside the reference's SeparableLinearFilter (another translation unit's unnamed namespace) and are not returned; they are
    cuda_gaussian_kernel(blur_kernel_size, blur_sigma)."""
    return BTVL1Class().process(frames, fwd, bwd, base, **params)


def cuda_class_btvl1_sequence(frames, flows, temporal_area_radius=4, **params):
    """createSuperResolution_BTVL1_CUDA() -> setInput(a list-backed FrameSource over `frames`, u8 or f32), setOpticalFlow(an algorithm that
    hands out `flows` -- a list of (x, y) planes -- in call order), nextFrame until it returns nothing.
    -> (list of u8 outputs, list of (index of frame0, index of frame1) per flow request, True if the frame after the last was empty twice)."""
    p = dict(BTV_DEFAULTS, **params)
    fr = np.ascontiguousarray(np.stack([np.ascontiguousarray(f) for f in frames]))
    assert fr.dtype in (np.uint8, np.float32)
    n, h, w = fr.shape[:3]
    cn = 1 if fr.ndim == 3 else fr.shape[3]
    fl = np.ascontiguousarray(np.stack([np.stack([_c(x), _c(y)]) for x, y in flows])) if len(flows) else np.zeros((0, 2, h, w), np.float32)
    s, bk = p["scale"], p["btv_kernel_size"]
    oh, ow = h * s - 2 * bk, w * s - 2 * bk
    max_out = n + 3
    out = np.zeros((max_out, oh, ow) + fr.shape[3:], np.uint8)
    calls = np.full((4 * n + 8, 2), -2, np.int32)
    n_out, ended, n_calls = C.c_int(0), C.c_int(0), C.c_int(0)
    L = lib()
    L.ref_cuhost_btvl1_sequence.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] + [C.c_int] * 4 + [C.c_double] * 3 + [C.c_int] * 2 + [C.c_double] + \
        [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    _ok(L.ref_cuhost_btvl1_sequence(_p(fr), n, h, w, cn, 0 if fr.dtype == np.uint8 else 1, _p(fl), len(flows), temporal_area_radius, s, p["iterations"],
                                    p["tau"], p["lambda_"], p["alpha"], bk, p["blur_kernel_size"], p["blur_sigma"], _p(out), max_out, C.byref(n_out),
                                    C.byref(ended), _p(calls), len(calls), C.byref(n_calls)))
    return [out[i].copy() for i in range(n_out.value)], [tuple(int(v) for v in c) for c in calls[:n_calls.value]], bool(ended.value)
