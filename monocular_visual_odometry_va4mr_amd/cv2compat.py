"""The reference's cv2 call surface, executed by libvo_hip.so on the GPU (boundary B1).

Same names, argument meanings, dtypes and output shapes as the OpenCV 4.6 calls made by
/root/reference/VisualOdometryPipeLine.py:

    goodFeaturesToTrack   :256        calcOpticalFlowPyrLK  :281,:287
    solvePnPRansac (P3P)  :343        Rodrigues             :354
    triangulatePoints     :188        SIFT_create / detectAndCompute :35,:226-227
    BFMatcher.knnMatch    :36,:229    findEssentialMat      :308
    recoverPose           :315

and, beyond the reference, cornerSubPix (the call behind goodFeaturesToTrack in most KLT front
ends) and solvePnPRefineLM, in this project's own arithmetic, and the four calls of a camera with
lens distortion: initUndistortRectifyMap, remap, undistort and undistortPoints.

Each call copies numpy inputs to the device, runs the HIP kernels and copies results
back (the drop-in mode; the device-resident path is engine.Engine).  Installing this
module as ``sys.modules['cv2']`` lets the reference class itself run on the GPU.
There is no CPU fallback: every function raises if the HIP library is unavailable.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from .engine import Engine, make_opts

RANSAC = 8
LMEDS = 4
SOLVEPNP_ITERATIVE = 0
SOLVEPNP_EPNP = 1
SOLVEPNP_P3P = 2
TERM_CRITERIA_COUNT = 1
TERM_CRITERIA_MAX_ITER = 1
TERM_CRITERIA_EPS = 2
IMREAD_GRAYSCALE = 0
OPTFLOW_USE_INITIAL_FLOW = 4
OPTFLOW_LK_GET_MIN_EIGENVALS = 8
NORM_L2 = 4
INTER_NEAREST = 0
INTER_LINEAR = 1
BORDER_CONSTANT = 0
CV_32FC1 = 5
CV_16SC2 = 11


class error(Exception):
    """Mirror of cv2.error."""


def _dev():
    if not torch.cuda.is_available():
        raise RuntimeError("cv2compat needs a ROCm GPU (no CPU fallback)")
    return torch.device("cuda")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: torch.Tensor):
    return C.c_void_p(t.data_ptr())


_DEFAULT_OPTS = {
    "min_dist_landmarks": 1, "max_dist_landmarks": 150, "min_baseline_angle": 2, "min_baseline_frames": 2,
    "feature_ratio": 0.8, "feature_max_corners": 1400, "feature_quality_level": 0.1, "feature_min_dist": 10,
    "feature_block_size": 3, "feature_use_harris": False, "winSize": (21, 21), "maxLevel": 3,
    "criteria": (3, 30, 0.01), "PnP_conf": 0.99, "PnP_error": 8.0, "PnP_iterations": 100,
}

_ENGINES: dict = {}


def _engine(W, H, **over):
    key = (W, H, tuple(sorted((k, v if not isinstance(v, list) else tuple(v)) for k, v in over.items())))
    eng = _ENGINES.get(key)
    if eng is None:
        opts = dict(_DEFAULT_OPTS)
        opts.update(over)
        eng = Engine(np.eye(3), opts, W, H, batch=1, ncap=256, pcap=256, fcap=4)
        _ENGINES[key] = eng
    return eng


def _gray(img):
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise error("expected a uint8 grayscale image (CV_8UC1)")
    return np.ascontiguousarray(a)


# ---------------------------------------------------------------- GFTT (:256)
def goodFeaturesToTrack(image, maxCorners, qualityLevel, minDistance, mask=None, blockSize=3,
                        useHarrisDetector=False, k=0.04):
    """cv2.goodFeaturesToTrack.  ``mask``: None, or a uint8 array of the image's shape whose non-zero
    pixels are the allowed ones (any non-zero value counts; vo_gftt_masked): the quality
    level scales the maximum over the allowed pixels, only allowed pixels become corners, and the
    3x3 local-maximum test still sees every neighbour.  A mask with no allowed pixel gives None."""
    img = _gray(image)
    H, W = img.shape
    d_mask = None
    if mask is not None:
        m = np.asarray(mask)
        if m.dtype != np.uint8 or m.shape != img.shape:
            raise error("mask must be uint8 (CV_8UC1) and of the image's size")
        d_mask = torch.from_numpy(np.ascontiguousarray(m)).to("cuda")
    eng = _engine(W, H, feature_max_corners=int(maxCorners), feature_quality_level=float(qualityLevel),
                  feature_min_dist=float(minDistance), feature_block_size=int(blockSize),
                  feature_use_harris=bool(useHarrisDetector))
    eng.opts.harris_k = float(k)
    eng.t["status"].zero_()
    eng.build_pyramid(img, 0)
    if d_mask is None:
        L.check(eng.lib.vo_gftt(eng._pd, eng._po, eng._ps, 0, _stream()), "vo_gftt")
    else:
        L.check(eng.lib.vo_gftt_masked(eng._pd, eng._po, eng._ps, 0, _p(d_mask), W * H, W, _stream()), "vo_gftt_masked")
    st = int(eng.t["status"][0])
    if st != 0:
        raise error(L.STATUS_NAMES.get(st, str(st)))
    n = int(eng.t["nCorners"][0])
    if n < 0:
        # more corners than the engine holds (maxCorners <= 0 and more than its 8192): the selection
        # reports it instead of truncating, as a chain's step does with VO_ST_CAPACITY
        raise error(L.STATUS_NAMES[L.ST_CAPACITY])
    if n == 0:
        return None
    return eng.t["corners"][0, :n].cpu().numpy().reshape(-1, 1, 2).copy()


# ---------------------------------------------------------------- LK (:281,:287)
def calcOpticalFlowPyrLK(prevImg, nextImg, prevPts, nextPts, winSize=(21, 21), maxLevel=3,
                         criteria=(TERM_CRITERIA_COUNT | TERM_CRITERIA_EPS, 30, 0.01), flags=0,
                         minEigThreshold=1e-4, *, illumination=None):
    """cv2.calcOpticalFlowPyrLK.  ``flags``: OPTFLOW_USE_INITIAL_FLOW (each point's estimate starts
    at ``nextPts``, float32 with as many points as ``prevPts``) and OPTFLOW_LK_GET_MIN_EIGENVALS
    (``err`` is the minimum eigenvalue of the level-0 tensor, for every point whose window is in
    bounds); any other bit raises NotImplementedError.  Without OPTFLOW_USE_INITIAL_FLOW a given
    ``nextPts`` is ignored (OpenCV only uses it as the output buffer); no input array is written.
    Supported ``winSize``: 3 to 32 pixels per side and at most 1024 pixels in all (the default
    21x21 included); any other window raises (vo_lk_points_ex returns VO_EARG).  15x15 runs the one-launch kernel k_lk_w, every other size
    the per-level k_lk; sides above the pyramid's 16-pixel border take the window's taps at
    reflect-101 coordinates with zero derivatives outside the image, as OpenCV's winSize-wide
    pyramid border does.  ``illumination`` is a keyword of this project's own (cv2 has none): None
    (off), "bias" or "gain_bias" frees the mismatch of an additive offset, or of an offset and a
    gain, of ``nextImg`` against ``prevImg`` (vo_lk_points_illum; every window then runs
    k_lk); any other value raises ValueError."""
    from .engine import ILLUMINATION_MODELS, parse_illumination
    illumination = parse_illumination({"lk_illumination": illumination})
    flags = int(flags)
    if flags & ~(OPTFLOW_USE_INITIAL_FLOW | OPTFLOW_LK_GET_MIN_EIGENVALS):
        raise NotImplementedError("only OPTFLOW_USE_INITIAL_FLOW and OPTFLOW_LK_GET_MIN_EIGENVALS are supported")
    p = np.asarray(prevPts)
    if p.dtype != np.float32:
        raise error("prevPts must be float32 (checkVector(2, CV_32F))")
    shape = p.shape
    pts = np.ascontiguousarray(p.reshape(-1, 2))
    n = pts.shape[0]
    ini = None
    if flags & OPTFLOW_USE_INITIAL_FLOW:
        if nextPts is None:
            raise error("OPTFLOW_USE_INITIAL_FLOW needs nextPts")
        q = np.asarray(nextPts)
        if q.dtype != np.float32 or q.size != 2 * n:
            raise error("nextPts must be float32 with as many points as prevPts (checkVector(2, CV_32F) == npoints)")
        ini = np.ascontiguousarray(q.reshape(-1, 2))
    a, b = _gray(prevImg), _gray(nextImg)
    if a.shape != b.shape:
        raise error("prevImg and nextImg must have the same size")
    H, W = a.shape
    eng = _engine(W, H, winSize=tuple(int(v) for v in winSize), maxLevel=int(maxLevel),
                  criteria=tuple(criteria))
    eng.opts.min_eig = float(minEigThreshold)
    eng.build_pyramid(a, 0)
    eng.build_pyramid(b, 1)
    dev = _dev()
    if n == 0:
        return np.zeros(shape, np.float32), np.zeros((0, 1), np.uint8), np.zeros((0, 1), np.float32)
    dp = torch.from_numpy(pts).to(dev).reshape(1, n, 2)
    cnt = torch.tensor([n], dtype=torch.int32, device=dev)
    out = torch.empty((1, n, 2), dtype=torch.float32, device=dev)
    st = torch.empty((1, n), dtype=torch.uint8, device=dev)
    err = torch.empty((1, n), dtype=torch.float32, device=dev)
    di = None if ini is None else torch.from_numpy(ini).to(dev).reshape(1, n, 2)
    if illumination is not None:
        L.check(eng.lib.vo_lk_points_illum(eng._pd, eng._po, eng._ps, 0, _p(dp), None if di is None else _p(di), _p(cnt),
                                           n, flags, ILLUMINATION_MODELS[illumination], C.c_double(0.0), None, _p(out),
                                           _p(st), _p(err), _stream()), "vo_lk_points_illum")
    else:
        L.check(eng.lib.vo_lk_points_ex(eng._pd, eng._po, eng._ps, 0, _p(dp), None if di is None else _p(di), _p(cnt), n,
                                        flags, _p(out), _p(st), _p(err), _stream()), "vo_lk_points_ex")
    return (out.cpu().numpy().reshape(shape), st.cpu().numpy().reshape(-1, 1),
            err.cpu().numpy().reshape(-1, 1))


# ---------------------------------------------------------------- cornerSubPix
SUBPIX_MAX_HALF_WIN = 7


def cornerSubPix(image, corners, winSize, zeroZone, criteria):
    """cv2.cornerSubPix's form over vo_corner_subpix: ``corners`` (float32, (N, 1, 2) or (N, 2)) are
    refined in place on the uint8 grayscale ``image`` and returned in the same shape.  ``winSize``
    is the half-window (w, h), 1..7 each (larger raises NotImplementedError); ``zeroZone``
    (-1, -1) or half sizes inside the window.  The iteration is this project's own, not
    OpenCV's arithmetic: criteria's count is the iteration limit, clamped to 1..100 (100 without
    the COUNT bit), its epsilon the step length that ends the walk (max(eps, 0); 0 without the
    EPS bit).  The image is not written."""
    img = _gray(image)
    if not isinstance(corners, np.ndarray) or corners.dtype != np.float32:
        raise error("cornerSubPix: corners must be a float32 array (checkVector(2, CV_32F))")
    if not ((corners.ndim == 2 and corners.shape[1] == 2) or (corners.ndim == 3 and corners.shape[1:] == (1, 2))):
        raise error("cornerSubPix: corners must have shape (N, 2) or (N, 1, 2)")
    try:
        w, h = (int(v) for v in winSize)
        zw, zh = (int(v) for v in zeroZone)
        ctype, count, eps = criteria
        ctype, count, eps = int(ctype), int(count), float(eps)
    except (TypeError, ValueError) as e:
        raise error(f"cornerSubPix: bad winSize, zeroZone or criteria ({e})") from None
    if w < 1 or h < 1:
        raise error("cornerSubPix: winSize must be at least (1, 1)")
    if w > SUBPIX_MAX_HALF_WIN or h > SUBPIX_MAX_HALF_WIN:
        raise NotImplementedError(f"cornerSubPix: half-windows above {SUBPIX_MAX_HALF_WIN} are not supported "
                                  f"(got {(w, h)})")
    if (zw, zh) != (-1, -1) and not (0 <= zw < w and 0 <= zh < h):
        raise error("cornerSubPix: zeroZone must be (-1, -1) or lie inside the window")
    max_iters = min(max(count, 1), 100) if ctype & TERM_CRITERIA_COUNT else 100
    eps = max(eps, 0.0) if ctype & TERM_CRITERIA_EPS else 0.0
    if not math.isfinite(eps):
        raise error("cornerSubPix: the criteria's epsilon must be finite")
    n = corners.shape[0]
    if n == 0:
        return corners
    H, W = img.shape
    dev = _dev()
    d_img = torch.from_numpy(img).to(dev)
    d_pts = torch.from_numpy(np.ascontiguousarray(corners.reshape(n, 2))).to(dev)
    cnt = torch.tensor([n], dtype=torch.int32, device=dev)
    L.check(L.lib().vo_corner_subpix(1, _p(d_img), W * H, W, W, H, _p(d_pts), _p(cnt), n, w, h, zw, zh, max_iters,
                                     C.c_double(eps), None, _stream()), "vo_corner_subpix")
    corners[...] = d_pts.cpu().numpy().reshape(corners.shape)
    return corners


# ---------------------------------------------------------------- lens distortion
def _camera(K, what):
    """K as nine C doubles; the form [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] is required."""
    a = np.asarray(K, np.float64)
    if a.shape == (3, 4):                       # a projection matrix: its camera part
        a = a[:, :3]
    if a.shape != (3, 3) or not np.all(np.isfinite(a)) or a[0, 1] != 0 or a[1, 0] != 0 or a[2, 0] != 0 or a[2, 1] != 0 \
            or a[2, 2] != 1 or a[0, 0] == 0 or a[1, 1] == 0:
        raise error(f"{what} must be a finite 3x3 matrix of the form [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]")
    return (C.c_double * 9)(*a.ravel())


def _dist(distCoeffs):
    """(C doubles or None, count) of 4, 5 or 8 coefficients k1 k2 p1 p2 [k3 [k4 k5 k6]]; None or empty = none."""
    d = np.zeros(0) if distCoeffs is None else np.asarray(distCoeffs, np.float64).ravel()
    if d.size in (12, 14):
        raise NotImplementedError("thin-prism and tilted-sensor models (12 or 14 distortion coefficients) are not supported")
    if d.size not in (0, 4, 5, 8):
        raise error("distCoeffs must hold 4, 5 or 8 coefficients (or be None)")
    return ((C.c_double * d.size)(*d) if d.size else None), int(d.size)


def _no_rotation(R):
    if R is not None and np.asarray(R).size and not np.array_equal(np.asarray(R, np.float64), np.eye(3)):
        raise NotImplementedError("a rectification rotation R other than None or the identity is not supported")


def _empty(m):
    return m is None or np.asarray(m).size == 0


def initUndistortRectifyMap(cameraMatrix, distCoeffs, R, newCameraMatrix, size, m1type):
    """cv2.initUndistortRectifyMap over vo_undistort_map (the project's own arithmetic).
    ``size`` is (W, H), each 1..16384.  ``m1type`` CV_16SC2 gives the fixed-point pair (map1 int16
    (H, W, 2), map2 uint16 (H, W)); CV_32FC1 gives two float32 (H, W) maps, the fp64 positions
    rounded once.  An empty ``newCameraMatrix`` is ``cameraMatrix``.  4, 5 or 8 coefficients; 12 or 14
    and a rotation ``R`` other than None or the identity raise NotImplementedError."""
    _no_rotation(R)
    if m1type not in (CV_16SC2, CV_32FC1):
        raise NotImplementedError("m1type must be CV_16SC2 or CV_32FC1")
    Kc = _camera(cameraMatrix, "cameraMatrix")
    Kn = None if _empty(newCameraMatrix) else _camera(newCameraMatrix, "newCameraMatrix")
    dc, nd = _dist(distCoeffs)
    W, H = (int(v) for v in size)
    if not (1 <= W <= 16384 and 1 <= H <= 16384):
        raise error("size must be (W, H) with both in 1..16384")
    dev = _dev()
    m1 = torch.empty((H, W, 2), dtype=torch.int16, device=dev)
    m2 = torch.empty((H, W), dtype=torch.int16, device=dev)
    md = torch.empty((H, W, 2), dtype=torch.float64, device=dev) if m1type == CV_32FC1 else None
    L.check(L.lib().vo_undistort_map(Kc, dc, nd, Kn, W, H, _p(m1), _p(m2), None if md is None else _p(md), _stream()),
            "vo_undistort_map")
    if md is not None:
        m = md.cpu().numpy().astype(np.float32)
        return np.ascontiguousarray(m[..., 0]), np.ascontiguousarray(m[..., 1])
    return m1.cpu().numpy(), m2.cpu().numpy().view(np.uint16)


def _fixed_point_maps(map1, map2):
    """The fixed-point pair of remap's map arguments: itself, or two float32 maps quantised on the host
    as vo_undistort_map quantises (rint(32 m), half to even, clamped to [-2^20, 2^20 - 1], NaN -> -2^20)."""
    a = np.asarray(map1)
    if a.dtype == np.int16 and a.ndim == 3 and a.shape[2] == 2:
        b = np.asarray(map2)
        if b.dtype != np.uint16 or b.shape != a.shape[:2]:
            raise error("with a CV_16SC2 map1, map2 must be uint16 (CV_16UC1) of the same size")
        return np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32 and a.ndim == 2 and not _empty(map2):
        b = np.asarray(map2)
        if b.dtype != np.float32 or b.shape != a.shape:
            raise error("with a CV_32FC1 map1, map2 must be float32 (CV_32FC1) of the same size")

        def q(m):
            with np.errstate(all="ignore"):
                t = np.rint(32.0 * m.astype(np.float64))
            return np.where(np.isnan(t), -1048576.0, np.clip(t, -1048576.0, 1048575.0)).astype(np.int64)
        iu, iv = q(a), q(b)
        return (np.ascontiguousarray(np.stack([iu >> 5, iv >> 5], -1).astype(np.int16)),
                ((iv & 31) * 32 + (iu & 31)).astype(np.uint16))
    raise NotImplementedError("maps must be the CV_16SC2 / CV_16UC1 pair or two CV_32FC1 maps")


def remap(src, map1, map2, interpolation, dst=None, borderMode=BORDER_CONSTANT, borderValue=0):
    """cv2.remap over vo_remap_u8: a uint8 single-channel ``src`` through the fixed-point pair of
    initUndistortRectifyMap(CV_16SC2), or through two float32 maps (quantised on the host to the same
    1/32 pixel), with INTER_LINEAR and a constant border of 0; anything else raises
    NotImplementedError.  The result has the maps' size."""
    if interpolation != INTER_LINEAR:
        raise NotImplementedError("only INTER_LINEAR is supported")
    if borderMode != BORDER_CONSTANT or np.any(np.asarray(borderValue) != 0):
        raise NotImplementedError("only borderMode=BORDER_CONSTANT with borderValue=0 is supported")
    a = np.asarray(src)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise NotImplementedError("remap takes a uint8 single-channel image (CV_8UC1)")
    img = np.ascontiguousarray(a)
    m1, m2 = _fixed_point_maps(map1, map2)
    H, W = m2.shape
    sH, sW = img.shape
    if not (1 <= W <= 16384 and 1 <= H <= 16384 and 1 <= sW <= 16384 and 1 <= sH <= 16384):
        raise error("image and map sides must be in 1..16384")
    dev = _dev()
    d_src = torch.from_numpy(img).to(dev)
    d_m1 = torch.from_numpy(m1).to(dev)
    d_m2 = torch.from_numpy(m2.view(np.int16)).to(dev)
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)
    L.check(L.lib().vo_remap_u8(1, _p(d_src), sW * sH, sW, sW, sH, _p(out), W * H, W, W, H, _p(d_m1), _p(d_m2), _stream()),
            "vo_remap_u8")
    res = out.cpu().numpy()
    if dst is not None:
        dst[...] = res
        return dst
    return res


def undistort(src, cameraMatrix, distCoeffs, dst=None, newCameraMatrix=None):
    """cv2.undistort: remap(src, *initUndistortRectifyMap(K, dist, None, newK, src's size, CV_16SC2),
    INTER_LINEAR), with the limits of both."""
    a = np.asarray(src)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise NotImplementedError("undistort takes a uint8 single-channel image (CV_8UC1)")
    m1, m2 = initUndistortRectifyMap(cameraMatrix, distCoeffs, None, newCameraMatrix, (a.shape[1], a.shape[0]), CV_16SC2)
    return remap(a, m1, m2, INTER_LINEAR, dst=dst)


def undistortPoints(src, cameraMatrix, distCoeffs, R=None, P=None):
    """cv2.undistortPoints over vo_undistort_points with OpenCV's default of 5 iterations (a fixed
    count, no epsilon test): ``src`` float32 or float64 of shape (N, 1, 2) or (N, 2) in raw
    pixels; returns (N, 1, 2) of the same dtype, normalised coordinates, or pixels through ``P``."""
    _no_rotation(R)
    p = np.asarray(src)
    if p.dtype not in (np.float32, np.float64):
        raise error("undistortPoints: src must be float32 or float64")
    if not ((p.ndim == 2 and p.shape[1] == 2) or (p.ndim == 3 and p.shape[1:] == (1, 2))):
        raise error("undistortPoints: src must have shape (N, 2) or (N, 1, 2)")
    Kc = _camera(cameraMatrix, "cameraMatrix")
    Pc = None if _empty(P) else _camera(P, "P")
    dc, nd = _dist(distCoeffs)
    n = p.shape[0]
    if n == 0:
        return np.zeros((0, 1, 2), p.dtype)
    dev = _dev()
    d_pts = torch.from_numpy(np.ascontiguousarray(p.reshape(n, 2).astype(np.float64))).to(dev)
    out = torch.empty((n, 2), dtype=torch.float64, device=dev)
    L.check(L.lib().vo_undistort_points(n, _p(d_pts), Kc, dc, nd, Pc, 5, _p(out), _stream()), "vo_undistort_points")
    return out.cpu().numpy().astype(p.dtype).reshape(n, 1, 2)


# ---------------------------------------------------------------- PnP (:343)
def solvePnPRansac(objectPoints, imagePoints, cameraMatrix, distCoeffs, rvec=None, tvec=None,
                   useExtrinsicGuess=False, iterationsCount=100, reprojectionError=8.0,
                   confidence=0.99, inliers=None, flags=SOLVEPNP_ITERATIVE):
    if flags != SOLVEPNP_P3P or useExtrinsicGuess:
        raise NotImplementedError("the reference uses flags=SOLVEPNP_P3P (:343)")
    if distCoeffs is not None and np.any(np.asarray(distCoeffs) != 0):
        raise NotImplementedError("non-zero distortion: rectify the image with undistort, or the points with "
                                  "undistortPoints(..., P=cameraMatrix), and pass distCoeffs=None")
    obj = np.ascontiguousarray(np.asarray(objectPoints, np.float32).reshape(-1, 3))
    img = np.ascontiguousarray(np.asarray(imagePoints, np.float32).reshape(-1, 2))
    n = obj.shape[0]
    if n < 4 or img.shape[0] != n:
        raise error("solvePnPRansac: npoints >= 4 && npoints == ipoints required")
    opts = dict(_DEFAULT_OPTS, PnP_conf=float(confidence), PnP_error=float(reprojectionError),
                PnP_iterations=int(iterationsCount))
    o = make_opts(np.asarray(cameraMatrix, np.float64), opts)
    dev = _dev()
    d_obj = torch.from_numpy(obj).to(dev)
    d_img = torch.from_numpy(img).to(dev)
    cnt = torch.tensor([n], dtype=torch.int32, device=dev)
    rv = torch.zeros(3, dtype=torch.float64, device=dev)
    tv = torch.zeros(3, dtype=torch.float64, device=dev)
    ok = torch.zeros(1, dtype=torch.int32, device=dev)
    mask = torch.zeros(n, dtype=torch.uint8, device=dev)
    ninl = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = 12 * n + 64
    work = torch.empty(ws, dtype=torch.float64, device=dev)
    L.check(L.lib().vo_pnp_ransac(C.byref(o), 1, _p(d_obj), _p(d_img), _p(cnt), n, _p(rv), _p(tv), _p(ok),
                                  _p(mask), _p(ninl), _p(work), ws, _stream()), "vo_pnp_ransac")
    success = bool(ok.item())
    if not success:
        return False, rv.cpu().numpy().reshape(3, 1), tv.cpu().numpy().reshape(3, 1), None
    inl = np.nonzero(mask.cpu().numpy())[0].astype(np.int32).reshape(-1, 1)
    return True, rv.cpu().numpy().reshape(3, 1), tv.cpu().numpy().reshape(3, 1), inl


FLT_EPSILON = 1.1920928955078125e-07


def solvePnPRefineLM(objectPoints, imagePoints, cameraMatrix, distCoeffs, rvec, tvec,
                     criteria=(TERM_CRITERIA_COUNT | TERM_CRITERIA_EPS, 20, FLT_EPSILON)):
    """cv2.solvePnPRefineLM's form over vo_pnp_refine: Levenberg-Marquardt on the reprojection
    error from (rvec, tvec); returns the refined (rvec, tvec) as 3x1 float64 and leaves its inputs
    alone.  The iteration is this project's own, not OpenCV's LMSolver: criteria's
    count is the iteration limit (100 without the COUNT bit), its epsilon the relative cost
    tolerance (0 without the EPS bit)."""
    if distCoeffs is not None and np.any(np.asarray(distCoeffs) != 0):
        raise NotImplementedError("non-zero distortion: rectify the image with undistort, or the points with "
                                  "undistortPoints(..., P=cameraMatrix), and pass distCoeffs=None")
    obj = np.ascontiguousarray(np.asarray(objectPoints, np.float32).reshape(-1, 3))
    img = np.ascontiguousarray(np.asarray(imagePoints, np.float32).reshape(-1, 2))
    n = obj.shape[0]
    if img.shape[0] != n:
        raise error("solvePnPRefineLM: npoints == ipoints required")
    ctype, count, eps = criteria
    max_iters = int(count) if int(ctype) & TERM_CRITERIA_COUNT else 100
    ftol = float(eps) if int(ctype) & TERM_CRITERIA_EPS else 0.0
    if not 0 <= max_iters <= 100 or not (math.isfinite(ftol) and ftol >= 0):
        raise error("solvePnPRefineLM: criteria must give 0..100 iterations and a finite epsilon >= 0")
    o = make_opts(np.asarray(cameraMatrix, np.float64), dict(_DEFAULT_OPTS))
    dev = _dev()
    d_obj = torch.from_numpy(obj).to(dev)
    d_img = torch.from_numpy(img).to(dev)
    cnt = torch.tensor([n], dtype=torch.int32, device=dev)
    rv = torch.from_numpy(np.array(rvec, np.float64).reshape(3)).to(dev)       # copies: the inputs stay
    tv = torch.from_numpy(np.array(tvec, np.float64).reshape(3)).to(dev)
    L.check(L.lib().vo_pnp_refine(C.byref(o), 1, _p(d_obj), _p(d_img), None, _p(cnt), n, None, max_iters,
                                  C.c_double(ftol), _p(rv), _p(tv), None, _stream()), "vo_pnp_refine")
    return rv.cpu().numpy().reshape(3, 1), tv.cpu().numpy().reshape(3, 1)


# ---------------------------------------------------------------- DLT (:188)
def triangulatePoints(projMatr1, projMatr2, projPoints1, projPoints2):
    x1 = np.asarray(projPoints1)
    if x1.dtype != np.float32:
        raise NotImplementedError("float32 points (the reference's dtype, Q10)")
    x1 = np.ascontiguousarray(x1.reshape(2, -1).T)
    x2 = np.ascontiguousarray(np.asarray(projPoints2, np.float32).reshape(2, -1).T)
    n = x1.shape[0]
    dev = _dev()
    P1 = torch.from_numpy(np.ascontiguousarray(np.asarray(projMatr1, np.float64).reshape(1, 12))).to(dev).expand(n, 12).contiguous()
    P2 = torch.from_numpy(np.ascontiguousarray(np.asarray(projMatr2, np.float64).reshape(1, 12))).to(dev).expand(n, 12).contiguous()
    a = torch.from_numpy(x1).to(dev)
    b = torch.from_numpy(x2).to(dev)
    out = torch.empty((n, 4), dtype=torch.float32, device=dev)
    L.check(L.lib().vo_triangulate_points(n, _p(P1), _p(P2), _p(a), _p(b), _p(out), _stream()), "vo_triangulate_points")
    return out.cpu().numpy().T.copy()


# ---------------------------------------------------------------- Rodrigues (:354)
def Rodrigues(src, dst=None, jacobian=None):
    s = np.asarray(src, np.float64)
    dev = _dev()
    if s.size == 3:
        inp = torch.from_numpy(np.ascontiguousarray(s.reshape(3))).to(dev)
        out = torch.empty(9, dtype=torch.float64, device=dev)
        L.check(L.lib().vo_rodrigues(1, 1, _p(inp), _p(out), _stream()), "vo_rodrigues")
        return out.cpu().numpy().reshape(3, 3), np.zeros((3, 9))
    if s.size != 9:
        raise error("Rodrigues expects a 3-vector or a 3x3 matrix")
    inp = torch.from_numpy(np.ascontiguousarray(s.reshape(9))).to(dev)
    out = torch.empty(3, dtype=torch.float64, device=dev)
    L.check(L.lib().vo_rodrigues(1, 0, _p(inp), _p(out), _stream()), "vo_rodrigues")
    return out.cpu().numpy().reshape(3, 1), np.zeros((9, 3))


# ---------------------------------------------------------------- SIFT / BF (:35-36, :226-229)
class KeyPoint:
    __slots__ = ("pt", "size", "angle", "response", "octave", "class_id")

    def __init__(self, x=0.0, y=0.0, size=0.0, angle=-1.0, response=0.0, octave=0, class_id=-1):
        self.pt = (float(x), float(y))
        self.size = float(size)
        self.angle = float(angle)
        self.response = float(response)
        self.octave = int(octave)
        self.class_id = int(class_id)


class DMatch:
    __slots__ = ("queryIdx", "trainIdx", "imgIdx", "distance")

    def __init__(self, queryIdx=-1, trainIdx=-1, imgIdx=0, distance=float(np.finfo(np.float32).max)):
        self.queryIdx = int(queryIdx)
        self.trainIdx = int(trainIdx)
        self.imgIdx = int(imgIdx)
        self.distance = float(distance)


_SIFTS: dict = {}


class _SIFT:
    def __init__(self, nfeatures: int = 0):
        self.nfeatures = int(nfeatures)

    def detectAndCompute(self, image, mask):
        from .features import Sift
        if mask is not None:
            raise NotImplementedError("mask is not used by the reference (:226 passes None)")
        img = _gray(image)
        H, W = img.shape
        s = _SIFTS.get((W, H, self.nfeatures))
        if s is None:
            s = _SIFTS[(W, H, self.nfeatures)] = Sift(W, H, _dev(), nfeatures=self.nfeatures)
        s.run(torch.from_numpy(img).to(_dev()))
        kp, desc = s.result()
        kps = tuple(KeyPoint(k[0], k[1], k[2], k[3], k[4], int(k[5])) for k in kp)
        return kps, (desc.copy() if len(kps) else None)


def SIFT_create(nfeatures=0, *args, **kwargs):
    """SIFT_create() (:35) or SIFT_create(nfeatures) (KeyPointsFilter::retainBest cap, BASELINE C5);
    the other SIFT parameters keep OpenCV's defaults."""
    if args or kwargs or int(nfeatures) < 0:
        raise NotImplementedError("only nfeatures may be set (the reference uses the default SIFT, :35)")
    return _SIFT(nfeatures)


class _BFMatcher:
    def knnMatch(self, queryDescriptors, trainDescriptors, k=2):
        from .features import bf_knn2
        if k != 2:
            raise NotImplementedError("the reference uses k=2 (:229)")
        q = np.ascontiguousarray(np.asarray(queryDescriptors, np.float32))
        t = np.ascontiguousarray(np.asarray(trainDescriptors, np.float32))
        if q.ndim != 2 or q.shape[1] != 128 or t.shape[1] != 128:
            raise NotImplementedError("128-D float descriptors (SIFT)")
        if not (np.array_equal(q, np.round(q)) and np.array_equal(t, np.round(t))):
            raise NotImplementedError("the MFMA matcher is exact for integer-valued (SIFT) descriptors")
        # the int8 kernel stores v - 128: exact for 0..255 (SIFT's saturate_cast<uchar> range),
        # anything outside would wrap into a wrong distance
        if (q.size and (q.min() < 0 or q.max() > 255)) or (t.size and (t.min() < 0 or t.max() > 255)):
            raise NotImplementedError("the MFMA matcher takes descriptor values 0..255 (SIFT)")
        dev = _dev()
        nq, nt = q.shape[0], t.shape[0]
        if nq == 0:
            return ()
        dq = torch.from_numpy(q).to(dev)
        dt = torch.from_numpy(t if nt else np.zeros((1, 128), np.float32)).to(dev)
        cq = torch.tensor([nq], dtype=torch.int32, device=dev)
        ct = torch.tensor([nt], dtype=torch.int32, device=dev)
        idx2, dist2 = bf_knn2(dq, cq, dt, ct, nq)
        idx2 = idx2.cpu().numpy()
        dist2 = dist2.cpu().numpy()
        out = []
        for i in range(nq):
            out.append(tuple(DMatch(i, int(idx2[i, j]), 0, float(dist2[i, j])) for j in range(2) if idx2[i, j] >= 0))
        return tuple(out)


def BFMatcher(normType=NORM_L2, crossCheck=False):
    if normType != NORM_L2 or crossCheck:
        raise NotImplementedError
    return _BFMatcher()


# ---------------------------------------------------------------- E / pose (:308, :315)
def findEssentialMat(points1, points2, cameraMatrix, method=RANSAC, prob=0.999, threshold=1.0, maxIters=1000,
                     mask=None):
    if method != RANSAC:
        raise NotImplementedError("the reference uses RANSAC (:308)")
    p0 = np.ascontiguousarray(np.asarray(points1, np.float32).reshape(-1, 2))
    p1 = np.ascontiguousarray(np.asarray(points2, np.float32).reshape(-1, 2))
    n = p0.shape[0]
    if p1.shape[0] != n:
        raise error("points1 and points2 must have the same size")
    o = make_opts(np.asarray(cameraMatrix, np.float64), _DEFAULT_OPTS)
    dev = _dev()
    a = torch.from_numpy(p0 if n else np.zeros((1, 2), np.float32)).to(dev)
    b = torch.from_numpy(p1 if n else np.zeros((1, 2), np.float32)).to(dev)
    cap = max(n, 1)
    cnt = torch.tensor([n], dtype=torch.int32, device=dev)
    E = torch.zeros(9, dtype=torch.float64, device=dev)
    m = torch.zeros(cap, dtype=torch.uint8, device=dev)
    ok = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = 4 * cap + 90 * 64 + 64
    work = torch.empty(ws, dtype=torch.float64, device=dev)
    L.check(L.lib().vo_find_essential(C.byref(o), 1, _p(a), _p(b), _p(cnt), cap, float(prob), float(threshold),
                                      int(maxIters), _p(E), _p(m), _p(ok), _p(work), ws, _stream()),
            "vo_find_essential")
    mk = m.cpu().numpy()[:n].reshape(-1, 1)
    if not int(ok.item()):
        return None, mk
    return E.cpu().numpy().reshape(3, 3), mk


def recoverPose(E, points1, points2, cameraMatrix, *args, **kwargs):
    if args or kwargs:
        raise NotImplementedError("the reference passes (E, p0, p1, K) only (:315)")
    p0 = np.ascontiguousarray(np.asarray(points1, np.float32).reshape(-1, 2))
    p1 = np.ascontiguousarray(np.asarray(points2, np.float32).reshape(-1, 2))
    n = p0.shape[0]
    o = make_opts(np.asarray(cameraMatrix, np.float64), _DEFAULT_OPTS)
    dev = _dev()
    cap = max(n, 1)
    a = torch.from_numpy(p0 if n else np.zeros((1, 2), np.float32)).to(dev)
    b = torch.from_numpy(p1 if n else np.zeros((1, 2), np.float32)).to(dev)
    cnt = torch.tensor([n], dtype=torch.int32, device=dev)
    dE = torch.from_numpy(np.ascontiguousarray(np.asarray(E, np.float64).reshape(9))).to(dev)
    R = torch.zeros(9, dtype=torch.float64, device=dev)
    t = torch.zeros(3, dtype=torch.float64, device=dev)
    m = torch.zeros(cap, dtype=torch.uint8, device=dev)
    ng = torch.zeros(1, dtype=torch.int32, device=dev)
    L.check(L.lib().vo_recover_pose(C.byref(o), 1, _p(dE), _p(a), _p(b), _p(cnt), cap, _p(R), _p(t), _p(m), _p(ng),
                                    _stream()), "vo_recover_pose")
    return (int(ng.item()), R.cpu().numpy().reshape(3, 3), t.cpu().numpy().reshape(3, 1),
            (m.cpu().numpy()[:n].reshape(-1, 1) * 255).astype(np.uint8))
