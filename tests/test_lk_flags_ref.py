"""A NumPy restatement of calcOpticalFlowPyrLK's per-point tracker with OpenCV's flags, and the
forward-backward gate built on it: the reference of test_gpu_lk_flags.py and test_gpu_lk_fb.py.

The C oracle's vo_o_lk (oracle/vo_oracle_img.c) has no flags.  py_lk below follows it operation
for operation (float32 / integer arithmetic, pyramids from oracle._olib.pyrdown, derivatives from
_olib.scharr, reflect-101 image borders and zero derivative borders of window width), all points
of a level at once, and adds

    OPTFLOW_USE_INITIAL_FLOW = 4      the estimate starts at init[i] * 2^-L at the top level L
    OPTFLOW_LK_GET_MIN_EIGENVALS = 8  err[i] = the tensor's minimum eigenvalue at every level whose
                                      prev window is in bounds (so level 0's where that one is),
                                      set before the threshold test; no level-0 L1 error pass

as OpenCV 4.6's lkpyramid.cpp does.  This file first pins py_lk(flags = 0) to
vo_o_lk bit for bit, then checks on py_lk alone that the init sets and flag cases the GPU tests
use are not vacuous.  Everything here runs on the CPU.

Crops and points re-create the recipes of test_gpu_lk_windows.py (same crop origins, same kinds of
points), about 400 points per case.
"""
import numpy as np
import pytest

USE_INITIAL_FLOW, GET_MIN_EIGENVALS = 4, 8
SIZES = {(160, 120): (430, 170), (131, 67): (700, 215), (96, 200): (250, 120)}   # (W, H): crop origin (x, y)
# one window per kernel instantiation: k_lk_w, k_lk<4, false>, k_lk<4, true>, k_lk<16, true>
WINDOWS = [(15, 15), (9, 15), (21, 9), (21, 21)]
LEVELS = [0, 3]
BASE_CRIT = (3, 30, 0.01)
MIN_EIG = 1e-4
F32 = np.float32


# ------------------------------------------------------------------ the restatement
def _refl101(i, n):
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def _levels(img, L, bx, by, with_deriv):
    """Per level: (w, h, padded image, padded derivative or None), as build_levels."""
    from oracle import _olib as O
    out = []
    cur = np.ascontiguousarray(img)
    for l in range(L + 1):
        if l > 0:
            cur = O.pyrdown(cur)
        h, w = cur.shape
        pad = cur[_refl101(np.arange(-by, h + by), h)][:, _refl101(np.arange(-bx, w + bx), w)].astype(np.int64)
        der = None
        if with_deriv:
            der = np.zeros((h + 2 * by, w + 2 * bx, 2), np.int64)
            der[by:by + h, bx:bx + w] = O.scharr(cur)
        out.append((w, h, pad, der))
    return out


def _weights(a, b):
    """iw00, iw01, iw10, iw11 of the float32 fractions a, b (lrintf = round half to even)."""
    s = F32(1 << 14)
    one = F32(1)
    iw00 = np.rint((one - a) * (one - b) * s).astype(np.int64)
    iw01 = np.rint(a * (one - b) * s).astype(np.int64)
    iw10 = np.rint((one - a) * b * s).astype(np.int64)
    return iw00, iw01, iw10, (1 << 14) - iw00 - iw01 - iw10


def _window(arr, ix, iy, bx, by, ww, wh):
    """The (wh + 1) x (ww + 1) patches at (ix, iy) of a padded array: [n, wh + 1, ww + 1, ...]."""
    ry = (iy + by)[:, None] + np.arange(wh + 1)[None, :]
    cx = (ix + bx)[:, None] + np.arange(ww + 1)[None, :]
    return arr[ry[:, :, None], cx[:, None, :]]


def _bilin(p, w, shift):
    """DESCALE(p00 w00 + p01 w01 + p10 w10 + p11 w11, shift) over the window."""
    w00, w01, w10, w11 = (v[:, None, None] for v in w)
    s = p[:, :-1, :-1] * w00 + p[:, :-1, 1:] * w01 + p[:, 1:, :-1] * w10 + p[:, 1:, 1:] * w11
    return (s + (1 << (shift - 1))) >> shift


def py_lk(prev, nxt, pts, win, max_level, criteria, min_eig, flags=0, init=None):
    """(out [n, 2] f32, status [n] u8, err [n] f32) of calcOpticalFlowPyrLK(prev, nxt, pts) with
    `flags`; `init` [n, 2] f32 is read only with USE_INITIAL_FLOW."""
    from oracle import _olib as O
    assert flags & ~(USE_INITIAL_FLOW | GET_MIN_EIGENVALS) == 0
    pts = np.asarray(pts, F32).reshape(-1, 2)
    n = len(pts)
    ww, wh = int(win[0]), int(win[1])
    H, W = prev.shape
    ctype, max_count, eps = criteria
    max_count = 30 if not (ctype & 1) else min(max(int(max_count), 0), 100)
    eps = 0.01 if not (ctype & 2) else min(max(float(eps), 0.0), 10.0)
    eps *= eps
    thr = F32(min_eig)
    L = O.pyr_maxlevel(W, H, (ww, wh), int(max_level))
    PI = _levels(prev, L, ww, wh, True)
    PJ = _levels(nxt, L, ww, wh, False)
    hx, hy = F32((ww - 1) * 0.5), F32((wh - 1) * 0.5)
    SCALE = F32(1.0 / (1 << 20))
    EPSF = np.finfo(F32).eps
    out = np.zeros((n, 2), F32)
    status = np.ones(n, np.uint8)
    err = np.zeros(n, F32)
    if n == 0:
        return out, status, err
    if flags & USE_INITIAL_FLOW:
        init = np.asarray(init, F32).reshape(-1, 2)
        assert len(init) == n
    for level in range(L, -1, -1):
        cols, rows, Iimg, Ider = PI[level]
        Jimg = PJ[level][2]
        sc = F32(1.0 / (1 << level))
        px, py = pts[:, 0] * sc, pts[:, 1] * sc
        if level == L:
            nx, ny = (init[:, 0] * sc, init[:, 1] * sc) if flags & USE_INITIAL_FLOW else (px.copy(), py.copy())
        else:
            nx, ny = out[:, 0] * F32(2), out[:, 1] * F32(2)
        out[:, 0], out[:, 1] = nx, ny
        px, py = px - hx, py - hy
        fpx, fpy = np.floor(px), np.floor(py)
        oob = (fpx < -ww) | (fpx >= cols) | (fpy < -wh) | (fpy >= rows) | ~np.isfinite(fpx) | ~np.isfinite(fpy)
        if level == 0:
            status[oob] = 0
            err[oob] = 0
        idx = np.flatnonzero(~oob)
        if idx.size == 0:
            continue
        ipx, ipy = fpx[idx].astype(np.int64), fpy[idx].astype(np.int64)
        wgt = _weights(px[idx] - ipx.astype(F32), py[idx] - ipy.astype(F32))
        Iwin = _bilin(_window(Iimg, ipx, ipy, ww, wh, ww, wh), wgt, 9)
        dwin = _window(Ider, ipx, ipy, ww, wh, ww, wh)
        Ix, Iy = _bilin(dwin[..., 0], wgt, 14), _bilin(dwin[..., 1], wgt, 14)
        A11 = (Ix * Ix).sum((1, 2)).astype(F32) * SCALE
        A12 = (Ix * Iy).sum((1, 2)).astype(F32) * SCALE
        A22 = (Iy * Iy).sum((1, 2)).astype(F32) * SCALE
        D = A11 * A22 - A12 * A12
        min_e = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + F32(4) * A12 * A12)) / F32(2 * ww * wh)
        if flags & GET_MIN_EIGENVALS:
            err[idx] = min_e
        rej = (min_e < thr) | (D < EPSF)
        if level == 0:
            status[idx[rej]] = 0
        keep = ~rej
        idx, Iwin, Ix, Iy = idx[keep], Iwin[keep], Ix[keep], Iy[keep]
        A11, A12, A22 = A11[keep], A12[keep], A22[keep]
        with np.errstate(divide="ignore"):
            D = F32(1) / D[keep]
        cx, cy = nx[idx] - hx, ny[idx] - hy
        pdx, pdy = np.zeros(len(idx), F32), np.zeros(len(idx), F32)
        run = np.arange(len(idx))               # positions (in idx) still iterating
        for j in range(max_count):
            if run.size == 0:
                break
            fx, fy = np.floor(cx[run]), np.floor(cy[run])
            ob = (fx < -ww) | (fx >= cols) | (fy < -wh) | (fy >= rows) | ~np.isfinite(fx) | ~np.isfinite(fy)
            if level == 0:
                status[idx[run[ob]]] = 0
            run, fx, fy = run[~ob], fx[~ob], fy[~ob]
            if run.size == 0:
                break
            inx, iny = fx.astype(np.int64), fy.astype(np.int64)
            wj = _weights(cx[run] - inx.astype(F32), cy[run] - iny.astype(F32))
            diff = _bilin(_window(Jimg, inx, iny, ww, wh, ww, wh), wj, 9) - Iwin[run]
            b1 = (diff * Ix[run]).sum((1, 2)).astype(F32) * SCALE
            b2 = (diff * Iy[run]).sum((1, 2)).astype(F32) * SCALE
            ddx = (A12[run] * b2 - A22[run] * b1) * D[run]
            ddy = (A12[run] * b1 - A11[run] * b2) * D[run]
            cx[run] += ddx
            cy[run] += ddy
            ox, oy = cx[run] + hx, cy[run] + hy
            conv = ddx.astype(np.float64) * ddx.astype(np.float64) + ddy.astype(np.float64) * ddy.astype(np.float64) <= eps
            osc = np.zeros(len(run), bool)
            if j > 0:
                osc = ~conv & (np.abs(ddx + pdx[run]) < F32(0.01)) & (np.abs(ddy + pdy[run]) < F32(0.01))
                ox = np.where(osc, ox - ddx * F32(0.5), ox)
                oy = np.where(osc, oy - ddy * F32(0.5), oy)
            out[idx[run], 0], out[idx[run], 1] = ox, oy
            pdx[run], pdy[run] = ddx, ddy
            run = run[~(conv | osc)]
        if level == 0 and not flags & GET_MIN_EIGENVALS:
            sel = np.flatnonzero(status[idx] == 1)
            g = idx[sel]
            fx, fy = out[g, 0] - hx, out[g, 1] - hy
            ffx, ffy = np.floor(fx), np.floor(fy)
            ob = (ffx < -ww) | (ffx >= cols) | (ffy < -wh) | (ffy >= rows) | ~np.isfinite(ffx) | ~np.isfinite(ffy)
            status[g[ob]] = 0
            sel, g, fx, fy, ffx, ffy = sel[~ob], g[~ob], fx[~ob], fy[~ob], ffx[~ob], ffy[~ob]
            if g.size:
                inx, iny = ffx.astype(np.int64), ffy.astype(np.int64)
                we = _weights(fx - inx.astype(F32), fy - iny.astype(F32))
                diff = _bilin(_window(Jimg, inx, iny, ww, wh, ww, wh), we, 9) - Iwin[sel]
                # a float sum of integers below 2^24 is exact in any order
                err[g] = np.abs(diff).sum((1, 2)).astype(F32) / F32(32 * ww * wh)
    return out, status, err


def fb_compose(prev, nxt, pts, win, max_level, criteria, min_eig, thr, flags=0, init=None, forward=None):
    """The forward-backward gate as a composition: (q, gate, err_f, back, st_f, st_b).  The forward
    pass is `forward` (default: the C oracle for flags 0, py_lk otherwise); the backward pass is the
    C oracle's plain call from nxt to prev on the forward-tracked points; the gate is taken in double."""
    from oracle import _olib as O
    pts = np.asarray(pts, F32).reshape(-1, 2)
    if forward is not None:
        q, sf, ef = forward
    elif flags == 0:
        q, sf, ef = O.lk(prev, nxt, pts, win, max_level, criteria, min_eig)
    else:
        q, sf, ef = py_lk(prev, nxt, pts, win, max_level, criteria, min_eig, flags, init)
    m = sf == 1
    back = np.zeros_like(q)
    sb = np.zeros_like(sf)
    if m.any():
        back[m], sb[m], _ = O.lk(nxt, prev, np.ascontiguousarray(q[m]), win, max_level, criteria, min_eig)
    dx = (back[:, 0] - pts[:, 0]).astype(np.float64)
    dy = (back[:, 1] - pts[:, 1]).astype(np.float64)
    with np.errstate(invalid="ignore"):
        gate = m & (sb == 1) & (dx * dx + dy * dy <= float(thr) * float(thr))
    return q, gate.astype(np.uint8), ef, back, sf, sb


# ------------------------------------------------------------------ inputs
_FRAMES = {}


def frames():
    if "fr" not in _FRAMES:
        from monocular_visual_odometry_va4mr_amd.synth import make_sequence
        _FRAMES["fr"] = make_sequence("kitti", 2, seed=1)[0]
    return _FRAMES["fr"]


def crop_pair(W, H, origin=None):
    """The (W, H) crop of frames 0 and 1 at `origin` (default: the size's own)."""
    x0, y0 = SIZES[(W, H)] if origin is None else origin
    fr = frames()
    return (np.ascontiguousarray(fr[0][y0:y0 + H, x0:x0 + W]), np.ascontiguousarray(fr[1][y0:y0 + H, x0:x0 + W]))


def make_points(img, win, seed, n_corners=200, n_uniform=110, n_tiny=40, n_edge=50):
    """About 400 float32 points: GFTT corners, uniform points over the image plus a window-wide
    margin, corners with 1e-3-scale sub-pixel offsets (iw11 goes negative there), and points on
    the acceptance edges ipx in {-win_w - 1, -win_w, cols - 1, cols} (likewise y)."""
    from oracle import _olib as O
    H, W = img.shape
    ww, wh = win
    rng = np.random.default_rng(seed)
    corners = O.gftt(img, n_corners, 0.01, 4, 3)
    uni = np.c_[rng.uniform(-ww - 2, W + ww + 2, n_uniform), rng.uniform(-wh - 2, H + wh + 2, n_uniform)]
    k = min(n_tiny, len(corners))
    tiny = corners[:k] + F32([[1e-3, 2e-3]]) * rng.integers(1, 8, (k, 2))
    hx, hy = (ww - 1) * 0.5, (wh - 1) * 0.5
    edge = []
    for i in range(n_edge):
        f = (0.0, 0.25, 0.5)[i % 3]
        if (i // 3) % 2 == 0:
            ip = (-ww - 1, -ww, W - 1, W)[(i // 6) % 4]
            edge.append((ip + hx + f, rng.uniform(-wh + hy, H - 1 + hy)))
        else:
            ip = (-wh - 1, -wh, H - 1, H)[(i // 6) % 4]
            edge.append((rng.uniform(-ww + hx, W - 1 + hx), ip + hy + f))
    return np.ascontiguousarray(np.concatenate([corners, uni, tiny, np.array(edge)]).astype(F32))


_CACHE = {}


def case_points(W, H, win, origin=None, seed=0, npts=None):
    key = ("pts", W, H, tuple(win), origin, seed, npts)
    if key not in _CACHE:
        pts = make_points(crop_pair(W, H, origin)[0], win, seed)
        if npts is not None:
            pts = np.ascontiguousarray(pts[np.random.default_rng(seed).permutation(len(pts))[:npts]])
        pts.setflags(write=False)
        _CACHE[key] = pts
    return _CACHE[key]


def ref_lk(W, H, win, max_level, flags=0, init_kind=None, origin=None, seed=0, npts=None):
    """(pts, init or None, out, status, err) of py_lk for one case; computed once and shared,
    read-only."""
    key = ("lk", W, H, tuple(win), max_level, flags, init_kind, origin, seed, npts)
    if key not in _CACHE:
        a, b = crop_pair(W, H, origin)
        pts = case_points(W, H, win, origin, seed, npts)
        init = make_init(W, H, win, init_kind, origin, seed, npts) if flags & USE_INITIAL_FLOW else None
        res = py_lk(a, b, pts, win, max_level, BASE_CRIT, MIN_EIG, flags, init)
        for v in res:
            v.setflags(write=False)
        _CACHE[key] = (pts, init) + res
    return _CACHE[key]


def oracle_lk(W, H, win, max_level, origin=None, seed=0, npts=None):
    """The C oracle's plain call on the same case."""
    from oracle import _olib as O
    key = ("olk", W, H, tuple(win), max_level, origin, seed, npts)
    if key not in _CACHE:
        a, b = crop_pair(W, H, origin)
        res = O.lk(a, b, case_points(W, H, win, origin, seed, npts), win, max_level, BASE_CRIT, MIN_EIG)
        for v in res:
            v.setflags(write=False)
        _CACHE[key] = res
    return _CACHE[key]


def make_init(W, H, win, kind, origin=None, seed=0, npts=None):
    """The init sets: "identity" (the points themselves), "const" (the points plus the median flow
    of the crop's maxLevel-3 result) and "random" (the points plus uniform(-3, 3), the first 20
    far outside the image)."""
    key = ("init", W, H, tuple(win), kind, origin, seed, npts)
    if key not in _CACHE:
        pts = case_points(W, H, win, origin, seed, npts)
        if kind == "identity":
            ini = pts.copy()
        elif kind == "const":
            out, st, _ = oracle_lk(W, H, win, 3, origin, seed, npts)
            m = st == 1
            flow = np.median((out - pts)[m], axis=0).astype(F32) if m.any() else np.zeros(2, F32)
            ini = pts + flow
        elif kind == "random":
            rng = np.random.default_rng(seed + 7)
            ini = (pts + rng.uniform(-3, 3, pts.shape)).astype(F32)
            k = min(20, len(ini))
            if k:
                ini[:k] = pts[:k] + F32([4 * W, -3 * H])       # the strongest corners: tracked by the plain call
        else:
            raise ValueError(kind)
        ini = np.ascontiguousarray(ini, F32)
        ini.setflags(write=False)
        _CACHE[key] = ini
    return _CACHE[key]


def same_point(a, b):
    return np.all(a == b, axis=1)


# ------------------------------------------------------------------ py_lk is the oracle where they overlap
@pytest.mark.parametrize("max_level", LEVELS)
@pytest.mark.parametrize("win", WINDOWS, ids=lambda w: f"{w[0]}x{w[1]}")
@pytest.mark.parametrize("W,H", list(SIZES))
def test_py_lk_equals_c_oracle(W, H, win, max_level):
    pts, _, out, st, err = ref_lk(W, H, win, max_level)
    ro, rs, re = oracle_lk(W, H, win, max_level)
    assert 350 <= len(pts) <= 450
    assert int((rs == 1).sum()) >= 20 and int((rs == 0).sum()) >= 20, (int((rs == 1).sum()), int((rs == 0).sum()))
    assert np.array_equal(st, rs), np.flatnonzero(st != rs)[:8]
    assert np.array_equal(out, ro), np.flatnonzero(~same_point(out, ro))[:8]
    m = rs == 1
    assert np.array_equal(err[m], re[m]), np.flatnonzero(m & (err != re))[:8]


@pytest.mark.parametrize("max_level", LEVELS)
@pytest.mark.parametrize("win", WINDOWS, ids=lambda w: f"{w[0]}x{w[1]}")
def test_identity_init_is_the_plain_call(win, max_level):
    W, H = 160, 120
    base = ref_lk(W, H, win, max_level)
    ini = ref_lk(W, H, win, max_level, USE_INITIAL_FLOW, "identity")
    for a, b in zip(base[2:], ini[2:]):
        assert np.array_equal(a, b)


def good_tracks(W, H, win, out, st):
    """Points with status 1 that end within half a pixel of the full pyramid's (maxLevel 3) result."""
    o3, s3, _ = oracle_lk(W, H, win, 3)
    return int(((st == 1) & (s3 == 1) & (np.linalg.norm(out - o3, axis=1) < 0.5)).sum())


@pytest.mark.parametrize("win", WINDOWS, ids=lambda w: f"{w[0]}x{w[1]}")
def test_const_init_is_not_vacuous(win):
    """96x200 at maxLevel 0: the flow is about 9 px and single-level LK loses most points; starting
    from the median flow of the maxLevel-3 result recovers them.  Single-level LK loses them by
    settling on another structure with status 1, not by clearing the status: of about 285 points
    the full pyramid tracks, flags 0 ends 72 to 104 within half a pixel of the pyramid's result
    and the constant offset 270 to 281 (per window), while the status-1 counts are 292 to 301
    against 286 to 300.  So "more points end tracked" is asserted on the points that end where the
    pyramid puts them, for every window, and on the plain status count for 21x9, where it also
    holds (293 -> 300; at 15x15 it is 301 -> 293)."""
    W, H = 96, 200
    pts, _, o0, s0, _ = ref_lk(W, H, win, 0)
    _, ini, o1, s1, _ = ref_lk(W, H, win, 0, USE_INITIAL_FLOW, "const")
    assert np.abs(ini - pts).max() > 3
    differ = int((~same_point(o0, o1) | (s0 != s1)).sum())
    assert differ >= 100, differ
    g0, g1 = good_tracks(W, H, win, o0, s0), good_tracks(W, H, win, o1, s1)
    assert g1 >= 2 * g0 and g1 >= g0 + 100, (g0, g1)
    if win == (21, 9):
        assert int(s1.sum()) > int(s0.sum()), (int(s1.sum()), int(s0.sum()))


@pytest.mark.parametrize("max_level", LEVELS)
def test_random_init_is_not_vacuous(max_level):
    W, H, win = 160, 120, (15, 15)
    _, _, o0, s0, _ = ref_lk(W, H, win, max_level)
    _, _, o1, s1, _ = ref_lk(W, H, win, max_level, USE_INITIAL_FLOW, "random")
    differ = int((~same_point(o0, o1) | (s0 != s1)).sum())
    assert differ >= 100, differ
    lost = int(((s0 == 1) & (s1 == 0)).sum())
    assert lost >= 10, lost


@pytest.mark.parametrize("max_level", LEVELS)
@pytest.mark.parametrize("win", WINDOWS, ids=lambda w: f"{w[0]}x{w[1]}")
def test_min_eigenvalue_err(win, max_level):
    """Bit 8: err is the level-0 tensor's minimum eigenvalue, recomputed here on its own from the
    level-0 window; points and (with the window of every tracked point inside the image) status are
    those of the plain call."""
    from oracle import _olib as O
    W, H = 160, 120
    pts, _, o0, s0, e0 = ref_lk(W, H, win, max_level)
    _, _, o8, s8, e8 = ref_lk(W, H, win, max_level, GET_MIN_EIGENVALS)
    assert np.array_equal(o0, o8)
    # the plain call's L1 pass can only clear a status (final window outside the image)
    assert np.all(s8 >= s0)
    a, _ = crop_pair(W, H)
    ww, wh = win
    lv = _levels(a, 0, ww, wh, True)[0]
    px, py = pts[:, 0] - F32((ww - 1) * 0.5), pts[:, 1] - F32((wh - 1) * 0.5)
    fx, fy = np.floor(px), np.floor(py)
    inb = (fx >= -ww) & (fx < W) & (fy >= -wh) & (fy < H)
    ipx, ipy = fx[inb].astype(np.int64), fy[inb].astype(np.int64)
    wgt = _weights(px[inb] - ipx.astype(F32), py[inb] - ipy.astype(F32))
    d = _window(lv[3], ipx, ipy, ww, wh, ww, wh)
    Ix, Iy = _bilin(d[..., 0], wgt, 14), _bilin(d[..., 1], wgt, 14)
    S = F32(1.0 / (1 << 20))
    A11, A12, A22 = ((Ix * Ix).sum((1, 2)).astype(F32) * S, (Ix * Iy).sum((1, 2)).astype(F32) * S,
                     (Iy * Iy).sum((1, 2)).astype(F32) * S)
    want = np.zeros(len(pts), F32)
    want[inb] = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + F32(4) * A12 * A12)) / F32(2 * ww * wh)
    assert np.array_equal(e8, want)
    assert int((e8 != e0).sum()) >= 100, int((e8 != e0).sum())
    assert int(((s8 == 0) & (e8 != 0)).sum()) >= 10, int(((s8 == 0) & (e8 != 0)).sum())
