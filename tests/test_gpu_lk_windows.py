"""Lucas-Kanade beyond the presets' one configuration: every window class of launch_lk, the
option handling of fill_lk and the chain / block mapping, against the oracle's
calcOpticalFlowPyrLK restatement (oracle._olib.lk) bit for bit: status, points, and err where
status is 1.

launch_lk sends 15x15 to k_lk_w and everything else to k_lk, by pixel count first: more than 256
pixels (17x17 is the first square one) to k_lk<16, true>; at most 256 pixels to k_lk<4, true> when
a side exceeds the pyramid's materialised 16-pixel border (21x9, 8x32) and to k_lk<4, false>
otherwise.  WINDOWS names the kernel of each window tested.  A point is accepted while its window's
corner ipx = floor(x - (win_w - 1) / 2) is >= -win_w and < cols (likewise in y), so a window wider
than the border reaches past it; there the taps take the reflect-101 value of the interior and a
zero derivative, as the oracle's (and OpenCV's) winSize-wide pyramid border holds.

Inputs are crops of two synthetic KITTI frames: 160x120 (W + 2 * VO_BORDER = 192 is exactly the
row pitch: no slack bytes after a row), 131x67 and 96x200.  About 600 points per case: GFTT
corners of the crop, uniform points over the image plus a window-wide margin, corners with
1e-3-scale sub-pixel offsets (the bilinear weight iw11 = 2^14 - iw00 - iw01 - iw10 goes negative
there), and points on the four acceptance edges ipx in {-win_w - 1, -win_w, cols - 1, cols}
(likewise y) at integer, quarter and half sub-pixel positions.  Every case first checks, on the
oracle's output alone, that it is not vacuous (enough tracked, enough rejected, and for wide
windows enough tracked points whose window reaches past the 16-pixel border).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BORDER = 16                                   # VO_BORDER (asserted against the library's in _engine)
SIZES = {(160, 120): (430, 170), (131, 67): (700, 215), (96, 200): (250, 120)}   # (W, H): crop origin (x, y)
# kernel per window (launch_lk tests the pixel count first): k_lk<4, false> for 3x3 .. 16x16 (256 pixels,
# both sides <= 16); k_lk<4, true> for 21x9 and 8x32 (a side > 16, at most 256 pixels; 8x32 is exactly
# 256); k_lk<16, true> for 17x17 (289 pixels), 9x31 (279), 21x21, 31x31 and 32x32 (1024, the cap)
WINDOWS = [(3, 3), (5, 5), (9, 15), (15, 9), (16, 16), (21, 9), (8, 32), (17, 17), (21, 21), (9, 31), (31, 31),
           (32, 32)]
CRITERIA = [(3, 0, 0.01), (3, 1, 0.01), (3, 100, 0.0), (3, 500, 1e-16), (3, 30, 50.0), (1, 7, 123.0), (2, 0, 0.03)]
BASE_CRIT = (3, 30, 0.01)
SENT_PT, SENT_ST, SENT_ERR = -7777.0, 0xAB, -5555.0


# ------------------------------------------------------------------ inputs (CPU only)
_FRAMES = {}


def _frames():
    if "fr" not in _FRAMES:
        from monocular_visual_odometry_va4mr_amd.synth import make_sequence
        _FRAMES["fr"] = make_sequence("kitti", 2, seed=1)[0]
    return _FRAMES["fr"]


def crop_pair(W, H, origin=None):
    """The (W, H) crop of frames 0 and 1 at `origin` (default: the size's own)."""
    x0, y0 = SIZES[(W, H)] if origin is None else origin
    fr = _frames()
    return (np.ascontiguousarray(fr[0][y0:y0 + H, x0:x0 + W]), np.ascontiguousarray(fr[1][y0:y0 + H, x0:x0 + W]))


def make_points(img, win, seed, n_uniform=180, n_corners=200, n_tiny=60, n_band=100):
    """~600 float32 points for one crop and window (see the module docstring)."""
    from oracle import _olib as O
    H, W = img.shape
    ww, wh = win
    rng = np.random.default_rng(seed)
    corners = O.gftt(img, n_corners, 0.01, 4, 3)
    uni = np.c_[rng.uniform(-ww - 2, W + ww + 2, n_uniform), rng.uniform(-wh - 2, H + wh + 2, n_uniform)]
    k = min(n_tiny, len(corners))
    tiny = corners[:k] + np.float32([[1e-3, 2e-3]]) * rng.integers(1, 8, (k, 2))
    hx, hy = (ww - 1) * 0.5, (wh - 1) * 0.5
    edge = []
    for f in (0.0, 0.25, 0.5):
        for ip in (-ww - 1, -ww, W - 1, W):          # ipx on the edge, y anywhere the window is accepted
            for _ in range(3):
                edge.append((ip + hx + f, rng.uniform(-wh + hy, H - 1 + hy)))
        for ip in (-wh - 1, -wh, H - 1, H):
            for _ in range(3):
                edge.append((rng.uniform(-ww + hx, W - 1 + hx), ip + hy + f))
    # both coordinates on an edge (window corners)
    for ipx in (-ww, W - 1):
        for ipy in (-wh, H - 1):
            edge.append((ipx + hx + 0.5, ipy + hy + 0.5))
    # the outermost accepted band on each side, at the corners' other coordinate (textured rows
    # and columns, so that some of these track): for a side > 16 exactly the positions whose
    # window reaches past the 16-pixel border, ipx in [-win_w, -17] and [cols + 16 - win_w, cols - 1]
    band = []
    dx = ww - BORDER if ww > BORDER else max(1, ww // 4)
    dy = wh - BORDER if wh > BORDER else max(1, wh // 4)
    for i in range(n_band):
        cx, cy = corners[i % len(corners)] if len(corners) else (W / 2, H / 2)
        side = (i // 2) % 2
        # one side only above the border (21x9, 8x32, 9x31): the whole band on that axis
        on_x = i % 2 == 0 if (ww > BORDER) == (wh > BORDER) else ww > BORDER
        if on_x:
            ip = rng.integers(-ww, -ww + dx) if side == 0 else rng.integers(W - dx, W)
            band.append((ip + hx + rng.uniform(0.05, 0.95), cy))
        else:
            ip = rng.integers(-wh, -wh + dy) if side == 0 else rng.integers(H - dy, H)
            band.append((cx, ip + hy + rng.uniform(0.05, 0.95)))
    pts = np.concatenate([corners, uni, tiny, np.array(edge), np.array(band)]).astype(np.float32)
    return np.ascontiguousarray(pts)


def deep_mask(pts, win, W, H):
    """Points whose level-0 window (taps ipx .. ipx + win_w, bilinear neighbour included) reaches
    more than VO_BORDER pixels outside the image."""
    ww, wh = win
    ipx = np.floor(pts[:, 0] - np.float32((ww - 1) * 0.5)).astype(np.int64)
    ipy = np.floor(pts[:, 1] - np.float32((wh - 1) * 0.5)).astype(np.int64)
    return (ipx < -BORDER) | (ipx + ww > W - 1 + BORDER) | (ipy < -BORDER) | (ipy + wh > H - 1 + BORDER)


_REF = {}


def oracle_lk(W, H, win, max_level, criteria=BASE_CRIT, min_eig=1e-4, origin=None, seed=0, npts=None):
    """(pts, out, status, err) of the oracle for one case; computed once and shared."""
    from oracle import _olib as O
    key = (W, H, tuple(win), max_level, tuple(criteria), min_eig, origin, seed, npts)
    if key not in _REF:
        a, b = crop_pair(W, H, origin)
        pts = make_points(a, win, seed)
        if npts is not None:
            pts = np.ascontiguousarray(pts[np.random.default_rng(seed).permutation(len(pts))[:npts]])
        ro, rs, re = O.lk(a, b, pts, tuple(win), max_level, tuple(criteria), min_eig)
        for v in (pts, ro, rs, re):
            v.setflags(write=False)
        _REF[key] = (pts, ro, rs, re)
    return _REF[key]


def check_not_vacuous(pts, rs, win, W, H):
    assert int((rs == 1).sum()) >= 100, f"only {int((rs == 1).sum())} tracked points"
    assert int((rs == 0).sum()) >= 20, f"only {int((rs == 0).sum())} rejected points"
    if max(win) > BORDER:
        dm = deep_mask(pts, win, W, H)
        deep = int((dm & (rs == 1)).sum())
        if max(win) == BORDER + 1:
            # A 17-pixel side reaches past the border only at ipx = -17 or ipx = cols - 1, where the
            # window holds one interior column (x = 0 or x = cols - 1).  The reflect-101 Scharr
            # dx is exactly 0 in those columns (likewise dy in rows 0 and rows - 1), so A11 = A12 = 0,
            # the minimum eigenvalue is 0 and no such point can end with status 1.  The strongest
            # condition that can hold: enough such points pass the bounds test (their windows
            # are gathered, and their status 0 and points are compared), and none is tracked.
            ww, wh = win
            ipx = np.floor(pts[:, 0] - np.float32((ww - 1) * 0.5))
            ipy = np.floor(pts[:, 1] - np.float32((wh - 1) * 0.5))
            acc = (ipx >= -ww) & (ipx < W) & (ipy >= -wh) & (ipy < H)
            assert deep == 0 and int((dm & acc).sum()) >= 10, (deep, int((dm & acc).sum()))
        else:
            assert deep >= 10, f"only {deep} tracked points with a window past the {BORDER}-pixel border"


# ------------------------------------------------------------------ GPU side
def _engine(W, H, win, max_level, criteria=BASE_CRIT, B=1, cap=1024):
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    from monocular_visual_odometry_va4mr_amd import options as Op
    from monocular_visual_odometry_va4mr_amd import _lib as L
    assert L.VO_BORDER == BORDER
    opts, _, _ = Op.get("kitti")
    opts.update(winSize=tuple(win), maxLevel=max_level, criteria=tuple(criteria))
    K = np.array([[300.0, 0, W / 2], [0, 300.0, H / 2], [0, 0, 1]])
    return Engine(K, opts, W, H, batch=B, ncap=cap, pcap=cap, fcap=4)


def run_lk(eng, prev, nxt, pts_per_chain, cap):
    """vo_lk_points on chains' own frames and points; outputs pre-filled with sentinels.
    Returns (rc, out [B, cap, 2], st [B, cap], err [B, cap])."""
    B = eng.B
    pts = np.zeros((B, cap, 2), np.float32)
    cnt = np.zeros(B, np.int32)
    for b, p in enumerate(pts_per_chain):
        pts[b, :len(p)] = p
        cnt[b] = len(p)
    eng.build_pyramid(torch.from_numpy(np.stack(prev)), 0)
    eng.build_pyramid(torch.from_numpy(np.stack(nxt)), 1)
    dp, dc = torch.from_numpy(pts).cuda(), torch.from_numpy(cnt).cuda()
    out = torch.full((B, cap, 2), SENT_PT, device="cuda")
    st = torch.full((B, cap), SENT_ST, dtype=torch.uint8, device="cuda")
    err = torch.full((B, cap), SENT_ERR, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = eng.lib.vo_lk_points(eng._pd, eng._po, eng._ps, 0, p(dp), p(dc), cap, p(out), p(st), p(err), eng.stream)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), st.cpu().numpy(), err.cpu().numpy()


def assert_matches(out, st, err, ref, what):
    pts, ro, rs, re = ref
    n = len(pts)
    bad_s = np.flatnonzero(st[:n] != rs)
    assert bad_s.size == 0, f"{what}: status differs at {bad_s[:8].tolist()} (points {pts[bad_s[:4]].tolist()})"
    bad_p = np.flatnonzero(~np.all(out[:n] == ro, axis=1))
    assert bad_p.size == 0, (f"{what}: {bad_p.size} points differ, first {bad_p[:8].tolist()}: in {pts[bad_p[:3]].tolist()} "
                             f"got {out[bad_p[:3]].tolist()} want {ro[bad_p[:3]].tolist()}")
    m = rs == 1
    bad_e = np.flatnonzero(m & (err[:n] != re))
    assert bad_e.size == 0, f"{what}: err differs at {bad_e[:8].tolist()}"
    assert np.all(out[n:] == SENT_PT) and np.all(st[n:] == SENT_ST) and np.all(err[n:] == SENT_ERR), \
        f"{what}: entries past the chain's count were written"


def run_case(W, H, win, max_level, criteria=BASE_CRIT, min_eig=1e-4, vacuity=True):
    ref = oracle_lk(W, H, win, max_level, criteria, min_eig)
    if vacuity:
        check_not_vacuous(ref[0], ref[2], win, W, H)
    a, b = crop_pair(W, H)
    eng = _engine(W, H, win, max_level, criteria)
    eng.opts.min_eig = min_eig
    rc, out, st, err = run_lk(eng, [a], [b], [ref[0]], 1024)
    assert rc == 0
    assert_matches(out[0], st[0], err[0], ref, f"{W}x{H} win {win} maxLevel {max_level} criteria {criteria} min_eig {min_eig}")


# ------------------------------------------------------------------ cases
@pytest.mark.parametrize("max_level", [0, 3])
@pytest.mark.parametrize("win", WINDOWS, ids=lambda w: f"{w[0]}x{w[1]}")
@pytest.mark.parametrize("W,H", list(SIZES))
def test_lk_window_bitexact(W, H, win, max_level):
    """k_lk<4, false> (3x3 .. 16x16: 256 pixels, half-integer hx), k_lk<4, true> (21x9 and 8x32: a
    side above the border and at most 256 pixels), k_lk<16, true> (17x17, 9x31, 21x21, 31x31,
    32x32: more than 256 pixels, up to the cap of 1024), one level and the full pyramid."""
    run_case(W, H, win, max_level)


def test_cv2compat_lk_defaults():
    """cv2compat.calcOpticalFlowPyrLK with every default (21x21, maxLevel 3, (3, 30, 0.01), 1e-4)
    against the oracle's function of the same name."""
    from monocular_visual_odometry_va4mr_amd import cv2compat as G
    from oracle import cv2_oracle as R
    W, H = 160, 120
    a, b = crop_pair(W, H)
    pts = oracle_lk(W, H, (21, 21), 3)[0].copy().reshape(-1, 1, 2)       # the shared array is read-only
    po, so, eo = R.calcOpticalFlowPyrLK(a, b, pts, None)
    check_not_vacuous(pts.reshape(-1, 2), so.ravel(), (21, 21), W, H)
    pg, sg, eg = G.calcOpticalFlowPyrLK(a, b, pts, None)
    assert pg.shape == po.shape and sg.shape == so.shape and eg.shape == eo.shape
    assert np.array_equal(sg, so)
    assert np.array_equal(pg, po)
    m = so.ravel() == 1
    assert np.array_equal(eg.ravel()[m], eo.ravel()[m])


@pytest.mark.parametrize("win", [(2, 5), (33, 32)], ids=lambda w: f"{w[0]}x{w[1]}")
def test_lk_rejects_unsupported_window(win):
    """Windows outside 3..32 per side: VO_EARG before any launch, outputs untouched."""
    W, H = 160, 120
    a, b = crop_pair(W, H)
    pts = oracle_lk(W, H, (15, 15), 0)[0]
    eng = _engine(W, H, win, 0)
    rc, out, st, err = run_lk(eng, [a], [b], [pts], 1024)
    assert rc == -1                                                     # VO_EARG
    assert np.all(out == SENT_PT) and np.all(st == SENT_ST) and np.all(err == SENT_ERR)


@pytest.mark.parametrize("criteria", CRITERIA, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]:g}")
@pytest.mark.parametrize("win", [(15, 15), (21, 21)], ids=lambda w: f"{w[0]}x{w[1]}")
def test_lk_criteria(win, criteria):
    """fill_lk's criteria normalisation on k_lk_w and k_lk<16>: no iteration at all, one, the count
    clamp (500 -> 100) with eps^2 below 2^-100 (k_lk_w's f32 convergence gates disabled), eps 0,
    the eps clamp (50 -> 10), a missing EPS bit (0.01) and a missing COUNT bit (30)."""
    run_case(160, 120, win, 3, criteria)


@pytest.mark.parametrize("win", [(15, 15), (21, 21)], ids=lambda w: f"{w[0]}x{w[1]}")
def test_lk_criteria_cases_are_distinct(win):
    """The criteria cases are not one case seven times: the oracle's outputs differ between every
    two of them (except eps 0 against eps 1e-16 at 100 iterations, and one iteration against
    eps 10, which may agree), and each clamped / defaulted triple equals its normalised form."""
    res = {c: oracle_lk(160, 120, win, 3, c) for c in CRITERIA + [BASE_CRIT]}
    # (3, 30, 50.0): eps 10 ends every point's loop after its first update, as a count of 1 does.
    # No step here exceeds 10 pixels, so this case cannot tell a missing clamp (eps 50) from the
    # clamp to 10: it pins the clamped path bit for bit, not the clamp's value.
    same_ok = {frozenset([(3, 100, 0.0), (3, 500, 1e-16)]), frozenset([(3, 1, 0.01), (3, 30, 50.0)])}
    keys = list(res)
    for i, c in enumerate(keys):
        for d in keys[i + 1:]:
            if frozenset([c, d]) in same_ok:
                continue
            assert not (np.array_equal(res[c][1], res[d][1]) and np.array_equal(res[c][2], res[d][2])), (c, d)
    for raw, norm in [((3, 500, 1e-16), (3, 100, 1e-16)), ((3, 30, 50.0), (3, 30, 10.0)),
                      ((1, 7, 123.0), (3, 7, 0.01)), ((2, 0, 0.03), (3, 30, 0.03))]:
        n = oracle_lk(160, 120, win, 3, norm)
        assert np.array_equal(res[raw][1], n[1]) and np.array_equal(res[raw][2], n[2]), (raw, norm)


@pytest.mark.parametrize("min_eig", [1e-4, 5e-3])
@pytest.mark.parametrize("win", [(15, 15), (21, 21)], ids=lambda w: f"{w[0]}x{w[1]}")
def test_lk_min_eig(win, min_eig):
    """vo_opts.min_eig (cv2's minEigThreshold), set on the engine's options after construction."""
    lo = oracle_lk(160, 120, win, 3, BASE_CRIT, 1e-4)
    hi = oracle_lk(160, 120, win, 3, BASE_CRIT, 5e-3)
    assert not np.array_equal(lo[2], hi[2]), "min_eig 5e-3 rejects no point that 1e-4 keeps"
    run_case(160, 120, win, 3, BASE_CRIT, min_eig)


@pytest.mark.parametrize("max_level", [0, 1, 2, 5])
@pytest.mark.parametrize("win", [(15, 15), (21, 21)], ids=lambda w: f"{w[0]}x{w[1]}")
def test_lk_max_level(win, max_level):
    """maxLevel 0, 1, 2 and 5; the pyramid stops where the next level is no larger than the window
    (pyr_max_level), which clips 5."""
    from monocular_visual_odometry_va4mr_amd.engine import pyr_max_level
    from oracle import _olib as O
    assert pyr_max_level(160, 120, win, 5) < 5
    assert pyr_max_level(160, 120, win, max_level) == O.pyr_maxlevel(160, 120, win, max_level)
    run_case(160, 120, win, max_level)


@pytest.mark.parametrize("win", [(15, 15), (21, 21)], ids=lambda w: f"{w[0]}x{w[1]}")
def test_lk_chain_mapping(win):
    """Ten chains: B >= 8 and not a multiple of 8 takes the XCD block map with padding blocks
    (blocks of chains 10..15 must do nothing).  Per-chain counts 0, 1, the capacity and mixed,
    each chain on its own crop pair and points; entries at or beyond a chain's count keep their
    sentinel."""
    W, H, B, cap = 160, 120, 10, 320
    counts = [0, 1, cap, 37, 200, 64, 65, 319, 128, 5]
    origins = [(40 + 110 * b, 150 + 9 * b) for b in range(B)]
    refs, prev, nxt = [], [], []
    for b in range(B):
        a, c = crop_pair(W, H, origins[b])
        prev.append(a)
        nxt.append(c)
        refs.append(oracle_lk(W, H, win, 3, origin=origins[b], seed=100 + b, npts=counts[b]))
        assert len(refs[b][0]) == counts[b]
    allp = np.concatenate([r[0] for r in refs])
    alls = np.concatenate([r[2] for r in refs])
    check_not_vacuous(allp, alls, win, W, H)
    eng = _engine(W, H, win, 3, B=B, cap=cap)
    rc, out, st, err = run_lk(eng, prev, nxt, [r[0] for r in refs], cap)
    assert rc == 0
    for b in range(B):
        assert_matches(out[b], st[b], err[b], refs[b], f"chain {b} ({counts[b]} points) win {win}")
