"""cv2's calcOpticalFlowPyrLK flags on the GPU: vo_lk_points_ex and cv2compat.calcOpticalFlowPyrLK
with OPTFLOW_USE_INITIAL_FLOW (4) and OPTFLOW_LK_GET_MIN_EIGENVALS (8) against py_lk, the NumPy
restatement of test_lk_flags_ref.py (pinned there to the C oracle where the two overlap), bit for
bit: status, points and err for every point (with bit 8 err is defined for every point; without it
where status is 1).

One window per kernel instantiation (15x15 k_lk_w, 9x15 k_lk<4, false>, 21x9 k_lk<4, true>, 21x21
k_lk<16, true>), one pyramid level and four, the constant-offset, random and identity init sets.
"""
import ctypes as C

import numpy as np
import pytest

import test_lk_flags_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT_PT, SENT_ST, SENT_ERR = -7777.0, 0xAB, -5555.0
WIN_IDS = lambda w: f"{w[0]}x{w[1]}"


_ENGINES = {}


def make_engine(W, H, win, max_level, B=1, cap=512):
    """One small engine per configuration, shared by the cases (the LK entries only read its
    pyramids, which every case rebuilds)."""
    key = (W, H, tuple(win), max_level, B, cap)
    if key not in _ENGINES:
        _ENGINES[key] = _make_engine(W, H, win, max_level, B, cap)
    return _ENGINES[key]


def _make_engine(W, H, win, max_level, B, cap):
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    from monocular_visual_odometry_va4mr_amd import options as Op
    opts, _, _ = Op.get("kitti")
    opts.update(winSize=tuple(win), maxLevel=max_level, criteria=R.BASE_CRIT)
    K = np.array([[300.0, 0, W / 2], [0, 300.0, H / 2], [0, 0, 1]])
    eng = Engine(K, opts, W, H, batch=B, ncap=cap, pcap=cap, fcap=4)
    eng.opts.min_eig = R.MIN_EIG
    return eng


def upload(eng, prev, nxt, pts_per_chain, init_per_chain, cap):
    B = eng.B
    pts = np.zeros((B, cap, 2), np.float32)
    ini = np.full((B, cap, 2), 1e9, np.float32)         # never read past a chain's count
    cnt = np.zeros(B, np.int32)
    for b, p in enumerate(pts_per_chain):
        pts[b, :len(p)] = p
        cnt[b] = len(p)
        if init_per_chain is not None:
            ini[b, :len(p)] = init_per_chain[b]
    eng.build_pyramid(torch.from_numpy(np.stack(prev)), 0)
    eng.build_pyramid(torch.from_numpy(np.stack(nxt)), 1)
    return torch.from_numpy(pts).cuda(), torch.from_numpy(ini).cuda(), torch.from_numpy(cnt).cuda()


def sentinels(B, cap):
    return (torch.full((B, cap, 2), SENT_PT, device="cuda"), torch.full((B, cap), SENT_ST, dtype=torch.uint8, device="cuda"),
            torch.full((B, cap), SENT_ERR, device="cuda"))


def run_ex(eng, prev, nxt, pts_per_chain, init_per_chain, flags, cap, null_init=False):
    """vo_lk_points_ex; outputs pre-filled with sentinels.  (rc, out [B, cap, 2], st, err)."""
    dp, di, dc = upload(eng, prev, nxt, pts_per_chain, init_per_chain, cap)
    out, st, err = sentinels(eng.B, cap)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = eng.lib.vo_lk_points_ex(eng._pd, eng._po, eng._ps, 0, p(dp), None if null_init else p(di), p(dc), cap,
                                 flags, p(out), p(st), p(err), eng.stream)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), st.cpu().numpy(), err.cpu().numpy()


def assert_matches(out, st, err, ref, flags, what):
    pts, _, ro, rs, re = ref
    n = len(pts)
    bad = np.flatnonzero(st[:n] != rs)
    assert bad.size == 0, f"{what}: status differs at {bad[:8].tolist()}"
    bad = np.flatnonzero(~R.same_point(out[:n], ro))
    assert bad.size == 0, f"{what}: {bad.size} points differ, first {bad[:8].tolist()}: got {out[bad[:3]].tolist()} want {ro[bad[:3]].tolist()}"
    m = np.ones(n, bool) if flags & R.GET_MIN_EIGENVALS else rs == 1
    bad = np.flatnonzero(m & (err[:n] != re))
    assert bad.size == 0, f"{what}: err differs at {bad[:8].tolist()}: got {err[bad[:3]].tolist()} want {re[bad[:3]].tolist()}"
    assert np.all(out[n:] == SENT_PT) and np.all(st[n:] == SENT_ST) and np.all(err[n:] == SENT_ERR), \
        f"{what}: entries past the chain's count were written"


# the crop of each init set: the constant offset on 96x200, where it matters (test_lk_flags_ref)
INIT_CASES = [("const", 96, 200), ("random", 160, 120), ("identity", 131, 67)]


@pytest.mark.parametrize("kind,W,H", INIT_CASES, ids=[c[0] for c in INIT_CASES])
@pytest.mark.parametrize("flags", [4, 12])
@pytest.mark.parametrize("max_level", R.LEVELS)
@pytest.mark.parametrize("win", R.WINDOWS, ids=WIN_IDS)
def test_lk_points_ex_initial_flow(win, max_level, flags, kind, W, H):
    ref = R.ref_lk(W, H, win, max_level, flags, kind)
    a, b = R.crop_pair(W, H)
    eng = make_engine(W, H, win, max_level)
    rc, out, st, err = run_ex(eng, [a], [b], [ref[0]], [ref[1]], flags, 512)
    assert rc == 0
    assert_matches(out[0], st[0], err[0], ref, flags, f"{W}x{H} win {win} maxLevel {max_level} flags {flags} init {kind}")


@pytest.mark.parametrize("W,H", list(R.SIZES))
@pytest.mark.parametrize("max_level", R.LEVELS)
@pytest.mark.parametrize("win", R.WINDOWS, ids=WIN_IDS)
def test_lk_points_ex_min_eigenvalues(win, max_level, W, H):
    """Bit 8 alone (init NULL), and flags 0 through the same entry (vo_lk_points itself)."""
    a, b = R.crop_pair(W, H)
    eng = make_engine(W, H, win, max_level)
    for flags in (8, 0):
        ref = R.ref_lk(W, H, win, max_level, flags)
        rc, out, st, err = run_ex(eng, [a], [b], [ref[0]], None, flags, 512, null_init=True)
        assert rc == 0
        assert_matches(out[0], st[0], err[0], ref, flags, f"{W}x{H} win {win} maxLevel {max_level} flags {flags}")


@pytest.mark.parametrize("win", [(15, 15), (21, 21)], ids=WIN_IDS)
def test_lk_points_ex_ten_chains(win):
    """Ten chains (the XCD block map with padding blocks), flags 12, counts 0, 1, the capacity and
    mixed, each chain on its own crop, points and (random) inits."""
    W, H, B, cap = 160, 120, 10, 320
    counts = [0, 1, cap, 37, 200, 64, 65, 319, 128, 5]
    origins = [(40 + 110 * b, 150 + 9 * b) for b in range(B)]
    refs, prev, nxt = [], [], []
    for b in range(B):
        a, c = R.crop_pair(W, H, origins[b])
        prev.append(a)
        nxt.append(c)
        refs.append(R.ref_lk(W, H, win, 3, 12, "random", origin=origins[b], seed=100 + b, npts=counts[b]))
        assert len(refs[b][0]) == counts[b]
    alls = np.concatenate([r[3] for r in refs])
    assert int((alls == 1).sum()) >= 100 and int((alls == 0).sum()) >= 20
    eng = make_engine(W, H, win, 3, B=B, cap=cap)
    rc, out, st, err = run_ex(eng, prev, nxt, [r[0] for r in refs], [r[1] for r in refs], 12, cap)
    assert rc == 0
    for b in range(B):
        assert_matches(out[b], st[b], err[b], refs[b], 12, f"chain {b} ({counts[b]} points) win {win}")


@pytest.mark.parametrize("flags,null_init", [(4, True), (12, True), (16, False), (4 | 16, False), (1, False)])
def test_lk_points_ex_bad_arguments(flags, null_init):
    """Bit 4 with init NULL, or any other flag bit: VO_EARG, outputs untouched."""
    W, H, win = 160, 120, (15, 15)
    pts = R.case_points(W, H, win)
    a, b = R.crop_pair(W, H)
    eng = make_engine(W, H, win, 3)
    rc, out, st, err = run_ex(eng, [a], [b], [pts], [pts], flags, 512, null_init=null_init)
    assert rc == -1
    assert np.all(out == SENT_PT) and np.all(st == SENT_ST) and np.all(err == SENT_ERR)


# ------------------------------------------------------------------ cv2compat
@pytest.mark.parametrize("flags", [4, 8, 12])
@pytest.mark.parametrize("win", [(15, 15), (21, 21)], ids=WIN_IDS)
def test_cv2compat_flags(win, flags):
    from monocular_visual_odometry_va4mr_amd import cv2compat as G
    assert G.OPTFLOW_USE_INITIAL_FLOW == 4 and G.OPTFLOW_LK_GET_MIN_EIGENVALS == 8
    W, H = 160, 120
    a, b = R.crop_pair(W, H)
    pts, ini, ro, rs, re = R.ref_lk(W, H, win, 3, flags, "random")
    p_in = pts.copy().reshape(-1, 1, 2)
    n_in = None if ini is None else ini.copy().reshape(-1, 1, 2)
    a0, b0 = a.copy(), b.copy()
    po, so, eo = G.calcOpticalFlowPyrLK(a, b, p_in, n_in, winSize=win, maxLevel=3, criteria=R.BASE_CRIT, flags=flags,
                                        minEigThreshold=R.MIN_EIG)
    assert po.shape == p_in.shape and so.shape == (len(pts), 1) and eo.shape == (len(pts), 1)
    assert np.array_equal(so.ravel(), rs)
    assert np.array_equal(po.reshape(-1, 2), ro)
    m = np.ones(len(pts), bool) if flags & 8 else rs == 1
    assert np.array_equal(eo.ravel()[m], re[m])
    assert np.array_equal(p_in.reshape(-1, 2), pts) and np.array_equal(a, a0) and np.array_equal(b, b0)
    if n_in is not None:
        assert np.array_equal(n_in.reshape(-1, 2), ini)


def test_cv2compat_next_pts_without_the_flag_is_ignored():
    """nextPts given with flags 0 (OpenCV's output buffer): the oracle's plain call, nextPts
    unchanged."""
    from monocular_visual_odometry_va4mr_amd import cv2compat as G
    from oracle import cv2_oracle as O
    W, H, win = 160, 120, (21, 21)
    a, b = R.crop_pair(W, H)
    pts = R.case_points(W, H, win).copy().reshape(-1, 1, 2)
    nxt = R.make_init(W, H, win, "random").copy().reshape(-1, 1, 2)
    keep = nxt.copy()
    po, so, eo = O.calcOpticalFlowPyrLK(a, b, pts, None)
    for flags in (0, 8):
        pg, sg, eg = G.calcOpticalFlowPyrLK(a, b, pts, nxt, flags=flags)
        assert np.array_equal(pg, po)
        assert np.array_equal(nxt, keep)
        if flags == 0:
            assert np.array_equal(sg, so)
            m = so.ravel() == 1
            assert np.array_equal(eg.ravel()[m], eo.ravel()[m])


def test_cv2compat_rejects_bad_initial_flow():
    from monocular_visual_odometry_va4mr_amd import cv2compat as G
    W, H, win = 160, 120, (15, 15)
    a, b = R.crop_pair(W, H)
    pts = R.case_points(W, H, win).copy().reshape(-1, 1, 2)
    with pytest.raises(G.error):
        G.calcOpticalFlowPyrLK(a, b, pts, None, winSize=win, flags=4)
    with pytest.raises(G.error):
        G.calcOpticalFlowPyrLK(a, b, pts, pts[:-1].copy(), winSize=win, flags=4)
    with pytest.raises(G.error):
        G.calcOpticalFlowPyrLK(a, b, pts, pts.astype(np.float64), winSize=win, flags=12)
    with pytest.raises(NotImplementedError):
        G.calcOpticalFlowPyrLK(a, b, pts, None, winSize=win, flags=16)
