"""The level-0 L1-error pass of LK runs only where the caller gives an err buffer.

vo_track_lk and vo_track leave trk_err untouched (nothing in the step reads it) and give the C
oracle's points and statuses; vo_lk_points without an err buffer gives what it gives with one.
vo_track_fb still writes trk_err: test_gpu_lk_fb.py::test_track_fb pins that.

One engine of nine chains (the XCD block map is active from eight, the ninth chain is its second
round) on 160x120 crops, maxLevel 3; chain by chain: landmarks and candidates, one candidate (not
tracked, :286), no candidates, candidates only, nothing, a stopped chain, 2500 points on 2048
blocks (some waves carry two), and two plain ones.  15x15 runs k_lk_w, 21x21 k_lk.
"""
import ctypes as C

import numpy as np
import pytest

import test_gpu_lk_flags as G
import test_lk_flags_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

W, H, CAP, B = 160, 120, 2048, 9
# (nL, nC, status)
CHAINS = [(300, 150, 0), (300, 1, 0), (300, 0, 0), (0, 200, 0), (0, 0, 0), (100, 50, 2), (2000, 500, 0),
          (120, 80, 0), (257, 64, 0)]

_POOL = {}


def pool(win):
    """About 3,200 points of the crop (eight point sets of test_lk_flags_ref), shared read-only."""
    key = tuple(win)
    if key not in _POOL:
        p = np.concatenate([R.case_points(W, H, win, seed=s) for s in range(8)])
        p.setflags(write=False)
        _POOL[key] = p
    return _POOL[key]


def chain_points(win):
    """Per chain (landmark keypoints, candidates): the head of the chain's own fixed shuffle of the pool."""
    key = ("chains", tuple(win))
    if key not in _POOL:
        out = []
        for b, (nL, nC, _) in enumerate(CHAINS):
            p = pool(win)
            sel = np.random.default_rng(50 + b).permutation(len(p))[:nL + nC]
            out.append((p[sel[:nL]].copy(), p[sel[nL:]].copy()))
        _POOL[key] = out
    return _POOL[key]


def tracked(lm, c):
    """The list LK tracks: landmarks, then the candidates where there is more than one."""
    return np.concatenate([lm, c]) if len(c) > 1 else lm


def oracle(win):
    """The C oracle's LK per chain on the concatenated points (computed once)."""
    from oracle import _olib as O
    key = ("oracle", tuple(win))
    if key not in _POOL:
        a, b = R.crop_pair(W, H)
        res = []
        for lm, c in chain_points(win):
            pts = np.ascontiguousarray(tracked(lm, c))
            res.append(O.lk(a, b, pts, win, 3, R.BASE_CRIT, R.MIN_EIG)[:2] if len(pts) else
                       (np.zeros((0, 2), np.float32), np.zeros(0, np.uint8)))
        _POOL[key] = res
    return _POOL[key]


def load_state(eng, win):
    """The chains' lists, counts and statuses into the engine, both pyramids built, every tracking
    output set to its sentinel."""
    a, b = R.crop_pair(W, H)
    n = eng.B
    lm, c = np.zeros((n, CAP, 2), np.float32), np.zeros((n, CAP, 2), np.float32)
    for i, (l, k) in enumerate(chain_points(win)):
        lm[i, :len(l)] = l
        c[i, :len(k)] = k
    T = eng.t
    T["lm_kp"].copy_(torch.from_numpy(lm))
    T["c_kp"].copy_(torch.from_numpy(c))
    T["nL"].copy_(torch.tensor([x[0] for x in CHAINS], dtype=torch.int32))
    T["nC"].copy_(torch.tensor([x[1] for x in CHAINS], dtype=torch.int32))
    T["status"].copy_(torch.tensor([x[2] for x in CHAINS], dtype=torch.int32))
    eng.prev = 0
    eng.build_pyramid(torch.from_numpy(np.stack([a] * n)), 0)
    eng.build_pyramid(torch.from_numpy(np.stack([b] * n)), 1)
    T["trk_pts"].fill_(G.SENT_PT)
    T["trk_st"].fill_(G.SENT_ST)
    T["trk_err"].fill_(G.SENT_ERR)


@pytest.mark.parametrize("entry", ["vo_track_lk", "vo_track"])
@pytest.mark.parametrize("win", [(15, 15), (21, 21)], ids=G.WIN_IDS)
def test_track_leaves_err_alone(win, entry):
    """trk_err keeps its sentinel everywhere; trk_pts / trk_st are the oracle's for every tracked
    index and the sentinel past each chain's count and in the stopped chain."""
    eng = G.make_engine(W, H, win, 3, B=B, cap=CAP)
    load_state(eng, win)
    rc = getattr(eng.lib, entry)(eng._pd, eng._po, eng._ps, 0, eng.stream)
    torch.cuda.synchronize()
    assert rc == 0
    p, s, e = (eng.t[k].cpu().numpy() for k in ("trk_pts", "trk_st", "trk_err"))
    assert np.all(e == G.SENT_ERR)
    n_ok = n_lost = 0
    for b, ((lm, c), (nL, nC, status), (ro, rs)) in enumerate(zip(chain_points(win), CHAINS, oracle(win))):
        ntot = 0 if status else len(tracked(lm, c))
        assert np.all(p[b, ntot:] == G.SENT_PT) and np.all(s[b, ntot:] == G.SENT_ST), f"chain {b}: written past {ntot}"
        if not ntot:
            continue
        assert np.array_equal(s[b, :ntot], rs), f"chain {b}: status"
        bad = np.flatnonzero(~R.same_point(p[b, :ntot], ro))
        assert bad.size == 0, f"chain {b}: {bad.size} points differ, first {bad[:6].tolist()}"
        n_ok += int((rs == 1).sum())
        n_lost += int((rs == 0).sum())
    assert n_ok >= 1000 and n_lost >= 200       # not vacuous: both outcomes, the final-window bounds status among them


@pytest.mark.parametrize("win", [(15, 15), (21, 21)], ids=G.WIN_IDS)
def test_lk_points_null_err(win):
    """vo_lk_points without an err buffer: the same points and statuses as with one (the oracle's),
    and the buffer of the other call holds the oracle's err where the status is 1."""
    pts = R.case_points(W, H, win)
    a, b = R.crop_pair(W, H)
    eng = G.make_engine(W, H, win, 3)
    dp, _, dc = G.upload(eng, [a], [b], [pts], None, 512)
    p = lambda t: C.c_void_p(t.data_ptr())
    res = []
    for with_err in (True, False):
        out, st, err = G.sentinels(1, 512)
        rc = eng.lib.vo_lk_points(eng._pd, eng._po, eng._ps, 0, p(dp), p(dc), 512, p(out), p(st),
                                  p(err) if with_err else None, eng.stream)
        torch.cuda.synchronize()
        assert rc == 0
        res.append((out.cpu().numpy(), st.cpu().numpy(), err.cpu().numpy()))
    (po, so, eo), (pn, sn, en) = res
    assert np.array_equal(po.view(np.int32), pn.view(np.int32)) and np.array_equal(so, sn)
    assert np.all(en == G.SENT_ERR)
    ro, rs, re = R.oracle_lk(W, H, win, 3)
    n = len(pts)
    assert np.array_equal(sn[0, :n], rs) and np.all(R.same_point(pn[0, :n], ro))
    assert np.array_equal(eo[0, :n][rs == 1], re[rs == 1])
    # the status the error pass's bounds test clears (final window off level 0) is among the cases
    assert int((rs == 0).sum()) >= 20
