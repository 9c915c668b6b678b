"""The LK tracker's illumination models on the GPU: vo_lk_points_illum, vo_track_illum,
cv2compat.calcOpticalFlowPyrLK(illumination=) and the engine option lk_illumination against
py_lk_illum, the NumPy restatement of test_lk_illum_ref.py (pinned there to py_lk with the model
off), bit for bit: points, status and err (err where status is 1; for every point with bit 8).

One window per k_lk instantiation (9x15 k_lk<4, false>, 21x9 k_lk<4, true>, 21x21 k_lk<16, true>)
and 15x15, which under a model runs k_lk<4, false> too (k_lk_w holds no model, so a 15x15 result
equal to the restatement's cannot have come from it).
"""
import ctypes as C

import numpy as np
import pytest

import test_lk_flags_ref as R
import test_lk_illum_ref as IR
from test_lk_illum_ref import BIAS, GAIN_BIAS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_lk_flags import SENT_ERR, SENT_PT, SENT_ST, WIN_IDS, assert_matches, make_engine, sentinels, upload   # noqa: E402
from test_gpu_lk_fb import KEYS, _import, assert_fb, check_not_vacuous, pipeline_reference   # noqa: E402

THR = 1.0
MODE_IDS = {BIAS: "bias", GAIN_BIAS: "gain_bias"}
modes = pytest.mark.parametrize("mode", [BIAS, GAIN_BIAS], ids=lambda m: MODE_IDS[m])
p_ = lambda t: C.c_void_p(t.data_ptr())


def run_illum(eng, prev, nxt, pts_per_chain, init_per_chain, flags, mode, cap, thr=0.0, null_init=False, null_back=False):
    """vo_lk_points_illum; outputs pre-filled with sentinels.  (rc, out [B, cap, 2], st, err, back)."""
    dp, di, dc = upload(eng, prev, nxt, pts_per_chain, init_per_chain, cap)
    out, st, err = sentinels(eng.B, cap)
    back = torch.full((eng.B, cap, 2), SENT_PT, device="cuda")
    rc = eng.lib.vo_lk_points_illum(eng._pd, eng._po, eng._ps, 0, p_(dp), None if null_init else p_(di), p_(dc), cap, flags,
                                    mode, C.c_double(thr), None if null_back else p_(back), p_(out), p_(st), p_(err),
                                    eng.stream)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), st.cpu().numpy(), err.cpu().numpy(), back.cpu().numpy()


def untouched(out, st, err, back):
    return bool(np.all(out == SENT_PT) and np.all(st == SENT_ST) and np.all(err == SENT_ERR) and np.all(back == SENT_PT))


# ------------------------------------------------------------------ vo_lk_points_illum
@pytest.mark.parametrize("W,H", [(160, 120), (131, 67)])
@pytest.mark.parametrize("max_level", R.LEVELS)
@pytest.mark.parametrize("win", R.WINDOWS, ids=WIN_IDS)
@modes
def test_lk_points_illum(mode, win, max_level, W, H):
    ref = IR.ref_illum(W, H, win, max_level, mode)
    plain = R.ref_lk(W, H, win, max_level)
    assert int((~R.same_point(plain[2], ref[2])).sum()) >= 100         # the model is at work
    assert int((ref[3] == 1).sum()) >= 20 and int((ref[3] == 0).sum()) >= 20
    a, b = R.crop_pair(W, H)
    eng = make_engine(W, H, win, max_level)
    rc, out, st, err, back = run_illum(eng, [a], [b], [ref[0]], None, 0, mode, 512, null_init=True, null_back=True)
    assert rc == 0
    assert_matches(out[0], st[0], err[0], ref, 0, f"{MODE_IDS[mode]} {W}x{H} win {win} maxLevel {max_level}")
    assert np.all(back == SENT_PT)


@pytest.mark.parametrize("win", [(15, 15), (21, 21)], ids=WIN_IDS)
@modes
def test_lk_points_illum_ten_chains(mode, win):
    """Both block mappings at B >= 8, counts on the edges; rows past a count stay untouched."""
    W, H, B, cap = 160, 120, 10, 320
    counts = [0, 1, cap, 37, 200, 64, 65, 319, 128, 5]
    origins = [(40 + 110 * b, 150 + 9 * b) for b in range(B)]
    refs, prev, nxt = [], [], []
    for b in range(B):
        a, c = R.crop_pair(W, H, origins[b])
        prev.append(a)
        nxt.append(c)
        refs.append(IR.ref_illum(W, H, win, 3, mode, origin=origins[b], seed=100 + b, npts=counts[b]))
    assert [len(r[0]) for r in refs] == counts
    eng = make_engine(W, H, win, 3, B=B, cap=cap)
    rc, out, st, err, _ = run_illum(eng, prev, nxt, [r[0] for r in refs], None, 0, mode, cap, null_init=True)
    assert rc == 0
    for b in range(B):
        assert_matches(out[b], st[b], err[b], refs[b], 0, f"{MODE_IDS[mode]} chain {b} ({counts[b]} points) win {win}")


FLAG_CASES = [(4, "const", 96, 200), (4, "random", 160, 120), (12, "const", 96, 200), (12, "random", 160, 120),
              (8, None, 160, 120)]


@pytest.mark.parametrize("flags,kind,W,H", FLAG_CASES, ids=[f"{c[0]}-{c[1]}" for c in FLAG_CASES])
@pytest.mark.parametrize("win", R.WINDOWS, ids=WIN_IDS)
@modes
def test_lk_points_illum_flags(mode, win, flags, kind, W, H):
    ref = IR.ref_illum(W, H, win, 3, mode, flags, kind)
    a, b = R.crop_pair(W, H)
    eng = make_engine(W, H, win, 3)
    rc, out, st, err, _ = run_illum(eng, [a], [b], [ref[0]], None if kind is None else [ref[1]], flags, mode, 512,
                                    null_init=kind is None)
    assert rc == 0
    assert_matches(out[0], st[0], err[0], ref, flags, f"{MODE_IDS[mode]} {W}x{H} win {win} flags {flags} init {kind}")
    if flags & 8:       # the compensated tensor's eigenvalue, not the plain one
        assert int((ref[4] != R.ref_lk(W, H, win, 3, flags, kind)[4]).sum()) >= 100


@pytest.mark.parametrize("flags,kind", [(0, None), (12, "random")], ids=["flags0", "flags12"])
@pytest.mark.parametrize("win", R.WINDOWS, ids=WIN_IDS)
@modes
def test_lk_points_illum_gate(mode, win, flags, kind):
    """The gate as fb_compose with py_lk_illum in both directions (the backward pass: flags 0)."""
    W, H = 160, 120
    ref = IR.ref_fb_illum(W, H, win, 3, mode, THR, flags, kind)
    check_not_vacuous([ref])
    a, b = R.crop_pair(W, H)
    eng = make_engine(W, H, win, 3)
    rc, out, st, err, back = run_illum(eng, [a], [b], [ref[0]], None if kind is None else [ref[1]], flags, mode, 512,
                                       thr=THR, null_init=kind is None)
    assert rc == 0
    assert_fb(out[0], st[0], err[0], back[0], ref, flags, f"{MODE_IDS[mode]} win {win} flags {flags}")


BAD_ARGS = {
    "illum_0": dict(mode=0),
    "illum_3": dict(mode=3),
    "illum_negative": dict(mode=-1),
    "flag_1": dict(flags=1),
    "flag_16": dict(flags=16),
    "flag_4_without_init": dict(flags=4, null_init=True),
    "negative_threshold": dict(thr=-1.0),
    "nan_threshold": dict(thr=float("nan")),
    "inf_threshold": dict(thr=float("inf")),
    "minus_inf_threshold": dict(thr=float("-inf")),
    "threshold_without_back": dict(thr=1.0, null_back=True),
    "window_too_wide": dict(win=(33, 15)),
    "window_too_wide_gated": dict(win=(33, 15), thr=1.0),
    "window_too_small": dict(win=(15, 2)),
}


@pytest.mark.parametrize("what", list(BAD_ARGS))
def test_lk_points_illum_rejects_bad_arguments(what):
    W, H, win = 160, 120, (15, 15)
    a_ = BAD_ARGS[what]
    pts = R.case_points(W, H, win)
    a, b = R.crop_pair(W, H)
    eng = make_engine(W, H, win, 3)
    keep = eng.opts.win_w, eng.opts.win_h
    eng.opts.win_w, eng.opts.win_h = a_.get("win", keep)
    try:
        rc, out, st, err, back = run_illum(eng, [a], [b], [pts], [pts], a_.get("flags", 0), a_.get("mode", BIAS), 512,
                                           thr=a_.get("thr", 0.0), null_init=a_.get("null_init", False),
                                           null_back=a_.get("null_back", False))
    finally:
        eng.opts.win_w, eng.opts.win_h = keep
    assert rc == -1
    assert untouched(out, st, err, back)


@pytest.mark.parametrize("win", [(15, 15), (21, 9), (21, 21)], ids=WIN_IDS)
@modes
def test_offset_invariance_on_the_device(mode, win):
    """next + 20 (no saturation: the crops' maximum is <= 224) gives the very points and status of
    next; err, the raw L1 mismatch, does not."""
    W, H = 160, 120
    a, b = R.crop_pair(W, H)
    assert int(b.max()) <= 224
    a2, b2 = IR.variant_pair(W, H, "plus20")
    ref, ref2 = IR.ref_illum(W, H, win, 3, mode), IR.ref_illum(W, H, win, 3, mode, variant="plus20")
    eng = make_engine(W, H, win, 3)
    rc, out, st, err, _ = run_illum(eng, [a], [b], [ref[0]], None, 0, mode, 512, null_init=True)
    rc2, out2, st2, err2, _ = run_illum(eng, [a2], [b2], [ref[0]], None, 0, mode, 512, null_init=True)
    assert rc == 0 and rc2 == 0
    assert np.array_equal(out, out2) and np.array_equal(st, st2)
    assert_matches(out2[0], st2[0], err2[0], ref2, 0, f"{MODE_IDS[mode]} win {win} next + 20")
    n = len(ref[0])
    assert int((err[0, :n] != err2[0, :n]).sum()) >= 100
    # the plain entry is not invariant
    res = []
    for x, y in ((a, b), (a2, b2)):
        dp, _, dc = upload(eng, [x], [y], [ref[0]], None, 512)
        o, s, e = sentinels(1, 512)
        assert eng.lib.vo_lk_points(eng._pd, eng._po, eng._ps, 0, p_(dp), p_(dc), 512, p_(o), p_(s), p_(e), eng.stream) == 0
        torch.cuda.synchronize()
        res.append((o.cpu().numpy()[0, :n], s.cpu().numpy()[0, :n]))
    assert int((~R.same_point(res[0][0], res[1][0]) | (res[0][1] != res[1][1])).sum()) > 100


# ------------------------------------------------------------------ cv2compat
@pytest.mark.parametrize("win", [(15, 15), (21, 21)], ids=WIN_IDS)
def test_cv2compat_illumination(win):
    from monocular_visual_odometry_va4mr_amd import cv2compat as G
    W, H = 160, 120
    a, b = R.crop_pair(W, H)
    for name, mode in IR.MODES.items():
        for flags, kind in ((0, None), (12, "random")):
            pts, ini, ro, rs, re = IR.ref_illum(W, H, win, 3, mode, flags, kind)
            p_in = pts.reshape(-1, 1, 2).copy()
            po, so, eo = G.calcOpticalFlowPyrLK(a, b, p_in, None if ini is None else ini.copy(), winSize=win, maxLevel=3,
                                                criteria=R.BASE_CRIT, flags=flags, minEigThreshold=R.MIN_EIG,
                                                illumination=name)
            assert po.shape == p_in.shape and so.shape == (len(pts), 1) and eo.shape == (len(pts), 1)
            assert np.array_equal(so.ravel(), rs) and np.array_equal(po.reshape(-1, 2), ro)
            m = np.ones(len(pts), bool) if flags & 8 else rs == 1
            assert np.array_equal(eo.ravel()[m], re[m])
    # None is today's call
    pts, _, ro, rs, re = R.ref_lk(W, H, win, 3)
    kw = dict(winSize=win, maxLevel=3, criteria=R.BASE_CRIT, minEigThreshold=R.MIN_EIG)
    base = G.calcOpticalFlowPyrLK(a, b, pts.copy(), None, **kw)
    off = G.calcOpticalFlowPyrLK(a, b, pts.copy(), None, illumination=None, **kw)
    for x, y in zip(base, off):
        assert np.array_equal(x, y)
    assert np.array_equal(base[0], ro) and np.array_equal(base[1].ravel(), rs)
    for bad in ("", "gain", 1, True, ("bias",)):
        with pytest.raises(ValueError):
            G.calcOpticalFlowPyrLK(a, b, pts.copy(), None, illumination=bad, **kw)
    with pytest.raises(TypeError):                  # keyword only: the positional parameters are cv2's
        G.calcOpticalFlowPyrLK(a, b, pts.copy(), None, win, 3, R.BASE_CRIT, 0, R.MIN_EIG, "bias")


# ------------------------------------------------------------------ vo_track_illum
@pytest.mark.parametrize("seeded,fb", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["plain", "seeded", "fb", "seeded-fb"])
@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("win", [(15, 15), (21, 21)], ids=WIN_IDS)
@modes
def test_track_illum(mode, win, compact, seeded, fb):
    """The chain state set with import_chain as in test_track_seeded: the landmarks' keypoints and
    the candidates are the case's points, the seeds the "random" init set."""
    W, H, cap, n_cand = 160, 120, 512, 150
    flags, kind = (4, "random") if seeded else (0, None)
    if fb:
        pts, ini, q, want_st, _, back, sf, _ = IR.ref_fb_illum(W, H, win, 3, mode, THR, flags, kind)
    else:
        pts, ini, q, want_st, _ = IR.ref_illum(W, H, win, 3, mode, flags, kind)
        back, sf = None, want_st
    nL = len(pts) - n_cand
    kp, cand = pts[:nL].copy(), pts[nL:].copy()
    ntrk = len(pts)
    rng = np.random.default_rng(3)
    lm = rng.normal(size=(nL, 3)).astype(np.float32)
    cfirst = rng.uniform(0, 100, (n_cand, 2)).astype(np.float32)
    ctau = np.arange(n_cand, dtype=np.float64).reshape(-1, 1)
    a, b = R.crop_pair(W, H)
    eng = make_engine(W, H, win, 3, cap=cap)
    eng.import_chain(0, landmarks=lm, keypoints=kp, cand=cand, cand_first=cfirst, cand_tau=ctau,
                     transforms=[(np.eye(3), np.zeros((3, 1)))], num_pts=[], prev_img=a)
    eng.build_pyramid(torch.from_numpy(b[None]), 1 - eng.prev)
    eng.t["trk_pts"].fill_(SENT_PT)
    eng.t["trk_st"].fill_(SENT_ST)
    eng.t["trk_err"].fill_(SENT_ERR)
    seeds = None
    if seeded:
        sd = np.full((1, 2 * cap, 2), 1e9, np.float32)             # never read past the tracked rows
        sd[0, :ntrk] = ini[:ntrk]
        seeds = torch.from_numpy(sd).cuda()
    scr = torch.full((1, 2 * cap, 2), SENT_PT, device="cuda")
    rc = eng.lib.vo_track_illum(eng._pd, eng._po, eng._ps, eng.prev, mode, None if seeds is None else p_(seeds),
                                C.c_double(THR if fb else 0.0), p_(scr) if fb else None, compact, eng.stream)
    torch.cuda.synchronize()
    assert rc == 0
    tp, ts, te = (eng.t[k][0].cpu().numpy() for k in ("trk_pts", "trk_st", "trk_err"))
    bk = scr[0].cpu().numpy()
    assert np.array_equal(ts[:ntrk], want_st[:ntrk])
    assert np.array_equal(tp[:ntrk], q[:ntrk])
    assert np.all(tp[ntrk:] == SENT_PT) and np.all(ts[ntrk:] == SENT_ST) and np.all(te == SENT_ERR)
    if fb:
        m = sf[:ntrk] == 1
        assert np.array_equal(bk[:ntrk][m], back[:ntrk][m]) and np.all(bk[ntrk:] == SENT_PT)
    else:
        assert np.all(bk == SENT_PT)
    e = eng.export_chain(0)
    gl, gc = want_st[:nL] == 1, want_st[nL:] == 1
    if compact:
        assert np.array_equal(e["keypoints"], q[:nL][gl]) and np.array_equal(e["landmarks"], lm[gl])
        assert np.array_equal(e["cand"], q[nL:][gc]) and np.array_equal(e["cand_first"], cfirst[gc])
        assert np.array_equal(e["cand_tau"], ctau[gc])
    else:
        assert np.array_equal(e["keypoints"], kp) and np.array_equal(e["landmarks"], lm) and np.array_equal(e["cand"], cand)


TRACK_BAD_ARGS = {
    "illum_0": dict(mode=0),
    "illum_3": dict(mode=3),
    "negative_threshold": dict(thr=-1.0),
    "nan_threshold": dict(thr=float("nan")),
    "inf_threshold": dict(thr=float("inf")),
    "threshold_without_scratch": dict(thr=1.0, scratch=False),
    "window_too_wide": dict(win=(33, 15), thr=1.0),
    "window_too_small": dict(win=(15, 2)),
}


@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("what", list(TRACK_BAD_ARGS))
def test_track_illum_rejects_bad_arguments(what, compact):
    W, H, cap, win = 160, 120, 512, (15, 15)
    a_ = TRACK_BAD_ARGS[what]
    pts = R.case_points(W, H, win)
    nL = len(pts) - 150
    x, y = R.crop_pair(W, H)
    eng = make_engine(W, H, win, 3, cap=cap)
    eng.import_chain(0, landmarks=np.ones((nL, 3), np.float32), keypoints=pts[:nL].copy(), cand=pts[nL:].copy(),
                     cand_first=pts[nL:].copy(), cand_tau=np.zeros((150, 1)), transforms=[(np.eye(3), np.zeros((3, 1)))],
                     num_pts=[], prev_img=x)
    eng.build_pyramid(torch.from_numpy(y[None]), 1 - eng.prev)
    eng.t["trk_pts"].fill_(SENT_PT)
    eng.t["trk_st"].fill_(SENT_ST)
    eng.t["trk_err"].fill_(SENT_ERR)
    scr = torch.full((1, 2 * cap, 2), SENT_PT, device="cuda")
    keep = eng.opts.win_w, eng.opts.win_h
    eng.opts.win_w, eng.opts.win_h = a_.get("win", keep)
    try:
        rc = eng.lib.vo_track_illum(eng._pd, eng._po, eng._ps, eng.prev, a_.get("mode", GAIN_BIAS), None,
                                    C.c_double(a_.get("thr", 0.0)), p_(scr) if a_.get("scratch", True) else None, compact,
                                    eng.stream)
    finally:
        eng.opts.win_w, eng.opts.win_h = keep
    torch.cuda.synchronize()
    assert rc == -1
    assert bool((eng.t["trk_pts"] == SENT_PT).all()) and bool((eng.t["trk_st"] == SENT_ST).all())
    assert bool((eng.t["trk_err"] == SENT_ERR).all()) and bool((scr == SENT_PT).all())
    e = eng.export_chain(0)
    assert np.array_equal(e["keypoints"], pts[:nL]) and np.array_equal(e["cand"], pts[nL:])


# ------------------------------------------------------------------ the engine
def _engine(K, opts, batch=1, **extra):
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    return Engine(K, dict(opts, **extra), 1241, 376, batch=batch, ncap=4096, pcap=8192, fcap=32)


def _state(eng):
    torch.cuda.synchronize()
    return {k: eng.t[k].cpu().numpy().copy() for k in KEYS}


@modes
def test_engine_tracks_through_the_model(mode):
    """The bootstrapped KITTI-size chain of test_gpu_lk_fb's pipeline_reference: after
    vo_track_illum(compact = 0), as the engine's step calls it, trk_pts / trk_st are py_lk_illum's
    on the state's lm_kp and c_kp."""
    fr, K, opts, s0, _ = pipeline_reference()
    eng = _engine(K, opts, lk_illumination=MODE_IDS[mode])
    assert eng.lk_illumination == MODE_IDS[mode]
    _import(eng, 0, s0)
    eng.build_pyramid(torch.from_numpy(np.ascontiguousarray(fr[3][None])), 1 - eng.prev)
    nL, nC = int(eng.t["nL"][0]), int(eng.t["nC"][0])
    assert nL >= 100 and nC >= 100
    pts = np.concatenate([eng.t["lm_kp"][0, :nL].cpu().numpy(), eng.t["c_kp"][0, :nC].cpu().numpy()])
    eng.t["trk_pts"].fill_(SENT_PT)
    eng.t["trk_st"].fill_(SENT_ST)
    assert eng.lib.vo_track_illum(eng._pd, eng._po, eng._ps, eng.prev, mode, None, C.c_double(0.0), None, 0, eng.stream) == 0
    torch.cuda.synchronize()
    win = (eng.opts.win_w, eng.opts.win_h)
    crit = (eng.opts.crit_type, eng.opts.crit_count, eng.opts.crit_eps)
    q, st, _ = IR.py_lk_illum(np.asarray(s0.prev_img), fr[3], pts, win, eng.opts.max_level, crit, eng.opts.min_eig, mode)
    plain = R.py_lk(np.asarray(s0.prev_img), fr[3], pts, win, eng.opts.max_level, crit, eng.opts.min_eig)
    assert int((~R.same_point(plain[0], q)).sum()) >= 100
    tp, ts = eng.t["trk_pts"][0].cpu().numpy(), eng.t["trk_st"][0].cpu().numpy()
    n = nL + nC
    assert np.array_equal(ts[:n], st) and np.array_equal(tp[:n], q)
    assert np.all(tp[n:] == SENT_PT) and np.all(ts[n:] == SENT_ST)
    # the engine's own step tracks the same way: its trk_pts / trk_st are these
    eng2 = _engine(K, opts, lk_illumination=MODE_IDS[mode])
    _import(eng2, 0, s0)
    eng2.step(fr[3])
    torch.cuda.synchronize()
    assert np.array_equal(eng2.t["trk_pts"][0, :n].cpu().numpy(), q) and np.array_equal(eng2.t["trk_st"][0, :n].cpu().numpy(), st)
    assert eng2.statuses()[0] == 0


FORMS = ["compact_in_track", "split", "track_stream", "graph", "prefetch"]
N_STEPS = 4


def _steps(eng, form, fr):
    frames = [torch.from_numpy(np.ascontiguousarray(fr[3 + k][None])).cuda() for k in range(N_STEPS)]
    if form == "split":
        eng.fuse_pnp_tri = False
    if form == "track_stream":
        eng.track_stream = torch.cuda.Stream()
    if form == "graph":
        eng.capture_step()
    out = []
    for k in range(N_STEPS):
        if form == "graph":
            eng.step_graph(frames[k])
        elif form == "prefetch":
            eng.step(frames[k], next_frames=frames[k + 1] if k + 1 < N_STEPS else None)
        else:
            eng.step(frames[k])
        out.append(_state(eng))
    return out


def _eager_states(mode, extra_key=()):
    key = ("eager", mode) + tuple(extra_key)
    if key not in IR._CACHE:
        fr, K, opts, s0, _ = pipeline_reference()
        eng = _engine(K, opts, lk_illumination=MODE_IDS[mode], **dict(extra_key))
        _import(eng, 0, s0)
        IR._CACHE[key] = _steps(eng, "default", fr)
    return IR._CACHE[key]


@pytest.mark.parametrize("form", FORMS)
@modes
def test_engine_step_forms_leave_the_same_state(mode, form, monkeypatch):
    monkeypatch.delenv("VO_COMPACT_IN_TRACK", raising=False)
    monkeypatch.delenv("VO_PREFETCH", raising=False)
    want = _eager_states(mode)
    assert all(int(s["status"][0]) == 0 for s in want)
    if form == "compact_in_track":
        monkeypatch.setenv("VO_COMPACT_IN_TRACK", "1")
    fr, K, opts, s0, _ = pipeline_reference()
    eng = _engine(K, opts, lk_illumination=MODE_IDS[mode])
    _import(eng, 0, s0)
    got = _steps(eng, form, fr)
    for k in range(N_STEPS):
        for name in KEYS:
            assert np.array_equal(got[k][name], want[k][name]), f"{form}: step {k}: {name}"


@pytest.mark.parametrize("form", ["default", "graph"])
@modes
def test_engine_with_gate_and_seeds_is_the_composed_calls(mode, form, monkeypatch):
    """lk_illumination with lk_fb_threshold and lk_motion_model: the step's trk_pts / trk_st are
    those of vo_predict_seeds + vo_track_illum(seeds, threshold) called by hand on an engine brought
    to the same state, and the seeds are predicted ones (third step: nF >= 3)."""
    monkeypatch.delenv("VO_COMPACT_IN_TRACK", raising=False)
    fr, K, opts, s0, _ = pipeline_reference()
    extra = dict(lk_illumination=MODE_IDS[mode], lk_fb_threshold=THR, lk_motion_model="constant_velocity")
    a, b = _engine(K, opts, **extra), _engine(K, opts, **extra)
    for e in (a, b):
        _import(e, 0, s0)
    frames = [torch.from_numpy(np.ascontiguousarray(fr[3 + k][None])).cuda() for k in range(3)]
    if form == "graph":
        a.capture_step()
    for k in range(3):
        (a.step_graph if form == "graph" else a.step)(frames[k])
    for k in range(2):
        b.step(frames[k])
    torch.cuda.synchronize()
    assert a.statuses()[0] == 0 and a.seed_info()[0, 1] > 0
    b.build_pyramid(frames[2], 1 - b.prev)
    nL, nC = int(b.t["nL"][0]), int(b.t["nC"][0])
    n = nL + (nC if nC > 1 else 0)
    sd, si, scr = b._seeds, b._seed_info, b._fb_scratch
    assert b.lib.vo_predict_seeds(b._pd, b._po, b._ps, p_(sd), p_(si), b.stream) == 0
    assert b.lib.vo_track_illum(b._pd, b._po, b._ps, b.prev, mode, p_(sd), C.c_double(THR), p_(scr), 0, b.stream) == 0
    torch.cuda.synchronize()
    assert n >= 200
    assert np.array_equal(a.t["trk_pts"][0, :n].cpu().numpy(), b.t["trk_pts"][0, :n].cpu().numpy())
    assert np.array_equal(a.t["trk_st"][0, :n].cpu().numpy(), b.t["trk_st"][0, :n].cpu().numpy())
    assert np.array_equal(a.seed_info(), si.cpu().numpy())
    # and not those of the same step without the model
    c = _engine(K, opts, lk_fb_threshold=THR, lk_motion_model="constant_velocity")
    _import(c, 0, s0)
    for k in range(3):
        c.step(frames[k])
    torch.cuda.synchronize()
    assert not np.array_equal(a.t["pose_t"].cpu().numpy(), c.t["pose_t"].cpu().numpy())


def test_engine_option_off():
    """lk_illumination absent or None is the engine as it was: the same state as an engine built
    without the key; with the option the state differs; bad values raise."""
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    fr, K, opts, s0, snaps = pipeline_reference()
    states = []
    for o in (dict(opts), dict(opts, lk_illumination=None), dict(opts, lk_illumination="bias"),
              dict(opts, lk_illumination="gain_bias")):
        eng = Engine(K, o, 1241, 376, batch=1, ncap=4096, pcap=8192, fcap=32)
        _import(eng, 0, s0)
        for k in range(3):
            eng.step(fr[3 + k])
        states.append((_state(eng), eng.lk_illumination))
    assert [s[1] for s in states] == [None, None, "bias", "gain_bias"]
    for k in KEYS:
        assert np.array_equal(states[0][0][k], states[1][0][k]), k
    for i, j in ((0, 2), (0, 3), (2, 3)):
        assert not np.array_equal(states[i][0]["pose_t"], states[j][0]["pose_t"])
    for bad in ("", "gain", "BIAS", 1, True, ("bias",)):
        with pytest.raises(ValueError):
            Engine(K, dict(opts, lk_illumination=bad), 1241, 376, batch=1, ncap=64, pcap=64, fcap=4)


def test_dropin_class_and_runners_pass_the_option_through():
    from monocular_visual_odometry_va4mr_amd import run_dataset as RD
    from monocular_visual_odometry_va4mr_amd import run_sequence as RS
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    from monocular_visual_odometry_va4mr_amd.VisualOdometryPipeLine import VisualOdometryPipeLine
    fr, K, opts, _, _ = pipeline_reference()
    n = 3
    vo = VisualOdometryPipeLine(K, dict(opts, lk_illumination="gain_bias"), max_frames=32, landmark_capacity=4096,
                                candidate_capacity=8192)
    vo.initialization(fr[0], fr[2])
    for k in range(n):
        vo.continuous_operation(fr[3 + k])
    assert vo._eng.lk_illumination == "gain_bias"
    eng = _engine(K, opts, lk_illumination="gain_bias")
    eng.bootstrap(fr[0][None], fr[2][None])
    for k in range(n):
        eng.step(fr[3 + k])
    e = eng.export_chain(0)
    assert e["status"] == 0 and len(e["transforms"]) == len(vo.transforms) == n + 2
    for (Ra, ta), (Rb, tb) in zip(e["transforms"], vo.transforms):
        assert np.array_equal(Ra, np.asarray(Rb)) and np.array_equal(ta.ravel(), np.asarray(tb).ravel())
    res = RD.run("synthetic-kitti", None, last_frame=7, plot=None, lk_illumination="bias")
    assert res["_vo"]._eng.lk_illumination == "bias" and res["frames"] == 4
    seen = []

    class Recording(Engine):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            seen.append(self.lk_illumination)

    rep = RS.run("kitti", 24, 2, overlap=4, engine_cls=Recording, lk_illumination="gain_bias")
    assert rep is not None and seen and all(v == "gain_bias" for v in seen)
