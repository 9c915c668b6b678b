"""The forward-backward gate on the GPU: vo_lk_points_fb, vo_track_fb and the engine option
lk_fb_threshold against the composition the project defines it as (test_lk_flags_ref.fb_compose):

    (q, st_f, err_f) = LK(prev -> next, p)          the C oracle; py_lk where flags are set
    (p', st_b, _)    = LK(next -> prev, q)          the C oracle, flags 0, only where st_f == 1
    keep iff st_f and st_b and (double)dx * dx + (double)dy * dy <= thr^2, dx = p'.x - p.x (float)

bit for bit: the gate status, q and err_f for every point, p' where st_f == 1.  The pipeline tests
run oracle.vo_pipeline_oracle with its calcOpticalFlowPyrLK replaced by that composition and
compare every pose, point count, landmark and candidate array of an Engine with
lk_fb_threshold = 1.0, in each of its step forms.
"""
import ctypes as C

import numpy as np
import pytest

import test_lk_flags_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_lk_flags import SENT_ERR, SENT_PT, SENT_ST, WIN_IDS, make_engine, sentinels, upload   # noqa: E402

THR = 1.0
_CACHE = {}
KEYS = ("status", "nL", "nC", "nF", "lm_X", "lm_kp", "c_kp", "c_first", "c_tau", "pose_R", "pose_t", "num_pts", "nInl")


def ref_fb(W, H, win, max_level, thr=THR, flags=0, init_kind=None, origin=None, seed=0, npts=None):
    """(pts, init, q, gate, err_f, back, st_f, st_b) of the composition; computed once, shared."""
    key = (W, H, tuple(win), max_level, thr, flags, init_kind, origin, seed, npts)
    if key not in _CACHE:
        a, b = R.crop_pair(W, H, origin)
        pts = R.case_points(W, H, win, origin, seed, npts)
        fwd = R.oracle_lk(W, H, win, max_level, origin, seed, npts) if flags == 0 else \
            R.ref_lk(W, H, win, max_level, flags, init_kind, origin, seed, npts)[2:]
        init = R.make_init(W, H, win, init_kind, origin, seed, npts) if flags & 4 else None
        res = R.fb_compose(a, b, pts, win, max_level, R.BASE_CRIT, R.MIN_EIG, thr, forward=fwd)
        for v in res:
            v.setflags(write=False)
        _CACHE[key] = (pts, init) + res
    return _CACHE[key]


def check_not_vacuous(refs):
    gate = np.concatenate([r[3] for r in refs])
    sf = np.concatenate([r[6] for r in refs])
    sb = np.concatenate([r[7] for r in refs])
    kept, rej, by_sb = int(gate.sum()), int(((sf == 1) & (gate == 0)).sum()), int(((sf == 1) & (sb == 0)).sum())
    assert kept >= 50 and rej >= 20 and by_sb >= 2, (kept, rej, by_sb)


def run_fb(eng, prev, nxt, pts_per_chain, init_per_chain, flags, thr, cap):
    """vo_lk_points_fb; outputs pre-filled with sentinels.  (rc, out, st, err, back)."""
    dp, di, dc = upload(eng, prev, nxt, pts_per_chain, init_per_chain, cap)
    out, st, err = sentinels(eng.B, cap)
    back = torch.full((eng.B, cap, 2), SENT_PT, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = eng.lib.vo_lk_points_fb(eng._pd, eng._po, eng._ps, 0, p(dp), p(di) if flags & 4 else None, p(dc), cap, flags,
                                 C.c_double(thr), p(back), p(out), p(st), p(err), eng.stream)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), st.cpu().numpy(), err.cpu().numpy(), back.cpu().numpy()


def assert_fb(out, st, err, back, ref, flags, what):
    pts, _, q, gate, ef, rb, sf, sb = ref
    n = len(pts)
    bad = np.flatnonzero(st[:n] != gate)
    assert bad.size == 0, f"{what}: gate differs at {bad[:8].tolist()} (st_f {sf[bad[:8]].tolist()} st_b {sb[bad[:8]].tolist()})"
    bad = np.flatnonzero(~R.same_point(out[:n], q))
    assert bad.size == 0, f"{what}: forward points differ at {bad[:8].tolist()}"
    m = np.ones(n, bool) if flags & 8 else sf == 1
    bad = np.flatnonzero(m & (err[:n] != ef))
    assert bad.size == 0, f"{what}: err differs at {bad[:8].tolist()}"
    m = sf == 1
    bad = np.flatnonzero(m & ~R.same_point(back[:n], rb))
    assert bad.size == 0, f"{what}: backward points differ at {bad[:8].tolist()}: got {back[bad[:3]].tolist()} want {rb[bad[:3]].tolist()}"
    assert np.all(out[n:] == SENT_PT) and np.all(st[n:] == SENT_ST) and np.all(err[n:] == SENT_ERR) and \
        np.all(back[n:] == SENT_PT), f"{what}: entries past the chain's count were written"


# ------------------------------------------------------------------ vo_lk_points_fb
@pytest.mark.parametrize("W,H", [(160, 120), (96, 200)])
@pytest.mark.parametrize("max_level", R.LEVELS)
@pytest.mark.parametrize("win", R.WINDOWS, ids=WIN_IDS)
def test_lk_points_fb(win, max_level, W, H):
    ref = ref_fb(W, H, win, max_level)
    check_not_vacuous([ref])
    a, b = R.crop_pair(W, H)
    eng = make_engine(W, H, win, max_level)
    rc, out, st, err, back = run_fb(eng, [a], [b], [ref[0]], None, 0, THR, 512)
    assert rc == 0
    assert_fb(out[0], st[0], err[0], back[0], ref, 0, f"{W}x{H} win {win} maxLevel {max_level}")


@pytest.mark.parametrize("win", R.WINDOWS, ids=WIN_IDS)
def test_lk_points_fb_with_flags(win):
    """The forward pass with an initial flow and the min-eigenvalue err (py_lk), gated."""
    W, H = 160, 120
    ref = ref_fb(W, H, win, 3, flags=12, init_kind="random")
    check_not_vacuous([ref])
    a, b = R.crop_pair(W, H)
    eng = make_engine(W, H, win, 3)
    rc, out, st, err, back = run_fb(eng, [a], [b], [ref[0]], [ref[1]], 12, THR, 512)
    assert rc == 0
    assert_fb(out[0], st[0], err[0], back[0], ref, 12, f"win {win} flags 12")


@pytest.mark.parametrize("win", [(15, 15), (21, 21)], ids=WIN_IDS)
def test_lk_points_fb_ten_chains(win):
    W, H, B, cap = 160, 120, 10, 320
    counts = [0, 1, cap, 37, 200, 64, 65, 319, 128, 5]
    origins = [(40 + 110 * b, 150 + 9 * b) for b in range(B)]
    refs, prev, nxt = [], [], []
    for b in range(B):
        a, c = R.crop_pair(W, H, origins[b])
        prev.append(a)
        nxt.append(c)
        refs.append(ref_fb(W, H, win, 3, origin=origins[b], seed=100 + b, npts=counts[b]))
    check_not_vacuous(refs)
    eng = make_engine(W, H, win, 3, B=B, cap=cap)
    rc, out, st, err, back = run_fb(eng, prev, nxt, [r[0] for r in refs], None, 0, THR, cap)
    assert rc == 0
    for b in range(B):
        assert_fb(out[b], st[b], err[b], back[b], refs[b], 0, f"chain {b} ({counts[b]} points) win {win}")


@pytest.mark.parametrize("win", [(15, 15), (21, 21)], ids=WIN_IDS)
def test_fb_threshold_changes_the_kept_set(win):
    W, H = 160, 120
    r1, r5 = ref_fb(W, H, win, 3, 1.0), ref_fb(W, H, win, 3, 0.5)
    assert int(r5[3].sum()) + 10 <= int(r1[3].sum()) and np.all(r5[3] <= r1[3])
    a, b = R.crop_pair(W, H)
    eng = make_engine(W, H, win, 3)
    rc, out, st, err, back = run_fb(eng, [a], [b], [r5[0]], None, 0, 0.5, 512)
    assert rc == 0
    assert_fb(out[0], st[0], err[0], back[0], r5, 0, f"win {win} threshold 0.5")


@pytest.mark.parametrize("thr", [0.0, -1.0, float("nan"), float("inf"), float("-inf")])
def test_fb_rejects_bad_threshold(thr):
    W, H, win = 160, 120, (15, 15)
    pts = R.case_points(W, H, win)
    a, b = R.crop_pair(W, H)
    eng = make_engine(W, H, win, 3)
    rc, out, st, err, back = run_fb(eng, [a], [b], [pts], None, 0, thr, 512)
    assert rc == -1
    assert np.all(out == SENT_PT) and np.all(st == SENT_ST) and np.all(err == SENT_ERR) and np.all(back == SENT_PT)
    scr = torch.zeros((1, 1024, 2), device="cuda")
    for compact in (0, 1):
        assert eng.lib.vo_track_fb(eng._pd, eng._po, eng._ps, 0, C.c_double(thr), C.c_void_p(scr.data_ptr()), compact,
                                   eng.stream) == -1
    assert eng.lib.vo_track_fb(eng._pd, eng._po, eng._ps, 0, C.c_double(1.0), None, 0, eng.stream) == -1


# ------------------------------------------------------------------ vo_track_fb
@pytest.mark.parametrize("n_cand", [150, 1], ids=["cands", "one-cand"])
@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("win", [(15, 15), (21, 21)], ids=WIN_IDS)
def test_track_fb(win, compact, n_cand):
    """The chain state set with import_chain: landmarks' keypoints and candidates are the case's
    points.  A candidate segment of exactly one is neither tracked nor filtered (:286)."""
    W, H, cap = 160, 120, 512
    ref = ref_fb(W, H, win, 3)
    pts, _, q, gate, ef, rb, sf, sb = ref
    check_not_vacuous([ref])
    nL = len(pts) - 150
    kp, cand = pts[:nL].copy(), pts[nL:nL + n_cand].copy()     # (the shared points are read-only)
    ntrk = nL + (n_cand if n_cand > 1 else 0)
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
    scr = torch.full((1, 2 * cap, 2), SENT_PT, device="cuda")
    rc = eng.lib.vo_track_fb(eng._pd, eng._po, eng._ps, eng.prev, C.c_double(THR), C.c_void_p(scr.data_ptr()), compact,
                             eng.stream)
    torch.cuda.synchronize()
    assert rc == 0
    tp, ts, te = (eng.t[k][0].cpu().numpy() for k in ("trk_pts", "trk_st", "trk_err"))
    bk = scr[0].cpu().numpy()
    assert np.array_equal(ts[:ntrk], gate[:ntrk])
    assert np.array_equal(tp[:ntrk], q[:ntrk])
    m = sf[:ntrk] == 1
    assert np.array_equal(te[:ntrk][m], ef[:ntrk][m])
    assert np.array_equal(bk[:ntrk][m], rb[:ntrk][m])
    assert np.all(tp[ntrk:] == SENT_PT) and np.all(ts[ntrk:] == SENT_ST) and np.all(te[ntrk:] == SENT_ERR) and \
        np.all(bk[ntrk:] == SENT_PT)
    e = eng.export_chain(0)
    gl = gate[:nL] == 1
    if compact:
        assert np.array_equal(e["keypoints"], q[:nL][gl]) and np.array_equal(e["landmarks"], lm[gl])
        if n_cand > 1:
            gc = gate[nL:nL + n_cand] == 1
            assert np.array_equal(e["cand"], q[nL:nL + n_cand][gc]) and np.array_equal(e["cand_first"], cfirst[gc])
            assert np.array_equal(e["cand_tau"], ctau[gc])
        else:
            assert np.array_equal(e["cand"], cand) and np.array_equal(e["cand_first"], cfirst)
    else:
        assert np.array_equal(e["keypoints"], kp) and np.array_equal(e["landmarks"], lm) and np.array_equal(e["cand"], cand)


# ------------------------------------------------------------------ the pipeline
N_STEPS = 8


def _snap_oracle(s):
    R_, t_ = s.transforms[-1]
    return dict(R=np.array(R_), t=np.array(t_), num_pts=int(s.num_pts[-1]), landmarks=np.array(s.lm),
                keypoints=np.array(s.kp), cand=np.array(s.cand), cand_first=np.array(s.cand_first),
                cand_tau=np.array(s.cand_tau))


def pipeline_reference():
    """The oracle pipeline on the synthetic KITTI sequence (bootstrap (0, 2), 8 steps) with
    calcOpticalFlowPyrLK replaced by the composition at threshold 1.0; also the ungated run's
    poses.  Computed once.  Returns (frames, K, opts, initial state, per-step snapshots)."""
    if "pipe" in _CACHE:
        return _CACHE["pipe"]
    import copy
    from oracle import cv2_oracle as CV
    from oracle import vo_pipeline_oracle as V
    from monocular_visual_odometry_va4mr_amd import options as Op
    from monocular_visual_odometry_va4mr_amd.synth import make_sequence
    fr, K, _, _ = make_sequence("kitti", 11, seed=1)
    opts, boot, _ = Op.get("kitti")
    assert boot == (0, 2)
    s0 = V.new_state(K, opts)
    V.initialize(s0, fr[0], fr[2])
    rejected = []

    def gated(prevImg, nextImg, prevPts, nextPts, winSize=(21, 21), maxLevel=3, criteria=(3, 30, 0.01), flags=0,
              minEigThreshold=1e-4):
        p = np.asarray(prevPts)
        assert flags == 0 and nextPts is None and p.dtype == np.float32
        q, gate, ef, _, sf, _ = R.fb_compose(prevImg, nextImg, p.reshape(-1, 2), tuple(winSize), int(maxLevel),
                                             tuple(criteria), float(minEigThreshold), THR)
        rejected.append(int(((sf == 1) & (gate == 0)).sum()))
        return q.reshape(p.shape), gate.reshape(-1, 1), ef.reshape(-1, 1)

    plain = copy.deepcopy(s0)
    plain_t = []
    for k in range(N_STEPS):
        V.step(plain, fr[3 + k])
        plain_t.append(np.array(plain.transforms[-1][1]))
    s = copy.deepcopy(s0)
    snaps = []
    keep = CV.calcOpticalFlowPyrLK
    CV.calcOpticalFlowPyrLK = gated          # the pipeline looks it up as cv.calcOpticalFlowPyrLK at call time
    try:
        for k in range(N_STEPS):
            V.step(s, fr[3 + k])
            snaps.append(_snap_oracle(s))
    finally:
        CV.calcOpticalFlowPyrLK = keep
    # the gate is at work in every LK call, and it changes the trajectory
    assert len(rejected) == 2 * N_STEPS and min(rejected) >= 7, rejected
    dt = [float(np.abs(snaps[k]["t"] - plain_t[k]).max()) for k in range(N_STEPS)]
    # (max |dt| against the ungated run: 0.09 after the first step, rising to 0.43 after the eighth)
    assert all(d > 0 for d in dt[1:]), dt
    assert 0.05 < dt[0] < dt[-1] and dt[-1] > 0.4 and all(b > a for a, b in zip(dt, dt[1:])), dt
    _CACHE["pipe"] = (fr, K, opts, s0, snaps)
    return _CACHE["pipe"]


def _import(eng, b, s0):
    eng.import_chain(b, landmarks=s0.lm, keypoints=s0.kp, cand=s0.cand, cand_first=s0.cand_first, cand_tau=s0.cand_tau,
                     transforms=s0.transforms, num_pts=s0.num_pts, prev_img=s0.prev_img)


def _assert_chain(eng, b, snap, what):
    e = eng.export_chain(b)
    assert e["status"] == 0, what
    R_g, t_g = e["transforms"][-1]
    assert np.array_equal(R_g, snap["R"]) and np.array_equal(t_g, snap["t"]), f"{what}: pose"
    assert e["num_pts"][-1] == snap["num_pts"], f"{what}: num_pts"
    for name in ("landmarks", "keypoints", "cand", "cand_first", "cand_tau"):
        assert np.array_equal(e[name], snap[name]), f"{what}: {name}"


FORMS = ["default", "compact_in_track", "split", "track_stream", "graph", "prefetch"]


@pytest.mark.parametrize("form", FORMS)
def test_engine_fb_pipeline_single_chain(form, monkeypatch):
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    fr, K, opts, s0, snaps = pipeline_reference()
    if form == "compact_in_track":
        monkeypatch.setenv("VO_COMPACT_IN_TRACK", "1")
    else:
        monkeypatch.delenv("VO_COMPACT_IN_TRACK", raising=False)
    monkeypatch.delenv("VO_PREFETCH", raising=False)
    o = dict(opts, lk_fb_threshold=THR)
    eng = Engine(K, o, 1241, 376, batch=1, ncap=4096, pcap=8192, fcap=32)
    assert eng._fb_scratch is not None and tuple(eng._fb_scratch.shape) == (1, 4096 + 8192, 2)
    if form == "split":
        eng.fuse_pnp_tri = False
    if form == "track_stream":
        eng.track_stream = torch.cuda.Stream()
    _import(eng, 0, s0)
    frames = [torch.from_numpy(np.ascontiguousarray(fr[3 + k][None])).cuda() for k in range(N_STEPS)]
    if form == "graph":
        eng.capture_step()
    for k in range(N_STEPS):
        if form == "graph":
            eng.step_graph(frames[k])
        elif form == "prefetch":
            eng.step(frames[k], next_frames=frames[k + 1] if k + 1 < N_STEPS else None)
        else:
            eng.step(frames[k])
        _assert_chain(eng, 0, snaps[k], f"{form}: step {k}")


@pytest.mark.parametrize("form", ["default", "graph"])
def test_engine_fb_pipeline_batch(form):
    """Chain 0 of a 3-chain batch (starts 0, 1, 3 over 14 frames, 7 steps); the other chains run
    their own sequences and must end with status 0."""
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    from monocular_visual_odometry_va4mr_amd.synth import make_sequence
    fr11, K, opts, s0, snaps = pipeline_reference()
    fr = make_sequence("kitti", 14, seed=1)[0]
    assert np.array_equal(fr[:11], fr11)
    frames = torch.from_numpy(np.ascontiguousarray(fr)).cuda()
    starts = [0, 1, 3]
    eng = Engine(K, dict(opts, lk_fb_threshold=THR), 1241, 376, batch=3, ncap=4096, pcap=8192, fcap=32)
    eng.bootstrap(frames[starts], frames[[s + 2 for s in starts]])
    _import(eng, 0, s0)                       # chain 0 from the reference's own initial state
    if form == "graph":
        eng.capture_step()
    for k in range(7):
        f = frames[[s + 3 + k for s in starts]]
        if form == "graph":
            eng.step_graph(f)
        else:
            eng.step(f)
        _assert_chain(eng, 0, snaps[k], f"{form}: step {k}")
    assert (eng.statuses() == 0).all()


def test_engine_fb_option_off():
    """lk_fb_threshold = None is an engine without the key: no scratch, the same state."""
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    fr, K, opts, s0, snaps = pipeline_reference()
    states = []
    for o in (dict(opts), dict(opts, lk_fb_threshold=None), dict(opts, lk_fb_threshold=THR)):
        eng = Engine(K, o, 1241, 376, batch=1, ncap=4096, pcap=8192, fcap=32)
        _import(eng, 0, s0)
        for k in range(3):
            eng.step(fr[3 + k])
        torch.cuda.synchronize()
        states.append(({k: eng.t[k].cpu().numpy().copy() for k in KEYS}, eng._fb_scratch))
    assert states[0][1] is None and states[1][1] is None and states[2][1] is not None
    for k in KEYS:
        assert np.array_equal(states[0][0][k], states[1][0][k]), k
    assert not np.array_equal(states[0][0]["pose_t"], states[2][0]["pose_t"])
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            Engine(K, dict(opts, lk_fb_threshold=bad), 1241, 376, batch=1, ncap=64, pcap=64, fcap=4)


def test_dropin_class_and_runner_pass_the_option_through():
    """VisualOdometryPipeLine hands its options dict to the engine unchanged: with lk_fb_threshold
    it gives the poses of an Engine stepped with the same option from the same bootstrap, and not
    those of the ungated class; run_dataset's lk_fb_threshold (--lk-fb-threshold) reaches it."""
    from monocular_visual_odometry_va4mr_amd import run_dataset as RD
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    from monocular_visual_odometry_va4mr_amd.VisualOdometryPipeLine import VisualOdometryPipeLine
    fr, K, opts, _, _ = pipeline_reference()
    n = 5

    def drop_in(o):
        vo = VisualOdometryPipeLine(K, o, max_frames=32, landmark_capacity=4096, candidate_capacity=8192)
        vo.initialization(fr[0], fr[2])
        for k in range(n):
            vo.continuous_operation(fr[3 + k])
        return vo

    gated, plain = drop_in(dict(opts, lk_fb_threshold=THR)), drop_in(dict(opts))
    assert gated._eng.lk_fb_threshold == THR and plain._eng.lk_fb_threshold is None
    eng = Engine(K, dict(opts, lk_fb_threshold=THR), 1241, 376, batch=1, ncap=4096, pcap=8192, fcap=32)
    eng.bootstrap(fr[0][None], fr[2][None])
    for k in range(n):
        eng.step(fr[3 + k])
    e = eng.export_chain(0)
    assert e["status"] == 0 and len(e["transforms"]) == len(gated.transforms) == n + 2
    for (Ra, ta), (Rb, tb) in zip(e["transforms"], gated.transforms):
        assert np.array_equal(Ra, np.asarray(Rb)) and np.array_equal(ta.ravel(), np.asarray(tb).ravel())
    assert not np.array_equal(np.asarray(gated.transforms[-1][1]), np.asarray(plain.transforms[-1][1]))
    res = RD.run("synthetic-kitti", None, last_frame=7, plot=None, lk_fb_threshold=THR)
    assert res["_vo"]._eng.lk_fb_threshold == THR and res["frames"] == 4
