"""The definition of the reprojection-error gate on new landmarks (option tri_max_reproj_error,
vo_tri_opts): a NumPy restatement, which the kernels match bit for bit
(test_gpu_tri_gate.py), and its own properties on the CPU.

A candidate that reached cv2.triangulatePoints and passed the depth gate becomes a landmark only if
its float32 point reprojects within max_err pixels of both observations it was made from; otherwise
it is dropped: neither a landmark nor a candidate any longer.  `reproj_err2` is one view's squared
pixel error, + - * / in fp64 on NumPy scalars, one rounding per operation, written expression by
expression (no @, whose order and fused multiply-adds are not the kernels').
`triangulate_candidates_ref` is oracle.vo_pipeline_oracle.triangulate_candidates with that branch.
"""
import copy

import numpy as np
import pytest

from oracle import cv2_oracle as CV
from oracle import vo_pipeline_oracle as V

N_STEPS = 8
_CACHE = {}


# ------------------------------------------------------------------ the restatement
def project(P, X32, x32):
    """(e, p_2) of the float32 point X32 (3) in the view with the 3x4 matrix P (float64) and the
    float32 observation x32 (2)."""
    P = np.asarray(P, np.float64)
    X, Y, Z = (np.float64(v) for v in np.asarray(X32, np.float32).ravel())
    x, y = (np.float64(v) for v in np.asarray(x32, np.float32).ravel())
    with np.errstate(all="ignore"):
        p = [((P[k, 0] * X + P[k, 1] * Y) + P[k, 2] * Z) + P[k, 3] for k in range(3)]
        u = p[0] / p[2]
        v = p[1] / p[2]
        du = u - x
        dv = v - y
        e = du * du + dv * dv
    return e, p[2]


def reproj_err2(P, X32, x32):
    """The view's squared pixel error e; +inf where the projective depth p_2 is not > 0."""
    e, p2 = project(P, X32, x32)
    return e if p2 > 0 else np.float64(np.inf)


def view_passes(P, X32, x32, thr2):
    """p_2 > 0 and e <= thr2; a NaN fails either comparison."""
    e, p2 = project(P, X32, x32)
    return bool(p2 > 0) and bool(e <= thr2)


def triangulate_candidates_ref(s, R_cur_CW, t_cur_CW, max_err, trace=None):
    """oracle.vo_pipeline_oracle.triangulate_candidates (triangulate_landmarks :107-206) with the
    gate: max_err None is that function statement for statement.  Returns the four counters:
    candidates that reached cv2.triangulatePoints, kept by the depth gate, dropped by this gate,
    appended.  trace: a list that receives (i, P_past, P_cur, X) of every candidate that passed the
    depth gate."""
    thr2 = None if max_err is None else np.float64(max_err) * np.float64(max_err)
    reached = depth_kept = dropped = appended = 0
    R_cur_WC, t_cur_WC = V._inv_rigid(R_cur_CW, t_cur_CW)
    P_cur = s.K @ np.hstack((R_cur_WC, t_cur_WC))
    retain = np.zeros((s.cand.shape[0],), dtype=bool)
    n_poses = len(s.transforms)
    for i in range(s.cand.shape[0]):
        if n_poses > 1 and n_poses - s.cand_tau[i] <= s.opts['min_baseline_frames']:   # :175-178
            retain[i] = True
            continue
        R_past_CW, t_past_CW = s.transforms[int(s.cand_tau[i, 0])]
        if V._too_small_angle(s, s.cand_first[i, :], s.cand[i, :], R_past_CW, R_cur_CW):
            retain[i] = True
            continue
        R_past_WC, t_past_WC = V._inv_rigid(R_past_CW, t_past_CW)
        P_past = s.K @ np.hstack((R_past_WC, t_past_WC))
        X = CV.triangulatePoints(P_past, P_cur, s.cand_first[i].reshape(-1, 1), s.cand[i].reshape(-1, 1))
        X = X[:3] / X[3]
        reached += 1
        if V._depth_ok(s, R_cur_WC, t_cur_WC, R_past_WC, t_past_WC, X):
            if trace is not None:
                trace.append((i, P_past, P_cur, X))
            if thr2 is not None:
                assert X.dtype == np.float32 and s.cand.dtype == np.float32 and s.cand_first.dtype == np.float32
                if not (view_passes(P_past, X, s.cand_first[i], thr2) and view_passes(P_cur, X, s.cand[i], thr2)):
                    dropped += 1                                         # retain[i] stays False: removed
                    continue
            appended += 1
            if len(s.lm) == 0:
                s.lm = X.T
                s.kp = s.cand[i].reshape(1, 2)
            else:
                s.lm = np.append(s.lm, X.T, axis=0)
                s.kp = np.append(s.kp, s.cand[i].reshape(1, 2), axis=0)
        else:
            depth_kept += 1
            retain[i] = True                                             # quirk Q5
    V._keep_cands(s, retain)
    return [reached, depth_kept, dropped, appended]


# ------------------------------------------------------------------ the oracle pipeline with it
def snap(s):
    R_, t_ = s.transforms[-1]
    return dict(R=np.array(R_), t=np.array(t_), num_pts=int(s.num_pts[-1]), landmarks=np.array(s.lm),
                keypoints=np.array(s.kp), cand=np.array(s.cand), cand_first=np.array(s.cand_first),
                cand_tau=np.array(s.cand_tau))


def kitti_start():
    """The 11-frame synthetic KITTI sequence (seed 1) and the oracle's state after the bootstrap
    (0, 2); computed once.  (frames, K, opts, state)"""
    if "start" not in _CACHE:
        from monocular_visual_odometry_va4mr_amd import options as Op
        from monocular_visual_odometry_va4mr_amd.synth import make_sequence
        fr, K, _, _ = make_sequence("kitti", 11, seed=1)
        opts, boot, _ = Op.get("kitti")
        assert boot == (0, 2)
        s0 = V.new_state(K, opts)
        V.initialize(s0, fr[0], fr[2])
        _CACHE["start"] = (fr, K, opts, s0)
    return _CACHE["start"]


def run_oracle(max_err, n_steps=N_STEPS, patched=True, pnp=None, lk=None):
    """n_steps of the oracle pipeline from kitti_start() with V.triangulate_candidates replaced by
    the restatement at max_err (looked up at call time by V.step; patched=False: the oracle's own).
    pnp / lk: replacements for cv2_oracle.solvePnPRansac / calcOpticalFlowPyrLK, given the original
    as their first argument.  Returns (snapshots, counters per step, final state)."""
    fr, K, opts, s0 = kitti_start()
    s = copy.deepcopy(s0)
    snaps, counts = [], []
    keep = V.triangulate_candidates, CV.solvePnPRansac, CV.calcOpticalFlowPyrLK

    def tri(s_, R, t):
        counts.append(triangulate_candidates_ref(s_, R, t, max_err))

    if patched:
        V.triangulate_candidates = tri
    if pnp is not None:
        CV.solvePnPRansac = lambda *a, **kw: pnp(keep[1], *a, **kw)
    if lk is not None:
        CV.calcOpticalFlowPyrLK = lambda *a, **kw: lk(keep[2], *a, **kw)
    try:
        for k in range(n_steps):
            V.step(s, fr[3 + k])
            snaps.append(snap(s))
    finally:
        V.triangulate_candidates, CV.solvePnPRansac, CV.calcOpticalFlowPyrLK = keep
    return snaps, counts, s


def state_before_triangulation(step=1):
    """(state, R_CW, t_CW) the plain oracle hands to triangulate_candidates in step `step` (default:
    the second tracked frame, the first whose candidates are old enough); computed once, copy it."""
    key = ("before", step)
    if key not in _CACHE:
        fr, K, opts, s0 = kitti_start()
        s = copy.deepcopy(s0)
        got = []
        keep = V.triangulate_candidates

        def tri(s_, R, t):
            got.append((copy.deepcopy(s_), R, t))          # (the pose arrays themselves: their memory order matters)
            keep(s_, R, t)

        V.triangulate_candidates = tri
        try:
            for k in range(step + 1):
                V.step(s, fr[3 + k])
        finally:
            V.triangulate_candidates = keep
        assert len(got) == step + 1
        _CACHE[key] = got[step]
    return _CACHE[key]


def pipeline(max_err, n_steps=N_STEPS):
    key = ("pipe", max_err, n_steps)
    if key not in _CACHE:
        _CACHE[key] = run_oracle(max_err, n_steps)[:2]
    return _CACHE[key]


def plain_pipeline(n_steps=N_STEPS):
    """The unpatched oracle's snapshots."""
    key = ("plain", n_steps)
    if key not in _CACHE:
        _CACHE[key] = run_oracle(None, n_steps, patched=False)[0]
    return _CACHE[key]


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) and np.asarray(a[k]).dtype == np.asarray(b[k]).dtype for k in a)


# ------------------------------------------------------------------ tests
def test_gate_off_is_the_oracle():
    """max_err None: every array and pose of 8 steps bit-identical to the unpatched oracle, and the
    counters account for every candidate that was triangulated."""
    plain = plain_pipeline()
    snaps, counts = pipeline(None)
    assert len(snaps) == len(plain) == N_STEPS and len(counts) == N_STEPS
    for k in range(N_STEPS):
        assert _same(snaps[k], plain[k]), f"step {k}"
        m, dk, dr, ap = counts[k]
        assert dr == 0 and m == dk + ap and (ap > 0 or k == 0), counts[k]


KK = np.array([[512.0, 0, 256], [0, 512.0, 128], [0, 0, 1]])
P_A = KK @ np.hstack((np.eye(3), np.zeros((3, 1))))
P_B = KK @ np.hstack((np.eye(3), np.array([[-1.0], [0], [0]])))


def test_known_answers():
    X = np.float32([0.5, -0.25, 4.0])                  # projects exactly: (320, 96) in A, (192, 96) in B
    assert reproj_err2(P_A, X, np.float32([320, 96])) == 0.0 and reproj_err2(P_B, X, np.float32([192, 96])) == 0.0
    # the observation of view A moved by 3 px: e = 9 there, 0 in the other view, on those exact inputs
    assert reproj_err2(P_A, X, np.float32([323, 96])) == 9.0 and reproj_err2(P_A, X, np.float32([320, 93])) == 9.0
    assert reproj_err2(P_B, X, np.float32([192, 96])) == 0.0
    assert view_passes(P_A, X, np.float32([323, 96]), 9.0) and not view_passes(P_A, X, np.float32([323, 96]), np.nextafter(9.0, 0))
    # behind either camera: +inf and a failure, whatever the threshold (an overflowed one included)
    back = np.float32([0.5, -0.25, -4.0])
    for P in (P_A, P_B):
        assert reproj_err2(P, back, np.float32([320, 96])) == np.inf
        assert not view_passes(P, back, np.float32([320, 96]), 1e300) and not view_passes(P, back, np.float32([320, 96]), np.inf)
    assert reproj_err2(P_A, np.float32([0.5, -0.25, 0.0]), np.float32([320, 96])) == np.inf          # p_2 = 0
    # a NaN anywhere fails
    for Xn, xn in ((np.float32([np.nan, 0, 4]), np.float32([320, 96])), (np.float32([0.5, -0.25, np.nan]), np.float32([320, 96])),
                   (X, np.float32([np.nan, 96])), (X, np.float32([320, np.nan]))):
        assert not view_passes(P_A, Xn, xn, 1e300)
    assert not view_passes(P_A, X, np.float32([320, 96]), np.nan)


def test_agrees_with_a_plain_matrix_product():
    """1,000 random frustum points seen from random poses, the observations a few pixels off the
    projection (so that e carries no cancellation): 1e-9 relative against P @ [X; 1]."""
    from monocular_visual_odometry_va4mr_amd import options as Op  # noqa: F401  (the package imports)
    rng = np.random.default_rng(5)
    K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]])
    worst = 0.0
    for _ in range(1000):
        rv = rng.normal(size=3) * 0.1
        R = CV.Rodrigues(rv.reshape(3, 1))[0]
        t = rng.normal(size=(3, 1))
        P = K @ np.hstack((R, t))
        Xc = np.array([rng.uniform(-0.8, 0.8), rng.uniform(-0.25, 0.25), 1.0]) * rng.uniform(3, 80)   # camera frame
        X = np.float32(R.T @ (Xc.reshape(3, 1) - t)).ravel()
        h = P @ np.append(np.float64(X), 1.0)
        assert h[2] > 0
        off = rng.uniform(0.5, 5.0, 2) * rng.choice([-1, 1], 2)
        x = np.float32(h[:2] / h[2] + off)
        want = float(((h[:2] / h[2] - np.float64(x)) ** 2).sum())
        got = float(reproj_err2(P, X, x))
        worst = max(worst, abs(got - want) / want)
    assert worst < 1e-9, worst


def _drops(counts):
    return [c[2] for c in counts]


@pytest.mark.parametrize("max_err,floor", [(8.0, 5), (2.0, 20)])
def test_gate_is_at_work(max_err, floor):
    """Synthetic KITTI, seed 1, bootstrap (0, 2), 8 steps.  Step 0 triangulates nothing (its
    candidates are the bootstrap's leftovers and one frame old); in each of steps 1 to 7 the gate
    drops candidates and landmarks are still appended, and the run ends elsewhere than the plain one.
    Dropped per step, this restatement: 8 px: 21, 16, 58, 33, 13, 22, 28; 2 px: 489, 194, 97, 117,
    89, 54, 132."""
    plain = plain_pipeline()
    snaps, counts = pipeline(max_err)
    print(max_err, "counters per step:", counts)
    for k in range(1, N_STEPS):
        m, dk, dr, ap = counts[k]
        assert m == dk + dr + ap
        assert dr >= floor, (k, counts)
        assert ap > 0, (k, counts)
    assert not np.array_equal(snaps[-1]["landmarks"], plain[-1]["landmarks"])
    assert not np.array_equal(snaps[-1]["cand"], plain[-1]["cand"])
    # every appended landmark is within the gate of both of its views, by construction; and the
    # tighter gate drops more
    if max_err == 2.0:
        loose = pipeline(8.0)[1]
        assert sum(_drops(counts)) > sum(_drops(loose))


def test_dropped_candidates_are_gone():
    """One triangulation call on the state two steps in: the gated call's landmarks are the plain
    call's minus the dropped ones, in the same order, and its candidates are exactly the plain
    call's (a dropped candidate is not kept)."""
    fr, K, opts, s0 = kitti_start()
    _, _, s = run_oracle(None, 1, patched=False)
    V.track(s, fr[4])
    R, t = s.transforms[-1]
    a, b = copy.deepcopy(s), copy.deepcopy(s)
    ca = triangulate_candidates_ref(a, R, t, None)
    cb = triangulate_candidates_ref(b, R, t, 2.0)
    assert ca[0] == cb[0] and ca[1] == cb[1] and cb[2] > 0 and ca[3] == cb[2] + cb[3], (ca, cb)
    assert np.array_equal(a.cand, b.cand) and np.array_equal(a.cand_first, b.cand_first) and np.array_equal(a.cand_tau, b.cand_tau)
    n0 = len(s.lm)
    new_a, new_b = a.lm[n0:], b.lm[n0:]
    rows = {r.tobytes(): i for i, r in enumerate(new_a)}
    idx = [rows[r.tobytes()] for r in new_b]
    assert len(new_b) == cb[3] and idx == sorted(idx)
    assert np.array_equal(a.lm[:n0], b.lm[:n0]) and np.array_equal(b.kp[n0:], a.kp[n0:][idx])


def test_abi_declares_the_entry_points():
    from monocular_visual_odometry_va4mr_amd import _lib as L
    import ctypes
    for name in ("vo_triangulate_gated", "vo_pnp_gated", "vo_pnp_triangulate_gated", "vo_filter_pnp_triangulate_gated",
                 "vo_triangulate_points_err"):
        assert name in L.exported_symbols()
    assert ctypes.sizeof(L.VoTriOpts) == 16 and L.VoTriOpts.info.offset == 8


def test_option_parsing():
    from monocular_visual_odometry_va4mr_amd.engine import parse_tri_gate
    assert parse_tri_gate({}) is None and parse_tri_gate({"tri_max_reproj_error": None}) is None
    assert parse_tri_gate({"tri_max_reproj_error": 8}) == 8.0 and parse_tri_gate({"tri_max_reproj_error": np.float32(0.5)}) == 0.5
    for bad in (0, -1.0, float("nan"), float("inf"), "8", True):
        with pytest.raises(ValueError):
            parse_tri_gate({"tri_max_reproj_error": bad})
