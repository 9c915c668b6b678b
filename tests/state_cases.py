"""The designed step: chain states whose post-tracking, post-PnP and post-triangulation counts and
keep / drop patterns are chosen, not found, for the step's ordered compactions and appends
(track_compact_block, pnp_apply_block, pnp_apply_split, tri_gate / tri_solve / tri_append).

test_state_cases_ref.py (CPU) asserts on the oracle alone that every design does what its table row
says; test_gpu_state_edges.py imports the designs as the chains of one engine, runs every launch
form of the step's state machinery and compares each chain bit for bit with the composition of
oracle calls below.  Nothing here needs a GPU, and everything is computed once per process.

How a design is made controllable:
  poses      the oracle's own parking_c1 state after four steps (six poses: 0 and 1 C-ordered, the
             later ones F-ordered, both summation orders of pose_inverse / depth_of).  No pose is
             ever hand-made: the bit pattern of a projection matrix depends on how the pipeline
             produced each array.
  tracking   LK's result for a point does not depend on the other points: one oracle LK call over a
             pool (jittered corners, uniform points, points off the image) from the state's frame
             to the next one; points are then picked by their status.
  PnP mask   an inlier's 3-D point is its tracked position back-projected at a random depth under
             the oracle's own pose for the next frame, an outlier's comes from a pixel 40-80 px
             away; solvePnPRansac then returns the designed mask.
  candidates only cand_first and tau are free.  F: tau in {4, 5} (frame-gated); S: cand_first on
             check_baseline's own rotated ray (small angle); A: a world point at the scene's depth
             projected into pose tau (appended); D: an A with the parallax reversed or a point
             beyond max_dist_landmarks (triangulated, kept by the depth gate, quirk Q5); G: an A
             whose cand_first is moved 20 px off the epipolar line (appended without the gate,
             dropped with max_reproj_error = 2).  Every pool candidate is classified with the
             oracle's own functions and used only where it came out as intended.
"""
import copy

import numpy as np

F32 = np.float32
IMG_W, IMG_H = 640, 480
NCAP, PCAP, FCAP = 1024, 4096, 16
MAX_ERR = 2.0                     # the gated forms' max_reproj_error
SENT_F32 = F32(-7777.25)          # what the state arrays are pre-filled with
SENT_I32 = -99
ISENT = -77                       # ... and the info rows
STOP_STATUS = 2                   # VO_ST_PNP_FAILED, preset on the stopped chain
N_CORNERS, N_UNIFORM, N_OFF = 5400, 200, 400
N_LM_POOL = 620                   # tracked pool points set aside for landmark slots
_CACHE = {}


def _V():
    from oracle import vo_pipeline_oracle as V
    return V


# ====================================================================== the base state
def base():
    """parking_c1 on the oracle after four steps (geom_cases.chain_base()'s S2 stepped twice more:
    six poses), the next frame, and the oracle's own pose for that frame (the PnP target)."""
    if "base" not in _CACHE:
        import geom_cases as GC
        V = _V()
        b = GC.chain_base()
        s = copy.deepcopy(b["S"][2])
        for k in range(2):
            V.step(s, b["fr"][b["next"] + k])
        nxt = b["fr"][b["next"] + 2]
        t = copy.deepcopy(s)
        V.step(t, nxt)
        assert len(s.transforms) == 6 and s.prev_img.shape == (IMG_H, IMG_W)
        _CACHE["base"] = dict(s=s, next_img=nxt, target=t.transforms[-1], stepped=t, opts=b["opts"], K=b["K"])
    return _CACHE["base"]


def _lk(prev, nxt, pts, o):
    from oracle import cv2_oracle as cv
    q, st, _ = cv.calcOpticalFlowPyrLK(prev, nxt, pts, None, winSize=o['winSize'], maxLevel=o['maxLevel'],
                                       criteria=o['criteria'])
    return q, (st == 1).ravel()


# ====================================================================== the pool
def classify(s, R_cur_CW, t_cur_CW, max_err=MAX_ERR):
    """The class letter of every candidate of s (tracked already) under the current pose, by the
    oracle's own functions in the order of triangulate_candidates: F frame-gated, S small angle, D
    kept by the depth gate, G within the depths but off its observations by more than max_err in
    a view, A appended in either form."""
    from oracle import cv2_oracle as CV
    import test_tri_gate_ref as TG
    V = _V()
    thr2 = np.float64(max_err) * np.float64(max_err)
    R_cur_WC, t_cur_WC = V._inv_rigid(R_cur_CW, t_cur_CW)
    P_cur = s.K @ np.hstack((R_cur_WC, t_cur_WC))
    n_poses = len(s.transforms)
    out = []
    for i in range(s.cand.shape[0]):
        if n_poses > 1 and n_poses - s.cand_tau[i] <= s.opts['min_baseline_frames']:
            out.append("F")
            continue
        R_past_CW, t_past_CW = s.transforms[int(s.cand_tau[i, 0])]
        if V._too_small_angle(s, s.cand_first[i, :], s.cand[i, :], R_past_CW, R_cur_CW):
            out.append("S")
            continue
        R_past_WC, t_past_WC = V._inv_rigid(R_past_CW, t_past_CW)
        P_past = s.K @ np.hstack((R_past_WC, t_past_WC))
        X = CV.triangulatePoints(P_past, P_cur, s.cand_first[i].reshape(-1, 1), s.cand[i].reshape(-1, 1))
        X = X[:3] / X[3]
        if not V._depth_ok(s, R_cur_WC, t_cur_WC, R_past_WC, t_past_WC, X):
            out.append("D")
        elif TG.view_passes(P_past, X, s.cand_first[i], thr2) and TG.view_passes(P_cur, X, s.cand[i], thr2):
            out.append("A")
        else:
            out.append("G")
    return np.array(out, dtype="U1")


def _design_first(s, target, cur, want, tau, rng):
    """cand_first [n][2] (float64) for candidates at the tracked positions cur [n][2] that should
    come out in class want[i] with past pose tau[i], under the current pose `target`."""
    V = _V()
    Rc, tc = target
    n = len(cur)
    ray = (s.K_inv @ np.c_[cur.astype(np.float64), np.ones(n)].T).T             # camera-frame rays
    first = np.zeros((n, 2))
    for i in range(n):
        c = cur[i].astype(np.float64)
        if want[i] == "F":
            first[i] = c + rng.uniform(-30, 30, 2)
            continue
        Rp, tp = s.transforms[int(tau[i])]
        if want[i] == "S":
            u = s.K @ (Rc.T @ Rp @ ray[i])
            first[i] = u[:2] / u[2] + rng.uniform(-3, 3, 2)
            continue
        Rpw, tpw = V._inv_rigid(Rp, tp)
        far = want[i] == "D" and rng.random() < 0.2
        depth = rng.uniform(60, 200) if far else rng.uniform(1.6, 2.8)
        Xw = Rc @ (depth * ray[i]).reshape(3, 1) + tc
        a = s.K @ (Rpw @ Xw + tpw)
        a = (a[:2] / a[2]).ravel()
        inf = s.K @ (Rpw @ (Rc @ ray[i].reshape(3, 1)))                           # the ray's vanishing point in the past view
        inf = (inf[:2] / inf[2]).ravel()
        par = a - inf
        if want[i] == "A" or far:
            first[i] = a
        elif want[i] == "D":
            first[i] = inf - par                                                # the parallax reversed
        else:
            d = par / max(np.linalg.norm(par), 1e-9)
            first[i] = a + 20.0 * rng.choice([-1.0, 1.0]) * np.array([-d[1], d[0]])
    return first


def _state_with(s, lm, kp, cand, first, tau):
    c = copy.deepcopy(s)
    c.lm = np.ascontiguousarray(lm, F32).reshape(-1, 3)
    c.kp = np.ascontiguousarray(kp, F32).reshape(-1, 2)
    c.cand = np.ascontiguousarray(cand, F32).reshape(-1, 2)
    c.cand_first = np.ascontiguousarray(first, F32).reshape(-1, 2)
    c.cand_tau = np.asarray(tau, np.float64).reshape(-1, 1)
    c.cand_desc = np.zeros((len(c.cand), 0), F32)
    return c


def pool():
    """dict(pts [n][2] f32 positions in the state's frame, q their oracle-tracked positions, ok the
    oracle's status, lm: tracked indices for landmark slots, lost: indices with status 0, first /
    tau: the candidate design of every other tracked index, by: class letter -> the indices whose
    oracle class under the target pose is the intended one, yield_: class -> (designed, kept))."""
    if "pool" in _CACHE:
        return _CACHE["pool"]
    from oracle import cv2_oracle as cv
    b = base()
    s, o = b["s"], b["opts"]
    rng = np.random.default_rng(20240607)
    corners = cv.goodFeaturesToTrack(s.prev_img, maxCorners=0, qualityLevel=0.001, minDistance=3, blockSize=3,
                                     useHarrisDetector=False).reshape(-1, 2)
    corners = corners[:N_CORNERS] + rng.uniform(-0.4, 0.4, (N_CORNERS, 2))            # the strongest ones
    uniform = rng.uniform([8, 8], [IMG_W - 8, IMG_H - 8], (N_UNIFORM, 2))
    # off the image on every side, 20 to 200 px out
    t = rng.uniform(0, 1, N_OFF)
    out = rng.uniform(20, 200, N_OFF)
    side = rng.integers(0, 4, N_OFF)
    off = np.c_[np.where(side == 0, -out, np.where(side == 1, IMG_W + out, t * IMG_W)),
                np.where(side == 2, -out, np.where(side == 3, IMG_H + out, t * IMG_H))]
    pts = np.vstack([corners, uniform, off]).astype(F32)
    q, ok = _lk(s.prev_img, b["next_img"], pts, o)
    # distinct rows only: neither two pool points nor two tracked positions may coincide
    seen, seen_q, uniq = set(), set(), np.zeros(len(pts), bool)
    for i in range(len(pts)):
        kp_, kq = pts[i].tobytes(), q[i].tobytes()
        if kp_ not in seen and (not ok[i] or kq not in seen_q):
            uniq[i] = True
            seen.add(kp_)
            if ok[i]:
                seen_q.add(kq)
    trk = np.flatnonzero(ok & uniq)
    lost = np.flatnonzero(~ok & uniq)
    trk = trk[rng.permutation(len(trk))]
    lm, cidx = trk[:N_LM_POOL], trk[N_LM_POOL:]
    want = rng.choice(list("FSADG"), len(cidx), p=[0.06, 0.07, 0.16, 0.56, 0.15])
    tau = np.where(want == "F", rng.integers(4, 6, len(cidx)), rng.integers(0, 4, len(cidx)))
    first = _design_first(s, b["target"], q[cidx], want, tau, rng).astype(F32)
    cls = classify(_state_with(s, np.zeros((0, 3)), np.zeros((0, 2)), q[cidx], first, tau), *b["target"])
    full_first = np.zeros((len(pts), 2), F32)
    full_tau = np.zeros(len(pts), np.int64)
    full_first[cidx], full_tau[cidx] = first, tau
    by = {c: cidx[(cls == c) & (want == c)] for c in "FSADG"}
    # the lost points' (never read after tracking) first positions and frames
    full_first[lost] = pts[lost] + rng.uniform(-30, 30, (len(lost), 2)).astype(F32)
    full_tau[lost] = rng.integers(0, 6, len(lost))
    _CACHE["pool"] = dict(pts=pts, q=q, ok=ok, lm=lm, lost=lost, first=full_first, tau=full_tau, by=by,
                          yield_={c: (int((want == c).sum()), len(by[c])) for c in "FSADG"})
    return _CACHE["pool"]


# ====================================================================== the table
def _pat(n, kind, rng):
    """bool [n] patterns by name"""
    m = np.zeros(n, bool)
    if kind == "all":
        m[:] = True
    elif kind == "alternating":
        m[::2] = True
    elif kind == "random":
        m = rng.random(n) < 0.7
    return m


def table():
    """name -> dict(L0, lm_lost [L0] bool, mask [L1] bool (True = inlier), C0, c_lost [C0] bool,
    classes [C1] of "FSADG" (C0 = 1: the class of the untracked candidate), stopped).  The builder
    fixes it; the reference test asserts its conditions on the oracle's results."""
    if "table" in _CACHE:
        return _CACHE["table"]
    rng = np.random.default_rng(11)
    T = {}

    def row(name, L0, lm_lost, mask, C0, c_lost, classes, stopped=False):
        lm_lost, c_lost = np.asarray(lm_lost, bool), np.asarray(c_lost, bool)
        assert len(lm_lost) == L0 and len(mask) == L0 - lm_lost.sum() and len(c_lost) == C0
        assert len(classes) == (C0 - c_lost.sum() if C0 > 1 else C0)
        T[name] = dict(L0=L0, lm_lost=lm_lost, mask=np.asarray(mask, bool), C0=C0, c_lost=c_lost,
                       classes=np.array(list(classes), dtype="U1"), stopped=stopped)

    def lost_at(n, idx):
        m = np.zeros(n, bool)
        m[list(idx)] = True
        return m

    none = lambda n: np.zeros(n, bool)
    # 9 -> 8 landmarks (the PnP guard's minimum), all inliers, no candidate
    row("l9_c0", 9, lost_at(9, [3]), _pat(8, "all", rng), 0, none(0), "")
    # 64 landmarks, alternating mask; one candidate: untouched and untriangulated (Q7, :366)
    row("l64_c1", 64, none(64), _pat(64, "alternating", rng), 1, none(1), "A")
    # 65 landmarks, the only outlier is the last one (alone in its 64-lane sub-chunk); two candidates, one lost
    row("l65_c2", 65, none(65), ~lost_at(65, [64]), 2, lost_at(2, [0]), "A")
    # 256 landmarks: sub-chunk 1 without an inlier, sub-chunk 2 only inliers, 0 and 3 mixed; 255 candidates, all appended
    m = _pat(256, "random", rng)
    m[64:128], m[128:192] = False, True
    m[[0, 1, 62, 200]], m[[2, 63, 201, 255]] = True, False
    row("l256_c255_allA", 256, none(256), m, 255, none(255), "A" * 255)
    # 257 landmarks of which only the last is lost; the only outlier at lane 63; 256 candidates, none reaches triangulatePoints
    row("l257_c256_FS", 257, lost_at(257, [256]), ~lost_at(256, [63]), 256, none(256),
        "".join(rng.choice(list("FS"), 256)))
    # 257 landmarks, none lost, random mask with the lone 257th an inlier; 258 candidates, the last lost;
    # of the 257 left only the last is appended
    m = _pat(257, "random", rng)
    m[256] = True
    row("l257_c257_lastA", 257, none(257), m, 258, lost_at(258, [257]), "".join(rng.choice(list("FSD"), 256)) + "A")
    # 513 landmarks, the whole first 256-pass lost; of the 257 left the lone last one an outlier; 808 candidates, the
    # whole first pass lost: a pass of A, a pass of retained ones, a partial pass of G
    m = _pat(257, "random", rng)
    m[256] = False
    row("l513_c552_AretG", 513, lost_at(513, range(256)), m, 808, lost_at(808, range(256)),
        "A" * 256 + "".join(rng.choice(list("FSD"), 256)) + "G" * 40)
    # 600 landmarks: a whole 256-pass of outliers, then inliers; 1026 candidates, every other one lost: 513, a
    # random mix of the five classes
    mix = list("FSADG") * 45 + list(rng.choice(list("FSADG"), 513 - 225))
    mix = "".join(np.array(mix)[rng.permutation(513)])
    row("l600_c513_mix", 600, none(600), ~lost_at(600, range(256)), 1026, ~_pat(1026, "alternating", rng), mix)
    # more than 2048 candidates reach triangulatePoints: pass 2's stride wraps (second round of 8 x 256, tenth of 256)
    long_ = "".join(np.array(list("A" * 430 + "G" * 380 + "D" * 1500))[rng.permutation(2310)])
    row("l64_c2310_long", 64, none(64), _pat(64, "all", rng), 2310, none(2310), long_)
    # the random mix again, with a status set before the step
    T["stopped"] = dict(T["l600_c513_mix"], stopped=True)
    _CACHE["table"] = T
    return T


NAMES = ("l9_c0", "l64_c1", "l65_c2", "l256_c255_allA", "l257_c256_FS", "l257_c257_lastA", "l513_c552_AretG",
         "l600_c513_mix", "l64_c2310_long", "stopped")
STOPPED = NAMES.index("stopped")


# ====================================================================== building and composing
def _build_state(name, row):
    """The oracle state of a design before tracking."""
    b, p = base(), pool()
    s, (Rt, tt) = b["s"], b["target"]
    rng = np.random.default_rng(sum(map(ord, name)))
    L0, C0 = row["L0"], row["C0"]
    # landmarks: pool points by status; 3-D points from the tracked positions and the mask
    lm_idx = np.zeros(L0, np.int64)
    lm_idx[row["lm_lost"]] = p["lost"][rng.permutation(len(p["lost"]))[:row["lm_lost"].sum()]]
    kept = p["lm"][rng.permutation(len(p["lm"]))[:L0 - row["lm_lost"].sum()]]
    lm_idx[~row["lm_lost"]] = kept
    X = rng.uniform([-3, -2, 1], [3, 2, 4], (L0, 3))                      # the lost ones: anywhere
    xq = p["q"][kept].astype(np.float64)
    out = ~row["mask"]
    ang, r = rng.uniform(0, 2 * np.pi, out.sum()), rng.uniform(40, 80, out.sum())
    xq[out] += np.c_[r * np.cos(ang), r * np.sin(ang)]
    depth = rng.uniform(1.6, 2.8, len(kept))
    ray = (s.K_inv @ np.c_[xq, np.ones(len(kept))].T) * depth
    X[~row["lm_lost"]] = (Rt @ ray + tt).T
    # candidates: pool points by status and class
    c_idx = np.zeros(C0, np.int64)
    first = np.zeros((C0, 2), F32)
    tau = np.zeros(C0, np.int64)
    cand = np.zeros((C0, 2), F32)
    if C0 == 1:
        # never tracked (Q7): an A candidate designed at the point itself
        for j in p["by"]["A"]:
            f = _design_first(s, b["target"], p["pts"][[j]], ["A"], [1], rng).astype(F32)
            if classify(_state_with(s, X[:0], X[:0, :2], p["pts"][[j]], f, [1]), Rt, tt)[0] == "A":
                c_idx[0], first[0], tau[0] = j, f[0], 1
                break
        else:
            raise AssertionError("no A candidate for the single-candidate chain")
        cand[0] = p["pts"][c_idx[0]]
    elif C0 > 1:
        c_idx[row["c_lost"]] = p["lost"][rng.permutation(len(p["lost"]))[:row["c_lost"].sum()]]
        nxt = {c: 0 for c in "FSADG"}
        order = {c: p["by"][c][rng.permutation(len(p["by"][c]))] for c in "FSADG"}
        kept_c = []
        for c in row["classes"]:
            assert nxt[c] < len(order[c]), f"{name}: the pool holds {len(order[c])} candidates of class {c}"
            kept_c.append(order[c][nxt[c]])
            nxt[c] += 1
        c_idx[~row["c_lost"]] = kept_c
        first, tau, cand = p["first"][c_idx], p["tau"][c_idx], p["pts"][c_idx]
    return _state_with(s, X, p["pts"][lm_idx], cand, first, tau), lm_idx, c_idx


def _snap(s, R, t, info=None):
    return dict(landmarks=np.array(s.lm, F32).reshape(-1, 3), keypoints=np.array(s.kp, F32).reshape(-1, 2),
                cand=np.array(s.cand, F32).reshape(-1, 2), cand_first=np.array(s.cand_first, F32).reshape(-1, 2),
                cand_tau=np.array(s.cand_tau, np.float64).reshape(-1, 1), inliers=np.array(s.inl_pts),
                outliers=np.array(s.outl_pts), R=np.array(R), t=np.array(t), info=info)


def compose_to_pnp(s, img):
    """continuous_operation up to the triangulation, as plain oracle calls on s (modified in place):
    V.track, cv.solvePnPRansac, the inlier filter, the inversion.  Returns (R_CW, t_CW, mask)."""
    from oracle import cv2_oracle as cv
    V = _V()
    o = s.opts
    V.track(s, img)
    assert len(s.kp) >= 8
    ok, rv, t_WC, inl = cv.solvePnPRansac(s.lm, s.kp, s.K, np.zeros(4), flags=cv.SOLVEPNP_P3P, confidence=o['PnP_conf'],
                                          reprojectionError=o['PnP_error'], iterationsCount=o['PnP_iterations'])
    assert ok
    keep = np.isin(np.arange(len(s.lm)), inl.squeeze()).astype(bool)
    s.outl_pts = s.kp[~keep]
    s.inl_pts = s.kp[keep]
    V._keep_landmarks(s, keep)
    R_CW, t_CW = V._inv_rigid(cv.Rodrigues(rv)[0], t_WC)
    return R_CW, t_CW, keep


def compose(s, img, max_err=None):
    """The whole step up to feature adding on a copy of s: compose_to_pnp, then (:366)
    V.triangulate_candidates, or with max_err the gate's restatement.  Returns the snapshot."""
    import test_tri_gate_ref as TG
    V = _V()
    s = copy.deepcopy(s)
    R, t, _ = compose_to_pnp(s, img)
    info = [0, 0, 0, 0]
    if s.cand.shape[0] > 1:
        if max_err is None:
            V.triangulate_candidates(s, R, t)
        else:
            info = TG.triangulate_candidates_ref(s, R, t, max_err)
    return _snap(s, R, t, info if max_err is not None else None)


def designs():
    """[dict(name, row, state (before tracking), lm_idx, c_idx (pool indices of its rows), L1, C1,
    tracked (the state after V.track), mask (the oracle's inlier mask over L1), R, t (the current
    pose), classes (the oracle's class of every tracked candidate under that pose; None where the
    chain does not triangulate), plain, gated (the expected snapshots))] in NAMES order."""
    if "designs" in _CACHE:
        return _CACHE["designs"]
    b, T = base(), table()
    out = []
    for name in NAMES:
        row = T[name]
        if row["stopped"]:
            src = next(d for d in out if d["name"] == "l600_c513_mix")
            out.append(dict(src, name=name, row=row))
            continue
        st, lm_idx, c_idx = _build_state(name, row)
        tr = copy.deepcopy(st)
        R, t, mask = compose_to_pnp(tr, b["next_img"])
        tracked = copy.deepcopy(st)
        _V().track(tracked, b["next_img"])
        cls = classify(tr, R, t) if tr.cand.shape[0] > 1 else None
        out.append(dict(name=name, row=row, state=st, lm_idx=lm_idx, c_idx=c_idx, L1=len(tracked.kp), C1=len(tracked.cand),
                        tracked=tracked, mask=mask, R=R, t=t, classes=cls, plain=compose(st, b["next_img"]),
                        gated=compose(st, b["next_img"], MAX_ERR)))
    _CACHE["designs"] = out
    return out


def force_cases():
    """[(state before triangulation, R_CW, t_CW, state after V.triangulate_candidates called
    directly)] for the chains with one candidate (an A) and with none: vo_triangulate(force = 1)."""
    if "force" not in _CACHE:
        b = base()
        out = []
        for d in designs()[:2][::-1]:
            s = copy.deepcopy(d["state"])
            R, t, _ = compose_to_pnp(s, b["next_img"])
            after = copy.deepcopy(s)
            _V().triangulate_candidates(after, R, t)
            out.append((s, R, t, after))
        _CACHE["force"] = out
    return _CACHE["force"]
