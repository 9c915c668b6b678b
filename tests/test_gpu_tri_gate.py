"""The reprojection-error gate on new landmarks on the GPU: vo_triangulate_points_err, the _gated
entry points and the engine option tri_max_reproj_error against the definition
(test_tri_gate_ref), bit for bit.

The pipeline tests run oracle.vo_pipeline_oracle with its triangulate_candidates replaced by the
restatement at 8 px and compare every pose, point count, landmark and candidate array and the four
counters of an Engine with tri_max_reproj_error = 8.0, in each of its step forms.
"""
import copy
import ctypes as C

import numpy as np
import pytest

import test_tri_gate_ref as G

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_lk_fb import KEYS, _assert_chain, _import   # noqa: E402

MAX_ERR = 8.0
N_STEPS = G.N_STEPS
SENT = -7.0
ISENT = -77
BAD = (0.0, -1.0, float("nan"), float("inf"))
_CACHE = {}


def _p(t):
    return C.c_void_p(t.data_ptr())


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).tobytes()


def _lib():
    from monocular_visual_odometry_va4mr_amd import _lib as L
    return L


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------ vo_triangulate_points_err
KITTI_K = np.array([[718.856, 0.0, 607.1928], [0.0, 718.856, 185.2157], [0.0, 0.0, 1.0]])
KINDS = ("behind", "parallax", "far", "noise0", "noise05", "noise5")


def points_problem():
    """257 rows cycling through KINDS: a pair whose rays diverge (the point lands behind a camera),
    a 0.1 degree parallax pair, a 60 m point, and points at 5 to 30 m with observation noise of 0,
    0.5 and 5 px.  (P1 [n][12], P2, x1 [n][2] f32, x2)"""
    if "pts" not in _CACHE:
        rng = np.random.default_rng(11)
        n = 257
        P1, P2 = np.zeros((n, 12)), np.zeros((n, 12))
        x1, x2 = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
        for i in range(n):
            kind = KINDS[i % len(KINDS)]
            Z = {"parallax": 20.0, "far": 60.0}.get(kind, rng.uniform(5, 30))
            base = Z * np.tan(np.radians(0.1)) if kind == "parallax" else 1.0
            Xw = np.array([rng.uniform(-0.6, 0.6) * Z, rng.uniform(-0.2, 0.2) * Z, Z, 1.0])
            rv = rng.normal(size=(3, 1)) * 0.02
            R2 = np.eye(3) if kind == "behind" else G.CV.Rodrigues(rv)[0]    # (a rotation could undo the flip below)
            A = KITTI_K @ np.hstack((np.eye(3), np.zeros((3, 1))))
            B = KITTI_K @ np.hstack((R2, np.array([[-base], [0.01], [0.05]])))
            a, b = A @ Xw, B @ Xw
            a, b = a[:2] / a[2], b[:2] / b[2]
            sig = {"noise05": 0.5, "noise5": 5.0}.get(kind, 0.0)
            a, b = a + rng.normal(size=2) * sig, b + rng.normal(size=2) * sig
            if kind == "behind":
                a, b = b, a                     # the disparity's sign flipped: the rays meet behind the cameras
            P1[i], P2[i], x1[i], x2[i] = A.ravel(), B.ravel(), a, b
        for v in (P1, P2, x1, x2):
            v.setflags(write=False)
        _CACHE["pts"] = (P1, P2, x1, x2)
    return _CACHE["pts"]


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_triangulate_points_err(n):
    L = _lib()
    P1, P2, x1, x2 = points_problem()
    pad = 3
    d = lambda a: torch.from_numpy(np.array(a)).cuda()
    dP1, dP2, dx1, dx2 = d(P1), d(P2), d(x1), d(x2)
    out = torch.full((n + pad, 4), SENT, dtype=torch.float32, device="cuda")
    err = torch.full((n + pad, 2), SENT, dtype=torch.float64, device="cuda")
    plain = torch.full((n + pad, 4), SENT, dtype=torch.float32, device="cuda")
    assert L.lib().vo_triangulate_points_err(n, _p(dP1), _p(dP2), _p(dx1), _p(dx2), _p(out), _p(err), _stream()) == 0
    assert L.lib().vo_triangulate_points(n, _p(dP1), _p(dP2), _p(dx1), _p(dx2), _p(plain), _stream()) == 0
    torch.cuda.synchronize()
    out, err, plain = out.cpu().numpy(), err.cpu().numpy(), plain.cpu().numpy()
    assert out.tobytes() == plain.tobytes()
    assert np.all(out[n:] == SENT) and np.all(err[n:] == SENT)           # rows past n untouched
    want = np.zeros((n, 2))
    for i in range(n):
        X = out[i, :3] / out[i, 3]
        assert X.dtype == np.float32
        want[i] = G.reproj_err2(P1[i].reshape(3, 4), X, x1[i]), G.reproj_err2(P2[i].reshape(3, 4), X, x2[i])
    assert _bits(err[:n]) == _bits(want), [(i, err[i].tolist(), want[i].tolist()) for i in range(n)
                                           if _bits(err[i]) != _bits(want[i])][:4]
    # the inputs are what they claim to be
    kinds = np.array([KINDS.index(KINDS[i % len(KINDS)]) for i in range(n)])
    assert np.all(np.isinf(want[kinds == 0]).any(axis=1)) and np.isinf(want[0]).any()
    if n >= 64:
        e = want.max(axis=1)
        assert np.all(np.isfinite(want[kinds != 0]))
        assert np.all(e[kinds == 3] < 1e-3)                               # exact observations, float32 rounding only
        assert np.median(e[kinds == 5]) > 10 * np.median(e[kinds == 4]) > 0


def test_triangulate_points_err_rejects_null_buffers():
    L = _lib()
    P1, P2, x1, x2 = points_problem()
    d = lambda a: torch.from_numpy(np.array(a)).cuda()
    dP1, dP2, dx1, dx2 = d(P1), d(P2), d(x1), d(x2)
    out = torch.zeros((4, 4), dtype=torch.float32, device="cuda")
    assert L.lib().vo_triangulate_points_err(4, _p(dP1), _p(dP2), _p(dx1), _p(dx2), _p(out), None, _stream()) == -1
    assert L.lib().vo_triangulate_points_err(-1, _p(dP1), _p(dP2), _p(dx1), _p(dx2), _p(out), None, _stream()) == -1
    assert L.lib().vo_triangulate_points_err(0, None, None, None, None, None, None, _stream()) == 0


# ------------------------------------------------------------------ vo_triangulate_gated on a state
def _engine(K, opts, batch=1, ncap=4096, **extra):
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    return Engine(K, dict(opts, **extra), 1241, 376, batch=batch, ncap=ncap, pcap=8192, fcap=32)


def _import_before(eng, b):
    """Chain b as the oracle's state right before the triangulation of the second tracked frame:
    the new pose in slot nF, not yet counted."""
    s, R, t = G.state_before_triangulation()
    eng.import_chain(b, landmarks=s.lm, keypoints=s.kp, cand=s.cand, cand_first=s.cand_first, cand_tau=s.cand_tau,
                     transforms=list(s.transforms) + [(R, t)], num_pts=s.num_pts, prev_img=s.prev_img)
    eng.t["nF"][b] -= 1


def _tri_ref(max_err):
    key = ("tri", max_err)
    if key not in _CACHE:
        s, R, t = G.state_before_triangulation()
        s = copy.deepcopy(s)
        n0 = len(s.lm)
        trace = []
        counts = G.triangulate_candidates_ref(s, R, t, max_err, trace)
        _CACHE[key] = (s, counts, n0, trace)
    return _CACHE[key]


def _tri_opts(max_err, info):
    return _lib().VoTriOpts(max_err, 0 if info is None else info.data_ptr())


def _state_bytes(eng):
    torch.cuda.synchronize()
    return {k: eng.t[k].cpu().numpy().tobytes() for k in KEYS}


def _assert_tri_state(eng, b, s, what):
    e = eng.export_chain(b)
    assert e["status"] == 0, what
    assert len(e["landmarks"]) == len(s.lm) and len(e["cand"]) == len(s.cand), f"{what}: nL / nC"
    for name, want in (("landmarks", s.lm), ("keypoints", s.kp), ("cand", s.cand), ("cand_first", s.cand_first),
                       ("cand_tau", s.cand_tau)):
        assert np.array_equal(e[name], want), f"{what}: {name}"


@pytest.mark.parametrize("max_err", [2.0, 8.0])
@pytest.mark.parametrize("form", ["split", "one_launch"])
def test_triangulate_gated_state(form, max_err, launch_cus):
    """Two chains with the same state, chain 1 with a status set: chain 0 equals the restatement,
    counters included, chain 1 and its counters' row are left alone.  split: two chains are fewer
    than the CUs (k_tri_gate, k_tri_solve_gated, k_tri_append_gated); one_launch: on "one CU"
    (k_triangulate_gated)."""
    L = _lib()
    fr, K, opts, _ = G.kitti_start()
    s, counts, n0, _ = _tri_ref(max_err)
    assert counts[2] > 0 and counts[3] > 0 and counts[1] > 0
    if form == "one_launch":
        launch_cus(1)
    eng = _engine(K, opts, batch=2)
    _import_before(eng, 0)
    _import_before(eng, 1)
    eng.t["status"][1] = L.ST_PNP_FAILED
    before = _state_bytes(eng)
    info = torch.full((2, 4), ISENT, dtype=torch.int32, device="cuda")
    tg = _tri_opts(max_err, info)
    assert eng.lib.vo_triangulate_gated(eng._pd, eng._po, eng._ps, 0, C.byref(tg), eng.stream) == 0
    _assert_tri_state(eng, 0, s, f"{form} {max_err}")
    info = info.cpu().numpy()
    assert info[0].tolist() == counts, (info[0].tolist(), counts)
    assert np.all(info[1] == ISENT)
    e1 = eng.export_chain(1)
    assert e1["status"] == L.ST_PNP_FAILED and len(e1["landmarks"]) == n0
    after = _state_bytes(eng)
    for k in KEYS:
        a = np.frombuffer(after[k], np.uint8).reshape(2, -1)[1]
        b = np.frombuffer(before[k], np.uint8).reshape(2, -1)[1]
        assert np.array_equal(a, b), k


def test_triangulate_gated_without_info_and_idle_chain():
    """info = NULL: the same state, nothing written; a chain with one candidate does not triangulate
    (:366) and reports four zeros."""
    fr, K, opts, _ = G.kitti_start()
    s, counts, _, _ = _tri_ref(MAX_ERR)
    eng = _engine(K, opts, batch=2)
    _import_before(eng, 0)
    _import_before(eng, 1)
    eng.t["nC"][1] = 1
    tg = _tri_opts(MAX_ERR, None)
    assert eng.lib.vo_triangulate_gated(eng._pd, eng._po, eng._ps, 0, C.byref(tg), eng.stream) == 0
    _assert_tri_state(eng, 0, s, "no info")
    eng2 = _engine(K, opts, batch=2)
    _import_before(eng2, 0)
    _import_before(eng2, 1)
    eng2.t["nC"][1] = 1
    info = torch.full((2, 4), ISENT, dtype=torch.int32, device="cuda")
    tg = _tri_opts(MAX_ERR, info)
    assert eng2.lib.vo_triangulate_gated(eng2._pd, eng2._po, eng2._ps, 0, C.byref(tg), eng2.stream) == 0
    torch.cuda.synchronize()
    assert info.cpu().numpy().tolist() == [counts, [0, 0, 0, 0]]
    assert int(eng2.t["nC"][1]) == 1 and int(eng2.t["nL"][1]) == int(eng.t["nL"][1])


def _smallest_root(e):
    """The smallest double m with m * m >= e."""
    m = np.sqrt(np.float64(e))
    while m * m >= e:
        m = np.nextafter(m, 0.0)
    while m * m < e:
        m = np.nextafter(m, np.inf)
    return float(m)


@pytest.mark.parametrize("form", ["split", "one_launch"])
def test_gate_boundary(form, launch_cus):
    """One candidate's e = max(e_past, e_cur) read from the primitive; with max_reproj_error the
    smallest double whose square reaches e the candidate becomes a landmark, one double below it is
    dropped."""
    L = _lib()
    fr, K, opts, _ = G.kitti_start()
    _, counts, n0, trace = _tri_ref(None)
    s_before = G.state_before_triangulation()[0]
    # the candidate in the middle of those that passed the depth gate
    i, P_past, P_cur, X = trace[len(trace) // 2]
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    dP1, dP2 = d(P_past.reshape(1, 12), np.float64), d(P_cur.reshape(1, 12), np.float64)
    dx1, dx2 = d(s_before.cand_first[i].reshape(1, 2), np.float32), d(s_before.cand[i].reshape(1, 2), np.float32)
    out = torch.zeros((1, 4), dtype=torch.float32, device="cuda")
    err = torch.zeros((1, 2), dtype=torch.float64, device="cuda")
    assert L.lib().vo_triangulate_points_err(1, _p(dP1), _p(dP2), _p(dx1), _p(dx2), _p(out), _p(err), _stream()) == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy()[0]
    assert np.array_equal(o[:3] / o[3], X.ravel())                       # the point the depth gate saw
    e = float(err.cpu().numpy().max())
    assert np.isfinite(e) and e > 0
    m = _smallest_root(e)
    assert m * m >= e and np.nextafter(m, 0.0) ** 2 < e
    if form == "one_launch":
        launch_cus(1)
    got = []
    for thr in (m, float(np.nextafter(m, 0.0))):
        eng = _engine(K, opts)
        _import_before(eng, 0)
        info = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
        tg = _tri_opts(thr, info)
        assert eng.lib.vo_triangulate_gated(eng._pd, eng._po, eng._ps, 0, C.byref(tg), eng.stream) == 0
        ex = eng.export_chain(0)
        new = np.hstack((ex["landmarks"][n0:], ex["keypoints"][n0:]))
        row = np.hstack((X.ravel(), s_before.cand[i]))
        is_lm = bool((new == row).all(axis=1).any())
        is_cand = bool((ex["cand_first"] == s_before.cand_first[i]).all(axis=1).any())
        got.append((is_lm, is_cand, info.cpu().numpy()[0].tolist()))
    assert got[0][0] and not got[0][1], got
    assert not got[1][0] and not got[1][1], got
    assert got[1][2][2] == got[0][2][2] + 1 and got[1][2][3] == got[0][2][3] - 1, got


@pytest.mark.parametrize("form", ["split", "one_launch"])
def test_gated_capacity(form, launch_cus):
    """ncap exactly what the gated step needs: status 0; one short: VO_ST_CAPACITY, as the ungated
    path.  The dropped candidates take no room: the ungated step does not fit the first engine."""
    L = _lib()
    fr, K, opts, _ = G.kitti_start()
    s, counts, n0, _ = _tri_ref(MAX_ERR)
    assert counts[2] > 0
    if form == "one_launch":
        launch_cus(1)
    need = n0 + counts[3]
    for ncap, tri, want in ((need, True, L.ST_OK), (need - 1, True, L.ST_CAPACITY), (need, False, L.ST_CAPACITY)):
        eng = _engine(K, opts, ncap=ncap)
        _import_before(eng, 0)
        info = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
        tg = _tri_opts(MAX_ERR, info)
        rc = eng.lib.vo_triangulate_gated(eng._pd, eng._po, eng._ps, 0, C.byref(tg) if tri else None, eng.stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert int(eng.t["status"][0]) == want, (ncap, tri)
        assert int(eng.t["nL"][0]) == ncap
        if tri:
            assert info.cpu().numpy()[0].tolist() == counts
            assert np.array_equal(eng.t["lm_X"][0].cpu().numpy(), s.lm[:ncap])


def _entry_points(eng, tg):
    lib, pd, po, ps = eng.lib, eng._pd, eng._po, eng._ps
    z = C.c_double(1e-10)
    return {
        "vo_triangulate_gated": lambda: lib.vo_triangulate_gated(pd, po, ps, 0, tg, eng.stream),
        "vo_pnp_gated": lambda: lib.vo_pnp_gated(pd, po, ps, 0, z, None, tg, eng.stream),
        "vo_pnp_triangulate_gated": lambda: lib.vo_pnp_triangulate_gated(pd, po, ps, 0, z, None, tg, eng.stream),
        "vo_filter_pnp_triangulate_gated": lambda: lib.vo_filter_pnp_triangulate_gated(pd, po, ps, 0, z, None, tg, eng.stream),
    }


def test_bad_arguments():
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    fr, K, opts, _ = G.kitti_start()
    eng = _engine(K, opts)
    _import_before(eng, 0)
    before = _state_bytes(eng)
    info = torch.full((1, 4), ISENT, dtype=torch.int32, device="cuda")
    for bad in BAD:
        tg = _tri_opts(bad, info)
        for name, call in _entry_points(eng, C.byref(tg)).items():
            assert call() == -1, (name, bad)
    assert _state_bytes(eng) == before and np.all(info.cpu().numpy() == ISENT)
    for bad in BAD:
        with pytest.raises(ValueError):
            Engine(K, dict(opts, tri_max_reproj_error=bad), 1241, 376, batch=1, ncap=64, pcap=64, fcap=4)


# ------------------------------------------------------------------ the pipeline
FORMS = ["default", "compact_in_track", "split", "track_stream", "graph", "prefetch", "launch_cus_1"]


def _refined_pnp(iters, ftol):
    import test_pnp_refine_ref as R

    def refined(keep, objectPoints, imagePoints, cameraMatrix, distCoeffs, **kw):
        ok, rv, tv, inl = keep(objectPoints, imagePoints, cameraMatrix, distCoeffs, **kw)
        assert ok
        idx = np.asarray(inl).ravel()
        obj = np.asarray(objectPoints, np.float32).reshape(-1, 3)
        img = np.asarray(imagePoints, np.float32).reshape(-1, 2)
        rv2, tv2, _ = R.refine_ref(obj[idx], img[idx], cameraMatrix, rv, tv, iters, ftol)
        return ok, rv2.reshape(np.shape(rv)), tv2.reshape(np.shape(tv)), inl
    return refined


def _fb_lk(thr):
    import test_lk_flags_ref as LKR

    def gated(keep, prevImg, nextImg, prevPts, nextPts, winSize=(21, 21), maxLevel=3, criteria=(3, 30, 0.01), flags=0,
              minEigThreshold=1e-4):
        p = np.asarray(prevPts)
        assert flags == 0 and nextPts is None and p.dtype == np.float32
        q, gate, ef, _, _, _ = LKR.fb_compose(prevImg, nextImg, p.reshape(-1, 2), tuple(winSize), int(maxLevel),
                                              tuple(criteria), float(minEigThreshold), thr)
        return q.reshape(p.shape), gate.reshape(-1, 1), ef.reshape(-1, 1)
    return gated


def _reference(refine=0, fb=None, n_steps=N_STEPS):
    """(snapshots, counters) of the oracle pipeline with the restatement at MAX_ERR, optionally with
    the pose refinement's and the forward-backward gate's restatements as well; computed once."""
    key = ("ref", refine, fb, n_steps)
    if key not in _CACHE:
        if not refine and fb is None:
            snaps, counts = G.pipeline(MAX_ERR, n_steps)
        else:
            snaps, counts, _ = G.run_oracle(MAX_ERR, n_steps, pnp=_refined_pnp(refine, 1e-10) if refine else None,
                                            lk=None if fb is None else _fb_lk(fb))
        assert len(snaps) == len(counts) == n_steps and sum(c[2] for c in counts) > 0
        _CACHE[key] = (snaps, counts)
    return _CACHE[key]


def _run_form(form, monkeypatch, launch_cus, refine=0, fb=None, n_steps=N_STEPS):
    fr, K, opts, s0 = G.kitti_start()
    snaps, counts = _reference(refine, fb, n_steps)
    if form == "compact_in_track":
        monkeypatch.setenv("VO_COMPACT_IN_TRACK", "1")
    else:
        monkeypatch.delenv("VO_COMPACT_IN_TRACK", raising=False)
    monkeypatch.delenv("VO_PREFETCH", raising=False)
    if form == "launch_cus_1":
        launch_cus(1)
    extra = dict(tri_max_reproj_error=MAX_ERR)
    if refine:
        extra["pnp_refine_iters"] = refine
    if fb is not None:
        extra["lk_fb_threshold"] = fb
    eng = _engine(K, opts, **extra)
    assert eng.tri_max_reproj_error == MAX_ERR and tuple(eng._tri_info.shape) == (1, 4)
    if form == "split":
        eng.fuse_pnp_tri = False
    if form == "track_stream":
        eng.track_stream = torch.cuda.Stream()
    _import(eng, 0, s0)
    frames = [torch.from_numpy(np.ascontiguousarray(fr[3 + k][None])).cuda() for k in range(n_steps)]
    if form == "graph":
        eng.capture_step()
    for k in range(n_steps):
        if form == "graph":
            eng.step_graph(frames[k])
        elif form == "prefetch":
            eng.step(frames[k], next_frames=frames[k + 1] if k + 1 < n_steps else None)
        else:
            eng.step(frames[k])
        _assert_chain(eng, 0, snaps[k], f"{form}: step {k}")
        assert eng.tri_gate_info()[0].tolist() == counts[k], f"{form}: step {k}: counters"
    return eng


@pytest.mark.parametrize("form", FORMS)
def test_engine_gate_pipeline_single_chain(form, monkeypatch, launch_cus):
    _run_form(form, monkeypatch, launch_cus)


@pytest.mark.parametrize("form", ["default", "split"])
def test_engine_gate_with_the_pose_refinement(form, monkeypatch, launch_cus):
    """pnp_refine_iters = 10 as well: the pose and the triangulation both go through their optional
    kernels (default: k_pnp_tri_gated<., true>; split: k_pnp_refine_state, then the gated
    triangulation)."""
    eng = _run_form(form, monkeypatch, launch_cus, refine=10)
    assert eng.refine_info()[0][1] >= 1
    plain = _reference()[0]
    assert not np.array_equal(_reference(refine=10)[0][-1]["t"], plain[-1]["t"])


def test_engine_gate_with_the_fb_gate(monkeypatch, launch_cus):
    _run_form("default", monkeypatch, launch_cus, fb=1.0, n_steps=5)


@pytest.mark.parametrize("form", ["default", "graph", "launch_cus_1"])
def test_engine_gate_pipeline_batch(form, launch_cus):
    """Chain 0 of a 3-chain batch (starts 0, 1, 3 over 14 frames, 7 steps); the other chains run
    their own sequences and must end with status 0.  launch_cus_1: three chains on "one CU" take
    the two-blocks-per-CU build of the fused kernel."""
    from monocular_visual_odometry_va4mr_amd.synth import make_sequence
    fr11, K, opts, s0 = G.kitti_start()
    snaps, counts = _reference()
    fr = make_sequence("kitti", 14, seed=1)[0]
    assert np.array_equal(fr[:11], fr11)
    frames = torch.from_numpy(np.ascontiguousarray(fr)).cuda()
    starts = [0, 1, 3]
    if form == "launch_cus_1":
        launch_cus(1)
    eng = _engine(K, opts, batch=3, tri_max_reproj_error=MAX_ERR)
    eng.bootstrap(frames[starts], frames[[s + 2 for s in starts]])
    _import(eng, 0, s0)                       # chain 0 from the reference's own initial state
    if form == "graph":
        eng.capture_step()
    dropped = np.zeros(3, np.int64)
    for k in range(7):
        f = frames[[s + 3 + k for s in starts]]
        if form == "graph":
            eng.step_graph(f)
        else:
            eng.step(f)
        _assert_chain(eng, 0, snaps[k], f"{form}: step {k}")
        info = eng.tri_gate_info()
        assert info[0].tolist() == counts[k]
        assert np.all(info[:, 0] == info[:, 1] + info[:, 2] + info[:, 3])
        dropped += info[:, 2]
    assert (eng.statuses() == 0).all() and np.all(dropped > 0)


class _NullStructLib:
    """The library with the plain step calls routed through the new entry points and a NULL struct."""

    def __init__(self, lib):
        self._lib = lib
        self.vo_triangulate = lambda pd, po, ps, force, st: lib.vo_triangulate_gated(pd, po, ps, force, None, st)
        self.vo_pnp = lambda pd, po, ps, st: lib.vo_pnp_gated(pd, po, ps, 0, C.c_double(0.0), None, None, st)
        self.vo_pnp_triangulate = lambda pd, po, ps, st: lib.vo_pnp_triangulate_gated(pd, po, ps, 0, C.c_double(0.0), None, None, st)
        self.vo_filter_pnp_triangulate = lambda pd, po, ps, st: lib.vo_filter_pnp_triangulate_gated(
            pd, po, ps, 0, C.c_double(0.0), None, None, st)

    def __getattr__(self, name):
        return getattr(self._lib, name)


@pytest.mark.parametrize("form", ["default", "compact_in_track", "split"])
@pytest.mark.parametrize("how", ["no_key", "null_struct"])
def test_off_is_off(how, form, monkeypatch):
    """An Engine without the key, or with None, has no counters and gives the plain oracle's state
    over the 8 steps; so does a NULL vo_tri_opts given to each new entry point (default:
    vo_filter_pnp_triangulate_gated; compact_in_track: vo_pnp_triangulate_gated; split:
    vo_pnp_gated + vo_triangulate_gated)."""
    fr, K, opts, s0 = G.kitti_start()
    plain = G.plain_pipeline()
    if form == "compact_in_track":
        monkeypatch.setenv("VO_COMPACT_IN_TRACK", "1")
    else:
        monkeypatch.delenv("VO_COMPACT_IN_TRACK", raising=False)
    eng = _engine(K, opts, **({"tri_max_reproj_error": None} if form == "split" else {}))
    assert eng.tri_max_reproj_error is None and eng._tri_info is None and eng.tri_gate_info() is None
    if how == "null_struct":
        eng.lib = _NullStructLib(eng.lib)
    if form == "split":
        eng.fuse_pnp_tri = False
    _import(eng, 0, s0)
    for k in range(N_STEPS):
        eng.step(fr[3 + k])
        _assert_chain(eng, 0, plain[k], f"{how} {form}: step {k}")


def test_dropin_class_and_runners_pass_the_option_through():
    from monocular_visual_odometry_va4mr_amd import run_dataset as RD
    from monocular_visual_odometry_va4mr_amd import run_sequence as RS
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    from monocular_visual_odometry_va4mr_amd.VisualOdometryPipeLine import VisualOdometryPipeLine
    fr, K, opts, _ = G.kitti_start()
    vo = VisualOdometryPipeLine(K, dict(opts, tri_max_reproj_error=2.0), max_frames=32, landmark_capacity=4096,
                                candidate_capacity=8192)
    vo.initialization(fr[0], fr[2])
    for k in range(3):
        vo.continuous_operation(fr[3 + k])
    assert vo._eng.tri_max_reproj_error == 2.0 and vo._eng.tri_gate_info()[0, 2] > 0
    res = RD.run("synthetic-kitti", None, last_frame=7, plot=None, tri_max_reproj_error=2.0)
    assert res["_vo"]._eng.tri_max_reproj_error == 2.0 and res["frames"] == 4
    assert res["_vo"]._eng.tri_gate_info()[0, 2] > 0
    seen = []

    class Recording(Engine):
        def __init__(self, K_, options, *a, **kw):
            super().__init__(K_, options, *a, **kw)
            seen.append(self.tri_max_reproj_error)

    rep = RS.run("kitti", 24, 2, overlap=4, engine_cls=Recording, tri_max_reproj_error=2.0)
    assert rep is not None and seen and all(s == 2.0 for s in seen)
