"""The PnP pose refinement on the GPU: vo_pnp_refine, cv2compat.solvePnPRefineLM and the engine
option pnp_refine_iters against the definition (test_pnp_refine_ref.refine_ref), bit for bit.

The pipeline tests run oracle.vo_pipeline_oracle with its solvePnPRansac followed by refine_ref on
the inliers (10 iterations) and compare every pose, point count, landmark and candidate array of an
Engine with pnp_refine_iters = 10, in each of its step forms.
"""
import copy
import ctypes as C

import numpy as np
import pytest

import test_lk_flags_ref as LKR
import test_pnp_refine_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_lk_fb import KEYS, _assert_chain, _import, _snap_oracle   # noqa: E402

ITERS, FTOL = 10, 1e-10
N_STEPS = 8
_CACHE = {}
SENT = -7.0


def _p(t):
    return C.c_void_p(t.data_ptr())


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).tobytes()


def _opts(K=R.KITTI_K):
    from monocular_visual_odometry_va4mr_amd import options as Op
    from monocular_visual_odometry_va4mr_amd.engine import make_opts
    return make_opts(K, Op.get("kitti")[0])


# ------------------------------------------------------------------ vo_pnp_refine
COUNTS = [0, 1, 4, 8, 63, 64, 65, 255, 256, 257, 700, 1400]
CAP = 1400
SKIPPED = (4, 8)               # chains (63 and 256 points) with success = 0


def batch_problem():
    """12 chains at the lane, wave and block boundaries of the summation; chain 10 starts ten times
    further off than the rest.  (obj [B][cap][3], img, rvec0 [B][3], tvec0)."""
    if "batch" not in _CACHE:
        B = len(COUNTS)
        obj = np.zeros((B, CAP, 3), np.float32)
        img = np.zeros((B, CAP, 2), np.float32)
        rv0 = np.zeros((B, 3))
        tv0 = np.zeros((B, 3))
        for b in range(B):
            o, i, _, _, r, t = R.make_problem(CAP, 50 + b, 0.5, far=b == 10)
            obj[b], img[b], rv0[b], tv0[b] = o, i, r, t
        for a in (obj, img, rv0, tv0):
            a.setflags(write=False)
        _CACHE["batch"] = (obj, img, rv0, tv0)
    return _CACHE["batch"]


def batch_reference(masked, iters):
    key = ("ref", masked, iters)
    if key not in _CACHE:
        obj, img, rv0, tv0 = batch_problem()
        mask = np.ones((len(COUNTS), CAP), np.uint8)
        if masked:
            mask[:, 2::3] = 0
        out = []
        for b, n in enumerate(COUNTS):
            m = mask[b, :n] != 0
            out.append(R.refine_ref(obj[b, :n][m], img[b, :n][m], R.KITTI_K, rv0[b], tv0[b], iters, FTOL))
        _CACHE[key] = (mask, out)
    return _CACHE[key]


def run_refine(obj, img, mask, counts, success, iters, ftol, rv0, tv0):
    from monocular_visual_odometry_va4mr_amd import _lib as L
    B, cap = obj.shape[:2]
    dev = "cuda"
    d = lambda a: torch.from_numpy(np.array(a)).to(dev)            # (a copy: the shared inputs are read-only)
    d_obj, d_img, d_cnt = d(obj), d(img), d(np.asarray(counts, np.int32))
    d_mask = None if mask is None else d(mask)
    d_ok = None if success is None else d(np.asarray(success, np.int32))
    rv, tv = d(np.array(rv0, np.float64)), d(np.array(tv0, np.float64))
    info = torch.full((B, 4), SENT, dtype=torch.float64, device=dev)
    o = _opts()
    rc = L.lib().vo_pnp_refine(C.byref(o), B, _p(d_obj), _p(d_img), None if d_mask is None else _p(d_mask), _p(d_cnt),
                               cap, None if d_ok is None else _p(d_ok), iters, C.c_double(ftol), _p(rv), _p(tv), _p(info),
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, rv.cpu().numpy(), tv.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize("iters", [1, 3, 10])
@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
def test_pnp_refine_matches_the_restatement(masked, iters):
    obj, img, rv0, tv0 = batch_problem()
    mask, ref = batch_reference(masked, iters)
    success = [0 if b in SKIPPED else 1 for b in range(len(COUNTS))]
    rc, rv, tv, info = run_refine(obj, img, mask if masked else None, COUNTS, success, iters, FTOL, rv0, tv0)
    assert rc == 0
    changed = rejected = 0
    for b, n in enumerate(COUNTS):
        what = f"chain {b} ({n} points, masked {masked}, {iters} iterations)"
        if b in SKIPPED:
            assert _bits(rv[b]) == _bits(rv0[b]) and _bits(tv[b]) == _bits(tv0[b]) and np.all(info[b] == SENT), what
            continue
        r_rv, r_tv, r_info = ref[b]
        assert _bits(info[b]) == _bits(r_info), f"{what}: info {info[b].tolist()} want {r_info.tolist()}"
        assert _bits(rv[b]) == _bits(r_rv), f"{what}: rvec {rv[b].tolist()} want {r_rv.tolist()}"
        assert _bits(tv[b]) == _bits(r_tv), f"{what}: tvec {tv[b].tolist()} want {r_tv.tolist()}"
        changed += int(_bits(rv[b]) != _bits(rv0[b]) and info[b][1] > 0)
        rejected += int(n >= 8 and info[b][1] < info[b][0])
    # not vacuous: the pose moved in at least 8 chains; a step was evaluated and rejected somewhere
    assert changed >= 8, changed
    if iters == 10:
        assert rejected >= 1


def test_pnp_refine_failed_start_leaves_the_pose():
    """A point behind the camera at the start: pose bits unchanged, 0 iterations, costs +inf; the
    chain next to it is refined as usual."""
    obj, img, _, _, rv0, tv0 = R.make_problem(64, 0, 0.5)
    obj = np.stack([obj, obj])
    obj[0, 17] = (0.0, 0.0, -5.0)
    img = np.stack([img, img])
    rc, rv, tv, info = run_refine(obj, img, None, [64, 64], None, 10, FTOL, [rv0, rv0], [tv0, tv0])
    assert rc == 0
    assert _bits(rv[0]) == _bits(rv0) and _bits(tv[0]) == _bits(tv0) and info[0].tolist() == [0.0, 0.0, np.inf, np.inf]
    want = R.refine_ref(obj[1], img[1], R.KITTI_K, rv0, tv0, 10, FTOL)
    assert _bits(rv[1]) == _bits(want[0]) and _bits(tv[1]) == _bits(want[1]) and _bits(info[1]) == _bits(want[2])


@pytest.mark.parametrize("iters,ftol", [(-1, 1e-10), (101, 1e-10), (10, float("nan")), (10, -1e-10), (10, float("inf"))])
def test_pnp_refine_rejects_bad_arguments(iters, ftol):
    obj, img, _, _, rv0, tv0 = R.make_problem(64, 0, 0.5)
    rc, rv, tv, info = run_refine(obj[None], img[None], None, [64], None, iters, ftol, [rv0], [tv0])
    assert rc == -1
    assert _bits(rv[0]) == _bits(rv0) and _bits(tv[0]) == _bits(tv0) and np.all(info == SENT)


def test_engine_entry_points_reject_bad_arguments():
    from monocular_visual_odometry_va4mr_amd import options as Op
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    eng = Engine(R.KITTI_K, Op.get("kitti")[0], 160, 120, batch=1, ncap=64, pcap=64, fcap=4)
    for f in (eng.lib.vo_pnp_ex, eng.lib.vo_pnp_triangulate_ex, eng.lib.vo_filter_pnp_triangulate_ex):
        for iters, ftol in [(-1, 1e-10), (101, 1e-10), (10, float("nan")), (10, -1.0)]:
            assert f(eng._pd, eng._po, eng._ps, iters, C.c_double(ftol), None, eng.stream) == -1


def test_cv2compat_solve_pnp_refine_lm():
    from monocular_visual_odometry_va4mr_amd import cv2compat as cv
    obj, img, _, _, rv0, tv0 = R.make_problem(300, 7, 0.5)
    rv_in, tv_in = rv0.reshape(3, 1).copy(), tv0.reshape(3, 1).copy()
    obj_in, img_in = obj.copy(), img.copy()
    rv, tv = cv.solvePnPRefineLM(obj_in, img_in, R.KITTI_K, np.zeros(4), rv_in, tv_in)
    want = R.refine_ref(obj, img, R.KITTI_K, rv0, tv0, 20, cv.FLT_EPSILON)
    assert rv.shape == (3, 1) and tv.shape == (3, 1) and rv.dtype == np.float64 and tv.dtype == np.float64
    assert _bits(rv) == _bits(want[0]) and _bits(tv) == _bits(want[1]) and want[2][1] >= 2
    assert np.array_equal(rv_in.ravel(), rv0) and np.array_equal(tv_in.ravel(), tv0)
    assert np.array_equal(obj_in, obj) and np.array_equal(img_in, img)
    rv3, _ = cv.solvePnPRefineLM(obj, img, R.KITTI_K, None, rv0, tv0, criteria=(cv.TERM_CRITERIA_COUNT, 1, 0.5))
    assert _bits(rv3) == _bits(R.refine_ref(obj, img, R.KITTI_K, rv0, tv0, 1, 0.0)[0])
    with pytest.raises(NotImplementedError):
        cv.solvePnPRefineLM(obj, img, R.KITTI_K, np.array([0.1, 0, 0, 0]), rv0, tv0)


# ------------------------------------------------------------------ the pipeline
def _gated_lk(thr):
    def gated(prevImg, nextImg, prevPts, nextPts, winSize=(21, 21), maxLevel=3, criteria=(3, 30, 0.01), flags=0,
              minEigThreshold=1e-4):
        p = np.asarray(prevPts)
        assert flags == 0 and nextPts is None and p.dtype == np.float32
        q, gate, ef, _, _, _ = LKR.fb_compose(prevImg, nextImg, p.reshape(-1, 2), tuple(winSize), int(maxLevel),
                                              tuple(criteria), float(minEigThreshold), thr)
        return q.reshape(p.shape), gate.reshape(-1, 1), ef.reshape(-1, 1)
    return gated


def pipeline_reference(fb=None, n_steps=N_STEPS):
    """The oracle pipeline on the synthetic KITTI sequence (bootstrap (0, 2)) with solvePnPRansac
    followed by refine_ref on obj[inl], img[inl]; fb: also the forward-backward gate at that
    threshold.  Returns (frames, K, opts, initial state, refined snapshots, their infos, plain
    snapshots); computed once."""
    key = ("pipe", fb, n_steps)
    if key in _CACHE:
        return _CACHE[key]
    from oracle import cv2_oracle as CV
    from oracle import vo_pipeline_oracle as V
    from monocular_visual_odometry_va4mr_amd import options as Op
    from monocular_visual_odometry_va4mr_amd.synth import make_sequence
    fr, K, _, _ = make_sequence("kitti", 11, seed=1)
    opts, boot, _ = Op.get("kitti")
    assert boot == (0, 2)
    s0 = V.new_state(K, opts)
    V.initialize(s0, fr[0], fr[2])
    infos = []
    keep_pnp, keep_lk = CV.solvePnPRansac, CV.calcOpticalFlowPyrLK

    def refined(objectPoints, imagePoints, cameraMatrix, distCoeffs, **kw):
        ok, rv, tv, inl = keep_pnp(objectPoints, imagePoints, cameraMatrix, distCoeffs, **kw)
        assert ok
        idx = np.asarray(inl).ravel()
        assert np.all(np.diff(idx) > 0)
        obj = np.asarray(objectPoints, np.float32).reshape(-1, 3)
        img = np.asarray(imagePoints, np.float32).reshape(-1, 2)
        rv2, tv2, info = R.refine_ref(obj[idx], img[idx], cameraMatrix, rv, tv, ITERS, FTOL)
        infos.append(info)
        return ok, rv2.reshape(np.shape(rv)), tv2.reshape(np.shape(tv)), inl

    def run_steps(pnp, lk):
        s = copy.deepcopy(s0)
        snaps = []
        CV.solvePnPRansac, CV.calcOpticalFlowPyrLK = pnp, lk     # looked up as cv.<name> at call time
        try:
            for k in range(n_steps):
                V.step(s, fr[3 + k])
                snaps.append(_snap_oracle(s))
        finally:
            CV.solvePnPRansac, CV.calcOpticalFlowPyrLK = keep_pnp, keep_lk
        return snaps

    lk = keep_lk if fb is None else _gated_lk(fb)
    plain = run_steps(keep_pnp, lk)
    snaps = run_steps(refined, lk)
    # the refinement is at work in every step, and it changes the trajectory
    assert len(infos) == n_steps
    for k in range(n_steps):
        assert infos[k][3] < infos[k][2] and infos[k][1] >= 1, infos[k]
        assert not np.array_equal(snaps[k]["t"], plain[k]["t"]) and not np.array_equal(snaps[k]["R"], plain[k]["R"])
    _CACHE[key] = (fr, K, opts, s0, snaps, infos, plain)
    return _CACHE[key]


def _engine(K, opts, batch=1, **extra):
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    return Engine(K, dict(opts, **extra), 1241, 376, batch=batch, ncap=4096, pcap=8192, fcap=32)


FORMS = ["default", "compact_in_track", "split", "track_stream", "graph", "prefetch"]


def _run_forms(form, monkeypatch, fb, n_steps):
    fr, K, opts, s0, snaps, infos, _ = pipeline_reference(fb, n_steps)
    if form == "compact_in_track":
        monkeypatch.setenv("VO_COMPACT_IN_TRACK", "1")
    else:
        monkeypatch.delenv("VO_COMPACT_IN_TRACK", raising=False)
    monkeypatch.delenv("VO_PREFETCH", raising=False)
    extra = dict(pnp_refine_iters=ITERS)
    if fb is not None:
        extra["lk_fb_threshold"] = fb
    eng = _engine(K, opts, **extra)
    assert eng.pnp_refine_iters == ITERS and eng.pnp_refine_ftol == FTOL and tuple(eng._refine_info.shape) == (1, 4)
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
        assert _bits(eng.refine_info()[0]) == _bits(infos[k]), f"{form}: step {k}: info"


@pytest.mark.parametrize("form", FORMS + ["launch_cus_1"])
def test_engine_refine_pipeline_single_chain(form, monkeypatch, launch_cus):
    # launch_cus_1: the launch-shape decisions on "one CU".  (One chain is not more chains than
    # CUs, so the two-blocks-per-CU k_pnp_tri_ref is the batch test's launch_cus_1 form.)
    if form == "launch_cus_1":
        launch_cus(1)
    _run_forms(form, monkeypatch, None, N_STEPS)


@pytest.mark.parametrize("form", ["default", "graph", "launch_cus_1"])
def test_engine_refine_pipeline_batch(form, launch_cus):
    """Chain 0 of a 3-chain batch (starts 0, 1, 3 over 14 frames, 7 steps); the other chains run
    their own sequences and must end with status 0.  launch_cus_1: three chains on "one CU" take
    the two-blocks-per-CU build of the fused kernel."""
    from monocular_visual_odometry_va4mr_amd.synth import make_sequence
    fr11, K, opts, s0, snaps, infos, _ = pipeline_reference()
    fr = make_sequence("kitti", 14, seed=1)[0]
    assert np.array_equal(fr[:11], fr11)
    frames = torch.from_numpy(np.ascontiguousarray(fr)).cuda()
    starts = [0, 1, 3]
    if form == "launch_cus_1":
        launch_cus(1)
    eng = _engine(K, opts, batch=3, pnp_refine_iters=ITERS)
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
        info = eng.refine_info()
        assert _bits(info[0]) == _bits(infos[k]) and np.all(info[1:, 3] < info[1:, 2])
    assert (eng.statuses() == 0).all()


def test_engine_refine_with_the_fb_gate(monkeypatch):
    _run_forms("default", monkeypatch, 1.0, 5)


def test_engine_refine_option_off():
    """Absent, None and 0 are the same engine: no info buffer, the plain oracle's state."""
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    fr, K, opts, s0, snaps, _, plain = pipeline_reference()
    states = []
    for extra in ({}, {"pnp_refine_iters": None}, {"pnp_refine_iters": 0, "pnp_refine_ftol": 1e-8}):
        eng = _engine(K, opts, **extra)
        assert eng.pnp_refine_iters == 0 and eng._refine_info is None and eng.refine_info() is None
        _import(eng, 0, s0)
        for k in range(3):
            eng.step(fr[3 + k])
            _assert_chain(eng, 0, plain[k], f"{extra}: step {k}")
        torch.cuda.synchronize()
        states.append({k: eng.t[k].cpu().numpy().copy() for k in KEYS})
    for k in KEYS:
        assert np.array_equal(states[0][k], states[1][k]) and np.array_equal(states[0][k], states[2][k]), k
    for bad in ({"pnp_refine_iters": -1}, {"pnp_refine_iters": 101}, {"pnp_refine_iters": 2.5},
                {"pnp_refine_iters": 5, "pnp_refine_ftol": float("nan")}, {"pnp_refine_iters": 5, "pnp_refine_ftol": -1.0}):
        with pytest.raises(ValueError):
            Engine(K, dict(opts, **bad), 1241, 376, batch=1, ncap=64, pcap=64, fcap=4)


def test_dropin_class_and_runners_pass_the_option_through():
    from monocular_visual_odometry_va4mr_amd import run_dataset as RD
    from monocular_visual_odometry_va4mr_amd import run_sequence as RS
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    from monocular_visual_odometry_va4mr_amd.VisualOdometryPipeLine import VisualOdometryPipeLine
    fr, K, opts, _, _, _, _ = pipeline_reference()
    n = 5

    def drop_in(o):
        vo = VisualOdometryPipeLine(K, o, max_frames=32, landmark_capacity=4096, candidate_capacity=8192)
        vo.initialization(fr[0], fr[2])
        for k in range(n):
            vo.continuous_operation(fr[3 + k])
        return vo

    refined, plain = drop_in(dict(opts, pnp_refine_iters=ITERS)), drop_in(dict(opts))
    assert refined._eng.pnp_refine_iters == ITERS and plain._eng.pnp_refine_iters == 0
    eng = _engine(K, opts, pnp_refine_iters=ITERS)
    eng.bootstrap(fr[0][None], fr[2][None])
    for k in range(n):
        eng.step(fr[3 + k])
    e = eng.export_chain(0)
    assert e["status"] == 0 and len(e["transforms"]) == len(refined.transforms) == n + 2
    for (Ra, ta), (Rb, tb) in zip(e["transforms"], refined.transforms):
        assert np.array_equal(Ra, np.asarray(Rb)) and np.array_equal(ta.ravel(), np.asarray(tb).ravel())
    assert not np.array_equal(np.asarray(refined.transforms[-1][1]), np.asarray(plain.transforms[-1][1]))
    res = RD.run("synthetic-kitti", None, last_frame=7, plot=None, pnp_refine_iters=3, pnp_refine_ftol=1e-9)
    assert res["_vo"]._eng.pnp_refine_iters == 3 and res["_vo"]._eng.pnp_refine_ftol == 1e-9 and res["frames"] == 4
    seen = []

    class Recording(Engine):
        def __init__(self, K_, options, *a, **kw):
            super().__init__(K_, options, *a, **kw)
            seen.append((self.pnp_refine_iters, self.pnp_refine_ftol))

    rep = RS.run("kitti", 24, 2, overlap=4, engine_cls=Recording, pnp_refine_iters=3, pnp_refine_ftol=1e-9)
    assert rep is not None and seen and all(s == (3, 1e-9) for s in seen)
