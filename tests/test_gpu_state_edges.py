"""The step's ordered compactions and appends at chunk edges: the designs of state_cases.py as the
chains of one engine (ragged counts side by side), run through every launch form of the step's
state machinery over the C ABI and compared bit for bit with the composition of oracle calls
(V.track, cv.solvePnPRansac, the inlier filter, the inversion, V.triangulate_candidates or the
gate's restatement at 2 px).  test_state_cases_ref.py proves on the CPU that every design does what
its name says.

What reaches what:
  deferred   vo_track_lk + vo_filter_pnp_triangulate   track_compact_block inside k_pnp_tri<1>,
                                                       pnp_apply_split, the one-block triangulation
  in_track   vo_track + vo_pnp_triangulate             k_track_compact
  separate   vo_track + vo_pnp + vo_triangulate        pnp_apply_block (k_pnp_fused), k_tri_gate /
                                                       k_tri_solve / k_tri_append
  cus = 1    the same three with vo_set_launch_cus(1)  k_pnp_tri<VO_PNP_WPE>, k_pnp_fused<VO_PNP_WPE>,
                                                       the one-block k_triangulate
  gated      all six through the _gated entry points   the tacc == 2 instantiations, the counters

Which design would change its expected result if a pass width or a prefix count were off by one:
  track_compact_block   l257_c256_FS: 257 landmarks of which only index 256 is lost (the lone
                        element of the second pass); l257_c257_lastA: that lone element kept;
                        l513_c552_AretG: the whole first pass lost and a lone 513th element kept
  pnp_apply_split       l256_c255_allA: sub-chunk 1 of the first pass has no inlier, sub-chunk 2
                        only inliers; l65_c2: the only outlier alone in its sub-chunk
  pnp_apply_block       l600_c513_mix: a whole 256-pass of outliers, then inliers
  tri_solve's stride    l64_c2310_long: m = 2310 > 2048 listed candidates (a second round of the
                        three-launch form, a tenth of the one-block forms)
  tri_append (plain)    l256_c255_allA: every candidate appended, nC becomes 0; l257_c257_lastA:
                        the only appended one is the lone element of the second pass
  tri_append (gated)    l513_c552_AretG: a pass of A, a pass of retained ones, a partial pass of G
                        only, which must advance neither the landmark scan nor the kept count
"""
import ctypes as C

import numpy as np
import pytest

import state_cases as SC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT_KEYS = ("lm_X", "lm_kp", "c_kp", "c_first", "c_tau", "inl_kp", "outl_kp")
STATE_KEYS = ("status", "nL", "nC", "nF", "nInl", "nOutl", "lm_X", "lm_kp", "c_kp", "c_first", "c_tau", "inl_kp", "outl_kp",
              "pose_R", "pose_t", "num_pts")
FORMS = ("deferred", "in_track", "separate")


def _engine(batch):
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    b = SC.base()
    eng = Engine(b["K"], b["opts"], SC.IMG_W, SC.IMG_H, batch=batch, ncap=SC.NCAP, pcap=SC.PCAP, fcap=SC.FCAP)
    for k in SENT_KEYS:
        eng.t[k].fill_(SC.SENT_I32 if k == "c_tau" else float(SC.SENT_F32))
    return eng


def _import(eng, b, s, extra_pose=None):
    tf = list(s.transforms) + ([extra_pose] if extra_pose is not None else [])
    eng.import_chain(b, landmarks=s.lm, keypoints=s.kp, cand=s.cand, cand_first=s.cand_first, cand_tau=s.cand_tau,
                     transforms=tf, num_pts=s.num_pts, prev_img=s.prev_img)
    if extra_pose is not None:
        eng.t["nF"][b] -= 1                    # the pose being triangulated sits in slot nF, not yet counted


def _snapshot(eng):
    torch.cuda.synchronize()
    return {k: eng.t[k].cpu().numpy().copy() for k in STATE_KEYS}


def _check(rc, what):
    assert rc == 0, f"{what} returned {rc}"


def _launch(eng, form, tg):
    lib, pd, po, ps, st, prev = eng.lib, eng._pd, eng._po, eng._ps, eng.stream, eng.prev
    tol = C.c_double(1e-10)
    if form == "deferred":
        _check(lib.vo_track_lk(pd, po, ps, prev, st), "vo_track_lk")
        if tg is None:
            _check(lib.vo_filter_pnp_triangulate(pd, po, ps, st), "vo_filter_pnp_triangulate")
        else:
            _check(lib.vo_filter_pnp_triangulate_gated(pd, po, ps, 0, tol, None, tg, st), "vo_filter_pnp_triangulate_gated")
    elif form == "in_track":
        _check(lib.vo_track(pd, po, ps, prev, st), "vo_track")
        if tg is None:
            _check(lib.vo_pnp_triangulate(pd, po, ps, st), "vo_pnp_triangulate")
        else:
            _check(lib.vo_pnp_triangulate_gated(pd, po, ps, 0, tol, None, tg, st), "vo_pnp_triangulate_gated")
    else:
        _check(lib.vo_track(pd, po, ps, prev, st), "vo_track")
        if tg is None:
            _check(lib.vo_pnp(pd, po, ps, st), "vo_pnp")
            _check(lib.vo_triangulate(pd, po, ps, 0, st), "vo_triangulate")
        else:
            _check(lib.vo_pnp_gated(pd, po, ps, 0, tol, None, tg, st), "vo_pnp_gated")
            _check(lib.vo_triangulate_gated(pd, po, ps, 0, tg, st), "vo_triangulate_gated")


def _assert_sentinels(after, b, L0, C0, what):
    """nothing outside the live range is written: rows at and past max(count before, count after)"""
    nL, nC, nI, nO = (int(after[k][b]) for k in ("nL", "nC", "nInl", "nOutl"))
    hl, hc = max(L0, nL), max(C0, nC)
    assert (after["lm_X"][b, hl:] == SC.SENT_F32).all() and (after["lm_kp"][b, hl:] == SC.SENT_F32).all(), f"{what}: landmark rows past {hl}"
    assert (after["c_kp"][b, hc:] == SC.SENT_F32).all() and (after["c_first"][b, hc:] == SC.SENT_F32).all() and \
        (after["c_tau"][b, hc:] == SC.SENT_I32).all(), f"{what}: candidate rows past {hc}"
    assert (after["inl_kp"][b, nI:] == SC.SENT_F32).all(), f"{what}: inlier rows past {nI}"
    assert (after["outl_kp"][b, nO:] == SC.SENT_F32).all(), f"{what}: outlier rows past {nO}"


def _assert_state(after, b, exp, what):
    """landmarks, keypoints and the three candidate arrays of chain b against a snapshot"""
    nL, nC = int(after["nL"][b]), int(after["nC"][b])
    assert nL == len(exp["landmarks"]), f"{what}: nL {nL}, expected {len(exp['landmarks'])}"
    assert nC == len(exp["cand"]), f"{what}: nC {nC}, expected {len(exp['cand'])}"
    for key, name in (("lm_X", "landmarks"), ("lm_kp", "keypoints"), ("c_kp", "cand"), ("c_first", "cand_first")):
        got = after[key][b, :len(exp[name])]
        if not np.array_equal(got, exp[name]):
            bad = np.flatnonzero((got != exp[name]).any(axis=1))
            raise AssertionError(f"{what}: {name} differs in {len(bad)} rows, first at {bad[:4].tolist()}")
    assert np.array_equal(after["c_tau"][b, :nC], exp["cand_tau"].ravel().astype(np.int32)), f"{what}: cand_tau"


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("cus", [0, 1])
@pytest.mark.parametrize("form", FORMS)
def test_designed_step(form, cus, gated, launch_cus):
    from monocular_visual_odometry_va4mr_amd import _lib as L
    assert SC.STOP_STATUS == L.ST_PNP_FAILED
    D = SC.designs()
    B = len(D)
    eng = _engine(B)
    for b, d in enumerate(D):
        _import(eng, b, d["state"])
    eng.t["status"][SC.STOPPED] = SC.STOP_STATUS
    nxt = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(SC.base()["next_img"], (B, SC.IMG_H, SC.IMG_W)))).cuda()
    eng.build_pyramid(nxt, 1 - eng.prev)
    before = _snapshot(eng)
    for b, d in enumerate(D):                                       # the import itself kept to its rows
        hl, hc = d["row"]["L0"], d["row"]["C0"]
        assert (before["lm_X"][b, hl:] == SC.SENT_F32).all() and (before["c_tau"][b, hc:] == SC.SENT_I32).all()
    info = tg = None
    if gated:
        info = torch.full((B, 4), SC.ISENT, dtype=torch.int32, device="cuda")
        tri = L.VoTriOpts(SC.MAX_ERR, info.data_ptr())
        tg = C.byref(tri)
    if cus:
        launch_cus(cus)
    _launch(eng, form, tg)
    after = _snapshot(eng)
    info = None if info is None else info.cpu().numpy()
    for b, d in enumerate(D):
        what = f"{form} cus={cus} {'gated' if gated else 'plain'}: chain {b} {d['name']}"
        print(what, "status", after["status"][b], "nL nC nInl nOutl", [int(after[k][b]) for k in ("nL", "nC", "nInl", "nOutl")],
              "info", None if info is None else info[b].tolist())
        if d["row"]["stopped"]:
            # every array, count and pose as imported, and its counters' row as pre-filled
            assert after["status"][b] == SC.STOP_STATUS, what
            for k in STATE_KEYS:
                assert np.array_equal(after[k][b], before[k][b]), f"{what}: {k} changed"
            if gated:
                assert (info[b] == SC.ISENT).all(), f"{what}: info {info[b].tolist()}"
            continue
        exp = d["gated" if gated else "plain"]
        assert after["status"][b] == 0, f"{what}: status {after['status'][b]}"
        _assert_state(after, b, exp, what)
        nI, nO, nF = int(after["nInl"][b]), int(after["nOutl"][b]), int(after["nF"][b])
        assert nI == len(exp["inliers"]) and nO == len(exp["outliers"]), f"{what}: nInl {nI} nOutl {nO}"
        assert np.array_equal(after["inl_kp"][b, :nI], exp["inliers"]), f"{what}: inliers"
        assert np.array_equal(after["outl_kp"][b, :nO], exp["outliers"]), f"{what}: outliers"
        assert nF == before["nF"][b] == len(d["state"].transforms), f"{what}: nF"
        assert np.array_equal(after["pose_R"][b, nF], np.asarray(exp["R"]).reshape(9)), f"{what}: R in slot nF"
        assert np.array_equal(after["pose_t"][b, nF], np.asarray(exp["t"]).reshape(3)), f"{what}: t in slot nF"
        assert np.array_equal(after["pose_R"][b, :nF], before["pose_R"][b, :nF]) and \
            np.array_equal(after["pose_t"][b, :nF], before["pose_t"][b, :nF]) and \
            np.array_equal(after["num_pts"][b], before["num_pts"][b]), f"{what}: earlier poses"
        _assert_sentinels(after, b, d["row"]["L0"], d["row"]["C0"], what)
        if gated:
            # the four counters; a chain that does not triangulate (C <= 1) reports four zeros
            assert info[b].tolist() == exp["info"], f"{what}: info {info[b].tolist()}, expected {exp['info']}"
            if d["C1"] <= 1:
                assert exp["info"] == [0, 0, 0, 0]


@pytest.mark.parametrize("cus", [0, 1])
def test_forced_triangulation(cus, launch_cus):
    """vo_triangulate(force = 1) on a chain with one candidate (an A: appended, nC becomes 0) and on
    one with none, against V.triangulate_candidates called directly; cus = 0: k_tri_gate /
    k_tri_solve / k_tri_append, cus = 1: the one-block k_triangulate.  Without force the same
    chains are left alone (:366)."""
    cases = SC.force_cases()
    for force in (1, 0):
        eng = _engine(len(cases))
        for b, (s, R, t, _) in enumerate(cases):
            _import(eng, b, s, extra_pose=(R, t))
        before = _snapshot(eng)
        if cus:
            launch_cus(cus)
        _check(eng.lib.vo_triangulate(eng._pd, eng._po, eng._ps, force, eng.stream), "vo_triangulate")
        after = _snapshot(eng)
        for b, (s, R, t, want) in enumerate(cases):
            what = f"force={force} cus={cus}: chain {b}"
            assert after["status"][b] == 0, what
            if not force:
                for k in STATE_KEYS:
                    assert np.array_equal(after[k][b], before[k][b]), f"{what}: {k} changed"
                continue
            exp = dict(landmarks=np.asarray(want.lm), keypoints=np.asarray(want.kp), cand=np.asarray(want.cand).reshape(-1, 2),
                       cand_first=np.asarray(want.cand_first).reshape(-1, 2), cand_tau=np.asarray(want.cand_tau))
            _assert_state(after, b, exp, what)
            assert (after["lm_X"][b, len(want.lm):] == SC.SENT_F32).all() and (after["lm_kp"][b, len(want.lm):] == SC.SENT_F32).all(), what
            assert (after["c_kp"][b, len(s.cand):] == SC.SENT_F32).all() and (after["c_tau"][b, len(s.cand):] == SC.SENT_I32).all(), what
            for k in ("pose_R", "pose_t", "nF", "inl_kp", "outl_kp", "nInl", "nOutl"):
                assert np.array_equal(after[k][b], before[k][b]), f"{what}: {k} changed"
