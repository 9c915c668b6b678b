"""The designs of state_cases.py do on the oracle what their table rows say: asserted on the CPU
oracle alone, so that no case of test_gpu_state_edges.py can go vacuous later (in the style of
test_geom_cases_ref.py).  Every condition below is computed from what the oracle calls return
(V.track, cv.solvePnPRansac, triangulate_candidates and the gate's restatement), not from the table;
deleting or thinning a design fails a test here.

The widths the designs aim at: track_compact_block, pnp_apply_block and tri_append walk 256 rows
per pass; pnp_apply_split walks four 64-lane sub-chunks per 256-row pass; tri_solve strides by 256
threads in the one-block forms and by TRI_SPLIT x 256 = 2048 in the three-launch vo_triangulate.
"""
import copy

import numpy as np
import pytest

import state_cases as SC

PASS, SUB, SPLIT_STRIDE = 256, 64, 8 * 256


@pytest.fixture(scope="module")
def D():
    return {d["name"]: d for d in SC.designs()}


def _rows(a):
    return [r.tobytes() for r in np.ascontiguousarray(a)]


def _distinct(a):
    r = _rows(a)
    return len(set(r)) == len(r)


def _live(D):
    return [d for d in D.values() if not d["row"]["stopped"]]


# ---------------------------------------------------------------------- the composition itself
def test_composition_is_the_step():
    """compose() on the unmodified state is V.step up to feature adding: the same landmarks,
    keypoints, inlier / outlier lists and pose, and step's candidates start with compose's."""
    b = SC.base()
    c = SC.compose(b["s"], b["next_img"])
    t = b["stepped"]
    R, tt = t.transforms[-1]
    assert np.array_equal(c["R"], R) and np.array_equal(c["t"], tt)
    assert np.array_equal(c["landmarks"], t.lm) and np.array_equal(c["keypoints"], t.kp)
    assert np.array_equal(c["inliers"], t.inl_pts) and np.array_equal(c["outliers"], t.outl_pts)
    n = len(c["cand"])
    assert 1 < n < len(t.cand)
    assert np.array_equal(c["cand"], t.cand[:n]) and np.array_equal(c["cand_first"], t.cand_first[:n])
    assert np.array_equal(c["cand_tau"], t.cand_tau[:n])
    assert len(c["landmarks"]) > len(c["inliers"])                              # it triangulated: landmarks were appended
    # with the gate's restatement at None: the same bits
    import test_tri_gate_ref as TG
    s = copy.deepcopy(b["s"])
    R2, t2, _ = SC.compose_to_pnp(s, b["next_img"])
    TG.triangulate_candidates_ref(s, R2, t2, None)
    assert np.array_equal(s.lm, t.lm) and np.array_equal(s.cand, t.cand[:n])


def test_base_has_both_pose_orders():
    """six poses, 0 and 1 C-ordered and the later ones F-ordered (the p >= 2 summation order of
    pose_inverse / depth_of); tau 0..3 reach the triangulation, 4 and 5 are frame-gated"""
    s = SC.base()["s"]
    assert len(s.transforms) == 6 and s.opts["min_baseline_frames"] == 2
    for p, (R, _) in enumerate(s.transforms):
        assert R.flags["C_CONTIGUOUS"] == (p < 2) and R.flags["F_CONTIGUOUS"] == (p >= 2), p
    R, _ = SC.base()["target"]
    assert R.flags["F_CONTIGUOUS"] and not R.flags["C_CONTIGUOUS"]


def test_exports_exist():
    from monocular_visual_odometry_va4mr_amd import _lib as L
    for name in ("vo_track", "vo_track_lk", "vo_pnp", "vo_triangulate", "vo_pnp_triangulate", "vo_filter_pnp_triangulate",
                 "vo_pnp_gated", "vo_triangulate_gated", "vo_pnp_triangulate_gated", "vo_filter_pnp_triangulate_gated",
                 "vo_pyr_build", "vo_set_launch_cus"):
        assert name in L.exported_symbols(), name


# ---------------------------------------------------------------------- the pool and the tracking
def test_pool_is_what_the_designs_need():
    p = SC.pool()
    assert len(p["pts"]) <= 6000 and _distinct(p["pts"])
    trk = np.flatnonzero(p["ok"])
    assert len(trk) > 3000 and len(p["lost"]) > 512
    # off-image points are lost, and so are some points on the image
    off = (p["pts"][:, 0] < 0) | (p["pts"][:, 1] < 0) | (p["pts"][:, 0] >= SC.IMG_W) | (p["pts"][:, 1] >= SC.IMG_H)
    assert off.sum() >= 300 and not p["ok"][off].any() and (~off[p["lost"]]).sum() > 100
    # two different frames: a tracked position is not its input, so a copy of the wrong source shows
    assert not (p["q"][trk] == p["pts"][trk]).all(axis=1).any()
    for c, (asked, got) in p["yield_"].items():
        assert got >= 0.8 * asked, (c, asked, got)


def test_tracking_lays_down_the_designed_patterns(D):
    """V.track on every design keeps exactly the rows the table says, with the pool's tracked
    positions (LK's result for a point does not depend on the other points)."""
    p = SC.pool()
    for d in _live(D):
        row, st, tr = d["row"], d["state"], d["tracked"]
        keep = ~row["lm_lost"]
        assert np.array_equal(p["ok"][d["lm_idx"]], keep), d["name"]
        assert np.array_equal(tr.kp, p["q"][d["lm_idx"][keep]]) and np.array_equal(tr.lm, st.lm[keep]), d["name"]
        assert d["L1"] == keep.sum()
        if row["C0"] > 1:
            ckeep = ~row["c_lost"]
            assert np.array_equal(p["ok"][d["c_idx"]], ckeep), d["name"]
            assert np.array_equal(tr.cand, p["q"][d["c_idx"][ckeep]]), d["name"]
            assert np.array_equal(tr.cand_first, st.cand_first[ckeep]) and np.array_equal(tr.cand_tau, st.cand_tau[ckeep])
            assert d["C1"] == ckeep.sum()
        else:
            assert np.array_equal(tr.cand, st.cand) and d["C1"] == row["C0"]                # Q7


def test_landmark_counts(D):
    live = _live(D)
    L1 = {d["L1"] for d in live}
    assert {8, 64, 65, 256, 257} <= L1 and max(L1) > 2 * PASS
    lost = {d["name"]: np.flatnonzero(~SC.pool()["ok"][d["lm_idx"]]) for d in live}
    L0 = {d["name"]: d["row"]["L0"] for d in live}
    assert any(L0[n] == 9 and len(lost[n]) == 1 and D[n]["L1"] == 8 for n in L0)
    assert any(L0[n] == 256 and len(lost[n]) == 0 for n in L0)
    assert any(L0[n] == 257 and lost[n].tolist() == [256] for n in L0)                      # the lone 257th element
    assert any(L0[n] == 513 and lost[n].tolist() == list(range(PASS)) for n in L0)          # the whole first pass


def _sub_chunks(mask):
    """inlier count and size of every 64-lane sub-chunk"""
    return [(int(mask[i:i + SUB].sum()), len(mask[i:i + SUB])) for i in range(0, len(mask), SUB)]


def test_pnp_masks(D):
    """the oracle's solvePnPRansac returns exactly the designed mask, and among the chains are the
    patterns the two inlier splits depend on"""
    live = _live(D)
    for d in live:
        assert np.array_equal(d["mask"], d["row"]["mask"]), d["name"]
        assert len(d["mask"]) == d["L1"] and len(d["plain"]["inliers"]) == d["mask"].sum()
        assert np.array_equal(d["plain"]["inliers"], d["tracked"].kp[d["mask"]])
        assert np.array_equal(d["plain"]["outliers"], d["tracked"].kp[~d["mask"]])
        # the current pose is what that call returned, not the target it was designed with
        assert not np.array_equal(d["t"], SC.base()["target"][1]) and np.allclose(d["t"], SC.base()["target"][1], atol=1e-4)
    masks = [d["mask"] for d in live]
    assert any(m.all() for m in masks)                                                      # all inliers
    assert any(len(m) >= SUB and np.array_equal(m, np.arange(len(m)) % 2 == 0) for m in masks)          # alternating
    subs = [_sub_chunks(m) for m in masks]
    # a sub-chunk with no inlier, in a pass that has inliers
    assert any(any(not m[i:i + SUB].any() and m[i // PASS * PASS:(i // PASS + 1) * PASS].any() for i in range(0, len(m) - SUB + 1, SUB))
               for m in masks)
    assert any(any(a == (SUB, SUB) and 0 < b[0] < b[1] for a, b in zip(s, s[1:])) or
               any(b == (SUB, SUB) and 0 < a[0] < a[1] for a, b in zip(s, s[1:])) for s in subs)        # only inliers beside a mixed one
    assert any(len(m) > PASS and not m[:PASS].any() and m[PASS:].all() for m in masks)      # a whole pass of outliers, then inliers
    assert any(np.flatnonzero(~m).tolist() == [SUB - 1] and len(m) > SUB for m in masks)    # the only outlier at lane 63
    assert any(np.flatnonzero(~m).tolist() == [len(m) - 1] and len(m) % SUB == 1 for m in masks)        # ... at the last index, alone in its sub-chunk
    assert any(len(m) == PASS + 1 and not m[PASS] and m[:PASS].any() for m in masks)        # a lone outlier in the last pass


def test_candidate_counts_and_losses(D):
    live = _live(D)
    assert {0, 1, 2} <= {d["row"]["C0"] for d in live}
    one = next(d for d in live if d["row"]["C0"] == 1)
    for k in ("cand", "cand_first", "cand_tau"):                                            # untouched and untriangulated
        assert np.array_equal(one["plain"][k], getattr(one["state"], k)) and np.array_equal(one["gated"][k], one["plain"][k])
    assert len(one["plain"]["landmarks"]) == one["mask"].sum()
    two = next(d for d in live if d["row"]["C0"] == 2)
    assert two["C1"] == 1 and len(two["plain"]["cand"]) == 1 and len(two["plain"]["landmarks"]) == two["mask"].sum()
    assert np.array_equal(two["plain"]["cand"], two["tracked"].cand)
    assert {255, 256, 257, 513} <= {d["C1"] for d in live}
    lost = [np.flatnonzero(~SC.pool()["ok"][d["c_idx"]]) for d in live if d["row"]["C0"] > 1]
    C0 = [d["row"]["C0"] for d in live if d["row"]["C0"] > 1]
    assert any(len(l) == 0 and n >= PASS - 1 for l, n in zip(lost, C0))                     # none
    assert any(n > 2 * PASS and l.tolist() == list(range(1, n, 2)) for l, n in zip(lost, C0))          # alternating
    assert any(n > PASS and l.tolist() == list(range(PASS)) for l, n in zip(lost, C0))      # the whole first pass
    assert any(n > PASS and l.tolist() == [n - 1] for l, n in zip(lost, C0))                # only the last index


def _check_against_reference(d):
    """the class letters account for what the two reference functions did with the tracked candidates"""
    cls, tr = d["classes"], d["tracked"]
    n = {c: int((cls == c).sum()) for c in "FSADG"}
    L2 = int(d["mask"].sum())
    assert d["gated"]["info"] == [n["A"] + n["D"] + n["G"], n["D"], n["G"], n["A"]], d["name"]
    kept = np.isin(cls, list("FSD"))
    for snap, app in ((d["plain"], np.isin(cls, list("AG"))), (d["gated"], cls == "A")):
        assert np.array_equal(snap["cand"], tr.cand[kept]) and np.array_equal(snap["cand_first"], tr.cand_first[kept])
        assert np.array_equal(snap["cand_tau"], tr.cand_tau[kept])
        assert len(snap["landmarks"]) == L2 + app.sum() <= SC.NCAP
        assert np.array_equal(snap["keypoints"][L2:], tr.cand[app])
        assert np.array_equal(snap["keypoints"][:L2], tr.kp[d["mask"]]) and np.array_equal(snap["landmarks"][:L2], tr.lm[d["mask"]])
    # the gated landmarks are the plain ones minus the G rows, in order
    sel = (cls == "A")[np.isin(cls, list("AG"))]
    assert np.array_equal(d["gated"]["landmarks"][L2:], d["plain"]["landmarks"][L2:][sel])
    return n


def test_class_patterns(D):
    live = [d for d in _live(D) if d["classes"] is not None]
    assert len(live) >= 6
    counts = {}
    for d in live:
        assert np.array_equal(d["classes"], d["row"]["classes"]), d["name"]
        counts[d["name"]] = _check_against_reference(d)
    cl = {d["name"]: d["classes"] for d in live}
    # every candidate appended: nC becomes 0
    assert any((c == "A").all() and len(D[n]["plain"]["cand"]) == 0 and len(D[n]["gated"]["cand"]) == 0 for n, c in cl.items())
    # only F and S: the list of pass 1 is empty
    assert any(np.isin(c, list("FS")).all() and "F" in c and "S" in c and D[n]["gated"]["info"][0] == 0 and len(c) == PASS
               for n, c in cl.items())
    # A only at the last index of a 257-candidate chain
    assert any(len(c) == PASS + 1 and np.flatnonzero(c == "A").tolist() == [PASS] and "G" not in c and "D" in c for n, c in cl.items())
    # a pass of A, a pass of retained ones, a partial pass of G only
    assert any(len(c) > 2 * PASS and (c[:PASS] == "A").all() and np.isin(c[PASS:2 * PASS], list("FSD")).all() and
               "D" in c[PASS:2 * PASS] and (c[2 * PASS:] == "G").all() and 1 < len(c) - 2 * PASS < PASS for n, c in cl.items())
    # a random mix of all five with at least 40 of each and every tau
    mix = [n for n, c in cl.items() if all((c == k).sum() >= 40 for k in "FSADG")]
    assert mix and any(set(D[n]["tracked"].cand_tau.ravel().tolist()) == {0.0, 1.0, 2.0, 3.0, 4.0, 5.0} for n in mix)
    for n in mix:                                            # both pose orders on the past pose of triangulated candidates
        tau = D[n]["tracked"].cand_tau.ravel()[np.isin(cl[n], list("ADG"))]
        assert (tau < 2).any() and (tau >= 2).any()


def test_long_list(D):
    """more than 2048 candidates reach triangulatePoints in one chain (a second round of the
    three-launch form's stride), more than 9 x 256 (a tenth round of the one-block forms'), of the
    classes A, D and G only"""
    d = max(_live(D), key=lambda d: d["C1"])
    m = d["gated"]["info"][0]
    assert m > SPLIT_STRIDE and m > 9 * PASS and m == d["C1"] <= SC.PCAP
    assert set(d["classes"].tolist()) == {"A", "D", "G"}
    assert all((d["classes"] == c).sum() > 300 for c in "ADG")


def test_stopped_chain_is_the_random_mix(D):
    s, m = D["stopped"], D["l600_c513_mix"]
    assert s["row"]["stopped"] and SC.STOP_STATUS != 0 and SC.NAMES[SC.STOPPED] == "stopped"
    assert s["state"] is m["state"] and len(m["state"].cand) > 2 * PASS and len(m["state"].lm) > 2 * PASS
    assert [d["name"] for d in SC.designs()] == list(SC.NAMES)


def test_force_cases():
    """vo_triangulate(force = 1)'s reference: V.triangulate_candidates called directly appends the
    single A candidate and leaves the chain without candidates alone"""
    (s1, R1, t1, a1), (s0, R0, t0, a0) = SC.force_cases()
    assert len(s1.cand) == 1 and len(a1.cand) == 0 and len(a1.lm) == len(s1.lm) + 1
    assert np.array_equal(a1.kp[-1], s1.cand[0]) and np.array_equal(a1.lm[:-1], s1.lm)
    assert len(s0.cand) == 0 and len(a0.cand) == 0 and np.array_equal(a0.lm, s0.lm) and len(s0.lm) == 8


def test_rows_are_distinct_and_fit(D):
    """no duplicate rows anywhere (an order mistake between equal rows could hide), and every count
    fits the engine the GPU half creates"""
    for d in _live(D):
        st, tr = d["state"], d["tracked"]
        for a in (st.lm, st.kp, tr.kp, d["plain"]["landmarks"], d["plain"]["keypoints"], d["gated"]["landmarks"]):
            assert _distinct(a), d["name"]
        if len(st.cand):
            for a in (st.cand, st.cand_first, tr.cand, tr.cand_first, np.c_[st.cand, st.cand_first]):
                assert _distinct(a), d["name"]
        assert len(st.lm) <= SC.NCAP and len(st.cand) <= SC.PCAP and len(st.transforms) + 1 < SC.FCAP
        assert len(d["plain"]["landmarks"]) <= SC.NCAP
    # ragged counts side by side
    assert len({d["row"]["L0"] for d in _live(D)}) >= 7 and len({d["row"]["C0"] for d in _live(D)}) >= 8
