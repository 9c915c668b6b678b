"""The cases of geom_cases.py reach what they are named for: asserted on the CPU oracle alone, so that
no case of test_gpu_geometry_edges.py / test_gpu_chain_status.py can go vacuous later (in the style of
test_lk_flags_ref.py).  Everything here runs without a GPU.

The constants of the kernels the cases aim at: k_pnp_ransac draws 32 hypotheses in its first round
and 64 in every later one (VO_PNP_CH1, HYP); k_essential<1> scores 24 and k_essential<2> 64 per
round (NH), so an iteration count above 64 means a second round in every form.
"""
import math

import numpy as np
import pytest

import geom_cases as GC

PNP_FIRST_ROUND = 32
ESS_ROUND = 64


@pytest.fixture(scope="module")
def pnp():
    c = GC.pnp_cases()
    return c, {k: GC.pnp_expect(*c[k], *GC.PNP_REF_OPTS) for k in GC.PNP_MAIN}


@pytest.fixture(scope="module")
def ess():
    c = GC.ess_cases()
    return c, {k: GC.ess_expect(*c[k], *GC.ESS_REF_OPTS) for k in GC.ESS_MAIN}


# ---------------------------------------------------------------------- PnP
def test_pnp_main_batch_covers_the_counts(pnp):
    c, _ = pnp
    counts = [len(c[k][0]) for k in GC.PNP_MAIN]
    for n in (0, 3, 4, 5, 6, 7, 8, 9, 12, 63, 64, 65, 255, 256, 257):
        assert n in counts
    assert counts.count(4) == 2 and max(counts) <= 320
    for names in GC.PNP_OTHER.values():
        assert all(k in c for k in names)


@pytest.mark.parametrize("n", [5, 6, 7, 8, 9, 12])
def test_pnp_few_clean_points_all_inliers(pnp, n):
    e = pnp[1][f"clean_{n}"]
    assert e["success"] and e["n_inl"] == n and e["mask"].all()
    assert 1 <= e["iters"] <= 3


@pytest.mark.parametrize("n", [5, 6, 8, 12])
def test_pnp_few_points_with_outliers_iterate(pnp, n):
    """several hypotheses of the first round are scored, drawn from n <= 12 indices: the serial tail
    of pnp_subsets (a repeated index drawn again) decides which"""
    e = pnp[1][f"small_outl_{n}"]
    assert e["success"] and 4 <= e["n_inl"] < n
    assert 1 < e["iters"] <= PNP_FIRST_ROUND
    # the draws replayed: hypotheses the result depends on (before the last iteration) repeated an
    # index and drew again, and the first round's 32 hypotheses need more than the 4 * 32 values
    # pnp_subsets generates ahead
    assert GC.pnp_subset_redraws(n, e["iters"]) > 0
    assert GC.pnp_subset_redraws(n, PNP_FIRST_ROUND) > 0


def test_pnp_four_points(pnp):
    assert pnp[1]["n4_solvable"]["success"] and pnp[1]["n4_solvable"]["n_inl"] == 4
    assert not pnp[1]["n4_identical"]["success"]
    assert pnp[1]["n0"]["mask"] is None and pnp[1]["n3"]["mask"] is None


def test_pnp_outlier_scenes_reach_later_rounds(pnp):
    e50, e80 = pnp[1]["outl50_300"], pnp[1]["outl80_300"]
    assert e50["success"] and e80["success"]
    assert PNP_FIRST_ROUND < e50["iters"] < 500          # a second round, ended by the adaptive count
    assert e80["iters"] == 500                           # every round up to iterationsCount
    for n in (63, 64, 65, 255, 256, 257):
        e = pnp[1][f"noisy_{n}"]
        assert e["success"] and 4 < e["n_inl"] < n


def test_pnp_random_image_points_fail_at_half_a_pixel():
    for name, (X, x) in GC.pnp_fail_cases().items():
        e = GC.pnp_expect(X, x, 100, 0.5, 0.99)
        assert not e["success"] and e["n_inl"] == 0 and not e["mask"].any(), name
        assert e["iters"] == 100, name


def test_pnp_random_image_points_at_8px_refit_on_four(pnp):
    """success with exactly the 4 sample points as inliers: the EPnP refit with m = 4"""
    for name in ("randimg_50", "randimg_300"):
        e = pnp[1][name]
        assert e["success"] and e["n_inl"] == 4 and e["iters"] == 500, name


def test_pnp_identical_and_planar(pnp):
    e = pnp[1]["identical_6"]
    assert not e["success"] and e["iters"] == 500        # the sh[2] <= 0 exit after every round
    for name, n in (("planar_8", 8), ("planar_100", 100)):
        X = pnp[0][name][0].astype(np.float64)
        assert np.linalg.matrix_rank(np.c_[X, np.ones(n)], tol=1e-4) == 3      # coplanar
        assert pnp[1][name]["success"] and pnp[1][name]["n_inl"] == n


def test_pnp_other_option_batches_are_mixed(pnp):
    c, _ = pnp
    for opts, names in GC.PNP_OTHER.items():
        ok = [GC.pnp_expect(*c[k], *opts)["success"] for k in names]
        assert any(ok) and not all(ok), opts


# ---------------------------------------------------------------------- E
def test_ess_main_batch_covers_the_counts(ess):
    c, _ = ess
    counts = [len(c[k][0]) for k in GC.ESS_MAIN]
    for n in (0, 1, 4, 5, 6, 7, 8, 9, 63, 64, 65, 257):
        assert n in counts
    assert max(counts) <= 320


@pytest.mark.parametrize("n", [5, 6, 7, 8, 9])
def test_ess_few_clean_points_all_inliers(ess, n):
    e = ess[1][f"clean_{n}"]
    assert e["ok"] and e["mask"].all() and len(e["mask"]) == n


def test_ess_below_five_points(ess):
    for n in (0, 1, 4):
        e = ess[1][f"n{n}"]
        assert not e["ok"] and not e["mask"].any() and len(e["mask"]) == n


def test_ess_outlier_scenes_reach_later_rounds_and_the_cap(ess):
    prob, _, max_iters = GC.ESS_REF_OPTS
    want = {}
    for pct in (30, 50, 60, 70):
        e = ess[1][f"outl{pct}_300"]
        assert e["ok"]
        want[pct] = GC.ransac_niters(prob, 300, int(e["mask"].sum()), 5, max_iters)
    assert 24 < want[30] < ESS_ROUND                      # a second round of k_essential<1> only
    assert ESS_ROUND < want[50] < 2 * ESS_ROUND + 24      # a few rounds in both forms
    assert 4 * ESS_ROUND < want[60] < max_iters
    assert want[70] >= max_iters                          # the max_iters cap


def test_ess_degenerate_scenes_are_ok(ess):
    for name in ("planar_200", "rotation_200", "identical_8"):
        assert ess[1][name]["ok"], name
    p0, p1 = ess[0]["rotation_200"]
    r = GC.recover_expect(ess[1]["rotation_200"]["E"], p0, p1)
    assert r["n_good"] < 20                               # recoverPose keeps few points without a baseline


@pytest.mark.parametrize("max_iters", [1, 50, 1000])
def test_ess_random_correspondences_are_ok(ess, max_iters):
    for n in (6, 8, 40):
        e = GC.ess_expect(*ess[0][f"random_{n}"], 0.99, 1.0, max_iters)
        assert e["ok"] and 5 <= e["mask"].sum() < n, (n, max_iters)


def test_ess_other_option_batches_change_the_result(ess):
    c, ref = ess
    differs = 0
    for opts, names in GC.ESS_OTHER.items():
        for k in names:
            e = GC.ess_expect(*c[k], *opts)
            assert e["ok"] == ref[k]["ok"]
            differs += not np.array_equal(e["mask"], ref[k]["mask"])
    assert differs >= 8


# ---------------------------------------------------------------------- recoverPose
def test_recover_cases():
    rc = GC.recover_cases()
    names = [r[0] for r in rc]
    counts = {r[0]: len(r[2]) for r in rc}
    for n in (0, 1, 255, 256, 257):
        assert counts[f"count_{n}"] == n
    assert sum(n.startswith("notE_") for n in names) == 8
    assert max(counts.values()) <= 320
    ex = {r[0]: GC.recover_expect(*r[1:]) for r in rc}
    # no point at all: the four counts tie at 0 and the first-of-equals rule alone picks (R1, t); the
    # points of the full scene pick another candidate, so the tie rule is what the case shows
    assert ex["count_0"]["n_good"] == 0 and np.isfinite(ex["count_0"]["R"]).all()
    assert not np.array_equal(ex["count_0"]["R"], ex["count_257"]["R"])
    # the swapped views pick other candidates than E does; -E, which takes recoverPose's det(U) < 0 /
    # det(V) < 0 sign fix-ups the other way, must describe the same pose
    other = sum(not np.array_equal(ex[n]["R"], ex[n[:-8]]["R"]) or not np.array_equal(ex[n]["t"], ex[n[:-8]]["t"])
                for n in names if n.endswith("_swapped"))
    assert other >= 3
    for n in names:
        if n.endswith("_neg"):
            assert ex[n]["n_good"] == ex[n[:-4]]["n_good"] and np.allclose(ex[n]["t"], ex[n[:-4]]["t"]), n
    # the 50-unit cut: some points of the scene pass, the ones beyond it do not
    e = ex["depth_cut"]
    assert 20 < e["n_good"] < 100 and e["n_good"] == e["mask"].sum()
    # an exactly skew E with zeros (t = (0.6, 0, 0.8), |t| = 1): its third singular value is exactly 0
    # and the one-sided Jacobi SVD leaves that column of U at zero, so recoverPose's "rotation" is
    # singular and t = 0 -- what the kernels must reproduce, not a pose
    name, E, _, _ = next(r for r in rc if r[0] == "infinity_skew_with_zeros")
    E = E.reshape(3, 3)
    assert np.array_equal(E, -E.T) and (E == 0).sum() == 5
    R = ex[name]["R"].reshape(3, 3)
    assert abs(np.linalg.det(R)) < 1e-12 and not ex[name]["t"].any() and ex[name]["n_good"] == 0
    # p0 == p1: the rays meet at infinity and the point is never counted
    assert not ex["infinity"]["mask"][:3].any() and ex["infinity"]["mask"].any()


# ---------------------------------------------------------------------- triangulatePoints
def test_tri_cases():
    P1, P2, x1, x2 = GC.tri_cases(1000)
    assert np.array_equal(P1[1], P2[1]) and np.array_equal(P1[2], P2[2]) and np.array_equal(x1[2], x2[2])
    assert not x1[4].any() and not x2[4].any()
    assert np.abs(x1[6]).max() == 1e6 and np.abs(P1[7]).max() > 1e6
    out = GC.tri_expect(P1[:16], P2[:16], x1[:16], x2[:16])
    assert np.isfinite(out).all()
    assert abs(out[3, 3]) < 1e-12 * np.abs(out[3, :3]).max()          # parallel rays: a point at infinity
    assert len({P1[i].tobytes() for i in range(1000)}) == 1000        # one camera pair per point


# ---------------------------------------------------------------------- Rodrigues
def test_rodrigues_cases_round_trip():
    from oracle import _olib as O
    vec = GC.rod_vectors()
    for name, v in vec.items():
        R = O.rodrigues(v)
        th = np.linalg.norm(v)
        if th < 2.220446049250313e-16:
            assert np.array_equal(R, np.eye(3)), name                  # theta < DBL_EPSILON
        else:
            assert not np.array_equal(R, np.eye(3)) or th < 1e-8, name
        r = O.rodrigues(R).ravel()
        assert np.isfinite(r).all(), name
        # the same rotation comes back (the vector itself up to the branch of theta and, at pi, the sign)
        assert np.allclose(O.rodrigues(r), R, atol=1e-9) or th < 1e-5, name
        rx, ry, rz = R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]
        s = math.sqrt((rx * rx + ry * ry + rz * rz) * 0.25)
        c = (np.trace(R) - 1) * 0.5
        if name.startswith("pi_") or name.startswith("pi-1e-7"):
            assert s < 1e-5 and c < 0, name                            # the fix-up branch near pi
        if name.startswith("pi-2e-5") or name.startswith("pi+1e-3"):
            assert s >= 1e-5 and c < 0, name                           # just outside it
        if name in ("norm_1e-08", "norm_5e-06"):
            assert s < 1e-5 and c > 0 and not r.any(), name            # the zero branch
        if name == "norm_2e-05":
            assert s >= 1e-5 and r.any()
    # the sign fix-ups: negative y, negative z, and the rz flip for the smallest |rx|
    signs = {tuple(np.sign(O.rodrigues(O.rodrigues(v)).ravel()).astype(int)) for k, v in vec.items() if k.startswith("pi_")}
    assert {(1, -1, 1), (1, 1, -1), (1, -1, -1), (1, 1, 1)} <= signs
    for name, m in GC.rod_matrices().items():
        assert np.isfinite(O.rodrigues(m)).all(), name
    m = GC.rod_matrices()
    for name in ("noisy", "2R", "rank2", "zero"):
        assert not np.allclose(m[name] @ m[name].T, np.eye(3), atol=1e-6), name    # the SVD has work to do
    for n in (1, 127, 128, 129):
        b = GC.rod_batch(vec.values(), n, n, (3,))
        assert b.shape == (n, 3) and np.array_equal(b[0], vec["zero"])


# ---------------------------------------------------------------------- ratio test
@pytest.mark.parametrize("ratio", [0.5, 0.8])
def test_ratio_cases(ratio):
    for d0, d1 in GC.ratio_ties(ratio)[:3]:
        assert float(np.float32(d0)) == ratio * float(np.float32(d1))   # an exact tie in double
    lo, hi = GC.ratio_ties(ratio)[3:]
    assert lo[0] < ratio * lo[1] < hi[0]
    kp0, kp1, idx, dist = GC.ratio_case(ratio, 5)
    assert kp0.shape[1] > max(GC.RATIO_NQ) and idx.shape[1] > max(GC.RATIO_NQ) and kp0.shape[1] != idx.shape[1]
    kept = []
    for b, nq in enumerate(GC.RATIO_NQ):
        p0, p1 = GC.ratio_expect(kp0[b], kp1[b], idx[b], dist[b], nq, ratio)
        kept.append(len(p0))
        assert len(p0) == len(p1) <= nq
    assert kept[0] == 0 and kept[2] > 20 and 100 < kept[3] < 700       # kept rows in all three 256-query passes
    i = np.arange(700)
    b = 3
    tie = (i % 5 == 4) & (i % 7 != 6) & (i % 11 != 10) & (i % 13 != 12)
    exact = tie & (dist[b, :700, 0].astype(np.float64) == ratio * dist[b, :700, 1].astype(np.float64))
    assert exact.sum() > 50                                             # ties that `<=` would keep
    assert ((idx[b, :700, 1] < 0) & (idx[b, :700, 0] >= 0)).sum() > 50
    assert (idx[b, :700] < 0).all(axis=1).sum() > 30
    assert (dist[b, :700] == GC.FLT_MAX).any()


# ---------------------------------------------------------------------- chain states
def test_initialize_from_matches_is_initialize():
    """oracle.initialize_from_matches on the ratio-test matches reproduces the recorded bootstrap of the
    reference class (first record of the golden run), i.e. what initialize gives; fewer matches take
    the other paths of the essential-matrix solver."""
    from oracle import cv2_oracle as cv
    from oracle import vo_pipeline_oracle as V
    b = GC.chain_base()
    g, s0 = b["g"], b["S"][0]
    R, t = s0.transforms[-1]
    assert np.array_equal(R, g["R"][0]) and np.array_equal(t, g["t"][0])
    assert s0.num_pts[0] == g["num_pts"][0] and len(s0.lm) == g["N"][0] and len(s0.cand) == g["P"][0]
    assert len(b["S"][2].lm) >= 12 and len(b["S"][2].cand) > 300
    # the bootstrap-status test's matches (malaga_c3): all of them give the recorded bootstrap, fewer
    # take the other paths of the essential-matrix solver
    m = GC.boot_base()
    n = len(m["p0"])
    assert n > max(GC.BOOT_TAKES)
    E, mask = cv.findEssentialMat(m["p0"][:3], m["p1"][:3], m["K"], method=cv.RANSAC, prob=0.99, threshold=1)
    assert E is None and not mask.any()                    # three matches: no model
    for k in (5, 6, 64, n):
        s = V.new_state(m["K"], m["opts"])
        V.initialize_from_matches(s, m["p0"][:k], m["p1"][:k], m["img1"])
        assert len(s.transforms) == 2 and len(s.lm) + len(s.cand) == s.num_pts[0] <= k
    g = m["g"]
    assert np.array_equal(s.transforms[-1][0], g["R"][0]) and np.array_equal(s.transforms[-1][1], g["t"][0])
    assert s.num_pts[0] == g["num_pts"][0] and len(s.lm) == g["N"][0] and len(s.cand) == g["P"][0]


def test_chain_table_is_what_the_oracle_does():
    b = GC.chain_base()
    frames = [b["fr"][b["next"] + j] for j in range(4)]
    for v, (what, stop) in GC.CHAIN_TABLE.items():
        rec = GC.chain_run(GC.chain_variant(b["S"][2], v), frames)
        if stop is None:
            assert all(r[0] == "ok" for r in rec), what
            continue
        at, exc, msg = stop
        assert all(r[0] == "ok" for r in rec[:at]) and rec[at][0] == "raise", what
        assert type(rec[at][1]) is exc and msg in str(rec[at][1]), what
    # chain 2 loses its three moved keypoints (and two more) in tracking, chain 3 fails inside PnP
    # with at least 8 points, chain 4's PnP "succeeds" on four inliers first
    r2 = GC.chain_run(GC.chain_variant(b["S"][2], 2), frames[:1])[0][2]
    assert len(r2["keypoints"]) < 8
    r3 = GC.chain_run(GC.chain_variant(b["S"][2], 3), frames[:1])[0][2]
    assert len(r3["keypoints"]) >= 8
    r4 = GC.chain_run(GC.chain_variant(b["S"][2], 4), frames[:1])[0][1]
    assert r4["num_pts"][-1] == 4 and len(r4["landmarks"]) < 8
    for name, (over, exc) in GC.GFTT_TABLE.items():
        import copy
        c = copy.deepcopy(b["S"][2])
        c.opts = dict(c.opts, **over)
        rec = GC.chain_run(c, frames[:1])
        assert rec[0][0] == "raise" and type(rec[0][1]) is exc, name
        assert len(rec[0][2]["transforms"]) == len(b["S"][2].transforms)
