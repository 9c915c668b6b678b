"""The batched geometry primitives of the C ABI against the oracle, per problem: B > 1, ragged counts,
scratch at exactly the documented minimum, every output pre-filled with a sentinel.

The cases are those of geom_cases.py (test_geom_cases_ref.py shows on the CPU what each reaches).
Every batch runs a second time in reversed chain order, and every problem's outputs must be the same
in both: a chain's result does not depend on its slot.  All comparisons are bit for bit, with NaNs
compared by position (geom_cases.same_bits).
"""
import numpy as np
import pytest

import geom_cases as GC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CAP = 320
_EXPECT = {}          # (kind, case, options) -> the oracle's result, shared by the launch forms


def _same_outputs(a, b):
    """every output of one problem in two launches, under the NaN rule (also what no oracle result is
    compared with: the pose of a failed PnP, E without a model, rows past the count)"""
    assert a.keys() == b.keys()
    for k in a:
        if a[k] is None or isinstance(a[k], int):
            same = a[k] == b[k]
        elif a[k].dtype.kind == "f":
            same = GC.same_bits(a[k], b[k])
        else:
            same = np.array_equal(a[k], b[k])
        if not same:
            return False
    return True


def _expect(kind, fn, name, args, opts):
    key = (kind, name, opts)
    if key not in _EXPECT:
        _EXPECT[key] = fn(*args, *opts)
    return _EXPECT[key]


# ---------------------------------------------------------------------- vo_pnp_ransac
@pytest.fixture(scope="module")
def pnp_cases():
    c = GC.pnp_cases()
    c.update({"fail_" + k: v for k, v in GC.pnp_fail_cases().items()})
    return c


def _check_pnp(names, cases, opts):
    problems = [cases[k] for k in names]
    fwd = GC.gpu_pnp(problems, *opts, CAP)
    rev = GC.gpu_pnp(problems[::-1], *opts, CAP)[::-1]
    for k, (X, x), g, r in zip(names, problems, fwd, rev):
        n = len(X)
        assert _same_outputs(g, r), f"{k} {opts}: the outputs depend on the chain's slot"
        e = _expect("pnp", GC.pnp_expect, k, (X, x), opts)
        for out, what in ((g, "forward"), (r, "reversed")):
            tag = f"{k} {opts} {what}"
            assert (out["mask"][n:] == GC.SENT_U8).all(), tag + ": mask rows past the count written"
            assert out["success"] == e["success"] and out["n_inl"] == e["n_inl"], tag
            if n < 4:
                assert (out["mask"] == GC.SENT_U8).all(), tag
                assert (out["rvec"] == GC.SENT_F64).all() and (out["tvec"] == GC.SENT_F64).all(), tag
            elif not e["success"]:
                assert not out["mask"][:n].any(), tag
            else:
                assert np.array_equal(out["mask"][:n], e["mask"]), tag
                assert GC.same_bits(out["rvec"], e["rvec"]) and GC.same_bits(out["tvec"], e["tvec"]), tag


def test_pnp_ransac_batch_reference_options(pnp_cases):
    """One launch at the reference's options over every count and scene kind: n < 4, n == 4 (solvable
    and not), the serial tail of pnp_subsets at small n, second and later hypothesis rounds, the
    failure exit after every round, the EPnP refit on four points."""
    _check_pnp(GC.PNP_MAIN, pnp_cases, GC.PNP_REF_OPTS)


def test_pnp_ransac_batch_all_fail(pnp_cases):
    names = ["fail_" + k for k in GC.pnp_fail_cases()]
    _check_pnp(names, pnp_cases, (100, 0.5, 0.99))


@pytest.mark.parametrize("opts", list(GC.PNP_OTHER))
def test_pnp_ransac_batch_other_options(pnp_cases, opts):
    _check_pnp(GC.PNP_OTHER[opts], pnp_cases, opts)


# ---------------------------------------------------------------------- vo_find_essential
@pytest.fixture(scope="module")
def ess_cases():
    return GC.ess_cases()


def _check_ess(names, cases, opts):
    problems = [cases[k] for k in names]
    fwd = GC.gpu_essential(problems, *opts, CAP)
    rev = GC.gpu_essential(problems[::-1], *opts, CAP)[::-1]
    for k, (p0, p1), g, r in zip(names, problems, fwd, rev):
        n = len(p0)
        assert _same_outputs(g, r), f"{k} {opts}: the outputs depend on the chain's slot"
        e = _expect("ess", GC.ess_expect, k, (p0, p1), opts)
        for out, what in ((g, "forward"), (r, "reversed")):
            tag = f"{k} {opts} {what}"
            assert (out["mask"][n:] == GC.SENT_U8).all(), tag + ": mask rows past the count written"
            assert out["ok"] == e["ok"], tag
            assert np.array_equal(out["mask"][:n], e["mask"]), tag
            if e["ok"]:
                assert GC.same_bits(out["E"], e["E"]), tag
            if n < 5:
                assert out["ok"] == 0 and not out["mask"][:n].any(), tag


@pytest.mark.parametrize("form", ["few_chains", "many_chains"])
@pytest.mark.parametrize("opts", [GC.ESS_REF_OPTS] + list(GC.ESS_OTHER))
def test_find_essential_batch(ess_cases, launch_cus, form, opts):
    """Both launch forms (k_essential<1>: 24 hypotheses per round on ten lanes each; k_essential<2>,
    taken with the CU count set to 1: 64 per round): n < 5, n == 5, rounds after the first, the
    max_iters cap, degenerate scenes."""
    if form == "many_chains":
        launch_cus(1)
    names = GC.ESS_MAIN if opts == GC.ESS_REF_OPTS else GC.ESS_OTHER[opts]
    _check_ess(names, ess_cases, opts)


# ---------------------------------------------------------------------- vo_recover_pose
@pytest.mark.parametrize("with_mask", [True, False])
def test_recover_pose_batch(with_mask):
    rc = GC.recover_cases()
    problems = [r[1:] for r in rc]
    fwd = GC.gpu_recover(problems, CAP, with_mask)
    rev = GC.gpu_recover(problems[::-1], CAP, with_mask)[::-1]
    for (name, E, p0, p1), g, r in zip(rc, fwd, rev):
        n = len(p0)
        assert _same_outputs(g, r), f"{name}: the outputs depend on the chain's slot"
        e = GC.recover_expect(E, p0, p1)
        for out, what in ((g, "forward"), (r, "reversed")):
            tag = f"{name} {what}"
            assert out["n_good"] == e["n_good"], tag
            assert GC.same_bits(out["R"], e["R"]) and GC.same_bits(out["t"], e["t"]), tag
            if with_mask:
                assert np.array_equal(out["mask"][:n], e["mask"]), tag
                assert (out["mask"][n:] == GC.SENT_U8).all(), tag + ": mask rows past the count written"
        if name == "count_0":
            assert g["n_good"] == 0                      # four counts of 0: the first candidate


# ---------------------------------------------------------------------- vo_triangulate_points
@pytest.fixture(scope="module")
def tri():
    P = GC.tri_cases(1000)
    return P, GC.tri_expect(*P)


@pytest.mark.parametrize("n", [1, 127, 128, 129, 1000])
def test_triangulate_points_one_pair_per_point(tri, n):
    (P1, P2, x1, x2), ref = tri
    got = GC.gpu_triangulate(P1[:n], P2[:n], x1[:n], x2[:n])
    bad = [i for i in range(n) if not GC.same_bits(got[i], ref[i])]
    assert not bad, bad[:8]


# ---------------------------------------------------------------------- vo_rodrigues
@pytest.mark.parametrize("n", [1, 127, 128, 129])
@pytest.mark.parametrize("to_matrix", [True, False])
def test_rodrigues_batch(n, to_matrix):
    if to_matrix:
        batch = GC.rod_batch(GC.rod_vectors().values(), n, n, (3,))
    else:
        batch = GC.rod_batch(GC.rod_matrices().values(), n, 1000 + n, (3, 3))
    got = GC.gpu_rodrigues(batch)
    ref = GC.rod_expect(batch)
    bad = [i for i in range(n) if not GC.same_bits(got[i], ref[i])]
    assert not bad, [(i, batch[i].tolist(), got[i].tolist(), ref[i].tolist()) for i in bad[:4]]


# ---------------------------------------------------------------------- vo_ratio_matches
@pytest.mark.parametrize("ratio", [0.5, 0.8])
def test_ratio_matches_batch(ratio):
    """B = 4 with nq = 0, 1, 257, 700 and strides larger than the counts: rows without two matches,
    exact ties in double (dropped by the strict <), FLT_MAX distances; rows at or past counts[b]
    keep the sentinel."""
    kp0, kp1, idx, dist = GC.ratio_case(ratio, 5)
    cap = max(GC.RATIO_NQ)
    pts0, pts1, cnt = GC.gpu_ratio(kp0, kp1, idx, dist, GC.RATIO_NQ, ratio, cap)
    for b, nq in enumerate(GC.RATIO_NQ):
        e0, e1 = GC.ratio_expect(kp0[b], kp1[b], idx[b], dist[b], nq, ratio)
        assert cnt[b] == len(e0), f"problem {b}"
        assert np.array_equal(pts0[b, :len(e0)], e0) and np.array_equal(pts1[b, :len(e0)], e1), f"problem {b}"
        assert (pts0[b, len(e0):] == GC.SENT_F32).all() and (pts1[b, len(e0):] == GC.SENT_F32).all(), f"problem {b}"


def test_ratio_matches_reports_overflow():
    """cap below the number of matches that pass: counts[b] is the number that passed (above cap: the
    overflow is reported, vo_bootstrap turns it into VO_ST_CAPACITY), the first cap of them are
    written and nothing past row cap; the problems that fit are unaffected."""
    ratio = 0.8
    kp0, kp1, idx, dist = GC.ratio_case(ratio, 5)
    exp = [GC.ratio_expect(kp0[b], kp1[b], idx[b], dist[b], nq, ratio) for b, nq in enumerate(GC.RATIO_NQ)]
    kept = [len(e[0]) for e in exp]
    cap = kept[3] - 1                                     # one short for the last problem, exact fit + for the others
    assert kept[2] < cap
    pts0, pts1, cnt = GC.gpu_ratio(kp0, kp1, idx, dist, GC.RATIO_NQ, ratio, cap)
    assert list(cnt) == kept and cnt[3] == cap + 1
    for b in range(4):
        m = min(kept[b], cap)
        assert np.array_equal(pts0[b, :m], exp[b][0][:m]) and np.array_equal(pts1[b, :m], exp[b][1][:m])
        assert (pts0[b, m:] == GC.SENT_F32).all() and (pts1[b, m:] == GC.SENT_F32).all()
    # exact fit
    pts0, pts1, cnt = GC.gpu_ratio(kp0, kp1, idx, dist, GC.RATIO_NQ, ratio, cap + 1)
    assert list(cnt) == kept
    assert np.array_equal(pts0[3], exp[3][0]) and np.array_equal(pts1[3], exp[3][1])
