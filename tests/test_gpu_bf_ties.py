"""The matcher's (distance, index) tie order against O.bf_knn2 on descriptor sets where every
query's best two distances are equal (sift_cases.py): ties inside a lane, across the two
half-waves, across 32-row sub-tiles, 128-row tiles and train splits, a three-way tie, ties in
the float-order fix-up path, and more problems than the device plan takes.  Each batch runs four
ways -- default (int8, device plan), VO_BF_PLAN=0 (capacity plan), VO_BF_BF16=1 (bf16 kernel), a
caller-owned scratch -- and the four results must be identical.  test_sift_cases_ref.py proves the
ties on the CPU.
"""
import os

import numpy as np
import pytest

import sift_cases as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FLT_MAX = np.finfo(np.float32).max


def _match(q, t, sizes, env=None, own_scratch=False):
    from monocular_visual_odometry_va4mr_amd.features import bf_knn2_batch, matcher_scratch_bytes
    dev = torch.device("cuda")
    nq = torch.tensor([s[0] for s in sizes], dtype=torch.int32, device=dev)
    nt = torch.tensor([s[1] for s in sizes], dtype=torch.int32, device=dev)
    scr = None
    if own_scratch:
        scr = torch.empty(matcher_scratch_bytes(q.shape[0], q.shape[1], t.shape[1]), dtype=torch.uint8, device=dev)
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        i2, d2 = bf_knn2_batch(torch.from_numpy(q).to(dev), nq, torch.from_numpy(t).to(dev), nt, scratch=scr)
        torch.cuda.synchronize()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return i2.cpu().numpy(), d2.cpu().numpy()


def _four_ways(q, t, sizes):
    """The batch through the four variants; returns the default's result after requiring the
    other three to equal it."""
    idx, dist = _match(q, t, sizes)
    for name, kw in (("VO_BF_PLAN=0", {"env": {"VO_BF_PLAN": "0"}}), ("VO_BF_BF16=1", {"env": {"VO_BF_BF16": "1"}}),
                     ("own scratch", {"own_scratch": True})):
        i2, d2 = _match(q, t, sizes, **kw)
        assert np.array_equal(i2, idx) and np.array_equal(d2, dist), name
    return idx, dist


def _assert_oracle(idx, dist, sizes, ref):
    for b, ((nq, nt), (ei, ed)) in enumerate(zip(sizes, ref)):
        wrong = np.flatnonzero((idx[b, :nq] != ei).any(axis=1) | (dist[b, :nq] != ed).any(axis=1))
        assert len(wrong) == 0, (f"problem {b} ({nq} x {nt}): queries {wrong[:8]}, got {idx[b, wrong[:8]].tolist()}, "
                                 f"oracle {ei[wrong[:8]].tolist()}")
        assert (idx[b, nq:] == -1).all() and (dist[b, nq:] == FLT_MAX).all()


def test_pool_ties_every_query():
    """Every query tied over about nt / 8 train rows: the answer is the two lowest indices of its
    pool row, across sub-tiles, tiles (three per split at 4,100 rows) and splits."""
    q, t, sizes = S.bf_pool_batch()
    idx, dist = _four_ways(q, t, sizes)
    _assert_oracle(idx, dist, sizes, S.bf_reference("pool", q, t, sizes))


def test_planted_pairs_and_triple():
    """One pool row planted at (a, a + d) only, d in 1, 4, 8, 31, 32, 127, 128 and a in 130, 0; at the
    two sides of a split boundary; in the first split and the one-row last tile; at (a, a + 4,
    a + 128): the lower index first, whatever lane, register, half-wave, tile or split holds it."""
    q, t, sizes, plants = S.bf_planted_batch()
    idx, dist = _four_ways(q, t, sizes)
    for b, p in enumerate(plants):
        assert idx[b, 0].tolist() == [p[0], p[1]], (p, idx[b, 0].tolist())
    _assert_oracle(idx, dist, sizes, S.bf_reference("planted", q, t, sizes))


def test_fixup_ties():
    """Squared distances above 2^22 with tied neighbours: k_bf_fixup's lane-strided walk and its
    (distance, index) lane merge."""
    q, t, sizes = S.bf_fixup_batch()
    idx, dist = _four_ways(q, t, sizes)
    ref = S.bf_reference("fixup", q, t, sizes)
    assert all((ed[:, 1] >= 2048.0).all() for _, ed in ref)
    _assert_oracle(idx, dist, sizes, ref)


def test_many_problems_capacity_plan():
    """1,025 problems (above BF_PLAN_MAXB: the capacity plan by itself) of at most 4 x 4 tied
    descriptors, and the first 1,024 of them through the device plan."""
    q, t, sizes = S.bf_many_batch()
    ref = S.bf_reference("many", q, t, sizes)
    idx, dist = _match(q, t, sizes)
    _assert_oracle(idx, dist, sizes, ref)
    i2, d2 = _match(np.ascontiguousarray(q[:1024]), np.ascontiguousarray(t[:1024]), sizes[:1024])
    _assert_oracle(i2, d2, sizes[:1024], ref[:1024])
    assert np.array_equal(i2, idx[:1024]) and np.array_equal(d2, dist[:1024])
