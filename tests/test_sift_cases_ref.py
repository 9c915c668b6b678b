"""CPU proof that every case of sift_cases.py reaches the path it is named for, with the oracle
alone (no GPU): keypoint counts, octaves, plateau ties, multiple orientations, removed duplicates,
per-tile extrema below the kernel's block list, and the planted matcher ties.  These are properties
of the inputs, not of the kernels; test_gpu_sift_stages.py / test_gpu_bf_ties.py run the same cases.
"""
import numpy as np
import pytest

import sift_cases as S

EX_W, EX_H, EX_LCAP, BORDER = 64, 16, 1024, 5      # k_extrema_t's tile, block list and border


def _ref(w, h, kind):
    return S.reference((w, h, kind))


def _octaves(kp):
    return sorted(set((kp[:, 5].astype(np.int32) & 255).astype(np.int8).tolist()))


def _per_location(kp):
    _, cnt = np.unique(kp[:, :3], axis=0, return_counts=True)
    return cnt


def test_case_list_is_complete():
    assert len(S.CASES) == len(S.SIZES) + len(S.KINDS) - 1 == len(set(S.CASES))
    assert {c[2] for c in S.CASES} == set(S.KINDS)
    assert {(c[0], c[1]) for c in S.CASES} == set(S.SIZES)
    for c in S.CASES:
        img = S.image(c[2], c[0], c[1])
        assert img.dtype == np.uint8 and img.shape == (c[1], c[0])


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_stages_agree_with_sift(case):
    """vo_o_sift_stages taps vo_o_sift's own run: its final count is O.sift's, DoG layer i is
    G[i+1] - G[i], octave sizes halve (rounding down) and the counts are ordered."""
    st, kp, desc = S.reference(case)
    W, H = case[0], case[1]
    assert st["n_final"] == len(kp) == len(desc)
    assert st["n_extrema"] == len(st["extrema"]) >= st["n_refined"]
    assert st["n_raw"] >= st["n_final"] and (st["n_raw"] > 0) == (st["n_refined"] > 0)
    assert st["up"].shape == (2 * H, 2 * W)
    assert st["up"].min() >= 0 and st["up"].max() <= 255
    ow, oh = 2 * W, 2 * H
    for o, (g, d) in enumerate(zip(st["gauss"], st["dog"])):
        if o > 0:
            ow, oh = ow // 2, oh // 2
        assert g.shape == d.shape == (5, oh, ow)
        assert np.array_equal(d[:4], g[1:5] - g[0:4])
    e = st["extrema"]
    if len(e):
        # scan order: octave, layer, row, column
        key = ((e[:, 0].astype(np.int64) * 8 + e[:, 1]) * 65536 + e[:, 2]) * 65536 + e[:, 3]
        assert (np.diff(key) > 0).all()
        assert e[:, 1].min() >= 1 and e[:, 1].max() <= 3


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_extrema_per_tile_below_block_list(case):
    """Extrema per 64 x 16 tile over the three layers of an octave stay below k_extrema_t's
    per-block list (measured maximum: 256, on hstripes3)."""
    e = S.reference(case)[0]["extrema"]
    if len(e) == 0:
        return
    tile = (e[:, 0] * 4096 + (e[:, 2] - BORDER) // EX_H) * 4096 + (e[:, 3] - BORDER) // EX_W
    assert np.unique(tile, return_counts=True)[1].max() < EX_LCAP


def test_blob_131x67_three_octaves():
    st, kp, _ = _ref(131, 67, "blob")
    assert len(kp) >= 100                                       # measured 164
    assert _octaves(kp) == [-1, 0, 1]
    assert (_per_location(kp) > 1).sum() >= 10                  # measured 33 multi-orientation


def test_blob_200x150_dense():
    assert len(_ref(200, 150, "blob")[1]) >= 300                # measured 541


@pytest.mark.parametrize("size", [(33, 97), (63, 31), (65, 33), (97, 33)])
def test_blob_small_sizes_have_keypoints(size):
    assert len(_ref(size[0], size[1], "blob")[1]) >= 10         # measured 41, 27, 30, 40


@pytest.mark.parametrize("case", [(1, 1, "blob"), (2, 3, "blob"), (5, 5, "blob"), (131, 67, "const"),
                                  (131, 67, "ramp")], ids=S.case_id)
def test_empty_cases(case):
    """No extremum and no keypoint: every octave is skipped (no pixel inside the 5-pixel border)
    or holds nothing above the threshold."""
    st, kp, desc = S.reference(case)
    assert st["n_extrema"] == 0 and st["n_raw"] == 0 and len(kp) == 0 and len(desc) == 0
    if case[2] == "blob":
        for g in st["gauss"]:
            assert g.shape[1] <= 2 * BORDER or g.shape[2] <= 2 * BORDER
    assert (len(st["gauss"]) == 0) == (case[:2] == (1, 1))      # the oracle's zero octaves


@pytest.mark.parametrize("kind", ["hstripes3", "vstripes3"])
def test_stripes_are_plateau_ties(kind):
    """Thousands of extrema (measured 7,560 / 5,208), every one with an equal neighbour in its own
    layer -- they are extrema only through '>=' -- and none survives refinement."""
    st, kp, _ = _ref(131, 67, kind)
    assert st["n_extrema"] >= 1000
    assert st["n_refined"] == 0 and len(kp) == 0
    for o, layer, r, c in st["extrema"]:
        d = st["dog"][o][layer]
        nb = d[r - 1:r + 2, c - 1:c + 2]
        assert (nb == d[r, c]).sum() >= 2


def test_checker6_four_orientations():
    st, kp, _ = _ref(131, 67, "checker6")
    assert (_per_location(kp) == 4).sum() >= 100                # measured 180 of 180 locations
    assert st["n_raw"] == 4 * st["n_refined"]


def test_binnoise2x_has_duplicates():
    st, kp, _ = _ref(131, 67, "binnoise2x")
    assert st["n_raw"] - st["n_final"] >= 1                     # measured 391 raw, 387 kept


def test_dots6_is_dense():
    """The capacity case: many extrema of which most fail refinement, several keypoints each."""
    st, kp, _ = _ref(131, 67, "dots6")
    assert st["n_extrema"] >= 500 and st["n_raw"] >= 1000       # measured 1,096 and 1,550
    assert st["n_extrema"] > st["n_refined"] and st["n_raw"] > st["n_refined"]


# ------------------------------------------------------------------ matcher tie cases
def test_bf_pool_every_query_tied():
    q, t, sizes = S.bf_pool_batch()
    assert sizes == S.BF_POOL_SIZES and q.shape[1] == 300 and t.shape[1] == 4200
    ref = S.bf_reference("pool", q, t, sizes)
    plan = S.bf_device_plan(sizes)
    assert plan[0] == (16, 3 * S.BF_TT)                         # (200, 4100): three tiles per split
    for b, ((nq, nt), (idx, dist)) in enumerate(zip(sizes, ref)):
        assert (dist[:, 0] == 2.0).all() and (dist[:, 1] == 2.0).all()
        for i in range(nq):
            # the expected answer: the two lowest indices of the query's pool row
            same = np.flatnonzero((t[b, :nt, 4:] == q[b, i, 4:]).all(axis=1))
            assert len(same) >= 2 and tuple(idx[i]) == (same[0], same[1])
    tied = [len(np.flatnonzero((t[0, :4100] == t[0, j]).all(axis=1))) for j in range(8)]
    assert min(tied) > 4100 // 16                               # about nt / 8 rows per value


def test_bf_planted_pairs():
    q, t, sizes, plants = S.bf_planted_batch()
    ref = S.bf_reference("planted", q, t, sizes)
    sp, per = S.bf_device_plan(sizes)[0]
    assert {(p[1] - p[0]) for p in plants if len(p) == 2 and p[0] in (0, 130)} >= set(S.BF_PLANT_OFFSETS)
    assert any(len(p) == 2 and p[0] // per != p[1] // per and p[0] == per - 1 for p in plants)
    assert any(len(p) == 3 for p in plants)
    for b, (p, (idx, dist)) in enumerate(zip(plants, ref)):
        assert max(p) < sizes[b][1]
        for qi in (0, 1, 2, S.BF_PLANT_NQ - 1):
            assert tuple(idx[qi]) == (p[0], p[1]) and dist[qi, 0] == dist[qi, 1] == 2.0
        assert (dist[3:-1, 0] > 2.0).all()                      # the random queries are not tied


def test_bf_fixup_every_query_tied_above_2048():
    q, t, sizes = S.bf_fixup_batch()
    for idx, dist in S.bf_reference("fixup", q, t, sizes):
        assert (dist[:, 1] >= 2048.0).all()                     # second distance^2 >= 2^22
        assert (dist[:, 0] == dist[:, 1]).all() and (idx[:, 0] < idx[:, 1]).all()
    assert max(nt for _, nt in sizes) > 64 * 8                  # several rows per lane of the walk


def test_bf_many_problems_have_ties():
    q, t, sizes = S.bf_many_batch()
    assert len(sizes) == 1025 and q.shape[1:] == (4, 128) and t.shape[1:] == (4, 128)
    ref = S.bf_reference("many", q, t, sizes)
    assert sum(1 for i, d in ref if len(d) and ((d[:, 0] == 2.0) & (d[:, 1] == 2.0)).any()) >= 200
    assert {nq for nq, _ in sizes} == set(range(5)) == {nt for _, nt in sizes}
