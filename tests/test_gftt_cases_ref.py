"""The cases of gftt_cases.py reach what they are named for: asserted on the CPU oracle alone, so that
no case of test_gpu_gftt_select_edges.py can go vacuous later (in the style of
test_geom_cases_ref.py).  Everything here runs without a GPU.

These are conditions on the inputs: a case that fails one gets another input, never a weaker
assertion.
"""
import itertools

import numpy as np
import pytest

import gftt_cases as GC

PAGE = GC.PAGE
THREE = [(w, p) for w in ("md40", "md15_5") for p in (False, True)]


def _ranks(img, quality, corners):
    _, addr = GC.passing_keys(img, quality)
    rank = {int(a): i for i, a in enumerate(addr)}
    return [rank[int(y) * img.shape[1] + int(x)] for x, y in corners]


def _has(corners, c):
    return bool(((corners[:, 0] == c[0]) & (corners[:, 1] == c[1])).any())


# ---------------------------------------------------------------------- the model is the oracle
@pytest.mark.parametrize("name", list(GC.cases()))
def test_walk_model_equals_oracle(name):
    img, q, md, mc = GC.cases()[name]
    got = GC.walk_model(img, q, md, mc)
    ref = GC.expect(name)
    assert got.shape == ref.shape and np.array_equal(got, ref), f"{name}: {len(got)} vs {len(ref)}"


# ---------------------------------------------------------------------- three corners in one cell
@pytest.mark.parametrize("which,one_page", THREE)
def test_three_in_cell_geometry(which, one_page):
    img, q, md, strong = GC.three_in_cell(which, one_page)
    assert img.shape == (240, 320)
    ref = GC.expect(f"three_in_cell_{which}" + ("_one_page" if one_page else ""))
    assert all(_has(ref, c) for c in strong)
    assert len(set(GC.cells_of(strong, md))) == 1, "the three corners do not share a cell"
    for a, b in itertools.combinations(strong, 2):
        assert (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2 >= md * md
    assert _ranks(img, q, strong) == [0, 1, 2]
    nkeys = len(GC.passing_keys(img, q)[0])
    if one_page:
        assert 3 < nkeys < PAGE
    else:
        assert nkeys > PAGE


@pytest.mark.parametrize("which", ["md40", "md15_5"])
def test_three_in_cell_losing_any_corner_shows(which):
    """a selection that forgets one of the three for the later pages returns another list, whichever
    of them it forgets (which one a two-slot cell loses depends on the order of its updates)"""
    img, q, md, strong = GC.three_in_cell(which)
    ref = GC.expect(f"three_in_cell_{which}")
    g = GC.THREE_MD40 if which == "md40" else GC.THREE_MD15_5
    for c in strong:
        lost = GC.walk_model(img, q, md, GC.MC, lose=c)
        assert not np.array_equal(lost, ref), (which, c)
        # one corner more: a key of a later page within md of the forgotten corner, which only the
        # grid can reject
        extra = [tuple(p) for p in lost.tolist() if not _has(ref, p)]
        assert len(lost) == len(ref) + 1 and len(extra) == 1, (which, c, extra)
        (ex, ey), = extra
        assert _ranks(img, q, extra)[0] >= PAGE and (ex - c[0]) ** 2 + (ey - c[1]) ** 2 < md * md
    assert min(_ranks(img, q, g["weak"])) >= PAGE
    assert not any(_has(ref, w) for w in g["weak"])


def test_three_in_cell_md40_figures():
    """the figures the case was designed with"""
    img, q, md, _ = GC.three_in_cell("md40")
    assert len(GC.passing_keys(img, q)[0]) == 5100
    assert len(GC.expect("three_in_cell_md40")) == 38


# ---------------------------------------------------------------------- tie runs
def test_checker4_one_run_across_the_pages():
    """one run of equal values from rank 0 across three page boundaries, keys after it, and at every
    boundary the last key of the page shares its upper 60 bits with the first key left out: only the
    last, 4-bit digit of the radix select separates them"""
    ck = GC.checker4()
    runs = GC.tie_runs(ck, GC.CHECKER_QUALITY)
    v, addr = GC.passing_keys(ck, GC.CHECKER_QUALITY)
    st, ln = max(runs, key=lambda r: r[1])
    assert st == 0 and ln > 3 * PAGE and len(v) > ln + 100
    for r in (PAGE, 2 * PAGE, 3 * PAGE):
        assert v[r - 1] == v[r] and addr[r - 1] >> 4 == addr[r] >> 4 and addr[r - 1] > addr[r]
    # the whole list falls into one value bucket of the split form's histogram (bucket width
    # (max - gate) / 4096 of the key range; the run is the maximum)
    assert v[0] == v[ln - 1]
    for md in (1.6, 2):
        ref = GC.expect(f"checker4_md{md}")
        r = np.array(_ranks(ck, GC.CHECKER_QUALITY, ref))
        assert (np.diff(r) > 0).all()
        assert (r < PAGE).any() and (r >= 3 * PAGE).any() and (r >= ln).any(), "corners from every page and past the run"


def test_binary_many_short_runs():
    img, q, md, mc = GC.cases()["binary_md2"]
    runs = GC.tie_runs(img, q)
    v, _ = GC.passing_keys(img, q)
    assert len(v) > PAGE and len(runs) > 1000
    assert max(ln for _, ln in runs) > 64                              # longer than one round of the walk
    assert any(st < PAGE < st + ln for st, ln in runs), "no run across the page boundary"


@pytest.mark.parametrize("name", ["ties_cut_page0", "ties_cut_page1", "ties_cut_mc1"])
def test_ties_cut_inside_a_run(name):
    """maxCorners ends the list strictly inside a run: the last corner returned, the one before it (if
    any) and the first one cut off have the same eigenvalue"""
    ck, q, md, mc = GC.cases()[name]
    full = GC.walk_model(ck, q, md, 0)
    assert 1 <= mc < len(full) - 1
    v, _ = GC.passing_keys(ck, q)
    r = _ranks(ck, q, full[:mc + 1])
    runs = GC.tie_runs(ck, q)
    st, ln = next((s, l) for s, l in runs if s <= r[mc - 1] < s + l)
    assert r[mc] < st + ln and v[r[mc - 1]] == v[r[mc]], "the first corner cut off is outside the run"
    assert st <= r[max(mc - 2, 0)] and st < r[mc]
    want_page = {"ties_cut_page0": 0, "ties_cut_page1": 1, "ties_cut_mc1": 0}[name]
    assert r[mc - 1] // PAGE == want_page and r[mc] // PAGE == want_page
    assert np.array_equal(GC.expect(name), full[:mc])


# ---------------------------------------------------------------------- grid geometry
def test_grid_edge_cases_reach_their_regimes():
    c = GC.cases()
    rint = lambda md: int(np.rint(md))
    assert (rint(1.5), rint(2.5), rint(15.5)) == (2, 2, 16)            # lrint: half to even
    for (W, H), mds in GC.GRID_EDGES.items():
        for md in mds:
            for kind in ("crop", "noise"):
                img, q, m, mc = c[f"{kind}_{W}x{H}_md{md}"]
                assert img.shape == (H, W) and m == md
                assert len(GC.passing_keys(img, q)[0]) > 100
    for md in GC.GRID_EDGES[(131, 67)]:
        cs = rint(md)
        assert 131 % cs and 67 % cs, "the image is a multiple of the cell"
    assert -(-37 // 40) == 1 and -(-300 // 40) > 1                      # one grid row
    assert -(-45 // 50) == 1 and -(-300 // 50) > 1                      # one grid column
    assert GC.split_applies(300, 37, 255, GC.MC) and not GC.split_applies(300, 37, 256, GC.MC)
    assert 64 * 64 * 8 + 4 > 4 * 64 * 64 >= 32 * 32 * 8 + 4             # the scratch test, cs 1 and cs 2
    assert not GC.split_applies(64, 64, 1.0, GC.MC) and GC.split_applies(64, 64, 1.6, GC.MC)
    assert not GC.split_applies(64, 64, 0.99, GC.MC) and not GC.split_applies(64, 64, 0, GC.MC)
    # the walk has something to reject wherever there is a grid, and something to keep
    for name, (img, q, md, mc) in c.items():
        if name.startswith(("crop_", "noise_")) and md >= 2 and mc == GC.MC:
            n = len(GC.passing_keys(img, q)[0])
            assert 1 <= len(GC.expect(name)) < n, name


def _grid_placement(W, H, md, mcap=GC.MC):
    """where k_gftt_select keeps its cell grid: the host's arithmetic (vo_select.hip), restated"""
    if md < 1:
        return "no grid"
    cs = int(np.rint(md))
    cells = -(-W // cs) * -(-H // cs)
    acc_lds = min(mcap, GC.ACC_MAX)
    if cells <= GC.GRID_LDS_CELLS and 16 * PAGE + 6 * acc_lds + 8 * cells <= GC.LDS_BUDGET:
        return "lds"
    if 8 * PAGE + 2 * cells <= W * H:
        return "l2 behind the conflict lists"
    return "l2 alone"


def test_grid_placements_are_all_reached():
    """every placement of k_gftt_select's grid has a case: the two cases built for the wave-serial
    walk over the L2 grid land there, and older cases land on the two parallel placements"""
    c = GC.cases()
    where = {name: _grid_placement(img.shape[1], img.shape[0], md) for name, (img, q, md, mc) in c.items()}
    serial = {"noise_200x120_md2.5", "binary_131x67_md1.49"}
    assert {n for n, w in where.items() if w == "l2 alone"} >= serial
    for name in serial:
        img, q, md, mc = c[name]
        n = len(GC.passing_keys(img, q)[0])
        assert mc == GC.MC and 64 < len(GC.expect(name)) < n < PAGE, name   # several rounds, rejections
    assert GC.split_applies(200, 120, 2.5, GC.MC) and not GC.split_applies(131, 67, 1.49, GC.MC)
    older = {n: w for n, w in where.items() if n not in serial}
    assert "lds" in older.values() and "l2 behind the conflict lists" in older.values()
    assert where["three_in_cell_md40"] == "lds" and where["checker4_md2"] == "l2 behind the conflict lists"


def test_max_corners_limits():
    c = GC.cases()
    assert len(GC.expect("noise_64x64_md1.6_mc1")) == 1
    full = GC.expect("noise_64x64_md1.6")
    assert len(full) > 100
    for mc in (0, -1):
        assert c[f"noise_64x64_md1.6_mc{mc}"][3] == mc
        assert np.array_equal(GC.expect(f"noise_64x64_md1.6_mc{mc}"), full)


def test_small_image_with_many_keys():
    """more candidates on one page than an eighth of the pixels: the conflict lists of k_gftt_select
    (16 u16 per candidate in the chain's W * H u32 of scratch) have no room for all of them"""
    img, q, md, mc = GC.cases()["checker_64_md1.6"]
    n = len(GC.passing_keys(img, q)[0])
    assert img.size // 8 < n < PAGE
    assert 100 < len(GC.expect("checker_64_md1.6")) < n


def test_sparse_dots_zero_one_two_keys():
    img, ratio = GC.sparse_dots()
    assert 0.1 < ratio < 0.9
    c = GC.cases()
    for name, n in (("sparse_0_keys", 0), ("sparse_1_key", 1), ("sparse_2_keys", 2)):
        q = c[name][1]
        assert c[name][0] is img and len(GC.passing_keys(img, q)[0]) == n, name
        ref = GC.expect(name)
        assert len(ref) == n
        assert [tuple(p) for p in ref.tolist()] == [(x, y) for x, y, _ in GC.SPARSE_DOTS[:n]]
    assert abs(c["sparse_1_key"][1] / ratio - 1) < 2e-3 and abs(c["sparse_2_keys"][1] / ratio - 1) < 2e-3


# ---------------------------------------------------------------------- cv2compat's capacity case
def test_capacity_image_has_more_corners_than_the_engine_holds():
    img, q, md = GC.capacity_case()
    from oracle import _olib as O
    assert len(O.gftt(img, 0, q, md)) > 8192
