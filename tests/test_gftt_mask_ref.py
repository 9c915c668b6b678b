"""What the cases of gftt_mask_cases.py reach, shown on the CPU: the disc masks against a plain
Python loop, the detector model against oracle.gftt with an all-set mask, and the properties that
make a masked detector differ from an unmasked one followed by a filter.  These are conditions on
the inputs; test_gpu_gftt_mask.py runs the same inputs on the GPU.
"""
import math

import numpy as np
import pytest

import gftt_cases as GC
import gftt_mask_cases as M


# ---------------------------------------------------------------------- disc masks
def test_mask_ref_is_the_closed_disc():
    """mask_ref against the predicate at every pixel in Python floats, and its edges"""
    W, H = 45, 37
    pts = [(10, 10), (20.5, 30.5), (-3, 10), (W + 2, 30), (40, -1), (44, 36), (-100, 5), (float("nan"), 5), (5, float("inf"))]
    for r in (0.5, 1.5, 5, 10):
        want = np.full((H, W), 255, np.uint8)
        for px, py in pts:
            if not (math.isfinite(px) and math.isfinite(py)):
                continue
            for y in range(H):
                for x in range(W):
                    dx, dy = float(x) - px, float(y) - py
                    if dx * dx + dy * dy <= r * r:
                        want[y, x] = 0
        assert np.array_equal(M.mask_ref(W, H, pts, r), want), r
    m = M.mask_ref(131, 67, [(50, 20)], 5)
    assert m[24, 53] == 0 and m[16, 47] == 0 and m[20, 55] == 0 and m[24, 54] == 255      # (3, 4) at r = 5
    assert int((m == 0).sum()) == 81


# ---------------------------------------------------------------------- the detector model
@pytest.mark.parametrize("name", list(M.cases()))
def test_model_with_all_set_mask_is_the_oracle(name):
    from oracle import _olib as O
    k = M.cases()[name]
    full = np.full(k["img"].shape, 255, np.uint8)
    want = O.gftt(k["img"], k["mc"], k["q"], k["md"], k["bs"], k["harris"])
    got = M.gftt_masked_model(k["img"], full, k["mc"], k["q"], k["md"], k["bs"], k["harris"])
    assert np.array_equal(got, want)
    if k["bs"] == 3 and not k["harris"]:
        assert np.array_equal(got, GC.walk_model(k["img"], k["q"], k["md"], k["mc"]))


def _facts(name):
    from oracle import _olib as O
    k = M.cases()[name]
    img, mask = k["img"], k["mask"]
    e = O.eigmap(img, k["bs"], k["harris"])
    unmasked = O.gftt(img, k["mc"], k["q"], k["md"], k["bs"], k["harris"])
    keep = mask[unmasked[:, 1].astype(int), unmasked[:, 0].astype(int)] != 0
    _, _, emax = M.masked_keys(img, mask, k["q"], k["bs"], k["harris"])
    return dict(e=e, unmasked=unmasked, filtered=unmasked[keep], masked=M.expect(name), emax=emax, gmax=e.max())


DISC_CASES = [n for n in M.cases() if n.startswith(("crop_", "noise_")) or n in ("harris_bs3", "mineig_bs5", "harris_bs7")]


def test_disc_cases_differ_from_filtering_and_refill_the_budget():
    """Over the disc cases: the masked list is never the unmasked list filtered by the mask, it never
    holds a masked-out pixel, and it holds corners the unmasked run did not return; the maximum over
    the mask is below the global one in some cases and equal to it in others."""
    below = equal = 0
    for name in DISC_CASES:
        k = M.cases()[name]
        f = _facts(name)
        got = f["masked"]
        assert len(f["filtered"]) < len(f["unmasked"]), name
        assert not np.array_equal(got, f["filtered"]), name
        assert (k["mask"][got[:, 1].astype(int), got[:, 0].astype(int)] != 0).all(), name
        new = set(map(tuple, got.tolist())) - set(map(tuple, f["unmasked"].tolist()))
        # with a budget the freed places are taken by new corners; without one (all_keys) only the
        # moved threshold can add any
        assert len(new) >= (3 if k["mc"] < GC.MC else 1), (name, len(new))
        assert f["emax"] > 0
        below += f["emax"] < f["gmax"]
        equal += f["emax"] == f["gmax"]
    assert below >= 5 and equal >= 5, (below, equal)
    # the threshold moves with the maximum: a case whose masked list holds a corner the global
    # threshold would have cut
    moved = 0
    for name in DISC_CASES:
        k = M.cases()[name]
        f = _facts(name)
        if f["emax"] < f["gmax"]:
            g = f["masked"]
            v = f["e"][g[:, 1].astype(int), g[:, 0].astype(int)]
            moved += bool((v <= np.float32(np.float64(f["gmax"]) * k["q"])).any())
    assert moved >= 1


def test_border_max_case():
    """The maximum over the mask sits on the image border, below the global maximum: the threshold is
    taken from a pixel that can never be a key."""
    k = M.cases()["border_max"]
    f = _facts("border_max")
    e, mask = f["e"], k["mask"]
    H, W = e.shape
    assert 0 < f["emax"] < f["gmax"]
    ys, xs = np.nonzero((e == f["emax"]) & (mask != 0))
    assert len(ys) >= 1 and all(x in (0, W - 1) or y in (0, H - 1) for x, y in zip(xs, ys))
    got = f["masked"]
    assert len(got) >= 5
    assert ((got[:, 0] >= 1) & (got[:, 0] <= W - 2) & (got[:, 1] >= 1) & (got[:, 1] <= H - 2)).all()
    assert not np.array_equal(got, f["filtered"])


@pytest.mark.parametrize("name", ["border_max", "crop_131x67", "crop_58x64", "noise_57x64"])
def test_nms_looks_at_masked_out_neighbours(name):
    k = M.cases()[name]
    assert M.nms_only_through_masked(k["img"], k["mask"], k["q"]) >= 1


SEAMS = [n for n in M.cases() if n.startswith("seam_")]


@pytest.mark.parametrize("name", SEAMS)
def test_seam_cases_have_an_interior_maximum_that_is_no_local_maximum(name):
    """The maximum over the mask is a single interior pixel on the named tile seam, below the global
    maximum, with a stronger masked-out neighbour; taking the maximum over the local maxima of the
    map, or over the allowed local maxima, gives another threshold and another list."""
    k = M.cases()[name]
    f = _facts(name)
    e, mask = f["e"], k["mask"]
    H, W = e.shape
    axis, line = ("col", int(name.split("col")[1])) if "col" in name else ("row", int(name.split("row")[1]))
    mm, (x, y) = M.seam_mask(k["img"], axis, line, k["bs"])
    assert np.array_equal(mm, mask) and (x if axis == "col" else y) == line
    assert 1 <= x <= W - 2 and 1 <= y <= H - 2
    assert 0 < f["emax"] == e[y, x] < f["gmax"]
    ys, xs = np.nonzero((e == f["emax"]) & (mask != 0))
    assert len(ys) == 1
    nb = e[y - 1:y + 2, x - 1:x + 2]
    stronger = nb > e[y, x]
    assert stronger.any() and not (mask[y - 1:y + 2, x - 1:x + 2][stronger] != 0).any()
    # what a maximum taken over local maxima only would be, and that it changes the result
    c = e[1:-1, 1:-1]
    loc = np.ones_like(c, bool)
    for dy in range(3):
        for dx in range(3):
            loc &= c >= e[dy:dy + H - 2, dx:dx + W - 2]
    lmax = c[loc & (mask[1:-1, 1:-1] != 0)].max()
    assert lmax < f["emax"]
    v = e[f["masked"][:, 1].astype(int), f["masked"][:, 0].astype(int)]
    thr, thr_wrong = np.float32(np.float64(f["emax"]) * k["q"]), np.float32(np.float64(lmax) * k["q"])
    assert thr_wrong < thr and (v > thr).all() and len(v) >= 3
    al = (mask != 0)[1:-1, 1:-1]
    assert int((loc & al & (c > 0) & (c > thr_wrong) & ~(c > thr)).sum()) >= 1, "the wrong threshold admits more keys"


def test_all_zero_one_pixel_and_mask_values():
    assert M.expect("all_zero").shape == (0, 2)
    k = M.cases()["one_pixel"]
    ys, xs = np.nonzero(k["mask"])
    assert len(ys) == 1
    assert np.array_equal(M.expect("one_pixel"), np.array([[xs[0], ys[0]]], np.float32))
    v = M.cases()["values_1_and_128"]["mask"]
    assert set(np.unique(v).tolist()) == {0, 1, 128}
    assert np.array_equal(v != 0, M.cases()["crop_131x67"]["mask"] != 0)
    assert np.array_equal(M.expect("values_1_and_128"), M.expect("crop_131x67"))
    assert len(M.expect("crop_131x67")) == 40                # the budget is full again


def test_sizes_and_generic_kernel_cases():
    names = set(M.cases())
    for W, H in M.TILE_SIZES + M.GRID_SIZES:
        assert any(n.endswith(f"_{W}x{H}") for n in names), (W, H)
    for W, H in M.GRID_SIZES:
        assert {f"crop_{W}x{H}", f"noise_{W}x{H}"} <= names
    kinds = {(k["bs"], k["harris"]) for k in M.cases().values()}
    assert {(3, False), (3, True), (5, False), (7, True)} <= kinds
    # the list the budget does not cut is longer than any budget used here
    assert len(M.expect("crop_131x67_all_keys")) > 40
