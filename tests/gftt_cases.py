"""Inputs for the corner selection of goodFeaturesToTrack (k_gftt_select and the split k_gsel_*) at
the regimes rendered frames never reach, and a host model of the walk.

Every case is (image, quality, minDistance, maxCorners).  The expected corner list always comes from
oracle.gftt; walk_model exists to show on the CPU that an input can tell a right selection from a
wrong one (test_gftt_cases_ref.py), and test_gpu_gftt_select_edges.py runs the same cases through
both selection forms.

The constants the cases aim at (vo_select.hip): k_gftt_select takes its keys in pages of PAGE = 4096,
decides inside a page on exact conflict lists and consults its cell grid only for corners accepted
on earlier pages; the grid's cells are cvRound(minDistance) pixels wide; the split form takes cells
up to 255 pixels wide whose u64 grid fits the eigen-map scratch (cells * 8 + 4 <= 4 * W * H).
"""
import functools

import numpy as np

PAGE = 4096
# where k_gftt_select keeps its cell grid (vo_select.hip): in LDS up to GRID_LDS_CELLS cells that fit
# the LDS budget beside the page and the accepted corners (at most ACC_MAX of them there), else in
# the chain's W * H u32 of scratch behind the conflict lists, else in that scratch with no room for
# the lists (the wave-serial walk)
GRID_LDS_CELLS = 22528
ACC_MAX = 8192
LDS_BUDGET = 150 * 1024


# ---------------------------------------------------------------------- the host model
def passing_keys(img, quality):
    """(values, addresses) of the keys that pass the quality gate, in rank order: interior pixels of
    oracle.eigmap with v > 0 that are >= their eight neighbours, above float32(double(max) * quality),
    by value descending and then by larger address first."""
    from oracle import _olib as O
    e = O.eigmap(img)
    H, W = e.shape
    thr = np.float32(np.float64(e.max()) * np.float64(quality))
    c = e[1:-1, 1:-1]
    nb = np.full_like(c, -np.inf)
    for dy in range(3):
        for dx in range(3):
            nb = np.maximum(nb, e[dy:dy + H - 2, dx:dx + W - 2])
    ok = (c > 0) & (c >= nb) & (c > thr)
    ys, xs = np.nonzero(ok)
    addr = (ys + 1).astype(np.int64) * W + (xs + 1)
    v = c[ys, xs]
    order = np.lexsort((-addr, -v.astype(np.float64)))
    return v[order], addr[order]


def walk_model(img, quality, min_dist, max_corners, lose=None):
    """OpenCV's sequential minDistance walk over passing_keys: a candidate is accepted when no accepted
    corner is closer than min_dist (float32 dx * dx + dy * dy compared in double against md * md; no
    test at all below min_dist 1).  lose=(x, y) forgets that accepted corner for the candidates of
    rank >= PAGE: what a grid that dropped it does to the later pages."""
    W = img.shape[1]
    _, addr = passing_keys(img, quality)
    xs = (addr % W).astype(np.float32)
    ys = (addr // W).astype(np.float32)
    want = max_corners if max_corners > 0 else len(addr)
    if min_dist < 1:
        n = min(want, len(addr))
        return np.stack([xs[:n], ys[:n]], 1).reshape(-1, 2)
    md2 = np.float64(min_dist) * np.float64(min_dist)
    ax = np.zeros(len(addr), np.float32)
    ay = np.zeros(len(addr), np.float32)
    seen = np.ones(len(addr), bool)                # which accepted corners later candidates still see
    n = 0
    for i in range(len(addr)):
        if n == want:
            break
        if i == PAGE and lose is not None:
            seen[:n] &= ~((ax[:n] == lose[0]) & (ay[:n] == lose[1]))
        dx = xs[i] - ax[:n]
        dy = ys[i] - ay[:n]
        if ((dx * dx + dy * dy).astype(np.float64)[seen[:n]] < md2).any():
            continue
        ax[n], ay[n] = xs[i], ys[i]
        n += 1
    return np.stack([ax[:n], ay[:n]], 1)


def tie_runs(img, quality):
    """(start rank, length) of every run of exactly equal values among the passing keys"""
    v, _ = passing_keys(img, quality)
    if len(v) == 0:
        return []
    cut = np.flatnonzero(np.diff(v) != 0) + 1
    st = np.concatenate([[0], cut])
    en = np.concatenate([cut, [len(v)]])
    return list(zip(st.tolist(), (en - st).tolist()))


def cells_of(corners, min_dist):
    """cell index pairs (x // cs, y // cs) of a corner list, cs = cvRound(min_dist)"""
    cs = int(np.rint(min_dist))
    return [(int(x) // cs, int(y) // cs) for x, y in corners]


# ---------------------------------------------------------------------- images
@functools.lru_cache(maxsize=None)
def rendered_frame():
    from monocular_visual_odometry_va4mr_amd.synth import make_sequence
    return make_sequence("kitti", 1, seed=1)[0][0]


def crop(W, H):
    fr = rendered_frame()
    y0 = min(150, fr.shape[0] - H)
    assert y0 >= 0 and 300 + W <= fr.shape[1]
    return np.ascontiguousarray(fr[y0:y0 + H, 300:300 + W])


def noise(W, H, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W)).astype(np.uint8)


def _dots(W, H, background, strong, weak, patch):
    """single bright pixels on a flat patch of 128: `strong` [(x, y, value)] and `weak` [(x, y)] of
    value 131; `background` is the image they are put on"""
    img = background.copy()
    r = patch // 2
    for (x, y, *_) in list(strong) + list(weak):
        img[y - r:y + r + 1, x - r:x + r + 1] = 128
    for (x, y, v) in strong:
        img[y, x] = v
    for (x, y) in weak:
        img[y, x] = 131
    return img


# three corners pairwise >= md apart inside one cell of cvRound(md) pixels, and one weak corner
# within md of exactly one of them (and of nothing else the walk accepts before it).  For md 15.5
# the noise leaves the corner of the image flat: at that spacing accepted noise corners would lie
# within md of every weak corner.
THREE_MD40 = dict(md=40.0, strong=[(120, 80, 255), (159, 90, 254), (130, 119, 253)],
                  weak=[(104, 72), (175, 90), (130, 135)], patch=11, flat=None)
THREE_MD15_5 = dict(md=15.5, strong=[(16, 16, 255), (31, 20, 254), (20, 31, 253)],
                    weak=[(8, 10), (39, 24), (22, 39)], patch=7, flat=(58, 58))
THREE_QUALITY = 0.0005
MC = 8192                       # the engine's largest corner capacity: both selection forms apply


@functools.lru_cache(maxsize=None)
def three_in_cell(which, one_page=False):
    """(image, quality, md, the three strong corners), 320x240.  On pixel noise in 90..165 more than
    PAGE keys pass and the weak corners rank last, on a later page than the strong ones; the one_page
    variant puts the same dots on a flat background."""
    g = THREE_MD40 if which == "md40" else THREE_MD15_5
    W, H = 320, 240
    if one_page:
        bg = np.full((H, W), 100, np.uint8)
    else:
        bg = np.random.default_rng(0).integers(90, 166, (H, W)).astype(np.uint8)
        if g["flat"]:
            bg[:g["flat"][1], :g["flat"][0]] = 128
    img = _dots(W, H, bg, g["strong"], g["weak"], g["patch"])
    return img, THREE_QUALITY, g["md"], [(x, y) for x, y, _ in g["strong"]]


def checker(W, H):
    """4-pixel checker, 60 / 190: every corner of it has the same eigenvalue.  The lowest sixth of
    the image is flat with single dots of falling strength, whose keys (and those along the edge of
    the checker) rank after the run of equal values."""
    x = np.arange(W)[None, :].repeat(H, 0)
    y = np.arange(H)[:, None].repeat(W, 1)
    img = np.where((x // 4 + y // 4) % 2 == 0, 60, 190).astype(np.uint8)
    h0 = H - H // 6
    img[h0:] = 128
    for i, v in enumerate([255, 220, 190, 160, 140, 134, 131]):
        if 20 + 40 * i < W - 2:
            img[(h0 + H) // 2, 20 + 40 * i] = v
    return np.ascontiguousarray(img)


@functools.lru_cache(maxsize=None)
def checker4():
    return checker(320, 240)


CHECKER_QUALITY = 0.0005


def binary(W, H):
    """random 0 / 255 pixels (the `binary` image of test_gpu_eig3_filter.py): many short tie runs"""
    rng = np.random.default_rng(1000 * W + H)
    return np.ascontiguousarray(rng.integers(0, 2, (H, W)) * 255, dtype=np.uint8)


SPARSE_DOTS = [(30, 30, 250), (100, 40, 200), (60, 90, 150)]


@functools.lru_cache(maxsize=None)
def sparse_dots():
    """(image, eigenvalue of the second-strongest dot / that of the strongest): three single pixels
    of different strength on a flat frame, one key each"""
    from oracle import _olib as O
    img = np.full((120, 160), 40, np.uint8)
    for (x, y, v) in SPARSE_DOTS:
        img[y, x] = v
    e = O.eigmap(img)
    (x0, y0, _), (x1, y1, _) = SPARSE_DOTS[:2]
    return img, float(np.float64(e[y1, x1]) / np.float64(e[y0, x0]))


# ---------------------------------------------------------------------- the cases
# grid geometry: (W, H) -> minDistance values; each on a rendered-frame crop and on noise
GRID_EDGES = {
    (131, 67): (1.5, 2.5, 7, 10, 15.5),      # sizes no multiple of the cell; lrint: 1.5 -> 2, 2.5 -> 2, 15.5 -> 16
    (300, 37): (40, 255, 256),               # one grid row; the split form's widest cell, and its fallback
    (45, 300): (50,),                        # one grid column
    (64, 64): (1.0, 1.6, 0.99, 0),           # the split form's scratch test on either side; no grid
}
GRID_QUALITY = 0.01


def split_applies(W, H, md, mc):
    """vo_gftt's conditions for the split form (mcap = min(mc, 8192))"""
    if md < 1 or mc < 1 or mc > 8192:
        return False
    cs = int(np.rint(md))
    cells = -(-W // cs) * -(-H // cs)
    return cs <= 255 and cells * 8 + 4 <= 4 * W * H


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (image, quality, minDistance, maxCorners)"""
    c = {}
    for which in ("md40", "md15_5"):
        for one_page in (False, True):
            img, q, md, _ = three_in_cell(which, one_page)
            c[f"three_in_cell_{which}" + ("_one_page" if one_page else "")] = (img, q, md, MC)
    ck = checker4()
    for md in (1.6, 2):
        c[f"checker4_md{md}"] = (ck, CHECKER_QUALITY, md, MC)
    c["checker4_md40"] = (ck, THREE_QUALITY, 40.0, MC)           # the mixed launch's configuration
    c["binary_md2"] = (binary(320, 240), 0.01, 2, MC)
    for name, mc in ties_cut().items():
        c[name] = (ck, CHECKER_QUALITY, 2, mc)
    c["checker_64_md1.6"] = (checker(64, 64), CHECKER_QUALITY, 1.6, MC)  # more keys than W * H / 8
    for (W, H), mds in GRID_EDGES.items():
        for md in mds:
            c[f"crop_{W}x{H}_md{md}"] = (crop(W, H), GRID_QUALITY, md, MC)
            c[f"noise_{W}x{H}_md{md}"] = (noise(W, H), GRID_QUALITY, md, MC)
    # a grid that fits neither LDS nor the scratch behind the conflict lists (k_gftt_select's
    # wave-serial walk over the L2 grid): 6,000 cells of 2 pixels, where the split form applies, and
    # 8,777 cells of 1 pixel, where it does not
    c["noise_200x120_md2.5"] = (noise(200, 120), GRID_QUALITY, 2.5, MC)
    c["binary_131x67_md1.49"] = (binary(131, 67), GRID_QUALITY, 1.49, MC)
    c["noise_64x64_md1.6_mc1"] = (noise(64, 64), GRID_QUALITY, 1.6, 1)
    c["noise_64x64_md1.6_mc0"] = (noise(64, 64), GRID_QUALITY, 1.6, 0)
    c["noise_64x64_md1.6_mc-1"] = (noise(64, 64), GRID_QUALITY, 1.6, -1)
    sp, r = sparse_dots()
    c["sparse_0_keys"] = (sp, 1.0, 10, MC)
    c["sparse_1_key"] = (sp, r * (1 + 1e-3), 10, MC)
    c["sparse_2_keys"] = (sp, r * (1 - 1e-3), 10, MC)
    return c


@functools.lru_cache(maxsize=None)
def ties_cut():
    """name -> maxCorners for checker4 at md 2: the list ends between two accepted corners of equal
    value on the first page, on a later page, and after the first corner"""
    from oracle import _olib as O
    ck = checker4()
    full = O.gftt(ck, 0, CHECKER_QUALITY, 2)
    v, addr = passing_keys(ck, CHECKER_QUALITY)
    rank = {int(a): i for i, a in enumerate(addr)}
    r = np.array([rank[int(y) * ck.shape[1] + int(x)] for x, y in full])
    first = int(np.searchsorted(r, PAGE // 2))            # a cut inside page 0
    later = int(np.searchsorted(r, PAGE + PAGE // 2))     # a cut inside page 1
    return {"ties_cut_page0": first, "ties_cut_page1": later, "ties_cut_mc1": 1}


@functools.lru_cache(maxsize=None)
def expect(name):
    from oracle import _olib as O
    img, q, md, mc = cases()[name]
    return O.gftt(img, mc, q, md)


@functools.lru_cache(maxsize=None)
def capacity_case():
    """(image, quality, md) with more corners than the 8192 an engine holds at most: what
    goodFeaturesToTrack meets with maxCorners <= 0"""
    return noise(512, 320), GRID_QUALITY, 1
