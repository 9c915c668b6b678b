"""Inputs for vo_add_corners_finish (k_add_finish and k_add_finish_lean, csrc/vo_add.hip) and a NumPy
model of feature adding and the step's bookkeeping (VisualOdometryPipeLine.py:248-268, :360-373).

A case is one launch: an image size, min_dist, pcap and a list of chains, each with its candidates,
the detector's corners (set directly; no detector runs) and its counters.  test_gpu_add_finish.py
shows on the CPU that the model is the reference's rule and that every case reaches what it is named
for, and runs the cases through both kernels.

The constants the cases aim at (vo_add.hip): candidates are filed in a grid of at most ADD_MAX_CELLS
cells of ceil(min_dist) pixels (at least 1; grown until the grid fits), one spare cell before the
image and two after it, candidates outside going to the border cells.  k_add_finish (1024 threads)
keeps the cell-sorted list in LDS up to ADD_MAX_ITEMS candidates and in the chain's int scratch
beyond, if it fits there; k_add_finish_lean (256 threads) keeps the fill counters and the list in the
scratch (ADD_MAX_CELLS + P ints) behind uint16 cell starts (P < 65536).  Otherwise every corner is
tested against every candidate.  Corners are appended in chunks of one block.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

ADD_MAX_CELLS = 8192
ADD_MAX_ITEMS = 16384
ST_PNP_FAILED, ST_GFTT_NONE, ST_GFTT_ONE, ST_CAPACITY = 2, 3, 4, 5
W0, H0 = 64, 48
FCAP = 8
CHUNKS = (256, 1024)                    # corners per chunk of the ordered append, lean and full


def f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, 2))


@dataclass
class Chain:
    cand: np.ndarray                    # [P][2] candidates before the call
    corners: np.ndarray                 # [>= max(M, 0)][2]
    n_corners: int = None               # nCorners; default len(corners)
    status: int = 0
    nF: int = 2
    nInl: int = 7
    intent: list = field(default_factory=list)      # (corner index, kept?) the placement is built for

    def __post_init__(self):
        self.cand, self.corners = f32(self.cand), f32(self.corners)
        if self.n_corners is None:
            self.n_corners = len(self.corners)

    # what c_first / c_tau hold for the candidates before the call: distinct from c_kp and from nF
    @property
    def first(self):
        return self.cand - np.float32(0.5)

    @property
    def tau(self):
        return (np.arange(len(self.cand)) % self.nF).astype(np.int32)


@dataclass
class Case:
    min_dist: float
    chains: list
    pcap: int = 1024
    ncap: int = 4096                    # with pcap, sizes the engine's int scratch
    W: int = W0
    H: int = H0
    iwork_stride: int = None            # vo_dims.iwork_stride of the call, if not the engine's


def engine_iwork_stride(case):
    """Engine.__init__'s int scratch per chain"""
    return 2 * max(case.pcap, case.ncap) + 4096


def cell_size(case):
    cs = max(int(np.ceil(case.min_dist)), 1)
    while (case.W // cs + 3) * (case.H // cs + 3) > ADD_MAX_CELLS:
        cs += 1
    return cs


def path(case, chain, lean):
    """'grid' or 'all_pairs': which test the form runs for this chain (vo_add.hip's predicates)"""
    P = len(chain.cand)
    stride = case.iwork_stride if case.iwork_stride is not None else engine_iwork_stride(case)
    if lean:
        return "grid" if P < 65536 and ADD_MAX_CELLS + P <= stride else "all_pairs"
    return "grid" if P <= ADD_MAX_ITEMS or P <= stride else "all_pairs"


# ---------------------------------------------------------------------- the model
def kept(corners, cand, min_dist):
    """:258 in float32: corner j is kept iff sqrt(dx * dx + dy * dy) > float32(min_dist) for every
    candidate"""
    corners, cand = f32(corners), f32(cand)
    if len(cand) == 0:
        return np.ones(len(corners), bool)
    dx = corners[:, None, 0] - cand[None, :, 0]
    dy = corners[:, None, 1] - cand[None, :, 1]
    d = np.sqrt(dx * dx + dy * dy)
    assert d.dtype == np.float32
    return (d > np.float32(min_dist)).all(axis=1)


def kept_literal(pts, potential_keys, min_dist):
    """the expression of VisualOdometryPipeLine.py:258 as it stands"""
    return np.array([np.all(np.linalg.norm(pts[i, :] - potential_keys, axis=1) > min_dist) for i in range(pts.shape[0])],
                    dtype=bool)


def model(case):
    """Per chain what the call leaves: c_kp, c_first, c_tau over [0, nC), nC, nF, num_pts, status.
    Only candidates that existed before the call count (quirk Q4)."""
    out = []
    for ch in case.chains:
        P, nF = len(ch.cand), ch.nF
        r = dict(c_kp=ch.cand, c_first=ch.first, c_tau=ch.tau, nC=P, nF=nF, num_pts=np.zeros(FCAP, np.int32),
                 status=ch.status)
        M = ch.n_corners
        if ch.status != 0:
            pass                                               # a stopped chain is untouched
        elif M < 0:
            r["status"] = ST_CAPACITY
        elif M == 0:
            r["status"] = ST_GFTT_NONE
        elif M == 1:
            r["status"] = ST_GFTT_ONE
        else:
            new = ch.corners[:M][kept(ch.corners[:M], ch.cand, case.min_dist)]
            if len(new) > case.pcap - P:
                new = new[:case.pcap - P]
                r["status"] = ST_CAPACITY
            r["c_kp"] = np.concatenate([ch.cand, new])
            r["c_first"] = np.concatenate([ch.first, new])
            r["c_tau"] = np.concatenate([ch.tau, np.full(len(new), nF, np.int32)])
            r["nC"] = P + len(new)
            r["num_pts"][nF] = ch.nInl
            r["nF"] = nF + 1
        out.append(r)
    return out


FIELDS = ("c_kp", "c_first", "c_tau", "nC", "nF", "num_pts", "status")


# ---------------------------------------------------------------------- the distance boundary
BACKGROUND = [(2.0, 2.0), (62.0, 46.0), (32.5, 2.5), (32.0, 45.0)]     # far from both spots
DIRS8 = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]


def boundary_scenarios(md):
    """(name, corner relative to the lower edge of its cell, candidates relative to the corner,
    kept?) for min_dist md in (5, 7), cells of md pixels"""
    h = md / 2.0
    exact = {5: [(3, 4), (-4, 3), (5, 0), (0, -5)], 7: [(7, 0), (0, 7), (-7, 0), (0, -7)]}[md]
    outside = {5: [(4, 4), (5, 1), (3.00001, 4)], 7: [(5, 5), (7, 1), (7.00001, 0)]}[md]
    sc = []
    for k, o in enumerate(exact):
        sc.append((f"exact{k}", (h, h), [o], False))
    for k, o in enumerate(outside):
        sc.append((f"outside{k}", (h, h), [o], True))
    for (ex, ey) in DIRS8:
        # from the cell's middle into the neighbouring cell, within md ...
        sc.append((f"nb{ex}{ey}", (h, h), [(ex * (h + 0.5), ey * (h + 0.5))], False))
        # ... and past it
        sc.append((f"far{ex}{ey}", (h, h), [(ex * (md + 0.75), ey * (md + 0.75))], True))
    # the corner in a corner of its cell, the candidate in the far corner of the diagonal cell
    sc.append(("diag_far_nw", (0.25, 0.25), [(-md, -md)], True))
    sc.append(("diag_far_se", (md - 0.25, md - 0.25), [(md, md)], True))
    # the corner on the cells' common corner, the candidate deep in the diagonal cell (at exactly
    # md for 5)
    sc.append(("diag_deep", (0.0, 0.0), [{5: (-4, -3), 7: (-4, -5)}[md]], False))
    # sub-pixel corners: exact, just inside and just outside
    sc.append(("frac_exact", (h - 0.25, h + 0.25), [exact[0]], False))
    sc.append(("frac_in", (h + 0.375, h - 0.125), [(outside[0][0] - 1.0, outside[0][1] - 0.5)], False))
    sc.append(("frac_out", (h + 0.375, h - 0.125), [outside[0], outside[1]], True))
    return sc


def boundary_case(md):
    """Two scenarios per chain, in cells 30 (md 5) or 28 (md 7) pixels apart, so that no candidate of
    one is within reach of the other's corner; plus a stopped chain and nCorners of -1, 0 and 1."""
    kx = {5: (3, 9), 7: (2, 6)}[md]
    ky = {5: 4, 7: 3}[md]
    sc = boundary_scenarios(md)
    if len(sc) % 2:
        sc.append(sc[0])
    chains = []
    for a, b in zip(sc[0::2], sc[1::2]):
        cand, cor, intent = list(BACKGROUND), [], []
        for k, (_, loc, offs, keep) in enumerate((a, b)):
            c = (md * kx[k] + loc[0], md * ky + loc[1])
            cor.append(c)
            cand += [(c[0] + o[0], c[1] + o[1]) for o in offs]
            intent.append((k, keep))
        chains.append(Chain(cand, cor, nF=2 + len(chains) % 4, nInl=10 + len(chains), intent=intent))
    live = chains[0]
    chains.insert(3, Chain(live.cand, live.corners, status=ST_PNP_FAILED, nF=3))       # stopped
    chains.insert(5, Chain(live.cand, live.corners, n_corners=-1))
    chains.insert(8, Chain(live.cand, live.corners, n_corners=0))
    chains.append(Chain(live.cand, live.corners, n_corners=1))
    return Case(float(md), chains)


# ---------------------------------------------------------------------- the other placements
def outside_case(md):
    """candidates that left the image on every side, corners along its edges"""
    cand = [(-30, 10), (W0 + 30, 10), (10, -30), (10, H0 + 30), (-30, -30), (W0 + 30, H0 + 30), (-30.5, 40.25),
            (20, 20)]
    cor = [(0, 10), (63, 10), (10, 0), (10, 47), (2, 2), (61, 45), (3.5, 40.25), (4.5, 40.25), (40, 30), (20, 24.5)]
    return Case(float(md), [Chain(cand, cor), Chain(cand[::-1][:5], cor[::-1], nF=4)])


def zero_dist_case():
    """min_dist 0: cells of one pixel; only a corner exactly on a candidate goes"""
    cand = [(10, 10), (20.5, 7.25), (30, 30), (63, 47), (0, 0), (40.75, 12.5)]
    cor = [(10, 10), (10.001, 10), (20.5, 7.25), (20.5, 7.375), (30, 31), (63, 47), (0, 0), (1, 0), (40.75, 12.5),
           (40.875, 12.5), (50, 20)]
    intent = [(0, False), (1, True), (2, False), (3, True), (4, True), (5, False), (6, False), (7, True), (8, False),
              (9, True), (10, True)]
    return Case(0.0, [Chain(cand, cor, intent=intent)])


def growth_case():
    """100 x 100 at min_dist 1: 103 * 103 cells do not fit, so the cells grow to 2 pixels"""
    rng = np.random.default_rng(5)
    gx, gy = np.meshgrid(np.arange(18), np.arange(18))
    cor = np.stack([3.0 + 5.25 * gx.ravel(), 2.5 + 5.25 * gy.ravel()], 1)
    offs = np.array([(1, 0), (0, -1), (0.75, 0.75), (0.6, 0.8), (-1.5, 0), (-0.5, 0.5), (0, 1.0625)])
    pick = rng.integers(-1, len(offs), len(cor))                 # -1: no candidate near this corner
    cand = np.array([c + offs[k] for c, k in zip(cor, pick) if k >= 0])
    return Case(1.0, [Chain(rng.permutation(cand), cor)], W=100, H=100)


@functools.lru_cache(maxsize=None)
def _seam_chain(M):
    """M corners on a 1.5-pixel lattice in shuffled order, min_dist 1; a corner goes iff it has a
    candidate of its own 0.25 beside it.  Which ones go alternates irregularly, with one run of
    rejects across each chunk boundary of either form that M reaches."""
    rng = np.random.default_rng(M)
    gx, gy = np.meshgrid(np.arange(42), np.arange(32))
    lattice = np.stack([0.75 + 1.5 * gx.ravel(), 0.75 + 1.5 * gy.ravel()], 1)
    cor = rng.permutation(lattice)[:M]
    reject = rng.random(M) < 0.4
    for c in CHUNKS:
        reject[max(c - 6, 0):c + 6] = True
    cand = rng.permutation(cor[reject] + np.array([0.25, 0.0]))
    return Chain(cand, cor, intent=[(j, not reject[j]) for j in range(M)])


def seam_case(M):
    return Case(1.0, [_seam_chain(M)], pcap=2048)


def seam_capacity_case(cut):
    """M = 1100 with room for the kept corners before corner `cut` only"""
    ch = _seam_chain(1100)
    keep = np.array([k for _, k in ch.intent])
    return Case(1.0, [ch], pcap=len(ch.cand) + int(keep[:cut].sum()))


def dense_case(P, pcap, M=100, iwork_stride=None, ncap=64, seed=0):
    """B = 1: P candidates over the left 40 columns, M corners over the whole image, min_dist 3"""
    rng = np.random.default_rng(1000 * seed + P)
    cand = rng.uniform([0, 0], [40, H0], (P, 2))
    cor = rng.uniform([0, 0], [W0, H0], (M, 2))
    return Case(3.0, [Chain(cand, cor, nF=5)], pcap=pcap, ncap=ncap, iwork_stride=iwork_stride)


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    for md in (5, 7):
        c[f"boundary_md{md}"] = boundary_case(md)
    c["outside_md5"] = outside_case(5)              # candidates clamped into the border cells
    c["outside_md35"] = outside_case(35)            # cells wide enough for them to reject a corner
    c["zero_dist"] = zero_dist_case()
    c["growth_100x100_md1"] = growth_case()
    c["seam_m257"] = seam_case(257)
    c["seam_m1025"] = seam_case(1025)
    c["seam_capacity_lean"] = seam_capacity_case(384)        # runs out in the lean form's second chunk
    c["seam_capacity_full"] = seam_capacity_case(1060)       # ... and in the full form's
    c["items_lds_p16384"] = dense_case(ADD_MAX_ITEMS, 16640)                      # full: the last in LDS
    c["items_iwork_p16385"] = dense_case(ADD_MAX_ITEMS + 1, 16640)                # full: the first in iwork
    c["all_pairs_p16385"] = dense_case(ADD_MAX_ITEMS + 1, 16640, iwork_stride=ADD_MAX_ITEMS)
    c["lean_grid_pcap4096"] = dense_case(3900, 4096)         # iwork_stride 12288 >= 8192 + P
    c["lean_all_pairs_pcap256"] = dense_case(150, 256)       # iwork_stride 4608 < 8192
    c["p65535"] = dense_case(65535, 65536)                   # lean: the last grid size
    c["p65536"] = dense_case(65536, 65536)                   # lean: the first all-pairs size
    return c
