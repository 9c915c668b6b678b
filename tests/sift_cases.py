"""Deterministic small images for the SIFT stage tests (test_gpu_sift_stages.py) and descriptor
sets with planted ties for the matcher's tie-order tests (test_gpu_bf_ties.py).

test_sift_cases_ref.py proves on the CPU, with the oracle alone, that each case reaches the path it
is named for; the GPU tests run every case listed here and never filter.

Sizes (W, H) sit around the 64 x 32 blur tile on the 2x-upsampled octave 0, the 64 x 16 extrema tile,
the largest blur radius (13: the reflection folds more than once on the small octaves), the
5-pixel extrema border (octaves that hold no interior pixel are skipped) and odd halvings.
"""
import numpy as np

SIZES = [(1, 1), (2, 3), (5, 5), (6, 40), (40, 6), (12, 12), (31, 15), (32, 16), (33, 17), (63, 31), (65, 33),
         (33, 97), (97, 33), (131, 67), (200, 150)]
KINDS = ["blob", "noise", "binnoise2x", "checker6", "hstripes3", "vstripes3", "squares", "dots6", "const", "ramp"]
MAIN = (131, 67)                      # the size every content kind is run at

# (W, H, kind): every size with blob content, every content kind at 131 x 67
CASES = [(w, h, "blob") for (w, h) in SIZES] + [(MAIN[0], MAIN[1], k) for k in KINDS if k != "blob"]
# cases whose extrema lists are compared
EXTREMA_CASES = [(MAIN[0], MAIN[1], k) for k in KINDS] + [(65, 33, "blob"), (33, 97, "blob"), (200, 150, "blob")]


def case_id(case):
    return f"{case[2]}-{case[0]}x{case[1]}"


_CACHE = {}


def image(kind, W, H):
    """uint8 [H, W] image of the named content (read-only, cached)."""
    key = (kind, int(W), int(H))
    if key not in _CACHE:
        img = np.ascontiguousarray(_make(kind, int(W), int(H)), dtype=np.uint8)
        assert img.shape == (H, W)
        img.setflags(write=False)
        _CACHE[key] = img
    return _CACHE[key]


def _make(kind, W, H):
    y, x = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(1000 * KINDS.index(kind) + 7 * W + H)
    if kind == "blob":
        # uniform noise, 7 x 7 box sums (edge-replicated), stretched to 0..255 in integers
        n = np.pad(rng.integers(0, 256, (H, W), dtype=np.int64), 3, mode="edge")
        s = sum(n[dy:dy + H, dx:dx + W] for dy in range(7) for dx in range(7))
        lo, hi = int(s.min()), int(s.max())
        return (s - lo) * 255 // max(hi - lo, 1)
    if kind == "noise":
        return rng.integers(0, 256, (H, W))
    if kind == "binnoise2x":
        b = 255 * rng.integers(0, 2, ((H + 1) // 2, (W + 1) // 2))
        return np.repeat(np.repeat(b, 2, axis=0), 2, axis=1)[:H, :W]
    if kind == "checker6":
        return ((x // 6 + y // 6) % 2) * 255
    if kind == "hstripes3":
        return ((y // 3) % 2) * 255
    if kind == "vstripes3":
        return ((x // 3) % 2) * 255
    if kind == "squares":
        return ((x % 14 < 7) & (y % 14 < 7)) * 255
    if kind == "dots6":
        return ((x % 6 < 2) & (y % 6 < 2)) * 255
    if kind == "const":
        return np.full((H, W), 200)
    if kind == "ramp":
        return (x + y) * 255 // max(W + H - 2, 1)
    raise ValueError(kind)


_REF = {}


def reference(case):
    """Oracle results of a case, computed once and shared: (stages dict, keypoints, descriptors)."""
    if case not in _REF:
        from oracle import _olib as O
        img = image(case[2], case[0], case[1])
        st = O.sift_stages(img)
        kp, desc = O.sift(img)
        for a in [st["up"], st["extrema"], kp, desc] + st["gauss"] + st["dog"]:
            a.setflags(write=False)
        _REF[case] = (st, kp, desc)
    return _REF[case]


# ------------------------------------------------------------------ matcher tie cases
BF_QCAP, BF_TCAP = 300, 4200
BF_POOL_SIZES = [(200, 4100), (300, 2049), (129, 129), (33, 128), (1, 127), (70, 37), (64, 5)]
BF_TT = 128                           # train rows per tile of the default (int8) kernel
BF_QB = 128                           # queries per block
BF_MAXSPLIT = 16
BF_TARGET = 2048                      # work items the device plan aims at


def bf_device_plan(sizes):
    """The device plan of csrc/vo_match.hip (k_bf_i8 / bf_plan) restated: per problem (splits, rows
    per split) for a batch with the given (nq, nt) counts."""
    nqb = [(nq + BF_QB - 1) // BF_QB if nq > 0 else 0 for nq, _ in sizes]
    tot = sum(nqb)
    sp_all = min(BF_MAXSPLIT, max(1, (BF_TARGET + tot - 1) // tot)) if tot > 0 else 1
    out = []
    for nq, nt in sizes:
        tiles = (nt + BF_TT - 1) // BF_TT
        sp = max(1, min(sp_all, tiles))
        per = (((nt + sp - 1) // sp + BF_TT - 1) // BF_TT) * BF_TT
        out.append((sp, per))
    return out


def _query_of(row):
    q = row.copy()
    q[..., :4] = np.minimum(q[..., :4] + 1, 255)
    return q


def bf_pool_batch():
    """Train rows drawn from a pool of 8 rows, queries = pool rows with the first four entries + 1:
    the nearest distance is 2.0, tied over about nt / 8 train rows.  Returns q [B, qcap, 128],
    t [B, tcap, 128] float32 and the (nq, nt) list."""
    rng = np.random.default_rng(20)
    pool = rng.integers(0, 255, (8, 128)).astype(np.float32)       # 0..254: the + 1 never clips
    B = len(BF_POOL_SIZES)
    q = np.zeros((B, BF_QCAP, 128), np.float32)
    t = np.zeros((B, BF_TCAP, 128), np.float32)
    for b, (nq, nt) in enumerate(BF_POOL_SIZES):
        members = rng.integers(0, 8 if nt >= 16 else 2, nt)
        t[b, :nt] = pool[members]
        twice = np.flatnonzero(np.bincount(members, minlength=8) >= 2)   # rows that can tie
        q[b, :nq] = _query_of(pool[twice[rng.integers(0, len(twice), nq)]])
    return q, t, list(BF_POOL_SIZES)


BF_PLANT_NQ, BF_PLANT_NT = 140, 2049          # two query blocks; 17 tiles, the last of one row
BF_PLANT_OFFSETS = [1, 4, 8, 31, 32, 127, 128]


def bf_planted_batch():
    """Random train rows with one pool row planted at chosen index sets only, one set per problem:
    pairs (a, a + d) for d in BF_PLANT_OFFSETS and a in (0, 130), one pair with an index in each of
    two train splits of the device plan, and the triple (a, a + 4, a + 128).  Every query of the
    problem is the planted row + 1 on four entries (queries 0, 1, 2, 139) or a random row.
    Returns q, t, sizes and the planted index tuples."""
    rng = np.random.default_rng(21)
    plants = [(a, a + d) for d in BF_PLANT_OFFSETS for a in (130, 0)]
    B = len(plants) + 3
    sizes = [(BF_PLANT_NQ, BF_PLANT_NT)] * B
    sp, per = bf_device_plan(sizes)[0]
    assert sp >= 2 and per < BF_PLANT_NT
    plants.append((per - 1, per))                 # the last row of split 0 and the first of split 1
    plants.append((3, BF_PLANT_NT - 1))           # the first split and the one-row last tile
    plants.append((130, 134, 258))
    q = rng.integers(0, 256, (B, BF_PLANT_NQ, 128)).astype(np.float32)
    t = rng.integers(0, 256, (B, BF_PLANT_NT, 128)).astype(np.float32)
    for b, idx in enumerate(plants):
        row = rng.integers(0, 255, 128).astype(np.float32)
        for i in idx:
            t[b, i] = row
        for qi in (0, 1, 2, BF_PLANT_NQ - 1):
            q[b, qi] = _query_of(row)
    return q, t, sizes, plants


def bf_fixup_batch():
    """0 / 255 descriptors from pools: queries at density 0.9, train rows at density 0.1, so every
    squared distance is far above 2^22 (the float-order fix-up path) and every query's nearest
    rows are tied over the copies of a pool row."""
    rng = np.random.default_rng(22)
    sizes = [(150, 700), (64, 65), (5, 130)]
    qcap, tcap = 150, 700
    tp = (255 * (rng.random((8, 128)) < 0.1)).astype(np.float32)
    qp = (255 * (rng.random((8, 128)) < 0.9)).astype(np.float32)
    B = len(sizes)
    q = np.zeros((B, qcap, 128), np.float32)
    t = np.zeros((B, tcap, 128), np.float32)
    for b, (nq, nt) in enumerate(sizes):
        t[b, :nt] = tp[rng.integers(0, 8, nt)]
        q[b, :nq] = qp[rng.integers(0, 8, nq)]
    return q, t, sizes


def bf_many_batch(B=1025):
    """B problems of at most 4 x 4 descriptors with ties (counts 0..4): above BF_PLAN_MAXB = 1024
    problems the matcher takes the capacity plan by itself."""
    rng = np.random.default_rng(23)
    pool = rng.integers(0, 255, (2, 128)).astype(np.float32)
    nq = rng.integers(0, 5, B)
    nt = rng.integers(0, 5, B)
    q = np.zeros((B, 4, 128), np.float32)
    t = np.zeros((B, 4, 128), np.float32)
    for b in range(B):
        t[b, :nt[b]] = pool[rng.integers(0, 2, nt[b])]
        q[b, :nq[b]] = _query_of(pool[rng.integers(0, 2, nq[b])])
    return q, t, [(int(a), int(c)) for a, c in zip(nq, nt)]


_BF_REF = {}


def bf_reference(name, q, t, sizes):
    """O.bf_knn2 per problem, computed once per named batch: list of (idx [nq, 2], dist [nq, 2])."""
    if name not in _BF_REF:
        from oracle import _olib as O
        out = []
        for b, (nq, nt) in enumerate(sizes):
            i, d = O.bf_knn2(np.ascontiguousarray(q[b, :nq]), np.ascontiguousarray(t[b, :nt]))
            i.setflags(write=False)
            d.setflags(write=False)
            out.append((i, d))
        _BF_REF[name] = out
    return _BF_REF[name]
