"""Inputs and host model for goodFeaturesToTrack's mask (vo_gftt_masked, cv2compat's mask=).

mask_ref builds the masks a KLT front end passes (a disc blanked around every point it already
tracks); gftt_masked_model is oracle.eigmap, the masked key rule of OpenCV 4.6's featureselect.cpp (the maximum over the allowed pixels, the 3x3
test on the unmasked map, keys from allowed interior pixels only) and the sequential minDistance
walk.  test_gftt_mask_ref.py shows on the CPU what each case reaches (and that the model with an
all-set mask is oracle.gftt on every input); test_gpu_gftt_mask.py runs the same cases on the GPU.

The constants the sizes aim at (vo_gftt.hip): k_eig3 works on tiles of 58 columns x 64 rows, k_eignms
on tiles of 64 columns x 16 rows.
"""
import functools

import numpy as np

import gftt_cases as GC

QUALITY = 0.01
SEAM_QUALITY = 0.5


# ---------------------------------------------------------------------- disc masks
def mask_ref(W, H, pts, r):
    """[H][W] u8: 255, except 0 at (x, y) when some point (px, py) with both coordinates finite has
    dx * dx + dy * dy <= r * r in float64, dx = float64(x) - float64(px), one rounding per operation.
    The predicate is evaluated on a window three pixels wider than the disc on every side (no pixel
    outside it can satisfy it); test_gftt_mask_ref.py compares with a loop over every pixel."""
    m = np.full((H, W), 255, np.uint8)
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    r = np.float64(r)
    r2 = r * r
    for px, py in pts.astype(np.float64):
        if not (np.isfinite(px) and np.isfinite(py)):
            continue
        if px < -r - 3 or py < -r - 3 or px > W + r + 3 or py > H + r + 3:
            continue
        x0, x1 = max(int(np.floor(px - r)) - 3, 0), min(int(np.ceil(px + r)) + 4, W)
        y0, y1 = max(int(np.floor(py - r)) - 3, 0), min(int(np.ceil(py + r)) + 4, H)
        dx = np.arange(x0, x1, dtype=np.float64)[None, :] - px
        dy = np.arange(y0, y1, dtype=np.float64)[:, None] - py
        m[y0:y1, x0:x1][dx * dx + dy * dy <= r2] = 0
    return m


# ---------------------------------------------------------------------- the detector model
def masked_keys(img, mask, quality, block_size=3, use_harris=False):
    """(values, addresses, maximum over the mask or None) of the keys the masked detector keeps, in
    rank order (value descending, then larger address first)."""
    from oracle import _olib as O
    e = O.eigmap(img, block_size, use_harris)
    H, W = e.shape
    al = np.asarray(mask) != 0
    assert al.shape == e.shape
    if not al.any():
        return np.zeros(0, np.float32), np.zeros(0, np.int64), None
    emax = e[al].max()
    thr = np.float32(np.float64(emax) * np.float64(quality))
    c = e[1:-1, 1:-1]
    nb = np.full_like(c, -np.inf)
    for dy in range(3):
        for dx in range(3):
            nb = np.maximum(nb, e[dy:dy + H - 2, dx:dx + W - 2])
    ok = (c > 0) & (c >= nb) & (c > thr) & al[1:-1, 1:-1]
    ys, xs = np.nonzero(ok)
    addr = (ys + 1).astype(np.int64) * W + (xs + 1)
    v = c[ys, xs]
    order = np.lexsort((-addr, -v.astype(np.float64)))
    return v[order], addr[order], emax


def walk(addr, W, min_dist, max_corners):
    """gftt_cases.walk_model's sequential walk over a ranked address list"""
    xs = (addr % W).astype(np.float32)
    ys = (addr // W).astype(np.float32)
    want = max_corners if max_corners > 0 else len(addr)
    if min_dist < 1:
        n = min(want, len(addr))
        return np.stack([xs[:n], ys[:n]], 1).reshape(-1, 2)
    md2 = np.float64(min_dist) * np.float64(min_dist)
    ax = np.zeros(len(addr), np.float32)
    ay = np.zeros(len(addr), np.float32)
    n = 0
    for i in range(len(addr)):
        if n == want:
            break
        dx = xs[i] - ax[:n]
        dy = ys[i] - ay[:n]
        if ((dx * dx + dy * dy).astype(np.float64) < md2).any():
            continue
        ax[n], ay[n] = xs[i], ys[i]
        n += 1
    return np.stack([ax[:n], ay[:n]], 1).reshape(-1, 2)


def gftt_masked_model(img, mask, max_corners, quality, min_dist, block_size=3, use_harris=False):
    """float32 [n][2] corners of goodFeaturesToTrack(img, ..., mask=mask)"""
    _, addr, _ = masked_keys(img, mask, quality, block_size, use_harris)
    return walk(addr, img.shape[1], min_dist, max_corners)


def nms_only_through_masked(img, mask, quality, block_size=3, use_harris=False):
    """how many allowed interior pixels above the masked threshold are >= every allowed neighbour and
    fail the 3x3 test only because of a masked-out neighbour"""
    from oracle import _olib as O
    e = O.eigmap(img, block_size, use_harris)
    H, W = e.shape
    al = np.asarray(mask) != 0
    thr = np.float32(np.float64(e[al].max()) * np.float64(quality))
    c = e[1:-1, 1:-1]
    nb_all = np.full_like(c, -np.inf)
    nb_al = np.full_like(c, -np.inf)
    ea = np.where(al, e, -np.inf)
    for dy in range(3):
        for dx in range(3):
            nb_all = np.maximum(nb_all, e[dy:dy + H - 2, dx:dx + W - 2])
            nb_al = np.maximum(nb_al, ea[dy:dy + H - 2, dx:dx + W - 2])
    return int((al[1:-1, 1:-1] & (c > 0) & (c > thr) & (c >= nb_al) & ~(c >= nb_all)).sum())


# ---------------------------------------------------------------------- detector cases
TILE_SIZES = [(w, h) for w in (57, 58, 59, 117) for h in (63, 64, 65)]      # around k_eig3's 58 x 64 tile
GRID_SIZES = [(131, 67), (300, 37), (45, 300), (64, 64)]                    # gftt_cases' sizes


def tracked_points(img, max_corners, quality, min_dist, which, seed):
    """every second corner of the unmasked run (from the first or from the second), moved by a
    sub-pixel amount: what a tracker holds a frame later"""
    from oracle import _olib as O
    ref = O.gftt(img, max_corners, quality, min_dist)
    rng = np.random.default_rng(seed)
    p = ref[which::2]
    return (p + rng.uniform(-0.45, 0.45, p.shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(img, mask, mc, q, md, bs, harris)"""
    c = {}

    def add(name, img, mask, mc, md, bs=3, harris=False, q=QUALITY):
        c[name] = dict(img=img, mask=np.ascontiguousarray(mask, np.uint8), mc=mc, q=q, md=float(md), bs=bs,
                       harris=harris)

    def discs(img, mc, md, which, seed):
        H, W = img.shape
        return mask_ref(W, H, tracked_points(img, mc, QUALITY, md, which, seed), md)

    for i, (W, H) in enumerate(TILE_SIZES):
        kind = "crop" if i % 2 == 0 else "noise"
        img = GC.crop(W, H) if kind == "crop" else GC.noise(W, H, seed=i)
        add(f"{kind}_{W}x{H}", img, discs(img, 30, 5, i // 2 % 2, i), 30, 5)
    for i, (W, H) in enumerate(GRID_SIZES):
        for kind in ("crop", "noise"):
            img = GC.crop(W, H) if kind == "crop" else GC.noise(W, H)
            add(f"{kind}_{W}x{H}", img, discs(img, 40, 7, i % 2, 100 + i), 40, 7)
    # every key the mask leaves, as the engine's capacity allows (the budget does not cut the list)
    img = GC.crop(131, 67)
    add("crop_131x67_all_keys", img, discs(img, 40, 7, 0, 7), GC.MC, 2)
    # the maximum over the mask on the image border: the border and every interior pixel below the
    # border's maximum are allowed
    add("border_max", img, border_max_mask(img), 40, 5)
    add("all_zero", img, np.zeros(img.shape, np.uint8), 40, 7)
    add("one_pixel", img, one_pixel_mask(img), 40, 7)
    m = c["crop_131x67"]["mask"].copy()
    m[(m != 0) & (np.arange(m.shape[1])[None, :] % 2 == 0)] = 1
    m[m == 255] = 128
    add("values_1_and_128", img, m, 40, 7)
    # k_eignms: Harris, blockSize 5 and 7
    add("harris_bs3", img, discs(img, 40, 7, 1, 11), 40, 7, bs=3, harris=True)
    n = GC.noise(117, 65, seed=5)
    add("mineig_bs5", n, discs(n, 40, 7, 0, 12), 40, 7, bs=5)
    add("harris_bs7", GC.crop(64, 64), discs(GC.crop(64, 64), 40, 7, 0, 13), 40, 7, bs=7, harris=True)
    # the maximum over the mask is an interior pixel beside a stronger masked-out one, so it is no
    # local maximum of the map, and it lies on a tile seam: k_eig3's columns 57 | 58 and rows 63 | 64
    # (row 63 is a tile's last own row), k_eignms's columns 63 | 64 and rows 15 | 16
    n = GC.noise(131, 67, seed=21)
    for axis, line in (("col", 57), ("col", 58), ("row", 63), ("row", 64)):
        add(f"seam_{axis}{line}", n, seam_mask(n, axis, line)[0], 40, 5, q=SEAM_QUALITY)
    for axis, line in (("col", 63), ("col", 64), ("row", 15), ("row", 16)):
        add(f"seam_bs5_{axis}{line}", n, seam_mask(n, axis, line, 5)[0], 40, 5, bs=5, q=SEAM_QUALITY)
    return c


def border_max_mask(img):
    from oracle import _olib as O
    e = O.eigmap(img)
    b = np.zeros(e.shape, bool)
    b[0, :] = b[-1, :] = b[:, 0] = b[:, -1] = True
    m = b | (e < e[b].max())
    return np.where(m, 255, 0).astype(np.uint8)


def seam_mask(img, axis, line, block_size=3, use_harris=False):
    """(mask, (x, y)): allowed are the strongest interior pixel of column / row `line` that has a
    stronger neighbour, and every pixel below 0.6 of its value.  With SEAM_QUALITY = 0.5 the threshold
    is half that pixel's value; a maximum taken from any other allowed pixel gives 0.3 of it at most."""
    from oracle import _olib as O
    e = O.eigmap(img, block_size, use_harris)
    H, W = e.shape
    c = e[1:-1, 1:-1]
    nb = np.full_like(c, -np.inf)
    for dy in range(3):
        for dx in range(3):
            nb = np.maximum(nb, e[dy:dy + H - 2, dx:dx + W - 2])
    cand = np.zeros(e.shape, bool)
    cand[1:-1, 1:-1] = (nb > c) & (c > 0)
    on = np.zeros(e.shape, bool)
    if axis == "col":
        on[:, line] = True
    else:
        on[line, :] = True
    v = np.where(cand & on, e, -1)
    y, x = np.unravel_index(int(np.argmax(v)), v.shape)
    m = e < np.float32(0.6) * e[y, x]
    m[y, x] = True
    return np.where(m, 255, 0).astype(np.uint8), (int(x), int(y))


def one_pixel_mask(img):
    from oracle import _olib as O
    x, y = O.gftt(img, 40, QUALITY, 7)[3]
    m = np.zeros(img.shape, np.uint8)
    m[int(y), int(x)] = 255
    return m


@functools.lru_cache(maxsize=None)
def expect(name):
    k = cases()[name]
    return gftt_masked_model(k["img"], k["mask"], k["mc"], k["q"], k["md"], k["bs"], k["harris"])
