"""Inputs and host references for the eigen pass of goodFeaturesToTrack (csrc/vo_gftt.hip): the tiled
generic kernel k_eignms at its 64 x 16 tile edges, for every block size and response, and the key
list's capacity ccap.  Importable without a GPU: test_eig_cases_ref.py shows on the oracle alone what
each input reaches, test_gpu_eig_generic.py and test_gpu_gftt_key_capacity.py run them through
libvo_hip.so (and test_gpu_eig3_filter.py takes its images and its reference from here).

The images of a size (NAMES, then one periodic image per block size):

  crop      a rendered frame's crop
  flat      a constant image: every box sum 0, no key, eig_max = fkey(0)
  binary    random 0 / 255 pixels: the largest box sums
  ramp      a pure horizontal ramp: det = 0, so Harris is negative wherever the box sees the ramp
  step      one vertical step edge: det = 0 along the edge
  checker   an 8-pixel checker: exactly equal neighbours
  col0      the map's maximum in image column 0    (not an NMS pixel, but in the maximum)
  lastrow   the map's maximum in image row H - 1
  periodic  one bs x bs cell repeated: the box sums of a bs x bs window do not depend on where it
            stands, so every pixel whose window stays clear of the reflected border ties, and every
            one of them is a local maximum (none for bs 1 and 2: a constant and a 2-periodic image
            have zero Sobel response)
"""
import functools

import numpy as np

NAMES = ("crop", "flat", "binary", "ramp", "step", "checker", "col0", "lastrow")

# around k_eignms's tile of 64 columns x 16 rows: one tile - 1, exact, + 1, two tiles + 1
TILE_WIDTHS = (63, 64, 65, 129)
TILE_HEIGHTS = (15, 16, 17, 33)
TILE_SIZES = [(w, h) for w in TILE_WIDTHS for h in TILE_HEIGHTS]
# sizes below the widest window: refl101 reflects more than once for blockSize 7 (reach 3 + 1 + 1)
TINY_SIZES = [(7, 5), (3, 3)]
SIZES = TILE_SIZES + TINY_SIZES

BLOCK_SIZES = (1, 2, 3, 4, 5, 6, 7)
HARRIS_K_OTHER = 0.15
# (name, useHarrisDetector, k, qualityLevel, minDistance): one quality and minDistance per response,
# see test_eig_cases_ref.test_detector_settings_keep_corners
RESPONSES = (
    ("mineig", False, 0.04, 0.01, 3.0),
    ("harris_k0.04", True, 0.04, 0.01, 3.0),
    ("harris_k0.15", True, HARRIS_K_OTHER, 0.01, 3.0),
)
CONFIGS = [(bs,) + r for bs in BLOCK_SIZES for r in RESPONSES]          # 21
MAX_CORNERS = 1024

# the cell seed of the periodic image per block size: among seeds 0-5 the one whose smallest count of
# local maxima over the three responses at 96 x 64 is largest (then the largest sum, then the lowest
# seed; test_eig_cases_ref.test_periodic_seeds_are_the_best_of_six)
PERIODIC_SEED = {1: 0, 2: 0, 3: 2, 4: 1, 5: 2, 6: 5, 7: 0}


@functools.lru_cache(maxsize=None)
def rendered_frame():
    from monocular_visual_odometry_va4mr_amd.synth import make_sequence
    return make_sequence("kitti", 1, seed=1)[0][0]


def images(W, H):
    """the eight images of NAMES, uint8 [8][H][W]; W >= 3 and H >= 3"""
    fr = rendered_frame()
    rng = np.random.default_rng(1000 * W + H)
    x = np.arange(W)[None, :].repeat(H, 0)
    y = np.arange(H)[:, None].repeat(W, 1)
    col0 = np.full((H, W), 50, np.uint8)
    col0[H // 2 - 1:H // 2 + 2, 0:2] = [[250, 250], [250, 10], [10, 10]]
    last = np.full((H, W), 50, np.uint8)
    c0 = min(20, W - 3)
    last[H - 2:H, c0:c0 + 3] = [[250, 10, 10], [10, 10, 250]]
    out = [
        fr[150:150 + H, 300:300 + W],
        np.full((H, W), 77, np.uint8),
        (rng.integers(0, 2, (H, W)) * 255),
        2 * x,
        np.where(x < W // 2, 40, 200),
        np.where((x // 8 + y // 8) % 2 == 0, 60, 190),
        col0,
        last,
    ]
    return np.stack([np.ascontiguousarray(a, dtype=np.uint8) for a in out])


def periodic(W, H, bs, seed=None, cols=None):
    """one bs x bs cell of default_rng(seed).integers(0, 256) repeated over the image; with cols, over
    its first cols columns only, the others flat"""
    seed = PERIODIC_SEED[bs] if seed is None else seed
    cell = np.random.default_rng(seed).integers(0, 256, (bs, bs))
    img = np.ascontiguousarray(np.tile(cell, (H // bs + 1, W // bs + 1))[:H, :W], dtype=np.uint8)
    if cols is not None:
        img[:, cols:] = 128
    return img


# the periodic chain of the map tests must fit the key list (ccap = W * H // 2 + 1024, engine.py), which
# a whole 129 x 33 image of ties does not: the pattern stops at this column
PERIODIC_COLS = 96


def chain_images(W, H, bs):
    """(names, uint8 [9][H][W]): the images of a launch at block size bs"""
    return NAMES + ("periodic",), np.concatenate([images(W, H), periodic(W, H, bs, cols=PERIODIC_COLS)[None]])


def fkey(v):
    """order-preserving u32 image of a float32 (vo_dev.h)"""
    u = np.asarray(v, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)


def local_maxima(e):
    """(ys, xs) of the interior pixels with v > 0 and v >= their 8 neighbours, in address order"""
    H, W = e.shape
    if H < 3 or W < 3:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    c = e[1:-1, 1:-1]
    nb = np.max([e[1 + i:H - 1 + i, 1 + j:W - 1 + j] for i in (-1, 0, 1) for j in (-1, 0, 1) if (i, j) != (0, 0)], axis=0)
    ys, xs = np.nonzero((c > 0) & (c >= nb))
    return ys + 1, xs + 1


def reference(img, bs=3, harris=False, k=0.04):
    """(sorted keys, eig_max key, eigen map) from the oracle's map: interior pixels with v > 0 and
    v >= their 8 neighbours, key = fkey(v) << 32 | y * W + x (vo_dev.h)."""
    from oracle import _olib as O
    e = O.eigmap(img, bs, harris, k)
    W = e.shape[1]
    ys, xs = local_maxima(e)
    keys = (fkey(e[ys, xs]) << np.uint64(32)) | (ys * W + xs).astype(np.uint64)
    return np.sort(keys), int(fkey(e.max())), e


# ---------------------------------------------------------------------- the masked form
MASK_CONFIGS = ((2, False), (4, False), (6, False), (5, True))          # (blockSize, useHarrisDetector), k = 0.04
MASK_SIZES = ((65, 17), (129, 33))
MASK_QUALITY, MASK_MIN_DIST, MASK_MAX_CORNERS = 0.01, 3.0, 40


@functools.lru_cache(maxsize=None)
def mask_cases():
    """name -> dict(img, mask, mc, q, md, bs, harris) in gftt_mask_cases' form: per size and
    configuration the disc mask of gftt_mask_cases (every second corner of the unmasked run blanked)
    and its seam masks on k_eignms's tile seams that are interior lines of the size (columns 63 | 64,
    rows 15 | 16)."""
    import gftt_cases as GC
    import gftt_mask_cases as M
    from oracle import _olib as O
    c = {}
    for (W, H) in MASK_SIZES:
        img = GC.crop(W, H)
        for i, (bs, harris) in enumerate(MASK_CONFIGS):
            tag = f"{W}x{H}_bs{bs}_{'harris' if harris else 'mineig'}"
            ref = O.gftt(img, MASK_MAX_CORNERS, MASK_QUALITY, MASK_MIN_DIST, bs, harris)
            rng = np.random.default_rng(50 + i)
            pts = (ref[i % 2::2] + rng.uniform(-0.45, 0.45, ref[i % 2::2].shape)).astype(np.float32)
            masks = {"disc": M.mask_ref(W, H, pts, MASK_MIN_DIST)}
            for axis, line in (("col", 63), ("col", 64), ("row", 15), ("row", 16)):
                if 1 <= line <= (W if axis == "col" else H) - 2:
                    masks[f"seam_{axis}{line}"] = M.seam_mask(img, axis, line, bs, harris)[0]
            for mname, m in masks.items():
                q = M.SEAM_QUALITY if mname.startswith("seam") else MASK_QUALITY
                c[f"{tag}_{mname}"] = dict(img=img, mask=np.ascontiguousarray(m, np.uint8), mc=MASK_MAX_CORNERS, q=q,
                                           md=MASK_MIN_DIST, bs=bs, harris=harris)
    return c


# ---------------------------------------------------------------------- the key list's capacity
CAP_W, CAP_H, CAP_B = 96, 64, 3
CAP_CCAP = CAP_W * CAP_H // 2 + 1024                      # the engine's own (engine.py): 4096
CAP_QUALITY, CAP_MIN_DIST, CAP_MAX_CORNERS = 0.01, 2.0, 8192
# kernel form -> (blockSize, useHarrisDetector, masked call): what launch_eig picks for it
CAP_FORMS = {
    "eig3_interval": (3, False, False),        # k_eig3<false>, the default
    "eig3_exact": (3, False, False),           # k_eig3<true>: a process with VO_EIG_EXACT=1
    "eig3_masked": (3, False, True),           # k_eig3<true, true>: an all-ones mask
    "eignms_bs5": (5, False, False),           # k_eignms<false>
    "eignms_harris_bs3": (3, True, False),     # k_eignms<false>
    "eignms_masked_bs5": (5, False, True),     # k_eignms<true>: an all-ones mask
}


def capacity_frames(bs):
    """uint8 [3][64][96]: crop, the periodic image of block size bs, crop flipped"""
    import gftt_cases as GC
    crop = GC.crop(CAP_W, CAP_H)
    return np.stack([crop, periodic(CAP_W, CAP_H, bs), np.ascontiguousarray(crop[::-1, ::-1])])


@functools.lru_cache(maxsize=None)
def capacity_reference(bs, harris):
    """per chain (sorted keys, corner list of oracle.gftt) at the capacity tests' detector settings"""
    from oracle import _olib as O
    out = []
    for img in capacity_frames(bs):
        keys, _, _ = reference(img, bs, harris)
        out.append((keys, O.gftt(img, CAP_MAX_CORNERS, CAP_QUALITY, CAP_MIN_DIST, bs, harris)))
    return out
