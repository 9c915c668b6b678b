"""What the inputs of eig_cases.py reach, shown on the CPU oracle alone: test_gpu_eig_generic.py and
test_gpu_gftt_key_capacity.py compare the GPU with the same oracle on the same inputs, and a
comparison of two empty key lists would prove nothing.  No GPU, no libvo_hip.so.
"""
import numpy as np
import pytest

import eig_cases as E

W0, H0 = 65, 17                           # one tile of k_eignms + 1 in both directions


def _by_name(W, H, bs):
    names, imgs = E.chain_images(W, H, bs)
    return dict(zip(names, imgs))


def _tied(keys):
    """how many keys share their value with another key"""
    v = (keys >> np.uint64(32)).astype(np.uint64)
    _, inv, cnt = np.unique(v, return_inverse=True, return_counts=True)
    return int((cnt[inv] >= 2).sum())


def test_sizes_and_configurations():
    assert len(E.TILE_SIZES) == 16 and len(E.SIZES) == 18 and len(E.CONFIGS) == 21
    assert {c[0] for c in E.CONFIGS} == set(range(1, 8))
    assert E.HARRIS_K_OTHER != 0.04
    for (W, H) in E.SIZES:
        names, imgs = E.chain_images(W, H, 5)
        assert imgs.shape == (9, H, W) and imgs.dtype == np.uint8 and len(names) == 9


def test_images_are_those_of_the_eig3_filter_test():
    """test_gpu_eig3_filter.py takes images / reference from here: same pixels as before at its sizes"""
    fr = E.rendered_frame()
    for (W, H) in ((58, 63), (117, 129)):
        im = E.images(W, H)
        assert np.array_equal(im[0], fr[150:150 + H, 300:300 + W])
        assert np.array_equal(im[7][H - 2:H, 20:23], [[250, 10, 10], [10, 10, 250]])
        assert (im[7][:H - 2] == 50).all() and (im[7][:, :20] == 50).all() and (im[7][:, 23:] == 50).all()


@pytest.mark.parametrize("bs,name,harris,k,q,md", [c for c in E.CONFIGS if c[0] >= 2], ids=lambda v: str(v))
def test_block_sizes_2_to_7_reach_keys_ties_edges(bs, name, harris, k, q, md):
    im = _by_name(W0, H0, bs)
    keys, kmax, e = E.reference(im["crop"], bs, harris, k)
    assert len(keys) >= 20, f"crop: {len(keys)} keys"
    ckeys, _, _ = E.reference(im["checker"], bs, harris, k)
    assert _tied(ckeys) >= 20, f"checker: {_tied(ckeys)} keys in exact-tie runs"
    # a key on the first or last NMS row / column (next to the image edge), in some image
    edge = 0
    for nm, img in im.items():
        kk, _, _ = E.reference(img, bs, harris, k)
        a = (kk & np.uint64(0xFFFFFFFF)).astype(np.int64)
        x, y = a % W0, a // W0
        edge += int(((x == 1) | (x == W0 - 2) | (y == 1) | (y == H0 - 2)).sum())
    assert edge >= 1
    _, _, e0 = E.reference(im["col0"], bs, harris, k)
    assert np.argmax(e0) % W0 == 0 and e0.max() > 0, "col0: the maximum is not in column 0"
    if harris:
        _, rmax, er = E.reference(im["ramp"], bs, harris, k)
        assert (er < 0).all(), "ramp: Harris is not negative at every pixel"
        assert rmax < 0x80000000 and rmax == int(E.fkey(er.max())), "eig_max is the fkey of a negative float"
        from oracle import _olib as O
        assert len(O.gftt(im["ramp"], E.MAX_CORNERS, q, md, bs, harris, k)) == 0
        assert (e < 0).any() and (e > 0).any(), "crop: Harris has one sign only"


@pytest.mark.parametrize("name,harris,k,q,md", E.RESPONSES, ids=[r[0] for r in E.RESPONSES])
def test_block_size_1_finds_nothing(name, harris, k, q, md):
    """det = 0 with one gradient per box: min-eigenvalue is exactly 0 (the square root is exact),
    Harris is -k T^2 <= 0 with exact zeros where the gradient vanishes: no key, no corner"""
    from oracle import _olib as O
    for (W, H) in ((W0, H0), (7, 5), (3, 3)):
        for nm, img in _by_name(W, H, 1).items():
            keys, kmax, e = E.reference(img, 1, harris, k)
            assert len(keys) == 0 and kmax <= 0x80000000
            if harris:
                assert (e <= 0).all() and (e == 0).any() and e.max() == 0 and kmax == 0x80000000
                if nm in ("crop", "binary"):
                    assert (e < 0).any()
            else:
                assert (e == 0).all() and not np.signbit(e).any() and kmax == 0x80000000
            assert len(O.gftt(img, E.MAX_CORNERS, q, md, 1, harris, k)) == 0


@pytest.mark.parametrize("bs", E.BLOCK_SIZES)
def test_periodic_image_ties_over_most_of_the_interior(bs):
    for (W, H) in E.TILE_SIZES + [(E.CAP_W, E.CAP_H)]:
        img = E.chain_images(W, H, bs)[1][-1]
        assert np.array_equal(img[:, :E.PERIODIC_COLS], E.periodic(W, H, bs)[:, :E.PERIODIC_COLS])
        for (name, harris, k, q, md) in E.RESPONSES:
            keys, _, e = E.reference(img, bs, harris, k)
            r = bs // 2 + 2
            wp = min(W, E.PERIODIC_COLS)
            if bs <= 2:
                assert len(keys) == 0 and (e[:, :wp - r] == 0).all()          # zero Sobel response
                continue
            # more keys than half the interior (of the pattern's columns, where it stops short of W)
            assert 2 * len(keys) > (wp - 2) * (H - 2), f"{W}x{H} {name}: {len(keys)} keys"
            # one value over the pixels whose window is clear of the border and of the pattern's end
            assert len(np.unique(e[r:H - r, r:wp - r])) == 1


def test_every_key_list_fits_the_engines():
    """the map tests never reach ccap = W * H // 2 + 1024 (test_gpu_gftt_key_capacity.py does, on purpose)"""
    for (W, H) in E.SIZES:
        for (bs, name, harris, k, q, md) in E.CONFIGS:
            for nm, img in _by_name(W, H, bs).items():
                n = len(E.reference(img, bs, harris, k)[0])
                assert n <= W * H // 2 + 1024 - 64, f"{W}x{H} bs {bs} {name} {nm}: {n} keys"


def test_periodic_seeds_are_the_best_of_six():
    for bs in (3, 4, 5, 6, 7):
        score = {}
        for seed in range(6):
            n = [len(E.reference(E.periodic(E.CAP_W, E.CAP_H, bs, seed), bs, h, k)[0]) for (_, h, k, _, _) in E.RESPONSES]
            score[seed] = (min(n), sum(n), -seed)
        assert max(score, key=score.get) == E.PERIODIC_SEED[bs], (bs, score)
    assert len(E.reference(E.periodic(E.CAP_W, E.CAP_H, 3), 3)[0]) == 5520


def test_detector_settings_keep_corners():
    """the quality and minDistance of each response leave crop and binary at least 10 corners at every
    tile size and block size >= 2, and the periodic image a tie run to walk"""
    from oracle import _olib as O
    for (W, H) in E.TILE_SIZES:
        for (bs, name, harris, k, q, md) in E.CONFIGS:
            if bs < 2:
                continue
            im = _by_name(W, H, bs)
            for nm in ("crop", "binary"):
                n = len(O.gftt(im[nm], E.MAX_CORNERS, q, md, bs, harris, k))
                assert 10 <= n < E.MAX_CORNERS, f"{W}x{H} bs {bs} {name} {nm}: {n} corners"
            if bs >= 3:
                assert 10 <= len(O.gftt(im["periodic"], E.MAX_CORNERS, q, md, bs, harris, k)) < E.MAX_CORNERS


def test_tiny_sizes_still_yield_keys():
    """3 x 3 has one NMS pixel; it is a key at block sizes 2 and 4 in several images, and at every
    block size >= 2 the maps, which the GPU test compares pixel by pixel, are not all zero there"""
    for (name, harris, k, q, md) in E.RESPONSES:
        for bs in (2, 4):
            n = [len(E.reference(img, bs, harris, k)[0]) for img in E.chain_images(3, 3, bs)[1]]
            assert max(n) == 1 and sum(n) >= 1, (bs, name, n)
        for bs in range(2, 8):
            for (W, H) in E.TINY_SIZES:
                assert sum(bool(E.reference(img, bs, harris, k)[2].any()) for img in E.chain_images(W, H, bs)[1]) >= 4
    n75 = sum(len(E.reference(img, bs, h, k)[0]) for (bs, _, h, k, _, _) in E.CONFIGS for img in E.chain_images(7, 5, bs)[1])
    assert n75 >= 20


def test_mask_cases_mask_something():
    import gftt_mask_cases as M
    from oracle import _olib as O
    cases = E.mask_cases()
    assert {(k["bs"], k["harris"]) for k in cases.values()} == set(E.MASK_CONFIGS)
    assert {k["img"].shape[::-1] for k in cases.values()} == set(E.MASK_SIZES)
    changed = 0
    for name, k in cases.items():
        assert k["mask"].shape == k["img"].shape and (k["mask"] == 0).any() and (k["mask"] != 0).any(), name
        want = M.gftt_masked_model(k["img"], k["mask"], k["mc"], k["q"], k["md"], k["bs"], k["harris"])
        plain = O.gftt(k["img"], k["mc"], k["q"], k["md"], k["bs"], k["harris"])
        assert len(want) >= 1, name
        changed += not np.array_equal(want, plain)
        ones = np.full(k["img"].shape, 255, np.uint8)
        assert np.array_equal(M.gftt_masked_model(k["img"], ones, k["mc"], k["q"], k["md"], k["bs"], k["harris"]), plain)
    assert changed >= len(cases) - 2, f"only {changed} of {len(cases)} masks change the corner list"


def test_capacity_inputs_overflow_the_key_list():
    assert E.CAP_CCAP == 4096
    seen = set()
    for form, (bs, harris, masked) in E.CAP_FORMS.items():
        ref = E.capacity_reference(bs, harris)
        n = [len(k) for k, _ in ref]
        assert n[1] > E.CAP_CCAP, f"{form}: the periodic image has {n[1]} keys"
        assert 20 <= n[0] < E.CAP_CCAP // 8 and 20 <= n[2] < E.CAP_CCAP // 8, f"{form}: crop has {n[0]}, {n[2]} keys"
        # the corner lists: a walk of thousands on the periodic image, at least two corners (no
        # VO_ST_GFTT_NONE / _ONE) on the neighbours, all below the corner and candidate capacity
        c = [len(x) for _, x in ref]
        assert 1000 < c[1] < E.CAP_MAX_CORNERS and 2 <= c[0] < E.CAP_MAX_CORNERS and 2 <= c[2] < E.CAP_MAX_CORNERS, (form, c)
        assert not np.array_equal(ref[0][1], ref[2][1])
        seen.add((bs, harris))
    assert seen == {(3, False), (5, False), (3, True)}
