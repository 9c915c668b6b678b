"""goodFeaturesToTrack's mask on the GPU: vo_gftt_masked and cv2compat.goodFeaturesToTrack(mask=) against
gftt_mask_cases.gftt_masked_model, in both selection forms, through k_eig3 and k_eignms.  Every
comparison is np.array_equal.  What the cases reach is shown on the CPU by test_gftt_mask_ref.py.
"""
import ctypes as C

import numpy as np
import pytest

import gftt_cases as GC
import gftt_mask_cases as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT_PT = -7.0
_ENGINES = {}


def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.fixture
def sel_mode():
    from monocular_visual_odometry_va4mr_amd import _lib as L

    def set_(m):
        L.check(L.lib().vo_set_gftt_select(int(m)), "vo_set_gftt_select")
    yield set_
    set_(0)


# ------------------------------------------------------------------ vo_gftt_masked
def _engine(W, H, B=1):
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    from monocular_visual_odometry_va4mr_amd import options as O
    if (W, H, B) not in _ENGINES:
        opts, _, _ = O.get("kitti")
        opts.update(feature_max_corners=GC.MC)
        _ENGINES[W, H, B] = Engine(np.eye(3), opts, W, H, batch=B, ncap=256, pcap=256, fcap=4)
    return _ENGINES[W, H, B]


def detect(eng, frames, masks, k, pad=0, status=None):
    """vo_gftt_masked (masks None: vo_gftt_masked with a NULL mask) with the corner buffer pre-filled;
    the mask's padding holds 255.  Returns [(corners, nCorners)] per chain."""
    eng.opts.feature_quality_level = float(k["q"])
    eng.opts.feature_min_dist = float(k["md"])
    eng.opts.feature_max_corners = int(k["mc"])
    eng.opts.feature_block_size = int(k["bs"])
    eng.opts.feature_use_harris = int(k["harris"])
    eng.opts.harris_k = 0.04
    H, W = eng.H, eng.W
    eng.t["status"].zero_()
    eng.build_pyramid(np.stack(frames), 0)
    if status is not None:
        eng.t["status"].copy_(torch.tensor(status, dtype=torch.int32))
    eng.t["corners"].fill_(SENT_PT)
    eng.t["nCorners"].fill_(-5)
    if masks is None:
        rc = eng.lib.vo_gftt_masked(eng._pd, eng._po, eng._ps, 0, None, 0, 0, eng.stream)
    else:
        buf = np.full((eng.B, H, W + pad), 255, np.uint8)
        for b, m in enumerate(masks):
            buf[b, :, :W] = m
        d_m = torch.from_numpy(buf).cuda()
        rc = eng.lib.vo_gftt_masked(eng._pd, eng._po, eng._ps, 0, _p(d_m), H * (W + pad), W + pad, eng.stream)
        torch.cuda.synchronize()
        assert np.array_equal(d_m.cpu().numpy(), buf), "the mask was written"
    torch.cuda.synchronize()
    assert rc == 0
    corners = eng.t["corners"].cpu().numpy()
    ns = eng.t["nCorners"].cpu().numpy()
    out = []
    for b in range(eng.B):
        n = int(ns[b])
        if n >= 0:
            assert (corners[b, n:] == SENT_PT).all(), f"chain {b}: rows past nCorners written"
        out.append((corners[b, :max(n, 0)], n))
    eng.t["status"].zero_()
    return out


@pytest.mark.parametrize("name", list(M.cases()))
def test_gftt_masked_matches_model_both_selection_forms(sel_mode, name):
    k = M.cases()[name]
    want = M.expect(name)
    H, W = k["img"].shape
    eng = _engine(W, H)
    bad = []
    for mode in (1, 2):
        sel_mode(mode)
        for pad in ((0, 13) if name in ("crop_131x67", "noise_59x64", "mineig_bs5", "seam_col58") else (0,)):
            ((got, n),) = detect(eng, [k["img"]], [k["mask"]], k, pad=pad)
            if not (n == len(want) and np.array_equal(got, want)):
                bad.append((mode, pad, n, len(want)))
    assert not bad, f"{name}: (mode, pad, got, want) {bad}"


def test_gftt_masked_null_mask_is_vo_gftt(sel_mode):
    from oracle import _olib as O
    for name in ("crop_131x67", "noise_64x64", "harris_bs3"):
        k = M.cases()[name]
        H, W = k["img"].shape
        eng = _engine(W, H)
        want = O.gftt(k["img"], k["mc"], k["q"], k["md"], k["bs"], k["harris"])
        for mode in (1, 2):
            sel_mode(mode)
            ((got, n),) = detect(eng, [k["img"]], None, k)
            assert n == len(want) and np.array_equal(got, want), (name, mode)
            ((got, n),) = detect(eng, [k["img"]], [np.full((H, W), 255, np.uint8)], k)
            assert n == len(want) and np.array_equal(got, want), (name, mode, "all-set mask")


def test_gftt_masked_three_chains_one_stopped(sel_mode):
    """B = 3: one image under three masks (discs, the border-maximum mask, every pixel), the middle
    chain stopped: its corners and count keep their sentinels."""
    from oracle import _olib as O
    k = M.cases()["crop_131x67"]
    img = k["img"]
    H, W = img.shape
    masks = [k["mask"], M.cases()["border_max"]["mask"], np.full((H, W), 255, np.uint8)]
    wants = [M.gftt_masked_model(img, m, k["mc"], k["q"], k["md"]) for m in masks]
    assert np.array_equal(wants[2], O.gftt(img, k["mc"], k["q"], k["md"]))
    assert not np.array_equal(wants[0], wants[1]) and not np.array_equal(wants[0], wants[2])
    eng = _engine(W, H, B=3)
    for mode in (1, 2):
        sel_mode(mode)
        for status in (None, [0, 2, 0]):
            out = detect(eng, [img] * 3, masks, k, pad=5, status=status)
            for b in range(3):
                got, n = out[b]
                if status is not None and status[b]:
                    assert n == -5 and bool((eng.t["corners"][b] == SENT_PT).all()), (mode, b)
                else:
                    assert n == len(wants[b]) and np.array_equal(got, wants[b]), (mode, b, n, len(wants[b]))


def test_gftt_masked_rejects_bad_arguments():
    k = M.cases()["noise_64x64"]
    eng = _engine(64, 64)
    eng.build_pyramid(k["img"], 0)
    eng.t["corners"].fill_(SENT_PT)
    m = torch.full((64 * 64,), 255, dtype=torch.uint8, device="cuda")
    f = eng.lib.vo_gftt_masked
    assert f(eng._pd, eng._po, eng._ps, 0, _p(m), 64 * 64, 63, eng.stream) == -1
    assert f(eng._pd, eng._po, eng._ps, 0, _p(m), -1, 64, eng.stream) == -1
    assert f(eng._pd, eng._po, eng._ps, 2, _p(m), 64 * 64, 64, eng.stream) == -1
    assert f(None, eng._po, eng._ps, 0, _p(m), 64 * 64, 64, eng.stream) == -1
    torch.cuda.synchronize()
    assert bool((eng.t["corners"] == SENT_PT).all())


# ------------------------------------------------------------------ cv2compat.goodFeaturesToTrack(mask=)
@pytest.mark.parametrize("name", ["crop_131x67", "noise_58x65", "border_max", "seam_row63", "seam_bs5_col64", "one_pixel",
                                  "values_1_and_128", "harris_bs3", "mineig_bs5", "all_zero"])
def test_cv2compat_mask(name):
    from monocular_visual_odometry_va4mr_amd import cv2compat as G
    k = M.cases()[name]
    want = M.expect(name)
    mask0 = k["mask"].copy()
    got = G.goodFeaturesToTrack(k["img"], k["mc"], k["q"], k["md"], mask=k["mask"], blockSize=k["bs"],
                                useHarrisDetector=k["harris"])
    assert np.array_equal(k["mask"], mask0)
    if name == "all_zero":
        assert got is None
        return
    assert got.dtype == np.float32 and got.shape == (len(want), 1, 2)
    assert np.array_equal(got[:, 0, :], want)
    # a non-contiguous view of the same mask, and mask=None right after on the same engine
    wide = np.zeros((k["mask"].shape[0], 2 * k["mask"].shape[1]), np.uint8)
    wide[:, ::2] = k["mask"]
    got = G.goodFeaturesToTrack(k["img"], k["mc"], k["q"], k["md"], mask=wide[:, ::2], blockSize=k["bs"],
                                useHarrisDetector=k["harris"])
    assert np.array_equal(got[:, 0, :], want)
    from oracle import _olib as O
    plain = G.goodFeaturesToTrack(k["img"], k["mc"], k["q"], k["md"], blockSize=k["bs"], useHarrisDetector=k["harris"])
    assert np.array_equal(plain[:, 0, :], O.gftt(k["img"], k["mc"], k["q"], k["md"], k["bs"], k["harris"]))


def test_cv2compat_mask_errors():
    from monocular_visual_odometry_va4mr_amd import cv2compat as G
    k = M.cases()["crop_131x67"]
    img, m = k["img"], k["mask"]
    for bad in (m.astype(bool), m.astype(np.float32), m.astype(np.int32), m[:-1], m[:, :-1], m.T, m[None], m.ravel()):
        with pytest.raises(G.error):
            G.goodFeaturesToTrack(img, 40, 0.01, 7, mask=bad)
