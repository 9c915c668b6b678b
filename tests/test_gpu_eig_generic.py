"""The generic eigen pass k_eignms (csrc/vo_gftt.hip) against the oracle's map: every block size 1..7
under min-eigenvalue, Harris k = 0.04 and Harris k = 0.15 (21 configurations; blockSize 3 with
min-eigenvalue goes through k_eig3 and stays as the control), at the sizes around its 64 x 16 tile and
at 7 x 5 and 3 x 3, on the images of eig_cases.py as the chains of one launch.  Per chain:

  keys, max   the sorted key set and eig_max of vo_gftt_keys against the ones formed from oracle.eigmap
  map         every pixel of vo_gftt_eigmap against oracle.eigmap
  corners     vo_gftt's corner list and count against oracle.gftt

then the masked form k_eignms<true> against gftt_mask_cases.gftt_masked_model, VO_EIG_GENERIC=1 (the
default configuration through k_eignms) in a process of its own, and cv2compat's blockSize / k.  Every
comparison is np.array_equal.  test_eig_cases_ref.py shows on the CPU what the inputs reach.

7 x 5 and 3 x 3 are included after reading the code for them: the pyramid build (k_pyr_rows level 0,
the only level with maxLevel 0) writes the 16-pixel border of such a level through refl101's loop and
the row loop of put_row; k_eignms reads pixel refl101(x) +- 1 and refl101(y) +- 1, inside that border,
and writes keys behind pos < ccap and map pixels behind x < W, y < H; k_eig3 holds its lanes inside
column W + 2 and its rows inside H + 1.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import eig_cases as E

SENT_PT = -7.0


def _engine(W, H, B, cache={}):
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    from monocular_visual_odometry_va4mr_amd import options as Op
    if (W, H, B) not in cache:
        opts, _, _ = Op.get("kitti")
        opts.update(feature_max_corners=E.MAX_CORNERS, maxLevel=0)
        cache[W, H, B] = Engine(np.eye(3), opts, W, H, batch=B, ncap=64, pcap=64, fcap=4)
    return cache[W, H, B]


def _configure(eng, bs, harris, k, q, md, mc):
    eng.opts.feature_block_size = int(bs)
    eng.opts.feature_use_harris = int(bool(harris))
    eng.opts.harris_k = float(k)
    eng.opts.feature_quality_level = float(q)
    eng.opts.feature_min_dist = float(md)
    eng.opts.feature_max_corners = int(mc)


def run_keys_and_maps(eng, imgs):
    """vo_gftt_keys, then vo_gftt_eigmap, over the chains `imgs` with the engine's detector options:
    per chain (sorted keys, eig_max), and the maps [B][H][W]"""
    import torch
    B, H, W = imgs.shape
    eng.t["status"].zero_()
    eng.build_pyramid(imgs, 0)
    assert eng.lib.vo_gftt_keys(eng._pd, eng._po, eng._ps, 0, eng.stream) == 0
    torch.cuda.synchronize()
    n = eng.t["gf_n"].cpu().numpy()
    assert (n >= 0).all() and (n <= eng.dims.ccap).all()
    keys = eng.t["gf_keys"].cpu().numpy().view(np.uint64)
    emax = eng.t["eig_max"].cpu().numpy().view(np.uint32)
    res = [(np.sort(keys[b, :n[b]]), int(emax[b])) for b in range(B)]
    assert eng.lib.vo_gftt_eigmap(eng._pd, eng._po, eng._ps, 0, eng.stream) == 0
    torch.cuda.synchronize()
    maps = eng.t["eig"].cpu().numpy().reshape(B, H, W).copy()
    emax2 = eng.t["eig_max"].cpu().numpy().view(np.uint32)
    assert np.array_equal(emax, emax2), "vo_gftt_keys and vo_gftt_eigmap disagree on the maximum"
    return res, maps


def run_corners(eng):
    """vo_gftt on the pyramid already built, the corner buffer pre-filled: [(corners, nCorners)]"""
    import torch
    eng.t["corners"].fill_(SENT_PT)
    eng.t["nCorners"].fill_(-5)
    assert eng.lib.vo_gftt(eng._pd, eng._po, eng._ps, 0, eng.stream) == 0
    torch.cuda.synchronize()
    assert not eng.t["status"].any()
    corners = eng.t["corners"].cpu().numpy()
    ns = eng.t["nCorners"].cpu().numpy()
    out = []
    for b in range(eng.B):
        n = int(ns[b])
        assert 0 <= n <= eng.dims.mcap, f"chain {b}: nCorners {n}"
        assert (corners[b, n:] == SENT_PT).all(), f"chain {b}: rows past nCorners written"
        out.append((corners[b, :n].copy(), n))
    return out


def generic_child(path):
    """the second process of test_generic_switch_runs_default_configuration: vo_gftt_keys and
    vo_gftt_eigmap at the engine's default configuration for every size and image of
    test_gpu_eig3_filter, into one .npz"""
    import test_gpu_eig3_filter as F
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    from monocular_visual_odometry_va4mr_amd import options as Op
    out = {"generic": np.int32(int(os.environ.get("VO_EIG_GENERIC", "0")))}
    for (W, H) in F.SIZES:
        opts, _, _ = Op.get("kitti")
        assert opts["feature_block_size"] == 3 and not opts["feature_use_harris"]
        imgs = E.images(W, H)
        eng = Engine(np.eye(3), opts, W, H, batch=len(imgs), ncap=64, pcap=64, fcap=4)
        res, maps = run_keys_and_maps(eng, imgs)
        for name, (k, m), e in zip(E.NAMES, res, maps):
            out[f"{W}x{H}_{name}_keys"] = k
            out[f"{W}x{H}_{name}_max"] = np.uint32(m)
            out[f"{W}x{H}_{name}_map"] = e
    np.savez(path, **out)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    generic_child(sys.argv[1])
    sys.exit(0)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture
def sel_mode():
    from monocular_visual_odometry_va4mr_amd import _lib as L

    def set_(m):
        L.check(L.lib().vo_set_gftt_select(int(m)), "vo_set_gftt_select")
    yield set_
    set_(0)


@pytest.mark.parametrize("W,H", E.SIZES)
def test_every_configuration_matches_oracle(W, H):
    """one engine per size, per configuration one launch of each entry point over the nine images"""
    from oracle import _olib as O
    assert os.environ.get("VO_EIG_GENERIC", "0") == "0", "this process keeps k_eig3 as the control"
    eng = _engine(W, H, len(E.NAMES) + 1)
    bad, ran = [], 0
    for (bs, rname, harris, k, q, md) in E.CONFIGS:
        names, imgs = E.chain_images(W, H, bs)
        _configure(eng, bs, harris, k, q, md, E.MAX_CORNERS)
        res, maps = run_keys_and_maps(eng, imgs)
        corners = run_corners(eng)
        ran += 1
        for b, (name, img) in enumerate(zip(names, imgs)):
            what = f"bs {bs} {rname} {name}"
            keys, kmax, e = E.reference(img, bs, harris, k)
            gk, gm = res[b]
            if not np.array_equal(maps[b], e):
                d = np.argwhere(maps[b] != e)
                bad.append(f"{what}: eigen map differs at {len(d)} pixels, first (y, x) {d[0].tolist()}")
            if gm != kmax:
                bad.append(f"{what}: eig_max {gm:#x} vs {kmax:#x}")
            if not (len(gk) == len(keys) and np.array_equal(gk, keys)):
                bad.append(f"{what}: {len(gk)} keys vs {len(keys)}")
            want = O.gftt(img, E.MAX_CORNERS, q, md, bs, harris, k)
            got, n = corners[b]
            if not (n == len(want) and np.array_equal(got, want)):
                bad.append(f"{what}: {n} corners vs {len(want)}")
            if bs == 1 or name == "flat" or (harris and name == "ramp"):
                assert len(keys) == 0 and len(want) == 0 and kmax <= 0x80000000, what    # "nothing found"
    print(f"{W}x{H}: {ran} configurations x {len(names)} images")
    assert ran == 21
    assert not bad, f"{W}x{H}: {len(bad)} differences: " + "; ".join(bad[:12])


def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("name", list(E.mask_cases()))
def test_masked_form_matches_model(sel_mode, name):
    """k_eignms<true>: blockSize 2, 4, 6 and Harris blockSize 5 under the disc and seam masks, both
    selection forms, the mask rows unpadded and padded"""
    import gftt_mask_cases as M
    k = E.mask_cases()[name]
    H, W = k["img"].shape
    want = M.gftt_masked_model(k["img"], k["mask"], k["mc"], k["q"], k["md"], k["bs"], k["harris"])
    eng = _engine(W, H, 1)
    _configure(eng, k["bs"], k["harris"], 0.04, k["q"], k["md"], k["mc"])
    bad = []
    for mode in (1, 2):
        sel_mode(mode)
        for pad in (0, 13):
            eng.t["status"].zero_()
            eng.build_pyramid(k["img"][None], 0)
            eng.t["corners"].fill_(SENT_PT)
            eng.t["nCorners"].fill_(-5)
            buf = np.full((1, H, W + pad), 255, np.uint8)
            buf[0, :, :W] = k["mask"]
            d_m = torch.from_numpy(buf).cuda()
            rc = eng.lib.vo_gftt_masked(eng._pd, eng._po, eng._ps, 0, _p(d_m), H * (W + pad), W + pad, eng.stream)
            torch.cuda.synchronize()
            assert rc == 0
            n = int(eng.t["nCorners"][0])
            got = eng.t["corners"][0].cpu().numpy()
            assert 0 <= n <= eng.dims.mcap and (got[n:] == SENT_PT).all()
            if not (n == len(want) and np.array_equal(got[:n], want)):
                bad.append((mode, pad, n, len(want)))
    assert not bad, f"{name}: (mode, pad, got, want) {bad}"


def test_generic_switch_runs_default_configuration(tmp_path):
    """VO_EIG_GENERIC=1 in a process of its own: k_eignms at blockSize 3 with min-eigenvalue gives, for
    every size and image of test_gpu_eig3_filter, the oracle's keys, maxima and maps (which is what
    test_gpu_eig3_filter asserts of k_eig3)."""
    import test_gpu_eig3_filter as F
    path = str(tmp_path / "generic.npz")
    env = dict(os.environ, VO_EIG_GENERIC="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True,
                       timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    g = np.load(path)
    assert int(g["generic"]) == 1
    bad = []
    for (W, H) in F.SIZES:
        for name, img in zip(E.NAMES, E.images(W, H)):
            keys, kmax, e = E.reference(img)
            t = f"{W}x{H}_{name}"
            if int(g[t + "_max"]) != kmax:
                bad.append(t + ": eig_max")
            if not np.array_equal(g[t + "_keys"], keys):
                bad.append(t + f": {len(g[t + '_keys'])} keys vs {len(keys)}")
            if not np.array_equal(g[t + "_map"], e):
                bad.append(t + ": eigen map")
    assert not bad, f"{len(bad)} differences: " + "; ".join(bad[:12])


def test_cv2compat_block_size_and_k():
    from monocular_visual_odometry_va4mr_amd import cv2compat as G
    from oracle import _olib as O
    img = E.images(129, 33)[0]
    q, md = 0.01, 3.0
    want = O.gftt(img, 100, q, md, 4, True, E.HARRIS_K_OTHER)
    assert len(want) >= 10 and not np.array_equal(want, O.gftt(img, 100, q, md, 4, True, 0.04))
    got = G.goodFeaturesToTrack(img, 100, q, md, blockSize=4, useHarrisDetector=True, k=E.HARRIS_K_OTHER)
    assert got.dtype == np.float32 and got.shape == (len(want), 1, 2)
    assert np.array_equal(got[:, 0, :], want)
    # beyond the kernel's window: an error, never the result of a clamped block size
    with pytest.raises((RuntimeError, ValueError, G.error)):
        G.goodFeaturesToTrack(img, 100, q, md, blockSize=8)
