"""k_eig3's interval filter: the key set and the maximum of the eigen pass (vo_gftt_keys), read
before the selection consumes them, against the ones formed from the oracle's eigen map.

k_eig3 decides the 3x3 NMS on f32 intervals and evaluates the exact double expression only for
the pixels the intervals cannot rule out (csrc/vo_gftt.hip); the keys, the maximum and the eigen
map of vo_gftt_eigmap must be bit for bit what the exact evaluation of every pixel gives.  The
sizes sit around the tile edges (one 58-column tile, one + 1, halo lanes exhausted at 61, two
tiles + 1; 64-row tiles - 1, exact, + 1, two + 1); one launch per size mixes the images:

  crop      a rendered frame's crop
  flat      a constant image: every box sum 0, no key, eig_max = fkey(0)
  binary    random 0 / 255 pixels: T >= 2^24, where fl(T) rounds
  ramp      a pure horizontal ramp: det = 0, v is 0 or what the cancellation leaves
  step      one vertical step edge: det = 0 along the edge
  checker   an 8-pixel checker: exactly equal neighbours, the overlapping-interval path (and,
            with most pixels flagged, the rows the queue has no room for)
  col0      the map's maximum in image column 0    (not an NMS pixel, but in the maximum)
  lastrow   the map's maximum in image row H - 1

VO_EIG_EXACT=1 (every pixel exact) is read once per process, so that setting runs in a second
process over the same images and must give the same keys.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import eig_cases as EC

WIDTHS = (58, 59, 61, 117)
HEIGHTS = (63, 64, 65, 129)
SIZES = [(w, h) for w in WIDTHS for h in HEIGHTS]
NAMES = EC.NAMES
rendered_frame = EC.rendered_frame
images = EC.images          # the eight images above (eig_cases.py, shared with test_gpu_eig_generic.py)
fkey = EC.fkey
reference = EC.reference    # (sorted keys, eig_max key, eigen map) of the oracle's map, here at its defaults


def run_gpu(W, H, with_map=True):
    """One launch of vo_gftt_keys over the size's images: per chain (sorted keys, eig_max); and the
    eigen maps of vo_gftt_eigmap."""
    import torch
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    from monocular_visual_odometry_va4mr_amd import options as Op
    opts, _, _ = Op.get("kitti")
    imgs = images(W, H)
    B = len(imgs)
    eng = Engine(np.eye(3), opts, W, H, batch=B, ncap=64, pcap=64, fcap=4)
    eng.build_pyramid(imgs, 0)
    assert eng.lib.vo_gftt_keys(eng._pd, eng._po, eng._ps, 0, eng.stream) == 0
    torch.cuda.synchronize()
    n = eng.t["gf_n"].cpu().numpy()
    assert (n >= 0).all() and (n <= eng.dims.ccap).all()
    keys = eng.t["gf_keys"].cpu().numpy().view(np.uint64)
    emax = eng.t["eig_max"].cpu().numpy().view(np.uint32)
    res = [(np.sort(keys[b, :n[b]]), int(emax[b])) for b in range(B)]
    maps = None
    if with_map:
        assert eng.lib.vo_gftt_eigmap(eng._pd, eng._po, eng._ps, 0, eng.stream) == 0
        torch.cuda.synchronize()
        maps = eng.t["eig"].cpu().numpy().reshape(B, H, W)
        emax2 = eng.t["eig_max"].cpu().numpy().view(np.uint32)
        assert np.array_equal(emax, emax2), "vo_gftt_keys and vo_gftt_eigmap disagree on the maximum"
    return res, maps


if __name__ == "__main__":
    # the second process of test_exact_everywhere_agrees: every size's keys into one .npz
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = {}
    for (W, H) in SIZES:
        res, _ = run_gpu(W, H, with_map=False)
        for name, (k, m) in zip(NAMES, res):
            out[f"{W}x{H}_{name}_keys"] = k
            out[f"{W}x{H}_{name}_max"] = np.uint32(m)
    np.savez(sys.argv[1], **out)
    sys.exit(0)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_GOT = {}


def got(W, H):
    assert os.environ.get("VO_EIG_EXACT", "0") == "0", "this process must run the interval form"
    if (W, H) not in _GOT:
        _GOT[W, H] = run_gpu(W, H)
    return _GOT[W, H]


@pytest.mark.parametrize("W,H", SIZES)
def test_keys_and_max_match_oracle_map(W, H):
    res, maps = got(W, H)
    for b, (name, img) in enumerate(zip(NAMES, images(W, H))):
        keys, kmax, e = reference(img)
        gk, gm = res[b]
        assert np.array_equal(maps[b], e), f"{name}: eigen map differs"
        assert gm == kmax, f"{name}: eig_max {gm:#x} vs {kmax:#x}"
        assert len(gk) == len(keys) and np.array_equal(gk, keys), f"{name}: {len(gk)} keys vs {len(keys)}"
        if name == "flat":
            assert len(keys) == 0 and kmax == 0x80000000
        elif name in ("crop", "binary", "checker"):
            assert len(keys) > 10
        elif name == "col0":
            assert np.argmax(e) % W == 0 and (e == e.max()).sum() == 1
        elif name == "lastrow":
            assert np.argmax(e) // W == H - 1 and (e == e.max()).sum() == 1


def test_exact_everywhere_agrees(tmp_path):
    """VO_EIG_EXACT=1 in a process of its own: the same keys and maxima for every size and image."""
    path = str(tmp_path / "exact.npz")
    env = dict(os.environ, VO_EIG_EXACT="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True,
                       timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    ex = np.load(path)
    for (W, H) in SIZES:
        res, _ = got(W, H)
        for name, (k, m) in zip(NAMES, res):
            assert int(ex[f"{W}x{H}_{name}_max"]) == m, f"{W}x{H} {name}: eig_max differs"
            assert np.array_equal(ex[f"{W}x{H}_{name}_keys"], k), f"{W}x{H} {name}: keys differ"
