"""The key list's capacity ccap at exact fit, one over and one under (capacities are reported,
never truncated silently).  All four eigen kernels append local maxima to gf_keys[b][ccap] behind
pos < ccap and still count every key in gf_n[b]; both selection forms turn gf_n > ccap into
nCorners = -1, and k_add_finish raises VO_ST_CAPACITY from it.  A guard that is off by one is silent:
chain b's slot ccap is chain b + 1's slot 0.

One engine of 96 x 64 and three chains: crop, a periodic image (eig_cases.py: n > 4096 local maxima,
all of one value), crop flipped.  dims.ccap is read from the struct at every call, so the tests give
the engine a key list and a sort scratch of n + 1 slots per chain and run ccap = n + 1, n, n - 1 and the
engine's own 4096 over it, the list pre-filled with a sentinel and followed by guard slots:

  vo_gftt_keys            gf_n is the true count of every chain; a chain's first min(gf_n, ccap) slots
                          are distinct keys of the oracle's set (all of it when it fits), the slots
                          behind them, the neighbours' and the guard keep the sentinel
  vo_gftt, both forms     nCorners = -1 for the periodic chain when n > ccap, else oracle.gftt's list
                          (a tie run of thousands); the neighbours always oracle.gftt's
  vo_add_corners_finish   VO_ST_CAPACITY for that chain alone, the neighbours' candidates as appended
                          from their full corner lists

per kernel form (eig_cases.CAP_FORMS): k_eig3<false>, k_eig3<true> (VO_EIG_EXACT=1, read once per
process: a process of its own runs the same checks), k_eig3<true, true> and k_eignms<true> (an
all-ones mask; checked after the selection only), k_eignms<false> (blockSize 5; Harris blockSize 3).
test_eig_cases_ref.py asserts the counts on the CPU.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import eig_cases as E

SENT_KEY = 0x5A5A5A5A5A5A5A5A
SENT_PT = -7.0
GUARD = 256
SETTINGS = ("one_spare", "exact_fit", "one_short", "engine_own")


def ccap_of(setting, n):
    return {"one_spare": n + 1, "exact_fit": n, "one_short": n - 1, "engine_own": E.CAP_CCAP}[setting]


def rig(bs, harris, cache={}):
    """(engine, n): the engine with a key list and a sort scratch of n + 1 slots per chain (+ guard) in
    place of its own, n = the oracle's key count of the periodic image"""
    import torch
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    from monocular_visual_odometry_va4mr_amd import _lib as L
    from monocular_visual_odometry_va4mr_amd import options as Op
    if (bs, harris) not in cache:
        opts, _, _ = Op.get("kitti")
        opts.update(feature_max_corners=E.CAP_MAX_CORNERS, feature_block_size=bs, feature_use_harris=harris, maxLevel=0)
        eng = Engine(np.eye(3), opts, E.CAP_W, E.CAP_H, batch=E.CAP_B, ncap=64, pcap=E.CAP_MAX_CORNERS, fcap=4)
        assert eng.dims.ccap == E.CAP_CCAP and eng.dims.mcap == E.CAP_MAX_CORNERS
        n = len(E.capacity_reference(bs, harris)[1][0])
        assert n > E.CAP_CCAP
        eng.t["gf_keys"] = torch.full((E.CAP_B * (n + 1) + GUARD,), SENT_KEY, dtype=torch.int64, device="cuda")
        eng.t["gf_sort"] = torch.zeros(E.CAP_B * (n + 1 + L.VO_GF_SORT_EXTRA), dtype=torch.int64, device="cuda")
        eng.state.gf_keys = eng.t["gf_keys"].data_ptr()
        eng.state.gf_sort = eng.t["gf_sort"].data_ptr()
        cache[bs, harris] = (eng, n)
    return cache[bs, harris]


def _reset(eng):
    """what a call must find: the sort scratch zeroed (its histogram sits behind ccap keys, so it moves
    with ccap), the key list, the corners and the candidates pre-filled, a fresh chain state"""
    eng.t["gf_sort"].zero_()
    eng.t["gf_keys"].fill_(SENT_KEY)
    eng.t["corners"].fill_(SENT_PT)
    eng.t["nCorners"].fill_(-5)
    for k in ("c_kp", "c_first"):
        eng.t[k].fill_(SENT_PT)
    eng.t["c_tau"].fill_(-9)
    for k in ("status", "nC", "nF", "nInl", "num_pts"):
        eng.t[k].zero_()


def check_keys(eng, n, ccap, ref, what):
    import torch
    _reset(eng)
    assert eng.lib.vo_gftt_keys(eng._pd, eng._po, eng._ps, 0, eng.stream) == 0
    torch.cuda.synchronize()
    gf_n = eng.t["gf_n"].cpu().numpy()
    buf = eng.t["gf_keys"].cpu().numpy().view(np.uint64)
    print(what, "gf_n", gf_n.tolist(), "ccap", ccap)
    assert gf_n.tolist() == [len(k) for k, _ in ref], f"{what}: gf_n {gf_n.tolist()}"
    for b, (keys, _) in enumerate(ref):
        row = buf[b * ccap:(b + 1) * ccap]
        m = min(len(keys), ccap)
        got = np.sort(row[:m])
        assert len(np.unique(got)) == m and np.isin(got, keys).all(), f"{what}: chain {b} holds keys that are not the oracle's"
        if len(keys) <= ccap:
            assert np.array_equal(got, keys), f"{what}: chain {b} key set"
        assert (row[m:] == SENT_KEY).all(), f"{what}: chain {b} slots {m}..{ccap} written"
    assert (buf[E.CAP_B * ccap:] == SENT_KEY).all(), f"{what}: slots behind the last chain written"


def check_corners_and_finish(eng, n, ccap, ref, masked, what):
    import torch
    from monocular_visual_odometry_va4mr_amd import _lib as L
    _reset(eng)
    if masked:
        ones = torch.full((E.CAP_B, E.CAP_H, E.CAP_W), 255, dtype=torch.uint8, device="cuda")
        rc = eng.lib.vo_gftt_masked(eng._pd, eng._po, eng._ps, 0, C.c_void_p(ones.data_ptr()), E.CAP_W * E.CAP_H, E.CAP_W,
                                    eng.stream)
    else:
        rc = eng.lib.vo_gftt(eng._pd, eng._po, eng._ps, 0, eng.stream)
    torch.cuda.synchronize()
    assert rc == 0
    ns = eng.t["nCorners"].cpu().numpy()
    corners = eng.t["corners"].cpu().numpy()
    over = n > ccap
    print(what, "nCorners", ns.tolist(), "oracle", [len(c) for _, c in ref], "over" if over else "fits")
    for b, (_, want) in enumerate(ref):
        if b == 1 and over:
            assert ns[b] == -1, f"{what}: nCorners {ns[b]} on the chain whose keys do not fit"
            continue
        assert ns[b] == len(want) and np.array_equal(corners[b, :ns[b]], want), f"{what}: chain {b}: {ns[b]} corners vs {len(want)}"
        assert (corners[b, ns[b]:] == SENT_PT).all(), f"{what}: chain {b}: rows past nCorners written"
    buf = eng.t["gf_keys"].cpu().numpy().view(np.uint64)
    assert (buf[E.CAP_B * ccap:] == SENT_KEY).all(), f"{what}: key slots behind the last chain written"
    assert eng.lib.vo_add_corners_finish(eng._pd, eng._po, eng._ps, eng.stream) == 0
    torch.cuda.synchronize()
    st = eng.t["status"].cpu().numpy()
    assert st.tolist() == [0, L.ST_CAPACITY if over else 0, 0], f"{what}: status {st.tolist()}"
    T = {k: eng.t[k].cpu().numpy() for k in ("nC", "nF", "c_kp", "c_first", "c_tau")}
    for b, (_, want) in enumerate(ref):
        if b == 1 and over:
            assert T["nC"][b] == 0 and T["nF"][b] == 0 and (T["c_kp"][b] == SENT_PT).all(), f"{what}: the stopped chain changed"
            continue
        m = len(want)
        assert T["nC"][b] == m and T["nF"][b] == 1, f"{what}: chain {b}: nC {T['nC'][b]}, nF {T['nF'][b]}"
        assert np.array_equal(T["c_kp"][b, :m], want) and np.array_equal(T["c_first"][b, :m], want) and \
            (T["c_tau"][b, :m] == 0).all(), f"{what}: chain {b}: candidates"
        assert (T["c_kp"][b, m:] == SENT_PT).all() and (T["c_tau"][b, m:] == -9).all(), f"{what}: chain {b}: rows past nC"


def check_form(form, setting):
    """every check of one kernel form at one ccap setting; returns how many launches were checked"""
    from monocular_visual_odometry_va4mr_amd import _lib as L
    bs, harris, masked = E.CAP_FORMS[form]
    want_exact = "1" if form == "eig3_exact" else "0"
    assert os.environ.get("VO_EIG_EXACT", "0") == want_exact and os.environ.get("VO_EIG_GENERIC", "0") == "0"
    eng, n = rig(bs, harris)
    ref = E.capacity_reference(bs, harris)
    ccap = ccap_of(setting, n)
    assert E.CAP_CCAP <= ccap <= n + 1
    eng.opts.feature_block_size, eng.opts.feature_use_harris, eng.opts.harris_k = bs, int(harris), 0.04
    eng.opts.feature_quality_level, eng.opts.feature_min_dist = E.CAP_QUALITY, E.CAP_MIN_DIST
    eng.opts.feature_max_corners = E.CAP_MAX_CORNERS
    eng.build_pyramid(E.capacity_frames(bs), 0)
    done = 0
    eng.dims.ccap = ccap
    try:
        if not masked:
            check_keys(eng, n, ccap, ref, f"{form} {setting} keys")
            done += 1
        for mode in (1, 2):
            L.check(L.lib().vo_set_gftt_select(mode), "vo_set_gftt_select")
            check_corners_and_finish(eng, n, ccap, ref, masked, f"{form} {setting} select {mode}")
            done += 1
    finally:
        eng.dims.ccap = E.CAP_CCAP
        L.lib().vo_set_gftt_select(0)
        eng.t["gf_sort"].zero_()
    return done


if __name__ == "__main__":
    # the second process of test_exact_everywhere_form: the same checks with VO_EIG_EXACT=1
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    total = sum(check_form("eig3_exact", s) for s in SETTINGS)
    print(f"VO_EIG_EXACT={os.environ['VO_EIG_EXACT']}: {total} launches checked")
    sys.exit(0)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("form", [f for f in E.CAP_FORMS if f != "eig3_exact"])
def test_key_capacity(form, setting):
    masked = E.CAP_FORMS[form][2]
    assert check_form(form, setting) == (2 if masked else 3)


def test_exact_everywhere_form():
    """k_eig3<true> appends through its batched flush: the four settings in a process with VO_EIG_EXACT=1"""
    env = dict(os.environ, VO_EIG_EXACT="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-2500:]
    assert f"VO_EIG_EXACT=1: {3 * len(SETTINGS)} launches checked" in p.stdout, p.stdout[-1500:]


def test_cv2compat_key_capacity_raises():
    """more local maxima than the engine's key list holds: an error naming the capacity status, as
    test_cv2compat_capacity_overflow_raises shows for the corner capacity"""
    from monocular_visual_odometry_va4mr_amd import cv2compat
    from monocular_visual_odometry_va4mr_amd import _lib as L
    for bs in (3, 5):                                      # k_eig3, k_eignms
        img = E.periodic(E.CAP_W, E.CAP_H, bs)
        with pytest.raises(cv2compat.error, match=L.STATUS_NAMES[L.ST_CAPACITY]):
            cv2compat.goodFeaturesToTrack(img, 100, E.CAP_QUALITY, E.CAP_MIN_DIST, blockSize=bs)
    # and the same engine goes on working
    import gftt_cases as GC
    from oracle import _olib as O
    crop = GC.crop(E.CAP_W, E.CAP_H)
    got = cv2compat.goodFeaturesToTrack(crop, 100, E.CAP_QUALITY, E.CAP_MIN_DIST)
    assert np.array_equal(got[:, 0, :], O.gftt(crop, 100, E.CAP_QUALITY, E.CAP_MIN_DIST))
