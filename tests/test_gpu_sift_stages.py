"""SIFT on the GPU pinned stage by stage against the oracle's stages (O.sift_stages), bit for bit,
at the small and ragged sizes of sift_cases.py: the upsampled image, every Gaussian and DoG layer
(borders included), the extrema list, the stage counters, the final keypoints and descriptors;
object reuse, unused batch slots, nfeatures around n, and the candidate / keypoint capacities at
exact fit and one short with guard rows.  test_sift_cases_ref.py proves on the CPU that each case
reaches the path it is named for.  No tolerances: both sides are built with -ffp-contract=off.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import sift_cases as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KP_CAP = 4096
SENT = 0x7FC12345                      # sentinel bit pattern (a quiet NaN as float32)
GENERIC_CASES = [(33, 17, "blob"), (65, 33, "blob"), (131, 67, "blob")]


def _dev_img(img):
    return torch.tensor(np.asarray(img), dtype=torch.uint8, device="cuda")    # a copy: the cases are read-only


def _counters(sift, b=0):
    return [int(v) for v in sift.t["counters"][b].cpu().numpy()]


def _layers(sift, n_oct):
    """(name, octave, layer, array) of tmp and the Gaussian / DoG layers 0..4 of n_oct octaves."""
    sb = sift.sb
    W, H = sift.W, sift.H
    gauss = sift.t["gauss"].cpu().numpy()
    dog = sift.t["dog"].cpu().numpy()
    out = [("up", -1, -1, sift.t["tmp"].cpu().numpy()[:4 * W * H].reshape(2 * H, 2 * W))]
    assert n_oct <= sb.n_oct
    for o in range(n_oct):
        w, h = sb.oct_w[o], sb.oct_h[o]
        for i in range(5):
            go, do = sb.gauss_off[o * 6 + i], sb.dog_off[o * 5 + i]
            out.append(("gauss", o, i, gauss[go:go + w * h].reshape(h, w)))
            out.append(("dog", o, i, dog[do:do + w * h].reshape(h, w)))
    return out


def _ref_layer(st, name, o, i):
    return st["up"] if name == "up" else st[name][o][i]


_RUNS = {}


def _run(case):
    """One GPU run per case, shared by the tests below: layers, candidates, counters, result."""
    if case not in _RUNS:
        from monocular_visual_odometry_va4mr_amd.features import Sift
        W, H, kind = case
        st = S.reference(case)[0]
        sift = Sift(W, H, kp_cap=KP_CAP)
        sift.run(_dev_img(S.image(kind, W, H)))
        torch.cuda.synchronize()
        cnt = _counters(sift)
        res = None
        if cnt[3] == 0:
            res = sift.result()
        _RUNS[case] = {
            "layers": _layers(sift, len(st["gauss"])),
            "counters": cnt,
            "cand": sift.t["cand"].cpu().numpy().reshape(-1, 4)[:min(cnt[0], 131072)].copy(),
            "result": res,
        }
    return _RUNS[case]


def _sorted_rows(a):
    a = np.asarray(a).reshape(-1, 4)
    return a[np.lexsort((a[:, 3], a[:, 2], a[:, 1], a[:, 0]))]


# ------------------------------------------------------------------ scale space
@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_scale_space_bit_exact(case):
    """k_upsample, k_blur_tile_n<11|13|17|21|27> (ragged tiles, reflection folding more than once
    on the small octaves) and k_nn_down (odd sizes): every pixel of every stored layer."""
    st = S.reference(case)[0]
    layers = _run(case)["layers"]
    assert len(layers) == 1 + 10 * len(st["gauss"])
    bad = [(name, o, i, int((got != _ref_layer(st, name, o, i)).sum()))
           for name, o, i, got in layers if not np.array_equal(got, _ref_layer(st, name, o, i))]
    assert not bad, f"layers that differ (name, octave, layer, pixels): {bad}"


def test_generic_blur_bit_exact():
    """k_blur_tile, the runtime-size kernel (VO_SIFT_BLUR_GENERIC=1, read once per process): the
    same comparison in one fresh child process."""
    env = dict(os.environ, VO_SIFT_BLUR_GENERIC="1")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, os.path.abspath(__file__), "--generic-child"], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("layer ")]
    want = sum(1 + 10 * len(S.reference(c)[0]["gauss"]) for c in GENERIC_CASES)
    assert len(lines) == want, r.stdout[-2000:]
    bad = [ln for ln in lines if ln[-1] != "1"]
    assert not bad, bad
    results = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("result ")]
    assert len(results) == len(GENERIC_CASES) and all(ln[-1] == "1" for ln in results), results
    assert "generic 1" in r.stdout


def _generic_child():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from monocular_visual_odometry_va4mr_amd.features import Sift
    print("generic", os.environ.get("VO_SIFT_BLUR_GENERIC"))
    for case in GENERIC_CASES:
        W, H, kind = case
        st = S.reference(case)[0]
        sift = Sift(W, H, kp_cap=KP_CAP)
        sift.run(_dev_img(S.image(kind, W, H)))
        torch.cuda.synchronize()
        for name, o, i, got in _layers(sift, len(st["gauss"])):
            print("layer", S.case_id(case), name, o, i, int(np.array_equal(got, _ref_layer(st, name, o, i))))
        kp, desc = sift.result()
        print("result", S.case_id(case), int(np.array_equal(kp, S.reference(case)[1])
                                                 and np.array_equal(desc, S.reference(case)[2])))


# ------------------------------------------------------------------ extrema and counters
@pytest.mark.parametrize("case", S.EXTREMA_CASES, ids=S.case_id)
def test_extrema_and_counters(case):
    """k_extrema_t's candidate list (as a set: its order is the atomics') and the four stage counts:
    extrema, refined candidates, raw keypoints, keypoints after removeDuplicatedSorted.  The
    stripes are thousands of plateau ties that exist only through '>=' and never become keypoints."""
    st, kp, _ = S.reference(case)
    run = _run(case)
    cnt = run["counters"]
    assert cnt[3] == 0
    assert (cnt[0], cnt[4], cnt[1], cnt[2]) == (st["n_extrema"], st["n_refined"], st["n_raw"], len(kp))
    assert np.array_equal(_sorted_rows(run["cand"]), _sorted_rows(st["extrema"]))


# ------------------------------------------------------------------ full result
@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_full_result(case):
    """Keypoints (x, y, size, angle, response, octave) and descriptors, the zero-keypoint cases
    included (nothing raised, counters[2] == 0)."""
    _, kp, desc = S.reference(case)
    run = _run(case)
    assert run["counters"][3] == 0 and run["counters"][2] == len(kp)
    gk, gd = run["result"]
    assert gk.shape == kp.shape and gd.shape == desc.shape
    assert np.array_equal(gk, kp)
    assert np.array_equal(gd, desc)


def test_reuse_on_sparser_images():
    """One Sift object on dots6, blob, const, blob: nothing of a denser earlier image survives."""
    from monocular_visual_odometry_va4mr_amd.features import Sift
    W, H = S.MAIN
    sift = Sift(W, H, kp_cap=KP_CAP)
    got = []
    for kind in ("dots6", "blob", "const", "blob"):
        st, kp, desc = S.reference((W, H, kind))
        sift.run(_dev_img(S.image(kind, W, H)))
        torch.cuda.synchronize()
        cnt = _counters(sift)
        assert (cnt[0], cnt[4], cnt[1], cnt[2], cnt[3]) == (st["n_extrema"], st["n_refined"], st["n_raw"], len(kp), 0)
        gk, gd = sift.result()
        assert np.array_equal(gk, kp) and np.array_equal(gd, desc), kind
        got.append((gk, gd))
    assert np.array_equal(got[1][0], got[3][0]) and np.array_equal(got[1][1], got[3][1])


def test_batch_with_unused_slot():
    """run_batch of 3 images in a batch-4 object: each slot equals vo_sift alone and the oracle; the
    fourth slot's kp_out / desc rows keep their sentinel."""
    from monocular_visual_odometry_va4mr_amd.features import Sift
    from monocular_visual_odometry_va4mr_amd import _lib as L
    W, H = S.MAIN
    kinds = ("dots6", "const", "checker6")
    sift = Sift(W, H, kp_cap=KP_CAP, batch=4)
    sift.t["kp_out"].view(torch.int32).fill_(SENT)
    sift.t["desc"].view(torch.int32).fill_(SENT)
    imgs = torch.stack([_dev_img(S.image(k, W, H)) for k in kinds])
    _, _, n = sift.run_batch(imgs)
    torch.cuda.synchronize()
    assert not sift.overflowed(3)
    single = Sift(W, H, kp_cap=KP_CAP)
    for b, kind in enumerate(kinds):
        st, kp, desc = S.reference((W, H, kind))
        assert int(n[b]) == len(kp)
        cnt = _counters(sift, b)
        assert (cnt[0], cnt[4], cnt[1], cnt[2], cnt[3]) == (st["n_extrema"], st["n_refined"], st["n_raw"], len(kp), 0)
        gk, gd = sift.result(b)
        assert np.array_equal(gk, kp) and np.array_equal(gd, desc), kind
        img = _dev_img(S.image(kind, W, H))
        st_ = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        L.check(L.lib().vo_sift(C.byref(single.sb), C.c_void_p(img.data_ptr()), W, H, st_), "vo_sift")
        torch.cuda.synchronize()
        sk, sd = single.result()
        assert np.array_equal(gk, sk) and np.array_equal(gd, sd), kind
    assert bool((sift.t["kp_out"][3].view(torch.int32) == SENT).all())
    assert bool((sift.t["desc"][3].view(torch.int32) == SENT).all())
    assert _counters(sift, 3) == [0] * 8


def test_nfeatures_around_n():
    """SIFT_create(nfeatures) for nfeatures in {1, n - 1, n, n + 1} on blob 200 x 150."""
    from monocular_visual_odometry_va4mr_amd.features import Sift
    from oracle import _olib as O
    W, H = 200, 150
    img = S.image("blob", W, H)
    n = len(S.reference((W, H, "blob"))[1])
    for nf in (1, n - 1, n, n + 1):
        kp, desc = O.sift(img, nfeatures=nf)
        assert min(nf, n) <= len(kp) <= n                               # ties at the cut are kept
        sift = Sift(W, H, kp_cap=KP_CAP, nfeatures=nf)
        sift.run(_dev_img(img))
        torch.cuda.synchronize()
        gk, gd = sift.result()
        assert np.array_equal(gk, kp) and np.array_equal(gd, desc), nf


# ------------------------------------------------------------------ capacities
CAND_ALLOC, KP_ALLOC, DECL = 8192, 4096, 2048


def _guarded_sift(cand_cap, kp_cap, nfeatures=0):
    """A Sift object allocated far above need whose declared capacities are lowered on the struct:
    the rows past them are guard rows holding the sentinel."""
    from monocular_visual_odometry_va4mr_amd.features import Sift
    sift = Sift(S.MAIN[0], S.MAIN[1], cand_cap=CAND_ALLOC, kp_cap=KP_ALLOC)
    for k in ("cand", "kp", "kp_out", "desc", "hist"):
        sift.t[k].view(torch.int32).fill_(SENT)
    sift.sb.cand_cap, sift.sb.kp_cap, sift.sb.nfeatures = int(cand_cap), int(kp_cap), int(nfeatures)
    return sift


def _assert_guards(sift, cand_cap, kp_cap):
    for k, per, cap in (("cand", 4, cand_cap), ("kp", 8, kp_cap), ("kp_out", 6, kp_cap), ("desc", 128, kp_cap),
                        ("hist", 360, kp_cap)):
        guard = sift.t[k].view(torch.int32).reshape(-1)[cap * per:]
        assert guard.numel() > 0 and bool((guard == SENT).all()), f"{k}: a guard row was written"


@pytest.mark.parametrize("which,short", [("cand", 0), ("cand", 1), ("kp", 0), ("kp", 1)])
def test_capacity_exact_fit_and_one_short(which, short):
    """dots6: cand_cap = the oracle's extrema count and kp_cap = its raw keypoint count give the
    oracle's result; one less raises the overflow flag; no row past a declared capacity is
    written either way."""
    case = (S.MAIN[0], S.MAIN[1], "dots6")
    st, kp, desc = S.reference(case)
    assert 0 < st["n_extrema"] < DECL and 0 < st["n_raw"] < DECL
    cand_cap = st["n_extrema"] - short if which == "cand" else DECL
    kp_cap = st["n_raw"] - short if which == "kp" else DECL
    sift = _guarded_sift(cand_cap, kp_cap)
    sift.run(_dev_img(S.image("dots6", *S.MAIN)))
    torch.cuda.synchronize()
    cnt = _counters(sift)
    _assert_guards(sift, cand_cap, kp_cap)
    assert cnt[0] == st["n_extrema"]
    if short:
        assert cnt[3] == 1
        with pytest.raises(RuntimeError):
            sift.result()
    else:
        assert cnt[3] == 0
        assert (cnt[4], cnt[1], cnt[2]) == (st["n_refined"], st["n_raw"], len(kp))
        gk, gd = sift.result()
        assert np.array_equal(gk, kp) and np.array_equal(gd, desc)


@pytest.mark.parametrize("cand_cap,kp_cap,nfeatures", [(DECL, DECL, 5), (DECL, 0, 0), (DECL, 32769, 0)])
def test_capacity_arguments_rejected(cand_cap, kp_cap, nfeatures):
    """nfeatures > 0 needs 4 * cand_cap >= 4 * kp_cap + 2 ints of scratch; kp_cap must be in
    1..32768: VO_EARG, and nothing is written."""
    sift = _guarded_sift(cand_cap, kp_cap, nfeatures)
    sift.t["counters"].fill_(SENT)
    for k in ("gauss", "dog", "tmp"):
        sift.t[k].view(torch.int32).fill_(SENT)
    with pytest.raises(RuntimeError, match="status -1"):
        sift.run(_dev_img(S.image("dots6", *S.MAIN)))
    torch.cuda.synchronize()
    for k in ("gauss", "dog", "tmp", "counters", "cand", "kp", "kp_out", "desc", "hist"):
        assert bool((sift.t[k].view(torch.int32) == SENT).all()), k


if __name__ == "__main__" and "--generic-child" in sys.argv:
    _generic_child()
