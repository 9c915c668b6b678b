"""Lens distortion on the GPU: vo_undistort_map, vo_remap_u8 and vo_undistort_points against the NumPy
definition (test_undistort_ref), the four cv2compat calls over them, and the engine option
dist_coeffs: an Engine given the raw frames of a distorted camera against an Engine without the
option given the frames remap_ref rectified, in each step form.  All bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import test_undistort_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_subpix import KEYS   # noqa: E402

_CACHE = {}
SENT = 0x5A
EARG = -1


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


def _lib():
    from monocular_visual_odometry_va4mr_amd import _lib as L
    return L.lib()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dbl(v):
    a = np.asarray(v, np.float64).ravel()
    return (C.c_double * a.size)(*a)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ------------------------------------------------------------------ vo_undistort_map
def run_map(K, dist, new_K, W, H, want_d=True):
    m1 = torch.full((H, W, 2), SENT, dtype=torch.int16, device="cuda")
    m2 = torch.full((H, W), SENT, dtype=torch.int16, device="cuda")
    md = torch.full((H, W, 2), -7.25, dtype=torch.float64, device="cuda")
    rc = _lib().vo_undistort_map(_dbl(K), _dbl(dist) if len(dist) else None, len(dist), None if new_K is None else _dbl(new_K),
                                 W, H, _p(m1), _p(m2), _p(md) if want_d else None, _stream())
    torch.cuda.synchronize()
    return rc, m1.cpu().numpy(), m2.cpu().numpy().view(np.uint16), md.cpu().numpy()


def assert_map(got, want, what):
    m1, m2, md = got
    w1, w2, wd = want
    assert np.array_equal(m1, w1), f"{what}: map1 differs at {np.argwhere(m1 != w1)[:4].tolist()}"
    assert np.array_equal(m2, w2), f"{what}: map2 differs at {np.argwhere(m2 != w2)[:4].tolist()}"
    if wd is not None:
        bad = np.argwhere(_bits(md) != _bits(wd))
        assert bad.size == 0, f"{what}: mapd differs at {bad[:4].tolist()}"


@pytest.mark.parametrize("W,H", R.SIZES, ids=[f"{w}x{h}" for w, h in R.SIZES])
@pytest.mark.parametrize("name", list(R.SETS))
def test_undistort_map_is_the_numpy_definition(name, W, H):
    rc, m1, m2, md = run_map(R.size_K(W, H), R.SETS[name], None, W, H)
    assert rc == 0
    assert_map((m1, m2, md), R.case_map(name, W, H), f"{name} {W}x{H}")


def test_undistort_map_new_matrix_null_mapd_and_coefficient_counts():
    W, H = 131, 67
    K = R.size_K(W, H)
    Kn = K.copy()
    Kn[0, 0] *= 0.85
    Kn[1, 1] *= 0.9
    Kn[0, 2] += 2.25
    Kn[1, 2] -= 1.5
    rc, m1, m2, md = run_map(K, R.SETS["C"], Kn, W, H)
    assert rc == 0
    want = R.map_ref(K, R.SETS["C"], Kn, W, H)
    assert_map((m1, m2, md), want, "new_K")
    assert not np.array_equal(want[0], R.case_map("C", W, H)[0])
    rc, m1, m2, md = run_map(K, R.SETS["A"], None, W, H, want_d=False)
    assert rc == 0 and np.all(md == -7.25)
    assert_map((m1, m2, None), R.case_map("A", W, H)[:2] + (None,), "mapd NULL")
    # 4 coefficients, and none at all
    rc, m1, m2, md = run_map(K, R.SETS["B"][:4], None, W, H)
    assert rc == 0
    assert_map((m1, m2, md), R.map_ref(K, R.SETS["B"][:4], None, W, H), "4 coefficients")
    rc, m1, m2, md = run_map(K, [], None, W, H)
    assert rc == 0
    assert_map((m1, m2, md), R.case_map("Z", W, H), "no coefficients")


# ------------------------------------------------------------------ vo_remap_u8
def sources(sW, sH, B):
    """B different sW x sH images cut from the synthetic parking frame (whole, flipped, mirrored at
    640 x 480)."""
    f = R.parking_frame()
    if (sW, sH) == (640, 480):
        return [np.ascontiguousarray(v) for v in (f, f[::-1], f[:, ::-1])][:B]
    return [R.crop(sW, sH, 37 + 61 * b, 21 + 43 * b) for b in range(B)]


def run_remap(srcs, m1, m2, src_pad=0, dst_pad=0, dst_off=0):
    """vo_remap_u8 on B images.  Every source image is followed by a guard row and every row by
    `src_pad` bytes, all 255 (a read outside an image would show as a wrong pixel); the destination
    likewise, with `dst_off` bytes in front.  Returns (rc, destination buffer as read back, expected
    buffer)."""
    B = len(srcs)
    sH, sW = srcs[0].shape
    H, W = m2.shape
    sp, dp = sW + src_pad, W + dst_pad
    sbuf = np.full((B, sH + 1, sp), 255, np.uint8)
    for b, im in enumerate(srcs):
        sbuf[b, :sH, :sW] = im
    n_dst = dst_off + B * (H + 1) * dp + 8
    want = np.full(n_dst, 255, np.uint8)
    body = want[dst_off:dst_off + B * (H + 1) * dp].reshape(B, H + 1, dp)
    for b, im in enumerate(srcs):
        body[b, :H, :W] = R.remap_ref(im, m1, m2)
    d_src = torch.from_numpy(sbuf).cuda()
    d_dst = torch.full((n_dst,), 255, dtype=torch.uint8, device="cuda")
    d_m1 = torch.from_numpy(np.ascontiguousarray(m1)).cuda()
    d_m2 = torch.from_numpy(np.ascontiguousarray(m2).view(np.int16)).cuda()
    rc = _lib().vo_remap_u8(B, _p(d_src), (sH + 1) * sp, sp, sW, sH, _p(d_dst, dst_off), (H + 1) * dp, dp, W, H,
                            _p(d_m1), _p(d_m2), _stream())
    torch.cuda.synchronize()
    assert np.array_equal(d_src.cpu().numpy(), sbuf), "the source was written"
    return rc, d_dst.cpu().numpy(), want


def assert_remap(rc, got, want, what):
    assert rc == 0, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at {bad[:6].tolist()}: got {got[bad[:6]].tolist()} want {want[bad[:6]].tolist()}"


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("W,H", R.SIZES, ids=[f"{w}x{h}" for w, h in R.SIZES])
@pytest.mark.parametrize("name", list(R.SETS))
def test_remap_is_the_numpy_definition(name, W, H, B):
    m1, m2, _ = R.case_map(name, W, H)
    rc, got, want = run_remap(sources(W, H, B), m1, m2)
    assert_remap(rc, got, want, f"{name} {W}x{H} B {B}")
    if name == "Z":
        assert np.array_equal(got[:W * H].reshape(H, W), sources(W, H, 1)[0])


def test_remap_source_of_another_size():
    m1, m2, _ = R.case_map("A", 131, 67)
    srcs = sources(70, 50, 2)
    n = R.taps_inside(m1, m2, 70, 50)
    assert (n == 0).any() and (n == 4).any() and ((n > 0) & (n < 4)).any()
    rc, got, want = run_remap(srcs, m1, m2, src_pad=3, dst_pad=5)
    assert_remap(rc, got, want, "70x50 into 131x67")


@pytest.mark.parametrize("dst_off", [0, 1, 2, 3])
@pytest.mark.parametrize("W", [1, 3, 4, 5, 63, 64, 65, 131])
def test_remap_row_heads_tails_pitches_and_odd_pointers(W, dst_off):
    """Rows start at every alignment (the pitch W + dst_pad is odd or even with W, the base pointer
    is moved by dst_off), so the four-pixel packing has heads and tails of every length; padding,
    guard rows and the bytes around the buffer stay 255."""
    H = 6
    K = R.size_K(W, H)
    for dst_pad, src_pad in ((0, 0), (3, 2), (8, 1)):
        m1, m2, _ = R.map_ref(K, R.SETS["B" if W > 4 else "Z"], None, W, H)
        rc, got, want = run_remap(sources(W, H, 3), m1, m2, src_pad=src_pad, dst_pad=dst_pad, dst_off=dst_off)
        assert_remap(rc, got, want, f"W {W} dst_pad {dst_pad} dst_off {dst_off}")


def test_remap_extreme_map_entries():
    """Clamp values, NaN and far coordinates through the float-map quantiser: those pixels are 0 and
    nothing outside the source is read."""
    mx = np.array([[3 + 1 / 64, 3 + 3 / 64, -1 / 64, np.nan, 1e9, -1e9, np.inf, -np.inf, 6.5, 7.0, 7.5, -1.0, -0.5]], np.float32)
    mx = np.repeat(mx, 3, 0)
    my = np.array([[0.0], [7.25], [-0.75]], np.float32) + np.zeros_like(mx)
    for a, b in ((mx, my), (my.T.copy(), mx.T.copy())):
        m1, m2 = R.quantise_ref(a, b)
        rc, got, want = run_remap(sources(8, 8, 2), m1, m2, src_pad=1, dst_pad=2)
        assert_remap(rc, got, want, "extreme entries")


# ------------------------------------------------------------------ vo_undistort_points
def raw_points(name, n):
    """n raw pixel positions that rectified pixels of set `name` map to (inside the model's range)."""
    md = R.case_map(name, 640, 480)[2].reshape(-1, 2)
    idx = np.random.default_rng(5).permutation(len(md))[:n]
    return np.ascontiguousarray(md[idx])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
@pytest.mark.parametrize("name", ["A", "C"])
def test_undistort_points_is_the_numpy_definition(name, n):
    K = R.size_K(640, 480)
    P = K.copy()
    P[0, 0] *= 1.1
    P[1, 2] += 4.0
    pts = raw_points(name, n)
    cap = n + 3
    buf = np.full((cap, 2), -3.5)
    buf[:n] = pts
    d_pts = torch.from_numpy(buf).cuda()
    for iters in (1, 5, 100):
        for Pm in (None, P):
            out = torch.full((cap, 2), -9.75, dtype=torch.float64, device="cuda")
            rc = _lib().vo_undistort_points(n, _p(d_pts), _dbl(K), _dbl(R.SETS[name]), len(R.SETS[name]),
                                            None if Pm is None else _dbl(Pm), iters, _p(out), _stream())
            torch.cuda.synchronize()
            assert rc == 0
            got = out.cpu().numpy()
            want = R.undistort_points_ref(pts, K, R.SETS[name], P=Pm, iters=iters)
            assert np.all(np.isfinite(want))
            bad = np.argwhere(_bits(got[:n]) != _bits(want))
            assert bad.size == 0, f"{name} n {n} iters {iters} P {Pm is not None}: {bad[:4].tolist()}"
            assert np.all(got[n:] == -9.75)
    assert np.array_equal(d_pts.cpu().numpy(), buf)


# ------------------------------------------------------------------ bad arguments
def test_bad_arguments_return_earg_and_write_nothing():
    lib, st = _lib(), _stream()
    W = H = 8
    K = R.size_K(W, H)
    skew, k22, fx0, nan = K.copy(), K.copy(), K.copy(), K.copy()
    skew[0, 1] = 0.5
    k22[2, 2] = 2.0
    fx0[0, 0] = 0.0
    nan[1, 2] = np.nan
    low = K.copy()
    low[2, 0] = 1e-3
    bad_K = [skew, k22, fx0, nan, low]
    d5 = _dbl(R.SETS["A"])
    m1 = torch.full((H, W, 2), SENT, dtype=torch.int16, device="cuda")
    m2 = torch.full((H, W), SENT, dtype=torch.int16, device="cuda")
    md = torch.full((H, W, 2), -7.25, dtype=torch.float64, device="cuda")
    f = lib.vo_undistort_map
    Kc = _dbl(K)
    assert f(None, d5, 5, None, W, H, _p(m1), _p(m2), _p(md), st) == EARG
    assert f(Kc, d5, 5, None, W, H, None, _p(m2), _p(md), st) == EARG
    assert f(Kc, d5, 5, None, W, H, _p(m1), None, _p(md), st) == EARG
    assert f(Kc, None, 5, None, W, H, _p(m1), _p(m2), _p(md), st) == EARG
    for w, h in ((0, H), (W, 0), (-1, H), (16385, H), (W, 16385)):
        assert f(Kc, d5, 5, None, w, h, _p(m1), _p(m2), _p(md), st) == EARG
    d14 = _dbl([0.0] * 14)
    for nd in (-1, 1, 2, 3, 6, 7, 9, 12, 14):
        assert f(Kc, d14, nd, None, W, H, _p(m1), _p(m2), _p(md), st) == EARG
    for Kb in bad_K:
        assert f(_dbl(Kb), d5, 5, None, W, H, _p(m1), _p(m2), _p(md), st) == EARG
        assert f(Kc, d5, 5, _dbl(Kb), W, H, _p(m1), _p(m2), _p(md), st) == EARG
    torch.cuda.synchronize()
    assert bool((m1 == SENT).all()) and bool((m2 == SENT).all()) and bool((md == -7.25).all())

    # vo_remap_u8: one buffer holds the source (first half) and the destination (second half)
    buf = torch.full((4096,), SENT, dtype=torch.uint8, device="cuda")
    g1 = torch.zeros((H, W, 2), dtype=torch.int16, device="cuda")
    g2 = torch.zeros((H, W), dtype=torch.int16, device="cuda")
    src, dst = _p(buf), _p(buf, 2048)
    ok = dict(B=2, src=src, ss=W * H, sp=W, sW=W, sH=H, dst=dst, ds=W * H, dp=W, W=W, H=H, m1=_p(g1), m2=_p(g2))

    def remap(**kw):
        a = dict(ok, **kw)
        return lib.vo_remap_u8(a["B"], a["src"], a["ss"], a["sp"], a["sW"], a["sH"], a["dst"], a["ds"], a["dp"], a["W"], a["H"],
                               a["m1"], a["m2"], st)

    for kw in (dict(src=None), dict(dst=None), dict(m1=None), dict(m2=None), dict(B=0), dict(B=-1),
               dict(W=0), dict(H=0), dict(W=16385, dp=16385), dict(H=16385), dict(sW=0), dict(sH=0), dict(sW=16385, sp=16385),
               dict(sH=16385), dict(sp=W - 1), dict(dp=W - 1), dict(ss=-1), dict(ds=-1), dict(ds=W * H - 1),
               dict(dst=src), dict(dst=_p(buf, 2 * W * H - 1)), dict(dst=_p(buf, 1)), dict(src=_p(buf, 2048 + W * H)),
               dict(src=_p(buf, 2048 - 2 * W * H + 1))):
        assert remap(**kw) == EARG, kw
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())
    assert remap() == 0                                    # the arguments the cases vary are good ones
    torch.cuda.synchronize()
    assert bool((buf[:2048] == SENT).all()) and bool((buf[2048 + 2 * W * H:] == SENT).all())

    # vo_undistort_points
    pts = torch.zeros((16, 2), dtype=torch.float64, device="cuda")
    out = torch.full((16, 2), -9.75, dtype=torch.float64, device="cuda")
    g = lib.vo_undistort_points
    assert g(16, None, Kc, d5, 5, None, 5, _p(out), st) == EARG
    assert g(16, _p(pts), Kc, d5, 5, None, 5, None, st) == EARG
    assert g(16, _p(pts), None, d5, 5, None, 5, _p(out), st) == EARG
    assert g(16, _p(pts), Kc, None, 5, None, 5, _p(out), st) == EARG
    assert g(-1, _p(pts), Kc, d5, 5, None, 5, _p(out), st) == EARG
    for it in (0, -1, 101):
        assert g(16, _p(pts), Kc, d5, 5, None, it, _p(out), st) == EARG
    for nd in (1, 3, 6, 12, 14):
        assert g(16, _p(pts), Kc, d14, nd, None, 5, _p(out), st) == EARG
    for Kb in bad_K:
        assert g(16, _p(pts), _dbl(Kb), d5, 5, None, 5, _p(out), st) == EARG
        assert g(16, _p(pts), Kc, d5, 5, _dbl(Kb), 5, _p(out), st) == EARG
    torch.cuda.synchronize()
    assert bool((out == -9.75).all())


# ------------------------------------------------------------------ cv2compat
def test_cv2compat_maps_remap_and_undistort():
    from monocular_visual_odometry_va4mr_amd import cv2compat as G
    W, H = 131, 67
    K = R.size_K(W, H)
    img = R.crop(W, H)
    for name in ("A", "B", "C", "Z"):
        w1, w2, wd = R.case_map(name, W, H)
        m1, m2 = G.initUndistortRectifyMap(K, np.array(R.SETS[name]), None, None, (W, H), G.CV_16SC2)
        assert m1.dtype == np.int16 and m2.dtype == np.uint16 and np.array_equal(m1, w1) and np.array_equal(m2, w2)
        f1, f2 = G.initUndistortRectifyMap(K, R.SETS[name], np.eye(3), np.zeros((0, 0)), (W, H), G.CV_32FC1)
        assert f1.dtype == np.float32 and f1.shape == (H, W) and f2.shape == (H, W)
        assert np.array_equal(f1, wd[..., 0].astype(np.float32)) and np.array_equal(f2, wd[..., 1].astype(np.float32))
        want = R.remap_ref(img, w1, w2)
        out = G.remap(img, m1, m2, G.INTER_LINEAR)
        assert out.dtype == np.uint8 and np.array_equal(out, want)
        assert np.array_equal(G.remap(img, m1, m2, G.INTER_LINEAR, borderMode=G.BORDER_CONSTANT, borderValue=0), want)
        q1, q2 = R.quantise_ref(f1, f2)
        assert np.array_equal(G.remap(img, f1, f2, G.INTER_LINEAR), R.remap_ref(img, q1, q2))
        assert np.array_equal(G.undistort(img, K, R.SETS[name]), want)
    Kn = K.copy()
    Kn[0, 0] *= 0.8
    n1, n2, _ = R.map_ref(K, R.SETS["A"], Kn, W, H)
    got = G.undistort(img, K, R.SETS["A"], newCameraMatrix=Kn)
    assert np.array_equal(got, R.remap_ref(img, n1, n2))
    assert np.array_equal(got, G.remap(img, *G.initUndistortRectifyMap(K, R.SETS["A"], None, Kn, (W, H), G.CV_16SC2), G.INTER_LINEAR))
    dst = np.zeros((H, W), np.uint8)
    assert G.undistort(img, K, R.SETS["A"], dst, Kn) is dst and np.array_equal(dst, got)
    # a source of another size than the map
    small = R.crop(70, 50)
    w1, w2, _ = R.case_map("A", W, H)
    assert np.array_equal(G.remap(small, w1, w2, G.INTER_LINEAR), R.remap_ref(small, w1, w2))


def test_cv2compat_undistort_points():
    from monocular_visual_odometry_va4mr_amd import cv2compat as G
    K = R.size_K(640, 480)
    P = K.copy()
    P[0, 2] += 5.0
    for name in ("A", "C"):
        pts = raw_points(name, 200)
        for dt in (np.float32, np.float64):
            for shape in ((-1, 1, 2), (-1, 2)):
                src = pts.astype(dt).reshape(shape)
                for Pm in (None, P):
                    got = G.undistortPoints(src, K, np.array(R.SETS[name]), None, Pm)
                    want = R.undistort_points_ref(src.reshape(-1, 2).astype(np.float64), K, R.SETS[name], P=Pm, iters=5)
                    assert got.dtype == dt and got.shape == (200, 1, 2)
                    assert np.array_equal(got.reshape(-1, 2), want.astype(dt))
    e = G.undistortPoints(np.zeros((0, 1, 2), np.float32), K, None)
    assert e.shape == (0, 1, 2) and e.dtype == np.float32
    # no coefficients: the normalisation alone
    got = G.undistortPoints(np.array([[[320.0, 240.0]], [[0.0, 0.0]]]), K, None)
    assert np.array_equal(got[:, 0], R.undistort_points_ref(np.array([[320.0, 240.0], [0.0, 0.0]]), K, None))


def test_cv2compat_not_implemented_and_errors():
    from monocular_visual_odometry_va4mr_amd import cv2compat as G
    W, H = 64, 48
    K = R.size_K(W, H)
    img = R.crop(W, H)
    A = R.SETS["A"]
    m1, m2, md = R.case_map("A", W, H)
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    for d in ([0.0] * 12, [0.0] * 14):
        with pytest.raises(NotImplementedError):
            G.initUndistortRectifyMap(K, d, None, None, (W, H), G.CV_16SC2)
        with pytest.raises(NotImplementedError):
            G.undistort(img, K, d)
        with pytest.raises(NotImplementedError):
            G.undistortPoints(np.zeros((3, 2)), K, d)
    with pytest.raises(NotImplementedError):
        G.initUndistortRectifyMap(K, A, Rz, None, (W, H), G.CV_16SC2)
    with pytest.raises(NotImplementedError):
        G.undistortPoints(np.zeros((3, 2)), K, A, R=Rz)
    with pytest.raises(NotImplementedError):
        G.initUndistortRectifyMap(K, A, None, None, (W, H), 13)
    with pytest.raises(NotImplementedError):
        G.remap(img, m1, m2, G.INTER_NEAREST)
    with pytest.raises(NotImplementedError):
        G.remap(img, m1, m2, G.INTER_LINEAR, borderMode=1)
    with pytest.raises(NotImplementedError):
        G.remap(img, m1, m2, G.INTER_LINEAR, borderValue=7)
    with pytest.raises(NotImplementedError):
        G.remap(np.stack([img] * 3, -1), m1, m2, G.INTER_LINEAR)
    with pytest.raises(NotImplementedError):
        G.remap(img.astype(np.float32), m1, m2, G.INTER_LINEAR)
    with pytest.raises(NotImplementedError):
        G.remap(img, md.astype(np.float32), None, G.INTER_LINEAR)
    with pytest.raises(G.error):
        G.remap(img, m1, m2.astype(np.int32), G.INTER_LINEAR)
    with pytest.raises(G.error):
        G.initUndistortRectifyMap(K, [0.0] * 6, None, None, (W, H), G.CV_16SC2)
    skew = K.copy()
    skew[0, 1] = 1.0
    with pytest.raises(G.error):
        G.initUndistortRectifyMap(skew, A, None, None, (W, H), G.CV_16SC2)
    with pytest.raises(G.error):
        G.undistortPoints(np.zeros((3, 2), np.int32), K, A)
    with pytest.raises(G.error):
        G.undistortPoints(np.zeros((3, 3)), K, A)
    # the PnP calls keep refusing distortion, and say where to go
    obj = np.zeros((4, 3), np.float32)
    pix = np.zeros((4, 2), np.float32)
    with pytest.raises(NotImplementedError, match="undistortPoints"):
        G.solvePnPRansac(obj, pix, K, np.array(A), flags=G.SOLVEPNP_P3P)
    with pytest.raises(NotImplementedError, match="undistortPoints"):
        G.solvePnPRefineLM(obj, pix, K, np.array(A), np.zeros(3), np.zeros(3))


# ------------------------------------------------------------------ the pipeline
N_FRAMES, BOOT, N_STEPS = 9, (0, 2), 6
CAPS = dict(ncap=4096, pcap=8192, fcap=32)


def distorted_sequence(seed):
    """(raw frames [9][480][640], rectified frames by remap_ref) of a parking camera with set A: the
    renderer's rays are those of the raw pixels, undistort_points_ref(grid, A, 100 iterations)."""
    key = ("seq", seed)
    if key not in _CACHE:
        from monocular_visual_odometry_va4mr_amd.synth import Renderer
        r = Renderer("parking", seed=seed)
        g = R.pixel_grid(r.W, r.H)
        n = R.undistort_points_ref(g, r.K, R.SETS["A"], iters=100)
        if "rays" not in _CACHE:
            # the rays are the camera's: the forward model takes them back to the grid
            k1, k2, p1, p2, k3 = R.SETS["A"]
            x, y = n[..., 0], n[..., 1]
            r2 = x * x + y * y
            kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
            xd = x * kr + p1 * (2 * x * y) + p2 * (r2 + 2 * x * x)
            yd = y * kr + p1 * (r2 + 2 * y * y) + p2 * (2 * x * y)
            back = np.stack([r.K[0, 0] * xd + r.K[0, 2], r.K[1, 1] * yd + r.K[1, 2]], -1)
            assert float(np.abs(back - g).max()) < 1e-9
            _CACHE["rays"] = True
        r.rx = torch.from_numpy(np.ascontiguousarray(n[..., 0]))
        r.ry = torch.from_numpy(np.ascontiguousarray(n[..., 1]))
        raw = torch.stack(r.frames(N_FRAMES)[0]).numpy()
        m1, m2, _ = R.case_map("A", r.W, r.H)
        rect = np.stack([R.remap_ref(f, m1, m2) for f in raw])
        assert not np.array_equal(raw, rect)
        _CACHE[key] = (raw, rect)
    return _CACHE[key]


def _setup(seeds):
    from monocular_visual_odometry_va4mr_amd import options as Op
    from monocular_visual_odometry_va4mr_amd.synth import intrinsics
    seqs = [distorted_sequence(s) for s in seeds]
    raw = np.stack([s[0] for s in seqs], 1)                 # [9][B][H][W]
    rect = np.stack([s[1] for s in seqs], 1)
    return intrinsics("parking"), Op.get("parking")[0], raw, rect


def _state(eng):
    torch.cuda.synchronize()
    return {k: eng.t[k].cpu().numpy().copy() for k in KEYS}


def plain_reference(seeds):
    """Per-step states of an Engine without the option on the rectified frames (and the first-step
    pose of one on the raw frames).  Computed once per seed set."""
    key = ("plain", tuple(seeds))
    if key not in _CACHE:
        from monocular_visual_odometry_va4mr_amd.engine import Engine
        K, opts, raw, rect = _setup(seeds)
        out = {}
        for what, fr in (("rect", rect), ("raw", raw)):
            eng = Engine(K, opts, 640, 480, batch=len(seeds), **CAPS)
            assert eng.dist is None and eng._map1 is None
            eng.bootstrap(fr[BOOT[0]], fr[BOOT[1]])
            states = [_state(eng)]
            for k in range(N_STEPS if what == "rect" else 1):
                eng.step(fr[BOOT[1] + 1 + k])
                states.append(_state(eng))
            assert (eng.statuses() == 0).all(), eng.statuses()
            out[what] = states
        nF = out["rect"][1]["nF"]
        assert (nF == 3).all()
        for b in range(len(seeds)):                          # not vacuous: the raw frames give another pose
            assert not np.array_equal(out["rect"][1]["pose_t"][b, 2], out["raw"][1]["pose_t"][b, 2])
        assert (out["rect"][-1]["nL"] > 20).all()
        _CACHE[key] = out["rect"]
    return _CACHE[key]


def assert_state(eng, want, what):
    got = _state(eng)
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), f"{what}: {k}"


class CountingLib:
    """The library with its calls counted by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        f = getattr(self._lib, name)

        def call(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return f(*a)
        return call


FORMS = ["eager", "split", "graph", "prefetch", "host_frames"]


@pytest.mark.parametrize("form", FORMS)
def test_engine_rectifies_raw_frames(form, monkeypatch):
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    seeds = [1]
    K, opts, raw, _ = _setup(seeds)
    want = plain_reference(seeds)
    monkeypatch.delenv("VO_COMPACT_IN_TRACK", raising=False)
    monkeypatch.delenv("VO_PREFETCH", raising=False)
    monkeypatch.delenv("VO_PNP_TRI_SPLIT", raising=False)
    if form == "split":
        monkeypatch.setenv("VO_PNP_TRI_SPLIT", "1")
    if form == "prefetch":
        monkeypatch.setenv("VO_PREFETCH", "1")
    eng = Engine(K, dict(opts, dist_coeffs=R.SETS["A"]), 640, 480, batch=1, **CAPS)
    assert eng.dist == (tuple(R.SETS["A"]), None) and np.array_equal(eng.K_rect, K)
    m1, m2, _ = R.case_map("A", 640, 480)
    assert np.array_equal(eng._map1.cpu().numpy(), m1) and np.array_equal(eng._map2.cpu().numpy().view(np.uint16), m2)
    eng.lib = lib = CountingLib(eng.lib)
    frames = raw if form == "host_frames" else torch.from_numpy(raw).cuda()
    eng.bootstrap(frames[BOOT[0]], frames[BOOT[1]])
    assert_state(eng, want[0], f"{form}: bootstrap")
    if form == "graph":
        eng.capture_step()
    lib.calls.clear()
    for k in range(N_STEPS):
        f = frames[BOOT[1] + 1 + k]
        if form == "graph":
            eng.step_graph(f)
        elif form == "prefetch":
            eng.step(f, next_frames=frames[BOOT[1] + 2 + k] if k + 1 < N_STEPS else None)
        else:
            eng.step(f)
        assert_state(eng, want[k + 1], f"{form}: step {k}")
    # one remap launch per frame in every form; with the prefetch one pyramid build per frame too
    # (the step that receives the prefetched frames finds its pyramid built), none in a replay
    assert lib.calls.get("vo_remap_u8") == N_STEPS, lib.calls
    assert lib.calls.get("vo_pyr_build", 0) == (0 if form == "graph" else N_STEPS), lib.calls


def test_engine_rectifies_a_batch_of_three():
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    seeds = [1, 2, 3]
    K, opts, raw, _ = _setup(seeds)
    want = plain_reference(seeds)
    for form in ("eager", "graph"):
        eng = Engine(K, dict(opts, dist_coeffs=tuple(R.SETS["A"])), 640, 480, batch=3, **CAPS)
        frames = torch.from_numpy(raw).cuda()
        eng.bootstrap(frames[BOOT[0]], frames[BOOT[1]])
        assert_state(eng, want[0], f"batch {form}: bootstrap")
        for k in range(N_STEPS):
            (eng.step_graph if form == "graph" else eng.step)(frames[BOOT[1] + 1 + k])
            assert_state(eng, want[k + 1], f"batch {form}: step {k}")


def test_engine_new_camera_matrix_and_zero_coefficients():
    """dist_new_camera_matrix is the pinhole camera every stage works in; all-zero coefficients run the
    remap and give the arrays of the option off."""
    from monocular_visual_odometry_va4mr_amd.engine import Engine
    seeds = [1]
    K, opts, raw, rect = _setup(seeds)
    Kn = K.copy()
    Kn[0, 0] *= 0.9
    Kn[1, 1] *= 0.9
    n1, n2, _ = R.map_ref(K, R.SETS["A"], Kn, 640, 480)
    rect_n = np.stack([R.remap_ref(f[0], n1, n2) for f in raw])[:, None]
    a = Engine(Kn, opts, 640, 480, batch=1, **CAPS)
    b = Engine(K, dict(opts, dist_coeffs=R.SETS["A"], dist_new_camera_matrix=Kn), 640, 480, batch=1, **CAPS)
    assert np.array_equal(b.K, K) and np.array_equal(b.K_rect, Kn) and list(b.opts.K) == list(a.opts.K)
    z = Engine(K, dict(opts, dist_coeffs=R.SETS["Z"]), 640, 480, batch=1, **CAPS)
    off = Engine(K, dict(opts, dist_coeffs=None), 640, 480, batch=1, **CAPS)
    z.lib = lib = CountingLib(z.lib)
    for eng, fr in ((a, rect_n), (b, raw), (z, raw), (off, raw)):
        eng.bootstrap(fr[BOOT[0]], fr[BOOT[1]])
        for k in range(3):
            eng.step(fr[BOOT[1] + 1 + k])
    assert (a.statuses() == 0).all()
    assert_state(b, _state(a), "new camera matrix")
    assert_state(z, _state(off), "zero coefficients")
    assert lib.calls.get("vo_remap_u8") == 5 and off.dist is None and z.dist is not None
    for bad in (dict(dist_coeffs=[0.0] * 6), dict(dist_coeffs=[0.0] * 12), dict(dist_coeffs="0,0,0,0"),
                dict(dist_coeffs=[0, 0, 0, float("nan")]), dict(dist_coeffs=R.SETS["A"], dist_new_camera_matrix=np.eye(4))):
        with pytest.raises(ValueError):
            Engine(K, dict(opts, **bad), 640, 480, batch=1, ncap=64, pcap=64, fcap=4)
    skew = K.copy()
    skew[0, 1] = 1.0
    with pytest.raises(ValueError):
        Engine(skew, dict(opts, dist_coeffs=R.SETS["A"]), 640, 480, batch=1, ncap=64, pcap=64, fcap=4)


def test_dropin_class_passes_the_option_through():
    from monocular_visual_odometry_va4mr_amd.VisualOdometryPipeLine import VisualOdometryPipeLine
    seeds = [1]
    K, opts, raw, _ = _setup(seeds)
    want = plain_reference(seeds)
    for use_graph in (False, True):
        vo = VisualOdometryPipeLine(K, dict(opts, dist_coeffs=R.SETS["A"]), max_frames=CAPS["fcap"],
                                    landmark_capacity=CAPS["ncap"], candidate_capacity=CAPS["pcap"], use_graph=use_graph)
        vo.initialization(raw[BOOT[0], 0], raw[BOOT[1], 0])
        for k in range(N_STEPS):
            vo.continuous_operation(raw[BOOT[1] + 1 + k, 0])
            assert_state(vo._eng, want[k + 1], f"drop-in (graph {use_graph}): step {k}")
        assert vo.K is K and vo._eng.dist is not None and vo.potential_frame is not None
        assert np.array_equal(np.asarray(vo.transforms[-1][1]).ravel(), want[-1]["pose_t"][0, N_STEPS + 1])
