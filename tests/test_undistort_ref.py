"""Lens distortion: the project's definition of the rectification map, the fixed-point remap and the
point undistortion, restated in NumPy, with the properties that hold on the CPU.

The definition has OpenCV's form (initUndistortRectifyMap with CV_16SC2, remap with INTER_LINEAR and
a constant border of 0, undistortPoints with a fixed iteration count) but is the project's own: cv2
is not available, so parity with OpenCV is not pinned here.  Everything is fp64 with one rounding per
operation (NumPy's elementwise ufuncs: no fused multiply-add), products written out and no
transcendental function; the remap is pure integer arithmetic.  csrc/vo_undistort.hip reproduces
all of it bit for bit (tests/test_gpu_undistort.py).
"""
import numpy as np
import pytest

# ------------------------------------------------------------------ the cases
SETS = {
    "A": [-0.28, 0.07, 2e-4, 2e-5, 0.0],                                   # barrel
    "B": [0.12, -0.05, -1e-3, 8e-4, 0.01],                                 # pincushion, with a border
    "C": [-0.2, 0.03, 1e-3, -5e-4, -0.002, 0.05, 0.01, 0.0],               # rational
    "Z": [0.0, 0.0, 0.0, 0.0, 0.0],                                        # the identity
}
SIZES = [(131, 67), (64, 48), (7, 5), (1, 1), (640, 480)]                  # (W, H) of the GPU file's map cases
Q_MIN, Q_MAX = -(1 << 20), (1 << 20) - 1
_CACHE = {}


def size_K(W, H):
    """Parking's intrinsics scaled to a W x H image (parking's own at 640 x 480)."""
    from monocular_visual_odometry_va4mr_amd.synth import intrinsics
    K = intrinsics("parking")
    if (W, H) != (640, 480):
        K[0] *= W / 640.0
        K[1] *= H / 480.0
    return K


def pinhole(K):
    """(fx, fy, cx, cy) of a matrix of the form [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]."""
    K = np.asarray(K, np.float64)
    if K.shape != (3, 3) or not np.all(np.isfinite(K)):
        raise ValueError("a camera matrix is 3x3 and finite")
    if K[0, 1] != 0 or K[1, 0] != 0 or K[2, 0] != 0 or K[2, 1] != 0 or K[2, 2] != 1 or K[0, 0] == 0 or K[1, 1] == 0:
        raise ValueError("a camera matrix has the form [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]")
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def coeffs(dist):
    """k1 k2 p1 p2 k3 k4 k5 k6 of 0, 4, 5 or 8 coefficients in OpenCV's order (missing ones 0)."""
    d = [] if dist is None else [float(v) for v in np.asarray(dist, np.float64).ravel()]
    if len(d) in (12, 14):
        raise NotImplementedError("thin-prism and tilted models (12 or 14 coefficients)")
    if len(d) not in (0, 4, 5, 8):
        raise ValueError("4, 5 or 8 distortion coefficients")
    return tuple(d + [0.0] * (8 - len(d)))


def map_double_ref(K, dist, new_K, W, H):
    """(mx, my) [H][W][2] float64: where the rectified pixel (u, v) lies in the raw image."""
    fx, fy, cx, cy = pinhole(K)
    nfx, nfy, ncx, ncy = pinhole(K if new_K is None else new_K)
    k1, k2, p1, p2, k3, k4, k5, k6 = coeffs(dist)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        x = (u - ncx) / nfx
        y = (v - ncy) / nfy
        r2 = x * x + y * y
        kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = x * kr + p1 * (2.0 * x * y) + p2 * (r2 + 2.0 * x * x)
        yd = y * kr + p1 * (r2 + 2.0 * y * y) + p2 * (2.0 * x * y)
        mx = fx * xd + cx
        my = fy * yd + cy
    return np.stack([mx, my], -1)


def quantise_ref(mx, my):
    """The fixed-point pair of two coordinate maps (float64, or float32 taken to float64 first):
    i = rint(32 m), half to even, clamped to [-2^20, 2^20 - 1], a NaN giving -2^20;
    map1 = (iu >> 5, iv >> 5) int16, map2 = (iv & 31) * 32 + (iu & 31) uint16."""
    def q(m):
        with np.errstate(all="ignore"):
            t = np.rint(32.0 * np.asarray(m, np.float64))
        t = np.where(np.isnan(t), float(Q_MIN), np.clip(t, float(Q_MIN), float(Q_MAX)))
        return t.astype(np.int64)
    iu, iv = q(mx), q(my)
    map1 = np.stack([iu >> 5, iv >> 5], -1).astype(np.int16)
    map2 = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    return map1, map2


def map_ref(K, dist, new_K, W, H):
    """initUndistortRectifyMap(K, dist, None, new_K, (W, H), CV_16SC2): (map1, map2, mapd)."""
    md = map_double_ref(K, dist, new_K, W, H)
    m1, m2 = quantise_ref(md[..., 0], md[..., 1])
    return m1, m2, md


def unpack_ref(map1, map2):
    """(ix, iy, a, b) as int64: the integer source pixel and the 1/32 weights of a fixed-point pair."""
    m2 = np.asarray(map2).astype(np.int64) & 1023
    return map1[..., 0].astype(np.int64), map1[..., 1].astype(np.int64), m2 & 31, m2 >> 5


def taps_inside(map1, map2, sW, sH):
    """[H][W] int: how many of a destination pixel's four taps lie inside an sW x sH source."""
    ix, iy, _, _ = unpack_ref(map1, map2)
    n = np.zeros(ix.shape, np.int64)
    for dx in (0, 1):
        for dy in (0, 1):
            n += (ix + dx >= 0) & (ix + dx < sW) & (iy + dy >= 0) & (iy + dy < sH)
    return n


def remap_ref(src, map1, map2):
    """remap(src, map1, map2, INTER_LINEAR, borderMode = BORDER_CONSTANT, borderValue = 0) of a uint8
    image through a fixed-point pair, in integers; every tap is tested on its own."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 2
    sH, sW = src.shape
    ix, iy, a, b = unpack_ref(map1, map2)

    def S(x, y):
        ok = (x >= 0) & (x < sW) & (y >= 0) & (y < sH)
        return np.where(ok, src[np.clip(y, 0, sH - 1), np.clip(x, 0, sW - 1)].astype(np.int64), 0)

    acc = ((32 - a) * (32 - b) * S(ix, iy) + a * (32 - b) * S(ix + 1, iy) + (32 - a) * b * S(ix, iy + 1)
           + a * b * S(ix + 1, iy + 1) + 512)
    return (acc >> 10).astype(np.uint8)


def undistort_points_ref(pts, K, dist, P=None, iters=5):
    """undistortPoints with a fixed iteration count: raw pixels [..., 2] -> ideal normalised
    coordinates, or pixels through P; float64."""
    fx, fy, cx, cy = pinhole(K)
    k1, k2, p1, p2, k3, k4, k5, k6 = coeffs(dist)
    pts = np.asarray(pts, np.float64)
    with np.errstate(all="ignore"):
        x0 = (pts[..., 0] - cx) / fx
        y0 = (pts[..., 1] - cy) / fy
        x, y = x0, y0
        for _ in range(int(iters)):
            r2 = x * x + y * y
            icd = (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            dx = p1 * (2.0 * x * y) + p2 * (r2 + 2.0 * x * x)
            dy = p1 * (r2 + 2.0 * y * y) + p2 * (2.0 * x * y)
            x = (x0 - dx) * icd
            y = (y0 - dy) * icd
        if P is not None:
            pfx, pfy, pcx, pcy = pinhole(P)
            x = pfx * x + pcx
            y = pfy * y + pcy
    return np.stack([x, y], -1)


def pixel_grid(W, H):
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return np.stack([u, v], -1)


def case_map(name, W, H):
    """(map1, map2, mapd) of coefficient set `name` at W x H with size_K, computed once."""
    key = (name, W, H)
    if key not in _CACHE:
        K = size_K(W, H)
        _CACHE[key] = map_ref(K, SETS[name], None, W, H)
    return _CACHE[key]


def parking_frame():
    """One synthetic 640 x 480 frame (the source of every crop), rendered once."""
    if "frame" not in _CACHE:
        from monocular_visual_odometry_va4mr_amd.synth import make_sequence
        _CACHE["frame"] = np.ascontiguousarray(make_sequence("parking", 1, seed=1)[0][0])
    return _CACHE["frame"]


def crop(W, H, x=37, y=21):
    return np.ascontiguousarray(parking_frame()[y:y + H, x:x + W])


# ------------------------------------------------------------------ properties
@pytest.mark.parametrize("preset", ["parking", "kitti"])
def test_zero_coefficients_are_the_identity(preset):
    from monocular_visual_odometry_va4mr_amd.synth import SIZES as PS, intrinsics
    W, H = PS[preset]
    m1, m2, md = map_ref(intrinsics(preset), SETS["Z"], None, W, H)
    g = pixel_grid(W, H)
    assert np.array_equal(m1, g.astype(np.int16)) and not m2.any()
    if preset == "parking":
        img = parking_frame()
        assert np.array_equal(remap_ref(img, m1, m2), img)
    # no coefficients at all are the same camera
    assert np.array_equal(map_double_ref(intrinsics(preset), None, None, W, H), md)


def test_pincushion_leaves_a_border():
    """B on parking: some destination pixels have all four taps outside the source and are 0, some
    have a part of them outside and blend with 0."""
    m1, m2, _ = case_map("B", 640, 480)
    n = taps_inside(m1, m2, 640, 480)
    frac = float((n == 0).mean())
    assert 0.10 < frac < 0.14, frac                          # 11.8 % here
    assert ((n > 0) & (n < 4)).any()
    img = np.full((480, 640), 200, np.uint8)
    out = remap_ref(img, m1, m2)
    assert np.all(out[n == 0] == 0) and np.all(out[n == 4] == 200)
    part = (n > 0) & (n < 4)
    ix, iy, a, b = unpack_ref(m1, m2)
    blended = part & (out > 0) & (out < 200)
    assert blended.any() and np.all(out[part] <= 200)
    from monocular_visual_odometry_va4mr_amd.synth import intrinsics
    mk = map_ref(intrinsics("kitti"), SETS["B"], None, 1241, 376)
    fk = float((taps_inside(mk[0], mk[1], 1241, 376) == 0).mean())
    assert 0.07 < fk < 0.09, fk                              # 8.1 % here


@pytest.mark.parametrize("name", ["A", "C"])
def test_barrel_and_rational_fill_the_frame(name):
    m1, m2, _ = case_map(name, 640, 480)
    assert (taps_inside(m1, m2, 640, 480) > 0).all()


def test_round_trip_through_the_point_undistortion():
    """undistort_points_ref(mapd, P = new_K) returns the pixel grid once it has converged; OpenCV's
    default of 5 iterations visibly has not."""
    K = size_K(640, 480)
    g = pixel_grid(640, 480)
    _, _, md = case_map("A", 640, 480)
    err = lambda it, d, name: float(np.abs(undistort_points_ref(d, K, SETS[name], P=K, iters=it) - g).max())
    e5, e50 = err(5, md, "A"), err(50, md, "A")
    assert e5 > 0.1 and e50 < 1e-9, (e5, e50)                # 0.55 px and 3.7e-13 px here
    _, _, mc = case_map("C", 640, 480)
    e100 = err(100, mc, "C")
    assert e100 < 1e-9, e100                                 # 7.6e-13 px here
    # another new matrix: the grid comes back through it
    Kn = K.copy()
    Kn[0, 0] *= 0.9
    Kn[1, 1] *= 0.9
    Kn[0, 2] += 3.5
    mn = map_double_ref(K, SETS["A"], Kn, 640, 480)
    assert float(np.abs(undistort_points_ref(mn, K, SETS["A"], P=Kn, iters=50) - g).max()) < 1e-9
    # without P the output is normalised
    n = undistort_points_ref(md[::37, ::41], K, SETS["A"], iters=50)
    assert np.allclose(n[..., 0] * K[0, 0] + K[0, 2], g[::37, ::41, 0], atol=1e-9)


def test_quantiser_ties_nan_and_clamp():
    mx = np.array([[3 + 1 / 64, 3 + 3 / 64, -1 / 64, np.nan, 1e9, -1e9, np.inf, -np.inf]], np.float32)
    my = np.zeros_like(mx)
    m1, m2 = quantise_ref(mx, my)
    iu = m1[..., 0].astype(np.int64) * 32 + (m2.astype(np.int64) & 31)
    assert iu[0].tolist() == [96, 98, 0, Q_MIN, Q_MAX, Q_MIN, Q_MAX, Q_MIN]
    assert m1.dtype == np.int16 and m2.dtype == np.uint16
    assert m1[0, 3, 0] == -32768 and m1[0, 4, 0] == 32767 and m2[0, 4] == 31 and m2[0, 3] == 0
    img = np.full((8, 8), 255, np.uint8)
    out = remap_ref(img, m1, m2)
    assert out[0, 3:].tolist() == [0, 0, 0, 0, 0] and out[0, 0] == 255
    # the same on the other axis
    m1, m2 = quantise_ref(my, mx)
    iv = m1[..., 1].astype(np.int64) * 32 + (m2.astype(np.int64) >> 5)
    assert iv[0].tolist() == [96, 98, 0, Q_MIN, Q_MAX, Q_MIN, Q_MAX, Q_MIN]


def test_every_weight_pair_is_exercised_and_map2_round_trips():
    seen = np.zeros((32, 32), bool)
    for name in SETS:
        for W, H in SIZES:
            m1, m2, md = case_map(name, W, H)
            _, _, a, b = unpack_ref(m1, m2)
            seen[a.ravel(), b.ravel()] = True
            assert m2.max() < 1024
            iu = np.rint(32.0 * md[..., 0]).astype(np.int64)
            iv = np.rint(32.0 * md[..., 1]).astype(np.int64)
            assert np.array_equal(m1[..., 0].astype(np.int64) * 32 + a, iu)
            assert np.array_equal(m1[..., 1].astype(np.int64) * 32 + b, iv)
    assert seen.all()
    a, b = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    packed = (b * 32 + a).astype(np.uint16)
    _, _, a2, b2 = unpack_ref(np.zeros((32, 32, 2), np.int16), packed)
    assert np.array_equal(a2, a) and np.array_equal(b2, b)


def test_the_weights_are_opencvs_table_over_32():
    """a/32 * b/32 * 32768 is an integer, so OpenCV's 15-bit weight table holds exactly 32 times these
    weights, and (sum + 2^14) >> 15 of the one is (sum + 512) >> 10 of the other."""
    a, b = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    w = np.stack([(32 - a) * (32 - b), a * (32 - b), (32 - a) * b, a * b], -1)
    assert np.all(w.sum(-1) == 1024)
    tab = np.stack([(1 - a / 32) * (1 - b / 32), a / 32 * (1 - b / 32), (1 - a / 32) * b / 32, a / 32 * b / 32], -1) * 32768
    assert np.array_equal(tab, np.rint(tab)) and np.array_equal(tab.astype(np.int64), 32 * w)
    rng = np.random.default_rng(0)
    s = rng.integers(0, 256, (32, 32, 4))
    assert np.array_equal(((32 * w * s).sum(-1) + (1 << 14)) >> 15, ((w * s).sum(-1) + 512) >> 10)


def test_argument_errors_of_the_restatement():
    K = size_K(64, 48)
    with pytest.raises(NotImplementedError):
        coeffs([0.0] * 12)
    with pytest.raises(NotImplementedError):
        coeffs([0.0] * 14)
    for n in (1, 3, 6, 7, 9):
        with pytest.raises(ValueError):
            coeffs([0.0] * n)
    bad = K.copy()
    bad[0, 1] = 0.5
    with pytest.raises(ValueError):
        map_ref(bad, SETS["A"], None, 4, 4)
    with pytest.raises(ValueError):
        map_ref(K, SETS["A"], np.eye(4), 4, 4)


# ------------------------------------------------------------------ symbols, options, drivers
def test_abi_declares_the_entry_points():
    import ctypes
    import os
    from monocular_visual_odometry_va4mr_amd import _lib as L
    for name in ("vo_undistort_map", "vo_remap_u8", "vo_undistort_points"):
        assert name in L.exported_symbols()
    if not os.path.exists(L.LIB_PATH):
        L.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    L._declare(lib)
    assert len(lib.vo_undistort_map.argtypes) == 10 and len(lib.vo_remap_u8.argtypes) == 14
    assert len(lib.vo_undistort_points.argtypes) == 9


def test_bad_host_arguments_are_rejected_without_a_gpu():
    """Every VO_EARG is decided on the host before anything is launched, so it shows without a device."""
    import ctypes as C
    import os
    from monocular_visual_odometry_va4mr_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        L.build()
    lib = C.CDLL(L.LIB_PATH)
    L._declare(lib)
    K = (C.c_double * 9)(300, 0, 32, 0, 300, 24, 0, 0, 1)
    Kbad = (C.c_double * 9)(300, 1, 32, 0, 300, 24, 0, 0, 1)
    d = (C.c_double * 8)()
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p)
    q = C.c_void_p(p.value + 2048)
    assert lib.vo_undistort_map(K, d, 6, None, 8, 8, p, q, None, None) == -1
    assert lib.vo_undistort_map(Kbad, d, 5, None, 8, 8, p, q, None, None) == -1
    assert lib.vo_undistort_map(K, d, 5, None, 0, 8, p, q, None, None) == -1
    assert lib.vo_undistort_map(K, d, 5, None, 8, 16385, p, q, None, None) == -1
    assert lib.vo_remap_u8(1, p, 64, 7, 8, 8, q, 64, 8, 8, 8, p, p, None) == -1        # pitch below width
    assert lib.vo_remap_u8(1, p, 64, 8, 8, 8, p, 64, 8, 8, 8, q, q, None) == -1        # dst is src
    assert lib.vo_undistort_points(4, p, K, d, 5, None, 0, q, None) == -1
    assert lib.vo_undistort_points(4, p, K, d, 5, None, 101, q, None) == -1
    assert lib.vo_undistort_points(0, p, K, d, 5, None, 5, q, None) == 0               # nothing to do, nothing launched


def test_parse_dist():
    from monocular_visual_odometry_va4mr_amd.engine import parse_dist
    assert parse_dist({}) is None and parse_dist({"dist_coeffs": None}) is None
    for name, d in SETS.items():
        got = parse_dist({"dist_coeffs": d})
        assert got == (tuple(d), None), name
    got = parse_dist({"dist_coeffs": np.array(SETS["A"], np.float32)[:4]})
    assert len(got[0]) == 4 and got[0][0] == float(np.float32(-0.28))
    Kn = size_K(64, 48)
    got = parse_dist({"dist_coeffs": tuple(SETS["C"]), "dist_new_camera_matrix": Kn.tolist()})
    assert got[0] == tuple(SETS["C"]) and np.array_equal(got[1], Kn) and got[1].dtype == np.float64
    for bad in ([], [0.1], [0.0] * 3, [0.0] * 6, [0.0] * 12, [0.0] * 14, 0.1, "0,0,0,0", [0, 0, 0, "x"], [0, 0, 0, float("nan")],
                [0, 0, float("inf"), 0], [True, 0, 0, 0], [[0, 0, 0, 0]], True):
        with pytest.raises(ValueError):
            parse_dist({"dist_coeffs": bad})
    skew = Kn.copy()
    skew[0, 1] = 1.0
    for bad in (np.eye(4), skew, "K", [1, 2, 3], np.full((3, 3), np.nan), np.diag([0.0, 1.0, 1.0])):
        with pytest.raises(ValueError):
            parse_dist({"dist_coeffs": SETS["A"], "dist_new_camera_matrix": bad})
    with pytest.raises(ValueError):                          # validated with the option off too
        parse_dist({"dist_new_camera_matrix": skew})
    assert parse_dist({"dist_new_camera_matrix": Kn}) is None


def test_drivers_pass_dist_coeffs_into_the_options(monkeypatch):
    """--dist-coeffs reaches the options dict the pipeline is built from, in both drivers; no engine
    and no GPU are involved: the pipeline class and the engine class are stand-ins that stop the run."""
    import sys
    from monocular_visual_odometry_va4mr_amd import options as Op
    from monocular_visual_odometry_va4mr_amd import run_dataset as RD
    from monocular_visual_odometry_va4mr_amd import run_sequence as RS
    from monocular_visual_odometry_va4mr_amd import VisualOdometryPipeLine as VP

    assert Op.parse_dist_arg("-0.28,0.07,2e-4,2e-5") == [-0.28, 0.07, 2e-4, 2e-5]
    assert Op.parse_dist_arg(" 1, 2,3 ,4,5,6,7,8") == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]
    for bad in ("", "1,2,3", "1,2,3,x", "1,2,3,4,5,6", "1,2,3,4,"):
        with pytest.raises(ValueError):
            Op.parse_dist_arg(bad)

    class Stop(Exception):
        pass

    seen = []

    class FakePipe:
        def __init__(self, K, options, **kw):
            seen.append(dict(options))
            raise Stop

    monkeypatch.setattr(VP, "VisualOdometryPipeLine", FakePipe)
    with pytest.raises(Stop):
        RD.run("synthetic-parking", None, last_frame=8, plot=None, device="cpu", dist_coeffs=SETS["A"])
    assert seen[-1]["dist_coeffs"] == SETS["A"]
    with pytest.raises(Stop):
        RD.run("synthetic-parking", None, last_frame=8, plot=None, device="cpu")
    assert "dist_coeffs" not in seen[-1]

    class FakeEngine:
        def __init__(self, K, options, *a, **kw):
            seen.append(dict(options))
            raise Stop

    with pytest.raises(Stop):
        RS.run("parking", 12, 1, overlap=2, device="cpu", engine_cls=FakeEngine, dist_coeffs=SETS["C"], prerender=False)
    assert seen[-1]["dist_coeffs"] == SETS["C"]

    # the command lines
    calls = []
    monkeypatch.setattr(RD, "run", lambda *a, **kw: calls.append(kw) or {"frames": 0})
    monkeypatch.setattr(sys, "argv", ["run_dataset", "--dataset", "synthetic-parking", "--dist-coeffs=-0.28,0.07,2e-4,2e-5,0"])
    RD.main()
    assert calls[-1]["dist_coeffs"] == SETS["A"]
    monkeypatch.setattr(sys, "argv", ["run_dataset", "--dataset", "synthetic-parking"])
    RD.main()
    assert calls[-1]["dist_coeffs"] is None
    monkeypatch.setattr(RS, "run", lambda *a, **kw: calls.append(kw) or None)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["run_sequence", "--dist-coeffs", "0.12,-0.05,-1e-3,8e-4,0.01"])
    monkeypatch.setattr(RS.torch.cuda, "set_device", lambda *a: None)
    RS.main()
    assert calls[-1]["dist_coeffs"] == SETS["B"]
