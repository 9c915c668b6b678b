"""Cases, oracle expectations and batched C-ABI wrappers for the geometry edge tests.

test_geom_cases_ref.py (CPU) asserts on the oracle alone that every case below reaches the code it
is named for; test_gpu_geometry_edges.py runs the same cases through libvo_hip.so with B > 1 and
ragged counts and compares every problem with the oracle run on that problem alone.

Scenes follow the recipes of test_pnp_ransac_matches_oracle / test_essential_and_recover_pose
(K_KITTI, points a few to 60 units ahead), every generator takes its own seeded default_rng.
Nothing here needs a GPU at import time.
"""
import ctypes as C
import math

import numpy as np

F32 = np.float32
IMG_W, IMG_H = 1241.0, 376.0
SENT_F64 = -7777.25          # sentinels the outputs are pre-filled with
SENT_F32 = F32(-7777.25)
SENT_I32 = -99
SENT_U8 = 0xAB


def K_():
    from monocular_visual_odometry_va4mr_amd.synth import K_KITTI
    return K_KITTI.copy()


def same_bits(a, b):
    """Bit-for-bit equality of two float arrays with the NaN rule: NaNs at the same positions (their
    sign and payload differ between host and device), the bit patterns of everything else."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return np.array_equal(a.view(u)[~na], b.view(u)[~nb])


# ====================================================================== PnP cases
def _project(X, R, t, K):
    x = (X @ R.T + t) @ K.T
    return x[:, :2] / x[:, 2:]


def _pose(rng):
    from oracle import _olib as O
    return O.rodrigues(rng.normal(size=3) * 0.05), rng.normal(size=3) * 0.5


def pnp_scene(seed, n, outlier_frac=0.0, noise=0.0, planar=False):
    """n points in front of a random pose, projected; the first outlier_frac * n image points are
    moved 10..80 px away.  planar: the object points lie on one tilted plane."""
    rng = np.random.default_rng(seed)
    R, t = _pose(rng)
    X = rng.uniform([-8, -3, 4], [8, 3, 60], (n, 3))
    if planar:
        X[:, 2] = 20.0 + 0.3 * X[:, 0] - 0.2 * X[:, 1]
    x = _project(X, R, t, K_())
    if noise:
        x = x + rng.normal(size=(n, 2)) * noise
    nout = int(round(outlier_frac * n))
    x[:nout] += rng.uniform(10, 80, (nout, 2)) * rng.choice([-1, 1], (nout, 2))
    return X.astype(F32), x.astype(F32)


def pnp_random_image(seed, n):
    """Object points of a scene, image points uniform over the image: no pose explains them."""
    rng = np.random.default_rng(seed)
    X = rng.uniform([-8, -3, 4], [8, 3, 60], (n, 3))
    x = np.c_[rng.uniform(0, IMG_W, n), rng.uniform(0, IMG_H, n)]
    return X.astype(F32), x.astype(F32)


def pnp_identical(n):
    X = np.tile(F32([[1.5, -0.5, 12.0]]), (n, 1))
    x = np.tile(F32([[700.25, 180.5]]), (n, 1))
    return X, x


# name -> (obj, img); the counts named by the issue, then the scene kinds
def pnp_cases():
    c = {}
    c["n0"] = (np.zeros((0, 3), F32), np.zeros((0, 2), F32))
    c["n3"] = tuple(a[:3] for a in pnp_scene(103, 8))
    c["n4_solvable"] = pnp_scene(104, 4)
    c["n4_identical"] = pnp_identical(4)
    for n in (5, 6, 7, 8, 9, 12):
        c[f"clean_{n}"] = pnp_scene(200 + n, n)
    for n in (63, 64, 65, 255, 256, 257):
        c[f"noisy_{n}"] = pnp_scene(300 + n, n, outlier_frac=0.3, noise=0.7)
    c["outl50_300"] = pnp_scene(350, 300, outlier_frac=0.5, noise=0.7)
    c["outl80_300"] = pnp_scene(380, 300, outlier_frac=0.8, noise=0.7)
    c["planar_8"] = pnp_scene(408, 8, planar=True)
    c["planar_100"] = pnp_scene(410, 100, planar=True)
    c["randimg_50"] = pnp_random_image(550, 50)
    c["randimg_300"] = pnp_random_image(560, 300)
    c["identical_6"] = pnp_identical(6)
    # few points, noise and one or two outliers: several iterations with the subsets drawn by the
    # serial tail of pnp_subsets (at n = 5 four draws repeat with probability 0.81)
    for n in (5, 6, 8, 12):
        X, x = pnp_scene(450 + 10 * n, n, noise=0.7)
        k = 1 if n < 8 else 2
        x[n - k:] += np.random.default_rng(n).uniform(20, 60, (k, 2)).astype(F32)
        c[f"small_outl_{n}"] = (X, x)
    return c


PNP_REF_OPTS = (500, 8.0, 0.99)           # the reference's iterationsCount, reprojectionError, confidence
PNP_MAIN = ["n0", "n3", "n4_solvable", "n4_identical", "clean_5", "clean_6", "clean_7", "clean_8", "clean_9",
            "clean_12", "noisy_63", "noisy_64", "noisy_65", "noisy_255", "noisy_256", "noisy_257", "outl50_300",
            "outl80_300", "planar_8", "planar_100", "randimg_50", "randimg_300", "identical_6", "small_outl_5",
            "small_outl_6", "small_outl_8", "small_outl_12"]


def pnp_fail_cases():
    """uniform-random image points, for the (100, 0.5 px, 0.99) batch: every one fails"""
    return {f"randimg_{n}": pnp_random_image(550 + i, n) for i, n in enumerate((5, 8, 50, 300))}


# the smaller batches at other options: (iterations, error, confidence) -> case names
PNP_OTHER = {
    (1, 8.0, 0.99): ["clean_5", "clean_12", "noisy_65", "outl50_300", "randimg_50", "n4_solvable", "n3",
                     "small_outl_5"],
    (100, 2.0, 0.9999): ["clean_6", "noisy_64", "noisy_257", "outl50_300", "planar_100", "randimg_300",
                         "small_outl_6", "small_outl_12"],
    (100, 8.0, 0.5): ["clean_7", "noisy_63", "noisy_256", "outl80_300", "planar_8", "identical_6"],
    (1000, 1.0, 0.999999): ["clean_9", "noisy_255", "outl50_300", "outl80_300", "n0", "n4_identical"],
}


def pnp_expect(obj, img, iters, err, conf):
    """The oracle on one problem: dict(success, n_inl, mask [n] u8, rvec, tvec, iters).  The oracle
    wrapper refuses n < 4 (as cv2 does); there the expectation is success = 0, n_inl = 0 and nothing
    else written (mask None)."""
    from oracle import _olib as O
    n = len(obj)
    if n < 4:
        return dict(success=0, n_inl=0, mask=None, rvec=None, tvec=None, iters=0)
    ok, rv, tv, inl, it = O.pnp_ransac_p3p(obj, img, K_(), iters, err, conf)
    mask = np.zeros(n, np.uint8)
    if ok:
        mask[inl] = 1
    return dict(success=int(ok), n_inl=len(inl) if ok else 0, mask=mask, rvec=rv.ravel() if ok else None,
                tvec=tv.ravel() if ok else None, iters=it)


# ====================================================================== E cases
def _two_view(rng, X, R, t, noise):
    K = K_()
    Xh = np.c_[X, np.ones(len(X))].T
    a = K @ np.hstack([np.eye(3), np.zeros((3, 1))]) @ Xh
    b = K @ np.hstack([R, np.reshape(t, (3, 1))]) @ Xh
    a = (a[:2] / a[2]).T + rng.normal(size=(len(X), 2)) * noise
    b = (b[:2] / b[2]).T + rng.normal(size=(len(X), 2)) * noise
    return a, b


def ess_scene(seed, n, outlier_frac=0.0, noise=0.0, kind="general"):
    """Two views of n points; kind: general / planar (points on one plane) / rotation (t = 0)."""
    from oracle import _olib as O
    rng = np.random.default_rng(seed)
    R = O.rodrigues(np.array([0.01, -0.03, 0.005]))
    t = np.array([0.05, -0.02, 1.0])
    X = rng.uniform([-10, -3, 6], [10, 3, 60], (n, 3))
    if kind == "planar":
        X[:, 2] = 25.0 + 0.4 * X[:, 0] - 0.3 * X[:, 1]
    if kind == "rotation":
        R, t = O.rodrigues(np.array([0.02, -0.06, 0.01])), np.zeros(3)
    a, b = _two_view(rng, X, R, t, noise)
    nout = int(round(outlier_frac * n))
    b[:nout] += rng.uniform(5, 40, (nout, 2))
    return a.astype(F32), b.astype(F32)


def ess_random(seed, n):
    rng = np.random.default_rng(seed)
    a = np.c_[rng.uniform(0, IMG_W, n), rng.uniform(0, IMG_H, n)]
    b = np.c_[rng.uniform(0, IMG_W, n), rng.uniform(0, IMG_H, n)]
    return a.astype(F32), b.astype(F32)


def ess_identical(n):
    return np.tile(F32([[400.5, 100.25]]), (n, 1)), np.tile(F32([[410.75, 99.5]]), (n, 1))


def ess_cases():
    c = {}
    for n in (0, 1, 4):
        c[f"n{n}"] = tuple(a[:n] for a in ess_scene(600 + n, 8))
    for n in (5, 6, 7, 8, 9):
        c[f"clean_{n}"] = ess_scene(610 + n, n)
    for n in (63, 64, 65, 257):
        c[f"noisy_{n}"] = ess_scene(700 + n, n, outlier_frac=0.2, noise=0.3)
    for pct in (30, 50, 60, 70):
        c[f"outl{pct}_300"] = ess_scene(800 + pct, 300, outlier_frac=pct / 100.0, noise=0.3)
    c["planar_200"] = ess_scene(901, 200, noise=0.3, kind="planar")
    c["rotation_200"] = ess_scene(902, 200, noise=0.3, kind="rotation")
    for n in (6, 8, 40):
        c[f"random_{n}"] = ess_random(910 + n, n)
    c["identical_8"] = ess_identical(8)
    return c


ESS_REF_OPTS = (0.99, 1.0, 1000)          # prob, threshold, max_iters of the bootstrap (:308)
ESS_MAIN = ["n0", "n1", "n4", "clean_5", "clean_6", "clean_7", "clean_8", "clean_9", "noisy_63", "noisy_64",
            "noisy_65", "noisy_257", "outl30_300", "outl50_300", "outl60_300", "outl70_300", "planar_200",
            "rotation_200", "random_6", "random_8", "random_40", "identical_8"]
_ESS_SMALL = ["clean_5", "clean_6", "noisy_65", "outl50_300", "planar_200", "rotation_200", "random_6", "random_8",
              "random_40", "identical_8", "n4"]
ESS_OTHER = {
    (0.999, 1.0, 1000): ["clean_6", "noisy_64", "noisy_257", "outl30_300", "outl60_300", "random_40"],
    (0.99, 0.5, 1000): _ESS_SMALL,
    (0.99, 3.0, 1000): _ESS_SMALL,
    (0.99, 1.0, 1): _ESS_SMALL,
    (0.99, 1.0, 50): _ESS_SMALL,
}


def ess_expect(p0, p1, prob, thr, max_iters):
    from oracle import _olib as O
    ok, E, mask = O.find_essential(p0, p1, K_(), prob, thr, max_iters)
    return dict(ok=int(ok), E=E.ravel(), mask=mask)


def ransac_niters(prob, n, good, model_points, max_iters):
    """RANSACUpdateNumIters from a final inlier count (a float; the kernels round it)"""
    ep = (n - good) / n
    den = 1.0 - (1.0 - ep) ** model_points
    if den <= 0:
        return 0.0
    if den >= 1:
        return float(max_iters)
    return min(float(max_iters), math.log(1.0 - prob) / math.log(den))


# ====================================================================== recoverPose cases
def recover_cases():
    """[(name, E [9], p0, p1)]: the oracle's E of every ok problem of the main E batch with its points,
    the same with the views swapped, -E; matrices that are no essential matrices; the counts 0, 1, 255,
    256, 257; depths either side of the 50-unit cut at |t| = 1; correspondences with p0 == p1."""
    from oracle import _olib as O
    out = []
    ec = ess_cases()
    for name in ESS_MAIN:
        p0, p1 = ec[name]
        e = ess_expect(p0, p1, *ESS_REF_OPTS)
        if not e["ok"]:
            continue
        out.append((f"E_{name}", e["E"], p0, p1))
        out.append((f"E_{name}_swapped", e["E"], p1, p0))
        out.append((f"E_{name}_neg", -e["E"], p0, p1))
    rng = np.random.default_rng(77)
    for i in range(8):
        n = int(rng.integers(1, 40))
        out.append((f"notE_{i}", rng.normal(size=9), *ess_random(1000 + i, n)))
    p0, p1 = ess_scene(1100, 257, outlier_frac=0.2, noise=0.3)
    E = ess_expect(p0, p1, *ESS_REF_OPTS)["E"]
    for n in (0, 1, 255, 256, 257):
        out.append((f"count_{n}", E, p0[:n], p1[:n]))
    # depths 30..70 with a unit baseline: both sides of recoverPose's distance cut of 50
    rng = np.random.default_rng(78)
    X = np.c_[rng.uniform(-10, 10, 120), rng.uniform(-3, 3, 120), rng.uniform(30, 70, 120)]
    R = O.rodrigues(np.array([0.01, -0.03, 0.005]))
    t = np.array([0.6, 0.0, 0.8])
    a, b = _two_view(rng, X, R, t, 0.0)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    out.append(("depth_cut", (tx @ R).ravel(), a.astype(F32), b.astype(F32)))
    # no rotation between the views: p0 == p1 is then a pair of parallel rays, a point at infinity
    for name, t2 in (("infinity", np.array([0.6, 0.1, 0.79])), ("infinity_skew_with_zeros", t)):
        a2, b2 = _two_view(rng, X[:20], np.eye(3), t2, 0.0)
        a2, b2 = a2.astype(F32), b2.astype(F32)
        b2[:3] = a2[:3]
        tx2 = np.array([[0, -t2[2], t2[1]], [t2[2], 0, -t2[0]], [-t2[1], t2[0], 0]])
        out.append((name, tx2.ravel(), a2, b2))
    return out


def recover_expect(E, p0, p1):
    from oracle import _olib as O
    ng, R, t, mask = O.recover_pose(np.reshape(E, (3, 3)), p0, p1, K_())
    return dict(n_good=ng, R=R.ravel(), t=t.ravel(), mask=mask)


# ====================================================================== triangulatePoints cases
def tri_cases(n=1000):
    """(P1 [n][12], P2 [n][12], x1 [n][2] f32, x2 [n][2] f32): one camera pair per point, K[R|t]
    cameras and rng.normal matrices mixed; the first points are the edges (point 0 is an ordinary
    one, so that n = 1 is the comfortable case of the existing test)."""
    from oracle import _olib as O
    rng = np.random.default_rng(21)
    K = K_()
    P1 = np.zeros((n, 12))
    P2 = np.zeros((n, 12))
    x1 = np.zeros((n, 2), F32)
    x2 = np.zeros((n, 2), F32)
    for i in range(n):
        if i % 3 == 2:
            P1[i], P2[i] = rng.normal(size=12), rng.normal(size=12)
            x1[i], x2[i] = rng.normal(size=2), rng.normal(size=2)
        else:
            Ra, ta = O.rodrigues(rng.normal(size=3) * 0.05), rng.normal(size=3) * 0.3
            Rb, tb = O.rodrigues(rng.normal(size=3) * 0.05), rng.normal(size=3) * 0.3 + [0, 0, 1.0]
            X = rng.uniform([-8, -3, 4], [8, 3, 60], (1, 3))
            P1[i] = (K @ np.c_[Ra, ta]).ravel()
            P2[i] = (K @ np.c_[Rb, tb]).ravel()
            x1[i] = _project(X, Ra, ta, K)[0] + rng.normal(size=2) * 0.5
            x2[i] = _project(X, Rb, tb, K)[0] + rng.normal(size=2) * 0.5
    if n > 8:
        P2[1] = P1[1]                                            # P1 == P2, different image points
        P2[2] = P1[2]; x2[2] = x1[2]                             # P1 == P2 and the same image point
        # exactly parallel rays: the same rotation, a sideways baseline, the same image point
        P1[3] = (K @ np.c_[np.eye(3), np.zeros(3)]).ravel()
        P2[3] = (K @ np.c_[np.eye(3), [1.0, 0, 0]]).ravel()
        x1[3] = x2[3] = F32([650.0, 190.0])
        x1[4] = 0; x2[4] = 0                                     # coordinates of exactly 0
        x1[5, 0] = 0; x2[5, 1] = 0
        x1[6] = F32([1e6, -1e6]); x2[6] = F32([-1e6, 1e6])       # magnitudes of 1e6
        P1[7] *= 1e6
        x1[8] = F32([1e6, 3.0])
    return P1, P2, x1, x2


def tri_expect(P1, P2, x1, x2):
    """The oracle takes one camera pair per call: one call per point.  [n][4] f32."""
    from oracle import _olib as O
    out = np.zeros((len(x1), 4), F32)
    for i in range(len(x1)):
        out[i] = O.triangulate(P1[i].reshape(3, 4), P2[i].reshape(3, 4), x1[i].reshape(2, 1),
                               x2[i].reshape(2, 1)).ravel()
    return out


# ====================================================================== Rodrigues cases
def rod_vectors():
    """name -> rotation vector"""
    pi = math.pi
    u = lambda *a: np.array(a, float) / np.linalg.norm(a)
    v = {"zero": np.zeros(3)}
    for nrm in (1e-17, 2.2e-16, 3e-16, 1e-8, 5e-6, 2e-5):
        v[f"norm_{nrm:g}"] = u(1, -2, 0.5) * nrm
    for name, ax in (("+x", (1, 0, 0)), ("-x", (-1, 0, 0)), ("+y", (0, 1, 0)), ("-y", (0, -1, 0)),
                     ("+z", (0, 0, 1)), ("-z", (0, 0, -1)), ("111", (1, 1, 1)), ("neg1", (1, -2, 3)),
                     ("neg1b", (-1, 2, 3)), ("neg2", (-1, -2, 3)), ("neg2b", (1, -2, -3)),
                     ("smallx", (0.1, -2, 3)), ("smallx2", (0.1, 2, -3))):
        v[f"pi_{name}"] = u(*ax) * pi
    for name, th in (("pi-1e-7", pi - 1e-7), ("pi-2e-5", pi - 2e-5), ("pi+1e-3", pi + 1e-3)):
        v[name] = u(1, -2, 0.5) * th
        v[name + "_b"] = u(0.1, 2, -3) * th
    v["321"] = np.array([3.0, 2.0, 1.0])
    v["norm_100"] = u(2, -1, 3) * 100.0
    return v


def rod_matrices():
    """name -> 3x3 for the matrix-to-vector direction: the images of rod_vectors, then matrices that
    are not rotations (the SVD orthogonalisation)."""
    from oracle import _olib as O
    rng = np.random.default_rng(31)
    m = {f"R({k})": O.rodrigues(v) for k, v in rod_vectors().items()}
    R = O.rodrigues(np.array([0.3, -0.2, 0.5]))
    m["noisy"] = R + 1e-3 * rng.normal(size=(3, 3))
    m["noisy_pi"] = O.rodrigues(np.array([0.1, 2, -3.0]) / np.linalg.norm([0.1, 2, -3]) * math.pi) \
        + 1e-3 * rng.normal(size=(3, 3))
    m["2R"] = 2.0 * R
    m["rank2"] = R @ np.diag([1.0, 0.5, 0.0])
    m["zero"] = np.zeros((3, 3))
    m["diag(1,-1,-1)"] = np.diag([1.0, -1.0, -1.0])
    m["diag(-1,1,-1)"] = np.diag([-1.0, 1.0, -1.0])
    m["diag(-1,-1,1)"] = np.diag([-1.0, -1.0, 1.0])
    return m


def rod_batch(specials, n, seed, shape):
    """n inputs: the specials tiled and interleaved with random ones (even slots special)"""
    rng = np.random.default_rng(seed)
    sp = list(specials)
    out = np.zeros((n,) + shape)
    for i in range(n):
        out[i] = sp[(i // 2) % len(sp)] if i % 2 == 0 else rng.normal(size=shape)
    return out


def rod_expect(batch):
    from oracle import _olib as O
    to_matrix = batch.shape[1:] == (3,)
    out = np.zeros((len(batch), 9 if to_matrix else 3))
    for i, a in enumerate(batch):
        out[i] = O.rodrigues(a).ravel()
    return out


# ====================================================================== ratio-test cases
FLT_MAX = float(np.finfo(F32).max)
RATIO_NQ = (0, 1, 257, 700)
RATIO_KP_STRIDE, RATIO_Q_STRIDE = 900, 800


def ratio_case(ratio, seed):
    """B = 4 problems, nq = 0, 1, 257, 700: keypoints kp0 / kp1 [B][kp_stride][6], idx2 / dist2
    [B][q_stride][2].  Every 7th row has idx[:, 1] = -1 (the one-train-descriptor shape), every 11th
    both -1, every 5th an exact tie d0 == ratio * d1 in double, every 13th a distance of FLT_MAX."""
    rng = np.random.default_rng(seed)
    B = len(RATIO_NQ)
    kp0 = rng.uniform(0, 1000, (B, RATIO_KP_STRIDE, 6)).astype(F32)
    kp1 = rng.uniform(0, 1000, (B, RATIO_KP_STRIDE, 6)).astype(F32)
    idx = rng.integers(0, RATIO_KP_STRIDE, (B, RATIO_Q_STRIDE, 2)).astype(np.int32)
    d1 = rng.uniform(50, 500, (B, RATIO_Q_STRIDE)).astype(F32)
    d0 = (d1 * rng.uniform(0.3, 1.0, d1.shape)).astype(F32)
    ties = ratio_ties(ratio)
    for b in range(B):
        for i in range(RATIO_Q_STRIDE):
            if i % 5 == 4:
                d0[b, i], d1[b, i] = ties[(i // 5) % len(ties)]
            if i % 13 == 12:
                if i % 2:
                    d0[b, i], d1[b, i] = FLT_MAX, FLT_MAX          # dropped: not < ratio * itself
                else:
                    d0[b, i], d1[b, i] = 1.0, FLT_MAX              # kept
            if i % 7 == 6:
                idx[b, i, 1] = -1
                d1[b, i] = FLT_MAX
            if i % 11 == 10:
                idx[b, i] = -1
                d0[b, i] = d1[b, i] = FLT_MAX
    dist = np.stack([d0, d1], -1).astype(F32)
    return kp0, kp1, idx, dist


def ratio_ties(ratio):
    """(d0, d1) float pairs with (double)d0 == ratio * (double)d1 exactly, then the neighbours of the
    first pair just below (kept) and just above (dropped)."""
    if ratio == 0.5:
        t = [(1.0, 2.0), (64.0, 128.0), (3.5, 7.0)]
    else:
        t = [(4.0, 5.0), (8.0, 10.0), (2.0, 2.5)]       # 0.8 * 5.0 rounds to 4.0 in double
    d0, d1 = t[0]
    t.append((float(np.nextafter(F32(d0), F32(0))), d1))
    t.append((float(np.nextafter(F32(d0), F32(1e9))), d1))
    return t


def ratio_expect(kp0, kp1, idx, dist, nq, ratio):
    """initial_feature_matching's two lines (VOPL:218-245) on one problem, in Python doubles: the
    matches m.distance < ratio * n.distance in query order, p0 = kp0[queryIdx].pt, p1 =
    kp1[trainIdx].pt.  A row without two matches (an index of -1) is no (m, n) pair: dropped."""
    p0, p1 = [], []
    for i in range(nq):
        if idx[i, 0] < 0 or idx[i, 1] < 0:
            continue
        if float(dist[i, 0]) < ratio * float(dist[i, 1]):
            p0.append(kp0[i, :2])
            p1.append(kp1[idx[i, 0], :2])
    return np.array(p0, F32).reshape(-1, 2), np.array(p1, F32).reshape(-1, 2)


# ====================================================================== batched C-ABI wrappers (GPU)
def _p(t):
    return C.c_void_p(t.data_ptr())


def _dev_opts(iters=100, err=8.0, conf=0.99):
    from monocular_visual_odometry_va4mr_amd import cv2compat as G
    from monocular_visual_odometry_va4mr_amd.engine import make_opts
    return make_opts(K_(), dict(G._DEFAULT_OPTS, PnP_conf=float(conf), PnP_error=float(err),
                                PnP_iterations=int(iters)))


def _pack(arrays, cap, width, dtype, fill):
    """[B][cap][width] with problem b's rows first and the sentinel after them"""
    out = np.full((len(arrays), cap, width), fill, dtype)
    for b, a in enumerate(arrays):
        assert len(a) <= cap
        out[b, :len(a)] = a
    return out


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def gpu_pnp(problems, iters, err, conf, cap):
    """vo_pnp_ransac on B problems [(obj, img)] in one launch, scratch at exactly the documented
    minimum (work_stride = 12 cap + 64) with one guard stride after the last chain.  Returns per
    problem dict(success, n_inl, mask [cap], rvec, tvec) and asserts the guard is untouched."""
    import torch
    from monocular_visual_odometry_va4mr_amd import _lib as L
    B = len(problems)
    dev = torch.device("cuda")
    o = _dev_opts(iters, err, conf)
    obj = torch.from_numpy(_pack([p[0] for p in problems], cap, 3, F32, 0)).to(dev)
    img = torch.from_numpy(_pack([p[1] for p in problems], cap, 2, F32, 0)).to(dev)
    cnt = torch.tensor([len(p[0]) for p in problems], dtype=torch.int32, device=dev)
    rv = torch.full((B, 3), SENT_F64, dtype=torch.float64, device=dev)
    tv = torch.full((B, 3), SENT_F64, dtype=torch.float64, device=dev)
    ok = torch.full((B,), SENT_I32, dtype=torch.int32, device=dev)
    ninl = torch.full((B,), SENT_I32, dtype=torch.int32, device=dev)
    mask = torch.full((B, cap), SENT_U8, dtype=torch.uint8, device=dev)
    ws = 12 * cap + 64
    work = torch.full((B + 1, ws), SENT_F64, dtype=torch.float64, device=dev)
    L.check(L.lib().vo_pnp_ransac(C.byref(o), B, _p(obj), _p(img), _p(cnt), cap, _p(rv), _p(tv), _p(ok), _p(mask),
                                  _p(ninl), _p(work), ws, _stream()), "vo_pnp_ransac")
    torch.cuda.synchronize()
    assert (work[B] == SENT_F64).all(), "scratch written past the last chain's share"
    rv, tv, ok, ninl, mask = (t.cpu().numpy() for t in (rv, tv, ok, ninl, mask))
    return [dict(success=int(ok[b]), n_inl=int(ninl[b]), mask=mask[b], rvec=rv[b], tvec=tv[b]) for b in range(B)]


def gpu_essential(problems, prob, thr, max_iters, cap):
    """vo_find_essential on B problems [(p0, p1)], scratch at exactly 4 cap + 90 * 64 doubles per
    chain plus one guard share.  Per problem dict(ok, E [9], mask [cap])."""
    import torch
    from monocular_visual_odometry_va4mr_amd import _lib as L
    B = len(problems)
    dev = torch.device("cuda")
    o = _dev_opts()
    p0 = torch.from_numpy(_pack([p[0] for p in problems], cap, 2, F32, 0)).to(dev)
    p1 = torch.from_numpy(_pack([p[1] for p in problems], cap, 2, F32, 0)).to(dev)
    cnt = torch.tensor([len(p[0]) for p in problems], dtype=torch.int32, device=dev)
    E = torch.full((B, 9), SENT_F64, dtype=torch.float64, device=dev)
    ok = torch.full((B,), SENT_I32, dtype=torch.int32, device=dev)
    mask = torch.full((B, cap), SENT_U8, dtype=torch.uint8, device=dev)
    ws = 4 * cap + 90 * 64
    work = torch.full((B + 1, ws), SENT_F64, dtype=torch.float64, device=dev)
    L.check(L.lib().vo_find_essential(C.byref(o), B, _p(p0), _p(p1), _p(cnt), cap, float(prob), float(thr),
                                      int(max_iters), _p(E), _p(mask), _p(ok), _p(work), ws, _stream()),
            "vo_find_essential")
    torch.cuda.synchronize()
    assert (work[B] == SENT_F64).all(), "scratch written past the last chain's share"
    E, ok, mask = (t.cpu().numpy() for t in (E, ok, mask))
    return [dict(ok=int(ok[b]), E=E[b], mask=mask[b]) for b in range(B)]


def gpu_recover(problems, cap, with_mask):
    """vo_recover_pose on B problems [(E, p0, p1)].  Per problem dict(n_good, R, t, mask [cap] or None)."""
    import torch
    from monocular_visual_odometry_va4mr_amd import _lib as L
    B = len(problems)
    dev = torch.device("cuda")
    o = _dev_opts()
    E = torch.from_numpy(np.stack([np.asarray(p[0], np.float64).reshape(9) for p in problems])).to(dev)
    p0 = torch.from_numpy(_pack([p[1] for p in problems], cap, 2, F32, 0)).to(dev)
    p1 = torch.from_numpy(_pack([p[2] for p in problems], cap, 2, F32, 0)).to(dev)
    cnt = torch.tensor([len(p[1]) for p in problems], dtype=torch.int32, device=dev)
    R = torch.full((B, 9), SENT_F64, dtype=torch.float64, device=dev)
    t = torch.full((B, 3), SENT_F64, dtype=torch.float64, device=dev)
    ng = torch.full((B,), SENT_I32, dtype=torch.int32, device=dev)
    mask = torch.full((B, cap), SENT_U8, dtype=torch.uint8, device=dev) if with_mask else None
    L.check(L.lib().vo_recover_pose(C.byref(o), B, _p(E), _p(p0), _p(p1), _p(cnt), cap, _p(R), _p(t),
                                    _p(mask) if with_mask else None, _p(ng), _stream()), "vo_recover_pose")
    torch.cuda.synchronize()
    R, t, ng = (x.cpu().numpy() for x in (R, t, ng))
    mk = mask.cpu().numpy() if with_mask else None
    return [dict(n_good=int(ng[b]), R=R[b], t=t[b], mask=mk[b] if with_mask else None) for b in range(B)]


def gpu_triangulate(P1, P2, x1, x2):
    """vo_triangulate_points on n rows; the output has one guard row.  [n][4] f32."""
    import torch
    from monocular_visual_odometry_va4mr_amd import _lib as L
    n = len(x1)
    dev = torch.device("cuda")
    a, b, c, d = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (P1, P2, x1, x2))
    out = torch.full((n + 1, 4), float(SENT_F32), dtype=torch.float32, device=dev)
    L.check(L.lib().vo_triangulate_points(n, _p(a), _p(b), _p(c), _p(d), _p(out), _stream()), "vo_triangulate_points")
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[n] == SENT_F32).all(), "row n written"
    return out[:n]


def gpu_rodrigues(batch):
    """vo_rodrigues on [n][3] (to matrices) or [n][3][3] (to vectors); one guard row."""
    import torch
    from monocular_visual_odometry_va4mr_amd import _lib as L
    n = len(batch)
    to_matrix = batch.shape[1:] == (3,)
    dev = torch.device("cuda")
    inp = torch.from_numpy(np.ascontiguousarray(batch.reshape(n, -1))).to(dev)
    out = torch.full((n + 1, 9 if to_matrix else 3), SENT_F64, dtype=torch.float64, device=dev)
    L.check(L.lib().vo_rodrigues(n, int(to_matrix), _p(inp), _p(out), _stream()), "vo_rodrigues")
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[n] == SENT_F64).all(), "row n written"
    return out[:n]


def gpu_ratio(kp0, kp1, idx, dist, nq, ratio, cap):
    """vo_ratio_matches on B problems.  (pts0 [B][cap][2], pts1, counts [B]), outputs pre-filled."""
    import torch
    from monocular_visual_odometry_va4mr_amd import _lib as L
    B = len(nq)
    dev = torch.device("cuda")
    a, b, c, d = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (kp0, kp1, idx, dist))
    n = torch.tensor(list(nq), dtype=torch.int32, device=dev)
    pts0 = torch.full((B, cap, 2), float(SENT_F32), dtype=torch.float32, device=dev)
    pts1 = torch.full((B, cap, 2), float(SENT_F32), dtype=torch.float32, device=dev)
    cnt = torch.full((B,), SENT_I32, dtype=torch.int32, device=dev)
    L.check(L.lib().vo_ratio_matches(B, _p(a), _p(b), kp0.shape[1], _p(c), _p(d), _p(n), idx.shape[1], float(ratio),
                                     _p(pts0), _p(pts1), _p(cnt), cap, _stream()), "vo_ratio_matches")
    torch.cuda.synchronize()
    return pts0.cpu().numpy(), pts1.cpu().numpy(), cnt.cpu().numpy()


# ====================================================================== chain states (oracle pipeline)
_CHAIN_BASE = {}


def chain_base():
    """The golden case parking_c1 on the oracle, computed once per process: the ratio-test matches of
    its bootstrap pair, and the states after initialization (S0), one step (S1) and two steps (S2)."""
    if not _CHAIN_BASE:
        import copy
        from conftest import golden_frames, load_golden
        from oracle import vo_pipeline_oracle as V
        from monocular_visual_odometry_va4mr_amd import options as Op
        g = load_golden("parking_c1")
        fr = golden_frames(g)
        opts, boot, _ = Op.get(str(g["preset"]))
        m = V.new_state(g["K"], opts)
        V.bootstrap_matches(m, fr[boot[0]], fr[boot[1]])
        p0, p1 = m.cand_first.copy(), m.cand.copy()
        s = V.new_state(g["K"], opts)
        V.initialize_from_matches(s, p0, p1, fr[boot[1]])
        S = [copy.deepcopy(s)]
        for k in range(2):
            V.step(s, fr[boot[1] + 1 + k])
            S.append(copy.deepcopy(s))
        _CHAIN_BASE.update(g=g, fr=fr, opts=opts, boot=boot, K=g["K"], p0=p0, p1=p1, S=S, next=boot[1] + 3)
    return _CHAIN_BASE


_BOOT_BASE = {}


def boot_base():
    """The ratio-test matches of the golden case malaga_c3's bootstrap pair (163: more than the 64 a
    chain of test_bootstrap_statuses_from_given_matches takes), computed once per process."""
    if not _BOOT_BASE:
        from conftest import golden_frames, load_golden
        from oracle import vo_pipeline_oracle as V
        from monocular_visual_odometry_va4mr_amd import options as Op
        g = load_golden("malaga_c3")
        fr = golden_frames(g)
        opts, boot, _ = Op.get(str(g["preset"]))
        m = V.new_state(g["K"], opts)
        V.bootstrap_matches(m, fr[boot[0]], fr[boot[1]])
        _BOOT_BASE.update(g=g, opts=opts, K=g["K"], img1=fr[boot[1]], p0=m.cand_first.copy(), p1=m.cand.copy())
    return _BOOT_BASE


BOOT_TAKES = (0, 3, 5, 6, 64)        # then all matches


def pnp_subset_redraws(n, iters):
    """The oracle's getSubset replayed for the first `iters` hypotheses over n points (the generator
    starts at ~0 and nothing else draws from it): how many draws repeated an index of their
    hypothesis and were drawn again -- the work of the serial tail of pnp_subsets."""
    from oracle import _olib as O
    rng = C.c_uint64(0xFFFFFFFFFFFFFFFF)
    redraws = 0
    for _ in range(iters):
        idx = []
        while len(idx) < 4:
            v = O.lib().vo_o_rng_next(C.byref(rng)) % n
            if v in idx:
                redraws += 1
            else:
                idx.append(v)
    return redraws


# chain -> (variant of S2, what the oracle does on the next frames); test_geom_cases_ref.py checks it
CHAIN_TABLE = {
    0: ("unchanged", None),
    1: ("first 7 landmarks", (0, ValueError, "Not enough keypoints")),
    2: ("first 10 landmarks, three keypoints off the image", (0, ValueError, "Not enough keypoints")),
    3: ("first 12 landmarks, 3-D rows rolled by one", (0, ValueError, "PnP failed")),
    4: ("all landmarks rolled by one", (1, ValueError, "Not enough keypoints")),
    5: ("unchanged", None),
    6: ("no candidate", None),
    7: ("one candidate", None),
    8: ("two candidates", None),
}
GFTT_TABLE = {
    "one": ({"feature_min_dist": 5000}, IndexError),
    "none": ({"feature_quality_level": 1.5}, AttributeError),
}


def chain_variant(s, v):
    import copy
    c = copy.deepcopy(s)
    if v == 1:
        c.lm, c.kp = c.lm[:7], c.kp[:7]
    elif v == 2:
        c.lm, c.kp = c.lm[:10].copy(), c.kp[:10].copy()
        c.kp[:3] = F32([[-50, -50], [700, 500], [-20, 240]])
    elif v == 3:
        c.lm, c.kp = np.roll(c.lm[:12], 1, axis=0), c.kp[:12]
    elif v == 4:
        c.lm = np.roll(c.lm, 1, axis=0)
    elif v in (6, 7, 8):
        chain_cut_candidates(c, v - 6)
    return c


def chain_cut_candidates(c, k):
    c.cand, c.cand_first, c.cand_tau = c.cand[:k], c.cand_first[:k], c.cand_tau[:k]
    return c


def chain_snapshot(s):
    return dict(landmarks=np.array(s.lm, F32).reshape(-1, 3), keypoints=np.array(s.kp, F32).reshape(-1, 2),
                cand=np.array(s.cand, F32).reshape(-1, 2), cand_first=np.array(s.cand_first, F32).reshape(-1, 2),
                cand_tau=np.array(s.cand_tau, np.float64).reshape(-1, 1),
                inliers=None if s.inl_pts is None else np.array(s.inl_pts), outliers=None if s.outl_pts is None else np.array(s.outl_pts),
                transforms=[(R.copy(), t.copy()) for R, t in s.transforms], num_pts=[int(v) for v in s.num_pts])


def chain_run(c, frames):
    """Step the oracle chain c over frames.  One record per frame: ("ok", snapshot after the step), or
    ("raise", exception, snapshot at the raise) for the step that raises and every one after it (a
    stopped chain stays where it was: the reference raises before transforms.append)."""
    from oracle import vo_pipeline_oracle as V
    out = []
    for f in frames:
        if out and out[-1][0] == "raise":
            out.append(out[-1])
            continue
        try:
            V.step(c, f)
            out.append(("ok", chain_snapshot(c)))
        except (ValueError, IndexError, AttributeError) as e:
            out.append(("raise", e, chain_snapshot(c)))
    return out
