"""CPU ORACLE restatement of the reference VO orchestration (test infrastructure only).

Restates /root/reference/VisualOdometryPipeLine.py (class at :4-373) as a small state
record plus free functions, calling the C oracle primitives through ``cv2_oracle``.
Every numpy expression keeps the reference's operand order so results are bit-for-bit
those of the reference class driven by the same primitives; tests/golden pins that.

It is used (a) by tests as the CPU model of the whole per-frame step and (b) by
bench.py's ``cpu_baseline`` leg ("port" baseline) on the GPU box, where the reference
itself is not available.  The product (monocular_visual_odometry_va4mr_amd) never
imports it.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import cv2_oracle as cv


@dataclass
class OracleState:
    """Fields mirror the reference attributes (VisualOdometryPipeLine.py:33-59)."""
    K: np.ndarray
    opts: dict
    K_inv: np.ndarray = None
    transforms: list = field(default_factory=list)       # [(R_CW f64 3x3, t_CW f64 3x1)]
    num_pts: list = field(default_factory=list)
    lm: object = field(default_factory=list)             # matched_landmarks f32 (N,3)
    kp: object = field(default_factory=list)             # matched_keypoints f32 (N,2)
    cand: object = field(default_factory=list)           # potential_keys f32 (P,2)
    cand_first: object = field(default_factory=list)     # potential_first_keys f32 (P,2)
    cand_tau: object = field(default_factory=list)       # potential_transforms f64 (P,1)
    cand_desc: object = field(default_factory=list)      # potential_descriptors (dead state, Q6)
    prev_img: np.ndarray = None                          # potential_frame
    inl_pts: np.ndarray = None
    outl_pts: np.ndarray = None
    ring: list = field(default_factory=list)             # num_tracked_landmarks_list


def new_state(K, opts) -> OracleState:
    s = OracleState(K=K, opts=opts)
    s.K_inv = np.linalg.inv(K)                                         # :38
    s.transforms.append((np.eye(3), np.zeros((3, 1))))                 # :43-45
    return s


def _inv_rigid(R, t):
    """:62-77 -- (R^T, -R^T t)."""
    Ri = R.T
    return Ri, -Ri @ t


def _keep_cands(s: OracleState, keep):
    """filter_potential :80-92 (descriptors only while lengths agree, quirk Q6)."""
    s.cand = s.cand[keep, :]
    s.cand_first = s.cand_first[keep, :]
    s.cand_tau = s.cand_tau[keep, :]
    if s.cand_desc.shape[0] == keep.shape[0]:
        s.cand_desc = s.cand_desc[keep, :]


def _keep_landmarks(s: OracleState, keep):
    """filter_landmarks :95-104."""
    s.lm = s.lm[keep, :]
    s.kp = s.kp[keep, :]


def _too_small_angle(s: OracleState, u_first, u_cur, R_past, R_cur) -> bool:
    """check_baseline :117-147 (with the (R_cur^T R_past)^T rotation, quirk Q3)."""
    v_cur = np.hstack((u_cur, [1])).reshape(3, 1)
    v_past = np.hstack((u_first, [1])).reshape(3, 1)
    v_cur = s.K_inv @ v_cur
    rel = (R_cur.T @ R_past).T
    v_past = np.matmul(rel, s.K_inv) @ v_past
    c = np.sum(v_cur.T * v_past.T, axis=1) / (np.linalg.norm(v_cur, axis=0) * np.linalg.norm(v_past, axis=0))
    c = np.clip(c, -1.0, 1.0)
    return np.degrees(np.arccos(c)) < s.opts['min_baseline_angle']


def _depth_ok(s: OracleState, R_cur_WC, t_cur_WC, R_past_WC, t_past_WC, X) -> bool:
    """disambguate_landmark :149-168."""
    z_c = (R_cur_WC @ X + t_cur_WC)[2]
    z_p = (R_past_WC @ X + t_past_WC)[2]
    lo, hi = s.opts['min_dist_landmarks'], s.opts['max_dist_landmarks']
    return z_c > lo and z_p > lo and z_c < hi and z_p < hi


def triangulate_candidates(s: OracleState, R_cur_CW, t_cur_CW):
    """triangulate_landmarks :107-206."""
    R_cur_WC, t_cur_WC = _inv_rigid(R_cur_CW, t_cur_CW)
    P_cur = s.K @ np.hstack((R_cur_WC, t_cur_WC))
    retain = np.zeros((s.cand.shape[0],), dtype=bool)
    n_poses = len(s.transforms)
    for i in range(s.cand.shape[0]):
        if n_poses > 1 and n_poses - s.cand_tau[i] <= s.opts['min_baseline_frames']:   # :175-178
            retain[i] = True
            continue
        R_past_CW, t_past_CW = s.transforms[int(s.cand_tau[i, 0])]
        if _too_small_angle(s, s.cand_first[i, :], s.cand[i, :], R_past_CW, R_cur_CW):
            retain[i] = True
            continue
        R_past_WC, t_past_WC = _inv_rigid(R_past_CW, t_past_CW)
        X = cv.triangulatePoints(s.K @ np.hstack((R_past_WC, t_past_WC)), P_cur,
                                 s.cand_first[i].reshape(-1, 1), s.cand[i].reshape(-1, 1))
        X = X[:3] / X[3]
        if _depth_ok(s, R_cur_WC, t_cur_WC, R_past_WC, t_past_WC, X):
            if len(s.lm) == 0:
                s.lm = X.T
                s.kp = s.cand[i].reshape(1, 2)
            else:
                s.lm = np.append(s.lm, X.T, axis=0)
                s.kp = np.append(s.kp, s.cand[i].reshape(1, 2), axis=0)
        else:
            retain[i] = True                                             # quirk Q5
    _keep_cands(s, retain)


def bootstrap_matches(s: OracleState, img0, img1):
    """initial_feature_matching :209-245 (``sift_nfeatures``: the C5 benchmark's capped SIFT;
    absent from the reference's option dicts, where SIFT_create() keeps every keypoint)."""
    sift = cv.SIFT_create(int(s.opts.get('sift_nfeatures', 0)))
    k0, d0 = sift.detectAndCompute(img0, None)
    k1, d1 = sift.detectAndCompute(img1, None)
    pairs = cv.BFMatcher().knnMatch(d0, d1, k=2)
    good = [m for m, n in pairs if m.distance < s.opts['feature_ratio'] * n.distance]
    p0 = np.float32([k0[m.queryIdx].pt for m in good]).reshape(-1, 2)
    p1 = np.float32([k1[m.trainIdx].pt for m in good]).reshape(-1, 2)
    if len(good) > 0:
        tau = np.ones((len(p1), 1)) * (len(s.transforms) - 1)
        desc = np.float32([d1[m.trainIdx] for m in good])
        if s.prev_img is None:
            s.cand, s.cand_first, s.cand_desc, s.cand_tau = p1, p0, desc, tau
        else:
            s.cand = np.append(s.cand, p1, axis=0)
            s.cand_first = np.append(s.cand_first, p0, axis=0)
            s.cand_desc = np.append(s.cand_desc, desc, axis=0)
            s.cand_tau = np.append(s.cand_tau, tau, axis=0)


def add_corners(s: OracleState, img):
    """feature_adding :248-268 (distance filter against candidates only, quirk Q4)."""
    o = s.opts
    pts = cv.goodFeaturesToTrack(img, maxCorners=o['feature_max_corners'], qualityLevel=o['feature_quality_level'],
                                 minDistance=o['feature_min_dist'], blockSize=o['feature_block_size'],
                                 useHarrisDetector=o['feature_use_harris'], mask=None).squeeze()
    far = np.array([np.all(np.linalg.norm(pts[i, :] - s.cand, axis=1) > o['feature_min_dist'])
                    for i in range(pts.shape[0])])
    pts = pts[far]
    tau = np.ones((len(pts), 1)) * len(s.transforms)
    if s.cand.shape[0] == 0:
        s.cand, s.cand_first, s.cand_tau = pts, pts, tau
    else:
        s.cand = np.append(s.cand, pts, axis=0)
        s.cand_first = np.append(s.cand_first, pts, axis=0)
        s.cand_tau = np.append(s.cand_tau, tau, axis=0)


def track(s: OracleState, img):
    """feature_tracking :271-290 (two LK calls, quirk Q8; candidates only if P > 1, Q7)."""
    o = s.opts
    kw = dict(winSize=o['winSize'], maxLevel=o['maxLevel'], criteria=o['criteria'])
    nxt, st, _ = cv.calcOpticalFlowPyrLK(s.prev_img, img, s.kp, None, **kw)
    ok = (st == 1).squeeze()
    s.kp = nxt[ok]
    s.lm = s.lm[ok]
    if s.cand.shape[0] > 1:
        nxt, st, _ = cv.calcOpticalFlowPyrLK(s.prev_img, img, s.cand, None, **kw)
        ok = (st == 1).squeeze()
        s.cand = nxt
        _keep_cands(s, ok)


def initialize(s: OracleState, img0, img1):
    """initialization :293-323."""
    bootstrap_matches(s, img0, img1)
    E, m = cv.findEssentialMat(s.cand_first, s.cand, s.K, method=cv.RANSAC, prob=0.99, threshold=1)
    inl = m.ravel() == 1
    s.outl_pts = s.cand[~inl]
    s.inl_pts = s.cand[inl]
    _keep_cands(s, inl)
    _, R, t, _ = cv.recoverPose(E, s.cand_first, s.cand, s.K)
    t *= np.sign(t[2])                                                  # quirk Q2
    triangulate_candidates(s, R, t)
    s.transforms.append((R, t))
    s.num_pts = [sum(inl)]
    s.prev_img = img1


def initialize_from_matches(s: OracleState, p0, p1, img1):
    """initialization :293-323 from given bootstrap matches (p0, p1 float32 (n, 2), what
    initial_feature_matching gathers from the ratio test) instead of SIFT + knnMatch: the statements
    of bootstrap_matches after the match list (a fresh state, potential_frame None; the dead
    descriptor state of quirk Q6 is not kept) followed by the rest of initialize, unchanged.  As in
    the reference, no matches leave the candidate lists empty, and too few for an essential matrix
    make recoverPose raise: the two cases the engine reports as VO_ST_NO_MATCHES and
    VO_ST_ESSENTIAL_FAILED."""
    p0 = np.float32(p0).reshape(-1, 2)
    p1 = np.float32(p1).reshape(-1, 2)
    if len(p0) > 0:
        s.cand, s.cand_first = p1, p0
        s.cand_tau = np.ones((len(p1), 1)) * (len(s.transforms) - 1)
        s.cand_desc = np.zeros((len(p1), 0), np.float32)
    E, m = cv.findEssentialMat(s.cand_first, s.cand, s.K, method=cv.RANSAC, prob=0.99, threshold=1)
    inl = m.ravel() == 1
    s.outl_pts = s.cand[~inl]
    s.inl_pts = s.cand[inl]
    _keep_cands(s, inl)
    _, R, t, _ = cv.recoverPose(E, s.cand_first, s.cand, s.K)
    t *= np.sign(t[2])                                                  # quirk Q2
    triangulate_candidates(s, R, t)
    s.transforms.append((R, t))
    s.num_pts = [sum(inl)]
    s.prev_img = img1


def step(s: OracleState, img):
    """continuous_operation :326-373."""
    track(s, img)
    if len(s.kp) < 8:
        raise ValueError("Not enough keypoints for PnP")                # :358
    o = s.opts
    ok, rv, t_WC, inl = cv.solvePnPRansac(s.lm, s.kp, s.K, np.zeros(4), flags=cv.SOLVEPNP_P3P,
                                          confidence=o['PnP_conf'], reprojectionError=o['PnP_error'],
                                          iterationsCount=o['PnP_iterations'])
    if not ok:
        raise ValueError("PnP failed")                                  # :352
    keep = np.isin(np.arange(len(s.lm)), inl.squeeze()).astype(bool)
    s.outl_pts = s.kp[~keep]
    s.inl_pts = s.kp[keep]
    _keep_landmarks(s, keep)
    R_WC = cv.Rodrigues(rv)[0]
    R_CW, t_CW = _inv_rigid(R_WC, t_WC)
    if len(s.ring) == 20:                                               # :360-364 (unused by main)
        s.ring.pop(0)
    s.ring.append(len(s.inl_pts))
    if s.cand.shape[0] > 1:
        triangulate_candidates(s, R_CW, t_CW)
    add_corners(s, img)
    s.transforms.append((R_CW, t_CW))
    s.num_pts.append(len(inl))
    s.prev_img = img
