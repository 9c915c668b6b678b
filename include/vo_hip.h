/*
 * vo_hip.h -- C ABI of libvo_hip.so, the MI355X (gfx950) VO hot path.
 *
 * Drop-in boundary.  The reference has no FFI: its hot path sits behind
 * (B1) nine cv2 calls made by /root/reference/VisualOdometryPipeLine.py and (B2) the
 * VisualOdometryPipeLine class itself.  Each entry point below names the reference
 * call it replaces.  The library never allocates on a call path: every buffer is a
 * caller-owned device pointer (PyTorch tensors are used purely as containers), every
 * call is asynchronous on the given HIP stream, returns an int status (0 = OK,
 * VO_E* < 0 on bad arguments / HIP launch errors) and leaves per-chain runtime
 * outcomes (the reference's ValueError conditions) in the device status word.
 *
 * Batching: B independent VO chains ("shards") are processed per call.  State arrays
 * are [B][capacity] with per-chain device counts, so a whole per-frame step is a fixed
 * sequence of launches with no host synchronisation (hipGraph-capturable).
 */
#ifndef VO_HIP_H
#define VO_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vo_stream_t; /* hipStream_t */

enum vo_err {
    VO_OK = 0,
    VO_EARG = -1,
    VO_EHIP = -2,
};

/* per-chain runtime status (device int32), set by the stage that detects it */
enum vo_chain_status {
    VO_ST_OK = 0,
    VO_ST_NOT_ENOUGH_KP = 1,   /* VisualOdometryPipeLine.py:357-358 ValueError      */
    VO_ST_PNP_FAILED = 2,      /* VisualOdometryPipeLine.py:351-352 ValueError      */
    VO_ST_GFTT_NONE = 3,       /* :256 goodFeaturesToTrack returned None -> crash  */
    VO_ST_GFTT_ONE = 4,        /* :256-258 single corner -> squeeze() breaks index */
    VO_ST_CAPACITY = 5,        /* a fixed capacity of this engine was exceeded     */
    VO_ST_ESSENTIAL_FAILED = 6,/* :308 findEssentialMat produced no model          */
    VO_ST_NO_MATCHES = 7,      /* :209-245 no bootstrap matches                    */
};

#define VO_MAX_LEVELS 8
#define VO_BORDER 16

/* Geometry of the per-chain image pyramid: u8 images with a VO_BORDER reflect-101 border;
 * derivative images as interleaved int16 (dx, dy) pairs with a zero border: the pixel at
 * pyramid byte offset o has dx at der[2o] and dy at der[2o + 1] (one dword per pixel).
 * The engine gives every level the pitch of level 0 (the LK kernel relies on it for
 * scalar row offsets; other pitches select the per-level LK kernels). */
typedef struct vo_dims {
    int32_t B, W, H;
    int32_t nlev;                 /* levels kept (maxLevel + 1 after the winSize cap)   */
    int32_t lvl_w[VO_MAX_LEVELS], lvl_h[VO_MAX_LEVELS], lvl_pitch[VO_MAX_LEVELS];
    int64_t lvl_off[VO_MAX_LEVELS];  /* byte offset of level l (padded origin)         */
    int64_t pyr_stride;           /* bytes per chain, u8 pyramid                          */
    int64_t der_stride;           /* int16 elements per chain (>= 2*pyr_stride): (dx, dy) */
    int32_t ncap, pcap, fcap;     /* landmark, candidate, pose capacities per chain       */
    int32_t ccap;                 /* GFTT local-maximum candidates per chain              */
    int32_t mcap;                 /* GFTT output corners per chain                        */
    int64_t work_stride;          /* fp64 scratch per chain (>= 16*max(ncap,pcap)+4096)   */
    int64_t iwork_stride;         /* int32 scratch per chain (>= 2*max(ncap,pcap)+4096)   */
} vo_dims;

/* Reference options (main.py:20-44 keys) plus host-derived constants. */
typedef struct vo_opts {
    double K[9], K_inv[9];
    double min_dist_landmarks, max_dist_landmarks;
    double min_baseline_angle;    /* degrees                                            */
    double cos_baseline;          /* smallest c with degrees(arccos(c)) < min_baseline_angle
                                     under the host's numpy (exact gate, :144-147); 2 = never */
    int32_t min_baseline_frames;
    double feature_ratio;
    int32_t feature_max_corners;
    double feature_quality_level, feature_min_dist;
    int32_t feature_block_size, feature_use_harris;
    double harris_k;
    int32_t win_w, win_h, max_level, crit_type, crit_count;
    double crit_eps;              /* raw epsilon (squared inside, as OpenCV)             */
    double min_eig;
    double pnp_conf, pnp_error;
    int32_t pnp_iters;
} vo_opts;

/* Device state of B chains; every pointer is [B][...] contiguous per chain. */
typedef struct vo_state {
    uint8_t* pyr[2];              /* ping-pong image pyramids  [B][pyr_stride]          */
    int16_t* der[2];              /* Scharr of pyr[0] / pyr[1]    [B][der_stride]       */
    float* lm_X;                  /* matched_landmarks  [B][ncap][3]                     */
    float* lm_kp;                 /* matched_keypoints  [B][ncap][2]                     */
    int32_t* nL;                  /* [B]                                                 */
    float* c_kp;                  /* potential_keys       [B][pcap][2]                   */
    float* c_first;               /* potential_first_keys [B][pcap][2]                   */
    int32_t* c_tau;               /* potential_transforms [B][pcap]                      */
    int32_t* nC;                  /* [B]                                                 */
    double* pose_R;               /* transforms (R_CW)  [B][fcap][9]                     */
    double* pose_t;               /* transforms (t_CW)  [B][fcap][3]                     */
    int32_t* nF;                  /* len(transforms) [B]                                 */
    int32_t* num_pts;             /* [B][fcap]                                           */
    float* outl_kp;               /* outlier_pts_current [B][max(ncap,pcap)][2]          */
    float* inl_kp;                /* inlier_pts_current  [B][max(ncap,pcap)][2]          */
    int32_t* nOutl;               /* [B]                                                 */
    int32_t* nInl;                /* len(inlier_pts_current) [B]                         */
    int32_t* status;              /* enum vo_chain_status [B]                            */
    /* scratch */
    float* trk_pts;               /* LK outputs [B][ncap+pcap][2]                        */
    uint8_t* trk_st;              /* LK status  [B][ncap+pcap]                           */
    float* trk_err;               /* LK err     [B][ncap+pcap]; written by vo_track_fb only
                                     (vo_track / vo_track_lk leave it untouched)          */
    float* eig;                   /* GFTT eigen map [B][W*H]                              */
    uint32_t* eig_max;            /* [B] order-preserving float bits                      */
    uint64_t* gf_keys;            /* [B][ccap]                                            */
    int32_t* gf_n;                /* [B]                                                  */
    float* corners;               /* [B][mcap][2]                                         */
    int32_t* nCorners;            /* [B]                                                  */
    double* pnp_rt;               /* PnP rvec,tvec [B][6]                                 */
    int32_t* pnp_ok;              /* PnP success [B]                                      */
    int32_t* pnp_ninl;            /* PnP inlier count [B]                                 */
    uint8_t* pnp_mask;            /* PnP inlier mask [B][ncap]                            */
    double* work;                 /* per-chain fp64 scratch [B][work_stride]              */
    int32_t* iwork;               /* per-chain int scratch  [B][iwork_stride]             */
    uint64_t* gf_sort;            /* GFTT selection scratch [B][ccap + VO_GF_SORT_EXTRA], zeroed
                                     at allocation (the split selection leaves it zeroed); NULL
                                     selects the one-block k_gftt_select                      */
} vo_state;

#define VO_GF_SORT_EXTRA 4096     /* u64 after the sorted keys: value histogram + counter   */

/* ---- library ---------------------------------------------------------------- */
const char* vo_version(void);
int vo_device_arch(char* buf, int len);          /* gcnArchName of the current device */
int vo_device_cus(void);                          /* compute units of the current device (or < 0) */
/* Launch-shape threshold: several entry points pick their kernel form by comparing the chain
 * count B with the device's compute units (vo_essential / vo_bootstrap / vo_triangulate /
 * vo_pnp / vo_pnp_triangulate: one block per chain at or above the CU count, split or
 * unconstrained forms below).  n > 0 makes those decisions assume n CUs (test hook: every form
 * on a small batch); n = 0 restores the device's own count.  Results never depend on it. */
int vo_set_launch_cus(int n);
/* Form of the GFTT corner selection inside vo_gftt (csrc/vo_select.hip: goodFeaturesToTrack's sort
 * + minDistance walk, VisualOdometryPipeLine.py:256): 0 = automatic (above 64 chains the split
 * one-wave kernels k_gsel_* where the configuration allows them, else k_gftt_select), 1 = always
 * the one-block k_gftt_select,
 * 2 = the split form where it applies.  Test / A-B hook; the corner lists are identical. */
int vo_set_gftt_select(int mode);
/* A HIP stream of the current device whose kernels may run on every compute unit except
 * `reserve` of them (every `stride`-th CU-mask bit from stride - 1, hipExtStreamCreateWithCUMask):
 * tracking on such a stream leaves those CUs to the one-block-per-chain latency kernels of the
 * other stream groups (measurement option of the sequence job, VO_TRACK_CU_RESERVE).  The caller
 * destroys it with vo_stream_destroy. */
int vo_stream_create_cumask(int reserve, int stride, vo_stream_t* out);
int vo_stream_destroy(vo_stream_t stream);

/* ---- per-frame step stages (replace VisualOdometryPipeLine.py:326-373) --------- */

/* Build the pyramid of the new frames into state->pyr[cur] and its Scharr derivatives into
 * state->der[cur] (buildOpticalFlowPyramid + calcSharrDeriv inside cv2.calcOpticalFlowPyrLK,
 * :281,287), one fused pass per level.  frames: [B][H][W] u8, frame_stride bytes between
 * chains.  The derivative buffers' zero border is never written (allocate them zeroed). */
int vo_pyr_build(const vo_dims* d, const vo_state* s, int cur, const uint8_t* frames,
                 int64_t frame_stride, vo_stream_t stream);
/* Scharr derivatives of pyramid `which` into state->der[which] (calcSharrDeriv), border
 * included; vo_pyr_build already produces them, this recomputes them alone. */
int vo_pyr_deriv(const vo_dims* d, const vo_state* s, int which, vo_stream_t stream);

/* feature_tracking (:271-290): LK of landmarks and (if P > 1) candidates from pyr[prev]
 * to pyr[1-prev], then the reference's status filtering (ordered compaction). */
int vo_track(const vo_dims* d, const vo_opts* o, const vo_state* s, int prev, vo_stream_t stream);

/* vo_track without the filtering: the calcOpticalFlowPyrLK calls (:281, :287) into the tracking
 * scratch (trk_pts, trk_st); vo_filter_pnp_triangulate then filters (:283-290) in its PnP block.
 * Neither this nor vo_track writes trk_err: nothing in the step reads it, so the L1-error pass is
 * not run (vo_track_fb still runs it and writes trk_err). */
int vo_track_lk(const vo_dims* d, const vo_opts* o, const vo_state* s, int prev, vo_stream_t stream);

/* PnP step (:338-358): guard N >= 8, cv2.solvePnPRansac(P3P) + EPnP refit, inlier
 * filtering, Rodrigues, inversion; writes pose slot nF (not yet counted). */
int vo_pnp(const vo_dims* d, const vo_opts* o, const vo_state* s, vo_stream_t stream);

/* triangulate_landmarks (:107-206) incl. cv2.triangulatePoints per candidate (:188),
 * using pose slot nF as the current pose.  Runs only where P > 1 (:366) unless force. */
int vo_triangulate(const vo_dims* d, const vo_opts* o, const vo_state* s, int force,
                   vo_stream_t stream);

/* vo_pnp followed by vo_triangulate(force = 0) as one launch, each chain's triangulation in the
 * block that solved its pose (the engine's step; same results as the two calls).  No reference
 * counterpart of its own: it replaces the pair VisualOdometryPipeLine.py:342-358 + :366-368. */
int vo_pnp_triangulate(const vo_dims* d, const vo_opts* o, const vo_state* s, vo_stream_t stream);

/* feature_tracking's status filtering (:283-290) after vo_track_lk, then vo_pnp_triangulate, in
 * one launch (the engine's step: one kernel boundary fewer between tracking and PnP). */
int vo_filter_pnp_triangulate(const vo_dims* d, const vo_opts* o, const vo_state* s, vo_stream_t stream);

/* cv2.goodFeaturesToTrack (:256) on pyramid level 0 of pyr[cur] -> state->corners. */
int vo_gftt(const vo_dims* d, const vo_opts* o, const vo_state* s, int cur, vo_stream_t stream);

/* vo_gftt with goodFeaturesToTrack's mask argument (OpenCV 4.6 featureselect.cpp; no reference
 * counterpart: the reference never passes one, :256).  mask: [B] images of H rows, u8, rows
 * mask_pitch bytes apart (mask_pitch >= W, else VO_EARG with nothing launched), chains mask_stride
 * bytes apart; a non-zero byte allows its pixel, any non-zero value counts.
 *   - the maximum that feature_quality_level scales is taken over the allowed pixels only
 *     (minMaxLoc(eig, ..., mask)), the allowed pixels of the image border included;
 *   - the 3x3 local-maximum test is vo_gftt's and looks at all eight neighbours whether they are
 *     allowed or not (dilate runs on the unmasked map): an allowed pixel beside a stronger
 *     masked-out pixel is no corner;
 *   - only an allowed interior pixel that passes that test becomes a corner candidate;
 *   - the sort, its tie order, the minDistance walk, feature_max_corners and the capacity flag are
 *     vo_gftt's.  A mask with no allowed pixel gives nCorners = 0.
 * mask == NULL is vo_gftt itself (the other two arguments are then ignored).  A chain whose status
 * is not 0 is skipped.  Both selection forms apply, chosen as in vo_gftt.  With a mask the eigen
 * pass evaluates every pixel exactly (vo_gftt's interval form finds the maximum among the local
 * maxima of the map, and the greatest allowed pixel need not be one).  Asynchronous, no host
 * synchronisation; the mask is only read.  Replay from a captured graph has not been verified for
 * masked calls. */
int vo_gftt_masked(const vo_dims* d, const vo_opts* o, const vo_state* s, int cur, const uint8_t* mask,
                   int64_t mask_stride, int32_t mask_pitch, vo_stream_t stream);

/* vo_corner_subpix on state->corners / nCorners after vo_gftt, reading level 0 of pyr[cur] (no
 * reference counterpart: the reference adds goodFeaturesToTrack's integer positions, :256-268;
 * engine option feature_subpix_win).  Same limits, VO_EARG with nothing launched outside them.  A
 * chain whose status is not 0 or whose nCorners is <= 0 is left alone, so the capacity flag (-1)
 * and the lists behind VO_ST_GFTT_NONE / VO_ST_GFTT_ONE reach vo_add_corners_finish unchanged.
 * Asynchronous and capturable like the other stages; call between vo_gftt and
 * vo_add_corners_finish on vo_gftt's stream. */
int vo_gftt_subpix(const vo_dims* d, const vo_state* s, int cur,
                   int32_t win_w, int32_t win_h, int32_t zero_w, int32_t zero_h,
                   int32_t max_iters, double eps, vo_stream_t stream);

/* Diagnostics: the cornerMinEigenVal / cornerHarris map goodFeaturesToTrack thresholds
 * (featureselect.cpp), written to state->eig ([B][W*H] f32) with its max in eig_max.
 * vo_gftt itself never stores this map. */
int vo_gftt_eigmap(const vo_dims* d, const vo_opts* o, const vo_state* s, int cur, vo_stream_t stream);

/* Diagnostics: the eigen pass of vo_gftt alone.  gf_keys [B][ccap] receives every local maximum
 * with v > 0 among the interior pixels as (fkey(v) << 32 | y * W + x), in no particular order,
 * gf_n their count per chain and eig_max the map's maximum (fkey form); no quality gate and no
 * selection runs, so the key set can be read before vo_gftt's selection consumes it. */
int vo_gftt_keys(const vo_dims* d, const vo_opts* o, const vo_state* s, int cur, vo_stream_t stream);

/* feature_adding distance filter + append (:258-268) and the pose/num_pts append
 * (:371-373).  Call after vo_gftt. */
int vo_add_corners_finish(const vo_dims* d, const vo_opts* o, const vo_state* s, vo_stream_t stream);

/* Chain 0's (status, inlier count) written by one kernel into dst[0..1], which may be pinned host
 * memory: what the drop-in class checks after every frame to raise the reference's ValueErrors
 * (:352, :358) and to append len(inlier_pts_current) (:360-364), without a gather + copy. */
int vo_status_word(const vo_state* s, int32_t* dst, vo_stream_t stream);

/* ---- single-call primitives for the cv2 surface (B1) --------------------------- */

/* cv2.calcOpticalFlowPyrLK (:281,287): points [B][n] with per-chain counts, using the
 * pyramids/derivatives already in state (prev = pyr[prev], next = pyr[1-prev]).  Windows
 * (vo_opts.win_w, win_h) of 3 to 32 pixels per side and at most 1024 pixels; anything else
 * returns VO_EARG with the outputs untouched (vo_track and vo_track_lk likewise). */
int vo_lk_points(const vo_dims* d, const vo_opts* o, const vo_state* s, int prev,
                 const float* pts, const int32_t* counts, int32_t cap, float* out_pts,
                 uint8_t* out_status, float* out_err, vo_stream_t stream);

/* cv2.calcOpticalFlowPyrLK's flags (OpenCV's values) */
#define VO_LK_USE_INITIAL_FLOW   4
#define VO_LK_GET_MIN_EIGENVALS  8

/* vo_lk_points with cv2's flags.  VO_LK_USE_INITIAL_FLOW: point i's estimate starts at
 * init[i] * 2^-L at the top level L instead of at pts[i] * 2^-L; init is [B][cap][2], read only with
 * that bit (else it may be NULL), and a distinct buffer from out_pts.  VO_LK_GET_MIN_EIGENVALS:
 * out_err receives the minimum eigenvalue of level 0's tensor (the value compared with
 * vo_opts.min_eig) wherever the level-0 window of pts[i] is in bounds, whatever the status, and
 * the L1 error pass does not run.  Any other flag bit, or bit 4 with init NULL: VO_EARG with the
 * outputs untouched.  flags = 0 is vo_lk_points. */
int vo_lk_points_ex(const vo_dims* d, const vo_opts* o, const vo_state* s, int prev,
                    const float* pts, const float* init, const int32_t* counts, int32_t cap,
                    int32_t flags, float* out_pts, uint8_t* out_status, float* out_err,
                    vo_stream_t stream);

/* vo_lk_points_ex followed by the forward-backward gate: every point tracked forward (status 1) is
 * tracked back from its result, next to prev, with flags 0 and the same window, levels, criteria
 * and min_eig, into back_pts [B][cap][2] (unspecified where the forward status is 0).  out_status
 * is 1 iff both passes succeeded and the point came back within fb_threshold pixels of pts[i]
 * ((double)dx * dx + (double)dy * dy <= fb_threshold^2 with float dx, dy); out_pts and out_err are
 * the forward pass's.  fb_threshold > 0 and finite, else VO_EARG with the outputs untouched. */
int vo_lk_points_fb(const vo_dims* d, const vo_opts* o, const vo_state* s, int prev,
                    const float* pts, const float* init, const int32_t* counts, int32_t cap,
                    int32_t flags, double fb_threshold, float* back_pts, float* out_pts,
                    uint8_t* out_status, float* out_err, vo_stream_t stream);

/* vo_track (compact = 1) or vo_track_lk (compact = 0) with the forward-backward gate applied to
 * trk_st before any filtering; scratch: [B][ncap + pcap][2] floats (the points tracked back). */
int vo_track_fb(const vo_dims* d, const vo_opts* o, const vo_state* s, int prev, double fb_threshold,
                float* scratch, int compact, vo_stream_t stream);

/* Constant-velocity seeds for the landmark tracks (engine option lk_motion_model; the project's own
 * definition, DESIGN 5h and the NumPy restatement tests/test_lk_seed_ref.py, reproduced bit for
 * bit).  No reference counterpart: the reference starts every search at the old pixel (nextPts =
 * None, :281).  With A = pose slot nF - 2 and B = pose slot nF - 1 (X_world = R X_cam + t), the next
 * pose is predicted as B (A^-1 B) and every landmark is projected through it with vo_opts.K, all in
 * fp64 with one rounding per operation.  The projection is the seed iff its depth is > 0, both
 * coordinates are finite and, as float32, inside [0, W) x [0, H); otherwise the seed is the
 * landmark's own lm_kp.  Candidates are never seeded.
 *   seeds: [B][ncap + pcap][2], laid out like trk_pts: rows [0, nL) the landmark seeds, rows
 * [nL, nL + nC) the candidates' own c_kp, rows past nL + nC not written.  A chain whose status is
 * not 0 writes nothing; a chain with status 0 and nF < 3 writes its own positions everywhere (with
 * nF == 2 the two poses are the identity and the bootstrap pose, which are not one frame apart).
 *   info: [B][4] int32 or NULL: landmarks seen, seeded, fallen back on the depth or a non-finite
 * value, fallen back on the image bounds (rows of chains whose status is not 0 are not written).
 * NULL d, o, s or seeds: VO_EARG with nothing launched.  Asynchronous, no host read-back,
 * capturable into a graph. */
int vo_predict_seeds(const vo_dims* d, const vo_opts* o, const vo_state* s, float* seeds, int32_t* info,
                     vo_stream_t stream);

/* Tracking with the forward pass started at seeds (VO_LK_USE_INITIAL_FLOW over the state's points;
 * seeds as vo_predict_seeds lays them out, read for every tracked row).  fb_threshold == 0: vo_track
 * (compact = 1) or vo_track_lk (compact = 0); fb_threshold > 0: vo_track_fb with that threshold and
 * fb_scratch as its scratch, the backward pass unseeded (flags 0) as vo_lk_points_fb defines it.
 * trk_err is not written in either case (the seeded step runs no L1-error pass).  NULL seeds, a
 * negative, NaN or infinite threshold, a positive threshold with NULL fb_scratch, or a window
 * outside vo_lk_points' sizes: VO_EARG with nothing written. */
int vo_track_seeded(const vo_dims* d, const vo_opts* o, const vo_state* s, int prev, const float* seeds,
                    double fb_threshold, float* fb_scratch, int compact, vo_stream_t stream);

/* Illumination models of the LK tracker (engine option lk_illumination; the project's own
 * definition, restated in NumPy in tests/test_lk_illum_ref.py and reproduced bit for bit).  No
 * reference counterpart: the reference assumes brightness constancy.  Inside every iteration the
 * mismatch J(x + d) - I(x) is freed by least squares of an additive offset (BIAS) or of an offset and
 * a gain (GAIN_BIAS) of J against I: the tensor and the right-hand side are built from centred
 * integer window sums (exact), a few fp64 operations in a fixed order and one rounding to float.
 * Everything after that (minEig and its tests, the update, the stop tests, bit 8's minimum
 * eigenvalue) is the plain tracker's on those values.  The level-0 L1 error is the raw one. */
#define VO_LK_ILLUM_BIAS       1
#define VO_LK_ILLUM_GAIN_BIAS  2

/* vo_lk_points_ex (fb_threshold == 0; back_pts may be NULL) or vo_lk_points_fb (fb_threshold > 0)
 * under illumination model illum; the gate's backward pass runs under the same model with flags 0.
 * Every window, 15x15 included, runs the generic per-level kernel.  illum outside {1, 2}, a bad
 * flag, bit 4 with init NULL, a negative, NaN or infinite threshold, a positive threshold with
 * back_pts NULL or a window outside vo_lk_points' sizes: VO_EARG with the outputs untouched. */
int vo_lk_points_illum(const vo_dims* d, const vo_opts* o, const vo_state* s, int prev,
                       const float* pts, const float* init, const int32_t* counts, int32_t cap,
                       int32_t flags, int32_t illum, double fb_threshold, float* back_pts,
                       float* out_pts, uint8_t* out_status, float* out_err, vo_stream_t stream);

/* vo_track_seeded under illumination model illum; seeds may be NULL (unseeded).  One entry for plain,
 * seeded, gated and seeded + gated tracking, compacting (compact = 1) or not.  trk_err is not
 * written.  Bad arguments as vo_track_seeded and vo_lk_points_illum: VO_EARG with nothing written. */
int vo_track_illum(const vo_dims* d, const vo_opts* o, const vo_state* s, int prev, int32_t illum,
                   const float* seeds, double fb_threshold, float* fb_scratch, int compact,
                   vo_stream_t stream);

/* Lens distortion (engine option dist_coeffs; the project's own definition in OpenCV's
 * form, restated in NumPy in tests/test_undistort_ref.py and reproduced bit for bit).  No reference
 * counterpart: the reference only reads rectified frames.  K, new_K and P are host pointers to
 * row-major 3x3 doubles of the form [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] (finite, fx and fy not
 * 0); dist is a host pointer to ndist = 0, 4, 5 or 8 doubles in OpenCV's order k1 k2 p1 p2 [k3 [k4 k5
 * k6]], missing ones 0 (12 or 14 coefficients and a rectification rotation are not supported).
 * All three calls are asynchronous on the stream, read nothing back and can be captured; on a bad
 * argument they return VO_EARG with nothing launched and nothing written.
 *
 * cv2.initUndistortRectifyMap(K, dist, None, new_K, (W, H), CV_16SC2): for every pixel (u, v) of
 * the W x H rectified grid, taken through new_K (NULL = K), the distortion model and K, the raw
 * position (mx, my) in fp64, quantised as rint(32 m) (half to even), clamped to [-2^20, 2^20 - 1]
 * (a NaN gives -2^20) and stored as map1 [H][W][2] int16 = (iu >> 5, iv >> 5) and map2 [H][W]
 * uint16 = (iv & 31) * 32 + (iu & 31).  mapd: [H][W][2] double or NULL, (mx, my) before the
 * quantisation.  W and H in 1..16384. */
int vo_undistort_map(const double* K, const double* dist, int ndist, const double* new_K, int W, int H,
                     int16_t* map1, uint16_t* map2, double* mapd, vo_stream_t stream);

/* cv2.remap(src, map1, map2, INTER_LINEAR, borderMode = BORDER_CONSTANT, borderValue = 0) for B
 * uint8 images through one fixed-point map: image b is read at src + b * src_stride (rows of
 * src_pitch bytes, sW x sH pixels) and written at dst + b * dst_stride (rows of dst_pitch bytes,
 * W x H pixels, the map's size).  With (ix, iy) = map1, a = map2 & 31, b = (map2 >> 5) & 31 and S
 * the source taken as 0 outside it,
 *   dst = ((32-a)(32-b) S(ix,iy) + a(32-b) S(ix+1,iy) + (32-a)b S(ix,iy+1) + ab S(ix+1,iy+1) + 512) >> 10
 * in integers, every tap tested on its own.  Only the W bytes of each destination row are written:
 * row padding and the bytes between images stay, and the source is not written.  VO_EARG: a NULL
 * pointer, B < 1, a side outside 1..16384, a pitch below its width, a negative stride, a
 * destination stride below an image's extent with B > 1, a source image of 2 GiB or more, or a
 * destination that overlaps the source.  Where dst_stride is a multiple of 4 one thread serves
 * eight images from one read of the map; any other stride is as valid and takes one image per
 * thread. */
int vo_remap_u8(int B, const uint8_t* src, int64_t src_stride, int64_t src_pitch, int sW, int sH, uint8_t* dst,
                int64_t dst_stride, int64_t dst_pitch, int W, int H, const int16_t* map1, const uint16_t* map2,
                vo_stream_t stream);

/* cv2.undistortPoints(pts, K, dist, None, P) with a fixed number of iterations (1..100; OpenCV's
 * default criteria give 5) and no epsilon test: pts [n][2] double raw pixels, out [n][2] double the
 * ideal normalised coordinates (P = NULL) or pixels through P; rows past n are not written; n = 0
 * launches nothing.  out may be pts. */
int vo_undistort_points(int n, const double* pts, const double* K, const double* dist, int ndist, const double* P,
                        int iters, double* out, vo_stream_t stream);

/* cv2.solvePnPRansac(..., SOLVEPNP_P3P) (:343) on [B][cap] points with counts.
 * out: rvec[B][3], tvec[B][3], success[B], inlier mask [B][cap] (u8), n_inl[B]. */
int vo_pnp_ransac(const vo_opts* o, int B, const float* obj, const float* img,
                  const int32_t* counts, int32_t cap, double* rvec, double* tvec,
                  int32_t* success, uint8_t* inl_mask, int32_t* n_inl, double* work,
                  int64_t work_stride, vo_stream_t stream);

/* Levenberg-Marquardt refinement of a pose on the reprojection error of its inliers, in the form
 * of cv2.solvePnPRefineLM (rvec, tvec in and out); the project's own definition (the
 * NumPy restatement tests/test_pnp_refine_ref.py), reproduced bit for bit.  obj [B][cap][3], img
 * [B][cap][2] with counts[B]; mask [B][cap] selects the inliers (NULL = every point); success
 * [B] (NULL = all): a chain with 0 is left untouched, info included.  max_iters 0..100, ftol finite
 * and >= 0, else VO_EARG with nothing written.  info [B][4] (NULL = not wanted): iterations used,
 * accepted steps, initial and final cost (sum of squared pixel residuals; +inf where the start
 * pose has a point at z <= 0 or a cost that is not finite: pose unchanged, 0 iterations). */
int vo_pnp_refine(const vo_opts* o, int B, const float* obj, const float* img, const uint8_t* mask,
                  const int32_t* counts, int32_t cap, const int32_t* success, int32_t max_iters,
                  double ftol, double* rvec, double* tvec, double* info, vo_stream_t stream);

/* vo_pnp, vo_pnp_triangulate and vo_filter_pnp_triangulate with that refinement applied to every
 * chain whose PnP succeeded, over its inliers, before anything reads the pose: pnp_rt, pose slot
 * nF and the triangulation use the refined pose; the inlier mask, the counts and the statuses are
 * those of the plain calls.  refine_iters = 0 is the plain call (the same launches); refine_info
 * [B][4] or NULL as vo_pnp_refine's info (rows of chains that are not refined are not written). */
int vo_pnp_ex(const vo_dims* d, const vo_opts* o, const vo_state* s, int32_t refine_iters,
              double refine_ftol, double* refine_info, vo_stream_t stream);
int vo_pnp_triangulate_ex(const vo_dims* d, const vo_opts* o, const vo_state* s, int32_t refine_iters,
                          double refine_ftol, double* refine_info, vo_stream_t stream);
int vo_filter_pnp_triangulate_ex(const vo_dims* d, const vo_opts* o, const vo_state* s,
                                 int32_t refine_iters, double refine_ftol, double* refine_info,
                                 vo_stream_t stream);

/* The optional reprojection-error gate on new landmarks (engine option tri_max_reproj_error; the
 * project's own definition, DESIGN 5g and the NumPy restatement tests/test_tri_gate_ref.py,
 * reproduced bit for bit).  No reference counterpart: triangulate_landmarks (:107-206) tests a
 * new point against the bearing angle (:117-147) and the two depths (:149-168) only.
 *   A candidate that reached cv2.triangulatePoints (:188) and passed the depth gate becomes a
 * landmark iff its float32 point X (the one the depth gate saw), promoted to double, reprojects
 * within max_reproj_error pixels of both observations it was made from: for the past view
 * (P_past, c_first) and the current view (P_cur, c_kp), with the very 3x4 matrices given to
 * cv2.triangulatePoints and one fp64 rounding per operation (no fused multiply-add),
 *     p_k = ((P_k0 X + P_k1 Y) + P_k2 Z) + P_k3   (k = 0, 1, 2)
 *     du = p_0 / p_2 - x,  dv = p_1 / p_2 - y,  e = du du + dv dv
 * and the view passes iff p_2 > 0 and e <= max_reproj_error^2 (squared once on the host, in
 * double; a NaN fails).  A candidate with a failing view is removed: neither appended to the
 * landmarks nor kept among the candidates.  The frame gate (:175-178), check_baseline, the depth
 * gate and its "keep", and the order of the appended landmarks and of the kept candidates stay the
 * reference's.  vo_bootstrap's triangulation (:319) is never gated.
 *   info: [B][4] int32 or NULL.  A chain that triangulates writes: candidates that reached
 * cv2.triangulatePoints, those of them the depth gate kept as candidates, those this gate dropped,
 * those appended as landmarks (counted even where the capacity could not hold them and the chain
 * ends with VO_ST_CAPACITY).  A chain with status 0 that does not triangulate (:366) writes four
 * zeros; a chain whose status is set keeps its row. */
typedef struct vo_tri_opts {
    double max_reproj_error;      /* pixels; finite and > 0                               */
    int32_t* info;                /* [B][4] counters (device memory) or NULL              */
} vo_tri_opts;

/* vo_triangulate with that gate, in both of its forms (one launch; gate / solve / append).
 * tri == NULL is vo_triangulate itself, with the same launches.  max_reproj_error that is not
 * finite and > 0: VO_EARG with nothing launched (so for the three calls below). */
int vo_triangulate_gated(const vo_dims* d, const vo_opts* o, const vo_state* s, int force,
                         const vo_tri_opts* tri, vo_stream_t stream);

/* vo_pnp_triangulate_ex and vo_filter_pnp_triangulate_ex with the gate in their triangulation,
 * with or without the pose refinement (refine_iters = 0: off), in kernels of their own.  tri ==
 * NULL is the _ex call, with the same launches. */
int vo_pnp_triangulate_gated(const vo_dims* d, const vo_opts* o, const vo_state* s, int32_t refine_iters,
                             double refine_ftol, double* refine_info, const vo_tri_opts* tri,
                             vo_stream_t stream);
int vo_filter_pnp_triangulate_gated(const vo_dims* d, const vo_opts* o, const vo_state* s,
                                    int32_t refine_iters, double refine_ftol, double* refine_info,
                                    const vo_tri_opts* tri, vo_stream_t stream);

/* vo_pnp_ex as the first half of the unfused gated step: it checks tri like the calls above, then
 * is vo_pnp_ex (PnP does not triangulate, so nothing else of tri is used; the vo_triangulate_gated
 * call that follows applies it). */
int vo_pnp_gated(const vo_dims* d, const vo_opts* o, const vo_state* s, int32_t refine_iters,
                 double refine_ftol, double* refine_info, const vo_tri_opts* tri, vo_stream_t stream);

/* Sub-pixel refinement of corner positions in the form of cv2.cornerSubPix; the project's own
 * definition (the NumPy restatement tests/test_subpix_ref.py), reproduced bit for bit.
 * Plain device images: image b is H rows of W u8 pixels at img + b * img_stride, `pitch` bytes
 * between rows (pitch >= W).  pts [B][cap][2] with counts[B]: pts[b][0..counts[b]) are refined in
 * place, rows past the count are not touched, a count <= 0 is skipped.  (win_w, win_h): half sizes
 * of the window, 1..7 each (the window is (2 win_w + 1) x (2 win_h + 1)); (zero_w, zero_h): half
 * sizes of the central zone with weight 0, (-1, -1) = none, else 0 <= zero_w < win_w and
 * 0 <= zero_h < win_h; max_iters 1..100; eps finite and >= 0 (a step of at most eps pixels ends
 * the walk).  A point that would end more than the half-window from its start on an axis, or
 * outside the image, keeps its start value; a start outside [0,W) x [0,H) is left alone.  iters
 * [B][cap] (NULL = not wanted): iterations walked per point.  Anything outside these limits, or a
 * count above cap, returns VO_EARG with nothing written.  The counts are device memory, so the
 * capacity check reads them back first: unlike the other entry points this one waits for the
 * stream before it launches and cannot be captured into a graph (vo_gftt_subpix can). */
int vo_corner_subpix(int B, const uint8_t* img, int64_t img_stride, int32_t pitch, int W, int H,
                     float* pts, const int32_t* counts, int32_t cap,
                     int32_t win_w, int32_t win_h, int32_t zero_w, int32_t zero_h,
                     int32_t max_iters, double eps, int32_t* iters /* [B][cap] or NULL */,
                     vo_stream_t stream);

/* cv2.triangulatePoints (:188) for float32 points: P1,P2 [n][12] (row-major 3x4 each,
 * one pair per point), x1,x2 [n][2] -> out [n][4] float32. */
int vo_triangulate_points(int n, const double* P1, const double* P2, const float* x1,
                          const float* x2, float* out4, vo_stream_t stream);

/* vo_triangulate_points, and the quantity the reprojection gate (vo_tri_opts) compares: err2
 * [n][2] double, the e of the float32 point out4[:3] / out4[3] (float32 divisions, as :189)
 * against (P1, x1) and (P2, x2), evaluated exactly as defined there; +inf where p_2 is not > 0.
 * out4 is vo_triangulate_points' bit for bit.  No reference counterpart. */
int vo_triangulate_points_err(int n, const double* P1, const double* P2, const float* x1,
                              const float* x2, float* out4, double* err2, vo_stream_t stream);

/* cv2.Rodrigues (:354): n vectors [n][3] -> matrices [n][9], or the inverse. */
int vo_rodrigues(int n, int to_matrix, const double* in, double* out, vo_stream_t stream);

/* ---- bootstrap (initialization, :293-323) --------------------------------------- */

/* Device buffers for one SIFT invocation.  Geometry (octave sizes/offsets) is filled by
 * vo_sift_plan(); the buffers are caller-allocated with the sizes it reports. */
#define VO_SIFT_MAX_OCT 16
typedef struct vo_sift_buf {
    int32_t W, H;                 /* input image size                                   */
    int32_t n_oct;
    int32_t oct_w[VO_SIFT_MAX_OCT], oct_h[VO_SIFT_MAX_OCT];
    int64_t gauss_off[VO_SIFT_MAX_OCT * 6];   /* float offsets into gauss            */
    int64_t dog_off[VO_SIFT_MAX_OCT * 5];     /* float offsets into dog              */
    int64_t gauss_floats, dog_floats, tmp_floats;
    float* gauss;                 /* Gaussian scale space                               */
    float* dog;                   /* difference of Gaussians                            */
    float* tmp;                   /* separable-blur scratch (2W*2H floats)              */
    float* consts;                /* [7*32 kernel taps][64 exp32f table] (host-filled)  */
    int32_t* counters;            /* [8]: n_cand, n_kp, n_out, overflow, n_refined, -   */
    int32_t* cand;                /* extrema candidates [cand_cap][4] (o, layer, r, c)  */
    float* kp;                    /* raw keypoints [kp_cap][8]                          */
    float* kp_out;                /* sorted, deduplicated keypoints [kp_cap][6]         */
    float* desc;                  /* descriptors [kp_cap][128] (integer-valued floats)  */
    float* hist;                  /* descriptor histogram scratch [kp_cap][360]         */
    int32_t cand_cap, kp_cap;     /* kp_cap <= 32768 (raw keypoints sorted in LDS)       */
    int32_t nfeatures;            /* SIFT_create(nfeatures): > 0 applies retainBest      */
} vo_sift_buf;

/* Fill the geometry of `sb` for a W x H image (host only, no device work); resets
 * nfeatures to 0 (no cap). */
int vo_sift_plan(vo_sift_buf* sb, int W, int H);

/* cv2.SIFT_create().detectAndCompute(img, None) (:35,226-227) for one image;
 * sb->nfeatures > 0 is SIFT_create(nfeatures) (BASELINE C5's capped SIFT): the keypoints are
 * cut by KeyPointsFilter::retainBest in libstdc++'s nth_element/partition order. */
int vo_sift(const vo_sift_buf* sb, const uint8_t* img, int W, int H, vo_stream_t stream);

/* detectAndCompute for B images per launch sequence (the bootstrap of B chains, :226-227
 * for every chain): image b at imgs + b * img_stride; every buffer of `sb` holds B
 * consecutive per-image blocks of the size vo_sift_plan reports (gauss_floats, dog_floats,
 * tmp_floats, 8 counters, cand_cap*4, kp_cap*{8,6,128,360}).  Image b's results are bit-
 * identical to vo_sift on that image alone. */
int vo_sift_batch(const vo_sift_buf* sb, int B, const uint8_t* imgs, int64_t img_stride, int W, int H,
                  vo_stream_t stream);

/* Test hook: KeyPointsFilter::retainBest (the SIFT_create(nfeatures) cap, VisualOdometryPipeLine.py:35
 * with BASELINE C5's nfeatures) as run inside vo_sift_batch, on caller-given rows kp_out [n][6]
 * (response in column 4), reordered in place; counters[2] = n on entry, the kept count on
 * return; scratch >= 4 n + 2 ints, tmp >= 6 n floats (all device memory); n <= 32768. */
int vo_sift_retain_best_rows(float* kp_out, int32_t n, int32_t nfeatures, int32_t* counters, int32_t* scratch,
                             float* tmp, vo_stream_t stream);

/* Batched BFMatcher().knnMatch(q, t, k=2) (:36,229) for B independent problems on MFMA
 * (csrc/vo_match.hip): q [B][qcap][128], t [B][tcap][128] integer-valued float descriptors
 * (SIFT: 0..255), device counts nq[B] / nt[B]; idx2 [B][qcap][2] (-1 if absent), dist2
 * [B][qcap][2] (FLT_MAX if absent); rows >= nq[b] untouched.  Same (distance, index) order and
 * float distances as OpenCV (batchDistance + the k = 2 insertion).  scratch: device bytes >= vo_bf_knn2_batch_scratch(). */
int64_t vo_bf_knn2_batch_scratch(int B, int32_t qcap, int32_t tcap);
int vo_bf_knn2_batch(int B, const float* q, const int32_t* nq, int32_t qcap, const float* t,
                     const int32_t* nt, int32_t tcap, int32_t dim, int32_t* idx2, float* dist2,
                     void* scratch, int64_t scratch_bytes, vo_stream_t stream);

/* Ratio test + match gathering of initial_feature_matching (:218-245) for B chains:
 * keeps query i iff both neighbours exist (idx >= 0) and dist0 < ratio * dist1 (in double, as
 * Python; a tie is dropped), in query order.  pts0 / pts1 are [B][cap][2]; counts[b] is the number
 * of matches that passed.  Overflow is reported, not truncated: where more than cap pass, counts[b]
 * is that larger number, the first cap matches are stored and no row at or past cap is written.
 * vo_bootstrap ends a chain whose count exceeds its cap with VO_ST_CAPACITY, and
 * vo_find_essential gives ok = 0 for it without reading its points. */
int vo_ratio_matches(int B, const float* kp0, const float* kp1, int32_t kp_stride,
                     const int32_t* idx2, const float* dist2, const int32_t* nq, int32_t q_stride,
                     double ratio, float* pts0, float* pts1, int32_t* counts, int32_t cap,
                     vo_stream_t stream);

/* cv2.findEssentialMat(p0,p1,K,RANSAC,prob,threshold) (:308) for B problems of
 * [B][cap] points with counts; E [B][9], mask [B][cap]; work: work_doubles >= 4 cap + 90 * 64 per
 * problem.  counts[b] < 5: ok = 0, mask[:counts[b]] = 0, E untouched.  counts[b] > cap (the
 * overflow vo_ratio_matches reports): ok = 0, nothing else read or written. */
int vo_find_essential(const vo_opts* o, int B, const float* p0, const float* p1,
                      const int32_t* counts, int32_t cap, double prob, double threshold,
                      int32_t max_iters, double* E, uint8_t* mask, int32_t* ok, double* work,
                      int32_t work_doubles, vo_stream_t stream);

/* cv2.recoverPose(E,p0,p1,K) (:315): R [B][9], t [B][3], mask [B][cap], n_good [B]. */
int vo_recover_pose(const vo_opts* o, int B, const double* E, const float* p0,
                    const float* p1, const int32_t* counts, int32_t cap, double* R, double* t,
                    uint8_t* mask, int32_t* n_good, vo_stream_t stream);

/* Bootstrap assembly into chain state (initial_feature_matching + :308-323): from the
 * per-chain bootstrap matches (pts0/pts1 [B][cap], counts) run E-RANSAC, inlier
 * filtering, recoverPose, sign fix, triangulation, pose append, num_pts.  Per chain: counts[b] = 0
 * -> VO_ST_NO_MATCHES; counts[b] > cap (vo_ratio_matches' overflow) or more matches than pcap ->
 * VO_ST_CAPACITY; no essential matrix -> VO_ST_ESSENTIAL_FAILED.  Such a chain keeps
 * transforms = [(I, 0)] (nF = 1) with no landmarks and no candidates. */
int vo_bootstrap(const vo_dims* d, const vo_opts* o, const vo_state* s, const float* pts0,
                 const float* pts1, const int32_t* counts, int32_t cap, vo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
