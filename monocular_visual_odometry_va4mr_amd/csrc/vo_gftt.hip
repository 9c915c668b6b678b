// goodFeaturesToTrack for gfx950: integer-exact min-eigenvalue (or Harris) map with 3x3 NMS into a
// key list, then the selection (vo_select.hip).
//
// Reference call site: VisualOdometryPipeLine.py:256.  Arithmetic follows oracle/vo_oracle_img.c
// operation by operation (that file restates OpenCV 4.6).
#include "vo_dev.h"

#include <math.h>
#include <type_traits>

namespace {

// ------------------------------------------------------------------ GFTT
struct EigParams {
    const uint8_t* pyr;
    int64_t pstride;
    int W, H, pitch;
    int64_t off;
    int bs, harris;
    double harris_k;
    uint32_t* eig_max;
    uint64_t* keys;
    int32_t* nkeys;
    int ccap;
    int B, tiles_x, tiles_y;
    const int32_t* chain_status;
    float* eig_out;          // optional [B][W*H] eigen map (diagnostics, vo_gftt_eigmap)
};
// the masked kernels' arguments (vo_gftt_masked): the detector mask, [B] images of H rows, u8,
// non-zero = allowed.  It gates what counts in the per-chain maximum and what is emitted as a key;
// the 3x3 test looks at all eight neighbours whether they are allowed or not (featureselect.cpp:
// minMaxLoc takes the mask, dilate does not).  The unmasked kernels keep EigParams, and with it
// the code they had.
struct EigParamsM : EigParams {
    const uint8_t* mask;
    int64_t mstride;
    int mpitch;
};
template <bool MASKED> using EigArgs = std::conditional_t<MASKED, EigParamsM, EigParams>;
template <bool MASKED> VO_DEV const uint8_t* eig_mask(const EigArgs<MASKED>& P, int b)
{
    if constexpr (MASKED) return P.mask + (int64_t)b * P.mstride;
    else return nullptr;
}
template <bool MASKED> VO_DEV int eig_mpitch(const EigArgs<MASKED>& P)
{
    if constexpr (MASKED) return P.mpitch;
    else return 0;
}

// Fused cornerMinEigenVal / cornerHarris + 3x3 local-maximum test of goodFeaturesToTrack
// (featureselect.cpp, corner.cpp) on a 64x16 output tile.
//  * gradients: 3x3 Sobel (integer) at every covariance position, the covariance
//    position reflected (BORDER_REFLECT_101 of boxFilter) and Sobel reading the
//    materialised reflect-101 border of level 0;
//  * box sums of the gradient products (integer), lambda_min in double -> float;
//  * the eigen map is never stored: the tile recomputes a 1-pixel halo, and a pixel is a
//    candidate iff v > 0 and v >= its 8 neighbours.  With thr = quality * max >= 0 this is
//    exactly OpenCV's "v > thr and v == dilate(threshold(eig, thr))(x,y)"; the v > thr part
//    needs the global max and is applied by k_gftt_select.
//  * candidates are appended as (fkey(v) << 32 | y*W + x) with one atomic per block (the
//    list order is irrelevant: keys are unique and k_gftt_select orders them).
#define EIG_TW 64
#define EIG_TH 16
#define EIG_MAXBS 7
#define EIG_CW (EIG_TW + 2 + EIG_MAXBS - 1)
#define EIG_CH (EIG_TH + 2 + EIG_MAXBS - 1)
template <bool MASKED>
__global__ void __launch_bounds__(256) k_eignms(EigArgs<MASKED> P)
{
    __shared__ int sdx[EIG_CW * EIG_CH];
    __shared__ int sdy[EIG_CW * EIG_CH];
    __shared__ float sE[(EIG_TH + 2) * (EIG_TW + 2)];
    __shared__ uint32_t smax;
    __shared__ int sh[16];
    __shared__ int sbase;
    const int ntile = P.tiles_x * P.tiles_y;
    const int item = xcd_item(blockIdx.x, P.B * ntile);
    if (item >= P.B * ntile) return;
    const int b = item / ntile, t = item - b * ntile;
    if (P.chain_status && P.chain_status[b] != 0) return;
    const int ty0 = t / P.tiles_x, tx0 = t - ty0 * P.tiles_x;
    const int x0 = tx0 * EIG_TW, y0 = ty0 * EIG_TH;
    const int bs = P.bs, a0 = bs / 2;
    const int ew = EIG_TW + 2, eh = EIG_TH + 2;          // eig region: tile + 1-px halo
    const int cw = ew + bs - 1, ch = eh + bs - 1;        // covariance region
    const uint8_t* img = P.pyr + b * P.pstride + P.off;
    const uint8_t* mk = eig_mask<MASKED>(P, b);
    const int mpitch = eig_mpitch<MASKED>(P);
    if (threadIdx.x == 0) smax = 0;
    for (int q = threadIdx.x; q < cw * ch; q += blockDim.x) {
        const int qy = q / cw, qx = q - qy * cw;
        const int cx = refl101(x0 - 1 - a0 + qx, P.W), cy = refl101(y0 - 1 - a0 + qy, P.H);
        const uint8_t* c = img + (int64_t)(cy + VO_BORDER) * P.pitch + (cx + VO_BORDER);
        const uint8_t* u = c - P.pitch;
        const uint8_t* l = c + P.pitch;
        sdx[q] = (u[1] - u[-1]) + 2 * (c[1] - c[-1]) + (l[1] - l[-1]);
        sdy[q] = (l[-1] - u[-1]) + 2 * (l[0] - u[0]) + (l[1] - u[1]);
    }
    __syncthreads();
    const double s = 1.0 / ((double)(1 << 2) * bs * 255.0);
    uint32_t lmax = 0;
    for (int e = threadIdx.x; e < ew * eh; e += blockDim.x) {
        const int ey = e / ew, ex = e - ey * ew;
        int sxx = 0, sxy = 0, syy = 0;
        for (int i = 0; i < bs; ++i)
            for (int j = 0; j < bs; ++j) {
                const int q = (ey + i) * cw + (ex + j);
                const int gx = sdx[q], gy = sdy[q];
                sxx += gx * gx;
                sxy += gx * gy;
                syy += gy * gy;
            }
        float v;
        if (!P.harris) {
            const int64_t T = (int64_t)sxx + syy;
            const int64_t dd = (int64_t)sxx - syy;
            const int64_t Dd = dd * dd + 4 * (int64_t)sxy * sxy;
            v = (float)(((double)T - sqrt((double)Dd)) * (s * s * 0.5));
        } else {
            const int64_t det = (int64_t)sxx * syy - (int64_t)sxy * sxy;
            const int64_t T = (int64_t)sxx + syy;
            v = (float)(((double)det - P.harris_k * (double)(T * T)) * (s * s * s * s));
        }
        sE[e] = v;
        // the global max counts each image pixel once: the tile's own pixels only
        const int x = x0 - 1 + ex, y = y0 - 1 + ey;
        if (ex >= 1 && ex <= EIG_TW && ey >= 1 && ey <= EIG_TH && x < P.W && y < P.H) {
            const uint32_t k = fkey(v);
            if (!MASKED || mk[(int64_t)y * mpitch + x]) lmax = k > lmax ? k : lmax;
            if (P.eig_out) P.eig_out[(int64_t)b * P.W * P.H + (int64_t)y * P.W + x] = v;
        }
    }
    // wave max, then one LDS atomic per wave
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t t2 = __shfl_xor(lmax, o, 64);
        lmax = t2 > lmax ? t2 : lmax;
    }
    __syncthreads();
    if (lane_id() == 0 && lmax) atomicMax(&smax, lmax);
    if (!P.keys) {
        __syncthreads();
        if (threadIdx.x == 0 && smax) atomicMax(&P.eig_max[b], smax);
        return;
    }
    // local maxima among the tile's interior pixels (4 per thread)
    uint64_t kk[4];
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = threadIdx.x + 256 * j;
        const int ly = k / EIG_TW, lx = k - ly * EIG_TW;
        const int x = x0 + lx, y = y0 + ly;
        kk[j] = 0;
        if (x >= 1 && x < P.W - 1 && y >= 1 && y < P.H - 1 && (!MASKED || mk[(int64_t)y * mpitch + x])) {
            const float* r = sE + ly * ew + lx;      // row above, centred at lx+1
            const float v = r[ew + 1];
            if (v > 0.f && v >= r[0] && v >= r[1] && v >= r[2] && v >= r[ew] && v >= r[ew + 2] &&
                v >= r[2 * ew] && v >= r[2 * ew + 1] && v >= r[2 * ew + 2]) {
                kk[j] = ((uint64_t)fkey(v) << 32) | (uint32_t)(y * P.W + x);
                ++cnt;
            }
        }
    }
    int tot;
    const int pre = block_scan_i32(cnt, sh, &tot);
    if (threadIdx.x == 0) {
        sbase = tot ? atomicAdd(&P.nkeys[b], tot) : 0;
        if (smax) atomicMax(&P.eig_max[b], smax);
    }
    __syncthreads();
    int pos = sbase + pre;
    uint64_t* out = P.keys + (int64_t)b * P.ccap;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (kk[j]) {
            if (pos < P.ccap) out[pos] = kk[j];
            ++pos;
        }
}

// ---------------------------------------------------------------------------------------
// k_eig3: the fused min-eigenvalue + 3x3 local-maximum pass of k_eignms, specialised to the
// reference's configuration (blockSize 3, useHarrisDetector False; main.py:31-33,61-63,91-93)
// as a row-streaming kernel.  One wave owns an E3_OUT-column x E3_TH-row tile; lane = image
// column (3 halo lanes each side) and the wave slides down the rows keeping every
// intermediate in registers: the Sobel row terms of the last two image rows, the box row
// sums of the last two gradient rows, the NMS state of the last two eigen rows.  Horizontal
// neighbours come from the adjacent lanes through DPP wave shifts.  Integers, the double
// expression of lambda_min, the reflect-101 handling and the emitted key set are those of
// k_eignms (the parity tests compare corner lists and eigen maps bit for bit).
//
// The exact value v = (float)(((double)T - sqrt((double)D)) * sc) is only consumed where a key is
// emitted (local maxima with v > 0) and in the per-chain maximum; everywhere else it is compared
// with its eight neighbours.  k_eig3<false> therefore runs the row loop on an f32 interval
// [lo, hi] that provably contains v (e3_interval), queues the pixels the intervals cannot rule
// out as maxima, and evaluates the double expression for queued pixels only, 64 at a time.
// k_eig3<true> evaluates it for every pixel (the eigen map of vo_gftt_eigmap, VO_EIG_EXACT=1).
#define E3_OUT 58
#define E3_TH 64
#define E3_CAP 512            // key buffer of the exact-everywhere form
#define E3_QCAP 256           // queue of possible maxima (16 bytes each), emptied after every 8 rows
#define E3_Q_MAXONLY 0x10000  // entry counts in the maximum only (image border: no NMS there)
#define E3_Q_DECIDED 0x20000  // entry's lower bound is >= every neighbour's upper bound

// lane i <- i-1 / i+1; the lane without a neighbour reads 0 (bound_ctrl)
VO_DEV int dpp_from_left(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xF, 0xF, true); }
VO_DEV int dpp_from_right(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x130, 0xF, 0xF, true); }
VO_DEV float dpp_max_lr(float v)
{
    const int i = __float_as_int(v);
    return fmaxf(__int_as_float(dpp_from_left(i)), __int_as_float(dpp_from_right(i)));
}
VO_DEV int dpp_max_lr(int v) { return max(dpp_from_left(v), dpp_from_right(v)); }

// lanes below this one set in a ballot mask
VO_DEV int lane_prefix(uint64_t m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
}

// sqrt of a double holding an integer in [0, 2^53): the compiler's correctly rounded sequence
// (v_rsq_f64 + Newton steps with a final fma correction) without its range reduction for inputs
// below 2^-767 and its class fix-ups, which such inputs never need; 0 (rsq = inf) selects 0.
// Bit-identical to sqrt() there, ~5 instructions shorter per pixel in k_eig3.
VO_DEV double sqrt_int_f64(double x)
{
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = 0.5 * y;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    double d = __builtin_fma(-g, g, x);
    g = __builtin_fma(d, h, g);
    d = __builtin_fma(-g, g, x);
    g = __builtin_fma(d, h, g);
    return x == 0.0 ? 0.0 : g;
}

// lambda_min * sc from the box sums: T = sxx + syy, dd = sxx - syy (the products are exact in
// double: |dd|, |sxy| < 2^24).  D <= T^2 (Cauchy-Schwarz on the box sums) and the square root is
// correctly rounded, so sqrt(D) <= T and v >= +0 at every pixel.
VO_DEV float e3_exact(int T, int dd, int sxy, double sc)
{
    const double Dd = (double)dd * (double)dd + 4.0 * ((double)sxy * (double)sxy);
    return (float)(((double)T - sqrt_int_f64(Dd)) * sc);
}

// f32 interval around e3_exact's value v.  With u = 2^-24, s = sqrt(D), A = (T + s) * sc:
//   Tf = fl(T)                      = T (1 + t),  |t| <= u      (T < 2^25; dd, sxy are exact)
//   Df = fl(fl(dd^2) + 4 fl(sxy^2)) = D (1 + d),  |d| <= 2u + u^2  (non-negative terms)
//   sf = v_sqrt_f32(Df), taken as 2 ulp off     = s (1 + e),  |e| <= u + 4u + O(u^2) <= 5.01u
//   vt = fl(fl(Tf - sf) * fl(sc))   = ((T - s) + T t - s e)(1 + h) sc,  |h| <= 3.01u
// so |vt - (T - s) sc| <= u (T + 5.01 s + 3.01 (T - s)) (1 + 4u) sc <= 4.02 u A.  The double
// sequence and its final rounding to float put v within 1.01 u A of (T - s) sc, and rounding
// lo = fl(vt - eps), hi = fl(vt + eps) moves a bound by at most u (|vt| + eps) <= 1.01 u A:
// 6.04 u A in all.  eps = fl(fl(2^-21 sc) * fl(Tf + sf)) >= 8 u A (1 - 9u) > 7.99 u A covers it
// with a third to spare.  Nothing here under- or overflows: sums are integers below 2^25,
// D < 2^49, and a non-zero Tf - sf is at least 2^-24, so vt >= 2^-49 in magnitude or 0.
// All sums zero gives vt = eps = 0 and v = 0 exactly.
// v >= 0 (e3_exact), so the lower bound is clamped at 0 and hi >= v >= 0: both bounds are
// non-negative floats, which order as their bit patterns do, and the NMS compares and maximises
// them as integers (DPP and v_max3_i32 directly, no NaN canonicalisation).  A -0 would only make
// a bound look lower than it is, which flags more, never less.
VO_DEV void e3_interval(int T, int dd, int sxy, float scf, float epk, int& lo, int& hi)
{
    const float Tf = (float)T, df = (float)dd, xf = (float)sxy;
    const float sf = __builtin_amdgcn_sqrtf(df * df + 4.f * (xf * xf));
    const float vt = (Tf - sf) * scf;
    const float eps = epk * (Tf + sf);
    lo = __float_as_int(fmaxf(vt - eps, 0.f));
    hi = __float_as_int(vt + eps);
}

// one pixel's box sums from the image, with k_eignms's arithmetic and reflect-101 handling (slow:
// only for the neighbours of a queued pixel whose interval overlaps theirs, and for rows the
// queue had no room for).  img is pixel (0,0) of a level-0 image (below 2^31 bytes), 0 <= x < W,
// 0 <= y < H.
VO_DEV void e3_sums(const uint8_t* img, int pitch, int W, int H, int x, int y, int& T, int& dd, int& sxy)
{
    const uint8_t* org = img - pitch - 1;                // pixel (-1,-1): offsets below are >= 0
    int sxx = 0, syy = 0;
    sxy = 0;
#pragma unroll 1
    for (int q = 0; q < 9; ++q) {
        const int i = q / 3, j = q - 3 * i;
        const int cx = refl101(x - 1 + j, W), cy = refl101(y - 1 + i, H);
        const uint8_t* u = org + (uint32_t)(cy * pitch + cx);     // row above, left neighbour first
        const uint8_t* c = u + pitch;
        const uint8_t* l = c + pitch;
        const int gx = (u[2] - u[0]) + 2 * (c[2] - c[0]) + (l[2] - l[0]);
        const int gy = (l[0] - u[0]) + 2 * (l[1] - u[1]) + (l[2] - u[2]);
        sxx += gx * gx;
        sxy += gx * gy;
        syy += gy * gy;
    }
    T = sxx + syy;
    dd = sxx - syy;
}

//
// MASKED (vo_gftt_masked), exact-everywhere form only: one mask byte per lane and eigen row, used in
// two places.  The per-chain maximum is the one over the allowed pixels, so a masked-out pixel
// never counts in it; and only an allowed pixel is emitted as a key.  The NMS itself keeps looking
// at all eight neighbours.  (The interval form finds the maximum among the possible local maxima
// of the map; the greatest allowed pixel need not be one, its stronger neighbours may all be
// masked out, so masked calls take the form that evaluates every pixel.)
//
// 8 waves per SIMD (64 VGPRs): the kernel hides its latencies with occupancy, and rides beside LK
template <bool EXACT, bool MASKED = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) k_eig3(EigArgs<MASKED> P)
{
    static_assert(EXACT || !MASKED, "the mask is implemented in the exact-everywhere form");
    __shared__ uint64_t kbuf[EXACT ? E3_CAP : 1];
    __shared__ int4 qbuf[EXACT ? 1 : E3_QCAP];
    const int tiles = P.tiles_x * P.tiles_y;
    const int item = xcd_item(blockIdx.x, P.B * tiles);
    if (item >= P.B * tiles) return;
    const int b = item / tiles, t = item - b * tiles;
    if (P.chain_status && P.chain_status[b] != 0) return;
    const int ty = t / P.tiles_x, tx = t - ty * P.tiles_x;
    const int x0 = tx * E3_OUT, y0 = ty * E3_TH;
    const int W = P.W, H = P.H;
    const int lane = lane_id();
    const int c = x0 - 3 + lane;                         // image column of this lane
    const uint8_t* img = P.pyr + (int64_t)b * P.pstride + P.off + (int64_t)VO_BORDER * P.pitch + VO_BORDER;
    // row loads: one wave-uniform pointer (row -1, column x0-3: inside the border) plus a 32-bit
    // offset per lane (a level-0 image is below 2^31 bytes); cl is the lane, held inside the
    // padded row (column W+2 at most), so cl == lane for every own lane
    const uint8_t* colp = img - P.pitch + (x0 - 3);
    const uint32_t cl = (uint32_t)min(lane, W + 2 - (x0 - 3));
    auto load_row = [&](int row) { return (int)colp[(uint32_t)((row + 1) * P.pitch) + cl]; };
    // the mask byte of image row `row` (0 <= row < H) at this lane's column, held inside the row: a
    // halo lane outside the image is no neighbour of any pixel the tile queues
    const uint8_t* mkp = eig_mask<MASKED>(P, b);
    const int mpitch = eig_mpitch<MASKED>(P);
    const uint32_t mcl = MASKED ? (uint32_t)min(max(c, 0), W - 1) : 0u;
    auto allowed_at = [&](int row) { return !MASKED || mkp[(int64_t)row * mpitch + mcl] != 0; };
    const int g0 = max(y0 - 2, 0), g1 = min(y0 + E3_TH + 1, H - 1);   // gradient / box rows
    const int e0 = max(y0 - 1, 0);                                     // first eigen row
    const int o0 = max(y0, 1), o1 = min(y0 + E3_TH, H - 1);            // NMS rows [o0, o1)
    const int m1 = min(y0 + E3_TH, H);                                 // own rows [y0, m1)
    const bool own = lane >= 3 && lane < 3 + E3_OUT && c < W;
    const bool edge_col = own && (c == 0 || c == W - 1);               // in the maximum, not in the NMS
    const bool nms_col = own && !edge_col;
    const bool hedge = x0 == 0 || x0 + E3_OUT + 3 > W - 1;             // tile reaches column 0 or W-1
    const double s = 1.0 / ((double)(1 << 2) * 3 * 255.0);
    const double sc = s * s * 0.5;
    const float scf = (float)sc, epk = (float)(sc * (1.0 / 2097152.0));
    // every own pixel has v >= +0 (e3_exact), so the interval form starts the maximum there and
    // only adds the pixels it evaluates exactly
    uint32_t kmax = (!EXACT && own) ? fkey(0.f) : 0u;
    uint64_t* out = P.keys ? P.keys + (int64_t)b * P.ccap : nullptr;
    // ---- exact-everywhere form: keys gathered in kbuf, one atomic per E3_CAP-sized batch
    int nbuf = 0;
    auto flush = [&]() {
        int base = 0;
        if (lane == 0) base = atomicAdd(&P.nkeys[b], nbuf);
        base = __builtin_amdgcn_readfirstlane(base);
        wave_lds_sync();
        for (int i = lane; i < nbuf; i += 64)
            if (base + i < P.ccap) out[base + i] = kbuf[i];
        wave_lds_sync();
        nbuf = 0;
    };
    float eB = 0.f;                                      // eigen row r-1
    // the NMS maxima of the last two rows, each formed once when its row is new: 3-neighbour max
    // of row r-2, left / right max of row r-1 (fmaxf is exact and order-free on these values)
    float mA3 = 0.f, mB2 = 0.f;
    // ---- interval form: the same row state over the lower (nA3, nB2) and upper (nA3H, nB2H)
    // bounds, the bounds and box sums of row r-1, and the queue of possible maxima
    int loB = 0, hiB = 0, nA3 = 0, nB2 = 0, nA3H = 0, nB2H = 0;
    int TB = 0, dB = 0, sB = 0;
    bool alB = true;                                     // masked: the pixel of row r-1 is allowed
    int nq = 0;
    uint64_t ovf = 0;                                    // own rows (bit rn - y0) the queue had no room for
    // one batch of up to 64 pixels, one per lane, from their box sums: the exact value, the
    // maximum, the eight neighbours' exact values (from the image) where the intervals left the
    // NMS open, and the keys appended with one atomic
    auto batch = [&](int4 e, bool act) {
        const float v = e3_exact(e.y, e.z, e.w, sc);
        const uint32_t k = fkey(v);
        if (act && k > kmax) kmax = k;
        const int x = x0 - 3 + (e.x & 63), y = y0 + ((e.x >> 8) & 63);
        bool cand = act && !(e.x & E3_Q_MAXONLY) && v > 0.f;
        bool open = cand && !(e.x & E3_Q_DECIDED);
#pragma unroll 1
        for (int q = 0; q < 9 && __ballot(open); ++q) {
            if (q == 4 || !open) continue;
            const int i = q / 3, j = q - 3 * i;
            int T, dd, sxy;
            e3_sums(img, P.pitch, W, H, x - 1 + j, y - 1 + i, T, dd, sxy);
            if (!(v >= e3_exact(T, dd, sxy, sc))) cand = open = false;
        }
        const uint64_t m = __ballot(cand);
        if (m) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&P.nkeys[b], __popcll(m));
            base = __builtin_amdgcn_readfirstlane(base) + lane_prefix(m);
            if (cand && base < P.ccap) out[base] = ((uint64_t)k << 32) | (uint32_t)(y * W + x);
        }
    };
    // empty the queue in batches while it holds `least` entries or more, then the own rows it
    // had no room for, their box sums taken from the image (only when a few rows flag more
    // pixels than the queue holds: periodic patterns, where most pixels tie)
    auto service = [&](int least) {
        for (;;) {
            int4 e = make_int4(0, 0, 0, 0);
            bool act;
            if (nq >= least) {
                wave_lds_sync();
                const int n = nq < 64 ? nq : 64;
                nq -= n;
                act = lane < n;
                e = qbuf[nq + lane];                     // nq + 64 <= E3_QCAP: inside the queue
                wave_lds_sync();
            } else if (ovf) {
                const int rn = y0 + __builtin_ctzll(ovf);
                ovf &= ovf - 1;
                act = own;
                if (own) {
                    e.x = (int)cl | ((rn - y0) << 8) | (nms_col && rn >= o0 && rn < o1 ? 0 : E3_Q_MAXONLY);
                    e3_sums(img, P.pitch, W, H, c, rn, e.y, e.z, e.w);
                }
            } else {
                break;
            }
            batch(e, act);
        }
    };
    // queue the pixels of own row rn with `q` set (box sums T, dd, sxy)
    auto push = [&](bool q, int rn, int flags, int T, int dd, int sxy) {
        const uint64_t m = __ballot(q);
        const int n = nq + __popcll(m);
        if (n <= E3_QCAP) {
            if (q) qbuf[nq + lane_prefix(m)] = make_int4((int)cl | ((rn - y0) << 8) | flags, T, dd, sxy);
            nq = n;
        } else {
            ovf |= 1ull << (rn - y0);
        }
    };
    // eigen row r from the box row sums of rows r-1, r, r+1; then the NMS of row r-1.  ST: a
    // steady-state row (r-1 is an NMS row of this tile).
    auto eig_row = [&](int r, int ax, int ay, int az, int bx, int by, int bz, int cx, int cy, int cz, auto st) {
        constexpr bool ST = decltype(st)::value;
        const int sxx = ax + bx + cx, sxy = ay + by + cy, syy = az + bz + cz;
        const int T = sxx + syy, dd = sxx - syy;
        const int rn = r - 1;
        if constexpr (EXACT) {
            const float v = e3_exact(T, dd, sxy, sc);
            const bool al = allowed_at(r);
            if (own && r >= y0 && r < m1) {
                const uint32_t k = fkey(v);
                if (al) kmax = k > kmax ? k : kmax;
                if (P.eig_out) P.eig_out[(int64_t)b * W * H + (int64_t)r * W + c] = v;
            }
            const float mV2 = dpp_max_lr(v);
            if (ST || (rn >= o0 && rn < o1)) {
                const float mV = fmaxf(mV2, v);
                const bool cand = nms_col && out && alB && eB > 0.f && eB >= fmaxf(fmaxf(mA3, mV), mB2);
                const uint64_t m = __ballot(cand);
                if (m) {
                    if (cand) kbuf[nbuf + lane_prefix(m)] = ((uint64_t)fkey(eB) << 32) | (uint32_t)(rn * W + c);
                    nbuf += __popcll(m);
                    if (nbuf > E3_CAP - 64) flush();
                }
            }
            mA3 = fmaxf(mB2, eB);
            mB2 = mV2;
            eB = v;
            alB = al;
        } else {
            int lo, hi;
            e3_interval(T, dd, sxy, scf, epk, lo, hi);
            const int nV2 = dpp_max_lr(lo), nV2H = dpp_max_lr(hi);
            if (ST || (rn >= o0 && rn < o1)) {
                // a pixel of row r-1 can be a maximum only if its upper bound is positive and reaches
                // every neighbour's lower bound (hi < a neighbour's lo means v < that neighbour's
                // v); it is one for any v > 0 if its lower bound reaches every neighbour's upper
                // bound.  All eight neighbours of an NMS pixel are inside the image.
                const int nlo = max(max(nA3, max(nV2, lo)), nB2);
                const int nhi = max(max(nA3H, max(nV2H, hi)), nB2H);
                const bool poss = nms_col && hiB > 0 && hiB >= nlo;
                push(poss || edge_col, rn, edge_col ? E3_Q_MAXONLY : (loB >= nhi ? E3_Q_DECIDED : 0), TB, dB, sB);
            } else if (rn >= y0 && rn < m1) {
                push(own, rn, E3_Q_MAXONLY, TB, dB, sB);         // image row 0
            }
            nA3 = max(nB2, loB);
            nA3H = max(nB2H, hiB);
            nB2 = nV2;
            nB2H = nV2H;
            loB = lo;
            hiB = hi;
            TB = T; dB = dd; sB = sxy;
        }
    };
    // image rows are loaded E3_PF rows ahead of their use (a register ring: pf[k] holds row
    // ir + k), so the row loop does not wait a full memory round trip per row
    constexpr int E3_PF = 8;
    static_assert(E3_PF < VO_BORDER, "the ring reads up to E3_PF rows below the image");
    int hsA = 0, hdA = 0, hsB = 0, hdB = 0;              // Sobel row terms of image rows ir-2, ir-1
    int xA = 0, yA = 0, zA = 0, xB = 0, yB = 0, zB = 0;  // box row sums (xx, xy, yy) of rows pr-2, pr-1
    int pf[E3_PF];
    const int ir_end = g1 + 1;
#pragma unroll
    for (int k = 0; k < E3_PF; ++k) pf[k] = load_row(min(g0 - 1 + k, ir_end));
    // image row ir (pixels iv): its Sobel row terms, the box row sums of gradient row pr = ir-1,
    // eigen row pr-1.  ST: none of the tile's or the image's first / last rows is involved, so
    // the row carries no test of them.
    auto row = [&](int ir, int iv, auto st) {
        constexpr bool ST = decltype(st)::value;
        const int il = dpp_from_left(iv), irt = dpp_from_right(iv);
        const int hs = il + 2 * iv + irt, hd = irt - il;
        if (ST || ir >= g0 + 1) {
            const int pr = ir - 1;                       // gradient row
            const int gx = hdA + 2 * hdB + hd, gy = hs - hsA;
            // |gx|, |gy| <= 4 * 255: 24-bit multiplies (full rate; v_mul_lo_u32 is quarter rate)
            const int pxx = __mul24(gx, gx), pxy = __mul24(gx, gy), pyy = __mul24(gy, gy);
            int lxx = dpp_from_left(pxx), lxy = dpp_from_left(pxy), lyy = dpp_from_left(pyy);
            int rxx = dpp_from_right(pxx), rxy = dpp_from_right(pxy), ryy = dpp_from_right(pyy);
            if (hedge) {                                 // boxFilter BORDER_REFLECT_101 in x
                if (c == 0) { lxx = rxx; lxy = rxy; lyy = ryy; }
                if (c == W - 1) { rxx = lxx; rxy = lxy; ryy = lyy; }
            }
            const int hx = lxx + pxx + rxx, hy = lxy + pxy + rxy, hz = lyy + pyy + ryy;
            const int r = pr - 1;                        // eigen row
            if constexpr (ST) {
                eig_row(r, xA, yA, zA, xB, yB, zB, hx, hy, hz, st);
            } else {
                if (r >= e0) {
                    const bool top = r == 0;             // BORDER_REFLECT_101 in y: row -1 is row 1
                    eig_row(r, top ? hx : xA, top ? hy : yA, top ? hz : zA, xB, yB, zB, hx, hy, hz, st);
                }
                if (pr == H - 1 && pr >= e0 && pr >= 1) {    // last image row: row H is row H-2
                    eig_row(pr, xB, yB, zB, hx, hy, hz, xB, yB, zB, st);
                    if constexpr (!EXACT)
                        if (pr < m1) push(own, pr, E3_Q_MAXONLY, TB, dB, sB);
                }
            }
            xA = xB; yA = yB; zA = zB;
            xB = hx; yB = hy; zB = hz;
        }
        hsA = hsB; hdA = hdB;
        hsB = hs; hdB = hd;
    };
    // one row with every edge test, the ring shifted by one: the tile's first and last rows
    auto edge_row = [&](int ir) {
        const int iv = pf[0];
#pragma unroll
        for (int k = 0; k + 1 < E3_PF; ++k) pf[k] = pf[k + 1];
        pf[E3_PF - 1] = load_row(min(ir + E3_PF, ir_end));       // past the end: a row never used
        row(ir, iv, std::false_type());
    };
    // steady rows [s_lo, s_hi + E3_PF): the NMS row ir-3 is an NMS row of this tile, the gradient
    // row ir-1 is above the image's last row and ir <= ir_end, for all E3_PF rows of a group
    const int s_lo = o0 + 3, s_hi = min(min(o1 - (E3_PF - 3), H - E3_PF), ir_end - (E3_PF - 1));
    int ir = g0 - 1;
    // a tile too short for one steady group runs as edge rows only.  (The steady loop is entered
    // without a test of its own: a path around it that carries the row state costs the
    // registers that keep 8 waves per SIMD.)
    if (s_lo <= s_hi) {
        for (; ir < s_lo; ++ir) edge_row(ir);            // queues one row at most (image row 0)
        // groups of E3_PF rows, unrolled: ring slot u holds row ir + u, and the row registers
        // (A / B rings) are renamed instead of moved every row
        do {
#pragma unroll
            for (int u = 0; u < E3_PF; ++u) {
                const int iv = pf[u];
                pf[u] = load_row(ir + u + E3_PF);        // <= ir_end + E3_PF <= H + 8: a border row
                row(ir + u, iv, std::true_type());
            }
            ir += E3_PF;
            if constexpr (!EXACT) {
                if (nq >= 64 || ovf) {
                    // the ring is loaded again after the batches instead of living through them:
                    // the batch code has the registers
                    service(64);
#pragma unroll
                    for (int k = 0; k < E3_PF; ++k) pf[k] = load_row(min(ir + k, ir_end));
                }
            }
        } while (ir <= s_hi);
    }
    // the remaining rows; the interval form empties its queue as it goes, and fully at the end
    for (;;) {
        const bool more = ir <= ir_end;
        if (more) edge_row(ir++);
        if constexpr (!EXACT) {
            if (nq >= (more ? 64 : 1) || ovf) {
                service(more ? 64 : 1);
#pragma unroll
                for (int k = 0; k < E3_PF; ++k) pf[k] = load_row(min(ir + k, ir_end));
            }
        }
        if (!more) break;
    }
    if constexpr (EXACT)
        if (out && nbuf) flush();
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t t2 = __shfl_xor(kmax, o, 64);
        kmax = t2 > kmax ? t2 : kmax;
    }
    if (lane == 0 && kmax) atomicMax(&P.eig_max[b], kmax);
}

}  // namespace

// ======================================================================= host side
// eigen + NMS pass: the row-streaming k_eig3 for blockSize 3 / min-eigenvalue (every
// reference configuration), the tiled k_eignms otherwise (or with VO_EIG_GENERIC=1).  k_eig3
// decides the NMS on f32 intervals and evaluates the double expression for the possible maxima
// only; with the eigen map asked for, no key list, or VO_EIG_EXACT=1 it evaluates every pixel.
static void launch_eig(EigParamsM E, hipStream_t st)
{
    static const int generic = vo_env_int("VO_EIG_GENERIC", 0);
    static const int exact = vo_env_int("VO_EIG_EXACT", 0);
    if (E.bs == 3 && !E.harris && !generic) {
        E.tiles_x = (E.W + E3_OUT - 1) / E3_OUT;
        E.tiles_y = (E.H + E3_TH - 1) / E3_TH;
        const int total = E.B * E.tiles_x * E.tiles_y;
        const dim3 grid(((total + 7) / 8) * 8);
        const bool ex = E.eig_out || !E.keys || exact;
        if (E.mask) {
            hipLaunchKernelGGL((k_eig3<true, true>), grid, dim3(64), 0, st, E);      // every pixel evaluated
        } else if (ex) {
            hipLaunchKernelGGL(k_eig3<true>, grid, dim3(64), 0, st, (EigParams)E);
        } else {
            hipLaunchKernelGGL(k_eig3<false>, grid, dim3(64), 0, st, (EigParams)E);
        }
        return;
    }
    const int total = E.B * E.tiles_x * E.tiles_y;
    if (E.mask) hipLaunchKernelGGL(k_eignms<true>, dim3(((total + 7) / 8) * 8), dim3(256), 0, st, E);
    else hipLaunchKernelGGL(k_eignms<false>, dim3(((total + 7) / 8) * 8), dim3(256), 0, st, (EigParams)E);
}

// what both eigen passes share: level 0 of pyramid `cur`, the detector's options and the tiling;
// the caller sets the outputs (keys / nkeys / ccap, chain_status, eig_out)
static void fill_eig(EigParamsM& E, const vo_dims* d, const vo_opts* o, const vo_state* s, int cur)
{
    E.pyr = s->pyr[cur]; E.pstride = d->pyr_stride; E.W = d->W; E.H = d->H; E.pitch = d->lvl_pitch[0];
    E.off = d->lvl_off[0]; E.bs = o->feature_block_size; E.harris = o->feature_use_harris; E.harris_k = o->harris_k;
    E.eig_max = s->eig_max;
    E.B = d->B; E.tiles_x = (d->W + EIG_TW - 1) / EIG_TW; E.tiles_y = (d->H + EIG_TH - 1) / EIG_TH;
    E.mask = nullptr; E.mstride = 0; E.mpitch = 0;
}

// what the entry points share: the argument checks, the per-call zeroing and the eigen pass, which
// leaves the key list (`keys`) or else the eigen map; VO_OK once it is launched
static int eig_pass(const vo_dims* d, const vo_opts* o, const vo_state* s, int cur, bool keys, const uint8_t* mask,
                    int64_t mask_stride, int32_t mask_pitch, hipStream_t st)
{
    if (!d || !o || !s || cur < 0 || cur > 1) return VO_EARG;
    if (o->feature_block_size < 1 || o->feature_block_size > EIG_MAXBS) return VO_EARG;
    if (mask && (mask_pitch < d->W || mask_stride < 0)) return VO_EARG;
    if (hipMemsetAsync(s->eig_max, 0, sizeof(uint32_t) * d->B, st) != hipSuccess) return VO_EHIP;
    if (keys && hipMemsetAsync(s->gf_n, 0, sizeof(int32_t) * d->B, st) != hipSuccess) return VO_EHIP;
    EigParamsM E;
    fill_eig(E, d, o, s, cur);
    E.keys = keys ? s->gf_keys : nullptr; E.nkeys = keys ? s->gf_n : nullptr; E.ccap = keys ? d->ccap : 0;
    E.chain_status = keys ? s->status : nullptr;
    E.eig_out = keys ? nullptr : s->eig;
    if (mask) { E.mask = mask; E.mstride = mask_stride; E.mpitch = mask_pitch; }
    launch_eig(E, st);
    return VO_OK;
}

extern "C" int vo_gftt_eigmap(const vo_dims* d, const vo_opts* o, const vo_state* s, int cur, vo_stream_t stream)
{
    const int rc = eig_pass(d, o, s, cur, false, nullptr, 0, 0, VO_STREAM(stream));
    return rc != VO_OK ? rc : hip_rc();
}

extern "C" int vo_gftt_keys(const vo_dims* d, const vo_opts* o, const vo_state* s, int cur, vo_stream_t stream)
{
    const int rc = eig_pass(d, o, s, cur, true, nullptr, 0, 0, VO_STREAM(stream));
    return rc != VO_OK ? rc : hip_rc();
}

extern "C" int vo_gftt(const vo_dims* d, const vo_opts* o, const vo_state* s, int cur, vo_stream_t stream)
{
    return vo_gftt_masked(d, o, s, cur, nullptr, 0, 0, stream);
}

extern "C" int vo_gftt_masked(const vo_dims* d, const vo_opts* o, const vo_state* s, int cur, const uint8_t* mask,
                              int64_t mask_stride, int32_t mask_pitch, vo_stream_t stream)
{
    const int rc = eig_pass(d, o, s, cur, true, mask, mask_stride, mask_pitch, VO_STREAM(stream));
    return rc != VO_OK ? rc : vo_gftt_select(d, o, s, VO_STREAM(stream));
}
