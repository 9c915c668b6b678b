// goodFeaturesToTrack for gfx950: integer-exact min-eigenvalue (or Harris) map with 3x3 NMS, then
// the selection in one of two forms -- paged radix-select + LDS bitonic sort + wave-parallel
// greedy min-distance walk in one block per chain (k_gftt_select), or split over several small
// launches (k_gsel_*).
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

// ---------------------------------------------------------------- GFTT selection
#define SEL_THREADS 512
#define PAGE 4096
#define ACC_MAX 8192
#define GRID_LDS_CELLS 22528

struct SelParams {
    uint64_t* keys;
    int32_t* nkeys;          // in: local maxima appended; out: how many passed the quality gate
    const uint32_t* eig_max;
    double quality;
    int ccap, W, H;
    int max_corners;
    double min_dist;
    float* corners;
    int32_t* ncorners;
    int mcap;
    uint32_t* gscratch;      // per-chain L2 grid when the LDS grid is too small ([B][W*H] u32)
    int acc_lds;             // accepted-corner slots in LDS (min(mcap, ACC_MAX))
    int grid_lds;            // grid cells held in LDS (0: grid in L2)
    int64_t gstride;
    int grid_glb;            // the parallel walk may keep its grid + cell lists in gscratch
    const int32_t* chain_status;
};

// A grid cell holds two accepted-corner indices (u16 each, 0xFFFF = empty, the low slot filled
// first); a third corner of the cell is chained to the high slot's corner in nxt3[] (u16 per
// accepted corner, 0xFFFF = none).  Three is the most: a cell spans cs - 1 <= minDistance - 0.5
// pixels (cs = round(minDistance)), three lattice points pairwise >= minDistance apart fit such a
// square once 1.035 * (cs - 1) >= minDistance (from minDistance 15.5; (16,16) (31,20) (20,31)),
// four need a side >= minDistance.
VO_DEV uint32_t cell_get(bool lds, uint32_t* lg, uint32_t* gg, int c)
{
    // the L2 copy is only written by atomics: read it at agent scope (past the CU's L1)
    return lds ? lg[c] : __hip_atomic_load(&gg[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
VO_DEV int head_get(bool lds, int* lh, int* gh, int c)
{
    return lds ? lh[c] : __hip_atomic_load(&gh[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the parallel walk's L2 grid + cell-list heads sit after the conflict lists in gscratch
#define SEL_GG_OFF (PAGE * 8)
VO_DEV void cell_set(bool lds, uint32_t* lg, uint32_t* gg, int c, uint32_t v)
{
    if (lds) lg[c] = v;
    else atomicExch(&gg[c], v);
}
// visit(id) for every accepted corner of a cell value
template <class F>
VO_DEV void cell_each(uint32_t cv, const uint16_t* nxt3, F&& visit)
{
    const uint32_t a = cv & 0xFFFFu, b = cv >> 16;
    if (a == 0xFFFFu) return;
    visit(a);
    if (b == 0xFFFFu) return;
    visit(b);
    const uint32_t c = nxt3[b];
    if (c != 0xFFFFu) visit(c);
}
// accepted corner `pos` into its cell; slot order inside a cell is irrelevant.  Several threads
// may insert into one cell at once: the first two take the slots by CAS, the third finds both
// taken (they never change again) and chains itself to the high slot's corner.
VO_DEV void cell_insert(bool lds, uint32_t* lg, uint32_t* gg, uint16_t* nxt3, int cell, int pos)
{
    uint32_t cur = cell_get(lds, lg, gg, cell);
    for (;;) {
        if ((cur >> 16) != 0xFFFFu) {
            nxt3[cur >> 16] = (uint16_t)pos;
            return;
        }
        const uint32_t nv = ((cur & 0xFFFFu) == 0xFFFFu) ? ((cur & 0xFFFF0000u) | (uint32_t)pos)
                                                        : ((cur & 0xFFFFu) | ((uint32_t)pos << 16));
        const uint32_t prev = lds ? atomicCAS(&lg[cell], cur, nv) : atomicCAS(&gg[cell], cur, nv);
        if (prev == cur) return;
        cur = prev;
    }
}

// hist[dgt] += 1 for every lane with `on` (12-bit digits), as one LDS atomic per distinct digit
// of the wave: peer lanes found with bit-sliced ballots
VO_DEV void wave_hist_add12(int* hist, bool on, int dgt)
{
    uint64_t peers = __ballot(on);
#pragma unroll
    for (int bit = 0; bit < 12; ++bit) {
        const bool b = (dgt >> bit) & 1;
        const uint64_t bm = __ballot(b);
        peers &= b ? bm : ~bm;
    }
    if (on && __ffsll((unsigned long long)peers) - 1 == lane_id()) atomicAdd(&hist[dgt], __popcll(peers));
}


#ifdef VO_SELECT_PROF
__device__ long long g_selprof[16];
}  // namespace
// diagnostics build only (libvo_hip_selprof.so, tools/sel_prof.py): block 0's phase timestamps
// of the last k_gftt_select launch (100 MHz wall clock)
extern "C" int vo_select_prof_read(long long* out)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_selprof), sizeof(long long) * 16) == hipSuccess ? 0 : -2;
}
namespace {
#define SELPROF(i) do { if (threadIdx.x == 0 && blockIdx.x == 0) g_selprof[i] = wall_clock64(); } while (0)
#else
#define SELPROF(i) do { } while (0)
#endif

template <int NT>
__global__ void __launch_bounds__(NT) k_gftt_select(SelParams P)
{
    // dynamic LDS sized by the host (vo_gftt): page | candidate xy | accepted xy | grid + cell
    // heads (if they fit) | two conflict slots per candidate | third-corner links of the cells
    extern __shared__ uint64_t sel_dyn[];
    uint64_t* page = sel_dyn;
    uint32_t* cand_xy = (uint32_t*)(sel_dyn + PAGE);
    uint32_t* acc_xy = cand_xy + PAGE;
    uint32_t* lgrid = acc_xy + P.acc_lds;
    int* head = (int*)(lgrid + P.grid_lds);
    // each candidate's first two earlier conflicts, in LDS (most have at most two); the rest of
    // its list (up to CONF_K) is in the per-chain global scratch
    uint16_t* cf2 = (uint16_t*)(head + P.grid_lds);
    uint16_t* nxt3 = cf2 + 2 * PAGE;
    __shared__ uint32_t round_xy[64];
    __shared__ int sh_int[16];
    __shared__ int sh_scan[16];
    __shared__ uint64_t sh_u64[4];
    const int b = blockIdx.x;
    if (P.chain_status[b] != 0) return;
    const int tid = threadIdx.x;
    SELPROF(0);
    const int nk_all = P.nkeys[b];
    if (nk_all > P.ccap) {
        if (tid == 0) P.ncorners[b] = -1;          // capacity: k_add_finish raises it
        return;
    }
    // quality gate of goodFeaturesToTrack: v > quality * max(eig)  (featureselect.cpp);
    // ordered in-place compaction of the passing keys
    uint64_t* keys = P.keys + (int64_t)b * P.ccap;
    const float thr = (float)((double)fkey_inv(P.eig_max[b]) * P.quality);
    const uint64_t lo = ((uint64_t)fkey(thr) + 1ull) << 32;
    int nk = 0;
    // eight consecutive keys per thread per pass (one block scan per 8 * NT keys); every key of
    // a pass is read before the scan's barrier, and writes never pass a later pass's reads
    constexpr int KPT = 8;
    for (int base = 0; base < nk_all; base += NT * KPT) {
        const int i0 = base + tid * KPT;
        uint64_t kk[KPT];
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            kk[j] = i0 + j < nk_all ? keys[i0 + j] : 0ull;
            cnt += (i0 + j < nk_all && kk[j] >= lo) ? 1 : 0;
        }
        int tot;
        int pos = nk + block_scan_i32(cnt, sh_int, &tot);
#pragma unroll
        for (int j = 0; j < KPT; ++j)
            if (i0 + j < nk_all && kk[j] >= lo) keys[pos++] = kk[j];
        nk += tot;
    }
    __syncthreads();
    SELPROF(1);
    if (tid == 0) P.nkeys[b] = nk;
    const double md = P.min_dist;
    const bool use_grid = md >= 1;
    const int cs = use_grid ? __double2int_rn(md) : 1;
    const int gw = (P.W + cs - 1) / cs, gh = (P.H + cs - 1) / cs;
    const double md2 = md * md;
    const int want = P.max_corners > 0 ? P.max_corners : 0x7FFFFFFF;
    const int cap = P.mcap < P.acc_lds ? P.mcap : P.acc_lds;
    const int limit = want < cap ? want : cap;
    const bool lds = (int64_t)gw * gh <= P.grid_lds;
    // parallel walk: grid in LDS, or (P.grid_glb) grid + cell-list heads in gscratch
    const bool par = use_grid && (lds || P.grid_glb);
    uint32_t* gg = P.gscratch + (int64_t)b * P.gstride + (lds || !P.grid_glb ? 0 : SEL_GG_OFF);
    int* ghead = (int*)(gg + gw * gh);
    if (use_grid) {
        for (int q = tid; q < gw * gh; q += blockDim.x) cell_set(lds, lgrid, gg, q, 0xFFFFFFFFu);
        if (par && !lds)
            for (int q = tid; q < gw * gh; q += blockDim.x) atomicExch(&ghead[q], -1);
        for (int q = tid; q < P.acc_lds; q += blockDim.x) nxt3[q] = 0xFFFFu;
    }
    float* out = P.corners + (int64_t)b * P.mcap * 2;
    int nacc = 0;
    bool has_upper = false;
    uint64_t upper = 0;
    int remaining = nk;
    __syncthreads();
    while (remaining > 0 && nacc < limit) {
        // ---- this page: the min(PAGE, remaining) largest keys below `upper`
        uint64_t thr = 0;
        const int take = remaining < PAGE ? remaining : PAGE;
        if (remaining > PAGE) {
            // radix select of the PAGE-th largest key, 12-bit digits (histogram in the page
            // buffer, free until the gather): usually three passes over the keys instead of eight
            uint64_t prefix = 0, mask = 0;
            int k = PAGE;
            int* hist4 = (int*)page;
            for (int shift = 52; shift >= -8; shift -= 12) {
                const int sh = shift < 0 ? 0 : shift;                      // last digit: bits 3..0
                const int dbits = shift < 0 ? 4 : 12;
                const uint64_t dmask = ((uint64_t)1 << dbits) - 1;
                for (int q = tid; q < 4096; q += NT) hist4[q] = 0;
                __syncthreads();
                for (int i0 = tid; i0 < nk; i0 += 4 * NT) {
                    uint64_t kk[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) kk[u] = i0 + u * NT < nk ? keys[i0 + u * NT] : 0ull;
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const bool on = i0 + u * NT < nk && (!has_upper || kk[u] < upper) && (kk[u] & mask) == prefix;
                        wave_hist_add12(hist4, on, (int)((kk[u] >> sh) & dmask));
                    }
                }
                __syncthreads();
                // the digit holding the k-th largest: descending digit order over the threads,
                // NT / 4096-bin slices, one block scan
                constexpr int BPT = 4096 / NT;
                const int hi = 4095 - tid * BPT;
                int loc = 0;
#pragma unroll
                for (int j = 0; j < BPT; ++j) loc += hist4[hi - j];
                int tot;
                const int before = block_scan_i32(loc, sh_scan, &tot);
                if (before < k && k <= before + loc) {
                    int cum = before;
                    for (int j = 0; j < BPT; ++j) {
                        const int h = hist4[hi - j];
                        if (cum + h >= k) {
                            sh_u64[0] = prefix | ((uint64_t)(hi - j) << sh);
                            sh_int[0] = k - cum;
                            sh_int[1] = h;
                            break;
                        }
                        cum += h;
                    }
                }
                __syncthreads();
                prefix = sh_u64[0];
                k = sh_int[0];
                const int in_bucket = sh_int[1];
                mask |= dmask << sh;
                __syncthreads();
                if (in_bucket == k) break;          // the whole bucket is in: prefix (low bits 0) is the threshold
            }            thr = prefix;
        }
        if (tid == 0) sh_int[1] = 0;
        __syncthreads();
        for (int i0 = tid; i0 < nk; i0 += 4 * NT) {
            uint64_t kk[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) kk[u] = i0 + u * NT < nk ? keys[i0 + u * NT] : 0ull;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                // page order is irrelevant (sorted next): one LDS atomic per wave
                const bool on = i0 + u * NT < nk && (!has_upper || kk[u] < upper) && kk[u] >= thr;
                const uint64_t m = __ballot(on);
                if (m == 0) continue;
                const int leader = __ffsll((unsigned long long)m) - 1;
                int base = 0;
                if (lane_id() == leader) base = atomicAdd(&sh_int[1], __popcll(m));
                base = __shfl(base, leader, 64);
                const int pos = base + __popcll(m & ((1ull << lane_id()) - 1ull));
                if (on && pos < PAGE) page[pos] = kk[u];
            }
        }
        __syncthreads();
        for (int i = take + tid; i < PAGE; i += blockDim.x) page[i] = 0;
        __syncthreads();
        SELPROF(2);
        // ---- bitonic sort, descending (value desc, then larger address first)
        for (int size = 2; size <= PAGE; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int i = tid; i < PAGE / 2; i += blockDim.x) {
                    const int lo = 2 * i - (i & (stride - 1));
                    const int hi = lo + stride;
                    const bool desc = ((lo & size) == 0);
                    const uint64_t a = page[lo], c = page[hi];
                    if ((a < c) == desc) { page[lo] = c; page[hi] = a; }
                }
                __syncthreads();
            }
        }
        SELPROF(3);
        const uint64_t page_last = page[take - 1];
        if (par) {
            // ---- exact parallel form of OpenCV's sequential minDistance walk.  Candidate i
            // (rank order) is accepted iff no earlier accepted candidate in its 3x3 cell
            // neighbourhood is closer than minDistance, and no corner accepted on an earlier
            // page is.  Decisions only depend on earlier candidates, so they are resolved in
            // parallel rounds (each round decides at least the lowest undecided candidate);
            // the first `limit` accepted in rank order are the corners.
            for (int i = tid; i < take; i += blockDim.x) {
                const uint32_t addr = (uint32_t)page[i];
                const int y = (int)(addr / (uint32_t)P.W), x = (int)(addr - (uint32_t)y * P.W);
                cand_xy[i] = (uint32_t)x | ((uint32_t)y << 16);
            }
            // candidates by cell: with the grid in LDS, a counting sort (head[] = counts, then
            // start offsets; nxt[] = the candidate indices cell by cell), so a cell's candidates
            // are read with independent loads; otherwise linked lists in the L2 grid
            const int ncell = gw * gh;
            if (lds)
                for (int q = tid; q < ncell; q += blockDim.x) head[q] = 0;
            __syncthreads();
            int* nxt = (int*)page;                                // page keys are dead now
            volatile uint8_t* stt = (volatile uint8_t*)(nxt + PAGE);
            constexpr int CPT = PAGE / NT;                        // candidates per thread
            int slot[CPT];
#pragma unroll
            for (int kq = 0; kq < CPT; ++kq) {
                const int i = tid + kq * NT;
                if (i >= take) break;
                const uint32_t xy = cand_xy[i];
                const int x = (int)(xy & 0xFFFF), y = (int)(xy >> 16);
                const int xc = x / cs, yc = y / cs;
                bool rej = false;
                if (nacc > 0) {
                    const int x1 = max(xc - 1, 0), y1 = max(yc - 1, 0);
                    const int x2 = min(xc + 1, gw - 1), y2 = min(yc + 1, gh - 1);
                    for (int yy = y1; yy <= y2; ++yy)
                        for (int xx = x1; xx <= x2; ++xx) {
                            cell_each(cell_get(lds, lgrid, gg, yy * gw + xx), nxt3, [&](uint32_t id) {
                                const uint32_t aa = acc_xy[id];
                                const float ddx = (float)x - (float)(aa & 0xFFFF);
                                const float ddy = (float)y - (float)(aa >> 16);
                                if ((double)(ddx * ddx + ddy * ddy) < md2) rej = true;
                            });
                        }
                }
                stt[i] = rej ? 2 : 0;                             // 0 undecided, 1 accepted, 2 rejected
                if (lds) slot[kq] = atomicAdd(&head[yc * gw + xc], 1);
                else nxt[i] = atomicExch(&ghead[yc * gw + xc], i);
            }
            __syncthreads();
            if (lds) {
                // exclusive scan of the cell counts in place, then the cell-ordered index array
                const int cpt = (ncell + NT - 1) / NT, q0 = tid * cpt, q1 = min(q0 + cpt, ncell);
                int sum = 0;
                for (int q = q0; q < q1; ++q) sum += head[q];
                int tot;
                int run = block_scan_i32(sum, sh_int, &tot);
                for (int q = q0; q < q1; ++q) {
                    const int cnt = head[q];
                    head[q] = run;
                    run += cnt;
                }
                __syncthreads();
#pragma unroll
                for (int kq = 0; kq < CPT; ++kq) {
                    const int i = tid + kq * NT;
                    if (i >= take) break;
                    const uint32_t xy = cand_xy[i];
                    nxt[head[((int)(xy >> 16) / cs) * gw + (int)(xy & 0xFFFF) / cs] + slot[kq]] = i;
                }
                __syncthreads();
            }
            // visit(j) for every candidate j in cell cc, until it returns true
            auto for_cell = [&](int cc, auto&& visit) {
                if (lds) {
                    const int e0 = cc + 1 < ncell ? head[cc + 1] : take;
                    for (int k = head[cc]; k < e0; ++k)
                        if (visit(nxt[k])) return true;
                } else {
                    for (int j = head_get(false, head, ghead, cc); j >= 0; j = nxt[j])
                        if (visit(j)) return true;
                }
                return false;
            };
            // each candidate's earlier conflicts (same test as OpenCV's walk), found once:
            // count in LDS, indices in the per-chain scratch (the eigen-map buffer, unused on
            // this path); more than CONF_K conflicts, or a candidate past the lists the scratch
            // has room for (an image of fewer than 8 * PAGE pixels) -> rescan the cells in every round
            constexpr int CONF_K = 16;
            uint16_t* conf = (uint16_t*)(P.gscratch + (int64_t)b * P.gstride);
            const int conf_cap = (int)min((int64_t)PAGE, P.gstride * 2 / CONF_K);
            uint8_t* ncf = (uint8_t*)(nxt + PAGE) + PAGE;          // PAGE bytes after stt
            for (int i = tid; i < take; i += blockDim.x) {
                if (stt[i] != 0) { ncf[i] = 0; continue; }
                const uint32_t xy = cand_xy[i];
                const int x = (int)(xy & 0xFFFF), y = (int)(xy >> 16);
                const int xc = x / cs, yc = y / cs;
                const int x1 = max(xc - 1, 0), y1 = max(yc - 1, 0);
                const int x2 = min(xc + 1, gw - 1), y2 = min(yc + 1, gh - 1);
                int c = 0;
                for (int yy = y1; yy <= y2; ++yy)
                    for (int xx = x1; xx <= x2; ++xx)
                        for_cell(yy * gw + xx, [&](int j) {
                            if (j >= i) return false;
                            const uint32_t aa = cand_xy[j];
                            const float ddx = (float)x - (float)(aa & 0xFFFF);
                            const float ddy = (float)y - (float)(aa >> 16);
                            if ((double)(ddx * ddx + ddy * ddy) < md2) {
                                if (c < 2) cf2[2 * i + c] = (uint16_t)j;
                                if (c < CONF_K && i < conf_cap) conf[(int64_t)i * CONF_K + c] = (uint16_t)j;
                                ++c;
                            }
                            return false;
                        });
                ncf[i] = (uint8_t)((c > 2 && i >= conf_cap) ? 255 : min(c, 255));
            }
            __syncthreads();
            SELPROF(5);
            for (;;) {
                if (tid == 0) sh_int[3] = 0;
                __syncthreads();
                bool changed = false;
                for (int i = tid; i < take; i += blockDim.x) {
                    if (stt[i] != 0) continue;
                    bool blocked = false, rej = false;
                    const int c = ncf[i];
                    if (c <= 2) {
                        for (int k = 0; k < c; ++k) {
                            const uint8_t sj = stt[cf2[2 * i + k]];
                            if (sj == 1) { rej = true; break; }
                            if (sj == 0) blocked = true;
                        }
                    } else if (c <= CONF_K) {
                        for (int k = 0; k < c; ++k) {
                            const uint8_t sj = stt[conf[(int64_t)i * CONF_K + k]];
                            if (sj == 1) { rej = true; break; }
                            if (sj == 0) blocked = true;
                        }
                    } else {
                        const uint32_t xy = cand_xy[i];
                        const int x = (int)(xy & 0xFFFF), y = (int)(xy >> 16);
                        const int xc = x / cs, yc = y / cs;
                        const int x1 = max(xc - 1, 0), y1 = max(yc - 1, 0);
                        const int x2 = min(xc + 1, gw - 1), y2 = min(yc + 1, gh - 1);
                        for (int yy = y1; yy <= y2 && !rej; ++yy)
                            for (int xx = x1; xx <= x2 && !rej; ++xx)
                                for_cell(yy * gw + xx, [&](int j) {
                                    if (j >= i) return false;
                                    const uint8_t sj = stt[j];
                                    if (sj == 2) return false;
                                    const uint32_t aa = cand_xy[j];
                                    const float ddx = (float)x - (float)(aa & 0xFFFF);
                                    const float ddy = (float)y - (float)(aa >> 16);
                                    if ((double)(ddx * ddx + ddy * ddy) < md2) {
                                        if (sj == 1) { rej = true; return true; }
                                        blocked = true;
                                    }
                                    return false;
                                });
                    }
                    if (rej) { stt[i] = 2; changed = true; }
                    else if (!blocked) { stt[i] = 1; changed = true; }
                }
                if (changed) sh_int[3] = 1;
                __syncthreads();
                const int any = sh_int[3];
                __syncthreads();
#ifdef VO_SELECT_PROF
                if (tid == 0 && blockIdx.x == 0) g_selprof[10]++;
#endif
                if (!any) break;
            }
            SELPROF(6);
            // accepted candidates in rank order -> corners (up to limit) and the grid
            for (int base = 0; base < take && nacc < limit; base += blockDim.x) {
                const int i = base + tid;
                const bool acc = i < take && stt[i] == 1;
                int tot;
                const int pos = nacc + block_scan_flag(acc, sh_int, &tot);
                if (acc && pos < limit) {
                    const uint32_t xy = cand_xy[i];
                    const int x = (int)(xy & 0xFFFF), y = (int)(xy >> 16);
                    acc_xy[pos] = xy;
                    out[2 * pos] = (float)x;
                    out[2 * pos + 1] = (float)y;
                    cell_insert(lds, lgrid, gg, nxt3, (y / cs) * gw + (x / cs), pos);
                }
                nacc = min(nacc + tot, limit);
            }
            if (!lds) {
                // empty the cell lists this page used (the next page rebuilds them)
                for (int i = tid; i < take; i += blockDim.x) {
                    const uint32_t xy = cand_xy[i];
                    atomicExch(&ghead[((int)(xy >> 16) / cs) * gw + (int)(xy & 0xFFFF) / cs], -1);
                }
            }
            if (tid == 0) sh_int[2] = nacc;
        } else {
        // ---- greedy selection by wave 0, 64 candidates per round in sorted order.
            // A candidate survives if no accepted corner in the 3x3 neighbouring cells is closer
            // than minDistance (OpenCV's grid test).  Within a round, lane i additionally needs
            // every earlier accepted lane j < i of the round to pass the same test; the lanes
            // form a conflict mask against earlier tentative lanes, and wave-uniform scalar code
            // walks the tentative lanes in order to pick the accepted set -- exactly OpenCV's
            // sequential walk, without a ballot/shuffle round trip per accepted corner.
            if (wave_id() == 0) {
                const int lane = lane_id();
                for (int s0 = 0; s0 < take && nacc < limit; s0 += 64) {
                    const int i = s0 + lane;
                    bool tent = i < take;
                    int x = 0, y = 0;
                    if (tent) {
                        const uint32_t addr = (uint32_t)page[i];
                        y = (int)(addr / (uint32_t)P.W);
                        x = (int)(addr - (uint32_t)y * P.W);
                    }
                    const int xc = x / cs, yc = y / cs;
                    if (tent && use_grid) {
                        const int x1 = max(xc - 1, 0), y1 = max(yc - 1, 0);
                        const int x2 = min(xc + 1, gw - 1), y2 = min(yc + 1, gh - 1);
                        for (int yy = y1; yy <= y2 && tent; ++yy)
                            for (int xx = x1; xx <= x2 && tent; ++xx) {
                                cell_each(cell_get(lds, lgrid, gg, yy * gw + xx), nxt3, [&](uint32_t id) {
                                    const uint32_t a = acc_xy[id];
                                    const float ddx = (float)x - (float)(a & 0xFFFF);
                                    const float ddy = (float)y - (float)(a >> 16);
                                    if ((double)(ddx * ddx + ddy * ddy) < md2) tent = false;
                                });
                            }
                    }
                    const uint64_t tmask = __ballot(tent);
                    if (tmask == 0) continue;
                    uint64_t amask = tmask;
                    if (use_grid) {
                        // conflicts with earlier tentative lanes of this round
                        round_xy[lane] = (uint32_t)x | ((uint32_t)y << 16);
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                        uint32_t clo = 0, chi = 0;
                        uint64_t rest = tmask & ((1ull << lane) - 1ull) & (tent ? ~0ull : 0ull);
                        // uniform walk over the tentative lanes; each lane keeps the earlier ones
                        for (uint64_t m = tmask; m; m &= m - 1) {
                            const int j = __builtin_ctzll(m);
                            if (!((rest >> j) & 1ull)) continue;
                            const uint32_t a = round_xy[j];
                            const int tx = (int)(a & 0xFFFF), ty = (int)(a >> 16);
                            if (abs(tx / cs - xc) <= 1 && abs(ty / cs - yc) <= 1) {
                                const float ddx = (float)x - (float)tx, ddy = (float)y - (float)ty;
                                if ((double)(ddx * ddx + ddy * ddy) < md2) {
                                    if (j < 32) clo |= 1u << j; else chi |= 1u << (j - 32);
                                }
                            }
                        }
                        // in-order resolution on scalar registers
                        amask = 0;
                        for (uint64_t m = tmask; m; m &= m - 1) {
                            const int j = __builtin_ctzll(m);
                            const uint64_t cj = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)clo, j) |
                                                ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)chi, j) << 32);
                            if ((cj & amask) == 0) amask |= 1ull << j;
                        }
                    }
                    // respect maxCorners: keep the first (limit - nacc) accepted lanes
                    int nnew = __popcll(amask);
                    if (nnew > limit - nacc) {
                        uint64_t m = amask, keep = 0;
                        for (int c = 0; c < limit - nacc; ++c) { const uint64_t lb = m & (~m + 1ull); keep |= lb; m ^= lb; }
                        amask = keep;
                        nnew = limit - nacc;
                    }
                    if ((amask >> lane) & 1ull) {
                        const int idx = nacc + __popcll(amask & ((1ull << lane) - 1ull));
                        acc_xy[idx] = (uint32_t)x | ((uint32_t)y << 16);
                        out[2 * idx] = (float)x;
                        out[2 * idx + 1] = (float)y;
                        if (use_grid) cell_insert(lds, lgrid, gg, nxt3, yc * gw + xc, idx);
                    }
                    nacc += nnew;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                }
                if (lane == 0) sh_int[2] = nacc;
            }
        }
        __syncthreads();
        SELPROF(4);
        nacc = sh_int[2];
        upper = page_last;
        has_upper = true;
        remaining -= take;
        __syncthreads();
    }
    if (tid == 0) {
        // more corners wanted than this engine can hold -> never truncate silently.  The
        // status word is not written here: GFTT runs on a side stream concurrently with PnP,
        // which owns it; k_add_finish turns ncorners < 0 into VO_ST_CAPACITY.
        P.ncorners[b] = (nacc == cap && cap < want && remaining > 0) ? -1 : nacc;
    }
}

// ---------------------------------------------------------------- GFTT selection, split form
// (round 6).  k_gftt_select is one block per chain holding ~110 KB of LDS (C2) and 8-16 waves;
// beside the other stream group's LK flood -- one-wave blocks refilling every wave slot the
// moment it frees -- such a block starts only once a whole CU has drained (headline: 0.7 ms
// alone, 5-6 ms in the step).  The split form does the same selection in five LK-shaped
// launches: one-wave blocks, no LDS except the walk's 1.3 KB, so each block starts in the
// first wave slot that frees.
//   k_gsel_gate     many waves per chain: quality gate v > quality * max (featureselect.cpp),
//                   passing keys appended to the chain's list in any order, and a histogram of
//                   GS_NB value buckets (bucket = (key_max - fkey(v)) >> shift: descending
//                   value order, ~1/512 octave wide at C5);
//   k_gsel_scan     one wave per chain: exclusive scan of the histogram (bucket starts);
//   k_gsel_scatter  many waves per chain: every passing key to its bucket's range;
//   k_gsel_rank     many waves per chain: a key's final place = its bucket's start + the keys of
//                   its bucket larger than it (buckets hold ~1-70 keys: 12 at C2, 66 at C5), so
//                   the list ends fully sorted, descending u64 key = (value desc, then larger
//                   address first) as k_gftt_select's bitonic sort;
//   k_gsel_walk     one wave per chain: OpenCV's sequential minDistance walk over the sorted list,
//                   64 candidates per round (as the wave path of k_gftt_select): the accepted
//                   corners' cell grid holds each corner's offset inside its cell (no corner
//                   table), as u64 cells in the chain's eigen-map scratch; conflicts between the
//                   candidates of one round are found through a 128-entry LDS cell hash of lane
//                   masks (1.3 KB of LDS).
// The corner list is the one k_gftt_select produces (the GFTT parity tests run both forms).
// The split kernels do not read the chain status for their work (GFTT runs concurrently with
// PnP, which may change it mid-way, and the kernels must agree on what the histogram holds);
// only the walk skips writing corners for a chain that is no longer running, as k_gftt_select.
#define GS_NB 4096
#define GS_HASH 128

struct SelSplitParams {
    uint64_t* keys;          // gf_keys [B][ccap]: local maxima (in), then the bucket-grouped keys
    int32_t* nkeys;          // gf_n [B]: local maxima (in); passing keys (out, as k_gftt_select)
    const uint32_t* eig_max;
    double quality;
    int ccap, W, H;
    float invW;
    int want;                // maxCorners, 1 <= want <= mcap
    double md2;              // minDistance^2
    int cs, gw, gh;          // cell size cvRound(minDistance), grid
    uint32_t cs_m;           // ceil(2^32 / cs): x / cs = umulhi(x, cs_m) for x < 2^16
    float* corners;
    int32_t* ncorners;
    int mcap;
    uint64_t* sorted;        // gf_sort [B][sstride]: sorted keys [ccap] | histogram u32[GS_NB] | npass
    int64_t sstride;
    float* ggrid;            // u64 cell grid in the eigen-map scratch, 8-byte aligned
    int64_t gstride;         // floats per chain (W * H)
    int wpc;                 // waves per chain of gate / scatter / rank
    const int32_t* chain_status;
};

// the histogram takes uint4 accesses: its start is rounded up to 16 bytes (an odd ccap, or an odd
// chain stride, leaves the key area's end only 8-byte aligned; the 4096-u64 extra has the room)
VO_DEV uint32_t* gs_hist(const SelSplitParams& P, int b)
{
    return (uint32_t*)(((uintptr_t)(P.sorted + (int64_t)b * P.sstride + P.ccap) + 15) & ~(uintptr_t)15);
}
VO_DEV int32_t* gs_npass(const SelSplitParams& P, int b) { return (int32_t*)(gs_hist(P, b) + GS_NB); }

// the chain's gate and bucket map: keys >= lo pass; bucket(k) = (kmax - (k >> 32)) >> shift
VO_DEV bool gs_range(const SelSplitParams& P, int b, uint64_t& lo, uint32_t& kmax, int& shift)
{
    kmax = P.eig_max[b];
    const float thr = (float)((double)fkey_inv(kmax) * P.quality);
    lo = ((uint64_t)fkey(thr) + 1ull) << 32;
    shift = 0;
    if ((uint64_t)kmax < (lo >> 32)) return false;
    const uint32_t R = kmax - (uint32_t)(lo >> 32);
    const int bits = R ? 32 - __clz(R) : 0;
    shift = bits > 12 ? bits - 12 : 0;
    return true;
}
VO_DEV int gs_bucket(uint64_t k, uint32_t kmax, int shift)
{
    const int q = (int)((kmax - (uint32_t)(k >> 32)) >> shift);
    return q < GS_NB - 1 ? q : GS_NB - 1;
}

__global__ void __launch_bounds__(64) k_gsel_gate(SelSplitParams P)
{
    const int b = blockIdx.x / P.wpc, w = blockIdx.x - b * P.wpc;
    const int nk_all = P.nkeys[b];
    if (nk_all > P.ccap) return;                         // capacity: the walk reports it
    uint64_t lo;
    uint32_t kmax;
    int sh;
    if (!gs_range(P, b, lo, kmax, sh)) return;
    const uint64_t* keys = P.keys + (int64_t)b * P.ccap;
    uint64_t* pass = P.sorted + (int64_t)b * P.sstride;
    uint32_t* hist = gs_hist(P, b);
    int32_t* npass = gs_npass(P, b);
    const int lane = lane_id();
    for (int base = w * 256; base < nk_all; base += P.wpc * 256) {
        uint64_t kk[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + u * 64 + lane;
            kk[u] = i < nk_all ? keys[i] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool on = kk[u] >= lo;                 // 0 (absent) never passes: lo >= 2^32
            const uint64_t m = __ballot(on);
            if (m == 0) continue;
            if (on) __hip_atomic_fetch_add(&hist[gs_bucket(kk[u], kmax, sh)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int leader = __ffsll((unsigned long long)m) - 1;
            int pos = 0;
            if (lane == leader) pos = atomicAdd(npass, __popcll(m));
            pos = __shfl(pos, leader, 64) + __popcll(m & ((1ull << lane) - 1ull));
            if (on) pass[pos] = kk[u];
        }
    }
}

__global__ void __launch_bounds__(64) k_gsel_scan(SelSplitParams P)
{
    const int b = blockIdx.x;
    uint32_t* hist = gs_hist(P, b);
    const int lane = lane_id();
    uint4* h4 = (uint4*)hist + lane * (GS_NB / 256);     // 64 consecutive bins per lane
    // two passes over the lane's bins (read to sum, re-read to write) keep it at <= 64 VGPRs, so
    // the wave fits the slot of one finished LK wave
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < GS_NB / 256; ++j) {
        const uint4 v = h4[j];
        sum += v.x + v.y + v.z + v.w;
    }
    // inclusive wave scan of the lane sums
    uint32_t inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (__ballot(sum != 0) == 0) return;                 // nothing passed (or the chain was skipped)
    uint32_t run = inc - sum;
#pragma unroll
    for (int j = 0; j < GS_NB / 256; ++j) {
        const uint4 v = h4[j];
        uint4 o;
        o.x = run; run += v.x;
        o.y = run; run += v.y;
        o.z = run; run += v.z;
        o.w = run; run += v.w;
        h4[j] = o;
    }
}

__global__ void __launch_bounds__(64) k_gsel_scatter(SelSplitParams P)
{
    const int b = blockIdx.x / P.wpc, w = blockIdx.x - b * P.wpc;
    const int n = *gs_npass(P, b);
    if (n == 0) return;
    uint64_t lo;
    uint32_t kmax;
    int sh;
    gs_range(P, b, lo, kmax, sh);
    const uint64_t* pass = P.sorted + (int64_t)b * P.sstride;
    uint32_t* hist = gs_hist(P, b);
    uint64_t* grouped = P.keys + (int64_t)b * P.ccap;
    for (int i = w * 64 + lane_id(); i < n; i += P.wpc * 64) {
        const uint64_t k = pass[i];
        const uint32_t pos = atomicAdd(&hist[gs_bucket(k, kmax, sh)], 1u);
        grouped[pos] = k;
    }
}

__global__ void __launch_bounds__(64) k_gsel_rank(SelSplitParams P)
{
    const int b = blockIdx.x / P.wpc, w = blockIdx.x - b * P.wpc;
    const int n = *gs_npass(P, b);
    if (n == 0) return;
    uint64_t lo;
    uint32_t kmax;
    int sh;
    gs_range(P, b, lo, kmax, sh);
    const uint32_t* hist = gs_hist(P, b);              // after the scatter: bucket ends
    const uint64_t* grouped = P.keys + (int64_t)b * P.ccap;
    uint64_t* sorted = P.sorted + (int64_t)b * P.sstride;
    for (int i = w * 64 + lane_id(); i < n; i += P.wpc * 64) {
        const uint64_t k = grouped[i];
        const int q = gs_bucket(k, kmax, sh);
        const int st = q ? (int)hist[q - 1] : 0, en = (int)hist[q];
        int cnt = 0;
        for (int j = st; j < en; ++j) cnt += grouped[j] > k ? 1 : 0;
        sorted[st + cnt] = k;
    }
}

// grid cells (u64 in the chain's eigen-map scratch): up to four corners, each stored as 1 + its
// offset inside the cell (ox | oy << 8).  Every access to the grid comes from this one wave, so
// all of them are atomics at workgroup scope (coherent among themselves by the memory model,
// served by the CU's own XCD instead of the device coherence point).  The grid stays out of
// LDS on purpose: beside the LK flood a block waits for a CU with that much LDS free (a 12 KB
// u16 cell table in LDS made the headline's walk 6-10 ms instead of 0.5 ms).
__global__ void __launch_bounds__(64) k_gsel_walk(SelSplitParams P)
{
    __shared__ uint64_t rhash[GS_HASH];
    __shared__ uint32_t rxy[64];
    const int b = blockIdx.x;
    const int lane = lane_id();
    // the histogram and the pass counter are this call's; zero them for the next one
    uint32_t* hist = gs_hist(P, b);
    int32_t* npass = gs_npass(P, b);
    const int n = *npass;
    const int nk_all = P.nkeys[b];
#pragma unroll
    for (int j = 0; j < GS_NB / 256; ++j) ((uint4*)hist)[j * 64 + lane] = make_uint4(0, 0, 0, 0);
    if (P.chain_status[b] != 0) {
        if (lane == 0) *npass = 0;
        return;
    }
    if (nk_all > P.ccap) {
        if (lane == 0) { *npass = 0; P.ncorners[b] = -1; }     // capacity: k_add_finish raises it
        return;
    }
    const int cs = P.cs, gw = P.gw, gh = P.gh, ncell = gw * gh;
    unsigned long long* gg =
        (unsigned long long*)(((uintptr_t)(P.ggrid + (int64_t)b * P.gstride) + 7) & ~(uintptr_t)7);
    for (int q = lane; q < ncell; q += 64) __hip_atomic_store(&gg[q], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    for (int q = lane; q < GS_HASH; q += 64) rhash[q] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const uint64_t* sorted = P.sorted + (int64_t)b * P.sstride;
    float* out = P.corners + (int64_t)b * P.mcap * 2;
    int nacc = 0;
    const int limit = P.want;
    const uint64_t below = (1ull << lane) - 1ull;
    uint64_t knext = lane < n ? sorted[lane] : 0ull;
    for (int s0 = 0; s0 < n && nacc < limit; s0 += 64) {
        const int i = s0 + lane;
        bool tent = i < n;
        const uint32_t addr = (uint32_t)knext;
        knext = i + 64 < n ? sorted[i + 64] : 0ull;         // the next round's keys, in flight
        int y = (int)((float)addr * P.invW);
        y += ((uint32_t)(y + 1) * (uint32_t)P.W <= addr) ? 1 : 0;
        y -= ((uint32_t)y * (uint32_t)P.W > addr) ? 1 : 0;
        const int x = (int)(addr - (uint32_t)y * (uint32_t)P.W);
        const int xc = (int)__umulhi((uint32_t)x, P.cs_m), yc = (int)__umulhi((uint32_t)y, P.cs_m);
        const int x1 = max(xc - 1, 0), y1 = max(yc - 1, 0);
        const int x2 = min(xc + 1, gw - 1), y2 = min(yc + 1, gh - 1);
        // OpenCV's grid test against the corners accepted so far: the (up to) nine cells are
        // loaded together, then tested
        if (tent) {
            unsigned long long cv[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int yy = y1 + k / 3, xx = x1 + k % 3;
                cv[k] = (yy <= y2 && xx <= x2)
                            ? __hip_atomic_load(&gg[yy * gw + xx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
                            : 0ull;
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int yy = y1 + k / 3, xx = x1 + k % 3;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t sl = (uint32_t)(cv[k] >> (16 * q)) & 0xFFFFu;
                    if (sl == 0) break;
                    const int ax = xx * cs + (int)((sl - 1) & 0xFFu), ay = yy * cs + (int)((sl - 1) >> 8);
                    const float ddx = (float)x - (float)ax, ddy = (float)y - (float)ay;
                    if ((double)(ddx * ddx + ddy * ddy) < P.md2) tent = false;
                }
            }
        }
        const uint64_t tmask = __ballot(tent);
        if (tmask == 0) continue;
        // conflicts with earlier candidates of this round: lanes register in a cell hash, each
        // reads the masks of its 3x3 neighbourhood and tests the (rare) earlier lanes exactly
        if (tent) {
            rxy[lane] = (uint32_t)x | ((uint32_t)y << 16);
            atomicOr((unsigned long long*)&rhash[(yc * gw + xc) & (GS_HASH - 1)], 1ull << lane);
        }
        wave_lds_sync();
        uint64_t conf = 0;
        if (tent) {
            uint64_t m = 0;
            for (int yy = y1; yy <= y2; ++yy)
                for (int xx = x1; xx <= x2; ++xx) m |= rhash[(yy * gw + xx) & (GS_HASH - 1)];
            m &= tmask & below;
            for (; m; m &= m - 1) {
                const int j = __builtin_ctzll(m);
                const uint32_t a = rxy[j];
                const int tx = (int)(a & 0xFFFF), ty = (int)(a >> 16);
                const int tcx = (int)__umulhi((uint32_t)tx, P.cs_m), tcy = (int)__umulhi((uint32_t)ty, P.cs_m);
                if (abs(tcx - xc) <= 1 && abs(tcy - yc) <= 1) {
                    const float ddx = (float)x - (float)tx, ddy = (float)y - (float)ty;
                    if ((double)(ddx * ddx + ddy * ddy) < P.md2) conf |= 1ull << j;
                }
            }
        }
        wave_lds_sync();
        if (tent) rhash[(yc * gw + xc) & (GS_HASH - 1)] = 0;
        // in-order resolution: a lane with conflicts is accepted iff none of its earlier
        // conflicting lanes is
        const uint64_t cm = __ballot(conf != 0);
        uint64_t amask = tmask & ~cm;
        for (uint64_t m = cm; m; m &= m - 1) {
            const int j = __builtin_ctzll(m);
            const uint64_t cj = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)conf, j) |
                                ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(conf >> 32), j) << 32);
            if ((cj & amask) == 0) amask |= 1ull << j;
        }
        // maxCorners: the first (limit - nacc) accepted lanes
        int nnew = __popcll(amask);
        if (nnew > limit - nacc) {
            uint64_t m = amask, keep = 0;
            for (int c = 0; c < limit - nacc; ++c) { const uint64_t lb = m & (~m + 1ull); keep |= lb; m ^= lb; }
            amask = keep;
            nnew = limit - nacc;
        }
        if ((amask >> lane) & 1ull) {
            const int idx = nacc + __popcll(amask & below);
            out[2 * idx] = (float)x;
            out[2 * idx + 1] = (float)y;
            // into the first free slot of its cell (two lanes of a round may share a cell); the
            // CAS returns before the wave goes on, so the next round's loads see it
            const unsigned long long code = 1ull + ((unsigned long long)(x - xc * cs) | ((unsigned long long)(y - yc * cs) << 8));
            unsigned long long* cp = &gg[yc * gw + xc];
            unsigned long long cur = __hip_atomic_load(cp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            for (;;) {
                int q = 0;
                while (q < 3 && ((cur >> (16 * q)) & 0xFFFFull)) ++q;
                const unsigned long long nv = cur | (code << (16 * q));
                if (__hip_atomic_compare_exchange_strong(cp, &cur, nv, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_WORKGROUP))
                    break;
            }
        }
        nacc += nnew;
        // one wave: its LDS operations and its returned atomics are complete in issue order; no
        // memory wait here (a fence would wait for the next round's key loads and the corner
        // stores every round)
        wave_lds_sync();
    }
    if (lane == 0) {
        P.ncorners[b] = nacc;
        P.nkeys[b] = n;
        *npass = 0;
    }
}

}  // namespace

// ======================================================================= host side
// GFTT selection form (vo_set_gftt_select): 0 = automatic, 1 = k_gftt_select, 2 = k_gsel_*
static int g_sel_mode = 0;
extern "C" int vo_set_gftt_select(int mode)
{
    if (mode < 0 || mode > 2) return VO_EARG;
    g_sel_mode = mode;
    return VO_OK;
}

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

extern "C" int vo_gftt_eigmap(const vo_dims* d, const vo_opts* o, const vo_state* s, int cur, vo_stream_t stream)
{
    if (!d || !o || !s || cur < 0 || cur > 1) return VO_EARG;
    if (o->feature_block_size < 1 || o->feature_block_size > EIG_MAXBS) return VO_EARG;
    hipStream_t st = VO_STREAM(stream);
    if (hipMemsetAsync(s->eig_max, 0, sizeof(uint32_t) * d->B, st) != hipSuccess) return VO_EHIP;
    EigParamsM E;
    fill_eig(E, d, o, s, cur);
    E.keys = nullptr; E.nkeys = nullptr; E.ccap = 0;
    E.chain_status = nullptr;
    E.eig_out = s->eig;
    launch_eig(E, st);
    return hip_ok() ? VO_OK : VO_EHIP;
}

extern "C" int vo_gftt_keys(const vo_dims* d, const vo_opts* o, const vo_state* s, int cur, vo_stream_t stream)
{
    if (!d || !o || !s || cur < 0 || cur > 1) return VO_EARG;
    if (o->feature_block_size < 1 || o->feature_block_size > EIG_MAXBS) return VO_EARG;
    hipStream_t st = VO_STREAM(stream);
    if (hipMemsetAsync(s->eig_max, 0, sizeof(uint32_t) * d->B, st) != hipSuccess) return VO_EHIP;
    if (hipMemsetAsync(s->gf_n, 0, sizeof(int32_t) * d->B, st) != hipSuccess) return VO_EHIP;
    EigParamsM E;
    fill_eig(E, d, o, s, cur);
    E.keys = s->gf_keys; E.nkeys = s->gf_n; E.ccap = d->ccap;
    E.chain_status = s->status;
    E.eig_out = nullptr;
    launch_eig(E, st);
    return hip_ok() ? VO_OK : VO_EHIP;
}

extern "C" int vo_gftt(const vo_dims* d, const vo_opts* o, const vo_state* s, int cur, vo_stream_t stream)
{
    return vo_gftt_masked(d, o, s, cur, nullptr, 0, 0, stream);
}

extern "C" int vo_gftt_masked(const vo_dims* d, const vo_opts* o, const vo_state* s, int cur, const uint8_t* mask,
                              int64_t mask_stride, int32_t mask_pitch, vo_stream_t stream)
{
    if (!d || !o || !s || cur < 0 || cur > 1) return VO_EARG;
    if (o->feature_block_size < 1 || o->feature_block_size > EIG_MAXBS) return VO_EARG;
    if (mask && (mask_pitch < d->W || mask_stride < 0)) return VO_EARG;
    hipStream_t st = VO_STREAM(stream);
    if (hipMemsetAsync(s->eig_max, 0, sizeof(uint32_t) * d->B, st) != hipSuccess) return VO_EHIP;
    if (hipMemsetAsync(s->gf_n, 0, sizeof(int32_t) * d->B, st) != hipSuccess) return VO_EHIP;
    EigParamsM E;
    fill_eig(E, d, o, s, cur);
    E.keys = s->gf_keys; E.nkeys = s->gf_n; E.ccap = d->ccap;
    E.chain_status = s->status;
    E.eig_out = nullptr;
    if (mask) { E.mask = mask; E.mstride = mask_stride; E.mpitch = mask_pitch; }
    launch_eig(E, st);
    {
        // the split selection (k_gsel_*) where it applies: a minDistance grid of cells cvRound(md)
        // <= 255 wide (u64 cells of four corners: five never fit a cell of side cs - 1 <=
        // md - 0.5) that fits the eigen-map scratch, and 1 <= maxCorners <= the corner capacity
        // (no capacity truncation to report)
        const double md = o->feature_min_dist;
        const int cs = md >= 1 ? (int)lrint(md) : 0;
        const int gw = cs ? (d->W + cs - 1) / cs : 0, gh = cs ? (d->H + cs - 1) / cs : 0;
        const int64_t cells = (int64_t)gw * gh;
        const int want = o->feature_max_corners;
        const bool ok = s->gf_sort && cs >= 1 && cs <= 255 && cells * 8 + 4 <= (int64_t)4 * d->W * d->H && want >= 1 &&
                        want <= d->mcap && d->W <= 65535 && d->H <= 65535;
        static const int env = vo_env_int("VO_SEL_SPLIT", -1);
        // automatic: the split form for more than 64 chains per launch, where the one-block
        // kernel waits for whole CUs beside the other stream group's LK flood (headline 384: the
        // GFTT stage 5.7 -> 1.9 ms; C5 128: 9.7k -> 10.2k frames/s); at 1-48 chains the GPU has
        // room for the fat block and its 512-1024 threads finish the walk sooner (one chain
        // 2,251 vs 2,213 frames/s; the 8-GPU slice of 2 x 12 chains 88.2k vs 82.7k predicted)
        const int mode = g_sel_mode ? g_sel_mode : (env >= 0 ? (env ? 2 : 1) : (d->B > 64 ? 2 : 1));
        if (ok && mode == 2) {
            SelSplitParams G;
            G.keys = s->gf_keys; G.nkeys = s->gf_n; G.eig_max = s->eig_max; G.quality = o->feature_quality_level;
            G.ccap = d->ccap; G.W = d->W; G.H = d->H; G.invW = 1.0f / (float)d->W;
            G.want = want; G.md2 = md * md; G.cs = cs; G.gw = gw; G.gh = gh;
            G.cs_m = (uint32_t)(((1ull << 32) + cs - 1) / cs);
            G.corners = s->corners; G.ncorners = s->nCorners; G.mcap = d->mcap;
            G.sorted = s->gf_sort; G.sstride = (int64_t)d->ccap + VO_GF_SORT_EXTRA;
            G.ggrid = s->eig; G.gstride = (int64_t)d->W * d->H;
            // waves per chain for the gate / scatter / rank: ~4k local maxima per wave at full
            // capacity (C2: 57, C5: 64); a wave with nothing left returns at once
            int wpc = d->ccap / 4096;
            G.wpc = wpc < 4 ? 4 : (wpc > 64 ? 64 : wpc);
            G.chain_status = s->status;
            const int nb = d->B * G.wpc;
            hipLaunchKernelGGL(k_gsel_gate, dim3(nb), dim3(64), 0, st, G);
            hipLaunchKernelGGL(k_gsel_scan, dim3(d->B), dim3(64), 0, st, G);
            hipLaunchKernelGGL(k_gsel_scatter, dim3(nb), dim3(64), 0, st, G);
            hipLaunchKernelGGL(k_gsel_rank, dim3(nb), dim3(64), 0, st, G);
            hipLaunchKernelGGL(k_gsel_walk, dim3(d->B), dim3(64), 0, st, G);
            return hip_ok() ? VO_OK : VO_EHIP;
        }
    }
    SelParams S;
    S.keys = s->gf_keys; S.nkeys = s->gf_n; S.ccap = d->ccap; S.W = d->W; S.H = d->H;
    S.eig_max = s->eig_max; S.quality = o->feature_quality_level;
    S.max_corners = o->feature_max_corners; S.min_dist = o->feature_min_dist;
    S.corners = s->corners; S.ncorners = s->nCorners; S.mcap = d->mcap; S.chain_status = s->status;
    S.gscratch = (uint32_t*)s->eig;      // L2 grid when the LDS grid is too small
    S.gstride = (int64_t)d->W * d->H;
    {
        // LDS sized to this configuration (page + corner cap + grid) instead of the maximum
        const double md = o->feature_min_dist;
        const int cs = md >= 1 ? (int)lrint(md) : 1;
        const int64_t cells = md >= 1 ? (int64_t)((d->W + cs - 1) / cs) * ((d->H + cs - 1) / cs) : 0;
        S.acc_lds = d->mcap < ACC_MAX ? d->mcap : ACC_MAX;
        S.grid_lds = cells <= GRID_LDS_CELLS ? (int)cells : 0;
        // grid + per-cell candidate lists in LDS when they fit, else in the eigen-map scratch
        // (after the conflict lists) for the same parallel walk, else the wave-serial L2 path
        if (16 * (size_t)PAGE + 6 * (size_t)S.acc_lds + 8 * (size_t)S.grid_lds > 150 * 1024) S.grid_lds = 0;
        static const int noglb = vo_env_int("VO_SEL_SERIAL_L2", 0);
        S.grid_glb = !noglb && S.grid_lds == 0 && SEL_GG_OFF + 2 * cells <= S.gstride;
        // page, candidate xy and conflict slots | accepted xy + third-corner links | grid + heads
        const size_t lds = 16 * (size_t)PAGE + 6 * (size_t)S.acc_lds + 8 * (size_t)S.grid_lds;
        static const bool attr_ok =
            hipFuncSetAttribute((const void*)k_gftt_select<SEL_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                150 * 1024) == hipSuccess &&
            hipFuncSetAttribute((const void*)k_gftt_select<1024>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024) ==
                hipSuccess;
        if (!attr_ok && lds > 64 * 1024) return VO_EHIP;
        // block size SEL_THREADS = 512 (same result at any size; headline bench: 512 threads 56.2k
        // frames/s, 1024 55.1k -- a select block holds its wave slots while the other stream
        // group's LK runs), or 1024 threads per chain at few chains, where the GPU is mostly idle
        // during the select
        if (d->B <= 128) hipLaunchKernelGGL(k_gftt_select<1024>, dim3(d->B), dim3(1024), lds, st, S);
        else hipLaunchKernelGGL(k_gftt_select<SEL_THREADS>, dim3(d->B), dim3(SEL_THREADS), lds, st, S);
    }
    return hip_ok() ? VO_OK : VO_EHIP;
}
