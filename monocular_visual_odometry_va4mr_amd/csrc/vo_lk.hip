// Pyramidal Lucas-Kanade for gfx950 (one 64-lane wave per point) and the tracking compaction.
//
// Reference call sites: VisualOdometryPipeLine.py:281,:287 (calcOpticalFlowPyrLK), :282-290 (the
// status filtering).  Arithmetic follows oracle/vo_oracle_img.c operation by operation (that file
// restates OpenCV 4.6): the window sums are integer and exact, the float stages use
// the same op order (built with -ffp-contract=off, correctly rounded f32 div/sqrt).
#include "vo_dev.h"

#include <float.h>
#include <math.h>
#include <type_traits>

namespace {

// ------------------------------------------------------------------ LK
struct LKParams {
    const uint8_t* prev;
    const int16_t* der;             // interleaved (dx, dy) int16 pairs, pixel o at der[2o], der[2o + 1]
    const uint8_t* next;
    int64_t pstride, dstride;
    int L;                          // top level used
    int lw[VO_MAX_LEVELS], lh[VO_MAX_LEVELS], lpitch[VO_MAX_LEVELS];
    int64_t loff[VO_MAX_LEVELS];
    int win_w, win_h, max_count;
    double eps2;
    float min_eig;
    // k_lk_w's convergence test decided in f32 where a margin settles it: fl32(ddx^2 + ddy^2)
    // <= eps2_lo means converged, >= eps2_hi not converged, anything between takes the exact
    // double test (fill_lk; both infinite when eps2 is too small for the f32 form)
    float eps2_lo, eps2_hi;
    // point segments: seg0 then seg1 (seg1 used only where its count > seg1_min)
    const float* p0;
    const int32_t* n0;
    int cap0;
    const float* p1;
    const int32_t* n1;
    int cap1;
    int seg1_min;
    const int32_t* chain_status;
    float* out;
    uint8_t* st;
    float* err;                     // level 0's L1 error per point, or null: the error pass is not run
    int ocap;
    // read by the EX instantiations alone (vo_lk_points_ex, vo_lk_points_fb, vo_track_fb)
    const float* init;              // OPTFLOW_USE_INITIAL_FLOW: [B][ocap][2], the estimate's start at level L (or null)
    int eig_err;                    // OPTFLOW_LK_GET_MIN_EIGENVALS: err = level 0's minEig, no L1 error pass
    // backward pass of the forward-backward gate (or null): the point tracked is fwd[oidx] (the
    // forward result), only where st[oidx] (the forward status) is 1; the segment point is where
    // it has to return to, and st[oidx] becomes the gate status && |out - point|^2 <= thr2
    const float* fwd;
    double thr2;
};

// Block -> (chain, point block).  With B >= 8 all blocks of one chain land on one XCD
// (hardware dispatch is round-robin over the 8 XCDs by linear block id), so the chain's
// pyramid level stays in that XCD's 4 MB L2 instead of being fetched by all eight.
// The mapping only affects speed; any block order gives the same results.
VO_DEV bool lk_block(int B, int nb, int& b, int& pb, bool xcd = true, int L = -1)
{
    if (L < 0) L = blockIdx.x;
    if (B >= 8 && xcd) {
        const int xcd = L & 7, k = L >> 3;
        b = xcd + 8 * (k / nb);
        pb = k % nb;
    } else {
        b = L / nb;
        pb = L % nb;
    }
    return b < B;
}

// One pyramid level of calcOpticalFlowPyrLK for every point (lkpyramid.cpp LKTrackerInvoker,
// SURVEY.md Appendix A): levels are separate launches, coarse to fine, and the point's
// running estimate lives in P.out between them (float, exactly as the in-register value).
// One wave per point; the 15x15 window is spread over the lanes (MAXJ pixels per lane).
// The next-image window moves every iteration, so each wave stages the J neighbourhood in
// LDS as packed 2x2 pixel quads (one ds_read_b32 = the four bilinear taps) and re-stages
// only when the estimate drifts more than M pixels.  The bilinear sum is two v_dot4_u32_u8
// over the 14-bit weights split into 7+7 bits; all window sums are integer and exact, so
// results match the CPU restatement bit for bit.
#define LK_M 4
// buffer resource over one chain's buffer: loads take 32-bit offsets (one VGPR, not a 64-bit
// address) and read zeros outside [0, bytes) instead of faulting
VO_DEV __amdgpu_buffer_rsrc_t lkq_rsrc(const void* base, int64_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, (int)bytes, 0x00020000);
}
#ifndef LK_JPRE
#define LK_JPRE 1
#endif

// a wave-uniform VALU result into an SGPR, where the arithmetic that consumes it (the weight
// packing) runs on the scalar unit instead of the VALU
VO_DEV int to_sgpr(int v)
{
    // an empty asm makes the VGPR value opaque, so the readfirstlane cannot be folded into the
    // conversion that produced it (an inline-asm readfirstlane instead broke LK on gfx950)
    asm volatile("" : "+v"(v));
    return __builtin_amdgcn_readfirstlane(v);
}
typedef short v2i16 __attribute__((ext_vector_type(2)));
VO_DEV v2i16 as_v2i16(uint32_t u) { return __builtin_bit_cast(v2i16, u); }
// v_dot2_i32_i16 (VOP3P) with its accumulator in an SGPR or as the inline constant 0: for a
// constant accumulator the compiler otherwise emits v_mov + v_dot2c (one VALU more)
VO_DEV int sdot2_sacc(uint32_t a, uint32_t b, int acc)
{
    int r;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(acc));
    return r;
}
VO_DEV int sdot2_0(uint32_t a, uint32_t b)
{
    int r;
    asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
VO_DEV uint32_t v2u(v2i16 v) { return __builtin_bit_cast(uint32_t, v); }

// k_lk_w's bilinear weights w (0 .. 2^14) as an 8 + 7-bit split, bytes in the quad order of its J
// tile (w00, w10, w01, w11): wlo = w & 255, whi = w >> 8.  From the weights' low halves (the
// float bit patterns of w + 1.5 * 2^23 carry w in their low bits) two 16-bit packs and a few
// masks on the scalar unit (~10 SALU; the 7 + 7 form took ~25, and k_lk_w is SALU-bound).
VO_DEV void pack_w8_halves(uint32_t p0, uint32_t p1, uint32_t& wlo, uint32_t& whi)
{
    wlo = (p0 & 0x00ff00ffu) | ((p1 & 0x00ff00ffu) << 8);
    whi = ((p0 >> 8) & 0x00ff00ffu) | (p1 & 0xff00ff00u);
}
// operands in SGPRs (the iteration's weights): the two 16-bit packs as s_pack_ll_b32_b16
VO_DEV void pack_w8(uint32_t u00, uint32_t u01, uint32_t u10, uint32_t w11, uint32_t& wlo, uint32_t& whi)
{
    uint32_t p0, p1;                                         // (w00, w01), (w10, w11)
    asm("s_pack_ll_b32_b16 %0, %1, %2" : "=s"(p0) : "s"(u00), "s"(u01));
    asm("s_pack_ll_b32_b16 %0, %1, %2" : "=s"(p1) : "s"(u10), "s"(w11));
    pack_w8_halves(p0, p1, wlo, whi);
}
// any operands (the level-0 error pass)
VO_DEV void pack_w8_v(uint32_t w00, uint32_t w01, uint32_t w10, uint32_t w11, uint32_t& wlo, uint32_t& whi)
{
    pack_w8_halves((w00 & 0xffffu) | (w01 << 16), (w10 & 0xffffu) | (w11 << 16), wlo, whi);
}
VO_DEV uint32_t pack_w(int w00, int w01, int w10, int w11, int shift, int mask)
{
    return (uint32_t)((w00 >> shift) & mask) | ((uint32_t)((w01 >> shift) & mask) << 8) |
           ((uint32_t)((w10 >> shift) & mask) << 16) | ((uint32_t)((w11 >> shift) & mask) << 24);
}

// Four bilinear taps (x, y) .. (x + 1, y + 1) of a window that may reach past the materialised
// border (a side > VO_BORDER): byte offsets inside the level at reflect-101 coordinates, which
// are the values a wider border would hold, and whether each tap lies in the interior (the
// derivative image is zero everywhere else).  Every offset is that of an interior pixel.
struct LKTaps {
    int o00, o01, o10, o11;
    bool in00, in01, in10, in11;
};
VO_DEV LKTaps lk_taps(int x, int y, int cols, int rows, int pitch)
{
    const int x0 = refl101(x, cols) + VO_BORDER, x1 = refl101(x + 1, cols) + VO_BORDER;
    const int r0 = (refl101(y, rows) + VO_BORDER) * pitch, r1 = (refl101(y + 1, rows) + VO_BORDER) * pitch;
    const bool ix0 = (unsigned)x < (unsigned)cols, ix1 = (unsigned)(x + 1) < (unsigned)cols;
    const bool iy0 = (unsigned)y < (unsigned)rows, iy1 = (unsigned)(y + 1) < (unsigned)rows;
    LKTaps t;
    t.o00 = r0 + x0; t.o01 = r0 + x1; t.o10 = r1 + x0; t.o11 = r1 + x1;
    t.in00 = ix0 && iy0; t.in01 = ix1 && iy0; t.in10 = ix0 && iy1; t.in11 = ix1 && iy1;
    return t;
}

// k_lk's illumination models (ILL): (float)((G - Ca Cb / V) / N), one centred window sum
// with the gain term taken out (GB, the caller passes it only with V > 0) or not; one multiply, one
// divide and one subtract in fp64, in that order
template <bool GB>
VO_DEV float lk_comp(int64_t G, int64_t Ca, int64_t Cb, int64_t V, int N)
{
    double g = (double)G;
    if (GB) g = g - ((double)Ca * (double)Cb) / (double)V;
    return (float)(g / (double)N);
}

// BIG: a window side exceeds VO_BORDER, so a window accepted by the bounds test (ipx >= -win_w,
// ipx < cols) can reach up to win - VO_BORDER pixels past the stored border.  Those instantiations
// address every tap through lk_taps (window gather, J staging, level-0 error pass); the others
// read the materialised border directly.
// EX: the variants behind cv2's flags and the forward-backward gate (LKParams::init, eig_err, fwd);
// the default instantiations hold none of that code.
// ILL: the illumination model, 0 = none, VO_LK_ILLUM_BIAS, VO_LK_ILLUM_GAIN_BIAS: the
// tensor and the right-hand side with an additive offset (and a gain) of J against I eliminated by
// least squares.  Extra exact integer window sums, then lk_comp's few fp64 operations; ILL = 0 holds
// none of that code.
template <int MAXJ, bool BIG, bool EX = false, int ILL = 0>
__global__ void __launch_bounds__(64) k_lk(LKParams P, int level, int B, int nb)
{
    extern __shared__ uint32_t lk_tile[];
    int b, pb;
    if (!lk_block(B, nb, b, pb)) return;
    if (P.chain_status && P.chain_status[b] != 0) return;
    const int lane = lane_id();
    const int n0 = P.n0 ? P.n0[b] : 0;
    int n1 = P.n1 ? P.n1[b] : 0;
    if (n1 <= P.seg1_min) n1 = 0;
    const int ntot = n0 + n1;
    const int ww = P.win_w, wh = P.win_h, npx = ww * wh;
    const int TW = ww + 2 * LK_M, TH = wh + 2 * LK_M;
    uint32_t* tile = lk_tile + wave_id() * TW * TH;
    const float hx = (ww - 1) * 0.5f, hy = (wh - 1) * 0.5f;
    const int wpb = blockDim.x >> 6;
    const int cols = P.lw[level], rows = P.lh[level], pitch = P.lpitch[level];
    const int prow = rows + 2 * VO_BORDER;
    const uint8_t* I = P.prev + b * P.pstride + P.loff[level];
    const int16_t* DI = P.der + b * P.dstride + 2 * P.loff[level];
    const uint8_t* J = P.next + b * P.pstride + P.loff[level];
    const float sc = (float)(1. / (1 << level));
    // per-lane window slots: offsets in the level image and in the tile; slots past the
    // window read pixel (0,0) and are zeroed through their gradients / the error mask
    int goff[MAXJ], toff[MAXJ], wxy[MAXJ];     // wxy (BIG): the slot's window position, wx | wy << 8
    bool live[MAXJ];
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        const int k = lane + 64 * j;
        const int wy = k / ww, wx = k - wy * ww;
        live[j] = k < npx;
        goff[j] = live[j] ? wy * pitch + wx : 0;
        toff[j] = live[j] ? wy * TW + wx : 0;
        wxy[j] = live[j] ? (wx | (wy << 8)) : 0;
    }
    for (int p = pb * wpb + wave_id(); p < ntot; p += nb * wpb) {
        const float* src = (p < n0) ? (P.p0 + ((int64_t)b * P.cap0 + p) * 2) : (P.p1 + ((int64_t)b * P.cap1 + (p - n0)) * 2);
        const int64_t oidx = (int64_t)b * P.ocap + p;
        float ptx = src[0], pty = src[1];
        const float gtx = ptx, gty = pty;       // EX: the gate's origin
        if constexpr (EX) {
            if (P.fwd) {
                if (!P.st[oidx]) continue;      // lost by the forward pass: nothing to track back
                ptx = P.fwd[2 * oidx];
                pty = P.fwd[2 * oidx + 1];
            }
        }
        int status = 1;
        float errv = 0.f;
        float px = ptx * sc, py = pty * sc;
        float ox, oy;   // nextPts[ptidx]
        if (level == P.L) {
            ox = px; oy = py;
            if constexpr (EX) {
                if (P.init) { ox = P.init[2 * oidx] * sc; oy = P.init[2 * oidx + 1] * sc; }
            }
        }
        else { ox = P.out[2 * oidx] * 2.f; oy = P.out[2 * oidx + 1] * 2.f; }
        px -= hx;
        py -= hy;
        const int ipx = (int)floorf(px), ipy = (int)floorf(py);
        do {
            if (ipx < -ww || ipx >= cols || ipy < -wh || ipy >= rows) {
                if (level == 0) { status = 0; errv = 0.f; }
                break;
            }
            float a = px - ipx, bb = py - ipy;
            int iw00 = __float2int_rn((1.f - a) * (1.f - bb) * (float)(1 << 14));
            int iw01 = __float2int_rn(a * (1.f - bb) * (float)(1 << 14));
            int iw10 = __float2int_rn((1.f - a) * bb * (float)(1 << 14));
            int iw11 = (1 << 14) - iw00 - iw01 - iw10;
            int ival[MAXJ], ixv[MAXJ], iyv[MAXJ];
            int a11 = 0, a12 = 0, a22 = 0;
            int tix = 0, tiy = 0, ti = 0, tii = 0, tiix = 0, tiiy = 0;     // ILL: sums of Ix, Iy, I, I^2, I Ix, I Iy
            const int64_t ib = (int64_t)(ipy + VO_BORDER) * pitch + (ipx + VO_BORDER);
#pragma unroll
            for (int j = 0; j < MAXJ; ++j) {
                int v, gx, gy;
                if constexpr (BIG) {
                    const LKTaps t = lk_taps(ipx + (wxy[j] & 255), ipy + (wxy[j] >> 8), cols, rows, pitch);
                    v = DESCALE(__mul24(I[t.o00], iw00) + __mul24(I[t.o01], iw01) + __mul24(I[t.o10], iw10) + __mul24(I[t.o11], iw11), 9);
                    const int x00 = t.in00 ? DI[2 * t.o00] : 0, x01 = t.in01 ? DI[2 * t.o01] : 0;
                    const int x10 = t.in10 ? DI[2 * t.o10] : 0, x11 = t.in11 ? DI[2 * t.o11] : 0;
                    const int y00 = t.in00 ? DI[2 * t.o00 + 1] : 0, y01 = t.in01 ? DI[2 * t.o01 + 1] : 0;
                    const int y10 = t.in10 ? DI[2 * t.o10 + 1] : 0, y11 = t.in11 ? DI[2 * t.o11 + 1] : 0;
                    gx = DESCALE(__mul24(x00, iw00) + __mul24(x01, iw01) + __mul24(x10, iw10) + __mul24(x11, iw11), 14);
                    gy = DESCALE(__mul24(y00, iw00) + __mul24(y01, iw01) + __mul24(y10, iw10) + __mul24(y11, iw11), 14);
                } else {
                    const int64_t o = ib + goff[j];
                    const uint8_t* s = I + o;
                    const int16_t* d = DI + 2 * o;              // (dx, dy) pairs
                    const int16_t* e = d + 1;
                    v = DESCALE(__mul24(s[0], iw00) + __mul24(s[1], iw01) + __mul24(s[pitch], iw10) + __mul24(s[pitch + 1], iw11), 9);
                    gx = DESCALE(__mul24(d[0], iw00) + __mul24(d[2], iw01) + __mul24(d[2 * pitch], iw10) + __mul24(d[2 * pitch + 2], iw11), 14);
                    gy = DESCALE(__mul24(e[0], iw00) + __mul24(e[2], iw01) + __mul24(e[2 * pitch], iw10) + __mul24(e[2 * pitch + 2], iw11), 14);
                }
                ival[j] = live[j] ? v : 0;
                ixv[j] = live[j] ? gx : 0;
                iyv[j] = live[j] ? gy : 0;
                a11 += __mul24(ixv[j], ixv[j]);
                a12 += __mul24(ixv[j], iyv[j]);
                a22 += __mul24(iyv[j], iyv[j]);
                if constexpr (ILL != 0) {       // per lane below 2^31 at MAXJ = 16: 16 * 8160^2
                    tix += ixv[j];
                    tiy += iyv[j];
                    ti += ival[j];
                    tii += __mul24(ival[j], ival[j]);
                    tiix += __mul24(ival[j], ixv[j]);
                    tiiy += __mul24(ival[j], iyv[j]);
                }
            }
            const int64_t iA11 = wave_sum_split(a11), iA12 = wave_sum_split(a12), iA22 = wave_sum_split(a22);
            const float FLT_SCALE = 1.f / (1 << 20);
            float A11, A12, A22;
            int64_t SIx = 0, SIy = 0, SI = 0, Cx = 0, Cy = 0, V = 0;
            bool gb = false;                    // gain_bias with V > 0: the gain term is taken out
            if constexpr (ILL != 0) {
                SIx = wave_sum_split(tix); SIy = wave_sum_split(tiy); SI = wave_sum_split(ti);
                const int64_t SII = wave_sum_split(tii), SIIx = wave_sum_split(tiix), SIIy = wave_sum_split(tiiy);
                const int64_t Gxx = npx * iA11 - SIx * SIx, Gxy = npx * iA12 - SIx * SIy, Gyy = npx * iA22 - SIy * SIy;
                Cx = npx * SIIx - SI * SIx;
                Cy = npx * SIIy - SI * SIy;
                V = npx * SII - SI * SI;
                gb = ILL == VO_LK_ILLUM_GAIN_BIAS && V > 0;
                if (gb) {
                    A11 = lk_comp<true>(Gxx, Cx, Cx, V, npx) * FLT_SCALE;
                    A12 = lk_comp<true>(Gxy, Cx, Cy, V, npx) * FLT_SCALE;
                    A22 = lk_comp<true>(Gyy, Cy, Cy, V, npx) * FLT_SCALE;
                } else {
                    A11 = lk_comp<false>(Gxx, 0, 0, 1, npx) * FLT_SCALE;
                    A12 = lk_comp<false>(Gxy, 0, 0, 1, npx) * FLT_SCALE;
                    A22 = lk_comp<false>(Gyy, 0, 0, 1, npx) * FLT_SCALE;
                }
            } else {
                A11 = (float)iA11 * FLT_SCALE; A12 = (float)iA12 * FLT_SCALE; A22 = (float)iA22 * FLT_SCALE;
            }
            float D = A11 * A22 - A12 * A12;
            const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * ww * wh);
            if constexpr (EX) {
                if (P.eig_err && level == 0) errv = minEig;
            }
            if (minEig < P.min_eig || D < FLT_EPSILON) {
                if (level == 0) status = 0;
                break;
            }
            D = 1.f / D;
            float nx = ox - hx, ny = oy - hy;
            float pdx = 0.f, pdy = 0.f;
            int tx0 = -(1 << 30), ty0 = -(1 << 30);
            for (int it = 0; it < P.max_count; ++it) {
                const int inx = (int)floorf(nx), iny = (int)floorf(ny);
                if (inx < -ww || inx >= cols || iny < -wh || iny >= rows) {
                    if (level == 0) status = 0;
                    break;
                }
                if (inx < tx0 || inx > tx0 + 2 * LK_M || iny < ty0 || iny > ty0 + 2 * LK_M) {
                    // (re)stage the quad tile around the window; with sides <= VO_BORDER bytes
                    // outside the padded level are never read by an in-bounds window
                    tx0 = inx - LK_M;
                    ty0 = iny - LK_M;
                    __builtin_amdgcn_wave_barrier();
                    for (int q = lane; q < TW * TH; q += 64) {
                        const int r = q / TW, c = q - r * TW;
                        const int gy = ty0 + r + VO_BORDER, gx = tx0 + c + VO_BORDER;
                        uint32_t v = 0;
                        if constexpr (BIG) {
                            const LKTaps t = lk_taps(tx0 + c, ty0 + r, cols, rows, pitch);
                            v = (uint32_t)J[t.o00] | ((uint32_t)J[t.o01] << 8) | ((uint32_t)J[t.o10] << 16) |
                                ((uint32_t)J[t.o11] << 24);
                        } else if (gy >= 0 && gy + 1 < prow && gx >= 0 && gx + 1 < pitch) {
                            const uint8_t* g = J + (int64_t)gy * pitch + gx;
                            v = (uint32_t)g[0] | ((uint32_t)g[1] << 8) | ((uint32_t)g[pitch] << 16) |
                                ((uint32_t)g[pitch + 1] << 24);
                        }
                        tile[q] = v;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                }
                a = nx - inx;
                bb = ny - iny;
                iw00 = __float2int_rn((1.f - a) * (1.f - bb) * (float)(1 << 14));
                iw01 = __float2int_rn(a * (1.f - bb) * (float)(1 << 14));
                iw10 = __float2int_rn((1.f - a) * bb * (float)(1 << 14));
                iw11 = (1 << 14) - iw00 - iw01 - iw10;
                // iw00..iw10 are in [0, 2^14]; iw11 = 2^14 - (the others) can be -1, which
                // the unsigned dot cannot take: use iw11 + 1 and subtract the tap once
                const int neg = iw11 < 0;
                const int w11 = iw11 + neg;
                const uint32_t wlo = pack_w(iw00, iw01, iw10, w11, 0, 127);
                const uint32_t whi = pack_w(iw00, iw01, iw10, w11, 7, 255);
                const uint32_t* tb = tile + (iny - ty0) * TW + (inx - tx0);
                int b1 = 0, b2 = 0;
                int td = 0, tdi = 0;            // ILL: sums of diff and diff I
#pragma unroll
                for (int j = 0; j < MAXJ; ++j) {
                    const uint32_t q = tb[toff[j]];
                    uint32_t sum = (__builtin_amdgcn_udot4(q, whi, 0u, false) << 7) +
                                   __builtin_amdgcn_udot4(q, wlo, 256u, false);
                    if (neg) sum -= q >> 24;
                    const int diff = (int)(sum >> 9) - ival[j];
                    b1 += __mul24(diff, ixv[j]);      // |diff| <= 8160, |grad| <= 4080
                    b2 += __mul24(diff, iyv[j]);
                    if constexpr (ILL != 0) {
                        td += live[j] ? diff : 0;       // a dead slot's diff is pixel (0, 0)'s; the products
                        tdi += __mul24(diff, ival[j]);  // need no mask: ival, ixv and iyv are zero there
                    }
                }
                // 32-bit reductions when every partial is below 2^24 (total < 2^30)
                const bool wide = __ballot((uint32_t)(b1 + (1 << 24)) >= (1u << 25) ||
                                           (uint32_t)(b2 + (1 << 24)) >= (1u << 25)) != 0;
                int64_t s1, s2;
                if (!wide) { s1 = wave_sum_dpp(b1); s2 = wave_sum_dpp(b2); }
                else { s1 = wave_sum_split(b1); s2 = wave_sum_split(b2); }
                float fb1, fb2;
                if constexpr (ILL != 0) {
                    const int64_t Sd = wave_sum_split(td), SdI = wave_sum_split(tdi);
                    const int64_t Bx = npx * s1 - Sd * SIx, By = npx * s2 - Sd * SIy, Cd = npx * SdI - SI * Sd;
                    if (gb) {
                        fb1 = lk_comp<true>(Bx, Cd, Cx, V, npx) * FLT_SCALE;
                        fb2 = lk_comp<true>(By, Cd, Cy, V, npx) * FLT_SCALE;
                    } else {
                        fb1 = lk_comp<false>(Bx, 0, 0, 1, npx) * FLT_SCALE;
                        fb2 = lk_comp<false>(By, 0, 0, 1, npx) * FLT_SCALE;
                    }
                } else {
                    fb1 = (float)s1 * FLT_SCALE;
                    fb2 = (float)s2 * FLT_SCALE;
                }
                const float ddx = (A12 * fb2 - A22 * fb1) * D;
                const float ddy = (A12 * fb1 - A11 * fb2) * D;
                nx += ddx;
                ny += ddy;
                ox = nx + hx;
                oy = ny + hy;
                if ((double)ddx * ddx + (double)ddy * ddy <= P.eps2) break;
                if (it > 0 && fabsf(ddx + pdx) < 0.01f && fabsf(ddy + pdy) < 0.01f) {
                    ox -= ddx * 0.5f;
                    oy -= ddy * 0.5f;
                    break;
                }
                pdx = ddx;
                pdy = ddy;
            }
            if (status && level == 0 && !(EX && P.eig_err)) {
                const float fx = ox - hx, fy = oy - hy;
                const int inx = (int)floorf(fx), iny = (int)floorf(fy);
                if (inx < -ww || inx >= cols || iny < -wh || iny >= rows) {
                    status = 0;
                    break;
                }
                if (!P.err) break;              // nobody reads the error; the status decision above stays
                const float aa = fx - inx, cc = fy - iny;
                iw00 = __float2int_rn((1.f - aa) * (1.f - cc) * (float)(1 << 14));
                iw01 = __float2int_rn(aa * (1.f - cc) * (float)(1 << 14));
                iw10 = __float2int_rn((1.f - aa) * cc * (float)(1 << 14));
                iw11 = (1 << 14) - iw00 - iw01 - iw10;
                const int64_t jb = (int64_t)(iny + VO_BORDER) * pitch + (inx + VO_BORDER);
                int es = 0;
#pragma unroll
                for (int j = 0; j < MAXJ; ++j) {
                    int diff;
                    if constexpr (BIG) {
                        const LKTaps t = lk_taps(inx + (wxy[j] & 255), iny + (wxy[j] >> 8), cols, rows, pitch);
                        diff = DESCALE(__mul24(J[t.o00], iw00) + __mul24(J[t.o01], iw01) + __mul24(J[t.o10], iw10) + __mul24(J[t.o11], iw11), 9) - ival[j];
                    } else {
                        const uint8_t* s = J + jb + goff[j];
                        diff = DESCALE(__mul24(s[0], iw00) + __mul24(s[1], iw01) + __mul24(s[pitch], iw10) + __mul24(s[pitch + 1], iw11), 9) - ival[j];
                    }
                    es += live[j] ? (diff < 0 ? -diff : diff) : 0;
                }
                errv = (float)wave_sum_dpp(es) / (float)(32 * ww * wh);
            }
        } while (false);
        if (lane == 0) {
            P.out[2 * oidx] = ox;
            P.out[2 * oidx + 1] = oy;
            if (level == 0) {
                if constexpr (EX) {
                    if (P.fwd) {
                        const float gdx = ox - gtx, gdy = oy - gty;
                        if (!((double)gdx * gdx + (double)gdy * gdy <= P.thr2)) status = 0;
                    }
                }
                P.st[oidx] = (uint8_t)status;
                if (P.err) P.err[oidx] = errv;
            }
        }
    }
}

#ifdef VO_LK_PROF
// per level, per block (first 1024): start, end (wall clock, 100 MHz), iterations, J stagings,
// then wall-clock ticks spent in: I/dI staging, structure tensor, J staging, iterations
__device__ long long g_lkprof[VO_MAX_LEVELS][1024][8];
#define LKPROF_SET(k, v) do { if (lane == 0 && blockIdx.x < 1024) g_lkprof[level][blockIdx.x][k] = (v); } while (0)
#define LKPROF_ADD(k, v) do { if (lane == 0 && blockIdx.x < 1024) g_lkprof[level][blockIdx.x][k] += (v); } while (0)
#else
#define LKPROF_SET(k, v) do { } while (0)
#define LKPROF_ADD(k, v) do { } while (0)
#endif
#ifdef VO_LK_PROF
#define LKPROF_T(var) const long long var = wall_clock64()
#else
#define LKPROF_T(var) do { } while (0)
#endif

#ifdef VO_LK_CHECK
// diagnostics build: bounds-check every global load of k_lk_w against its chain's buffer;
// a bad address is reported and not dereferenced
#define LKCHK(ptr, base, bytes, what) \
    (((const char*)(ptr) >= (const char*)(base) && (const char*)(ptr) + 4 <= (const char*)(base) + (bytes)) ? true : \
     (printf("LKCHK %s b=%d p=%d level=%d off=%lld size=%lld\n", what, b, pcur, level, \
             (long long)((const char*)(ptr) - (const char*)(base)), (long long)(bytes)), false))
#else
#define LKCHK(ptr, base, bytes, what) true
#endif
#ifdef VO_LK_CHECK
// offset form for the buffer loads of k_lk_w (which read zeros past the chain's buffer)
#define LKCHKO(off, bytes, what) \
    do { if ((off) < 0 || (int64_t)(off) + 4 > (int64_t)(bytes)) \
        printf("LKCHK %s b=%d p=%d level=%d off=%lld size=%lld\n", what, b, pcur, level, (long long)(off), (long long)(bytes)); } while (0)
#else
#define LKCHKO(off, bytes, what) do { } while (0)
#endif

// ---------------------------------------------------------------------------------------
// k_lk_w<WW, WH>: the same LK level as k_lk for a compile-time window (the reference uses
// 15x15 for every dataset, main.py:36,66,96), with all window data staged through LDS by
// coalesced dword loads instead of per-lane byte gathers:
//   IR/DR  raw rows of I (u8) and dI (int16 pairs) under the (WW+1)x(WH+1) bilinear window,
//   QT     the J tile ((TW+1)x(TH+1), TW = WW + 2M) as packed 2x2 quads, read by the
//          iterations; built straight from registers (rows r and r + 1 loaded by every lane,
//          the next dword from the neighbouring lane): no raw-row LDS image.
// The tile origin is clamped so every staged row lies inside the padded level; dword rows
// may run up to 3 bytes past a row end (next row, or the >= 64-byte tail slack that the
// caller must leave after each pyramid -- launch_lk checks it).  Arithmetic is identical to
// k_lk (bit-exact with the CPU restatement).
// ERR (the instantiations without EX; EX decides by P.err at run time): the level-0 L1-error pass
// exists only where the caller gave an err buffer.  Its bounds test is a status decision and stays.
template <int WW, int WH, bool EX = false, bool ERR = true>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) k_lk_w(LKParams P, int level_hi, int level_lo, int B, int nb, int xcd)
{
    constexpr int WPB = 1;
    constexpr int NPX = WW * WH, MAXJ = (NPX + 63) / 64;
    constexpr int TW = WW + 2 * LK_M, TH = WH + 2 * LK_M;
    constexpr int JRW = (TW + 1 + 3 + 3) / 4, IRW = (WW + 1 + 3 + 3) / 4, DRW = WW + 1;
    constexpr int QM = (TW + 3) / 4, QS = 4 * QM;      // QT: quads of 4 columns, row stride QS
    // LDS rows: QT quads, the I window bytes and the dI dwords all have the row stride QS (in
    // their element), so one per-lane offset toff = row * QS + col indexes all three; J rows are
    // loaded as 8 dwords, so the staging lane -> (row, dword) map is (lane / 8, lane % 8)
    constexpr int IRS = QS / 4, JRS = 8;
    static_assert(JRW >= QM + 1 && JRW <= JRS && IRW <= IRS && IRW <= 8 && DRW == 16 && QS % 4 == 0,
                  "k_lk_w staging layout");
    // one spare row in QT / IR / DR: read (never used) by the dead lanes of window row 15
    __shared__ uint4 QT4_all[WPB][(TH + 1) * QM];
    __shared__ uint32_t IR_all[WPB][(WH + 2) * IRS];
    __shared__ uint32_t DR_all[WPB][(WH + 2) * QS];
    const int wv = WPB > 1 ? (int)(threadIdx.x >> 6) : 0;
    uint4* QT4 = QT4_all[wv];
    const uint32_t* QT = reinterpret_cast<const uint32_t*>(QT4);
    uint32_t* IR = IR_all[wv];
    uint32_t* DR = DR_all[wv];
    const uint8_t* ir8 = (const uint8_t*)IR;
    int b, pb, pcur = -1;
    const int lane = lane_id();
    int level = level_lo;
    LKPROF_SET(0, wall_clock64()); LKPROF_SET(1, 0);
    for (level = level_hi; level >= level_lo; --level)
        for (int k = 2; k < 8; ++k) LKPROF_SET(k, 0);
    level = level_lo;
    if (!lk_block(B, nb, b, pb, xcd != 0, (int)blockIdx.x * WPB + wv)) return;
    if (P.chain_status && P.chain_status[b] != 0) return;
    const int n0 = P.n0 ? P.n0[b] : 0;
    int n1 = P.n1 ? P.n1[b] : 0;
    if (n1 <= P.seg1_min) n1 = 0;
    const int ntot = n0 + n1;
    const float hx = (WW - 1) * 0.5f, hy = (WH - 1) * 0.5f;
    // held in registers: read from the kernel arguments inside the iteration loop it costs a
    // scalar load and its wait per iteration
    double eps2;
    asm volatile("" : "=s"(eps2) : "0"(P.eps2));
    float eps2_lo, eps2_hi;
    asm volatile("" : "=s"(eps2_lo) : "0"(P.eps2_lo));
    asm volatile("" : "=s"(eps2_hi) : "0"(P.eps2_hi));
    // window pixels of a lane: column lane % 16, rows 4 j + s with s = (lane / 32) + 2 (lane / 16
    // % 2), so that a 32-lane half reads rows s and s + 2 (row offsets 0 and 2 * QS = 48 dwords,
    // 16 banks apart: conflict-free) and pixel j sits at the constant offset toff + 4 j QS
    // (folded into the LDS instruction).  Column 15 and row 15 are dead lanes.
    static_assert(WW <= 16 && WH <= 16 && MAXJ == 4 && (2 * QS) % 32 == 16, "k_lk_w window map");
    const int wrow = ((lane >> 5) & 1) + 2 * ((lane >> 4) & 1), wcol = lane & 15;
    const int toff0 = wrow * QS + wcol;
    int toff[MAXJ];
    bool live[MAXJ];
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        live[j] = wcol < WW && wrow + 4 * j < WH;
        toff[j] = toff0 + 4 * j * QS;
    }
    int tx0 = 0, ty0 = 0, jsh = 0;
    int cols = 0, rows = 0, pitch = 0, loff = 0;
    const __amdgpu_buffer_rsrc_t rI = lkq_rsrc(P.prev + (int64_t)b * P.pstride, P.pstride);
    const __amdgpu_buffer_rsrc_t rJ = lkq_rsrc(P.next + (int64_t)b * P.pstride, P.pstride);
    const __amdgpu_buffer_rsrc_t rD = lkq_rsrc(P.der + (int64_t)b * P.dstride, 2 * P.dstride);
    // Staging is split into issue (global loads into registers, fixed unrolled trip counts)
    // and store (LDS writes), so that every load of a stage is in flight at once: one memory
    // round trip per stage instead of one per loop trip.
    constexpr int NIR = ((WH + 1) * 8 + 63) / 64, NDR = ((WH + 1) * 16 + 63) / 64;
    constexpr int NJR = (TH * JRS + 63) / 64;             // 8 quad rows per load round
    // J tile origin covering the window at (inx, iny)
    auto j_origin = [&](int inx, int iny) {
        tx0 = max(inx - LK_M, -VO_BORDER);
        ty0 = min(max(iny - LK_M, -VO_BORDER), rows + VO_BORDER - 1 - TH);
        jsh = (tx0 + VO_BORDER) & 3;
    };
    // J rows r (a) and r + 1 (b) of the tile straight into registers, lane -> row 8 k + lane / 8
    // (+ 1 for b), aligned dword lane % 8 -- no raw-row LDS image: the quad build below takes
    // the dword to the right from the neighbouring lane (DPP) and row r + 1 from its own b load
    auto j_issue = [&](uint32_t (&v)[2][NJR]) {
        const int gx0 = tx0 + VO_BORDER, gy0 = ty0 + VO_BORDER;
        const int ln = lane;
        const int vo = loff + gy0 * pitch + (gx0 & ~3) + (ln >> 3) * pitch + 4 * (ln & 7);
#pragma unroll
        for (int k = 0; k < NJR; ++k) {
            v[0][k] = 0u;
            v[1][k] = 0u;
            if ((lane >> 3) + 8 * k < TH) {               // quad rows 0 .. TH - 1 use rows r, r + 1
                LKCHKO(vo + 8 * k * pitch + pitch, P.pstride, "J");
                v[0][k] = __builtin_amdgcn_raw_buffer_load_b32(rJ, vo, 8 * k * pitch, 0);
                v[1][k] = __builtin_amdgcn_raw_buffer_load_b32(rJ, vo, 8 * k * pitch + pitch, 0);
            }
        }
    };
    // the packed 2x2 quads QT: one item = quad row r, columns 4m..4m+3 (lane: r = 8 k + lane / 8,
    // m = lane % 8 < QM), built from the aligned dwords m, m + 1 of rows r and r + 1 (dword m + 1
    // from lane + 1 by DPP row_shl:1; m + 1 <= QM < 8 stays in the lane's 8-group) with byte-align
    // and two rounds of byte permutes, stored as one 16-B write; quad byte order (J[r][c],
    // J[r][c+1], J[r+1][c], J[r+1][c+1])
    auto j_store = [&](const uint32_t (&v)[2][NJR]) {
        const int ln = lane;
        const int m = ln & 7;
        const uint32_t jsel1 = (uint32_t)(jsh + 1) * 0x01010101u + 0x03020100u;   // bytes jsh+1 .. jsh+4
#pragma unroll
        for (int k = 0; k < NJR; ++k) {
            const uint32_t a0 = v[0][k], b0 = v[1][k];
            const uint32_t a1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)a0, 0x101, 0xF, 0xF, false);   // row_shl:1
            const uint32_t b1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)b0, 0x101, 0xF, 0xF, false);
            const int r = (ln >> 3) + 8 * k;
            if (m < QM && r < TH) {
                // row r bytes Wa0..Wa4 = bytes jsh .. jsh + 4 of (a1:a0), row r + 1 likewise Wb: A / C
                // hold W0..W3, Bv / D hold W1..W4 (byte-select by an SGPR selector, which also
                // covers jsh + 1 = 4); quad i = (Wa_i, Wb_i, Wa_i+1, Wb_i+1) (the weights' byte
                // order, pack_w8), one permute each
                const uint32_t A = __builtin_amdgcn_alignbyte(a1, a0, jsh);
                const uint32_t Bv = __builtin_amdgcn_perm(a1, a0, jsel1);
                const uint32_t C = __builtin_amdgcn_alignbyte(b1, b0, jsh);
                const uint32_t D = __builtin_amdgcn_perm(b1, b0, jsel1);
                QT4[r * QM + m] = make_uint4(__builtin_amdgcn_perm(C, A, 0x05010400u), __builtin_amdgcn_perm(C, A, 0x06020501u),
                                             __builtin_amdgcn_perm(C, A, 0x07030602u), __builtin_amdgcn_perm(D, Bv, 0x07030602u));
            }
        }
        wave_lds_sync();
    };
    // (re)stage the J tile so that it covers the window at (inx, iny)
    auto stage_j = [&](int inx, int iny) {
        LKPROF_ADD(3, 1);
        LKPROF_T(tj0);
        j_origin(inx, iny);
        uint32_t v[2][NJR];
        j_issue(v);
        wave_lds_sync();
        j_store(v);
        LKPROF_T(tj1);
        LKPROF_ADD(6, tj1 - tj0);
    };
    for (int p = pb + 0; p < ntot; p += nb) {
        const float* src = (p < n0) ? (P.p0 + ((int64_t)b * P.cap0 + p) * 2) : (P.p1 + ((int64_t)b * P.cap1 + (p - n0)) * 2);
        const int64_t oidx = (int64_t)b * P.ocap + p;
        pcur = p;
#ifdef VO_LK_CHECK
        if ((p < n0 && p >= P.cap0) || (p >= n0 && p - n0 >= P.cap1) || p >= P.ocap) {
            if (lane == 0) printf("LKCHK src b=%d p=%d n0=%d n1=%d\n", b, p, n0, n1);
            continue;
        }
#else
        (void)pcur;
#endif
        // per-point values are wave-uniform: keep them (and the addresses built from them)
        // in scalar registers
        float ptx = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(src[0])));
        float pty = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(src[1])));
        const float gtx = ptx, gty = pty;       // EX: the gate's origin
        if constexpr (EX) {
            if (P.fwd) {
                if (!__builtin_amdgcn_readfirstlane((int)P.st[oidx])) continue;   // lost by the forward pass
                ptx = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(P.fwd[2 * oidx])));
                pty = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(P.fwd[2 * oidx + 1])));
            }
        }
        int status = 1;
        float errv = 0.f;
        float ox = 0.f, oy = 0.f;   // nextPts[ptidx]
        for (level = level_hi; level >= level_lo; --level) {
        cols = P.lw[level]; rows = P.lh[level]; pitch = P.lpitch[level]; loff = (int)P.loff[level];
        const unsigned colsW = (unsigned)(cols + WW), rowsW = (unsigned)(rows + WH);
        const float sc = __builtin_ldexpf(1.f, -level);     // 1 / 2^level, exact (no f64 division)
        float px = ptx * sc, py = pty * sc;
        if (level == P.L) {
            ox = px; oy = py;
            if constexpr (EX) {
                if (P.init) {
                    ox = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(P.init[2 * oidx]))) * sc;
                    oy = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(P.init[2 * oidx + 1]))) * sc;
                }
            }
        }
        else if (level == level_hi) {
            ox = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(P.out[2 * oidx]))) * 2.f;
            oy = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(P.out[2 * oidx + 1]))) * 2.f;
        } else {                // fused levels: the previous level's estimate, still in registers
            ox *= 2.f;
            oy *= 2.f;
        }
        px -= hx;
        py -= hy;
        const int ipx = (int)floorf(px), ipy = (int)floorf(py);
        do {
            if ((unsigned)(ipx + WW) >= colsW || (unsigned)(ipy + WH) >= rowsW) {   // outside the level
                if (level == 0) { status = 0; errv = 0.f; }
                break;
            }
            // stage I (u8) and dI (int16 x2) rows under the window, together with the J tile
            // of the first iteration (same bounds test as the iteration's): one round trip
            bool staged = false;
            {
                LKPROF_T(ti0);
                const int gx = ipx + VO_BORDER, gy = ipy + VO_BORDER;
                const int ish = gx & 3;
                const int ln = lane;
                const int vi = loff + gy * pitch + (gx & ~3) + (ln >> 3) * pitch + 4 * (ln & 7);   // 8 dwords / row
                // 16 (dx, dy) per row; lane -> row 4k + 2 ((ln >> 4) & 1) + (ln >> 5): the two rows a
                // 32-lane half stores are 2 apart (2 QS = 48 dwords, 16 banks), so the ds_write_b32
                // of DR below is conflict-free (rows r, r + 1 at QS = 24 collided 2-way)
                const int drow = 2 * ((ln >> 4) & 1) + (ln >> 5);
                const int vd = 4 * (loff + gy * pitch + gx + drow * pitch + (ln & 15));
                uint32_t vir[NIR], vdd[NDR], vjr[2][NJR];
#pragma unroll
                for (int k = 0; k < NIR; ++k) {
                    LKCHKO(vi + 8 * k * pitch, P.pstride, "I");
                    vir[k] = __builtin_amdgcn_raw_buffer_load_b32(rI, vi, 8 * k * pitch, 0);
                }
#pragma unroll
                for (int k = 0; k < NDR; ++k) {
                    LKCHKO(vd + 16 * k * pitch, 2 * P.dstride, "D");
                    vdd[k] = __builtin_amdgcn_raw_buffer_load_b32(rD, vd, 16 * k * pitch, 0);
                }
                {
                    const int jx = (int)floorf(ox - hx), jy = (int)floorf(oy - hy);
                    staged = LK_JPRE && (unsigned)(jx + WW) < colsW && (unsigned)(jy + WH) < rowsW && P.max_count > 0;
                    if (staged) {
                        LKPROF_ADD(3, 1);
                        j_origin(jx, jy);
                        j_issue(vjr);
                    } else {
                        tx0 = ty0 = -(1 << 28);        // no tile: the first iteration's test restages
                    }
                }
                wave_lds_sync();
#pragma unroll
                for (int k = 0; k < NIR; ++k) {
                    const int r = (ln >> 3) + 8 * k, c = ln & 7;
                    if (c < IRS) IR[r * IRS + c] = vir[k];
                }
#pragma unroll
                for (int k = 0; k < NDR; ++k) {
                    const int r = drow + 4 * k, c = ln & 15;
                    DR[r * QS + c] = vdd[k];
                }
                if (staged) j_store(vjr);      // syncs
                else wave_lds_sync();
                LKPROF_T(ti1);
                LKPROF_ADD(4, ti1 - ti0);
                float a = px - ipx, bb = py - ipy;
                const int iw00 = __float2int_rn((1.f - a) * (1.f - bb) * (float)(1 << 14));
                const int iw01 = __float2int_rn(a * (1.f - bb) * (float)(1 << 14));
                const int iw10 = __float2int_rn((1.f - a) * bb * (float)(1 << 14));
                const int iw11 = (1 << 14) - iw00 - iw01 - iw10;
                int ival[MAXJ], ixv[MAXJ], iyv[MAXJ];
                // dot accumulator seed 256 - 512 * I: the iteration's (bilinear sum + 256) >> 9 - I
                // becomes one arithmetic shift of the seeded sum (exact: the sum is >= 0 and
                // 512 * I is a multiple of the shift; the int32 result is in range)
                uint32_t iseed[MAXJ];
                int a11 = 0, a12 = 0, a22 = 0;
                // dI taps as int16 pairs against packed int16 weight pairs: two v_dot2_i32_i16
                // per sum (exact: |dI| <= 4080, weights <= 2^14)
                const v2i16 wp0 = as_v2i16((uint32_t)(iw00 & 0xffff) | ((uint32_t)iw01 << 16));
                const v2i16 wp1 = as_v2i16((uint32_t)(iw10 & 0xffff) | ((uint32_t)iw11 << 16));
#pragma unroll
                for (int j = 0; j < MAXJ; ++j) {
                    const uint8_t* s = ir8 + toff[j] + ish;
                    const uint32_t* d = DR + toff[j];
                    const uint32_t d00 = d[0], d01 = d[1], d10 = d[QS], d11 = d[QS + 1];
                    const int v = DESCALE(__mul24((int)s[0], iw00) + __mul24((int)s[1], iw01) +
                                          __mul24((int)s[QS], iw10) + __mul24((int)s[QS + 1], iw11), 9);
                    const int gx2 = __builtin_amdgcn_sdot2(as_v2i16(__builtin_amdgcn_perm(d11, d10, 0x05040100u)), wp1,
                                        sdot2_sacc(__builtin_amdgcn_perm(d01, d00, 0x05040100u), v2u(wp0), 1 << 13),
                                        false) >> 14;
                    const int gy2 = __builtin_amdgcn_sdot2(as_v2i16(__builtin_amdgcn_perm(d11, d10, 0x07060302u)), wp1,
                                        sdot2_sacc(__builtin_amdgcn_perm(d01, d00, 0x07060302u), v2u(wp0), 1 << 13),
                                        false) >> 14;
                    // a dead slot's I needs no mask: its gradients are zeroed below, so its
                    // mismatch never reaches b1 / b2 (|J - I| <= 8160 still fits the int16 pair),
                    // and the level-0 error masks it by live[j]
                    ival[j] = v;
                    iseed[j] = 256u - ((uint32_t)ival[j] << 9);
                    ixv[j] = live[j] ? gx2 : 0;
                    iyv[j] = live[j] ? gy2 : 0;
                }
                // the gradients as int16 pairs of pixels (0, 1) and (2, 3) (|dI| <= 4080): the
                // tensor here and the iteration's b1, b2 below are v_dot2_i32_i16 sums (exact)
                const v2i16 gxp0 = as_v2i16(__builtin_amdgcn_perm((uint32_t)ixv[1], (uint32_t)ixv[0], 0x05040100u));
                const v2i16 gxp1 = as_v2i16(__builtin_amdgcn_perm((uint32_t)ixv[3], (uint32_t)ixv[2], 0x05040100u));
                const v2i16 gyp0 = as_v2i16(__builtin_amdgcn_perm((uint32_t)iyv[1], (uint32_t)iyv[0], 0x05040100u));
                const v2i16 gyp1 = as_v2i16(__builtin_amdgcn_perm((uint32_t)iyv[3], (uint32_t)iyv[2], 0x05040100u));
                a11 = __builtin_amdgcn_sdot2(gxp0, gxp0, sdot2_0(v2u(gxp1), v2u(gxp1)), false);
                a12 = __builtin_amdgcn_sdot2(gxp0, gyp0, sdot2_sacc(v2u(gxp1), v2u(gyp1), 1 << 24), false);   // a12 + 2^24
                a22 = __builtin_amdgcn_sdot2(gyp0, gyp0, sdot2_0(v2u(gyp1), v2u(gyp1)), false);
                // one exact 32-bit reduction each when every lane has a11, a22 (>= 0) and the seeded
                // a12 below 2^25 (|a12| < 2^24): the 64 partials then sum below 2^31 (the a12 seeds
                // come off as 2^30); otherwise the split sums
                const bool twide = __ballot(max(max((uint32_t)a11, (uint32_t)a22), (uint32_t)a12) >= (1u << 25)) != 0;
                const float FLT_SCALE = 1.f / (1 << 20);
                float A11, A12, A22;
                if (!twide) {
                    wave_sum3_swap(a11, a22, a12);
                    A11 = (float)a11 * FLT_SCALE; A12 = (float)(a12 - (1 << 30)) * FLT_SCALE; A22 = (float)a22 * FLT_SCALE;
                } else {
                    A11 = (float)wave_sum_split(a11) * FLT_SCALE; A12 = (float)wave_sum_split(a12 - (1 << 24)) * FLT_SCALE;
                    A22 = (float)wave_sum_split(a22) * FLT_SCALE;
                }
                float D = A11 * A22 - A12 * A12;
                // minEig = (A22 + A11 - sqrtf(t)) / (2 WW WH) against min_eig: the correctly rounded
                // sqrt and division (~30 VALU) only where the raw v_sqrt_f32 (<= 2 ulp) and a
                // multiply by the reciprocal cannot settle the comparison.  Their error is below
                // 2^-21 (s + sum) / (2 WW WH) + 2^-21 |m|, inside the margin mg (exact decision).
                const float tq = (A11 - A22) * (A11 - A22) + 4.f * A12 * A12;
                const float sum2 = A22 + A11;
                const float sa = __builtin_amdgcn_sqrtf(tq);
                const float inv_n = 1.f / (float)(2 * WW * WH);
                const float ma = (sum2 - sa) * inv_n;
                const float mg = __builtin_fmaf(0x1p-20f, (sa + sum2) * inv_n + fabsf(ma), 0x1p-100f);
                if constexpr (EX) {
                    if (P.eig_err && level == 0) errv = (sum2 - sqrtf(tq)) / (float)(2 * WW * WH);
                }
                bool reject;
                if (ma + mg < P.min_eig) reject = true;
                else if (ma - mg >= P.min_eig) reject = false;
                else reject = (sum2 - sqrtf(tq)) / (float)(2 * WW * WH) < P.min_eig;
                if (reject || D < FLT_EPSILON) {
                    if (level == 0) status = 0;
                    break;
                }
                D = 1.f / D;
                float nx = ox - hx, ny = oy - hy;
                float pdx = 0.f, pdy = 0.f;
                LKPROF_T(ta1);
                LKPROF_ADD(5, ta1 - ti1);
                for (int it = 0; it < P.max_count; ++it) {
                    // floor(n) as a float is exact, so n - floor(n) == n - (float)(int)floor(n)
                    const float fnx = floorf(nx), fny = floorf(ny);
                    const int inx = (int)fnx, iny = (int)fny;
                    // inx < -WW || inx >= cols || iny < -WH || iny >= rows, as two unsigned compares
                    if ((unsigned)(inx + WW) >= colsW || (unsigned)(iny + WH) >= rowsW) {
                        if (level == 0) status = 0;
                        break;
                    }
                    // (tx0, ty0 hold a far-away sentinel while no tile is staged at this level)
                    if ((unsigned)(inx - tx0) > 2u * LK_M || (unsigned)(iny - ty0) > 2u * LK_M) stage_j(inx, iny);
                    a = nx - fnx;
                    bb = ny - fny;
                    // wave-uniform weights: into scalar registers, packed by the scalar unit.
                    // cvRound(w) for w in [0, 2^14] is the low bits of the float w + 1.5 * 2^23
                    // (the add rounds half to even at unit spacing, as rint does), so one VALU add
                    // replaces round + convert; the bit fields the packing takes are those of w.
                    // (x * y) * 2^14 == (x * 2^14) * y exactly (power-of-two scaling, normal
                    // range), so the three products share two scaled factors.
                    const float LK_RND = 12582912.f;
                    const float xa = (1.f - a) * (float)(1 << 14), ya = 1.f - bb;
                    const uint32_t u00 = (uint32_t)to_sgpr(__float_as_int(xa * ya + LK_RND));
                    const uint32_t u01 = (uint32_t)to_sgpr(__float_as_int((a * (float)(1 << 14)) * ya + LK_RND));
                    const uint32_t u10 = (uint32_t)to_sgpr(__float_as_int(xa * bb + LK_RND));
                    const int w11 = (int)((1u << 14) + 3u * 0x4B400000u - u00 - u01 - u10);
                    // iw11 can be -1: dot with w11 + 1 and subtract the tap once
                    const int neg = w11 < 0;
                    uint32_t wlo, whi;
                    pack_w8(u00, u01, u10, (uint32_t)(w11 + neg), wlo, whi);
                    const uint32_t* tb = QT + (iny - ty0) * QS + (inx - tx0);
                    int b1 = 0, b2 = 0;
                    // all four quads read before the (wave-uniform) branch: one LDS round trip
                    uint32_t qv[MAXJ];
#pragma unroll
                    for (int j = 0; j < MAXJ; ++j) qv[j] = tb[toff[j]];
                    // the iw11 = -1 correction only in its own (wave-uniform) copy of the loop
                    auto mismatch = [&](auto negc) {
                        uint32_t dd[MAXJ];
#pragma unroll
                        for (int j = 0; j < MAXJ; ++j) {
                            const uint32_t q = qv[j];
                            uint32_t sum = (__builtin_amdgcn_udot4(q, whi, 0u, false) << 8) +
                                           __builtin_amdgcn_udot4(q, wlo, iseed[j], false);
                            if (decltype(negc)::value) sum -= q >> 24;
                            dd[j] = (uint32_t)((int)sum >> 9);       // |diff| <= 8160: an int16
                        }
                        // b1 = sum diff * Ix, b2 = sum diff * Iy as int16-pair dot products, each
                        // seeded with 2^24 (an SGPR operand): b' = b + 2^24
                        const uint32_t d01 = __builtin_amdgcn_perm(dd[1], dd[0], 0x05040100u);
                        const uint32_t d23 = __builtin_amdgcn_perm(dd[3], dd[2], 0x05040100u);
                        b1 = __builtin_amdgcn_sdot2(as_v2i16(d01), gxp0, sdot2_sacc(d23, v2u(gxp1), 1 << 24), false);
                        b2 = __builtin_amdgcn_sdot2(as_v2i16(d01), gyp0, sdot2_sacc(d23, v2u(gyp1), 1 << 24), false);
                    };
                    if (neg) mismatch(std::true_type());
                    else mismatch(std::false_type());
                    // |b| < 2^24 in every lane <=> b' in [0, 2^25): then the 64 seeded partials sum
                    // exactly in int32 (< 2^31) and the seeds come off as 64 * 2^24 = 2^30
                    const bool wide = __ballot(max((uint32_t)b1, (uint32_t)b2) >= (1u << 25)) != 0;
                    // int32 -> float and int64 -> float round the same integer identically
                    float fb1, fb2;
                    if (!wide) {
                        wave_sum2_swap(b1, b2);
                        fb1 = (float)(b1 - (1 << 30)) * FLT_SCALE; fb2 = (float)(b2 - (1 << 30)) * FLT_SCALE;
                    }
                    else {
                        fb1 = (float)wave_sum_split(b1 - (1 << 24)) * FLT_SCALE;
                        fb2 = (float)wave_sum_split(b2 - (1 << 24)) * FLT_SCALE;
                    }
                    const float ddx = (A12 * fb2 - A22 * fb1) * D;
                    const float ddy = (A12 * fb1 - A11 * fb2) * D;
                    nx += ddx;
                    ny += ddy;
                    ox = nx + hx;
                    oy = ny + hy;
                    // squares of floats are exact in double, so one fma rounds the same sum; the
                    // f32 form decides it outside the margin (P.eps2_lo / eps2_hi, fill_lk)
                    const float q2 = __builtin_fmaf(ddx, ddx, ddy * ddy);
                    if (q2 <= eps2_lo) break;
                    if (!(q2 >= eps2_hi)) {
                        const double dy2 = (double)ddy * ddy;
                        if (__builtin_fma((double)ddx, (double)ddx, dy2) <= eps2) break;
                    }
                    if (it > 0 && fabsf(ddx + pdx) < 0.01f && fabsf(ddy + pdy) < 0.01f) {
                        ox -= ddx * 0.5f;
                        oy -= ddy * 0.5f;
                        break;
                    }
                    pdx = ddx;
                    pdy = ddy;
                    LKPROF_ADD(2, 1);
                }
                {
                    LKPROF_T(te);
                    LKPROF_ADD(7, te - ta1);
                }
                if (status && level == 0 && !(EX && P.eig_err)) {
                    const float fx = ox - hx, fy = oy - hy;
                    const int inx = (int)floorf(fx), iny = (int)floorf(fy);
                    if (inx < -WW || inx >= cols || iny < -WH || iny >= rows) {
                        status = 0;
                        break;
                    }
                    // the pass itself (restage, taps, reduction) only where err is wanted
                    if (EX ? !P.err : !ERR) break;
                    if ((unsigned)(inx - tx0) > 2u * LK_M || (unsigned)(iny - ty0) > 2u * LK_M) stage_j(inx, iny);
                    const float aa = fx - inx, cc = fy - iny;
                    const int w00 = __float2int_rn((1.f - aa) * (1.f - cc) * (float)(1 << 14));
                    const int w01 = __float2int_rn(aa * (1.f - cc) * (float)(1 << 14));
                    const int w10 = __float2int_rn((1.f - aa) * cc * (float)(1 << 14));
                    const int w11 = (1 << 14) - w00 - w01 - w10;
                    const int neg = w11 < 0;
                    uint32_t wlo, whi;
                    pack_w8_v((uint32_t)w00, (uint32_t)w01, (uint32_t)w10, (uint32_t)(w11 + neg), wlo, whi);
                    const uint32_t* tb = QT + (iny - ty0) * QS + (inx - tx0);
                    int es = 0;
#pragma unroll
                    for (int j = 0; j < MAXJ; ++j) {
                        const uint32_t q = tb[toff[j]];
                        uint32_t sum = (__builtin_amdgcn_udot4(q, whi, 0u, false) << 8) +
                                       __builtin_amdgcn_udot4(q, wlo, iseed[j], false);
                        if (neg) sum -= q >> 24;
                        const int diff = (int)sum >> 9;
                        es += live[j] ? (diff < 0 ? -diff : diff) : 0;
                    }
                    errv = (float)wave_sum_dpp(es) / (float)(32 * WW * WH);
                }
            }
        } while (false);
        }   // levels
        if (lane == 0) {
            P.out[2 * oidx] = ox;
            P.out[2 * oidx + 1] = oy;
            if (level_lo == 0) {
                if constexpr (EX) {
                    if (P.fwd) {
                        const float gdx = ox - gtx, gdy = oy - gty;
                        if (!((double)gdx * gdx + (double)gdy * gdy <= P.thr2)) status = 0;
                    }
                }
                P.st[oidx] = (uint8_t)status;
                if ((EX || ERR) && P.err) P.err[oidx] = errv;
            }
        }
    }
    level = level_lo;
    LKPROF_SET(1, wall_clock64());
}

// ---------------------------------------------------- tracking compaction (:282-290)
// feature_tracking's status filtering (:283-290) as its own launch (vo_track); the engine's
// step runs the same block function at the start of the PnP block (vo_filter_pnp_triangulate)
__global__ void __launch_bounds__(256) k_track_compact(vo_dims d, vo_state s) { track_compact_block(d, s); }

}  // namespace

// ======================================================================= host side
static void fill_lk(LKParams& P, const vo_dims* d, const vo_opts* o, const vo_state* s, int prev)
{
    P.prev = s->pyr[prev];
    P.next = s->pyr[1 - prev];
    P.der = s->der[prev];
    P.pstride = d->pyr_stride;
    P.dstride = d->der_stride;
    P.L = d->nlev - 1;
    for (int l = 0; l < VO_MAX_LEVELS; ++l) {
        P.lw[l] = d->lvl_w[l];
        P.lh[l] = d->lvl_h[l];
        P.lpitch[l] = d->lvl_pitch[l];
        P.loff[l] = d->lvl_off[l];
    }
    P.win_w = o->win_w;
    P.win_h = o->win_h;
    int mc = o->crit_count;
    double eps = o->crit_eps;
    if (!(o->crit_type & 1)) mc = 30;
    else mc = mc < 0 ? 0 : (mc > 100 ? 100 : mc);
    if (!(o->crit_type & 2)) eps = 0.01;
    else eps = eps < 0 ? 0 : (eps > 10 ? 10 : eps);
    P.max_count = mc;
    P.eps2 = eps * eps;
    P.min_eig = (float)o->min_eig;
    // fl32(ddx^2 + ddy^2) (one rounded square, one fma) is within 2^-23 of the exact sum, plus
    // 2^-125 absolute near underflow: outside eps2 * (1 -+ 2^-20) it decides the double test
    // (eps2 >= 2^-100 keeps the absolute part far below the margin)
    if (P.eps2 >= 0x1p-100 && P.eps2 <= 0x1p100) {
        P.eps2_lo = nextafterf((float)(P.eps2 * (1. - 0x1p-20)), 0.f);
        P.eps2_hi = nextafterf((float)(P.eps2 * (1. + 0x1p-20)), INFINITY);
    } else {
        P.eps2_lo = -INFINITY;
        P.eps2_hi = INFINITY;
    }
    P.init = nullptr;
    P.eig_err = 0;
    P.fwd = nullptr;
    P.thr2 = 0.;
}

// ILL (with EX): an illumination model; every window then goes through k_lk, one launch per level
// (k_lk_w holds no model)
template <bool EX, int ILL = 0>
static int launch_lk_t(const LKParams& P, int B, hipStream_t st)
{
    static_assert(EX || ILL == 0, "the illumination model lives in the EX instantiations");
    const int npx = P.win_w * P.win_h;
    if (P.win_w <= 2 || P.win_h <= 2 || P.win_w > 32 || P.win_h > 32 || npx > 64 * 16 || B < 1) return VO_EARG;
    // One wave per block (iteration counts differ wildly between points, so a wave's slot
    // must free as soon as its own points are done), 2048 blocks per chain.
    static const int nb_env = vo_env_int("VO_LK_NB", 0);
    static const int xcd_env = vo_env_int("VO_LK_XCD", 0);
    // 2048 blocks per chain: at ~1,900 points per C2 chain most waves carry one point, which
    // evens out the tail (headline 56.8k vs 56.1k frames/s with 1024, 56.7k with 4096)
    const int nb = nb_env > 0 ? nb_env : 2048;
    const int nblk = (B >= 8 ? ((B + 7) / 8) * 8 : B) * nb;
    // the LDS-staged 15x15 kernel reads whole dwords: it needs >= 64 bytes of slack after
    // the last pyramid level
    const int L = P.L;
    const int64_t pyr_end = P.loff[L] + (int64_t)(P.lh[L] + 2 * VO_BORDER) * P.lpitch[L];
    const bool staged15 = ILL == 0 && P.win_w == 15 && P.win_h == 15 && P.pstride >= pyr_end + 64;
    const size_t lds = 4 * (size_t)(P.win_w + 2 * LK_M) * (P.win_h + 2 * LK_M);
    if (lds > 60 * 1024) return VO_EARG;
    // 15x15 (every reference configuration, main.py:36,66,96): all levels in one launch, each
    // wave carrying its point from the coarsest level to level 0 in registers.  Other window
    // sizes (cv2.calcOpticalFlowPyrLK's default 21x21 on the cv2compat surface): k_lk, one
    // launch per level.
    if (staged15) {
        // without EX the error pass is compiled in only for a caller that gave an err buffer
        if (EX || P.err) hipLaunchKernelGGL((k_lk_w<15, 15, EX>), dim3(nblk), dim3(64), 0, st, P, L, 0, B, nb, xcd_env);
        else hipLaunchKernelGGL((k_lk_w<15, 15, false, false>), dim3(nblk), dim3(64), 0, st, P, L, 0, B, nb, xcd_env);
        return hip_ok() ? VO_OK : VO_EHIP;
    }
    // a side beyond the materialised border: the instantiations that reflect every tap
    // (more than 256 pixels always has such a side)
    const bool big = P.win_w > VO_BORDER || P.win_h > VO_BORDER;
    for (int level = P.L; level >= 0; --level) {
        if (npx > 256) hipLaunchKernelGGL((k_lk<16, true, EX, ILL>), dim3(nblk), dim3(64), lds, st, P, level, B, nb);
        else if (big) hipLaunchKernelGGL((k_lk<4, true, EX, ILL>), dim3(nblk), dim3(64), lds, st, P, level, B, nb);
        else hipLaunchKernelGGL((k_lk<4, false, EX, ILL>), dim3(nblk), dim3(64), lds, st, P, level, B, nb);
    }
    return hip_ok() ? VO_OK : VO_EHIP;
}

static int launch_lk(const LKParams& P, int B, hipStream_t st) { return launch_lk_t<false>(P, B, st); }

// the EX launch under illumination model illum (0: none)
static int launch_lk_illum(const LKParams& P, int B, hipStream_t st, int illum)
{
    if (illum == VO_LK_ILLUM_BIAS) return launch_lk_t<true, VO_LK_ILLUM_BIAS>(P, B, st);
    if (illum == VO_LK_ILLUM_GAIN_BIAS) return launch_lk_t<true, VO_LK_ILLUM_GAIN_BIAS>(P, B, st);
    return illum == 0 ? launch_lk_t<true>(P, B, st) : VO_EARG;
}

// the argument test of launch_lk_t alone: entries that launch twice (the gate) ask before the first
static bool lk_window_ok(const vo_opts* o)
{
    const int64_t lds = 4 * (int64_t)(o->win_w + 2 * LK_M) * (o->win_h + 2 * LK_M);
    return o->win_w > 2 && o->win_h > 2 && o->win_w <= 32 && o->win_h <= 32 && o->win_w * o->win_h <= 64 * 16 &&
           lds <= 60 * 1024;
}

// The backward pass of the forward-backward gate for the forward call F (already launched on st):
// LK with flags 0 from next to prev (fill_lk with the roles swapped gives the other pyramid's
// derivatives) of F's results where F's status is 1, into `back`; each wave then writes its point's
// gate over F's status.  F's point segments stay: they give the count and the gate's origin.
static int launch_lk_back(const LKParams& F, const vo_dims* d, const vo_opts* o, const vo_state* s, int prev,
                          double thr, float* back, hipStream_t st, int illum = 0)
{
    LKParams P;
    fill_lk(P, d, o, s, 1 - prev);
    P.p0 = F.p0; P.n0 = F.n0; P.cap0 = F.cap0;
    P.p1 = F.p1; P.n1 = F.n1; P.cap1 = F.cap1; P.seg1_min = F.seg1_min;
    P.chain_status = F.chain_status;
    P.out = back; P.st = F.st; P.err = nullptr; P.ocap = F.ocap;
    P.fwd = F.out;
    P.thr2 = thr * thr;
    return launch_lk_illum(P, d->B, st, illum);
}

static bool lk_thr_ok(double thr) { return thr > 0. && thr <= DBL_MAX; }   // false for NaN too

// the engine's points: tracked landmarks, then the candidates where a chain has more than one
// (:286 "if P > 1"), into the tracking scratch
// (nothing in the step reads the L1 error, so only vo_track_fb, whose callers may, asks for it)
static void lk_state_segments(LKParams& P, const vo_dims* d, const vo_state* s, float* err)
{
    P.p0 = s->lm_kp; P.n0 = s->nL; P.cap0 = d->ncap;
    P.p1 = s->c_kp; P.n1 = s->nC; P.cap1 = d->pcap; P.seg1_min = 1;
    P.chain_status = s->status;
    P.out = s->trk_pts; P.st = s->trk_st; P.err = err; P.ocap = d->ncap + d->pcap;
}

// the caller's points: one segment of cap points per chain, every chain tracked
static void lk_point_segments(LKParams& P, const float* pts, const int32_t* counts, int32_t cap, float* out,
                              uint8_t* st, float* err)
{
    P.p0 = pts; P.n0 = counts; P.cap0 = cap;
    P.p1 = nullptr; P.n1 = nullptr; P.cap1 = 0; P.seg1_min = 0;
    P.chain_status = nullptr;
    P.out = out; P.st = st; P.err = err; P.ocap = cap;
}

extern "C" int vo_lk_points_ex(const vo_dims* d, const vo_opts* o, const vo_state* s, int prev, const float* pts,
                               const float* init, const int32_t* counts, int32_t cap, int32_t flags, float* out_pts,
                               uint8_t* out_status, float* out_err, vo_stream_t stream)
{
    if (!d || !o || !s || !pts || !counts || !out_pts || !out_status || prev < 0 || prev > 1) return VO_EARG;
    if ((flags & ~(VO_LK_USE_INITIAL_FLOW | VO_LK_GET_MIN_EIGENVALS)) || ((flags & VO_LK_USE_INITIAL_FLOW) && !init))
        return VO_EARG;
    LKParams P;
    fill_lk(P, d, o, s, prev);
    lk_point_segments(P, pts, counts, cap, out_pts, out_status, out_err);
    if (!flags) return launch_lk(P, d->B, VO_STREAM(stream));
    P.init = (flags & VO_LK_USE_INITIAL_FLOW) ? init : nullptr;
    P.eig_err = (flags & VO_LK_GET_MIN_EIGENVALS) != 0;
    return launch_lk_t<true>(P, d->B, VO_STREAM(stream));
}

extern "C" int vo_lk_points_fb(const vo_dims* d, const vo_opts* o, const vo_state* s, int prev, const float* pts,
                               const float* init, const int32_t* counts, int32_t cap, int32_t flags,
                               double fb_threshold, float* back_pts, float* out_pts, uint8_t* out_status,
                               float* out_err, vo_stream_t stream)
{
    if (!back_pts || !lk_thr_ok(fb_threshold)) return VO_EARG;
    int rc = vo_lk_points_ex(d, o, s, prev, pts, init, counts, cap, flags, out_pts, out_status, out_err, stream);
    if (rc) return rc;
    LKParams F = {};
    lk_point_segments(F, pts, counts, cap, out_pts, out_status, nullptr);
    return launch_lk_back(F, d, o, s, prev, fb_threshold, back_pts, VO_STREAM(stream));
}

extern "C" int vo_track_fb(const vo_dims* d, const vo_opts* o, const vo_state* s, int prev, double fb_threshold,
                           float* scratch, int compact, vo_stream_t stream)
{
    if (!d || !o || !s || prev < 0 || prev > 1 || !scratch || !lk_thr_ok(fb_threshold)) return VO_EARG;
    LKParams P;
    fill_lk(P, d, o, s, prev);
    lk_state_segments(P, d, s, s->trk_err);      // the one entry that still writes trk_err
    int rc = launch_lk(P, d->B, VO_STREAM(stream));
    if (rc) return rc;
    rc = launch_lk_back(P, d, o, s, prev, fb_threshold, scratch, VO_STREAM(stream));
    if (rc || !compact) return rc;
    hipLaunchKernelGGL(k_track_compact, dim3(d->B), dim3(256), 0, VO_STREAM(stream), *d, *s);
    return hip_ok() ? VO_OK : VO_EHIP;
}

// vo_track / vo_track_lk / vo_track_fb with the forward pass started at `seeds` (vo_predict_seeds):
// the EX instantiations with LKParams::init, no err buffer (so no L1-error pass), then the gate's
// backward pass, which launch_lk_back leaves unseeded
extern "C" int vo_track_seeded(const vo_dims* d, const vo_opts* o, const vo_state* s, int prev, const float* seeds,
                               double fb_threshold, float* fb_scratch, int compact, vo_stream_t stream)
{
    if (!d || !o || !s || prev < 0 || prev > 1 || !seeds) return VO_EARG;
    const bool fb = !(fb_threshold == 0.);          // NaN: a threshold, and a bad one
    if (fb && (!lk_thr_ok(fb_threshold) || !fb_scratch)) return VO_EARG;
    LKParams P;
    fill_lk(P, d, o, s, prev);
    lk_state_segments(P, d, s, nullptr);
    P.init = seeds;
    int rc = launch_lk_t<true>(P, d->B, VO_STREAM(stream));
    if (rc) return rc;
    if (fb) {
        rc = launch_lk_back(P, d, o, s, prev, fb_threshold, fb_scratch, VO_STREAM(stream));
        if (rc) return rc;
    }
    if (!compact) return VO_OK;
    hipLaunchKernelGGL(k_track_compact, dim3(d->B), dim3(256), 0, VO_STREAM(stream), *d, *s);
    return hip_ok() ? VO_OK : VO_EHIP;
}

extern "C" int vo_lk_points_illum(const vo_dims* d, const vo_opts* o, const vo_state* s, int prev, const float* pts,
                                  const float* init, const int32_t* counts, int32_t cap, int32_t flags, int32_t illum,
                                  double fb_threshold, float* back_pts, float* out_pts, uint8_t* out_status,
                                  float* out_err, vo_stream_t stream)
{
    if (!d || !o || !s || !pts || !counts || !out_pts || !out_status || prev < 0 || prev > 1) return VO_EARG;
    if ((flags & ~(VO_LK_USE_INITIAL_FLOW | VO_LK_GET_MIN_EIGENVALS)) || ((flags & VO_LK_USE_INITIAL_FLOW) && !init))
        return VO_EARG;
    if (illum != VO_LK_ILLUM_BIAS && illum != VO_LK_ILLUM_GAIN_BIAS) return VO_EARG;
    const bool fb = !(fb_threshold == 0.);          // NaN: a threshold, and a bad one
    if (fb && (!lk_thr_ok(fb_threshold) || !back_pts)) return VO_EARG;
    if (!lk_window_ok(o) || d->B < 1) return VO_EARG;
    LKParams P;
    fill_lk(P, d, o, s, prev);
    lk_point_segments(P, pts, counts, cap, out_pts, out_status, out_err);
    P.init = (flags & VO_LK_USE_INITIAL_FLOW) ? init : nullptr;
    P.eig_err = (flags & VO_LK_GET_MIN_EIGENVALS) != 0;
    int rc = launch_lk_illum(P, d->B, VO_STREAM(stream), illum);
    if (rc || !fb) return rc;
    LKParams F = {};
    lk_point_segments(F, pts, counts, cap, out_pts, out_status, nullptr);
    return launch_lk_back(F, d, o, s, prev, fb_threshold, back_pts, VO_STREAM(stream), illum);
}

// vo_track_seeded under an illumination model, seeded or not: the forward pass, the gate's backward
// pass under the same model, the compaction
extern "C" int vo_track_illum(const vo_dims* d, const vo_opts* o, const vo_state* s, int prev, int32_t illum,
                              const float* seeds, double fb_threshold, float* fb_scratch, int compact,
                              vo_stream_t stream)
{
    if (!d || !o || !s || prev < 0 || prev > 1) return VO_EARG;
    if (illum != VO_LK_ILLUM_BIAS && illum != VO_LK_ILLUM_GAIN_BIAS) return VO_EARG;
    const bool fb = !(fb_threshold == 0.);          // NaN: a threshold, and a bad one
    if (fb && (!lk_thr_ok(fb_threshold) || !fb_scratch)) return VO_EARG;
    if (!lk_window_ok(o) || d->B < 1) return VO_EARG;
    LKParams P;
    fill_lk(P, d, o, s, prev);
    lk_state_segments(P, d, s, nullptr);
    P.init = seeds;
    int rc = launch_lk_illum(P, d->B, VO_STREAM(stream), illum);
    if (rc) return rc;
    if (fb) {
        rc = launch_lk_back(P, d, o, s, prev, fb_threshold, fb_scratch, VO_STREAM(stream), illum);
        if (rc) return rc;
    }
    if (!compact) return VO_OK;
    hipLaunchKernelGGL(k_track_compact, dim3(d->B), dim3(256), 0, VO_STREAM(stream), *d, *s);
    return hip_ok() ? VO_OK : VO_EHIP;
}

extern "C" int vo_track_lk(const vo_dims* d, const vo_opts* o, const vo_state* s, int prev, vo_stream_t stream)
{
    if (!d || !o || !s || prev < 0 || prev > 1) return VO_EARG;
    LKParams P;
    fill_lk(P, d, o, s, prev);
    lk_state_segments(P, d, s, nullptr);
    return launch_lk(P, d->B, VO_STREAM(stream));
}

extern "C" int vo_track(const vo_dims* d, const vo_opts* o, const vo_state* s, int prev, vo_stream_t stream)
{
    const int rc = vo_track_lk(d, o, s, prev, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_track_compact, dim3(d->B), dim3(256), 0, VO_STREAM(stream), *d, *s);
    return hip_ok() ? VO_OK : VO_EHIP;
}

// Kept apart from vo_lk_points_ex(init = nullptr, flags = 0): this entry has never range-checked
// prev, and its return codes stay as they are.
extern "C" int vo_lk_points(const vo_dims* d, const vo_opts* o, const vo_state* s, int prev, const float* pts,
                            const int32_t* counts, int32_t cap, float* out_pts, uint8_t* out_status, float* out_err,
                            vo_stream_t stream)
{
    if (!d || !o || !s || !pts || !counts || !out_pts || !out_status) return VO_EARG;
    LKParams P;
    fill_lk(P, d, o, s, prev);
    lk_point_segments(P, pts, counts, cap, out_pts, out_status, out_err);
    return launch_lk(P, d->B, VO_STREAM(stream));
}

#ifdef VO_LK_PROF
extern "C" int vo_lk_prof_read(long long* out)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lkprof), sizeof g_lkprof) == hipSuccess ? VO_OK : VO_EHIP;
}
#endif

