// Pyramid kernels for gfx950: frame ingest + pyrDown and the Scharr derivatives of every level
// (buildOpticalFlowPyramid + calcSharrDeriv).
//
// Arithmetic follows oracle/vo_oracle_img.c operation by operation (that file restates OpenCV
// 4.6); every stage here is integer, so the bytes and derivatives are bit-exact.
#include "vo_dev.h"

namespace {

// ------------------------------------------------------------------ pyramid
// Levels are stored with a materialised VO_BORDER reflect-101 border and a 64-byte-multiple
// pitch.  One wave per row (256-thread blocks cover 4 rows); every lane writes an aligned
// vector (16, 4 or 16 bytes).  Bytes between the padded width and the pitch may be written
// with don't-care values.

// One pyramid level and its Scharr derivatives in one pass (buildOpticalFlowPyramid +
// calcSharrDeriv semantics).  A 256-thread block owns a PT_W x PT_H tile of
// the padded level: it materialises the level's values (with the reflect-101 border and a
// 1-pixel halo) in LDS, writes the tile to the pyramid with dword stores, and computes the
// int16 (dx, dy) Scharr of the tile's interior pixels from the same LDS tile.
//  * level 0: the values are frame bytes at reflect-101 coordinates;
//  * level l >= 1: cv::pyrDown of level l-1 ([1 4 6 4 1]^2 / 256).  The source rectangle
//    under the tile is staged with aligned dword loads, filtered horizontally once per
//    staged row into LDS, then vertically per output pixel (exact integers; the order of
//    the two passes does not change the result).
// The derivative image's zero border is never written: the derivative buffers are
// zero-initialised and only interior pixels are stored (zeros fill partial vectors).
#define PT_W 128
#define PT_H 16
#ifndef PYR0_TH
#define PYR0_TH 32                          // level-0 tile rows
#endif
#define PV_W (PT_W + 8)                     // tile cols px0-4 .. px0+PT_W+3
#define PV_H (PT_H + 2)                     // tile rows py0-1 .. py0+PT_H
#define PS_H (2 * PV_H + 3)                 // staged source rows (level >= 1)
#define PS_W ((2 * PV_W + 3 + 8 + 3) / 4 * 4)  // staged source cols incl. dword alignment slack

struct PyrLevelArgs {
    const uint8_t* src;     // level 0: frames [B][H][W]; else the pyramid (level l-1 inside)
    int64_t sstride;        // per chain: frame bytes or pyramid stride
    int sw, sh, spitch;     // source level l-1 (level >= 1)
    int64_t soff;
    uint8_t* pyr;           // destination pyramid (level l)
    int64_t pstride;
    int16_t* der;           // destination derivatives (level l): interleaved (dx, dy) int16 pairs
    int64_t dstride;
    int w, h, pitch;
    int64_t off;
    int level;
};

// L0: level 0 (frame bytes; its instantiation carries no source-staging LDS, so more blocks
// fit per CU).  FSRC (pyrDown levels): the source level is level 0 read straight from the frame
// at reflect-101 coordinates -- the values level 0's materialised border holds -- so level 1
// needs no level-0 tile of another block (k_pyr01 builds both in one launch).
template <bool L0, int TH, bool FSRC>
VO_DEV void pyr_tile(const PyrLevelArgs& A, int px0, int py0)
{
    constexpr int PH = TH + 2, SH = 2 * PH + 3, RPT = TH / 8;   // tile rows + halo, staged source rows, rows / thread
    __shared__ uint32_t PVw[PH * PV_W / 4];
    __shared__ int yk[PH], xc[PV_W];
    __shared__ int mm[4];
    uint8_t* PV = (uint8_t*)PVw;
    const int tid = threadIdx.x;
    const int b = blockIdx.z;
    const int pw = A.w + 2 * VO_BORDER, ph = A.h + 2 * VO_BORDER;
    // level coordinates of the tile's rows / cols (-1: outside the padded level)
    if (tid < 4) mm[tid] = (tid & 1) ? -1 : 0x7fffffff;
    __syncthreads();
    if (tid < PH) {
        const int py = py0 - 1 + tid;
        const int y = (py >= 0 && py < ph) ? refl101(py - VO_BORDER, A.h) : -1;
        yk[tid] = y;
        if (y >= 0) { atomicMin(&mm[0], y); atomicMax(&mm[1], y); }
    }
    if (tid < PV_W) {
        const int px = px0 - 4 + tid;
        const int x = (px >= 0 && px < pw) ? refl101(px - VO_BORDER, A.w) : -1;
        xc[tid] = x;
        if (x >= 0) { atomicMin(&mm[2], x); atomicMax(&mm[3], x); }
    }
    __syncthreads();
    // every load of a phase is issued before the first one is consumed (fixed trip counts,
    // unrolled): the staging is latency-bound otherwise
    constexpr int NPV = (PH * PV_W + 255) / 256;
    if constexpr (L0) {
        const uint8_t* fr = A.src + (int64_t)b * A.sstride;
        uint32_t v[NPV];
#pragma unroll
        for (int i = 0; i < NPV; ++i) {
            const int e = tid + 256 * i;
            // unconditional load from a clamped address (keeps the loads in one batch)
            const int ee = min(e, PH * PV_W - 1);
            const int k = ee / PV_W, c = ee - k * PV_W;
            const int y = yk[k], x = xc[c];
            v[i] = fr[(int64_t)max(y, 0) * A.w + max(x, 0)];
            if (y < 0 || x < 0) v[i] = 0;
        }
#pragma unroll
        for (int i = 0; i < NPV; ++i) {
            const int e = tid + 256 * i;
            if (e < PH * PV_W) PV[e] = (uint8_t)v[i];
        }
    } else {
        __shared__ uint32_t SRw[SH * PS_W / 4];
        __shared__ uint2 HSw[SH * PV_W / 4];                 // horizontal sums: u16 column quads
        const uint8_t* SR = (const uint8_t*)SRw;
        // source rectangle (level l-1 coordinates) under the tile
        const int sy0 = 2 * mm[0] - 2, sy1 = 2 * mm[1] + 2;
        const int sx0 = 2 * mm[2] - 2, sx1 = 2 * mm[3] + 2;
        const int nsr = sy1 - sy0 + 1;
        const int gx0 = sx0 + VO_BORDER;                 // padded source column of sx0
        const int ax0 = gx0 & ~3, sh = gx0 - ax0;
        const int nwd = (sx1 + VO_BORDER - ax0) / 4 + 1; // dwords per staged row
        constexpr int NSR = (SH * (PS_W / 4) + 255) / 256;
        uint32_t v[NSR];
        if constexpr (FSRC) {
            // staged byte j of row r = level-0 padded column ax0 + j = frame column
            // refl101(ax0 + j - VO_BORDER), frame row refl101(sy0 + r)
            const uint8_t* fr = A.src + (int64_t)b * A.sstride;
#pragma unroll
            for (int i = 0; i < NSR; ++i) {
                const int e = tid + 256 * i;
                const int r = e / (PS_W / 4), c = e - r * (PS_W / 4);
                const bool in = r < nsr && c < nwd;
                const uint8_t* row = fr + (int64_t)refl101(sy0 + (in ? r : 0), A.sh) * A.sw;
                const int cb = ax0 - VO_BORDER + 4 * (in ? c : 0);
                v[i] = (uint32_t)row[refl101(cb, A.sw)] | ((uint32_t)row[refl101(cb + 1, A.sw)] << 8) |
                       ((uint32_t)row[refl101(cb + 2, A.sw)] << 16) | ((uint32_t)row[refl101(cb + 3, A.sw)] << 24);
            }
        } else {
            const uint8_t* sbase = A.src + (int64_t)b * A.sstride + A.soff + ax0;
#pragma unroll
            for (int i = 0; i < NSR; ++i) {
                const int e = tid + 256 * i;
                const int r = e / (PS_W / 4), c = e - r * (PS_W / 4);
                const bool in = r < nsr && c < nwd;
                v[i] = *(const uint32_t*)(sbase + (int64_t)(sy0 + (in ? r : 0) + VO_BORDER) * A.spitch + 4 * (in ? c : 0));
            }
        }
#pragma unroll
        for (int i = 0; i < NSR; ++i) {
            const int e = tid + 256 * i;
            if (e < SH * (PS_W / 4)) SRw[e] = v[i];
        }
        __syncthreads();
        // horizontal [1 4 6 4 1] at the tile's columns, every staged row: four columns per
        // item.  Interior quads (four consecutive level columns) take their 11 source bytes
        // from four LDS dwords: byte-align to the first byte, then one v_dot4 per output with
        // weights (1,4,6,4) plus the fifth tap; quads that touch the reflect-101 border or
        // the outside of the level take the per-column path.
        static_assert(PV_W % 4 == 0, "pyrDown column quads");
        constexpr int PQ = PV_W / 4;
        uint2* HS2 = HSw;
        for (int e = tid; e < nsr * PQ; e += 256) {
            const int r = e / PQ, cq = e - r * PQ;
            const int x0 = xc[4 * cq], x3 = xc[4 * cq + 3];
            uint32_t o[4];
            if (x0 >= 0 && x3 == x0 + 3 && xc[4 * cq + 1] == x0 + 1 && xc[4 * cq + 2] == x0 + 2) {
                const int ob = r * PS_W + sh + (2 * x0 - 2 - sx0);
                const uint32_t* wp = SRw + (ob >> 2);
                const uint32_t sa = (uint32_t)(ob & 3);
                const uint32_t W0 = wp[0], W1 = wp[1], W2 = wp[2], W3 = wp[3];
                const uint32_t T0 = __builtin_amdgcn_alignbyte(W1, W0, sa);     // source bytes 0..3
                const uint32_t T1 = __builtin_amdgcn_alignbyte(W2, W1, sa);     // 4..7
                const uint32_t T2 = __builtin_amdgcn_alignbyte(W3, W2, sa);     // 8..11
                constexpr uint32_t K4 = 0x04060401u;                            // taps 1,4,6,4
                o[0] = __builtin_amdgcn_udot4(T0, K4, T1 & 0xffu, false);
                o[1] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(T1, T0, 2), K4, (T1 >> 16) & 0xffu, false);
                o[2] = __builtin_amdgcn_udot4(T1, K4, T2 & 0xffu, false);
                o[3] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(T2, T1, 2), K4, (T2 >> 16) & 0xffu, false);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int x = xc[4 * cq + i];
                    o[i] = 0;
                    if (x >= 0) {
                        const uint8_t* q = SR + r * PS_W + sh + (2 * x - 2 - sx0);
                        o[i] = q[0] + 4 * q[1] + 6 * q[2] + 4 * q[3] + q[4];
                    }
                }
            }
            HS2[r * PQ + cq] = make_uint2(o[0] | (o[1] << 16), o[2] | (o[3] << 16));
        }
        __syncthreads();
        // vertical [1 4 6 4 1] + (acc + 128) >> 8 on packed column pairs: a horizontal sum is
        // <= 16 * 255 and a vertical one <= 65280, so the two 16-bit halves never carry into
        // each other (columns outside the level hold 0 and give 0)
        const uint2* HSq = HSw;
        for (int e = tid; e < PH * PQ; e += 256) {
            const int k = e / PQ, cq = e - k * PQ;
            const int y = yk[k];
            uint32_t v = 0;
            if (y >= 0) {
                const uint2* q = HSq + (2 * y - 2 - sy0) * PQ + cq;
                const uint2 q0 = q[0], q1 = q[PQ], q2 = q[2 * PQ], q3 = q[3 * PQ], q4 = q[4 * PQ];
                const uint32_t ax = q0.x + 4 * q1.x + 6 * q2.x + 4 * q3.x + q4.x + 0x00800080u;
                const uint32_t ay = q0.y + 4 * q1.y + 6 * q2.y + 4 * q3.y + q4.y + 0x00800080u;
                // bytes (ax >> 8), (ax >> 24), (ay >> 8), (ay >> 24)
                v = __builtin_amdgcn_perm(ay, ax, 0x07050301u);
            }
            PVw[k * (PV_W / 4) + cq] = v;
        }
    }    __syncthreads();
    // 4 pixels x RPT rows per thread: pyramid dword stores, then the Scharr of interior pixels
    const int tc = tid & 31, tr = tid >> 5;
    const int px = px0 + 4 * tc;
#pragma unroll
    for (int rr = 0; rr < RPT; ++rr) {
        const int k = 1 + RPT * tr + rr;
        const int py = py0 + RPT * tr + rr;
        if (py >= ph || px >= A.pitch) continue;
        const uint32_t* rowc = PVw + (k * PV_W) / 4 + 1 + tc;      // cols px..px+3
        *(uint32_t*)(A.pyr + (int64_t)b * A.pstride + A.off + (int64_t)py * A.pitch + px) = rowc[0];
        const int y = py - VO_BORDER, x0 = px - VO_BORDER;
        if (!A.der || y < 0 || y >= A.h || x0 + 3 < 0 || x0 >= A.w) continue;
        // rows k-1, k, k+1; bytes: col px-1 = byte 3 of dword [-1], px..px+3 = dword [0],
        // px+4 = byte 0 of dword [1]
        uint32_t o[4];
        const uint32_t* ru = rowc - PV_W / 4;
        const uint32_t* rl = rowc + PV_W / 4;
        const uint64_t U = ((uint64_t)ru[0] << 8) | (ru[-1] >> 24), L = ((uint64_t)rl[0] << 8) | (rl[-1] >> 24),
                       Cc = ((uint64_t)rowc[0] << 8) | (rowc[-1] >> 24);
        const uint64_t U5 = U | ((uint64_t)(ru[1] & 0xff) << 40), L5 = L | ((uint64_t)(rl[1] & 0xff) << 40),
                       C5 = Cc | ((uint64_t)(rowc[1] & 0xff) << 40);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int dx = 0, dy = 0;
            const int x = x0 + i;
            if (x >= 0 && x < A.w) {
                const int ul = (int)((U5 >> (8 * i)) & 0xff), uc = (int)((U5 >> (8 * i + 8)) & 0xff),
                          ur = (int)((U5 >> (8 * i + 16)) & 0xff);
                const int ll = (int)((L5 >> (8 * i)) & 0xff), lc = (int)((L5 >> (8 * i + 8)) & 0xff),
                          lr = (int)((L5 >> (8 * i + 16)) & 0xff);
                const int cl = (int)((C5 >> (8 * i)) & 0xff), cr = (int)((C5 >> (8 * i + 16)) & 0xff);
                const int t0l = (ul + ll) * 3 + cl * 10;
                const int t0r = (ur + lr) * 3 + cr * 10;
                dx = t0r - t0l;
                dy = ((lr - ur) + (ll - ul)) * 3 + (lc - uc) * 10;
            }
            o[i] = (uint32_t)(uint16_t)(int16_t)dx | ((uint32_t)(uint16_t)(int16_t)dy << 16);
        }
        int16_t* dq = A.der + (int64_t)b * A.dstride + 2 * (A.off + (int64_t)py * A.pitch + px);
        *(uint4*)dq = make_uint4(o[0], o[1], o[2], o[3]);          // (dx, dy) of 4 pixels, 16 B
    }
}


// Levels 0 and 1 in one launch (few chains, where a launch is mostly latency): blocks with
// blockIdx.y < ty0 take level-0 tiles, the others level-1 tiles computed from the frame
// (pyr_tile FSRC); both grids' columns are covered by gridDim.x, surplus blocks exit.
__global__ void __launch_bounds__(256) k_pyr01(PyrLevelArgs A0, PyrLevelArgs A1, int tx0, int ty0, int tx1)
{
    if ((int)blockIdx.y < ty0) {
        if ((int)blockIdx.x < tx0) pyr_tile<true, PYR0_TH, false>(A0, blockIdx.x * PT_W, blockIdx.y * PYR0_TH);
    } else if ((int)blockIdx.x < tx1) {
        pyr_tile<false, PT_H, true>(A1, blockIdx.x * PT_W, (blockIdx.y - ty0) * PT_H);
    }
}

// k_pyr_rows<L0>: one pyramid level and its Scharr derivatives, streamed down the rows by
// single waves without LDS (round 5).  pyr_tile's blocks hold four wave slots and 25 KB of
// LDS each, so while another stream group's LK waves fill the CUs they wait for a CU to drain;
// a block of this kernel fits in the slot one finished LK wave frees.  A wave owns R level
// rows of a strip of 64 x 4 padded columns (lane = 4 consecutive columns; lanes 0 and 63 are
// halo lanes that only feed their neighbours' Scharr taps; strips step by PR_STEP columns and
// the last one is right-aligned, so it alone writes the right border):
//   level 0  row y is frame row y: two aligned dword loads and a byte align per lane (buffer
//            loads: a row end never reads past the frame buffer);
//   pyrDown  the horizontal [1 4 6 4 1] of source rows 2y-2 .. 2y+2 as packed u16 pairs (8
//            aligned source bytes per lane, the two outer taps from the neighbour lanes by DPP
//            wave shifts), kept in a five-row ring that advances two source rows per level
//            row, then the vertical taps and (acc + 128) >> 8 -- pyr_tile's integers exactly.
// Reflect-101 columns take their mirror column's byte by ds_bpermute inside the strip; the
// mirrored border rows are written by the wave that computes their source row; the Scharr of
// row y reads rows y-1, y, y+1 (the chunk's two halo rows evaluated on their own, reflect-101
// at the level's first and last row).  Same bytes and derivatives as pyr_tile.
#define PR_STEP 248
// one wave's item of a level: strip sx, rows sy R .. sy R + R - 1, chain b
// RAGGED (level 0): the frame's byte count is no multiple of 4, see ld_dw
template <bool L0, bool RAGGED = false>
VO_DEV void pyr_rows_wave(const PyrLevelArgs& A, int R, int sx, int sy, int b)
{
    const int lane = lane_id();
    const int wo = A.w, ho = A.h;
    const int pw = wo + 2 * VO_BORDER, ph = ho + 2 * VO_BORDER;
    const int pwa = (pw + 3) & ~3;
    const int ns = (pwa + PR_STEP - 1) / PR_STEP;
    const bool lastst = sx == ns - 1;
    const int base = lastst ? max(pwa - 252, -4) : sx * PR_STEP - 4;
    const int px = base + 4 * lane;
    const int y0 = sy * R;
    if (y0 >= ho || sx >= ns) return;
    const int y1 = min(y0 + R, ho);
    // columns this wave writes: [lo, hi); the earlier strips stop short of the last one's range,
    // so a border column and the Scharr taps next to it come from one wave only
    const int lo = lastst ? max(pwa - PR_STEP, 0) : sx * PR_STEP;
    const int hi = lastst ? pwa : min(sx * PR_STEP + PR_STEP, pwa - PR_STEP);
    const bool wlane = lane >= 1 && lane <= 62 && px >= lo && px < hi && px < pw;
    const bool dlane = wlane && px + 3 >= VO_BORDER && px < VO_BORDER + wo;
    // per byte of the lane: the strip position (lane * 4 + byte) holding its value
    int fsrc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = px + j;
        const int sp = (c >= 0 && c < pw) ? VO_BORDER + refl101(c - VO_BORDER, wo) : c;
        const int rel = sp - base;
        fsrc[j] = (rel >= 0 && rel < 256) ? rel : 4 * lane + j;
    }
    const bool fixcols = base < VO_BORDER || base + 256 > VO_BORDER + wo;   // wave-uniform
    auto fix = [&](uint32_t v) -> uint32_t {
        if (!fixcols) return v;
        uint32_t o = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t t = (uint32_t)__builtin_amdgcn_ds_bpermute((fsrc[j] >> 2) << 2, (int)v);
            o |= ((t >> (8 * (fsrc[j] & 3))) & 0xffu) << (8 * j);
        }
        return o;
    };
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void*)(A.src + (int64_t)b * A.sstride), (short)0, (int)A.sstride, 0x00020000);
    uint8_t* dst = A.pyr + (int64_t)b * A.pstride + A.off;
    // write level row y (+ the border rows that mirror it)
    auto put_row = [&](int y, uint32_t v) {
        if (!wlane) return;
        *(uint32_t*)(dst + (int64_t)(VO_BORDER + y) * A.pitch + px) = v;
        if (ho >= VO_BORDER + 2) {
            if (y >= 1 && y <= VO_BORDER) *(uint32_t*)(dst + (int64_t)(VO_BORDER - y) * A.pitch + px) = v;
            if (y >= ho - 1 - VO_BORDER && y <= ho - 2)
                *(uint32_t*)(dst + (int64_t)(VO_BORDER + 2 * ho - 2 - y) * A.pitch + px) = v;
        } else {
            for (int py = 0; py < ph; ++py) {
                if (py == VO_BORDER) py = VO_BORDER + ho;
                if (py < ph && refl101(py - VO_BORDER, ho) == y) *(uint32_t*)(dst + (int64_t)py * A.pitch + px) = v;
            }
        }
    };
    // Scharr of level row y from rows u = y-1, c = y, l = y+1 (calcSharrDeriv, as pyr_tile)
    auto put_der = [&](int y, uint32_t u, uint32_t c, uint32_t l) {
        const uint32_t ul = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x138, 0xF, 0xF, false);   // lane - 1
        const uint32_t cl = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)c, 0x138, 0xF, 0xF, false);
        const uint32_t ll = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)l, 0x138, 0xF, 0xF, false);
        const uint32_t ur = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x130, 0xF, 0xF, false);   // lane + 1
        const uint32_t cr = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)c, 0x130, 0xF, 0xF, false);
        const uint32_t lr = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)l, 0x130, 0xF, 0xF, false);
        if (!dlane || !A.der) return;
        const uint64_t U5 = ((uint64_t)u << 8) | (ul >> 24) | ((uint64_t)(ur & 0xff) << 40);
        const uint64_t L5 = ((uint64_t)l << 8) | (ll >> 24) | ((uint64_t)(lr & 0xff) << 40);
        const uint64_t C5 = ((uint64_t)c << 8) | (cl >> 24) | ((uint64_t)(cr & 0xff) << 40);
        uint32_t o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int dx = 0, dy = 0;
            const int x = px + i - VO_BORDER;
            if (x >= 0 && x < wo) {
                const int uL = (int)((U5 >> (8 * i)) & 0xff), uc = (int)((U5 >> (8 * i + 8)) & 0xff),
                          uR = (int)((U5 >> (8 * i + 16)) & 0xff);
                const int lL = (int)((L5 >> (8 * i)) & 0xff), lc = (int)((L5 >> (8 * i + 8)) & 0xff),
                          lR = (int)((L5 >> (8 * i + 16)) & 0xff);
                const int cL = (int)((C5 >> (8 * i)) & 0xff), cR = (int)((C5 >> (8 * i + 16)) & 0xff);
                dx = ((uR + lR) * 3 + cR * 10) - ((uL + lL) * 3 + cL * 10);
                dy = ((lR - uR) + (lL - uL)) * 3 + (lc - uc) * 10;
            }
            o[i] = (uint32_t)(uint16_t)(int16_t)dx | ((uint32_t)(uint16_t)(int16_t)dy << 16);
        }
        int16_t* dq = A.der + (int64_t)b * A.dstride + 2 * (A.off + (int64_t)(VO_BORDER + y) * A.pitch + px);
        *(uint4*)dq = make_uint4(o[0], o[1], o[2], o[3]);
    };
    if constexpr (L0) {
        // A dword load that crosses the end of the chain's buffer returns 0 as a whole, so when
        // the frame's byte count is no multiple of 4 (131x67, 1242x375) its last 1-3 pixels are
        // fetched as bytes (which read 0 past the end on their own).
        // Frames of whole dwords keep the plain instantiation (vo_pyr_build picks it).
        auto ld_dw = [&](int o) -> uint32_t {
            uint32_t v = __builtin_amdgcn_raw_buffer_load_b32(rs, o, 0, 0);
            if constexpr (RAGGED) {
                const int fbytes = (int)A.sstride;
                if (o < fbytes && o + 4 > fbytes) {
                    v = 0;
#pragma unroll
                    for (int k = 0; k < 3; ++k) v |= (uint32_t)(uint8_t)__builtin_amdgcn_raw_buffer_load_b8(rs, o + k, 0, 0) << (8 * k);
                }
            }
            return v;
        };
        // frame row y: bytes px - B .. px - B + 3 (byte align shift uniform over the wave)
        auto ld_row = [&](int y, uint32_t& d0, uint32_t& d1) {
            const int ro = y * wo + base - VO_BORDER;
            const int al = (ro & ~3) + 4 * lane;
            d0 = ld_dw(al);
            d1 = ld_dw(al + 4);
        };
        auto val = [&](int y, uint32_t d0, uint32_t d1) {
            return fix(__builtin_amdgcn_alignbyte(d1, d0, (uint32_t)((y * wo + base - VO_BORDER) & 3)));
        };
        uint32_t a0, a1, c0, c1, n0, n1;
        const int yh = refl101(y0 - 1, ho);
        ld_row(yh, a0, a1);
        ld_row(y0, c0, c1);
        ld_row(y0 + 1 < y1 ? y0 + 1 : refl101(y1, ho), n0, n1);
        uint32_t vu = val(yh, a0, a1);
        uint32_t vc = val(y0, c0, c1);
        put_row(y0, vc);
        for (int y = y0; y < y1; ++y) {
            const int yn = y + 1 < y1 ? y + 1 : refl101(y1, ho);
            const uint32_t vl = val(yn, n0, n1);
            // the row after next, in flight while this row's Scharr runs
            const int y2 = y + 2 < y1 ? y + 2 : refl101(y1, ho);
            if (y + 1 < y1) ld_row(y2, n0, n1);
            if (y + 1 < y1) put_row(y + 1, vl);
            put_der(y, vu, vc, vl);
            vu = vc;
            vc = vl;
        }
    } else {
        const int loff = 2 * px - VO_BORDER;              // 8-aligned source column of byte 0
        auto ld_src = [&](int sr, uint32_t& d0, uint32_t& d1) {
            const int o = (int)A.soff + (VO_BORDER + sr) * A.spitch + loff;
            d0 = __builtin_amdgcn_raw_buffer_load_b32(rs, o, 0, 0);
            d1 = __builtin_amdgcn_raw_buffer_load_b32(rs, o + 4, 0, 0);
        };
        constexpr uint32_t K4 = 0x04060401u;               // taps 1, 4, 6, 4 (+ the fifth)
        auto hsum = [&](uint32_t D0, uint32_t D1, uint32_t& h01, uint32_t& h23) {
            const uint32_t L1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)D1, 0x138, 0xF, 0xF, false);   // lane - 1
            const uint32_t R0 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)D0, 0x130, 0xF, 0xF, false);   // lane + 1
            const uint32_t o0 = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(D0, L1, 2), K4, (D0 >> 16) & 0xffu, false);
            const uint32_t o1 = __builtin_amdgcn_udot4(D0, K4, D1 & 0xffu, false);
            const uint32_t o2 = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(D1, D0, 2), K4, (D1 >> 16) & 0xffu, false);
            const uint32_t o3 = __builtin_amdgcn_udot4(D1, K4, R0 & 0xffu, false);
            h01 = o0 | (o1 << 16);
            h23 = o2 | (o3 << 16);
        };
        auto vert = [&](const uint32_t (&hx)[5], const uint32_t (&hy)[5]) {
            const uint32_t ax = hx[0] + 4 * hx[1] + 6 * hx[2] + 4 * hx[3] + hx[4] + 0x00800080u;
            const uint32_t ay = hy[0] + 4 * hy[1] + 6 * hy[2] + 4 * hy[3] + hy[4] + 0x00800080u;
            return fix(__builtin_amdgcn_perm(ay, ax, 0x07050301u));
        };
        // one level row on its own (the halo rows): five source rows, loads issued together
        auto direct = [&](int y) {
            uint32_t d[5][2], hx[5], hy[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) ld_src(2 * y - 2 + k, d[k][0], d[k][1]);
#pragma unroll
            for (int k = 0; k < 5; ++k) hsum(d[k][0], d[k][1], hx[k], hy[k]);
            return vert(hx, hy);
        };
        uint32_t hx[5], hy[5];
        {
            uint32_t d[5][2];
#pragma unroll
            for (int k = 0; k < 5; ++k) ld_src(2 * y0 - 2 + k, d[k][0], d[k][1]);
#pragma unroll
            for (int k = 0; k < 5; ++k) hsum(d[k][0], d[k][1], hx[k], hy[k]);
        }
        uint32_t p0, p1, q0, q1;                           // source rows 2y+3, 2y+4, in flight
        ld_src(2 * y0 + 3, p0, p1);
        ld_src(2 * y0 + 4, q0, q1);
        uint32_t vu = direct(refl101(y0 - 1, ho));
        uint32_t vc = vert(hx, hy);
        put_row(y0, vc);
        for (int y = y0; y < y1; ++y) {
            uint32_t vl;
            if (y + 1 < y1) {
                hx[0] = hx[2]; hy[0] = hy[2];
                hx[1] = hx[3]; hy[1] = hy[3];
                hx[2] = hx[4]; hy[2] = hy[4];
                hsum(p0, p1, hx[3], hy[3]);
                hsum(q0, q1, hx[4], hy[4]);
                ld_src(2 * y + 5, p0, p1);
                ld_src(2 * y + 6, q0, q1);
                vl = vert(hx, hy);
                put_row(y + 1, vl);
            } else {
                vl = direct(refl101(y1, ho));
            }
            put_der(y, vu, vc, vl);
            vu = vc;
            vc = vl;
        }
    }
}

template <bool L0, bool RAGGED = false>
__global__ void __launch_bounds__(64) k_pyr_rows(PyrLevelArgs A, int R)
{
    pyr_rows_wave<L0, RAGGED>(A, R, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z);
}

// The small pyrDown levels of few chains in one launch (round 5): one 16-wave block per chain
// walks the levels in order, each wave taking (strip, row chunk) items of pyr_rows_wave, with a
// block barrier between levels (a level reads the one before).  At a few chains each level
// launch of k_pyr_rows was a ~12 us step of the frame's latency chain, mostly launch and
// dependency wait; the same items give the same bytes.
#define PYR_TAIL_MAX 6
struct PyrTailArgs {
    PyrLevelArgs a[PYR_TAIL_MAX];
    int R[PYR_TAIL_MAX];
    int n;
};
__global__ void __launch_bounds__(1024) k_pyr_tail(PyrTailArgs T)
{
    const int w = wave_id(), nw = (int)(blockDim.x >> 6);
    for (int l = 0; l < T.n; ++l) {
        const PyrLevelArgs& A = T.a[l];
        const int R = T.R[l];
        const int pwa = (A.w + 2 * VO_BORDER + 3) & ~3;
        const int ns = (pwa + PR_STEP - 1) / PR_STEP, nch = (A.h + R - 1) / R;
        for (int it = w; it < ns * nch; it += nw) pyr_rows_wave<false>(A, R, it % ns, it / ns, (int)blockIdx.x);
        __syncthreads();
    }
}

// Scharr (calcSharrDeriv) of one level: interleaved int16 (dx, dy) pairs, zero outside the
// image (the derivative image's constant border); 4 pixels (16 bytes) per lane
__global__ void __launch_bounds__(256) k_scharr(const uint8_t* __restrict__ pyr, int64_t pstride,
                                                int16_t* __restrict__ der, int64_t dstride,
                                                int w, int h, int pitch, int64_t off)
{
    const int b = blockIdx.z;
    const int px0 = (blockIdx.x * 64 + lane_id()) * 4;
    const int py = blockIdx.y * 4 + wave_id();
    if (px0 >= w + 2 * VO_BORDER || py >= h + 2 * VO_BORDER) return;
    const int y = py - VO_BORDER;
    const uint8_t* c = pyr + b * pstride + off + (int64_t)py * pitch;
    const uint8_t* u = c - pitch;   // reflect-101 border rows/cols are materialised
    const uint8_t* l = c + pitch;
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int px = px0 + k, x = px - VO_BORDER;
        int dx = 0, dy = 0;
        if (x >= 0 && x < w && y >= 0 && y < h) {
            const int t0l = (u[px - 1] + l[px - 1]) * 3 + c[px - 1] * 10;
            const int t0r = (u[px + 1] + l[px + 1]) * 3 + c[px + 1] * 10;
            const int t1l = l[px - 1] - u[px - 1], t1c = l[px] - u[px], t1r = l[px + 1] - u[px + 1];
            dx = t0r - t0l;
            dy = (t1r + t1l) * 3 + t1c * 10;
        }
        o[k] = (uint32_t)(uint16_t)(int16_t)dx | ((uint32_t)(uint16_t)(int16_t)dy << 16);
    }
    int16_t* dq = der + b * dstride + 2 * (off + (int64_t)py * pitch + px0);
    *(uint4*)dq = make_uint4(o[0], o[1], o[2], o[3]);
}

}  // namespace

// ======================================================================= host side
// Level l's kernel arguments: the source is the frame for level 0, else level l - 1 of the same
// pyramid.  False where the level's pitch cannot hold the vector stores.
static bool pyr_level_args(const vo_dims* d, const vo_state* s, int cur, int l, const uint8_t* frames,
                           int64_t frame_stride, PyrLevelArgs* A)
{
    if (l == 0) {
        A->src = frames; A->sstride = frame_stride; A->sw = A->sh = A->spitch = 0; A->soff = 0;
    } else {
        A->src = s->pyr[cur]; A->sstride = d->pyr_stride;
        A->sw = d->lvl_w[l - 1]; A->sh = d->lvl_h[l - 1]; A->spitch = d->lvl_pitch[l - 1]; A->soff = d->lvl_off[l - 1];
    }
    A->pyr = s->pyr[cur]; A->pstride = d->pyr_stride;
    A->der = s->der[cur]; A->dstride = d->der_stride;
    A->w = d->lvl_w[l]; A->h = d->lvl_h[l]; A->pitch = d->lvl_pitch[l]; A->off = d->lvl_off[l];
    A->level = l;
    return A->pitch % 64 == 0 && A->pitch >= A->w + 2 * VO_BORDER;
}

extern "C" int vo_pyr_build(const vo_dims* d, const vo_state* s, int cur, const uint8_t* frames,
                            int64_t frame_stride, vo_stream_t stream)
{
    if (!d || !s || !frames || cur < 0 || cur > 1 || d->nlev < 1) return VO_EARG;
    // very few chains (the drop-in class's one): levels 0 and 1 in one launch (k_pyr01; one chain
    // 1,992-2,015 -> 2,029-2,049 frames/s eager).  At 32 chains per launch (the sequence job) the
    // fused kernel's 30 KB of LDS and byte-wise frame staging cost more than the launch saves
    // (29.4k -> 29.0k frames/s).  VO_PYR01=0 / 1 forces it off / on.
    static const int p01_env = vo_env_int("VO_PYR01", -1);
    const bool fuse01 = d->nlev >= 2 && (p01_env >= 0 ? p01_env == 1 : d->B <= 8);
    if (fuse01) {
        PyrLevelArgs A0, A1;
        if (!pyr_level_args(d, s, cur, 0, frames, frame_stride, &A0)) return VO_EARG;
        if (!pyr_level_args(d, s, cur, 1, frames, frame_stride, &A1)) return VO_EARG;
        // level 1 reads the frame itself (pyr_tile FSRC), not the level-0 tiles of other blocks:
        // sw / sh stay level 0's size
        A1.src = frames; A1.sstride = frame_stride; A1.spitch = 0; A1.soff = 0;
        const int pw0 = A0.w + 2 * VO_BORDER, ph0 = A0.h + 2 * VO_BORDER;
        const int pw1 = A1.w + 2 * VO_BORDER, ph1 = A1.h + 2 * VO_BORDER;
        const int tx0 = (pw0 + PT_W - 1) / PT_W, ty0 = (ph0 + PYR0_TH - 1) / PYR0_TH;
        const int tx1 = (pw1 + PT_W - 1) / PT_W, ty1 = (ph1 + PT_H - 1) / PT_H;
        dim3 g(tx0 > tx1 ? tx0 : tx1, ty0 + ty1, d->B);
        hipLaunchKernelGGL(k_pyr01, g, dim3(256), 0, VO_STREAM(stream), A0, A1, tx0, ty0, tx1);
    }
    // levels 2.. of 9 to 64 chains in one launch (k_pyr_tail; VO_PYR_TAIL=0 / 1 forces it off /
    // on).  Rank 0 of the 8-GPU sequence plan (2 groups of 12 chains) 79.5-80.9k -> 83.0-83.9k
    // frames/s predicted; at one chain the per-level launches, with 48 waves a level instead of
    // 16, are faster (2,250 vs 2,185 frames/s; profiles/r5_pyr_tail_ab.jsonl)
    static const int tail_env = vo_env_int("VO_PYR_TAIL", -1);
    const int ltail = 2;
    const bool tail = d->nlev > ltail && d->nlev - ltail <= PYR_TAIL_MAX &&
                      (tail_env >= 0 ? tail_env == 1 : d->B > 8 && d->B <= 64);
    PyrTailArgs T;
    T.n = tail ? d->nlev - ltail : 0;
    for (int i = 0; i < T.n; ++i) {
        PyrLevelArgs& A = T.a[i];
        if (!pyr_level_args(d, s, cur, ltail + i, frames, frame_stride, &A)) return VO_EARG;
        // about one item per wave of the 16-wave block
        const int pwa = (A.w + 2 * VO_BORDER + 3) & ~3, ns = (pwa + PR_STEP - 1) / PR_STEP;
        const int want = ns >= 16 ? 1 : 16 / ns;
        const int R = (A.h + want - 1) / want;
        T.R[i] = R < 2 ? 2 : R;
    }
    // the other levels: row-streaming single waves (k_pyr_rows), one launch per level
    const int lend = tail ? ltail : d->nlev;
    for (int l = fuse01 ? 2 : 0; l < lend; ++l) {
        PyrLevelArgs A;
        if (!pyr_level_args(d, s, cur, l, frames, frame_stride, &A)) return VO_EARG;
        // rows per wave: 16, fewer on small levels so that a launch still has >= 8k waves
        const int pw = A.w + 2 * VO_BORDER;
        const int ns = ((pw + 3) / 4 * 4 + PR_STEP - 1) / PR_STEP;
        int R = 16;
        while (R > 4 && (int64_t)ns * ((A.h + R - 1) / R) * d->B < 8192) R >>= 1;
        dim3 g(ns, (A.h + R - 1) / R, d->B);
        if (l == 0 && (frame_stride & 3)) hipLaunchKernelGGL((k_pyr_rows<true, true>), g, dim3(64), 0, VO_STREAM(stream), A, R);
        else if (l == 0) hipLaunchKernelGGL(k_pyr_rows<true>, g, dim3(64), 0, VO_STREAM(stream), A, R);
        else hipLaunchKernelGGL(k_pyr_rows<false>, g, dim3(64), 0, VO_STREAM(stream), A, R);
    }
    if (tail) hipLaunchKernelGGL(k_pyr_tail, dim3(d->B), dim3(1024), 0, VO_STREAM(stream), T);
    return hip_ok() ? VO_OK : VO_EHIP;
}

extern "C" int vo_pyr_deriv(const vo_dims* d, const vo_state* s, int which, vo_stream_t stream)
{
    if (!d || !s || which < 0 || which > 1) return VO_EARG;
    for (int l = 0; l < d->nlev; ++l) {
        const int pw = d->lvl_w[l] + 2 * VO_BORDER, ph = d->lvl_h[l] + 2 * VO_BORDER;
        dim3 g((pw + 4 * 64 - 1) / (4 * 64), (ph + 3) / 4, d->B);
        hipLaunchKernelGGL(k_scharr, g, dim3(256), 0, VO_STREAM(stream), s->pyr[which], d->pyr_stride, s->der[which],
                           d->der_stride, d->lvl_w[l], d->lvl_h[l], d->lvl_pitch[l], d->lvl_off[l]);
    }
    return hip_ok() ? VO_OK : VO_EHIP;
}

