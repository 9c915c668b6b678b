// Sub-pixel corner refinement in the form of cv::cornerSubPix (vo_corner_subpix, vo_gftt_subpix;
// the engine option feature_subpix_win, off by default).  The definition is the project's own
// (the NumPy restatement tests/test_subpix_ref.py) and this kernel reproduces it bit
// for bit: fp32 bilinear patch and gradient products, fp64 sums in a fixed order, one rounding
// per operation (-ffp-contract=off), exp from vo_crmath.h.
//
// One wave per corner in one-wave blocks, grid (blocks, B); a wave strides over its chain's
// corners.  Per iteration the lanes fill the (2w+3) x (2h+3) patch in LDS with bilinear samples of
// the u8 image (every coordinate clamped to the image), lane l takes taps l, l + 64, l + 128, l + 192
// in that order into its five fp64 partials, the partials fold p[l] += p[l + s], s = 32..1
// (__shfl_down across rows, DPP row shifts inside a row), and every lane repeats the 2 x 2 solve and
// the stop tests on lane 0's sums, so the control flow is wave-uniform.
#include <float.h>

#include "vo_crmath.h"
#include "vo_dev.h"

#define SPX_MAXW 7
#define SPX_PATCH ((2 * SPX_MAXW + 3) * (2 * SPX_MAXW + 3))      // 289 floats
#define SPX_DET_MIN 0x1p-104                                      // DBL_EPSILON^2
#define SPX_LOG2E 0x1.71547652b82fep+0

struct SubpixArgs {
    const uint8_t* img;      // chain b's image at img + b * img_stride + off
    int64_t img_stride, off;
    int32_t pitch, W, H;
    float* pts;              // [B][cap][2], refined in place
    const int32_t* counts;   // [B]
    int32_t cap;
    const int32_t* status;   // [B] or NULL: a chain whose status is not 0 is skipped
    int32_t w, h, zw, zh, max_iters;
    double eps2;
    int32_t* iters;          // [B][cap] or NULL
};

// v + the value of lane (l + N) of the same 16-lane row, N = 8, 4, 2, 1 (DPP row_shl: a lane whose
// source is past its row keeps its own value, which no lower lane reads afterwards)
template <int N>
VO_DEV double spx_add_row_shl(double v)
{
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int slo = __builtin_amdgcn_update_dpp(lo, lo, 0x100 + N, 0xF, 0xF, false);
    const int shi = __builtin_amdgcn_update_dpp(hi, hi, 0x100 + N, 0xF, 0xF, false);
    return v + __hiloint2double(shi, slo);
}

// fold of the definition: p[l] += p[l + s] for s = 32..1; every lane returns lane 0's sum.  The two
// steps that cross 16-lane rows go through __shfl_down, the four inside a row through DPP.
VO_DEV double spx_fold(double v)
{
    v = v + __shfl_down(v, 32, 64);
    v = v + __shfl_down(v, 16, 64);
    v = spx_add_row_shl<8>(v);
    v = spx_add_row_shl<4>(v);
    v = spx_add_row_shl<2>(v);
    v = spx_add_row_shl<1>(v);
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                            __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

__global__ void __launch_bounds__(64) k_corner_subpix(SubpixArgs A)
{
    __shared__ float S[SPX_PATCH];
    __shared__ float g1[2 * (2 * SPX_MAXW + 1)];       // gx [2w+1], then gy [2h+1]
    const int b = blockIdx.y, lane = threadIdx.x;
    if (A.status && A.status[b] != 0) return;
    int n = A.counts[b];
    if (n > A.cap) n = A.cap;
    if ((int)blockIdx.x >= n) return;                  // n <= 0 included
    const int w = A.w, h = A.h, W = A.W, H = A.H;
    const int tw = 2 * w + 1, th = 2 * h + 1, pw = tw + 2, ph = th + 2, ntap = tw * th;
    // the 1-D weights, one lane per weight
    if (lane < tw + th) {
        const int hw = lane < tw ? w : h;
        const int j = lane < tw ? lane : lane - tw;
        const float t = (float)(j - hw) / (float)hw;
        const float x = -(t * t);
        g1[lane] = (float)vcr_exp2((double)x * SPX_LOG2E);
    }
    __syncthreads();
    // this lane's taps: weight, patch index of the tap's centre, offsets from the window's centre
    float tm[4];
    int tp[4];
    double tx[4], ty[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int k = lane + 64 * q;
        tm[q] = 0.f; tp[q] = pw + 1; tx[q] = 0.; ty[q] = 0.;
        if (k < ntap) {
            const int i = k / tw, j = k - i * tw;
            float m = g1[tw + i] * g1[j];
            const int di = i - h, dj = j - w;
            if (A.zw >= 0 && di >= -A.zh && di <= A.zh && dj >= -A.zw && dj <= A.zw) m = 0.f;
            tm[q] = m;
            tp[q] = (i + 1) * pw + (j + 1);
            tx[q] = (double)dj;
            ty[q] = (double)di;
        }
    }
    // this lane's patch samples e = lane + 64 k as (row << 8 | column); -1 past the patch
    int pe[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int e = lane + 64 * k;
        const int r = e / pw;
        pe[k] = e < pw * ph ? (r << 8 | (e - r * pw)) : -1;
    }
    const uint8_t* img = A.img + (int64_t)b * A.img_stride + A.off;
    const float fW = (float)W, fH = (float)H;
    for (int c = blockIdx.x; c < n; c += gridDim.x) {
        float* p = A.pts + ((int64_t)b * A.cap + c) * 2;
        const float sx = p[0], sy = p[1];
        float cx = sx, cy = sy;
        int it = 0;
        bool go = sx >= 0.f && sx < fW && sy >= 0.f && sy < fH;       // false for NaN
        while (go) {
            const float x0 = cx - (float)(w + 1), y0 = cy - (float)(h + 1);
            const float fx = floorf(x0), fy = floorf(y0);
            const float a = x0 - fx, bq = y0 - fy;
            const int ix = (int)fx, iy = (int)fy;                      // the centre is inside the image
            const float w00 = (1.f - a) * (1.f - bq), w01 = a * (1.f - bq), w10 = (1.f - a) * bq, w11 = a * bq;
            __syncthreads();                                           // the last iteration's reads are done
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                if (pe[k] < 0) continue;
                const int e = lane + 64 * k, r = pe[k] >> 8, q = pe[k] & 255;
                const int xa = min(max(ix + q, 0), W - 1), xb = min(max(ix + q + 1, 0), W - 1);
                const int ya = min(max(iy + r, 0), H - 1), yb = min(max(iy + r + 1, 0), H - 1);
                const uint8_t* ra = img + (int64_t)ya * A.pitch;
                const uint8_t* rb = img + (int64_t)yb * A.pitch;
                const float p00 = (float)ra[xa], p01 = (float)ra[xb], p10 = (float)rb[xa], p11 = (float)rb[xb];
                S[e] = (p00 * w00 + p01 * w01) + (p10 * w10 + p11 * w11);
            }
            __syncthreads();
            double sa = 0., sb = 0., sc = 0., s1 = 0., s2 = 0.;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (lane + 64 * q < ntap) {
                    const int o = tp[q];
                    const float tgx = S[o + 1] - S[o - 1];
                    const float tgy = S[o + pw] - S[o - pw];
                    const double gxx = (double)((tgx * tgx) * tm[q]);
                    const double gxy = (double)((tgx * tgy) * tm[q]);
                    const double gyy = (double)((tgy * tgy) * tm[q]);
                    sa = sa + gxx;
                    sb = sb + gxy;
                    sc = sc + gyy;
                    s1 = s1 + (gxx * tx[q] + gxy * ty[q]);
                    s2 = s2 + (gxy * tx[q] + gyy * ty[q]);
                }
            }
            sa = spx_fold(sa); sb = spx_fold(sb); sc = spx_fold(sc); s1 = spx_fold(s1); s2 = spx_fold(s2);
            const double det = sa * sc - sb * sb;
            if (!(fabs(det) > SPX_DET_MIN)) break;                     // NaN stops too
            const double s = 1.0 / det;
            const float nx = (float)((double)cx + sc * s * s1 - sb * s * s2);
            const float ny = (float)((double)cy - sb * s * s1 + sa * s * s2);
            const double dx = (double)nx - (double)cx, dy = (double)ny - (double)cy;
            const double err = dx * dx + dy * dy;
            cx = nx; cy = ny;
            ++it;
            if (!(cx >= 0.f && cx < fW && cy >= 0.f && cy < fH)) break;
            go = it < A.max_iters && err > A.eps2;
        }
        const bool keep = cx >= 0.f && cx < fW && cy >= 0.f && cy < fH && fabsf(cx - sx) <= (float)w &&
                          fabsf(cy - sy) <= (float)h;
        if (lane == 0) {
            if (keep && it > 0) { p[0] = cx; p[1] = cy; }
            if (A.iters) A.iters[(int64_t)b * A.cap + c] = it;
        }
    }
}

static bool subpix_args_ok(int32_t w, int32_t h, int32_t zw, int32_t zh, int32_t max_iters, double eps)
{
    if (w < 1 || w > SPX_MAXW || h < 1 || h > SPX_MAXW) return false;
    if (!(zw == -1 && zh == -1) && !(zw >= 0 && zw < w && zh >= 0 && zh < h)) return false;
    if (max_iters < 1 || max_iters > 100) return false;
    return eps >= 0. && eps <= DBL_MAX;                // false for NaN
}

static int launch_subpix(SubpixArgs& A, int B, int32_t w, int32_t h, int32_t zw, int32_t zh, int32_t max_iters,
                         double eps, hipStream_t st)
{
    A.w = w; A.h = h; A.zw = zw; A.zh = zh; A.max_iters = max_iters; A.eps2 = eps * eps;
    if (A.cap == 0) return VO_OK;
    // a wave per corner where the chains are few, at least 32 waves per chain where they are many
    int nb = 8192 / B;
    nb = nb < 32 ? 32 : nb;
    nb = nb > A.cap ? A.cap : nb;
    hipLaunchKernelGGL(k_corner_subpix, dim3(nb, B), dim3(64), 0, st, A);
    return hipGetLastError() == hipSuccess ? VO_OK : VO_EHIP;
}

extern "C" int vo_corner_subpix(int B, const uint8_t* img, int64_t img_stride, int32_t pitch, int W, int H, float* pts,
                                const int32_t* counts, int32_t cap, int32_t win_w, int32_t win_h, int32_t zero_w,
                                int32_t zero_h, int32_t max_iters, double eps, int32_t* iters, vo_stream_t stream)
{
    if (B < 1 || B > 65535 || !img || !pts || !counts || cap < 0 || W < 1 || H < 1 || pitch < W || img_stride < 0)
        return VO_EARG;
    if (!subpix_args_ok(win_w, win_h, zero_w, zero_h, max_iters, eps)) return VO_EARG;
    hipStream_t st = VO_STREAM(stream);
    // the counts are checked against the capacity before anything is launched (the one host read
    // of device memory on this surface: this entry point waits for the stream and cannot be
    // captured into a graph; vo_gftt_subpix can)
    for (int b0 = 0; b0 < B; b0 += 256) {
        int32_t hc[256];
        const int nb = B - b0 < 256 ? B - b0 : 256;
        if (hipMemcpyAsync(hc, counts + b0, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, st) != hipSuccess) return VO_EHIP;
        if (hipStreamSynchronize(st) != hipSuccess) return VO_EHIP;
        for (int i = 0; i < nb; ++i)
            if (hc[i] > cap) return VO_EARG;
    }
    SubpixArgs A;
    A.img = img; A.img_stride = img_stride; A.off = 0; A.pitch = pitch; A.W = W; A.H = H;
    A.pts = pts; A.counts = counts; A.cap = cap; A.status = nullptr; A.iters = iters;
    return launch_subpix(A, B, win_w, win_h, zero_w, zero_h, max_iters, eps, st);
}

extern "C" int vo_gftt_subpix(const vo_dims* d, const vo_state* s, int cur, int32_t win_w, int32_t win_h, int32_t zero_w,
                              int32_t zero_h, int32_t max_iters, double eps, vo_stream_t stream)
{
    if (!d || !s || cur < 0 || cur > 1 || d->B < 1 || d->B > 65535 || d->W < 1 || d->H < 1 || d->mcap < 0) return VO_EARG;
    if (!subpix_args_ok(win_w, win_h, zero_w, zero_h, max_iters, eps)) return VO_EARG;
    SubpixArgs A;
    // level 0 of pyr[cur]: lvl_off[0] is the padded origin, the image starts VO_BORDER rows and
    // columns inside it; the clamp keeps every read inside the W x H image
    A.img = s->pyr[cur]; A.img_stride = d->pyr_stride;
    A.off = d->lvl_off[0] + (int64_t)VO_BORDER * d->lvl_pitch[0] + VO_BORDER;
    A.pitch = d->lvl_pitch[0]; A.W = d->W; A.H = d->H;
    A.pts = s->corners; A.counts = s->nCorners; A.cap = d->mcap; A.status = s->status; A.iters = nullptr;
    return launch_subpix(A, d->B, win_w, win_h, zero_w, zero_h, max_iters, eps, VO_STREAM(stream));
}
