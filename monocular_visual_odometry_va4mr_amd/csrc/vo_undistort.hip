// Lens distortion on gfx950: the rectification map of a Brown-Conrady camera, the fixed-point
// bilinear remap that turns raw frames into rectified ones (engine option dist_coeffs), and the
// iterative undistortion of points.
//
// No reference counterpart: the reference only reads rectified data.  The project's own definition,
// in OpenCV's form (initUndistortRectifyMap with CV_16SC2, remap with INTER_LINEAR and a constant
// border of 0, undistortPoints with a fixed iteration count), is DESIGN 5i and the NumPy restatement
// tests/test_undistort_ref.py; the kernels reproduce it bit for bit (fp64, one rounding per
// operation, the Makefile's -ffp-contract=off, every line associated as written there; the remap
// is 32-bit integer arithmetic).
#include "vo_dev.h"

#include <math.h>

namespace {

#define UND_THREADS 256
#define UND_MAX_SIDE 16384
#define UND_QMIN (-1048576)          // the quantised coordinate's clamp: [-2^20, 2^20 - 1]
#define UND_QMAX 1048575

// a camera by value: (fx, fy, cx, cy) of K and of the new matrix, k1 k2 p1 p2 k3 k4 k5 k6
struct UndCam {
    double fx, fy, cx, cy;
    double nfx, nfy, ncx, ncy;
    double k1, k2, p1, p2, k3, k4, k5, k6;
};

// rint(32 m), round-half-even, clamped; a NaN gives the lower clamp value
VO_DEV int und_quant(double m)
{
    const double t = rint(32.0 * m);
    if (t != t) return UND_QMIN;
    return (int)fmin(fmax(t, (double)UND_QMIN), (double)UND_QMAX);
}

// one thread per destination pixel (runs once per camera)
__global__ void __launch_bounds__(UND_THREADS) k_undistort_map(UndCam c, int W, int H, int16_t* map1, uint16_t* map2,
                                                               double* mapd)
{
    const int64_t i = (int64_t)blockIdx.x * UND_THREADS + threadIdx.x;
    if (i >= (int64_t)W * H) return;
    const int v = (int)(i / W), u = (int)(i - (int64_t)v * W);
    const double x = ((double)u - c.ncx) / c.nfx, y = ((double)v - c.ncy) / c.nfy;
    const double r2 = x * x + y * y;
    const double kr = (1.0 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2) / (1.0 + ((c.k6 * r2 + c.k5) * r2 + c.k4) * r2);
    const double xd = x * kr + c.p1 * (2.0 * x * y) + c.p2 * (r2 + 2.0 * x * x);
    const double yd = y * kr + c.p1 * (r2 + 2.0 * y * y) + c.p2 * (2.0 * x * y);
    const double mx = c.fx * xd + c.cx, my = c.fy * yd + c.cy;
    if (mapd) {
        mapd[2 * i] = mx;
        mapd[2 * i + 1] = my;
    }
    const int iu = und_quant(mx), iv = und_quant(my);
    map1[2 * i] = (int16_t)(iu >> 5);
    map1[2 * i + 1] = (int16_t)(iv >> 5);
    map2[i] = (uint16_t)((iv & 31) * 32 + (iu & 31));
}

// one thread per point
__global__ void __launch_bounds__(UND_THREADS) k_undistort_points(UndCam c, int n, const double* pts, int has_p, int iters,
                                                                  double* out)
{
    const int i = blockIdx.x * UND_THREADS + threadIdx.x;
    if (i >= n) return;
    const double x0 = (pts[2 * (int64_t)i] - c.cx) / c.fx, y0 = (pts[2 * (int64_t)i + 1] - c.cy) / c.fy;
    double x = x0, y = y0;
    for (int it = 0; it < iters; ++it) {
        const double r2 = x * x + y * y;
        const double icd = (1.0 + ((c.k6 * r2 + c.k5) * r2 + c.k4) * r2) / (1.0 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2);
        const double dx = c.p1 * (2.0 * x * y) + c.p2 * (r2 + 2.0 * x * x);
        const double dy = c.p1 * (r2 + 2.0 * y * y) + c.p2 * (2.0 * x * y);
        x = (x0 - dx) * icd;
        y = (y0 - dy) * icd;
    }
    out[2 * (int64_t)i] = has_p ? c.nfx * x + c.ncx : x;
    out[2 * (int64_t)i + 1] = has_p ? c.nfy * y + c.ncy : y;
}

// four map entries with the alignment the map guarantees for any width (entries, not quads)
struct __attribute__((packed, aligned(4))) Map1x4 {
    int16_t v[8];
};
struct __attribute__((packed, aligned(2))) Map2x4 {
    uint16_t v[4];
};

// two bytes at any address (the hardware reads them in one access)
struct __attribute__((packed, aligned(1))) Pair {
    uint16_t v;
};

// One destination pixel's taps, the same for every image.  The two taps of a row are the two bytes
// of one 16-bit load at column xq = ix clamped to [0, sW - 2] (a source one pixel wide loads the
// single byte at column 0 instead, its high byte reading as 0), and the two
// rows are iy and iy + 1 clamped into the source: every load lies inside the image and can be
// issued at once.  Each tap is tested on its own and its weight goes to the byte it fell on (a tap
// outside the source has none, so that byte gets 0): at ix = sW - 1 the left tap is the pair's
// high byte, at ix = -1 the right tap is its low byte.  off: byte offsets of the two pairs in an
// image; w: the integer weights of (upper low, upper high, lower low, lower high).
VO_DEV void remap_taps(int64_t pitch, int sW, int sH, int ix, int iy, uint32_t m2, uint32_t* off, uint32_t* w)
{
    const uint32_t a = m2 & 31u, b = (m2 >> 5) & 31u;
    const int xq = max(min(ix, sW - 2), 0);
    const uint32_t t0 = (uint32_t)(ix - xq), t1 = (uint32_t)(ix + 1 - xq);     // the byte each x tap fell on: 0, 1 or none
    const uint32_t wl = (t0 == 0u ? 32u - a : 0u) + (t1 == 0u ? a : 0u);       // at most one term each: t1 = t0 + 1
    const uint32_t wh = (t0 == 1u ? 32u - a : 0u) + (t1 == 1u ? a : 0u);
    const bool y0 = (uint32_t)iy < (uint32_t)sH, y1 = (uint32_t)(iy + 1) < (uint32_t)sH;
    off[0] = (uint32_t)((int64_t)min(max(iy, 0), sH - 1) * pitch) + (uint32_t)xq;        // an image is below 2 GiB (host check)
    off[1] = (uint32_t)((int64_t)min(max(iy + 1, 0), sH - 1) * pitch) + (uint32_t)xq;
    const uint32_t wa = y0 ? 32u - b : 0u, wb = y1 ? b : 0u;
    w[0] = wl * wa;
    w[1] = wh * wa;
    w[2] = wl * wb;
    w[3] = wh * wb;
}

#define REMAP_QUADS 64           // block: 64 quads of four pixels x 4 rows
#define REMAP_ROWS 4
#define REMAP_IMGS 8             // images per thread where their rows share an alignment
#define REMAP_UNROLL 2           // images whose loads are in flight together

// Thread (q, r) of block (row group, image chunk): the four destination bytes of the dword at the
// row's aligned base + 4q, that is pixels x = 4q - s + j with s the row address's misalignment, in
// `nimg` consecutive images (1, or REMAP_IMGS where the images' rows share s: dst_stride % 4 == 0).
// The map entries, tap offsets and weights are read and made once and serve every image of the
// chunk; per image that leaves eight 16-bit loads, sixteen multiply-adds and one store.  A quad
// inside the row loads its map entries as one 16-byte and one 8-byte access and stores one dword per
// image; the row's head and tail quads go pixel by pixel and write no byte outside [0, W).
// blockIdx.x = row group * chunks + chunk: the blocks in flight together share their map rows.
template <bool ONE>          // ONE: the source is one pixel wide
__global__ void __launch_bounds__(REMAP_QUADS * REMAP_ROWS) k_remap_u8(int B, int nimg, int chunks,
                                                                       const uint8_t* __restrict__ src, int64_t src_stride,
                                                                       int64_t src_pitch, int sW, int sH,
                                                                       uint8_t* __restrict__ dst, int64_t dst_stride,
                                                                       int64_t dst_pitch, int W, int H,
                                                                       const int16_t* __restrict__ map1,
                                                                       const uint16_t* __restrict__ map2)
{
    const int b0 = (blockIdx.x % chunks) * nimg, y = (blockIdx.x / chunks) * REMAP_ROWS + threadIdx.y;
    if (y >= H) return;
    uint8_t* row = dst + (int64_t)b0 * dst_stride + (int64_t)y * dst_pitch;
    const int s = (int)((uintptr_t)row & 3u);
    const int x = 4 * (blockIdx.y * REMAP_QUADS + threadIdx.x) - s;
    if (x >= W) return;
    const int nb = min(nimg, B - b0);
    const int64_t m = (int64_t)y * W + x;
    const bool full = x >= 0 && x + 3 < W;
    uint32_t off[4][2], w[4][4];
    if (full) {
        const Map1x4 m1 = *reinterpret_cast<const Map1x4*>(map1 + 2 * m);
        const Map2x4 m2 = *reinterpret_cast<const Map2x4*>(map2 + m);
#pragma unroll
        for (int j = 0; j < 4; ++j) remap_taps(src_pitch, sW, sH, m1.v[2 * j], m1.v[2 * j + 1], m2.v[j], off[j], w[j]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = x + j >= 0 && x + j < W;          // a pixel outside the row: weights 0, offset 0, never stored
            remap_taps(src_pitch, sW, sH, in ? map1[2 * (m + j)] : -2, in ? map1[2 * (m + j) + 1] : -2, in ? map2[m + j] : 0,
                       off[j], w[j]);
        }
    }
    const uint8_t* img = src + (int64_t)b0 * src_stride;
    for (int i = 0; i < nb; i += REMAP_UNROLL) {
        uint32_t v[REMAP_UNROLL][4][2];
#pragma unroll
        for (int u = 0; u < REMAP_UNROLL; ++u) {
            const uint8_t* p = img + (int64_t)min(i + u, nb - 1) * src_stride;      // past the chunk: its last image again
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t = 0; t < 2; ++t) v[u][j][t] = ONE ? p[off[j][t]] : reinterpret_cast<const Pair*>(p + off[j][t])->v;
        }
#pragma unroll
        for (int u = 0; u < REMAP_UNROLL; ++u) {
            if (i + u >= nb) break;
            uint8_t* r = row + (int64_t)(i + u) * dst_stride;
            uint32_t o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                o[j] = (w[j][0] * (v[u][j][0] & 255u) + w[j][1] * (v[u][j][0] >> 8) + w[j][2] * (v[u][j][1] & 255u) +
                        w[j][3] * (v[u][j][1] >> 8) + 512u) >> 10;
            if (full) {
                *reinterpret_cast<uint32_t*>(r + x) = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x + j >= 0 && x + j < W) r[x + j] = (uint8_t)o[j];
            }
        }
    }
}

// K of the form [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] with finite entries and non-zero focal lengths
bool und_pinhole(const double* K)
{
    if (!(K[1] == 0. && K[3] == 0. && K[6] == 0. && K[7] == 0. && K[8] == 1.)) return false;
    if (!(isfinite(K[0]) && isfinite(K[4]) && isfinite(K[2]) && isfinite(K[5]))) return false;
    return K[0] != 0. && K[4] != 0.;
}

bool und_camera(const double* K, const double* dist, int ndist, const double* new_K, UndCam* c)
{
    if (!K || !und_pinhole(K) || (new_K && !und_pinhole(new_K))) return false;
    if (!(ndist == 0 || ndist == 4 || ndist == 5 || ndist == 8) || (ndist && !dist)) return false;
    const double* N = new_K ? new_K : K;
    double k[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
    for (int i = 0; i < ndist; ++i) k[i] = dist[i];
    *c = UndCam{K[0], K[4], K[2], K[5], N[0], N[4], N[2], N[5], k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7]};
    return true;
}

}  // namespace

extern "C" int vo_undistort_map(const double* K, const double* dist, int ndist, const double* new_K, int W, int H,
                                int16_t* map1, uint16_t* map2, double* mapd, vo_stream_t stream)
{
    UndCam c;
    if (!map1 || !map2 || W < 1 || W > UND_MAX_SIDE || H < 1 || H > UND_MAX_SIDE) return VO_EARG;
    if (!und_camera(K, dist, ndist, new_K, &c)) return VO_EARG;
    const int64_t n = (int64_t)W * H;
    hipLaunchKernelGGL(k_undistort_map, dim3((unsigned)((n + UND_THREADS - 1) / UND_THREADS)), dim3(UND_THREADS), 0,
                       VO_STREAM(stream), c, W, H, map1, map2, mapd);
    return hip_rc();
}

extern "C" int vo_remap_u8(int B, const uint8_t* src, int64_t src_stride, int64_t src_pitch, int sW, int sH, uint8_t* dst,
                           int64_t dst_stride, int64_t dst_pitch, int W, int H, const int16_t* map1, const uint16_t* map2,
                           vo_stream_t stream)
{
    if (!src || !dst || !map1 || !map2 || B < 1) return VO_EARG;
    if (W < 1 || W > UND_MAX_SIDE || H < 1 || H > UND_MAX_SIDE || sW < 1 || sW > UND_MAX_SIDE || sH < 1 || sH > UND_MAX_SIDE)
        return VO_EARG;
    if (src_pitch < sW || dst_pitch < W || src_stride < 0 || dst_stride < 0) return VO_EARG;
    const int64_t dst_img = (int64_t)(H - 1) * dst_pitch + W, src_img = (int64_t)(sH - 1) * src_pitch + sW;
    if (B > 1 && dst_stride < dst_img) return VO_EARG;          // the destination images must not overlap each other
    if (src_img > 0x7fffffffLL) return VO_EARG;                 // tap offsets inside an image are 32-bit
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)((B - 1) * dst_stride + dst_img);
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)((B - 1) * src_stride + src_img);
    if (d0 < s1 && s0 < d1) return VO_EARG;
    // the images of a thread's chunk must share their rows' alignment (the quads are cut at dword
    // boundaries of the destination)
    const int nimg = (B > 1 && dst_stride % 4 == 0) ? REMAP_IMGS : 1;
    const int64_t chunks = (B + nimg - 1) / nimg, groups = (H + REMAP_ROWS - 1) / REMAP_ROWS;
    if (groups * chunks > 0x7fffffffLL) return VO_EARG;         // the grid's x dimension
    const unsigned gy = (unsigned)((W + 3 + 4 * REMAP_QUADS - 1) / (4 * REMAP_QUADS));     // up to 3 head bytes
    const dim3 grid((unsigned)(groups * chunks), gy), block(REMAP_QUADS, REMAP_ROWS);
    if (sW == 1)
        hipLaunchKernelGGL(k_remap_u8<true>, grid, block, 0, VO_STREAM(stream), B, nimg, (int)chunks, src, src_stride, src_pitch,
                           sW, sH, dst, dst_stride, dst_pitch, W, H, map1, map2);
    else
        hipLaunchKernelGGL(k_remap_u8<false>, grid, block, 0, VO_STREAM(stream), B, nimg, (int)chunks, src, src_stride, src_pitch,
                           sW, sH, dst, dst_stride, dst_pitch, W, H, map1, map2);
    return hip_rc();
}

extern "C" int vo_undistort_points(int n, const double* pts, const double* K, const double* dist, int ndist, const double* P,
                                   int iters, double* out, vo_stream_t stream)
{
    UndCam c;
    if (n < 0 || !pts || !out || iters < 1 || iters > 100) return VO_EARG;
    if (!und_camera(K, dist, ndist, P, &c)) return VO_EARG;
    if (n == 0) return VO_OK;
    hipLaunchKernelGGL(k_undistort_points, dim3((n + UND_THREADS - 1) / UND_THREADS), dim3(UND_THREADS), 0, VO_STREAM(stream),
                       c, n, pts, P ? 1 : 0, iters, out);
    return hip_rc();
}
