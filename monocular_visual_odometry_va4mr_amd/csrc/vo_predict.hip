// Constant-velocity seeds for the landmark tracks on gfx950 (engine option lk_motion_model).
//
// No reference counterpart: the reference starts every LK search at the point's old pixel
// (nextPts = None, VisualOdometryPipeLine.py:281).  The project's own definition is DESIGN 5h and
// the NumPy restatement tests/test_lk_seed_ref.py; k_predict_seeds reproduces it bit for bit (fp64,
// one rounding per operation, the Makefile's -ffp-contract=off, the sums in the order written there).
#include "vo_dev.h"

#include <math.h>

namespace {

#define PRED_THREADS 256

struct PredK {
    double k[9];
};

// info row of every chain that will be predicted or copied: landmarks seen, then three counters the
// seeding kernel adds to
__global__ void __launch_bounds__(64) k_predict_begin(vo_dims d, vo_state s, int32_t* info)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= d.B || s.status[b] != 0) return;
    const int nL = min(max(s.nL[b], 0), d.ncap);
    info[4 * b] = nL;
    info[4 * b + 1] = 0;
    info[4 * b + 2] = 0;
    info[4 * b + 3] = 0;
}

// Row p of chain blockIdx.y.  The chain's poses and K are the same for every lane (scalar loads),
// so the predicted pose is built once per wave; a landmark then costs 3 subtractions, two 3x3
// products and two divisions in fp64 and 28 bytes of traffic (12 + 8 read, 8 written).
__global__ void __launch_bounds__(PRED_THREADS) k_predict_seeds(vo_dims d, vo_state s, PredK Kc, float* seeds, int32_t* info)
{
    const int b = blockIdx.y;
    if (s.status[b] != 0) return;
    const int nL = min(max(s.nL[b], 0), d.ncap), nC = min(max(s.nC[b], 0), d.pcap);
    const int p0 = blockIdx.x * PRED_THREADS;
    if (p0 >= nL + nC) return;                      // the whole block lies past the chain's points
    const int p = p0 + threadIdx.x;
    const int nF = s.nF[b];
    // nF == 2: slot 0 is the identity and slot 1 the bootstrap pose, `boot` frames apart and not one
    const bool predict = nF >= 3 && nF <= d.fcap;
    float* out = seeds + ((int64_t)b * (d.ncap + d.pcap) + p) * 2;
    int cls = -1;                                   // 0 seeded, 1 fell back on p2 / non-finite, 2 on the bounds
    if (p >= nL) {
        if (p < nL + nC) {
            const float* c = s.c_kp + ((int64_t)b * d.pcap + (p - nL)) * 2;
            out[0] = c[0];
            out[1] = c[1];
        }
    } else if (!predict) {
        const float* kp = s.lm_kp + ((int64_t)b * d.ncap + p) * 2;
        out[0] = kp[0];
        out[1] = kp[1];
    } else {
        const double* Ra = s.pose_R + ((int64_t)b * d.fcap + (nF - 2)) * 9;
        const double* Rb = Ra + 9;
        const double* ta = s.pose_t + ((int64_t)b * d.fcap + (nF - 2)) * 3;
        const double* tb = ta + 3;
        double Rm[3][3], tm[3], Rp[3][3], tp[3];
        const double d0 = tb[0] - ta[0], d1 = tb[1] - ta[1], d2 = tb[2] - ta[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) Rm[i][j] = (Ra[i] * Rb[j] + Ra[3 + i] * Rb[3 + j]) + Ra[6 + i] * Rb[6 + j];
            tm[i] = (Ra[i] * d0 + Ra[3 + i] * d1) + Ra[6 + i] * d2;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                Rp[i][j] = (Rb[3 * i] * Rm[0][j] + Rb[3 * i + 1] * Rm[1][j]) + Rb[3 * i + 2] * Rm[2][j];
            tp[i] = ((Rb[3 * i] * tm[0] + Rb[3 * i + 1] * tm[1]) + Rb[3 * i + 2] * tm[2]) + tb[i];
        }
        const float* X = s.lm_X + ((int64_t)b * d.ncap + p) * 3;
        const float* kp = s.lm_kp + ((int64_t)b * d.ncap + p) * 2;
        const double e0 = (double)X[0] - tp[0], e1 = (double)X[1] - tp[1], e2 = (double)X[2] - tp[2];
        double c[3], q[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) c[i] = (Rp[0][i] * e0 + Rp[1][i] * e1) + Rp[2][i] * e2;
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = (Kc.k[3 * k] * c[0] + Kc.k[3 * k + 1] * c[1]) + Kc.k[3 * k + 2] * c[2];
        const double u = q[0] / q[2], v = q[1] / q[2];
        const float fu = (float)u, fv = (float)v;
        cls = 1;
        if (q[2] > 0. && isfinite(u) && isfinite(v))
            cls = (fu >= 0.f && fu < (float)d.W && fv >= 0.f && fv < (float)d.H) ? 0 : 2;
        out[0] = cls == 0 ? fu : kp[0];
        out[1] = cls == 0 ? fv : kp[1];
    }
    if (info) {
        // every lane of the wave is here again (the early exits above are the block's)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int n = __popcll(__ballot(cls == k));
            if (lane_id() == 0 && n) atomicAdd(info + 4 * b + 1 + k, n);
        }
    }
}

}  // namespace

extern "C" int vo_predict_seeds(const vo_dims* d, const vo_opts* o, const vo_state* s, float* seeds, int32_t* info,
                                vo_stream_t stream)
{
    if (!d || !o || !s || !seeds || d->B < 1 || d->ncap < 0 || d->pcap < 0 || d->ncap + d->pcap < 1) return VO_EARG;
    PredK Kc;
    for (int i = 0; i < 9; ++i) Kc.k[i] = o->K[i];
    if (info) hipLaunchKernelGGL(k_predict_begin, dim3((d->B + 63) / 64), dim3(64), 0, VO_STREAM(stream), *d, *s, info);
    const int nblk = (d->ncap + d->pcap + PRED_THREADS - 1) / PRED_THREADS;
    hipLaunchKernelGGL(k_predict_seeds, dim3(nblk, d->B), dim3(PRED_THREADS), 0, VO_STREAM(stream), *d, *s, Kc, seeds, info);
    return hip_rc();
}
