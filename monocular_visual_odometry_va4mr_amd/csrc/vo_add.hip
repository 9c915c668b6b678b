// Feature adding and the step's bookkeeping for gfx950: the minimum-distance filter of the new
// corners against the existing candidates, their ordered append, and the frame counters.
//
// Reference call sites: VisualOdometryPipeLine.py:248-268 (feature_adding filter) and :360-373
// (bookkeeping).  One body, add_finish_block<Form>, in two block shapes (AddFull, AddLean).
#include "vo_dev.h"

namespace {

#define ADD_MAX_CELLS 8192
#define ADD_MAX_ITEMS 16384

struct AddArgs {
    vo_dims d;
    vo_state s;
    double min_dist;
};

// where a form keeps the per-cell fill counters and the cell-sorted candidate list of a chain
struct AddLists {
    int* cfill;     // [ADD_MAX_CELLS]
    int* items;     // [P]
};

// 16 waves, everything in LDS (128 KB): the form for up to 255 chains per launch
struct AddFull {
    static constexpr int THREADS = 1024;
    typedef int cstart_t;
    // the candidate list lives in LDS, or for more than ADD_MAX_ITEMS candidates (C5: ~15k points
    // per chain) in the chain's int scratch, free once PnP is done (same stream)
    static VO_DEV AddLists lists(const vo_dims& d, const vo_state& s, int b, int P)
    {
        __shared__ int cfill[ADD_MAX_CELLS];
        __shared__ int items_lds[ADD_MAX_ITEMS];
        int* items = items_lds;
        if (P > ADD_MAX_ITEMS) items = s.iwork + (int64_t)b * d.iwork_stride;
        return {cfill, items};
    }
    static VO_DEV bool grid_ok(const vo_dims& d, int P) { return P <= ADD_MAX_ITEMS || P <= d.iwork_stride; }
};

// For many chains per launch (round 5, the headline's 384): a 4-wave block whose only LDS is the
// cell start table (uint16, 16 KB); the per-cell fill counters and the cell-sorted candidate list
// live in the chain's int scratch (free once PnP is done, same stream).  The 16-wave, 128 KB-LDS
// form needed a CU with nearly all of its LDS free, which under another stream group's LK flood
// (~4 KB of LDS per wave) meant waiting for a CU to drain (headline 65.7k -> 66.2-66.5k frames/s;
// at 1-128 chains per launch the 16-wave form is faster, 2-5 %: profiles/r5_add_lean_ab.jsonl).
// The result does not depend on the block shape: the grid only narrows which existing candidates
// a corner is tested against (any one within min_dist rejects it), and the corners are appended
// in their order by the chunked block scan.
struct AddLean {
    static constexpr int THREADS = 256;
    typedef uint16_t cstart_t;
    static VO_DEV AddLists lists(const vo_dims& d, const vo_state& s, int b, int)
    {
        int* cfill = s.iwork + (int64_t)b * d.iwork_stride;
        return {cfill, cfill + ADD_MAX_CELLS};
    }
    // the list has to fit the scratch, and its offsets uint16
    static VO_DEV bool grid_ok(const vo_dims& d, int P) { return P < 65536 && (int64_t)ADD_MAX_CELLS + P <= d.iwork_stride; }
};

// gw x gh cells of cs pixels, one spare column / row before the image and two after it
struct AddGrid {
    int cs, gw, gh;
};

// the (unclamped) cell of a point
VO_DEV void add_cell(const AddGrid& g, float x, float y, int& cx, int& cy)
{
    cx = (int)floorf(x / (float)g.cs) + 1;
    cy = (int)floorf(y / (float)g.cs) + 1;
}

// the cell a candidate is filed under: points outside the image go to the border cells
VO_DEV int add_cell_clamped(const AddGrid& g, const float* ck, int i)
{
    int cx, cy;
    add_cell(g, ck[2 * i], ck[2 * i + 1], cx, cy);
    cx = cx < 0 ? 0 : (cx > g.gw - 1 ? g.gw - 1 : cx);
    cy = cy < 0 ? 0 : (cy > g.gh - 1 ? g.gh - 1 : cy);
    return cy * g.gw + cx;
}

// counting sort of the P candidates by cell: cstart[c] .. cstart[c + 1] index the candidates of
// cell c in items (count, block-wide exclusive scan, scatter), by a block of NT threads
template <int NT, class CStart>
VO_DEV void add_sort_cells(const AddGrid& g, const float* ck, int P, CStart* cstart, int* cfill, int* items, int* sh_scan)
{
    const int tid = threadIdx.x;
    const int ncell = g.gw * g.gh;
    for (int q = tid; q < ncell; q += NT) cfill[q] = 0;
    __syncthreads();
    for (int i = tid; i < P; i += NT) atomicAdd(&cfill[add_cell_clamped(g, ck, i)], 1);
    __syncthreads();
    // exclusive scan of the cell counts (sequential chunks per thread)
    const int per = (ncell + NT - 1) / NT;
    const int q0 = tid * per, q1 = min(q0 + per, ncell);
    int local = 0;
    for (int q = q0; q < q1; ++q) local += cfill[q];
    int incl = local;
    for (int o = 1; o < 64; o <<= 1) { int v = __shfl_up(incl, o, 64); if (lane_id() >= o) incl += v; }
    if (lane_id() == 63) sh_scan[wave_id()] = incl;
    __syncthreads();
    int wbase = 0;
    for (int w = 0; w < wave_id(); ++w) wbase += sh_scan[w];
    int run = wbase + incl - local;
    for (int q = q0; q < q1; ++q) { const int c = cfill[q]; cstart[q] = (CStart)run; run += c; cfill[q] = 0; }
    if (tid == 0) cstart[ncell] = (CStart)P;
    __syncthreads();
    for (int i = tid; i < P; i += NT) {
        const int cell = add_cell_clamped(g, ck, i);
        items[cstart[cell] + atomicAdd(&cfill[cell], 1)] = i;
    }
    __syncthreads();
}

// chain blockIdx.x: keep the corners farther than min_dist from every candidate that existed
// before the call (quirk Q4: not from each other), append them in order, and close the step
template <class Form>
VO_DEV void add_finish_block(const AddArgs& A)
{
    __shared__ typename Form::cstart_t cstart[ADD_MAX_CELLS + 1];
    __shared__ int lds[16];
    __shared__ int sh_scan[Form::THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const vo_dims& d = A.d;
    const vo_state& s = A.s;
    if (s.status[b] != 0) return;
    const int nF = s.nF[b];
    const int M = s.nCorners[b];
    if (M < 0) { if (tid == 0) s.status[b] = VO_ST_CAPACITY; return; }      // k_gftt_select overflow
    if (M == 0) { if (tid == 0) s.status[b] = VO_ST_GFTT_NONE; return; }   // None.squeeze()
    if (M == 1) { if (tid == 0) s.status[b] = VO_ST_GFTT_ONE; return; }    // (2,) indexing
    const int P = s.nC[b];
    float* ck = s.c_kp + (int64_t)b * d.pcap * 2;
    float* cf = s.c_first + (int64_t)b * d.pcap * 2;
    int32_t* ct = s.c_tau + (int64_t)b * d.pcap;
    const float* cor = s.corners + (int64_t)b * d.mcap * 2;
    const float mdf = (float)A.min_dist;
    // cells of at least minDistance: the 3x3 neighbourhood holds every candidate within it.
    // Coarser cells keep that exact, so they grow until the grid fits the cell tables.
    int cs = (int)ceil(A.min_dist) > 0 ? (int)ceil(A.min_dist) : 1;
    while ((d.W / cs + 3) * (d.H / cs + 3) > ADD_MAX_CELLS) ++cs;
    const AddGrid g = {cs, d.W / cs + 3, d.H / cs + 3};
    const AddLists L = Form::lists(d, s, b, P);
    // the all-pairs test below (O(M * P)) when the form has no room for the candidate list
    const bool grid = Form::grid_ok(d, P);
    if (grid) add_sort_cells<Form::THREADS>(g, ck, P, cstart, L.cfill, L.items, sh_scan);
    int nC = P;
    for (int base = 0; base < M; base += Form::THREADS) {
        const int j = base + tid;
        bool keep = false;
        float x = 0, y = 0;
        if (j < M) {
            x = cor[2 * j]; y = cor[2 * j + 1];
            keep = true;
            if (grid) {
                int cx, cy;
                add_cell(g, x, y, cx, cy);
                for (int yy = cy - 1; yy <= cy + 1 && keep; ++yy) {
                    if (yy < 0 || yy >= g.gh) continue;
                    for (int xx = cx - 1; xx <= cx + 1 && keep; ++xx) {
                        if (xx < 0 || xx >= g.gw) continue;
                        const int cell = yy * g.gw + xx;
                        for (int q = cstart[cell]; q < cstart[cell + 1]; ++q) {
                            const int i = L.items[q];
                            const float dx = x - ck[2 * i], dy = y - ck[2 * i + 1];
                            if (!(sqrtf(dx * dx + dy * dy) > mdf)) { keep = false; break; }
                        }
                    }
                }
            } else {
                for (int i = 0; i < P && keep; ++i) {
                    const float dx = x - ck[2 * i], dy = y - ck[2 * i + 1];
                    if (!(sqrtf(dx * dx + dy * dy) > mdf)) keep = false;
                }
            }
        }
        __syncthreads();   // all reads of ck in this chunk done before appends
        int tot;
        const int pos = nC + block_scan_flag(keep, lds, &tot);
        if (keep && pos < d.pcap) {
            ck[2 * pos] = x; ck[2 * pos + 1] = y;
            cf[2 * pos] = x; cf[2 * pos + 1] = y;
            ct[pos] = nF;                                             // tau = len(transforms)
        }
        nC += tot;
        __syncthreads();
    }
    if (tid == 0) {
        if (nC > d.pcap) { s.status[b] = VO_ST_CAPACITY; nC = d.pcap; }
        s.nC[b] = nC;
        s.num_pts[(int64_t)b * d.fcap + nF] = s.nInl[b];
        s.nF[b] = nF + 1;
    }
}

__global__ void __launch_bounds__(AddFull::THREADS) k_add_finish(AddArgs A) { add_finish_block<AddFull>(A); }
__global__ void __launch_bounds__(AddLean::THREADS) k_add_finish_lean(AddArgs A) { add_finish_block<AddLean>(A); }

}  // namespace

extern "C" int vo_add_corners_finish(const vo_dims* d, const vo_opts* o, const vo_state* s, vo_stream_t stream)
{
    if (!d || !o || !s) return VO_EARG;
    AddArgs A;
    A.d = *d;
    A.s = *s;
    A.min_dist = o->feature_min_dist;
    // the lean form from 256 chains per launch (VO_ADD_LEAN=0 / 1 forces it off / on)
    static const int lean_env = vo_env_int("VO_ADD_LEAN", -1);
    if (lean_env >= 0 ? lean_env == 1 : d->B >= 256)
        hipLaunchKernelGGL(k_add_finish_lean, dim3(d->B), dim3(AddLean::THREADS), 0, VO_STREAM(stream), A);
    else
        hipLaunchKernelGGL(k_add_finish, dim3(d->B), dim3(AddFull::THREADS), 0, VO_STREAM(stream), A);
    return hip_rc();
}
