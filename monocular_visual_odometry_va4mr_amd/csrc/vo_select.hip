// goodFeaturesToTrack's corner selection for gfx950, over the key list of the eigen pass
// (vo_gftt.hip), in one of two forms -- paged radix-select + LDS bitonic sort + wave-parallel
// greedy min-distance walk in one block per chain (k_gftt_select), or split over several small
// launches (k_gsel_*).
//
// Reference call site: VisualOdometryPipeLine.py:256.  Arithmetic follows oracle/vo_oracle_img.c
// operation by operation (that file restates OpenCV 4.6).
#include "vo_dev.h"

#include <math.h>

namespace {

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

// ---- what both forms share
// quality gate of goodFeaturesToTrack, v > quality * max(eig) (featureselect.cpp): keys >= this pass
VO_DEV uint64_t sel_gate_key(uint32_t kmax, double quality)
{
    const float thr = (float)((double)fkey_inv(kmax) * quality);
    return ((uint64_t)fkey(thr) + 1ull) << 32;
}
// key address y * W + x -> (x, y): by division (k_gftt_select), or by the reciprocal 1 / W with
// the two corrections that make it exact (k_gsel_walk)
VO_DEV void sel_xy_div(uint32_t addr, int W, int& x, int& y)
{
    y = (int)(addr / (uint32_t)W);
    x = (int)(addr - (uint32_t)y * W);
}
VO_DEV void sel_xy_rcp(uint32_t addr, int W, float invW, int& x, int& y)
{
    y = (int)((float)addr * invW);
    y += ((uint32_t)(y + 1) * (uint32_t)W <= addr) ? 1 : 0;
    y -= ((uint32_t)y * (uint32_t)W > addr) ? 1 : 0;
    x = (int)(addr - (uint32_t)y * (uint32_t)W);
}
// a pixel as one word, x | y << 16
VO_DEV uint32_t xy_pack(int x, int y) { return (uint32_t)x | ((uint32_t)y << 16); }
VO_DEV int xy_x(uint32_t xy) { return (int)(xy & 0xFFFF); }
VO_DEV int xy_y(uint32_t xy) { return (int)(xy >> 16); }
// the 3x3 cells around cell (xc, yc), clamped to the grid
struct SelNb { int x1, y1, x2, y2; };
VO_DEV SelNb sel_nb3(int xc, int yc, int gw, int gh)
{
    return {max(xc - 1, 0), max(yc - 1, 0), min(xc + 1, gw - 1), min(yc + 1, gh - 1)};
}
// OpenCV's distance test: float dx * dx + dy * dy, compared in double against minDistance^2
VO_DEV bool sel_closer(int x, int y, int ax, int ay, double md2)
{
    const float ddx = (float)x - (float)ax, ddy = (float)y - (float)ay;
    return (double)(ddx * ddx + ddy * ddy) < md2;
}
// One round of the sequential walk, up to 64 candidates in rank order, one per lane: `tmask` are
// the lanes no corner of an earlier round rejects, `conf` a lane's earlier lanes of the round that
// are closer to it than minDistance.  A lane is accepted iff none of its conflicting lanes is,
// resolved in lane order on scalar registers; of those, the first `room` are kept (maxCorners).
VO_DEV uint64_t sel_round_accept(uint64_t tmask, uint64_t conf, int room)
{
    const uint64_t cm = __ballot(conf != 0);
    uint64_t amask = tmask & ~cm;
    for (uint64_t m = cm; m; m &= m - 1) {
        const int j = __builtin_ctzll(m);
        const uint64_t cj = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)conf, j) |
                            ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(conf >> 32), j) << 32);
        if ((cj & amask) == 0) amask |= 1ull << j;
    }
    if (__popcll(amask) > room) {
        uint64_t m = amask, keep = 0;
        for (int c = 0; c < room; ++c) { const uint64_t lb = m & (~m + 1ull); keep |= lb; m ^= lb; }
        amask = keep;
    }
    return amask;
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

// One chain's block of k_gftt_select: the chain's constants and where its data lives.  The phases
// below are functions over it; the kernel is the page loop that calls them.
struct SelBlock {
    int tid, W;
    uint64_t* keys;          // the chain's keys; after the gate the nk passing ones, compacted in place
    int nk;
    bool use_grid;           // minDistance >= 1
    int cs, gw, gh;          // cell size cvRound(minDistance), grid
    double md2;
    int want, cap, limit;    // maxCorners (or all), the corner capacity, the smaller of the two
    bool lds;                // the grid is in LDS (lgrid, head), else in L2 (gg, ghead)
    bool par;                // the parallel walk: grid in LDS, or grid + cell-list heads behind the conflict lists
    uint32_t* gg;
    int* ghead;
    uint16_t* conf;          // conflict lists past a candidate's first two, in the chain's scratch
    int conf_cap;            // candidates the scratch has lists for
    float* out;
    // dynamic LDS, sized by the host (vo_gftt_select)
    uint64_t* page;          // PAGE keys: gather and sort
    uint32_t* cand_xy;       // PAGE candidates' pixels (parallel walk)
    uint32_t* acc_xy;        // accepted corners' pixels
    uint32_t* lgrid;         // grid cells, if they fit
    int* head;               // per cell: candidate count, then start in nxt (parallel walk, grid in LDS)
    uint16_t* cf2;           // each candidate's first two earlier conflicts
    uint16_t* nxt3;          // third-corner links of the cells
    // the page area again, at other times of a page:
    // 4096 digit counts of the radix select, before the gather
    VO_DEV int* hist4() const { return (int*)page; }
    // after the sort: candidates cell by cell (LDS grid) or list links (L2 grid)
    VO_DEV int* nxt() const { return (int*)page; }
    // after the sort, behind nxt: 0 undecided, 1 accepted, 2 rejected
    VO_DEV volatile uint8_t* stt() const { return (volatile uint8_t*)(nxt() + PAGE); }
    // after the sort, behind stt: a candidate's conflict count
    VO_DEV uint8_t* ncf() const { return (uint8_t*)(nxt() + PAGE) + PAGE; }
    // static LDS of the kernel
    uint32_t* round_xy;      // [64] the wave walk's candidates of a round
    int* sh_int;             // [16] block scans; [1] gather count, [2] corners so far, [3] round changed
    int* sh_scan;            // [16]
    uint64_t* sh_u64;        // [4]
    VO_DEV int cell_of(int x, int y) const { return (y / cs) * gw + x / cs; }
};
#define CONF_K 16            // conflicts listed per candidate; more -> its cells are rescanned every round

VO_DEV void sel_block_init(SelBlock& S, const SelParams& P, int b, uint32_t* round_xy, int* sh_int, int* sh_scan,
                           uint64_t* sh_u64)
{
    extern __shared__ uint64_t sel_dyn[];
    S.page = sel_dyn;
    S.cand_xy = (uint32_t*)(sel_dyn + PAGE);
    S.acc_xy = S.cand_xy + PAGE;
    S.lgrid = S.acc_xy + P.acc_lds;
    S.head = (int*)(S.lgrid + P.grid_lds);
    S.cf2 = (uint16_t*)(S.head + P.grid_lds);
    S.nxt3 = S.cf2 + 2 * PAGE;
    S.round_xy = round_xy; S.sh_int = sh_int; S.sh_scan = sh_scan; S.sh_u64 = sh_u64;
    S.tid = threadIdx.x;
    S.W = P.W;
    S.keys = P.keys + (int64_t)b * P.ccap;
    S.nk = 0;
    const double md = P.min_dist;
    S.use_grid = md >= 1;
    S.cs = S.use_grid ? __double2int_rn(md) : 1;
    S.gw = (P.W + S.cs - 1) / S.cs;
    S.gh = (P.H + S.cs - 1) / S.cs;
    S.md2 = md * md;
    S.want = P.max_corners > 0 ? P.max_corners : 0x7FFFFFFF;
    S.cap = P.mcap < P.acc_lds ? P.mcap : P.acc_lds;
    S.limit = S.want < S.cap ? S.want : S.cap;
    S.lds = (int64_t)S.gw * S.gh <= P.grid_lds;
    S.par = S.use_grid && (S.lds || P.grid_glb);
    uint32_t* scratch = P.gscratch + (int64_t)b * P.gstride;
    S.gg = scratch + (S.lds || !P.grid_glb ? 0 : SEL_GG_OFF);
    S.ghead = (int*)(S.gg + S.gw * S.gh);
    // the eigen-map buffer, unused on this path; an image of fewer than 8 * PAGE pixels has no room
    // for every candidate's list
    S.conf = (uint16_t*)scratch;
    S.conf_cap = (int)min((int64_t)PAGE, P.gstride * 2 / CONF_K);
    S.out = P.corners + (int64_t)b * P.mcap * 2;
}

// ordered in-place compaction of the keys >= lo: the count.  Eight consecutive keys per thread per
// pass (one block scan per 8 * NT keys); every key of a pass is read before the scan's barrier,
// and writes never pass a later pass's reads
template <int NT>
VO_DEV int sel_gate_compact(const SelBlock& S, int nk_all, uint64_t lo)
{
    uint64_t* keys = S.keys;
    const int tid = S.tid;
    int nk = 0;
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
        int pos = nk + block_scan_i32(cnt, S.sh_int, &tot);
#pragma unroll
        for (int j = 0; j < KPT; ++j)
            if (i0 + j < nk_all && kk[j] >= lo) keys[pos++] = kk[j];
        nk += tot;
    }
    __syncthreads();
    return nk;
}

VO_DEV void sel_grid_clear(const SelBlock& S, int acc_lds)
{
    if (!S.use_grid) return;
    const int tid = S.tid;
    for (int q = tid; q < S.gw * S.gh; q += blockDim.x) cell_set(S.lds, S.lgrid, S.gg, q, 0xFFFFFFFFu);
    if (S.par && !S.lds)
        for (int q = tid; q < S.gw * S.gh; q += blockDim.x) atomicExch(&S.ghead[q], -1);
    for (int q = tid; q < acc_lds; q += blockDim.x) S.nxt3[q] = 0xFFFFu;
}

// the keys a page may still take: those below the last key of the page before
struct SelRest { bool has_upper; uint64_t upper; };

// the PAGE-th largest key of the rest: radix select, 12-bit digits (histogram in the page buffer,
// free until the gather): usually three passes over the keys instead of eight
template <int NT>
VO_DEV uint64_t sel_page_threshold(const SelBlock& S, SelRest R)
{
    const uint64_t* keys = S.keys;
    const int tid = S.tid, nk = S.nk;
    int* hist4 = S.hist4();
    uint64_t prefix = 0, mask = 0;
    int k = PAGE;
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
                const bool on = i0 + u * NT < nk && (!R.has_upper || kk[u] < R.upper) && (kk[u] & mask) == prefix;
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
        const int before = block_scan_i32(loc, S.sh_scan, &tot);
        if (before < k && k <= before + loc) {
            int cum = before;
            for (int j = 0; j < BPT; ++j) {
                const int h = hist4[hi - j];
                if (cum + h >= k) {
                    S.sh_u64[0] = prefix | ((uint64_t)(hi - j) << sh);
                    S.sh_int[0] = k - cum;
                    S.sh_int[1] = h;
                    break;
                }
                cum += h;
            }
        }
        __syncthreads();
        prefix = S.sh_u64[0];
        k = S.sh_int[0];
        const int in_bucket = S.sh_int[1];
        mask |= dmask << sh;
        __syncthreads();
        if (in_bucket == k) break;          // the whole bucket is in: prefix (low bits 0) is the threshold
    }
    return prefix;
}

// the rest's keys >= thr into the page (`take` of them), zeros behind them
template <int NT>
VO_DEV void sel_page_gather(const SelBlock& S, SelRest R, uint64_t thr, int take)
{
    const uint64_t* keys = S.keys;
    uint64_t* page = S.page;
    const int tid = S.tid, nk = S.nk;
    if (tid == 0) S.sh_int[1] = 0;
    __syncthreads();
    for (int i0 = tid; i0 < nk; i0 += 4 * NT) {
        uint64_t kk[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) kk[u] = i0 + u * NT < nk ? keys[i0 + u * NT] : 0ull;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            // page order is irrelevant (sorted next): one LDS atomic per wave
            const bool on = i0 + u * NT < nk && (!R.has_upper || kk[u] < R.upper) && kk[u] >= thr;
            const uint64_t m = __ballot(on);
            if (m == 0) continue;
            const int leader = __ffsll((unsigned long long)m) - 1;
            int base = 0;
            if (lane_id() == leader) base = atomicAdd(&S.sh_int[1], __popcll(m));
            base = __shfl(base, leader, 64);
            const int pos = base + __popcll(m & ((1ull << lane_id()) - 1ull));
            if (on && pos < PAGE) page[pos] = kk[u];
        }
    }
    __syncthreads();
    for (int i = take + tid; i < PAGE; i += blockDim.x) page[i] = 0;
    __syncthreads();
}

// bitonic sort of the page, descending (value desc, then larger address first)
VO_DEV void sel_page_sort(const SelBlock& S)
{
    uint64_t* page = S.page;
    for (int size = 2; size <= PAGE; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = S.tid; i < PAGE / 2; i += blockDim.x) {
                const int lo = 2 * i - (i & (stride - 1));
                const int hi = lo + stride;
                const bool desc = ((lo & size) == 0);
                const uint64_t a = page[lo], c = page[hi];
                if ((a < c) == desc) { page[lo] = c; page[hi] = a; }
            }
            __syncthreads();
        }
    }
}

// OpenCV's grid test: an accepted corner in the 3x3 cells around (x, y)'s is closer than minDistance
VO_DEV bool sel_near_accepted(const SelBlock& S, int x, int y, int xc, int yc)
{
    const SelNb n = sel_nb3(xc, yc, S.gw, S.gh);
    bool near = false;
    for (int yy = n.y1; yy <= n.y2 && !near; ++yy)
        for (int xx = n.x1; xx <= n.x2 && !near; ++xx)
            cell_each(cell_get(S.lds, S.lgrid, S.gg, yy * S.gw + xx), S.nxt3, [&](uint32_t id) {
                const uint32_t a = S.acc_xy[id];
                if (sel_closer(x, y, xy_x(a), xy_y(a), S.md2)) near = true;
            });
    return near;
}

// accepted corner `pos` at (x, y): the output, the LDS table and (with a grid) its cell
VO_DEV void sel_emit(const SelBlock& S, int pos, int x, int y)
{
    S.acc_xy[pos] = xy_pack(x, y);
    S.out[2 * pos] = (float)x;
    S.out[2 * pos + 1] = (float)y;
    if (S.use_grid) cell_insert(S.lds, S.lgrid, S.gg, S.nxt3, S.cell_of(x, y), pos);
}

// Exact parallel form of OpenCV's sequential minDistance walk over the sorted page, by the whole
// block; the corner count after it goes to sh_int[2].  Candidate i (rank order) is accepted iff no
// earlier accepted candidate in its 3x3 cell neighbourhood is closer than minDistance, and no
// corner accepted on an earlier page is.  Decisions only depend on earlier candidates, so they are
// resolved in parallel rounds (each round decides at least the lowest undecided candidate); the
// first `limit` accepted in rank order are the corners.
template <int NT>
VO_DEV void sel_walk_parallel(const SelBlock& S, int take, int nacc)
{
    const int tid = S.tid, cs = S.cs, gw = S.gw, gh = S.gh;
    const bool lds = S.lds;
    uint32_t* cand_xy = S.cand_xy;
    int* head = S.head;
    int* nxt = S.nxt();
    volatile uint8_t* stt = S.stt();
    for (int i = tid; i < take; i += blockDim.x) {
        int x, y;
        sel_xy_div((uint32_t)S.page[i], S.W, x, y);
        cand_xy[i] = xy_pack(x, y);
    }
    // candidates by cell: with the grid in LDS, a counting sort (head[] = counts, then start
    // offsets; nxt[] = the candidate indices cell by cell), so a cell's candidates are read with
    // independent loads; otherwise linked lists in the L2 grid
    const int ncell = gw * gh;
    if (lds)
        for (int q = tid; q < ncell; q += blockDim.x) head[q] = 0;
    __syncthreads();                                      // page keys are dead now: nxt, stt, ncf
    constexpr int CPT = PAGE / NT;                        // candidates per thread
    int slot[CPT];
#pragma unroll
    for (int kq = 0; kq < CPT; ++kq) {
        const int i = tid + kq * NT;
        if (i >= take) break;
        const int x = xy_x(cand_xy[i]), y = xy_y(cand_xy[i]);
        const int xc = x / cs, yc = y / cs;
        const bool rej = nacc > 0 && sel_near_accepted(S, x, y, xc, yc);
        stt[i] = rej ? 2 : 0;
        if (lds) slot[kq] = atomicAdd(&head[yc * gw + xc], 1);
        else nxt[i] = atomicExch(&S.ghead[yc * gw + xc], i);
    }
    __syncthreads();
    if (lds) {
        // exclusive scan of the cell counts in place, then the cell-ordered index array
        const int cpt = (ncell + NT - 1) / NT, q0 = tid * cpt, q1 = min(q0 + cpt, ncell);
        int sum = 0;
        for (int q = q0; q < q1; ++q) sum += head[q];
        int tot;
        int run = block_scan_i32(sum, S.sh_int, &tot);
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
            nxt[head[S.cell_of(xy_x(cand_xy[i]), xy_y(cand_xy[i]))] + slot[kq]] = i;
        }
        __syncthreads();
    }
    // visit(j, is (x, y) closer than minDistance to j) for every earlier candidate j in the 3x3
    // cells around candidate i, until it returns true
    auto for_earlier = [&](int i, auto&& visit) {
        const int x = xy_x(cand_xy[i]), y = xy_y(cand_xy[i]);
        const SelNb n = sel_nb3(x / cs, y / cs, gw, gh);
        auto one = [&](int j) { return j < i && visit(j, [&] { return sel_closer(x, y, xy_x(cand_xy[j]), xy_y(cand_xy[j]), S.md2); }); };
        for (int yy = n.y1; yy <= n.y2; ++yy)
            for (int xx = n.x1; xx <= n.x2; ++xx) {
                const int cc = yy * gw + xx;
                if (lds) {
                    const int e0 = cc + 1 < ncell ? head[cc + 1] : take;
                    for (int k = head[cc]; k < e0; ++k)
                        if (one(nxt[k])) return;
                } else {
                    for (int j = __hip_atomic_load(&S.ghead[cc], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); j >= 0; j = nxt[j])
                        if (one(j)) return;
                }
            }
    };
    // each candidate's earlier conflicts (same test as OpenCV's walk), found once: count in LDS,
    // the first two in LDS (most have at most two), up to CONF_K in the per-chain scratch; more
    // than CONF_K, or a candidate past the lists the scratch has room for -> rescan the cells in
    // every round
    uint16_t* cf2 = S.cf2;
    uint16_t* conf = S.conf;
    uint8_t* ncf = S.ncf();
    const int conf_cap = S.conf_cap;
    for (int i = tid; i < take; i += blockDim.x) {
        if (stt[i] != 0) { ncf[i] = 0; continue; }
        int c = 0;
        for_earlier(i, [&](int j, auto&& closer) {
            if (closer()) {
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
        if (tid == 0) S.sh_int[3] = 0;
        __syncthreads();
        bool changed = false;
        for (int i = tid; i < take; i += blockDim.x) {
            if (stt[i] != 0) continue;
            // an earlier conflict that is accepted rejects i, an undecided one blocks it
            bool blocked = false, rej = false;
            const int c = ncf[i];
            if (c <= 2) {
                for (int k = 0; k < c && !rej; ++k) {
                    const uint8_t sj = stt[cf2[2 * i + k]];
                    rej = sj == 1;
                    blocked |= sj == 0;
                }
            } else if (c <= CONF_K) {
                for (int k = 0; k < c && !rej; ++k) {
                    const uint8_t sj = stt[conf[(int64_t)i * CONF_K + k]];
                    rej = sj == 1;
                    blocked |= sj == 0;
                }
            } else {
                for_earlier(i, [&](int j, auto&& closer) {
                    const uint8_t sj = stt[j];
                    if (sj == 2 || !closer()) return false;
                    rej = sj == 1;
                    blocked |= sj == 0;
                    return rej;
                });
            }
            if (rej) { stt[i] = 2; changed = true; }
            else if (!blocked) { stt[i] = 1; changed = true; }
        }
        if (changed) S.sh_int[3] = 1;
        __syncthreads();
        const int any = S.sh_int[3];
        __syncthreads();
#ifdef VO_SELECT_PROF
        if (tid == 0 && blockIdx.x == 0) g_selprof[10]++;
#endif
        if (!any) break;
    }
    SELPROF(6);
    // accepted candidates in rank order -> corners (up to limit) and the grid
    for (int base = 0; base < take && nacc < S.limit; base += blockDim.x) {
        const int i = base + tid;
        const bool acc = i < take && stt[i] == 1;
        int tot;
        const int pos = nacc + block_scan_flag(acc, S.sh_int, &tot);
        if (acc && pos < S.limit) sel_emit(S, pos, xy_x(cand_xy[i]), xy_y(cand_xy[i]));
        nacc = min(nacc + tot, S.limit);
    }
    if (!lds) {
        // empty the cell lists this page used (the next page rebuilds them)
        for (int i = tid; i < take; i += blockDim.x)
            atomicExch(&S.ghead[S.cell_of(xy_x(cand_xy[i]), xy_y(cand_xy[i]))], -1);
    }
    if (tid == 0) S.sh_int[2] = nacc;
}

// The same walk by wave 0 alone, 64 candidates per round in sorted order (no grid, or a grid in
// L2 with no room for the cell lists); the corner count after it goes to sh_int[2].  A candidate
// survives if no accepted corner in the 3x3 neighbouring cells is closer than minDistance
// (OpenCV's grid test).  Within a round, lane i additionally needs every earlier accepted lane
// j < i of the round to pass the same test; the lanes form a conflict mask against earlier
// tentative lanes, and wave-uniform scalar code walks the tentative lanes in order to pick the
// accepted set -- exactly OpenCV's sequential walk, without a ballot/shuffle round trip per
// accepted corner.
VO_DEV void sel_walk_wave(const SelBlock& S, int take, int nacc)
{
    if (wave_id() != 0) return;
    const int lane = lane_id(), cs = S.cs;
    for (int s0 = 0; s0 < take && nacc < S.limit; s0 += 64) {
        const int i = s0 + lane;
        bool tent = i < take;
        int x = 0, y = 0;
        if (tent) sel_xy_div((uint32_t)S.page[i], S.W, x, y);
        const int xc = x / cs, yc = y / cs;
        if (tent && S.use_grid) tent = !sel_near_accepted(S, x, y, xc, yc);
        const uint64_t tmask = __ballot(tent);
        if (tmask == 0) continue;
        uint64_t conf = 0;
        if (S.use_grid) {
            // conflicts with earlier tentative lanes of this round
            S.round_xy[lane] = xy_pack(x, y);
            wave_lds_sync();
            const uint64_t rest = tmask & ((1ull << lane) - 1ull) & (tent ? ~0ull : 0ull);
            // uniform walk over the tentative lanes; each lane keeps the earlier ones
            for (uint64_t m = tmask; m; m &= m - 1) {
                const int j = __builtin_ctzll(m);
                if (!((rest >> j) & 1ull)) continue;
                const int tx = xy_x(S.round_xy[j]), ty = xy_y(S.round_xy[j]);
                if (abs(tx / cs - xc) <= 1 && abs(ty / cs - yc) <= 1 && sel_closer(x, y, tx, ty, S.md2)) conf |= 1ull << j;
            }
        }
        const uint64_t amask = sel_round_accept(tmask, conf, S.limit - nacc);
        if ((amask >> lane) & 1ull) sel_emit(S, nacc + __popcll(amask & ((1ull << lane) - 1ull)), x, y);
        nacc += __popcll(amask);
        wave_lds_sync();
    }
    if (lane == 0) S.sh_int[2] = nacc;
}

template <int NT>
__global__ void __launch_bounds__(NT) k_gftt_select(SelParams P)
{
    __shared__ uint32_t round_xy[64];
    __shared__ int sh_int[16];
    __shared__ int sh_scan[16];
    __shared__ uint64_t sh_u64[4];
    const int b = blockIdx.x;
    if (P.chain_status[b] != 0) return;
    SELPROF(0);
    const int nk_all = P.nkeys[b];
    if (nk_all > P.ccap) {
        if (threadIdx.x == 0) P.ncorners[b] = -1;      // capacity: k_add_finish raises it
        return;
    }
    SelBlock S;
    sel_block_init(S, P, b, round_xy, sh_int, sh_scan, sh_u64);
    S.nk = sel_gate_compact<NT>(S, nk_all, sel_gate_key(P.eig_max[b], P.quality));
    SELPROF(1);
    if (S.tid == 0) P.nkeys[b] = S.nk;
    sel_grid_clear(S, P.acc_lds);
    int nacc = 0, remaining = S.nk;
    SelRest R = {false, 0};
    __syncthreads();
    while (remaining > 0 && nacc < S.limit) {
        // ---- this page: the min(PAGE, remaining) largest keys of the rest
        const int take = remaining < PAGE ? remaining : PAGE;
        const uint64_t thr = remaining > PAGE ? sel_page_threshold<NT>(S, R) : 0;
        sel_page_gather<NT>(S, R, thr, take);
        SELPROF(2);
        sel_page_sort(S);
        SELPROF(3);
        const uint64_t page_last = S.page[take - 1];
        if (S.par) sel_walk_parallel<NT>(S, take, nacc);
        else sel_walk_wave(S, take, nacc);
        __syncthreads();
        SELPROF(4);
        nacc = sh_int[2];
        R = {true, page_last};
        remaining -= take;
        __syncthreads();
    }
    if (S.tid == 0) {
        // more corners wanted than this engine can hold -> never truncate silently.  The
        // status word is not written here: GFTT runs on a side stream concurrently with PnP,
        // which owns it; k_add_finish turns ncorners < 0 into VO_ST_CAPACITY.
        P.ncorners[b] = (nacc == S.cap && S.cap < S.want && remaining > 0) ? -1 : nacc;
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
struct GsRange {
    uint64_t lo;
    uint32_t kmax;
    int shift;
    bool any;                // false: the gate lies above the maximum, nothing passes
    VO_DEV int bucket(uint64_t k) const
    {
        const int q = (int)((kmax - (uint32_t)(k >> 32)) >> shift);
        return q < GS_NB - 1 ? q : GS_NB - 1;
    }
};
VO_DEV GsRange gs_range(const SelSplitParams& P, int b)
{
    GsRange r = {sel_gate_key(P.eig_max[b], P.quality), P.eig_max[b], 0, false};
    if ((uint64_t)r.kmax < (r.lo >> 32)) return r;
    const uint32_t R = r.kmax - (uint32_t)(r.lo >> 32);
    const int bits = R ? 32 - __clz(R) : 0;
    r.shift = bits > 12 ? bits - 12 : 0;
    r.any = true;
    return r;
}

__global__ void __launch_bounds__(64) k_gsel_gate(SelSplitParams P)
{
    const int b = blockIdx.x / P.wpc, w = blockIdx.x - b * P.wpc;
    const int nk_all = P.nkeys[b];
    if (nk_all > P.ccap) return;                         // capacity: the walk reports it
    const GsRange r = gs_range(P, b);
    if (!r.any) return;
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
            const bool on = kk[u] >= r.lo;               // 0 (absent) never passes: lo >= 2^32
            const uint64_t m = __ballot(on);
            if (m == 0) continue;
            if (on) __hip_atomic_fetch_add(&hist[r.bucket(kk[u])], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
    const GsRange r = gs_range(P, b);
    const uint64_t* pass = P.sorted + (int64_t)b * P.sstride;
    uint32_t* hist = gs_hist(P, b);
    uint64_t* grouped = P.keys + (int64_t)b * P.ccap;
    for (int i = w * 64 + lane_id(); i < n; i += P.wpc * 64) {
        const uint64_t k = pass[i];
        const uint32_t pos = atomicAdd(&hist[r.bucket(k)], 1u);
        grouped[pos] = k;
    }
}

__global__ void __launch_bounds__(64) k_gsel_rank(SelSplitParams P)
{
    const int b = blockIdx.x / P.wpc, w = blockIdx.x - b * P.wpc;
    const int n = *gs_npass(P, b);
    if (n == 0) return;
    const GsRange r = gs_range(P, b);
    const uint32_t* hist = gs_hist(P, b);              // after the scatter: bucket ends
    const uint64_t* grouped = P.keys + (int64_t)b * P.ccap;
    uint64_t* sorted = P.sorted + (int64_t)b * P.sstride;
    for (int i = w * 64 + lane_id(); i < n; i += P.wpc * 64) {
        const uint64_t k = grouped[i];
        const int q = r.bucket(k);
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
        int x, y;
        sel_xy_rcp(addr, P.W, P.invW, x, y);
        const int xc = (int)__umulhi((uint32_t)x, P.cs_m), yc = (int)__umulhi((uint32_t)y, P.cs_m);
        const SelNb nb = sel_nb3(xc, yc, gw, gh);
        const int x1 = nb.x1, y1 = nb.y1, x2 = nb.x2, y2 = nb.y2;
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
                    if (sel_closer(x, y, ax, ay, P.md2)) tent = false;
                }
            }
        }
        const uint64_t tmask = __ballot(tent);
        if (tmask == 0) continue;
        // conflicts with earlier candidates of this round: lanes register in a cell hash, each
        // reads the masks of its 3x3 neighbourhood and tests the (rare) earlier lanes exactly
        if (tent) {
            rxy[lane] = xy_pack(x, y);
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
                const int tx = xy_x(rxy[j]), ty = xy_y(rxy[j]);
                const int tcx = (int)__umulhi((uint32_t)tx, P.cs_m), tcy = (int)__umulhi((uint32_t)ty, P.cs_m);
                if (abs(tcx - xc) <= 1 && abs(tcy - yc) <= 1 && sel_closer(x, y, tx, ty, P.md2)) conf |= 1ull << j;
            }
        }
        wave_lds_sync();
        if (tent) rhash[(yc * gw + xc) & (GS_HASH - 1)] = 0;
        const uint64_t amask = sel_round_accept(tmask, conf, limit - nacc);
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
        nacc += __popcll(amask);
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

#define SEL_LDS_BUDGET (150 * 1024)
// the minDistance grid of a configuration, and where k_gftt_select keeps it
struct SelGrid {
    int cs, gw, gh;          // cell size cvRound(minDistance) and grid; 0 below minDistance 1 (no grid)
    int64_t cells;
    int acc_lds;             // accepted-corner slots in LDS
    int grid_lds;            // cells in LDS, with the per-cell candidate lists (0: they do not fit)
    bool grid_glb;           // else: grid + lists in the eigen-map scratch, after the conflict lists
                             // (neither: grid alone in the scratch, the wave-serial walk)
    size_t lds;              // dynamic LDS: page, candidate xy and conflict slots | accepted xy +
                             // third-corner links | grid + heads
};
static SelGrid sel_grid(const vo_dims* d, const vo_opts* o)
{
    SelGrid g;
    const double md = o->feature_min_dist;
    g.cs = md >= 1 ? (int)lrint(md) : 0;
    g.gw = g.cs ? (d->W + g.cs - 1) / g.cs : 0;
    g.gh = g.cs ? (d->H + g.cs - 1) / g.cs : 0;
    g.cells = (int64_t)g.gw * g.gh;
    g.acc_lds = d->mcap < ACC_MAX ? d->mcap : ACC_MAX;
    const size_t fixed = 16 * (size_t)PAGE + 6 * (size_t)g.acc_lds;
    g.grid_lds = g.cells <= GRID_LDS_CELLS && fixed + 8 * (size_t)g.cells <= SEL_LDS_BUDGET ? (int)g.cells : 0;
    g.grid_glb = g.grid_lds == 0 && SEL_GG_OFF + 2 * g.cells <= (int64_t)d->W * d->H;
    g.lds = fixed + 8 * (size_t)g.grid_lds;
    return g;
}

// The split selection (k_gsel_*) where it applies: a minDistance grid of cells cvRound(md) <= 255
// wide (u64 cells of four corners: five never fit a cell of side cs - 1 <= md - 0.5) that fits
// the eigen-map scratch, and 1 <= maxCorners <= the corner capacity (no capacity truncation to
// report).
static bool sel_split_applies(const vo_dims* d, const vo_opts* o, const vo_state* s, const SelGrid& g)
{
    const int want = o->feature_max_corners;
    return s->gf_sort && g.cs >= 1 && g.cs <= 255 && g.cells * 8 + 4 <= (int64_t)4 * d->W * d->H && want >= 1 &&
           want <= d->mcap && d->W <= 65535 && d->H <= 65535;
}

static void launch_split(const vo_dims* d, const vo_opts* o, const vo_state* s, const SelGrid& g, hipStream_t st)
{
    SelSplitParams G;
    G.keys = s->gf_keys; G.nkeys = s->gf_n; G.eig_max = s->eig_max; G.quality = o->feature_quality_level;
    G.ccap = d->ccap; G.W = d->W; G.H = d->H; G.invW = 1.0f / (float)d->W;
    G.want = o->feature_max_corners; G.md2 = o->feature_min_dist * o->feature_min_dist;
    G.cs = g.cs; G.gw = g.gw; G.gh = g.gh;
    G.cs_m = (uint32_t)(((1ull << 32) + g.cs - 1) / g.cs);
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
}

// the selection over the keys the eigen pass left in s->gf_keys / s->gf_n (vo_gftt, vo_gftt_masked)
int vo_gftt_select(const vo_dims* d, const vo_opts* o, const vo_state* s, hipStream_t st)
{
    const SelGrid g = sel_grid(d, o);
    // automatic: the split form for more than 64 chains per launch, where the one-block
    // kernel waits for whole CUs beside the other stream group's LK flood (headline 384: the
    // GFTT stage 5.7 -> 1.9 ms; C5 128: 9.7k -> 10.2k frames/s); at 1-48 chains the GPU has
    // room for the fat block and its 512-1024 threads finish the walk sooner (one chain
    // 2,251 vs 2,213 frames/s; the 8-GPU slice of 2 x 12 chains 88.2k vs 82.7k predicted)
    const int mode = g_sel_mode ? g_sel_mode : (d->B > 64 ? 2 : 1);
    if (mode == 2 && sel_split_applies(d, o, s, g)) {
        launch_split(d, o, s, g, st);
        return hip_ok() ? VO_OK : VO_EHIP;
    }
    SelParams S;
    S.keys = s->gf_keys; S.nkeys = s->gf_n; S.ccap = d->ccap; S.W = d->W; S.H = d->H;
    S.eig_max = s->eig_max; S.quality = o->feature_quality_level;
    S.max_corners = o->feature_max_corners; S.min_dist = o->feature_min_dist;
    S.corners = s->corners; S.ncorners = s->nCorners; S.mcap = d->mcap; S.chain_status = s->status;
    S.gscratch = (uint32_t*)s->eig;      // L2 grid when the LDS grid is too small
    S.gstride = (int64_t)d->W * d->H;
    // LDS sized to this configuration (page + corner cap + grid) instead of the maximum
    S.acc_lds = g.acc_lds; S.grid_lds = g.grid_lds; S.grid_glb = g.grid_glb;
    static const bool attr_ok =
        hipFuncSetAttribute((const void*)k_gftt_select<SEL_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            SEL_LDS_BUDGET) == hipSuccess &&
        hipFuncSetAttribute((const void*)k_gftt_select<1024>, hipFuncAttributeMaxDynamicSharedMemorySize, SEL_LDS_BUDGET) ==
            hipSuccess;
    if (!attr_ok && g.lds > 64 * 1024) return VO_EHIP;
    // block size SEL_THREADS = 512 (same result at any size; headline bench: 512 threads 56.2k
    // frames/s, 1024 55.1k -- a select block holds its wave slots while the other stream
    // group's LK runs), or 1024 threads per chain at few chains, where the GPU is mostly idle
    // during the select
    if (d->B <= 128) hipLaunchKernelGGL(k_gftt_select<1024>, dim3(d->B), dim3(1024), g.lds, st, S);
    else hipLaunchKernelGGL(k_gftt_select<SEL_THREADS>, dim3(d->B), dim3(SEL_THREADS), g.lds, st, S);
    return hip_ok() ? VO_OK : VO_EHIP;
}
