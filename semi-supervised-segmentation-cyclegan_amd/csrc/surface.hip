// Surface distances of the evaluation (include/sscg.h: sscg_surface_stats): the per-case records behind HD, HD95, ASSD and NSD of a
// ground-truth / predicted pair of label maps.  Forward only; without `--surface` nothing launches it.
//
// Direction 0 measures from the true surfaces to the predicted ones (T->P), direction 1 the other way; a GROUP is one (direction,
// sample, class), g = (dir * N + n) * C + c.  The per-pixel products are two byte maps (the class whose surface a pixel lies on, NONE
// elsewhere - a pixel is on the surface of at most one class per map), two int32 maps of d^2 (-1 where there is none) and, per chunk of
// SURF_CH classes, the column distances - none of them is multiplied by C.
//   1. surface_mark_kernel   both byte maps, d^2 = -1 everywhere, cnt per group (LDS bins, 64-bit integer atomics);
//   2. per class chunk:
//      surface_column_kernel one thread per (map, sample, class, column) walks its column down and up and writes the vertical distance
//                            to the nearest surface pixel of the class as uint16 (NONE: the column has none); lanes on consecutive
//                            columns.  A class with an empty surface in either map of the sample is skipped: its case is not defined;
//      surface_row_kernel    one workgroup per (direction, sample, row): per class present on the row, the other map's column
//                            distances of that row staged in LDS, and per source pixel the exact minimum over x' of
//                            (x - x')^2 + g[x']^2 by a walk outwards from x that stops when dx^2 >= best - no window, no cap.
//                            within / max2 through LDS bins and integer atomics; sum of sqrt(d^2) as one fp64 record per (group, row),
//                            reduced in a fixed order;
//   3. the selection         an exact radix select of rank lo = ((cnt - 1) pct) / 100 for all groups at once: three digits of ten bits,
//                            most significant first (d^2 < 2^30).  surface_hist_kernel bins the d^2 that carry the digits chosen so far
//                            (LDS histograms per class of a chunk, one integer add per non-empty bin to the [group][1024] table),
//                            surface_scan_kernel - one workgroup per group - picks the bin and clears its table row for the next digit.
//                            The value of rank hi = min(lo + 1, cnt - 1) is v_lo itself unless rank lo is the last of its value; then
//                            it is the smallest d^2 above v_lo (surface_next_kernel: LDS minima, integer atomicMin);
//   4. surface_finish_kernel one thread per group: the records added in row order, -1 / 0 for the cases that are not defined.
// Every loop has a bound known at launch (grid-stride loops over work items included), no workgroup waits on another, integers go
// through atomics (order-free), fp64 through records (fixed order): the result does not depend on scheduling.
#include "common.h"
#include "head_common.h"
#include "sscg_internal.h"

namespace {

constexpr int SURF_CH = 8;                      // classes per chunk of the column / row passes: 32 B of column distances per pixel
constexpr int SURF_BINS = 1024;                 // ten bits per digit
constexpr int SURF_DIGITS = 3;                  // d^2 < 2^30
constexpr unsigned SURF_NONE8 = 0xFFu;          // byte maps: on no class's surface
constexpr unsigned SURF_NONE16 = 0xFFFFu;       // column distances: the column holds no surface pixel of the class
constexpr unsigned SURF_INF = 0x7FFFFFFFu;
constexpr int SURF_GRID_CAP = 1 << 16;          // blocks of a launch; work items beyond it are taken grid-stride
constexpr size_t SURF_ALIGN = 256;

struct SurfState {
    uint32_t prefix;      // the digits chosen so far; after the last scan: v_lo
    uint32_t rank;        // 1-based rank of v_lo among the d^2 that carry the prefix; 0: the case is not defined
    uint32_t need_next;   // rank hi is the first of the next larger value
    uint32_t next;        // that value (surface_next_kernel); 0xFFFFFFFF until then
};

struct SurfGeom {
    int N, H, W, C;
    int hw;               // H * W
    int bps;              // blocks per sample of the histogram and next-value passes (each clears and flushes LDS bins)
    int mbps;             // blocks per sample of the mark pass
    int nchunks;          // ceil(C / SURF_CH)
    int chs;              // classes the column distances have room for: min(C, SURF_CH)
};

struct SurfWs {
    uint8_t* mark;        // [2][N][H][W]
    int32_t* d2;          // [2][N][H][W]
    uint16_t* g;          // [2][min(C, SURF_CH)][N][H][W]
    uint32_t* table;      // [G][SURF_BINS]
    SurfState* state;     // [G]
    double* rec;          // [G][H]
};

static inline size_t surf_up(size_t b) { return (b + SURF_ALIGN - 1) / SURF_ALIGN * SURF_ALIGN; }

static inline size_t surf_carve(int N, int H, int W, int C, void* base, SurfWs* ws) {
    const size_t pix = (size_t)N * H * W, G = (size_t)2 * N * C;
    const size_t ch = C < SURF_CH ? C : SURF_CH;
    size_t off = 0;
    char* b = reinterpret_cast<char*>(base);
    auto take = [&](size_t bytes) { char* p = b + off; off += surf_up(bytes); return p; };
    uint8_t* mark = reinterpret_cast<uint8_t*>(take(2 * pix));
    int32_t* d2 = reinterpret_cast<int32_t*>(take(2 * pix * sizeof(int32_t)));
    uint16_t* g = reinterpret_cast<uint16_t*>(take(2 * ch * pix * sizeof(uint16_t)));
    uint32_t* table = reinterpret_cast<uint32_t*>(take(G * SURF_BINS * sizeof(uint32_t)));   // table | state: zeroed as one range
    SurfState* state = reinterpret_cast<SurfState*>(take(G * sizeof(SurfState)));
    double* rec = reinterpret_cast<double*>(take(G * (size_t)H * sizeof(double)));
    if (ws) { ws->mark = mark; ws->d2 = d2; ws->g = g; ws->table = table; ws->state = state; ws->rec = rec; }
    return off;
}

static inline dim3 surf_grid(long long items) { return dim3((unsigned)(items < SURF_GRID_CAP ? items : SURF_GRID_CAP)); }

__global__ __launch_bounds__(256) void surface_zero_kernel(uint32_t* __restrict__ a, size_t na, uint32_t* __restrict__ b, size_t nb) {
    const size_t step = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < na; i += step) a[i] = 0u;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nb; i += step) b[i] = 0u;
}

// the class a label belongs to, NONE for a label outside [0, C)
__device__ __forceinline__ unsigned surf_true(int64_t t, int C) { return (t >= 0 && t < C) ? (unsigned)t : SURF_NONE8; }
__device__ __forceinline__ unsigned surf_pred(unsigned p, int C) { return p < (unsigned)C ? p : SURF_NONE8; }

// Work item = (sample n, block blk of mbps): pixels blk * 256 + tid, + mbps * 256, ... of the sample.  A pixel of class c is on c's
// surface when one of its four neighbours lies outside the image or is not of class c.
__global__ __launch_bounds__(256) void surface_mark_kernel(const int64_t* __restrict__ lt, const uint8_t* __restrict__ lp,
                                                           uint8_t* __restrict__ mark, int32_t* __restrict__ d2,
                                                           unsigned long long* __restrict__ stats, SurfGeom g) {
    __shared__ unsigned int bins[2 * SSCG_MAXC];
    const int C = g.C, H = g.H, W = g.W;
    const size_t pix = (size_t)g.N * g.hw;
    const long long items = (long long)g.N * g.mbps;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int n = (int)(it / g.mbps), blk = (int)(it - (long long)n * g.mbps);
        sscg_bins_clear(bins, 2 * C);
        const size_t base = (size_t)n * g.hw;
        for (long long o_raw = (long long)blk * 256 + threadIdx.x; o_raw < g.hw; o_raw += (long long)g.mbps * 256) {
            const int o = (int)o_raw;
            const int y = o / W, x = o - y * W;
            const bool edge = y == 0 || y == H - 1 || x == 0 || x == W - 1;
            const size_t p = base + o;
            const unsigned tc = surf_true(lt[p], C), pc = surf_pred(lp[p], C);
            bool st = tc != SURF_NONE8 && edge, sp = pc != SURF_NONE8 && edge;
            if (!edge) {                                                       // all four neighbours are inside the image
                st = tc != SURF_NONE8 && (surf_true(lt[p - W], C) != tc || surf_true(lt[p + W], C) != tc ||
                                          surf_true(lt[p - 1], C) != tc || surf_true(lt[p + 1], C) != tc);
                sp = pc != SURF_NONE8 && (surf_pred(lp[p - W], C) != pc || surf_pred(lp[p + W], C) != pc ||
                                          surf_pred(lp[p - 1], C) != pc || surf_pred(lp[p + 1], C) != pc);
            }
            mark[p] = (uint8_t)(st ? tc : SURF_NONE8);
            mark[pix + p] = (uint8_t)(sp ? pc : SURF_NONE8);
            d2[p] = -1;
            d2[pix + p] = -1;
            if (st) atomicAdd(&bins[tc], 1u);
            if (sp) atomicAdd(&bins[C + pc], 1u);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 2 * C; i += 256)
            if (bins[i]) {
                const int dir = i >= C, c = i - dir * C;
                atomicAdd(&stats[(((size_t)dir * g.N + n) * C + c) * 5 + 0], (unsigned long long)bins[i]);
            }
        __syncthreads();
    }
}

// Work item = (map m, sample n, class c0 + cc, block of 64 columns).  g[m][cc][n][y][x] = |y - y'| to the nearest y' with
// mark[m][n][y'][x] == c, NONE where the column has none.  A class whose surface is empty in either map of the sample is skipped.
__global__ __launch_bounds__(64) void surface_column_kernel(const uint8_t* __restrict__ mark, const unsigned long long* __restrict__ stats,
                                                            uint16_t* __restrict__ gd, int c0, int nch, SurfGeom g) {
    const int H = g.H, W = g.W, N = g.N, C = g.C;
    const int xb = (W + 63) / 64;
    const size_t pix = (size_t)N * g.hw;
    const long long items = (long long)2 * N * nch * xb;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int bx = (int)(it % xb);
        long long r = it / xb;
        const int cc = (int)(r % nch);
        r /= nch;
        const int n = (int)(r % N), m = (int)(r / N);
        const int c = c0 + cc;
        if (stats[((size_t)n * C + c) * 5] == 0ull || stats[(((size_t)N + n) * C + c) * 5] == 0ull) continue;      // block-uniform
        const int x = bx * 64 + (int)threadIdx.x;
        if (x >= W) continue;
        const uint8_t* mk = mark + (size_t)m * pix + (size_t)n * g.hw + x;
        uint16_t* out = gd + (((size_t)m * g.chs + cc) * N + n) * g.hw + x;
        unsigned dist = SURF_NONE16;
#pragma unroll 8
        for (int y = 0; y < H; ++y) {
            const unsigned k = mk[(size_t)y * W];
            dist = k == (unsigned)c ? 0u : (dist == SURF_NONE16 ? SURF_NONE16 : dist + 1u);       // dist <= H - 1 < 2^15
            out[(size_t)y * W] = (uint16_t)dist;
        }
        dist = SURF_NONE16;
#pragma unroll 8
        for (int y = H - 1; y >= 0; --y) {
            const unsigned k = mk[(size_t)y * W];
            dist = k == (unsigned)c ? 0u : (dist == SURF_NONE16 ? SURF_NONE16 : dist + 1u);
            const unsigned down = out[(size_t)y * W];
            out[(size_t)y * W] = (uint16_t)(dist < down ? dist : down);
        }
    }
}

// Work item = (direction dir, sample n, row y).  The source map is dir's (0: true, 1: predicted), the target the other one.
__global__ __launch_bounds__(256) void surface_row_kernel(const uint8_t* __restrict__ mark, const uint16_t* __restrict__ gd,
                                                          int32_t* __restrict__ d2, unsigned long long* __restrict__ stats,
                                                          double* __restrict__ rec, int c0, int nch, unsigned tol2, SurfGeom g) {
    extern __shared__ unsigned short grow[];             // [W] the target's column distances of this row for one class
    __shared__ unsigned int present[SURF_CH], tgt[SURF_CH], bwithin[SURF_CH], bmax[SURF_CH];
    __shared__ double red[4];
    const int H = g.H, W = g.W, N = g.N, C = g.C;
    const size_t pix = (size_t)N * g.hw;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long items = (long long)2 * N * H;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int y = (int)(it % H);
        const long long r = it / H;
        const int n = (int)(r % N), dir = (int)(r / N);
        const size_t row = (size_t)n * g.hw + (size_t)y * W;
        const uint8_t* src = mark + (size_t)dir * pix + row;
        int32_t* d2row = d2 + (size_t)dir * pix + row;
        if (tid < SURF_CH) {
            present[tid] = 0u; bwithin[tid] = 0u; bmax[tid] = 0u;
            tgt[tid] = tid < nch ? (stats[(((size_t)(1 - dir) * N + n) * C + c0 + tid) * 5] != 0ull) : 0u;
        }
        __syncthreads();
        for (int x = tid; x < W; x += 256) {
            const int cc = (int)src[x] - c0;
            if (cc >= 0 && cc < nch) present[cc] = 1u;
        }
        __syncthreads();
        for (int cc = 0; cc < nch; ++cc) {
            const int c = c0 + cc;
            double* out = rec + (((size_t)dir * N + n) * C + c) * H + y;
            if (!(present[cc] && tgt[cc])) {                                    // block-uniform
                if (tid == 0) *out = 0.0;
                continue;
            }
            const uint16_t* gr = gd + (((size_t)(1 - dir) * g.chs + cc) * N + n) * g.hw + (size_t)y * W;
            for (int x = tid; x < W; x += 256) grow[x] = gr[x];
            __syncthreads();
            double s = 0.0;
            for (int x = tid; x < W; x += 256) {
                if (src[x] != (unsigned)c) continue;
                const unsigned v0 = grow[x];
                unsigned best = v0 == SURF_NONE16 ? SURF_INF : v0 * v0;
                for (int dx = 1; dx < W; ++dx) {                                // exact: no column farther than sqrt(best) can win
                    const unsigned dx2 = (unsigned)dx * (unsigned)dx;
                    if (dx2 >= best) break;
                    if (x - dx >= 0) {
                        const unsigned v = grow[x - dx];
                        if (v != SURF_NONE16) { const unsigned k = dx2 + v * v; best = k < best ? k : best; }
                    }
                    if (x + dx < W) {
                        const unsigned v = grow[x + dx];
                        if (v != SURF_NONE16) { const unsigned k = dx2 + v * v; best = k < best ? k : best; }
                    }
                }
                d2row[x] = (int32_t)best;                // finite: the target surface exists, so some column of this row reaches it
                s += sqrt((double)best);
                if (best <= tol2) atomicAdd(&bwithin[cc], 1u);
                atomicMax(&bmax[cc], best);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
            if (lane == 0) red[wave] = s;
            __syncthreads();
            if (tid == 0) *out = ((red[0] + red[1]) + red[2]) + red[3];
        }
        __syncthreads();
        if (tid < nch && present[tid] && tgt[tid]) {
            unsigned long long* sg = stats + (((size_t)dir * N + n) * C + c0 + tid) * 5;
            if (bwithin[tid]) atomicAdd(&sg[1], (unsigned long long)bwithin[tid]);
            atomicMax(&sg[2], (unsigned long long)bmax[tid]);
        }
        __syncthreads();
    }
}

// Work item = (direction, sample, class chunk, block blk of bps).  Digit d of the d^2 that carry the d digits chosen so far.
__global__ __launch_bounds__(256) void surface_hist_kernel(const uint8_t* __restrict__ mark, const int32_t* __restrict__ d2,
                                                           const SurfState* __restrict__ st, int d, uint32_t* __restrict__ table,
                                                           SurfGeom g) {
    __shared__ unsigned int bins[SURF_CH * SURF_BINS];
    __shared__ uint32_t prefix[SURF_CH], active[SURF_CH];
    const int N = g.N, C = g.C;
    const size_t pix = (size_t)N * g.hw;
    const int shift = 10 * (SURF_DIGITS - 1 - d);
    const long long items = (long long)2 * N * g.nchunks * g.bps;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int blk = (int)(it % g.bps);
        long long r = it / g.bps;
        const int chunk = (int)(r % g.nchunks);
        r /= g.nchunks;
        const int n = (int)(r % N), dir = (int)(r / N);
        const int c0 = chunk * SURF_CH, nch = C - c0 < SURF_CH ? C - c0 : SURF_CH;
        const size_t g0 = ((size_t)dir * N + n) * C + c0;
        if (threadIdx.x < SURF_CH) {
            const bool in = (int)threadIdx.x < nch;
            prefix[threadIdx.x] = (in && d) ? st[g0 + threadIdx.x].prefix : 0u;
            active[threadIdx.x] = in && (d == 0 || st[g0 + threadIdx.x].rank != 0u);
        }
        __syncthreads();
        unsigned any = 0;
        for (int i = 0; i < SURF_CH; ++i) any |= active[i];
        if (any) {                                                              // block-uniform
            for (int i = threadIdx.x; i < nch * SURF_BINS; i += 256) bins[i] = 0u;
            __syncthreads();
            const size_t base = (size_t)dir * pix + (size_t)n * g.hw;
            for (long long o = (long long)blk * 256 + threadIdx.x; o < g.hw; o += (long long)g.bps * 256) {
                const int cc = (int)mark[base + o] - c0;
                if (cc < 0 || cc >= nch || !active[cc]) continue;
                const int32_t k = d2[base + o];
                if (k < 0) continue;
                const uint32_t u = (uint32_t)k;
                if ((u >> (shift + 10)) == prefix[cc]) atomicAdd(&bins[cc * SURF_BINS + ((u >> shift) & (SURF_BINS - 1))], 1u);
            }
            __syncthreads();
            for (int i = threadIdx.x; i < nch * SURF_BINS; i += 256)
                if (bins[i]) atomicAdd(&table[g0 * SURF_BINS + i], bins[i]);
        }
        __syncthreads();
    }
}

// Work item = group.  The bin of digit d that holds the remaining rank (ohem_scan_kernel's scan: thread t owns bins 4t .. 4t+3); the
// table row is cleared for the next digit.  d == 0 forms the rank from cnt; the last digit completes v_lo and decides need_next.
__global__ __launch_bounds__(256) void surface_scan_kernel(uint32_t* __restrict__ table, SurfState* __restrict__ st,
                                                           const unsigned long long* __restrict__ stats, int d, int pct, SurfGeom g) {
    __shared__ uint32_t wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = g.N, C = g.C;
    const long long groups = (long long)2 * N * C;
    for (long long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int c = (int)(grp % C);
        const long long r = grp / C;
        const int n = (int)(r % N), dir = (int)(r / N);
        uint32_t* row = table + (size_t)grp * SURF_BINS;
        uint32_t cb[4], own = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) { cb[j] = row[4 * tid + j]; own += cb[j]; row[4 * tid + j] = 0u; }
        const unsigned long long cnt = stats[(size_t)grp * 5];
        const unsigned long long other = stats[((((size_t)(1 - dir)) * N + n) * C + c) * 5];
        const bool defined = cnt != 0ull && other != 0ull;
        const unsigned long long lo = defined ? ((cnt - 1ull) * (unsigned long long)pct) / 100ull : 0ull;
        const uint32_t prefix = d ? st[grp].prefix : 0u;
        const uint32_t rank = d ? st[grp].rank : (defined ? (uint32_t)lo + 1u : 0u);
        uint32_t incl = own;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();                                   // (also: every thread has read the state before one of them writes it)
        uint32_t before = 0;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        incl += before;
        if (rank == 0u) {
            if (tid == 0) { st[grp].prefix = 0u; st[grp].rank = 0u; st[grp].need_next = 0u; st[grp].next = 0xFFFFFFFFu; }
        } else {
            uint32_t excl = incl - own;
            if (excl < rank && rank <= incl) {
                int j = 0;
                while (j < 3 && excl + cb[j] < rank) { excl += cb[j]; ++j; }
                const uint32_t left = rank - excl;             // 1-based rank inside bin j, 1 <= left <= cb[j]
                st[grp].prefix = (prefix << 10) | (uint32_t)(4 * tid + j);
                st[grp].rank = left;
                st[grp].need_next = (d == SURF_DIGITS - 1 && lo + 1ull < cnt && left == cb[j]) ? 1u : 0u;
                st[grp].next = 0xFFFFFFFFu;
            }
        }
        __syncthreads();                                   // wsum is reused by the next group
    }
}

// Work item = (direction, sample, block blk of bps): the smallest d^2 above v_lo of the groups that need it.
__global__ __launch_bounds__(256) void surface_next_kernel(const uint8_t* __restrict__ mark, const int32_t* __restrict__ d2,
                                                           SurfState* __restrict__ st, SurfGeom g) {
    __shared__ uint32_t vlo[SSCG_MAXC], need[SSCG_MAXC], mins[SSCG_MAXC];
    __shared__ uint32_t any;
    const int N = g.N, C = g.C;
    const size_t pix = (size_t)N * g.hw;
    const long long items = (long long)2 * N * g.bps;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int blk = (int)(it % g.bps);
        const long long r = it / g.bps;
        const int n = (int)(r % N), dir = (int)(r / N);
        const size_t g0 = ((size_t)dir * N + n) * C;
        if (threadIdx.x == 0) any = 0u;
        __syncthreads();
        if ((int)threadIdx.x < C) {
            const SurfState s = st[g0 + threadIdx.x];
            vlo[threadIdx.x] = s.prefix; need[threadIdx.x] = s.need_next; mins[threadIdx.x] = 0xFFFFFFFFu;
            if (s.need_next) any = 1u;
        }
        __syncthreads();
        if (any) {                                                              // block-uniform
            const size_t base = (size_t)dir * pix + (size_t)n * g.hw;
            for (long long o = (long long)blk * 256 + threadIdx.x; o < g.hw; o += (long long)g.bps * 256) {
                const unsigned c = mark[base + o];
                if (c >= (unsigned)C || !need[c]) continue;
                const int32_t k = d2[base + o];
                if (k >= 0 && (uint32_t)k > vlo[c]) atomicMin(&mins[c], (uint32_t)k);
            }
            __syncthreads();
            if ((int)threadIdx.x < C && mins[threadIdx.x] != 0xFFFFFFFFu) atomicMin(&st[g0 + threadIdx.x].next, mins[threadIdx.x]);
        }
        __syncthreads();
    }
}

// One thread per group: the case's records completed.  cnt / within / max2 hold the sums of the atomics.
__global__ __launch_bounds__(256) void surface_finish_kernel(int64_t* __restrict__ stats, double* __restrict__ sums,
                                                             const SurfState* __restrict__ st, const double* __restrict__ rec,
                                                             SurfGeom g) {
    const int N = g.N, C = g.C, H = g.H;
    const long long groups = (long long)2 * N * C;
    for (long long grp = (long long)blockIdx.x * 256 + threadIdx.x; grp < groups; grp += (long long)gridDim.x * 256) {
        const int c = (int)(grp % C);
        const long long r = grp / C;
        const int n = (int)(r % N), dir = (int)(r / N);
        int64_t* s = stats + (size_t)grp * 5;
        const int64_t other = stats[((((size_t)(1 - dir)) * N + n) * C + c) * 5];
        if (s[0] != 0 && other != 0) {
            const SurfState v = st[grp];
            s[3] = (int64_t)v.prefix;
            s[4] = (int64_t)(v.need_next ? v.next : v.prefix);
            double acc = 0.0;
            const double* rr = rec + (size_t)grp * H;
            for (int y = 0; y < H; ++y) acc += rr[y];
            sums[grp] = acc;
        } else {
            s[1] = 0; s[2] = -1; s[3] = -1; s[4] = -1;
            sums[grp] = 0.0;
        }
    }
}

static inline int surf_bps(int hw, int per_thread, int cap) {
    const int b = (hw + 256 * per_thread - 1) / (256 * per_thread);
    return b < 1 ? 1 : (b > cap ? cap : b);
}

static inline bool surf_args_ok(int N, int H, int W, int C) { return N > 0 && H > 0 && W > 0 && C >= 1 && C <= SSCG_MAXC; }

static inline bool surf_too_large(int N, int H, int W) {
    const uint64_t rows = (uint64_t)N * (uint64_t)H;                   // < 2^62: the second product cannot wrap once this one is small
    if (rows >= ((uint64_t)1 << 31) || rows * (uint64_t)W >= ((uint64_t)1 << 31)) return true;
    const uint64_t dy = (uint64_t)(H - 1), dx = (uint64_t)(W - 1);
    return dy * dy + dx * dx >= ((uint64_t)1 << (10 * SURF_DIGITS));  // the selection's three digits cover d^2 < 2^30
}

}  // namespace

extern "C" size_t sscg_surface_workspace(int N, int H, int W, int C) {
    if (!surf_args_ok(N, H, W, C) || surf_too_large(N, H, W)) return 0;
    return surf_carve(N, H, W, C, nullptr, nullptr);
}

extern "C" int sscg_surface_stats(const int64_t* label_true, const uint8_t* label_pred, int N, int H, int W, int C, int tol2, int pct,
                                  int64_t* stats, double* sums, void* ws, size_t ws_bytes, void* stream) {
    if (!label_true || !label_pred || !stats || !sums || !ws) return SSCG_ERR_BAD_ARG;
    if (!surf_args_ok(N, H, W, C) || tol2 < 0 || pct < 1 || pct > 100) return SSCG_ERR_BAD_ARG;
    if (surf_too_large(N, H, W)) return SSCG_ERR_UNSUPPORTED;
    SurfWs w;
    if (ws_bytes < surf_carve(N, H, W, C, ws, &w)) return SSCG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    SurfGeom g;
    g.N = N; g.H = H; g.W = W; g.C = C;
    g.hw = H * W;
    g.bps = surf_bps(g.hw, 16, 64);
    g.mbps = surf_bps(g.hw, 4, 1024);                 // ten loads per pixel and no bins to speak of: many small blocks
    g.nchunks = (C + SURF_CH - 1) / SURF_CH;
    g.chs = C < SURF_CH ? C : SURF_CH;
    const size_t G = (size_t)2 * N * C;
    unsigned long long* ustats = reinterpret_cast<unsigned long long*>(stats);

    const size_t nz_stats = G * 5 * 2;                                                          // 32-bit words
    const size_t nz_table = (surf_up(G * SURF_BINS * sizeof(uint32_t)) + G * sizeof(SurfState)) / sizeof(uint32_t);
    hipLaunchKernelGGL(surface_zero_kernel, dim3(ew_blocks(nz_table, 1024)), dim3(256), 0, st, reinterpret_cast<uint32_t*>(stats),
                       nz_stats, w.table, nz_table);
    hipLaunchKernelGGL(surface_mark_kernel, surf_grid((long long)N * g.mbps), dim3(256), 0, st, label_true, label_pred, w.mark, w.d2,
                       ustats, g);
    const int xb = (W + 63) / 64;
    for (int chunk = 0; chunk < g.nchunks; ++chunk) {
        const int c0 = chunk * SURF_CH, nch = C - c0 < SURF_CH ? C - c0 : SURF_CH;
        hipLaunchKernelGGL(surface_column_kernel, surf_grid((long long)2 * N * nch * xb), dim3(64), 0, st, w.mark, ustats, w.g, c0, nch, g);
        hipLaunchKernelGGL(surface_row_kernel, surf_grid((long long)2 * N * H), dim3(256), ((size_t)W * sizeof(uint16_t) + 15) / 16 * 16,
                           st, w.mark, w.g, w.d2, ustats, w.rec, c0, nch, (unsigned)tol2, g);
    }
    for (int d = 0; d < SURF_DIGITS; ++d) {
        hipLaunchKernelGGL(surface_hist_kernel, surf_grid((long long)2 * N * g.nchunks * g.bps), dim3(256), 0, st, w.mark, w.d2, w.state,
                           d, w.table, g);
        hipLaunchKernelGGL(surface_scan_kernel, surf_grid((long long)G), dim3(256), 0, st, w.table, w.state, ustats, d, pct, g);
    }
    hipLaunchKernelGGL(surface_next_kernel, surf_grid((long long)2 * N * g.bps), dim3(256), 0, st, w.mark, w.d2, w.state, g);
    hipLaunchKernelGGL(surface_finish_kernel, dim3(ew_blocks(G, 1024)), dim3(256), 0, st, stats, sums, w.state, w.rec, g);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}
