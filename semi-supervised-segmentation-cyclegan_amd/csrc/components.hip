// Connected-component filtering of predicted label maps (include/sscg.h: sscg_components_filter): the components of every predicted
// class are labelled per sample, the largest one and / or the ones of at least min_area pixels are kept, the rest become `fill`.
// Forward only; without `--components` nothing launches it.
//
// A block-based union-find over the batch-linear pixel index p = (n * H + y) * W + x < 2^31: one int32 parent and one int32 area per
// pixel, one 64-bit selection key per (sample, class).  Unions are by minimum index, so the root of a component is its ANCHOR, the
// smallest row-major index - which makes "ties go to the smallest anchor" one integer comparison.  Five launches on the caller's
// stream, no host synchronisation, no memset:
//   1. components_tile_kernel    one workgroup per CC_T x CC_T tile: the bytes staged in LDS, union-find in LDS - every pixel starts
//                                under the first pixel of its horizontal run (one ballot per row), runs of equal class meet the
//                                runs of the row above (conn 8: diagonally too) by atomicMin on LDS - areas counted per tile-local
//                                root with LDS atomics; writes EVERY pixel's parent (the batch-linear index of its tile-local root; a byte >= C
//                                is its own parent) and area (the local area at tile-local roots, 0 elsewhere), and zeroes the keys and
//                                the stats - nothing is ever read from what the workspace held;
//   2. components_seam_kernel    one thread per pixel on the first row / column of a tile (not of the image): union with the
//                                equal-class neighbours across the seam (conn 8: the diagonal ones too, tile corners included) by
//                                global atomicMin;
//   3. components_fold_kernel    every pixel finds its root and stores it; a tile-local root that is not the global root adds its area
//                                to the global root's (targets are global roots, sources are not: no cell is both);
//   4. components_select_kernel  every global root counts its class's components and, for a non-exempt class, offers
//                                (area << 32) | (0xFFFFFFFF - anchor) to the 64-bit maximum of its (sample, class) - through LDS bins;
//   5. components_write_kernel   per pixel the keep decision and label_out; hist, the pixel counts and the kept-component counts through
//                                per-workgroup LDS bins, then 64-bit integer atomics (as confusion_hist_kernel).
//
// A union-find whose loops can spin would be a hang; three invariants keep every loop finite, each noted at its loop:
//   (a) parents only decrease: parent[i] <= i always, and a parent only ever changes to a smaller index of the same component, so a
//       find visits strictly decreasing indices and ends;
//   (b) a union retries only on progress: the pair it continues with has a strictly smaller maximum; it never waits for another
//       workgroup, polls no flag and spins on no value;
//   (c) stale reads are harmless: a stale parent is an earlier parent, hence a larger index of the same component, and only the
//       atomic's return value decides.  Kernel boundaries are the only synchronisation relied on.
// All results are integers formed by order-free atomics (min, max, add): they do not depend on scheduling.
#include "common.h"
#include "head_common.h"
#include "sscg_internal.h"

namespace {

constexpr int CC_T = 32;                        // tile edge
constexpr int CC_TT = CC_T * CC_T;
constexpr unsigned CC_NONE = 0xFFu;             // LDS class byte of a pixel outside the image or with a byte >= C: joins nothing
constexpr int CC_GRID_CAP = 1 << 16;            // blocks of a launch; work items beyond it are taken grid-stride
constexpr size_t CC_ALIGN = 256;

struct CcGeom {
    int N, H, W, C;
    int hw;               // H * W
    int tx, ty;           // tiles per row / column of a sample
    int bps;              // blocks per sample of the select and write passes (each clears and flushes LDS bins)
    int conn8, largest, min_area, fill;
    unsigned long long exempt;   // bit c: class c is always kept (the fill class included)
};

struct CcWs {
    int* parent;                  // [N][H][W]
    int* area;                    // [N][H][W]
    unsigned long long* key;      // [N][C]
};

static inline size_t cc_up(size_t b) { return (b + CC_ALIGN - 1) / CC_ALIGN * CC_ALIGN; }

static inline size_t cc_carve(int N, int H, int W, int C, void* base, CcWs* ws) {
    const size_t pix = (size_t)N * H * W;
    size_t off = 0;
    char* b = reinterpret_cast<char*>(base);
    auto take = [&](size_t bytes) { char* p = b + off; off += cc_up(bytes); return p; };
    int* parent = reinterpret_cast<int*>(take(pix * sizeof(int)));
    int* area = reinterpret_cast<int*>(take(pix * sizeof(int)));
    unsigned long long* key = reinterpret_cast<unsigned long long*>(take((size_t)N * C * sizeof(unsigned long long)));
    if (ws) { ws->parent = parent; ws->area = area; ws->key = key; }
    return off;
}

static inline dim3 cc_grid(long long items) { return dim3((unsigned)(items < CC_GRID_CAP ? items : CC_GRID_CAP)); }

// ---- LDS union-find of one tile ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ int cc_lds_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ __forceinline__ int cc_lds_find(const int* par, int x) {
    // (a): par[x] <= x and x only ever moves to par[x] < x, so this ends after at most CC_TT steps; (c) a stale value is an ancestor
    for (int p = cc_lds_load(par + x); p != x; p = cc_lds_load(par + x)) x = p;
    return x;
}

__device__ __forceinline__ void cc_lds_union(int* par, int a, int b) {
    // (b): every further round continues with (old, lo), both < hi - the larger index of the pair strictly decreases
    for (;;) {
        a = cc_lds_find(par, a);
        b = cc_lds_find(par, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = atomicMin(&par[hi], lo);
        if (old == hi) return;                   // hi was a root and now hangs under lo
        a = old; b = lo;                         // hi had a parent old < hi already: old's tree and lo's still have to meet
    }
}

// ---- global union-find --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int cc_find(const int* parent, int x) {
    // (a): parent[x] <= x and x only ever moves to parent[x] < x: strictly decreasing, bounded below by 0; (c) a stale parent is an
    // earlier parent of x - a larger index of the same component - so the walk still ends at an index of the component
    for (int p = cc_load(parent + x); p != x; p = cc_load(parent + x)) x = p;
    return x;
}

__device__ __forceinline__ void cc_union(int* parent, int a, int b) {
    // (b): no wait on anybody - either the atomic linked a root (done) or it returned a parent old < hi and the next round runs on
    // (old, lo), whose larger index is strictly smaller than hi; (c) a find that ended on a stale "root" only makes old != hi
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = atomicMin(&parent[hi], lo);
        if (old == hi) return;
        a = old; b = lo;
    }
}

// 1. Work item = (sample, tile).  256 threads, four pixels each: thread t owns the local pixels t, t + 256, t + 512, t + 768 (local
// index = ly * CC_T + lx: its order is the row-major order of the sample restricted to the tile, so the local minimum is the tile's
// anchor).  A row of the tile is one half of a wave, so the horizontal RUNS of equal class come from one ballot: a pixel's first parent
// is the start of its run, and only the pixels where a run first meets a run of the row above union (a pixel whose left neighbour is
// of its run and whose upper-left neighbour is of the upper run leaves the union to that neighbour) - a few atomics per run, not four
// per pixel.  Also zeroes key[] and stats[] (grid-stride, every block a share): both are first touched by launch 4.
__global__ __launch_bounds__(256) void components_tile_kernel(const uint8_t* lp, int* __restrict__ parent, int* __restrict__ area,
                                                              unsigned long long* __restrict__ key,
                                                              unsigned long long* __restrict__ stats, CcGeom g) {
    __shared__ unsigned char cls[CC_TT];
    __shared__ int par[CC_TT];
    __shared__ int cnt[CC_TT];
    const int H = g.H, W = g.W, C = g.C;
    const size_t nk = (size_t)g.N * C, ns = stats ? nk * 4 : 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nk; i += (size_t)gridDim.x * 256) key[i] = 0ull;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < ns; i += (size_t)gridDim.x * 256) stats[i] = 0ull;

    const long long tps = (long long)g.tx * g.ty, items = (long long)g.N * tps;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int n = (int)(it / tps), t = (int)(it - (long long)n * tps);
        const int y0 = (t / g.tx) * CC_T, x0 = (t % g.tx) * CC_T;
        const int base = n * g.hw;                                            // < 2^31 (checked by the host)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = threadIdx.x + k * 256, ly = i / CC_T, lx = i % CC_T;
            const int y = y0 + ly, x = x0 + lx;
            unsigned c = CC_NONE;
            if (y < H && x < W) {
                c = lp[(size_t)base + (size_t)y * W + x];
                if (c >= (unsigned)C) c = CC_NONE;
            }
            cls[i] = (unsigned char)c;
            cnt[i] = 0;
        }
        __syncthreads();
        int len[4];                                                            // at the start of a run of a class: its length; else 0
#pragma unroll
        for (int k = 0; k < 4; ++k) {                                          // every lane of the wave is here: the ballot is whole
            const int i = threadIdx.x + k * 256, lx = i % CC_T;
            const unsigned c = cls[i];
            const bool start = lx == 0 || c == CC_NONE || cls[i - 1] != c;     // a pixel of no class is a "run" of its own
            const unsigned long long m = __ballot(start);
            const unsigned bits = (unsigned)(m >> (threadIdx.x & 32));         // this row's starts: bit 0 is always set
            const int s = 31 - __clz((int)(bits & (0xFFFFFFFFu >> (31 - lx))));
            const unsigned above = bits & ~((2u << lx) - 1u);                  // lx = 31: 2u << 31 = 0, the mask is empty
            par[i] = i - lx + s;                                               // (a): <= i, and of i's component
            len[k] = (start && c != CC_NONE) ? (above ? __ffs((int)above) - 1 : CC_T) - lx : 0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = threadIdx.x + k * 256, ly = i / CC_T, lx = i % CC_T;
            const unsigned c = cls[i];
            if (c == CC_NONE || ly == 0) continue;
            const bool left_same = lx > 0 && cls[i - 1] == c;
            if (cls[i - CC_T] == c) {                                          // the upper diagonals of its class are of the upper run
                if (!(left_same && cls[i - CC_T - 1] == c)) cc_lds_union(par, i, i - CC_T);
            } else if (g.conn8) {
                if (lx > 0 && !left_same && cls[i - CC_T - 1] == c) cc_lds_union(par, i, i - CC_T - 1);
                if (lx < CC_T - 1 && cls[i - CC_T + 1] == c) cc_lds_union(par, i, i - CC_T + 1);
            }
        }
        __syncthreads();
        int root[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {                                          // no union runs any more: par[] is only read here
            const int i = threadIdx.x + k * 256;
            root[k] = cc_lds_find(par, i);
            if (len[k]) atomicAdd(&cnt[root[k]], len[k]);                      // one add per run
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = threadIdx.x + k * 256, ly = i / CC_T, lx = i % CC_T;
            const int y = y0 + ly, x = x0 + lx;
            if (y < H && x < W) {
                const int r = root[k];
                const int p = base + y * W + x;
                parent[p] = base + (y0 + r / CC_T) * W + (x0 + r % CC_T);     // r <= i lies in the image whenever i does: same class
                area[p] = r == i ? cnt[i] : 0;
            }
        }
        __syncthreads();                                                       // the next item reuses the LDS arrays
    }
}

// 2. Work item = one pixel (y, x) of a sample with y % CC_T == 0, y > 0 (row seams: `rows` of them, W pixels each) or with
// x % CC_T == 0, x > 0 (column seams).  A row-seam pixel meets (y - 1, x + dx), a column-seam pixel (y + dy, x - 1), dx, dy = 0 and,
// for conn 8, -1 and +1.  Two neighbours in different tiles differ in their tile row (then the lower one is a row-seam pixel) or
// only in their tile column (then the right one is a column-seam pixel): every adjacency across a seam is met; the diagonal at a tile
// corner is met twice, which a union does not mind.
__global__ __launch_bounds__(256) void components_seam_kernel(const uint8_t* lp, int* parent, CcGeom g) {
    const int H = g.H, W = g.W, C = g.C;
    const int rows = g.ty - 1, cols = g.tx - 1;
    const long long per = (long long)rows * W + (long long)cols * H, items = (long long)g.N * per;
    for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long long)gridDim.x * 256) {
        const int n = (int)(it / per);
        long long r = it - (long long)n * per;
        const int base = n * g.hw;
        int y, x, sy, sx;                                                      // the pixel, and the step along the seam
        if (r < (long long)rows * W) { y = ((int)(r / W) + 1) * CC_T; x = (int)(r % W); sy = 0; sx = 1; }
        else { r -= (long long)rows * W; x = ((int)(r / H) + 1) * CC_T; y = (int)(r % H); sy = 1; sx = 0; }
        const int p = base + y * W + x;
        const unsigned c = lp[p];
        if (c >= (unsigned)C) continue;
        const int qy = y - sx, qx = x - sy;                                    // straight across the seam
        for (int d = g.conn8 ? -1 : 0; d <= (g.conn8 ? 1 : 0); ++d) {
            const int ny = qy + d * sy, nx = qx + d * sx;
            if (ny < 0 || ny >= H || nx < 0 || nx >= W) continue;
            const int q = base + ny * W + nx;
            if (lp[q] == c) cc_union(parent, p, q);
        }
    }
}

// 3. One thread per pixel.  No union runs in this launch, so the roots are fixed and a find ends on a true root; the stores only
// replace a parent by that root - a smaller index of the same component, (a) - and a concurrent find that reads the old value, (c),
// walks one step more.  area[] of a non-root is never a target of the adds, so reading it here is reading a value launch 1 wrote; the
// adds are the block-level partial sums of launch 1 (one per tile-local component), not one per pixel.
__global__ __launch_bounds__(256) void components_fold_kernel(int* parent, int* area, long long pix) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < pix; i += (long long)gridDim.x * 256) {
        const int p = (int)i;
        const int first = cc_load(parent + p);
        if (first == p) continue;
        const int r = cc_find(parent, first);
        if (r != first) __hip_atomic_store(parent + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int a = area[p];
        if (a) atomicAdd(&area[r], a);
    }
}

// 4. Work item = (sample n, block blk of bps): pixels blk * 256 + tid, + bps * 256, ... of the sample.  Global roots only.
__global__ __launch_bounds__(256) void components_select_kernel(const uint8_t* lp, const int* __restrict__ parent,
                                                                const int* __restrict__ area, unsigned long long* __restrict__ key,
                                                                unsigned long long* __restrict__ stats, CcGeom g) {
    __shared__ unsigned int ncomp[SSCG_MAXC];
    __shared__ unsigned long long best[SSCG_MAXC];
    const int C = g.C;
    const long long items = (long long)g.N * g.bps;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int n = (int)(it / g.bps), blk = (int)(it - (long long)n * g.bps);
        if ((int)threadIdx.x < C) { ncomp[threadIdx.x] = 0u; best[threadIdx.x] = 0ull; }
        __syncthreads();
        const int base = n * g.hw;
        for (long long o = (long long)blk * 256 + threadIdx.x; o < g.hw; o += (long long)g.bps * 256) {
            const int p = base + (int)o;
            if (parent[p] != p) continue;
            const unsigned c = lp[p];
            if (c >= (unsigned)C) continue;
            atomicAdd(&ncomp[c], 1u);
            if (!((g.exempt >> c) & 1ull))
                atomicMax(&best[c], ((unsigned long long)(unsigned)area[p] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)o));
        }
        __syncthreads();
        if ((int)threadIdx.x < C) {
            const int c = threadIdx.x;
            if (stats && ncomp[c]) atomicAdd(&stats[((size_t)n * C + c) * 4 + 0], (unsigned long long)ncomp[c]);
            if (best[c]) atomicMax(&key[(size_t)n * C + c], best[c]);
        }
        __syncthreads();
    }
}

// 5. Work item as in 4.  label_out may be label_pred: a pixel's byte is read and written by the same thread, nothing else reads it.
// bins: [C * C] hist (when asked for) | [3][C] kept components, pixels before, pixels after.
__global__ __launch_bounds__(256) void components_write_kernel(const uint8_t* lp, const int64_t* __restrict__ lt,
                                                               const int* __restrict__ parent, const int* __restrict__ area,
                                                               const unsigned long long* __restrict__ key, uint8_t* out,
                                                               unsigned long long* __restrict__ hist,
                                                               unsigned long long* __restrict__ stats, CcGeom g) {
    extern __shared__ unsigned int bins[];
    const int C = g.C;
    const int nh = hist ? C * C : 0, nb = nh + (stats ? 3 * C : 0);
    unsigned int* sb = bins + nh;
    const long long items = (long long)g.N * g.bps;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int n = (int)(it / g.bps), blk = (int)(it - (long long)n * g.bps);
        sscg_bins_clear(bins, nb);
        const int base = n * g.hw;
        for (long long o = (long long)blk * 256 + threadIdx.x; o < g.hw; o += (long long)g.bps * 256) {
            const int p = base + (int)o;
            const unsigned c = lp[p];
            unsigned q = c;
            if (c < (unsigned)C) {
                const int r = parent[p];
                bool keep = true;
                if (!((g.exempt >> c) & 1ull)) {
                    const unsigned a = (unsigned)area[r];
                    keep = a >= (unsigned)g.min_area;
                    if (g.largest)
                        keep = keep && key[(size_t)n * C + c] == (((unsigned long long)a << 32) | (0xFFFFFFFFu - (unsigned)(r - base)));
                }
                if (!keep) q = (unsigned)g.fill;
                if (stats) {
                    if (keep && r == p) atomicAdd(&sb[c], 1u);
                    atomicAdd(&sb[C + c], 1u);
                    atomicAdd(&sb[2 * C + q], 1u);
                }
                if (hist) sscg_bins_count(bins, C, lt[p], (int)q);
            }
            out[p] = (uint8_t)q;
        }
        sscg_bins_flush(bins, nh, hist);
        if (stats) {
            if (!nh) __syncthreads();
            for (int i = threadIdx.x; i < 3 * C; i += 256)
                if (sb[i]) atomicAdd(&stats[((size_t)n * C + i % C) * 4 + 1 + i / C], (unsigned long long)sb[i]);
        }
        __syncthreads();
    }
}

static inline bool cc_args_ok(int N, int H, int W, int C) { return N > 0 && H > 0 && W > 0 && C >= 1 && C <= SSCG_MAXC; }

static inline bool cc_too_large(int N, int H, int W) {
    const uint64_t rows = (uint64_t)N * (uint64_t)H;                   // < 2^62: the second product cannot wrap once this one is small
    return rows >= ((uint64_t)1 << 31) || rows * (uint64_t)W >= ((uint64_t)1 << 31);
}

static inline int cc_bps(int hw, int per_thread, int cap) {
    const int b = (hw + 256 * per_thread - 1) / (256 * per_thread);
    return b < 1 ? 1 : (b > cap ? cap : b);
}

}  // namespace

extern "C" size_t sscg_components_workspace(int N, int H, int W, int C) {
    if (!cc_args_ok(N, H, W, C) || cc_too_large(N, H, W)) return 0;
    return cc_carve(N, H, W, C, nullptr, nullptr);
}

extern "C" int sscg_components_filter(const uint8_t* label_pred, const int64_t* label_true, int N, int H, int W, int C, int conn,
                                      int largest, int min_area, int fill, uint64_t exempt_mask, uint8_t* label_out, int64_t* hist,
                                      int64_t* stats, void* ws, size_t ws_bytes, void* stream) {
    if (!label_pred || !label_out || !ws || (hist && !label_true)) return SSCG_ERR_BAD_ARG;
    if (!cc_args_ok(N, H, W, C) || (conn != 4 && conn != 8) || (largest != 0 && largest != 1) || min_area < 0 || fill < 0 || fill >= C)
        return SSCG_ERR_BAD_ARG;
    if (C < 64 && (exempt_mask >> C) != 0) return SSCG_ERR_BAD_ARG;
    if (cc_too_large(N, H, W)) return SSCG_ERR_UNSUPPORTED;
    CcWs w;
    if (ws_bytes < cc_carve(N, H, W, C, ws, &w)) return SSCG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    CcGeom g;
    g.N = N; g.H = H; g.W = W; g.C = C;
    g.hw = H * W;
    g.tx = (W + CC_T - 1) / CC_T;
    g.ty = (H + CC_T - 1) / CC_T;
    g.bps = cc_bps(g.hw, 16, 64);
    g.conn8 = conn == 8; g.largest = largest; g.min_area = min_area; g.fill = fill;
    g.exempt = exempt_mask | (1ull << fill);
    const long long pix = (long long)N * g.hw;
    unsigned long long* ustats = reinterpret_cast<unsigned long long*>(stats);
    unsigned long long* uhist = reinterpret_cast<unsigned long long*>(hist);

    hipLaunchKernelGGL(components_tile_kernel, cc_grid((long long)N * g.tx * g.ty), dim3(256), 0, st, label_pred, w.parent, w.area, w.key,
                       ustats, g);
    const long long seams = (long long)N * ((long long)(g.ty - 1) * W + (long long)(g.tx - 1) * H);
    if (seams > 0)
        hipLaunchKernelGGL(components_seam_kernel, dim3(ew_blocks((size_t)seams, 4096)), dim3(256), 0, st, label_pred, w.parent, g);
    hipLaunchKernelGGL(components_fold_kernel, dim3(ew_blocks((size_t)pix, 4096)), dim3(256), 0, st, w.parent, w.area, pix);
    hipLaunchKernelGGL(components_select_kernel, cc_grid((long long)N * g.bps), dim3(256), 0, st, label_pred, w.parent, w.area, w.key,
                       ustats, g);
    const size_t lds = ((size_t)(hist ? C * C : 0) + (size_t)(stats ? 3 * C : 0)) * sizeof(unsigned int);
    hipLaunchKernelGGL(components_write_kernel, cc_grid((long long)N * g.bps), dim3(256), lds, st, label_pred, label_true, w.parent,
                       w.area, w.key, label_out, uhist, ustats, g);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}
