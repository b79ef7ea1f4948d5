// Lovasz-softmax loss of the segmentation head (include/sscg.h: sscg_lovasz_fwd / sscg_lovasz_scale_add): Berman, Triki, Blaschko,
// "The Lovasz-Softmax loss: a tractable surrogate for the optimization of the intersection-over-union measure" (CVPR 2018).
//
// With p = softmax_C(resize(z)) (the pinned arithmetic of head_common.h; identity sizes: p = softmax_C(z)) and a pixel COUNTED when its
// label y lies in [0, C): for a segment s (the call, or one sample) and a class c the errors e_i = |[y_i == c] - p_i,c| of its V counted
// pixels are ordered descending, ties by ascending pixel index, and loss_{s,c} = sum_j e_(j) g_j with the Lovasz gradient g of the
// Jaccard index (the closed form below).  g is a constant of the backward, so the forward leaves the whole gradient with respect to
// the softmax map: coef[pixel][c] = +-g_rank * k - the layout and the meaning of the dy_soft operand of the head's backward entries.
//   1. lovasz_key_kernel    one thread per OUTPUT pixel, no block straddles a sample (ohem_key_kernel's frame): the pixel's logits
//                           and its softmax in registers, one key per class into the class-major plane [segment][class][pixel]:
//                           bits(e) + 1 for a counted pixel, 0 for an ignored one - which therefore sorts strictly last.  G (the
//                           foreground pixels per segment and class) and V through LDS bins and integer atomics;
//   2. sscg_sort_u32_desc   (sort.hip) the planes in descending order with their source pixels;
//   3. lovasz_count_kernel  the foreground flags labels[pixel] == c of every block's chunk of the sorted order, counted;
//      lovasz_scan_kernel   one block per plane: exclusive prefix sums of those counts.  A launch boundary on either side: no block
//                           waits for another;
//      lovasz_prep_kernel   one block: which classes enter which segment's mean, the live segments, the factor k of each plane;
//   4. lovasz_grad_kernel   the chunk again: F_j from the block's offset and ballots, g_j in fp64 from exact integers, e_(j) g_j
//                           into one fp64 record per block, the coefficient scattered to its pixel - every element of the map is
//                           written exactly once, a zero where the pixel is ignored or the class takes no part;
//   5. lovasz_finish_kernel one block: the records in index order, the means, the scalar.
// No float atomics, and nothing is read from the workspace before this call wrote it: the same bits from call to call.
#include "common.h"
#include "head_common.h"
#include "head_geom.h"
#include "scan_common.h"
#include "sscg_internal.h"

namespace {

constexpr int LV_KEY_BLOCKS = 256;        // key-pass blocks per sample, grid-stride beyond (ohem_key_kernel's frame)
constexpr int LV_ROUNDS = 4;
constexpr int LV_CHUNK = 256 * LV_ROUNDS; // sorted positions per block of the count and gradient passes
constexpr uint32_t LV_KEY_UPPER = 0x3F800002u;      // every key is at most bits(1.0f) + 1

struct LvGeom {
    sscg_resize_geom r;
    int npix;         // OH * OW
    int bps;          // key-pass blocks per sample
    int per_image;
    int L;            // pixels of a segment
};

// the workspace, every part rounded up to 256 bytes
struct LvLayout {
    size_t cnt, ksc, lsc, bsum, rec, skeys, sidx, sort, total;
    int nseg, planes, L, nbk;
};

size_t lv_round(size_t n) { return (n + 255) / 256 * 256; }

bool lv_layout(LvLayout* w, int N, int OH, int OW, int C, int per_image) {
    if (N <= 0 || OH <= 0 || OW <= 0 || C <= 0 || C > SSCG_MAXC) return false;
    const size_t npix = (size_t)OH * OW;
    if ((size_t)N * npix * C >= ((size_t)1 << 31)) return false;
    w->nseg = per_image ? N : 1;
    w->planes = w->nseg * C;
    w->L = (int)(per_image ? npix : (size_t)N * npix);
    w->nbk = (w->L + LV_CHUNK - 1) / LV_CHUNK;
    const size_t sort_ws = sscg_sort_ws_bytes(w->planes, w->L);
    if (sort_ws == 0) return false;
    size_t o = 0;
    w->cnt = o;   o += lv_round(((size_t)w->planes + w->nseg) * sizeof(uint32_t));
    w->ksc = o;   o += lv_round(((size_t)w->planes + 1) * sizeof(double));
    w->lsc = o;   o += lv_round((size_t)w->planes * sizeof(double));
    w->bsum = o;  o += lv_round((size_t)w->planes * w->nbk * sizeof(uint32_t));
    w->rec = o;   o += lv_round((size_t)w->planes * w->nbk * sizeof(double));
    w->skeys = o; o += lv_round((size_t)w->planes * w->L * sizeof(uint32_t));
    w->sidx = o;  o += lv_round((size_t)w->planes * w->L * sizeof(int32_t));
    w->sort = o;  o += sort_ws;
    w->total = o;
    return true;
}

__global__ __launch_bounds__(256) void lovasz_zero_kernel(uint32_t* __restrict__ words, int n) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) words[i] = 0u;
}

// e = |f - p| with p = v * inv rounded to fp32 first - the probability softmax_fwd_kernel stores: nothing here may contract
__device__ __forceinline__ uint32_t lovasz_key(float v, float inv, bool fg) {
#pragma clang fp contract(off)
    const float p = v * inv;
    const float e = fg ? 1.f - p : p;
    return __float_as_uint(e) + 1u;
}

template <int CT, bool RESIZE>
__global__ __launch_bounds__(256) void lovasz_key_kernel(const float* __restrict__ x, const int64_t* __restrict__ lab,
                                                         uint32_t* __restrict__ keys, uint32_t* __restrict__ cnt, LvGeom g, int nseg) {
    __shared__ unsigned int bins[SSCG_MAXC + 1];
    const int C = CT ? CT : g.r.C;
    if ((int)threadIdx.x <= C) bins[threadIdx.x] = 0u;
    __syncthreads();
    const int n = blockIdx.x / g.bps, blk = blockIdx.x - n * g.bps;
    const float* xn = x + (size_t)n * g.r.H * g.r.W * C;
    const size_t base = (size_t)n * g.npix;
    const int s = g.per_image ? n : 0;
    const size_t in_seg = g.per_image ? 0 : base;                 // the first pixel of this sample within its segment
    uint32_t* kp = keys + (size_t)s * C * g.L + in_seg;
    for (long o_raw = (long)blk * 256 + threadIdx.x; o_raw < g.npix; o_raw += (long)g.bps * 256) {
        const int o = (int)o_raw;
        const int64_t l64 = lab[base + o];
        if (l64 >= 0 && l64 < C) {
            const int l = (int)l64;
            float v[CT ? CT : SSCG_MAXC];
            const int oy = RESIZE ? fd_div(o, g.r.dow) : 0;
            sscg_pixel_logits<CT, !RESIZE>(xn, 0, oy, o - oy * g.r.OW, g.r.H, g.r.W, g.r.sh, g.r.sw, C, v);
            const float inv = sscg_softmax_exp<CT>(v, C);
#pragma unroll
            for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
                if (CT || c < C) kp[(size_t)c * g.L + o] = lovasz_key(v[c], inv, c == l);
            atomicAdd(&bins[l], 1u);
            atomicAdd(&bins[C], 1u);
        } else {
            for (int c = 0; c < C; ++c) kp[(size_t)c * g.L + o] = 0u;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < C) { if (bins[threadIdx.x]) atomicAdd(&cnt[s * C + threadIdx.x], bins[threadIdx.x]); }
    else if ((int)threadIdx.x == C) { if (bins[C]) atomicAdd(&cnt[nseg * C + s], bins[C]); }
}

// plane = s * C + c, block b: its chunk of the sorted order.  The flag of position p: the pixel there carries class c.
__device__ __forceinline__ bool lovasz_flag(const int32_t* __restrict__ sidx, const int64_t* __restrict__ lab, size_t plane_off,
                                            size_t seg_off, long p, uint32_t V, int c, int L) {
    if (p >= (long)V) return false;                               // ignored pixels rank last and carry no class
    const uint32_t i = (uint32_t)sidx[plane_off + p];
    return i < (uint32_t)L && lab[seg_off + i] == (int64_t)c;    // (i < L always: the sort wrote a permutation)
}

__global__ __launch_bounds__(256) void lovasz_count_kernel(const int32_t* __restrict__ sidx, const int64_t* __restrict__ lab,
                                                           const uint32_t* __restrict__ cnt, uint32_t* __restrict__ bsum, int C, int L,
                                                           int nbk, int nseg) {
    __shared__ uint32_t wc[4];
    const int plane = blockIdx.x / nbk, b = blockIdx.x - plane * nbk;
    const int s = plane / C, c = plane - s * C;
    const uint32_t V = cnt[nseg * C + s];
    const size_t plane_off = (size_t)plane * L, seg_off = (size_t)s * L;
    uint32_t own = 0;
#pragma unroll
    for (int r = 0; r < LV_ROUNDS; ++r) {
        const long p = (long)b * LV_CHUNK + r * 256 + threadIdx.x;
        own += (uint32_t)__popcll(__ballot(lovasz_flag(sidx, lab, plane_off, seg_off, p, V, c, L)));
    }
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = own;
    __syncthreads();
    if (threadIdx.x == 0) bsum[(size_t)plane * nbk + b] = (wc[0] + wc[1]) + (wc[2] + wc[3]);
}

__global__ __launch_bounds__(256) void lovasz_scan_kernel(uint32_t* __restrict__ bsum, int nbk) {
    __shared__ uint32_t wsum[4];
    block_excl_scan_u32(bsum + (size_t)blockIdx.x * nbk, (size_t)nbk, wsum);
}

// One block.  A class enters a segment's mean when it is not skipped and (all classes, or it has a foreground pixel there); a segment
// is live when it has a counted pixel (per sample) - the call as one segment always is.  ksc[plane] = 1 / (classes of the segment *
// live segments), 0 where the plane takes no part; ksc[planes] = the number of live segments.
__global__ __launch_bounds__(256) void lovasz_prep_kernel(const uint32_t* __restrict__ cnt, double* __restrict__ ksc, int C, int nseg,
                                                          int per_image, int classes_all, unsigned long long skip) {
    __shared__ unsigned int live;
    if (threadIdx.x == 0) live = 0u;
    __syncthreads();
    for (int s = threadIdx.x; s < nseg; s += 256)
        if (!per_image || cnt[nseg * C + s] > 0u) atomicAdd(&live, 1u);
    __syncthreads();
    const double nlive = (double)live;
    for (int s = threadIdx.x; s < nseg; s += 256) {
        const bool alive = !per_image || cnt[nseg * C + s] > 0u;
        int ncls = 0;
        for (int c = 0; c < C; ++c)
            ncls += (!((skip >> c) & 1ull) && (classes_all || cnt[s * C + c] > 0u)) ? 1 : 0;
        for (int c = 0; c < C; ++c) {
            const bool in = !((skip >> c) & 1ull) && (classes_all || cnt[s * C + c] > 0u);
            ksc[s * C + c] = (alive && in) ? 1.0 / ((double)ncls * nlive) : 0.0;
        }
    }
    if (threadIdx.x == 0) ksc[(size_t)nseg * C] = nlive;
}

// Rank j = p + 1 of a counted pixel, F = the foreground pixels among the first j, G those of the plane:
//   I = G - F, U = G + j - F;   foreground: g = 1 / U;   background: g = I / (U (U - 1)), at j = 1: 1 / (G + 1)
// - the differences J_j - J_{j-1} of J = 1 - I / U in closed form, from exact integers in fp64.
__global__ __launch_bounds__(256) void lovasz_grad_kernel(const uint32_t* __restrict__ skeys, const int32_t* __restrict__ sidx,
                                                          const int64_t* __restrict__ lab, const uint32_t* __restrict__ cnt,
                                                          const uint32_t* __restrict__ bsum, const double* __restrict__ ksc,
                                                          double* __restrict__ rec, float* __restrict__ coef, int C, int L, int nbk,
                                                          int nseg) {
    __shared__ uint32_t wc[LV_ROUNDS][4];
    __shared__ double sm[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int plane = blockIdx.x / nbk, b = blockIdx.x - plane * nbk;
    const int s = plane / C, c = plane - s * C;
    const uint32_t V = cnt[nseg * C + s], G = cnt[plane];
    const double k = ksc[plane];
    const size_t plane_off = (size_t)plane * L, seg_off = (size_t)s * L;
    const unsigned long long below = (1ull << lane) - 1ull;
    bool flag[LV_ROUNDS];
    uint32_t before[LV_ROUNDS];
#pragma unroll
    for (int r = 0; r < LV_ROUNDS; ++r) {
        const long p = (long)b * LV_CHUNK + r * 256 + tid;
        flag[r] = lovasz_flag(sidx, lab, plane_off, seg_off, p, V, c, L);
        const unsigned long long m = __ballot(flag[r]);
        before[r] = (uint32_t)__popcll(m & below);
        if (lane == 0) wc[r][wave] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    uint32_t run = bsum[(size_t)plane * nbk + b];
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < LV_ROUNDS; ++r) {
        uint32_t F = run + before[r];
        for (int w = 0; w < wave; ++w) F += wc[r][w];
        run += (wc[r][0] + wc[r][1]) + (wc[r][2] + wc[r][3]);
        const long p = (long)b * LV_CHUNK + r * 256 + tid;
        if (p >= L) continue;
        const uint32_t i = (uint32_t)sidx[plane_off + p];
        if (i >= (uint32_t)L) continue;                           // (never: the sort wrote a permutation)
        const size_t pixel = seg_off + i;
        float out = 0.f;
        if (p < (long)V) {
            F += flag[r] ? 1u : 0u;                                // inclusive
            const double j = (double)(p + 1), Gd = (double)G, Fd = (double)F;
            const double I = Gd - Fd, U = Gd + j - Fd;
            double gj;
            if (flag[r]) gj = 1.0 / U;
            else gj = p == 0 ? 1.0 / (Gd + 1.0) : I / (U * (U - 1.0));
            const double e = (double)__uint_as_float(skeys[plane_off + p] - 1u);
            if (k != 0.0) {
                acc += e * gj;
                out = (float)((flag[r] ? -gj : gj) * k);
            }
        }
        coef[pixel * C + c] = out;
    }
    acc = wave_sum(acc);
    if (lane == 0) sm[wave] = acc;
    __syncthreads();
    if (tid == 0) rec[(size_t)plane * nbk + b] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

// One block: loss_{s,c} = its records in index order; the loss = sum of ksc * loss_{s,c} (strided partial sums, then the 256 in
// order); per_class[c] = the mean of loss_{s,c} over the live segments in which the class took part.
__global__ __launch_bounds__(256) void lovasz_finish_kernel(const double* __restrict__ rec, const double* __restrict__ ksc,
                                                            double* __restrict__ lsc, int planes, int nbk, int C, float* __restrict__ loss,
                                                            float* __restrict__ per_class) {
    __shared__ double sm[256];
    double part = 0.0;
    for (int pl = threadIdx.x; pl < planes; pl += 256) {
        double t = 0.0;
        for (int b = 0; b < nbk; ++b) t += rec[(size_t)pl * nbk + b];
        lsc[pl] = t;
        part += t * ksc[pl];
    }
    sm[threadIdx.x] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < 256; ++i) t += sm[i];
        *loss = (float)t;
    }
    if (per_class && (int)threadIdx.x < C) {
        const double nlive = ksc[planes];
        double t = 0.0;
        for (int pl = threadIdx.x; pl < planes; pl += C)
            if (ksc[pl] != 0.0) t += lsc[pl];
        per_class[threadIdx.x] = nlive > 0.0 ? (float)(t / nlive) : 0.f;
    }
}

__global__ __launch_bounds__(256) void lovasz_scale_add_kernel(const float* __restrict__ coef, const float* __restrict__ g,
                                                               const float* __restrict__ dy, float* __restrict__ out, size_t n) {
    const float gs = *g;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        out[i] = dy ? dy[i] + gs * coef[i] : gs * coef[i];
}

int lv_bps(int OH, int OW) {
    const long b = ((long)OH * OW + 255) / 256;
    return (int)(b > LV_KEY_BLOCKS ? LV_KEY_BLOCKS : b);
}

template <bool RESIZE>
void launch_lovasz_keys(const LvGeom& g, int N, int nseg, hipStream_t st, const float* x, const int64_t* lab, uint32_t* keys, uint32_t* cnt) {
    const dim3 grid((unsigned)N * g.bps), blk(256);
    sscg_dispatch_classes(g.r.C, [&](auto ct) {
        hipLaunchKernelGGL((lovasz_key_kernel<decltype(ct)::value, RESIZE>), grid, blk, 0, st, x, lab, keys, cnt, g, nseg);
    });
}

}  // namespace

extern "C" size_t sscg_lovasz_workspace(int N, int OH, int OW, int C, int per_image) {
    LvLayout w;
    return lv_layout(&w, N, OH, OW, C, per_image) ? w.total : 0;
}

extern "C" int sscg_lovasz_fwd(const float* x, const int64_t* labels, int N, int H, int W, int C, int OH, int OW, int classes_all,
                               int per_image, uint64_t skip_mask, uint32_t* keys, float* coef, float* loss, float* per_class, void* ws,
                               size_t ws_bytes, void* stream) {
    if (!x || !labels || !keys || !coef || !loss || !sizes_ok(N, H, W, C, OH, OW)) return SSCG_ERR_BAD_ARG;
    if ((classes_all != 0 && classes_all != 1) || (per_image != 0 && per_image != 1)) return SSCG_ERR_BAD_ARG;
    const uint64_t every = C == 64 ? ~(uint64_t)0 : (((uint64_t)1 << C) - 1);
    if ((skip_mask & ~every) != 0 || (classes_all && (skip_mask & every) == every)) return SSCG_ERR_BAD_ARG;
    if (too_large(N, H, W, OH, OW)) return SSCG_ERR_UNSUPPORTED;
    LvLayout w;
    if (!lv_layout(&w, N, OH, OW, C, per_image)) return SSCG_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < w.total) return SSCG_ERR_WORKSPACE;
    if (((uintptr_t)ws & 7u) != 0) return SSCG_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    char* base = reinterpret_cast<char*>(ws);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(base + w.cnt);
    double* ksc = reinterpret_cast<double*>(base + w.ksc);
    double* lsc = reinterpret_cast<double*>(base + w.lsc);
    uint32_t* bsum = reinterpret_cast<uint32_t*>(base + w.bsum);
    double* rec = reinterpret_cast<double*>(base + w.rec);
    uint32_t* skeys = reinterpret_cast<uint32_t*>(base + w.skeys);
    int32_t* sidx = reinterpret_cast<int32_t*>(base + w.sidx);
    const LvGeom g = {sscg_make_resize_geom(H, W, C, OH, OW), OH * OW, lv_bps(OH, OW), per_image, w.L};
    hipLaunchKernelGGL(lovasz_zero_kernel, dim3(ew_blocks((size_t)w.planes + w.nseg, 64)), dim3(256), 0, st, cnt, w.planes + w.nseg);
    if (OH == H && OW == W) launch_lovasz_keys<false>(g, N, w.nseg, st, x, labels, keys, cnt);
    else launch_lovasz_keys<true>(g, N, w.nseg, st, x, labels, keys, cnt);
    const int rc = sscg_sort_u32_desc(keys, w.planes, w.L, LV_KEY_UPPER, skeys, sidx, base + w.sort, ws_bytes - w.sort, stream);
    if (rc != SSCG_OK) return rc;
    const dim3 grid((unsigned)w.planes * (unsigned)w.nbk), blk(256);
    hipLaunchKernelGGL(lovasz_count_kernel, grid, blk, 0, st, sidx, labels, cnt, bsum, C, w.L, w.nbk, w.nseg);
    hipLaunchKernelGGL(lovasz_scan_kernel, dim3((unsigned)w.planes), blk, 0, st, bsum, w.nbk);
    hipLaunchKernelGGL(lovasz_prep_kernel, dim3(1), blk, 0, st, cnt, ksc, C, w.nseg, per_image, classes_all, (unsigned long long)skip_mask);
    hipLaunchKernelGGL(lovasz_grad_kernel, grid, blk, 0, st, skeys, sidx, labels, cnt, bsum, ksc, rec, coef, C, w.L, w.nbk, w.nseg);
    hipLaunchKernelGGL(lovasz_finish_kernel, dim3(1), blk, 0, st, rec, ksc, lsc, w.planes, w.nbk, C, loss, per_class);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_lovasz_scale_add(const float* coef, const float* g, const float* dy_soft, float* out, int64_t n, void* stream) {
    if (!coef || !g || !out || n <= 0) return SSCG_ERR_BAD_ARG;
    hipLaunchKernelGGL(lovasz_scale_add_kernel, dim3(ew_blocks((size_t)n)), dim3(256), 0, (hipStream_t)stream, coef, g, dy_soft, out, (size_t)n);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}
