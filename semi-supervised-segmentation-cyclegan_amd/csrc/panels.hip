// Per-epoch image panels (include/sscg.h lists the reference call sites): the tail of the reference's epoch loop on the device.
//   sscg_panel_labels: low-resolution logits -> resize -> softmax -> first maximum -> uint8 ids + the fp32 one-hot map Gis consumes
//   sscg_panel_range:  min / max of a panel's pre-normalisation values (make_grid(normalize=True) takes them over the whole batch)
//   sscg_panel_grid:   make_grid(nrow, normalize=True) + the float -> byte conversion of the image writer, CHW bytes in one launch
// Forward only; the training step never launches them.  The per-pixel arithmetic of the head is head_common.h's, the arithmetic of
// the grid is stated in the header so that a host restatement agrees byte for byte.
#include "common.h"
#include "head_common.h"
#include "sscg_internal.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef int64_t i64x2 __attribute__((ext_vector_type(2)));

constexpr int PANEL_THREADS = 256;
// the stores of a panel are a few MB to a few tens of MB: 4 workgroups per CU keep every CU's store queue fed, more only lengthens
// the tail of partial results (range) and the palette copies per launch (grid)
constexpr int PANEL_MAX_BLOCKS = 1024;

// ------------------------------------------------------------------------------------------------------------------ labels
struct LabelGeom {
    sscg_resize_geom r;
    FastDiv dc;
};

// A workgroup takes 256 consecutive output pixels at a time.  Phase 1: one thread per pixel, its C logits in registers, the functions
// of head_common.h as in predict_head_kernel - the id goes to LDS.  Phase 2 writes what the 256 ids stand for: their bytes as 16
// 16-byte stores, and the chunk's 256 * C one-hot floats - one contiguous range of the [pixels][C] map - as 16-byte vectors, a wave's
// store covering 1 KB of consecutive addresses (a thread per pixel would scatter C four-byte stores 4 * C bytes apart).  `mis`: floats
// by which the one-hot base misses 16-byte alignment (0..3; 4 = not even float aligned: scalar stores only); elements in front of the
// first aligned address of a chunk and behind its last full vector leave as scalars.
template <int CT, bool IDENT>
__global__ __launch_bounds__(PANEL_THREADS) void panel_labels_kernel(const float* __restrict__ x, uint8_t* __restrict__ label_u8,
                                                                     float* __restrict__ onehot, int total, int mis, LabelGeom g) {
    __shared__ __attribute__((aligned(16))) uint8_t ids[PANEL_THREADS];
    const int C = CT ? CT : g.r.C;
    const int chunks = (total + PANEL_THREADS - 1) / PANEL_THREADS;
    const bool u8_vec = ((size_t)label_u8 & 15) == 0;
    for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        const int p0 = ch * PANEL_THREADS;
        const int np = min(PANEL_THREADS, total - p0);
        const int o = p0 + (int)threadIdx.x;
        if (o < total) {
            float v[CT ? CT : SSCG_MAXC];
            const sscg_pixel p = IDENT ? sscg_pixel{0, 0, o} : sscg_pixel_of(o, g.r);
            sscg_pixel_logits<CT, IDENT>(x, p.n, p.oy, p.ox, g.r.H, g.r.W, g.r.sh, g.r.sw, C, v);
            const float inv = sscg_softmax_exp<CT>(v, C);
            ids[threadIdx.x] = (uint8_t)sscg_first_max_scaled<CT>(v, inv, C);
        }
        __syncthreads();
        // ---- the ids as bytes
        if (u8_vec && np == PANEL_THREADS) {        // p0 is a multiple of 256: the chunk starts 16-byte aligned
            if (threadIdx.x < PANEL_THREADS / 16)
                reinterpret_cast<u32x4*>(label_u8 + p0)[threadIdx.x] = reinterpret_cast<const u32x4*>(ids)[threadIdx.x];
        } else if ((int)threadIdx.x < np) {
            label_u8[p0 + threadIdx.x] = ids[threadIdx.x];
        }
        // ---- the one-hot rows of the chunk: floats [0, ne) behind `row0`
        if (onehot) {
            float* row0 = onehot + (size_t)p0 * C;
            const int ne = np * C;
            // p0 * C is a multiple of 4, so the chunk misses alignment by what the base misses it
            const int head = mis >= 4 ? ne : min((4 - mis) & 3, ne);
            const int nvec = (ne - head) >> 2;
            for (int j = threadIdx.x; j < nvec; j += PANEL_THREADS) {
                const int e = head + 4 * j;
                int p = CT ? e / (CT ? CT : 1) : fd_div(e, g.dc);
                int c = e - p * C;
                float w[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    w[k] = (int)ids[p] == c ? 1.f : 0.f;
                    if (++c == C) { c = 0; ++p; }       // p may pass the chunk's last pixel only behind its last element
                }
                *reinterpret_cast<f32x4*>(row0 + e) = f32x4{w[0], w[1], w[2], w[3]};
            }
            const int tail0 = head + 4 * nvec;
            const int nscal = head + (ne - tail0);       // at most 3 + 3 elements per chunk (all of them when unaligned)
            for (int j = threadIdx.x; j < nscal; j += PANEL_THREADS) {
                const int e = j < head ? j : tail0 + (j - head);
                const int p = CT ? e / (CT ? CT : 1) : fd_div(e, g.dc);
                row0[e] = (int)ids[p] == e - p * C ? 1.f : 0.f;
            }
        }
        __syncthreads();            // the next chunk overwrites ids
    }
}

template <bool IDENT>
void launch_labels(const LabelGeom& g, int total, int mis, hipStream_t st, const float* x, uint8_t* label_u8, float* onehot) {
    const int chunks = (total + PANEL_THREADS - 1) / PANEL_THREADS;
    const dim3 grid(chunks > PANEL_MAX_BLOCKS ? PANEL_MAX_BLOCKS : chunks), blk(PANEL_THREADS);
    sscg_dispatch_classes(g.r.C, [&](auto ct) {
        hipLaunchKernelGGL((panel_labels_kernel<decltype(ct)::value, IDENT>), grid, blk, 0, st, x, label_u8, onehot, total, mis, g);
    });
}

// ------------------------------------------------------------------------------------------------------------------ values
enum { KIND_IMAGE = SSCG_PANEL_IMAGE, KIND_COLOUR = SSCG_PANEL_COLOUR, KIND_GREY = SSCG_PANEL_GREY };

// the un-normalise of model.py:603-615: a multiply, then an add, each rounded to fp32 on its own.  Plain operators under the pragma
// (pixel_u8 of predict.hip says why not __fmul_rn / __fadd_rn).
__device__ __forceinline__ float panel_unnorm(float x, float scale, float shift) {
#pragma clang fp contract(off)
    const float m = x * scale;
    return m + shift;
}

template <int KIND> struct panel_elem;
template <> struct panel_elem<KIND_IMAGE> { typedef float type; };
template <> struct panel_elem<KIND_COLOUR> { typedef uint8_t type; };
template <> struct panel_elem<KIND_GREY> { typedef int64_t type; };

struct MinMax {
    float lo, hi;
    __device__ __forceinline__ void take(float v) { lo = fminf(lo, v); hi = fmaxf(hi, v); }
    __device__ __forceinline__ void take(float a, float b) { lo = fminf(lo, a); hi = fmaxf(hi, b); }
};

// wave shuffles, then LDS across the four waves: thread 0 returns the workgroup's pair.  min / max of finite values: exact and
// independent of the order.
__device__ __forceinline__ MinMax block_minmax(MinMax m) {
    __shared__ float part[2 * (PANEL_THREADS / 64)];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m.lo = fminf(m.lo, __shfl_xor(m.lo, o, 64));
        m.hi = fmaxf(m.hi, __shfl_xor(m.hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        part[2 * (threadIdx.x >> 6)] = m.lo;
        part[2 * (threadIdx.x >> 6) + 1] = m.hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < PANEL_THREADS / 64; ++w) m.take(part[2 * w], part[2 * w + 1]);
    }
    return m;
}

// Pass 1: every workgroup reduces a strided share of the n source elements to one (min, max) pair in out[2 * blockIdx.x].  Elements
// [head, head + VEC * nvec) are read as 16-byte vectors (head: elements in front of the first aligned address), the rest one by one.
// COLOUR reduces per id over the three palette channels at once: LDS holds each id's smallest and largest channel.
template <int KIND>
__global__ __launch_bounds__(PANEL_THREADS) void panel_range_kernel(const void* __restrict__ src_, int64_t n, int64_t head, int64_t nvec,
                                                                    float scale, float shift, const uint8_t* __restrict__ palette,
                                                                    float* __restrict__ out) {
    typedef typename panel_elem<KIND>::type T;
    constexpr int VEC = 16 / (int)sizeof(T);
    const T* __restrict__ src = static_cast<const T*>(src_);
    __shared__ float pal_lo[KIND == KIND_COLOUR ? 256 : 1], pal_hi[KIND == KIND_COLOUR ? 256 : 1];
    if constexpr (KIND == KIND_COLOUR) {
        const uint8_t* p = palette + 3 * threadIdx.x;
        pal_lo[threadIdx.x] = (float)min(min(p[0], p[1]), p[2]);
        pal_hi[threadIdx.x] = (float)max(max(p[0], p[1]), p[2]);
        __syncthreads();
    }
    MinMax m = {INFINITY, -INFINITY};
    auto one = [&](T e) {
        if constexpr (KIND == KIND_IMAGE) m.take(panel_unnorm(e, scale, shift));
        else if constexpr (KIND == KIND_COLOUR) m.take(pal_lo[e], pal_hi[e]);
        else m.take((float)e);
    };
    const int64_t stride = (int64_t)gridDim.x * PANEL_THREADS;
    const int64_t t0 = (int64_t)blockIdx.x * PANEL_THREADS + threadIdx.x;
    for (int64_t q = t0; q < nvec; q += stride) {
        const T* p = src + head + q * VEC;
        if constexpr (KIND == KIND_IMAGE) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
            for (int k = 0; k < 4; ++k) one(v[k]);
        } else if constexpr (KIND == KIND_COLOUR) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
            for (int k = 0; k < 16; ++k) one((uint8_t)(v[k >> 2] >> (8 * (k & 3))));
        } else {
            const i64x2 v = *reinterpret_cast<const i64x2*>(p);
            one(v[0]);
            one(v[1]);
        }
    }
    const int64_t tail0 = head + nvec * VEC;
    const int64_t nscal = head + (n - tail0);
    for (int64_t j = t0; j < nscal; j += stride) one(src[j < head ? j : tail0 + (j - head)]);
    m = block_minmax(m);
    if (threadIdx.x == 0) {
        out[2 * blockIdx.x] = m.lo;
        out[2 * blockIdx.x + 1] = m.hi;
    }
}

// Pass 2 (more than one workgroup in pass 1): the pairs of the workspace -> range[0], range[1]
__global__ __launch_bounds__(PANEL_THREADS) void panel_range_tail_kernel(const float* __restrict__ part, int nparts, float* __restrict__ range) {
    MinMax m = {INFINITY, -INFINITY};
    for (int i = threadIdx.x; i < nparts; i += PANEL_THREADS) m.take(part[2 * i], part[2 * i + 1]);
    m = block_minmax(m);
    if (threadIdx.x == 0) {
        range[0] = m.lo;
        range[1] = m.hi;
    }
}

int range_blocks(int64_t pixels, int C) {
    // a thread's unit of work is one 16-byte vector; every kind fits at least 2 elements into one
    const int64_t work = (pixels * (C > 0 ? C : 1) + 1) / 2;
    const int64_t b = (work + PANEL_THREADS - 1) / PANEL_THREADS;
    return b > PANEL_MAX_BLOCKS ? PANEL_MAX_BLOCKS : (b < 1 ? 1 : (int)b);
}

// ------------------------------------------------------------------------------------------------------------------ grid
struct GridGeom {
    int N, H, W, C;
    int pad, xmaps, GH, GW;         // pad = 0 and GH x GW = H x W for torchvision's N == 1 case
    FastDiv dgw, dgh, dcw, dch;     // by GW, GH, the cell sizes W + pad, H + pad
};

// one byte of the grid at channel ch, row gy, column gx
template <int KIND>
__device__ __forceinline__ uint8_t grid_byte(const void* __restrict__ src, const float* pal, const GridGeom& g, int ch, int gy, int gx,
                                             float scale, float shift, float lo, float d) {
    const int ty = gy - g.pad, tx = gx - g.pad;
    if (ty < 0 || tx < 0) return 0;
    const int cy = fd_div(ty, g.dch), cx = fd_div(tx, g.dcw);
    const int y = ty - cy * (g.H + g.pad), x = tx - cx * (g.W + g.pad);
    const int k = cy * g.xmaps + cx;
    if (y >= g.H || x >= g.W || k >= g.N) return 0;         // the border behind a tile, an unused cell
    const size_t pix = ((size_t)k * g.H + y) * g.W + x;
    float v;
    if constexpr (KIND == KIND_IMAGE) v = panel_unnorm(static_cast<const float*>(src)[pix * g.C + (g.C == 3 ? ch : 0)], scale, shift);
    else if constexpr (KIND == KIND_COLOUR) v = pal[3 * static_cast<const uint8_t*>(src)[pix] + ch];
    else v = (float)static_cast<const int64_t*>(src)[pix];
    const float u = __fdiv_rn(__fsub_rn(v, lo), d);
    return (uint8_t)(int)fminf(fmaxf(__fmul_rn(u, 255.f), 0.f), 255.f);
}

// Every thread owns 16 consecutive bytes of the flat [3][GH][GW] grid (a group may straddle a row, a tile edge or a channel plane)
// and stores them as one 16-byte vector.  Bytes [0, head) in front of the first aligned address and those behind the last full group
// leave one by one.
template <int KIND>
__global__ __launch_bounds__(PANEL_THREADS) void panel_grid_kernel(const void* __restrict__ src, const uint8_t* __restrict__ palette,
                                                                   const float* __restrict__ range, uint8_t* __restrict__ grid, GridGeom g,
                                                                   float scale, float shift, int total, int head, int groups) {
    __shared__ float pal[KIND == KIND_COLOUR ? 768 : 1];
    if constexpr (KIND == KIND_COLOUR) {
        for (int i = threadIdx.x; i < 768; i += PANEL_THREADS) pal[i] = (float)palette[i];
        __syncthreads();
    }
    const float lo = range[0], hi = range[1];
    const float d = (float)fmax((double)hi - (double)lo, 1e-5);
    const int stride = gridDim.x * PANEL_THREADS;
    const int t0 = blockIdx.x * PANEL_THREADS + threadIdx.x;
    for (int q = t0; q < groups; q += stride) {
        const int i0 = head + 16 * q;
        const int r = fd_div(i0, g.dgw);
        int gx = i0 - r * g.GW;
        int ch = fd_div(r, g.dgh);
        int gy = r - ch * g.GH;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            w[e >> 2] |= (uint32_t)grid_byte<KIND>(src, pal, g, ch, gy, gx, scale, shift, lo, d) << (8 * (e & 3));
            if (e < 15 && ++gx == g.GW) {           // the next byte of the group is in range: i0 + 15 < total
                gx = 0;
                if (++gy == g.GH) { gy = 0; ++ch; }
            }
        }
        *reinterpret_cast<u32x4*>(grid + i0) = u32x4{w[0], w[1], w[2], w[3]};
    }
    const int tail0 = head + 16 * groups;
    const int nscal = head + (total - tail0);
    for (int j = t0; j < nscal; j += stride) {
        const int i = j < head ? j : tail0 + (j - head);
        const int r = fd_div(i, g.dgw);
        const int ch = fd_div(r, g.dgh);
        grid[i] = grid_byte<KIND>(src, pal, g, ch, r - ch * g.GH, i - r * g.GW, scale, shift, lo, d);
    }
}

// shared argument rules of the range and the grid
int panel_kind_check(const void* src, int kind, int C, const uint8_t* palette) {
    if (!src || (kind != KIND_IMAGE && kind != KIND_COLOUR && kind != KIND_GREY)) return SSCG_ERR_BAD_ARG;
    if (kind == KIND_IMAGE ? (C != 1 && C != 3) : C != 1) return SSCG_ERR_BAD_ARG;
    if (kind == KIND_COLOUR && !palette) return SSCG_ERR_BAD_ARG;
    return SSCG_OK;
}

}  // namespace

extern "C" int sscg_panel_labels(const float* x, int N, int H, int W, int C, int OH, int OW, uint8_t* label_u8, float* onehot, void* stream) {
    if (!x || !label_u8 || N <= 0 || H <= 0 || W <= 0 || C <= 0 || OH <= 0 || OW <= 0) return SSCG_ERR_BAD_ARG;
    if (C > SSCG_MAXC) return SSCG_ERR_UNSUPPORTED;
    const size_t pixels = (size_t)N * OH * OW;
    if (pixels * (onehot ? (size_t)C : 1) >= ((size_t)1 << 31)) return SSCG_ERR_UNSUPPORTED;
    const LabelGeom g = {sscg_make_resize_geom(H, W, C, OH, OW), make_fastdiv(C)};
    const int mis = ((size_t)onehot & 3) ? 4 : (int)(((size_t)onehot >> 2) & 3);
    if (OH == H && OW == W) launch_labels<true>(g, (int)pixels, mis, (hipStream_t)stream, x, label_u8, onehot);
    else launch_labels<false>(g, (int)pixels, mis, (hipStream_t)stream, x, label_u8, onehot);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" size_t sscg_panel_range_workspace(int64_t pixels, int C) {
    if (pixels <= 0) return 0;
    const int b = range_blocks(pixels, C);
    return b > 1 ? (size_t)b * 2 * sizeof(float) : 0;
}

extern "C" int sscg_panel_range(const void* src, int kind, int64_t pixels, int C, float scale, float shift, const uint8_t* palette,
                                float* range, void* ws, size_t ws_bytes, void* stream) {
    const int rc = panel_kind_check(src, kind, C, palette);
    if (rc != SSCG_OK) return rc;
    if (!range || pixels <= 0) return SSCG_ERR_BAD_ARG;
    const int blocks = range_blocks(pixels, C);
    if (blocks > 1 && (!ws || ws_bytes < (size_t)blocks * 2 * sizeof(float))) return SSCG_ERR_WORKSPACE;
    const int64_t n = pixels * C;
    const size_t esz = kind == KIND_IMAGE ? 4 : (kind == KIND_COLOUR ? 1 : 8);
    const size_t a = (size_t)src;
    // elements in front of the first 16-byte aligned address; a source that is not even element aligned is read one by one
    int64_t head = (a % esz) ? n : (int64_t)(((16 - (a & 15)) & 15) / esz);
    if (head > n) head = n;
    const int64_t nvec = (n - head) / (int64_t)(16 / esz);
    float* out = blocks > 1 ? static_cast<float*>(ws) : range;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid(blocks), blk(PANEL_THREADS);
    if (kind == KIND_IMAGE) hipLaunchKernelGGL(panel_range_kernel<KIND_IMAGE>, grid, blk, 0, st, src, n, head, nvec, scale, shift, palette, out);
    else if (kind == KIND_COLOUR) hipLaunchKernelGGL(panel_range_kernel<KIND_COLOUR>, grid, blk, 0, st, src, n, head, nvec, scale, shift, palette, out);
    else hipLaunchKernelGGL(panel_range_kernel<KIND_GREY>, grid, blk, 0, st, src, n, head, nvec, scale, shift, palette, out);
    SSCG_LAUNCH_CHECK();
    if (blocks > 1) {
        hipLaunchKernelGGL(panel_range_tail_kernel, dim3(1), blk, 0, st, out, blocks, range);
        SSCG_LAUNCH_CHECK();
    }
    return SSCG_OK;
}

extern "C" int sscg_panel_grid(const void* src, int kind, int N, int H, int W, int C, float scale, float shift, const uint8_t* palette,
                               const float* range, int nrow, int padding, uint8_t* grid, void* stream) {
    const int rc = panel_kind_check(src, kind, C, palette);
    if (rc != SSCG_OK) return rc;
    if (!range || !grid || N <= 0 || H <= 0 || W <= 0 || nrow <= 0 || padding < 0) return SSCG_ERR_BAD_ARG;
    GridGeom g;
    g.N = N; g.H = H; g.W = W; g.C = C;
    g.pad = N == 1 ? 0 : padding;                   // make_grid returns a single image as it is
    g.xmaps = nrow < N ? nrow : N;
    const int ymaps = (N + g.xmaps - 1) / g.xmaps;
    const int64_t gh = (int64_t)ymaps * ((int64_t)H + g.pad) + g.pad, gw = (int64_t)g.xmaps * ((int64_t)W + g.pad) + g.pad;
    const int64_t lim = (int64_t)1 << 31;
    // (the tiles lie inside the grid: gh * gw below the limit bounds N * H * W too)
    if (gh >= lim || gw >= lim || gh * gw >= lim || 3 * gh * gw >= lim || (int64_t)N * H * W * C >= lim) return SSCG_ERR_UNSUPPORTED;
    g.GH = (int)gh; g.GW = (int)gw;
    g.dgw = make_fastdiv(g.GW);
    g.dgh = make_fastdiv(g.GH);
    g.dcw = make_fastdiv(W + g.pad);
    g.dch = make_fastdiv(H + g.pad);
    const int total = (int)(3 * gh * gw);
    int head = (int)((16 - ((size_t)grid & 15)) & 15);
    if (head > total) head = total;
    const int groups = (total - head) / 16;
    const int work = groups + 32;                   // the scalar ends: at most 15 + 15 bytes
    int blocks = (work + PANEL_THREADS - 1) / PANEL_THREADS;
    if (blocks > PANEL_MAX_BLOCKS) blocks = PANEL_MAX_BLOCKS;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 gr(blocks), blk(PANEL_THREADS);
    if (kind == KIND_IMAGE) hipLaunchKernelGGL(panel_grid_kernel<KIND_IMAGE>, gr, blk, 0, st, src, palette, range, grid, g, scale, shift, total, head, groups);
    else if (kind == KIND_COLOUR) hipLaunchKernelGGL(panel_grid_kernel<KIND_COLOUR>, gr, blk, 0, st, src, palette, range, grid, g, scale, shift, total, head, groups);
    else hipLaunchKernelGGL(panel_grid_kernel<KIND_GREY>, gr, blk, 0, st, src, palette, range, grid, g, scale, shift, total, head, groups);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}
