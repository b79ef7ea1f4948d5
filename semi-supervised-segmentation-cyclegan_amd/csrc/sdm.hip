// Boundary loss on signed distance maps (include/sscg.h: sscg_sdm, sscg_boundary_loss_fwd / _bwd; the head's backward with the
// boundary term, sscg_upsample_head_bwd_b, is in head_bwd.hip).  Opt-in: without `--boundary_loss` nothing here is launched.
//
// sdm[n][y][x][c] (int32, class innermost) = +d2 at a non-member of class c, -d2 at a member, d2 = the exact squared Euclidean distance
// to the nearest pixel of the OPPOSITE membership in the same sample; a plane whose class has no member in the sample, or nothing but
// members, is zero.  The dense form of surface.hip's transform - every pixel of every class, both signs:
//   1. sdm_zero_kernel / sdm_count_kernel  members per (sample, class): LDS bins, integer atomics (order-free);
//   2. per chunk of SDM_CH classes:
//      sdm_column_kernel  one thread per (sample, group of SDM_CG classes, column), lanes on consecutive columns, walks its column down
//                         and up: per pixel the vertical distance d to the nearest pixel of the opposite membership IN ITS COLUMN, packed
//                         with the pixel's own membership m into a uint16 e = m << 15 | d.  d >= 1 where it exists (the pixel itself
//                         is of its own membership), so d == 0 encodes "the column holds none", and d <= H - 1 < 2^15;
//      sdm_row_kernel     one workgroup per (sample, row); per live class of the chunk the row's e staged in LDS, and per pixel the
//                         exact minimum over x' of dx^2 + v(x')^2, v = 0 where column x' has the opposite membership on this row,
//                         else its d (skipped when it has none), by a walk outwards from x that stops when dx^2 >= best.  A live
//                         class has members and non-members in the sample, so every pixel finds a finite minimum.  The planes of the
//                         other classes are written as zeros.
// The loss, with p = softmax_C(resize(z)) and phi = sscg_level_set(sdm) (head_common.h):
//     loss = k * sum over counted pixels, sum_c w_c p_c phi_c          k = 1 / (V * sum_c w_c), V = the counted pixels (V == 0: k = 0)
//   3. bl_stats_kernel    one thread per OUTPUT pixel, no block straddles a sample; per block one fp64 record [C + 1] = the sums of
//                         p_c phi_c over its counted pixels and their number - products and sums in fp64 from the fp32 factors;
//      bl_reduce_kernel   one block per (sample, column of the record): the sample's records in a fixed tree;
//      bl_finish_kernel   one block: the samples in index order -> sums [N][C], V, k, the loss.
//   4. the backward       d loss / d p_c = k w_c phi_c at a counted pixel: flat (bl_bwd_kernel: one thread per pixel) or as one more
//                         term of q_c in the head's one backward kernel (head_bwd.hip).
// Every loop has a bound known at launch (grid-stride loops included), no workgroup waits on another, nothing spins on a value;
// integers go through atomics, fp64 through records in a fixed order: the result does not depend on scheduling.
#include "common.h"
#include "head_common.h"
#include "head_geom.h"
#include "sscg_internal.h"

namespace {

constexpr int SDM_CH = 16;                       // classes per chunk of the column / row passes: 32 B of column distances per pixel
constexpr int SDM_CG = 2;                        // classes one column thread carries: more waves for a pass that is a chain of rows
constexpr int SDM_STAGE_W = 24576;               // widest row staged in LDS (48 KB); wider rows are read from the workspace
constexpr unsigned SDM_NONE = 0xFFFFu;           // inside the column walk: no pixel of that membership seen yet
constexpr unsigned SDM_INF = 0x7FFFFFFFu;
constexpr int SDM_GRID_CAP = 1 << 16;            // blocks of a launch; work items beyond it are taken grid-stride
constexpr size_t SDM_ALIGN = 256;
constexpr int BL_BLOCKS = 256;                   // statistics blocks per sample, grid-stride beyond (the reduce's tree holds 256 records)

struct SdmGeom {
    int N, H, W, C;
    int hw;               // H * W
    int cbps;             // blocks per sample of the count pass
    int chs;              // classes the column distances have room for: min(C, SDM_CH)
};

static inline size_t sdm_up(size_t b) { return (b + SDM_ALIGN - 1) / SDM_ALIGN * SDM_ALIGN; }
static inline dim3 sdm_grid(long long items) { return dim3((unsigned)(items < SDM_GRID_CAP ? items : SDM_GRID_CAP)); }

static inline size_t sdm_carve(int N, int H, int W, int C, void* base, uint32_t** cnt, uint16_t** gd) {
    const size_t pix = (size_t)N * H * W;
    const size_t ch = C < SDM_CH ? C : SDM_CH;
    char* b = reinterpret_cast<char*>(base);
    const size_t off_g = sdm_up((size_t)N * C * sizeof(uint32_t));
    if (cnt) *cnt = reinterpret_cast<uint32_t*>(b);
    if (gd) *gd = reinterpret_cast<uint16_t*>(b + off_g);
    return off_g + sdm_up(ch * pix * sizeof(uint16_t));
}

__global__ __launch_bounds__(256) void sdm_zero_kernel(uint32_t* __restrict__ a, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) a[i] = 0u;
}

// Work item = (sample n, block blk of cbps): pixels blk * 256 + tid, + cbps * 256, ... of the sample.
__global__ __launch_bounds__(256) void sdm_count_kernel(const int64_t* __restrict__ lab, uint32_t* __restrict__ cnt, SdmGeom g) {
    __shared__ unsigned int bins[SSCG_MAXC];
    const int C = g.C;
    const long long items = (long long)g.N * g.cbps;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int n = (int)(it / g.cbps), blk = (int)(it - (long long)n * g.cbps);
        sscg_bins_clear(bins, C);
        const int64_t* ln = lab + (size_t)n * g.hw;
        for (long long o = (long long)blk * 256 + threadIdx.x; o < g.hw; o += (long long)g.cbps * 256) {
            const int64_t l = ln[o];
            if (l >= 0 && l < C) atomicAdd(&bins[(int)l], 1u);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < C; i += 256)
            if (bins[i]) atomicAdd(&cnt[(size_t)n * C + i], bins[i]);       // a sample holds fewer than 2^31 pixels
        __syncthreads();
    }
}

// Work item = (sample n, class group cg of the chunk, block of 64 columns).  gd[cc][n][y][x] = m << 15 | d (the file comment).
__global__ __launch_bounds__(64) void sdm_column_kernel(const int64_t* __restrict__ lab, uint16_t* __restrict__ gd, int c0, int nch,
                                                        SdmGeom g) {
    const int H = g.H, W = g.W, N = g.N;
    const int xb = (W + 63) / 64, ngr = (nch + SDM_CG - 1) / SDM_CG;
    const long long items = (long long)N * ngr * xb;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int bx = (int)(it % xb);
        const long long r = it / xb;
        const int cg = (int)(r % ngr), n = (int)(r / ngr);
        const int x = bx * 64 + (int)threadIdx.x;
        if (x >= W) continue;
        const int64_t* ln = lab + (size_t)n * g.hw + x;
        const int cc0 = cg * SDM_CG;
        uint16_t* out = gd + ((size_t)cc0 * N + n) * g.hw + x;             // class cc0 + j: + j * N * hw
        const size_t cstride = (size_t)N * g.hw;
        unsigned dm[SDM_CG], dn[SDM_CG];                                   // distance to the last member / non-member seen
#pragma unroll
        for (int j = 0; j < SDM_CG; ++j) { dm[j] = SDM_NONE; dn[j] = SDM_NONE; }
#pragma unroll 8
        for (int y = 0; y < H; ++y) {                                      // (unrolled: eight rows' loads in flight, not one)
            const int64_t l = ln[(size_t)y * W];
#pragma unroll
            for (int j = 0; j < SDM_CG; ++j)
                if (cc0 + j < nch) {
                    const bool m = l == (int64_t)(c0 + cc0 + j);
                    dm[j] = m ? 0u : (dm[j] == SDM_NONE ? SDM_NONE : dm[j] + 1u);      // <= H - 1 < 2^15
                    dn[j] = m ? (dn[j] == SDM_NONE ? SDM_NONE : dn[j] + 1u) : 0u;
                    out[j * cstride + (size_t)y * W] = (uint16_t)(m ? dn[j] : dm[j]);
                }
        }
#pragma unroll
        for (int j = 0; j < SDM_CG; ++j) { dm[j] = SDM_NONE; dn[j] = SDM_NONE; }
#pragma unroll 8
        for (int y = H - 1; y >= 0; --y) {
            const int64_t l = ln[(size_t)y * W];
#pragma unroll
            for (int j = 0; j < SDM_CG; ++j)
                if (cc0 + j < nch) {
                    const bool m = l == (int64_t)(c0 + cc0 + j);
                    dm[j] = m ? 0u : (dm[j] == SDM_NONE ? SDM_NONE : dm[j] + 1u);
                    dn[j] = m ? (dn[j] == SDM_NONE ? SDM_NONE : dn[j] + 1u) : 0u;
                    const unsigned up = m ? dn[j] : dm[j], down = out[j * cstride + (size_t)y * W];
                    const unsigned d = up < down ? up : down;
                    out[j * cstride + (size_t)y * W] = (uint16_t)((m ? 0x8000u : 0u) | (d == SDM_NONE ? 0u : d));
                }
        }
    }
}

// Work item = (sample n, row y).  STAGED: the row's packed column distances of one class sit in LDS (W <= SDM_STAGE_W); else they are
// read where the column pass left them.
template <bool STAGED>
__global__ __launch_bounds__(256) void sdm_row_kernel(const uint16_t* __restrict__ gd, const uint32_t* __restrict__ cnt,
                                                      int32_t* __restrict__ sdm, int c0, int nch, SdmGeom g) {
    extern __shared__ unsigned short grow[];             // [W] (STAGED)
    const int H = g.H, W = g.W, N = g.N, C = g.C;
    const int tid = threadIdx.x;
    const long long items = (long long)N * H;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int y = (int)(it % H), n = (int)(it / H);
        const size_t row = (size_t)n * g.hw + (size_t)y * W;
        int32_t* orow = sdm + row * C;
        for (int cc = 0; cc < nch; ++cc) {
            const int c = c0 + cc;
            const uint32_t members = cnt[(size_t)n * C + c];
            if (members == 0u || members == (uint32_t)g.hw) {                   // block-uniform: no contour in this sample
                for (int x = tid; x < W; x += 256) orow[(size_t)x * C + c] = 0;
                continue;
            }
            const uint16_t* gr = gd + ((size_t)cc * N + n) * g.hw + (size_t)y * W;
            if (STAGED) {
                for (int x = tid; x < W; x += 256) grow[x] = gr[x];
                __syncthreads();
            }
            const auto at = [&](int x) -> unsigned { return STAGED ? (unsigned)grow[x] : (unsigned)gr[x]; };
            for (int x = tid; x < W; x += 256) {
                const unsigned e0 = at(x);
                const unsigned m = e0 >> 15, d0 = e0 & 0x7FFFu;
                unsigned best = d0 ? d0 * d0 : SDM_INF;
                for (int dx = 1; dx < W; ++dx) {                                // exact: no column farther than sqrt(best) can win
                    const unsigned dx2 = (unsigned)dx * (unsigned)dx;
                    if (dx2 >= best) break;
                    if (x - dx >= 0) {
                        const unsigned e = at(x - dx), d = e & 0x7FFFu;
                        const unsigned k = (e >> 15) != m ? dx2 : (d ? dx2 + d * d : SDM_INF);      // < 2^31: dx, d < 2^15
                        best = k < best ? k : best;
                    }
                    if (x + dx < W) {
                        const unsigned e = at(x + dx), d = e & 0x7FFFu;
                        const unsigned k = (e >> 15) != m ? dx2 : (d ? dx2 + d * d : SDM_INF);
                        best = k < best ? k : best;
                    }
                }
                // finite: the class is live in the sample, so some column of this row reaches the opposite membership
                orow[(size_t)x * C + c] = m ? -(int32_t)best : (int32_t)best;
            }
            if (STAGED) __syncthreads();                                        // grow is restaged for the next class
        }
    }
}

// ---- the loss

struct BlGeom {
    sscg_resize_geom r;
    int npix;      // OH * OW: output pixels of a sample
    int bps;       // blocks (= records) per sample
};

// One thread per output pixel of ONE sample (block b serves sample b / bps), as dice_stats_kernel: the pixel's C logits in registers
// (RESIZE: the pinned arithmetic of head_common.h; !RESIZE: the row itself), sscg_softmax_exp, p = v * inv in fp32 (the bits
// sscg_softmax_fwd stores), phi from the pixel's C contiguous sdm values, the product and every sum above it in fp64: the thread's
// pixels, the wave (butterfly), the four waves in order into the block's record [C + 1] (the last entry: its counted pixels).
template <int CT, bool RESIZE>
__global__ __launch_bounds__(256) void bl_stats_kernel(const float* __restrict__ x, const int64_t* __restrict__ lab,
                                                       const int32_t* __restrict__ sdm, double* __restrict__ part, BlGeom g) {
    __shared__ double red[4][SSCG_MAXC + 1];
    const int C = CT ? CT : g.r.C;
    const int n = blockIdx.x / g.bps, blk = blockIdx.x - n * g.bps;
    const float* xn = x + (size_t)n * g.r.H * g.r.W * C;
    const int64_t* ln = lab + (size_t)n * g.npix;
    const int32_t* sn = sdm + (size_t)n * g.npix * C;
    double S[CT ? CT : SSCG_MAXC];
#pragma unroll
    for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c) S[c] = 0.0;
    int cnt = 0;
    for (long base = (long)blk * 256; base < g.npix; base += (long)g.bps * 256) {
        const long o_raw = base + threadIdx.x;
        if (o_raw >= g.npix) break;
        const int o = (int)o_raw;
        const int64_t l64 = ln[o];
        if (l64 < 0 || l64 >= C) continue;
        ++cnt;
        float v[CT ? CT : SSCG_MAXC];
        const int oy = RESIZE ? fd_div(o, g.r.dow) : 0;       // the pixel within its sample: xn is the sample's map
        sscg_pixel_logits<CT, !RESIZE>(xn, 0, oy, o - oy * g.r.OW, g.r.H, g.r.W, g.r.sh, g.r.sw, C, v);
        const float inv = sscg_softmax_exp<CT>(v, C);
        const int32_t* sr = sn + (size_t)o * C;
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
            if (CT || c < C) {
                const float p = v[c] * inv;
                S[c] += (double)p * (double)sscg_level_set(sr[c]);
            }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
        if (CT || c < C) {
            const double s = wave_sum(S[c]);
            if (lane == 0) red[wave][c] = s;
        }
    const double sc = wave_sum((double)cnt);
    if (lane == 0) red[wave][C] = sc;
    __syncthreads();
    if ((int)threadIdx.x <= C)
        part[(size_t)blockIdx.x * (C + 1) + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// The records of one (sample, column j of C + 1) -> that sample's sum: thread t holds record t (bps <= 256), then a halving tree.
__global__ __launch_bounds__(256) void bl_reduce_kernel(const double* __restrict__ part, int bps, int C1, double* __restrict__ ssum) {
    __shared__ double sm[256];
    const int n = blockIdx.x / C1, j = blockIdx.x - n * C1;
    sm[threadIdx.x] = (int)threadIdx.x < bps ? part[((size_t)n * bps + threadIdx.x) * C1 + j] : 0.0;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sm[threadIdx.x] += sm[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) ssum[blockIdx.x] = sm[0];
}

// One block for the whole call: thread c adds class c's samples in index order, thread 0 the classes in order.
__global__ __launch_bounds__(64) void bl_finish_kernel(const double* __restrict__ ssum, int N, int C, const float* __restrict__ class_w,
                                                       float* __restrict__ loss, double* __restrict__ sums, int64_t* __restrict__ counted,
                                                       float* __restrict__ coef) {
    __shared__ double tot[SSCG_MAXC];
    const int c = threadIdx.x;
    if (c < C) {
        double t = 0.0;
        for (int n = 0; n < N; ++n) {
            const double s = ssum[(size_t)n * (C + 1) + c];
            if (sums) sums[(size_t)n * C + c] = s;
            t += s;
        }
        tot[c] = (double)(class_w ? class_w[c] : 1.f) * t;
    }
    __syncthreads();
    if (c == 0) {
        double v = 0.0, wsum = 0.0, t = 0.0;
        for (int n = 0; n < N; ++n) v += ssum[(size_t)n * (C + 1) + C];
        for (int k = 0; k < C; ++k) { wsum += (double)(class_w ? class_w[k] : 1.f); t += tot[k]; }
        const double k = (v > 0.0 && wsum > 0.0) ? 1.0 / (v * wsum) : 0.0;     // (sum w == 0 is refused by the host: no NaN here either)
        if (counted) *counted = (int64_t)v;                                    // exact: whole numbers below 2^31
        *coef = (float)k;
        *loss = (float)(k * t);
    }
}

// Flat backward: dx[r][c] = scale * p_c (q_c - sum_k p_k q_k) with q_c = k w_c phi_c; a zero row for a pixel that is not counted.
template <int CT>
__global__ __launch_bounds__(256) void bl_bwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ lab,
                                                     const int32_t* __restrict__ sdm, size_t rows, int Cr, const float* __restrict__ class_w,
                                                     const float* __restrict__ coef, const float* __restrict__ gscale, float w,
                                                     float* __restrict__ dx) {
    const int C = CT ? CT : Cr;
    const float kq = *coef;
    const float scale = (gscale ? *gscale : 1.f) * w;
    for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (size_t)gridDim.x * 256) {
        const int64_t l64 = lab[r];
        float* dr = dx + r * C;
        if (l64 < 0 || l64 >= C) {
#pragma unroll
            for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
                if (CT || c < C) dr[c] = 0.f;
            continue;
        }
        const float* xr = x + r * C;
        const int32_t* sr = sdm + r * C;
        float v[CT ? CT : SSCG_MAXC], q[CT ? CT : SSCG_MAXC];
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
            if (CT || c < C) v[c] = xr[c];
        const float inv = sscg_softmax_exp<CT>(v, C);
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
            if (CT || c < C) {
                v[c] *= inv;
                q[c] = kq * class_weight(class_w, c) * sscg_level_set(sr[c]);
                dot += v[c] * q[c];
            }
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
            if (CT || c < C) dr[c] = scale * (v[c] * (q[c] - dot));
    }
}

int bl_bps(int OH, int OW) {
    const long npix = (long)OH * OW;
    const long b = (npix + 255) / 256;
    return (int)(b > BL_BLOCKS ? BL_BLOCKS : b);
}

template <bool RESIZE>
void launch_bl_stats(const BlGeom& g, int N, hipStream_t st, const float* x, const int64_t* lab, const int32_t* sdm, double* part) {
    const dim3 grid((unsigned)N * g.bps), blk(256);
    sscg_dispatch_classes(g.r.C, [&](auto ct) {
        hipLaunchKernelGGL((bl_stats_kernel<decltype(ct)::value, RESIZE>), grid, blk, 0, st, x, lab, sdm, part, g);
    });
}

static inline bool sdm_args_ok(int N, int H, int W, int C) { return N > 0 && H > 0 && W > 0 && C >= 1 && C <= SSCG_MAXC; }

// pixels are indexed with 32-bit integers, and |sdm| <= (H-1)^2 + (W-1)^2 stays below 2^30
static inline bool sdm_too_large(int N, int H, int W) {
    const uint64_t rows = (uint64_t)N * (uint64_t)H;                   // < 2^62: the second product cannot wrap once this one is small
    if (rows >= ((uint64_t)1 << 31) || rows * (uint64_t)W >= ((uint64_t)1 << 31)) return true;
    const uint64_t dy = (uint64_t)(H - 1), dx = (uint64_t)(W - 1);
    return dy * dy + dx * dx >= ((uint64_t)1 << 30);
}

}  // namespace

extern "C" size_t sscg_sdm_workspace(int N, int H, int W, int C) {
    if (!sdm_args_ok(N, H, W, C) || sdm_too_large(N, H, W)) return 0;
    return sdm_carve(N, H, W, C, nullptr, nullptr, nullptr);
}

extern "C" int sscg_sdm(const int64_t* labels, int N, int H, int W, int C, int32_t* sdm, void* ws, size_t ws_bytes, void* stream) {
    if (!labels || !sdm || !sdm_args_ok(N, H, W, C)) return SSCG_ERR_BAD_ARG;
    if (sdm_too_large(N, H, W)) return SSCG_ERR_UNSUPPORTED;
    uint32_t* cnt;
    uint16_t* gd;
    if (!ws || ws_bytes < sdm_carve(N, H, W, C, ws, &cnt, &gd)) return SSCG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    SdmGeom g;
    g.N = N; g.H = H; g.W = W; g.C = C;
    g.hw = H * W;
    const int cb = (g.hw + 256 * 16 - 1) / (256 * 16);
    g.cbps = cb < 1 ? 1 : (cb > 64 ? 64 : cb);
    g.chs = C < SDM_CH ? C : SDM_CH;
    hipLaunchKernelGGL(sdm_zero_kernel, dim3(ew_blocks((size_t)N * C, 1024)), dim3(256), 0, st, cnt, (size_t)N * C);
    hipLaunchKernelGGL(sdm_count_kernel, sdm_grid((long long)N * g.cbps), dim3(256), 0, st, labels, cnt, g);
    const int xb = (W + 63) / 64;
    const bool staged = W <= SDM_STAGE_W;
    for (int c0 = 0; c0 < C; c0 += SDM_CH) {
        const int nch = C - c0 < SDM_CH ? C - c0 : SDM_CH;
        const int ngr = (nch + SDM_CG - 1) / SDM_CG;
        hipLaunchKernelGGL(sdm_column_kernel, sdm_grid((long long)N * ngr * xb), dim3(64), 0, st, labels, gd, c0, nch, g);
        if (staged)
            hipLaunchKernelGGL(sdm_row_kernel<true>, sdm_grid((long long)N * H), dim3(256), ((size_t)W * sizeof(uint16_t) + 15) / 16 * 16, st,
                               gd, cnt, sdm, c0, nch, g);
        else
            hipLaunchKernelGGL(sdm_row_kernel<false>, sdm_grid((long long)N * H), dim3(256), 0, st, gd, cnt, sdm, c0, nch, g);
    }
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" size_t sscg_boundary_loss_workspace(int N, int OH, int OW, int C) {
    if (!sdm_args_ok(N, OH, OW, C) || sdm_too_large(N, OH, OW)) return 0;
    return (size_t)N * (size_t)(C + 1) * ((size_t)bl_bps(OH, OW) + 1) * sizeof(double);      // the blocks' records + the samples' sums
}

extern "C" int sscg_boundary_loss_fwd(const float* x, const int64_t* labels, const int32_t* sdm, int N, int H, int W, int C, int OH,
                                      int OW, const float* class_w, float* loss, double* sums, int64_t* counted, float* coef, void* ws,
                                      size_t ws_bytes, void* stream) {
    if (!x || !labels || !sdm || !loss || !coef || !sizes_ok(N, H, W, C, OH, OW)) return SSCG_ERR_BAD_ARG;
    if (too_large(N, H, W, OH, OW) || sdm_too_large(N, OH, OW)) return SSCG_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < sscg_boundary_loss_workspace(N, OH, OW, C)) return SSCG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const BlGeom g = {sscg_make_resize_geom(H, W, C, OH, OW), OH * OW, bl_bps(OH, OW)};
    double* part = reinterpret_cast<double*>(ws);
    if (OH == H && OW == W) launch_bl_stats<false>(g, N, st, x, labels, sdm, part);
    else launch_bl_stats<true>(g, N, st, x, labels, sdm, part);
    double* ssum = part + (size_t)N * g.bps * (C + 1);
    hipLaunchKernelGGL(bl_reduce_kernel, dim3((unsigned)N * (C + 1)), dim3(256), 0, st, part, g.bps, C + 1, ssum);
    hipLaunchKernelGGL(bl_finish_kernel, dim3(1), dim3(64), 0, st, ssum, N, C, class_w, loss, sums, counted, coef);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_boundary_loss_bwd(const float* x, const int64_t* labels, const int32_t* sdm, int N, int H, int W, int C,
                                      const float* class_w, const float* coef, const float* g, float w, float* dx, void* stream) {
    if (!x || !labels || !sdm || !coef || !dx || !sdm_args_ok(N, H, W, C)) return SSCG_ERR_BAD_ARG;
    if (sdm_too_large(N, H, W)) return SSCG_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const size_t rows = (size_t)N * H * W;
    const dim3 grid(ew_blocks(rows)), blk(256);
    sscg_dispatch_classes(C, [&](auto ct) {
        hipLaunchKernelGGL(bl_bwd_kernel<decltype(ct)::value>, grid, blk, 0, st, x, labels, sdm, rows, C, class_w, coef, g, w, dx);
    });
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}
