// Structural similarity (SSIM) of two images fused with their L1 distance (include/sscg.h: sscg_ssim_workspace, sscg_l1_ssim_fwd /
// _bwd).  Opt-in: without `--ssim_weight` nothing here is launched.  The reference has no such term.
//
// a (the prediction) and b (the data) are fp32 [N][H][W][C], C <= 4.  The window is k x k (k odd, 3..11), separable, its 1-D weights
// g[i] = exp(-(i - (k-1)/2)^2 / (2 sigma^2)) normalised to sum 1 in fp64 on the host and rounded to fp32 once; they reach the kernels by
// value.  The map is "valid": H' = H - k + 1 by W' = W - k + 1 positions p per (sample, channel), no padding.
//
//   forward   ssim_fwd_kernel: one workgroup per (sample, tile of SSIM_T x SSIM_T map positions), all C channels.  The tile of a and b
//             with its k-1 halo, (T+k-1)^2 pixels, is staged in LDS with a per-channel pivot subtracted (the mean of a and b over the
//             staged pixels: the variances and the covariance do not change under a common shift, and E[a^2] - mu_a^2 no longer
//             cancels on a flat region - the backgrounds of the images are constant; a pivot far from the local mean, such as one
//             pixel's value, would make it cancel MORE on noise); a row pass leaves the five moments' row sums in LDS, a column
//             pass finishes them, S follows in registers.  The block adds S of its positions and |a - b| of the input pixels it OWNS (its
//             T x T corner of the staged region; the last tile of a row / column of tiles also owns the k-1 pixels beyond: every input
//             pixel is counted once) in fp64 into one record each.  With `coef` it stores P1, P2, P3 of every position.
//             ssim_finish_kernel: one block, the records in a fixed order -> per_sample, ssim_loss, l1.
//   backward  ssim_bwd_kernel: one workgroup per (sample, tile of T x T pixels q of da).  The three coefficient maps over the
//             (T+k-1)^2 positions whose windows reach the tile are staged in LDS, zero outside the map; the adjoint of the valid filter
//             is the full correlation: a row pass and a column pass over the staged tile; then
//                 da(q) = -(g_ssim w_ssim / M) [ (G^T P1)(q) + 2 a(q) (G^T P2)(q) + b(q) (G^T P3)(q) ] + g_l1 w_l1 sign(a - b) / (NCHW).
//             Without g_ssim the launch is l1_only_kernel: sscg_l1_bwd's per-element expression, nothing added to it.
// LDS words are addressed by (row, x * C + c): consecutive lanes take consecutive words in both passes (the row pass steps by C words
// per tap, the column pass by a whole row of T * C words), so neither pass has a bank conflict beyond the one row change inside a wave.
// Every loop has a bound known at launch; no float atomics; sums go through fp64 records added in a fixed order.
#include <math.h>

#include "common.h"
#include "sscg_internal.h"

namespace {

constexpr int SSIM_T = 16;           // tile side: map positions (forward), pixels of da (backward)
constexpr int SSIM_KMAX = 11;
constexpr int SSIM_CMAX = 4;

struct SsimWin { float g[SSIM_KMAX]; };

struct SsimGeom {
    int N, H, W, C, k;
    int Ho, Wo;      // the map: H - k + 1, W - k + 1
    int tx, ty;      // tiles per row / column of tiles
    float c1, c2;
};

// LDS floats: the staged tile(s) [planes][SR][SR * C] + the row pass's output [mids][SR][T * C], SR = T + k - 1
static inline size_t ssim_lds_bytes(int C, int k, int planes, int mids) {
    const size_t SR = SSIM_T + k - 1;
    return (planes * SR * SR * C + mids * SR * SSIM_T * C) * sizeof(float);
}

__device__ __forceinline__ float l1_sign(float d, float g) { return d > 0.f ? g : (d < 0.f ? -g : 0.f); }

template <int CT, int KT>
__global__ __launch_bounds__(256) void ssim_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, SsimGeom g, SsimWin win,
                                                       double* __restrict__ rec_s, double* __restrict__ rec_l1, float* __restrict__ coef) {
    extern __shared__ float lds[];
    __shared__ double red[2][4];
    __shared__ float spiv[SSIM_CMAX];
    __shared__ float pred[4][SSIM_CMAX];
    constexpr int C = CT, T = SSIM_T, MW = T * C;
    const int k = KT ? KT : g.k;
    const int SR = T + k - 1, SW = SR * C;
    float* sa = lds;
    float* sb = sa + SR * SW;
    float* mid = sb + SR * SW;                       // [5][SR][MW]
    const int tid = threadIdx.x;
    int bid = blockIdx.x;
    const int bx = bid % g.tx;
    bid /= g.tx;
    const int by = bid % g.ty, n = bid / g.ty;
    const int y0 = by * T, x0 = bx * T;
    const size_t origin = (((size_t)n * g.H + y0) * g.W + x0) * C;
    const int rows = min(SR, g.H - y0), cols = min(SW, (g.W - x0) * C);          // what of the staged tile lies inside the image
    const int own_r = by == g.ty - 1 ? g.H - y0 : T;                             // <= rows
    const int own_c = (bx == g.tx - 1 ? g.W - x0 : T) * C;                       // <= cols
    const int wave = tid >> 6, lane = tid & 63;
    double l1 = 0.0;
    float csum[C];                                                               // a + b over the staged pixels, per channel
#pragma unroll
    for (int c = 0; c < C; ++c) csum[c] = 0.f;
    for (int t = tid; t < SR * SW; t += 256) {
        const int r = t / SW, j = t - r * SW;
        float fa = 0.f, fb = 0.f;
        if (r < rows && j < cols) {
            const size_t o = origin + (size_t)r * g.W * C + j;
            fa = a[o];
            fb = b[o];
            if (rec_l1 && r < own_r && j < own_c) l1 += (double)fabsf(fa - fb);
        }
        const int ch = t % C;                                                    // SW is a multiple of C
#pragma unroll
        for (int c = 0; c < C; ++c) csum[c] += ch == c ? fa + fb : 0.f;
        sa[t] = fa;
        sb[t] = fb;
    }
    // the pivot: the mean of a and b over the tile, per channel.  Any value is a valid pivot (the moments are shifted back exactly where
    // they are used); one near the local mean keeps the shifted moments small.  Every thread reads the same value from LDS.
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float s = wave_sum(csum[c]);
        if (lane == 0) pred[wave][c] = s;
    }
    __syncthreads();
    if (tid < C) spiv[tid] = ((pred[0][tid] + pred[1][tid]) + (pred[2][tid] + pred[3][tid])) / (2.f * (float)(rows * (cols / C)));
    __syncthreads();
    for (int t = tid; t < SR * SW; t += 256) {
        const int r = t / SW, j = t - r * SW;
        if (r < rows && j < cols) {
            const float piv = spiv[t % C];
            sa[t] -= piv;
            sb[t] -= piv;
        }
    }
    __syncthreads();
    const int msz = SR * MW;
    for (int t = tid; t < msz; t += 256) {
        const int r = t / MW, j = t - r * MW;
        const float* pa = sa + r * SW + j;
        const float* pb = sb + r * SW + j;
        float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
        for (int i = 0; i < (KT ? KT : SSIM_KMAX); ++i)
            if (KT || i < k) {
                const float x = pa[i * C], y = pb[i * C];
                const float wx = win.g[i] * x, wy = win.g[i] * y;
                m0 += wx;
                m1 += wy;
                m2 = fmaf(wx, x, m2);
                m3 = fmaf(wy, y, m3);
                m4 = fmaf(wx, y, m4);
            }
        mid[t] = m0;
        mid[msz + t] = m1;
        mid[2 * msz + t] = m2;
        mid[3 * msz + t] = m3;
        mid[4 * msz + t] = m4;
    }
    __syncthreads();
    const int oh = min(T, g.Ho - y0), ow = min(T, g.Wo - x0) * C;                // the tile's positions inside the map
    const size_t M = (size_t)g.N * g.Ho * g.Wo * C;
    double ssum = 0.0;
    for (int t = tid; t < T * MW; t += 256) {
        const int y = t / MW, j = t - y * MW;
        if (y >= oh || j >= ow) continue;
        float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < (KT ? KT : SSIM_KMAX); ++i)
            if (KT || i < k) {
#pragma unroll
                for (int q = 0; q < 5; ++q) m[q] = fmaf(win.g[i], mid[q * msz + t + i * MW], m[q]);
            }
        const float piv = spiv[j % C];
        const float mua = m[0] + piv, mub = m[1] + piv;
        const float va = m[2] - m[0] * m[0], vb = m[3] - m[1] * m[1], cov = m[4] - m[0] * m[1];
        const float A1 = 2.f * mua * mub + g.c1, A2 = 2.f * cov + g.c2;
        const float B1 = mua * mua + mub * mub + g.c1, B2 = va + vb + g.c2;
        const float S = (A1 * A2) / (B1 * B2);
        ssum += (double)S;
        if (coef) {
            const float inv = 1.f / (B1 * B2);
            const size_t o = (((size_t)n * g.Ho + y0 + y) * g.Wo + x0) * C + j;
            coef[o] = 2.f * mub * (A2 - A1) * inv - 2.f * mua * S * (1.f / B1 - 1.f / B2);
            coef[M + o] = -S / B2;
            coef[2 * M + o] = 2.f * A1 * inv;
        }
    }
    const double s = wave_sum(ssum), l = wave_sum(l1);
    if (lane == 0) {
        red[0][wave] = s;
        red[1][wave] = l;
    }
    __syncthreads();
    if (tid == 0) {
        rec_s[blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        if (rec_l1) rec_l1[blockIdx.x] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

// One block, a fixed order throughout.  S: wave w takes the samples w, w + 4, ... - lane l adds the sample's records l, l + 64, ...,
// the wave's butterfly gives the sample's sum (per_sample), lane 0 adds its samples' sums in index order; the four waves' totals are
// added in order.  |a - b|: thread t adds the records t, t + 256, ... of the whole call, then the waves and the four totals.
__global__ __launch_bounds__(256) void ssim_finish_kernel(const double* __restrict__ rec_s, const double* __restrict__ rec_l1, int N, int bps,
                                                          double inv_map, double inv_l1, float* __restrict__ l1, float* __restrict__ ssim_loss,
                                                          float* __restrict__ per_sample) {
    __shared__ double tot[2][4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    double ws = 0.0;
    for (int n = wave; n < N; n += 4) {
        double s = 0.0;
        for (int i = lane; i < bps; i += 64) s += rec_s[(size_t)n * bps + i];
        s = wave_sum(s);
        ws += s;
        if (per_sample && lane == 0) per_sample[n] = (float)(s * inv_map);
    }
    double wl = 0.0;
    if (l1) {
        const size_t nrec = (size_t)N * bps;
        for (size_t i = tid; i < nrec; i += 256) wl += rec_l1[i];
        wl = wave_sum(wl);
    }
    if (lane == 0) {
        tot[0][wave] = ws;
        tot[1][wave] = wl;
    }
    __syncthreads();
    if (tid == 0) {
        *ssim_loss = (float)(1.0 - ((tot[0][0] + tot[0][1]) + (tot[0][2] + tot[0][3])) * inv_map / (double)N);
        if (l1) *l1 = (float)(((tot[1][0] + tot[1][1]) + (tot[1][2] + tot[1][3])) * inv_l1);
    }
}

template <int CT, int KT>
__global__ __launch_bounds__(256) void ssim_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ coef,
                                                       SsimGeom g, SsimWin win, const float* __restrict__ g_l1, float w_l1,
                                                       const float* __restrict__ g_ssim, float w_ssim, float* __restrict__ da) {
    extern __shared__ float lds[];
    constexpr int C = CT, T = SSIM_T, MW = T * C;
    const int k = KT ? KT : g.k;
    const int SR = T + k - 1, SW = SR * C;
    const int ssz = SR * SW, msz = SR * MW;
    float* sp = lds;                                 // [3][SR][SW]
    float* mid = lds + 3 * ssz;                      // [3][SR][MW]
    const int tid = threadIdx.x;
    int bid = blockIdx.x;
    const int bx = bid % g.tx;
    bid /= g.tx;
    const int by = bid % g.ty, n = bid / g.ty;
    const int qy0 = by * T, qx0 = bx * T;
    const size_t M = (size_t)g.N * g.Ho * g.Wo * C;
    const int py0 = qy0 - (k - 1), pc0 = (qx0 - (k - 1)) * C, wc = g.Wo * C;
    for (int t = tid; t < ssz; t += 256) {
        const int r = t / SW, j = t - r * SW;
        const int py = py0 + r, pc = pc0 + j;
        float v0 = 0.f, v1 = 0.f, v2 = 0.f;
        if (py >= 0 && py < g.Ho && pc >= 0 && pc < wc) {
            const size_t o = ((size_t)n * g.Ho + py) * wc + pc;
            v0 = coef[o];
            v1 = coef[M + o];
            v2 = coef[2 * M + o];
        }
        sp[t] = v0;
        sp[ssz + t] = v1;
        sp[2 * ssz + t] = v2;
    }
    __syncthreads();
    // pixel q of the tile (local y, x) collects positions q - (i, i'): staged rows y + k-1 - i, staged columns x + k-1 - i'
    for (int t = tid; t < msz; t += 256) {
        const int r = t / MW, j = t - r * MW;
        const float* p = sp + r * SW + j + (k - 1) * C;
        float m0 = 0.f, m1 = 0.f, m2 = 0.f;
#pragma unroll
        for (int i = 0; i < (KT ? KT : SSIM_KMAX); ++i)
            if (KT || i < k) {
                m0 = fmaf(win.g[i], p[-i * C], m0);
                m1 = fmaf(win.g[i], p[ssz - i * C], m1);
                m2 = fmaf(win.g[i], p[2 * ssz - i * C], m2);
            }
        mid[t] = m0;
        mid[msz + t] = m1;
        mid[2 * msz + t] = m2;
    }
    __syncthreads();
    const float gs = *g_ssim * w_ssim;
    const float gl = g_l1 ? *g_l1 * w_l1 : 0.f;
    const int qh = min(T, g.H - qy0), qw = min(T, g.W - qx0) * C;
    for (int t = tid; t < T * MW; t += 256) {
        const int y = t / MW, j = t - y * MW;
        if (y >= qh || j >= qw) continue;
        const float* p = mid + t + (k - 1) * MW;
        float t0 = 0.f, t1 = 0.f, t2 = 0.f;
#pragma unroll
        for (int i = 0; i < (KT ? KT : SSIM_KMAX); ++i)
            if (KT || i < k) {
                t0 = fmaf(win.g[i], p[-i * MW], t0);
                t1 = fmaf(win.g[i], p[msz - i * MW], t1);
                t2 = fmaf(win.g[i], p[2 * msz - i * MW], t2);
            }
        const size_t o = (((size_t)n * g.H + qy0 + y) * g.W + qx0) * C + j;
        const float fa = a[o], fb = b[o];
        float v = -gs * (t0 + 2.f * fa * t1 + fb * t2);
        if (g_l1) v += l1_sign(fa - fb, gl);
        da[o] = v;
    }
}

// sscg_l1_bwd's kernel (loss_optim.hip), expression for expression: the bits of that entry
__global__ void l1_only_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n, const float* __restrict__ gscale, float w,
                               float* __restrict__ da) {
    const float g = *gscale * w;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float d = a[i] - b[i];
        da[i] = l1_sign(d, g);
    }
}

static void make_window(int k, float sigma, SsimWin* w) {
    double t[SSIM_KMAX], s = 0.0;
    const double s2 = 2.0 * (double)sigma * (double)sigma;
    for (int i = 0; i < k; ++i) {
        const double d = (double)i - (double)(k - 1) / 2.0;
        t[i] = exp(-(d * d) / s2);
        s += t[i];
    }
    for (int i = 0; i < SSIM_KMAX; ++i) w->g[i] = i < k ? (float)(t[i] / s) : 0.f;
}

// the refusals every entry shares, in the order BAD_ARG, UNSUPPORTED
static int ssim_sizes(int N, int H, int W, int C, int win) {
    if (N <= 0 || H <= 0 || W <= 0 || win < 3 || win > SSIM_KMAX || !(win & 1) || H < win || W < win) return SSCG_ERR_BAD_ARG;
    if (C < 1 || C > SSIM_CMAX) return SSCG_ERR_UNSUPPORTED;
    const uint64_t rows = (uint64_t)N * (uint64_t)H;                   // < 2^62: the next product cannot wrap once this one is small
    if (rows >= ((uint64_t)1 << 31) || rows * (uint64_t)W * (uint64_t)C >= ((uint64_t)1 << 31)) return SSCG_ERR_UNSUPPORTED;
    return SSCG_OK;
}

static SsimGeom make_geom(int N, int H, int W, int C, int win, bool over_map) {
    SsimGeom g;
    g.N = N; g.H = H; g.W = W; g.C = C; g.k = win;
    g.Ho = H - win + 1;
    g.Wo = W - win + 1;
    g.ty = ((over_map ? g.Ho : H) + SSIM_T - 1) / SSIM_T;
    g.tx = ((over_map ? g.Wo : W) + SSIM_T - 1) / SSIM_T;
    g.c1 = g.c2 = 0.f;
    return g;
}

template <int KT>
void launch_fwd(const SsimGeom& g, const SsimWin& w, hipStream_t st, const float* a, const float* b, double* rec_s, double* rec_l1,
                float* coef) {
    const dim3 grid((unsigned)g.N * g.ty * g.tx), blk(256);
    const size_t smem = ssim_lds_bytes(g.C, g.k, 2, 5);
    switch (g.C) {
        case 1: hipLaunchKernelGGL((ssim_fwd_kernel<1, KT>), grid, blk, smem, st, a, b, g, w, rec_s, rec_l1, coef); break;
        case 2: hipLaunchKernelGGL((ssim_fwd_kernel<2, KT>), grid, blk, smem, st, a, b, g, w, rec_s, rec_l1, coef); break;
        case 3: hipLaunchKernelGGL((ssim_fwd_kernel<3, KT>), grid, blk, smem, st, a, b, g, w, rec_s, rec_l1, coef); break;
        default: hipLaunchKernelGGL((ssim_fwd_kernel<4, KT>), grid, blk, smem, st, a, b, g, w, rec_s, rec_l1, coef); break;
    }
}

template <int KT>
void launch_bwd(const SsimGeom& g, const SsimWin& w, hipStream_t st, const float* a, const float* b, const float* coef, const float* g_l1,
                float w_l1, const float* g_ssim, float w_ssim, float* da) {
    const dim3 grid((unsigned)g.N * g.ty * g.tx), blk(256);
    const size_t smem = ssim_lds_bytes(g.C, g.k, 3, 3);
    switch (g.C) {
        case 1: hipLaunchKernelGGL((ssim_bwd_kernel<1, KT>), grid, blk, smem, st, a, b, coef, g, w, g_l1, w_l1, g_ssim, w_ssim, da); break;
        case 2: hipLaunchKernelGGL((ssim_bwd_kernel<2, KT>), grid, blk, smem, st, a, b, coef, g, w, g_l1, w_l1, g_ssim, w_ssim, da); break;
        case 3: hipLaunchKernelGGL((ssim_bwd_kernel<3, KT>), grid, blk, smem, st, a, b, coef, g, w, g_l1, w_l1, g_ssim, w_ssim, da); break;
        default: hipLaunchKernelGGL((ssim_bwd_kernel<4, KT>), grid, blk, smem, st, a, b, coef, g, w, g_l1, w_l1, g_ssim, w_ssim, da); break;
    }
}

}  // namespace

extern "C" size_t sscg_ssim_workspace(int N, int H, int W, int C, int win) {
    if (ssim_sizes(N, H, W, C, win) != SSCG_OK) return 0;
    const SsimGeom g = make_geom(N, H, W, C, win, true);
    return (size_t)2 * g.N * g.ty * g.tx * sizeof(double);             // per forward block one record of S and one of |a - b|
}

extern "C" int sscg_l1_ssim_fwd(const float* a, const float* b, int N, int H, int W, int C, int win, float sigma, float c1, float c2,
                                float* l1, float* ssim_loss, float* per_sample, float* coef, void* ws, size_t ws_bytes, void* stream) {
    if (!a || !b || !ssim_loss || !(sigma > 0.f) || !(c1 >= 0.f) || !(c2 >= 0.f)) return SSCG_ERR_BAD_ARG;
    const int rc = ssim_sizes(N, H, W, C, win);
    if (rc != SSCG_OK) return rc;
    if (!ws || ((uintptr_t)ws & 7) || ws_bytes < sscg_ssim_workspace(N, H, W, C, win)) return SSCG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    SsimGeom g = make_geom(N, H, W, C, win, true);
    g.c1 = c1;
    g.c2 = c2;
    SsimWin w;
    make_window(win, sigma, &w);
    const int bps = g.ty * g.tx;
    double* rec_s = reinterpret_cast<double*>(ws);
    double* rec_l1 = rec_s + (size_t)N * bps;
    if (win == SSIM_KMAX) launch_fwd<SSIM_KMAX>(g, w, st, a, b, rec_s, l1 ? rec_l1 : nullptr, coef);
    else launch_fwd<0>(g, w, st, a, b, rec_s, l1 ? rec_l1 : nullptr, coef);
    hipLaunchKernelGGL(ssim_finish_kernel, dim3(1), dim3(256), 0, st, rec_s, rec_l1, N, bps, 1.0 / ((double)g.Ho * g.Wo * C),
                       1.0 / ((double)N * H * W * C), l1, ssim_loss, per_sample);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_l1_ssim_bwd(const float* a, const float* b, const float* coef, int N, int H, int W, int C, int win, float sigma,
                                const float* g_l1, float w_l1, const float* g_ssim, float w_ssim, float* da, void* stream) {
    if (!a || !b || !da || (!g_l1 && !g_ssim) || (g_ssim && !coef) || !(sigma > 0.f)) return SSCG_ERR_BAD_ARG;
    const int rc = ssim_sizes(N, H, W, C, win);
    if (rc != SSCG_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)N * H * W * C;
    if (!g_ssim) {
        hipLaunchKernelGGL(l1_only_kernel, dim3(ew_blocks(n)), dim3(256), 0, st, a, b, (size_t)n, g_l1, w_l1 / (float)n, da);
        SSCG_LAUNCH_CHECK();
        return SSCG_OK;
    }
    const SsimGeom g = make_geom(N, H, W, C, win, false);
    SsimWin w;
    make_window(win, sigma, &w);
    const float ws_m = (float)((double)w_ssim / ((double)N * g.Ho * g.Wo * C));
    if (win == SSIM_KMAX) launch_bwd<SSIM_KMAX>(g, w, st, a, b, coef, g_l1, w_l1 / (float)n, g_ssim, ws_m, da);
    else launch_bwd<0>(g, w, st, a, b, coef, g_l1, w_l1 / (float)n, g_ssim, ws_m, da);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}
