// The geometry of the fused label head (resize -> softmax -> losses from the low-resolution logits), shared by loss_optim.hip (the
// forward, head_kernel), head_bwd.hip (the one backward, head_bwd_kernel) and the entries of dice.hip / ohem.hip / unl.hip: the launch geometry
// and the argument checks the entries share, the resized logits of one output pixel, the stencil weight of a source row / column, and
// the frame of a gather block - one block per SOURCE pixel: its window of candidate output pixels (also upsample_bwd_kernel's,
// pointwise.hip) and the block sum that ends it.  Device code is not linked across translation units: this header is instantiated in
// each, in an unnamed namespace as the kernels that use it are.
#pragma once
#include "common.h"
#include "head_common.h"

namespace {

struct HeadGeom { int N, H, W, C, OH, OW; float sh, sw, inv_sh, inv_sw; };

// class weight of the weighted cross entropy (sscg_ce_fwd_w's formulas, loss_optim.hip); class_w == NULL: all ones
__device__ __forceinline__ float class_weight(const float* __restrict__ class_w, int c) { return class_w ? class_w[c] : 1.f; }

template <int CT>
__device__ __forceinline__ void head_logits(const float* __restrict__ xn, const HeadGeom& g, int oy, int ox, int C, float* v,
                                            int* y0o, int* x0o) {
    // the arithmetic of upsample_fwd_kernel (pointwise.hip)
    // NOT head_common.h's pinned sscg_bilerp, on purpose: contraction is the compiler's here and the training step's bits depend on it
    const float fy = g.sh * oy, fx = g.sw * ox;
    const int y0 = (int)fy, x0 = (int)fx;
    const int yp = y0 < g.H - 1 ? 1 : 0, xp = x0 < g.W - 1 ? 1 : 0;
    const float ly = fy - y0, lx = fx - x0;
    const float hy = 1.f - ly, hx = 1.f - lx;
    const float* r00 = xn + ((size_t)y0 * g.W + x0) * C;
    const float* r01 = r00 + (size_t)xp * C;
    const float* r10 = r00 + (size_t)yp * g.W * C;
    const float* r11 = r10 + (size_t)xp * C;
#pragma unroll
    for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c) {
        if (CT == 0 && c >= C) break;
        v[c] = hy * (hx * r00[c] + lx * r01[c]) + ly * (hx * r10[c] + lx * r11[c]);
    }
    *y0o = y0; *x0o = x0;
}

// weight of source row / column `i` in the stencil of output row / column `o` (upsample_bwd_kernel's)
__device__ __forceinline__ float head_weight(float scale, int o, int i, int n_src) {
    const float f = scale * o;
    const int i0 = (int)f;
    const int ip = i0 < n_src - 1 ? 1 : 0;
    const float l = f - i0;
    float w = 0.f;
    if (i0 == i) w += 1.f - l;
    if (i0 + ip == i) w += l;
    return w;
}

// source pixel (n, iy, ix) and the output rows / columns whose stencil can touch it (a superset: head_weight decides)
struct HeadWindow { int n, iy, ix, oy_lo, oy_hi, ox_lo, ox_hi; };

__device__ __forceinline__ HeadWindow head_window_at(int n, int iy, int ix, int OH, int OW, float inv_sh, float inv_sw) {
    HeadWindow w;
    w.n = n; w.iy = iy; w.ix = ix;
    int oy_lo = (int)floorf((iy - 1) * inv_sh) - 1, oy_hi = (int)ceilf((iy + 1) * inv_sh) + 1;
    int ox_lo = (int)floorf((ix - 1) * inv_sw) - 1, ox_hi = (int)ceilf((ix + 1) * inv_sw) + 1;
    w.oy_lo = max(oy_lo, 0); w.ox_lo = max(ox_lo, 0);
    w.oy_hi = min(oy_hi, OH - 1); w.ox_hi = min(ox_hi, OW - 1);
    return w;
}

// block b of a grid of N * H * W: its source pixel and window
__device__ __forceinline__ HeadWindow head_window(const HeadGeom& g, int b) {
    return head_window_at(b / (g.W * g.H), (b / g.W) % g.H, b % g.W, g.OH, g.OW, g.inv_sh, g.inv_sw);
}

// The end of a gather block: acc[c] summed over the block's 256 threads (wave butterflies, then the four waves in a fixed order), plus
// - dl_ce != NULL - the cross-entropy gradient the forward left, scaled by g_ce / valid; row b of out.
template <int CT>
__device__ __forceinline__ void head_store_sum(const float (&acc)[CT ? CT : SSCG_MAXC], float (&red)[4][SSCG_MAXC], int C, int b, const float* __restrict__ dl_ce,
                                               const float* __restrict__ g_ce, const float* __restrict__ valid, float* __restrict__ out) {
#pragma unroll
    for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
        if (CT || c < C) {
            const float r = wave_sum(acc[c]);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][c] = r;
        }
    __syncthreads();
    if ((int)threadIdx.x < C) {
        const int c = threadIdx.x;
        float r = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
        if (dl_ce) {
            const float nv = valid ? *valid : 0.f;
            r += dl_ce[(size_t)b * C + c] * ((g_ce ? *g_ce : 1.f) * (nv > 0.f ? 1.f / nv : 0.f));
        }
        out[(size_t)b * C + c] = r;
    }
}

// ---- the losses of the unlabelled head (unl.hip's flat backward and the UNL term of head_bwd_kernel share these)
constexpr int UNL_DROPPED = 255;   // the pseudo-label map's value of a pixel below the threshold (C <= 64: never a class id)

// the per-call factors of the three gradients: ke = g_ent / (V ln C) (C == 1: / V), km = g_msq / V, kp = g_pl / max(K, 1), K = sums[3];
// a NULL upstream scalar: that loss took no part, its factor is 0
struct UnlCoef { float ke, km, kp; };

__device__ __forceinline__ UnlCoef unl_coef(const float* __restrict__ g_ent, const float* __restrict__ g_msq, const float* __restrict__ g_pl,
                                            const double* __restrict__ sums, double V, int C) {
    UnlCoef k;
    k.ke = g_ent ? (float)((double)*g_ent / (V * (C > 1 ? log((double)C) : 1.0))) : 0.f;
    k.km = g_msq ? (float)((double)*g_msq / V) : 0.f;
    k.kp = 0.f;
    if (g_pl) {
        const double K = sums[3];
        k.kp = (float)((double)*g_pl / (K > 1.0 ? K : 1.0));
    }
    return k;
}

// q_c without the softmax map's gradient: -ke u_c - km p_c (u_c = z_c - max z: finite where p_c has vanished, so p_c q_c is 0, not NaN)
__device__ __forceinline__ float unl_upstream(const UnlCoef& k, float u, float p) { return -(k.ke * u) - k.km * p; }

}  // namespace

// the scales of a resize H x W -> OH x OW and the bounds the windows invert them by
static void head_scales(HeadGeom* g, int N, int H, int W, int C, int OH, int OW) {
    g->N = N; g->H = H; g->W = W; g->C = C; g->OH = OH; g->OW = OW;
    g->sh = sscg_resize_scale(H, OH); g->sw = sscg_resize_scale(W, OW);
    g->inv_sh = sscg_resize_inv_scale(g->sh, OH); g->inv_sw = sscg_resize_inv_scale(g->sw, OW);
}

// ---- host: the argument checks the entries of the head, the Dice loss and the mined cross entropy share
static inline bool sizes_ok(int N, int H, int W, int C, int OH, int OW) { return N > 0 && H > 0 && W > 0 && C > 0 && C <= SSCG_MAXC && OH > 0 && OW > 0; }

// the kernels index source and output pixels with 32-bit integers
static inline bool too_large(int N, int H, int W, int OH, int OW) {
    const size_t lim = (size_t)1 << 31;
    return (size_t)N * OH * OW >= lim || (size_t)N * H * W >= lim;
}

static inline bool smoothing_ok(float smoothing) { return smoothing >= 0.f && smoothing < 1.f; }     // (false for a NaN)

static bool head_geom(HeadGeom* g, int N, int H, int W, int C, int OH, int OW) {
    if (!sizes_ok(N, H, W, C, OH, OW)) return false;
    if ((size_t)N * H * W >= ((size_t)1 << 31)) return false;
    head_scales(g, N, H, W, C, OH, OW);
    return true;
}
