// Per-pixel arithmetic that more than one kernel must compute to the same bits.
//   * The bilinear resize (align_corners=True) is where multiplies feed adds, i.e. where contraction into FMAs decides the last bit.
//     Left to the compiler, the same expression contracts differently from kernel to kernel (it depends on what else is in flight:
//     packed multiplies, the uses of an intermediate), so the operations are PINNED here: contraction is switched off inside these
//     functions and the fused multiply-adds are written out - the ones upsample_fwd_kernel (pointwise.hip) has always computed.
//     That kernel and the inference heads (predict.hip) inline the same functions.
//   * The softmax and first-maximum over the class axis as the inference heads hold them in registers: the operations of
//     softmax_fwd_kernel / argmax_onehot_kernel in their order (max, exp(v - max), running sum, one reciprocal, one multiply per class,
//     strict > from class 0 up).  No multiply feeds an add there, so nothing can contract.
//   * The sum of several views' probabilities (tta.hip): there a multiply does feed an add - the probability v[c] * inv, which the
//     separate passes store as an fp32 value, into the accumulator - so that function is pinned as well.
// Around that arithmetic, everything else the class-axis kernels share (predict.hip, tta.hip, panels.hip, dice.hip, loss_optim.hip):
// the class limit, the resize scales and the output-pixel geometry, the loader of one pixel's logits, the element fetch of the
// element-wise resizes, the per-workgroup confusion bins and the host dispatch over the instantiated class counts.
#pragma once
#include "common.h"
#include <type_traits>

constexpr int SSCG_MAXC = 64;   // class axis is 4 / 20 / 21 in the reference (model.py:205-210)

// torch upsample_bilinear2d arithmetic for one output row / column pair: src = scale * dst in fp32
struct sscg_bilin {
    int y0, x0, yp, xp;        // top-left source pixel, +1 steps (0 on the last row / column)
    float ly, lx, hy, hx;
};

__device__ __forceinline__ sscg_bilin sscg_bilin_at(int oy, int ox, int H, int W, float sh, float sw) {
#pragma clang fp contract(off)
    sscg_bilin b;
    const float foy = (float)oy, fox = (float)ox;
    const float fy = sh * foy, fx = sw * fox;
    b.y0 = (int)fy; b.x0 = (int)fx;
    b.yp = b.y0 < H - 1 ? 1 : 0; b.xp = b.x0 < W - 1 ? 1 : 0;
    b.ly = __builtin_fmaf(sh, foy, -(float)b.y0);       // scale * dst - floor in one rounding
    b.lx = __builtin_fmaf(sw, fox, -(float)b.x0);
    b.hy = 1.f - b.ly; b.hx = 1.f - b.lx;
    return b;
}

__device__ __forceinline__ float sscg_bilerp(const sscg_bilin& b, float v00, float v01, float v10, float v11) {
#pragma clang fp contract(off)
    const float top = __builtin_fmaf(b.lx, v01, b.hx * v00);
    const float bot = __builtin_fmaf(b.lx, v11, b.hx * v10);
    const float a = b.hy * top, c = b.ly * bot;
    return a + c;
}

// ---- host: the align_corners=True scale of one axis (src = scale * dst) and the bound the gather kernels invert it by
static inline float sscg_resize_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }
// scale == 0 (a single source row / column) => every output row touches it: scan the full range
static inline float sscg_resize_inv_scale(float scale, int out) { return scale > 0.f ? 1.f / scale : (float)out; }

// output pixel -> source stencil: what a kernel with one thread per output pixel / element needs
struct sscg_resize_geom {
    int H, W, C, OH, OW;
    float sh, sw;
    FastDiv dow, doh;
};

static inline sscg_resize_geom sscg_make_resize_geom(int H, int W, int C, int OH, int OW) {
    sscg_resize_geom g;
    g.H = H; g.W = W; g.C = C; g.OH = OH; g.OW = OW;
    g.sh = sscg_resize_scale(H, OH); g.sw = sscg_resize_scale(W, OW);
    g.dow = make_fastdiv(OW); g.doh = make_fastdiv(OH);
    return g;
}

struct sscg_pixel { int n, oy, ox; };

// output index o = (n * OH + oy) * OW + ox
__device__ __forceinline__ sscg_pixel sscg_pixel_of(int o, const sscg_resize_geom& g) {
    sscg_pixel p;
    const int t = fd_div(o, g.dow);
    p.ox = o - t * g.OW;
    p.n = fd_div(t, g.doh);
    p.oy = t - p.n * g.OH;
    return p;
}

// The C logits of output pixel (n, oy, ox) in registers, from the [.][H][W][C] map x.  IDENT: the map has the output's size - the pixel's
// own row (n = oy = 0 and ox = the flat pixel index address the same row without the split); else the four source rows through the
// pinned stencil.  ox is the column in the MAP's coordinates: a mirrored view passes OW - 1 - ox.
// CT: class count at compile time (0 = any C <= SSCG_MAXC, every loop predicated on c < C so that v[] stays in registers).
template <int CT, bool IDENT>
__device__ __forceinline__ void sscg_pixel_logits(const float* __restrict__ x, int n, int oy, int ox, int H, int W, float sh, float sw,
                                                  int C, float* v) {
    if (IDENT) {
        const float* r = x + (((size_t)n * H + oy) * W + ox) * C;
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
            if (CT || c < C) v[c] = r[c];
    } else {
        const sscg_bilin b = sscg_bilin_at(oy, ox, H, W, sh, sw);
        const float* r00 = x + (((size_t)n * H + b.y0) * W + b.x0) * C;
        const float* r01 = r00 + (size_t)b.xp * C;
        const float* r10 = r00 + (size_t)b.yp * W * C;
        const float* r11 = r10 + (size_t)b.xp * C;
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
            if (CT || c < C) v[c] = sscg_bilerp(b, r00[c], r01[c], r10[c], r11[c]);
    }
}

// One element through the stencil: p = the sample's map + the channel, C floats from pixel to pixel.
__device__ __forceinline__ float sscg_bilerp_elem(const float* __restrict__ p, const sscg_bilin& b, int W, int C) {
    const float v00 = p[((size_t)b.y0 * W + b.x0) * C], v01 = p[((size_t)b.y0 * W + b.x0 + b.xp) * C];
    const float v10 = p[((size_t)(b.y0 + b.yp) * W + b.x0) * C], v11 = p[((size_t)(b.y0 + b.yp) * W + b.x0 + b.xp) * C];
    return sscg_bilerp(b, v00, v01, v10, v11);
}

// nn.Softmax2d of one pixel's C values, in place: v[c] <- exp(v[c] - max); returns 1 / sum, the factor every v[c] is multiplied by.
// CT > 0: the class count at compile time (values in registers); CT == 0: C <= SSCG_MAXC at run time.
template <int CT>
__device__ __forceinline__ float sscg_softmax_exp(float* v, int C) {
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
        if (CT || c < C) m = fmaxf(m, v[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
        if (CT || c < C) { v[c] = expf(v[c] - m); s += v[c]; }
    return 1.f / s;
}

// argmax over c of v[c] * inv, first maximum wins (argmax_onehot_kernel's strict > on the probabilities softmax_fwd_kernel stores)
template <int CT>
__device__ __forceinline__ int sscg_first_max_scaled(const float* v, float inv, int C) {
    float best = v[0] * inv;
    int bi = 0;
#pragma unroll
    for (int c = 1; c < (CT ? CT : SSCG_MAXC); ++c)
        if (CT || c < C) {
            const float p = v[c] * inv;
            if (p > best) { best = p; bi = c; }
        }
    return bi;
}

// acc[c] <- (first ? 0 : acc[c]) + v[c] * inv: one view's probabilities (what softmax_fwd_kernel stores) added to the running sum of the
// views before it by a plain fp32 add.  The product is rounded to fp32 before the add - the stored value of the separate passes - so
// nothing here may contract into an FMA.
template <int CT>
__device__ __forceinline__ void sscg_prob_accumulate(float* acc, const float* v, float inv, int C, bool first) {
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
        if (CT || c < C) {
            const float p = v[c] * inv;
            acc[c] = first ? p : acc[c] + p;
        }
}

// acc[c] <- (first ? 0 : acc[c]) + g * (v[c] * inv): one window's probabilities times its blend weight g (sliding.hip).  The separate
// passes store the probability, then the weighted probability, each as an fp32 value, and add the latter in place: three roundings,
// none of which may contract.
template <int CT>
__device__ __forceinline__ void sscg_prob_accumulate_weighted(float* acc, const float* v, float inv, float g, int C, bool first) {
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
        if (CT || c < C) {
            const float t = v[c] * inv;
            const float p = g * t;
            acc[c] = first ? p : acc[c] + p;
        }
}

// argmax over c of a[c], first maximum wins (argmax_onehot_kernel's strict > from class 0 up)
template <int CT>
__device__ __forceinline__ int sscg_first_max(const float* a, int C) {
    float best = a[0];
    int bi = 0;
#pragma unroll
    for (int c = 1; c < (CT ? CT : SSCG_MAXC); ++c)
        if (CT || c < C) {
            if (a[c] > best) { best = a[c]; bi = c; }
        }
    return bi;
}

// The level set of the boundary loss from one signed squared distance (include/sscg.h: sscg_sdm): sqrt(s) outside the class,
// 1 - sqrt(-s) inside, 0 on a plane without a contour.  The conversion, the square root and the subtraction are each rounded once:
// the bits of numpy's sqrt on the fp32 cast.  Nothing here can contract.
__device__ __forceinline__ float sscg_level_set(int s) {
    if (s > 0) return __fsqrt_rn((float)s);
    if (s < 0) return 1.f - __fsqrt_rn((float)(-s));
    return 0.f;
}

// ---- the [C][C] confusion counts of one workgroup of 256 threads in LDS (nb = C * C bins; nb == 0, block-uniform: no histogram asked
// for, nothing happens): clear, count while the pixels are walked, flush with one 64-bit atomic per bin that was hit.  Integer sums:
// the result does not depend on the order.
__device__ __forceinline__ void sscg_bins_clear(unsigned int* bins, int nb) {
    for (int i = threadIdx.x; i < nb; i += 256) bins[i] = 0u;
    if (nb) __syncthreads();
}

__device__ __forceinline__ void sscg_bins_count(unsigned int* bins, int C, int64_t truth, int pred) {      // pred in [0, C)
    if (truth >= 0 && truth < C) atomicAdd(&bins[(int)truth * C + pred], 1u);
}

__device__ __forceinline__ void sscg_bins_flush(const unsigned int* bins, int nb, unsigned long long* __restrict__ hist) {
    if (nb) __syncthreads();
    for (int i = threadIdx.x; i < nb; i += 256)
        if (bins[i]) atomicAdd(&hist[i], (unsigned long long)bins[i]);
}

// ---- host: f(std::integral_constant<int, CT>) for the instantiated class count that serves C - 21, 20, 4, or 0 = C at run time
template <class F>
static inline void sscg_dispatch_classes(int C, F&& f) {
    if (C == 21) f(std::integral_constant<int, 21>{});
    else if (C == 20) f(std::integral_constant<int, 20>{});
    else if (C == 4) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 0>{});
}
