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
#pragma once
#include "common.h"

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
