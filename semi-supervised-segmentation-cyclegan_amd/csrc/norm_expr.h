// The per-element expressions of the normalisation layers, each defined ONCE: norm.hip's forward, backward and head kernels, the
// eval-mode BatchNorm folded into a convolution's store phase (sscg_conv2d_fwd_affine; conv_split.hip, conv_bf16.hip) and the second
// stage of a split-K tail (reduce_common.h) all call these functions.  Routes that promise equal bits - flat and slab kernels, the
// folded launch against sscg_rstd_from_var + sscg_norm_apply, the backward's recomputed activation mask against the forward's output
// sign - therefore evaluate the same operations in the same order.  The arithmetic is PINNED, as head_common.h pins the bilinear
// resize: contraction is switched off and every fused multiply-add is written out:
//     t = (x - mean) * rstd               two roundings              sscg_norm_xhat
//     v = fma(t, gamma, beta)             one rounding               sscg_norm_pre   (affine layers; the mask's source)
//     v = v + residual                    one rounding               sscg_bn_fold    (units a shortcut joins)
// followed by the activation (a compare and a select: nothing to contract), and in the backward
//     d = fma(-t, c2, gg - c1)            two roundings              sscg_norm_bwd_elem
//     dx = d * rstd * gamma               two roundings
#pragma once
#include "common.h"

// rstd_from_var_kernel's expression (norm.hip).  The fp64 square root and division are correctly rounded, so the value does not
// depend on the kernel that evaluates it.
__device__ __forceinline__ float sscg_bn_rstd(float var, float eps) { return (float)(1.0 / sqrt((double)var + (double)eps)); }

__device__ __forceinline__ float sscg_norm_xhat(float x, float mean, float rstd) {
#pragma clang fp contract(off)
    return (x - mean) * rstd;
}

// the pre-activation of an affine layer; its sign is the activation mask the backward recomputes
__device__ __forceinline__ float sscg_norm_pre(float xhat, float gamma, float beta) { return __builtin_fmaf(xhat, gamma, beta); }

__device__ __forceinline__ float sscg_bn_fold(float x, float mean, float rstd, float gamma, float beta, bool has_g, float res, bool has_r) {
#pragma clang fp contract(off)
    float v = sscg_norm_xhat(x, mean, rstd);
    if (has_g) v = sscg_norm_pre(v, gamma, beta);
    if (has_r) v = v + res;
    return v;
}

// gradient through the activation, from the forward's output (or its recomputed pre-activation: same sign)
__device__ __forceinline__ float sscg_act_grad(float dy, float y, int act, float slope) {
    if (act == SSCG_ACT_RELU) return y > 0.f ? dy : 0.f;
    if (act == SSCG_ACT_LRELU) return y > 0.f ? dy : dy * slope;
    if (act == SSCG_ACT_TANH) return dy * (1.f - y * y);
    return dy;
}

// dx of one element from the activation's gradient gg; (c1, c2) = (mean of gg, mean of gg * xhat) over the statistics' rows
// (has_c false: the statistics are constants)
__device__ __forceinline__ float sscg_norm_bwd_elem(float gg, float xhat, float c1, float c2, float rstd, float gamma, bool has_c) {
#pragma clang fp contract(off)
    float v = gg;
    if (has_c) v = __builtin_fmaf(-xhat, c2, gg - c1);
    return v * rstd * gamma;
}

// the folded layer's parameters as an entry point hands them to a kernel family (host side)
struct sscg_bn_fold_args {
    const float* mean;       // running_mean [K]
    const float* var;        // running_var [K]
    const float* gamma;      // [K] or null (then beta is null too)
    const float* beta;
    const void* residual;    // [N][P][Q][K] in y's dtype, or null
    float eps;
};
