// Eval-mode BatchNorm folded into a convolution's store phase (sscg_conv2d_fwd_affine; conv_split.hip, conv_bf16.hip).
// The fused launch must give the bits of the separate passes it replaces - sscg_rstd_from_var, then sscg_norm_apply on the stored
// conv output - so the per-element arithmetic is PINNED here, as head_common.h pins the bilinear resize: contraction is switched off
// and the operations are written out the way norm.hip's apply kernels have always been compiled (every instance of
// norm_apply_kernel / norm_apply_slab_kernel: v_sub, v_mul, v_fma, v_add):
//     t = (x - mean) * rstd          two roundings
//     v = fma(t, gamma, beta)        one rounding (affine layers)
//     v = v + residual               one rounding (units a shortcut joins)
// followed by the activation (a compare and a select: nothing to contract).
#pragma once
#include "common.h"

// rstd_from_var_kernel's expression (norm.hip).  The fp64 square root and division are correctly rounded, so the value does not
// depend on the kernel that evaluates it.
__device__ __forceinline__ float sscg_bn_rstd(float var, float eps) { return (float)(1.0 / sqrt((double)var + (double)eps)); }

__device__ __forceinline__ float sscg_bn_fold(float x, float mean, float rstd, float gamma, float beta, bool has_g, float res, bool has_r) {
#pragma clang fp contract(off)
    float v = (x - mean) * rstd;
    if (has_g) v = __builtin_fmaf(v, gamma, beta);
    if (has_r) v = v + res;
    return v;
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
