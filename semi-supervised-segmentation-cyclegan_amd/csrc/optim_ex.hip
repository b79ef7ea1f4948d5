// Optimiser options of the flat-arena Adam (include/sscg.h, K14): the global gradient norm with its clip coefficient, and the Adam
// launch with that coefficient, weight decay (Adam-L2 or decoupled AdamW) and an EMA stream.  The plain step stays sscg_adam_step
// (loss_optim.hip); sscg_adam_step_ex hands over to it when no option is set.
//
// Bit contract: with a coefficient of exactly 1.0f and/or an EMA and no decay, param / both moments / shadow leave this kernel with
// the bits adam_kernel gives them.  Left to the compiler the same expression contracts differently from kernel to kernel, so the
// arithmetic is PINNED (as head_common.h and norm_expr.h pin theirs): contraction is switched off and the FMAs that adam_kernel
// compiles to on gfx950 are written out -
//     d     = fma(g, scale, -m)              the scaled gradient is NOT rounded on its way into the first moment
//     m'    = fma(1 - beta1, d, m)
//     v'    = fma(v, beta2, ((g * scale) * (g * scale)) * (1 - beta2))
//     denom = fma(1 / sqrt(bc2), sqrt(v'), eps)
//     p'    = fma(-step_size, m' / denom, p)
// `scale` is grad_scale * clip, formed once per thread: with clip == 1.0f it is grad_scale itself, so the contract holds for every
// grad_scale (not only the powers of two for which g * grad_scale is exact).
#include <cmath>

#include "common.h"
#include "sscg_internal.h"

namespace {

constexpr int NORM_BLOCKS = 2048;     // 256 CUs x 8 workgroups of 4 waves: every SIMD full, the rest of the arena is strided over
constexpr int ADAM_BLOCKS = 16384;    // as the plain launch

inline int capped_blocks(size_t work, int cap) {
    size_t b = (work + 255) / 256;
    if (b > (size_t)cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

// ---------------------------------------------------------------- global gradient norm
// Stage 1: every thread sums (double)t * t of its elements, t = fp32(grad * grad_scale), in a fixed order; one fp64 partial per
// workgroup (wave shuffle, then four wave sums in order).  16-byte loads over the aligned body [head, head + 4 * nvec); the up to
// three elements in front of it and the up to three behind it go to threads of workgroup 0.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, size_t n, size_t head, size_t nvec,
                                                         float grad_scale, double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double sm[4];
    double acc = 0.0;
    const f32x4* __restrict__ gv = reinterpret_cast<const f32x4*>(g + head);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
        const f32x4 t = gv[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double s = (double)(t[e] * grad_scale);
            acc += s * s;
        }
    }
    if (blockIdx.x == 0) {
        const size_t tail0 = head + 4 * nvec;
        size_t i = n;
        if (threadIdx.x < 4) i = threadIdx.x < head ? threadIdx.x : n;
        else if (threadIdx.x < 8) i = tail0 + (threadIdx.x - 4);
        if (i < n) {
            const double s = (double)(g[i] * grad_scale);
            acc += s * s;
        }
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = sm[0] + sm[1] + sm[2] + sm[3];
}

// Stage 2: the partials in a fixed order; norm and torch.nn.utils.clip_grad_norm_'s coefficient, both fp32 device scalars.
__global__ void finish_norm_kernel(const double* __restrict__ part, int nparts, float max_norm, float* __restrict__ norm,
                                   float* __restrict__ clip) {
#pragma clang fp contract(off)
    __shared__ double sm[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) s += part[i];
    sm[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < 256; ++i) t += sm[i];
        const float nrm = (float)sqrt(t);
        const float c = max_norm / (nrm + 1e-6f);
        if (norm) *norm = nrm;
        if (clip) *clip = c > 1.0f ? 1.0f : c;       // (a NaN coefficient stays NaN, as torch.clamp keeps it)
    }
}

// ---------------------------------------------------------------- Adam with options
enum { DECAY_NONE = 0, DECAY_L2 = 1, DECAY_DECOUPLED = 2 };

template <int DECAY>
__global__ void adam_ex_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                               __bf16* __restrict__ p16, int split, float* __restrict__ ema, size_t n, float step_size, float omb1,
                               float beta2, float omb2, float eps, float inv_bc2_sqrt, float grad_scale,
                               const float* __restrict__ clip, float wd, float keep, float ome) {
#pragma clang fp contract(off)
    const float scale = clip ? grad_scale * *clip : grad_scale;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float graw = g[i];
        float mi = m[i], vi = v[i], pi = p[i];
        float gi = graw * scale, d;
        if (DECAY == DECAY_L2) {
            gi = __builtin_fmaf(wd, pi, gi);         // torch.optim.Adam(weight_decay=): grad.add(param, alpha=wd), after the clip
            d = gi - mi;
        } else {
            d = __builtin_fmaf(graw, scale, -mi);
        }
        if (DECAY == DECAY_DECOUPLED) pi = pi * keep;    // torch.optim.AdamW: param.mul_(1 - lr * wd)
        mi = __builtin_fmaf(omb1, d, mi);
        vi = __builtin_fmaf(vi, beta2, (gi * gi) * omb2);
        const float denom = __builtin_fmaf(inv_bc2_sqrt, sqrtf(vi), eps);
        const float pn = __builtin_fmaf(-step_size, mi / denom, pi);
        p[i] = pn;
        if (p16) {
            if (split) {
                const sscg_bf3 t = sscg_split3(pn);
                p16[i] = t.h; p16[n + i] = t.m; p16[2 * n + i] = t.l;
            } else {
                p16[i] = (__bf16)pn;
            }
        }
        m[i] = mi;
        v[i] = vi;
        if (ema) {
            const float e = ema[i];
            ema[i] = __builtin_fmaf(ome, pn - e, e);     // ema.lerp_(param, 1 - ema_decay)
        }
    }
}

}  // namespace

extern "C" size_t sscg_grad_norm_workspace(int64_t n) {
    (void)n;
    return (size_t)NORM_BLOCKS * sizeof(double);
}

extern "C" int sscg_grad_norm(const float* grad, int64_t n, float grad_scale, float max_norm, float* norm, float* clip, void* ws,
                              size_t ws_bytes, void* stream) {
    if (!grad || n <= 0 || !(max_norm > 0.f) || (!norm && !clip)) return SSCG_ERR_BAD_ARG;      // (a NaN max_norm fails the compare)
    if (((uintptr_t)grad & 3) != 0) return SSCG_ERR_BAD_ARG;
    if (!ws || ws_bytes < sscg_grad_norm_workspace(n)) return SSCG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    size_t head = ((16 - ((uintptr_t)grad & 15)) & 15) / 4;
    if (head > (size_t)n) head = (size_t)n;
    const size_t nvec = ((size_t)n - head) / 4;
    const int nb = capped_blocks(nvec, NORM_BLOCKS);
    double* part = reinterpret_cast<double*>(ws);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(nb), dim3(256), 0, st, grad, (size_t)n, head, nvec, grad_scale, part);
    hipLaunchKernelGGL(finish_norm_kernel, dim3(1), dim3(256), 0, st, part, nb, max_norm, norm, clip);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_adam_step_ex(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow, int shadow_dtype,
                                 float* ema, int64_t n, double lr, double beta1, double beta2, double eps, int step, float grad_scale,
                                 const float* clip, double weight_decay, int decoupled, double ema_decay, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0 || step <= 0) return SSCG_ERR_BAD_ARG;
    if (shadow && shadow_dtype != SSCG_BF16 && shadow_dtype != SSCG_BF16X3) return SSCG_ERR_BAD_ARG;
    if (!std::isfinite(weight_decay) || weight_decay < 0.0) return SSCG_ERR_BAD_ARG;
    if (ema && !(ema_decay >= 0.0 && ema_decay < 1.0)) return SSCG_ERR_BAD_ARG;                  // (false for a NaN)
    if (!clip && weight_decay == 0.0 && !ema)
        return sscg_adam_step(param, grad, exp_avg, exp_avg_sq, shadow, shadow_dtype, n, lr, beta1, beta2, eps, step, grad_scale, stream);
    // hyper-parameters arrive as doubles (python floats): 1 - beta, 1 - lr * wd and 1 - ema_decay must not be formed in fp32
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    const float step_size = (float)(lr / bc1);
    const float inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    const float keep = (float)(1.0 - lr * weight_decay);
    const float ome = ema ? (float)(1.0 - ema_decay) : 0.f;
    const int decay = weight_decay > 0.0 ? (decoupled ? DECAY_DECOUPLED : DECAY_L2) : DECAY_NONE;
    const dim3 grid(capped_blocks((size_t)n, ADAM_BLOCKS)), block(256);
    hipStream_t st = (hipStream_t)stream;
#define SSCG_ADAM_EX(D)                                                                                                              \
    hipLaunchKernelGGL(adam_ex_kernel<D>, grid, block, 0, st, param, grad, exp_avg, exp_avg_sq, reinterpret_cast<__bf16*>(shadow),  \
                       shadow_dtype == SSCG_BF16X3 ? 1 : 0, ema, (size_t)n, step_size, (float)(1.0 - beta1), (float)beta2,           \
                       (float)(1.0 - beta2), (float)eps, inv_bc2_sqrt, grad_scale, clip, (float)weight_decay, keep, ome)
    if (decay == DECAY_L2) SSCG_ADAM_EX(DECAY_L2);
    else if (decay == DECAY_DECOUPLED) SSCG_ADAM_EX(DECAY_DECOUPLED);
    else SSCG_ADAM_EX(DECAY_NONE);
#undef SSCG_ADAM_EX
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}
