// Class-axis ops, loss/grad kernels and the fused Adam step.  Reference call sites per entry point
// are listed in include/sscg.h.  Losses are mean reductions accumulated in fp64 in two fixed-order
// stages (deterministic), written as one fp32 device scalar.
#include "common.h"
#include "head_geom.h"
#include "sscg_internal.h"

namespace {

constexpr int LOSS_BLOCKS = 1024;

__device__ __forceinline__ void block_sum_to(double v, double* out) {
    __shared__ double sm[4];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) *out = sm[0] + sm[1] + sm[2] + sm[3];
}

__global__ void finish_loss_kernel(const double* __restrict__ part, int nparts, double inv_n, float* __restrict__ loss) {
    __shared__ double sm[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) s += part[i];
    sm[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < 256; ++i) t += sm[i];
        *loss = (float)(t * inv_n);
    }
}

// ---------------------------------------------------------------- softmax / argmax / one-hot
__global__ void softmax_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, size_t rows, int C) {
    for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (size_t)gridDim.x * 256) {
        const float* xr = x + r * C;
        float v[SSCG_MAXC];
        float m = -INFINITY;
        for (int c = 0; c < C; ++c) { v[c] = xr[c]; m = fmaxf(m, v[c]); }
        float s = 0.f;
        for (int c = 0; c < C; ++c) { v[c] = expf(v[c] - m); s += v[c]; }
        float inv = 1.f / s;
        float* yr = y + r * C;
        for (int c = 0; c < C; ++c) yr[c] = v[c] * inv;
    }
}

__global__ void softmax_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ dx,
                                   size_t rows, int C) {
    for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (size_t)gridDim.x * 256) {
        const float* yr = y + r * C;
        const float* gr = dy + r * C;
        float dot = 0.f;
        for (int c = 0; c < C; ++c) dot += yr[c] * gr[c];
        float* dr = dx + r * C;
        for (int c = 0; c < C; ++c) dr[c] = yr[c] * (gr[c] - dot);
    }
}

__global__ void argmax_onehot_kernel(const float* __restrict__ x, float* __restrict__ oh, int64_t* __restrict__ index,
                                     size_t rows, int C) {
    for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (size_t)gridDim.x * 256) {
        const float* xr = x + r * C;
        float best = xr[0];
        int bi = 0;
        for (int c = 1; c < C; ++c) {
            float v = xr[c];
            if (v > best) { best = v; bi = c; }  // strict: first maximum wins (torch.max(dim) tie rule)
        }
        if (oh) {
            float* o = oh + r * C;
            for (int c = 0; c < C; ++c) o[c] = (c == bi) ? 1.f : 0.f;
        }
        if (index) index[r] = bi;
    }
}

__global__ void label_onehot_kernel(const int64_t* __restrict__ lab, float* __restrict__ oh, size_t rows, int C) {
    for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (size_t)gridDim.x * 256) {
        const int64_t l64 = lab[r];
        const int l = (l64 < 0 || l64 >= C) ? -1 : (int)l64;     // out-of-range id: an all-zero row, as scatter_ would refuse it
        float* o = oh + r * C;
        for (int c = 0; c < C; ++c) o[c] = (c == l) ? 1.f : 0.f;
    }
}

// ---------------------------------------------------------------- cross entropy
// Pixels whose label lies outside [0, C) take no part in the loss (nn.CrossEntropyLoss's ignore_index semantics,
// extended to every out-of-range id: the 255 "void" of an un-relabelled VOC map, a raw Cityscapes id, -100): they add
// nothing to the sum, are not counted in the mean and get a zero gradient - never an out-of-bounds read.
//
// WT (class weights w and / or label smoothing eps; sscg_ce_fwd_w / _bwd_w / sscg_upsample_head_fwd_w) is a separate instantiation of
// each kernel - the plain ones keep their instruction stream.  With p = softmax(z), W = sum_c w[c], a counted pixel adds
//     term = (1-eps) * w[y] * (-log p[y]) + (eps/C) * sum_c w[c] * (-log p[c])          to the loss sum,
//     w[y]                                                                              to the divisor D (`valid`),
//     d term / d z[c] = (1-eps) * w[y] * (p[c] - [c==y]) + (eps/C) * (p[c] * W - w[c])  to the gradient (times g / D in the backward)
// - F.cross_entropy(weight=w, label_smoothing=eps).  sum_c w[c] * (-log p[c]) = W * log(s) - sum_c w[c] * (z[c] - m) with m = max z,
// s = sum exp(z - m): one FMA per class in the loop that forms the exponentials.  class_w == NULL: all ones.

template <bool WT>
__global__ void ce_fwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ lab, size_t rows, int C,
                              double* __restrict__ part, int nparts, const float* __restrict__ class_w, float smoothing) {
    double acc = 0.0, cnt = 0.0;
    float wsum = 0.f;
    if (WT)
        for (int c = 0; c < C; ++c) wsum += class_weight(class_w, c);
    for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (size_t)gridDim.x * 256) {
        const int64_t l = lab[r];
        if (l < 0 || l >= C) continue;
        const float* xr = x + r * C;
        float m = -INFINITY;
        for (int c = 0; c < C; ++c) m = fmaxf(m, xr[c]);
        float s = 0.f;
        if (WT) {
            float swd = 0.f;
            for (int c = 0; c < C; ++c) {
                const float d = xr[c] - m;
                swd += class_weight(class_w, c) * d;
                s += expf(d);
            }
            const float wl = class_weight(class_w, (int)l), ls = logf(s);
            acc += (double)((1.f - smoothing) * wl * (ls + m - xr[l]) + smoothing / (float)C * (ls * wsum - swd));
            cnt += (double)wl;
            continue;
        }
        for (int c = 0; c < C; ++c) s += expf(xr[c] - m);
        acc += (double)(logf(s) + m - xr[l]);
        cnt += 1.0;
    }
    block_sum_to(acc, part + blockIdx.x);
    __syncthreads();
    block_sum_to(cnt, part + nparts + blockIdx.x);
}

// loss = sum / count; count (the number of pixels with a valid label) also goes to `valid` for the backward pass
__global__ void finish_ce_kernel(const double* __restrict__ part, int nparts, float* __restrict__ loss, float* __restrict__ valid) {
    __shared__ double sm[512];
    double s = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) { s += part[i]; c += part[nparts + i]; }
    sm[threadIdx.x] = s;
    sm[256 + threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0, n = 0.0;
        for (int i = 0; i < 256; ++i) { t += sm[i]; n += sm[256 + i]; }
        *loss = n > 0.0 ? (float)(t / n) : __builtin_nanf("");      // no pixel with a label in [0, C): NaN, as nn.CrossEntropyLoss gives
        if (valid) *valid = (float)n;
    }
}

template <bool WT>
__global__ void ce_bwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ lab, size_t rows, int C,
                              const float* __restrict__ gscale, float w, const float* __restrict__ valid,
                              float* __restrict__ dx, const float* __restrict__ class_w, float smoothing) {
    const float n = valid ? *valid : (float)rows;
    const float g = (gscale ? *gscale : 1.f) * (n > 0.f ? w / n : 0.f);
    float wsum = 0.f;
    if (WT)
        for (int c = 0; c < C; ++c) wsum += class_weight(class_w, c);
    for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (size_t)gridDim.x * 256) {
        const float* xr = x + r * C;
        const int64_t l64 = lab[r];
        if (l64 < 0 || l64 >= C) {
            float* dr = dx + r * C;
            for (int c = 0; c < C; ++c) dr[c] = 0.f;
            continue;
        }
        float v[SSCG_MAXC];
        float m = -INFINITY;
        for (int c = 0; c < C; ++c) { v[c] = xr[c]; m = fmaxf(m, v[c]); }
        float s = 0.f;
        for (int c = 0; c < C; ++c) { v[c] = expf(v[c] - m); s += v[c]; }
        float inv = 1.f / s;
        const int l = (int)l64;
        float* dr = dx + r * C;
        if (WT) {
            const float a = (1.f - smoothing) * class_weight(class_w, l), bs = smoothing / (float)C;
            const float k = a + bs * wsum;
            for (int c = 0; c < C; ++c) dr[c] = (v[c] * inv * k - (c == l ? a : 0.f) - bs * class_weight(class_w, c)) * g;
            continue;
        }
        for (int c = 0; c < C; ++c) dr[c] = (v[c] * inv - (c == l ? 1.f : 0.f)) * g;
    }
}

// ---------------------------------------------------------------- upsample -> {softmax, cross entropy} from the low-resolution logits
// model.py:390-392 (interp = bilinear, align_corners=True, to the crop size), :398 / :455 (CrossEntropyLoss on the resized logits),
// :401-402 (softmax of the resized logits).  The resized [N][OH][OW][C] logits are never written: one block per SOURCE pixel walks
// the output pixels whose bilinear stencil touches it (gather form: deterministic, no atomics), interpolates their logits from the
// low-resolution map (L2-resident: N x 33 x 33 x 21 fp32 = 0.7 MB), and
//   * the block that owns an output pixel (its stencil's top-left corner) adds its loss term / writes its softmax row,
//   * every block sums weight * d(loss)/d(resized logit) of its output pixels: the gradient with respect to the low-resolution
//     logits, which for the cross entropy depends on nothing but logits and labels - so the FORWARD pass already leaves it
//     (unscaled; the backward is an elementwise scale by g / valid).
// This is the forward (labels and / or softmax output); the backward is head_bwd_kernel (head_bwd.hip).  WT: the class-weighted /
// label-smoothed cross entropy - see ce_fwd_kernel; `cnt` then sums w[y], and what is left in dlo is still the gradient up to
// g / valid, so head_bwd_kernel and head_scale_kernel serve it as is.
template <int CT, bool WT>
__global__ __launch_bounds__(256) void head_kernel(const float* __restrict__ x, const int64_t* __restrict__ lab, float* __restrict__ y_soft,
                                                   float* __restrict__ dlo, double* __restrict__ part, int nparts, HeadGeom g,
                                                   const float* __restrict__ class_w, float smoothing) {
    __shared__ float red[4][SSCG_MAXC];
    const int C = CT ? CT : g.C;
    const int b = blockIdx.x;
    const HeadWindow win = head_window(g, b);
    const int ix = win.ix, iy = win.iy, n = win.n, oy_lo = win.oy_lo, ox_lo = win.ox_lo;
    const int nx = win.ox_hi - ox_lo + 1, cand = (win.oy_hi - oy_lo + 1) * nx;
    const float* xn = x + (size_t)n * g.H * g.W * C;
    float acc[CT ? CT : SSCG_MAXC];
#pragma unroll
    for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c) acc[c] = 0.f;
    double loss = 0.0, cnt = 0.0;
    float wr[WT ? (CT ? CT : SSCG_MAXC) : 1];      // WT: the class weights (block-uniform loads) and their sum, once per block
    float wsum = 0.f;
    if (WT) {
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c) {
            if (CT == 0 && c >= C) break;
            wr[c] = class_weight(class_w, c);
            wsum += wr[c];
        }
    }
    for (int t = threadIdx.x; t < cand; t += 256) {
        const int oy = oy_lo + t / nx, ox = ox_lo + t % nx;
        const float wy = head_weight(g.sh, oy, iy, g.H);
        if (wy == 0.f) continue;
        const float wx = head_weight(g.sw, ox, ix, g.W);
        if (wx == 0.f) continue;
        const float w = wy * wx;
        float v[CT ? CT : SSCG_MAXC];
        int y0, x0;
        head_logits<CT>(xn, g, oy, ox, C, v, &y0, &x0);
        const bool owner = y0 == iy && x0 == ix;
        const size_t o = ((size_t)n * g.OH + oy) * g.OW + ox;
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c) { if (CT == 0 && c >= C) break; m = fmaxf(m, v[c]); }
        int l = -1;
        float vl = 0.f;
        if (lab) {
            const int64_t l64 = lab[o];
            l = (l64 < 0 || l64 >= C) ? -1 : (int)l64;
        }
        float s = 0.f, swd = 0.f;
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c) {
            if (CT == 0 && c >= C) break;
            if (c == l) vl = v[c];
            if (WT) swd += wr[c] * (v[c] - m);
            v[c] = expf(v[c] - m);
            s += v[c];
        }
        const float inv = 1.f / s;
        if (WT) {
            if (owner && y_soft) {
                float* yr = y_soft + o * C;
#pragma unroll
                for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c) { if (CT == 0 && c >= C) break; yr[c] = v[c] * inv; }
            }
            if (l >= 0) {
                const float wl = class_weight(class_w, l);
                const float a = (1.f - smoothing) * wl, bs = smoothing / (float)C;
                if (owner) {
                    const float ls = logf(s);
                    loss += (double)(a * (ls + m - vl) + bs * (ls * wsum - swd));
                    cnt += (double)wl;
                }
                const float k = a + bs * wsum;
#pragma unroll
                for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c) {
                    if (CT == 0 && c >= C) break;
                    acc[c] += w * (v[c] * inv * k - (c == l ? a : 0.f) - bs * wr[c]);
                }
            }
        } else {
            if (owner && l >= 0) { loss += (double)(logf(s) + m - vl); cnt += 1.0; }
            if (owner && y_soft) {
                float* yr = y_soft + o * C;
#pragma unroll
                for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c) { if (CT == 0 && c >= C) break; yr[c] = v[c] * inv; }
            }
            if (l >= 0) {
#pragma unroll
                for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c) { if (CT == 0 && c >= C) break; acc[c] += w * (v[c] * inv - (c == l ? 1.f : 0.f)); }
            }
        }
    }
    if (lab && dlo) head_store_sum<CT>(acc, red, C, b, nullptr, nullptr, nullptr, dlo);
    if (lab && part) {
        __syncthreads();
        block_sum_to(loss, part + b);
        __syncthreads();
        block_sum_to(cnt, part + nparts + b);
    }
}

// ---------------------------------------------------------------- MSE vs constant, L1
__global__ void mse_const_fwd_kernel(const float* __restrict__ x, size_t n, float target, double* __restrict__ part) {
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float d = x[i] - target;
        acc += (double)(d * d);
    }
    block_sum_to(acc, part + blockIdx.x);
}

__global__ void mse_const_bwd_kernel(const float* __restrict__ x, size_t n, float target, const float* __restrict__ gscale,
                                     float w, float* __restrict__ dx) {
    const float g = (gscale ? *gscale : 1.f) * w;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dx[i] = (x[i] - target) * g;
}

__global__ void l1_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n, double* __restrict__ part) {
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        acc += (double)fabsf(a[i] - b[i]);
    block_sum_to(acc, part + blockIdx.x);
}

__global__ void l1_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n,
                              const float* __restrict__ gscale, float w, float* __restrict__ da) {
    const float g = (gscale ? *gscale : 1.f) * w;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float d = a[i] - b[i];
        da[i] = d > 0.f ? g : (d < 0.f ? -g : 0.f);
    }
}

// nn.MSELoss()(a, b) between two tensors (utils.perceptual_loss, utils.py:205-206); gradient to a (and to b when db != NULL)
__global__ void mse_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n, double* __restrict__ part) {
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const double d = (double)a[i] - (double)b[i];
        acc += d * d;
    }
    block_sum_to(acc, part + blockIdx.x);
}

__global__ void mse_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n, const float* __restrict__ gscale,
                               float w, float* __restrict__ da, float* __restrict__ db) {
    const float g = (gscale ? *gscale : 1.f) * w;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float d = (a[i] - b[i]) * g;
        da[i] = d;
        if (db) db[i] = -d;
    }
}

struct WsumArgs {
    const float* t[16];
    float w[16];
    int n;
};

__global__ void weighted_sum_kernel(WsumArgs a, float* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < a.n; ++i) s += a.w[i] * (*a.t[i]);
        *out = s;
    }
}

// ---------------------------------------------------------------- Adam (torch.optim.Adam single-tensor arithmetic)
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                            __bf16* __restrict__ p16, int split, size_t n, float step_size, float omb1, float beta2, float omb2, float eps,
                            float inv_bc2_sqrt, float grad_scale) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float gi = g[i] * grad_scale;
        float mi = m[i], vi = v[i];
        mi = mi + (gi - mi) * omb1;          // exp_avg.lerp_(grad, 1 - beta1)
        vi = vi * beta2 + gi * gi * omb2;    // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        float denom = sqrtf(vi) * inv_bc2_sqrt + eps;
        const float pn = p[i] - step_size * (mi / denom);
        p[i] = pn;
        if (p16) {
            if (split) {      // the three bf16 planes of the split contraction (conv_split.hip), n elements apart
                const sscg_bf3 t = sscg_split3(pn);
                p16[i] = t.h; p16[n + i] = t.m; p16[2 * n + i] = t.l;
            } else {
                p16[i] = (__bf16)pn;       // bf16 operand copy of the fp32 master weight (RNE)
            }
        }
        m[i] = mi;
        v[i] = vi;
    }
}

}  // namespace

extern "C" int sscg_softmax_fwd(const float* x, float* y, int64_t rows, int C, void* stream) {
    if (!x || !y || rows <= 0 || C <= 0 || C > SSCG_MAXC) return SSCG_ERR_BAD_ARG;
    hipLaunchKernelGGL(softmax_fwd_kernel, dim3(ew_blocks(rows)), dim3(256), 0, (hipStream_t)stream, x, y, (size_t)rows, C);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_softmax_bwd(const float* dy, const float* y, float* dx, int64_t rows, int C, void* stream) {
    if (!dy || !y || !dx || rows <= 0 || C <= 0 || C > SSCG_MAXC) return SSCG_ERR_BAD_ARG;
    hipLaunchKernelGGL(softmax_bwd_kernel, dim3(ew_blocks(rows)), dim3(256), 0, (hipStream_t)stream, dy, y, dx, (size_t)rows, C);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_argmax_onehot(const float* x, float* onehot, int64_t* index, int64_t rows, int C, void* stream) {
    if (!x || (!onehot && !index) || rows <= 0 || C <= 0) return SSCG_ERR_BAD_ARG;
    hipLaunchKernelGGL(argmax_onehot_kernel, dim3(ew_blocks(rows)), dim3(256), 0, (hipStream_t)stream, x, onehot, index,
                       (size_t)rows, C);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_label_onehot(const int64_t* labels, float* onehot, int64_t rows, int C, void* stream) {
    if (!labels || !onehot || rows <= 0 || C <= 0) return SSCG_ERR_BAD_ARG;
    hipLaunchKernelGGL(label_onehot_kernel, dim3(ew_blocks(rows)), dim3(256), 0, (hipStream_t)stream, labels, onehot,
                       (size_t)rows, C);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

// Confusion matrix of the evaluation pass: per-block LDS histogram (int32), then integer atomics into the global
// int64 matrix - integer sums are order independent, so this is bit-exact against np.bincount.
__global__ __launch_bounds__(256) void confusion_hist_kernel(const int64_t* __restrict__ lt, const int64_t* __restrict__ lp,
                                                              int64_t n, int C, unsigned long long* __restrict__ hist) {
    extern __shared__ unsigned int bins[];
    const int nb = C * C;
    sscg_bins_clear(bins, nb);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t q = lp[i];
        if (q >= 0 && q < C) sscg_bins_count(bins, C, lt[i], (int)q);
    }
    sscg_bins_flush(bins, nb, hist);
}

extern "C" int sscg_confusion_hist(const int64_t* label_true, const int64_t* label_pred, int64_t n, int C, int64_t* hist,
                                   void* stream) {
    if (!label_true || !label_pred || !hist || n < 0 || C <= 0 || C > SSCG_MAXC) return SSCG_ERR_BAD_ARG;
    if (n == 0) return SSCG_OK;
    int64_t blocks = (n + 256 * 16 - 1) / (256 * 16);   // ~16 pixels per thread: few global atomics
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(confusion_hist_kernel, dim3((unsigned)blocks), dim3(256), (size_t)C * C * sizeof(unsigned int),
                       (hipStream_t)stream, label_true, label_pred, n, C, reinterpret_cast<unsigned long long*>(hist));
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

// Class frequencies of a label map (the input of the class-weight rules): the same scheme with C bins.
__global__ __launch_bounds__(256) void label_hist_kernel(const int64_t* __restrict__ lab, int64_t n, int C,
                                                          unsigned long long* __restrict__ counts) {
    __shared__ unsigned int bins[SSCG_MAXC];
    if (threadIdx.x < SSCG_MAXC) bins[threadIdx.x] = 0u;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t l = lab[i];
        if (l >= 0 && l < C) atomicAdd(&bins[(int)l], 1u);
    }
    __syncthreads();
    if ((int)threadIdx.x < C && bins[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)bins[threadIdx.x]);
}

extern "C" int sscg_label_hist(const int64_t* labels, int64_t n, int C, int64_t* counts, void* stream) {
    if (!labels || !counts || n < 0 || C <= 0 || C > SSCG_MAXC) return SSCG_ERR_BAD_ARG;
    if (n == 0) return SSCG_OK;
    int64_t blocks = (n + 256 * 16 - 1) / (256 * 16);   // as sscg_confusion_hist: a block's int32 bins hold at most n / blocks < 2^32 counts
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(label_hist_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, labels, n, C,
                       reinterpret_cast<unsigned long long*>(counts));
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" size_t sscg_loss_workspace(int64_t n) {
    (void)n;
    return (size_t)2 * LOSS_BLOCKS * sizeof(double);   // cross entropy keeps (sum, count) partials
}

// The plain entries and their _w twins share one implementation each.  A _w entry refuses a smoothing outside [0, 1) first; with no
// class weights and no smoothing (class_w == NULL, smoothing == 0: what the plain entry passes) the plain instantiation runs.

static int ce_fwd(const float* logits, const int64_t* labels, int64_t rows, int C, const float* class_w, float smoothing, float* loss,
                  float* valid, void* ws, size_t ws_bytes, void* stream) {
    if (!logits || !labels || !loss || rows <= 0 || C <= 0 || C > SSCG_MAXC) return SSCG_ERR_BAD_ARG;
    if (!ws || ws_bytes < sscg_loss_workspace(rows)) return SSCG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int nb = ew_blocks(rows, LOSS_BLOCKS);
    double* part = reinterpret_cast<double*>(ws);
    if (class_w || smoothing != 0.f)
        hipLaunchKernelGGL(ce_fwd_kernel<true>, dim3(nb), dim3(256), 0, st, logits, labels, (size_t)rows, C, part, nb, class_w, smoothing);
    else
        hipLaunchKernelGGL(ce_fwd_kernel<false>, dim3(nb), dim3(256), 0, st, logits, labels, (size_t)rows, C, part, nb, class_w, smoothing);
    hipLaunchKernelGGL(finish_ce_kernel, dim3(1), dim3(256), 0, st, part, nb, loss, valid);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_ce_fwd(const float* logits, const int64_t* labels, int64_t rows, int C, float* loss, float* valid,
                           void* ws, size_t ws_bytes, void* stream) {
    return ce_fwd(logits, labels, rows, C, nullptr, 0.f, loss, valid, ws, ws_bytes, stream);
}

extern "C" int sscg_ce_fwd_w(const float* logits, const int64_t* labels, int64_t rows, int C, const float* class_w, float smoothing,
                             float* loss, float* valid, void* ws, size_t ws_bytes, void* stream) {
    if (!smoothing_ok(smoothing)) return SSCG_ERR_BAD_ARG;
    return ce_fwd(logits, labels, rows, C, class_w, smoothing, loss, valid, ws, ws_bytes, stream);
}

template <bool WT>
static void launch_head(const HeadGeom& g, hipStream_t st, const float* x, const int64_t* lab, float* y_soft, float* dlo, double* part,
                        int nparts, const float* class_w, float smoothing) {
    const dim3 grid(nparts), blk(256);
    sscg_dispatch_classes(g.C, [&](auto ct) {
        hipLaunchKernelGGL((head_kernel<decltype(ct)::value, WT>), grid, blk, 0, st, x, lab, y_soft, dlo, part, nparts, g, class_w, smoothing);
    });
}

extern "C" size_t sscg_upsample_head_workspace(int N, int H, int W) {
    return (size_t)2 * (size_t)(N > 0 ? N : 0) * (size_t)(H > 0 ? H : 0) * (size_t)(W > 0 ? W : 0) * sizeof(double);
}

static int head_fwd(const float* x, const int64_t* labels, const float* class_w, float smoothing, float* y_soft, float* loss, float* valid,
                    float* dlogits, int N, int H, int W, int C, int OH, int OW, void* ws, size_t ws_bytes, void* stream) {
    HeadGeom g;
    if (!x || !head_geom(&g, N, H, W, C, OH, OW) || (!labels && !y_soft)) return SSCG_ERR_BAD_ARG;
    if (labels && (!loss || !valid || !dlogits)) return SSCG_ERR_BAD_ARG;
    if (labels && (!ws || ws_bytes < sscg_upsample_head_workspace(N, H, W))) return SSCG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int nparts = N * H * W;
    double* part = labels ? reinterpret_cast<double*>(ws) : nullptr;
    float* dlo = labels ? dlogits : nullptr;
    if (labels && (class_w || smoothing != 0.f))      // else nothing weighted to compute: the plain instantiations
        launch_head<true>(g, st, x, labels, y_soft, dlo, part, nparts, class_w, smoothing);
    else
        launch_head<false>(g, st, x, labels, y_soft, dlo, part, nparts, nullptr, 0.f);
    if (labels) hipLaunchKernelGGL(finish_ce_kernel, dim3(1), dim3(256), 0, st, part, nparts, loss, valid);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_upsample_head_fwd(const float* x, const int64_t* labels, float* y_soft, float* loss, float* valid, float* dlogits,
                                      int N, int H, int W, int C, int OH, int OW, void* ws, size_t ws_bytes, void* stream) {
    return head_fwd(x, labels, nullptr, 0.f, y_soft, loss, valid, dlogits, N, H, W, C, OH, OW, ws, ws_bytes, stream);
}

extern "C" int sscg_upsample_head_fwd_w(const float* x, const int64_t* labels, const float* class_w, float smoothing, float* y_soft,
                                        float* loss, float* valid, float* dlogits, int N, int H, int W, int C, int OH, int OW, void* ws,
                                        size_t ws_bytes, void* stream) {
    if (!smoothing_ok(smoothing)) return SSCG_ERR_BAD_ARG;
    return head_fwd(x, labels, class_w, smoothing, y_soft, loss, valid, dlogits, N, H, W, C, OH, OW, ws, ws_bytes, stream);
}

static int ce_bwd(const float* logits, const int64_t* labels, int64_t rows, int C, const float* class_w, float smoothing,
                  const float* gscale, float w, const float* valid, float* dx, void* stream) {
    if (!logits || !labels || !dx || rows <= 0 || C <= 0 || C > SSCG_MAXC) return SSCG_ERR_BAD_ARG;
    const dim3 grid(ew_blocks(rows)), blk(256);
    hipStream_t st = (hipStream_t)stream;
    if (class_w || smoothing != 0.f)
        hipLaunchKernelGGL(ce_bwd_kernel<true>, grid, blk, 0, st, logits, labels, (size_t)rows, C, gscale, w, valid, dx, class_w, smoothing);
    else
        hipLaunchKernelGGL(ce_bwd_kernel<false>, grid, blk, 0, st, logits, labels, (size_t)rows, C, gscale, w, valid, dx, class_w, smoothing);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_ce_bwd(const float* logits, const int64_t* labels, int64_t rows, int C, const float* gscale, float w,
                           const float* valid, float* dx, void* stream) {
    return ce_bwd(logits, labels, rows, C, nullptr, 0.f, gscale, w, valid, dx, stream);
}

extern "C" int sscg_ce_bwd_w(const float* logits, const int64_t* labels, int64_t rows, int C, const float* class_w, float smoothing,
                             const float* gscale, float w, const float* valid, float* dx, void* stream) {
    if (!smoothing_ok(smoothing)) return SSCG_ERR_BAD_ARG;
    return ce_bwd(logits, labels, rows, C, class_w, smoothing, gscale, w, valid, dx, stream);
}

extern "C" int sscg_mse_const_fwd(const float* x, int64_t n, float target, float* loss, void* ws, size_t ws_bytes,
                                  void* stream) {
    if (!x || !loss || n <= 0) return SSCG_ERR_BAD_ARG;
    if (!ws || ws_bytes < sscg_loss_workspace(n)) return SSCG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int nb = ew_blocks(n, LOSS_BLOCKS);
    double* part = reinterpret_cast<double*>(ws);
    hipLaunchKernelGGL(mse_const_fwd_kernel, dim3(nb), dim3(256), 0, st, x, (size_t)n, target, part);
    hipLaunchKernelGGL(finish_loss_kernel, dim3(1), dim3(256), 0, st, part, nb, 1.0 / (double)n, loss);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_mse_const_bwd(const float* x, int64_t n, float target, const float* gscale, float w, float* dx,
                                  void* stream) {
    if (!x || !dx || n <= 0) return SSCG_ERR_BAD_ARG;
    hipLaunchKernelGGL(mse_const_bwd_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, (size_t)n, target,
                       gscale, 2.f * w / (float)n, dx);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_l1_fwd(const float* a, const float* b, int64_t n, float* loss, void* ws, size_t ws_bytes, void* stream) {
    if (!a || !b || !loss || n <= 0) return SSCG_ERR_BAD_ARG;
    if (!ws || ws_bytes < sscg_loss_workspace(n)) return SSCG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int nb = ew_blocks(n, LOSS_BLOCKS);
    double* part = reinterpret_cast<double*>(ws);
    hipLaunchKernelGGL(l1_fwd_kernel, dim3(nb), dim3(256), 0, st, a, b, (size_t)n, part);
    hipLaunchKernelGGL(finish_loss_kernel, dim3(1), dim3(256), 0, st, part, nb, 1.0 / (double)n, loss);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_l1_bwd(const float* a, const float* b, int64_t n, const float* gscale, float w, float* da, void* stream) {
    if (!a || !b || !da || n <= 0) return SSCG_ERR_BAD_ARG;
    hipLaunchKernelGGL(l1_bwd_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, a, b, (size_t)n, gscale,
                       w / (float)n, da);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_mse_fwd(const float* a, const float* b, int64_t n, float* loss, void* ws, size_t ws_bytes, void* stream) {
    if (!a || !b || !loss || n <= 0) return SSCG_ERR_BAD_ARG;
    if (!ws || ws_bytes < sscg_loss_workspace(n)) return SSCG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int nb = ew_blocks(n, LOSS_BLOCKS);
    double* part = reinterpret_cast<double*>(ws);
    hipLaunchKernelGGL(mse_fwd_kernel, dim3(nb), dim3(256), 0, st, a, b, (size_t)n, part);
    hipLaunchKernelGGL(finish_loss_kernel, dim3(1), dim3(256), 0, st, part, nb, 1.0 / (double)n, loss);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_mse_bwd(const float* a, const float* b, int64_t n, const float* gscale, float w, float* da, float* db, void* stream) {
    if (!a || !b || !da || n <= 0) return SSCG_ERR_BAD_ARG;
    hipLaunchKernelGGL(mse_bwd_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, a, b, (size_t)n, gscale,
                       2.f * w / (float)n, da, db);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_weighted_sum(const float* const* terms, const float* w, int n, float* out, void* stream) {
    if (!terms || !w || !out || n <= 0 || n > 16) return SSCG_ERR_BAD_ARG;
    WsumArgs a;
    for (int i = 0; i < 16; ++i) { a.t[i] = i < n ? terms[i] : nullptr; a.w[i] = i < n ? w[i] : 0.f; }
    a.n = n;
    hipLaunchKernelGGL(weighted_sum_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a, out);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow, int shadow_dtype, int64_t n,
                              double lr, double beta1, double beta2, double eps, int step, float grad_scale, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0 || step <= 0) return SSCG_ERR_BAD_ARG;
    if (shadow && shadow_dtype != SSCG_BF16 && shadow_dtype != SSCG_BF16X3) return SSCG_ERR_BAD_ARG;
    // hyper-parameters arrive as doubles (python floats): 1 - beta must not be formed in fp32
    double bc1 = 1.0 - pow(beta1, (double)step);
    double bc2 = 1.0 - pow(beta2, (double)step);
    float step_size = (float)(lr / bc1);
    float inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    hipLaunchKernelGGL(adam_kernel, dim3(ew_blocks(n, 16384)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                       exp_avg_sq, reinterpret_cast<__bf16*>(shadow), shadow_dtype == SSCG_BF16X3 ? 1 : 0, (size_t)n, step_size, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps,
                       inv_bc2_sqrt, grad_scale);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}
