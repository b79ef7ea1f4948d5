// The losses of the UNLABELLED head (include/sscg.h: sscg_unl_fwd / sscg_unl_bwd; sscg_upsample_head_bwd_u is in head_bwd.hip): entropy
// minimisation, the maximum-squares loss and the confidence-thresholded pseudo-label cross entropy of the model's own prediction.
//
// With z = resize(x) (bilinear, align_corners=True; identity sizes: z = x), per output pixel u_c = z_c - max_k z_k, s = sum_c exp(u_c),
// p = exp(u) / s, V = every pixel of the call (there is no void on this side):
//     H      = ln s - sum_c p_c u_c                           L_ent = sum H / (V ln C)          (C == 1: the divisor is V, H is 0)
//     L_msq  = -sum_o sum_c p_c^2 / (2 V)
//     y*     = the first maximum of p, conf = p[y*], KEPT <=> conf >= tau, K = the kept pixels
//     L_pl   = sum over the kept pixels of (ln s - u[y*]) / max(K, 1)
// u_c is the logit difference, held BEFORE the exponentiation: the logarithm of a vanished exp(u_c) would turn p_c u_c into 0 * -inf.
// Three steps, none of which writes the resized logits or the probabilities (dice.hip's shape):
//   1. unl_stats_kernel    one thread per OUTPUT pixel, no block straddles a sample; per block one fp64 record (sum H, sum p^2, sum of the
//                          kept cross entropies, K) in the workspace, and - asked for - the pseudo-label map: y* of a kept pixel, 255 of a
//                          dropped one.  The backward READS its labels and keep decisions there: it recomputes the logits with
//                          head_logits (head_geom.h), whose last bit may differ from the pinned arithmetic used here, and a decision
//                          re-derived from them could differ from the one K counted.
//   2. unl_reduce_kernel   (unl_rows.h) one block per sample: its records in index order;
//      unl_finish_kernel   one block: the samples in index order -> sums[4] (fp64) and the three losses (fp32).
//   3. the backward        flat (unl_bwd_kernel: one thread per pixel) or through the adjoint of the resize: the UNL term of the head's
//                          one backward kernel (head_bwd_kernel, head_bwd.hip), in the same launch as the softmax map's gradient.
// No float atomics, every sum in a fixed order: the same call twice gives the same bits.
#include "common.h"
#include "head_common.h"
#include "head_geom.h"
#include "sscg_internal.h"
#include "unl_rows.h"

namespace {

struct UnlGeom {
    sscg_resize_geom r;
    int npix;      // OH * OW: output pixels of a sample
    int bps;       // blocks (= records) per sample
    float tau;
};

// dice_stats_kernel's frame: block b serves sample b / bps, consecutive lanes on consecutive pixels of a row, every thread of the block
// makes the same number of trips (the ballot needs the whole wave; a thread past the end computes the sample's last pixel and adds
// nothing).  Per thread the three float sums of its own pixels in fp32 - a thread takes ceil(OH * OW / 65536) of them - K per WAVE by
// ballot as integers; a wave's 64 values by the fixed butterfly, the four waves in order in fp64 into the block's record.
template <int CT, bool RESIZE>
__global__ __launch_bounds__(256) void unl_stats_kernel(const float* __restrict__ x, double* __restrict__ part,
                                                        uint8_t* __restrict__ pmap, UnlGeom g) {
    __shared__ float redf[4][3];
    __shared__ int redk[4];
    const int C = CT ? CT : g.r.C;
    const int n = blockIdx.x / g.bps, blk = blockIdx.x - n * g.bps;
    const float* xn = x + (size_t)n * g.r.H * g.r.W * C;
    uint8_t* pn = pmap ? pmap + (size_t)n * g.npix : nullptr;
    float sh = 0.f, sq = 0.f, sc = 0.f;
    int kw = 0;
    for (long base = (long)blk * 256; base < g.npix; base += (long)g.bps * 256) {      // (long: npix may sit just below 2^31)
        const long o_raw = base + threadIdx.x;
        const bool in = o_raw < g.npix;
        const int o = in ? (int)o_raw : g.npix - 1;
        float v[CT ? CT : SSCG_MAXC], u[CT ? CT : SSCG_MAXC];
        const int oy = RESIZE ? fd_div(o, g.r.dow) : 0;       // the pixel within its sample: xn is the sample's map
        sscg_pixel_logits<CT, !RESIZE>(xn, 0, oy, o - oy * g.r.OW, g.r.H, g.r.W, g.r.sh, g.r.sw, C, v);
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
            if (CT || c < C) m = fmaxf(m, v[c]);
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
            if (CT || c < C) u[c] = v[c] - m;
        const float inv = sscg_softmax_exp<CT>(v, C);
        const int y = sscg_first_max_scaled<CT>(v, inv, C);
        float conf = 0.f, pu = 0.f, pp = 0.f, uy = 0.f;
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
            if (CT || c < C) {
                const float p = v[c] * inv;
                conf = fmaxf(conf, p);           // = p[y]: the value the first maximum was chosen by
                pu += p * u[c];
                pp += p * p;
                uy += c == y ? u[c] : 0.f;
            }
        const float lns = -logf(inv);            // ln s (inv = 1 / s; s = 1 gives exactly 0)
        const bool keep = in && conf >= g.tau;
        sh += in ? lns - pu : 0.f;
        sq += in ? pp : 0.f;
        sc += keep ? lns - uy : 0.f;
        kw += __popcll(__ballot(keep));
        if (in && pn) pn[o] = (uint8_t)(keep ? y : UNL_DROPPED);
    }
    const int wave = threadIdx.x >> 6;
    const float th = wave_sum(sh), tq = wave_sum(sq), tc = wave_sum(sc);
    if ((threadIdx.x & 63) == 0) { redf[wave][0] = th; redf[wave][1] = tq; redf[wave][2] = tc; redk[wave] = kw; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        double* rec = part + (size_t)blockIdx.x * 4;
        if (k < 3) rec[k] = ((double)redf[0][k] + (double)redf[1][k]) + ((double)redf[2][k] + (double)redf[3][k]);
        else rec[3] = (double)((redk[0] + redk[1]) + (redk[2] + redk[3]));
    }
}

__global__ __launch_bounds__(256) void unl_finish_kernel(const double* __restrict__ ssum, int N, double V, int C,
                                                         double* __restrict__ sums, float* __restrict__ losses) {
    __shared__ double sm[256];
    __shared__ double tot[4];
    const double t = unl_sum_rows(ssum, N, sm);
    if (threadIdx.x < 4) { tot[threadIdx.x] = t; sums[threadIdx.x] = t; }
    __syncthreads();
    if (threadIdx.x == 0) {
        losses[0] = (float)(tot[0] / (V * (C > 1 ? log((double)C) : 1.0)));
        losses[1] = (float)(-tot[1] / (2.0 * V));
        losses[2] = (float)(tot[2] / (tot[3] > 1.0 ? tot[3] : 1.0));       // K == 0: 0 / 1
    }
}

// Flat backward: one thread per pixel of full-resolution logits, grid-stride.  dx[r][c] = p_c (q_c - sum_k p_k q_k) + [r kept] kp (p_c -
// [c == y*_r]) with q_c = -ke u_c - km p_c (unl_coef, head_geom.h); the label and the keep decision are the map's byte.
template <int CT>
__global__ __launch_bounds__(256) void unl_bwd_kernel(const float* __restrict__ x, const uint8_t* __restrict__ pmap, size_t rows, int Cr,
                                                      const float* __restrict__ g_ent, const float* __restrict__ g_msq,
                                                      const float* __restrict__ g_pl, const double* __restrict__ sums,
                                                      float* __restrict__ dx) {
    const int C = CT ? CT : Cr;
    const UnlCoef k = unl_coef(g_ent, g_msq, g_pl, sums, (double)rows, C);
    for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (size_t)gridDim.x * 256) {
        const float* xr = x + r * C;
        float* dr = dx + r * C;
        const int ys = g_pl ? (int)pmap[r] : UNL_DROPPED;
        float v[CT ? CT : SSCG_MAXC], u[CT ? CT : SSCG_MAXC];
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
            if (CT || c < C) { v[c] = xr[c]; m = fmaxf(m, v[c]); }
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
            if (CT || c < C) u[c] = v[c] - m;
        const float inv = sscg_softmax_exp<CT>(v, C);
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
            if (CT || c < C) {
                v[c] *= inv;
                dot += v[c] * unl_upstream(k, u[c], v[c]);
            }
        const float kp = ys != UNL_DROPPED ? k.kp : 0.f;
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
            if (CT || c < C) dr[c] = v[c] * (unl_upstream(k, u[c], v[c]) - dot) + kp * (v[c] - (c == ys ? 1.f : 0.f));
    }
}

template <bool RESIZE>
void launch_stats(const UnlGeom& g, int N, hipStream_t st, const float* x, double* part, uint8_t* pmap) {
    const dim3 grid((unsigned)N * g.bps), blk(256);
    sscg_dispatch_classes(g.r.C, [&](auto ct) {
        hipLaunchKernelGGL((unl_stats_kernel<decltype(ct)::value, RESIZE>), grid, blk, 0, st, x, part, pmap, g);
    });
}

}  // namespace

extern "C" size_t sscg_unl_workspace(int N, int OH, int OW) {
    if (N <= 0 || OH <= 0 || OW <= 0) return 0;
    return (size_t)N * 4 * ((size_t)unl_bps(OH, OW) + 1) * sizeof(double);      // the blocks' records + the samples' sums
}

extern "C" int sscg_unl_fwd(const float* x, int N, int H, int W, int C, int OH, int OW, float thresh, float* losses, double* sums,
                            uint8_t* pseudo, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !losses || !sums || !sizes_ok(N, H, W, C, OH, OW) || !thresh_ok(thresh)) return SSCG_ERR_BAD_ARG;
    if (too_large(N, H, W, OH, OW)) return SSCG_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < sscg_unl_workspace(N, OH, OW)) return SSCG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const UnlGeom g = {sscg_make_resize_geom(H, W, C, OH, OW), OH * OW, unl_bps(OH, OW), thresh};
    double* part = reinterpret_cast<double*>(ws);
    if (OH == H && OW == W) launch_stats<false>(g, N, st, x, part, pseudo);
    else launch_stats<true>(g, N, st, x, part, pseudo);
    double* ssum = part + (size_t)N * g.bps * 4;
    hipLaunchKernelGGL(unl_reduce_kernel, dim3((unsigned)N), dim3(256), 0, st, part, g.bps, ssum);
    hipLaunchKernelGGL(unl_finish_kernel, dim3(1), dim3(256), 0, st, ssum, N, (double)N * OH * OW, C, sums, losses);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_unl_bwd(const float* x, const uint8_t* pseudo, int N, int H, int W, int C, const float* g_ent, const float* g_msq,
                            const float* g_pl, const double* sums, float* dx, void* stream) {
    if (!x || !dx || !sums || N <= 0 || H <= 0 || W <= 0 || C <= 0 || C > SSCG_MAXC) return SSCG_ERR_BAD_ARG;
    if ((!g_ent && !g_msq && !g_pl) || (g_pl && !pseudo)) return SSCG_ERR_BAD_ARG;
    if (too_large(N, H, W, H, W)) return SSCG_ERR_UNSUPPORTED;
    const size_t rows = (size_t)N * H * W;
    const dim3 grid(ew_blocks(rows)), blk(256);
    sscg_dispatch_classes(C, [&](auto ct) {
        hipLaunchKernelGGL(unl_bwd_kernel<decltype(ct)::value>, grid, blk, 0, (hipStream_t)stream, x, pseudo, rows, C, g_ent, g_msq, g_pl,
                           sums, dx);
    });
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}
