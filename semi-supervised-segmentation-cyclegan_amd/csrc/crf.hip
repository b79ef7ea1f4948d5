// Windowed dense-CRF refinement of a predicted class map (include/sscg.h: sscg_crf_head).  Forward only; the training step never
// launches it, and without `--crf` neither does anything else.
//   crf_init_kernel:      low-resolution logits (resized) or full-resolution scores -> the unary u = log-probabilities and Q0 = softmax(u)
//   crf_iter_kernel:      one mean-field step Q' = softmax(u + msg), msg_c(i) = sum over the dilated (2r+1)^2 window of k(i, j) * Q_c(j);
//                         the last step goes straight to the label maps / the confusion matrix and writes Q only when asked
//   crf_first_max_kernel: iterations == 0 on scores - the first maximum of x, nothing else
// The summation order is part of the contract: the taps are walked in row-major (dy, dx) order into ONE fp32 accumulator per class, a
// thread owns its pixel from the first tap to the label, and nothing is summed across threads - so the result depends neither on the
// tiling nor on N.
#include "common.h"
#include "crf_common.h"
#include "head_common.h"
#include "sscg_internal.h"
#include <cfloat>
#include <cmath>

namespace {

constexpr int MAX_BLOCKS = 2048;                      // crf_init / crf_first_max: 8 workgroups per CU, grid-stride beyond
constexpr int TILE = CRF_TILE, RMAX = CRF_RMAX, SIDE = CRF_SIDE, STAGE = CRF_STAGE, REACH_MAX = CRF_REACH_MAX;      // crf_common.h
constexpr int KIND_LOGITS_RESIZE = 0, KIND_LOGITS_IDENT = 1, KIND_PROBS = 2;

// u and Q0 of one output pixel.  LOGITS: u_c = (z_c - m) - logf(s), m = max z, s = sum expf(z_c - m) over c ascending; PROBS:
// u_c = logf(max(x_c, FLT_MIN)).  Q0 = softmax(u) by sscg_softmax_exp's operations.
template <int CT, int KIND>
__global__ __launch_bounds__(256) void crf_init_kernel(const float* __restrict__ x, float* __restrict__ u, float* __restrict__ q,
                                                       int total, sscg_resize_geom g) {
    const int C = CT ? CT : g.C;
    for (int o = blockIdx.x * 256 + threadIdx.x; o < total; o += gridDim.x * 256) {
        float v[CT ? CT : SSCG_MAXC];
        if (KIND == KIND_LOGITS_RESIZE) {
            const sscg_pixel p = sscg_pixel_of(o, g);
            sscg_pixel_logits<CT, false>(x, p.n, p.oy, p.ox, g.H, g.W, g.sh, g.sw, C, v);
        } else {
            sscg_pixel_logits<CT, true>(x, 0, 0, o, g.OH, g.OW, 0.f, 0.f, C, v);
        }
        if (KIND == KIND_PROBS) {
#pragma unroll
            for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
                if (CT || c < C) v[c] = logf(fmaxf(v[c], FLT_MIN));
        } else {
            float m = -INFINITY;
#pragma unroll
            for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
                if (CT || c < C) m = fmaxf(m, v[c]);
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
                if (CT || c < C) { v[c] = v[c] - m; s += expf(v[c]); }
            const float ls = logf(s);
#pragma unroll
            for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
                if (CT || c < C) v[c] = v[c] - ls;
        }
        float* up = u + (size_t)o * C;
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
            if (CT || c < C) up[c] = v[c];
        const float inv = sscg_softmax_exp<CT>(v, C);
        float* qp = q + (size_t)o * C;
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
            if (CT || c < C) qp[c] = v[c] * inv;
    }
}

// One mean-field step.  Workgroup = one TILE x TILE tile of one sample, thread = one pixel of it; the tile's halo (side x side
// pixels, `reach` beyond the tile on every side) goes through ONE LDS region of side * pitch float4:
//   1. the guide image's halo (channels zero-padded to four) - from it each thread forms the weights k[] of its own taps once, in
//      registers: both tap loops are unrolled over the (2 RT + 1)^2 grid, so every k[] index is a compile-time one.  RT = 3 (48
//      weights) serves radius <= 3, RT = 5 (120) the rest.  A tap beyond the radius or outside the map gets k = 0 (and reads the centre /
//      a Q staged as 0): it adds +0 to a non-negative accumulator, which is to skip it.  No branch per tap: a branch ends the basic
//      block, and the LDS read of every tap then waits out its latency alone (profiles/crf.txt);
//   2. then, four classes at a time, Q's halo as one float4 per pixel: a tap is one 16-byte LDS read and four multiply-adds.  msg_c is
//      independent per class, so the chunking changes no bit.  pitch % 16 == 0 keeps a wave's four rows of 16 float4 on distinct banks.
// v[] holds u and gains each chunk's msg; the softmax and (LAST) the first maximum are head_common.h's.
// LAST: q_out is nullable, the label outputs and the confusion bins as in predict_head_kernel.
template <int CT, int RT, bool LAST>
__global__ __launch_bounds__(256, (CT && RT <= 3) ? 3 : 2) void crf_iter_kernel(const float* __restrict__ u, const float* __restrict__ q_in,
                                                       const float* __restrict__ img, float* __restrict__ q_out,
                                                       int64_t* __restrict__ index, uint8_t* __restrict__ label_u8,
                                                       const int64_t* __restrict__ lt, unsigned long long* __restrict__ hist, CrfGeom g,
                                                       CrfTaps tp) {
    extern __shared__ float4 stage[];                 // [side][pitch]; LAST with hist: the [C][C] bins behind it
    constexpr int CMAX = CT ? CT : SSCG_MAXC;
    const int C = CT ? CT : g.C;
    unsigned int* bins = reinterpret_cast<unsigned int*>(stage + g.side * g.pitch);
    const int nb = (LAST && hist) ? C * C : 0;
    if (LAST) sscg_bins_clear(bins, nb);

    const int bt = fd_div((int)blockIdx.x, g.dtx);
    const int bx = (int)blockIdx.x - bt * g.tiles_x;
    const int n = fd_div(bt, g.dty);
    const int by = bt - n * g.tiles_y;
    const int tx = threadIdx.x & (TILE - 1), ty = threadIdx.x >> 4;
    const int oy = by * TILE + ty, ox = bx * TILE + tx;
    const bool inside = oy < g.OH && ox < g.OW;
    const int hy0 = by * TILE - g.reach, hx0 = bx * TILE - g.reach;
    const int npix = g.side * g.side;
    const size_t map0 = (size_t)n * g.OH * g.OW;       // the sample's first pixel

    for (int e = threadIdx.x; e < npix; e += 256) {
        const int hy = fd_div(e, g.dside), hx = e - hy * g.side;
        const int y = hy0 + hy, x = hx0 + hx;
        float4 px = make_float4(0.f, 0.f, 0.f, 0.f);
        if (y >= 0 && y < g.OH && x >= 0 && x < g.OW) {
            const float* p = img + (map0 + (size_t)y * g.OW + x) * g.IC;
            px.x = p[0];
            if (g.IC > 1) px.y = p[1];
            if (g.IC > 2) px.z = p[2];
            if (g.IC > 3) px.w = p[3];
        }
        stage[hy * g.pitch + hx] = px;
    }
    __syncthreads();

    const int centre = (ty + g.reach) * g.pitch + tx + g.reach;
    const int step_y = g.d * g.pitch, step_x = g.d;
    constexpr int KS = 2 * RT + 1;
    float k[KS * KS];
    {
        const float4 ci = stage[centre];
#pragma unroll
        for (int dy = -RT; dy <= RT; ++dy)
#pragma unroll
            for (int dx = -RT; dx <= RT; ++dx) {
                const int ring = (dy < 0 ? -dy : dy) > (dx < 0 ? -dx : dx) ? (dy < 0 ? -dy : dy) : (dx < 0 ? -dx : dx);
                if (ring != 0) {
                    const bool on = ring <= g.r;                       // uniform; a select, not a branch: see above
                    const int t = (dy + RMAX) * SIDE + dx + RMAX;
                    const int y = oy + dy * g.d, x = ox + dx * g.d;
                    const float w = crf_weight(ci, stage[on ? centre + dy * step_y + dx * step_x : centre], tp.d2a[t], tp.spatial[t], g.wb, g.ib);
                    k[(dy + RT) * KS + dx + RT] = (on && y >= 0 && y < g.OH && x >= 0 && x < g.OW) ? w : 0.f;
                }
            }
    }

    // v[] starts as the unary (loaded here, ahead of the staging that hides its latency) and receives each quad's message once
    const int o = (int)map0 + oy * g.OW + ox;
    float v[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
        if (CT || c < C) v[c] = inside ? u[(size_t)o * C + c] : 0.f;
    float* sf = reinterpret_cast<float*>(stage);
#pragma unroll
    for (int c0 = 0; c0 < CMAX; c0 += 4) {
        if (CT || c0 < C) {                            // uniform
            __syncthreads();                           // the region's previous content (the image, the quad before) has been read
            // consecutive lanes take consecutive floats of a pixel's quad, then the next pixel; STAGE loads are issued before the
            // first of them is stored, so a thread waits for memory once per batch, not once per element
            for (int e0 = threadIdx.x; e0 < npix * 4; e0 += 256 * STAGE) {
                float val[STAGE];
                int at[STAGE];
#pragma unroll
                for (int s = 0; s < STAGE; ++s) {
                    const int e = e0 + s * 256;
                    const int pe = e >> 2, j = e & 3;
                    const int hy = fd_div(pe, g.dside), hx = pe - hy * g.side;
                    const int y = hy0 + hy, x = hx0 + hx;
                    at[s] = e < npix * 4 ? (hy * g.pitch + hx) * 4 + j : -1;
                    val[s] = 0.f;
                    if (at[s] >= 0 && y >= 0 && y < g.OH && x >= 0 && x < g.OW && c0 + j < C)
                        val[s] = q_in[((int)map0 + y * g.OW + x) * C + c0 + j];          // < 2^31 elements: checked by the entry
                }
#pragma unroll
                for (int s = 0; s < STAGE; ++s)
                    if (at[s] >= 0) sf[at[s]] = val[s];
            }
            __syncthreads();
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int dy = -RT; dy <= RT; ++dy)
#pragma unroll
                for (int dx = -RT; dx <= RT; ++dx) {
                    const int ring = (dy < 0 ? -dy : dy) > (dx < 0 ? -dx : dx) ? (dy < 0 ? -dy : dy) : (dx < 0 ? -dx : dx);
                    if (ring != 0) {
                        const float kt = k[(dy + RT) * KS + dx + RT];
                        const float4 qj = stage[ring <= g.r ? centre + dy * step_y + dx * step_x : centre];
                        acc.x = fmaf(kt, qj.x, acc.x);
                        acc.y = fmaf(kt, qj.y, acc.y);
                        acc.z = fmaf(kt, qj.z, acc.z);
                        acc.w = fmaf(kt, qj.w, acc.w);
                    }
                }
            v[c0] = v[c0] + acc.x;
            if (c0 + 1 < CMAX) v[c0 + 1] = v[c0 + 1] + acc.y;
            if (c0 + 2 < CMAX) v[c0 + 2] = v[c0 + 2] + acc.z;
            if (c0 + 3 < CMAX) v[c0 + 3] = v[c0 + 3] + acc.w;
        }
    }

    if (inside) {
        const float inv = sscg_softmax_exp<CT>(v, C);
        if (q_out) {
            float* qp = q_out + (size_t)o * C;
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (CT || c < C) qp[c] = v[c] * inv;
        }
        if (LAST) {
            const int bi = sscg_first_max_scaled<CT>(v, inv, C);
            if (index) index[o] = bi;
            if (label_u8) label_u8[o] = (uint8_t)bi;
            if (hist) sscg_bins_count(bins, C, lt[o], bi);
        }
    }
    if (LAST) sscg_bins_flush(bins, nb, hist);
}

// iterations == 0 on scores: the first maximum of each pixel's C values (sscg_first_max: what sscg_predict_head_ms takes of its sum)
template <int CT>
__global__ __launch_bounds__(256) void crf_first_max_kernel(const float* __restrict__ x, int64_t* __restrict__ index,
                                                            uint8_t* __restrict__ label_u8, const int64_t* __restrict__ lt,
                                                            unsigned long long* __restrict__ hist, int total, int Crt) {
    extern __shared__ unsigned int fm_bins[];
    const int C = CT ? CT : Crt;
    const int nb = hist ? C * C : 0;
    sscg_bins_clear(fm_bins, nb);
    for (int o = blockIdx.x * 256 + threadIdx.x; o < total; o += gridDim.x * 256) {
        float v[CT ? CT : SSCG_MAXC];
        sscg_pixel_logits<CT, true>(x, 0, 0, o, 1, total, 0.f, 0.f, C, v);
        const int bi = sscg_first_max<CT>(v, C);
        if (index) index[o] = bi;
        if (label_u8) label_u8[o] = (uint8_t)bi;
        if (hist) sscg_bins_count(fm_bins, C, lt[o], bi);
    }
    sscg_bins_flush(fm_bins, nb, hist);
}

template <int CT, int RT>
void launch_iter(bool last, dim3 grid, size_t stage_lds, size_t bins_lds, hipStream_t st, const float* u, const float* q_in, const float* img,
                 float* q_out, int64_t* index, uint8_t* label_u8, const int64_t* lt, unsigned long long* hist, const CrfGeom& g,
                 const CrfTaps& tp) {
    if (last)
        hipLaunchKernelGGL((crf_iter_kernel<CT, RT, true>), grid, dim3(256), stage_lds + bins_lds, st, u, q_in, img, q_out, index, label_u8,
                           lt, hist, g, tp);
    else
        hipLaunchKernelGGL((crf_iter_kernel<CT, RT, false>), grid, dim3(256), stage_lds, st, u, q_in, img, q_out, (int64_t*)nullptr,
                           (uint8_t*)nullptr, (const int64_t*)nullptr, (unsigned long long*)nullptr, g, tp);
}

}  // namespace

extern "C" size_t sscg_crf_workspace(int N, int C, int OH, int OW, int iterations) {
    if (N <= 0 || C <= 0 || OH <= 0 || OW <= 0 || iterations <= 0) return 0;
    return 3 * (size_t)N * (size_t)OH * (size_t)OW * (size_t)C * sizeof(float);      // u and the two Q buffers
}

extern "C" int sscg_crf_head(const float* x, int kind, int N, int H, int W, int C, int OH, int OW, const float* img, int IC,
                             const sscg_crf_params* p, float* q_out, int64_t* index, uint8_t* label_u8, const int64_t* label_true,
                             int64_t* hist, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !img || !p || (kind != SSCG_CRF_LOGITS && kind != SSCG_CRF_PROBS)) return SSCG_ERR_BAD_ARG;
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C > SSCG_MAXC || OH <= 0 || OW <= 0 || IC < 1 || IC > 4) return SSCG_ERR_BAD_ARG;
    if (p->radius < 1 || p->radius > RMAX || p->dilation < 1 || p->iterations < 0) return SSCG_ERR_BAD_ARG;
    if (!crf_finite_nonneg(p->w_bilateral) || !crf_finite_nonneg(p->w_spatial)) return SSCG_ERR_BAD_ARG;             // (false for a NaN)
    float ia, ib, ig;
    if (!crf_inv_two_theta_sq(p->theta_alpha, &ia) || !crf_inv_two_theta_sq(p->theta_beta, &ib) || !crf_inv_two_theta_sq(p->theta_gamma, &ig))
        return SSCG_ERR_BAD_ARG;
    if ((!q_out && !index && !label_u8 && !hist) || (label_true == nullptr) != (hist == nullptr)) return SSCG_ERR_BAD_ARG;
    if (p->iterations == 0 && q_out) return SSCG_ERR_BAD_ARG;                    // no mean-field step, no Q
    if (kind == SSCG_CRF_PROBS && (H != OH || W != OW)) return SSCG_ERR_BAD_ARG;
    if ((int64_t)p->radius * p->dilation > REACH_MAX) return SSCG_ERR_UNSUPPORTED;
    const size_t pixels = (size_t)N * OH * OW;
    if (pixels * C >= ((size_t)1 << 31)) return SSCG_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* h = reinterpret_cast<unsigned long long*>(hist);
    const int total = (int)pixels;
    const size_t bins_lds = hist ? (size_t)C * C * sizeof(unsigned int) : 0;       // <= 16 KB

    if (p->iterations == 0) {
        if (kind == SSCG_CRF_LOGITS) return sscg_predict_head(x, N, H, W, C, OH, OW, index, label_u8, label_true, hist, stream);
        const dim3 grid(ew_blocks(pixels, MAX_BLOCKS)), blk(256);
        sscg_dispatch_classes(C, [&](auto ct) {
            hipLaunchKernelGGL(crf_first_max_kernel<decltype(ct)::value>, grid, blk, bins_lds, st, x, index, label_u8, label_true, h, total, C);
        });
        SSCG_LAUNCH_CHECK();
        return SSCG_OK;
    }
    if (!ws || ws_bytes < sscg_crf_workspace(N, C, OH, OW, p->iterations)) return SSCG_ERR_WORKSPACE;

    float* u = reinterpret_cast<float*>(ws);
    float* qa = u + pixels * C;
    float* qb = qa + pixels * C;
    {
        const sscg_resize_geom rg = sscg_make_resize_geom(H, W, C, OH, OW);
        const dim3 grid(ew_blocks(pixels, MAX_BLOCKS)), blk(256);
        const int k3 = kind == SSCG_CRF_PROBS ? KIND_PROBS : (OH == H && OW == W ? KIND_LOGITS_IDENT : KIND_LOGITS_RESIZE);
        sscg_dispatch_classes(C, [&](auto ct) {
            constexpr int CT = decltype(ct)::value;
            if (k3 == KIND_PROBS) hipLaunchKernelGGL((crf_init_kernel<CT, KIND_PROBS>), grid, blk, 0, st, x, u, qa, total, rg);
            else if (k3 == KIND_LOGITS_IDENT) hipLaunchKernelGGL((crf_init_kernel<CT, KIND_LOGITS_IDENT>), grid, blk, 0, st, x, u, qa, total, rg);
            else hipLaunchKernelGGL((crf_init_kernel<CT, KIND_LOGITS_RESIZE>), grid, blk, 0, st, x, u, qa, total, rg);
        });
        SSCG_LAUNCH_CHECK();
    }

    CrfGeom g;
    CrfTaps tp;
    crf_setup(C, OH, OW, IC, p->radius, p->dilation, p->w_bilateral, p->w_spatial, ia, ib, ig, &g, &tp);
    const size_t stage_lds = (size_t)g.side * g.pitch * sizeof(float4);             // <= 36 KB
    const dim3 grid((unsigned)((size_t)N * g.tiles_x * g.tiles_y));
    for (int it = 0; it < p->iterations; ++it) {
        const bool last = it == p->iterations - 1;
        sscg_dispatch_classes(C, [&](auto ct) {
            constexpr int CT = decltype(ct)::value;
            if (g.r <= 3) launch_iter<CT, 3>(last, grid, stage_lds, bins_lds, st, u, qa, img, last ? q_out : qb, index, label_u8, label_true, h, g, tp);
            else launch_iter<CT, RMAX>(last, grid, stage_lds, bins_lds, st, u, qa, img, last ? q_out : qb, index, label_u8, label_true, h, g, tp);
        });
        SSCG_LAUNCH_CHECK();
        float* t = qa; qa = qb; qb = t;
    }
    return SSCG_OK;
}
