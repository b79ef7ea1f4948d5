// The backward of the fused label head (include/sscg.h: sscg_upsample_head_bwd / _bwd_d / _bwd_h / _bwd_b / _bwd_u): ONE gather kernel for every
// branch that can be live - the softmax map's upstream gradient, the cross entropy (plain or mined), the Dice loss and the boundary
// loss - through the adjoint of the resize.  One block per SOURCE pixel walks the output pixels whose stencil touches it (head_window /
// head_weight / head_logits of head_geom.h: the forward's candidates, weights and order).  Per output pixel, with p = softmax(resized
// logits):
//     q_c = dy_soft[c]   (SOFT)   + g_dice * (A[c] [y == c] + B[c])   (DICE; counted pixels: y in [0, C))
//                                 + g_bnd * k * wb_c * phi_c            (BND; counted pixels; phi = sscg_level_set(sdm[o][c]), sdm.hip)
//     d_c = p_c (q_c - sum_k p_k q_k)  +  [kept] ge ((a + bs W) p_c - a [c == y] - bs w_c)          (MINED; a = (1-eps) w_y, bs = eps / C,
//                                                                                                   ge = g_ce / D, kept: keys <= tau)
// weighted by the stencil weight and summed over the block by head_store_sum, which - !MINED - adds the cross-entropy gradient the
// forward left (dl_ce * g_ce / valid): that gradient depends on the pixel alone, the mined one on the selection, so it is formed here.
// The UNLABELLED head (sscg_upsample_head_bwd_u; the losses of unl.hip) is the same kernel without a label branch:
//     q_c = dy_soft[c]   (SOFT)   - ke u_c - km p_c                       (UNL; u_c = z_c - max z, the factors of unl_coef, head_geom.h)
//     d_c = p_c (q_c - sum_k p_k q_k)  +  [kept] kp (p_c - [c == y*])     (kept and y*: the byte of the forward's pseudo-label map)
#include "common.h"
#include "head_geom.h"
#include "sscg_internal.h"

namespace {

// SOFT / DICE / MINED: which terms the instantiation carries.  The three that serve sscg_upsample_head_bwd (SOFT alone) read no label
// and no LDS but `red`: sA / sB (the group's (A, B) rows times g_dice) are referenced under DICE only, sW (the class weights) under
// MINED only.  A MINED instantiation serves every call of sscg_upsample_head_bwd_h and so keeps its two loss branches as RUN-TIME
// tests (`dice`: coef given, `ce`: keys given) - with a branch off it still adds that branch's zero, which a compile-time flag would
// drop, and the sum's signed zeros with it.
// BND: the boundary term of sscg_upsample_head_bwd_b, on top of a MINED instantiation.  There the cross entropy is live when `valid`
// is given and mined when `keys` is given too: without keys every counted pixel is kept, which is the unmined cross entropy formed in
// the stencil (that entry takes no gradient the forward left).  Per touched pixel it reads the C contiguous int32 of sdm.
struct HeadBnd { const int32_t* sdm; const float* coef; const float* w; const float* g; };
// UNL: the entropy, max-squares and pseudo-label terms of the unlabelled head, with or without SOFT and with no label branch.  Each of
// the three is a RUN-TIME factor (0 where its upstream scalar is NULL), as the loss branches of a MINED instantiation are.
struct HeadUnl { const uint8_t* pseudo; const float* g_ent; const float* g_msq; const float* g_pl; const double* sums; };

template <int CT, bool SOFT, bool DICE, bool MINED, bool BND = false, bool UNL = false>
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ lab,
                                                       const float* __restrict__ dy_soft, const float* __restrict__ dl_ce,
                                                       const float* __restrict__ g_ce, const float* __restrict__ valid,
                                                       const float* __restrict__ coef, const float* __restrict__ g_dice, int batch,
                                                       const float* __restrict__ keys, const float* __restrict__ thr,
                                                       const float* __restrict__ class_w, float smoothing, float* __restrict__ dx, HeadGeom g,
                                                       HeadBnd bnd, HeadUnl unl) {
    static_assert(SOFT || DICE || UNL, "an instantiation with nothing to gather");
    static_assert(!UNL || !DICE, "the unlabelled head has no label branch");
    static_assert(DICE || !MINED, "the mined instantiations carry the Dice branch as a run-time test");
    static_assert(MINED || !BND, "the boundary instantiations are mined ones with one more term");
    // the run-time class count without a loss branch keeps its class loops rolled (a `break`, as head_logits): unrolled and predicated
    // that instance needs 168 registers instead of 104 and loses a wave per SIMD; the instances with a loss branch do not
    constexpr bool ROLLED = CT == 0 && !DICE;
    __shared__ float red[4][SSCG_MAXC];
    __shared__ float sA[SSCG_MAXC], sB[SSCG_MAXC], sW[SSCG_MAXC], sQ[SSCG_MAXC];
    const int C = CT ? CT : g.C;
    const int b = blockIdx.x;
    const HeadWindow win = head_window(g, b);
    const int ix = win.ix, iy = win.iy, n = win.n, oy_lo = win.oy_lo, ox_lo = win.ox_lo;
    const bool dice = DICE && (!MINED || coef != nullptr), ce = MINED && (BND ? valid != nullptr : keys != nullptr);
    float wsum = 0.f, bs = 0.f, tau = 0.f, ge = 0.f;
    if constexpr (DICE) {
        if ((int)threadIdx.x < C) {
            float qa = 0.f, qb = 0.f;
            if (dice) {
                const float gd = g_dice ? *g_dice : 1.f;
                const float* q = coef + ((size_t)(batch ? 0 : n) * C + threadIdx.x) * 2;
                qa = gd * q[0]; qb = gd * q[1];
            }
            sA[threadIdx.x] = qa; sB[threadIdx.x] = qb;
            if constexpr (MINED) sW[threadIdx.x] = class_weight(class_w, threadIdx.x);
            if constexpr (BND) sQ[threadIdx.x] = (bnd.g ? *bnd.g : 1.f) * *bnd.coef * class_weight(bnd.w, threadIdx.x);
        }
        __syncthreads();
    }
    if constexpr (MINED) {
        for (int c = 0; c < C; ++c) wsum += sW[c];
        bs = smoothing / (float)C;
        if (ce) {
            const float nv = *valid;
            if constexpr (BND) tau = keys ? *thr : 0.f;
            else tau = *thr;
            ge = (g_ce ? *g_ce : 1.f) * (nv > 0.f ? 1.f / nv : 0.f);
        }
    }
    UnlCoef uk = {0.f, 0.f, 0.f};
    if constexpr (UNL) uk = unl_coef(unl.g_ent, unl.g_msq, unl.g_pl, unl.sums, (double)g.N * g.OH * g.OW, C);
    const int nx = win.ox_hi - ox_lo + 1, cand = (win.oy_hi - oy_lo + 1) * nx;
    const float* xn = x + (size_t)n * g.H * g.W * C;
    float acc[CT ? CT : SSCG_MAXC];
#pragma unroll
    for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c) acc[c] = 0.f;
    for (int t = threadIdx.x; t < cand; t += 256) {
        const int oy = oy_lo + t / nx, ox = ox_lo + t % nx;
        const float wy = head_weight(g.sh, oy, iy, g.H);
        if (wy == 0.f) continue;
        const float wx = head_weight(g.sw, ox, ix, g.W);
        if (wx == 0.f) continue;
        const float w = wy * wx;
        const size_t o = ((size_t)n * g.OH + oy) * g.OW + ox;
        int l = -1;
        if (MINED ? lab != nullptr : DICE) {
            const int64_t l64 = lab[o];
            l = (l64 < 0 || l64 >= C) ? -1 : (int)l64;
        }
        bool kept;
        if constexpr (BND) kept = ce && l >= 0 && (keys == nullptr || keys[o] <= tau);
        else kept = ce && l >= 0 && keys[o] <= tau;
        const bool dq = dice && l >= 0;
        if constexpr (!UNL)
            if (!SOFT && !kept && !dq && !(BND && l >= 0)) continue;     // nothing flows through this pixel
        float v[CT ? CT : SSCG_MAXC];
        int y0, x0;
        head_logits<CT>(xn, g, oy, ox, C, v, &y0, &x0);
        // UNL: u_c = z_c - max z, HELD beside v and acc before v becomes exp(u_c) (the register tables: profiles/unl.txt)
        float u[UNL ? (CT ? CT : SSCG_MAXC) : 1];
        int ys = UNL_DROPPED;
        if constexpr (UNL) {
            float m = -INFINITY;
#pragma unroll
            for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c) {
                if (ROLLED && c >= C) break;
                if (CT || c < C) m = fmaxf(m, v[c]);
            }
#pragma unroll
            for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c) {
                if (ROLLED && c >= C) break;
                if (CT || c < C) u[c] = v[c] - m;
            }
            if (unl.g_pl) ys = unl.pseudo[o];
        }
        const float inv = sscg_softmax_exp<CT>(v, C);
        const float* gr = SOFT ? dy_soft + o * C : nullptr;
        // The boundary term of q_c is used twice per class.  HOLD: formed once and held in registers.  Beside v and acc that costs the
        // instantiations of 20 / 21 classes without dy_soft (the training step's) their second wave per SIMD - 290 registers against
        // 254 - so those form it where it is used instead: the second read of sdm hits the cache (measured: profiles/boundary_loss.txt).
        constexpr bool HOLD = BND && !(CT >= 16 && !SOFT);
        const int32_t* sr = BND ? bnd.sdm + o * C : nullptr;
        float qb[HOLD ? (CT ? CT : SSCG_MAXC) : 1];
        if constexpr (HOLD) {
#pragma unroll
            for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
                if (CT || c < C) qb[c] = l >= 0 ? sQ[c] * sscg_level_set(sr[c]) : 0.f;
        }
        const auto upstream = [&](int c) {           // q_c
            if constexpr (UNL) {
                const float q = unl_upstream(uk, u[c], v[c]);
                if constexpr (SOFT) return q + gr[c];
                else return q;
            } else if constexpr (!DICE) return gr[c];
            else {
                float q = dq ? (c == l ? sA[c] : 0.f) + sB[c] : 0.f;
                if constexpr (HOLD) q += qb[c];
                else if constexpr (BND) q += l >= 0 ? sQ[c] * sscg_level_set(sr[c]) : 0.f;
                if constexpr (SOFT) return q + gr[c];
                else return q;
            }
        };
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c) {
            if (ROLLED && c >= C) break;
            if (CT || c < C) {
                v[c] *= inv;
                dot += v[c] * upstream(c);
            }
        }
        float a = 0.f, gk = 0.f, k = 0.f;
        if constexpr (MINED) {
            a = kept ? (1.f - smoothing) * sW[l] : 0.f;
            gk = kept ? ge : 0.f;
            k = a + bs * wsum;
        }
        const float kpl = UNL && ys != UNL_DROPPED ? uk.kp : 0.f;       // the kept pixel's pseudo-label cross entropy
        const auto mined = [&](int c) { return gk * (v[c] * k - (c == l ? a : 0.f) - bs * sW[c]); };      // the kept pixel's cross entropy
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c) {
            if (ROLLED && c >= C) break;
            if (CT || c < C) {
                float d = v[c] * (upstream(c) - dot);
                if constexpr (MINED) d += mined(c);
                if constexpr (UNL) d += kpl * (v[c] - (c == ys ? 1.f : 0.f));
                acc[c] += w * d;
            }
        }
    }
    head_store_sum<CT>(acc, red, C, b, (MINED || UNL) ? nullptr : dl_ce, g_ce, valid, dx);
}

// backward of the cross entropy alone: dx = dl * g / valid
__global__ void head_scale_kernel(const float* __restrict__ dl, const float* __restrict__ g_ce, const float* __restrict__ valid,
                                  float* __restrict__ dx, size_t n) {
    const float nv = valid ? *valid : 0.f;
    const float k = (g_ce ? *g_ce : 1.f) * (nv > 0.f ? 1.f / nv : 0.f);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dx[i] = dl[i] * k;
}

// dice / mined: the entry's branches; SOFT follows dy_soft.  The argument order is the kernel's.
void launch_head_bwd(const HeadGeom& g, hipStream_t st, bool dice, bool mined, const float* x, const int64_t* lab, const float* dy_soft,
                     const float* dl_ce, const float* g_ce, const float* valid, const float* coef, const float* g_dice, int batch,
                     const float* keys, const float* thr, const float* class_w, float smoothing, float* dx, const HeadBnd& bnd = HeadBnd()) {
    const HeadUnl unl = HeadUnl();
    const dim3 grid((unsigned)(g.N * g.H * g.W)), blk(256);
    sscg_dispatch_classes(g.C, [&](auto ct) {
        constexpr int CT = decltype(ct)::value;
        const auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, blk, 0, st, x, lab, dy_soft, dl_ce, g_ce, valid, coef, g_dice, batch, keys, thr, class_w, smoothing, dx, g, bnd, unl);
        };
        if (bnd.sdm) dy_soft ? go(head_bwd_kernel<CT, true, true, true, true>) : go(head_bwd_kernel<CT, false, true, true, true>);
        else if (mined) dy_soft ? go(head_bwd_kernel<CT, true, true, true>) : go(head_bwd_kernel<CT, false, true, true>);
        else if (dice) dy_soft ? go(head_bwd_kernel<CT, true, true, false>) : go(head_bwd_kernel<CT, false, true, false>);
        else go(head_bwd_kernel<CT, true, false, false>);
    });
}

// the unlabelled head: SOFT follows dy_soft, every label argument is absent
void launch_head_bwd_unl(const HeadGeom& g, hipStream_t st, const float* x, const float* dy_soft, float* dx, const HeadUnl& unl) {
    const dim3 grid((unsigned)(g.N * g.H * g.W)), blk(256);
    sscg_dispatch_classes(g.C, [&](auto ct) {
        constexpr int CT = decltype(ct)::value;
        const auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, blk, 0, st, x, (const int64_t*)nullptr, dy_soft, (const float*)nullptr, (const float*)nullptr,
                               (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, 0, (const float*)nullptr,
                               (const float*)nullptr, (const float*)nullptr, 0.f, dx, g, HeadBnd(), unl);
        };
        dy_soft ? go(head_bwd_kernel<CT, true, false, false, false, true>) : go(head_bwd_kernel<CT, false, false, false, false, true>);
    });
}

}  // namespace

extern "C" int sscg_upsample_head_bwd(const float* x, const float* dy_soft, const float* dlogits, const float* g_ce, const float* valid,
                                      float* dx, int N, int H, int W, int C, int OH, int OW, void* stream) {
    HeadGeom g;
    if (!x || !dx || !head_geom(&g, N, H, W, C, OH, OW) || (!dy_soft && !dlogits)) return SSCG_ERR_BAD_ARG;
    if (dlogits && !valid) return SSCG_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (dy_soft)
        launch_head_bwd(g, st, false, false, x, nullptr, dy_soft, dlogits, g_ce, valid, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0.f, dx);
    else {
        const size_t n = (size_t)N * H * W * C;
        hipLaunchKernelGGL(head_scale_kernel, dim3(ew_blocks(n)), dim3(256), 0, st, dlogits, g_ce, valid, dx, n);
    }
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_upsample_head_bwd_d(const float* x, const int64_t* labels, const float* dy_soft, const float* dlogits,
                                        const float* g_ce, const float* valid, const float* coef, const float* g_dice, int batch,
                                        float* dx, int N, int H, int W, int C, int OH, int OW, void* stream) {
    if (!x || !labels || !coef || !dx || !sizes_ok(N, H, W, C, OH, OW)) return SSCG_ERR_BAD_ARG;
    if ((batch != 0 && batch != 1) || (dlogits && !valid)) return SSCG_ERR_BAD_ARG;
    if (too_large(N, H, W, OH, OW)) return SSCG_ERR_UNSUPPORTED;
    HeadGeom g;
    if (!head_geom(&g, N, H, W, C, OH, OW)) return SSCG_ERR_BAD_ARG;
    launch_head_bwd(g, (hipStream_t)stream, true, false, x, labels, dy_soft, dlogits, g_ce, valid, coef, g_dice, batch, nullptr, nullptr, nullptr,
                    0.f, dx);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_upsample_head_bwd_h(const float* x, const int64_t* labels, const float* keys, const float* thr, const float* class_w,
                                        float smoothing, const float* dy_soft, const float* g_ce, const float* valid, const float* coef,
                                        const float* g_dice, int batch, float* dx, int N, int H, int W, int C, int OH, int OW,
                                        void* stream) {
    if (!x || !dx || !sizes_ok(N, H, W, C, OH, OW) || (!keys && !dy_soft && !coef)) return SSCG_ERR_BAD_ARG;
    if ((keys && (!thr || !valid)) || ((keys || coef) && !labels)) return SSCG_ERR_BAD_ARG;
    if (!smoothing_ok(smoothing) || (batch != 0 && batch != 1)) return SSCG_ERR_BAD_ARG;
    if (too_large(N, H, W, OH, OW)) return SSCG_ERR_UNSUPPORTED;
    HeadGeom g;
    if (!head_geom(&g, N, H, W, C, OH, OW)) return SSCG_ERR_BAD_ARG;
    launch_head_bwd(g, (hipStream_t)stream, true, true, x, labels, dy_soft, nullptr, g_ce, valid, coef, g_dice, batch, keys, thr, class_w, smoothing,
                    dx);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_upsample_head_bwd_b(const float* x, const int64_t* labels, const float* keys, const float* thr, const float* class_w,
                                        float smoothing, const float* dy_soft, const float* g_ce, const float* valid, const float* coef,
                                        const float* g_dice, int batch, float* dx, int N, int H, int W, int C, int OH, int OW,
                                        const int32_t* sdm, const float* bnd_coef, const float* bnd_w, const float* g_bnd, void* stream) {
    if (!sdm) {
        // the unmined cross entropy exists in the boundary instantiations only: here it would be dropped without a word
        if (!keys && valid) return SSCG_ERR_BAD_ARG;
        return sscg_upsample_head_bwd_h(x, labels, keys, thr, class_w, smoothing, dy_soft, g_ce, valid, coef, g_dice, batch, dx, N, H, W, C,
                                        OH, OW, stream);
    }
    if (!x || !dx || !labels || !bnd_coef || !sizes_ok(N, H, W, C, OH, OW)) return SSCG_ERR_BAD_ARG;
    if (keys && (!thr || !valid)) return SSCG_ERR_BAD_ARG;
    if (!smoothing_ok(smoothing) || (batch != 0 && batch != 1)) return SSCG_ERR_BAD_ARG;
    if (too_large(N, H, W, OH, OW)) return SSCG_ERR_UNSUPPORTED;
    const uint64_t ey = (uint64_t)(OH - 1), ex = (uint64_t)(OW - 1);
    if (ey * ey + ex * ex >= ((uint64_t)1 << 30)) return SSCG_ERR_UNSUPPORTED;      // sscg_sdm's range
    HeadGeom g;
    if (!head_geom(&g, N, H, W, C, OH, OW)) return SSCG_ERR_BAD_ARG;
    const HeadBnd bnd = {sdm, bnd_coef, bnd_w, g_bnd};
    launch_head_bwd(g, (hipStream_t)stream, true, true, x, labels, dy_soft, nullptr, g_ce, valid, coef, g_dice, batch, keys, thr, class_w, smoothing,
                    dx, bnd);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_upsample_head_bwd_u(const float* x, const uint8_t* pseudo, const float* dy_soft, const float* g_ent, const float* g_msq,
                                        const float* g_pl, const double* sums, float* dx, int N, int H, int W, int C, int OH, int OW,
                                        void* stream) {
    // no loss received a gradient: the plain head's backward itself (the same kernels, the same bits)
    if (!g_ent && !g_msq && !g_pl) return sscg_upsample_head_bwd(x, dy_soft, nullptr, nullptr, nullptr, dx, N, H, W, C, OH, OW, stream);
    if (!x || !dx || !sums || !sizes_ok(N, H, W, C, OH, OW) || (g_pl && !pseudo)) return SSCG_ERR_BAD_ARG;
    if (too_large(N, H, W, OH, OW)) return SSCG_ERR_UNSUPPORTED;
    HeadGeom g;
    if (!head_geom(&g, N, H, W, C, OH, OW)) return SSCG_ERR_BAD_ARG;
    const HeadUnl unl = {pseudo, g_ent, g_msq, g_pl, sums};
    launch_head_bwd_unl(g, (hipStream_t)stream, x, dy_soft, dx, unl);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}
