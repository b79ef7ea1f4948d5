// Soft Dice loss of the segmentation head (include/sscg.h: sscg_dice_fwd / sscg_dice_bwd; sscg_upsample_head_bwd_d is in head_bwd.hip).
//
// With p = softmax_C(resize(z)) (bilinear, align_corners=True; identity sizes: p = softmax_C(z)), a pixel COUNTED when its label y lies
// in [0, C), groups g = the samples (batch == 0) or the whole call (batch == 1), and over the counted pixels of a group
//     I[c] = sum p_c [y == c]     P[c] = sum p_c     T[c] = sum [y == c]
//     dice[g][c] = (2 I + s) / (P + T + s)          loss = 1 - sum_{g,c} w_c dice[g][c] / (G sum_c w_c)
// Unlike the cross entropy, whose gradient depends on the pixel alone (so the head's forward leaves it), Dice couples every pixel of a
// group through the three sums.  Three steps, none of which writes the resized logits or probabilities:
//   1. dice_stats_kernel   one thread per OUTPUT pixel (1x the work, not the stencil's 4x), no block straddles a sample; per block one
//                          fp64 record [C][3] = (I, P, T) in the workspace - no float atomics, every sum in a fixed order;
//   2. dice_reduce_kernel  one block per (sample, class): the sample's records in index order -> its (I, P, T);
//      dice_finish_kernel  one block, tiny: per group the samples in index order -> sums, the loss, and the table (A, B) per (group,
//                          class) with d loss / d p_c = A [y == c] + B at a counted pixel (A = -2 k / Den, B = k Num / Den^2,
//                          k = w_c / (G sum w)).  (One block per GROUP over the records was measured first: with batch == 1 a single
//                          block then reads every record - 1-2 MB at the step's sizes - and cost more than the statistics.)
//   3. the backward        flat (dice_bwd_kernel: one thread per pixel) or through the adjoint of the resize: the DICE term of the
//                          head's one backward kernel (head_bwd_kernel, head_bwd.hip: sscg_upsample_head_bwd_d) - one block per SOURCE
//                          pixel gathers its stencil, and the softmax-output and cross-entropy branches ride in the same launch.
#include "common.h"
#include "head_common.h"
#include "head_geom.h"
#include "sscg_internal.h"

namespace {

constexpr int DICE_BLOCKS = 256;   // statistics blocks per sample, grid-stride beyond: bounds the records the finish step reads

struct DiceGeom {
    sscg_resize_geom r;
    int npix;      // OH * OW: output pixels of a sample
    int bps;       // blocks (= records) per sample
};

// One thread per output pixel of ONE sample (block b serves sample b / bps), consecutive lanes on consecutive pixels of a row.  The
// pixel's C logits live in registers (RESIZE: interpolated from the four source rows by the pinned arithmetic of head_common.h - the
// bits sscg_upsample_bilinear_fwd stores; !RESIZE: the row itself), then sscg_softmax_exp.  Per thread P[c] and I[c] (by select) are
// fp32 sums of its own pixels - a thread takes ceil(OH * OW / 65536) of them - and T[c] is counted per WAVE by ballot: wave-uniform
// integers, no vector register.  A wave's 64 values are summed in fp32 (fixed butterfly order), everything above it in fp64: the four
// waves of the block in order into the block's record, the records in index order in dice_reduce_kernel.
template <int CT, bool RESIZE>
__global__ __launch_bounds__(256) void dice_stats_kernel(const float* __restrict__ x, const int64_t* __restrict__ lab,
                                                         double* __restrict__ part, DiceGeom g) {
    __shared__ float redf[4][2 * SSCG_MAXC];
    __shared__ int redt[4][SSCG_MAXC];
    const int C = CT ? CT : g.r.C;
    const int n = blockIdx.x / g.bps, blk = blockIdx.x - n * g.bps;
    const float* xn = x + (size_t)n * g.r.H * g.r.W * C;
    const int64_t* ln = lab + (size_t)n * g.npix;
    float P[CT ? CT : SSCG_MAXC], I[CT ? CT : SSCG_MAXC];
    int T[CT ? CT : SSCG_MAXC];
#pragma unroll
    for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c) { P[c] = 0.f; I[c] = 0.f; T[c] = 0; }
    // every thread of the block makes the same number of trips (the ballots below need the whole wave): a thread past the end
    // computes the sample's last pixel and adds nothing
    for (long base = (long)blk * 256; base < g.npix; base += (long)g.bps * 256) {      // (long: npix may sit just below 2^31)
        const long o_raw = base + threadIdx.x;
        const bool in = o_raw < g.npix;
        const int o = in ? (int)o_raw : g.npix - 1;
        float v[CT ? CT : SSCG_MAXC];
        const int oy = RESIZE ? fd_div(o, g.r.dow) : 0;       // the pixel within its sample: xn is the sample's map
        sscg_pixel_logits<CT, !RESIZE>(xn, 0, oy, o - oy * g.r.OW, g.r.H, g.r.W, g.r.sh, g.r.sw, C, v);
        const int64_t l64 = ln[o];
        const int l = (in && l64 >= 0 && l64 < C) ? (int)l64 : -1;
        const float inv = sscg_softmax_exp<CT>(v, C);
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
            if (CT || c < C) {
                const float p = v[c] * inv;
                P[c] += l >= 0 ? p : 0.f;
                I[c] += c == l ? p : 0.f;
                T[c] += __popcll(__ballot(c == l));
            }
    }
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
        if (CT || c < C) {
            const float sp = wave_sum(P[c]), si = wave_sum(I[c]);
            if ((threadIdx.x & 63) == 0) { redf[wave][c] = si; redf[wave][SSCG_MAXC + c] = sp; redt[wave][c] = T[c]; }
        }
    __syncthreads();
    if ((int)threadIdx.x < C) {
        const int c = threadIdx.x;
        double* rec = part + ((size_t)blockIdx.x * C + c) * 3;
        rec[0] = ((double)redf[0][c] + (double)redf[1][c]) + ((double)redf[2][c] + (double)redf[3][c]);
        rec[1] = ((double)redf[0][SSCG_MAXC + c] + (double)redf[1][SSCG_MAXC + c]) + ((double)redf[2][SSCG_MAXC + c] + (double)redf[3][SSCG_MAXC + c]);
        rec[2] = (double)((redt[0][c] + redt[1][c]) + (redt[2][c] + redt[3][c]));
    }
}

// The records of one (sample, class) -> that sample's (I, P, T) for the class: one block each, the three columns summed by 85 row lanes
// (lane r takes records r, r + 85, ... in order; bps <= 256: at most four each), the lanes in order by the column's first thread.
__global__ __launch_bounds__(256) void dice_reduce_kernel(const double* __restrict__ part, int bps, int C, double* __restrict__ ssum) {
    __shared__ double sm[256];
    const int n = blockIdx.x / C, c = blockIdx.x - n * C;
    const int k = threadIdx.x % 3, rl = threadIdx.x / 3;         // 85 lanes of three threads; thread 255 idles
    const double* pc = part + ((size_t)n * bps * C + c) * 3 + k;
    double s = 0.0;
    if (rl < 85)
        for (int r = rl; r < bps; r += 85) s += pc[(size_t)r * C * 3];
    sm[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < 3) {
        double t = 0.0;
        for (int r = 0; r < 85; ++r) t += sm[r * 3 + k];
        ssum[(size_t)blockIdx.x * 3 + k] = t;
    }
}

// One block for the whole call - G * C <= N * 64 ratios: the tiny step.  Per (group, class) the group's samples are added in index
// order (batch == 0: the sample itself), then sums (fp64), the (A, B) table (fp32) and the term k_c * dice[g][c]; the terms are summed
// in a fixed order (thread t takes t, t + 256, ..., thread 0 the 256 lane sums) into the loss.
__global__ __launch_bounds__(256) void dice_finish_kernel(const double* __restrict__ ssum, int N, int G, int C,
                                                          const float* __restrict__ class_w, double smooth, double* __restrict__ sums,
                                                          float* __restrict__ coef, float* __restrict__ loss) {
    __shared__ double sm[256];
    double wsum = 0.0;
    for (int c = 0; c < C; ++c) wsum += (double)(class_w ? class_w[c] : 1.f);
    const double kden = wsum > 0.0 ? 1.0 / ((double)G * wsum) : 0.0;      // (sum w == 0 is refused by the host: no NaN here either)
    const int per = G == 1 ? N : 1;               // samples per group
    double lsum = 0.0;
    for (int i = threadIdx.x; i < G * C; i += 256) {
        const int g = i / C, c = i - g * C;
        double si = 0.0, sp = 0.0, st = 0.0;
        for (int n = g * per; n < (g + 1) * per; ++n) {
            const double* q = ssum + ((size_t)n * C + c) * 3;
            si += q[0]; sp += q[1]; st += q[2];
        }
        const double num = 2.0 * si + smooth, den = sp + st + smooth;
        const double k = (double)(class_w ? class_w[c] : 1.f) * kden;
        if (sums) {
            double* o = sums + (size_t)i * 3;
            o[0] = si; o[1] = sp; o[2] = st;
        }
        coef[(size_t)i * 2] = (float)(-2.0 * k / den);
        coef[(size_t)i * 2 + 1] = (float)(k * num / (den * den));
        lsum += k * (num / den);
    }
    sm[threadIdx.x] = lsum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int r = 0; r < 256; ++r) t += sm[r];
        *loss = (float)(wsum > 0.0 ? 1.0 - t : 0.0);
    }
}

// Flat backward: dx[r][c] = scale * p_c (g_c - sum_k p_k g_k) with g_c = A[c] [y == c] + B[c] of the pixel's group; a zero row for a
// pixel that is not counted.  One thread per pixel; the (A, B) rows are a handful of cache lines every lane of a wave shares.
template <int CT>
__global__ __launch_bounds__(256) void dice_bwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ lab, size_t rows,
                                                       int Cr, int per_group, const float* __restrict__ coef,
                                                       const float* __restrict__ gscale, float w, float* __restrict__ dx) {
    const int C = CT ? CT : Cr;
    const float scale = (gscale ? *gscale : 1.f) * w;
    for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (size_t)gridDim.x * 256) {
        const int64_t l64 = lab[r];
        float* dr = dx + r * C;
        if (l64 < 0 || l64 >= C) {
#pragma unroll
            for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
                if (CT || c < C) dr[c] = 0.f;
            continue;
        }
        const int l = (int)l64;
        const float* xr = x + r * C;
        const float* q = coef + (per_group ? (r / (size_t)per_group) : 0) * C * 2;
        float v[CT ? CT : SSCG_MAXC];
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
            if (CT || c < C) v[c] = xr[c];
        const float inv = sscg_softmax_exp<CT>(v, C);
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
            if (CT || c < C) {
                v[c] *= inv;
                dot += v[c] * ((c == l ? q[2 * c] : 0.f) + q[2 * c + 1]);
            }
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
            if (CT || c < C) dr[c] = scale * (v[c] * (((c == l ? q[2 * c] : 0.f) + q[2 * c + 1]) - dot));
    }
}

int dice_bps(int OH, int OW) {
    const long npix = (long)OH * OW;
    const long b = (npix + 255) / 256;
    return (int)(b > DICE_BLOCKS ? DICE_BLOCKS : b);
}

template <bool RESIZE>
void launch_stats(const DiceGeom& g, int N, hipStream_t st, const float* x, const int64_t* lab, double* part) {
    const dim3 grid((unsigned)N * g.bps), blk(256);
    sscg_dispatch_classes(g.r.C, [&](auto ct) {
        hipLaunchKernelGGL((dice_stats_kernel<decltype(ct)::value, RESIZE>), grid, blk, 0, st, x, lab, part, g);
    });
}

}  // namespace

extern "C" size_t sscg_dice_workspace(int N, int OH, int OW, int C) {
    if (N <= 0 || OH <= 0 || OW <= 0 || C <= 0) return 0;
    return (size_t)N * (size_t)C * (3 * (size_t)dice_bps(OH, OW) + 3) * sizeof(double);      // the blocks' records + the samples' sums
}

extern "C" int sscg_dice_fwd(const float* x, const int64_t* labels, int N, int H, int W, int C, int OH, int OW, const float* class_w,
                             float smooth, int batch, float* loss, double* sums, float* coef, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !labels || !loss || !coef || !sizes_ok(N, H, W, C, OH, OW)) return SSCG_ERR_BAD_ARG;
    if (!(smooth > 0.f) || smooth > 3.0e38f || (batch != 0 && batch != 1)) return SSCG_ERR_BAD_ARG;      // (false for a NaN)
    if (too_large(N, H, W, OH, OW)) return SSCG_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < sscg_dice_workspace(N, OH, OW, C)) return SSCG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const DiceGeom g = {sscg_make_resize_geom(H, W, C, OH, OW), OH * OW, dice_bps(OH, OW)};
    double* part = reinterpret_cast<double*>(ws);
    if (OH == H && OW == W) launch_stats<false>(g, N, st, x, labels, part);
    else launch_stats<true>(g, N, st, x, labels, part);
    double* ssum = part + (size_t)N * g.bps * C * 3;
    hipLaunchKernelGGL(dice_reduce_kernel, dim3((unsigned)N * C), dim3(256), 0, st, part, g.bps, C, ssum);
    hipLaunchKernelGGL(dice_finish_kernel, dim3(1), dim3(256), 0, st, ssum, N, batch ? 1 : N, C, class_w, (double)smooth, sums, coef, loss);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_dice_bwd(const float* x, const int64_t* labels, int N, int H, int W, int C, const float* coef, int batch,
                             const float* g, float w, float* dx, void* stream) {
    if (!x || !labels || !coef || !dx || N <= 0 || H <= 0 || W <= 0 || C <= 0 || C > SSCG_MAXC) return SSCG_ERR_BAD_ARG;
    if (batch != 0 && batch != 1) return SSCG_ERR_BAD_ARG;
    if (too_large(N, H, W, H, W)) return SSCG_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const size_t rows = (size_t)N * H * W;
    const int per_group = batch ? 0 : H * W;
    const dim3 grid(ew_blocks(rows)), blk(256);
    sscg_dispatch_classes(C, [&](auto ct) {
        hipLaunchKernelGGL(dice_bwd_kernel<decltype(ct)::value>, grid, blk, 0, st, x, labels, rows, C, per_group, coef, g, w, dx);
    });
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}
