// Calibration scores of the evaluation (include/sscg.h: sscg_calib_stats): the counts behind the expected / maximum calibration error
// over a reliability diagram, the per-class confidence gap, the negative log-likelihood and the Brier score of the probabilities the
// inference heads take their labels from - at up to 8 temperatures in one pass, so that the NLL-optimal temperature can be read off.
// Forward only; the training step never launches it.
//
// Per COUNTED output pixel (label in [0, C): sscg_confusion_hist's rule) and per temperature t = 0 .. NT-1, in that order:
//     z      = the resized logits (head_common.h: the pinned stencil; identity sizes: the pixel's own logits)
//     v_c    = z_c * inv_temps[t]            one fp32 multiply, rounded on its own (it may not contract into the softmax's subtraction):
//                                            inv_temps[t] == 1.f leaves the bits sscg_predict_head sees
//     p_c    = softmax(v)_c                  sscg_softmax_exp, then v_c * inv: the values softmax_fwd_kernel stores
//              (scores, kind == 1: p_c = x_c * scale, one fp32 multiply, no softmax)
//     pred   = the first maximum of p, conf = p[pred], hit = pred == label
//     b      = min(B - 1, (int)(conf * (float)B)),  q = (int64)(conf * 2^24)       (Q24: confidence sums are integers)
//     bins[t][b] += (1, hit, q)   cls[t][pred] += (1, hit, q)   sums[t] += (-log(max((double)p[label], 2^-126)), sum_c ((double)p_c - [c == label])^2)
// Two launches:
//   1. calib_stats_kernel  one thread per output pixel, grid-stride: at most CALIB_BLOCKS = 512 workgroups of 256 threads, so a thread
//                          owns ceil(N OH OW / 131072) pixels.  Integers: per-workgroup LDS bins of 64 bits - (count | hits << 32) and
//                          the Q24 sum, which 256 pixels of confidence 1 already carry past 32 bits - flushed with one 64-bit atomic per
//                          value of a bin that was hit.  fp64: a thread's own pixels in loop order into its LDS slot, a wave's 64 slots by
//                          the fixed butterfly, the four waves in order: one record of NT x 2 doubles per workgroup in the workspace.
//   2. calib_finish_kernel one block: the records in index order, the call's total added to sums.
// Integer sums do not depend on the order; the fp64 sums have no atomics and a fixed order: the same call twice gives the same bits.
#include "common.h"
#include "head_common.h"
#include "head_geom.h"
#include "sscg_internal.h"

namespace {

constexpr int CALIB_BLOCKS = 512;     // the grid cap: 2 workgroups per CU, grid-stride beyond; bounds the records and the bins flushed
constexpr int CALIB_MAXT = 8;         // temperatures of a call
constexpr int CALIB_MAXB = 32;        // confidence bins

enum { CALIB_RESIZE = 0, CALIB_IDENT = 1, CALIB_SCORES = 2 };

struct CalibArgs {
    sscg_resize_geom r;
    int total;                 // N * OH * OW
    int NT, B;
    float fB;                  // (float)B
    float scale;               // kind == 1: the factor of the scores
    float it[CALIB_MAXT];      // the inverse temperatures
};

// z * inv_t as a value of its own: the product is what the separate passes store before the softmax reads it
__device__ __forceinline__ float calib_scaled(float z, float it) {
#pragma clang fp contract(off)
    const float v = z * it;
    return v;
}

// LDS: [NT][B + C][2] 64-bit bins (row r < B: confidence bin r; row B + c: predicted class c; word 0 = count | hits << 32, word 1 = the
// Q24 sum), then [NT * 2][256] doubles, a slot per thread for (nll, brier) of every temperature.  A workgroup counts at most
// ceil(2^31 / (512 * 256)) * 256 = 2^22 pixels: count and hits stay below 2^32, a Q24 sum below 2^47.
template <int CT, int MODE>
__global__ __launch_bounds__(256) void calib_stats_kernel(const float* __restrict__ x, const int64_t* __restrict__ lt,
                                                          unsigned long long* __restrict__ bins_out,
                                                          unsigned long long* __restrict__ cls_out, double* __restrict__ part, CalibArgs a) {
    extern __shared__ unsigned long long calib_lds[];
    __shared__ double red[4][CALIB_MAXT * 2];
    const int C = CT ? CT : a.r.C;
    const int rows = a.B + C;
    const int nrow = a.NT * rows;
    unsigned long long* bins = calib_lds;
    double* acc = reinterpret_cast<double*>(calib_lds + (size_t)nrow * 2);
    for (int i = threadIdx.x; i < nrow * 2; i += 256) bins[i] = 0ull;
    for (int k = 0; k < a.NT * 2; ++k) acc[k * 256 + threadIdx.x] = 0.0;
    __syncthreads();
    for (long o = (long)blockIdx.x * 256 + threadIdx.x; o < a.total; o += (long)gridDim.x * 256) {       // (long: total may sit just below 2^31)
        const int64_t lab = lt[o];
        if (lab < 0 || lab >= C) continue;                // not counted: adds to nothing
        const int y = (int)lab;
        float z[CT ? CT : SSCG_MAXC];
        if (MODE == CALIB_RESIZE) {
            const sscg_pixel p = sscg_pixel_of((int)o, a.r);
            sscg_pixel_logits<CT, false>(x, p.n, p.oy, p.ox, a.r.H, a.r.W, a.r.sh, a.r.sw, C, z);
        } else {
            sscg_pixel_logits<CT, true>(x, 0, 0, (int)o, a.r.H, a.r.W, 0.f, 0.f, C, z);
        }
#pragma unroll 1
        for (int t = 0; t < a.NT; ++t) {
            float v[CT ? CT : SSCG_MAXC];
            float inv;
            if (MODE == CALIB_SCORES) {
#pragma unroll
                for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
                    if (CT || c < C) v[c] = z[c];
                inv = a.scale;
            } else {
                const float it = a.it[t];
#pragma unroll
                for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
                    if (CT || c < C) v[c] = calib_scaled(z[c], it);
                inv = sscg_softmax_exp<CT>(v, C);
            }
            const int pred = sscg_first_max_scaled<CT>(v, inv, C);
            float conf = 0.f, py = 0.f;
            double br = 0.0;
#pragma unroll
            for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
                if (CT || c < C) {
                    const float p = v[c] * inv;          // the product the first maximum was chosen by
                    conf = c == pred ? p : conf;
                    py = c == y ? p : py;
                    const double d = (double)p - (c == y ? 1.0 : 0.0);
                    br += d * d;
                }
            const float cb = conf * a.fB;
            int b = cb < a.fB ? (int)cb : a.B - 1;       // min(B - 1, (int)(conf * B)) without converting a value past the int range
            b = b < 0 ? 0 : b;                           // (scores are non-negative by contract; no bin index leaves the table)
            const unsigned long long q = (unsigned long long)(long long)(conf * 16777216.f);
            const unsigned long long one = 1ull | ((unsigned long long)(pred == y ? 1 : 0) << 32);
            unsigned long long* tb = bins + (size_t)t * rows * 2;
            atomicAdd(&tb[b * 2], one);
            atomicAdd(&tb[b * 2 + 1], q);
            atomicAdd(&tb[(a.B + pred) * 2], one);
            atomicAdd(&tb[(a.B + pred) * 2 + 1], q);
            const double pl = fmax((double)py, 0x1p-126);
            acc[(t * 2) * 256 + threadIdx.x] += -log(pl);
            acc[(t * 2 + 1) * 256 + threadIdx.x] += br;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nrow; i += 256) {
        const unsigned long long w0 = bins[i * 2], w1 = bins[i * 2 + 1];
        if (w0) {
            const int t = i / rows, r = i - t * rows;
            unsigned long long* dst = r < a.B ? bins_out + ((size_t)t * a.B + r) * 3 : cls_out + ((size_t)t * C + (r - a.B)) * 3;
            atomicAdd(dst, w0 & 0xffffffffull);
            if (w0 >> 32) atomicAdd(dst + 1, w0 >> 32);
            if (w1) atomicAdd(dst + 2, w1);
        }
    }
    const int wave = threadIdx.x >> 6;
    for (int k = 0; k < a.NT * 2; ++k) {
        const double s = wave_sum(acc[k * 256 + threadIdx.x]);
        if ((threadIdx.x & 63) == 0) red[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < a.NT * 2) {
        const int k = threadIdx.x;
        part[(size_t)blockIdx.x * a.NT * 2 + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    }
}

// `nblk` records of `cols` <= 16 doubles -> sums[cols] += their total: 16 row lanes of 16 threads (lane r takes records r, r + 16, ... in
// order), then the lanes in order by the column's first thread.  One block, one writer per element.
__global__ __launch_bounds__(256) void calib_finish_kernel(const double* __restrict__ part, int nblk, int cols, double* __restrict__ sums) {
    __shared__ double sm[256];
    const int k = threadIdx.x & 15, rl = threadIdx.x >> 4;
    double s = 0.0;
    if (k < cols)
        for (int r = rl; r < nblk; r += 16) s += part[(size_t)r * cols + k];
    sm[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < cols) {
        double t = 0.0;
        for (int r = 0; r < 16; ++r) t += sm[r * 16 + threadIdx.x];
        sums[threadIdx.x] += t;
    }
}

// n * a * b >= 2^31 for positive ints, without overflow on the way (the first product stays below 2^62)
bool calib_too_large(int n, int a, int b) {
    const uint64_t lim = (uint64_t)1 << 31, p = (uint64_t)n * (uint64_t)a;
    return p >= lim || p * (uint64_t)b >= lim;
}

int calib_blocks(int N, int OH, int OW) { return ew_blocks((size_t)N * OH * OW, CALIB_BLOCKS); }

template <int MODE>
void launch_calib(const CalibArgs& a, int blocks, hipStream_t st, const float* x, const int64_t* lt, unsigned long long* bins,
                  unsigned long long* cls, double* part) {
    const size_t lds = ((size_t)a.NT * (a.B + a.r.C) * 2 + (size_t)a.NT * 2 * 256) * 8;      // <= 12 KB of bins + 32 KB of slots
    sscg_dispatch_classes(a.r.C, [&](auto ct) {
        hipLaunchKernelGGL((calib_stats_kernel<decltype(ct)::value, MODE>), dim3((unsigned)blocks), dim3(256), lds, st, x, lt, bins, cls,
                           part, a);
    });
}

}  // namespace

extern "C" size_t sscg_calib_workspace(int N, int OH, int OW, int NT) {
    if (N <= 0 || OH <= 0 || OW <= 0 || NT < 1 || NT > CALIB_MAXT || calib_too_large(N, OH, OW)) return 0;
    return (size_t)calib_blocks(N, OH, OW) * NT * 2 * sizeof(double);       // one record per workgroup
}

extern "C" int sscg_calib_stats(const float* x, int kind, float scale, int N, int H, int W, int C, int OH, int OW, const int64_t* label_true,
                                const float* inv_temps, int NT, int B, int64_t* bins, int64_t* cls, double* sums, void* ws, size_t ws_bytes,
                                void* stream) {
    if (!x || !label_true || !inv_temps || !bins || !cls || !sums || !sizes_ok(N, H, W, C, OH, OW)) return SSCG_ERR_BAD_ARG;
    if ((kind != 0 && kind != 1) || B < 2 || B > CALIB_MAXB || NT < 1 || NT > CALIB_MAXT) return SSCG_ERR_BAD_ARG;
    for (int t = 0; t < NT; ++t)
        if (!(inv_temps[t] > 0.f && inv_temps[t] < INFINITY)) return SSCG_ERR_BAD_ARG;      // (false for a NaN)
    if (kind == 1 && (H != OH || W != OW || NT != 1 || inv_temps[0] != 1.f || !(scale >= 0.f && scale < INFINITY))) return SSCG_ERR_BAD_ARG;
    if (calib_too_large(N, OH, OW) || calib_too_large(N, H, W)) return SSCG_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < sscg_calib_workspace(N, OH, OW, NT)) return SSCG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    CalibArgs a;
    a.r = sscg_make_resize_geom(H, W, C, OH, OW);
    a.total = N * OH * OW;
    a.NT = NT; a.B = B; a.fB = (float)B; a.scale = scale;
    for (int t = 0; t < CALIB_MAXT; ++t) a.it[t] = t < NT ? inv_temps[t] : 1.f;
    const int blocks = calib_blocks(N, OH, OW);
    double* part = reinterpret_cast<double*>(ws);
    unsigned long long* b64 = reinterpret_cast<unsigned long long*>(bins);
    unsigned long long* c64 = reinterpret_cast<unsigned long long*>(cls);
    if (kind == 1) launch_calib<CALIB_SCORES>(a, blocks, st, x, label_true, b64, c64, part);
    else if (OH == H && OW == W) launch_calib<CALIB_IDENT>(a, blocks, st, x, label_true, b64, c64, part);
    else launch_calib<CALIB_RESIZE>(a, blocks, st, x, label_true, b64, c64, part);
    hipLaunchKernelGGL(calib_finish_kernel, dim3(1), dim3(256), 0, st, part, blocks, NT * 2, sums);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}
