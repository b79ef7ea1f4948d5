// Hard-pixel mining (OHEM) cross entropy of the segmentation head (include/sscg.h: sscg_ohem_fwd / sscg_ce_bwd_ohem;
// sscg_upsample_head_bwd_h is in head_bwd.hip).
//
// With p = softmax_C(resize(z)) (bilinear, align_corners=True; identity sizes: p = softmax_C(z)) and a pixel COUNTED when its label y lies
// in [0, C), the KEY of a counted pixel is k = p[y].  Of the V counted pixels of the call the r hardest - the r smallest keys,
// r = clamp(max(min_kept, ceil(min_frac * V)), 1, V) - are always kept, and so is every pixel whose key does not exceed `thresh`:
//     m = the r-th smallest key (exact, ties included)     tau = max(m, thresh)     kept <=> counted and k <= tau
// The cross entropy (class weights, label smoothing: the formulas of sscg_ce_fwd_w) then runs over the kept pixels only.  Like Dice, the
// selection couples every pixel of the call - through one order statistic - so the forward leaves no gradient:
//   1. ohem_key_kernel     one thread per OUTPUT pixel, no block straddles a sample (dice_stats_kernel's frame): the pixel's logits in
//                          registers by the pinned arithmetic of head_common.h, its key (2.0f where not counted) and its loss term, one
//                          fp32 each - the only per-pixel maps; the first digit's histogram is taken while the key is in a register;
//   2. the selection       a non-negative fp32 orders like its bit pattern and a key is at most 1.0f, so its pattern has 30 significant
//                          bits: a radix select over three digits of ten bits, most significant first.  Per digit ohem_hist_kernel bins
//                          the keys that carry the digits chosen so far (per-block histograms in LDS, one integer add per non-empty bin
//                          and block to the global table), ohem_scan_kernel - one block - picks the bin that holds the remaining rank.
//                          Integer atomics only: the result does not depend on any order.  V, r, m and tau stay on the device;
//   3. ohem_loss_kernel    sum of the kept terms, D = sum of the kept w[y] and the kept count: per-block fp64 records, summed in index
//      ohem_finish_kernel  order by one block - no float atomics;
//   4. the backward        flat (ohem_ce_bwd_kernel: one thread per pixel) or through the adjoint of the resize: the MINED term of the
//                          head's one backward kernel (head_bwd_kernel, head_bwd.hip: sscg_upsample_head_bwd_h), with the softmax-output
//                          and Dice branches in the same launch.  Both READ the keep decision - keys[o] <= tau - and never re-derive
//                          it from recomputed probabilities.
#include "common.h"
#include "head_common.h"
#include "head_geom.h"
#include "sscg_internal.h"

namespace {

constexpr int OHEM_KEY_BLOCKS = 256;      // key-pass blocks per sample, grid-stride beyond (dice_stats_kernel's frame)
constexpr int OHEM_BINS = 1024;           // ten bits per digit
constexpr int OHEM_DIGITS = 3;            // 30 bits: every key <= 1.0f = 0x3F800000 lies below 2^30
constexpr int OHEM_HIST_BLOCKS = 2048;    // grid cap of the histogram passes
constexpr int OHEM_LOSS_BLOCKS = 1024;    // grid cap of the loss pass = records the finish reads per sum

// the selection's state in the workspace: written by one thread of ohem_scan_kernel, read by the passes after it
struct OhemState {
    uint32_t prefix;      // the digits chosen so far (most significant first); after the last scan: the bits of m
    uint32_t rank;        // 1-based rank of m among the keys that carry the prefix; 0: no counted pixel
    uint32_t V;           // counted pixels of the call
    float thr;            // tau
};

// workspace: [3][1024] uint32 tables | state (256 B) | [3][OHEM_LOSS_BLOCKS] fp64 records | term fp32 [N * OH * OW]
constexpr size_t OHEM_TABLE_BYTES = (size_t)OHEM_DIGITS * OHEM_BINS * sizeof(uint32_t);
constexpr size_t OHEM_STATE_BYTES = 256;
constexpr size_t OHEM_PART_BYTES = (size_t)3 * OHEM_LOSS_BLOCKS * sizeof(double);
constexpr size_t OHEM_HEAD_BYTES = OHEM_TABLE_BYTES + OHEM_STATE_BYTES + OHEM_PART_BYTES;

struct OhemGeom {
    sscg_resize_geom r;
    int npix;      // OH * OW: output pixels of a sample
    int bps;       // key-pass blocks per sample
};

// the tables and the state, zeroed on the stream by every call: nothing depends on what the workspace held
__global__ __launch_bounds__(256) void ohem_zero_kernel(uint32_t* __restrict__ words, int n) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) words[i] = 0u;
}

__device__ __forceinline__ void ohem_bins_clear(unsigned int* bins) {
    for (int i = threadIdx.x; i < OHEM_BINS; i += 256) bins[i] = 0u;
    __syncthreads();
}

__device__ __forceinline__ void ohem_bins_flush(const unsigned int* bins, uint32_t* __restrict__ table) {
    __syncthreads();
    for (int i = threadIdx.x; i < OHEM_BINS; i += 256)
        if (bins[i]) atomicAdd(&table[i], bins[i]);
}

// One thread per output pixel of ONE sample (block b serves sample b / bps), consecutive lanes on consecutive pixels of a row.  A pixel
// that is not counted costs its label load and two stores.  A counted pixel: its C logits (RESIZE: the pinned stencil - the bits
// sscg_upsample_bilinear_fwd stores; !RESIZE: the row itself), sscg_softmax_exp, key = exp(z_y - max) * (1 / sum) - the probability
// softmax_fwd_kernel stores - and the term of sscg_ce_fwd_w (ce_fwd_kernel's expressions); then the first digit's bin.
template <int CT, bool RESIZE>
__global__ __launch_bounds__(256) void ohem_key_kernel(const float* __restrict__ x, const int64_t* __restrict__ lab,
                                                       const float* __restrict__ class_w, float smoothing, float* __restrict__ keys,
                                                       float* __restrict__ term, uint32_t* __restrict__ table0, OhemGeom g) {
    __shared__ unsigned int bins[OHEM_BINS];
    __shared__ float sW[SSCG_MAXC];
    const int C = CT ? CT : g.r.C;
    if ((int)threadIdx.x < C) sW[threadIdx.x] = class_weight(class_w, threadIdx.x);
    ohem_bins_clear(bins);
    float wsum = 0.f;
    for (int c = 0; c < C; ++c) wsum += sW[c];
    const float bs = smoothing / (float)C, a0 = 1.f - smoothing;
    const int n = blockIdx.x / g.bps, blk = blockIdx.x - n * g.bps;
    const float* xn = x + (size_t)n * g.r.H * g.r.W * C;
    const size_t base = (size_t)n * g.npix;
    for (long o_raw = (long)blk * 256 + threadIdx.x; o_raw < g.npix; o_raw += (long)g.bps * 256) {      // (long: npix may sit just below 2^31)
        const int o = (int)o_raw;
        const int64_t l64 = lab[base + o];
        float key = 2.0f, t = 0.f;
        if (l64 >= 0 && l64 < C) {
            const int l = (int)l64;
            float v[CT ? CT : SSCG_MAXC];
            const int oy = RESIZE ? fd_div(o, g.r.dow) : 0;       // the pixel within its sample: xn is the sample's map
            sscg_pixel_logits<CT, !RESIZE>(xn, 0, oy, o - oy * g.r.OW, g.r.H, g.r.W, g.r.sh, g.r.sw, C, v);
            float m = -INFINITY, vl = 0.f;
#pragma unroll
            for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
                if (CT || c < C) { m = fmaxf(m, v[c]); vl = c == l ? v[c] : vl; }
            float swd = 0.f;
            if (bs != 0.f) {
#pragma unroll
                for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
                    if (CT || c < C) swd += sW[c] * (v[c] - m);
            }
            const float inv = sscg_softmax_exp<CT>(v, C);
            float s = 0.f, el = 0.f;
#pragma unroll
            for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
                if (CT || c < C) { s += v[c]; el = c == l ? v[c] : el; }      // the sum sscg_softmax_exp formed, in its order
            key = el * inv;
            const float ls = logf(s);
            t = a0 * sW[l] * (ls + m - vl) + (bs != 0.f ? bs * (ls * wsum - swd) : 0.f);
            atomicAdd(&bins[(__float_as_uint(key) >> 20) & (OHEM_BINS - 1)], 1u);
        }
        keys[base + o] = key;
        term[base + o] = t;
    }
    ohem_bins_flush(bins, table0);
}

// Digit d (1 or 2) of the keys that carry the d digits chosen so far.  The sentinel 2.0f = 0x40000000 carries no prefix.
__global__ __launch_bounds__(256) void ohem_hist_kernel(const float* __restrict__ keys, size_t total, const OhemState* __restrict__ st,
                                                        int d, uint32_t* __restrict__ table) {
    __shared__ unsigned int bins[OHEM_BINS];
    ohem_bins_clear(bins);
    const uint32_t prefix = st->prefix;
    const int shift = 10 * (OHEM_DIGITS - 1 - d);
    if (st->rank != 0) {                                                   // (block-uniform; 0: no counted pixel, nothing to select)
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
            const uint32_t b = __float_as_uint(keys[i]);
            if ((b >> (shift + 10)) == prefix) atomicAdd(&bins[(b >> shift) & (OHEM_BINS - 1)], 1u);
        }
    }
    ohem_bins_flush(bins, table);
}

// One block: the bin of digit d that holds the remaining rank.  Thread t owns bins 4t .. 4t+3; an inclusive scan of the threads' sums
// (wave shuffles, then the four waves in order), and the one thread whose range holds the rank walks its four bins.  d == 0 first forms
// V (the table's total) and r; the last digit completes m and writes tau.
__global__ __launch_bounds__(256) void ohem_scan_kernel(const uint32_t* __restrict__ table, OhemState* __restrict__ st, int d, float thresh,
                                                        long long min_kept, float min_frac, float* __restrict__ thr_out) {
    __shared__ uint32_t wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t c[4], own = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { c[j] = table[4 * tid + j]; own += c[j]; }
    const uint32_t prefix = d ? st->prefix : 0u;
    uint32_t rank = d ? st->rank : 0u;
    uint32_t incl = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();                                       // (also: every thread has read the state before one of them writes it)
    uint32_t before = 0;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    incl += before;
    if (d == 0) {
        const uint32_t V = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (V != 0) {
            const long long frac = (long long)ceil((double)min_frac * (double)V);
            long long need = min_kept > frac ? min_kept : frac;
            need = need < 1 ? 1 : need;
            rank = need > (long long)V ? V : (uint32_t)need;
        }
        if (tid == 0) st->V = V;
    }
    if (rank == 0) {                                       // no counted pixel: nothing is kept whatever tau is
        if (tid == 0) {
            st->prefix = 0u; st->rank = 0u;
            if (d == OHEM_DIGITS - 1) { st->thr = thresh; *thr_out = thresh; }
        }
        return;
    }
    uint32_t excl = incl - own;
    if (excl < rank && rank <= incl) {
        int j = 0;
        while (j < 3 && excl + c[j] < rank) { excl += c[j]; ++j; }
        const uint32_t p = (prefix << 10) | (uint32_t)(4 * tid + j);
        st->prefix = p;
        st->rank = rank - excl;
        if (d == OHEM_DIGITS - 1) {
            const float tau = fmaxf(__uint_as_float(p), thresh);
            st->thr = tau;
            *thr_out = tau;
        }
    }
}

// Sum of the kept terms, D and the kept count: per block one fp64 record each.  A kept pixel is counted (the sentinel exceeds every tau).
template <bool CW>
__global__ __launch_bounds__(256) void ohem_loss_kernel(const float* __restrict__ keys, const float* __restrict__ term,
                                                        const int64_t* __restrict__ lab, const float* __restrict__ class_w, int C,
                                                        size_t total, const OhemState* __restrict__ st, double* __restrict__ part,
                                                        int nparts) {
    __shared__ double sm[4][3];
    const float tau = st->thr;
    double acc = 0.0, den = 0.0, cnt = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        if (!(keys[i] <= tau)) continue;
        acc += (double)term[i];
        cnt += 1.0;
        if (CW) {
            const int64_t l = lab[i];
            den += (l >= 0 && l < C) ? (double)class_w[l] : 0.0;
        }
    }
    if (!CW) den = cnt;
    acc = wave_sum(acc); den = wave_sum(den); cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6][0] = acc; sm[threadIdx.x >> 6][1] = den; sm[threadIdx.x >> 6][2] = cnt; }
    __syncthreads();
    if (threadIdx.x < 3) part[(size_t)threadIdx.x * nparts + blockIdx.x] = (sm[0][threadIdx.x] + sm[1][threadIdx.x]) + (sm[2][threadIdx.x] + sm[3][threadIdx.x]);
}

// loss = sum / D (NaN when D == 0: sscg_ce_fwd_w's rule), valid = D, counts = {kept, V}: the records in a fixed order
__global__ __launch_bounds__(256) void ohem_finish_kernel(const double* __restrict__ part, int nparts, const OhemState* __restrict__ st,
                                                          float* __restrict__ loss, float* __restrict__ valid, int64_t* __restrict__ counts) {
    __shared__ double sm[3][256];
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nparts; i += 256)
        for (int k = 0; k < 3; ++k) s[k] += part[(size_t)k * nparts + i];
    for (int k = 0; k < 3; ++k) sm[k][threadIdx.x] = s[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[3] = {0.0, 0.0, 0.0};
        for (int i = 0; i < 256; ++i)
            for (int k = 0; k < 3; ++k) t[k] += sm[k][i];
        *loss = t[1] > 0.0 ? (float)(t[0] / t[1]) : __builtin_nanf("");
        *valid = (float)t[1];
        counts[0] = (int64_t)t[2];
        counts[1] = (int64_t)st->V;
    }
}

// Flat backward: ce_bwd_kernel's gradient for a kept pixel (keys[r] <= tau, read - not re-derived), a zero row for every other pixel.
template <int CT>
__global__ __launch_bounds__(256) void ohem_ce_bwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ lab,
                                                          const float* __restrict__ keys, const float* __restrict__ thr, size_t rows, int Cr,
                                                          const float* __restrict__ class_w, float smoothing,
                                                          const float* __restrict__ gscale, float w, const float* __restrict__ valid,
                                                          float* __restrict__ dx) {
    const int C = CT ? CT : Cr;
    const float nv = *valid, tau = *thr;
    const float g = (gscale ? *gscale : 1.f) * (nv > 0.f ? w / nv : 0.f);
    float wsum = 0.f;
    for (int c = 0; c < C; ++c) wsum += class_weight(class_w, c);
    const float bs = smoothing / (float)C;
    for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (size_t)gridDim.x * 256) {
        const int64_t l64 = lab[r];
        float* dr = dx + r * C;
        if (l64 < 0 || l64 >= C || !(keys[r] <= tau)) {
#pragma unroll
            for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
                if (CT || c < C) dr[c] = 0.f;
            continue;
        }
        const int l = (int)l64;
        const float* xr = x + r * C;
        float v[CT ? CT : SSCG_MAXC];
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
            if (CT || c < C) v[c] = xr[c];
        const float inv = sscg_softmax_exp<CT>(v, C);
        const float a = (1.f - smoothing) * class_weight(class_w, l);
        const float k = a + bs * wsum;
#pragma unroll
        for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
            if (CT || c < C) dr[c] = (v[c] * inv * k - (c == l ? a : 0.f) - bs * class_weight(class_w, c)) * g;
    }
}

int ohem_bps(int OH, int OW) {
    const long npix = (long)OH * OW;
    const long b = (npix + 255) / 256;
    return (int)(b > OHEM_KEY_BLOCKS ? OHEM_KEY_BLOCKS : b);
}

template <bool RESIZE>
void launch_keys(const OhemGeom& g, int N, hipStream_t st, const float* x, const int64_t* lab, const float* class_w, float smoothing,
                 float* keys, float* term, uint32_t* table0) {
    const dim3 grid((unsigned)N * g.bps), blk(256);
    sscg_dispatch_classes(g.r.C, [&](auto ct) {
        hipLaunchKernelGGL((ohem_key_kernel<decltype(ct)::value, RESIZE>), grid, blk, 0, st, x, lab, class_w, smoothing, keys, term, table0, g);
    });
}

}  // namespace

extern "C" size_t sscg_ohem_workspace(int N, int OH, int OW) {
    if (N <= 0 || OH <= 0 || OW <= 0) return 0;
    return OHEM_HEAD_BYTES + (size_t)N * (size_t)OH * (size_t)OW * sizeof(float);
}

extern "C" int sscg_ohem_fwd(const float* x, const int64_t* labels, int N, int H, int W, int C, int OH, int OW, const float* class_w,
                             float smoothing, float thresh, int64_t min_kept, float min_frac, float* keys, float* loss, float* valid,
                             float* thr, int64_t* counts, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !labels || !keys || !loss || !valid || !thr || !counts || !sizes_ok(N, H, W, C, OH, OW)) return SSCG_ERR_BAD_ARG;
    if (!smoothing_ok(smoothing) || !(thresh > 0.f && thresh <= 1.f) || min_kept < 0 || !(min_frac >= 0.f && min_frac <= 1.f))
        return SSCG_ERR_BAD_ARG;                                                                                     // (each false for a NaN)
    if (too_large(N, H, W, OH, OW)) return SSCG_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < sscg_ohem_workspace(N, OH, OW)) return SSCG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const OhemGeom g = {sscg_make_resize_geom(H, W, C, OH, OW), OH * OW, ohem_bps(OH, OW)};
    char* base = reinterpret_cast<char*>(ws);
    uint32_t* table = reinterpret_cast<uint32_t*>(base);
    OhemState* state = reinterpret_cast<OhemState*>(base + OHEM_TABLE_BYTES);
    double* part = reinterpret_cast<double*>(base + OHEM_TABLE_BYTES + OHEM_STATE_BYTES);
    float* term = reinterpret_cast<float*>(base + OHEM_HEAD_BYTES);
    const size_t total = (size_t)N * OH * OW;
    const int nzero = (int)((OHEM_TABLE_BYTES + OHEM_STATE_BYTES) / sizeof(uint32_t));
    hipLaunchKernelGGL(ohem_zero_kernel, dim3(4), dim3(256), 0, st, table, nzero);
    if (OH == H && OW == W) launch_keys<false>(g, N, st, x, labels, class_w, smoothing, keys, term, table);
    else launch_keys<true>(g, N, st, x, labels, class_w, smoothing, keys, term, table);
    for (int d = 0; d < OHEM_DIGITS; ++d) {
        uint32_t* td = table + (size_t)d * OHEM_BINS;
        if (d) hipLaunchKernelGGL(ohem_hist_kernel, dim3(ew_blocks(total, OHEM_HIST_BLOCKS)), dim3(256), 0, st, keys, total, state, d, td);
        hipLaunchKernelGGL(ohem_scan_kernel, dim3(1), dim3(256), 0, st, td, state, d, thresh, (long long)min_kept, min_frac, thr);
    }
    const int nb = ew_blocks(total, OHEM_LOSS_BLOCKS);
    if (class_w)
        hipLaunchKernelGGL(ohem_loss_kernel<true>, dim3(nb), dim3(256), 0, st, keys, term, labels, class_w, C, total, state, part, nb);
    else
        hipLaunchKernelGGL(ohem_loss_kernel<false>, dim3(nb), dim3(256), 0, st, keys, term, labels, class_w, C, total, state, part, nb);
    hipLaunchKernelGGL(ohem_finish_kernel, dim3(1), dim3(256), 0, st, part, nb, state, loss, valid, counts);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_ce_bwd_ohem(const float* logits, const int64_t* labels, const float* keys, const float* thr, int64_t rows, int C,
                                const float* class_w, float smoothing, const float* gscale, float w, const float* valid, float* dx,
                                void* stream) {
    if (!logits || !labels || !keys || !thr || !valid || !dx || rows <= 0 || C <= 0 || C > SSCG_MAXC) return SSCG_ERR_BAD_ARG;
    if (!smoothing_ok(smoothing)) return SSCG_ERR_BAD_ARG;
    if (rows >= ((int64_t)1 << 31)) return SSCG_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(ew_blocks((size_t)rows)), blk(256);
    sscg_dispatch_classes(C, [&](auto ct) {
        hipLaunchKernelGGL(ohem_ce_bwd_kernel<decltype(ct)::value>, grid, blk, 0, st, logits, labels, keys, thr, (size_t)rows, C, class_w, smoothing,
                           gscale, w, valid, dx);
    });
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}
