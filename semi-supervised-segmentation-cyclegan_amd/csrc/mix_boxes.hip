// CutMix of a FINISHED fp32 batch (include/sscg.h: sscg_mix_boxes): y[n][h][w][:] = pasted(n, h, w) ? x[p][h][w][:] : x[n][h][w][:]
// with p = table[n][0], the rows of sscg_augment_mix_u8's table (partner, x0, y0, x1, y1, mask_lo, mask_hi, 0) - the student's input
// of the mean teacher's CutMix consistency (--unl_cutmix), whose teacher side is sscg_teacher_fwd_mix.  A pure copy in one launch:
// every element of y is written once, from x alone (y == x is refused: a partner's pixel is its pixel before mixing).
// The flat element index decides everything: the sample, the pixel, the row of the table.  Where a sample's H*W*C elements are a
// multiple of 4 and both pointers are 16-byte aligned, a thread moves 4 consecutive floats (they stay inside one sample, but may span
// pixels - C = 1: four, C = 3: parts of two - so the box is decided per element); otherwise one float per thread.  The grid covers
// the elements once, no cap and no loop: N*H*W*C < 2^31 gives fewer than 2^23 blocks.
#include "common.h"
#include "sscg_internal.h"

namespace {

typedef float mixb_f4 __attribute__((ext_vector_type(4)));

// the row of sample n, reduced to what a pixel needs: a partner that mixes nothing leaves the empty box and is never an index
struct mixb_row {
    int p, x0, y0, x1, y1;
    __device__ __forceinline__ mixb_row(const int32_t* __restrict__ table, int n, int N) {
        const int32_t* row = table + (size_t)n * 8;
        p = row[0];
        x0 = y0 = x1 = y1 = 0;
        if (p >= 0 && p < N && p != n) { x0 = row[1]; y0 = row[2]; x1 = row[3]; y1 = row[4]; }
        else p = n;
    }
    __device__ __forceinline__ bool pasted(int h, int w) const { return w >= x0 && w < x1 && h >= y0 && h < y1; }
};

// S = H * W * C, the elements of a sample; `work` = the threads with something to do (elements, or groups of 4)
template <bool VEC>
__global__ __launch_bounds__(256) void mix_boxes_kernel(const float* __restrict__ x, float* __restrict__ y, const int32_t* __restrict__ table,
                                                        int N, int W, int C, uint32_t S, uint32_t work) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= work) return;
    const uint32_t e = VEC ? i * 4u : i;                 // (< 2^31)
    const uint32_t n = e / S, r = e - n * S;
    const uint32_t pix = r / (uint32_t)C;
    int c = (int)(r - pix * (uint32_t)C);
    int h = (int)(pix / (uint32_t)W), w = (int)(pix - (uint32_t)h * (uint32_t)W);
    const mixb_row row(table, (int)n, N);
    if constexpr (!VEC) {
        y[e] = x[row.pasted(h, w) ? (size_t)row.p * S + r : (size_t)e];
    } else {
        mixb_f4 v = *reinterpret_cast<const mixb_f4*>(x + e);
        unsigned take = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            take |= (unsigned)row.pasted(h, w) << k;
            if (++c == C) { c = 0; if (++w == W) { w = 0; ++h; } }      // (the 4 elements stay inside the sample: h < H)
        }
        if (take) {
            const mixb_f4 u = *reinterpret_cast<const mixb_f4*>(x + (size_t)row.p * S + r);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = (take >> k & 1) ? u[k] : v[k];
        }
        *reinterpret_cast<mixb_f4*>(y + e) = v;
    }
}

}  // namespace

extern "C" int sscg_mix_boxes(const float* x, float* y, const int32_t* table, int N, int H, int W, int C, void* stream) {
    if (!x || !y || !table || y == x || N <= 0 || H <= 0 || W <= 0 || C <= 0) return SSCG_ERR_BAD_ARG;
    const uint64_t lim = (uint64_t)1 << 31, HW = (uint64_t)H * W;      // (each product is bounded before the next factor joins)
    if (HW >= lim || HW * (uint64_t)C >= lim || HW * (uint64_t)C * (uint64_t)N >= lim) return SSCG_ERR_UNSUPPORTED;
    const uint64_t S = HW * (uint64_t)C;
    const uint32_t total = (uint32_t)(S * (uint64_t)N);
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = S % 4 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
    const uint32_t work = vec ? total / 4 : total;
    const dim3 grid((work + 255) / 256), blk(256);
    if (vec) hipLaunchKernelGGL(mix_boxes_kernel<true>, grid, blk, 0, st, x, y, table, N, W, C, (uint32_t)S, work);
    else hipLaunchKernelGGL(mix_boxes_kernel<false>, grid, blk, 0, st, x, y, table, N, W, C, (uint32_t)S, work);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}
