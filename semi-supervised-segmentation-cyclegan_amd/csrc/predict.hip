// Inference heads: from a generator's output to what its consumer keeps, in one launch each (include/sscg.h lists the reference
// call sites).  Forward only; the training step never launches them.
//   sscg_predict_head: low-resolution logits -> resize -> softmax -> first maximum -> int64 / uint8 label maps, confusion matrix
//   sscg_image_head:   image generator output -> resize -> tanh -> fp32 NHWC and / or the uint8 pixels of the saved image
// Both equal the unfused chains bit for bit: the per-pixel arithmetic is the functions of head_common.h.
#include "common.h"
#include "head_common.h"
#include "sscg_internal.h"

namespace {

constexpr int MAX_BLOCKS = 2048;   // 8 workgroups per CU, grid-stride beyond: bounds the LDS histograms flushed per launch

typedef sscg_resize_geom PredGeom;

// One thread per OUTPUT pixel, consecutive lanes on consecutive pixels of a row: a wave's uint8 stores form one 64-byte segment, its
// int64 stores one of 512 bytes.  The C logits of the pixel live in registers; the four source rows are contiguous C-vectors of the
// low-resolution map (N x 33 x 33 x 21 fp32 = 0.7 MB: cache resident, and the lanes of a wave share a handful of source pixels).
// CT: class count at compile time (0 = any C <= SSCG_MAXC, every loop predicated on c < C so that v[] stays in registers).
// IDENT: OH == H && OW == W, the identity resize: the pixel's own logits, no interpolation arithmetic.
template <int CT, bool IDENT>
__global__ __launch_bounds__(256) void predict_head_kernel(const float* __restrict__ x, int64_t* __restrict__ index,
                                                           uint8_t* __restrict__ label_u8, const int64_t* __restrict__ lt,
                                                           unsigned long long* __restrict__ hist, int total, PredGeom g) {
    extern __shared__ unsigned int bins[];      // [C][C] counts of this workgroup (hist != NULL only)
    const int C = CT ? CT : g.C;
    const int nb = hist ? C * C : 0;
    sscg_bins_clear(bins, nb);
    for (int o = blockIdx.x * 256 + threadIdx.x; o < total; o += gridDim.x * 256) {
        float v[CT ? CT : SSCG_MAXC];
        const sscg_pixel p = IDENT ? sscg_pixel{0, 0, o} : sscg_pixel_of(o, g);
        sscg_pixel_logits<CT, IDENT>(x, p.n, p.oy, p.ox, g.H, g.W, g.sh, g.sw, C, v);
        const float inv = sscg_softmax_exp<CT>(v, C);
        const int bi = sscg_first_max_scaled<CT>(v, inv, C);
        if (index) index[o] = bi;
        if (label_u8) label_u8[o] = (uint8_t)bi;
        if (hist) sscg_bins_count(bins, C, lt[o], bi);
    }
    sscg_bins_flush(bins, nb, hist);
}

// t * 0.5 + 0.5 (validation.py), then x * 255 + 0.5, clamp, truncate (save_image): the host rounds each of the four operations to fp32
// on its own, so nothing may contract.  Plain operators under the pragma: it reaches the operations written in this body only - the
// bodies of __fmul_rn / __fadd_rn are inlined from the runtime's headers with their own contraction setting and did fuse into FMAs.
__device__ __forceinline__ uint8_t pixel_u8(float t) {
#pragma clang fp contract(off)
    const float h = t * 0.5f;
    const float u01 = h + 0.5f;
    const float s = u01 * 255.f;
    const float px = s + 0.5f;
    return (uint8_t)(int)fminf(fmaxf(px, 0.f), 255.f);
}

// One thread per output ELEMENT (n, oy, ox, c): fp32 and uint8 stores of a wave are contiguous.
template <bool IDENT>
__global__ __launch_bounds__(256) void image_head_kernel(const float* __restrict__ x, float* __restrict__ y, uint8_t* __restrict__ rgb,
                                                         int total, PredGeom g, FastDiv dc) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        float r;
        if (IDENT) {
            r = x[i];
        } else {
            const int t = fd_div(i, dc);
            const int c = i - t * g.C;
            const sscg_pixel p = sscg_pixel_of(t, g);
            const sscg_bilin b = sscg_bilin_at(p.oy, p.ox, g.H, g.W, g.sh, g.sw);
            r = sscg_bilerp_elem(x + (size_t)p.n * g.H * g.W * g.C + c, b, g.W, g.C);
        }
        const float th = sscg_act(r, SSCG_ACT_TANH, 0.f);       // sscg_act_fwd's routine
        if (y) y[i] = th;
        if (rgb) rgb[i] = pixel_u8(th);
    }
}

bool pred_geom(PredGeom* g, int* total, int N, int H, int W, int C, int OH, int OW, int per_pixel) {
    const size_t n_out = (size_t)N * OH * OW * per_pixel;
    if (n_out >= ((size_t)1 << 31)) return false;
    *g = sscg_make_resize_geom(H, W, C, OH, OW);
    *total = (int)n_out;
    return true;
}

template <bool IDENT>
void launch_predict(const PredGeom& g, int total, size_t lds, hipStream_t st, const float* x, int64_t* index, uint8_t* label_u8,
                    const int64_t* lt, unsigned long long* hist) {
    const dim3 grid(ew_blocks(total, MAX_BLOCKS)), blk(256);
    sscg_dispatch_classes(g.C, [&](auto ct) {
        hipLaunchKernelGGL((predict_head_kernel<decltype(ct)::value, IDENT>), grid, blk, lds, st, x, index, label_u8, lt, hist, total, g);
    });
}

}  // namespace

extern "C" int sscg_predict_head(const float* x, int N, int H, int W, int C, int OH, int OW, int64_t* index, uint8_t* label_u8,
                                 const int64_t* label_true, int64_t* hist, void* stream) {
    if (!x || N <= 0 || H <= 0 || W <= 0 || C <= 0 || C > SSCG_MAXC || OH <= 0 || OW <= 0) return SSCG_ERR_BAD_ARG;
    if ((!index && !label_u8 && !hist) || (label_true == nullptr) != (hist == nullptr)) return SSCG_ERR_BAD_ARG;
    PredGeom g;
    int total;
    if (!pred_geom(&g, &total, N, H, W, C, OH, OW, 1)) return SSCG_ERR_UNSUPPORTED;
    const size_t lds = hist ? (size_t)C * C * sizeof(unsigned int) : 0;       // <= 16 KB
    unsigned long long* h = reinterpret_cast<unsigned long long*>(hist);
    if (OH == H && OW == W) launch_predict<true>(g, total, lds, (hipStream_t)stream, x, index, label_u8, label_true, h);
    else launch_predict<false>(g, total, lds, (hipStream_t)stream, x, index, label_u8, label_true, h);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_image_head(const float* x, int N, int H, int W, int C, int OH, int OW, float* y_nhwc, uint8_t* rgb_u8, void* stream) {
    if (!x || N <= 0 || H <= 0 || W <= 0 || C <= 0 || C > 4 || OH <= 0 || OW <= 0 || (!y_nhwc && !rgb_u8)) return SSCG_ERR_BAD_ARG;
    PredGeom g;
    int total;
    if (!pred_geom(&g, &total, N, H, W, C, OH, OW, C)) return SSCG_ERR_UNSUPPORTED;
    const dim3 grid(ew_blocks(total, MAX_BLOCKS)), blk(256);
    if (OH == H && OW == W)
        hipLaunchKernelGGL(image_head_kernel<true>, grid, blk, 0, (hipStream_t)stream, x, y_nhwc, rgb_u8, total, g, make_fastdiv(C));
    else
        hipLaunchKernelGGL(image_head_kernel<false>, grid, blk, 0, (hipStream_t)stream, x, y_nhwc, rgb_u8, total, g, make_fastdiv(C));
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}
