// Multi-scale / mirrored inference (include/sscg.h): the views of one batch fused into one label map.  Forward only; the training
// step never launches them.
//   sscg_predict_head_ms: up to 8 low-resolution logit maps -> per view resize (+ mirror) -> softmax -> summed probabilities ->
//                         first maximum -> int64 / uint8 label maps, confusion matrix, and / or the summed probabilities themselves
//   sscg_resize_flip:     the network input of one view: bilinear resize of the batch with the output columns mirrored on request
// Both equal the chains of separate passes bit for bit: the per-pixel arithmetic is the functions of head_common.h.
#include "common.h"
#include "head_common.h"
#include "sscg_internal.h"

namespace {

constexpr int MAX_BLOCKS = 2048;   // 8 workgroups per CU, grid-stride beyond: bounds the LDS histograms flushed per launch
constexpr int MAX_VIEWS = 8;

// The views travel in the kernel's argument block: the host arrays are copied here during the call, no pointer table on the device.
struct MsViews {
    const float* x[MAX_VIEWS];
    int H[MAX_VIEWS], W[MAX_VIEWS];
    float sh[MAX_VIEWS], sw[MAX_VIEWS];      // sscg_upsample_bilinear_fwd's scales of each view
    int S;
    uint32_t flip;
};

typedef sscg_resize_geom MsGeom;      // C, OH, OW and the pixel split; H, W and the scales are per view (MsViews)

// One thread per OUTPUT pixel, consecutive lanes on consecutive pixels of a row, with a loop over the views inside: v[] holds the
// view's C logits / exponentials (sscg_pixel_logits), acc[] the running sum of the views' probabilities, both in
// registers (every class loop is unrolled, so no index is a run-time one).  The views are walked in order and every lane of a wave
// walks the same one: its geometry comes from the argument block through uniform loads.  The low-resolution maps are about a
// megabyte each and stay cache resident; only the outputs asked for are written.
// CT: class count at compile time (0 = any C <= SSCG_MAXC, every loop predicated on c < C).
template <int CT>
__global__ __launch_bounds__(256) void predict_head_ms_kernel(MsViews vw, float* __restrict__ prob_sum, int64_t* __restrict__ index,
                                                              uint8_t* __restrict__ label_u8, const int64_t* __restrict__ lt,
                                                              unsigned long long* __restrict__ hist, int total, MsGeom g) {
    extern __shared__ unsigned int bins[];      // [C][C] counts of this workgroup (hist != NULL only)
    const int C = CT ? CT : g.C;
    const int nb = hist ? C * C : 0;
    sscg_bins_clear(bins, nb);
    for (int o = blockIdx.x * 256 + threadIdx.x; o < total; o += gridDim.x * 256) {
        const sscg_pixel p = sscg_pixel_of(o, g);
        float acc[CT ? CT : SSCG_MAXC] = {};
#pragma nounroll
        for (int s = 0; s < vw.S; ++s) {
            const int H = vw.H[s], W = vw.W[s];
            const float* __restrict__ x = vw.x[s];
            const int oxs = (vw.flip >> s) & 1u ? g.OW - 1 - p.ox : p.ox;       // a mirrored view's map is in mirrored coordinates
            float v[CT ? CT : SSCG_MAXC];
            if (H == g.OH && W == g.OW) sscg_pixel_logits<CT, true>(x, p.n, p.oy, oxs, H, W, 0.f, 0.f, C, v);      // identity resize
            else sscg_pixel_logits<CT, false>(x, p.n, p.oy, oxs, H, W, vw.sh[s], vw.sw[s], C, v);
            const float inv = sscg_softmax_exp<CT>(v, C);
            sscg_prob_accumulate<CT>(acc, v, inv, C, s == 0);
        }
        if (prob_sum) {
            float* p = prob_sum + (size_t)o * C;
#pragma unroll
            for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
                if (CT || c < C) p[c] = acc[c];
        }
        const int bi = sscg_first_max<CT>(acc, C);
        if (index) index[o] = bi;
        if (label_u8) label_u8[o] = (uint8_t)bi;
        if (hist) sscg_bins_count(bins, C, lt[o], bi);
    }
    sscg_bins_flush(bins, nb, hist);
}

typedef sscg_resize_geom FlipGeom;      // (the 64-bit element index is split by plain divisions: dow / doh are not used)

// One thread per output ELEMENT (n, oy, ox, c); output column ox takes the resized
// map's column OW - 1 - ox when FLIP.  IDENT: OH == H && OW == W, a pure mirror copy.
template <bool IDENT, bool FLIP>
__global__ __launch_bounds__(256) void resize_flip_kernel(const float* __restrict__ x, float* __restrict__ y, size_t total, FlipGeom g) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % g.C);
        size_t t = i / g.C;
        const int ox = (int)(t % g.OW); t /= g.OW;
        const int oy = (int)(t % g.OH);
        const int n = (int)(t / g.OH);
        const int oxs = FLIP ? g.OW - 1 - ox : ox;
        const float* b = x + (size_t)n * g.H * g.W * g.C + c;
        if (IDENT) {
            y[i] = b[((size_t)oy * g.W + oxs) * g.C];
        } else {
            y[i] = sscg_bilerp_elem(b, sscg_bilin_at(oy, oxs, g.H, g.W, g.sh, g.sw), g.W, g.C);
        }
    }
}

}  // namespace

extern "C" int sscg_predict_head_ms(const float* const* xs, const int* Hs, const int* Ws, int S, uint32_t flip_mask, int N, int C, int OH,
                                    int OW, float* prob_sum, int64_t* index, uint8_t* label_u8, const int64_t* label_true, int64_t* hist,
                                    void* stream) {
    if (!xs || !Hs || !Ws || S < 1 || S > MAX_VIEWS || (flip_mask >> S) != 0u) return SSCG_ERR_BAD_ARG;
    if (N <= 0 || C <= 0 || C > SSCG_MAXC || OH <= 0 || OW <= 0) return SSCG_ERR_BAD_ARG;
    if ((!prob_sum && !index && !label_u8 && !hist) || (label_true == nullptr) != (hist == nullptr)) return SSCG_ERR_BAD_ARG;
    MsViews vw;
    for (int s = 0; s < MAX_VIEWS; ++s) {
        const int u = s < S ? s : 0;            // the unused slots repeat view 0: never read, never garbage
        if (!xs[u] || Hs[u] <= 0 || Ws[u] <= 0) return SSCG_ERR_BAD_ARG;
        vw.x[s] = xs[u]; vw.H[s] = Hs[u]; vw.W[s] = Ws[u];
        vw.sh[s] = sscg_resize_scale(Hs[u], OH);
        vw.sw[s] = sscg_resize_scale(Ws[u], OW);
    }
    vw.S = S; vw.flip = flip_mask;
    const size_t pixels = (size_t)N * OH * OW;
    if (pixels >= ((size_t)1 << 31) || (prob_sum && pixels * C >= ((size_t)1 << 31))) return SSCG_ERR_UNSUPPORTED;
    const MsGeom g = sscg_make_resize_geom(OH, OW, C, OH, OW);
    const int total = (int)pixels;
    const size_t lds = hist ? (size_t)C * C * sizeof(unsigned int) : 0;       // <= 16 KB
    unsigned long long* h = reinterpret_cast<unsigned long long*>(hist);
    const dim3 grid(ew_blocks(pixels, MAX_BLOCKS)), blk(256);
    hipStream_t st = (hipStream_t)stream;
    sscg_dispatch_classes(C, [&](auto ct) {
        hipLaunchKernelGGL(predict_head_ms_kernel<decltype(ct)::value>, grid, blk, lds, st, vw, prob_sum, index, label_u8, label_true, h, total, g);
    });
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_resize_flip(const float* x, float* y, int N, int H, int W, int C, int OH, int OW, int flip, void* stream) {
    if (!x || !y || N <= 0 || H <= 0 || W <= 0 || C <= 0 || OH <= 0 || OW <= 0) return SSCG_ERR_BAD_ARG;
    const FlipGeom g = sscg_make_resize_geom(H, W, C, OH, OW);
    const size_t total = (size_t)N * OH * OW * C;
    const dim3 grid(ew_blocks(total)), blk(256);
    hipStream_t st = (hipStream_t)stream;
    const bool ident = OH == H && OW == W;
    if (ident && flip) hipLaunchKernelGGL((resize_flip_kernel<true, true>), grid, blk, 0, st, x, y, total, g);
    else if (ident) hipLaunchKernelGGL((resize_flip_kernel<true, false>), grid, blk, 0, st, x, y, total, g);
    else if (flip) hipLaunchKernelGGL((resize_flip_kernel<false, true>), grid, blk, 0, st, x, y, total, g);
    else hipLaunchKernelGGL((resize_flip_kernel<false, false>), grid, blk, 0, st, x, y, total, g);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}
