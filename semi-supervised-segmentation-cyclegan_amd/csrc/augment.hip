// Batched affine augmentation fused into the batch finish: uint8 pixels / label ids of a batch -> the fp32 image and int64 label
// tensors the step consumes, warped per sample by an integer (Q16) affine map.  One launch replaces image_u8_to_f32_kernel +
// label_lut_kernel (pointwise.hip); with identity matrices the outputs equal theirs bit for bit.  The arithmetic is stated in
// include/sscg.h (sscg_augment_u8): integers up to the last two fp32 divisions, so a host restatement agrees exactly.
#include "common.h"
#include "sscg_internal.h"

namespace {

typedef int64_t i64x2 __attribute__((ext_vector_type(2)));

constexpr int AUG_THREADS = 256;
// 3 blocks per CU of the 256: every thread already holds 16 independent taps per channel in flight, so residency beyond that buys
// no more latency hiding; larger batches go round the grid-stride loop
constexpr int AUG_MAX_BLOCKS = 768;

struct aug_geom {
    int H, W, OH, OW;
    int image_fill, label_fill;
};

// the six Q16 coefficients of one sample
struct aug_mat { int32_t m[6]; };

__device__ __forceinline__ aug_mat aug_load_mat(const int32_t* __restrict__ mats, int n) {
    aug_mat a;
#pragma unroll
    for (int e = 0; e < 6; ++e) a.m[e] = mats[(size_t)n * 6 + e];
    return a;
}

// one output pixel (n, oy, ox): C normalised channels into out[], the raw source label id as the return value (LABEL only)
template <int C, bool LABEL>
__device__ __forceinline__ int aug_pixel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ gt, const aug_mat& a, const aug_geom& g,
                                         int n, int oy, int ox, const float* mean, const float* stdev, float* out) {
    const int64_t sx = (int64_t)a.m[0] * ox + (int64_t)a.m[1] * oy + a.m[2];
    const int64_t sy = (int64_t)a.m[3] * ox + (int64_t)a.m[4] * oy + a.m[5];
    const size_t plane = (size_t)n * g.H * g.W;
    // ---- image: four taps, 8-bit weights
    const int64_t x0 = sx >> 16, y0 = sy >> 16;
    const int fx = (int)(sx & 0xFFFF) >> 8, fy = (int)(sy & 0xFFFF) >> 8;
    // a tap whose weight is zero is never read: its product is an exact 0 whatever the byte
    const bool inx0 = (uint64_t)x0 < (uint64_t)g.W, inx1 = fx != 0 && (uint64_t)(x0 + 1) < (uint64_t)g.W;
    const bool iny0 = (uint64_t)y0 < (uint64_t)g.H, iny1 = fy != 0 && (uint64_t)(y0 + 1) < (uint64_t)g.H;
    const uint8_t* p00 = img + (plane + (size_t)(y0 * g.W + x0)) * C;      // dereferenced only under its in-range flags
    const uint8_t* p10 = p00 + (size_t)g.W * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int v00 = (iny0 && inx0) ? p00[c] : g.image_fill;
        const int v01 = (iny0 && inx1) ? p00[C + c] : g.image_fill;
        const int v10 = (iny1 && inx0) ? p10[c] : g.image_fill;
        const int v11 = (iny1 && inx1) ? p10[C + c] : g.image_fill;
        const int top = v00 * (256 - fx) + v01 * fx;
        const int bot = v10 * (256 - fx) + v11 * fx;
        const int v = top * (256 - fy) + bot * fy;                          // < 2^24: exact in fp32
        const float t = __fdiv_rn(__fmul_rn((float)v, 0x1p-16f), 255.0f);
        out[c] = __fdiv_rn(__fsub_rn(t, mean[c]), stdev[c]);
    }
    // ---- label: nearest source index
    int id = 0;
    if constexpr (LABEL) {
        const int64_t ix = (sx + 0x8000) >> 16, iy = (sy + 0x8000) >> 16;
        id = g.label_fill;
        if ((uint64_t)ix < (uint64_t)g.W && (uint64_t)iy < (uint64_t)g.H) id = gt[plane + (size_t)(iy * g.W + ix)];
    }
    return id;
}

// Every thread owns four consecutive pixels of the flat [N * OH * OW] range (a group may straddle a row or a sample) and stores them
// as 16-byte vectors: 4 * C floats = C stores, four labels = two stores.  `groups` = 0 sends every pixel down the scalar tail.
template <int C, bool LABEL>
__global__ __launch_bounds__(AUG_THREADS) void augment_u8_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ gt,
                                                                 const int32_t* __restrict__ mats, float* __restrict__ out_img,
                                                                 int64_t* __restrict__ out_gt, const float* __restrict__ mean,
                                                                 const float* __restrict__ stdev, const int64_t* __restrict__ lut,
                                                                 aug_geom g, uint32_t total, uint32_t groups) {
    __shared__ int64_t t[256];
    if constexpr (LABEL) {
        t[threadIdx.x] = lut[threadIdx.x];
        __syncthreads();
    }
    float mu[C], sd[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { mu[c] = mean[c]; sd[c] = stdev[c]; }
    const uint32_t hw = (uint32_t)g.OH * (uint32_t)g.OW;
    const uint32_t stride = gridDim.x * AUG_THREADS;
    for (uint32_t q = blockIdx.x * AUG_THREADS + threadIdx.x; q < groups; q += stride) {
        const uint32_t p0 = q * 4;
        int n = (int)(p0 / hw);
        const uint32_t r = p0 - (uint32_t)n * hw;
        int oy = (int)(r / (uint32_t)g.OW);
        int ox = (int)(r - (uint32_t)oy * (uint32_t)g.OW);
        aug_mat a = aug_load_mat(mats, n);
        float v[4 * C];
        int64_t lab[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int id = aug_pixel<C, LABEL>(img, gt, a, g, n, oy, ox, mu, sd, v + e * C);
            if constexpr (LABEL) lab[e] = t[id];
            if (e < 3 && ++ox == g.OW) {
                ox = 0;
                if (++oy == g.OH) {                 // the next pixel of the group is in range: p0 + 3 < total
                    oy = 0;
                    a = aug_load_mat(mats, ++n);
                }
            }
        }
        f32x4* o = reinterpret_cast<f32x4*>(out_img + (size_t)p0 * C);
#pragma unroll
        for (int k = 0; k < C; ++k) o[k] = f32x4{v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]};
        if constexpr (LABEL) {
            i64x2* ol = reinterpret_cast<i64x2*>(out_gt + p0);
            ol[0] = i64x2{lab[0], lab[1]};
            ol[1] = i64x2{lab[2], lab[3]};
        }
    }
    // scalar tail: the last total % 4 pixels (or all of them)
    for (uint32_t p = groups * 4 + blockIdx.x * AUG_THREADS + threadIdx.x; p < total; p += stride) {
        const int n = (int)(p / hw);
        const uint32_t r = p - (uint32_t)n * hw;
        const int oy = (int)(r / (uint32_t)g.OW);
        const int ox = (int)(r - (uint32_t)oy * (uint32_t)g.OW);
        const aug_mat a = aug_load_mat(mats, n);
        float v[C];
        const int id = aug_pixel<C, LABEL>(img, gt, a, g, n, oy, ox, mu, sd, v);
#pragma unroll
        for (int c = 0; c < C; ++c) out_img[(size_t)p * C + c] = v[c];
        if constexpr (LABEL) out_gt[p] = t[id];
    }
}

template <int C>
void aug_launch(bool label, dim3 grid, hipStream_t st, const uint8_t* img, const uint8_t* gt, const int32_t* mats, float* out_img,
                int64_t* out_gt, const float* mean, const float* stdev, const int64_t* lut, const aug_geom& g, uint32_t total,
                uint32_t groups) {
    if (label)
        hipLaunchKernelGGL((augment_u8_kernel<C, true>), grid, dim3(AUG_THREADS), 0, st, img, gt, mats, out_img, out_gt, mean, stdev, lut, g,
                           total, groups);
    else
        hipLaunchKernelGGL((augment_u8_kernel<C, false>), grid, dim3(AUG_THREADS), 0, st, img, gt, mats, out_img, out_gt, mean, stdev, lut, g,
                           total, groups);
}

}  // namespace

extern "C" int sscg_augment_u8(const uint8_t* img, const uint8_t* gt, const int32_t* mats, float* out_img, int64_t* out_gt, int N, int H,
                               int W, int C, int OH, int OW, const float* mean, const float* stdev, const int64_t* lut256, int image_fill,
                               int label_fill, void* stream) {
    if (!img || !mats || !out_img || !mean || !stdev) return SSCG_ERR_BAD_ARG;
    if (C < 1 || C > 4 || N <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return SSCG_ERR_BAD_ARG;
    if (image_fill < 0 || image_fill > 255 || label_fill < 0 || label_fill > 255) return SSCG_ERR_BAD_ARG;
    if (gt ? (!lut256 || !out_gt) : out_gt != nullptr) return SSCG_ERR_BAD_ARG;
    const int64_t total = (int64_t)N * OH * OW;
    if (total >= ((int64_t)1 << 31) || H > 32767 || W > 32767) return SSCG_ERR_UNSUPPORTED;
    // the 16-byte stores need 16-byte aligned outputs (every group starts a multiple of 16 bytes behind them)
    const bool aligned = (((size_t)out_img | (size_t)out_gt) & 15) == 0;
    const uint32_t groups = aligned ? (uint32_t)(total / 4) : 0u;
    const uint32_t work = groups ? groups + (uint32_t)(total - (int64_t)groups * 4 > 0) : (uint32_t)total;
    uint32_t blocks = (work + AUG_THREADS - 1) / AUG_THREADS;
    if (blocks > AUG_MAX_BLOCKS) blocks = AUG_MAX_BLOCKS;
    const aug_geom g = {H, W, OH, OW, image_fill, label_fill};
    const hipStream_t st = (hipStream_t)stream;
    const bool label = gt != nullptr;
    switch (C) {
        case 1: aug_launch<1>(label, dim3(blocks), st, img, gt, mats, out_img, out_gt, mean, stdev, lut256, g, (uint32_t)total, groups); break;
        case 2: aug_launch<2>(label, dim3(blocks), st, img, gt, mats, out_img, out_gt, mean, stdev, lut256, g, (uint32_t)total, groups); break;
        case 3: aug_launch<3>(label, dim3(blocks), st, img, gt, mats, out_img, out_gt, mean, stdev, lut256, g, (uint32_t)total, groups); break;
        default: aug_launch<4>(label, dim3(blocks), st, img, gt, mats, out_img, out_gt, mean, stdev, lut256, g, (uint32_t)total, groups); break;
    }
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}
