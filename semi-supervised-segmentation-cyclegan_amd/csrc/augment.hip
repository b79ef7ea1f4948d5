// Batched affine augmentation fused into the batch finish: uint8 pixels / label ids of a batch -> the fp32 image and int64 label
// tensors the step consumes, warped per sample by an integer (Q16) affine map.  One launch replaces image_u8_to_f32_kernel +
// label_lut_kernel (pointwise.hip); with identity matrices the outputs equal theirs bit for bit.  The arithmetic is stated in
// include/sscg.h (sscg_augment_u8): integers up to the last two fp32 divisions, so a host restatement agrees exactly.
// sscg_augment_colour_u8 is the same launch with a per-sample colour table between the warp and the normalisation (COLOUR
// instantiations of the same kernel body), in front of it - only when the table uses the image mean - a pass that sums the warped
// integer pixels of every sample.
// sscg_augment_elastic_u8 adds a free-form deformation to the affine source coordinate (ELASTIC instantiations of the same three
// kernels): a cubic B-spline over a coarse lattice of int32 control nodes per sample, integers throughout.
// sscg_augment_mix_u8 composes two samples (CutMix, ClassMix) inside the same launch (MIX instantiations of the apply kernel): a
// table row per sample names a partner, a box and a class mask, and every output pixel is its own sample's or the partner's.
#include <type_traits>

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

// The colour table of one sample as the apply pass holds it: A row-major and o = B.mu + b, which no pixel changes.  One-channel images
// are scalar: [0][0] and [0] of the [N][21] table.
template <int C> struct aug_col { float A[C * C]; float o[C]; };

// (m0*x0 + m1*x1) + m2*x2 + last, every product and sum rounded on its own.  hip's __fmul_rn / __fadd_rn are a plain * and + once
// inlined and would fuse under the default -ffp-contract, so the expression is written here with contraction switched off.
template <int C>
__device__ __forceinline__ float aug_row(const float* m, const float* x, float last) {
#pragma clang fp contract(off)
    float s = m[0] * x[0];
    if constexpr (C == 3) {
        s = s + m[1] * x[1];
        s = s + m[2] * x[2];
    }
    return s + last;
}

// `sums` = null: no mean (mu = 0)
template <int C>
__device__ __forceinline__ aug_col<C> aug_load_col(const float* __restrict__ colour, const int64_t* __restrict__ sums, int n, double denom) {
    const float* t = colour + (size_t)n * 21;
    float mu[C];
#pragma unroll
    for (int c = 0; c < C; ++c) mu[c] = sums ? (float)__ddiv_rn((double)sums[(size_t)n * 3 + c], denom) : 0.f;
    aug_col<C> k;
#pragma unroll
    for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int j = 0; j < C; ++j) k.A[c * C + j] = t[c * 3 + j];
        k.o[c] = aug_row<C>(t + 9 + c * 3, mu, t[18 + c]);
    }
    return k;
}

// the four taps of output pixel (n, oy, ox) at Q16 source coordinates (sx, sy): 8-bit weights, in-range flags, the upper-left address
template <int C>
struct aug_taps {
    int fx, fy;
    bool inx0, inx1, iny0, iny1;
    const uint8_t *p00, *p10;

    __device__ __forceinline__ aug_taps(const uint8_t* __restrict__ img, const aug_geom& g, size_t plane, int64_t sx, int64_t sy) {
        const int64_t x0 = sx >> 16, y0 = sy >> 16;
        fx = (int)(sx & 0xFFFF) >> 8, fy = (int)(sy & 0xFFFF) >> 8;
        // a tap whose weight is zero is never read: its product is an exact 0 whatever the byte
        inx0 = (uint64_t)x0 < (uint64_t)g.W, inx1 = fx != 0 && (uint64_t)(x0 + 1) < (uint64_t)g.W;
        iny0 = (uint64_t)y0 < (uint64_t)g.H, iny1 = fy != 0 && (uint64_t)(y0 + 1) < (uint64_t)g.H;
        p00 = img + (plane + (size_t)(y0 * g.W + x0)) * C;                  // dereferenced only under its in-range flags
        p10 = p00 + (size_t)g.W * C;
    }
    // the integer value of channel c
    __device__ __forceinline__ int value(int c, int image_fill) const {
        const int v00 = (iny0 && inx0) ? p00[c] : image_fill;
        const int v01 = (iny0 && inx1) ? p00[C + c] : image_fill;
        const int v10 = (iny1 && inx0) ? p10[c] : image_fill;
        const int v11 = (iny1 && inx1) ? p10[C + c] : image_fill;
        const int top = v00 * (256 - fx) + v01 * fx;
        const int bot = v10 * (256 - fx) + v11 * fx;
        return top * (256 - fy) + bot * fy;                                 // < 2^24: exact in fp32
    }
};

// ---- the elastic term (include/sscg.h, sscg_augment_elastic_u8): what an elastic launch adds to the arguments, and its arithmetic
struct aug_elastic_args {
    const int32_t* nodes;    // [N][GH][GW][2]
    int grid, GH, GW;
};

// the displacement of one pixel, Q16 source pixels (zero in the launches without a lattice, where it folds away)
struct aug_disp { int32_t x, y; };

// the four B-spline numerators at t in 0..255, over D = 6 * 2^24: non-negative, each below 2^27
__device__ __forceinline__ void aug_bspline(int t, int32_t* n) {
    const int u = 256 - t, t2 = t * t, t3 = t2 * t;
    n[0] = u * u * u;
    n[1] = 3 * t3 - 1536 * t2 + (4 << 24);
    n[2] = -3 * t3 + 768 * t2 + 196608 * t + (1 << 24);
    n[3] = t3;
}

// floor((s + D/2) / D), D = 3 * 2^25, for |s| <= D * 2^26: the arithmetic shift floors, what it leaves is below 2^28 in magnitude, so
// the floor division by 3 is an unsigned 32-bit one behind an offset of 3 * 2^28
__device__ __forceinline__ int32_t aug_div_d(int64_t s) {
    const int32_t v = (int32_t)((s + (3ll << 24)) >> 25);
    return (int32_t)((uint32_t)(v + (3 << 28)) / 3u) - (1 << 28);
}

// the y pass of one node column: p = &node[cy][cx + j][0], `row` = GW * 2 int32 to the node below
__device__ __forceinline__ aug_disp aug_ypass(const int32_t* __restrict__ p, int row, const int32_t* ny) {
    int64_t sx = 0, sy = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        sx += (int64_t)ny[i] * p[(size_t)i * row];
        sy += (int64_t)ny[i] * p[(size_t)i * row + 1];
    }
    return {aug_div_d(sx), aug_div_d(sy)};
}

// the x pass over four consecutive columns of the y pass
__device__ __forceinline__ aug_disp aug_xpass(const aug_disp* c, int tx) {
    int32_t nx[4];
    aug_bspline(tx, nx);
    int64_t sx = 0, sy = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        sx += (int64_t)nx[j] * c[j].x;
        sy += (int64_t)nx[j] * c[j].y;
    }
    return {aug_div_d(sx), aug_div_d(sy)};
}

// one pixel on its own: both passes
__device__ __forceinline__ aug_disp aug_elastic_pixel(const aug_elastic_args& el, int n, int oy, int ox) {
    const int cy = oy / el.grid, cx = ox / el.grid;
    const int ty = ((oy - cy * el.grid) * 256) / el.grid, tx = ((ox - cx * el.grid) * 256) / el.grid;
    int32_t ny[4];
    aug_bspline(ty, ny);
    const int row = el.GW * 2;
    const int32_t* p = el.nodes + (((size_t)n * el.GH + cy) * el.GW + cx) * 2;
    aug_disp c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = aug_ypass(p + j * 2, row, ny);
    return aug_xpass(c, tx);
}

// The same as a call, for the rare pixels of the apply pass that take it (groups that straddle a row or a sample, the scalar tail):
// inlined four times beside the row path it costs the kernel 194 VGPRs and 1700 instructions; as a call the kernel has 80 to 100
// VGPRs, as the affine ones (no difference in time was measured between the two: profiles/augment_elastic.txt).  Arguments by
// value: they travel in registers, the kernel needs no stack.
__device__ __noinline__ aug_disp aug_elastic_pixel_call(aug_elastic_args el, int n, int oy, int ox) { return aug_elastic_pixel(el, n, oy, ox); }

// four consecutive pixels of one row, (oy, ox) .. (oy, ox + 3) with ox + 3 < OW: at grid >= 4 they lie in at most two cells, so the y
// pass runs once per node column - four, or five when the group crosses into the next cell (only then does the fifth exist).
// MASKED (a mix launch, where a pixel has one source sample): a pixel whose bit of `need` is clear takes no x pass, d[e] stays
template <bool MASKED = false>
__device__ __forceinline__ void aug_elastic_row4(const aug_elastic_args& el, int n, int oy, int ox, aug_disp* d, unsigned need = 0xF) {
    const int cy = oy / el.grid, cx = ox / el.grid;
    const int ty = ((oy - cy * el.grid) * 256) / el.grid;
    const int rem = ox - cx * el.grid;
    int32_t ny[4];
    aug_bspline(ty, ny);
    const int row = el.GW * 2;
    const int32_t* p = el.nodes + (((size_t)n * el.GH + cy) * el.GW + cx) * 2;
    aug_disp c[5];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = aug_ypass(p + j * 2, row, ny);
    c[4] = {0, 0};
    if (rem + 3 >= el.grid) c[4] = aug_ypass(p + 8, row, ny);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const bool next = rem + e >= el.grid;
        const int r = next ? rem + e - el.grid : rem + e;
        aug_disp w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = next ? c[j + 1] : c[j];
        if constexpr (MASKED) {
            if (need >> e & 1) d[e] = aug_xpass(w, (r * 256) / el.grid);
        } else d[e] = aug_xpass(w, (r * 256) / el.grid);
    }
}

// the argument of type T among the trailing ones of a launch, or an empty one
template <typename T>
__device__ __forceinline__ T aug_pick() { return T{}; }
template <typename T, typename A0, typename... A>
__device__ __forceinline__ T aug_pick(A0 a0, A... a) {
    if constexpr (std::is_same_v<T, A0>) return a0;
    else return aug_pick<T>(a...);
}

// one output pixel (n, oy, ox): C normalised channels into out[], the raw source label id as the return value (LABEL only)
template <int C, bool LABEL, bool COLOUR, bool ELASTIC>
__device__ __forceinline__ int aug_pixel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ gt, const aug_mat& a, const aug_col<C>& k,
                                         const aug_geom& g, int n, int oy, int ox, aug_disp d, const float* mean, const float* stdev,
                                         float* out) {
    int64_t sx = (int64_t)a.m[0] * ox + (int64_t)a.m[1] * oy + a.m[2];
    int64_t sy = (int64_t)a.m[3] * ox + (int64_t)a.m[4] * oy + a.m[5];
    if constexpr (ELASTIC) { sx += d.x; sy += d.y; }
    const size_t plane = (size_t)n * g.H * g.W;
    // ---- image
    const aug_taps<C> taps(img, g, plane, sx, sy);
    float tc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int v = taps.value(c, g.image_fill);
        const float t = __fdiv_rn(__fmul_rn((float)v, 0x1p-16f), 255.0f);
        if constexpr (COLOUR) tc[c] = t;
        else out[c] = __fdiv_rn(__fsub_rn(t, mean[c]), stdev[c]);
    }
    if constexpr (COLOUR) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float u = fminf(fmaxf(aug_row<C>(k.A + c * C, tc, k.o[c]), 0.f), 1.f);
            out[c] = __fdiv_rn(__fsub_rn(u, mean[c]), stdev[c]);
        }
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

// what a colour launch adds to the arguments
struct aug_colour_args {
    const float* table;      // [N][21]
    const int64_t* sums;     // [N][3] from the sum pass, or null = no mean
};

// ---- mixing (include/sscg.h, sscg_augment_mix_u8): what a mix launch adds to the arguments, and the decision per pixel
struct aug_mix_args {
    const int32_t* table;    // [N][8] = (partner, x0, y0, x1, y1, mask_lo, mask_hi, 0)
    int N, classes;
};

// one sample's row of the table beside what a pasted pixel is made from: the partner's matrix and colour table.  They travel with
// the sample's own and are reloaded wherever those are.
template <int C>
struct aug_mix {
    int p;                   // the partner, or -1: the sample is not mixed (whatever the table holds, nothing else indexes memory)
    int x0, y0, x1, y1;
    uint64_t mask;
    aug_mat a;
    aug_col<C> k;

    __device__ __forceinline__ bool in_box(int oy, int ox) const { return p >= 0 && ox >= x0 && ox < x1 && oy >= y0 && oy < y1; }
};

template <int C, bool COLOUR>
__device__ __forceinline__ aug_mix<C> aug_load_mix(const aug_mix_args& mx, const int32_t* __restrict__ mats, const float* __restrict__ colour,
                                                   const int64_t* __restrict__ sums, int n, double denom) {
    const int32_t* r = mx.table + (size_t)n * 8;
    aug_mix<C> m = {};
    m.p = r[0];
    if ((uint32_t)m.p >= (uint32_t)mx.N || m.p == n) m.p = -1;
    m.x0 = r[1], m.y0 = r[2], m.x1 = r[3], m.y1 = r[4];
    m.mask = ((uint64_t)(uint32_t)r[6] << 32) | (uint32_t)r[5];
    if (m.p >= 0) {
        m.a = aug_load_mat(mats, m.p);
        if constexpr (COLOUR) m.k = aug_load_col<C>(colour, sums, m.p, denom);
    }
    return m;
}

// the class rule at (oy, ox) of a mixed sample: the partner's raw id there - its own map, its own displacement d, the label rule of
// aug_pixel - through the table `t`; a class outside 0..63 never pastes
template <int C>
__device__ __forceinline__ bool aug_mix_class(const aug_mix<C>& m, const uint8_t* __restrict__ gt, const aug_geom& g, int oy, int ox, aug_disp d,
                                              const int64_t* t) {
    const int64_t sx = (int64_t)m.a.m[0] * ox + (int64_t)m.a.m[1] * oy + m.a.m[2] + d.x;
    const int64_t sy = (int64_t)m.a.m[3] * ox + (int64_t)m.a.m[4] * oy + m.a.m[5] + d.y;
    const int64_t ix = (sx + 0x8000) >> 16, iy = (sy + 0x8000) >> 16;
    int id = g.label_fill;
    if ((uint64_t)ix < (uint64_t)g.W && (uint64_t)iy < (uint64_t)g.H) id = gt[(size_t)m.p * g.H * g.W + (size_t)(iy * g.W + ix)];
    const int64_t cls = t[id];
    return (uint64_t)cls < 64u && (m.mask >> cls & 1) != 0;
}

// One pixel of sample n on its own: is it pasted - and, with a lattice, the displacement `d` of the sample it then comes from.  The
// partner's is evaluated only where the partner's coordinate is needed (in the box, or anywhere under the class rule), the own only
// for an unpasted pixel.
template <int C, bool LABEL, bool ELASTIC>
__device__ __forceinline__ bool aug_mix_pixel(const aug_mix<C>& m, int classes, const aug_elastic_args& el, const uint8_t* __restrict__ gt,
                                              const aug_geom& g, int n, int oy, int ox, const int64_t* t, aug_disp& d) {
    bool paste = m.in_box(oy, ox);
    const bool partner = paste || (LABEL && classes != 0 && m.p >= 0);
    aug_disp dp = {};
    if constexpr (ELASTIC) {
        if (partner) dp = aug_elastic_pixel_call(el, m.p, oy, ox);
    }
    if constexpr (LABEL) {
        if (partner && !paste) paste = aug_mix_class<C>(m, gt, g, oy, ox, dp, t);
    }
    if constexpr (ELASTIC) d = paste ? dp : aug_elastic_pixel_call(el, n, oy, ox);
    return paste;
}

// Every thread owns four consecutive pixels of the flat [N * OH * OW] range (a group may straddle a row or a sample) and stores them
// as 16-byte vectors: 4 * C floats = C stores, four labels = two stores.  `groups` = 0 sends every pixel down the scalar tail.
// The colour flag is the argument pack: COL is empty - the plain launch, whose arguments and with them whose instruction stream are
// those it had before the colour instantiations existed - or aug_colour_args, and then the sample's colour table travels with its
// matrix and is reloaded wherever the matrix is - and / or aug_elastic_args, and then every pixel's source coordinate takes the
// displacement of the sample's lattice: one y pass per group where its four pixels share a row, pixel by pixel elsewhere - and / or
// aug_mix_args, and then every pixel first decides which sample it shows, its own or (pasted) the sample's partner, and aug_pixel
// runs once, for that one: same taps, same stores.
template <int C, bool LABEL, typename... COL>
__global__ __launch_bounds__(AUG_THREADS) void augment_u8_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ gt,
                                                                 const int32_t* __restrict__ mats, float* __restrict__ out_img,
                                                                 int64_t* __restrict__ out_gt, const float* __restrict__ mean,
                                                                 const float* __restrict__ stdev, const int64_t* __restrict__ lut,
                                                                 aug_geom g, uint32_t total, uint32_t groups, COL... col) {
    constexpr bool COLOUR = (std::is_same_v<COL, aug_colour_args> || ...);
    constexpr bool ELASTIC = (std::is_same_v<COL, aug_elastic_args> || ...);
    constexpr bool MIX = (std::is_same_v<COL, aug_mix_args> || ...);
    const aug_mix_args mx = aug_pick<aug_mix_args>(col...);
    const aug_colour_args ca = aug_pick<aug_colour_args>(col...);
    const float* colour = ca.table;
    const int64_t* sums = ca.sums;
    const aug_elastic_args el = aug_pick<aug_elastic_args>(col...);
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
    double denom = 0.0;
    if constexpr (COLOUR) denom = __dmul_rn((double)hw, 16711680.0);
    for (uint32_t q = blockIdx.x * AUG_THREADS + threadIdx.x; q < groups; q += stride) {
        const uint32_t p0 = q * 4;
        int n = (int)(p0 / hw);
        const uint32_t r = p0 - (uint32_t)n * hw;
        int oy = (int)(r / (uint32_t)g.OW);
        int ox = (int)(r - (uint32_t)oy * (uint32_t)g.OW);
        aug_mat a = aug_load_mat(mats, n);
        aug_col<C> k;
        if constexpr (COLOUR) k = aug_load_col<C>(colour, sums, n, denom);
        float v[4 * C];
        int64_t lab[4];
        aug_disp d[4] = {};
        aug_mix<C> m;
        unsigned pasted = 0;                        // MIX with a lattice, four pixels of one row: decided here, with the shared y pass
        bool row = false;
        if constexpr (MIX) {
            m = aug_load_mix<C, COLOUR>(mx, mats, colour, sums, n, denom);
            if constexpr (ELASTIC) {
                if ((row = ox + 3 < g.OW)) {
                    unsigned box = 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) box |= (unsigned)m.in_box(oy, ox + e) << e;
                    const unsigned partner = m.p < 0 ? 0u : (LABEL && mx.classes != 0) ? 0xFu : box;
                    aug_disp dp[4] = {};
                    if (partner) aug_elastic_row4<true>(el, m.p, oy, ox, dp, partner);
                    pasted = box;
                    if constexpr (LABEL) {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if ((partner & ~box) >> e & 1) pasted |= (unsigned)aug_mix_class<C>(m, gt, g, oy, ox + e, dp[e], t) << e;
                    }
                    if (pasted != 0xF) aug_elastic_row4<true>(el, n, oy, ox, d, ~pasted & 0xF);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (pasted >> e & 1) d[e] = dp[e];
                }
            }
        }
        if constexpr (ELASTIC && !MIX) {
            if (ox + 3 < g.OW) {
                aug_elastic_row4(el, n, oy, ox, d);
            } else {                                // the group straddles a row or a sample: pixel by pixel, walking as the loop below
                int dn = n, dy = oy, dx = ox;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    d[e] = aug_elastic_pixel_call(el, dn, dy, dx);
                    if (e < 3 && ++dx == g.OW) {
                        dx = 0;
                        if (++dy == g.OH) { dy = 0; ++dn; }
                    }
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            bool paste = false;
            if constexpr (MIX) paste = row ? (pasted >> e & 1) != 0 : aug_mix_pixel<C, LABEL, ELASTIC>(m, mx.classes, el, gt, g, n, oy, ox, t, d[e]);
            const int id = aug_pixel<C, LABEL, COLOUR, ELASTIC>(img, gt, paste ? m.a : a, paste ? m.k : k, g, paste ? m.p : n, oy, ox, d[e], mu, sd,
                                                                v + e * C);
            if constexpr (LABEL) lab[e] = t[id];
            if (e < 3 && ++ox == g.OW) {
                ox = 0;
                if (++oy == g.OH) {                 // the next pixel of the group is in range: p0 + 3 < total
                    oy = 0;
                    a = aug_load_mat(mats, ++n);
                    if constexpr (COLOUR) k = aug_load_col<C>(colour, sums, n, denom);
                    if constexpr (MIX) m = aug_load_mix<C, COLOUR>(mx, mats, colour, sums, n, denom);
                }
            }
        }
        f32x4* o = reinterpret_cast<f32x4*>(out_img + (size_t)p0 * C);
#pragma unroll
        for (int k4 = 0; k4 < C; ++k4) o[k4] = f32x4{v[4 * k4], v[4 * k4 + 1], v[4 * k4 + 2], v[4 * k4 + 3]};
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
        aug_col<C> k;
        if constexpr (COLOUR) k = aug_load_col<C>(colour, sums, n, denom);
        float v[C];
        aug_disp d = {};
        aug_mix<C> m;
        bool paste = false;
        if constexpr (MIX) {
            m = aug_load_mix<C, COLOUR>(mx, mats, colour, sums, n, denom);
            paste = aug_mix_pixel<C, LABEL, ELASTIC>(m, mx.classes, el, gt, g, n, oy, ox, t, d);
        } else if constexpr (ELASTIC) d = aug_elastic_pixel_call(el, n, oy, ox);
        const int id = aug_pixel<C, LABEL, COLOUR, ELASTIC>(img, gt, paste ? m.a : a, paste ? m.k : k, g, paste ? m.p : n, oy, ox, d, mu, sd, v);
#pragma unroll
        for (int c = 0; c < C; ++c) out_img[(size_t)p * C + c] = v[c];
        if constexpr (LABEL) out_gt[p] = t[id];
    }
}

// ---- the sum pass of the image mean: sums[n][c] += the integer values v[c] of the sample's OH * OW warped pixels.  blockIdx.y is the
// sample, so a block never straddles two; a block covers AUG_THREADS consecutive pixels per round of its loop and the grid is sized for
// AUG_SUM_ROUNDS rounds.  Wave sum, the block's four waves through LDS, one 64-bit integer atomic per channel and block: integer
// sums do not depend on the order, so the result is exact and the same in every run.
constexpr int AUG_SUM_ROUNDS = 4;
constexpr int AUG_SUM_MAX_BLOCKS = 2048;      // 8 per CU: the pass is a latency-bound gather in ~32 VGPRs, so every wave slot is used

__global__ __launch_bounds__(AUG_THREADS) void augment_zero_kernel(int64_t* __restrict__ sums, int n) {
    for (int i = blockIdx.x * AUG_THREADS + threadIdx.x; i < n; i += gridDim.x * AUG_THREADS) sums[i] = 0;
}

// EL is empty - the affine pass, with the arguments it had before the elastic one existed - or aug_elastic_args
template <int C, typename... EL>
__global__ __launch_bounds__(AUG_THREADS) void augment_sum_kernel(const uint8_t* __restrict__ img, const int32_t* __restrict__ mats, aug_geom g,
                                                                  int64_t* __restrict__ sums, EL... ela) {
    constexpr bool ELASTIC = sizeof...(EL) != 0;
    __shared__ int64_t part[AUG_THREADS / 64][C];
    const int n = blockIdx.y;
    const aug_mat a = aug_load_mat(mats, n);
    const size_t plane = (size_t)n * g.H * g.W;
    const uint32_t hw = (uint32_t)g.OH * (uint32_t)g.OW;
    int64_t s[C];
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = 0;
    for (uint32_t p = blockIdx.x * AUG_THREADS + threadIdx.x; p < hw; p += gridDim.x * AUG_THREADS) {
        const int oy = (int)(p / (uint32_t)g.OW);
        const int ox = (int)(p - (uint32_t)oy * (uint32_t)g.OW);
        int64_t sx = (int64_t)a.m[0] * ox + (int64_t)a.m[1] * oy + a.m[2];
        int64_t sy = (int64_t)a.m[3] * ox + (int64_t)a.m[4] * oy + a.m[5];
        if constexpr (ELASTIC) {
            const aug_disp d = aug_elastic_pixel(aug_pick<aug_elastic_args>(ela...), n, oy, ox);
            sx += d.x;
            sy += d.y;
        }
        const aug_taps<C> taps(img, g, plane, sx, sy);
#pragma unroll
        for (int c = 0; c < C; ++c) s[c] += taps.value(c, g.image_fill);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[c] += __shfl_xor((long long)s[c], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) part[threadIdx.x >> 6][c] = s[c];
    }
    __syncthreads();
    if (threadIdx.x < C) {
        int64_t tot = 0;
#pragma unroll
        for (int w = 0; w < AUG_THREADS / 64; ++w) tot += part[w][threadIdx.x];
        atomicAdd(reinterpret_cast<unsigned long long*>(sums + (size_t)n * 3 + threadIdx.x), (unsigned long long)tot);
    }
}

// `el`: the trailing arguments of the apply kernel - nothing, or any of aug_colour_args, aug_elastic_args, aug_mix_args, in that order
template <int C, typename... EL>
void aug_launch(bool label, dim3 grid, hipStream_t st, const uint8_t* img, const uint8_t* gt, const int32_t* mats, float* out_img,
                int64_t* out_gt, const float* mean, const float* stdev, const int64_t* lut, const aug_geom& g, uint32_t total,
                uint32_t groups, EL... el) {
    if (label)
        hipLaunchKernelGGL((augment_u8_kernel<C, true, EL...>), grid, dim3(AUG_THREADS), 0, st, img, gt, mats, out_img, out_gt, mean, stdev, lut, g,
                           total, groups, el...);
    else
        hipLaunchKernelGGL((augment_u8_kernel<C, false, EL...>), grid, dim3(AUG_THREADS), 0, st, img, gt, mats, out_img, out_gt, mean, stdev, lut, g,
                           total, groups, el...);
}

// the two launches in front of a colour launch whose table uses the image mean
template <int C, typename... EL>
void aug_launch_sums(hipStream_t st, const uint8_t* img, const int32_t* mats, const aug_geom& g, int64_t* sums, int N, EL... el) {
    const uint32_t hw = (uint32_t)g.OH * (uint32_t)g.OW;
    const int cap = AUG_SUM_MAX_BLOCKS / N > 0 ? AUG_SUM_MAX_BLOCKS / N : 1;
    int bx = cdiv((long)hw, (long)AUG_THREADS * AUG_SUM_ROUNDS);
    if (bx > cap) bx = cap;
    hipLaunchKernelGGL(augment_zero_kernel, dim3(ew_blocks((size_t)N * 3, 64)), dim3(AUG_THREADS), 0, st, sums, N * 3);
    hipLaunchKernelGGL((augment_sum_kernel<C, EL...>), dim3(bx, N), dim3(AUG_THREADS), 0, st, img, mats, g, sums, el...);
}

template <int C, typename... EL>
void aug_launch_colour(bool label, dim3 grid, hipStream_t st, const uint8_t* img, const uint8_t* gt, const int32_t* mats, float* out_img,
                       int64_t* out_gt, const float* mean, const float* stdev, const int64_t* lut, const aug_geom& g, uint32_t total,
                       uint32_t groups, const float* colour, int64_t* sums, int N, EL... el) {
    if (sums) aug_launch_sums<C>(st, img, mats, g, sums, N, el...);
    aug_launch<C>(label, grid, st, img, gt, mats, out_img, out_gt, mean, stdev, lut, g, total, groups, aug_colour_args{colour, sums}, el...);
}

// a mix launch: the sum pass is that of the launch without the table (every sample's mean is that of its own unmixed pixels), the
// apply pass takes the table behind whatever of the colour table and the lattice there is.  colour / el: null = none
template <int C>
void aug_launch_mix(bool label, dim3 grid, hipStream_t st, const uint8_t* img, const uint8_t* gt, const int32_t* mats, float* out_img,
                    int64_t* out_gt, const float* mean, const float* stdev, const int64_t* lut, const aug_geom& g, uint32_t total, uint32_t groups,
                    const float* colour, int64_t* sums, int N, const aug_elastic_args* el, const aug_mix_args& mx) {
    if (sums) {
        if (el) aug_launch_sums<C>(st, img, mats, g, sums, N, *el);
        else aug_launch_sums<C>(st, img, mats, g, sums, N);
    }
    const aug_colour_args ca = {colour, sums};
    if (colour && el) aug_launch<C>(label, grid, st, img, gt, mats, out_img, out_gt, mean, stdev, lut, g, total, groups, ca, *el, mx);
    else if (colour) aug_launch<C>(label, grid, st, img, gt, mats, out_img, out_gt, mean, stdev, lut, g, total, groups, ca, mx);
    else if (el) aug_launch<C>(label, grid, st, img, gt, mats, out_img, out_gt, mean, stdev, lut, g, total, groups, *el, mx);
    else aug_launch<C>(label, grid, st, img, gt, mats, out_img, out_gt, mean, stdev, lut, g, total, groups, mx);
}

// the argument rules both entries share; 0 = go on
int aug_check(const uint8_t* img, const uint8_t* gt, const int32_t* mats, const float* out_img, const int64_t* out_gt, int N, int H, int W,
              int C, int OH, int OW, const float* mean, const float* stdev, const int64_t* lut256, int image_fill, int label_fill) {
    if (!img || !mats || !out_img || !mean || !stdev) return SSCG_ERR_BAD_ARG;
    if (C < 1 || C > 4 || N <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return SSCG_ERR_BAD_ARG;
    if (image_fill < 0 || image_fill > 255 || label_fill < 0 || label_fill > 255) return SSCG_ERR_BAD_ARG;
    if (gt ? (!lut256 || !out_gt) : out_gt != nullptr) return SSCG_ERR_BAD_ARG;
    const int64_t total = (int64_t)N * OH * OW;
    if (total >= ((int64_t)1 << 31) || H > 32767 || W > 32767) return SSCG_ERR_UNSUPPORTED;
    return SSCG_OK;
}

// groups of four and the grid of the apply pass
uint32_t aug_plan(const float* out_img, const int64_t* out_gt, int64_t total, uint32_t* groups) {
    // the 16-byte stores need 16-byte aligned outputs (every group starts a multiple of 16 bytes behind them)
    const bool aligned = (((size_t)out_img | (size_t)out_gt) & 15) == 0;
    *groups = aligned ? (uint32_t)(total / 4) : 0u;
    const uint32_t work = *groups ? *groups + (uint32_t)(total - (int64_t)*groups * 4 > 0) : (uint32_t)total;
    uint32_t blocks = (work + AUG_THREADS - 1) / AUG_THREADS;
    return blocks > AUG_MAX_BLOCKS ? AUG_MAX_BLOCKS : blocks;
}

}  // namespace

extern "C" int sscg_augment_u8(const uint8_t* img, const uint8_t* gt, const int32_t* mats, float* out_img, int64_t* out_gt, int N, int H,
                               int W, int C, int OH, int OW, const float* mean, const float* stdev, const int64_t* lut256, int image_fill,
                               int label_fill, void* stream) {
    const int bad = aug_check(img, gt, mats, out_img, out_gt, N, H, W, C, OH, OW, mean, stdev, lut256, image_fill, label_fill);
    if (bad) return bad;
    const int64_t total = (int64_t)N * OH * OW;
    uint32_t groups;
    const uint32_t blocks = aug_plan(out_img, out_gt, total, &groups);
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

extern "C" size_t sscg_augment_colour_workspace(int N) { return N > 0 ? (size_t)N * 3 * sizeof(int64_t) : 0; }

extern "C" int sscg_augment_colour_u8(const uint8_t* img, const uint8_t* gt, const int32_t* mats, float* out_img, int64_t* out_gt, int N,
                                      int H, int W, int C, int OH, int OW, const float* mean, const float* stdev, const int64_t* lut256,
                                      int image_fill, int label_fill, const float* colour, int need_mean, void* ws, void* stream) {
    const int bad = aug_check(img, gt, mats, out_img, out_gt, N, H, W, C, OH, OW, mean, stdev, lut256, image_fill, label_fill);
    if (bad == SSCG_ERR_BAD_ARG) return bad;
    if (!colour || (need_mean && (!ws || ((size_t)ws & 7) != 0))) return SSCG_ERR_BAD_ARG;
    if (bad) return bad;
    // the sum pass takes the sample from blockIdx.y
    if (C == 2 || C == 4 || (need_mean && N > 65535)) return SSCG_ERR_UNSUPPORTED;
    const int64_t total = (int64_t)N * OH * OW;
    uint32_t groups;
    const uint32_t blocks = aug_plan(out_img, out_gt, total, &groups);
    const aug_geom g = {H, W, OH, OW, image_fill, label_fill};
    const hipStream_t st = (hipStream_t)stream;
    const bool label = gt != nullptr;
    int64_t* sums = need_mean ? reinterpret_cast<int64_t*>(ws) : nullptr;
    if (C == 1)
        aug_launch_colour<1>(label, dim3(blocks), st, img, gt, mats, out_img, out_gt, mean, stdev, lut256, g, (uint32_t)total, groups, colour, sums, N);
    else
        aug_launch_colour<3>(label, dim3(blocks), st, img, gt, mats, out_img, out_gt, mean, stdev, lut256, g, (uint32_t)total, groups, colour, sums, N);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_augment_elastic_u8(const uint8_t* img, const uint8_t* gt, const int32_t* mats, float* out_img, int64_t* out_gt, int N,
                                       int H, int W, int C, int OH, int OW, const float* mean, const float* stdev, const int64_t* lut256,
                                       int image_fill, int label_fill, const float* colour, int need_mean, void* ws, const int32_t* nodes,
                                       int grid, int GH, int GW, void* stream) {
    const int bad = aug_check(img, gt, mats, out_img, out_gt, N, H, W, C, OH, OW, mean, stdev, lut256, image_fill, label_fill);
    if (bad == SSCG_ERR_BAD_ARG) return bad;
    if (!nodes || grid < 4 || GH != (OH - 1) / grid + 4 || GW != (OW - 1) / grid + 4) return SSCG_ERR_BAD_ARG;
    if (!colour) need_mean = 0;
    if (need_mean && (!ws || ((size_t)ws & 7) != 0)) return SSCG_ERR_BAD_ARG;
    if (bad) return bad;
    // (the position inside a cell) * 256 stays an int
    if (grid > (1 << 22) || (colour && (C == 2 || C == 4 || (need_mean && N > 65535)))) return SSCG_ERR_UNSUPPORTED;
    const int64_t total = (int64_t)N * OH * OW;
    uint32_t groups;
    const dim3 blocks(aug_plan(out_img, out_gt, total, &groups));
    const aug_geom g = {H, W, OH, OW, image_fill, label_fill};
    const hipStream_t st = (hipStream_t)stream;
    const bool label = gt != nullptr;
    const aug_elastic_args el = {nodes, grid, GH, GW};
    const uint32_t tot = (uint32_t)total;
    if (colour) {
        int64_t* sums = need_mean ? reinterpret_cast<int64_t*>(ws) : nullptr;
        if (C == 1) aug_launch_colour<1>(label, blocks, st, img, gt, mats, out_img, out_gt, mean, stdev, lut256, g, tot, groups, colour, sums, N, el);
        else aug_launch_colour<3>(label, blocks, st, img, gt, mats, out_img, out_gt, mean, stdev, lut256, g, tot, groups, colour, sums, N, el);
    } else {
        switch (C) {
            case 1: aug_launch<1>(label, blocks, st, img, gt, mats, out_img, out_gt, mean, stdev, lut256, g, tot, groups, el); break;
            case 2: aug_launch<2>(label, blocks, st, img, gt, mats, out_img, out_gt, mean, stdev, lut256, g, tot, groups, el); break;
            case 3: aug_launch<3>(label, blocks, st, img, gt, mats, out_img, out_gt, mean, stdev, lut256, g, tot, groups, el); break;
            default: aug_launch<4>(label, blocks, st, img, gt, mats, out_img, out_gt, mean, stdev, lut256, g, tot, groups, el); break;
        }
    }
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_augment_mix_u8(const uint8_t* img, const uint8_t* gt, const int32_t* mats, float* out_img, int64_t* out_gt, int N, int H,
                                   int W, int C, int OH, int OW, const float* mean, const float* stdev, const int64_t* lut256, int image_fill,
                                   int label_fill, const float* colour, int need_mean, void* ws, const int32_t* nodes, int grid, int GH, int GW,
                                   const int32_t* mix, int classes, void* stream) {
    const int bad = aug_check(img, gt, mats, out_img, out_gt, N, H, W, C, OH, OW, mean, stdev, lut256, image_fill, label_fill);
    if (bad == SSCG_ERR_BAD_ARG) return bad;
    if (!mix || (classes != 0 && !gt)) return SSCG_ERR_BAD_ARG;
    if (nodes && (grid < 4 || GH != (OH - 1) / grid + 4 || GW != (OW - 1) / grid + 4)) return SSCG_ERR_BAD_ARG;
    if (!colour) need_mean = 0;
    if (need_mean && (!ws || ((size_t)ws & 7) != 0)) return SSCG_ERR_BAD_ARG;
    if (bad) return bad;
    if (C == 2 || C == 4 || (nodes && grid > (1 << 22)) || (need_mean && N > 65535)) return SSCG_ERR_UNSUPPORTED;
    const int64_t total = (int64_t)N * OH * OW;
    uint32_t groups;
    const dim3 blocks(aug_plan(out_img, out_gt, total, &groups));
    const aug_geom g = {H, W, OH, OW, image_fill, label_fill};
    const hipStream_t st = (hipStream_t)stream;
    const bool label = gt != nullptr;
    const aug_elastic_args ela = {nodes, grid, GH, GW};
    const aug_elastic_args* el = nodes ? &ela : nullptr;
    const aug_mix_args mx = {mix, N, classes != 0};
    int64_t* sums = need_mean ? reinterpret_cast<int64_t*>(ws) : nullptr;
    if (C == 1) aug_launch_mix<1>(label, blocks, st, img, gt, mats, out_img, out_gt, mean, stdev, lut256, g, (uint32_t)total, groups, colour, sums, N, el, mx);
    else aug_launch_mix<3>(label, blocks, st, img, gt, mats, out_img, out_gt, mean, stdev, lut256, g, (uint32_t)total, groups, colour, sums, N, el, mx);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}
