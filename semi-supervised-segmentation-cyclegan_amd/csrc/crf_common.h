// The windowed pairwise kernel of the dense CRF, shared by crf.hip (the mean-field refinement, sscg_crf_head) and crf_loss.hip (the
// gated CRF loss, sscg_crf_loss_fwd): the tile geometry, the per-tap constants made on the host, the weight k(i, j) and the checks
// of an sscg_crf_params.  Device code is not linked across translation units: this header is instantiated in each.
#pragma once
#include "common.h"
#include <cmath>

constexpr int CRF_TILE = 16;                          // a workgroup of 256 threads owns CRF_TILE x CRF_TILE output pixels
constexpr int CRF_RMAX = 5;                           // radius <= 5: at most 11 x 11 - 1 = 120 taps
constexpr int CRF_SIDE = 2 * CRF_RMAX + 1;
constexpr int CRF_TAPS = CRF_SIDE * CRF_SIDE;         // the full grid, centre included (its slot is never read)
constexpr int CRF_STAGE = 4;                          // global loads a thread has in flight while a class quad is staged
constexpr int CRF_REACH_MAX = 16;                     // radius * dilation: the halo is at most 48 x 48 pixels

// The per-tap constants, made on the host, in the kernel's argument block (uniform loads): slot (dy + RMAX) * SIDE + (dx + RMAX).
struct CrfTaps {
    float spatial[CRF_TAPS];      // w_spatial * expf(-d2 * ig)
    float d2a[CRF_TAPS];          // d2 * ia
};

struct CrfGeom {
    int C, OH, OW, IC;
    int r, d, reach;          // radius, dilation, radius * dilation
    int side, pitch;          // halo side TILE + 2 * reach; its row pitch in LDS (pixels, a multiple of 16)
    int tiles_x, tiles_y;
    FastDiv dtx, dty, dside;
    float wb, ib;
};

// k(i, j) = w_bilateral * expf(-(d2 * ia + c2 * ib)) + w_spatial * expf(-d2 * ig); c2 over the (zero-padded) four guide channels.
// c2 is a sum of squares of differences and d2a / spatial depend on |dy|, |dx| only: k(i, j) == k(j, i) bit for bit.
__device__ __forceinline__ float crf_weight(const float4& a, const float4& b, float d2a, float spatial, float wb, float ib) {
    const float e0 = a.x - b.x, e1 = a.y - b.y, e2 = a.z - b.z, e3 = a.w - b.w;
    const float c2 = e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3;
    return wb * expf(-(d2a + c2 * ib)) + spatial;
}

static inline bool crf_finite_nonneg(float w) { return w >= 0.f && w < INFINITY; }

// 1 / (2 theta^2) formed in double and rounded to fp32 once; false unless theta > 0 and the result is a finite fp32 number
static inline bool crf_inv_two_theta_sq(float theta, float* out) {
    if (!(theta > 0.f)) return false;
    const float v = (float)(1.0 / (2.0 * (double)theta * (double)theta));
    *out = v;
    return v < INFINITY;
}

// The launch geometry and the tap table of one call; ia / ib / ig: crf_inv_two_theta_sq of the three thetas.
static inline void crf_setup(int C, int OH, int OW, int IC, int radius, int dilation, float w_bilateral, float w_spatial, float ia, float ib,
                             float ig, CrfGeom* geom, CrfTaps* taps) {
    CrfGeom& g = *geom;
    g.C = C; g.OH = OH; g.OW = OW; g.IC = IC;
    g.r = radius; g.d = dilation; g.reach = radius * dilation;
    g.side = CRF_TILE + 2 * g.reach;
    g.pitch = (g.side + 15) / 16 * 16;
    g.tiles_x = (OW + CRF_TILE - 1) / CRF_TILE; g.tiles_y = (OH + CRF_TILE - 1) / CRF_TILE;
    g.dtx = make_fastdiv(g.tiles_x); g.dty = make_fastdiv(g.tiles_y); g.dside = make_fastdiv(g.side);
    g.wb = w_bilateral; g.ib = ib;
    for (int dy = -CRF_RMAX; dy <= CRF_RMAX; ++dy)
        for (int dx = -CRF_RMAX; dx <= CRF_RMAX; ++dx) {
            const float d2 = (float)((dy * g.d) * (dy * g.d) + (dx * g.d) * (dx * g.d));       // <= 2 * 16^2 inside the radius: exact
            const int t = (dy + CRF_RMAX) * CRF_SIDE + dx + CRF_RMAX;
            taps->spatial[t] = w_spatial * expf(-d2 * ig);
            taps->d2a[t] = d2 * ia;
        }
}
