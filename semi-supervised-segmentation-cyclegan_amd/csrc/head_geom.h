// The geometry of the fused label head (resize -> softmax -> losses from the low-resolution logits), shared by loss_optim.hip (the
// cross-entropy head) and dice.hip (the Dice statistics and the head backward with Dice): the launch geometry, the resized logits
// of one output pixel and the stencil weight of a source row / column.  Device code is not linked across translation units: this
// header is instantiated in each, in an unnamed namespace as the kernels that use it are.
#pragma once
#include "common.h"

namespace {

constexpr int MAXC = 64;  // class axis is 4 / 20 / 21 in the reference (model.py:205-210)

struct HeadGeom { int N, H, W, C, OH, OW; float sh, sw, inv_sh, inv_sw; };

template <int CT>
__device__ __forceinline__ void head_logits(const float* __restrict__ xn, const HeadGeom& g, int oy, int ox, int C, float* v,
                                            int* y0o, int* x0o) {
    // the arithmetic of upsample_fwd_kernel (pointwise.hip)
    const float fy = g.sh * oy, fx = g.sw * ox;
    const int y0 = (int)fy, x0 = (int)fx;
    const int yp = y0 < g.H - 1 ? 1 : 0, xp = x0 < g.W - 1 ? 1 : 0;
    const float ly = fy - y0, lx = fx - x0;
    const float hy = 1.f - ly, hx = 1.f - lx;
    const float* r00 = xn + ((size_t)y0 * g.W + x0) * C;
    const float* r01 = r00 + (size_t)xp * C;
    const float* r10 = r00 + (size_t)yp * g.W * C;
    const float* r11 = r10 + (size_t)xp * C;
#pragma unroll
    for (int c = 0; c < (CT ? CT : MAXC); ++c) {
        if (CT == 0 && c >= C) break;
        v[c] = hy * (hx * r00[c] + lx * r01[c]) + ly * (hx * r10[c] + lx * r11[c]);
    }
    *y0o = y0; *x0o = x0;
}

// weight of source row / column `i` in the stencil of output row / column `o` (upsample_bwd_kernel's)
__device__ __forceinline__ float head_weight(float scale, int o, int i, int n_src) {
    const float f = scale * o;
    const int i0 = (int)f;
    const int ip = i0 < n_src - 1 ? 1 : 0;
    const float l = f - i0;
    float w = 0.f;
    if (i0 == i) w += 1.f - l;
    if (i0 + ip == i) w += l;
    return w;
}

}  // namespace

static bool head_geom(HeadGeom* g, int N, int H, int W, int C, int OH, int OW) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C > MAXC || OH <= 0 || OW <= 0) return false;
    if ((size_t)N * H * W >= ((size_t)1 << 31)) return false;
    g->N = N; g->H = H; g->W = W; g->C = C; g->OH = OH; g->OW = OW;
    g->sh = OH > 1 ? (float)(H - 1) / (float)(OH - 1) : 0.f;
    g->sw = OW > 1 ? (float)(W - 1) / (float)(OW - 1) : 0.f;
    g->inv_sh = g->sh > 0.f ? 1.f / g->sh : (float)OH;
    g->inv_sw = g->sw > 0.f ? 1.f / g->sw : (float)OW;
    return true;
}
