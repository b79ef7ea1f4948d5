// Sliding-window inference (include/sscg.h): the network run on overlapping crop-sized windows of a larger image, the windows'
// probabilities blended by a separable importance map into one label map.  Forward only; the training step never launches them.
//   sscg_window_gather:   the network input of every window (and of its mirrored twin) from the batch, a pure copy
//   sscg_predict_head_sw: the windows' low-resolution logit maps -> per covering window resize (+ mirror) -> softmax -> weighted sum ->
//                         first maximum -> int64 / uint8 label maps, confusion matrix, and / or the normalised probabilities
// Both equal the chains of separate passes bit for bit: the per-pixel arithmetic is the functions of head_common.h.
#include "common.h"
#include "head_common.h"
#include "sscg_internal.h"

namespace {

constexpr int MAX_BLOCKS = 2048;   // 8 workgroups per CU, grid-stride beyond: bounds the LDS histograms flushed per launch

// Window i of an axis sits at min(i * s, last) with last = L - w (the last window flush with the edge); (k - 1) * s >= last.
struct SwAxis {
    int s, k, last, win;
    FastDiv ds;
};

static inline SwAxis make_axis(int L, int win, int s, int k) {
    SwAxis a;
    a.s = s; a.k = k; a.last = L - win; a.win = win;
    a.ds = make_fastdiv(s);
    return a;
}

__device__ __forceinline__ int sw_pos(int i, const SwAxis& a) { return min(i * a.s, a.last); }

// the windows [lo, hi] that cover coordinate o: pos_i <= o < pos_i + win.  pos_i is non-decreasing in i and pos_{k-1} = last.
__device__ __forceinline__ void sw_cover(int o, const SwAxis& a, int& lo, int& hi) {
    hi = o >= a.last ? a.k - 1 : min(a.k - 1, fd_div(o, a.ds));
    const int t = o - a.win + 1;                 // the smallest position that still reaches o; t <= last
    lo = t <= 0 ? 0 : fd_div(t + a.s - 1, a.ds);     // ceil(t / s) <= k - 1 because (k - 1) * s >= last >= t
}

struct SwGeom {
    sscg_resize_geom px;        // H, W = the logit maps' size; OH, OW = the output; sh, sw = the scales of the resize to the WINDOW
    SwAxis ay, ax;
    int F;                      // views per window: 1, or 2 = every window also mirrored
};

// One thread per OUTPUT pixel, consecutive lanes on consecutive pixels of a row, with a loop over the windows that cover it: v[] holds
// the window's C logits / exponentials (sscg_pixel_logits), acc[] the running weighted sum of the windows' probabilities, both in
// registers (every class loop is unrolled, so no index is a run-time one; the window loops are not, they would multiply the class
// loops' code).  Lanes near a window's border walk different window counts; inside a window's core the whole wave walks the same ones.
// The logit maps are tens of kilobytes each and stay cache resident; only the outputs asked for are written.
// CT: class count at compile time (0 = any C <= SSCG_MAXC, every loop predicated on c < C).  IDENT: the maps have the window's size.
template <int CT, bool IDENT>
__global__ __launch_bounds__(256) void predict_head_sw_kernel(const float* __restrict__ x, const float* __restrict__ wy,
                                                              const float* __restrict__ wx, const float* __restrict__ ry,
                                                              const float* __restrict__ rx, float* __restrict__ prob,
                                                              int64_t* __restrict__ index, uint8_t* __restrict__ label_u8,
                                                              const int64_t* __restrict__ lt, unsigned long long* __restrict__ hist,
                                                              int total, SwGeom g) {
    extern __shared__ unsigned int bins[];      // [C][C] counts of this workgroup (hist != NULL only)
    const int C = CT ? CT : g.px.C;
    const int nb = hist ? C * C : 0;
    sscg_bins_clear(bins, nb);
    for (int o = blockIdx.x * 256 + threadIdx.x; o < total; o += gridDim.x * 256) {
        const sscg_pixel p = sscg_pixel_of(o, g.px);
        int y_lo, y_hi, x_lo, x_hi;
        sw_cover(p.oy, g.ay, y_lo, y_hi);
        sw_cover(p.ox, g.ax, x_lo, x_hi);
        float acc[CT ? CT : SSCG_MAXC] = {};
        bool first = true;
#pragma nounroll
        for (int iy = y_lo; iy <= y_hi; ++iy) {
            const int ly = p.oy - sw_pos(iy, g.ay);
            const float gy = wy[ly];
#pragma nounroll
            for (int ix = x_lo; ix <= x_hi; ++ix) {
                const int lx = p.ox - sw_pos(ix, g.ax);
                const float gw = gy * wx[lx];            // feeds multiplies only: nothing to contract
                const int base = ((p.n * g.ay.k + iy) * g.ax.k + ix) * g.F;
#pragma nounroll
                for (int f = 0; f < g.F; ++f) {
                    const int lxs = f ? g.ax.win - 1 - lx : lx;          // a mirrored view's map is in mirrored coordinates
                    float v[CT ? CT : SSCG_MAXC];
                    sscg_pixel_logits<CT, IDENT>(x, base + f, ly, lxs, g.px.H, g.px.W, g.px.sh, g.px.sw, C, v);
                    const float inv = sscg_softmax_exp<CT>(v, C);
                    sscg_prob_accumulate_weighted<CT>(acc, v, inv, gw, C, first);
                    first = false;
                }
            }
        }
        if (prob) {
            float* q = prob + (size_t)o * C;
            const float r = ry[p.oy] * rx[p.ox];          // two multiplies, each rounded: no add follows, nothing contracts
#pragma unroll
            for (int c = 0; c < (CT ? CT : SSCG_MAXC); ++c)
                if (CT || c < C) q[c] = acc[c] * r;
        }
        const int bi = sscg_first_max<CT>(acc, C);
        if (index) index[o] = bi;
        if (label_u8) label_u8[o] = (uint8_t)bi;
        if (hist) sscg_bins_count(bins, C, lt[o], bi);
    }
    sscg_bins_flush(bins, nb, hist);
}

struct GatherGeom {
    int H, W, C, F;
    SwAxis ay, ax;
};

// One thread per output ELEMENT (window, ly, lx, c), the 64-bit element index split by plain divisions.
__global__ __launch_bounds__(256) void window_gather_kernel(const float* __restrict__ x, float* __restrict__ y, size_t total, GatherGeom g) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % g.C);
        size_t t = i / g.C;
        const int lx = (int)(t % g.ax.win); t /= g.ax.win;
        const int ly = (int)(t % g.ay.win); t /= g.ay.win;
        const int f = (int)(t % g.F); t /= g.F;
        const int ix = (int)(t % g.ax.k); t /= g.ax.k;
        const int iy = (int)(t % g.ay.k);
        const int n = (int)(t / g.ay.k);
        const int sy = sw_pos(iy, g.ay) + ly;                              // <= last + win - 1 = H - 1
        const int sx = sw_pos(ix, g.ax) + (f ? g.ax.win - 1 - lx : lx);
        y[i] = x[(((size_t)n * g.H + sy) * g.W + sx) * g.C + c];
    }
}

// the checks both entries share: sizes, and windows that cover the axes
static inline bool sw_axes_ok(int L_y, int L_x, int wh, int ww, int sy, int sx, int ky, int kx) {
    if (L_y <= 0 || L_x <= 0 || wh <= 0 || ww <= 0 || sy <= 0 || sx <= 0 || ky <= 0 || kx <= 0) return false;
    if (wh > L_y || ww > L_x || sy > L_y || sx > L_x) return false;      // (a stride beyond the axis serves no window)
    return (int64_t)(ky - 1) * sy >= (int64_t)(L_y - wh) && (int64_t)(kx - 1) * sx >= (int64_t)(L_x - ww);
}

}  // namespace

extern "C" int sscg_window_gather(const float* x, float* y, int N, int H, int W, int C, int wh, int ww, int sy, int sx, int ky, int kx,
                                  int flip, void* stream) {
    if (!x || !y || N <= 0 || C <= 0 || !sw_axes_ok(H, W, wh, ww, sy, sx, ky, kx)) return SSCG_ERR_BAD_ARG;
    const int F = flip ? 2 : 1;
    const size_t windows = (size_t)N * ky * kx * F;
    if (H >= (1 << 30) || W >= (1 << 30) || windows >= ((size_t)1 << 31) || (size_t)ky * sy >= ((size_t)1 << 31) || (size_t)kx * sx >= ((size_t)1 << 31)) return SSCG_ERR_UNSUPPORTED;
    GatherGeom g;
    g.H = H; g.W = W; g.C = C; g.F = F;
    g.ay = make_axis(H, wh, sy, ky); g.ax = make_axis(W, ww, sx, kx);
    const size_t total = windows * wh * ww * C;
    const dim3 grid(ew_blocks(total)), blk(256);
    hipLaunchKernelGGL(window_gather_kernel, grid, blk, 0, (hipStream_t)stream, x, y, total, g);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

extern "C" int sscg_predict_head_sw(const float* x, int N, int h, int w, int C, int wh, int ww, int sy, int sx, int ky, int kx, int flip,
                                    int OH, int OW, const float* wy, const float* wx, const float* ry, const float* rx, float* prob,
                                    int64_t* index, uint8_t* label_u8, const int64_t* label_true, int64_t* hist, void* stream) {
    if (!x || !wy || !wx || !ry || !rx || N <= 0 || h <= 0 || w <= 0 || C <= 0 || C > SSCG_MAXC) return SSCG_ERR_BAD_ARG;
    if (!sw_axes_ok(OH, OW, wh, ww, sy, sx, ky, kx)) return SSCG_ERR_BAD_ARG;
    if ((!prob && !index && !label_u8 && !hist) || (label_true == nullptr) != (hist == nullptr)) return SSCG_ERR_BAD_ARG;
    const int F = flip ? 2 : 1;
    const size_t pixels = (size_t)N * OH * OW;
    if (pixels >= ((size_t)1 << 31) || (prob && pixels * C >= ((size_t)1 << 31))) return SSCG_ERR_UNSUPPORTED;
    if (OH >= (1 << 30) || OW >= (1 << 30) || (size_t)N * ky * kx * F >= ((size_t)1 << 31) || (size_t)ky * sy >= ((size_t)1 << 31) || (size_t)kx * sx >= ((size_t)1 << 31))
        return SSCG_ERR_UNSUPPORTED;
    SwGeom g;
    g.px = sscg_make_resize_geom(h, w, C, OH, OW);          // the pixel split of the OUTPUT ...
    g.px.sh = sscg_resize_scale(h, wh);                     // ... and the scales of the resize to the WINDOW
    g.px.sw = sscg_resize_scale(w, ww);
    g.ay = make_axis(OH, wh, sy, ky); g.ax = make_axis(OW, ww, sx, kx);
    g.F = F;
    const int total = (int)pixels;
    const size_t lds = hist ? (size_t)C * C * sizeof(unsigned int) : 0;       // <= 16 KB
    unsigned long long* hh = reinterpret_cast<unsigned long long*>(hist);
    const dim3 grid(ew_blocks(pixels, MAX_BLOCKS)), blk(256);
    hipStream_t st = (hipStream_t)stream;
    const bool ident = h == wh && w == ww;
    sscg_dispatch_classes(C, [&](auto ct) {
        constexpr int CT = decltype(ct)::value;
        if (ident) hipLaunchKernelGGL((predict_head_sw_kernel<CT, true>), grid, blk, lds, st, x, wy, wx, ry, rx, prob, index, label_u8, label_true, hh, total, g);
        else hipLaunchKernelGGL((predict_head_sw_kernel<CT, false>), grid, blk, lds, st, x, wy, wx, ry, rx, prob, index, label_u8, label_true, hh, total, g);
    });
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}
