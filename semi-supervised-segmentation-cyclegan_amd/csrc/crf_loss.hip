// The gated (relaxed dense) CRF loss of a softmax map (include/sscg.h: sscg_crf_loss_fwd): the training-side counterpart of crf.hip.
// With k(i, j) the pairwise weight of sscg_crf_head (crf_common.h) over the dilated (2r+1)^2 window, centre excluded:
//     msg_c(i) = sum_taps k(i, j) p_c(j)        ksum(i) = sum_taps k(i, j)        e(i) = ksum(i) - sum_c p_c(i) msg_c(i)
//     loss = sum_i e(i) / M                     coef[i][c] = (-2 / M) msg_c(i) = d loss / d p_c(i)       (k is symmetric bit for bit)
//   crf_loss_kernel:        crf_iter_kernel's frame - one 16 x 16 tile of one sample per workgroup, the guide's halo staged once, the
//                           weights of a thread's own taps in registers, p's halo staged four classes at a time - with, instead of the
//                           softmax, ksum, the running product sum and the store of s * msg; then e and ksum of the tile's pixels into
//                           the block's fp64 record: a wave's 64 values by the fixed butterfly, the four waves in order.
//   crf_loss_finish_kernel: one block, the records in index order -> sums[2] (fp64) and the loss (fp32).
// No float atomics, every sum in a fixed order: the same call twice gives the same bits.  The backward of the Python node is
// sscg_lovasz_scale_add on coef: there is no backward kernel here.
#include "common.h"
#include "crf_common.h"
#include "head_common.h"
#include "sscg_internal.h"

namespace {

constexpr int TILE = CRF_TILE, RMAX = CRF_RMAX, SIDE = CRF_SIDE, STAGE = CRF_STAGE;

// coef is nullable (the value only).  A tap beyond the radius or outside the map gets k = 0 as a select and reads the centre / a p
// staged as 0: it adds +0 to non-negative sums, which is to skip it (crf.hip says why there is no branch per tap).  A thread outside
// the map (a ragged tile) walks the taps like the others - the barriers need it - and contributes e = ksum = 0.
// CT: 21, 4, or 0 = the class count at run time (20 classes included: see the entry).
template <int CT, int RT>
__global__ __launch_bounds__(256, (CT && RT <= 3) ? 3 : 2) void crf_loss_kernel(const float* __restrict__ p, const float* __restrict__ img,
                                                                                float* __restrict__ coef, double* __restrict__ part,
                                                                                float s, CrfGeom g, CrfTaps tp) {
    extern __shared__ float4 stage[];                 // [side][pitch], the four waves' two fp64 sums behind it
    double (*red)[2] = reinterpret_cast<double (*)[2]>(stage + g.side * g.pitch);
    const int C = CT ? CT : g.C;

    const int bt = fd_div((int)blockIdx.x, g.dtx);
    const int bx = (int)blockIdx.x - bt * g.tiles_x;
    const int n = fd_div(bt, g.dty);
    const int by = bt - n * g.tiles_y;
    const int tx = threadIdx.x & (TILE - 1), ty = threadIdx.x >> 4;
    const int oy = by * TILE + ty, ox = bx * TILE + tx;
    const bool inside = oy < g.OH && ox < g.OW;
    const int hy0 = by * TILE - g.reach, hx0 = bx * TILE - g.reach;
    const int npix = g.side * g.side;
    const size_t map0 = (size_t)n * g.OH * g.OW;       // the sample's first pixel

    for (int e = threadIdx.x; e < npix; e += 256) {
        const int hy = fd_div(e, g.dside), hx = e - hy * g.side;
        const int y = hy0 + hy, x = hx0 + hx;
        float4 px = make_float4(0.f, 0.f, 0.f, 0.f);
        if (y >= 0 && y < g.OH && x >= 0 && x < g.OW) {
            const float* ip = img + (map0 + (size_t)y * g.OW + x) * g.IC;
            px.x = ip[0];
            if (g.IC > 1) px.y = ip[1];
            if (g.IC > 2) px.z = ip[2];
            if (g.IC > 3) px.w = ip[3];
        }
        stage[hy * g.pitch + hx] = px;
    }
    __syncthreads();

    const int centre = (ty + g.reach) * g.pitch + tx + g.reach;
    const int step_y = g.d * g.pitch, step_x = g.d;
    constexpr int KS = 2 * RT + 1;
    float k[KS * KS];
    float ksum = 0.f;
    {
        const float4 ci = stage[centre];
#pragma unroll
        for (int dy = -RT; dy <= RT; ++dy)
#pragma unroll
            for (int dx = -RT; dx <= RT; ++dx) {
                const int ring = (dy < 0 ? -dy : dy) > (dx < 0 ? -dx : dx) ? (dy < 0 ? -dy : dy) : (dx < 0 ? -dx : dx);
                if (ring != 0) {
                    const bool on = ring <= g.r;                       // uniform; a select, not a branch
                    const int t = (dy + RMAX) * SIDE + dx + RMAX;
                    const int y = oy + dy * g.d, x = ox + dx * g.d;
                    const float w = crf_weight(ci, stage[on ? centre + dy * step_y + dx * step_x : centre], tp.d2a[t], tp.spatial[t], g.wb, g.ib);
                    const float kt = (on && y >= 0 && y < g.OH && x >= 0 && x < g.OW) ? w : 0.f;
                    k[(dy + RT) * KS + dx + RT] = kt;
                    ksum += kt;
                }
            }
    }

    const int o = (int)map0 + oy * g.OW + ox;
    float* sf = reinterpret_cast<float*>(stage);
    float dot = 0.f;
    // not unrolled over the quads: the unrolled body hoists every quad's staging addresses and spills (profiles/crf_loss.txt)
#pragma unroll 1
    for (int c0 = 0; c0 < C; c0 += 4) {
        __syncthreads();                               // the region's previous content (the image, the quad before) has been read
        // consecutive lanes take consecutive floats of a pixel's quad, then the next pixel; STAGE loads are issued before the first
        // of them is stored, so a thread waits for memory once per batch, not once per element
        for (int e0 = threadIdx.x; e0 < npix * 4; e0 += 256 * STAGE) {
            float val[STAGE];
            int at[STAGE];
#pragma unroll
            for (int st = 0; st < STAGE; ++st) {
                const int e = e0 + st * 256;
                const int pe = e >> 2, j = e & 3;
                const int hy = fd_div(pe, g.dside), hx = pe - hy * g.side;
                const int y = hy0 + hy, x = hx0 + hx;
                at[st] = e < npix * 4 ? (hy * g.pitch + hx) * 4 + j : -1;
                val[st] = 0.f;
                if (at[st] >= 0 && y >= 0 && y < g.OH && x >= 0 && x < g.OW && c0 + j < C)
                    val[st] = p[((int)map0 + y * g.OW + x) * C + c0 + j];          // < 2^31 elements: checked by the entry
            }
#pragma unroll
            for (int st = 0; st < STAGE; ++st)
                if (at[st] >= 0) sf[at[st]] = val[st];
        }
        __syncthreads();
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int dy = -RT; dy <= RT; ++dy)
#pragma unroll
            for (int dx = -RT; dx <= RT; ++dx) {
                const int ring = (dy < 0 ? -dy : dy) > (dx < 0 ? -dx : dx) ? (dy < 0 ? -dy : dy) : (dx < 0 ? -dx : dx);
                if (ring != 0) {
                    const float kt = k[(dy + RT) * KS + dx + RT];
                    const float4 pj = stage[ring <= g.r ? centre + dy * step_y + dx * step_x : centre];
                    acc.x = fmaf(kt, pj.x, acc.x);
                    acc.y = fmaf(kt, pj.y, acc.y);
                    acc.z = fmaf(kt, pj.z, acc.z);
                    acc.w = fmaf(kt, pj.w, acc.w);
                }
            }
        // the pixel's own quad is in the halo; classes at or above C take no part (they were staged as 0 and are not stored)
        const float4 pi = stage[centre];
        const bool c1 = c0 + 1 < C, c2 = c0 + 2 < C, c3 = c0 + 3 < C;
        dot = fmaf(pi.x, acc.x, dot);
        if (c1) dot = fmaf(pi.y, acc.y, dot);
        if (c2) dot = fmaf(pi.z, acc.z, dot);
        if (c3) dot = fmaf(pi.w, acc.w, dot);
        if (coef && inside) {
            float* cp = coef + (size_t)o * C + c0;
            cp[0] = s * acc.x;
            if (c1) cp[1] = s * acc.y;
            if (c2) cp[2] = s * acc.z;
            if (c3) cp[3] = s * acc.w;
        }
    }

    const double te = wave_sum(inside ? (double)(ksum - dot) : 0.0), tk = wave_sum(inside ? (double)ksum : 0.0);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wave][0] = te; red[wave][1] = tk; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int j = threadIdx.x;
        part[(size_t)blockIdx.x * 2 + j] = ((red[0][j] + red[1][j]) + (red[2][j] + red[3][j]));
    }
}

// `blocks` records of two doubles -> sums[2] and the loss: 128 row lanes of two threads (lane r takes records r, r + 128, ... in
// order), then the lanes in order by the column's first thread.
__global__ __launch_bounds__(256) void crf_loss_finish_kernel(const double* __restrict__ part, int blocks, double M, double* __restrict__ sums,
                                                              float* __restrict__ loss) {
    __shared__ double sm[256];
    const int j = threadIdx.x & 1, rl = threadIdx.x >> 1;
    double t = 0.0;
    for (int r = rl; r < blocks; r += 128) t += part[(size_t)r * 2 + j];
    sm[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x < 2) {
        double tot = 0.0;
        for (int r = 0; r < 128; ++r) tot += sm[r * 2 + j];
        sums[j] = tot;
        if (j == 0) loss[0] = (float)(tot / M);
    }
}

size_t loss_blocks(int N, int OH, int OW) {
    return (size_t)N * ((OW + TILE - 1) / TILE) * ((OH + TILE - 1) / TILE);
}

}  // namespace

extern "C" size_t sscg_crf_loss_workspace(int N, int OH, int OW) {
    if (N <= 0 || OH <= 0 || OW <= 0) return 0;
    return loss_blocks(N, OH, OW) * 2 * sizeof(double);      // one record (sum e, sum ksum) per tile
}

extern "C" int sscg_crf_loss_fwd(const float* p, int N, int OH, int OW, int C, const float* img, int IC, const sscg_crf_params* prm,
                                 float* loss, double* sums, float* coef, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !img || !prm || !loss || !sums) return SSCG_ERR_BAD_ARG;
    if (N <= 0 || OH <= 0 || OW <= 0 || C <= 0 || C > SSCG_MAXC || IC < 1 || IC > 4) return SSCG_ERR_BAD_ARG;
    if (prm->radius < 1 || prm->radius > RMAX || prm->dilation < 1) return SSCG_ERR_BAD_ARG;          // (iterations: ignored)
    if (!crf_finite_nonneg(prm->w_bilateral) || !crf_finite_nonneg(prm->w_spatial)) return SSCG_ERR_BAD_ARG;      // (false for a NaN)
    float ia, ib, ig;
    if (!crf_inv_two_theta_sq(prm->theta_alpha, &ia) || !crf_inv_two_theta_sq(prm->theta_beta, &ib) ||
        !crf_inv_two_theta_sq(prm->theta_gamma, &ig))
        return SSCG_ERR_BAD_ARG;
    if ((int64_t)prm->radius * prm->dilation > CRF_REACH_MAX) return SSCG_ERR_UNSUPPORTED;
    const size_t pixels = (size_t)N * OH * OW;
    if (pixels * C >= ((size_t)1 << 31)) return SSCG_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < sscg_crf_loss_workspace(N, OH, OW)) return SSCG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;

    CrfGeom g;
    CrfTaps tp;
    crf_setup(C, OH, OW, IC, prm->radius, prm->dilation, prm->w_bilateral, prm->w_spatial, ia, ib, ig, &g, &tp);
    const size_t stage_lds = (size_t)g.side * g.pitch * sizeof(float4) + 4 * 2 * sizeof(double);      // <= 36 KB + 64 B
    const int blocks = (int)loss_blocks(N, OH, OW);
    const float s = (float)(-2.0 / (double)pixels);
    double* part = reinterpret_cast<double*>(ws);
    // crf.hip's arms but for C = 20, which goes to the run-time arm: its own instance is the one at radius <= 3 that spills (104 B per
    // lane) and took 1.6x the run-time arm's time at 16 x 20 x 256 x 512 (profiles/crf_loss.txt); the bits are the same on every arm
    auto launch = [&](auto ct) {
        constexpr int CT = decltype(ct)::value;
        if (g.r <= 3) hipLaunchKernelGGL((crf_loss_kernel<CT, 3>), dim3((unsigned)blocks), dim3(256), stage_lds, st, p, img, coef, part, s, g, tp);
        else hipLaunchKernelGGL((crf_loss_kernel<CT, RMAX>), dim3((unsigned)blocks), dim3(256), stage_lds, st, p, img, coef, part, s, g, tp);
    };
    if (C == 21) launch(std::integral_constant<int, 21>{});
    else if (C == 4) launch(std::integral_constant<int, 4>{});
    else launch(std::integral_constant<int, 0>{});
    hipLaunchKernelGGL(crf_loss_finish_kernel, dim3(1), dim3(256), 0, st, part, blocks, (double)pixels, sums, loss);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}
