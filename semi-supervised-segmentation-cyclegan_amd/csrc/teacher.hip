// Mean-teacher consistency on the unlabelled head (include/sscg.h: sscg_teacher_fwd): the student's prediction against the prediction
// of a TEACHER - the same network under the exponential moving average of its weights (Tarvainen & Valpola 2017; French et al. 2020
// for segmentation) - on the same image, optionally seen mirrored.  The squared distance of the two probability maps and the cross
// entropy against the teacher's confidence-masked hard labels (FixMatch's form).
//
// With z = resize(x), zt = resize(t) read at the mirrored column where flip[n] is set (bilinear, align_corners=True, the pinned
// arithmetic of head_common.h; identity sizes: no interpolation arithmetic), per output pixel
//     u_c = z_c - max z, s = sum_c exp(u_c), p = exp(u) / s              the student (the bits of the head's softmax map)
//     v_c = zt_c * inv_temp, q = softmax(v)                              the teacher (one fp32 multiply, calib.hip's temperature)
//     y*  = the first maximum of q, conf = q[y*], KEPT <=> conf >= tau
//     d   = sum_c (p_c - q_c)^2, ce = ln s - u[y*], agree = kept and the first maximum of p is y*
//     sums = (sum_kept d, A, sum_kept ce, K);  L_mse = sums[0] / (C V);  L_ce = sums[2] / max(K, 1)
// unl.hip's frame: one thread per output pixel, no block straddles a sample, K and A per wave by ballot, one fp64 record per block,
// unl_reduce_kernel and a one-block finish - no float atomics, every sum in a fixed order.  In the plain instances the teacher's
// sample is the block's own, so its base pointer and flip[n] are uniform over a block.
// sscg_teacher_fwd_mix (CutMix consistency, French et al. 2020: the student saw a CutMix of the batch, the teacher the unmixed one):
// the MIX instances read one row (partner, x0, y0, x1, y1, ...) of an int32 [N][8] table per block - still uniform - and then every
// THREAD decides whether its output pixel lies in the pasted box and takes the teacher's rows of the partner there: the source sample
// `src`, its base pointer `tn` and its mirror flip[src] are per thread in those instances, nothing else changes, and the resized
// teacher [N][OH][OW][C] that a select after the resize would need is never written.
// The thread holds TWO tables of C floats, not three: the teacher is streamed first and leaves q and y*; of the student's logit
// differences only u[y*] is ever read, so it is picked while the student's logits are still logits and u is never a table.  A class
// count known only at run time holds NO table (teacher_pixel_stream): two tables of 64 floats fill the register file.
// No backward of its own: `pseudo` and `sums` feed the pseudo-label slot of sscg_upsample_head_bwd_u / sscg_unl_bwd, and `coef` =
// d L_mse / d p joins the softmax map's upstream gradient through sscg_lovasz_scale_add.
#include "common.h"
#include "head_common.h"
#include "head_geom.h"
#include "sscg_internal.h"
#include "unl_rows.h"

namespace {

struct TeacherGeom {
    sscg_resize_geom r;
    int npix;        // OH * OW: output pixels of a sample
    int bps;         // blocks (= records) per sample
    float tau;
    float inv_temp;
    float cscale;    // (float)(2 / (C V)): coef = cscale * (p - q)
};

// zt * inv_temp as a value of its own (calib.hip's calib_scaled): inv_temp == 1 leaves the bits the student's loader would give
__device__ __forceinline__ float teacher_scaled(float z, float it) {
#pragma clang fp contract(off)
    const float v = z * it;
    return v;
}

// p_c - q_c from the two exponentials and their reciprocal sums: both probabilities are rounded to fp32 before the subtraction - the
// values the softmax map holds - so that equal logits give a difference of exactly 0.  Nothing here may contract.
__device__ __forceinline__ float teacher_diff(float ev, float inv, float eq, float invq) {
#pragma clang fp contract(off)
    const float p = ev * inv, q = eq * invq;
    return p - q;
}

// What one output pixel adds to the sums; its coefficient row is written on the way (cr != NULL; `in`: the pixel exists).
struct TeacherPixel {
    int y, ys;       // the first maxima of q and of p
    float conf;      // q[y]
    float d;         // sum_c (p_c - q_c)^2
    float ce;        // ln s - u[y]
};

__device__ __forceinline__ void teacher_coef_row(float* __restrict__ cr, int c, bool keep, float cscale, float e) {
    cr[c] = keep ? cscale * e : 0.f;
}

// The class count at compile time: both tables in registers.  The teacher first - it leaves q and y* - then the student.
template <int CT, bool RESIZE>
__device__ __forceinline__ TeacherPixel teacher_pixel_tables(const float* __restrict__ xn, const float* __restrict__ tn, int oy, int ox, int oxt,
                                                             const TeacherGeom& g, bool in, float* __restrict__ cr) {
    static_assert(CT > 0, "the run-time class count takes teacher_pixel_stream");
    TeacherPixel r;
    float q[CT];
    sscg_pixel_logits<CT, !RESIZE>(tn, 0, oy, oxt, g.r.H, g.r.W, g.r.sh, g.r.sw, CT, q);
#pragma unroll
    for (int c = 0; c < CT; ++c) q[c] = teacher_scaled(q[c], g.inv_temp);
    const float invq = sscg_softmax_exp<CT>(q, CT);
    r.y = sscg_first_max_scaled<CT>(q, invq, CT);
    r.conf = 0.f;
#pragma unroll
    for (int c = 0; c < CT; ++c) r.conf = fmaxf(r.conf, q[c] * invq);          // = q[y*]: the value the first maximum was chosen by
    float v[CT];
    sscg_pixel_logits<CT, !RESIZE>(xn, 0, oy, ox, g.r.H, g.r.W, g.r.sh, g.r.sw, CT, v);
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < CT; ++c) m = fmaxf(m, v[c]);
    float uy = 0.f;
#pragma unroll
    for (int c = 0; c < CT; ++c) uy += c == r.y ? v[c] - m : 0.f;
    const float inv = sscg_softmax_exp<CT>(v, CT);
    r.ys = sscg_first_max_scaled<CT>(v, inv, CT);
    const bool keep = in && r.conf >= g.tau;
    r.d = 0.f;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const float e = teacher_diff(v[c], inv, q[c], invq);
        r.d = __builtin_fmaf(e, e, r.d);
        if (in && cr) teacher_coef_row(cr, c, keep, g.cscale, e);
    }
    r.ce = -logf(inv) - uy;          // ln s (inv = 1 / s; s = 1 gives exactly 0) - u[y*]
    return r;
}

// One map's pixel as a function of the class: the loader's arithmetic (sscg_pixel_logits), one element at a time.
template <bool IDENT>
struct TeacherSource {
    const float *r00, *r01, *r10, *r11;
    sscg_bilin b;
    __device__ __forceinline__ TeacherSource(const float* __restrict__ xn, int oy, int ox, const sscg_resize_geom& g) {
        if (IDENT) {
            r00 = r01 = r10 = r11 = xn + ((size_t)oy * g.W + ox) * g.C;
        } else {
            b = sscg_bilin_at(oy, ox, g.H, g.W, g.sh, g.sw);
            r00 = xn + ((size_t)b.y0 * g.W + b.x0) * g.C;
            r01 = r00 + (size_t)b.xp * g.C;
            r10 = r00 + (size_t)b.yp * g.W * g.C;
            r11 = r10 + (size_t)b.xp * g.C;
        }
    }
    __device__ __forceinline__ float at(int c) const { return IDENT ? r00[c] : sscg_bilerp(b, r00[c], r01[c], r10[c], r11[c]); }
};

// max, 1 / sum exp, the first maximum of the probabilities and its value, of logits given by a function of the class: the operations of
// sscg_softmax_exp and sscg_first_max_scaled in their order, each logit formed again where it is read
template <class L>
__device__ __forceinline__ void teacher_softmax_stream(int C, L logit, float* m_out, float* inv_out, int* y_out, float* conf_out) {
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, logit(c));
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(logit(c) - m);
    const float inv = 1.f / s;
    float best = expf(logit(0) - m) * inv;
    int bi = 0;
    for (int c = 1; c < C; ++c) {
        const float p = expf(logit(c) - m) * inv;
        if (p > best) { best = p; bi = c; }
    }
    *m_out = m; *inv_out = inv; *y_out = bi; *conf_out = best;
}

// The class count at run time (C <= 64, none of the instantiated counts): no table at all.  Two tables of 64 floats fill the register
// file (profiles/unl_teacher.txt), so every pass forms its logits again from the source rows - the same pinned arithmetic, hence the
// same bits - and the rows stay in cache between the passes.
template <bool RESIZE>
__device__ __forceinline__ TeacherPixel teacher_pixel_stream(const float* __restrict__ xn, const float* __restrict__ tn, int oy, int ox, int oxt,
                                                             const TeacherGeom& g, bool in, float* __restrict__ cr) {
    const int C = g.r.C;
    const TeacherSource<!RESIZE> ts(tn, oy, oxt, g.r), xs(xn, oy, ox, g.r);
    const float it = g.inv_temp;
    auto teacher = [&](int c) { return teacher_scaled(ts.at(c), it); };
    auto student = [&](int c) { return xs.at(c); };
    TeacherPixel r;
    float mq, invq, m, inv, pmax;
    teacher_softmax_stream(C, teacher, &mq, &invq, &r.y, &r.conf);
    teacher_softmax_stream(C, student, &m, &inv, &r.ys, &pmax);
    const bool keep = in && r.conf >= g.tau;
    r.d = 0.f;
    for (int c = 0; c < C; ++c) {
        const float e = teacher_diff(expf(student(c) - m), inv, expf(teacher(c) - mq), invq);
        r.d = __builtin_fmaf(e, e, r.d);
        if (in && cr) teacher_coef_row(cr, c, keep, g.cscale, e);
    }
    r.ce = -logf(inv) - (0.f + (student(r.y) - m));
    return r;
}

// Which sample's teacher an output pixel reads.  Plain: its own.  Table: the partner inside the half-open box of the sample's row
// (partner, x0, y0, x1, y1, mask_lo, mask_hi, 0) - plain integer compares on whatever the row holds; the partner is range-checked
// before anything is indexed by it, and a partner outside [0, N) or equal to n mixes nothing.
struct TeacherPlain {
    static constexpr bool kMix = false;
};
struct TeacherTable {
    static constexpr bool kMix = true;
    const int32_t* table;
    int N;
};

template <int CT, bool RESIZE, class MIX>
__global__ __launch_bounds__(256) void teacher_stats_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                            const uint8_t* __restrict__ flip, double* __restrict__ part,
                                                            uint8_t* __restrict__ pmap, float* __restrict__ coef, TeacherGeom g, MIX mix) {
    __shared__ float redf[4][2];
    __shared__ int redk[4][2];
    const int C = CT ? CT : g.r.C;
    const int n = blockIdx.x / g.bps, blk = blockIdx.x - n * g.bps;
    const float* xn = x + (size_t)n * g.r.H * g.r.W * C;
    const float* tn = t + (size_t)n * g.r.H * g.r.W * C;
    uint8_t* pn = pmap ? pmap + (size_t)n * g.npix : nullptr;
    float* cn = coef ? coef + (size_t)n * g.npix * C : nullptr;
    const bool mirrored = flip && flip[n] != 0;
    [[maybe_unused]] int bx0 = 0, by0 = 0, bx1 = 0, by1 = 0;          // (the empty box: nothing is pasted)
    [[maybe_unused]] const float* tp = tn;
    [[maybe_unused]] bool pmirrored = mirrored;
    if constexpr (MIX::kMix) {
        const int32_t* row = mix.table + (size_t)n * 8;
        const int p = row[0];
        if (p >= 0 && p < mix.N && p != n) {           // (else the box stays empty and nothing is indexed by p)
            bx0 = row[1]; by0 = row[2]; bx1 = row[3]; by1 = row[4];
            tp = t + (size_t)p * g.r.H * g.r.W * C;
            pmirrored = flip && flip[p] != 0;
        }
    }
    float sd = 0.f, sc = 0.f;
    int kw = 0, aw = 0;
    for (long base = (long)blk * 256; base < g.npix; base += (long)g.bps * 256) {      // (long: npix may sit just below 2^31)
        const long o_raw = base + threadIdx.x;
        const bool in = o_raw < g.npix;
        const int o = in ? (int)o_raw : g.npix - 1;
        const int oy = fd_div(o, g.r.dow), ox = o - oy * g.r.OW;
        const float* ts = tn;
        bool mir = mirrored;
        if constexpr (MIX::kMix) {
            const bool pasted = ox >= bx0 && ox < bx1 && oy >= by0 && oy < by1;
            ts = pasted ? tp : tn;
            mir = pasted ? pmirrored : mirrored;        // the PARTNER's flip: its teacher saw its own image mirrored, or not
        }
        const int oxt = mir ? g.r.OW - 1 - ox : ox;
        float* cr = cn ? cn + (size_t)o * C : nullptr;
        TeacherPixel r;
        if constexpr (CT > 0) r = teacher_pixel_tables<CT, RESIZE>(xn, ts, oy, ox, oxt, g, in, cr);
        else r = teacher_pixel_stream<RESIZE>(xn, ts, oy, ox, oxt, g, in, cr);
        const bool keep = in && r.conf >= g.tau;
        const bool agree = keep && r.ys == r.y;
        sd += keep ? r.d : 0.f;
        sc += keep ? r.ce : 0.f;
        kw += __popcll(__ballot(keep));
        aw += __popcll(__ballot(agree));
        if (in && pn) pn[o] = (uint8_t)(keep ? r.y : UNL_DROPPED);
    }
    const int wave = threadIdx.x >> 6;
    const float td = wave_sum(sd), tc = wave_sum(sc);
    if ((threadIdx.x & 63) == 0) { redf[wave][0] = td; redf[wave][1] = tc; redk[wave][0] = aw; redk[wave][1] = kw; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        double* rec = part + (size_t)blockIdx.x * 4;
        if ((k & 1) == 0) rec[k] = ((double)redf[0][k >> 1] + (double)redf[1][k >> 1]) + ((double)redf[2][k >> 1] + (double)redf[3][k >> 1]);
        else rec[k] = (double)((redk[0][k >> 1] + redk[1][k >> 1]) + (redk[2][k >> 1] + redk[3][k >> 1]));
    }
}

__global__ __launch_bounds__(256) void teacher_finish_kernel(const double* __restrict__ ssum, int N, double V, int C,
                                                             double* __restrict__ sums, float* __restrict__ losses) {
    __shared__ double sm[256];
    __shared__ double tot[4];
    const double t = unl_sum_rows(ssum, N, sm);
    if (threadIdx.x < 4) { tot[threadIdx.x] = t; sums[threadIdx.x] = t; }
    __syncthreads();
    if (threadIdx.x == 0) {
        losses[0] = (float)(tot[0] / ((double)C * V));
        losses[1] = (float)(tot[2] / (tot[3] > 1.0 ? tot[3] : 1.0));       // K == 0: 0 / 1
    }
}

template <bool RESIZE, class MIX>
void launch_stats(const TeacherGeom& g, int N, hipStream_t st, const float* x, const float* t, const uint8_t* flip, double* part,
                  uint8_t* pmap, float* coef, MIX mix) {
    const dim3 grid((unsigned)N * g.bps), blk(256);
    sscg_dispatch_classes(g.r.C, [&](auto ct) {
        hipLaunchKernelGGL((teacher_stats_kernel<decltype(ct)::value, RESIZE, MIX>), grid, blk, 0, st, x, t, flip, part, pmap, coef, g, mix);
    });
}

// Both entries: table == NULL runs the plain instances.
int teacher_fwd(const float* x, const float* t, const uint8_t* flip, const int32_t* table, int N, int H, int W, int C, int OH, int OW,
                float inv_temp, float thresh, float* losses, double* sums, uint8_t* pseudo, float* coef, void* ws, size_t ws_bytes,
                void* stream) {
    if (!x || !t || !losses || !sums || !sizes_ok(N, H, W, C, OH, OW) || !thresh_ok(thresh)) return SSCG_ERR_BAD_ARG;
    if (!(inv_temp > 0.f && inv_temp < INFINITY)) return SSCG_ERR_BAD_ARG;      // (false for a NaN)
    if (too_large(N, H, W, OH, OW)) return SSCG_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < sscg_teacher_workspace(N, OH, OW)) return SSCG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const double V = (double)N * OH * OW;
    const TeacherGeom g = {sscg_make_resize_geom(H, W, C, OH, OW), OH * OW, unl_bps(OH, OW), thresh, inv_temp, (float)(2.0 / ((double)C * V))};
    double* part = reinterpret_cast<double*>(ws);
    const bool resize = !(OH == H && OW == W);
    if (table) {
        const TeacherTable mix = {table, N};
        if (resize) launch_stats<true>(g, N, st, x, t, flip, part, pseudo, coef, mix);
        else launch_stats<false>(g, N, st, x, t, flip, part, pseudo, coef, mix);
    } else {
        if (resize) launch_stats<true>(g, N, st, x, t, flip, part, pseudo, coef, TeacherPlain{});
        else launch_stats<false>(g, N, st, x, t, flip, part, pseudo, coef, TeacherPlain{});
    }
    double* ssum = part + (size_t)N * g.bps * 4;
    hipLaunchKernelGGL(unl_reduce_kernel, dim3((unsigned)N), dim3(256), 0, st, part, g.bps, ssum);
    hipLaunchKernelGGL(teacher_finish_kernel, dim3(1), dim3(256), 0, st, ssum, N, V, C, sums, losses);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}

}  // namespace

extern "C" size_t sscg_teacher_workspace(int N, int OH, int OW) {
    if (N <= 0 || OH <= 0 || OW <= 0 || (size_t)N * OH * OW >= ((size_t)1 << 31)) return 0;
    return (size_t)N * 4 * ((size_t)unl_bps(OH, OW) + 1) * sizeof(double);      // the blocks' records + the samples' sums
}

extern "C" int sscg_teacher_fwd(const float* x, const float* t, const uint8_t* flip, int N, int H, int W, int C, int OH, int OW,
                                float inv_temp, float thresh, float* losses, double* sums, uint8_t* pseudo, float* coef, void* ws,
                                size_t ws_bytes, void* stream) {
    return teacher_fwd(x, t, flip, nullptr, N, H, W, C, OH, OW, inv_temp, thresh, losses, sums, pseudo, coef, ws, ws_bytes, stream);
}

extern "C" int sscg_teacher_fwd_mix(const float* x, const float* t, const uint8_t* flip, const int32_t* table, int N, int H, int W, int C,
                                    int OH, int OW, float inv_temp, float thresh, float* losses, double* sums, uint8_t* pseudo,
                                    float* coef, void* ws, size_t ws_bytes, void* stream) {
    return teacher_fwd(x, t, flip, table, N, H, W, C, OH, OW, inv_temp, thresh, losses, sums, pseudo, coef, ws, ws_bytes, stream);
}
