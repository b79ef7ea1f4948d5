/*
 * sscg.h - C ABI of libsscg.so: the MI355X (gfx950) kernels behind the CycleGAN training step of
 * arnab39/Semi-supervised-segmentation-cycleGAN (model.py:370-552, `semisuper_cycleGAN.train`).
 *
 * The reference has no FFI of its own: every arithmetic op on its hot path is a stock torch.nn module
 * (SURVEY.md section 8(b)).  Each entry point below therefore names the torch call site it replaces
 * (reference file:line).  INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C: device pointers + sizes, no torch types.  Tensors are channels-last (NHWC: [N][H][W][C]); conv weights
 *     [K][R][S][C] (= torch `[K,C,R,S]` in channels_last); labels int64.  Activations and conv weights are fp32
 *     (SSCG_F32, the reference's dtype and BASELINE config 2) or bfloat16 (SSCG_BF16, BASELINE configs 3/5): entry points
 *     that touch them take `void*` plus a dtype code.  Statistics, losses, biases, weight gradients, optimiser state: fp32.
 *   - `stream` is a hipStream_t passed as void*.  Calls are asynchronous and stream ordered, re-entrant,
 *     allocate nothing and keep no mutable state (tile-class / split overrides of tools and tests travel in
 *     sscg_conv_desc.tuning / wgrad_tuning); scratch memory is caller provided (`ws`) and sized by the matching
 *     *_workspace() query.
 *   - return value: 0 = ok, <0 = library error (SSCG_ERR_*), >0 = hipError_t.  Never throws/aborts.
 */
#ifndef SSCG_H
#define SSCG_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSCG_ABI_VERSION 18

/* element types of activation / weight tensors */
#define SSCG_F32 0
#define SSCG_BF16 1
#define SSCG_BF16X3 2 /* conv WEIGHT operands only: an fp32 weight split into three bfloat16 planes h + m + l (sscg_split3), the operand
                       * of the fp32-accurate "split" contraction on the bf16 matrix cores */

#define SSCG_ERR_BAD_ARG (-1)
#define SSCG_ERR_UNSUPPORTED (-2)
#define SSCG_ERR_WORKSPACE (-3)

/* activation codes (conv epilogue, norm apply) */
#define SSCG_ACT_NONE 0
#define SSCG_ACT_RELU 1  /* nn.ReLU            arch/ops.py:50,57 */
#define SSCG_ACT_LRELU 2 /* nn.LeakyReLU(0.2)  arch/ops.py:44, arch/discriminators.py:46,71,74 */
#define SSCG_ACT_TANH 3  /* nn.Tanh            arch/generators.py:91 */

#define SSCG_PAD_ZEROS 0
#define SSCG_PAD_REFLECT 1 /* nn.ReflectionPad2d folded into the conv loader: arch/ops.py:62,67; arch/generators.py:73,84,89 */

int sscg_abi_version(void);
/* Measurement aid (no reference counterpart): on != 0 turns every kernel launch of the library into a no-op while the host side of
 * each entry point (checks, planning, workspace carving) still runs; returns the previous setting.  bench.py times the host's issue
 * cost of a training step with it (no back-pressure from the device).  Results are undefined while it is on. */
int sscg_set_dry_run(int on);

/* ------------------------------------------------------------------ convolution (K1, K2, K5) */
typedef struct sscg_conv_desc {
    int32_t N, H, W, C; /* input  [N][H][W][C] */
    int32_t K, R, S;    /* weight [K][R][S][C] */
    int32_t P, Q;       /* output [N][P][Q][K];  P = (H + 2*pad - dil*(R-1) - 1)/stride + 1 */
    int32_t stride, pad, dil;
    int32_t pad_mode;   /* SSCG_PAD_* (reflect: forward and wgrad only) */
    int32_t act;        /* fused epilogue activation of the forward */
    float slope;        /* LeakyReLU slope */
    int32_t x_dtype;    /* SSCG_F32 / SSCG_BF16 of the [N][H][W][C] tensor (forward input, dgrad output, wgrad x) */
    int32_t w_dtype;    /* ... of the weight operand handed to forward ([K][R][S][C]) / dgrad ([C][R][S][K]) */
    int32_t y_dtype;    /* ... of the [N][P][Q][K] tensor (forward output, dgrad / wgrad dy) */
    int32_t precision;  /* fp32 tensors only: 0 = exact fp32 MFMA (v_mfma_f32_32x32x2_f32); 1 = operands rounded to bf16
                         * (RNE) between LDS and the matrix cores, v_mfma_f32_32x32x16_bf16, fp32 accumulation; 2 (weight
                         * gradient only) = both operands split into three bf16 pieces between LDS and the matrix cores, six
                         * exact piece products accumulated in fp32 (fp32-accurate; the two LDS-DMA tile classes, exact fp32
                         * elsewhere).  Forward / data gradient select the split contraction through w_dtype = SSCG_BF16X3. */
    int32_t tuning;     /* 0 = the library's own plan.  Tuning / test aid carried by the call (the library keeps no mutable state):
                         * bits 0..7 = 1 + forced tile class of the forward / data-gradient kernel family that serves the call,
                         * bits 8..15 = split-K (1 = never, n > 1 = every tile cut in n) */
    int64_t w_plane;    /* w_dtype == SSCG_BF16X3: elements between two planes of the weight operand; 0 = K*R*S*C (dense) */
    int32_t wgrad_tuning; /* 0 = the library's cost model.  bits 0..7 = 1 + forced weight-gradient tile class (0 = 128x128,
                         * 1 = 64x64) with bits 8..23 = pixel splits; precision 2 only: class 2 = never the pre-split-planes
                         * kernel (operands split on the fly), class 3 = the planes kernel also for 1x1 filters; bits 24..31 =
                         * kernel-variant switches (bf16 weight gradient: tools/conv16_bench.py; planes kernel: bit 24 = two
                         * copy stages) */
} sscg_conv_desc;
/* Supported dtype combinations.  forward: (x, w) both fp32 -> y fp32|bf16 (fp32 MFMA kernel: stems and few-channel
 * inputs); (x, w) both bf16 with C % 64 == 0 -> y fp32|bf16 (bf16 MFMA kernel, bf16 LDS tiles).  dgrad: the same with
 * (dy, wt) as the operands and dx as the result (K % 64 == 0 for bf16).  wgrad: x, dy each fp32|bf16, dw fp32. */

/* nn.Conv2d forward: arch/ops.py:43,49,68; arch/generators.py:85,90,325,331,336,373,388,415;
 * arch/discriminators.py:45,58,70-75.  y = act(conv(x, w) + bias); bias may be NULL. */
size_t sscg_conv2d_fwd_workspace(const sscg_conv_desc* d);   /* split-K scratch for few-channel heads; may be 0 */
int sscg_conv2d_fwd(const sscg_conv_desc* d, const void* x, const void* w, const float* bias, void* y, void* ws,
                    size_t ws_bytes, void* stream);

/* Forward with the statistics of the normalisation layer that follows fused into the epilogue ("Conv + InstanceNorm /
 * BatchNorm" blocks, arch/ops.py:40-57, arch/generators.py:345-365): besides y, per-tile column sums of y and y^2 (fp64,
 * taken from the fp32 accumulators) go to `stats`; sscg_norm_stats_from_conv turns them into mean / rstd (and the
 * running-statistics update) without reading y again.  The output rows are viewed as G groups of L rows (G*L = N*P*Q).
 * sscg_conv2d_fwd_stats_bytes returns 0 when the fusion does not apply to this geometry (then use sscg_norm_stats). */
size_t sscg_conv2d_fwd_stats_bytes(const sscg_conv_desc* d, int G, int64_t L);
size_t sscg_conv2d_fwd_stats_workspace(const sscg_conv_desc* d);
int sscg_conv2d_fwd_stats(const sscg_conv_desc* d, const void* x, const void* w, const float* bias, void* y, int G, int64_t L,
                          void* stats, size_t stats_bytes, void* ws, size_t ws_bytes, void* stream);
int sscg_norm_stats_from_conv(const sscg_conv_desc* d, const void* stats, int G, int64_t L, float eps, float* mean, float* rstd,
                              float* running_mean, float* running_var, float momentum, void* stream);

/* Eval-mode nn.Conv2d -> nn.BatchNorm2d [+ residual] -> activation as ONE launch (added to ABI v18; see below): the DeepLab units of
 * arch/generators.py:345-365 as model.py:555-574 (evaluate()), validation.py and testing.py run them, under .eval() and
 * torch.no_grad().  There the normalisation is a per-channel affine known before the conv starts, and the conv's store phase applies it:
 *   y = act(((conv(x, w) + bias) - running_mean) * rstd * gamma + beta + residual),  rstd = (float)(1 / sqrt((double)running_var + eps))
 * - bit for bit what sscg_conv2d_fwd (act NONE), sscg_rstd_from_var and sscg_norm_apply compute in three launches, without the round trip
 * of the conv's output through memory (with bf16 tensors the conv's result is rounded to bf16 in front of the affine, as the stored map
 * is).  d->act / d->slope is the activation BEHIND the norm (NONE / RELU / LRELU), not a conv activation.  gamma and beta: both or
 * neither.  residual: NULL or [N][P][Q][K] in y's dtype.  ws: sscg_conv2d_fwd_workspace(d) bytes (the split-K plan is the plain
 * forward's; the tail's reduction carries the affine).  sscg_conv2d_fwd_affine_applies: 1 for fp32 tensors with w = SSCG_BF16X3 split
 * planes (C % 32 == 0, K % 4 == 0, K > 32) and for bf16 tensors (C % 64 == 0, K % 8 == 0, K > 32, y bf16); 0 for the exact-fp32 kernel
 * (which also serves the 3-channel stems), the thin 1x1 kernels, the heads' 32-column tile classes and tanh - the caller then runs the
 * separate passes.  Errors before any HIP call: SSCG_ERR_BAD_ARG (null tensors, gamma without beta), SSCG_ERR_UNSUPPORTED (applies ==
 * 0), SSCG_ERR_WORKSPACE. */
/* (The two entries are an addition: no existing entry, struct or code changes meaning, so SSCG_ABI_VERSION stays 18 and a caller
 * built against the v18 header keeps working; a binding that needs them finds them by name.) */
int sscg_conv2d_fwd_affine_applies(const sscg_conv_desc* d);
int sscg_conv2d_fwd_affine(const sscg_conv_desc* d, const void* x, const void* w, const float* bias, const float* running_mean,
                           const float* running_var, float eps, const float* gamma, const float* beta, const void* residual, void* y,
                           void* ws, size_t ws_bytes, void* stream);

/* PixelDiscriminator's front half as ONE launch (arch/discriminators.py:70-73: nn.Conv2d(input_nc, ndf, 1) -> nn.LeakyReLU(0.2) ->
 * nn.Conv2d(ndf, 2 ndf, 1) [-> the statistics of the InstanceNorm / BatchNorm layer at :73]).  `d` describes the SECOND conv (C = 64
 * source channels, 1x1, stride 1, no padding, fp32 tensors, w = its SSCG_BF16X3 split planes); `xf` [N*H*W][cin] fp32 is the FIRST
 * conv's input, (w1 [64][cin], b1 [64] or NULL, slope1) its parameters and LeakyReLU slope.  The 64-channel map between the two convs
 * is formed per workgroup in LDS (exact fp32 FMAs) and is written to `h1` ([N*H*W][64] fp32) only when the caller passes it (a
 * backward pass that wants it stored) - the launch itself never reads it back.  G > 0: `stats` receives the records of
 * sscg_conv2d_fwd_stats for `d` (same size, finalised by sscg_norm_stats_from_conv).  sscg_conv2d_front_applies: cin in {3, 4, 20, 21}
 * and a geometry whose tile class carries the fused prologue (else run the two convs separately). */
int sscg_conv2d_front_applies(const sscg_conv_desc* d, int cin);
int sscg_conv2d_front_fwd(const sscg_conv_desc* d, const void* xf, int cin, const float* w1, const float* b1, float slope1, void* h1,
                          const void* w, const float* bias, void* y, int G, int64_t L, void* stats, size_t stats_bytes, void* stream);

/* Data gradient of the same conv (autograd of model.py:472,539), and nn.ConvTranspose2d forward
 * (arch/ops.py:55-56): dx = act(dgrad(dy, wt) + bias).  `wt` = weight re-laid as [C][R][S][K]
 * by sscg_weight_krsc_to_crsk.  bias NULL / act NONE for a pure gradient. */
size_t sscg_conv2d_dgrad_workspace(const sscg_conv_desc* d);
int sscg_conv2d_dgrad(const sscg_conv_desc* d, const void* dy, const void* wt, const float* bias, void* dx,
                      int act, float slope, void* ws, size_t ws_bytes, void* stream);

/* Weight gradient: dw = beta*dw + wgrad(x, dy); dw is fp32 [K][R][S][C]. */
size_t sscg_conv2d_wgrad_workspace(const sscg_conv_desc* d);
int sscg_conv2d_wgrad(const sscg_conv_desc* d, const void* x, const void* dy, float* dw, float beta, void* ws,
                      size_t ws_bytes, void* stream);

/* [K][RS][C] -> [C][RS][K]; source and destination dtypes may differ (fp32 master weight -> bf16 operand copy) */
int sscg_weight_krsc_to_crsk(const void* w, int w_dtype, void* wt, int wt_dtype, int K, int RS, int C, void* stream);
/* The same re-layout of MANY weights in one launch (the operand copies of every conv that sees a backward pass are rebuilt after each
 * optimiser step: ~230 launches of a few microseconds each at the top of the step otherwise).  `jobs` is a table IN DEVICE MEMORY;
 * job i covers the 32x32 tiles [block0, block0 of job i+1) in the order (c-tile fastest, then k-tile, then tap) - block0 ascending,
 * job 0 at 0, `n_blocks` the total.  Same dtype pairs and bit-identical results as sscg_weight_krsc_to_crsk. */
typedef struct sscg_wt_job {
    const void* w;
    void* wt;
    int32_t w_dtype, wt_dtype;
    int32_t K, RS, C;
    int32_t block0;
} sscg_wt_job;
int sscg_weight_krsc_to_crsk_batch(const sscg_wt_job* jobs, int n_jobs, int n_blocks, void* stream);
/* The "split" contraction (fp32 accuracy on the bf16 matrix cores): dst = three bfloat16 planes h, m, l (each n elements,
 * `plane_stride` elements apart) with src[i] = h[i] + m[i] + l[i] to 2^-24 (round to nearest at every step).  A conv weight in
 * this form is passed with w_dtype = SSCG_BF16X3 (forward: planes of [K][R][S][C]; dgrad: planes of [C][R][S][K], which
 * sscg_weight_krsc_to_crsk produces directly with wt_dtype = SSCG_BF16X3). */
int sscg_split3(const float* src, void* dst, int64_t n, int64_t plane_stride, void* stream);
/* 1 when the split kernels serve this call (kind 0 = forward, 1 = data gradient; dtypes of `d` are ignored: fp32 tensors are
 * implied), 0 when the caller should use the exact-fp32 path (few-channel stems and heads, ragged channels).  (The weight
 * gradient takes precision = 2 for every geometry and falls back to exact fp32 by itself.) */
int sscg_conv2d_split_applies(const sscg_conv_desc* d, int kind);
/* dst[i] = (dst_dtype) src[i] */
int sscg_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, void* stream);

/* out[c] = beta*out[c] + sum_r x[r][c]  (bias gradient).  ws: sscg_colsum_workspace bytes. */
size_t sscg_colsum_workspace(int64_t rows, int cols);
int sscg_colsum(const void* x, int dtype, float* out, int64_t rows, int cols, float beta, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ normalisation (K3, K4, K7)
 * x is viewed as [G][L][C]: InstanceNorm2d (arch/ops.py:11: affine=False, no running stats) has G = N,
 * L = H*W; BatchNorm2d (arch/generators.py:326-337,390,417; arch/ops.py:9) has G = 1, L = N*H*W.
 * eps 1e-5, biased variance for normalisation, unbiased for running_var (torch semantics). */
size_t sscg_norm_stats_workspace(int G, int64_t L, int C);
/* mean[G][C], rstd[G][C]; if running_mean != NULL:
 * running = (1-momentum)*running + momentum*batch (running_var from the unbiased batch variance), applied once per
 * group in the order g = 0..G-1.  G > 1 with running statistics is BatchNorm2d over G batches stacked along N in one
 * launch ("grouped"): bit-identical to G successive forwards of the layer, each on its own batch. */
int sscg_norm_stats(const void* x, int dtype, int G, int64_t L, int C, float eps, float* mean, float* rstd,
                    float* running_mean, float* running_var, float momentum, void* ws, size_t ws_bytes, void* stream);
/* y = act((x-mean)*rstd*gamma + beta + residual); gamma/beta/residual nullable (gamma,beta are [C]).
 * x, residual, y share `dtype`. */
int sscg_norm_apply(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                    const void* residual, void* y, int dtype, int G, int64_t L, int C, int act, float slope, void* stream);
/* eval-mode BatchNorm: mean = running_mean, rstd = 1/sqrt(running_var + eps) */
/* The reduction pass of a normalisation layer's backward, fused into the data gradient that produces its upstream gradient
 * ("Conv -> norm -> ReLU -> Conv" chains: arch/ops.py:40-57, the Bottleneck's conv1-bn1-relu-conv2-bn2-relu-conv3 and the
 * bn3 + residual -> relu -> next block's conv1 link, arch/generators.py:345-365; autograd of model.py:472,539).
 * sscg_conv2d_dgrad_bsums is sscg_conv2d_dgrad (no bias, no activation) of the CONSUMER convolution; its result dx
 * (+ addend, below) is the gradient at the output of act(norm(nx) [+ residual]) with nx [G * L][C] (C = d->C), and its epilogue
 * also leaves, per tile row and channel, the fp64 sums of gg and gg * xhat (gg = act'(...) dx, xhat = (nx - mean) * rstd) in `sums`.
 * The ReLU / LeakyReLU mask is the sign of gamma * xhat + beta for a unit without a residual (nz NULL), and the sign of the unit's
 * forward output nz ([G * L][C]; this conv's own input) for a unit a residual joined (fp32 tensors only).
 * addend (nullable, [N][H][W][C] like dx; fp32 tensors only): dx = dgrad(dy, wt) + addend - the gradient another consumer of the
 * same tensor left (a residual block's input feeds conv1 and the shortcut): the fan-in joins in the store phase, the sums see the
 * total.  sscg_norm_bwd_from_sums (same descriptor d) then finishes that layer's backward - finalize + apply, no pass over
 * (dx, nx) for the sums; y / dres (nullable): the unit's forward output and the residual's gradient, for a unit a residual joined.
 * sscg_conv2d_dgrad_bsums_bytes returns 0 when the fusion does not apply to the geometry (strided / few-channel data gradients,
 * groups shorter than a tile): use sscg_conv2d_dgrad + sscg_norm_bwd.
 * sscg_conv2d_dgrad_add: the addend alone (no sums), wherever sscg_conv2d_dgrad_add_applies (the split family, any stride).
 * sscg_conv2d_dgrad_bsums_masked: the same arguments, the same sums; dx receives the MASKED gradient gg = mask ? dgrad + addend : +0
 * instead of the total - bit for bit what sscg_norm_bwd_from_sums would form from the total and the mask source (and write to dres).
 * That call then runs with act = SSCG_ACT_NONE, y = NULL, dres = NULL on this dx (the same expression on the same values, one
 * tensor less read and one less written); the residual's gradient is dx itself.  act == SSCG_ACT_RELU only - a 0 / 1 mask may be
 * applied a second time by a caller that lost the records, LeakyReLU's may not.  SSCG_ERR_UNSUPPORTED, before any launch: any other
 * activation, the bf16 family, every geometry for which sscg_conv2d_dgrad_bsums_bytes is 0.  (An addition: no existing entry
 * changes meaning, so SSCG_ABI_VERSION stays 18.) */
size_t sscg_conv2d_dgrad_bsums_bytes(const sscg_conv_desc* d, int G, int64_t L);
int sscg_conv2d_dgrad_bsums(const sscg_conv_desc* d, const void* dy, const void* wt, void* dx, const void* nx, const void* nz,
                            const void* addend, const float* mean, const float* rstd, const float* gamma, const float* beta, int G,
                            int64_t L, int act, float slope, void* sums, size_t sums_bytes, void* ws, size_t ws_bytes, void* stream);
int sscg_conv2d_dgrad_bsums_masked(const sscg_conv_desc* d, const void* dy, const void* wt, void* dx, const void* nx, const void* nz,
                                   const void* addend, const float* mean, const float* rstd, const float* gamma, const float* beta, int G,
                                   int64_t L, int act, float slope, void* sums, size_t sums_bytes, void* ws, size_t ws_bytes,
                                   void* stream);
int sscg_conv2d_dgrad_add_applies(const sscg_conv_desc* d);
int sscg_conv2d_dgrad_add(const sscg_conv_desc* d, const void* dy, const void* wt, const void* addend, void* dx, void* ws,
                          size_t ws_bytes, void* stream);
/* flags: bit 1 = dgamma / dbeta are written (else accumulated); ws: G * C * 2 floats.
 * A dy left by sscg_conv2d_dgrad_bsums_masked already IS gg: pass act = SSCG_ACT_NONE, y = NULL, dres = NULL. */
int sscg_norm_bwd_from_sums(const sscg_conv_desc* d, const void* sums, const void* dy, const void* x, const void* y, const float* mean,
                            const float* rstd, const float* gamma, const float* beta, void* dx, void* dres, float* dgamma, float* dbeta,
                            int dtype, int G, int64_t L, int C, int act, float slope, int flags, void* ws, size_t ws_bytes, void* stream);

int sscg_rstd_from_var(const float* var, float* rstd, int n, float eps, void* stream);
/* backward of norm_apply (+ of the statistics): dx always; dres (= masked dy) if non-NULL;
 * dgamma/dbeta accumulate (+=) if non-NULL.  `y` (the forward output) supplies the activation mask; with ReLU / LeakyReLU
 * and NO residual in the forward, y may be NULL: the mask is then recomputed as gamma * xhat + beta > 0 (the forward's own
 * expression; beta is only read in that case) and the kernels read one tensor less.
 * stats_grad bit 0: 0 = the statistics are constants (eval-mode BN); bit 1 (value 2): dgamma / dbeta are WRITTEN instead of
 * accumulated (the caller then needs no zero-fill). */
size_t sscg_norm_bwd_workspace(int G, int64_t L, int C);
int sscg_norm_bwd(const void* dy, const void* x, const void* y, const float* mean, const float* rstd,
                  const float* gamma, const float* beta, void* dx, void* dres, float* dgamma, float* dbeta, int dtype, int G,
                  int64_t L, int C, int act, float slope, int stats_grad, void* ws, size_t ws_bytes, void* stream);   /* dy, x, y, dx, dres share `dtype` */

/* PixelDiscriminator tail, arch/discriminators.py:72-75: norm_layer(2 ndf) -> nn.LeakyReLU(0.2) -> nn.Conv2d(2 ndf, 1, 1x1) as ONE
 * pass over the C-channel map x (the conv output the statistics were taken from): out[r] = bias + sum_c w[c] * act(norm(x)[r][c]),
 * out fp32 [G * L].  The normalised map is never materialised, in either direction: the backward recomputes it from x, forms
 * dy[r][c] = dout[r] * w[c] in registers, and produces dx (gradient at x, dtype of x), dw[C] / dbias[1] (the head's weight and bias
 * gradient) and dgamma / dbeta.  flags: bit 0 = the statistics are functions of x (training-mode normalisation), bit 1 = dgamma /
 * dbeta are written (else accumulated), bit 2 = dw / dbias are written (else accumulated).  C: a power of two in [16, 256]
 * (sscg_norm_head_applies); act: none / ReLU / LeakyReLU. */
int sscg_norm_head_applies(int C);
int sscg_norm_head_fwd(const void* x, int dtype, const float* mean, const float* rstd, const float* gamma, const float* beta,
                       const float* w, const float* bias, float* out, int G, int64_t L, int C, int act, float slope, void* stream);
size_t sscg_norm_head_bwd_workspace(int G, int64_t L, int C);
int sscg_norm_head_bwd(const float* dout, const float* w, const void* x, const float* mean, const float* rstd, const float* gamma,
                       const float* beta, void* dx, float* dw, float* dbias, float* dgamma, float* dbeta, int dtype, int G, int64_t L,
                       int C, int act, float slope, int flags, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ pointwise / pooling / resize */
/* standalone activation (nn.ReLU / nn.LeakyReLU / nn.Tanh not adjacent to a norm) */
int sscg_act_fwd(const void* x, void* y, int dtype, int64_t n, int act, float slope, void* stream);
int sscg_act_bwd(const void* dy, const void* y, void* dx, int dtype, int64_t n, int act, float slope, void* stream);
/* y = a + b */
int sscg_add(const void* a, const void* b, void* y, int dtype, int64_t n, void* stream);
/* dst[r][c] = (c < Cs) ? src[r][c] : 0 for c < Cd, r < rows (fp32): an NHWC tensor (or a [K][R][S][C] weight) with its channels
 * padded with zeros (Cd > Cs) or cut (Cd < Cs).  No reference counterpart: the 21-channel stems (arch/generators.py:73,373 on a
 * one-hot / softmax map) run as 32-channel convolutions on the split contraction - a zero channel meets a zero weight - and the data
 * gradient's extra channels are cut again. */
int sscg_resize_channels(const float* src, float* dst, int64_t rows, int Cs, int Cd, void* stream);
/* nn.Dropout(0.5) in training mode (arch/ops.py:66): y = x * keep / (1-p); keep is derived from a
 * counter-based hash of (seed, element index), so backward can regenerate it. */
int sscg_dropout(const void* x, void* y, int dtype, int64_t n, float p, uint64_t seed, void* stream);
/* utils.GaussianNoise (utils.py:116-140; call site model.py:486-488): y = x + sigma * x * n, n ~ N(0, 1) drawn from a
 * counter-based hash of (seed, element index) through Box-Muller. */
int sscg_gauss_noise(const float* x, float* y, int64_t n, float sigma, uint64_t seed, void* stream);
/* nn.MaxPool2d(2, 2) (floor mode: P = H / 2, Q = W / 2) of torchvision's VGG16 features (utils.Vgg16, utils.py:147-164);
 * idx = window position 0..3 of the first max */
int sscg_maxpool2x2_fwd(const void* x, void* y, uint8_t* idx, int dtype, int N, int H, int W, int C, void* stream);
int sscg_maxpool2x2_bwd(const void* dy, const uint8_t* idx, void* dx, int dtype, int N, int H, int W, int C, void* stream);
/* nn.MaxPool2d(3, 2, 1, ceil_mode=True) (arch/generators.py:394); idx = window position 0..8 of the first max */
int sscg_maxpool3x3s2_fwd(const void* x, void* y, uint8_t* idx, int dtype, int N, int H, int W, int C, int P, int Q, void* stream);
int sscg_maxpool3x3s2_bwd(const void* dy, const uint8_t* idx, void* dx, int dtype, int N, int H, int W, int C, int P, int Q, void* stream);
/* nn.Upsample(size, mode='bilinear', align_corners=True) (model.py:268, calls :390-392,:413-415) */
int sscg_upsample_bilinear_fwd(const float* x, float* y, int N, int H, int W, int C, int OH, int OW, void* stream);
int sscg_upsample_bilinear_bwd(const float* dy, float* dx, int N, int H, int W, int C, int OH, int OW, void* stream);
/* nn.ReflectionPad2d as a materialised copy (only for callers that cannot fold it) */
int sscg_reflect_pad(const void* x, void* y, int dtype, int N, int H, int W, int C, int pad, void* stream);
int sscg_reflect_pad_bwd(const void* dy, void* dx, int dtype, int N, int H, int W, int C, int pad, void* stream);
/* layout plumbing at the NCHW boundary of the reference's module interface */
int sscg_nchw_to_nhwc(const float* x, float* y, int N, int C, int H, int W, void* stream);
int sscg_nhwc_to_nchw(const float* x, float* y, int N, int C, int H, int W, void* stream);

/* ------------------------------------------------------------------ class-axis ops (K10, K12) : x is [rows][C] */
/* nn.Softmax2d (model.py:273, calls :401-402,:420-421) */
int sscg_softmax_fwd(const float* x, float* y, int64_t rows, int C, void* stream);
int sscg_softmax_bwd(const float* dy, const float* y, float* dx, int64_t rows, int C, void* stream);
/* fake_gt.data.max(1)[1] -> make_one_hot (model.py:435-437,:509-511; utils.py:344-348): first max wins */
int sscg_argmax_onehot(const float* x, float* onehot, int64_t* index, int64_t rows, int C, void* stream);
/* make_one_hot(labels) (utils.py:314-350) */
int sscg_label_onehot(const int64_t* labels, float* onehot, int64_t rows, int C, void* stream);
/* runningScore._fast_hist (utils.py:363-369) of the per-epoch evaluation (model.py:555-574):
 * hist[C*t + p] += 1 for every pixel with 0 <= t < C (others, e.g. the 255 "void" label, are ignored).
 * `hist` is int64 [C][C] on the device and is accumulated into; C <= 64. */
int sscg_confusion_hist(const int64_t* label_true, const int64_t* label_pred, int64_t n, int C, int64_t* hist, void* stream);
/* Class frequencies of a label map, the input of the class-weight rules of the weighted cross entropy (median-frequency balancing,
 * ENet's 1 / ln(k + f)): counts[c] += #{labels == c}; ids outside [0, C) are ignored.  `counts` is int64 [C] on the device and is
 * accumulated into; C <= 64.  Per-block LDS histogram, then integer atomics: exact, as sscg_confusion_hist.  n == 0 is a no-op. */
int sscg_label_hist(const int64_t* labels, int64_t n, int C, int64_t* counts, void* stream);

/* ------------------------------------------------------------------ input pipeline
 * The tail of the reference's per-sample transforms, batched on the device: images travel to HBM as the uint8
 * pixels PIL decoded / resized / cropped, labels as their uint8 ids.
 * ToTensor + Normalize (data_utils/__init__.py:126-150): y = ((float)u / 255 - mean[c]) / std[c], the same two fp32
 * operations in the same order => bit-exact.  src uint8 [rows][C] (HWC pixels of a batch), dst fp32 NHWC. */
int sscg_image_u8_to_f32(const uint8_t* src, float* dst, int64_t rows, int C, const float* mean, const float* stdev, void* stream);
/* ToLabel + Relabel(255, 0) (data_utils/__init__.py:34-58) / CityscapesDataset.encode_segmap (dataloader.py:260-267) as
 * one 256-entry table: dst[i] = lut[src[i]] (int64 out, the dtype of `.long()`). */
int sscg_label_lut(const uint8_t* src, int64_t* dst, int64_t n, const int64_t* lut256, void* stream);
/* Batched affine augmentation fused into the two passes above: one launch warps every sample of a uint8 batch by its own integer
 * affine map and finishes it.  img uint8 [N][H][W][C] (C in 1..4), gt (nullable) uint8 [N][H][W], mats int32 [N][6] on the device,
 * out_img fp32 [N][OH][OW][C], out_gt (with gt) int64 [N][OH][OW].  For output pixel (ox, oy) of sample n, m = mats[n], in int64:
 *     sx = m0*ox + m1*oy + m2        sy = m3*ox + m4*oy + m5          Q16 source INDEX coordinates (the pixel-centre offsets of
 *                                                                     both grids are folded into m2 / m5 by the host)
 *   label: ix = (sx + 0x8000) >> 16, iy = (sy + 0x8000) >> 16 (arithmetic shifts); id = gt[n][iy][ix], or label_fill outside
 *     [0, W) x [0, H); out_gt = lut256[id] (label_fill is a raw id: it goes through the table like a source pixel).
 *   image: x0 = sx >> 16, y0 = sy >> 16, fx = (sx & 0xFFFF) >> 8, fy = (sy & 0xFFFF) >> 8; the four taps (y0 | y0+1, x0 | x0+1), a
 *     tap outside the image = image_fill; per channel top = a*(256-fx) + b*fx, bot likewise for the lower row,
 *     v = top*(256-fy) + bot*fy (an exact integer < 2^24); t = ((float)v * 2^-16) / 255; out = (t - mean[c]) / stdev[c], every
 *     operation rounded to nearest on its own - the last two are sscg_image_u8_to_f32's, so with the identity map (m0 = m4 = 65536,
 *     the rest 0, OH = H, OW = W) both outputs equal sscg_image_u8_to_f32's and sscg_label_lut's bit for bit.
 * Bilinear without antialiasing (a minifying map samples, it does not average).  Errors before any HIP call: SSCG_ERR_BAD_ARG (null
 * tensors, C outside 1..4, non-positive sizes, a fill outside 0..255, gt without lut256 or out_gt, out_gt without gt),
 * SSCG_ERR_UNSUPPORTED (N*OH*OW >= 2^31, H or W above 32767).
 * (An addition: no existing entry changes meaning, so SSCG_ABI_VERSION stays 18, as for the inference heads below.) */
int sscg_augment_u8(const uint8_t* img, const uint8_t* gt, const int32_t* mats, float* out_img, int64_t* out_gt, int N, int H, int W, int C,
                    int OH, int OW, const float* mean, const float* stdev, const int64_t* lut256, int image_fill, int label_fill,
                    void* stream);
/* sscg_augment_u8 with a per-sample colour map between the warp and the normalisation (brightness, contrast, saturation, hue, grey,
 * composed on the host: data_utils/augmentations.py).  colour fp32 [N][21] on the device = (A 3x3 row-major, B 3x3 row-major, b[3])
 * of every sample; the other arguments, the warp, v and t[c] = ((float)v[c] * 2^-16) / 255, the labels and the errors are
 * sscg_augment_u8's.  Definition, every fp32 product and sum rounded to nearest on its own (no fused multiply-add):
 *   mean:   need_mean != 0:  S[n][c] = the sum of the integer v[c] over the sample's OH*OW output pixels, fill pixels included
 *           (int64: exact, and the same in every run);  mu[c] = (float)((double)S[n][c] / ((double)(OH*OW) * 16711680.0)), one
 *           rounding per fp64 operation and one for the narrowing.  need_mean == 0: mu = 0.
 *   offset: o[c] = ((B[c][0]*mu[0] + B[c][1]*mu[1]) + B[c][2]*mu[2]) + b[c]
 *   pixel:  u[c] = ((A[c][0]*t[0] + A[c][1]*t[1]) + A[c][2]*t[2]) + o[c];  u[c] = min(max(u[c], 0), 1);
 *           out = (u[c] - mean[c]) / stdev[c]
 *   C == 1: o = B[0][0]*mu[0] + b[0], u = A[0][0]*t[0] + o (only these three entries of the 21 are read).
 * With A = I, B = 0, b = 0 every step is exact: the outputs equal sscg_augment_u8's bit for bit.  Table entries are finite.
 * One launch; with need_mean two more in front of it, on the same stream: ws is cleared and a sum pass warps the batch once more
 * for S (uint8 gathers, one 64-bit integer atomic per block and channel).  ws: sscg_augment_colour_workspace(N) bytes (int64
 * [N][3]), 8-byte aligned; may be NULL without need_mean.  Errors before any HIP call: SSCG_ERR_BAD_ARG (sscg_augment_u8's cases, a
 * NULL colour, need_mean with a NULL or misaligned ws), SSCG_ERR_UNSUPPORTED (sscg_augment_u8's size limits, C of 2 or 4, need_mean
 * with N above 65535). */
size_t sscg_augment_colour_workspace(int N);
int sscg_augment_colour_u8(const uint8_t* img, const uint8_t* gt, const int32_t* mats, float* out_img, int64_t* out_gt, int N, int H, int W,
                           int C, int OH, int OW, const float* mean, const float* stdev, const int64_t* lut256, int image_fill,
                           int label_fill, const float* colour, int need_mean, void* ws, void* stream);
/* sscg_augment_colour_u8 with an elastic (free-form) deformation added to the affine source coordinate: a uniform cubic B-spline over
 * a coarse lattice of control nodes per sample, evaluated per output pixel in integers.  colour may be NULL = no colour stage (then
 * need_mean and ws are ignored and every C in 1..4 is taken); the other arguments of sscg_augment_colour_u8 mean what they mean there.
 *   lattice: nodes int32 [N][GH][GW][2] on the device, grid >= 4 the node spacing in OUTPUT pixels, GH = (OH-1)/grid + 4,
 *            GW = (OW-1)/grid + 4 (integer division).  Component 0 is the x, component 1 the y displacement, in SOURCE pixels, Q16:
 *            the host has multiplied the 2x2 linear part of the sample's affine map into its lattice (the interpolation is linear in
 *            the nodes, so that is exact up to the rounding of the nodes).  |node| < 2^26.
 *   cell:    for output pixel (oy, ox): cx = ox / grid, tx = ((ox - cx*grid) * 256) / grid; cy, ty likewise from oy.
 *   weights: the four B-spline weights at t in 0..255 are the integer numerators over D = 6 * 2^24
 *              n0 = (256-t)^3    n1 = 3t^3 - 6*256 t^2 + 4*256^3    n2 = -3t^3 + 3*256 t^2 + 3*256^2 t + 256^3    n3 = t^3
 *            (non-negative, each below 2^31, the four sum to D exactly).
 *   y pass, then x pass, per component, in int64 with FLOOR division (negative values too; every sum stays below 2^53):
 *              c_j = floor((sum_i n_i(ty) * node[cy+i][cx+j] + D/2) / D)   j = 0..3
 *              d   = floor((sum_j n_j(tx) * c_j + D/2) / D)
 *   sample:  sx = m0*ox + m1*oy + m2 + d_x    sy = m3*ox + m4*oy + m5 + d_y; everything behind (sx, sy) is sscg_augment_u8's and
 *            sscg_augment_colour_u8's: taps and fill, the nearest label index, the tables, the two fp32 divisions - and the sum pass
 *            of need_mean sums the DISPLACED pixels.
 * An all-zero lattice gives the bits of the affine entries; a constant lattice (a, b) those of the affine entries with m2 + a and
 * m5 + b (the weights sum to D).  Errors before any HIP call: SSCG_ERR_BAD_ARG (sscg_augment_u8's cases, a NULL nodes, grid < 4, GH or
 * GW other than the formula's, with a colour table need_mean with a NULL or misaligned ws), SSCG_ERR_UNSUPPORTED (sscg_augment_u8's
 * size limits, grid above 2^22; with a colour table C of 2 or 4 and need_mean with N above 65535).
 * (An addition: no existing entry changes meaning or bits, so SSCG_ABI_VERSION stays 18.) */
int sscg_augment_elastic_u8(const uint8_t* img, const uint8_t* gt, const int32_t* mats, float* out_img, int64_t* out_gt, int N, int H, int W,
                            int C, int OH, int OW, const float* mean, const float* stdev, const int64_t* lut256, int image_fill,
                            int label_fill, const float* colour, int need_mean, void* ws, const int32_t* nodes, int grid, int GH, int GW,
                            void* stream);
/* sscg_augment_elastic_u8 with mixed-sample augmentation (CutMix, ClassMix): every output pixel shows its own sample or, pasted, the
 * sample's partner, image and label alike, decided inside the same launch.  colour may be NULL as there; nodes may be NULL too = no
 * lattice (grid, GH and GW are then ignored); the other arguments of sscg_augment_elastic_u8 mean what they mean there.
 *   table:   mix int32 [N][8] on the device = (partner, x0, y0, x1, y1, mask_lo, mask_hi, 0) per sample.  p = mix[n][0] outside
 *            [0, N), or p == n: sample n is not mixed.  No table content is an error and none is unsafe: only a valid p indexes
 *            memory, the other fields are compared and shifted.
 *   pasted:  output pixel (n, oy, ox) of a mixed sample is pasted if
 *              (box)   x0 <= ox < x1 and y0 <= oy < y1 - a half-open rectangle of OUTPUT pixels, which may be empty or reach beyond
 *                      the output: the comparisons alone decide - or
 *              (class) classes != 0, the pixel is not in the box, and with id_p the raw label id of sample p at (oy, ox) - p's own
 *                      matrix, p's own lattice, the nearest index, label_fill outside the source: sscg_augment_u8's label rule -
 *                      cls = lut256[id_p] satisfies 0 <= cls < 64 and bit cls of (mask_hi << 32) | (uint32)mask_lo is set.
 *   pixel:   a pasted pixel's C channels and its label are those of sample p at (oy, ox): p's matrix, p's lattice, p's colour table
 *            with p's mean; an unpasted pixel is sample n's own.  The partner's pixel is always p's UNMIXED pixel: chains (n takes
 *            from p while p takes from q) do not propagate.  The sum pass of need_mean is unchanged: every sample's mean is that of
 *            its own unmixed warped pixels.
 * So out[n] = where(pasted, plain[p], plain[n]) bit for bit, image and label, plain being what sscg_augment_u8, _colour_u8 or
 * _elastic_u8 (whichever fits the other arguments) returns for the batch; an all-unmixed table gives plain.  Same taps per output
 * pixel (the source sample is decided first), at most one more label gather, nothing more written.
 * Errors before any HIP call: SSCG_ERR_BAD_ARG (sscg_augment_u8's cases, a NULL mix, classes != 0 without gt, with nodes grid < 4 or
 * GH or GW other than the formula's, with a colour table need_mean with a NULL or misaligned ws), SSCG_ERR_UNSUPPORTED
 * (sscg_augment_u8's size limits, C of 2 or 4, with nodes grid above 2^22, need_mean with N above 65535).
 * (An addition: no existing entry changes meaning or bits, so SSCG_ABI_VERSION stays 18.) */
int sscg_augment_mix_u8(const uint8_t* img, const uint8_t* gt, const int32_t* mats, float* out_img, int64_t* out_gt, int N, int H, int W,
                        int C, int OH, int OW, const float* mean, const float* stdev, const int64_t* lut256, int image_fill, int label_fill,
                        const float* colour, int need_mean, void* ws, const int32_t* nodes, int grid, int GH, int GW, const int32_t* mix,
                        int classes, void* stream);

/* ------------------------------------------------------------------ losses (K10, K11), mean reduction
 * Each forward writes one fp32 scalar to `loss` (device).  Each backward takes the upstream gradient as
 * a device scalar `gscale` (NULL = 1) times the host factor `w`. */
size_t sscg_loss_workspace(int64_t n);
/* nn.CrossEntropyLoss (model.py:272; calls :398,:455): logits [rows][C], labels [rows].  Pixels whose label is outside
 * [0, C) are ignored (no read past the row, excluded from the mean, zero gradient) - torch's ignore_index behaviour for
 * every out-of-range id.  `valid` (nullable) receives the number of counted pixels; the backward divides by it
 * (NULL = rows).  No counted pixel at all: the loss is NaN (torch's 0 / 0), the gradient zero. */
int sscg_ce_fwd(const float* logits, const int64_t* labels, int64_t rows, int C, float* loss, float* valid, void* ws,
                size_t ws_bytes, void* stream);
int sscg_ce_bwd(const float* logits, const int64_t* labels, int64_t rows, int C, const float* gscale, float w,
                const float* valid, float* dx, void* stream);
/* Class-weighted, label-smoothed cross entropy: F.cross_entropy(logits, labels, weight=class_w, label_smoothing=smoothing) once
 * every label outside [0, C) is mapped to the ignore index - sscg_ce_fwd / _bwd plus two arguments.  class_w: device pointer to [C]
 * fp32, NULL = all ones; smoothing (eps) in [0, 1).  With p = softmax(z) of a pixel, y its label, W = sum_c class_w[c], and a pixel
 * COUNTED when 0 <= y < C:
 *     term    = (1-eps) * w[y] * (-log p[y]) + (eps/C) * sum_c w[c] * (-log p[c])
 *     loss    = sum over the counted pixels of term / D,      D = sum over the counted pixels of w[y]
 *     d loss / d z[c] = ((1-eps) * w[y] * (p[c] - [c==y]) + (eps/C) * (p[c] * W - w[c])) / D        (0 for a pixel not counted)
 * The smoothing part of a counted pixel is NOT multiplied by w[y]: a pixel of a weight-0 class still adds it.  `valid` receives D (a
 * float rounded from the fp64 sum); the backward divides by it (NULL = rows).  D == 0 - no counted pixel, or every counted pixel in a
 * weight-0 class: the loss is NaN, the gradient zero (sscg_ce_fwd's rule for "no counted pixel").  class_w == NULL && smoothing == 0
 * runs sscg_ce_fwd / _bwd themselves: the same kernels, the same bits.  The weights are not checked here (the host checks them once,
 * when it makes them: finite, >= 0).  Errors before any HIP call: SSCG_ERR_BAD_ARG (smoothing outside [0, 1) or NaN; then the rules of
 * sscg_ce_fwd / _bwd), SSCG_ERR_WORKSPACE.  (An addition: no existing entry changes meaning, so SSCG_ABI_VERSION stays 18.) */
int sscg_ce_fwd_w(const float* logits, const int64_t* labels, int64_t rows, int C, const float* class_w, float smoothing, float* loss,
                  float* valid, void* ws, size_t ws_bytes, void* stream);
int sscg_ce_bwd_w(const float* logits, const int64_t* labels, int64_t rows, int C, const float* class_w, float smoothing,
                  const float* gscale, float w, const float* valid, float* dx, void* stream);
/* The head of the segmentation generator without the resized logits in memory (ABI v12): x = low-resolution logits [N][H][W][C]
 * (C <= 64), resized to [OH][OW] by bilinear interpolation with align_corners=True (model.py:390-392, the arithmetic of
 * sscg_upsample_bilinear_fwd), then
 *   labels != NULL ([N][OH][OW]): nn.CrossEntropyLoss of the resized logits (model.py:398, :455; sscg_ce_fwd's label rules) into
 *     `loss` / `valid`, and `dlogits` [N][H][W][C] = sum over the counted pixels of d(their loss term) / dx - the gradient with
 *     respect to x up to the factor g / valid, which sscg_upsample_head_bwd applies;
 *   y_soft != NULL ([N][OH][OW][C]): softmax over C of the resized logits (model.py:401-402).
 * sscg_upsample_head_bwd: dx = adjoint of the resize applied to softmax_bwd(dy_soft, y_soft) (dy_soft NULL: that branch is unused)
 * + dlogits * g_ce / valid (dlogits NULL: no cross-entropy branch; g_ce NULL = 1).  Gather form, fixed summation order.
 * It serves sscg_upsample_head_fwd_w unchanged: that forward leaves dlogits = sum over the counted pixels of d(their weighted,
 * smoothed term) / dx and valid = D, and the gradient is again dlogits * g_ce / valid.
 * ws: sscg_upsample_head_workspace bytes (cross-entropy branch only).
 * sscg_upsample_head_fwd_w: sscg_upsample_head_fwd with the cross entropy of sscg_ce_fwd_w (class_w NULL = all ones, smoothing in
 * [0, 1); the formulas above, on the resized logits): `loss`, `valid` (= D) and `dlogits` follow them, the forward still leaves the
 * gradient, the y_soft branch is untouched (the same bits).  The weighted form is its own kernel instantiation; labels == NULL, or
 * class_w == NULL && smoothing == 0, runs sscg_upsample_head_fwd itself.  Errors before any HIP call: SSCG_ERR_BAD_ARG for a smoothing
 * outside [0, 1), then sscg_upsample_head_fwd's rules. */
size_t sscg_upsample_head_workspace(int N, int H, int W);
int sscg_upsample_head_fwd(const float* x, const int64_t* labels, float* y_soft, float* loss, float* valid, float* dlogits, int N, int H,
                           int W, int C, int OH, int OW, void* ws, size_t ws_bytes, void* stream);
int sscg_upsample_head_fwd_w(const float* x, const int64_t* labels, const float* class_w, float smoothing, float* y_soft, float* loss,
                             float* valid, float* dlogits, int N, int H, int W, int C, int OH, int OW, void* ws, size_t ws_bytes,
                             void* stream);
int sscg_upsample_head_bwd(const float* x, const float* dy_soft, const float* dlogits, const float* g_ce, const float* valid, float* dx,
                           int N, int H, int W, int C, int OH, int OW, void* stream);
/* Soft Dice loss of the same head (opt-in; the reference has none).  x = logits [N][H][W][C] (C <= 64), labels [N][OH][OW];
 * p = softmax over C of the logits resized to [OH][OW] (bilinear, align_corners=True, the arithmetic of sscg_upsample_bilinear_fwd;
 * OH == H && OW == W: the logits themselves - the flat Dice of [rows][C] logits, no interpolation arithmetic).  class_w: device
 * pointer to [C] fp32 weights w_c >= 0, NULL = all ones; smooth s > 0; batch in {0, 1}.  A pixel is COUNTED when 0 <= y < C
 * (sscg_ce_fwd's rule: 255 and -100 are void).  Groups: G = N, one per sample (batch == 0), or G = 1, the whole call (batch == 1).
 * Per group g and class c, over the counted pixels of the group:
 *     I = sum p_c [y == c]     P = sum p_c     T = sum [y == c]          Num = 2 I + s     Den = P + T + s
 *     dice[g][c] = Num / Den                  loss = 1 - sum_{g,c} w_c dice[g][c] / (G sum_c w_c)
 * and with k_c = w_c / (G sum_c w_c) the derivative with respect to a counted pixel's probability is A[g][c] [y == c] + B[g][c],
 *     A = -2 k_c / Den          B = k_c Num / Den^2
 * (0 for a pixel not counted); then d loss / d z_c = p_c (g_c - sum_k p_k g_k), through the adjoint of the resize.
 * s > 0 keeps every Den positive: a group with no counted pixel has dice = 1 for every class (it adds nothing to the loss and gets a
 * zero gradient - never a NaN), a class absent from a group's labels (T = 0) still gets the B part.  The weights are not checked here
 * (the host checks them once: finite, >= 0, not all zero).  Under data parallelism the sums are per rank.
 * sscg_dice_fwd: `loss` (fp32 scalar), `sums` (nullable) [G][C][3] fp64 in the order (I, P, T), `coef` [G][C][2] fp32 in the order
 *   (A, B) - all the backward needs.  Three launches: the statistics (one thread per output pixel, no block straddles a sample, fp64
 *   records in the workspace), their sum per (sample, class), and the finish (one small block; with batch the samples are added in
 *   index order).  Deterministic: no float atomics, every sum in a fixed order - the
 *   same call twice gives the same bits, and the resized form gives the bits of the identity form on sscg_upsample_bilinear_fwd's
 *   output.  Neither the resized logits nor the probabilities are written.  ws: sscg_dice_workspace(N, OH, OW, C) bytes.
 * sscg_dice_bwd: the flat backward (logits [N][H][W][C], labels [N][H][W], the coef of an identity-size sscg_dice_fwd with the same
 *   N and batch): dx = (g ? *g : 1) * w * p_c (g_c - sum_k p_k g_k), a zero row for a pixel that is not counted.
 * sscg_upsample_head_bwd_d: the WHOLE backward of the head in one launch when the Dice branch is live - sscg_upsample_head_bwd plus
 *   the Dice term: dx = adjoint of the resize applied to softmax_bwd(dy_soft + g_dice * (A [y == c] + B), y_soft)
 *   + dlogits * g_ce / valid.  dy_soft and dlogits are nullable (those branches unused; g_ce NULL = 1, g_dice NULL = 1); coef and
 *   labels are required.  Gather form (one block per source pixel), fixed summation order.  dlogits / valid are what
 *   sscg_upsample_head_fwd[_w] left - with Dice on, the head's forward is that entry (where the cross entropy or y_soft is wanted)
 *   plus sscg_dice_fwd; those entries are untouched.
 * Errors before any HIP call: SSCG_ERR_BAD_ARG (null tensors, C outside 1..64, non-positive sizes, smooth <= 0 / NaN / infinite,
 * batch outside {0, 1}, dlogits without valid), SSCG_ERR_UNSUPPORTED (N*OH*OW or N*H*W >= 2^31), SSCG_ERR_WORKSPACE.
 * (Additions: no existing entry changes meaning, so SSCG_ABI_VERSION stays 18.) */
size_t sscg_dice_workspace(int N, int OH, int OW, int C);
int sscg_dice_fwd(const float* x, const int64_t* labels, int N, int H, int W, int C, int OH, int OW, const float* class_w, float smooth,
                  int batch, float* loss, double* sums, float* coef, void* ws, size_t ws_bytes, void* stream);
int sscg_dice_bwd(const float* x, const int64_t* labels, int N, int H, int W, int C, const float* coef, int batch, const float* g,
                  float w, float* dx, void* stream);
int sscg_upsample_head_bwd_d(const float* x, const int64_t* labels, const float* dy_soft, const float* dlogits, const float* g_ce,
                             const float* valid, const float* coef, const float* g_dice, int batch, float* dx, int N, int H, int W,
                             int C, int OH, int OW, void* stream);
/* Hard-pixel mining (OHEM) cross entropy of the same head (opt-in; the reference has none): the cross entropy of sscg_ce_fwd_w over the
 * hardest pixels only.  x = logits [N][H][W][C] (C <= 64), labels [N][OH][OW]; p = softmax over C of the logits resized to [OH][OW]
 * (bilinear, align_corners=True, the pinned arithmetic of sscg_upsample_bilinear_fwd and sscg_softmax_fwd - what sscg_predict_head
 * computes per pixel; OH == H && OW == W: p = softmax(x), the flat form on [rows][C] logits, no interpolation arithmetic).  A pixel is
 * COUNTED when 0 <= y < C (sscg_ce_fwd's rule).  Selection:
 *     key     k = p[y], an fp32 value in [0, 1], of every counted pixel;          V = the counted pixels of the call (the whole batch
 *             of this rank: under data parallelism the selection is per rank, as the Dice sums are)
 *     thresh  theta in (0, 1];     min_kept K >= 0;     min_frac f in [0, 1]
 *     r     = clamp(max(K, ceil(f * V)), 1, V), formed on the device (the product in fp64 from the fp32 f)
 *     m     = the r-th smallest key (1-based, exact, ties included)               tau = max(m, theta)
 *     KEPT <=> counted and k <= tau
 * so at least r pixels are always kept, every tie at m is kept, and nothing depends on an order among equal keys.  The comparison is
 * <= on purpose, where HRNet's and mmsegmentation's OHEM compare with a strict <: with < a batch whose keys are all equal keeps
 * nothing and the loss is 0 / 0.  Loss and gradient are sscg_ce_fwd_w's with "counted" replaced by "kept":
 *     term    = (1-eps) * w[y] * (-log p[y]) + (eps/C) * sum_c w[c] * (-log p[c])
 *     loss    = sum over the kept pixels of term / D,      D = sum over the kept pixels of w[y]
 *     d loss / d z[c] = ((1-eps) * w[y] * (p[c] - [c==y]) + (eps/C) * (p[c] * W - w[c])) / D   at a kept pixel, 0 at every other
 * The selection is a constant: no gradient flows through tau.  V == 0 or D == 0: the loss is NaN, the gradient zero (sscg_ce_fwd_w's
 * rule).  NaN logits are unspecified (no access leaves the buffers).
 * sscg_ohem_fwd: `keys` fp32 [N][OH][OW] - the key of a counted pixel, 2.0f (a sentinel above every key) elsewhere; `loss`; `valid` =
 *   D; `thr` = tau (fp32 scalar); `counts` int64 [2] = {kept pixels, V} - all on the device, no host sync.  keys and thr are all the
 *   backward needs.  The key pass (one thread per output pixel, no block straddles a sample) writes keys and one more fp32 per pixel
 *   (term) in the workspace; neither the resized logits nor the probabilities reach memory.  m comes from an exact radix select over
 *   the keys' bit patterns (a non-negative fp32 orders like its pattern; a key has 30 significant bits: three digits of ten bits,
 *   per-block histograms in LDS, integer adds to a table the call zeroes on the stream, a one-block scan per digit), then the kept terms
 *   are summed into per-block fp64 records and finished in a fixed order.  No sort, integer atomics only, no float atomics: the same call
 *   twice gives the same bits, and the resized form gives the keys, thr and counts of the identity form on sscg_upsample_bilinear_fwd's
 *   output bit for bit.  ws: sscg_ohem_workspace(N, OH, OW) bytes, contents irrelevant.
 * sscg_ce_bwd_ohem: the flat backward (logits [rows][C], labels / keys [rows], thr / valid from an identity-size sscg_ohem_fwd):
 *   dx = (gscale ? *gscale : 1) * w / D * d term / d z at a pixel with keys[r] <= tau, a zero row elsewhere.
 * sscg_upsample_head_bwd_h: the WHOLE backward of the head in one launch when the cross entropy mines - sscg_upsample_head_bwd_d with
 *   the cross-entropy gradient of the kept pixels formed in the stencil (the forward leaves none): dx = adjoint of the resize applied to
 *   softmax_bwd(dy_soft + g_dice * (A [y == c] + B), y_soft) + [keys <= tau] * (g_ce / D) * d term / d z.  keys NULL: the cross entropy
 *   took no part (else thr and valid are required; g_ce NULL = 1); dy_soft NULL, coef NULL: those branches unused (g_dice NULL = 1;
 *   batch as in sscg_dice_fwd).  At least one branch is required; labels with keys or coef.  Gather form, fixed summation order.
 * Both backwards READ the keep decision from keys and thr; it is never re-derived from recomputed probabilities.
 * Errors before any HIP call: SSCG_ERR_BAD_ARG (null tensors, C outside 1..64, non-positive sizes, smoothing outside [0, 1), thresh
 * outside (0, 1], min_kept < 0, min_frac outside [0, 1] - NaNs included - batch outside {0, 1}, keys without thr / valid),
 * SSCG_ERR_UNSUPPORTED (N*OH*OW, N*H*W or rows >= 2^31), SSCG_ERR_WORKSPACE.
 * (Additions: no existing entry changes meaning, so SSCG_ABI_VERSION stays 18.) */
size_t sscg_ohem_workspace(int N, int OH, int OW);
int sscg_ohem_fwd(const float* x, const int64_t* labels, int N, int H, int W, int C, int OH, int OW, const float* class_w, float smoothing,
                  float thresh, int64_t min_kept, float min_frac, float* keys, float* loss, float* valid, float* thr, int64_t* counts,
                  void* ws, size_t ws_bytes, void* stream);
int sscg_ce_bwd_ohem(const float* logits, const int64_t* labels, const float* keys, const float* thr, int64_t rows, int C,
                     const float* class_w, float smoothing, const float* gscale, float w, const float* valid, float* dx, void* stream);
int sscg_upsample_head_bwd_h(const float* x, const int64_t* labels, const float* keys, const float* thr, const float* class_w,
                             float smoothing, const float* dy_soft, const float* g_ce, const float* valid, const float* coef,
                             const float* g_dice, int batch, float* dx, int N, int H, int W, int C, int OH, int OW, void* stream);
/* Boundary loss on signed distance maps of the same head (opt-in; the reference has none): Kervadec et al., "Boundary loss for highly
 * unbalanced segmentation" (MIDL 2019).  Labels are [N][OH][OW] int64; a pixel is COUNTED when 0 <= y < C (sscg_ce_fwd's rule: 255,
 * -100 and any id >= C are void).
 * Signed squared distance map  sdm[n][oy][ox][c], int32, class innermost (the layout the head's stencil reads):
 *   - for sample n and class c the MEMBERS are the pixels with y == c; void pixels are non-members of every class;
 *   - d2 = the squared Euclidean distance, in pixels, from a pixel to the nearest pixel of the opposite membership in the same sample:
 *     exact at any separation, no window, never across samples;
 *   - sdm = +d2 at a non-member, -d2 at a member;
 *   - sdm = 0 everywhere in the plane when the class has no member in the sample (Kervadec's one_hot2dist leaves zeros for an absent
 *     class) or every pixel of the sample is a member (pinned to zero: there is no opposite pixel to measure to).
 * Level set  phi, fp32, formed from sdm wherever it is needed and never stored:
 *     s > 0: phi = sqrt_rn((float)s)        s < 0: phi = 1 - sqrt_rn((float)(-s))        s == 0: phi = 0
 *   which is distance(neg) * neg - (distance(pos) - 1) * pos; every step is correctly rounded, so sqrt on the fp32 cast gives the same
 *   bits on the host.
 * Loss: p = softmax over C of the logits resized to [OH][OW] (the pinned arithmetic of sscg_upsample_bilinear_fwd and
 *   sscg_softmax_fwd, as in sscg_dice_fwd; OH == H && OW == W: the flat form, no interpolation arithmetic); class_w [C] fp32 >= 0
 *   (NULL = all ones), Wsum = sum_c w_c, V = the counted pixels of the call;
 *     loss = (1 / (V * Wsum)) * sum over counted pixels, sum_c w_c p_c phi_c
 *   V == 0: loss 0, gradient zero (no 0 / 0).  The host refuses Wsum == 0.  The loss may be negative: a perfect prediction sits at
 *   its minimum.  Under data parallelism V is per rank.
 * Gradient: d loss / d p_c = k w_c phi_c at a counted pixel, k = 1 / (V * Wsum); it enters the head's backward as one more term of q_c
 *   in d_c = p_c (q_c - sum_k p_k q_k), beside dy_soft and the Dice term.  The forward leaves k on the device (`coef`).
 * sscg_sdm: a presence pass (members per (n, c): integer atomics through LDS bins), then per chunk of 16 classes a column pass (the
 *   vertical distance to the nearest pixel of the opposite membership, lanes on consecutive columns) and a row pass (a row's column
 *   distances of one class staged in LDS, per pixel the exact minimum of dx^2 + g[x']^2 by a walk outwards that stops when
 *   dx^2 >= best) over EVERY pixel.  Every loop's bound is known at launch, no workgroup waits on another, nothing spins on a value.
 *   Every element of sdm is written (the planes without a contour as zeros); nothing is read from what sdm or the workspace held.
 *   ws: sscg_sdm_workspace(N, H, W, C) bytes: 4 N C for the counts + 2 min(C, 16) bytes per label pixel, 256-byte aligned parts.
 *   sdm itself is 4 C bytes per label pixel.
 * sscg_boundary_loss_fwd: `loss` (fp32 scalar), `sums` (nullable) [N][C] fp64 = per sample and class the sum of p_c phi_c over the
 *   counted pixels (unweighted), `counted` (nullable) = V, `coef` = k (fp32 scalar).  One thread per output pixel, per-block fp64
 *   records, fixed-order reduction, a one-block finish; no float atomics: the same call twice gives the same bits, and the resized form
 *   gives the bits of the identity form on sscg_upsample_bilinear_fwd's output.  Neither the resized logits nor the probabilities are
 *   written.  ws: sscg_boundary_loss_workspace(N, OH, OW, C) bytes.
 * sscg_boundary_loss_bwd: the flat backward (logits [N][H][W][C], labels and sdm at the same size, coef of an identity-size forward):
 *   dx = (g ? *g : 1) * w * p_c (q_c - sum_k p_k q_k), q_c = k w_c phi_c; a zero row for a pixel that is not counted.
 * sscg_upsample_head_bwd_b: the WHOLE backward of the head in one stencil launch when the boundary branch is live - the arguments of
 *   sscg_upsample_head_bwd_h plus sdm, bnd_coef (k), bnd_w (the class weights of the boundary term, NULL = ones) and g_bnd (NULL = 1).
 *   With sdm: labels and bnd_coef are required; the cross entropy is live when `valid` is given - over the pixels with keys <= tau when
 *   keys (and thr) are given, over every counted pixel otherwise (the unmined cross entropy of sscg_ce_fwd_w formed in the stencil, D =
 *   valid) - dy_soft and coef as in _bwd_h.  With sdm == NULL it runs sscg_upsample_head_bwd_h itself (the same kernels, the same
 *   bits), except that valid without keys is refused there: that entry would drop the cross entropy.
 * Errors before any HIP call: SSCG_ERR_BAD_ARG (null tensors, C outside 1..64, non-positive sizes, what _bwd_h refuses),
 * SSCG_ERR_UNSUPPORTED (N*OH*OW or N*H*W >= 2^31, (OH-1)^2 + (OW-1)^2 >= 2^30), SSCG_ERR_WORKSPACE; the workspace queries return 0 for
 * sizes the entries refuse.  (Additions: no existing entry changes meaning, so SSCG_ABI_VERSION stays 18.) */
size_t sscg_sdm_workspace(int N, int H, int W, int C);
int sscg_sdm(const int64_t* labels, int N, int H, int W, int C, int32_t* sdm, void* ws, size_t ws_bytes, void* stream);
size_t sscg_boundary_loss_workspace(int N, int OH, int OW, int C);
int sscg_boundary_loss_fwd(const float* x, const int64_t* labels, const int32_t* sdm, int N, int H, int W, int C, int OH, int OW,
                           const float* class_w, float* loss, double* sums, int64_t* counted, float* coef, void* ws, size_t ws_bytes,
                           void* stream);
int sscg_boundary_loss_bwd(const float* x, const int64_t* labels, const int32_t* sdm, int N, int H, int W, int C, const float* class_w,
                           const float* coef, const float* g, float w, float* dx, void* stream);
int sscg_upsample_head_bwd_b(const float* x, const int64_t* labels, const float* keys, const float* thr, const float* class_w,
                             float smoothing, const float* dy_soft, const float* g_ce, const float* valid, const float* coef,
                             const float* g_dice, int batch, float* dx, int N, int H, int W, int C, int OH, int OW, const int32_t* sdm,
                             const float* bnd_coef, const float* bnd_w, const float* g_bnd, void* stream);
/* The losses of the UNLABELLED head (opt-in; the reference has none): entropy minimisation (Grandvalet & Bengio 2004; ADVENT's MinEnt, Vu
 * et al., CVPR 2019), the maximum-squares loss (Chen et al., ICCV 2019) and the confidence-thresholded pseudo-label cross entropy
 * (self-training, Lee 2013) of the model's own prediction.  x = logits [N][H][W][C] (C <= 64); z = x resized to [OH][OW] (bilinear,
 * align_corners=True, the pinned arithmetic of sscg_upsample_bilinear_fwd and sscg_softmax_fwd as in sscg_dice_fwd; OH == H && OW == W:
 * z = x, the flat form, no interpolation arithmetic).  Per output pixel u_c = z_c - max_k z_k, s = sum_c exp(u_c), p_c = exp(u_c) / s;
 * V = N * OH * OW, every pixel of the call (there is no void on this side; under data parallelism V is per rank):
 *     H     = ln s - sum_c p_c u_c                         L_ent = sum_o H / (V ln C)  in [0, 1]   (C == 1: the divisor is V, H is 0)
 *     L_msq = -sum_o sum_c p_c^2 / (2 V)                   in [-1/2, -1/(2C)]
 *     y*    = the first maximum of p (sscg_argmax_onehot's rule), conf = p[y*];  KEPT <=> conf >= tau;  K = the kept pixels
 *     L_pl  = sum over the kept pixels of (ln s - u[y*]) / max(K, 1)             (K == 0: loss 0, gradient 0)
 * u_c is the logit difference held before the exponentiation, never the logarithm of p_c: a vanished p_c adds exactly 0, not NaN.
 * y* and the keep decision are constants: no gradient flows through them.  With g_e, g_m, g_p the upstream scalars of the three losses:
 *     q_c = dy_soft[c] - (g_e / (V ln C)) u_c - (g_m / V) p_c
 *     d loss / d z_c = p_c (q_c - sum_k p_k q_k) + [kept] (g_p / max(K, 1)) (p_c - [c == y*])
 * sscg_unl_fwd: `losses` fp32 [3] = (L_ent, L_msq, L_pl); `sums` fp64 [4] = (sum H in nats, sum sum p^2, the kept cross entropies' sum,
 *   K) - K is what the backward divides by; `pseudo` (nullable) uint8 [N][OH][OW] = y* of a kept pixel, 255 of a dropped one; thresh =
 *   tau in [0, 1].  One thread per output pixel (no block straddles a sample; K per wave by ballot), one fp64 record per block in the
 *   workspace, a reduce step in index order and a one-block finish: no float atomics - the same call twice gives the same bits, and the
 *   resized form gives the bits of the identity form on sscg_upsample_bilinear_fwd's output (losses, sums and map).  Neither the resized
 *   logits nor the probabilities are written.  ws: sscg_unl_workspace(N, OH, OW) bytes, contents irrelevant.
 * sscg_unl_bwd: the flat backward (logits [N][H][W][C], pseudo / sums from an identity-size sscg_unl_fwd): dx = d loss / d z above
 *   without dy_soft.  g_ent / g_msq / g_pl: device scalars, NULL = that loss took no part (at least one is required; pseudo with g_pl).
 * sscg_upsample_head_bwd_u: the WHOLE backward of the unlabelled head in one stencil launch - sscg_upsample_head_bwd's softmax-map branch
 *   (dy_soft, nullable) plus whichever of the three losses received a gradient, through the adjoint of the resize; pseudo may be NULL
 *   when g_pl is.  Both backwards READ y* and the keep decision from `pseudo`: they are never re-derived from recomputed logits, whose
 *   last bit may differ from the forward's.  With g_ent, g_msq and g_pl all NULL it runs sscg_upsample_head_bwd itself (the same
 *   kernels, the same bits).  Gather form, fixed summation order.
 * Errors before any HIP call: SSCG_ERR_BAD_ARG (null tensors, C outside 1..64, non-positive sizes, thresh outside [0, 1] or NaN, g_pl
 * without pseudo), SSCG_ERR_UNSUPPORTED (N*OH*OW or N*H*W >= 2^31), SSCG_ERR_WORKSPACE; the workspace query returns 0 for sizes the
 * entries refuse.  (Additions: no existing entry changes meaning, so SSCG_ABI_VERSION stays 18.) */
size_t sscg_unl_workspace(int N, int OH, int OW);
int sscg_unl_fwd(const float* x, int N, int H, int W, int C, int OH, int OW, float thresh, float* losses, double* sums, uint8_t* pseudo,
                 void* ws, size_t ws_bytes, void* stream);
int sscg_unl_bwd(const float* x, const uint8_t* pseudo, int N, int H, int W, int C, const float* g_ent, const float* g_msq,
                 const float* g_pl, const double* sums, float* dx, void* stream);
int sscg_upsample_head_bwd_u(const float* x, const uint8_t* pseudo, const float* dy_soft, const float* g_ent, const float* g_msq,
                             const float* g_pl, const double* sums, float* dx, int N, int H, int W, int C, int OH, int OW, void* stream);
/* Mean-teacher consistency of the UNLABELLED head (opt-in, `--unl_teacher`; the reference has none): the student's prediction against
 * the prediction of the same network under the exponential moving average of its weights (Tarvainen & Valpola 2017; French et al. 2020
 * for segmentation), as a squared distance of the probability maps and as a cross entropy against the teacher's confidence-masked hard
 * labels (FixMatch, Sohn et al. 2020).  x = the student's logits [N][H][W][C], t = the teacher's, same shape, 1 <= C <= 64; flip
 * (nullable) uint8 [N]: non-zero = that sample's teacher saw the image mirrored on W.  Per output pixel (n, oy, ox), V = N * OH * OW:
 *     z  = x resized to [OH][OW] (bilinear, align_corners=True, the pinned arithmetic of sscg_upsample_bilinear_fwd as in sscg_unl_fwd;
 *          OH == H && OW == W: the flat form, no interpolation arithmetic), u_c = z_c - max z, s = sum_c exp(u_c), p_c = exp(u_c) / s -
 *          the bits of the head's softmax map;
 *     zt = t resized the same way, read at column ox' = flip[n] ? OW - 1 - ox : ox - sscg_upsample_bilinear_fwd followed by a mirror
 *          on W; v_c = zt_c * inv_temp, ONE fp32 multiply after the resize (sscg_calibration's temperature); q = softmax(v);
 *     y* = the first maximum of q (sscg_argmax_onehot's rule), conf = q[y*];  KEPT <=> conf >= thresh;
 *     d  = sum_c (p_c - q_c)^2: the fp32 difference of the two rounded probabilities, then fmaf from 0 with c ascending;
 *     ce = ln s - u[y*]: sscg_unl_fwd's kept term, from the student's logit difference, never from log p;
 *     agree <=> kept and the first maximum of p is y*.
 * The teacher, y* and the keep decision are constants: no gradient flows through them.
 *   sums   fp64 [4] = (sum over the kept pixels of d, A = the agreeing kept pixels, sum over the kept pixels of ce, K = the kept pixels):
 *          index 3 is K, what the pseudo-label slot of sscg_upsample_head_bwd_u / sscg_unl_bwd divides by;
 *   losses fp32 [2] = (L_mse = sums[0] / (C V), L_ce = sums[2] / max(K, 1)) - the squared distance is averaged over every class of every
 *          pixel (French et al.): a dropped pixel lowers it, and its scale is known at launch;
 *   pseudo (nullable) uint8 [N][OH][OW] = y* of a kept pixel, 255 of a dropped one: sscg_unl_fwd's map, from the teacher;
 *   coef   (nullable) fp32 [N][OH][OW][C] = s (p_c - q_c) at a kept pixel, s = (float)(2.0 / ((double)C V)), one multiply; exactly +0 at
 *          a dropped pixel.  It is d L_mse / d p_c, the dy_soft operand of the head's backward entries: the backward of a node built on
 *          this entry is sscg_lovasz_scale_add(coef, g_mse, dy_soft, out, n) and ONE sscg_upsample_head_bwd_u launch whose pseudo-label
 *          slot takes (pseudo, g_ce, sums).  No backward entry of its own.
 * sscg_unl_fwd's frame: one thread per output pixel, no block straddles a sample, K and A per wave by ballot, one fp64 record per block
 * in the workspace, a reduce step in index order and a one-block finish; no float atomics - the same call twice gives the same bits,
 * whatever ws held - and the resized form gives the bits of the identity form on sscg_upsample_bilinear_fwd's output (mirrored where
 * flip is set).  With t == x, flip NULL and inv_temp == 1: pseudo, sums[3] and sums[2] are sscg_unl_fwd's at the same thresh, sums[0]
 * is 0, A == K and coef is all zeros.  ws: sscg_teacher_workspace(N, OH, OW) bytes, contents irrelevant.
 * Errors before any HIP call: SSCG_ERR_BAD_ARG (a null x, t, losses or sums; non-positive sizes; C outside 1..64; thresh outside [0, 1]
 * or NaN; inv_temp not finite or <= 0), SSCG_ERR_UNSUPPORTED (N*OH*OW or N*H*W >= 2^31), SSCG_ERR_WORKSPACE; the workspace query returns
 * 0 for sizes the entry refuses.  (Additions: no existing entry changes meaning, so SSCG_ABI_VERSION stays 18.) */
size_t sscg_teacher_workspace(int N, int OH, int OW);
int sscg_teacher_fwd(const float* x, const float* t, const uint8_t* flip, int N, int H, int W, int C, int OH, int OW, float inv_temp,
                     float thresh, float* losses, double* sums, uint8_t* pseudo, float* coef, void* ws, size_t ws_bytes, void* stream);
/* CutMix consistency for the mean teacher (opt-in, `--unl_cutmix`; French et al. 2020: the student sees a CutMix of two unlabelled
 * images and is held to the same CutMix of the teacher's predictions of the two UNMIXED images).  Both entries read an int32 [N][8]
 * `table`, sscg_augment_mix_u8's rows (partner, x0, y0, x1, y1, mask_lo, mask_hi, 0); the mask words are not read.  With p = table[n][0]
 *     pasted(n, h, w) <=> 0 <= p < N and p != n and x0 <= w < x1 and y0 <= h < y1
 * - plain integer compares on whatever the row holds: boxes that are empty or reach outside the map are safe and need no clamping,
 * and the partner is range-checked before anything is indexed by it.
 * sscg_mix_boxes: the student's input.  x, y fp32 [N][H][W][C]; y[n][h][w][:] = pasted(n, h, w) ? x[p][h][w][:] : x[n][h][w][:].
 *   Every partner pixel is the partner's pixel before mixing, so y == x is refused.  One launch, a pure copy, every element of y
 *   written once; four floats per thread where H*W*C is a multiple of 4 and both pointers are 16-byte aligned, one otherwise.
 *   Errors before any HIP call: SSCG_ERR_BAD_ARG (a null x, y or table; y == x; non-positive sizes), SSCG_ERR_UNSUPPORTED
 *   (N*H*W*C >= 2^31).
 * sscg_teacher_fwd_mix: the teacher's side - sscg_teacher_fwd, every word of it, except for the sample the TEACHER's logits of an
 *   output pixel (n, oy, ox) come from: src = pasted(n, oy, ox) ? p : n with the box in OUTPUT pixels, and zt = sample src of t,
 *   resized by the pinned arithmetic and read at column flip[src] ? OW - 1 - ox : ox - the partner's flip, not the pixel's own
 *   sample's.  The teacher's logits are low resolution and the box lives at the output resolution, so they cannot be mixed before the
 *   resize; here the resized teacher is never written.  The student, q, y*, the keep rule, d, ce, agree, sums, losses, pseudo, coef,
 *   the workspace (sscg_teacher_workspace) and the finish are sscg_teacher_fwd's: the backward of a node built on this entry is that of
 *   one built on sscg_teacher_fwd.  table == NULL: sscg_teacher_fwd's own kernels, the same bits - as are a table that mixes nothing.
 *   The resized form gives the bits of the identity form on sscg_upsample_bilinear_fwd's outputs of x and t.  Errors: sscg_teacher_fwd's.
 * (Additions: no existing entry changes meaning, so SSCG_ABI_VERSION stays 18.) */
int sscg_mix_boxes(const float* x, float* y, const int32_t* table, int N, int H, int W, int C, void* stream);
int sscg_teacher_fwd_mix(const float* x, const float* t, const uint8_t* flip, const int32_t* table, int N, int H, int W, int C,
                         int OH, int OW, float inv_temp, float thresh, float* losses, double* sums, uint8_t* pseudo, float* coef,
                         void* ws, size_t ws_bytes, void* stream);
/* Segmented stable radix sort (no reference counterpart): S segments of L uint32 keys each, [S][L].  out_keys: every segment in
 * DESCENDING order; out_index: the position (0 .. L-1, int32) each key had in its segment; equal keys keep ascending index.  upper:
 * every key is below it (0: no bound) - a pass over eight-bit digits that are zero in every key is skipped; keys at or above a
 * non-zero `upper` are ordered by their low digits only.  Least significant digit first, three launches per pass (per-block digit
 * histograms in LDS, an exclusive scan of the [digit][block] table, a stable scatter); no block waits for another block of its
 * launch.  Integer arithmetic only, and nothing is read from the workspace before the call wrote it: the same bits from call to
 * call.  The entry reads `keys` and writes the two output planes and `ws` (sscg_sort_ws_bytes(S, L) bytes, 4-byte aligned: two
 * planes of S * L words and the tables) - nothing else.  sscg_sort_chunk: the keys one block of the histogram and scatter passes
 * serves.  Errors before any HIP call: SSCG_ERR_BAD_ARG (null or misaligned pointers, out_keys == keys, non-positive sizes),
 * SSCG_ERR_UNSUPPORTED (S * L >= 2^31, or a table of 2^31 entries; the query then returns 0), SSCG_ERR_WORKSPACE.
 * (Additions: no existing entry changes meaning, so SSCG_ABI_VERSION stays 18.) */
int sscg_sort_chunk(void);
size_t sscg_sort_ws_bytes(int64_t S, int64_t L);
int sscg_sort_u32_desc(const uint32_t* keys, int S, int L, uint32_t upper, uint32_t* out_keys, int32_t* out_index, void* ws,
                       size_t ws_bytes, void* stream);
/* Lovasz-softmax loss of the label head (opt-in; the reference has none): Berman, Triki, Blaschko (CVPR 2018).  x = logits
 * [N][H][W][C] (C <= 64), labels [N][OH][OW]; p = softmax over C of the logits resized to [OH][OW] (bilinear, align_corners=True, the
 * arithmetic of sscg_upsample_bilinear_fwd; OH == H && OW == W: the logits themselves, the flat form).  A pixel is COUNTED when its
 * label lies in [0, C).  A SEGMENT is the whole call (per_image == 0) or one sample.  For a segment s and a class c:
 *     f_i = [y_i == c]   e_i = |f_i - p_i,c| in fp32   G = sum_i f_i   over the V counted pixels i of the segment;
 *     the pixels ordered by e descending, ties by ascending pixel index; for rank j = 1 .. V: F_j = the foreground pixels among the
 *     first j, I_j = G - F_j, U_j = G + j - F_j, J_j = 1 - I_j / U_j, J_0 = 0, g_j = J_j - J_{j-1};   loss_{s,c} = sum_j e_(j) g_j.
 *   g_j is formed in closed form from exact integers in fp64: 1 / U_j at a foreground pixel, I_j / (U_j (U_j - 1)) at a background
 *   pixel, 1 / (G + 1) at a background pixel of rank 1 (which covers an absent class: G = 0, J_1 = 1).
 *   The segment's loss is the mean of loss_{s,c} over the classes that take part: never a class of skip_mask (bit c set: class c is
 *   skipped); with classes_all == 0 ("present") only classes with G > 0 - a segment with none gives 0 - with classes_all == 1 every
 *   class that is not skipped.  The loss is the mean over the segments; with per_image only samples with a counted pixel enter it,
 *   with none the loss is 0.  Ignored pixels take no rank, shift no rank, and get gradient 0.
 * sscg_lovasz_fwd: keys [segments][C][pixels of a segment] uint32 (N * C * OH * OW words): bits(e) + 1 for a counted pixel, 0 for an
 *   ignored one; loss: the scalar; per_class (fp32 [C], nullable): per class the mean of loss_{s,c} over the live segments in which
 *   the class took part; coef fp32 [N][OH][OW][C]: d loss / d p with g held constant, (f ? -1 : +1) * g_rank / (classes of the segment
 *   * live segments), exactly 0 at ignored pixels and at classes that take no part - the layout and the meaning of the dy_soft operand
 *   of sscg_upsample_head_bwd[_d|_h|_b] and of dy in sscg_softmax_bwd, which are the loss's backward: no stencil of its own.  Every
 *   element of keys and coef is written.  The key pass (one thread per output pixel; G and V through LDS bins and integer atomics),
 *   sscg_sort_u32_desc, a multi-block integer scan of the foreground flags in sorted order, one pass that forms g_j, adds e_(j) g_j
 *   into fixed-order fp64 block records and scatters the coefficients, a one-block finish.  No float atomics; neither the resized
 *   logits nor the probabilities reach memory; the same bits from call to call.  ws: sscg_lovasz_workspace bytes, 8-byte aligned -
 *   the sorted keys, their pixels and the sort's two planes (4 * N * C * OH * OW bytes each) and the tables.
 * sscg_lovasz_scale_add: out[i] = (dy_soft ? dy_soft[i] : 0) + *g * coef[i], n elements: the upstream gradient of the softmax map
 *   the backward entries receive (g: the loss's upstream scalar on the device; out may be dy_soft).
 * Errors before any HIP call: SSCG_ERR_BAD_ARG (null tensors, C outside 1..64, non-positive sizes, flags outside {0, 1}, a skip bit
 * at or above C, classes_all with every class skipped), SSCG_ERR_UNSUPPORTED (N * C * OH * OW >= 2^31, N*H*W >= 2^31; the query
 * then returns 0), SSCG_ERR_WORKSPACE.  (Additions: no existing entry changes meaning, so SSCG_ABI_VERSION stays 18.) */
size_t sscg_lovasz_workspace(int N, int OH, int OW, int C, int per_image);
int sscg_lovasz_fwd(const float* x, const int64_t* labels, int N, int H, int W, int C, int OH, int OW, int classes_all, int per_image,
                    uint64_t skip_mask, uint32_t* keys, float* coef, float* loss, float* per_class, void* ws, size_t ws_bytes,
                    void* stream);
int sscg_lovasz_scale_add(const float* coef, const float* g, const float* dy_soft, float* out, int64_t n, void* stream);
/* ------------------------------------------------------------------ inference heads (ABI v18): one launch from a generator's output
 * to what its consumer keeps.  Forward only; never launched by the training step.
 *
 * sscg_predict_head: label maps from the segmentation generator's low-resolution logits x [N][H][W][C] (C <= 64) - the per-epoch
 * evaluation (model.py:555-574: interp -> Softmax2d -> .max(1)[1] -> runningScore._fast_hist), validation.py:97-120 and
 * testing.py:43 (softmax -> argmax on the net's own output).  Per output pixel: the bilinear resize to [OH][OW] with
 * align_corners=True (the arithmetic of sscg_upsample_bilinear_fwd), the softmax over C (sscg_softmax_fwd's), the first maximum
 * (sscg_argmax_onehot's rule) - the same expressions in the same order, so every output equals the unfused chain's bit for bit; the
 * resized logits and the probabilities never reach memory.  OH == H && OW == W is the identity resize: no interpolation arithmetic.
 *   index      (nullable) int64 [N][OH][OW]: what sscg_argmax_onehot writes;
 *   label_u8   (nullable) uint8 [N][OH][OW]: the same class ids as bytes (the paletted PNGs of the drivers);
 *   label_true / hist (nullable together) int64 [N][OH][OW] / int64 [C][C]: hist[C*t + p] += 1 under sscg_confusion_hist's rules
 *              (t outside [0, C) ignored; accumulated into; integer atomics, exact).
 * At least one of index / label_u8 / hist is required.
 *
 * sscg_image_head: the image generator's output x [N][H][W][C] (C <= 4) as validation.py:108-114 consumes it:
 *   y_nhwc (nullable) fp32 [N][OH][OW][C] = tanh(resize(x)) - sscg_upsample_bilinear_fwd then sscg_act_fwd(SSCG_ACT_TANH), bit for
 *          bit: the tensor validation.py feeds back into Gsi;
 *   rgb_u8 (nullable) uint8 [N][OH][OW][C] = uint8(clamp((t * 0.5f + 0.5f) * 255.f + 0.5f, 0, 255)) with t = y_nhwc's value and every
 *          operation rounded to fp32 on its own: un-normalise (validation.py) + torchvision's save_image (x * 255 + 0.5, clamp,
 *          truncate), the bytes the host wrote from the fp32 tensor.
 * At least one of the two is required. */
int sscg_predict_head(const float* x, int N, int H, int W, int C, int OH, int OW, int64_t* index, uint8_t* label_u8,
                      const int64_t* label_true, int64_t* hist, void* stream);
int sscg_image_head(const float* x, int N, int H, int W, int C, int OH, int OW, float* y_nhwc, uint8_t* rgb_u8, void* stream);
/* ------------------------------------------------------------------ multi-scale / mirrored inference: several views of one batch
 * (the network run on resized and / or horizontally mirrored copies of the images) fused into one label map, the way DeepLab-v2 nets
 * are conventionally evaluated.  The reference evaluates one view only, so there is no call site to name; opt-in (`--tta`), forward
 * only, never launched by the training step.  (An addition: no existing entry changes meaning, so SSCG_ABI_VERSION stays 18.)
 *
 * sscg_predict_head_ms: xs / Hs / Ws are HOST arrays of length S (1 <= S <= 8), read during the call and copied into the kernel's
 * arguments (no pointer table on the device, no host sync): xs[s] = device pointer to view s's logits [N][Hs[s]][Ws[s]][C] fp32,
 * C <= 64.  Bit s of flip_mask: view s was computed from the horizontally mirrored image, its map is in mirrored coordinates.
 * Per output pixel (n, oy, ox), for s = 0 .. S-1 in that order: the source column ox_s = flip ? OW-1-ox : ox; the bilinear resize of
 * view s at (oy, ox_s) with align_corners=True (sscg_upsample_bilinear_fwd's arithmetic; Hs[s] == OH && Ws[s] == OW is the identity
 * resize, no interpolation arithmetic); the softmax over C (sscg_softmax_fwd's); acc[c] = s == 0 ? p[c] : acc[c] + p[c], the
 * probability rounded to fp32 before the add.  Then the first maximum of acc[] (sscg_argmax_onehot's rule).  No division by S.
 * Every output equals the separate passes' bit for bit - per view sscg_upsample_bilinear_fwd, a mirror of the W axis where flagged,
 * sscg_softmax_fwd, an fp32 add into the accumulator; then sscg_argmax_onehot's index and sscg_confusion_hist - and with S = 1,
 * flip_mask = 0 it equals sscg_predict_head's.  Neither the resized logits nor a view's probabilities reach memory.
 *   prob_sum   (nullable) fp32 [N][OH][OW][C]: the SUM of the views' probabilities;
 *   index / label_u8 / label_true + hist: exactly as in sscg_predict_head (hist accumulated into, t outside [0, C) ignored).
 * At least one output is required.  Errors before any HIP call: SSCG_ERR_BAD_ARG (null xs / Hs / Ws or a null xs[s]; S outside 1..8;
 * flip bits at or above S; non-positive sizes; C outside 1..64; no output; label_true without hist or the reverse),
 * SSCG_ERR_UNSUPPORTED (N*OH*OW, or N*OH*OW*C with prob_sum, >= 2^31).
 *
 * sscg_resize_flip: the network input of one view from the batch, x [N][H][W][C] -> y [N][OH][OW][C]: sscg_upsample_bilinear_fwd's
 * arithmetic (bilinear, align_corners=True, no antialiasing: a minifying resize samples) with the output columns mirrored when flip
 * != 0 - y[n][oy][ox] = resized[n][oy][OW-1-ox], bit for bit sscg_upsample_bilinear_fwd followed by a flip of the W axis.
 * OH == H && OW == W with flip is a pure mirror copy. */
int sscg_predict_head_ms(const float* const* xs, const int* Hs, const int* Ws, int S, uint32_t flip_mask, int N, int C, int OH, int OW,
                         float* prob_sum, int64_t* index, uint8_t* label_u8, const int64_t* label_true, int64_t* hist, void* stream);
int sscg_resize_flip(const float* x, float* y, int N, int H, int W, int C, int OH, int OW, int flip, void* stream);
/* ------------------------------------------------------------------ sliding-window inference: the network run on overlapping windows
 * of its training size over a larger image, the windows' probabilities blended with a separable importance map (nnU-Net / MONAI
 * sliding-window inference, mmseg mode='slide').  The reference resizes every image to the crop, so there is no call site to name;
 * opt-in (`--sliding`), forward only, never launched by the training step.  (Additions: no existing entry changes meaning, so
 * SSCG_ABI_VERSION stays 18.)
 *
 * Geometry, per axis (y: image rows OH, window rows wh, stride sy, ky windows; x alike): window i sits at pos_i = min(i * s, L - w),
 * the last one flush with the edge; (k - 1) * s >= L - w is required, so the windows cover the axis.  Window index
 * ((n * ky + iy) * kx + ix) * F + f with F = flip ? 2 : 1; f = 1 is the horizontally mirrored twin of f = 0.
 *
 * sscg_window_gather: x [N][H][W][C] fp32 -> y [(N ky kx F)][wh][ww][C], y[widx][ly][lx] = x[n][pos_iy + ly][pos_ix + (f ? ww-1-lx : lx)]:
 * a pure copy, one launch - the network input of every window.  Errors before any HIP call: SSCG_ERR_BAD_ARG (null pointers,
 * non-positive sizes, wh > H, ww > W, (ky-1)*sy < H - wh, (kx-1)*sx < W - ww), SSCG_ERR_UNSUPPORTED (2^31 windows or more).
 *
 * sscg_predict_head_sw: x holds the windows' low-resolution logits [(N ky kx F)][h][w][C] fp32 (C <= 64) in the gather's order; wy[wh],
 * wx[ww] are the window's weight tables, ry[OH], rx[OW] the reciprocals of the summed weights per row / column (the blend is separable,
 * so ry[oy] * rx[ox] normalises pixel (oy, ox); with flip, ry carries the factor 0.5) - all four fp32 in device memory.
 * Per output pixel (n, oy, ox): the windows that cover it, found by arithmetic on (oy, sy, ky, OH - wh) and (ox, sx, kx, OW - ww), in
 * ascending (iy, ix) order, f = 0 before f = 1; with (ly, lx) = (oy - pos_iy, ox - pos_ix): the bilinear resize of the window's map to
 * [wh][ww] at (ly, f ? ww-1-lx : lx) with align_corners=True (sscg_upsample_bilinear_fwd's arithmetic; h == wh && w == ww is the
 * identity resize), the softmax over C (sscg_softmax_fwd's), then t = p[c], g = wy[ly] * wx[lx], acc[c] = first ? g * t : acc[c] + g * t,
 * every product rounded to fp32 before the add.  Then the first maximum of acc[] (sscg_argmax_onehot's rule), unnormalised.
 * Every output equals the separate passes' bit for bit - per window sscg_upsample_bilinear_fwd, sscg_softmax_fwd, a mirror of the W
 * axis for f = 1, an fp32 multiply by the outer product of wy and wx, an fp32 add into the window's place of a zeroed accumulator; then
 * sscg_argmax_onehot's index, sscg_confusion_hist and an fp32 multiply by the outer product of ry and rx.  No window's resized logits
 * or probabilities reach memory.
 *   prob       (nullable) fp32 [N][OH][OW][C]: acc[c] * (ry[oy] * rx[ox]), two roundings - the blended probabilities;
 *   index / label_u8 / label_true + hist: exactly as in sscg_predict_head (hist accumulated into, t outside [0, C) ignored).
 * At least one output is required.  Errors before any HIP call: SSCG_ERR_BAD_ARG (a null x or table; non-positive sizes or strides;
 * C outside 1..64; wh > OH, ww > OW, (ky-1)*sy < OH - wh, (kx-1)*sx < OW - ww; no output; label_true without hist or the reverse),
 * SSCG_ERR_UNSUPPORTED (N*OH*OW, or N*OH*OW*C with prob, or the number of windows >= 2^31). */
int sscg_window_gather(const float* x, float* y, int N, int H, int W, int C, int wh, int ww, int sy, int sx, int ky, int kx, int flip,
                       void* stream);
int sscg_predict_head_sw(const float* x, int N, int h, int w, int C, int wh, int ww, int sy, int sx, int ky, int kx, int flip, int OH,
                         int OW, const float* wy, const float* wx, const float* ry, const float* rx, float* prob, int64_t* index,
                         uint8_t* label_u8, const int64_t* label_true, int64_t* hist, void* stream);
/* ------------------------------------------------------------------ windowed dense-CRF refinement of a predicted class map: the
 * mean-field update of the fully connected CRF that conventionally follows a DeepLab-v2 net, with the pairwise sum truncated to a
 * dilated (2r+1)^2 window.  The reference has no CRF, so there is no call site to name; opt-in (`--crf`), forward only, never launched
 * by the training step.  (An addition: no existing entry changes meaning, so SSCG_ABI_VERSION stays 18.)
 *
 * sscg_crf_head: x is, by `kind`,
 *   SSCG_CRF_LOGITS  fp32 [N][H][W][C] low-resolution logits, resized to [OH][OW] by sscg_upsample_bilinear_fwd's arithmetic
 *                    (OH == H && OW == W: the identity resize);
 *   SSCG_CRF_PROBS   fp32 [N][OH][OW][C] non-negative scores, e.g. prob_sum of sscg_predict_head_ms; H == OH && W == OW required.
 * img = the guide image, fp32 [N][OH][OW][IC], 1 <= IC <= 4, in whatever units theta_beta is given in; C <= 64.
 * Unary, per output pixel: LOGITS u_c = (z_c - m) - logf(s) with z the resized logits, m their maximum and s = sum_c expf(z_c - m);
 * PROBS u_c = logf(fmaxf(x_c, FLT_MIN)).  Q0 = softmax_c(u) by sscg_softmax_fwd's operations.
 * Pairwise weight between pixel i and its tap at offset (dy * d, dx * d), dy, dx in [-r, r], centre excluded:
 *   k = w_bilateral * expf(-(d2 * ia + c2 * ib)) + w_spatial * expf(-d2 * ig),  d2 = (dy d)^2 + (dx d)^2,
 *   c2 = sum over the IC channels of (img_i - img_j)^2,  ia = 1 / (2 theta_alpha^2), ib = 1 / (2 theta_beta^2), ig = 1 / (2 theta_gamma^2),
 * each formed in double and rounded to fp32 once.  A tap outside the map is skipped; nothing is renormalised.
 * One mean-field step (Potts compatibility): msg_c(i) = sum over the taps of k * Q_c(j), the taps in row-major (dy, dx) order into one
 * fp32 accumulator per class; Q'(i) = softmax_c(u_c(i) + msg_c(i)).  After `iterations` steps the label is the first maximum of Q
 * (sscg_argmax_onehot's rule).  The order is part of the contract: the result depends neither on the workgroup tiling nor on N.
 *   q_out      (nullable) fp32 [N][OH][OW][C]: Q after the last step;
 *   index / label_u8 / label_true + hist: exactly as in sscg_predict_head (hist accumulated into, t outside [0, C) ignored).
 * At least one output is required.  ws: sscg_crf_workspace bytes (u and two Q buffers: three [N][OH][OW][C] fp32 maps; 0 when
 * iterations == 0), fully written before it is read.
 * iterations == 0: no CRF launch - LOGITS is sscg_predict_head itself, PROBS the first maximum of x (what sscg_predict_head_ms takes of
 * its sum); img and the parameters are checked but not used, q_out must be null.
 * Errors before any HIP call: SSCG_ERR_BAD_ARG (null x / img / p; unknown kind; non-positive sizes; C outside 1..64; IC outside 1..4;
 * radius outside 1..5; dilation < 1; iterations < 0; a weight that is negative or not finite; a theta that is not > 0, or so small that
 * 1 / (2 theta^2) is not a finite fp32 number; no output; q_out with iterations == 0; label_true without hist or the reverse; PROBS
 * with H != OH or W != OW), SSCG_ERR_UNSUPPORTED (radius * dilation > 16; N*OH*OW*C >= 2^31), SSCG_ERR_WORKSPACE. */
#define SSCG_CRF_LOGITS 0
#define SSCG_CRF_PROBS 1
typedef struct sscg_crf_params {
    int32_t radius, dilation, iterations;
    float w_bilateral, w_spatial, theta_alpha, theta_beta, theta_gamma;
} sscg_crf_params;
size_t sscg_crf_workspace(int N, int C, int OH, int OW, int iterations);
int sscg_crf_head(const float* x, int kind, int N, int H, int W, int C, int OH, int OW, const float* img, int IC,
                  const sscg_crf_params* p, float* q_out, int64_t* index, uint8_t* label_u8, const int64_t* label_true, int64_t* hist,
                  void* ws, size_t ws_bytes, void* stream);
/* ------------------------------------------------------------------ gated (relaxed dense) CRF loss of a softmax map: the regulariser
 * of Tang et al. (ECCV 2018) / Obukhov et al. (2019) - two nearby pixels of similar colour that disagree are penalised - with the
 * pairwise weight of sscg_crf_head.  The reference has no such term, so there is no call site to name; opt-in (`--unl_crf`), the
 * training-side counterpart of `--crf`.  (Additions: no existing entry changes meaning, so SSCG_ABI_VERSION stays 18.)
 *
 * sscg_crf_loss_fwd: p fp32 [N][OH][OW][C], the channels-last softmax map (rows need not sum to exactly 1), 1 <= C <= 64; img the guide
 * image fp32 [N][OH][OW][IC], 1 <= IC <= 4; prm as for sscg_crf_head, its `iterations` member ignored.  k(i, j) is sscg_crf_head's
 * pairwise weight exactly - the formula, the three 1 / (2 theta^2) constants formed in double and rounded to fp32 once, the same
 * operations - over the taps in row-major (dy, dx) order, centre excluded; a tap outside the map is skipped, nothing is renormalised.
 * Per pixel i:
 *   msg_c(i) = sum over the taps of k(i, j) * p_c(j): one fp32 accumulator per class, filled with fmaf in tap order - the bits of the
 *              message of a mean-field step of sscg_crf_head on Q = p;
 *   ksum(i)  = sum over the taps of k(i, j), in the same tap order with plain fp32 adds;
 *   e(i)     = ksum(i) - sum_c p_c(i) * msg_c(i): the product sum over c ascending with fmaf from 0, then one subtraction.
 * loss = (sum_i e(i)) / M, M = N * OH * OW: e(i) and ksum(i) widened to fp64, one record (sum e, sum ksum) per 16 x 16 tile in a fixed
 * order, the records summed in a fixed order by one block; no float atomics - the same bits from call to call, whatever ws held.
 *   loss  fp32 [1] = (float)(sums[0] / M);      sums fp64 [2] = (sum e, sum ksum);
 *   coef  (nullable: the value only) fp32 [N][OH][OW][C]: coef[i][c] = s * msg_c(i), s = (float)(-2.0 / (double)M), one fp32 multiply.
 *         It is d loss / d p_c(i) exactly: k(i, j) == k(j, i) bit for bit and the tap sets are symmetric, so the scatter half of the
 *         derivative equals the gather half.  No gradient reaches the guide image.
 * For rows that sum to 1, e(i) = sum over the taps of k(i, j) (1 - p(i) . p(j)) >= 0.  The VALUE of e cancels where the prediction is
 * already smooth (ksum and the product sum agree in their leading digits), so its absolute error is a few ulp of ksum, not of e; the
 * gradient is a plain sum of non-negative products and does not cancel.
 * ws: sscg_crf_loss_workspace(N, OH, OW) bytes (one record of two doubles per tile), fully written before it is read.
 * Errors before any HIP call: SSCG_ERR_BAD_ARG (null p / img / prm / loss / sums; non-positive sizes; C outside 1..64; IC outside 1..4;
 * radius outside 1..5; dilation < 1; a weight that is negative or not finite; a theta that is not > 0, or so small that 1 / (2 theta^2)
 * is not a finite fp32 number), SSCG_ERR_UNSUPPORTED (radius * dilation > 16; N*OH*OW*C >= 2^31), SSCG_ERR_WORKSPACE.
 * The backward of a node built on it is sscg_lovasz_scale_add(coef, g, NULL, out, n): out = g * coef. */
size_t sscg_crf_loss_workspace(int N, int OH, int OW);
int sscg_crf_loss_fwd(const float* p, int N, int OH, int OW, int C, const float* img, int IC, const sscg_crf_params* prm, float* loss,
                      double* sums, float* coef, void* ws, size_t ws_bytes, void* stream);
/* ------------------------------------------------------------------ contour scores of the evaluation: the counts behind the Boundary
 * IoU (Cheng et al., CVPR 2021) and the trimap mIoU of the DeepLab papers, beside the confusion matrix of runningScore (utils.py:357-412,
 * the call site whose evaluation this extends; the reference has neither score).  Opt-in (`--boundary`), forward only, never launched by
 * the training step.  (An addition: no existing entry changes meaning, so SSCG_ABI_VERSION stays 18.)
 *
 * sscg_boundary_counts: label_true int64 [N][H][W] (any values), label_pred uint8 [N][H][W], 1 <= C <= 64, width 1 <= d <= 32 in
 * pixels of the chessboard metric (the published Boundary IoU erodes d times with a 3x3 element).  With
 *   t(p) = label_true(p) inside [0, C), else VOID;  r(p) = label_pred(p) - a byte >= C takes part in the comparisons, is counted in
 *          no bin and indexes no memory;
 *   Win_d(p) = the (2d+1) x (2d+1) window around p CLIPPED to the image;
 *   in_t(p) = some q in Win_d(p) has t(q) != t(p) (VOID is a label like any other);  in_r(p) = the same on r;
 *   out(p) = the unclipped window leaves the image: y < d || y >= H - d || x < d || x >= W - d;
 *   valid(p) = t(p) != VOID;  E_t = valid & (in_t | out);  E_r = valid & (in_r | out);  band = valid & in_t
 * (the image border is a contour, as in the published code, which pads with zeros before eroding; alone it puts no pixel into the
 * trimap band), counts is int64 [3 C + C C] on the device, ACCUMULATED into:
 *   counts[c]               bt[c]     += #{p : E_t(p), t(p) = c}
 *   counts[C + c]           bp[c]     += #{p : E_r(p), r(p) = c}
 *   counts[2 C + c]         bi[c]     += #{p : E_t(p) & E_r(p), t(p) = r(p) = c}
 *   counts[3 C + C c + k]   tri[c][k] += #{p : band(p), t(p) = c, r(p) = k}
 * Boundary IoU of class c = bi / (bt + bp - bi); the trimap IoU is the confusion-matrix IoU of tri.  One launch; per-workgroup LDS
 * bins, then 64-bit integer atomics: exact and independent of scheduling, as sscg_confusion_hist.  The work per pixel grows with d,
 * not d^2 (a window is uniform iff each of its clipped row segments is uniform with the same value).
 * Errors before any HIP call: SSCG_ERR_BAD_ARG (null tensors, non-positive sizes, C outside 1..64, d outside 1..32),
 * SSCG_ERR_UNSUPPORTED (N*H*W >= 2^31). */
int sscg_boundary_counts(const int64_t* label_true, const uint8_t* label_pred, int N, int H, int W, int C, int d, int64_t* counts,
                         void* stream);
/* ------------------------------------------------------------------ surface distances of the evaluation: the per-case records behind
 * the Hausdorff distance (HD), its percentile (HD95), the average symmetric surface distance (ASSD) and the normalised surface Dice (NSD)
 * of a ground-truth / predicted pair of label maps - the second metric of the ACDC challenge beside Dice, which no width-limited contour
 * band can give (the reference has none of them).  Opt-in (`--surface`), forward only, never launched by the training step.  (An
 * addition: no existing entry changes meaning, so SSCG_ABI_VERSION stays 18.)
 *
 * sscg_surface_stats: label_true int64 [N][H][W] (any values), label_pred uint8 [N][H][W], 1 <= C <= 64, unit pixel spacing.  With
 *   T_c = {label_true == c}, P_c = {label_pred == c} (a true label outside [0, C) and a predicted byte >= C belong to no class);
 *   S(M) = the pixels of M with a 4-neighbour that is not in M or lies outside the image (M minus its erosion by the cross, border
 *          value 0: the edge definition of MONAI and medpy);
 *   direction 0 (T->P): D2 = { min over q in S(P_c) of |r - q|^2 : r in S(T_c) };  direction 1 (P->T) the other way round - integers;
 * per direction dir, sample n and class c, OVERWRITTEN (nothing is accumulated, nothing depends on what ws, stats or sums held):
 *   stats[dir][n][c][0]  cnt     number of source surface pixels (reported whenever the source surface exists)
 *   stats[dir][n][c][1]  within  number with d^2 <= tol2 (tol2 = floor(tol^2): for an integer d^2 exactly d <= tol)
 *   stats[dir][n][c][2]  max2    the largest d^2
 *   stats[dir][n][c][3]  v_lo    the d^2 of ascending zero-based rank lo = ((cnt - 1) * pct) / 100 (integer arithmetic)
 *   stats[dir][n][c][4]  v_hi    the d^2 of rank hi = min(lo + 1, cnt - 1)
 *   sums[dir][n][c]      sum     the sum of sqrt(d^2) in fp64
 * When the source or the target surface is empty: within = 0, max2 = v_lo = v_hi = -1, sum = 0.  From these the host forms
 *   hd = sqrt(max of the two max2),  hd95 = max over the directions of a + (b - a) * (((cnt - 1) * pct) % 100) / 100 with a = sqrt(v_lo),
 *   b = sqrt(v_hi) (numpy's linear percentile, per direction),  assd = (sum0 + sum1) / (cnt0 + cnt1),  nsd = (within0 + within1) /
 *   (cnt0 + cnt1) (utils.surface_scores).
 * The distances are exact at any separation (a column pass and a row pass of the squared Euclidean distance transform, no window);
 * cnt / within / max2 are integer atomics, v_lo / v_hi an exact radix select over three ten-bit digits, sum is added from per-row fp64
 * records in a fixed order: the integers are independent of scheduling and the sums reproduce bit for bit.  Everything stays on the
 * stream.  ws: sscg_surface_workspace(N, H, W, C) bytes (0 for sizes sscg_surface_stats refuses), 256-byte aligned - about
 * 10 + 4 min(C, 8) bytes per pixel of the batch plus 2 N C (4112 + 8 H) bytes.
 * Errors before any HIP call: SSCG_ERR_BAD_ARG (a null pointer, non-positive sizes, C outside 1..64, tol2 < 0, pct outside 1..100),
 * SSCG_ERR_UNSUPPORTED (N*H*W >= 2^31; (H-1)^2 + (W-1)^2 >= 2^30, the largest d^2 the selection's digits cover), SSCG_ERR_WORKSPACE. */
size_t sscg_surface_workspace(int N, int H, int W, int C);
int sscg_surface_stats(const int64_t* label_true, const uint8_t* label_pred, int N, int H, int W, int C, int tol2, int pct,
                       int64_t* stats, double* sums, void* ws, size_t ws_bytes, void* stream);
/* ------------------------------------------------------------------ connected-component filtering of predicted label maps: the
 * post-processing of the ACDC / nnU-Net style pipelines - label the connected components of every predicted class, keep the largest one
 * per sample and / or the ones of at least min_area pixels, relabel the rest - without which one stray speckle far from its structure
 * sets the Hausdorff distance of --surface (the reference has no such step: its validation scores the argmax as it is).  Opt-in
 * (`--components`), forward only, never launched by the training step.  (An addition: no existing entry changes meaning, so
 * SSCG_ABI_VERSION stays 18.)
 *
 * sscg_components_filter: label_pred uint8 [N][H][W] (the map the heads write), 1 <= C <= 64, conn = 4 or 8, largest = 0 or 1,
 * min_area >= 0, 0 <= fill < C; bit c of exempt_mask exempts class c, the fill class is always exempt.
 *   COMPONENT of class c in sample n: a maximal conn-connected set of pixels of sample n with label_pred == c.  Connectivity never
 *     crosses a sample or the image border.  A byte >= C belongs to no component, joins nothing and is copied through unchanged.
 *   ANCHOR of a component: its smallest row-major pixel index within the sample;  AREA: its pixel count.
 *   A component of a non-exempt class c is KEPT iff area >= min_area and, if largest, it is the component of (n, c) with the largest
 *     area, ties going to the smallest anchor.  Components of exempt classes are always kept.
 *   label_out[p] = label_pred[p] on kept components and on bytes >= C, fill otherwise; every byte is written; label_out == label_pred
 *     (in place) is allowed.
 *   hist (non-null only together with label_true int64 [N][H][W]): int64 [C][C], ACCUMULATED, hist[t][label_out] under exactly
 *     sscg_confusion_hist's rules (a true label outside [0, C) and a byte >= C are counted nowhere) - equal to calling that entry on
 *     label_out.
 *   stats (nullable): int64 [N][C][4], OVERWRITTEN: the number of components, the number of kept components, the pixels of the class
 *     before filtering, the pixels after (for the fill class "after" includes what was relabelled into it).
 * Nothing depends on what ws, label_out or stats held, or on scheduling: all results are integers formed by order-free atomics and
 * reproduce bit for bit.  A block-based union-find (csrc/components.hip): one int32 parent and one int32 area per pixel of the batch,
 * unions by minimum index inside 32x32 tiles in LDS, then across the tile seams by global atomicMin, so that the root of a component
 * is its anchor; one 64-bit key (area << 32 | ~anchor) per (sample, class) selects the largest.  Five launches on the stream, no host
 * synchronisation, no copy.  ws: sscg_components_workspace(N, H, W, C) bytes (0 for sizes sscg_components_filter refuses), 256-byte
 * aligned - 8 bytes per pixel of the batch plus 8 N C.
 * Errors before any HIP call: SSCG_ERR_BAD_ARG (label_pred / label_out / ws null, non-positive sizes, C outside 1..64, conn not 4 or 8,
 * largest not 0 or 1, min_area < 0, fill outside [0, C), hist without label_true, exempt_mask bits at or above C),
 * SSCG_ERR_UNSUPPORTED (N*H*W >= 2^31), SSCG_ERR_WORKSPACE. */
size_t sscg_components_workspace(int N, int H, int W, int C);
int sscg_components_filter(const uint8_t* label_pred, const int64_t* label_true /*nullable*/, int N, int H, int W, int C,
                           int conn, int largest, int min_area, int fill, uint64_t exempt_mask,
                           uint8_t* label_out, int64_t* hist /*nullable, accumulated*/, int64_t* stats /*nullable, overwritten*/,
                           void* ws, size_t ws_bytes, void* stream);
/* ------------------------------------------------------------------ calibration scores of the evaluation: the counts behind the
 * expected / maximum calibration error (ECE / MCE) over a reliability diagram, the per-class confidence gap, the negative log-likelihood
 * (NLL), the Brier score and the NLL-optimal temperature of the probabilities the heads above take their labels from - the softmax
 * output --unl_pseudo_thresh, --ohem_thresh, --crf and --tta trust as a probability (the reference scores label maps only,
 * utils.py:357-412).  Opt-in (`--calibration`), forward only, never launched by the training step; the N x C x OH x OW probability map
 * never reaches memory.  (An addition: no existing entry changes meaning, so SSCG_ABI_VERSION stays 18.)
 *
 * sscg_calib_stats: x is, by `kind`,
 *   0  fp32 [N][H][W][C] logits, C <= 64, resized to [OH][OW] by sscg_upsample_bilinear_fwd's arithmetic (OH == H && OW == W: the
 *      identity resize, no interpolation arithmetic) - what sscg_predict_head takes; `scale` is not used;
 *   1  fp32 [N][OH][OW][C] non-negative scores, H == OH && W == OW, NT == 1 and inv_temps[0] == 1.f required: the probability is
 *      x[c] * scale, one fp32 multiply and no softmax (prob_sum of sscg_predict_head_ms with scale = 1.f / S; q_out of sscg_crf_head
 *      with scale = 1.f); scale finite and >= 0.
 * inv_temps is a HOST array of NT floats (1 <= NT <= 8, each finite and > 0), read during the call and copied into the kernel's
 * arguments (no table on the device, no host sync).  B = the number of equal-width confidence bins, 2 <= B <= 32.  label_true is int64
 * [N][OH][OW]; a pixel is COUNTED when its label is in [0, C) (sscg_confusion_hist's rule), every other pixel adds to nothing.
 * Per counted output pixel and per temperature t = 0 .. NT-1, in that order:
 *   v[c] = z[c] * inv_temps[t] with z the resized logits - one fp32 multiply per class AFTER the resize, rounded on its own (it never
 *          contracts into the softmax), so inv_temps[t] == 1.f gives sscg_predict_head's bits; p[c] = sscg_softmax_fwd's value of v;
 *   pred = the first maximum of p (sscg_argmax_onehot's rule), conf = p[pred], hit = (pred == label);
 *   b    = min(B - 1, (int)(conf * (float)B)): one fp32 multiply and a truncation, so conf = k / B exactly opens bin k;
 *   q    = (int64)(conf * 16777216.f): the confidence in Q24 (the multiply is exact, the conversion truncates) - confidence sums are
 *          integers, independent of the order and identical from call to call;
 *   bins[t][b] += (1, hit, q)    int64 [NT][B][3]          cls[t][pred] += (1, hit, q)    int64 [NT][C][3]
 *   sums[t]    += (-log(max((double)p[label], 0x1p-126)), sum_c ((double)p[c] - [c == label])^2)    double [NT][2], in fp64 from the
 *          fp32 probabilities: a true class whose probability underflowed to 0 costs 126 ln 2, not infinity.
 * All three outputs are ACCUMULATED into: a caller zeroes them once per evaluation, as it does hist.  From them the host forms
 *   ECE = sum_b n_b / n |hit_b / n_b - qsum_b / (2^24 n_b)|, MCE = the largest such gap, NLL = sums[.][0] / n, Brier = sums[.][1] / n,
 *   the gap conf_c - acc_c of every predicted class and the temperature that minimises the NLL (utils.calibration_scores).
 * Two launches: one thread per output pixel, grid-stride over at most 512 workgroups of 256 threads (a thread owns
 * ceil(N OH OW / 131072) pixels); the integers through 64-bit per-workgroup LDS bins (256 pixels of confidence 1 carry a Q24 sum past 32
 * bits) and one 64-bit integer atomic per value of a bin that was hit; the fp64 sums through one record per workgroup in ws, reduced in
 * a fixed order by a one-block finish that adds the call's total to sums - no float atomics: the same call twice gives the same bits.
 * ws: sscg_calib_workspace(N, OH, OW, NT) = min(ceil(N OH OW / 256), 512) * NT * 2 * 8 bytes (0 for sizes sscg_calib_stats refuses),
 * 8-byte aligned, fully written before it is read.
 * Errors before any HIP call: SSCG_ERR_BAD_ARG (a null pointer; non-positive sizes; C outside 1..64; B outside 2..32; NT outside 1..8;
 * an inv_temps[t] that is not finite and > 0; kind outside {0, 1}; kind 1 with H != OH, W != OW, NT != 1, inv_temps[0] != 1 or a scale
 * that is negative or not finite), SSCG_ERR_UNSUPPORTED (N*OH*OW or N*H*W >= 2^31), SSCG_ERR_WORKSPACE. */
size_t sscg_calib_workspace(int N, int OH, int OW, int NT);
int sscg_calib_stats(const float* x, int kind, float scale, int N, int H, int W, int C, int OH, int OW,
                     const int64_t* label_true, const float* inv_temps, int NT, int B,
                     int64_t* bins, int64_t* cls, double* sums, void* ws, size_t ws_bytes, void* stream);
/* ------------------------------------------------------------------ per-epoch image panels: the image grids the reference sends to
 * TensorBoard at the end of every epoch (model.py:576-638; supervised_model: model.py:164-186), without the host round trip of
 * full-resolution maps, the per-pixel Python loop of utils.PIL_to_tensor (utils.py:59-94) and make_grid on the host.  Forward only;
 * never launched by the training step.  (An addition: no existing entry changes meaning, so SSCG_ABI_VERSION stays 18.)
 *
 * sscg_panel_labels (model.py:580-585, :593-597: interp -> Softmax2d -> .max(1)[1] -> make_one_hot): x = low-resolution logits
 * [N][H][W][C], C <= 64.  Per output pixel the resize, softmax and first maximum of sscg_predict_head - the same functions, so every
 * id equals that head's label_u8 bit for bit; OH == H && OW == W is the identity resize.
 *   label_u8 (required) uint8 [N][OH][OW]: the class ids;
 *   onehot   (nullable) fp32 [N][OH][OW][C]: 1.0f at the id, 0.0f elsewhere, every element written - what sscg_label_onehot makes of
 *            the same ids: the input of the image generator (model.py:586).
 * Neither the resized logits, the probabilities nor an int64 map reach memory.
 *
 * A panel is one of three kinds of source, each with a pre-normalisation value v per pixel and channel:
 *   SSCG_PANEL_IMAGE   src fp32 [pixels][C], C in {1, 3}: v = x * scale + shift, a multiply then an add, each rounded to fp32 on its
 *                      own - the un-normalise of model.py:603-615 (scale = std, shift = mean);
 *   SSCG_PANEL_COLOUR  src uint8 ids [pixels] (C = 1): v_c = (float)palette[3 * id + c], palette uint8 [256][3] on the device -
 *                      utils.colorize_mask + utils.PIL_to_tensor (model.py:622-625, :629-632);
 *   SSCG_PANEL_GREY    src int64 [pixels] (C = 1): v = (float)id - display_tensor_gt[i] = val_gt[i] (model.py:627).
 *
 * sscg_panel_range: range[0] / range[1] (device) = the minimum / maximum of v over all pixels and channels, what make_grid(normalize=
 * True) takes over the whole batch (model.py:634-638).  Exact and independent of order; inputs are finite by contract.  The result
 * stays on the device.  ws: sscg_panel_range_workspace bytes (one pair per workgroup; 0 for small panels).
 *
 * sscg_panel_grid: torchvision.utils.make_grid(t, nrow, padding, normalize=True) followed by the image writer's float -> byte
 * conversion, in one launch.  src [N][H][W](C) as above; with xmaps = min(nrow, N) and ymaps = ceil(N / xmaps), grid is uint8
 * [3][ymaps * (H + padding) + padding][xmaps * (W + padding) + padding], CHW; tile k starts at row (k / xmaps) * (H + padding) +
 * padding, column (k % xmaps) * (W + padding) + padding.  N == 1 is torchvision's special case: the image itself, [3][H][W], no
 * border.  A one-channel source fills all three channels.  Every byte outside a tile is 0, unused cells included; every byte of grid
 * is written.  Inside a tile, with lo = range[0], hi = range[1]:
 *     d = (float)max((double)hi - (double)lo, 1e-5);  u = (v - lo) / d;  byte = (uint8_t)min(max(u * 255.f, 0.f), 255.f)
 * every operation rounded to fp32 on its own, the division IEEE, the conversion truncating.
 *
 * Errors before any HIP call: SSCG_ERR_BAD_ARG (null tensors, an unknown kind, C outside the kind's set, non-positive sizes or nrow,
 * negative padding, COLOUR without a palette), SSCG_ERR_UNSUPPORTED (C > 64 in the labels head, an output of >= 2^31 elements),
 * SSCG_ERR_WORKSPACE. */
#define SSCG_PANEL_IMAGE 0
#define SSCG_PANEL_COLOUR 1
#define SSCG_PANEL_GREY 2
int sscg_panel_labels(const float* x, int N, int H, int W, int C, int OH, int OW, uint8_t* label_u8, float* onehot, void* stream);
size_t sscg_panel_range_workspace(int64_t pixels, int C);
int sscg_panel_range(const void* src, int kind, int64_t pixels, int C, float scale, float shift, const uint8_t* palette, float* range,
                     void* ws, size_t ws_bytes, void* stream);
int sscg_panel_grid(const void* src, int kind, int N, int H, int W, int C, float scale, float shift, const uint8_t* palette,
                    const float* range, int nrow, int padding, uint8_t* grid, void* stream);
/* nn.MSELoss against a constant target map of ones/zeros (LSGAN; model.py:445-446,452,521-528) */
int sscg_mse_const_fwd(const float* x, int64_t n, float target, float* loss, void* ws, size_t ws_bytes, void* stream);
int sscg_mse_const_bwd(const float* x, int64_t n, float target, const float* gscale, float w, float* dx, void* stream);
/* nn.MSELoss between two tensors (utils.perceptual_loss, utils.py:205-206): gradient to a, and to b when db != NULL */
int sscg_mse_fwd(const float* a, const float* b, int64_t n, float* loss, void* ws, size_t ws_bytes, void* stream);
int sscg_mse_bwd(const float* a, const float* b, int64_t n, const float* gscale, float w, float* da, float* db, void* stream);
/* nn.L1Loss (model.py:271; call :461) */
int sscg_l1_fwd(const float* a, const float* b, int64_t n, float* loss, void* ws, size_t ws_bytes, void* stream);
int sscg_l1_bwd(const float* a, const float* b, int64_t n, const float* gscale, float w, float* da, void* stream);
/* Structural similarity fused with that L1 term (`--ssim_weight`; the reference has no such term: its image terms are the plain L1 of
 * model.py:461 and the commented-out :453).  a (the prediction, gets the gradient) and b (the data) are fp32 [N][H][W][C], C <= 4.
 * Window: win x win, win odd in 3..11, separable, g[i] = exp(-(i - (win-1)/2)^2 / (2 sigma^2)) normalised to sum 1 in fp64 on the
 *   host, rounded to fp32 once.  "Valid": the map has H' = H - win + 1 by W' = W - win + 1 positions, no padding.
 * Per (n, c, p), with the window's weighted moments mu_a, mu_b, E[a^2], E[b^2], E[ab]:
 *     va = E[a^2] - mu_a^2    vb = E[b^2] - mu_b^2    cov = E[ab] - mu_a mu_b
 *     A1 = 2 mu_a mu_b + c1   A2 = 2 cov + c2         B1 = mu_a^2 + mu_b^2 + c1    B2 = va + vb + c2        S = A1 A2 / (B1 B2)
 *   ssim_loss = 1 - mean S over M = N C H' W' positions; per_sample (nullable) [N] = the mean S of a sample; l1 (nullable) = mean |a - b|
 *   over N C H W, taken in the same launch, every input pixel once.  c1 = (0.01 L)^2, c2 = (0.03 L)^2 for a data range L.
 * Gradient: with P1 = 2 mu_b (A2 - A1) / (B1 B2) - 2 mu_a S (1 / B1 - 1 / B2), P2 = -S / B2, P3 = 2 A1 / (B1 B2) per position and G^T
 *   the adjoint of the valid filter (a full correlation; border pixels receive fewer windows),
 *     d ssim_loss / d a(q) = -(1 / M) [ (G^T P1)(q) + 2 a(q) (G^T P2)(q) + b(q) (G^T P3)(q) ].
 * sscg_l1_ssim_fwd: one tiled stencil launch (16 x 16 positions per workgroup, the tile of a and b with its win-1 halo staged in LDS, a
 *   row pass and a column pass of the five moments) and a one-block finish; fp64 block records in a fixed order, no float atomics: the
 *   same call twice gives the same bits, whatever the workspace held.  coef (nullable; wanted with a gradient) receives P1, P2, P3 as
 *   [3][N][H'][W'][C] fp32.  ws: sscg_ssim_workspace(N, H, W, C, win) bytes, 8-byte aligned.
 * sscg_l1_ssim_bwd: one stencil launch that writes every element of
 *     da = (*g_ssim) w_ssim d ssim_loss / d a + (*g_l1) w_l1 sign(a - b) / (N C H W);
 *   a NULL g_l1 or g_ssim drops its term (both NULL: refused).  With g_ssim == NULL coef is not read and da has sscg_l1_bwd's bits.
 * Errors before any HIP call: SSCG_ERR_BAD_ARG (null tensors, win even or outside 3..11, sigma <= 0, H < win or W < win, c1 or c2 < 0,
 * non-positive sizes), SSCG_ERR_UNSUPPORTED (C outside 1..4, N H W C >= 2^31), SSCG_ERR_WORKSPACE; sscg_ssim_workspace returns 0 for
 * sizes the entries refuse.  (Additions: no existing entry changes meaning, so SSCG_ABI_VERSION stays 18.) */
size_t sscg_ssim_workspace(int N, int H, int W, int C, int win);
int sscg_l1_ssim_fwd(const float* a, const float* b, int N, int H, int W, int C, int win, float sigma, float c1, float c2, float* l1,
                     float* ssim_loss, float* per_sample, float* coef, void* ws, size_t ws_bytes, void* stream);
int sscg_l1_ssim_bwd(const float* a, const float* b, const float* coef, int N, int H, int W, int C, int win, float sigma,
                     const float* g_l1, float w_l1, const float* g_ssim, float w_ssim, float* da, void* stream);
/* out = sum_i w[i] * (*terms[i]) for up to 16 device scalars (gen_loss / discriminator_loss, model.py:464-468,538) */
int sscg_weighted_sum(const float* const* terms, const float* w, int n, float* out, void* stream);

/* ------------------------------------------------------------------ optimiser (K14)
 * torch.optim.Adam (model.py:286-287; steps :474,:542): eps 1e-8, no amsgrad.  sscg_adam_step is that optimiser and nothing else;
 * gradient-norm clipping, weight decay and an EMA of the parameters are the opt-in sscg_grad_norm / sscg_adam_step_ex below.
 * One launch over a flat arena; grad is multiplied by grad_scale first (1/world_size under data parallel).
 * `shadow` (nullable): an operand copy of the parameter arena rewritten in the same pass - the copy the convolutions read (the
 * fp32 arena stays the master copy): shadow_dtype SSCG_BF16 = a bfloat16 arena of n elements; SSCG_BF16X3 = the three planes
 * of the split contraction (sscg_split3), n elements apart. */
int sscg_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow, int shadow_dtype, int64_t n,
                   double lr, double beta1, double beta2, double eps, int step, float grad_scale, void* stream);
/* Global L2 norm of grad * grad_scale over the arena and torch.nn.utils.clip_grad_norm_'s coefficient, both left on the device:
 * t = fp32(grad[i] * grad_scale) - the value the Adam kernel sees -, sum of (double)t * t in two fixed-order fp64 stages (no atomics:
 * equal bits from call to call), *norm = (float)sqrt(sum), *clip = min(1.0f, max_norm / (*norm + 1e-6f)) in fp32; a non-finite norm
 * propagates as in torch (a NaN coefficient stays NaN).  norm or clip may be null, not both.  Any n >= 1 and any 4-byte-aligned grad.
 * ws: sscg_grad_norm_workspace(n) bytes. */
size_t sscg_grad_norm_workspace(int64_t n);
int sscg_grad_norm(const float* grad, int64_t n, float grad_scale, float max_norm, float* norm, float* clip, void* ws, size_t ws_bytes,
                   void* stream);
/* sscg_adam_step with options, still one launch.  Per element: g = grad * grad_scale (* *clip when `clip`, a device scalar, is given:
 * the two factors are multiplied first, so *clip == 1.0f changes no bit); weight_decay > 0 with decoupled == 0: g = fma(wd, param, g)
 * (torch.optim.Adam(weight_decay=): after the clip, and not part of the norm); with decoupled != 0: param *= (float)(1 - lr * wd)
 * first (torch.optim.AdamW); then sscg_adam_step's update and shadow write; `ema` (nullable, n floats): ema += (param_new - ema) *
 * (float)(1 - ema_decay), ema_decay in [0, 1).  With no clip, no decay and no ema this IS sscg_adam_step; with *clip == 1.0f and / or
 * an ema and no decay, param, both moments and shadow get sscg_adam_step's bits.  Zero param with zero grad (arena padding) stays zero
 * in param and ema under every option. */
int sscg_adam_step_ex(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow, int shadow_dtype, float* ema,
                      int64_t n, double lr, double beta1, double beta2, double eps, int step, float grad_scale, const float* clip,
                      double weight_decay, int decoupled, double ema_decay, void* stream);
int sscg_fill(float* x, int64_t n, float v, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSCG_H */
