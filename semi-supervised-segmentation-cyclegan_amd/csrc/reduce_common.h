// Second stage of a tail-split / split-K convolution launch, shared by conv_igemm.hip, conv_split.hip and conv_bf16.hip (device
// code is not linked across translation units: this header is instantiated in each).  The first stage left `splits` fp32 partial
// sums [splits][rows][Ng] of the rows that went through split-K; this pass forms y = epilogue(sum_s part[s] + bias) for them.
#pragma once
#include "common.h"
#include "norm_expr.h"

// What a family's launcher hands over (host side, and the kernels' argument).  Pointers are those of the TAIL: y, addend and res
// start at the first split row.
struct SplitTail {
    const float* part;       // [splits][rows][Ng]
    const float* bias;       // [Ng] or null
    void* y;                 // [rows][Ng], fp32 or bf16
    int out_bf16;
    int rows, Ng, splits;
    int act;
    float slope;
    const void* addend;      // plain epilogue: [rows][Ng] in y's dtype, joined behind the activation; or null
    double* xstats;          // plain epilogue: non-null = the column statistics' records (split_reduce_stats_kernel)
    bool affine;             // the eval-mode BatchNorm of a folded launch (norm_expr.h) between bias and activation
    const float* mean;       // [Ng] running_mean, running_var; gamma / beta [Ng] or both null
    const float* var;
    const float* gamma;
    const float* beta;
    const void* res;         // [rows][Ng] in y's dtype, or null
    float eps;
};

// the fp32 sum over the splits in index order (fixed order => deterministic), V consecutive elements from element i on
template <int V>
__device__ __forceinline__ void split_sum(const float* __restrict__ part, size_t n, size_t i, int splits, float (&a)[V]) {
    float s[V];
#pragma unroll
    for (int e = 0; e < V; ++e) s[e] = 0.f;
#pragma unroll 8
    for (int k = 0; k < splits; ++k) {
        float t[V];
        if constexpr (V == 4) ld4<float>(part + (size_t)k * n + i, t); else t[0] = part[(size_t)k * n + i];
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] += t[e];
    }
#pragma unroll
    for (int e = 0; e < V; ++e) a[e] = s[e];
}

template <int V> __device__ __forceinline__ void split_bias(const float* __restrict__ bias, int c, float (&bv)[V]) {
    float b[V];
#pragma unroll
    for (int e = 0; e < V; ++e) b[e] = bias ? bias[c + e] : 0.f;
#pragma unroll
    for (int e = 0; e < V; ++e) bv[e] = b[e];
}

// V elements of a tensor that is fp32 or bf16 at run time
template <int V> __device__ __forceinline__ void split_load(const void* p, int is_bf16, size_t i, float (&v)[V]) {
    if (is_bf16) {
        const __bf16* q = reinterpret_cast<const __bf16*>(p) + i;
        if constexpr (V == 4) ld4<__bf16>(q, v); else v[0] = ld1<__bf16>(q);
    } else {
        const float* q = reinterpret_cast<const float*>(p) + i;
        if constexpr (V == 4) ld4<float>(q, v); else v[0] = ld1<float>(q);
    }
}
template <int V> __device__ __forceinline__ void split_store(void* p, int is_bf16, size_t i, const float (&v)[V]) {
    if (is_bf16) {
        __bf16* q = reinterpret_cast<__bf16*>(p) + i;
        if constexpr (V == 4) st4<__bf16>(q, v); else st1<__bf16>(q, v[0]);
    } else {
        float* q = reinterpret_cast<float*>(p) + i;
        if constexpr (V == 4) st4<float>(q, v); else st1<float>(q, v[0]);
    }
}

// plain epilogue of one element: pre = sum + bias, the result act(pre)
__device__ __forceinline__ float split_plain(float sum, float bias, int act, float slope, float& pre) {
    pre = sum + bias;
    return sscg_act(pre, act, slope);
}

// y[i] = act(sum_s part[s][i] + bias[i % Ng]) [+ addend[i]], or with AFFINE the folded launch's
// y[i] = act(bn(sum_s part[s][i] + bias) + res[i]): per element what the plain pass followed by sscg_norm_apply computes - for bf16
// tensors the sum is rounded to bf16 (the conv's stored output) and widened again in front of the affine.  V elements per thread;
// V == 4 only when Ng % 4 == 0: the V channels are consecutive.
template <int V, bool AFFINE>
__global__ __launch_bounds__(256) void split_reduce_kernel(SplitTail t) {
    const size_t n = (size_t)t.rows * t.Ng;
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (i >= n) return;
    const int c = (int)(i % t.Ng);
    float a[V], bv[V], o[V], pre;
    split_sum<V>(t.part, n, i, t.splits, a);
    split_bias<V>(t.bias, c, bv);
    if constexpr (AFFINE) {
        float rv[V];
#pragma unroll
        for (int e = 0; e < V; ++e) rv[e] = 0.f;
        if (t.res) split_load<V>(t.res, t.out_bf16, i, rv);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float x = a[e] + bv[e];
            if (t.out_bf16) x = (float)(__bf16)x;
            o[e] = sscg_act(sscg_bn_fold(x, t.mean[c + e], sscg_bn_rstd(t.var[c + e], t.eps), t.gamma ? t.gamma[c + e] : 1.f,
                                         t.gamma ? t.beta[c + e] : 0.f, t.gamma != nullptr, rv[e], t.res != nullptr), t.act, t.slope);
        }
    } else {
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = split_plain(a[e], bv[e], t.act, t.slope, pre);
        if (t.addend) {
            float av[V];
            split_load<V>(t.addend, t.out_bf16, i, av);
#pragma unroll
            for (int e = 0; e < V; ++e) o[e] += av[e];
        }
    }
    split_store<V>(t.y, t.out_bf16, i, o);
}

// The plain pass AND the column statistics of the pre-activation values for the fused normalisation statistics: one record
// [Ng][2] (sum, sum of squares; fp64) per block of `rows_per_block` rows.  V channels per thread.
template <int V>
__global__ __launch_bounds__(256) void split_reduce_stats_kernel(const float* __restrict__ part, const float* __restrict__ bias,
                                                                  void* __restrict__ y, int out_bf16, int rows, int Ng, int splits,
                                                                  int act, float slope, double* __restrict__ recs, int rows_per_block) {
    extern __shared__ __attribute__((aligned(16))) char sm_raw[];
    double* sm = reinterpret_cast<double*>(sm_raw);          // [256][V][2]
    const int cgs = Ng / V;                                  // channel groups of the tensor
    const int cg_blk = cgs < 256 ? cgs : 256;                // ... owned by one block
    const int lanes = 256 / cg_blk;                          // row lanes of the block
    const int cl = threadIdx.x % cg_blk;
    const int rl = threadIdx.x / cg_blk;
    const int cg = blockIdx.y * cg_blk + cl;
    const bool on = cg < cgs && rl < lanes;
    const int r0 = blockIdx.x * rows_per_block;
    const int r1 = min(rows, r0 + rows_per_block);
    const size_t n = (size_t)rows * Ng;
    double s[V], q[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { s[e] = 0.0; q[e] = 0.0; }
    if (on) {
        float bv[V];
        split_bias<V>(bias, cg * V, bv);
        for (int r = r0 + rl; r < r1; r += lanes) {
            const size_t i = (size_t)r * Ng + (size_t)cg * V;
            float a[V], o[V];
            split_sum<V>(part, n, i, splits, a);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                float pre;
                o[e] = split_plain(a[e], bv[e], act, slope, pre);
                const double d = (double)pre;
                s[e] += d;
                q[e] += d * d;
            }
            split_store<V>(y, out_bf16, i, o);
        }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) { sm[(threadIdx.x * V + e) * 2] = s[e]; sm[(threadIdx.x * V + e) * 2 + 1] = q[e]; }
    __syncthreads();
    if (on && rl == 0) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
            double a = 0.0, b = 0.0;
            for (int l = 0; l < lanes; ++l) {
                a += sm[((l * cg_blk + cl) * V + e) * 2];
                b += sm[((l * cg_blk + cl) * V + e) * 2 + 1];
            }
            double* rec = recs + ((size_t)blockIdx.x * Ng + (size_t)cg * V + e) * 2;
            rec[0] = a;
            rec[1] = b;
        }
    }
}

// Rows per block (= per statistics record) of the split reduction: one row per row-lane, at least 4.  The split rows are
// a few hundred to a thousand; the reduction sits on the critical path of its layer (conv -> statistics -> normalise), so
// it is spread over >= 100 workgroups rather than kept compact.
static inline int split_stats_rpb(int Ng) {
    const int cgs = Ng % 4 == 0 ? Ng / 4 : Ng;
    const int lanes = 256 / (cgs < 256 ? cgs : 256);
    return lanes > 4 ? lanes : 4;
}

static inline int split_stats_records(long rows, int Ng) {
    const int rpb = split_stats_rpb(Ng);
    return (int)((rows + rpb - 1) / rpb);
}

// the tail of a launch whose parameters carry the families' common fields; the caller adds addend, xstats or the affine
static inline SplitTail split_tail_of(const float* part, const float* bias, void* dst, int out_bf16, long M, long m_tail0, int Ng,
                                      int splits, int act, float slope) {
    SplitTail t = {};
    t.part = part; t.bias = bias;
    t.y = reinterpret_cast<char*>(dst) + (size_t)m_tail0 * Ng * (out_bf16 ? 2 : 4);
    t.out_bf16 = out_bf16;
    t.rows = (int)(M - m_tail0); t.Ng = Ng; t.splits = splits; t.act = act; t.slope = slope;
    return t;
}

// a tensor of y's shape and dtype from the tail's first row on (addend, residual)
static inline const void* split_tail_ptr(const void* p, const SplitTail& t, long m_tail0) {
    return p ? reinterpret_cast<const char*>(p) + (size_t)m_tail0 * t.Ng * (t.out_bf16 ? 2 : 4) : nullptr;
}

// One rule for every family: four elements per thread exactly when rows of Ng elements keep four-element accesses aligned and
// the tensors start aligned (16 bytes of fp32, 8 bytes of bf16); element by element otherwise.
static inline int launch_split_reduce(const SplitTail& t, hipStream_t st) {
    const size_t am = t.out_bf16 ? 7 : 15;
    const bool v4 = t.Ng % 4 == 0 && ((size_t)t.part & 15) == 0 && (((size_t)t.y | (size_t)t.addend | (size_t)t.res) & am) == 0;
    const size_t n = (size_t)t.rows * t.Ng;
    const dim3 grid(cdiv((long)(v4 ? n / 4 : n), 256));
    if (t.affine) {
        if (v4) hipLaunchKernelGGL((split_reduce_kernel<4, true>), grid, dim3(256), 0, st, t);
        else hipLaunchKernelGGL((split_reduce_kernel<1, true>), grid, dim3(256), 0, st, t);
    } else if (t.xstats) {      // the split rows' column statistics come out of their reduction pass
        const int cgs = v4 ? t.Ng / 4 : t.Ng;
        const int cg_blk = cgs < 256 ? cgs : 256;
        const dim3 sgrid(split_stats_records(t.rows, t.Ng), (cgs + cg_blk - 1) / cg_blk);
        const size_t smem = (size_t)256 * (v4 ? 4 : 1) * 2 * sizeof(double);
        if (v4) hipLaunchKernelGGL(split_reduce_stats_kernel<4>, sgrid, dim3(256), smem, st, t.part, t.bias, t.y, t.out_bf16, t.rows, t.Ng, t.splits, t.act,
                                   t.slope, t.xstats, split_stats_rpb(t.Ng));
        else hipLaunchKernelGGL(split_reduce_stats_kernel<1>, sgrid, dim3(256), smem, st, t.part, t.bias, t.y, t.out_bf16, t.rows, t.Ng, t.splits, t.act,
                                   t.slope, t.xstats, split_stats_rpb(t.Ng));
    } else {
        if (v4) hipLaunchKernelGGL((split_reduce_kernel<4, false>), grid, dim3(256), 0, st, t);
        else hipLaunchKernelGGL((split_reduce_kernel<1, false>), grid, dim3(256), 0, st, t);
    }
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}
