// Segmented stable radix sort of uint32 keys, descending, with the source index of every key (include/sscg.h: sscg_sort_u32_desc).
//
// S segments of L keys each.  Least significant digit first, eight bits per digit, so every pass must be stable; the last pass
// leaves the keys in descending order, equal keys by ascending source index.  Descending = ascending in d = 255 - digit.  A pass
// whose digit is zero in every key (the caller's `upper` bound says so) is skipped.  Every pass is three launches, and a dependency
// between workgroups is always a launch boundary - no block waits for another block of its launch:
//   1. sort_hist_kernel     block b of segment s counts the digits of its chunk of SORT_CHUNK keys in LDS (integer atomics) and
//                           STORES its 256 counts to table[s][d][b] - every entry is written, nothing is accumulated in memory;
//   2. sort_scan_kernel     one block per segment: the exclusive prefix sums of its [d][b] table in place - the first position
//                           of block b's keys with digit d;
//   3. sort_scatter_kernel  the same chunk again.  Wave w of a block owns a contiguous quarter of the chunk and walks it in rounds of
//                           64 keys.  Per round the lanes with equal digits find each other with nine 64-bit ballots (one per
//                           digit bit, one for the tail), the lowest of them adds their number to the wave's own LDS counter
//                           and hands the old value to its peers: the rank of a key among the wave's keys of that digit, in
//                           index order.  After a barrier thread d turns the four waves' counters of digit d into their
//                           starting positions, taken in wave order; a key's place is that plus its rank.
// Only integers: the result does not depend on any order of execution, and nothing is read from the workspace before this call
// wrote it.
//
// What rests on a guide's number: a wave is 64 lanes and __ballot returns 64 bits; a wave's LDS operations complete in order,
// so its counter needs no barrier between rounds; consecutive lanes load consecutive keys (4 B per lane, 256 B per wave
// instruction: coalesced, though not the 16 B per lane the guide calls the widest).  The counters sit at [wave][digit]: the
// 32-bank rule of ds_write_b32 makes the barrier-side accesses (thread d on digit d) conflict free.
// What rests on nothing measured: eight-bit digits (four passes for the loss's 30-bit keys, where ten-bit digits would take three
// with four times the counters), eight keys per lane, the histogram's plain LDS atomics (64-way contention on one bin when all keys
// agree), and the scatter's stores, which are contiguous only within a run of equal digits of one wave.
#include "common.h"
#include "scan_common.h"
#include "sscg_internal.h"

namespace {

constexpr int SORT_BINS = 256;                              // eight bits per digit
constexpr int SORT_ITEMS = 8;                               // keys per lane
constexpr int SORT_WAVE_KEYS = SORT_ITEMS * 64;             // the contiguous keys of one wave
constexpr int SORT_CHUNK = 4 * SORT_WAVE_KEYS;              // keys per block, in the histogram and in the scatter alike

__device__ __forceinline__ uint32_t sort_digit(uint32_t key, int shift) { return 255u - ((key >> shift) & 255u); }

__global__ __launch_bounds__(256) void sort_hist_kernel(const uint32_t* __restrict__ keys, uint32_t* __restrict__ table, int L, int nb,
                                                        int shift) {
    __shared__ unsigned int bins[SORT_BINS];
    const int s = blockIdx.x / nb, b = blockIdx.x - s * nb;
    bins[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t* ks = keys + (size_t)s * L;
    const long base = (long)b * SORT_CHUNK;
#pragma unroll
    for (int r = 0; r < SORT_CHUNK / 256; ++r) {
        const long i = base + r * 256 + threadIdx.x;
        if (i < L) atomicAdd(&bins[sort_digit(ks[i], shift)], 1u);
    }
    __syncthreads();
    table[((size_t)s * SORT_BINS + threadIdx.x) * nb + b] = bins[threadIdx.x];
}

__global__ __launch_bounds__(256) void sort_scan_kernel(uint32_t* __restrict__ table, int nb) {
    __shared__ uint32_t wsum[4];
    block_excl_scan_u32(table + (size_t)blockIdx.x * SORT_BINS * nb, (size_t)SORT_BINS * nb, wsum);
}

// FIRST: the source index of a key is its position (the first pass reads no index plane)
template <bool FIRST>
__global__ __launch_bounds__(256) void sort_scatter_kernel(const uint32_t* __restrict__ kin, const int32_t* __restrict__ iin,
                                                           uint32_t* __restrict__ kout, int32_t* __restrict__ iout,
                                                           const uint32_t* __restrict__ table, int L, int nb, int shift) {
    __shared__ unsigned int cnt[4][SORT_BINS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x / nb, b = blockIdx.x - s * nb;
#pragma unroll
    for (int w = 0; w < 4; ++w) cnt[w][tid] = 0u;
    __syncthreads();
    const size_t seg = (size_t)s * L;
    const long base = (long)b * SORT_CHUNK + (long)wave * SORT_WAVE_KEYS;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t k[SORT_ITEMS], rk[SORT_ITEMS];
    int32_t ix[SORT_ITEMS];
#pragma unroll
    for (int r = 0; r < SORT_ITEMS; ++r) {
        const long i = base + r * 64 + lane;
        const bool valid = i < L;
        k[r] = valid ? kin[seg + i] : 0u;
        ix[r] = FIRST ? (int32_t)i : (valid ? iin[seg + i] : 0);
        const uint32_t d = sort_digit(k[r], shift);
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool on = (d >> bit) & 1u;
            const unsigned long long m = __ballot(on);
            peers &= on ? m : ~m;
        }
        const int leader = peers ? __ffsll(peers) - 1 : 0;
        uint32_t old = 0u;
        if (valid && lane == leader) old = atomicAdd(&cnt[wave][d], (unsigned int)__popcll(peers));
        old = __shfl(old, leader, 64);
        rk[r] = old + (uint32_t)__popcll(peers & below);
    }
    __syncthreads();
    {
        uint32_t run = table[((size_t)s * SORT_BINS + tid) * nb + b];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t t = cnt[w][tid];
            cnt[w][tid] = run;
            run += t;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SORT_ITEMS; ++r) {
        const long i = base + r * 64 + lane;
        if (i < L) {
            const uint32_t pos = cnt[wave][sort_digit(k[r], shift)] + rk[r];
            if (pos < (uint32_t)L) {              // (always: the positions come from the counts of these very digits)
                kout[seg + pos] = k[r];
                iout[seg + pos] = ix[r];
            }
        }
    }
}

constexpr size_t SORT_ALIGN = 256;
size_t sort_round(size_t n) { return (n + SORT_ALIGN - 1) / SORT_ALIGN * SORT_ALIGN; }

bool sort_sizes_ok(int64_t S, int64_t L) {
    if (S <= 0 || L <= 0) return false;
    const int64_t lim = (int64_t)1 << 31;
    if (S >= lim || L >= lim || S * L >= lim) return false;
    const int64_t nb = (L + SORT_CHUNK - 1) / SORT_CHUNK;
    return S * nb * SORT_BINS < lim;
}

}  // namespace

extern "C" int sscg_sort_chunk(void) { return SORT_CHUNK; }

extern "C" size_t sscg_sort_ws_bytes(int64_t S, int64_t L) {
    if (!sort_sizes_ok(S, L)) return 0;
    const size_t nb = (size_t)((L + SORT_CHUNK - 1) / SORT_CHUNK);
    return sort_round((size_t)S * SORT_BINS * nb * sizeof(uint32_t)) + 2 * sort_round((size_t)S * (size_t)L * sizeof(uint32_t));
}

extern "C" int sscg_sort_u32_desc(const uint32_t* keys, int S, int L, uint32_t upper, uint32_t* out_keys, int32_t* out_index, void* ws,
                                  size_t ws_bytes, void* stream) {
    if (!keys || !out_keys || !out_index || keys == out_keys || S <= 0 || L <= 0) return SSCG_ERR_BAD_ARG;
    if (!sort_sizes_ok(S, L)) return SSCG_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < sscg_sort_ws_bytes(S, L)) return SSCG_ERR_WORKSPACE;
    if (((uintptr_t)ws & 3u) != 0) return SSCG_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int nb = (int)(((long)L + SORT_CHUNK - 1) / SORT_CHUNK);
    char* base = reinterpret_cast<char*>(ws);
    uint32_t* table = reinterpret_cast<uint32_t*>(base);
    const size_t plane = sort_round((size_t)S * (size_t)L * sizeof(uint32_t));
    uint32_t* tmp_k = reinterpret_cast<uint32_t*>(base + sort_round((size_t)S * SORT_BINS * nb * sizeof(uint32_t)));
    int32_t* tmp_i = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(tmp_k) + plane);
    // digits that can be non-zero: every key is below `upper` (0: no bound)
    int passes = 4;
    if (upper != 0u) {
        const uint32_t top = upper - 1u;
        passes = top >> 24 ? 4 : top >> 16 ? 3 : top >> 8 ? 2 : 1;
    }
    const dim3 grid((unsigned)S * (unsigned)nb), blk(256);
    const uint32_t* src_k = keys;
    const int32_t* src_i = nullptr;
    for (int p = 0; p < passes; ++p) {
        const bool to_out = ((passes - p) & 1) != 0;          // the last pass lands in the caller's planes
        uint32_t* dst_k = to_out ? out_keys : tmp_k;
        int32_t* dst_i = to_out ? out_index : tmp_i;
        const int shift = 8 * p;
        hipLaunchKernelGGL(sort_hist_kernel, grid, blk, 0, st, src_k, table, L, nb, shift);
        hipLaunchKernelGGL(sort_scan_kernel, dim3((unsigned)S), blk, 0, st, table, nb);
        if (p == 0)
            hipLaunchKernelGGL(sort_scatter_kernel<true>, grid, blk, 0, st, src_k, src_i, dst_k, dst_i, table, L, nb, shift);
        else
            hipLaunchKernelGGL(sort_scatter_kernel<false>, grid, blk, 0, st, src_k, src_i, dst_k, dst_i, table, L, nb, shift);
        src_k = dst_k;
        src_i = dst_i;
    }
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}
