// Integer scans one workgroup of 256 threads makes on its own (sort.hip, lovasz.hip).  A scan that spans workgroups is split at
// launch boundaries by its callers: no block here ever waits for another.
#pragma once
#include "common.h"

// wave64 inclusive sum through shuffles
__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(v, o, 64);
        if (lane >= o) v += up;
    }
    return v;
}

// a[0 .. n) <- its exclusive prefix sums, in place, by one block of 256 threads: thread t owns a contiguous slice, the slices' sums
// are scanned (shuffles, then the four waves in order), the slice is rewritten.  wsum: four words of LDS.
__device__ __forceinline__ void block_excl_scan_u32(uint32_t* __restrict__ a, size_t n, uint32_t* wsum) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t per = (n + 255) / 256;
    size_t lo = (size_t)tid * per, hi = lo + per;
    lo = lo < n ? lo : n;
    hi = hi < n ? hi : n;
    uint32_t own = 0;
    for (size_t i = lo; i < hi; ++i) own += a[i];
    const uint32_t incl = wave_incl_scan_u32(own);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t run = incl - own;
    for (int w = 0; w < wave; ++w) run += wsum[w];
    for (size_t i = lo; i < hi; ++i) {
        const uint32_t t = a[i];
        a[i] = run;
        run += t;
    }
}
