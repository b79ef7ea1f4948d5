// The reduction frame the statistics entries of the unlabelled head share (unl.hip: sscg_unl_fwd; teacher.hip: sscg_teacher_fwd): how
// many blocks serve a sample, and the two fixed-order steps that turn the blocks' records of four doubles into the samples' sums.
// Device code is not linked across translation units: this header is instantiated in each, in an unnamed namespace.
#pragma once
#include "common.h"

namespace {

constexpr int UNL_BLOCKS = 256;    // statistics blocks per sample, grid-stride beyond (dice.hip's DICE_BLOCKS)

// `cnt` rows of four doubles -> one row: 64 row lanes of four threads (lane r takes rows r, r + 64, ... in order), the lanes in order by
// the column's first thread.  unl_reduce_kernel: block n sums sample n's records; the finish kernels: one block sums the samples.
__device__ __forceinline__ double unl_sum_rows(const double* __restrict__ rows, int cnt, double (&sm)[256]) {
    const int k = threadIdx.x & 3, rl = threadIdx.x >> 2;
    double s = 0.0;
    for (int r = rl; r < cnt; r += 64) s += rows[(size_t)r * 4 + k];
    sm[threadIdx.x] = s;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x < 4)
        for (int r = 0; r < 64; ++r) t += sm[r * 4 + k];
    return t;       // threads 0..3: column k
}

__global__ __launch_bounds__(256) void unl_reduce_kernel(const double* __restrict__ part, int bps, double* __restrict__ ssum) {
    __shared__ double sm[256];
    const double t = unl_sum_rows(part + (size_t)blockIdx.x * bps * 4, bps, sm);
    if (threadIdx.x < 4) ssum[(size_t)blockIdx.x * 4 + threadIdx.x] = t;
}

int unl_bps(int OH, int OW) {
    const long b = ((long)OH * OW + 255) / 256;
    return (int)(b > UNL_BLOCKS ? UNL_BLOCKS : b);
}

bool thresh_ok(float t) { return t >= 0.f && t <= 1.f; }      // (false for a NaN)

}  // namespace
