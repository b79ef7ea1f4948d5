// Contour scores of the evaluation (include/sscg.h: sscg_boundary_counts): the integer counts behind the Boundary IoU and the trimap
// mIoU of a ground-truth / predicted pair of label maps.  Forward only; without `--boundary` nothing launches it.
//   boundary_counts_kernel: one workgroup = one TILE x TILE tile of one sample and its d-pixel halo of BOTH maps, in three steps:
//     1. stage: a halo pixel becomes one 16-bit word - low byte t (the true label, VOID where it lies outside [0, C)), high byte r
//        (the predicted byte as it is).  Halo positions outside the image are never loaded and never read: the window is clipped.
//     2. row pass: per staged row inside the image and tile column, whether the clipped row segment [x - d, x + d] is uniform, for
//        both maps at once: the OR of (tap ^ centre) over the segment has a zero low / high byte.  The answer is one 32-bit word per
//        (row, column): the segment's label, or NOT_UNIFORM (a ninth bit no label has), t in the low half, r in the high half.
//     3. column pass: a window is uniform with value v iff every clipped row segment is uniform with value v, so a pixel compares the
//        2 d + 1 words of its column with its own label pair: in_t / in_r are a non-zero low / high half of the OR of the differences.
//   The work per pixel is 2 (2 d + 1) LDS reads for both maps together (the row pass also serves the 2 d halo rows), not (2 d + 1)^2.
// Counting: per-workgroup LDS bins [bt | bp | bi | tri], flushed with one 64-bit integer atomic per bin that was hit - integer sums,
// so the result is exact and independent of the order.  A predicted byte >= C takes part in every comparison and indexes nothing.
#include "common.h"
#include "head_common.h"
#include "sscg_internal.h"

namespace {

constexpr int TILE = 32;                              // a workgroup of 256 threads owns TILE x TILE output pixels, four per thread
constexpr int DMAX = 32;                              // the halo: at most 96 x 96 pixels
constexpr unsigned NOT_UNIFORM = 0x100u;              // per 16-bit half of a row-pass word: no byte label has this bit

struct BoundaryGeom {
    int H, W, C, d;
    int side, pitch;          // halo side TILE + 2 d; its row pitch in LDS (16-bit words, even: rows start on a dword)
    int tiles_x, tiles_y;
    FastDiv dtx, dty, dside;
};

__global__ __launch_bounds__(256) void boundary_counts_kernel(const int64_t* __restrict__ lt, const uint8_t* __restrict__ lp,
                                                              unsigned long long* __restrict__ counts, BoundaryGeom g) {
    extern __shared__ unsigned int lds[];             // [side][TILE] row-pass words | [nb] bins | [side][pitch] 16-bit label pairs
    const int C = g.C;
    const int nb = 3 * C + C * C;
    unsigned int* rowu = lds;
    unsigned int* bins = lds + g.side * TILE;
    unsigned short* lab = reinterpret_cast<unsigned short*>(bins + nb);
    sscg_bins_clear(bins, nb);

    const int bt = fd_div((int)blockIdx.x, g.dtx);
    const int bx = (int)blockIdx.x - bt * g.tiles_x;
    const int n = fd_div(bt, g.dty);
    const int by = bt - n * g.tiles_y;
    const int hy0 = by * TILE - g.d, hx0 = bx * TILE - g.d;      // the halo's first row / column in image coordinates
    const size_t map0 = (size_t)n * g.H * g.W;                    // the sample's first pixel (N*H*W < 2^31: checked by the entry)

    // 1. the halo of both maps; outside the image nothing is loaded and the LDS slot stays unwritten (it is never read)
    const int npix = g.side * g.side;
    for (int e = threadIdx.x; e < npix; e += 256) {
        const int hy = fd_div(e, g.dside), hx = e - hy * g.side;
        const int y = hy0 + hy, x = hx0 + hx;
        if (y >= 0 && y < g.H && x >= 0 && x < g.W) {
            const size_t o = map0 + (size_t)y * g.W + x;
            const int64_t t = lt[o];
            const unsigned tc = (t >= 0 && t < C) ? (unsigned)t : (unsigned)C;        // VOID = C <= 64
            lab[hy * g.pitch + hx] = (unsigned short)(tc | ((unsigned)lp[o] << 8));
        }
    }
    __syncthreads();

    // 2. row pass: (staged row hy, tile column tx) -> the label pair of the clipped segment, NOT_UNIFORM per half where it is mixed
    const int tx = threadIdx.x & (TILE - 1);
    const int x = bx * TILE + tx;
    const int sx_lo = (x - g.d > 0 ? x - g.d : 0) - hx0, sx_hi = (x + g.d < g.W - 1 ? x + g.d : g.W - 1) - hx0;
    for (int hy = threadIdx.x >> 5; hy < g.side; hy += 8) {
        const int y = hy0 + hy;
        if (y < 0 || y >= g.H || x >= g.W) continue;
        const unsigned short* row = lab + hy * g.pitch;
        const unsigned c = row[tx + g.d];
        unsigned diff = 0;
        for (int s = sx_lo; s <= sx_hi; ++s) diff |= row[s] ^ c;
        rowu[hy * TILE + tx] = ((diff & 0xffu) ? NOT_UNIFORM : (c & 0xffu)) | (((diff >> 8) ? NOT_UNIFORM : (c >> 8)) << 16);
    }
    __syncthreads();

    // 3. column pass and counting: thread = column tx of rows ty, ty + 8, ty + 16, ty + 24
    if (x < g.W) {
        const bool out_x = x < g.d || x >= g.W - g.d;
        for (int ty = threadIdx.x >> 5; ty < TILE; ty += 8) {
            const int y = by * TILE + ty;
            if (y >= g.H) break;
            const unsigned c = lab[(ty + g.d) * g.pitch + tx + g.d];
            const unsigned tc = c & 0xffu, rc = c >> 8;
            if (tc == (unsigned)C) continue;                       // not valid: counted nowhere
            const unsigned cw = tc | (rc << 16);
            const int sy_lo = (y - g.d > 0 ? y - g.d : 0) - hy0, sy_hi = (y + g.d < g.H - 1 ? y + g.d : g.H - 1) - hy0;
            unsigned diff = 0;
            for (int s = sy_lo; s <= sy_hi; ++s) diff |= rowu[s * TILE + tx] ^ cw;
            const bool in_t = (diff & 0xffffu) != 0, in_r = (diff >> 16) != 0;
            const bool out = out_x || y < g.d || y >= g.H - g.d;
            const bool et = in_t || out, er = in_r || out;
            if (et) atomicAdd(&bins[tc], 1u);
            if (rc < (unsigned)C) {                                // a predicted byte >= C is counted in no bin
                if (er) atomicAdd(&bins[C + rc], 1u);
                if (et && er && rc == tc) atomicAdd(&bins[2 * C + tc], 1u);
                if (in_t) atomicAdd(&bins[3 * C + tc * C + rc], 1u);
            }
        }
    }
    sscg_bins_flush(bins, nb, counts);
}

}  // namespace

extern "C" int sscg_boundary_counts(const int64_t* label_true, const uint8_t* label_pred, int N, int H, int W, int C, int d,
                                    int64_t* counts, void* stream) {
    if (!label_true || !label_pred || !counts) return SSCG_ERR_BAD_ARG;
    if (N <= 0 || H <= 0 || W <= 0 || C < 1 || C > SSCG_MAXC || d < 1 || d > DMAX) return SSCG_ERR_BAD_ARG;
    const uint64_t rows = (uint64_t)N * (uint64_t)H;                   // < 2^62: the second product cannot wrap once this one is small
    if (rows >= ((uint64_t)1 << 31) || rows * (uint64_t)W >= ((uint64_t)1 << 31)) return SSCG_ERR_UNSUPPORTED;
    BoundaryGeom g;
    g.H = H; g.W = W; g.C = C; g.d = d;
    g.side = TILE + 2 * d;
    g.pitch = g.side;                                                   // TILE + 2 d is even
    g.tiles_x = (W + TILE - 1) / TILE; g.tiles_y = (H + TILE - 1) / TILE;
    g.dtx = make_fastdiv(g.tiles_x); g.dty = make_fastdiv(g.tiles_y); g.dside = make_fastdiv(g.side);
    const size_t smem = ((size_t)g.side * TILE + (size_t)(3 * C + C * C)) * sizeof(unsigned int) +
                        (size_t)g.side * g.pitch * sizeof(unsigned short);            // <= 12 KB + 17 KB + 18 KB
    const dim3 grid((unsigned)((size_t)N * g.tiles_x * g.tiles_y));
    hipLaunchKernelGGL(boundary_counts_kernel, grid, dim3(256), smem, (hipStream_t)stream, label_true, label_pred,
                       reinterpret_cast<unsigned long long*>(counts), g);
    SSCG_LAUNCH_CHECK();
    return SSCG_OK;
}
