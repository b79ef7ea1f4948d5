// Host side of a convolution launch, shared by the three kernel families (conv_igemm.hip Kc*, conv_split.hip Ks*, conv_bf16.hip
// K16*): descriptor -> GEMM geometry, the split-K plan of the tail, the stride-2 parity decomposition, the grid.  Host code only.
// The helpers are templates over the family's parameter struct (KcParams / KsParams / K16Params keep their own definitions: they are
// kernel arguments); what a family decides differently - its tile classes, its reduction length, which split rules it takes - stays in
// a short policy function in its own file (plan_kc_split, ks_plan, plan16).
#pragma once
#include <type_traits>
#include "common.h"
#include "sscg_internal.h"

// ---- split-K plan: which tiles are cut along K, and how often
// tiles [0, full_tiles) are computed whole by one workgroup each; the rest (the rows from m_tail0 on) in `splits` pieces of `ksplit` k-tiles
struct ConvSplit { int splits, ksplit, full_tiles, m_tail0; };

inline size_t split_bytes(const ConvSplit& sp, long M, int Ng) {
    return sp.splits > 1 ? (size_t)sp.splits * (M - sp.m_tail0) * Ng * sizeof(float) : 0;
}

// the tile grid of a launch in its family's chosen class; nk = k-tiles of the reduction
struct ConvTiles {
    long M;
    int nk, bm, tiles_m, tiles_n;
    int tiles() const { return tiles_m * tiles_n; }
};

inline ConvTiles conv_tiles(long M, int Ng, int nk, int bm, int bn) { return {M, nk, bm, cdiv(M, bm), cdiv(Ng, bn)}; }

inline ConvSplit unsplit(const ConvTiles& t) { return {1, t.nk, t.tiles(), (int)t.M}; }

// every tile in (about) s pieces
inline ConvSplit split_every_tile(const ConvTiles& t, int s) {
    const int ksplit = cdiv(t.nk, s);
    return {cdiv(t.nk, ksplit), ksplit, 0, 0};
}

// `tuning` = sscg_conv_desc.tuning (include/sscg.h): bits 0..7 = 1 + forced tile class, bits 8..15 = forced split-K
// (1 = never split, n > 1 = every tile cut in n).  False: the bits are clear, the family's own rules decide.
inline bool forced_split(const ConvTiles& t, int tuning, ConvSplit* sp) {
    const int force = (tuning >> 8) & 0xff;
    if (force == 0) return false;
    *sp = force == 1 ? unsplit(t) : split_every_tile(t, force);
    return true;
}

// Few-channel heads (Ng <= 32) on few rows: every tile (one 128x32 tile column gives only M/128 workgroups), towards 512 workgroups,
// for reductions of at least min_nk k-tiles and pieces of at least min_ksplit of them.
inline ConvSplit split_heads(const ConvTiles& t, int min_nk, int min_ksplit) {
    if (t.tiles() >= 256 || t.nk < min_nk) return unsplit(t);
    int s = cdiv(512, t.tiles());
    if (s > t.nk / min_ksplit) s = t.nk / min_ksplit;
    if (s > 32) s = 32;
    return s < 2 ? unsplit(t) : split_every_tile(t, s);
}

// Only the TAIL - the tiles beyond the last whole round of 256 workgroups.  The DeepLab stride-8 maps give 8712 rows -> 548 tiles of
// 64x64: 512 whole tiles (2 per CU) + 36 tail tiles cut in 7, so every CU gets 2 1/7 tiles of work instead of 2 or 3 (71 % balance),
// and only 6.5 % of the output goes through partial sums.  (34320 rows = 538 tiles of 128x128: 512 run whole, two per CU side by side,
// the other 26 would keep a tenth of the chip busy for a whole tile time.)
inline ConvSplit split_tail(const ConvTiles& t) {
    const int tiles = t.tiles();
    if (t.nk < 8 || tiles > 2300) return unsplit(t);
    const int q = tiles / 256;
    const int full_m = (q * 256) / t.tiles_n;          // whole tile rows handled unsplit
    const int tail = tiles - full_m * t.tiles_n;
    if (tail <= 0 || tail > 208) return unsplit(t);    // an almost complete round is left alone
    int s = 256 / tail;
    if (s > 8) s = 8;
    if (s > t.nk / 4) s = t.nk / 4;
    if (s < 2) return unsplit(t);
    ConvSplit r = split_every_tile(t, s);
    r.full_tiles = full_m * t.tiles_n;
    r.m_tail0 = full_m * t.bm;
    return r;
}

// stat_L > 0: the launch also produces normalisation statistics.  Split tiles write partial sums, not results, so their rows are
// summed separately (one extra group of records): they must all lie in ONE normalisation group, else the launch is not split.
inline ConvSplit keep_split_rows_in_one_group(const ConvSplit& sp, const ConvTiles& t, long stat_L) {
    if (stat_L > 0 && sp.splits > 1 && (sp.full_tiles == 0 || sp.m_tail0 / stat_L != (t.M - 1) / stat_L)) return unsplit(t);
    return sp;
}

// a store phase that takes sums or joins an addend sees whole tiles only: the partial tiles' reduction knows neither
inline ConvSplit no_split_with_fused_epilogue(const ConvSplit& sp, const ConvTiles& t, bool fused) { return fused ? unsplit(t) : sp; }

// the plan into the launch parameters; `ws` holds the partial tiles
template <class P>
int apply_split(P& p, const ConvSplit& sp, void* ws, size_t ws_bytes) {
    if (sp.splits > 1 && (!ws || ws_bytes < split_bytes(sp, p.M, p.Ng))) return SSCG_ERR_WORKSPACE;
    p.splits = sp.splits; p.ksplit = sp.ksplit; p.full_tiles = sp.full_tiles; p.m_tail0 = sp.m_tail0;
    p.part = reinterpret_cast<float*>(ws);
    return SSCG_OK;
}

// ---- descriptor -> GEMM geometry (the family sets its operands, dtypes and byte extents itself)
// launch walks every tap of a dense [R][S] weight and writes rows in order
template <class P>
void dense_taps(P& p) {
    p.pad_x = p.pad; p.wKtot = p.Ktot;
    p.wt_ky0 = 0; p.wt_kx0 = 0; p.wt_step = 1; p.wt_S = p.S;
    p.o_step = 1; p.o_a = 0; p.o_b = 0; p.o_W = 0; p.o_HW = 0;
}

// forward: rows = output pixels, columns = output channels, reduction over (tap, input channel)
template <class P>
void set_fwd_geometry(P& p, const sscg_conv_desc* d) {
    p.M = d->N * d->P * d->Q; p.Ng = d->K; p.Cs = d->C; p.Ktot = d->R * d->S * d->C;
    p.SH = d->H; p.SW = d->W; p.OH = d->P; p.OW = d->Q;
    p.R = d->R; p.S = d->S; p.stride = d->stride; p.pad = d->pad; p.dil = d->dil;
    p.pad_mode = d->pad_mode; p.act = d->act; p.slope = d->slope;
    dense_taps(p);
}

// data gradient: rows = input pixels, columns = input channels, reduction over (tap, output channel); zero padding only
template <class P>
void set_dgrad_geometry(P& p, const sscg_conv_desc* d, int act, float slope) {
    p.M = d->N * d->H * d->W; p.Ng = d->C; p.Cs = d->K; p.Ktot = d->R * d->S * d->K;
    p.SH = d->P; p.SW = d->Q; p.OH = d->H; p.OW = d->W;
    p.R = d->R; p.S = d->S; p.stride = d->stride; p.pad = d->pad; p.dil = d->dil;
    p.pad_mode = 0; p.act = act; p.slope = slope;
    dense_taps(p);
}

// Stride-2 data gradient (p: set_dgrad_geometry of d): an output pixel (2i+a, 2j+b) only meets the taps with ky = a+pad, kx = b+pad
// (mod 2).  Each of the four parity classes is a stride-1 data gradient over its own sub-lattice of taps, written interleaved into
// dx: a quarter of the multiply-adds of walking all R*S taps with three quarters of them masked.  launch(q) issues one class, unsplit.
template <class P, class F>
int for_each_dgrad_parity_class(P p, const sscg_conv_desc* d, F launch) {
    p.splits = 1; p.ksplit = 0; p.part = nullptr;
    p.stride = 1; p.wt_step = 2; p.wt_S = d->S;
    p.o_step = 2; p.o_W = d->W; p.o_HW = d->H * d->W;
    for (int a = 0; a < 2; ++a) {
        for (int b = 0; b < 2; ++b) {
            const int Ha = (d->H - a + 1) / 2, Wb = (d->W - b + 1) / 2;
            if (Ha <= 0 || Wb <= 0) continue;
            const int ky0 = (a + d->pad) & 1, kx0 = (b + d->pad) & 1;
            P q = p;
            q.R = ky0 < d->R ? (d->R - ky0 + 1) / 2 : 0;
            q.S = kx0 < d->S ? (d->S - kx0 + 1) / 2 : 0;
            if (q.R == 0 || q.S == 0) { q.R = 0; q.S = 0; }     // no tap meets this class: dx = act(bias)
            q.pad = (a + d->pad - ky0) / 2;
            q.pad_x = (b + d->pad - kx0) / 2;
            q.wt_ky0 = ky0; q.wt_kx0 = kx0;
            q.o_a = a; q.o_b = b;
            q.OH = Ha; q.OW = Wb;
            q.M = d->N * Ha * Wb;
            q.Ktot = q.R * q.S * q.Cs;
            const int rc = launch(q);
            if (rc) return rc;
        }
    }
    return SSCG_OK;
}

// ---- launch: the tile grid of a BM x BN class; returns the number of workgroups.  Families whose kernels decode tiles and rows
// without integer divisions carry four FastDivs: by tiles_n, OH * OW, OW and the rows of a normalisation group (bn_L of a data
// gradient with fused backward sums, else stat_L).
template <class P, class = void> struct has_fastdivs : std::false_type {};
template <class P> struct has_fastdivs<P, std::void_t<decltype(P::div_tn)>> : std::true_type {};

template <class P>
int launch_prologue(P& p, int BM, int BN) {
    p.tiles_n = cdiv(p.Ng, BN);
    p.tiles = cdiv(p.M, BM) * p.tiles_n;
    if (p.splits <= 1) { p.full_tiles = p.tiles; p.m_tail0 = p.M; }
    if constexpr (has_fastdivs<P>::value) {
        p.div_tn = make_fastdiv(p.tiles_n);
        p.div_hw = make_fastdiv(p.OH * p.OW);
        p.div_w = make_fastdiv(p.OW);
        p.div_gl = make_fastdiv(p.bn_sums != nullptr ? p.bn_L : (p.stat_L > 0 ? p.stat_L : 1));
    }
    return p.full_tiles + (p.tiles - p.full_tiles) * p.splits;
}

// ---- records of the backward sums a data gradient's store phase takes (sscg_conv2d_dgrad_bsums): G groups of L rows, tiles of bm
// rows, groups at least one tile tall (a tile then meets at most one group boundary): one record per tile and group
inline bool bsums_record_geometry(long M, int G, long L, int tile_bm, int* bm, int* wm, int* chunks) {
    if (G <= 0 || L <= 0 || (long)G * L != M || L < tile_bm) return false;
    *bm = tile_bm;
    *wm = 1;
    *chunks = (int)(cdiv(L, (long)tile_bm) + 1);
    return true;
}
