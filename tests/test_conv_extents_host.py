"""The case table of tests/test_conv_extents_gpu.py and the preconditions that make each case worth running (no GPU: the size queries
of include/sscg.h make no HIP call).

The GPU file runs the convolution entries between sentinel guards, with workspaces of exactly the size the library's own queries
promise.  A case checks something only while the planner still reaches the regime the case was chosen for - a split-K tail whose
last tile is ragged, partial tiles of every tile, records of the fused statistics / backward sums, several partial copies of a weight
gradient.  Those regimes are asserted HERE, from the queries, so that a planner change that makes a case vacuous fails this file instead
of passing silently on the GPU.

Shapes are (N, H, W, C, K, R, stride, pad, dil).  Kernel families: "f32x" the exact fp32 MFMA family (fp32 tensors, fp32 weight), "f32s"
the split contraction (fp32 tensors, three-plane bf16 weight; a geometry the split kernels do not serve falls to the exact family, as in
functional.py), "bf16" bf16 tensors and weights.  Split-K partial tiles are `pieces * rows * Ng * 4` bytes (csrc/conv_plan.h): rows =
all M output rows, or the tail rows M - m_tail0 behind the last whole round of workgroups; Ng = K (forward) or C (data gradient).

What each family documents about `tuning` = 0x300 ("every tile cut in three", csrc/conv_plan.h split_every_tile):
  * exact (conv_igemm.hip plan_kc_split) and split (conv_split.hip ks_plan): the bits count; the piece count is
    cdiv(nk, cdiv(nk, 3)) over nk k-tiles, i.e. 3 unless the reduction is only 2 or 4 k-tiles long (then 2: `forced` below names it);
    a stride-2 data gradient runs by parity class, planned unsplit (conv_split.hip "the forced-split bits do not reach them",
    conv_igemm.hip dgrad_by_parity): workspace 0;
  * bf16 (conv_bf16.hip plan16): "the forced-split bits of `tuning` do NOT count" - the forced-split case is dropped for that family;
    this file asserts that its answers do not move with the bits;
  * the thin 1x1 kernels (conv_thin.hip) take no workspace at all.
"""
import ctypes as C

import pytest

from conftest import load_sub

F32, BF16, BF16X3 = 0, 1, 2
ERR_UNSUPPORTED, ERR_WORKSPACE = -2, -3
FAMILIES = ("f32x", "f32s", "bf16")
TILE_H = 64        # rows of the 64x64 tile class, the only one whose tail is split at these sizes (the 128-row classes are multiples of it)
# forced tile classes per family (functional.tuning(tile_class=)): the exact family's classes as test_conv_all_tile_configs names them
# (class 8, the 256 x 4 tile, only where K <= 4), the split family's four (test_split_conv_every_tile_class), the bf16 family's as
# test_conv_bf16_every_tile_class names them
TILE_CLASSES = {"f32x": (0, 1, 2, 3, 4, 5, 6, 7), "f32s": (0, 1, 2, 3), "bf16": (0, 1, 3, 4, 5), "bf16c": (0, 3)}

# id -> case.  Keys besides `shape`:
#   tail:    {family: (tail rows, pieces)} of the forward's natural plan (tuning 0): 0 < workspace < every-tile bytes, ragged last tile
#   tail_dg: the same for the data gradient
#   every:   {family: pieces}: the natural forward plan cuts EVERY tile (workspace = pieces * M * K * 4)
#   every_dg: the same for the data gradient (M = N*H*W, Ng = C)
#   forced:  {entry: pieces} under tuning 0x300 for the exact and split families (default 3 where omitted; 0 = documented as unsplit)
#   records: families whose forward takes fused statistics AND whose data gradient takes backward sums (both queries > 0, G = 1)
#   stats:   families whose forward takes fused statistics only
#   wgrad:   {family: workspace bytes}: more than one partial copy of dw
#   why:     what the case reaches
CASES = {
    "tail91": dict(shape=(2, 91, 91, 64, 64, 3, 1, 1, 1), why="natural tail split: 178 tail rows = 2 tiles + a 50-row tile, cut in 4 (bf16: 2)",
                   tail={"f32x": (178, 4), "f32s": (178, 4), "bf16": (178, 2)}, tail_dg={"f32x": (178, 4), "f32s": (178, 4), "bf16": (178, 2)},
                   records=("f32s", "bf16"), stats=("f32x",), wgrad={"f32x": 4128768, "f32s": 4128768, "bf16": 7667712}),
    "tail65": dict(shape=(4, 65, 65, 64, 64, 3, 1, 1, 1), why="tail of 516 rows = 8 tiles + 4 rows",
                   tail={"f32x": (516, 4), "f32s": (516, 4), "bf16": (516, 2)}, records=("f32s", "bf16"), stats=("f32x",)),
    "k192": dict(shape=(2, 17, 15, 64, 192, 3, 1, 1, 1), why="every tile split; M = 510 ragged; K = 192 ragged in 128-column classes",
                 every={"f32x": 4, "f32s": 4, "bf16": 2}, every_dg={"f32x": 8, "f32s": 8, "bf16": 6}, records=("f32s", "bf16"), stats=("f32x",)),
    "p1x1": dict(shape=(3, 9, 7, 128, 320, 1, 1, 0, 1), why="1x1; M = 189; K = 320; forward unsplit, data gradient split in 2 (bf16: unsplit)",
                 every_dg={"f32x": 2, "f32s": 2}, forced={"fwd": 2}, wgrad={"f32s": 491520}),
    "head21": dict(shape=(2, 9, 9, 512, 21, 3, 1, 6, 6), why="21-column head in 32-column tiles, pad > half the map, split_heads",
                   every={"f32x": 18, "f32s": 8, "bf16": 18}),
    "head3": dict(shape=(2, 14, 12, 64, 3, 7, 1, 3, 1), why="3-column head (tanh, reflect variant too)",
                  every={"f32x": 11, "f32s": 11, "bf16": 10}, wgrad={"f32x": 150528, "f32s": 150528}),
    "stem3": dict(shape=(2, 20, 18, 3, 64, 7, 2, 3, 1), why="3-channel stem, stride 2", forced={"dgrad": 0},
                  stats=("f32x",), wgrad={"f32x": 112896, "f32s": 112896}),
    "stem20": dict(shape=(2, 20, 18, 20, 64, 7, 2, 3, 1), why="20-channel stem (padded to 32 channels in the split mode)", forced={"dgrad": 0},
                   every={"f32x": 7, "f32s": 7}, stats=("f32x",)),
    "stem21": dict(shape=(2, 20, 18, 21, 64, 7, 2, 3, 1), why="21-channel stem (padded to 32 channels in the split mode)", forced={"dgrad": 0},
                   every={"f32x": 7, "f32s": 7}, stats=("f32x",)),
    "s2odd": dict(shape=(2, 17, 15, 64, 64, 3, 2, 1, 1), why="stride-2 data gradient by parity class on an odd map; forward every tile split",
                  every={"f32x": 4, "f32s": 4, "bf16": 2}, forced={"dgrad": 0}, stats=("f32x", "f32s", "bf16")),
    "s2even": dict(shape=(2, 16, 16, 64, 128, 4, 2, 1, 1), why="4x4 stride-2 data gradient by parity class; forward every tile split",
                   every={"f32x": 8, "f32s": 8, "bf16": 4}, forced={"dgrad": 0}, stats=("f32x", "f32s", "bf16"), wgrad={"f32s": 1048576}),
    "m2115": dict(shape=(1, 47, 45, 128, 128, 3, 1, 1, 1), why="M = 2115, every tile split",
                  every={"f32x": 3, "f32s": 3, "bf16": 3}, every_dg={"f32x": 3, "f32s": 3, "bf16": 3}, records=("f32s", "bf16"), stats=("f32x",),
                  wgrad={"f32x": 4128768, "f32s": 12096000, "bf16": 4128768}),
    # at least 65536 pixels and 3 channels on one side: the streaming weight gradient (test_thin_1x1_weight_gradient); forward and data
    # gradient are conv_thin.hip's (no workspace); nothing is forced here
    "thin": dict(shape=(1, 256, 257, 3, 16, 1, 1, 0, 1), why="thin 1x1 weight gradient, 65792 pixels, 3 channels", thin=True,
                 wgrad={"f32x": 196608, "f32s": 196608}),       # 1024 blocks x 16 x 3 floats (K = 16 keeps dy at 1.05 M elements)
    # the second conv of the PixelDiscriminator front on an odd map (sscg_conv2d_front_fwd, cin 3 and 21); also the eval-fold case
    "front": dict(shape=(3, 37, 29, 64, 128, 1, 1, 0, 1), why="PixelDiscriminator front (cin 3 / 21) on an odd map; eval fold", front=(3, 21),
                  affine=("f32s", "bf16"), forced={"fwd": 2, "dgrad": 2}, records=("f32s", "bf16"), stats=("f32x",),
                  wgrad={"f32x": 1114112, "f32s": 1114112, "bf16": 360448}),
}
AFFINE_CASES = ("front", "tail91", "k192")       # sscg_conv2d_fwd_affine_applies in the split and bf16 families (asserted below)
BF16C_CASE = "tail91"                            # the one case the "bf16c" mode (fp32 tensors, precision 1) runs
CASE_IDS = tuple(CASES)


def out_size(h, r, s, p, d):
    return (h + 2 * p - d * (r - 1) - 1) // s + 1


def geometry(shape):
    """(M of the forward, M of the data gradient, P, Q)"""
    N, H, W, Cin, K, R, s, p, d = shape
    P, Q = out_size(H, R, s, p, d), out_size(W, R, s, p, d)
    return N * P * Q, N * H * W, P, Q


def served_shape(L, shape, fam, kind):
    """The (shape, dtype triple) the wrappers of functional.py build a descriptor from for this family; kind 0 forward, 1 data gradient.
    Split mode: 17-31 source channels run zero-padded to 32 (functional._padded_stem); a geometry the split kernels do not serve runs
    on the exact family."""
    if fam == "bf16":
        return shape, (BF16, BF16, BF16)
    if fam == "f32x":
        return shape, (F32, F32, F32)
    N, H, W, Cin, K, R, s, p, d = shape
    if 16 < Cin < 32 and K >= 16:
        padded = (N, H, W, 32, K, R, s, p, d)
        if L.lib.sscg_conv2d_split_applies(C.byref(desc(L, padded, (F32, F32, F32))), kind):
            return padded, (F32, BF16X3, F32)
    if L.lib.sscg_conv2d_split_applies(C.byref(desc(L, shape, (F32, F32, F32))), kind):
        return shape, (F32, BF16X3, F32)
    return shape, (F32, F32, F32)


def desc(L, shape, dtypes, tuning=0, precision=0, act=0):
    N, H, W, Cin, K, R, s, p, d = shape
    _, _, P, Q = geometry(shape)
    return L.ConvDesc(N=N, H=H, W=W, C=Cin, K=K, R=R, S=R, P=P, Q=Q, stride=s, pad=p, dil=d, pad_mode=0, act=act, slope=0.0,
                      x_dtype=dtypes[0], w_dtype=dtypes[1], y_dtype=dtypes[2], precision=precision, tuning=tuning)


def wgrad_desc(L, shape, fam):
    """descriptor of functional.conv2d_wgrad: tensor dtypes, the mode's precision (f32x 0, f32s 2, bf16 1), the weight dtype unset"""
    dt = BF16 if fam == "bf16" else F32
    return desc(L, shape, (dt, F32, dt), precision={"f32x": 0, "f32s": 2, "bf16": 1}[fam])


def queries(L, shape, fam, tuning=0):
    """the size queries of one case and family, each on the descriptor the wrappers would build"""
    fs, fdt = served_shape(L, shape, fam, 0)
    ds, ddt = served_shape(L, shape, fam, 1)
    df, dd = desc(L, fs, fdt, tuning), desc(L, ds, ddt, tuning)
    lib = L.lib
    mf, md, _, _ = geometry(shape)
    return dict(fwd=lib.sscg_conv2d_fwd_workspace(C.byref(df)), dgrad=lib.sscg_conv2d_dgrad_workspace(C.byref(dd)),
                stats=lib.sscg_conv2d_fwd_stats_bytes(C.byref(df), 1, mf), bsums=lib.sscg_conv2d_dgrad_bsums_bytes(C.byref(dd), 1, md),
                wgrad=lib.sscg_conv2d_wgrad_workspace(C.byref(wgrad_desc(L, shape, fam))),
                affine=lib.sscg_conv2d_fwd_affine_applies(C.byref(df)), fwd_desc=df, dgrad_desc=dd,
                Ng_fwd=fs[4], Ng_dgrad=ds[3])


@pytest.fixture(scope="module")
def L():
    return load_sub("_lib")


def _runs(case, fam):
    """bf16 tensors need 64-channel multiples on the operand side (functional._fwd_operands / conv2d_dgrad_param)"""
    Cin, K = case["shape"][3], case["shape"][4]
    return dict(fwd=fam != "bf16" or Cin % 64 == 0, dgrad=fam != "bf16" or K % 64 == 0)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_every_case_reaches_the_regime_it_was_chosen_for(cid, L):
    case = CASES[cid]
    shape = case["shape"]
    mf, md, _, _ = geometry(shape)
    N, H, W, Cin, K = shape[:5]
    assert max(N * H * W * Cin, mf * K, K * Cin * shape[5] ** 2) <= 1.1e6, "inputs stay at or below about 1.1 M elements"
    for fam in FAMILIES:
        q = queries(L, shape, fam)
        runs = _runs(case, fam)
        print("conv_extents host %s %s: fwd ws %d dgrad ws %d stats %d bsums %d wgrad ws %d affine %d" % (
            cid, fam, q["fwd"], q["dgrad"], q["stats"], q["bsums"], q["wgrad"], q["affine"]))
        for key, entry, M in (("tail", "fwd", mf), ("tail_dg", "dgrad", md)):
            if fam in case.get(key, {}) and runs[entry]:
                rows, pieces = case[key][fam]
                Ng = q["Ng_" + entry]
                every = pieces * M * Ng * 4
                assert 0 < q[entry] < every, (cid, fam, entry, q[entry], every)
                assert q[entry] == rows * Ng * 4 * pieces, (cid, fam, entry, q[entry])
                assert rows % TILE_H != 0 and 0 < rows < M, (cid, fam, entry, rows)
        for key, entry, M in (("every", "fwd", mf), ("every_dg", "dgrad", md)):
            if fam in case.get(key, {}) and runs[entry]:
                pieces = case[key][fam]
                assert pieces > 1 and q[entry] == pieces * M * q["Ng_" + entry] * 4, (cid, fam, entry, q[entry], pieces)
        if fam in case.get("records", ()):
            assert q["stats"] > 0 and q["bsums"] > 0, (cid, fam, q["stats"], q["bsums"])
        if fam in case.get("stats", ()):
            assert q["stats"] > 0, (cid, fam)
        if fam in case.get("wgrad", {}):
            dw_bytes = K * Cin * shape[5] ** 2 * 4
            assert q["wgrad"] == case["wgrad"][fam] and q["wgrad"] > dw_bytes, (cid, fam, q["wgrad"], dw_bytes)
        if fam in case.get("affine", ()) or (cid in AFFINE_CASES and fam != "f32x"):
            assert q["affine"] == 1, (cid, fam)
    if case.get("thin"):
        assert shape[5] == 1 and N * H * W >= 65536 and min(Cin, K) <= 32
    for cin in case.get("front", ()):
        assert H % 2 == 1 and W % 2 == 1
        q = queries(L, shape, "f32s")
        assert L.lib.sscg_conv2d_front_applies(C.byref(q["fwd_desc"]), cin) == 1, (cid, cin)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_forced_split_cuts_every_tile_or_is_documented_as_ignored(cid, L):
    """tuning = 0x300: the exact and split families answer pieces * M * Ng * 4 with pieces = 3 (2 where the table says the reduction is
    too short for three, 0 where the data gradient runs by parity class); the bf16 family's answers do not move with the bits."""
    case = CASES[cid]
    shape = case["shape"]
    mf, md, _, _ = geometry(shape)
    for fam in FAMILIES:
        q0, q3 = queries(L, shape, fam, 0), queries(L, shape, fam, 0x300)
        print("conv_extents host %s %s forced split 3: fwd ws %d dgrad ws %d" % (cid, fam, q3["fwd"], q3["dgrad"]))
        if fam == "bf16" and shape[3] % 64 == 0 and shape[4] % 64 == 0:
            assert (q3["fwd"], q3["dgrad"]) == (q0["fwd"], q0["dgrad"]), (cid, "the bf16 family ignores the forced-split bits")
            continue
        if fam == "bf16" or case.get("thin"):
            continue        # (fp32-boundary layers of the bf16 mode run the exact family: covered under f32x; thin: no workspace)
        for entry, M in (("fwd", mf), ("dgrad", md)):
            pieces = case.get("forced", {}).get(entry, 3)
            assert q3[entry] == pieces * M * q3["Ng_" + entry] * 4, (cid, fam, entry, q3[entry], pieces)


def _thin_territory(d):
    """conv_thin.hip's shapes: no workspace check in front of its launch (tests/golden/gen_conv_plans.py)"""
    return d.R == 1 and (d.K <= 4 or d.C <= 32)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_one_byte_short_of_the_promised_workspace_is_refused_before_any_launch(cid, L):
    """every entry with need > 0, called with ws_bytes = need - 1 and never-dereferenced pointers: SSCG_ERR_WORKSPACE (the entries check
    the workspace in front of their first launch: conv_plan.h apply_split, conv_wgrad.hip sscg_conv2d_wgrad and the kernels behind it)"""
    case = CASES[cid]
    one = C.c_void_p(16)        # never dereferenced
    lib = L.lib
    refused = 0
    for fam in FAMILIES:
        for tuning in (0, 0x300):
            q = queries(L, case["shape"], fam, tuning)
            runs = _runs(case, fam)
            df, dd = q["fwd_desc"], q["dgrad_desc"]
            rcs = {}
            if q["fwd"] > 0 and runs["fwd"] and not _thin_territory(df):
                rcs["fwd"] = lib.sscg_conv2d_fwd(C.byref(df), one, one, None, one, one, q["fwd"] - 1, None)
                if q["affine"]:
                    rcs["fwd_affine"] = lib.sscg_conv2d_fwd_affine(C.byref(df), one, one, None, one, one, 1e-5, None, None, None, one, one,
                                                                   q["fwd"] - 1, None)
            if q["dgrad"] > 0 and runs["dgrad"] and not _thin_territory(dd):
                rcs["dgrad"] = lib.sscg_conv2d_dgrad(C.byref(dd), one, one, None, one, 0, 0.0, one, q["dgrad"] - 1, None)
            if q["wgrad"] > 0 and tuning == 0:
                rcs["wgrad"] = lib.sscg_conv2d_wgrad(C.byref(wgrad_desc(L, case["shape"], fam)), one, one, one, 0.0, one, q["wgrad"] - 1, None)
            bad = {e: rc for e, rc in rcs.items() if rc != ERR_WORKSPACE}
            assert not bad, (cid, fam, hex(tuning), bad)
            refused += len(rcs)
    assert refused > 0, cid


# [G][L][C] views the normalisation entries run on in the GPU file
NORM_SHAPES = ((1, 8712, 256), (3, 143, 64), (2, 4097, 20), (1, 510, 132), (2, 81, 2048), (1, 65792, 3))


@pytest.mark.parametrize("glc", NORM_SHAPES, ids=lambda s: "g%d_l%d_c%d" % s)
def test_norm_entries_refuse_a_short_workspace(glc, L):
    G, Ln, Cn = glc
    lib = L.lib
    one = C.c_void_p(16)
    need = lib.sscg_colsum_workspace(G * Ln, Cn)
    assert need > 0 and lib.sscg_colsum(one, F32, one, G * Ln, Cn, 0.0, one, need - 1, None) == ERR_WORKSPACE
    need = lib.sscg_norm_stats_workspace(G, Ln, Cn)
    assert need > 0 and lib.sscg_norm_stats(one, F32, G, Ln, Cn, 1e-5, one, one, None, None, 0.1, one, need - 1, None) == ERR_WORKSPACE
    need = lib.sscg_norm_bwd_workspace(G, Ln, Cn)
    assert need > 0 and lib.sscg_norm_bwd(one, one, None, one, one, None, None, one, None, None, None, F32, G, Ln, Cn, 0, 0.0, 1, one,
                                          need - 1, None) == ERR_WORKSPACE
    for ch in (16, 256):
        need = lib.sscg_norm_head_bwd_workspace(G, Ln, ch)
        assert need > 0 and lib.sscg_norm_head_bwd(one, one, one, one, one, None, None, one, one, one, None, None, F32, G, Ln, ch, 2, 0.2, 7,
                                                   one, need - 1, None) == ERR_WORKSPACE
