"""sscg_conv2d_dgrad_bsums_masked: declared, exported, bound, and its refusals come back before any HIP call (no GPU needed)."""
import ctypes as C
import os

from conftest import ROOT, load_sub

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3


def _call(L, name, d, act, sums_bytes=0):
    one = C.c_void_p(16)          # never dereferenced
    return getattr(L.lib, name)(C.byref(d), one, one, one, one, one, None, one, one, None, None, 1, d.N * d.H * d.W, act, 0.0, one,
                                sums_bytes, None, 0, None)


def test_entry_is_an_addition_with_the_signature_of_its_twin():
    L = load_sub("_lib")
    hdr = open(os.path.join(ROOT, "include", "sscg.h")).read()
    assert "sscg_conv2d_dgrad_bsums_masked(" in hdr and "#define SSCG_ABI_VERSION %d" % L.ABI_VERSION in hdr
    assert L.SIGNATURES["sscg_conv2d_dgrad_bsums_masked"] == L.SIGNATURES["sscg_conv2d_dgrad_bsums"]
    assert L.lib.sscg_abi_version() == L.ABI_VERSION


def test_refusals_come_before_any_launch():
    L = load_sub("_lib")
    geo = dict(N=8, H=33, W=33, C=256, K=256, R=3, S=3, P=33, Q=33, stride=1, pad=2, dil=2, pad_mode=0, act=0, slope=0.0)
    split = L.ConvDesc(x_dtype=L.F32, w_dtype=L.BF16X3, y_dtype=L.F32, precision=2, **geo)
    rows = 8 * 33 * 33
    assert L.lib.sscg_conv2d_dgrad_bsums_bytes(C.byref(split), 1, rows) > 0
    # ReLU on the split family passes every check (the next one is the size of `sums`); the existing entry likewise, for all three
    assert _call(L, "sscg_conv2d_dgrad_bsums_masked", split, L.ACT_RELU) == WORKSPACE
    for act in (L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU):
        assert _call(L, "sscg_conv2d_dgrad_bsums", split, act) == WORKSPACE
    # any other activation
    for act in (L.ACT_NONE, L.ACT_LRELU, L.ACT_TANH):
        assert _call(L, "sscg_conv2d_dgrad_bsums_masked", split, act) == UNSUPPORTED
    # the bf16 family takes sums for this geometry, but stores the total
    b16 = L.ConvDesc(x_dtype=L.BF16, w_dtype=L.BF16, y_dtype=L.BF16, precision=0, **geo)
    assert L.lib.sscg_conv2d_dgrad_bsums_bytes(C.byref(b16), 1, rows) > 0
    assert _call(L, "sscg_conv2d_dgrad_bsums", b16, L.ACT_RELU) == WORKSPACE
    assert _call(L, "sscg_conv2d_dgrad_bsums_masked", b16, L.ACT_RELU) == UNSUPPORTED
    # geometries without fused sums: a strided data gradient, groups shorter than a tile
    s2 = L.ConvDesc(x_dtype=L.F32, w_dtype=L.BF16X3, y_dtype=L.F32, precision=2, N=2, H=32, W=32, C=64, K=128, R=3, S=3, P=16, Q=16,
                    stride=2, pad=1, dil=1, pad_mode=0, act=0, slope=0.0)
    assert L.lib.sscg_conv2d_dgrad_bsums_bytes(C.byref(s2), 1, 2 * 32 * 32) == 0
    assert _call(L, "sscg_conv2d_dgrad_bsums_masked", s2, L.ACT_RELU) == UNSUPPORTED
    short = L.ConvDesc(x_dtype=L.F32, w_dtype=L.BF16X3, y_dtype=L.F32, precision=2, N=2, H=4, W=4, C=64, K=64, R=1, S=1, P=4, Q=4,
                       stride=1, pad=0, dil=1, pad_mode=0, act=0, slope=0.0)
    assert L.lib.sscg_conv2d_dgrad_bsums_bytes(C.byref(short), 2, 16) == 0
    assert _call(L, "sscg_conv2d_dgrad_bsums_masked", short, L.ACT_RELU) == UNSUPPORTED
    # null tensors are argument errors, as for the existing entry
    assert L.lib.sscg_conv2d_dgrad_bsums_masked(C.byref(split), None, None, None, None, None, None, None, None, None, None, 1, rows,
                                                L.ACT_RELU, 0.0, None, 0, None, 0, None) == BAD_ARG
