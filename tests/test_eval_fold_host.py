"""Eval-mode BatchNorm folded into the conv (sscg_conv2d_fwd_affine) on a GPU-less host: the entry is declared, exported and
bound (tests/test_abi.py holds the three layers together), it returns argument errors before any HIP call, and its `_applies` query
answers for the DeepLab geometries of tests/golden/bench_conv_shapes.txt."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, load_sub

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
ONE = C.c_void_p(16)          # never dereferenced


def desc(L, n, h, w, c, k, r, stride, pad, dil, kind, act=1):
    p = (h + 2 * pad - dil * (r - 1) - 1) // stride + 1
    q = (w + 2 * pad - dil * (r - 1) - 1) // stride + 1
    xdt, wdt, ydt = {"split": (L.F32, L.BF16X3, L.F32), "bf16": (L.BF16, L.BF16, L.BF16), "f32": (L.F32, L.F32, L.F32)}[kind]
    return L.ConvDesc(N=n, H=h, W=w, C=c, K=k, R=r, S=r, P=p, Q=q, stride=stride, pad=pad, dil=dil, pad_mode=0, act=act, slope=0.0,
                      x_dtype=xdt, w_dtype=wdt, y_dtype=ydt, precision=0 if kind != "bf16" else 1)


def call(lib, d, x=ONE, w=ONE, mean=ONE, var=ONE, gamma=ONE, beta=ONE, res=None, y=ONE, ws=None, ws_bytes=0):
    return lib.sscg_conv2d_fwd_affine(C.byref(d), x, w, None, mean, var, 1e-5, gamma, beta, res, y, ws, ws_bytes, None)


def test_both_entries_are_declared_exported_and_bound():
    """The entries are an addition to the ABI (no existing entry changes), so header, library and binding agree on the version they had."""
    L = load_sub("_lib")
    hdr = open(os.path.join(ROOT, "include", "sscg.h")).read()
    assert L.lib.sscg_abi_version() == L.ABI_VERSION and "#define SSCG_ABI_VERSION %d" % L.ABI_VERSION in hdr
    assert "int sscg_conv2d_fwd_affine_applies(const sscg_conv_desc* d);" in hdr and "int sscg_conv2d_fwd_affine(" in hdr
    assert callable(L.lib.sscg_conv2d_fwd_affine) and callable(L.lib.sscg_conv2d_fwd_affine_applies)
    assert len(L.SIGNATURES["sscg_conv2d_fwd_affine"][1]) == 14 and len(L.SIGNATURES["sscg_conv2d_fwd_affine_applies"][1]) == 1


@pytest.mark.parametrize("kind", ["split", "bf16"])
def test_argument_errors_are_returned_before_any_launch(kind):
    L = load_sub("_lib")
    lib = L.lib
    d = desc(L, 8, 33, 33, 256, 256, 3, 1, 2, 2, kind)            # the bench-size DeepLab 3x3, dilation 2
    assert lib.sscg_conv2d_fwd_affine_applies(C.byref(d)) == 1
    assert lib.sscg_conv2d_fwd_affine_applies(None) == 0
    assert call(lib, d, x=None) == BAD_ARG and call(lib, d, w=None) == BAD_ARG and call(lib, d, y=None) == BAD_ARG
    assert call(lib, d, mean=None) == BAD_ARG and call(lib, d, var=None) == BAD_ARG
    assert call(lib, d, beta=None) == BAD_ARG and call(lib, d, gamma=None) == BAD_ARG            # gamma and beta: both or neither
    assert lib.sscg_conv2d_fwd_affine(None, ONE, ONE, None, ONE, ONE, 1e-5, None, None, None, ONE, None, 0, None) == BAD_ARG
    # the plan of this launch is the plain forward's: where that cuts a tail along K, a missing workspace is refused before any launch
    need = lib.sscg_conv2d_fwd_workspace(C.byref(d))
    if need:
        assert call(lib, d) == WORKSPACE
        assert call(lib, d, gamma=None, beta=None, ws=ONE, ws_bytes=need - 1) == WORKSPACE
    if kind == "split":
        assert need > 0           # tests/test_abi.py: this geometry's split plan has a tail


def test_stems_heads_and_thin_shapes_are_refused():
    L = load_sub("_lib")
    lib = L.lib
    stem = desc(L, 8, 256, 256, 3, 64, 7, 2, 3, 1, "f32")          # DeepLab's stem: the exact-fp32 kernel
    assert lib.sscg_conv2d_fwd_affine_applies(C.byref(stem)) == 0 and call(lib, stem) == UNSUPPORTED
    stem3 = desc(L, 8, 256, 256, 3, 64, 7, 2, 3, 1, "split")       # (split planes do not change that: C % 32 != 0)
    assert lib.sscg_conv2d_fwd_affine_applies(C.byref(stem3)) == 0 and call(lib, stem3) == UNSUPPORTED
    for kind in ("split", "bf16"):
        head = desc(L, 8, 33, 33, 2048, 21, 3, 1, 6, 6, kind)      # the classifier's class: 32 columns
        assert lib.sscg_conv2d_fwd_affine_applies(C.byref(head)) == 0 and call(lib, head) == UNSUPPORTED
        tanh = desc(L, 8, 33, 33, 256, 256, 3, 1, 2, 2, kind, act=3)
        assert lib.sscg_conv2d_fwd_affine_applies(C.byref(tanh)) == 0 and call(lib, tanh) == UNSUPPORTED
    f32y = desc(L, 8, 33, 33, 256, 256, 3, 1, 2, 2, "bf16")
    f32y.y_dtype = L.F32                                            # a bf16 network's fp32 head output
    assert lib.sscg_conv2d_fwd_affine_applies(C.byref(f32y)) == 0
    bad = desc(L, 8, 33, 33, 256, 256, 3, 1, 2, 2, "split")
    bad.P = 32                                                      # inconsistent geometry: BAD_ARG, as everywhere
    assert lib.sscg_conv2d_fwd_affine_applies(C.byref(bad)) == 0 and call(lib, bad) == BAD_ARG


def deeplab_shapes():
    out = []
    for line in open(os.path.join(ROOT, "tests", "golden", "bench_conv_shapes.txt")):
        m = re.match(r"(\d+)x(\d+)x(\d+) c(\d+) k(\d+) r(\d+) s(\d+) p(\d+) d(\d+)", line)
        if not m:
            continue
        n, h, w, c, k, r, s, p, d = map(int, m.groups())
        # the DeepLab trunk: 1x1 / 3x3 convolutions over a multiple of 64 channels into at least 64 (generators.py:345-365)
        if r in (1, 3) and c % 64 == 0 and k >= 64 and k % 64 == 0 and c >= 64 and (h in (33, 65) or d > 1 or c >= 256):
            out.append((n, h, w, c, k, r, s, p, d))
    return out


def test_applies_for_the_deeplab_shapes_in_both_modes():
    L = load_sub("_lib")
    shapes = deeplab_shapes()
    assert len(shapes) >= 10 and any(s[5] == 3 and s[8] > 1 for s in shapes) and any(s[5] == 1 for s in shapes)
    for (n, h, w, c, k, r, s, p, d) in shapes:
        for kind in ("split", "bf16"):
            dd = desc(L, n, h, w, c, k, r, s, p, d, kind)
            assert L.lib.sscg_conv2d_fwd_affine_applies(C.byref(dd)) == 1, (kind, n, h, w, c, k, r, s, p, d)


def test_wrapper_refuses_cpu_tensors_and_the_switch_is_read_from_the_environment():
    F, L = load_sub("functional"), load_sub("_lib")
    with pytest.raises(L.SscgError):
        F.conv_bn_eval_act(torch.zeros(1, 64, 9, 9), torch.zeros(64, 64, 1, 1), None, torch.zeros(64), torch.ones(64))
    assert isinstance(F.FUSE_EVAL_NORM[0], bool)
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); from conftest import load_sub; "
            "print(load_sub('functional').FUSE_EVAL_NORM[0])" % (ROOT, os.path.join(ROOT, "tests")))
    for val, want in ((None, "True"), ("0", "False"), ("1", "True")):
        env = dict(os.environ)
        env.pop("SSCG_FUSE_EVAL_NORM", None)
        if val is not None:
            env["SSCG_FUSE_EVAL_NORM"] = val
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.stdout.strip().splitlines()[-1] == want, (r.stdout, r.stderr[-2000:])
