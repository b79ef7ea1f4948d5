"""The second stage of a split-K tail (csrc/reduce_common.h split_reduce_kernel) in every convolution family, at the smallest shapes
whose plan still splits: a tail that is the whole output (m_tail0 = 0), rows of Ng elements that are no multiple of four (the
element-by-element instances), and a tail behind whole tiles whose output, residual and addend pointers start m_tail0 * Ng elements in.

Every test first asserts its regime from the workspace query (the host-only queries of test_conv_extents_host): a planner change
cannot make it vacuous.  References are torch fp64 on the values the device tensors hold (bf16 tensors: rounded first); the bounds are
those test_conv_extents_gpu and test_bf16_gpu use for these entries."""
import functools

import pytest
import torch
import torch.nn.functional as TF

from conftest import load_sub
import test_conv_extents_host as H
from test_conv_extents_gpu import BF, CL, EPS, F32, TOL_FWD, _act64, _mode, _rel, _rnd, _tdt, _tol
from test_pointwise_regimes_gpu import _table

pytestmark = pytest.mark.gpu
TINY = (1, 16, 16, 64, 64, 3, 1, 1, 1)        # M = 256: every tile of every family is cut along K
NG21 = (1, 16, 16, 128, 21, 3, 1, 1, 1)       # 21 output channels: rows of the tail are no multiple of 16 bytes
TAIL91 = H.CASES["tail91"]["shape"]           # 16562 rows: 178 tail rows behind 16384 rows of whole tiles
PIECES_TINY = {"f32x": 4, "f32s": 4, "bf16": 2}
PIECES_NG21 = {"f32x": 4, "f32s": 8, "bf16": 4}


@functools.lru_cache(maxsize=None)
def _case(shape, rounded):
    """operands (fp32 CPU tensors holding fp32 or bf16 values) and the fp64 convolution, its bias and data gradient; computed once"""
    N, Hh, W, Cin, K, R, s, p, d = shape
    fam = "bf16" if rounded else "f32x"
    x = _rnd(_table((N, Cin, Hh, W), 4001), fam)
    w = _rnd(_table((K, Cin, R, R), 4002, lo=-1.0, hi=1.0, noise=0.1, period=257) / (Cin * R * R) ** 0.5, fam)
    b = _table((K,), 4003, lo=-0.5, hi=0.5, noise=0.1, period=7)
    _, _, P, Q = H.geometry(shape)
    gy = _rnd(_table((N, K, P, Q), 4004, lo=-1.0, hi=1.0, noise=0.25, period=4093), fam)
    add = _rnd(_table((N, Cin, Hh, W), 4005, lo=-1.0, hi=1.0, noise=0.25, period=2039), fam)
    xr = x.double().requires_grad_(True)
    conv = TF.conv2d(xr, w.double(), None, s, p, d)
    conv.backward(gy.double())
    return dict(x=x, w=w, b=b, gy=gy, add=add, pre=conv.detach() + b.double().view(1, K, 1, 1), dx=xr.grad, P=P, Q=Q)


def _put(t, dev, dt=F32):
    t = t.to(dev).to(dt)
    return t.contiguous(memory_format=CL) if t.dim() == 4 else t


def _check(label, got, ref, bound):
    err = _rel(got, ref)
    print("split_tail %s err %.3e bound %.3e" % (label, err, bound))
    assert err < bound, (label, err, bound)


@pytest.mark.parametrize("fam", H.FAMILIES)
def test_a_tail_that_is_the_whole_output(fam, F, dev):
    """256 rows, every one through the reduction: forward with bias and ReLU, the data gradient, and in the split family the data
    gradient whose reduction joins an addend (sscg_conv2d_dgrad_add)."""
    N, Hh, W, Cin, K, R, s, p, d = TINY
    q = H.queries(load_sub("_lib"), TINY, fam)
    assert q["fwd"] == PIECES_TINY[fam] * 256 * K * 4 and q["dgrad"] == PIECES_TINY[fam] * 256 * Cin * 4, (fam, q["fwd"], q["dgrad"])
    c = _case(TINY, fam == "bf16")
    dt = _tdt(fam)
    xshape, wshape = (N, Cin, Hh, W), (K, Cin, R, R)
    with _mode(F, fam), torch.no_grad():
        x, w, b, gy = _put(c["x"], dev, dt), _put(c["w"], dev), _put(c["b"], dev), _put(c["gy"], dev, dt)
        y = F.conv2d_fwd(x, w, b, s, p, d, F.PAD_ZEROS, F.ACT_RELU, 0.0, out_f32=False)
        assert y.dtype == dt
        _check("tiny %s fwd" % fam, y, _act64(c["pre"], 1), _tol(fam, dt))
        wt = F.dgrad_operand(w, xshape, s, p, d, dy_dtype=dt)
        dx = F.conv2d_dgrad(gy, wt, xshape, wshape, s, p, d, out_dtype=dt)
        _check("tiny %s dgrad" % fam, dx, c["dx"], _tol(fam, dt))
        if fam == "f32s":
            add = _put(c["add"], dev)
            dxa, rec, joined = F.conv2d_dgrad(gy, wt, xshape, wshape, s, p, d, out_dtype=dt, addend=add)
            assert rec is None and joined, "the addend joins in the launch"
            _check("tiny f32s dgrad + addend", dxa, c["dx"] + c["add"].double(), TOL_FWD)


@pytest.mark.parametrize("fam", H.FAMILIES)
def test_rows_that_are_no_multiple_of_four_elements(fam, F, dev):
    """21 output channels: the element-by-element instances, fp32 and (bf16 family) bf16 outputs.  (The exact family's launcher can
    also ask for a bf16 output, but no wrapper of functional.py does in its mode: that instance's bf16 store is reached through the
    bf16 family alone - the kernel is the same template in every family.)"""
    N, Hh, W, Cin, K, R, s, p, d = NG21
    q = H.queries(load_sub("_lib"), NG21, fam)
    assert q["fwd"] == PIECES_NG21[fam] * 256 * K * 4, (fam, q["fwd"])
    c = _case(NG21, fam == "bf16")
    dt = _tdt(fam)
    with _mode(F, fam), torch.no_grad():
        x, w, b = _put(c["x"], dev, dt), _put(c["w"], dev), _put(c["b"], dev)
        for out_f32 in ((True, False) if fam == "bf16" else (True,)):
            y = F.conv2d_fwd(x, w, b, s, p, d, F.PAD_ZEROS, F.ACT_RELU, 0.0, out_f32=out_f32)
            assert y.dtype == (F32 if out_f32 else dt)
            _check("ng21 %s fwd out %s" % (fam, y.dtype), y, _act64(c["pre"], 1), _tol(fam, y.dtype))


@pytest.mark.parametrize("fam", ["f32s", "bf16"])
def test_folded_batchnorm_in_a_tail_behind_whole_tiles(fam, F, dev):
    """conv_bn_eval_act with gamma / beta and a residual where the last 178 rows go through split-K: the reduction carries the affine and
    reads the residual from row m_tail0 on; bit for bit the separate passes."""
    N, Hh, W, Cin, K, R, s, p, d = TAIL91
    rows, pieces = H.CASES["tail91"]["tail"][fam]
    q = H.queries(load_sub("_lib"), TAIL91, fam)
    assert q["affine"] == 1 and q["fwd"] == pieces * rows * K * 4 and 0 < rows < N * Hh * W, (fam, q["fwd"])
    dt = _tdt(fam)
    g = torch.Generator().manual_seed(91)
    x = _put(torch.randn(N, Cin, Hh, W, generator=g), dev, dt)
    w = _put(torch.randn(K, Cin, R, R, generator=g) * (1.0 / (Cin * R * R) ** 0.5), dev)
    bias = (torch.randn(K, generator=g) * 0.1).to(dev)
    rm, rv = (torch.randn(K, generator=g) * 0.3).to(dev), (torch.rand(K, generator=g) * 1.5 + 0.25).to(dev)
    ga, be = (torch.randn(K, generator=g) * 0.2 + 1.0).to(dev), (torch.randn(K, generator=g) * 0.2).to(dev)
    res = _put(torch.randn(N, K, Hh, W, generator=g), dev, dt)
    with _mode(F, fam), torch.no_grad():
        assert F.conv_bn_eval_applies(x, w, s, p, d, F.PAD_ZEROS, F.ACT_RELU, 0.0)
        y0 = F.conv2d(x, w, bias, s, p, d, F.PAD_ZEROS, F.ACT_NONE, 0.0, out_f32=False)
        want = F.batch_norm_act(y0, ga, be, rm, rv, False, 0.1, EPS, F.ACT_RELU, 0.0, res)
        got = F.conv_bn_eval_act(x, w, bias, rm, rv, ga, be, res, s, p, d, F.PAD_ZEROS, EPS, F.ACT_RELU, 0.0)
    assert got.dtype == want.dtype == dt and torch.isfinite(got.float()).all() and float(got.float().max()) > 0
    tail = got.permute(0, 2, 3, 1).reshape(-1, K)[-rows:]
    assert float(tail.float().max()) > 0 and float(tail.float().min()) == 0.0
    assert torch.equal(got, want), "%s: %d of %d elements differ" % (fam, int((got != want).sum()), got.numel())
