"""The data gradient that takes a ReLU unit's backward sums stores the MASKED gradient (sscg_conv2d_dgrad_bsums_masked, functional.PREMASK):
the unit's apply pass then reads no mask source and writes no residual gradient.  Nothing may change by a bit - every comparison here is
between the new entry and the existing one on the same inputs, as int32 bit patterns."""
import ctypes as C

import pytest
import torch

from conftest import load_sub

pytestmark = pytest.mark.gpu
CL = torch.channels_last

# N = 2 images of 12 x 12 as two stacked BatchNorm groups: G = 2, L = 144, M = 288 - the group boundary falls inside the second 128-row
# tile (and inside the third 64-row one), the last tile is ragged
N, H, W, G = 2, 12, 12, 2
L = (N // G) * H * W


def bits(t):
    return t.contiguous(memory_format=CL).view(torch.int32) if t.dim() == 4 else t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def _valid_records_equal(a, b, c, bm):
    """The records [G][chunks][C][2] (fp64) two launches left, bit for bit.  Group g owns one record per tile row that holds rows of it
    (chunk = tile row - the first such tile row); the slots behind them are never written (and never read by the finalize)."""
    a, b = a.view(torch.int64).view(G, -1, c, 2), b.view(torch.int64).view(G, -1, c, 2)
    assert a.shape == b.shape and a.shape[1] == -(-L // bm) + 1
    ok = True
    for g in range(G):
        used = ((g + 1) * L - 1) // bm - (g * L) // bm + 1
        ok = ok and bool((a[g, :used] == b[g, :used]).all())
    return ok


def _unit(F, dev, c, k, r, variant, seed):
    """A ReLU unit's tensors (z = relu(norm(nx) [+ residual]) over two groups) and the consumer conv's operands."""
    g = torch.Generator(device=dev).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)
    w = (rn(k, c, r, r) * (1.0 / (c * r * r) ** 0.5)).contiguous(memory_format=CL)
    dy = rn(N, k, H, W).contiguous(memory_format=CL)
    nx = (rn(N, c, H, W) * 1.7 + 0.3).contiguous(memory_format=CL)
    gamma, beta = (rn(c) * 0.3 + 1.0), rn(c) * 0.2
    res = variant != "plain"
    resid = rn(N, c, H, W).contiguous(memory_format=CL) if res else None
    addend = rn(N, c, H, W).contiguous(memory_format=CL) if variant == "res_add" else None
    mean, rstd = F.norm_stats(nx, G)
    z = F.norm_apply(nx, mean, rstd, gamma, beta, resid, G, F.ACT_RELU)
    return w, dy, nx, gamma, beta, mean, rstd, z, res, addend


@pytest.mark.parametrize("variant", ["res_add", "res", "plain"])
@pytest.mark.parametrize("kern", [(1, 0, 1), (3, 2, 2)], ids=["1x1", "3x3_d2"])
@pytest.mark.parametrize("cls", [0, 1, 2, 3], ids=["128x128", "64x64", "128x64", "128x32"])
def test_masked_store_equals_the_apply_pass_mask_bit_for_bit(cls, kern, variant, F, dev):
    """Every data-gradient tile class (forced through the descriptor's tuning field), C = 64 / 128 / 256 gradient channels, K = 64 / 256
    reduction channels, 1x1 and dilated 3x3, {residual + addend, residual, no residual}: same records; dx_masked = where(z > 0, dx, +0)
    with no negative zero; the unit's backward finished from either dx gives the same input gradient, d gamma, d beta; the old dres IS
    dx_masked."""
    r, pad, dil = kern
    F.set_conv_precision("f32s")
    old = F.tuning(tile_class=cls)
    try:
        for c in (64, 128, 256):
            for k in (64, 256):
                w, dy, nx, gamma, beta, mean, rstd, z, res, addend = _unit(F, dev, c, k, r, variant, 1000 * cls + 10 * c + k + r)
                wt = F.dgrad_operand(w, z.shape, 1, pad, dil)
                info = (nx, mean, rstd, gamma, beta, (G, L, c), F.ACT_RELU, 0.0) + ((True,) if res else ())
                dx, rec, joined = F.conv2d_dgrad(dy, wt, z.shape, w.shape, 1, pad, dil, bsums=info, addend=addend, z=z)
                dxm, recm, joinedm = F.conv2d_dgrad(dy, wt, z.shape, w.shape, 1, pad, dil, bsums=info, addend=addend, z=z, premask=True)
                tag = "C %d K %d" % (c, k)
                assert rec is not None and recm is not None, "the fused route must serve this shape (%s)" % tag
                assert joined == joinedm == (addend is not None), tag
                assert _valid_records_equal(rec[1], recm[1], c, (128, 64, 128, 128)[cls]), "records differ (%s)" % tag
                want = torch.where(z > 0, dx, torch.zeros_like(dx))
                assert same_bits(dxm, want), "dx_masked != where(z > 0, dx, +0) (%s)" % tag
                assert not bool(((bits(dxm) == -2 ** 31)).any()), "a negative zero was stored (%s)" % tag
                assert bool((z > 0).any()) and bool((z <= 0).any())
                dgb = torch.empty((2, 2, c), dtype=torch.float32, device=dev)
                dnx, dres = F.norm_bwd_from_sums(rec, dx, nx, mean, rstd, gamma, beta, G, F.ACT_RELU, 0.0, dgb[0, 0], dgb[0, 1],
                                                 y=z if res else None, want_dres=res)
                dnxm, dresm = F.norm_bwd_from_sums(recm, dxm, nx, mean, rstd, gamma, beta, G, F.ACT_NONE, 0.0, dgb[1, 0], dgb[1, 1])
                assert dresm is None
                assert same_bits(dnx, dnxm), "input gradient (%s)" % tag
                assert same_bits(dgb[0], dgb[1]), "d gamma / d beta (%s)" % tag
                if res:
                    assert same_bits(dres, dxm), "the apply pass's dres != dx_masked (%s)" % tag
    finally:
        F.TUNING[0], F.WGRAD_TUNING[0] = old
        F.set_conv_precision("f32")


def test_masked_entry_refuses_leaky_relu(F, dev):
    """A 0 / 1 mask may be applied twice, LeakyReLU's may not: SSCG_ERR_UNSUPPORTED from the C entry, an error from the Python one."""
    L_ = load_sub("_lib")
    c, k = 64, 64
    F.set_conv_precision("f32s")
    try:
        w, dy, nx, gamma, beta, mean, rstd, z, res, addend = _unit(F, dev, c, k, 1, "res", 7)
        wt = F.dgrad_operand(w, z.shape, 1, 0, 1)
        info = (nx, mean, rstd, gamma, beta, (G, L, c), F.ACT_RELU, 0.0, True)
        dx, rec, _ = F.conv2d_dgrad(dy, wt, z.shape, w.shape, 1, 0, 1, bsums=info, z=z)
        d, sums = rec[0], rec[1]
        ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
        args = lambda act: (C.byref(d), dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), nx.data_ptr(), z.data_ptr(), None, mean.data_ptr(),
                            rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), G, L, act, 0.2, sums.data_ptr(), sums.numel(), ws.data_ptr(),
                            ws.numel(), None)
        before = dx.clone()
        assert L_.lib.sscg_conv2d_dgrad_bsums_masked(*args(F.ACT_LRELU)) == -2
        assert L_.lib.sscg_conv2d_dgrad_bsums_masked(*args(F.ACT_NONE)) == -2
        torch.cuda.synchronize()
        assert torch.equal(dx, before)          # nothing ran
        linfo = info[:6] + (F.ACT_LRELU, 0.2, True)
        with pytest.raises(L_.SscgError):
            F.conv2d_dgrad(dy, wt, z.shape, w.shape, 1, 0, 1, bsums=linfo, z=z, premask=True)
    finally:
        F.set_conv_precision("f32")


# ------------------------------------------------------------------------------------------------------------------- autograd level
def _bottleneck_grads(F, dev, blocks, x0, gys, premask, second_consumer, spy=None):
    gen_params = [p for b in blocks for p in b.parameters() if p.requires_grad]
    arch = load_sub("arch")
    was, real = F.PREMASK[0], F._norm_backward
    F.PREMASK[0] = premask
    if spy is not None:
        def wrapped(dy, *a, **kk):
            out = real(dy, *a, **kk)
            spy.append((dy, out[3], a[-1]))
            return out
        F._norm_backward = wrapped
    try:
        for p in gen_params:
            p.grad = None
        for b in blocks:
            for bn in (b.bn1, b.bn2, b.bn3):
                bn.running_mean.zero_(); bn.running_var.fill_(1.0)
        x = x0.clone().requires_grad_(True)
        with arch.batch_groups(G):
            y1 = blocks[0](x)
            y2 = blocks[1](y1)
        loss = (y2 * gys[0]).sum()
        if second_consumer:             # y1 is read outside block 2's fan-out too: the engine accumulates, block 1's records are dropped
            loss = loss + (y1 * gys[1]).sum()
        F.backward(loss)
        F.SideStream.join(dev)
        torch.cuda.synchronize()
        return [x.grad.clone()] + [p.grad.clone() for p in gen_params]
    finally:
        F.PREMASK[0] = was
        F._norm_backward = real


@pytest.fixture(scope="module")
def chain(dev):
    gen = load_sub("arch.generators")
    torch.manual_seed(23)
    blocks = [gen.Bottleneck(256, 64).to(dev) for _ in range(2)]
    x0 = torch.randn(N, 256, H, W).to(dev).contiguous(memory_format=CL)
    gys = [torch.randn(N, 256, H, W).to(dev).contiguous(memory_format=CL) for _ in range(2)]
    return blocks, x0, gys


@pytest.mark.parametrize("second_consumer", [False, True], ids=["chain", "second_consumer"])
def test_two_bottlenecks_bitwise_equal_with_premask_on_and_off(second_consumer, chain, F, dev):
    """Two chained Bottlenecks (64 planes, 256 channels, two BatchNorm groups of 144 rows): the gradients of the input and of every
    parameter are the same bits with PREMASK on and off - also when the first block's output has a second consumer outside the join,
    so that autograd accumulates into the masked gradient, the records are dropped and the ordinary pass masks a second time."""
    blocks, x0, gys = chain
    on = _bottleneck_grads(F, dev, blocks, x0, gys, True, second_consumer)
    off = _bottleneck_grads(F, dev, blocks, x0, gys, False, second_consumer)
    assert len(on) == len(off) == 7
    for i, (a, b) in enumerate(zip(on, off)):
        assert same_bits(a, b), "gradient %d differs between PREMASK on and off" % i


def test_residual_gradient_is_the_incoming_gradient_object(chain, F, dev):
    """With PREMASK on the bn3 + shortcut -> ReLU unit of block 1 (its upstream gradient comes masked from block 2's conv1) allocates no
    residual gradient: the dres it returns is the tensor it was handed.  Block 2's own bn3 unit (gradient from the loss, no records)
    and every unit with PREMASK off still write one."""
    blocks, x0, gys = chain
    for premask, aliased in ((True, 1), (False, 0)):
        seen = []
        real_sums, calls = F.norm_bwd_from_sums, []
        F.norm_bwd_from_sums = lambda *a, **kk: (calls.append((a[8], kk.get("want_dres", False))), real_sums(*a, **kk))[1]
        try:
            _bottleneck_grads(F, dev, blocks, x0, gys, premask, False, spy=seen)
        finally:
            F.norm_bwd_from_sums = real_sums
        res_units = [(dy, dres) for dy, dres, want in seen if want]
        assert len(seen) == 6 and len(res_units) == 2
        assert sum(1 for dy, dres in res_units if dres is dy) == aliased
        assert all(dres is not None and dres.shape == dy.shape for dy, dres in res_units)
        # five units finish from the records (all but block 2's bn3); with PREMASK every one of them runs maskless and writes no dres
        assert len(calls) == 5
        if premask:
            assert all(act == F.ACT_NONE and not want for act, want in calls), calls
        else:
            assert sum(1 for act, want in calls if want) == 1 and all(act == F.ACT_RELU for act, _ in calls), calls
