"""Soft Dice loss on the MI355X: sscg_dice_fwd / sscg_dice_bwd (flat), the resized statistics and sscg_upsample_head_bwd_d (the fused
label head with the Dice branch), against the definition written with torch ops in fp64 on the CPU (tests/test_dice_host.py's
dice_reference: F.interpolate(align_corners=True) -> softmax -> sums -> loss, gradient by autograd).

Tolerance (README): 1e-3 relative for an fp32 loss against the fp64 reference; for a gradient the max-abs difference
over the max-abs of the reference gradient.  Two absolute floors, as in tests/test_weighted_ce_gpu.py, cover references that are exactly
zero (C = 1: p = 1, the loss and every gradient entry vanish): 1e-7 on a loss, and 8 fp32 roundings of max(|A|, |B|), the largest term
of a gradient entry (taken over the groups that have a counted pixel: the table of a void-only group multiplies nothing), on a gradient.
Where a total gradient also carries a cross-entropy term, that term brings that file's own floor with it - 8 fp32 roundings of
max(w) / D - each floor times the weight its term has in the total (the smoothed cross entropy of the existing head leaves O(1e-9)
where the reference is exactly 0 at C = 1).
Every test prints the distances it observed (`dice ...` lines; run with -s); profiles/dice.txt keeps them."""
import contextlib
import io
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as TF

from conftest import ROOT, load_sub
from test_dice_host import CLASSES, GEOMS, dice_reference, make_labels, make_weights

pytestmark = pytest.mark.gpu

CL = torch.channels_last
EPS32 = 2.0 ** -23


def gpu(t, dev):
    return t.float().to(dev).contiguous(memory_format=CL) if t.dim() == 4 else t.float().to(dev)


def ce_reference(logits64, lab, w32, eps, resize=None):
    """(loss, gradient) of torch's cross entropy in fp64 on the CPU, every label outside [0, C) mapped to the ignore index"""
    C = logits64.shape[1]
    x = logits64.clone().requires_grad_(True)
    up = x if resize is None else TF.interpolate(x, size=resize, mode="bilinear", align_corners=True)
    ref_lab = lab.clone()
    ref_lab[(lab < 0) | (lab >= C)] = -100
    loss = TF.cross_entropy(up, ref_lab, weight=None if w32 is None else w32.double(), label_smoothing=eps, ignore_index=-100)
    return loss.detach(), torch.autograd.grad(loss, x)[0]


def soft_reference(logits64, R64, resize):
    """gradient of sum(softmax(interp(x)) * R) in fp64"""
    x = logits64.clone().requires_grad_(True)
    up = TF.interpolate(x, size=resize, mode="bilinear", align_corners=True)
    return torch.autograd.grad((torch.softmax(up, 1) * R64).sum(), x)[0]


def ab_floor(ref):
    live = ref["sums"][:, :, 2].sum(1) > 0                  # groups with a counted pixel (all of them if there is none)
    A, B = (ref["A"][live], ref["B"][live]) if live.any() else (ref["A"], ref["B"])
    return 8 * EPS32 * max(float(A.abs().max()), float(B.abs().max()))


def ce_floor(lab, w32, C):
    """tests/test_weighted_ce_gpu.py's floor of a cross-entropy gradient: 8 fp32 roundings of max(w) / D"""
    counted = lab[(lab >= 0) & (lab < C)]
    D = float(counted.numel()) if w32 is None else float(w32.double()[counted].sum())
    return 8 * EPS32 * (1.0 if w32 is None else float(w32.max())) / D


def check_loss(tag, loss, ref_loss):
    loss, ref_loss = float(loss.detach()), float(ref_loss)
    d = abs(loss - ref_loss)
    print("dice %-58s loss %.9g ref %.9g rel %.2e" % (tag, loss, ref_loss, d / max(abs(ref_loss), 1e-30)))
    assert math.isfinite(loss) and d <= 1e-3 * abs(ref_loss) + 1e-7, (tag, loss, ref_loss)


def check_grad(tag, grad, ref_grad, floor):
    grad = grad.detach().double().cpu()
    dg, gmax = float((grad - ref_grad).abs().max()), float(ref_grad.abs().max())
    print("dice %-58s grad max-abs diff %.2e of %.2e rel %.2e (floor %.1e)" % (tag, dg, gmax, dg / max(gmax, 1e-30), floor))
    assert torch.isfinite(grad).all() and dg <= 1e-3 * gmax + floor, (tag, dg, gmax)


def check_sums(tag, sums, ref):
    """T exactly; I and P to 1e-6 relative"""
    s, r = sums.cpu(), ref["sums"]
    assert s.dtype == torch.float64 and s.shape == r.shape, (tag, s.shape, r.shape)
    assert torch.equal(s[:, :, 2], r[:, :, 2]), tag
    worst = 0.0
    for k in (0, 1):
        d = (s[:, :, k] - r[:, :, k]).abs()
        assert (d <= 1e-6 * r[:, :, k].abs()).all(), (tag, "IP"[k], float(d.max()))
        nz = r[:, :, k] > 0
        if nz.any():
            worst = max(worst, float((d[nz] / r[:, :, k][nz]).max()))
    print("dice %-58s sums: T exact, I / P rel <= %.2e" % (tag, worst))


def dice_weight_dev(F, w32, C, dev):
    return None if w32 is None else F.dice_weight(w32.tolist(), C, dev)


# ------------------------------------------------------------------------------------------ 1. flat Dice
@pytest.mark.parametrize("C", CLASSES)
def test_flat_dice_value_gradient_sums(C, F, dev):
    g = torch.Generator().manual_seed(100 + C)
    x = torch.randn(2, C, 7, 9, generator=g, dtype=torch.float64) * 2
    lab = make_labels(g, (2, 7, 9), C)
    assert (lab == 255).any() and (lab == -100).any() and (lab[1] == 255).all()
    wts = make_weights(g, C)
    for batch in (False, True):
        for s in (1.0, 1e-5):
            for w32 in (None, wts):
                tag = "flat C=%d batch=%d s=%g w=%s" % (C, batch, s, "w" if w32 is not None else None)
                ref = dice_reference(x, lab, w32, s, batch)
                assert C == 1 or 0.2 < float(ref["loss"]) < 1.0
                xg = gpu(x, dev).requires_grad_(True)
                wd = dice_weight_dev(F, w32, C, dev)
                loss = F.dice_loss(xg, lab.to(dev), weight=wd, smooth=s, batch=batch)
                F.weighted_sum([loss], [0.37]).backward()                  # the upstream gradient scales it
                check_loss(tag, loss, ref["loss"])
                check_grad(tag, xg.grad / 0.37, ref["grad"], ab_floor(ref))
                assert torch.count_nonzero(xg.grad[1]) == 0                 # the void-only sample
                l2, coef, sums = F.dice_fwd(xg.detach(), lab.to(dev), (7, 9), wd, s, batch, want_sums=True)
                assert torch.equal(l2, loss.detach())
                check_sums(tag, sums, ref)
                cf = coef.double().cpu()
                assert torch.allclose(cf[:, :, 0], ref["A"], rtol=1e-5, atol=0) and torch.allclose(cf[:, :, 1], ref["B"], rtol=1e-5, atol=0)


# ------------------------------------------------------------------------------------------ 2. the fused head
def raw_head_plain(F, dev, x_nhwc, lab, w, eps, OH, OW, want_soft, labels=True):
    """sscg_upsample_head_fwd[_w] alone on fresh outputs: (loss, valid, dlogits, y_soft)"""
    lib = F.lib
    N, H, W, C = x_nhwc.shape
    loss, valid = torch.full((1,), 7.0, device=dev), torch.full((1,), 7.0, device=dev)
    dl = torch.full((N, H, W, C), 7.0, device=dev)
    y = torch.full((N, OH, OW, C), 7.0, device=dev) if want_soft else None
    ws = torch.zeros(lib.sscg_upsample_head_workspace(N, H, W), dtype=torch.uint8, device=dev)
    yp = y.data_ptr() if want_soft else None
    if w is not None or eps:
        rc = lib.sscg_upsample_head_fwd_w(x_nhwc.data_ptr(), lab.data_ptr(), None if w is None else w.data_ptr(), eps, yp, loss.data_ptr(),
                                          valid.data_ptr(), dl.data_ptr(), N, H, W, C, OH, OW, ws.data_ptr(), ws.numel(), F._stream())
    else:
        rc = lib.sscg_upsample_head_fwd(x_nhwc.data_ptr(), lab.data_ptr() if labels else None, yp, loss.data_ptr(), valid.data_ptr(),
                                        dl.data_ptr(), N, H, W, C, OH, OW, ws.data_ptr(), ws.numel(), F._stream())
    assert rc == 0
    torch.cuda.synchronize()
    return loss, valid, dl, y


def raw_dice_fwd(F, dev, x_nhwc, lab, OH, OW, w, s, batch):
    """sscg_dice_fwd itself on sentinel-guarded outputs: (loss, sums [G, C, 3], coef [G, C, 2])"""
    lib = F.lib
    N, H, W, C = x_nhwc.shape
    G = 1 if batch else N
    gl, gs, gc = torch.full((33,), 7.0, device=dev), torch.full((G * C * 3 + 32,), 7.0, device=dev, dtype=torch.float64), torch.full((G * C * 2 + 32,), 7.0, device=dev)
    loss, sums, coef = gl[16:17], gs[16:16 + G * C * 3], gc[16:16 + G * C * 2]
    nbytes = lib.sscg_dice_workspace(N, OH, OW, C)
    ws = torch.full((nbytes + 256,), 0x5A, dtype=torch.uint8, device=dev)
    rc = lib.sscg_dice_fwd(x_nhwc.data_ptr(), lab.data_ptr(), N, H, W, C, OH, OW, None if w is None else w.data_ptr(), s, 1 if batch else 0,
                           loss.data_ptr(), sums.data_ptr(), coef.data_ptr(), ws.data_ptr(), nbytes, F._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert (gl[:16] == 7).all() and (gl[17:] == 7).all() and (gs[:16] == 7).all() and (gs[-16:] == 7).all()
    assert (gc[:16] == 7).all() and (gc[-16:] == 7).all() and (ws[nbytes:] == 0x5A).all()
    return loss.clone().reshape(()), sums.clone().view(G, C, 3), coef.clone().view(G, C, 2)


def scalar(v, dev):
    return torch.full((), float(v), device=dev)


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("geom", GEOMS)
def test_fused_head_losses_and_gradient(geom, C, F, dev):
    N, H, W, OH, OW = geom
    g = torch.Generator().manual_seed(1000 * C + H * W)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 2
    lab = make_labels(g, (N, OH, OW), C)                       # class C-1 is absent; for N = 2 sample 1 is entirely void
    assert C == 1 or not (lab == C - 1).any()
    w_ce, w_d = make_weights(g, C), make_weights(g, C)
    R = torch.randn(N, C, OH, OW, generator=g, dtype=torch.float64)
    labd, Rg = lab.to(dev), gpu(R, dev)
    xg0 = gpu(x, dev)
    assert F._head_applies(xg0, OH, OW)
    y_plain = F.UpsampleHeadFn.apply(xg0, OH, OW, None, True)[0]
    soft_grad = soft_reference(x, R, (OH, OW))
    geo = "%dx%dx%d->%dx%d C=%d" % (N, H, W, OH, OW, C)
    #            tag          CE?    CE weights, eps   Dice: weights, smooth, batch
    configs = [("dice only", False, None, 0.0, None, 1.0, False),
               ("dice+ce", True, None, 0.0, w_d, 1e-5, True),
               ("dice+wce", True, w_ce if C > 1 else None, 0.1, w_d, 1.0, False)]
    for name, want_ce, cw, eps, dw, s, batch in configs:
        ref = dice_reference(x, lab, dw, s, batch, resize=(OH, OW))
        ce_ref = ce_reference(x, lab, cw, eps, resize=(OH, OW)) if want_ce else None
        assert C == 1 or 0.2 < float(ref["loss"]) < 1.0
        cwd = None if cw is None else F.ce_weight(cw.tolist(), C, dev)
        opts = F.DiceOptions(weight=dice_weight_dev(F, dw, C, dev), smooth=s, batch=batch, ce=want_ce)
        for soft in (True, False):
            tag = "head %s %s soft=%d" % (geo, name, soft)
            xg = gpu(x, dev).requires_grad_(True)
            y, ce, d = F.upsample_softmax_ce_dice(xg, (OH, OW), labd, want_soft=soft, weight=cwd, label_smoothing=eps, dice=opts)
            assert (y is not None) == soft and (ce is not None) == want_ce
            valid = d.grad_fn.saved_tensors[3]                  # (read before the backward frees it)
            total, want, floor = 0.7 * d, 0.7 * ref["grad"], 0.7 * ab_floor(ref)
            if want_ce:
                total, want, floor = total + 1.3 * ce, want + 1.3 * ce_ref[1], floor + 1.3 * ce_floor(lab, cw, C)
            if soft:
                total, want = total + (y * Rg).sum(), want + soft_grad
            total.backward()
            check_loss(tag, d, ref["loss"])
            check_grad(tag, xg.grad, want, floor)
            if soft:
                assert torch.equal(y.detach(), y_plain)          # the softmax branch: the plain head's bits
            if want_ce:
                check_loss(tag + " (CE)", ce, ce_ref[0])
                # with Dice on, the cross entropy and `valid` are those of the head's own entry alone: the same bits
                pl, pv, _, _ = raw_head_plain(F, dev, xg.detach().permute(0, 2, 3, 1), labd, cwd, eps, OH, OW, soft)
                assert torch.equal(ce.detach().reshape(1), pl) and torch.equal(valid.reshape(1), pv), tag
            else:
                assert valid is None
            if N == 2 and not soft:
                assert torch.count_nonzero(xg.grad[1]) == 0       # the void-only sample: neither loss reaches it
    # the raw ABI: every branch of sscg_upsample_head_bwd_d in one call, on sentinel-guarded outputs
    xh = xg0.permute(0, 2, 3, 1)
    assert xh.is_contiguous()
    name, _, cw, eps, dw, s, batch = configs[2]
    cwd, dwd = (None if cw is None else F.ce_weight(cw.tolist(), C, dev)), dice_weight_dev(F, dw, C, dev)
    ref, ce_ref = dice_reference(x, lab, dw, s, batch, resize=(OH, OW)), ce_reference(x, lab, cw, eps, resize=(OH, OW))
    ce_loss, valid, dl, _ = raw_head_plain(F, dev, xh, labd, cwd, eps, OH, OW, False)
    dloss, sums, coef = raw_dice_fwd(F, dev, xh, labd, OH, OW, dwd, s, batch)
    check_loss("raw  %s" % geo, dloss, ref["loss"])
    check_sums("raw  %s" % geo, sums, ref)
    dyn = Rg.permute(0, 2, 3, 1).contiguous()
    g_ce, g_dice = scalar(1.3, dev), scalar(0.7, dev)             # (held: a temporary's block would be handed to the next allocation)
    for branches, use_soft, use_ce in (("soft + CE + Dice", True, True), ("CE + Dice", False, True), ("soft + Dice", True, False),
                                       ("Dice only", False, False)):
        guard = torch.full((N * H * W * C + 64,), 7.0, device=dev)
        dx = guard[32:32 + N * H * W * C]
        rc = F.lib.sscg_upsample_head_bwd_d(xh.data_ptr(), labd.data_ptr(), dyn.data_ptr() if use_soft else None, dl.data_ptr() if use_ce else None,
                                            g_ce.data_ptr() if use_ce else None, valid.data_ptr() if use_ce else None, coef.data_ptr(),
                                            g_dice.data_ptr(), 1 if batch else 0, dx.data_ptr(), N, H, W, C, OH, OW, F._stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert (guard[:32] == 7).all() and (guard[-32:] == 7).all()
        want = 0.7 * ref["grad"] + (1.3 * ce_ref[1] if use_ce else 0) + (soft_grad if use_soft else 0)
        floor = 0.7 * ab_floor(ref) + (1.3 * ce_floor(lab, cw, C) if use_ce else 0.0)
        check_grad("raw  %s %s" % (geo, branches), dx.view(N, H, W, C).permute(0, 3, 1, 2), want, floor)


# ------------------------------------------------------------------------------------------ 3. fused against flat
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("geom", GEOMS)
def test_resized_statistics_equal_the_flat_ones_bit_for_bit(geom, C, F, dev):
    """sscg_dice_fwd with the resize against the identity call on F.upsample_bilinear's materialised output: the same kernel, the same
    pixel-to-thread map, the pinned resize arithmetic - loss, sums and coef bit for bit.  The gradients (fused stencil against
    upsample_bwd(dice_bwd)) agree within the tolerance."""
    N, H, W, OH, OW = geom
    g = torch.Generator().manual_seed(31 * C + H)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 2
    lab = make_labels(g, (N, OH, OW), C)
    wts = make_weights(g, C)
    labd = lab.to(dev)
    for batch, s, w32 in ((False, 1.0, None), (True, 1e-5, wts)):
        wd = dice_weight_dev(F, w32, C, dev)
        xg = gpu(x, dev)
        up = F.upsample_bilinear(xg, (OH, OW))
        assert up.shape == (N, C, OH, OW)
        fused = F.dice_fwd(xg, labd, (OH, OW), wd, s, batch, want_sums=True)
        flat = F.dice_fwd(up, labd, (OH, OW), wd, s, batch, want_sums=True)
        for a, b in zip(fused, flat):
            assert torch.equal(a, b)
        ref = dice_reference(x, lab, w32, s, batch, resize=(OH, OW))
        grads = []
        for fuse in (True, False):
            was = F.FUSE_HEAD[0]
            F.FUSE_HEAD[0] = fuse
            try:
                xr = gpu(x, dev).requires_grad_(True)
                _, ce, d = F.upsample_softmax_ce_dice(xr, (OH, OW), labd, want_soft=False, dice=F.DiceOptions(wd, s, batch, ce=False))
                assert ce is None and torch.equal(d.detach(), fused[0])
                d.backward()
                grads.append(xr.grad)
            finally:
                F.FUSE_HEAD[0] = was
        tag = "fused-vs-flat %dx%dx%d->%dx%d C=%d batch=%d" % (N, H, W, OH, OW, C, batch)
        check_grad(tag + " fused", grads[0], ref["grad"], ab_floor(ref))
        check_grad(tag + " separate", grads[1], ref["grad"], ab_floor(ref))
        check_grad(tag + " fused vs separate", grads[0], grads[1].double().cpu(), ab_floor(ref))


# ------------------------------------------------------------------------------------------ 4. the void-only sample
def test_void_only_sample(F, dev):
    N, H, W, OH, OW, C = 2, 3, 4, 13, 17, 4
    g = torch.Generator().manual_seed(77)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 2
    lab = make_labels(g, (N, OH, OW), C, absent=False)
    assert (lab[1] == 255).all()
    labd = lab.to(dev)
    for s in (1.0, 1e-5):
        xg = gpu(x, dev).requires_grad_(True)
        loss, coef, sums = F.dice_fwd(xg.detach(), labd, (OH, OW), None, s, False, want_sums=True)
        assert torch.count_nonzero(sums[1]) == 0                                # I = P = T = 0: dice = s / s = 1 for every class
        dice = (2 * sums[:, :, 0] + s) / (sums[:, :, 1] + sums[:, :, 2] + s)
        assert torch.equal(dice[1], torch.ones(C, dtype=torch.float64, device=dev)) and math.isfinite(float(loss))
        _, _, d = F.upsample_softmax_ce_dice(xg, (OH, OW), labd, want_soft=False, dice=F.DiceOptions(smooth=s, ce=False))
        d.backward()
        assert torch.count_nonzero(xg.grad[1]) == 0 and torch.count_nonzero(xg.grad[0]) > 0
        check_loss("void sample s=%g" % s, d, dice_reference(x, lab, None, s, False, resize=(OH, OW))["loss"])
        # batch=True: the other sample alone decides the result
        both = F.dice_fwd(xg.detach(), labd, (OH, OW), None, s, True, want_sums=True)
        alone = F.dice_fwd(xg.detach()[:1], labd[:1], (OH, OW), None, s, True, want_sums=True)
        for a, b in zip(both, alone):
            assert torch.equal(a, b)
        xb = gpu(x, dev).requires_grad_(True)
        F.upsample_softmax_ce_dice(xb, (OH, OW), labd, want_soft=False, dice=F.DiceOptions(smooth=s, batch=True, ce=False))[2].backward()
        xa = gpu(x[:1], dev).requires_grad_(True)
        F.upsample_softmax_ce_dice(xa, (OH, OW), labd[:1], want_soft=False, dice=F.DiceOptions(smooth=s, batch=True, ce=False))[2].backward()
        assert torch.equal(xb.grad[:1], xa.grad) and torch.count_nonzero(xb.grad[1]) == 0
    # no counted pixel at all: loss 0 (every dice is 1), finite, zero gradient - flat and fused
    void = torch.full((N, OH, OW), 255, dtype=torch.int64, device=dev)
    xg = gpu(x, dev).requires_grad_(True)
    _, _, d = F.upsample_softmax_ce_dice(xg, (OH, OW), void, want_soft=False, dice=F.DiceOptions(ce=False))
    d.backward()
    assert abs(float(d)) <= 1e-7 and torch.count_nonzero(xg.grad) == 0
    up = gpu(torch.randn(N, C, OH, OW, generator=g), dev).requires_grad_(True)
    d = F.dice_loss(up, void)
    d.backward()
    assert abs(float(d)) <= 1e-7 and torch.count_nonzero(up.grad) == 0


# ------------------------------------------------------------------------------------------ 5. determinism
@pytest.mark.parametrize("C", [4, 21])
def test_the_same_call_twice_gives_the_same_bits(C, F, dev):
    N, H, W, OH, OW = 2, 9, 11, 67, 83            # 22 statistics blocks per sample, a ragged last one
    g = torch.Generator().manual_seed(5 + C)
    x = torch.randn(N, C, H, W, generator=g) * 2
    lab = make_labels(g, (N, OH, OW), C)
    lab[1] = torch.randint(0, C, (OH, OW), generator=g)
    R = gpu(torch.randn(N, C, OH, OW, generator=g), dev)
    labd, wd = lab.to(dev), F.dice_weight(make_weights(g, C).tolist(), C, dev)
    runs = []
    for _ in range(2):
        out = []
        for batch in (False, True):
            xg = gpu(x, dev).requires_grad_(True)
            out += list(F.dice_fwd(xg.detach(), labd, (OH, OW), wd, 1.0, batch, want_sums=True))
            y, ce, d = F.upsample_softmax_ce_dice(xg, (OH, OW), labd, dice=F.DiceOptions(wd, 1.0, batch))
            (d + ce + (y * R).sum()).backward()
            out += [y.detach(), ce.detach(), d.detach(), xg.grad]
            up = F.upsample_bilinear(xg.detach(), (OH, OW)).requires_grad_(True)
            fl = F.dice_loss(up, labd, wd, 1.0, batch)
            fl.backward()
            out += [fl.detach(), up.grad]
        runs.append(out)
    assert len(runs[0]) == 18 and all(torch.equal(a, b) for a, b in zip(*runs))


# ------------------------------------------------------------------------------------------ 6. past the caps
@pytest.mark.parametrize("case", ["grid cap", "finish block", "backward cap"])
def test_past_the_caps(case, F, dev):
    """C = 4 (the host reference stays in seconds), flat, ragged tails; outputs guarded by sentinels on both sides.
      grid cap:      363 x 363 = 131769 pixels > 2 * 256 blocks * 256 threads: every thread takes 2 pixels, 697 of them a third
      finish block:  3 samples x 89 blocks = 267 records of the one group (batch) > a block's 256 threads, 89 > the 85 row lanes of the
                     per-sample reduction; 150 x 151 % 256 = 122
      backward cap:  1449 x 1449 = 2099601 pixels > the flat backward's 8192 blocks * 256 threads (and 33 pixels per statistics thread)"""
    C = 4
    N, H, W, batch = {"grid cap": (1, 363, 363, False), "finish block": (3, 150, 151, True), "backward cap": (1, 1449, 1449, False)}[case]
    lib = F.lib
    assert lib.sscg_dice_workspace(N, H, W, C) == N * (min((H * W + 255) // 256, 256) + 1) * C * 3 * 8
    if case == "grid cap":
        assert H * W > 2 * 256 * 256 and (H * W) % 256
    if case == "finish block":
        assert N * ((H * W + 255) // 256) > 256 and (H * W) % 256
    if case == "backward cap":
        assert H * W > 8192 * 256 and (H * W) % 256
    g = torch.Generator().manual_seed(len(case))
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 2
    lab = make_labels(g, (N, H, W), C)
    wts = make_weights(g, C)
    ref = dice_reference(x, lab, wts, 1.0, batch)
    xh = gpu(x, dev).permute(0, 2, 3, 1)
    labd, wd = lab.to(dev), F.dice_weight(wts.tolist(), C, dev)
    loss, sums, coef = raw_dice_fwd(F, dev, xh, labd, H, W, wd, 1.0, batch)
    tag = "caps %s %dx%dx%d" % (case, N, H, W)
    check_loss(tag, loss, ref["loss"])
    check_sums(tag, sums, ref)
    rows = N * H * W
    guard = torch.full((rows * C + 64,), 7.0, device=dev)
    dx = guard[32:32 + rows * C]
    rc = lib.sscg_dice_bwd(xh.data_ptr(), labd.data_ptr(), N, H, W, C, coef.data_ptr(), 1 if batch else 0, None, 0.37, dx.data_ptr(), F._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert (guard[:32] == 7).all() and (guard[-32:] == 7).all()
    check_grad(tag, dx.view(N, H, W, C).permute(0, 3, 1, 2) / 0.37, ref["grad"], ab_floor(ref))


# ------------------------------------------------------------------------------------------ 8. through the model
def _args(dev, tmp_path, **kw):
    FX = __import__("oracle.fixtures", fromlist=["x"])
    return FX.make_args(dataset="acdc", crop_height=64, crop_width=64, batch_size=2, gpu_ids=[dev.index or 0], ngf=8, ndf=8,
                        checkpoint_dir=str(tmp_path / "ckpt"), as_written=True, **kw)


def test_supervised_step_reports_torchs_ce_and_dice(F, dev, tmp_path):
    md, data = load_sub("model"), load_sub("data")
    args = _args(dev, tmp_path, model="supervised_model", dice_weight=0.5, dice_skip="0", dice_smooth=1.0)
    torch.manual_seed(21)
    with contextlib.redirect_stdout(io.StringIO()):
        m = md.supervised_model(args)
        loader = data.synthetic_loaders(args, 4, steps=2)[0]
    assert m.dice_w == 0.5 and m.dice_options.weight.tolist() == [0.0, 1.0, 1.0, 1.0]
    l_img, l_gt, _ = next(iter(loader))
    l_img, l_gt = l_img.to(dev), l_gt.to(dev)
    with torch.no_grad():
        logits = m.Gsi(l_img).float().cpu()
    before = [p.detach().clone() for p in m.Gsi.parameters()]
    ce = float(m.step(l_img, l_gt))
    dice = float(m.extras["dice_loss"])
    lab = l_gt.cpu().squeeze(1)
    ce_ref = float(ce_reference(logits.double(), lab, None, 0.0, resize=(64, 64))[0])
    d_ref = float(dice_reference(logits.double(), lab, torch.tensor([0.0, 1.0, 1.0, 1.0]), 1.0, False, resize=(64, 64))["loss"])
    print("dice supervised step: CE %.9g ref %.9g (rel %.2e); Dice %.9g ref %.9g (rel %.2e)" % (
        ce, ce_ref, abs(ce - ce_ref) / abs(ce_ref), dice, d_ref, abs(dice - d_ref) / abs(d_ref)))
    assert abs(ce - ce_ref) <= 1e-3 * abs(ce_ref) and abs(dice - d_ref) <= 1e-3 * abs(d_ref) and 0.0 < dice <= 1.0
    assert any(not torch.equal(a, b) for a, b in zip(before, m.Gsi.parameters()))            # the update was applied


def test_semisupervised_step_takes_the_flag(F, dev, tmp_path):
    md, data = load_sub("model"), load_sub("data")
    got = {}
    for tag, kw in (("default", {}), ("dice", dict(dice_weight=0.5))):
        args = _args(dev, tmp_path, **kw)
        torch.manual_seed(22)
        with contextlib.redirect_stdout(io.StringIO()):
            m = md.semisuper_cycleGAN(args)
            labeled, unlabeled, _ = data.synthetic_loaders(args, 4, steps=1)
        (l_img, l_gt, _), (unl_img, _, _) = next(iter(labeled)), next(iter(unlabeled))
        torch.manual_seed(23)
        losses = m.step(l_img.to(dev), l_gt.to(dev), unl_img.to(dev))
        m.sync_losses()
        got[tag] = {k: float(v) for k, v in losses.items()}
        assert all(math.isfinite(v) for v in got[tag].values()), got[tag]
        F.flush_side_work()
        torch.cuda.synchronize()
    assert set(got["dice"]) - set(got["default"]) == {"lab_loss_dice", "gt_cycle_dice"} and set(got["default"]) == set(md.LOSS_KEYS)
    print("dice semisupervised step: lab_loss_dice %.6g, gt_cycle_dice %.6g; lab_loss_CE %.6g / %.6g, lab_loss_MSE %.6g / %.6g" % (
        got["dice"]["lab_loss_dice"], got["dice"]["gt_cycle_dice"], got["dice"]["lab_loss_CE"], got["default"]["lab_loss_CE"],
        got["dice"]["lab_loss_MSE"], got["default"]["lab_loss_MSE"]))
    assert 0.0 < got["dice"]["lab_loss_dice"] <= 1.0 and 0.0 < got["dice"]["gt_cycle_dice"] <= 1.0
    # the networks' first forward does not depend on the loss flags: the terms the flag cannot reach agree
    assert got["dice"]["lab_loss_MSE"] == pytest.approx(got["default"]["lab_loss_MSE"], rel=1e-3)
    assert got["dice"]["lab_loss_CE"] == pytest.approx(got["default"]["lab_loss_CE"], rel=1e-3)


# ------------------------------------------------------------------------------------------ 9. flags off: no new launch
CENSUS = r"""
import contextlib, io, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
from conftest import load_sub
md, data = load_sub("model"), load_sub("data")
FX = __import__("oracle.fixtures", fromlist=["x"])
dev = torch.device("cuda:0")
def args(**kw):
    return FX.make_args(dataset="acdc", crop_height=64, crop_width=64, batch_size=2, gpu_ids=[0], ngf=8, ndf=8, checkpoint_dir=%r,
                        as_written=True, **kw)
def batch(a):
    labeled, unlabeled, _ = data.synthetic_loaders(a, 4, steps=1)
    (l_img, l_gt, _), (unl_img, _, _) = next(iter(labeled)), next(iter(unlabeled))
    return l_img.to(dev), l_gt.to(dev), unl_img.to(dev)
for tag, kw in (("sup off", dict(model="supervised_model")), ("sup on", dict(model="supervised_model", dice_weight=0.5)), ("semi off", {})):
    a = args(**kw)
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        m = md.supervised_model(a) if tag.startswith("sup") else md.semisuper_cycleGAN(a)
    l_img, l_gt, unl_img = batch(a)
    torch.cuda.synchronize()
    sys.stderr.write("[census] begin %%s\n" %% tag)
    if tag.startswith("sup"):
        m.step(l_img, l_gt)
    else:
        m.step(l_img, l_gt, unl_img)
        m.sync_losses()
    load_sub("functional").flush_side_work()
    torch.cuda.synchronize()
    sys.stderr.write("[census] end %%s\n" %% tag)
"""


def test_flags_off_a_step_names_none_of_the_new_entries(tmp_path):
    env = dict(os.environ, SSCG_TRACE="1")
    for k in ("SSCG_RACECHECK", "SSCG_FUZZ", "SSCG_FUSE_HEAD"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", CENSUS % (ROOT, os.path.join(ROOT, "tests"), str(tmp_path / "ckpt"))], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    new = {"sscg_dice_workspace", "sscg_dice_fwd", "sscg_dice_bwd", "sscg_upsample_head_bwd_d"}
    calls = {}
    for tag in ("sup off", "sup on", "semi off"):
        body = r.stderr[r.stderr.index("[census] begin " + tag):r.stderr.index("[census] end " + tag)]
        names = [line[7:].split("(")[0] for line in body.splitlines() if line.startswith("[sscg] ")]
        calls[tag] = {n: names.count(n) for n in set(names)}
    assert calls["sup off"].get("sscg_upsample_head_fwd") == 1 and calls["sup off"].get("sscg_upsample_head_bwd") == 1
    assert not new & set(calls["sup off"]) and not new & set(calls["semi off"]), calls
    assert calls["semi off"].get("sscg_upsample_head_fwd") == 3 and calls["semi off"].get("sscg_upsample_head_bwd") == 3
    # the control: with the flag the log does name them - one Dice entry forward, ONE stencil launch backward
    on = calls["sup on"]
    assert on.get("sscg_dice_fwd") == 1 and on.get("sscg_upsample_head_bwd_d") == 1 and on.get("sscg_upsample_head_fwd") == 1
    assert "sscg_upsample_head_bwd" not in on and "sscg_dice_bwd" not in on
    # every other launch of the step is the one it was (host-side size / applies queries are cached per process: left out)
    def launches(c):
        return {k: v for k, v in c.items() if k not in new and k not in ("sscg_upsample_head_bwd", "sscg_weighted_sum")
                and not k.endswith(("_workspace", "_bytes", "_applies"))}
    assert launches(on) == launches(calls["sup off"]), (launches(on), launches(calls["sup off"]))
