"""Hard-pixel mining (OHEM) cross entropy on the MI355X: sscg_ohem_fwd (key pass, exact radix selection, loss), sscg_ce_bwd_ohem (flat)
and sscg_upsample_head_bwd_h (the fused label head), against tests/test_ohem_host.py's ohem_reference - the definition written with
torch ops in fp64 on the CPU.

What is compared with what:
  * the SELECTION is exact on the kernel's own keys: thr, counts and the sentinel bit for bit against torch.kthvalue of those keys;
  * the KEYS against fp64 within 4 e, e = the largest |fp32 - fp64| of the same keys computed by torch on the CPU (the reference
    arithmetic's own error, measured in the test; 1e-7 .. 4e-7 on these geometries);
  * the MASK against the reference's own mask everywhere except within 8 e of the fp64 threshold, where an fp32 key may fall on either
    side; that band may hold at most max(2, 0.1 % of V) pixels (the reference alone leaves 0 or 1 there: the rank pixel itself);
  * LOSS and GRADIENT against the fp64 reference evaluated with the kernel's mask (teacher forcing), with the distances of
    tests/test_dice_gpu.py / test_weighted_ce_gpu.py: 1e-3 relative on a loss plus 1e-7; a gradient's max-abs difference against 1e-3 of
    the reference's max-abs plus the cross-entropy floor, 8 fp32 roundings of max(w) / D (and the Dice floor where Dice is live).
Every test prints the distances it observed (`ohem ...` lines; run with -s); profiles/ohem.txt keeps them."""
import contextlib
import io
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as TF

from conftest import ROOT, load_sub
from test_dice_gpu import ab_floor, gpu, scalar, soft_reference
from test_dice_host import dice_reference
from test_ohem_host import CLASSES, GEOMS, SELECT, THETA_MID, f32, make_case, make_weights, ohem_rank, ohem_reference, selections

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
NEW = {"sscg_ohem_workspace", "sscg_ohem_fwd", "sscg_ce_bwd_ohem", "sscg_upsample_head_bwd_h"}


def bits(t):
    return t.contiguous().view(torch.int32)


def check_loss(tag, loss, ref_loss):
    loss, ref_loss = float(loss.detach()), float(ref_loss)
    d = abs(loss - ref_loss)
    print("ohem %-62s loss %.9g ref %.9g rel %.2e" % (tag, loss, ref_loss, d / max(abs(ref_loss), 1e-30)))
    assert math.isfinite(loss) and d <= 1e-3 * abs(ref_loss) + 1e-7, (tag, loss, ref_loss)


def check_grad(tag, grad, ref_grad, floor):
    grad = grad.detach().double().cpu()
    dg, gmax = float((grad - ref_grad).abs().max()), float(ref_grad.abs().max())
    print("ohem %-62s grad max-abs diff %.2e of %.2e rel %.2e (floor %.1e)" % (tag, dg, gmax, dg / max(gmax, 1e-30), floor))
    assert torch.isfinite(grad).all() and dg <= 1e-3 * gmax + floor, (tag, dg, gmax)


def ce_floor(ref, w32):
    """tests/test_weighted_ce_gpu.py's floor of a cross-entropy gradient, 8 fp32 roundings of max(w) / D, with D over the KEPT pixels"""
    return 8 * EPS32 * (1.0 if w32 is None else float(w32.max())) / ref["D"] if ref["D"] > 0 else 0.0


def raw_ohem_fwd(F, dev, x_nhwc, lab, OH, OW, w, eps, th, K, f):
    """sscg_ohem_fwd itself on sentinel-guarded outputs: dict(keys [N, OH, OW], loss, valid, thr, counts [2]) on the device"""
    lib = F.lib
    N, H, W, Cn = x_nhwc.shape
    n = N * OH * OW
    gk, gs = torch.full((n + 128,), 7.0, device=dev), torch.full((3 * 48,), 7.0, device=dev)
    gc = torch.full((34,), 7, device=dev, dtype=torch.int64)
    keys, counts = gk[64:64 + n], gc[16:18]
    loss, valid, thr = gs[16:17], gs[64:65], gs[112:113]
    nbytes = lib.sscg_ohem_workspace(N, OH, OW)
    ws = torch.full((nbytes + 256,), 0x5A, dtype=torch.uint8, device=dev)
    rc = lib.sscg_ohem_fwd(x_nhwc.data_ptr(), lab.data_ptr(), N, H, W, Cn, OH, OW, None if w is None else w.data_ptr(), eps, th, K, f,
                           keys.data_ptr(), loss.data_ptr(), valid.data_ptr(), thr.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes,
                           F._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert (gk[:64] == 7).all() and (gk[-64:] == 7).all(), "guard bytes around keys"
    live = torch.zeros(3 * 48, dtype=torch.bool, device=dev)
    live[16] = live[64] = live[112] = True
    assert (gs[~live] == 7).all() and (gc[:16] == 7).all() and (gc[18:] == 7).all() and (ws[nbytes:] == 0x5A).all()
    return dict(keys=keys.clone().view(N, OH, OW), loss=loss.clone().reshape(()), valid=valid.clone().reshape(()), thr=thr.clone().reshape(()),
                counts=counts.clone())


def check_selection(tag, out, lab, Cn, th, K, f):
    """thr == max(theta, kthvalue(keys[counted], r)) bit for bit, counts == (#(keys <= thr & counted), V), 2.0f in the other slots"""
    keys, thr, counts = out["keys"].cpu(), out["thr"].cpu(), out["counts"].cpu().tolist()
    counted = (lab >= 0) & (lab < Cn)
    V = int(counted.sum())
    assert (keys[~counted] == 2.0).all() and (keys[counted] >= 0).all() and (keys[counted] <= 1.0).all(), tag
    if V == 0:
        assert counts == [0, 0], (tag, counts)
        return None, 0
    r = ohem_rank(V, K, f)
    kth = torch.kthvalue(keys[counted], r).values
    want = torch.maximum(kth, torch.tensor(th, dtype=torch.float32))
    assert torch.equal(bits(thr.reshape(1)), bits(want.reshape(1))), (tag, float(thr), float(want), r, V)
    mask = counted & (keys <= thr)
    assert counts == [int(mask.sum()), V] and counts[0] >= r, (tag, counts, int(mask.sum()), V, r)
    return mask, r


def ohem_dev(F, th, K, f):
    return F.OhemOptions(th, min_kept=K, min_frac=f)


# ------------------------------------------------------------------------------------------ 1, 3, 4, 7: selection, keys, mask, resized == flat
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("geom", GEOMS, ids=["5x7-40x56", "9x9-65x65", "flat24"])
def test_selection_keys_and_mask(geom, C, F, dev):
    N, H, W, OH, OW = geom
    gi = GEOMS.index(geom)
    x, lab = make_case(1000 * gi + C, N, C, H, W, OH, OW)
    rs = None if (OH, OW) == (H, W) else (OH, OW)
    geo = "%dx%dx%d->%dx%d C=%d" % (N, H, W, OH, OW, C)
    xh = gpu(x, dev).permute(0, 2, 3, 1)
    assert xh.is_contiguous()
    labd = lab.to(dev)
    counted = (lab >= 0) & (lab < C)
    # e: the reference arithmetic's own fp32 error on these keys (torch, CPU)
    x32 = x.float()
    up32 = x32 if rs is None else TF.interpolate(x32, size=rs, mode="bilinear", align_corners=True)
    safe = torch.where(counted, lab, torch.zeros_like(lab))
    k32 = torch.softmax(up32, 1).gather(1, safe.unsqueeze(1)).squeeze(1)
    wts = make_weights(C, C)
    wd = F.ce_weight(wts.tolist(), C, dev)
    if rs is not None:                                              # 7: the flat call on sscg_upsample_bilinear_fwd's output
        up_dev = F.upsample_fwd(gpu(x, dev), OH, OW).permute(0, 2, 3, 1)
        assert up_dev.is_contiguous()
    first = None
    for (th, K, f) in selections(C):
        ref = ohem_reference(x, lab, None, 0.0, th, K, f, resize=rs)
        k64 = ref["keys"]
        e = float((k32.double() - k64)[counted].abs().max())
        for w, eps in ((None, 0.0), (wd, 0.1)):
            tag = "%s th=%g K=%d f=%g %s" % (geo, th, K, f, "w+eps" if w is not None else "plain")
            out = raw_ohem_fwd(F, dev, xh, labd, OH, OW, w, eps, th, K, f)
            mask, r = check_selection(tag, out, lab, C, f32(th), K, f)
            keys = out["keys"].cpu()
            if first is None:
                first = keys
            assert torch.equal(bits(keys), bits(first)), tag          # the keys depend on neither the selection nor the weights
            dk = float((keys.double() - k64)[counted].abs().max())
            band = counted & ((k64 - ref["tau"]).abs() <= 8 * e)
            differ = (mask != ref["mask"]) & ~band
            print("ohem %-62s keys max |fp32 - fp64| %.2e (e %.2e); thr %.9g tau64 %.9g; kept %d of %d (r %d); band %d" % (
                tag, dk, e, float(out["thr"]), ref["tau"], int(mask.sum()), ref["V"], r, int(band.sum())))
            assert dk <= 4 * e, (tag, dk, e)
            assert not differ.any(), (tag, int(differ.sum()))
            assert int(band.sum()) <= max(2, int(0.001 * ref["V"])), (tag, int(band.sum()))
            if th == THETA_MID[C]:
                assert 0.1 < ref["kept"] / ref["V"] < 0.9
            if rs is not None:
                flat = raw_ohem_fwd(F, dev, up_dev, labd, OH, OW, w, eps, th, K, f)
                assert torch.equal(bits(flat["keys"]), bits(out["keys"])) and torch.equal(bits(flat["thr"].reshape(1)), bits(out["thr"].reshape(1)))
                assert torch.equal(flat["counts"], out["counts"]), tag


# ------------------------------------------------------------------------------------------ 2. adversarial keys
def _flat2(F, dev, d, lab, th, K, f, want_grad=True):
    """flat call, C = 2, one row of pixels: logits (0, d[i]), so key = 1 / (1 + exp(d)) for label 0.  Returns the raw outputs and, through
    functional.cross_entropy, the loss and the gradient."""
    n = d.numel()
    x = torch.stack([torch.zeros_like(d), d], 1).view(1, 1, n, 2).float().to(dev)             # NHWC storage [1][1][n][2]
    labd = lab.view(1, 1, n).to(dev)
    out = raw_ohem_fwd(F, dev, x, labd, 1, n, None, 0.0, th, K, f)
    if want_grad:
        xg = x.permute(0, 3, 1, 2).detach().requires_grad_(True)                               # [1, 2, 1, n], channels-last
        loss = F.cross_entropy(xg, labd, ohem=ohem_dev(F, th, K, f))
        loss.backward()
        out["f_loss"], out["grad"] = loss.detach(), xg.grad
        thr, kept, V = F.ohem_stats()
        assert torch.equal(thr, out["thr"]) and [int(kept), int(V)] == out["counts"].tolist()
    return out


def test_adversarial_keys_for_every_digit(F, dev):
    """C = 2, flat.  The key of every candidate logit difference is taken from the kernel itself (two ramps: 4096 steps of 2.5e-8 next to
    0 - keys a few ulps apart just below 0.5 - and 2^18 steps over [-16, 16]); the cases then pick pixels by the bit patterns of those
    keys, so that each of the three ten-bit digits - and each byte - is the one that decides."""
    fine = torch.arange(4096, dtype=torch.float64) * 2.5e-8
    wide = torch.linspace(-16.0, 16.0, 2 ** 18, dtype=torch.float64)
    d_all = torch.cat([fine, wide]).float()
    zeros = torch.zeros(d_all.numel(), dtype=torch.int64)
    ramp = _flat2(F, dev, d_all, zeros, 1e-30, 1, 0.0, want_grad=False)
    check_selection("ramp", ramp, zeros.view(1, 1, -1), 2, f32(1e-30), 1, 0.0)
    kb = bits(ramp["keys"].cpu().view(-1)).long()
    assert (kb >= 0).all() and (kb <= 0x3F800000).all()

    def run(tag, idx, lab=None, th=1e-30, K=1, f=0.0):
        d = d_all[idx]
        lab = torch.zeros(d.numel(), dtype=torch.int64) if lab is None else lab
        out = _flat2(F, dev, d, lab, th, K, f)
        counted = lab == 0
        assert torch.equal(bits(out["keys"].cpu().view(-1))[counted].long(), kb[idx][counted]), tag        # the ramp's keys again
        mask, r = check_selection(tag, out, lab.view(1, 1, -1), 2, f32(th), K, f)
        if mask is None:
            mask = torch.zeros(1, 1, d.numel(), dtype=torch.bool)
        x64 = torch.zeros(1, 2, 1, d.numel(), dtype=torch.float64)
        x64[0, 1, 0] = d.double()
        ref = ohem_reference(x64, lab.view(1, 1, -1), None, 0.0, th, K, f, mask=mask)
        if ref["D"] > 0:
            check_loss(tag, out["f_loss"], ref["loss"])
            check_grad(tag, out["grad"], ref["grad"], ce_floor(ref, None))
            assert torch.equal(out["f_loss"], out["loss"])
        print("ohem %-62s thr bits 0x%08X kept %d of %d" % (tag, int(bits(out["thr"].cpu().reshape(1))), *out["counts"].tolist()))
        return out, mask

    # all equal: everything is kept (<=), whatever r is
    same = torch.full((700,), 4096 + 2 ** 17, dtype=torch.int64)
    for K in (1, 350, 700, 10 ** 6):
        out, mask = run("all equal K=%d" % K, same, K=K)
        assert out["counts"].tolist() == [700, 700] and int(bits(out["thr"].cpu().reshape(1))) == int(kb[same[0]])
    # two values one ulp apart, r on either side of the step
    uniq = torch.unique(kb[:4096], sorted=True)
    step = (uniq[1:] - uniq[:-1] == 1).nonzero()
    assert step.numel(), "the fine ramp holds no two keys one ulp apart"
    lo_bits, hi_bits = int(uniq[step[0, 0]]), int(uniq[step[0, 0] + 1])
    i_lo, i_hi = int((kb[:4096] == lo_bits).nonzero()[0, 0]), int((kb[:4096] == hi_bits).nonzero()[0, 0])
    pair = torch.tensor([i_lo] * 300 + [i_hi] * 200)[torch.randperm(500, generator=torch.Generator().manual_seed(1))]
    out, _ = run("one ulp apart r=300", pair, K=300)
    assert out["counts"].tolist() == [300, 500] and int(bits(out["thr"].cpu().reshape(1))) == lo_bits
    out, _ = run("one ulp apart r=301", pair, K=301)
    assert out["counts"].tolist() == [500, 500] and int(bits(out["thr"].cpu().reshape(1))) == hi_bits
    # values that differ in the lowest byte only: the fullest group of the fine ramp that shares its upper 24 bits
    grp, cnt = torch.unique(kb[:4096] >> 8, return_counts=True)
    g = int(grp[cnt.argmax()])
    low = (kb[:4096] >> 8 == g).nonzero().view(-1)
    assert torch.unique(kb[low]).numel() >= 8
    for K in (1, low.numel() // 3, low.numel()):
        run("lowest byte only K=%d" % K, low, K=K)
    # values that differ in the top byte only: two keys of the wide ramp with the same low 24 bits
    wb = kb[4096:]
    order = torch.argsort(wb & 0xFFFFFF)
    sl, sh = (wb & 0xFFFFFF)[order], (wb >> 24)[order]
    hit = ((sl[1:] == sl[:-1]) & (sh[1:] != sh[:-1])).nonzero()
    assert hit.numel(), "the wide ramp holds no two keys that differ in the top byte only"
    a, b = int(order[hit[0, 0]]) + 4096, int(order[hit[0, 0] + 1]) + 4096
    top = torch.tensor([a] * 129 + [b] * 257)[torch.randperm(386, generator=torch.Generator().manual_seed(2))]
    n_small = 129 if kb[a] < kb[b] else 257
    for K, kept in ((n_small, n_small), (n_small + 1, 386)):
        out, _ = run("top byte only K=%d" % K, top, K=K)
        assert out["counts"].tolist() == [kept, 386]
    # spread over every byte; r = 1, r = V, in between, by share; thresh-dominated
    spread = 4096 + torch.randperm(2 ** 18, generator=torch.Generator().manual_seed(3))[:3001]
    for th, K, f in ((1e-30, 1, 0.0), (1e-30, 3001, 0.0), (1e-30, 10 ** 12, 0.0), (1e-30, 1777, 0.0), (1e-30, 0, 0.5), (0.3, 5, 0.0), (1.0, 0, 0.0)):
        out, mask = run("every byte th=%g K=%d f=%g" % (th, K, f), spread, th=th, K=K, f=f)
        if th == 1e-30 and not f:
            assert out["counts"].tolist()[0] == min(K, 3001)          # distinct keys: exactly r are kept
    # V = 1; V = 0; a void stretch (one "sample") beside a live one
    lab1 = torch.full((300,), 255, dtype=torch.int64)
    lab1[123] = 0
    out, _ = run("V = 1", spread[:300], lab=lab1, K=7)
    assert out["counts"].tolist() == [1, 1] and torch.count_nonzero(out["grad"]) == 2
    void = torch.full((300,), -100, dtype=torch.int64)
    void[::2] = 255
    void[5] = 2                                                           # C = 2: id 2 is out of range too
    out, _ = run("V = 0", spread[:300], lab=void, K=7, f=0.5)
    assert out["counts"].tolist() == [0, 0] and math.isnan(float(out["loss"])) and math.isnan(float(out["f_loss"]))
    assert float(out["valid"]) == 0.0 and torch.count_nonzero(out["grad"]) == 0


def test_one_sample_entirely_void(F, dev):
    N, H, W, C = 2, 24, 24, 2
    x, lab = make_case(77, N, C, H, W, H, W)
    lab[1] = 255
    labd = lab.to(dev)
    for th, K, f in ((0.7, 1, 0.0), (0.05, 400, 0.0), (0.3, 0, 0.5)):
        xg = gpu(x, dev).requires_grad_(True)
        out = raw_ohem_fwd(F, dev, xg.detach().permute(0, 2, 3, 1), labd, H, W, None, 0.0, th, K, f)
        mask, r = check_selection("void sample", out, lab, C, f32(th), K, f)
        assert not mask[1].any() and (out["keys"][1] == 2.0).all()
        loss = F.cross_entropy(xg, labd, ohem=ohem_dev(F, th, K, f))
        loss.backward()
        ref = ohem_reference(x, lab, None, 0.0, th, K, f, mask=mask)
        check_loss("void sample th=%g K=%d f=%g" % (th, K, f), loss, ref["loss"])
        check_grad("void sample th=%g K=%d f=%g" % (th, K, f), xg.grad, ref["grad"], ce_floor(ref, None))
        assert torch.count_nonzero(xg.grad[1]) == 0


# ------------------------------------------------------------------------------------------ 5. loss and gradient, teacher-forced
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("geom", GEOMS, ids=["5x7-40x56", "9x9-65x65", "flat24"])
def test_loss_and_gradient_on_the_kernels_mask(geom, C, F, dev):
    N, H, W, OH, OW = geom
    gi = GEOMS.index(geom)
    x, lab = make_case(1000 * gi + C, N, C, H, W, OH, OW)
    fused = (OH, OW) != (H, W)
    rs = (OH, OW) if fused else None
    geo = "%dx%dx%d->%dx%d C=%d" % (N, H, W, OH, OW, C)
    labd = lab.to(dev)
    wts = make_weights(C, C)
    wd = F.ce_weight(wts.tolist(), C, dev)
    g = torch.Generator().manual_seed(5 + C)
    R = torch.randn(N, C, OH, OW, generator=g, dtype=torch.float64)
    Rg = gpu(R, dev)
    dwts = make_weights(C + 1, C)
    dopts = F.DiceOptions(weight=F.dice_weight(dwts.tolist(), C, dev), smooth=1.0, batch=False)
    x0 = gpu(x, dev)
    assert F._head_applies(x0, OH, OW) == fused
    soft_grad = soft_reference(x, R, (OH, OW))
    dref = dice_reference(x, lab, dwts, 1.0, False, resize=rs)
    y_plain = F.upsample_softmax_ce(x0, (OH, OW))[0]
    for (th, K, f) in selections(C):
        opt = ohem_dev(F, th, K, f)
        for w32, w, eps in ((None, None, 0.0), (wts, wd, 0.1)):
            tag = "%s th=%g K=%d f=%g %s" % (geo, th, K, f, "w+eps" if w is not None else "plain")
            out = F.ohem_fwd(x0, labd, (OH, OW), opt, w, eps)
            mask = (out[2] <= out[3]).cpu()
            ref = ohem_reference(x, lab, w32, eps, th, K, f, resize=rs, mask=mask)
            assert ref["kept"] == int(out[4][0]) and ref["V"] == int(out[4][1])
            assert abs(float(out[1]) - ref["D"]) <= 1e-6 * ref["D"]
            # the cross entropy alone (flat: sscg_ce_bwd_ohem; fused: sscg_upsample_head_bwd_h with the one branch)
            xg = gpu(x, dev).requires_grad_(True)
            if fused:
                y, ce = F.upsample_softmax_ce(xg, (OH, OW), labd, want_soft=False, weight=w, label_smoothing=eps, ohem=opt)
                assert y is None
            else:
                ce = F.cross_entropy(xg, labd, w, eps, ohem=opt)
            F.weighted_sum([ce], [0.37]).backward()
            check_loss(tag, ce, ref["loss"])
            check_grad(tag, xg.grad / 0.37, ref["grad"], ce_floor(ref, w32))
            assert torch.equal(ce.detach(), out[0])
            # with the softmax output live: (y * R).sum() as in the Dice tests
            xg = gpu(x, dev).requires_grad_(True)
            y, ce = F.upsample_softmax_ce(xg, (OH, OW), labd, weight=w, label_smoothing=eps, ohem=opt)
            (1.3 * ce + (y * Rg).sum()).backward()
            check_grad(tag + " +soft", xg.grad, 1.3 * ref["grad"] + soft_grad, 1.3 * ce_floor(ref, w32))
            assert torch.equal(y.detach(), y_plain) and torch.equal(ce.detach(), out[0])
            # with Dice live: the total of three terms, one stencil launch
            xg = gpu(x, dev).requires_grad_(True)
            y, ce, d = F.upsample_softmax_ce_dice(xg, (OH, OW), labd, weight=w, label_smoothing=eps, dice=dopts, ohem=opt)
            (1.3 * ce + 0.7 * d + (y * Rg).sum()).backward()
            check_loss(tag + " +soft+dice (Dice)", d, dref["loss"])
            check_grad(tag + " +soft+dice", xg.grad, 1.3 * ref["grad"] + 0.7 * dref["grad"] + soft_grad,
                       1.3 * ce_floor(ref, w32) + 0.7 * ab_floor(dref))
            assert torch.equal(ce.detach(), out[0])
            # Dice and the mined cross entropy without the softmax output
            xg = gpu(x, dev).requires_grad_(True)
            y, ce, d = F.upsample_softmax_ce_dice(xg, (OH, OW), labd, want_soft=False, weight=w, label_smoothing=eps, dice=dopts, ohem=opt)
            (1.3 * ce + 0.7 * d).backward()
            check_grad(tag + " +dice", xg.grad, 1.3 * ref["grad"] + 0.7 * dref["grad"], 1.3 * ce_floor(ref, w32) + 0.7 * ab_floor(dref))


def test_the_raw_head_backward_branch_by_branch(F, dev):
    """sscg_upsample_head_bwd_h itself, every combination of its three branches, on sentinel-guarded outputs (C = 21, 9x9 -> 65x65)"""
    N, H, W, OH, OW = GEOMS[1]
    C = 21
    x, lab = make_case(1021, N, C, H, W, OH, OW)
    th, K, f = SELECT[2]
    wts, dwts = make_weights(C, C), make_weights(C + 1, C)
    wd, dwd = F.ce_weight(wts.tolist(), C, dev), F.dice_weight(dwts.tolist(), C, dev)
    labd = lab.to(dev)
    xh = gpu(x, dev).permute(0, 2, 3, 1)
    out = raw_ohem_fwd(F, dev, xh, labd, OH, OW, wd, 0.1, th, K, f)
    mask, _ = check_selection("raw head", out, lab, C, f32(th), K, f)
    ref = ohem_reference(x, lab, wts, 0.1, th, K, f, resize=(OH, OW), mask=mask)
    dref = dice_reference(x, lab, dwts, 1.0, True, resize=(OH, OW))
    _, coef, _ = F.dice_fwd(gpu(x, dev), labd, (OH, OW), dwd, 1.0, True)
    g = torch.Generator().manual_seed(9)
    R = torch.randn(N, C, OH, OW, generator=g, dtype=torch.float64)
    dyn = gpu(R, dev).permute(0, 2, 3, 1).contiguous()
    soft_grad = soft_reference(x, R, (OH, OW))
    g_ce, g_dice = scalar(1.3, dev), scalar(0.7, dev)
    for use_ce in (True, False):
        for use_soft in (True, False):
            for use_dice in (True, False):
                if not (use_ce or use_soft or use_dice):
                    continue
                guard = torch.full((N * H * W * C + 64,), 7.0, device=dev)
                dx = guard[32:32 + N * H * W * C]
                rc = F.lib.sscg_upsample_head_bwd_h(
                    xh.data_ptr(), labd.data_ptr(), out["keys"].data_ptr() if use_ce else None, out["thr"].data_ptr() if use_ce else None,
                    wd.data_ptr(), 0.1, dyn.data_ptr() if use_soft else None, g_ce.data_ptr() if use_ce else None,
                    out["valid"].data_ptr() if use_ce else None, coef.data_ptr() if use_dice else None, g_dice.data_ptr() if use_dice else None,
                    1, dx.data_ptr(), N, H, W, C, OH, OW, F._stream())
                assert rc == 0
                torch.cuda.synchronize()
                assert (guard[:32] == 7).all() and (guard[-32:] == 7).all()
                want = (1.3 * ref["grad"] if use_ce else 0) + (0.7 * dref["grad"] if use_dice else 0) + (soft_grad if use_soft else 0)
                floor = (1.3 * ce_floor(ref, wts) if use_ce else 0.0) + (0.7 * ab_floor(dref) if use_dice else 0.0)
                check_grad("raw head ce=%d soft=%d dice=%d" % (use_ce, use_soft, use_dice), dx.view(N, H, W, C).permute(0, 3, 1, 2), want, floor)


# ------------------------------------------------------------------------------------------ 6. everything kept
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("geom", [GEOMS[0], GEOMS[2]], ids=["5x7-40x56", "flat24"])
def test_everything_kept_is_the_plain_cross_entropy(geom, C, F, dev):
    N, H, W, OH, OW = geom
    x, lab = make_case(300 + C, N, C, H, W, OH, OW)
    labd = lab.to(dev)
    wts = make_weights(C, C)
    wd = F.ce_weight(wts.tolist(), C, dev)
    V = int(((lab >= 0) & (lab < C)).sum())
    opt = ohem_dev(F, 1.0, V + 5, 0.0)
    for w32, w, eps in ((None, None, 0.0), (wts, wd, 0.1)):
        got = []
        for o in (None, opt):
            xg = gpu(x, dev).requires_grad_(True)
            kw = {} if o is None else {"ohem": o}
            if (OH, OW) != (H, W):
                ce = F.upsample_softmax_ce(xg, (OH, OW), labd, want_soft=False, weight=w, label_smoothing=eps, **kw)[1]
            else:
                ce = F.cross_entropy(xg, labd, w, eps, **kw)
            ce.backward()
            got.append((ce.detach().double().cpu(), xg.grad.double().cpu()))
        thr, kept, counted = F.ohem_stats()
        assert float(thr) == 1.0 and int(kept) == V == int(counted)
        D = float(V) if w32 is None else float(wts.double()[lab[(lab >= 0) & (lab < C)]].sum())
        tag = "all kept %dx%dx%d->%dx%d C=%d %s" % (N, H, W, OH, OW, C, "w+eps" if w is not None else "plain")
        check_loss(tag, got[1][0], got[0][0])
        check_grad(tag, got[1][1], got[0][1], 8 * EPS32 * (1.0 if w32 is None else float(wts.max())) / D)


# ------------------------------------------------------------------------------------------ 8. determinism
@pytest.mark.parametrize("C", [4, 21])
def test_the_same_call_twice_gives_the_same_bits(C, F, dev):
    N, H, W, OH, OW = 2, 9, 11, 67, 83
    x, lab = make_case(800 + C, N, C, H, W, OH, OW)
    labd = lab.to(dev)
    R = gpu(torch.randn(N, C, OH, OW, generator=torch.Generator().manual_seed(8)), dev)
    wd = F.ce_weight(make_weights(C, C).tolist(), C, dev)
    dopts = F.DiceOptions(None, 1.0, True)
    runs = []
    for _ in range(2):
        outs = []
        for (th, K, f) in selections(C):
            opt = ohem_dev(F, th, K, f)
            xg = gpu(x, dev).requires_grad_(True)
            outs += list(F.ohem_fwd(xg.detach(), labd, (OH, OW), opt, wd, 0.1))
            y, ce, d = F.upsample_softmax_ce_dice(xg, (OH, OW), labd, weight=wd, label_smoothing=0.1, dice=dopts, ohem=opt)
            (ce + d + (y * R).sum()).backward()
            outs += [y.detach(), ce.detach(), d.detach(), xg.grad] + list(F.ohem_stats())
            up = F.upsample_bilinear(xg.detach(), (OH, OW)).requires_grad_(True)
            fl = F.cross_entropy(up, labd, wd, 0.1, ohem=opt)
            fl.backward()
            outs += [fl.detach(), up.grad]
        runs.append(outs)
    assert len(runs[0]) == 14 * len(selections(C))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ------------------------------------------------------------------------------------------ 9. past the caps
@pytest.mark.parametrize("case", ["key trip", "histogram", "backward cap"])
def test_past_the_caps(case, F, dev):
    """C = 4 (the host reference stays in seconds), flat, ragged tails; outputs guarded by sentinels on both sides.  The caps of
    csrc/ohem.hip: the key pass runs at most 256 blocks x 256 threads per sample and trip; a histogram pass at most 2048 blocks, each
    flushing up to 1024 bins per digit; the loss pass at most 1024 blocks (= records); the flat backward at most 8192 blocks x 256.
      key trip:      363 x 363 = 131769 pixels of ONE sample > 256 * 256 = 65536: every thread takes 2 pixels, 697 of them a third
      histogram:     600 x 601 = 360600 pixels -> 1409 histogram blocks > the 1024 bins of a digit (and > the 1024 loss records)
      backward cap:  1449 x 1449 = 2099601 pixels > the flat backward's 8192 * 256 (and 2048 histogram blocks: that cap too)"""
    C = 4
    N, H, W = {"key trip": (1, 363, 363), "histogram": (1, 600, 601), "backward cap": (1, 1449, 1449)}[case]
    assert (H * W) % 256
    if case == "key trip":
        assert H * W > 256 * 256
    if case == "histogram":
        assert (H * W + 255) // 256 > 1024
    if case == "backward cap":
        assert H * W > 8192 * 256 and (H * W + 255) // 256 > 2048
    assert F.lib.sscg_ohem_workspace(N, H, W) == 3 * 1024 * 4 + 256 + 3 * 1024 * 8 + N * H * W * 4
    x, lab = make_case(len(case), N, C, H, W, H, W)
    wts = make_weights(C, C)
    wd = F.ce_weight(wts.tolist(), C, dev)
    xh = gpu(x, dev).permute(0, 2, 3, 1)
    labd = lab.to(dev)
    th, K, f = 0.3, 1000, 0.25
    out = raw_ohem_fwd(F, dev, xh, labd, H, W, wd, 0.1, th, K, f)
    tag = "caps %s %dx%dx%d" % (case, N, H, W)
    mask, r = check_selection(tag, out, lab, C, f32(th), K, f)
    ref = ohem_reference(x, lab, wts, 0.1, th, K, f, mask=mask)
    assert ref["r"] == r and ref["kept"] == int(mask.sum())
    check_loss(tag, out["loss"], ref["loss"])
    assert abs(float(out["valid"]) - ref["D"]) <= 1e-6 * ref["D"]
    rows = N * H * W
    guard = torch.full((rows * C + 64,), 7.0, device=dev)
    dx = guard[32:32 + rows * C]
    rc = F.lib.sscg_ce_bwd_ohem(xh.data_ptr(), labd.data_ptr(), out["keys"].data_ptr(), out["thr"].data_ptr(), rows, C, wd.data_ptr(), 0.1,
                                None, 0.37, out["valid"].data_ptr(), dx.data_ptr(), F._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert (guard[:32] == 7).all() and (guard[-32:] == 7).all()
    check_grad(tag, dx.view(N, H, W, C).permute(0, 3, 1, 2) / 0.37, ref["grad"], ce_floor(ref, wts))


# ------------------------------------------------------------------------------------------ 10. through the model
def _args(dev, tmp_path, **kw):
    FX = __import__("oracle.fixtures", fromlist=["x"])
    return FX.make_args(dataset="acdc", crop_height=64, crop_width=64, batch_size=2, gpu_ids=[dev.index or 0], ngf=8, ndf=8,
                        checkpoint_dir=str(tmp_path / "ckpt"), as_written=True, **kw)


@pytest.mark.parametrize("dice", [False, True], ids=["ohem", "ohem+dice"])
def test_supervised_step_reports_the_mined_loss(dice, F, dev, tmp_path):
    md, data = load_sub("model"), load_sub("data")
    th, K, f = 0.25, 100, 0.0625
    extra = dict(dice_weight=0.5) if dice else {}
    args = _args(dev, tmp_path, model="supervised_model", ohem_thresh=th, ohem_min_kept=K, **extra)
    torch.manual_seed(21)
    with contextlib.redirect_stdout(io.StringIO()):
        m = md.supervised_model(args)
        loader = data.synthetic_loaders(args, 4, steps=2)[0]
    o = m.ohem_options
    assert (o.thresh, o.min_kept, o.min_frac) == (th, K, f)
    l_img, l_gt, _ = next(iter(loader))
    l_img, l_gt = l_img.to(dev), l_gt.to(dev)
    lab = l_gt.cpu().squeeze(1)
    with torch.no_grad():
        logits = m.Gsi(l_img).float()
        out = F.ohem_fwd(F.to_nhwc(logits), l_gt.squeeze(1).contiguous(), (64, 64), o)
        mask = (out[2] <= out[3]).cpu()
    before = [p.detach().clone() for p in m.Gsi.parameters()]
    ce = float(m.step(l_img, l_gt))
    share = float(m.extras["ohem_kept"])
    assert set(m.extras) == ({"ohem_kept", "dice_loss"} if dice else {"ohem_kept"})
    ref = ohem_reference(logits.double().cpu(), lab, None, 0.0, th, K, f, resize=(64, 64), mask=mask)
    own = ohem_reference(logits.double().cpu(), lab, None, 0.0, th, K, f, resize=(64, 64))
    print("ohem supervised step (dice=%d): loss %.9g ref %.9g (rel %.2e; on the reference's own mask %.9g); kept share %.4f ref %.4f" % (
        dice, ce, float(ref["loss"]), abs(ce - float(ref["loss"])) / abs(float(ref["loss"])), float(own["loss"]), share, own["kept"] / own["V"]))
    assert math.isfinite(ce) and abs(ce - float(ref["loss"])) <= 1e-3 * abs(float(ref["loss"])) + 1e-7
    # (the step runs the network again: a pixel within an fp32 rounding of the threshold may change sides between the two forwards)
    assert 0.0 < share <= 1.0 and abs(share - ref["kept"] / ref["V"]) <= 2.0 / ref["V"] + 1e-6
    if dice:
        assert 0.0 < float(m.extras["dice_loss"]) <= 1.0
    assert any(not torch.equal(a, b) for a, b in zip(before, m.Gsi.parameters()))            # the update was applied


def test_semisupervised_step_takes_the_flags(F, dev, tmp_path):
    md, data = load_sub("model"), load_sub("data")
    got = {}
    for tag, kw in (("default", {}), ("ohem", dict(ohem_thresh=0.25, ohem_min_kept=100)), ("ohem+dice", dict(ohem_thresh=0.25, dice_weight=0.5))):
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
    assert set(got["default"]) == set(md.LOSS_KEYS)
    assert set(got["ohem"]) - set(got["default"]) == {"lab_ohem_kept", "gt_cycle_ohem_kept"}
    assert set(got["ohem+dice"]) - set(got["default"]) == {"lab_ohem_kept", "gt_cycle_ohem_kept", "lab_loss_dice", "gt_cycle_dice"}
    print("ohem semisupervised step: kept shares %.4f / %.4f; lab_loss_CE %.6g (mined) / %.6g (plain); lab_loss_MSE %.6g / %.6g" % (
        got["ohem"]["lab_ohem_kept"], got["ohem"]["gt_cycle_ohem_kept"], got["ohem"]["lab_loss_CE"], got["default"]["lab_loss_CE"],
        got["ohem"]["lab_loss_MSE"], got["default"]["lab_loss_MSE"]))
    for tag in ("ohem", "ohem+dice"):
        assert 0.0 < got[tag]["lab_ohem_kept"] <= 1.0 and 0.0 < got[tag]["gt_cycle_ohem_kept"] <= 1.0
        # the networks' first forward does not depend on the loss flags: the term the flag cannot reach agrees; the mined loss, a mean
        # over the hardest pixels, is at least the plain one
        assert got[tag]["lab_loss_MSE"] == pytest.approx(got["default"]["lab_loss_MSE"], rel=1e-3)
        assert got[tag]["lab_loss_CE"] >= got["default"]["lab_loss_CE"] * (1 - 1e-3)


# ------------------------------------------------------------------------------------------ 11. flags off: no new launch, no new key
CENSUS = r"""
import contextlib, io, json, sys
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
for tag, kw in (("sup off", dict(model="supervised_model")), ("sup on", dict(model="supervised_model", ohem_thresh=0.25)), ("semi off", {})):
    a = args(**kw)
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        m = md.supervised_model(a) if tag.startswith("sup") else md.semisuper_cycleGAN(a)
    l_img, l_gt, unl_img = batch(a)
    torch.cuda.synchronize()
    sys.stderr.write("[census] begin %%s\n" %% tag)
    if tag.startswith("sup"):
        m.step(l_img, l_gt)
        keys = sorted(getattr(m, "extras", {}))
    else:
        keys = sorted(m.step(l_img, l_gt, unl_img))
        m.sync_losses()
    load_sub("functional").flush_side_work()
    torch.cuda.synchronize()
    sys.stderr.write("[census] end %%s\n" %% tag)
    sys.stderr.write("[census] keys %%s %%s\n" %% (tag, json.dumps(keys)))
"""


def test_flags_off_a_step_names_none_of_the_new_entries(tmp_path):
    env = dict(os.environ, SSCG_TRACE="1")
    for k in ("SSCG_RACECHECK", "SSCG_FUZZ", "SSCG_FUSE_HEAD"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", CENSUS % (ROOT, os.path.join(ROOT, "tests"), str(tmp_path / "ckpt"))], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    calls, keys = {}, {}
    for tag in ("sup off", "sup on", "semi off"):
        body = r.stderr[r.stderr.index("[census] begin " + tag):r.stderr.index("[census] end " + tag)]
        names = [line[7:].split("(")[0] for line in body.splitlines() if line.startswith("[sscg] ")]
        calls[tag] = {n: names.count(n) for n in set(names)}
        keys[tag] = json.loads(r.stderr.split("[census] keys %s " % tag)[1].splitlines()[0])
    assert calls["sup off"].get("sscg_upsample_head_fwd") == 1 and calls["sup off"].get("sscg_upsample_head_bwd") == 1
    assert not NEW & set(calls["sup off"]) and not NEW & set(calls["semi off"]), calls
    assert calls["semi off"].get("sscg_upsample_head_fwd") == 3 and calls["semi off"].get("sscg_upsample_head_bwd") == 3
    assert keys["sup off"] == [] and keys["semi off"] == sorted(load_sub("model").LOSS_KEYS) and keys["sup on"] == ["ohem_kept"]
    # the control: with the flag the log does name them - one forward entry, ONE stencil launch backward, no head entry at all
    on = calls["sup on"]
    assert on.get("sscg_ohem_fwd") == 1 and on.get("sscg_upsample_head_bwd_h") == 1
    assert not {"sscg_upsample_head_fwd", "sscg_upsample_head_bwd", "sscg_ce_bwd_ohem"} & set(on)

    def launches(c):
        return {k: v for k, v in c.items() if k not in NEW and k not in ("sscg_upsample_head_fwd", "sscg_upsample_head_bwd")
                and not k.endswith(("_workspace", "_bytes", "_applies"))}
    assert launches(on) == launches(calls["sup off"]), (launches(on), launches(calls["sup off"]))
