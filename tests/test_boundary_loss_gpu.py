"""Boundary loss on signed distance maps on the MI355X: sscg_sdm bit for bit against tests/sdm_reference.py (scipy), the loss forward
against the fp64 restatement, the flat backward and the fused label head with the boundary branch (sscg_upsample_head_bwd_b) against
fp64 autograd, and one step of each driver with --boundary_loss.

Tolerances.  The integers of sdm: torch.equal.  A sum of p_c phi_c (sums[n][c], the loss) cancels by sign, so it is held to
1e-6 * S + 1e-7 with S the same sum over |p_c phi_c| from the reference - on the resized logits whose bits the loss is defined on
(sscg_upsample_bilinear_fwd's output), softmax and sums in fp64.  A gradient: the project's rule (tests/test_dice_gpu.py), max-abs
difference <= 1e-3 * max-abs of the fp64 gradient + floor, the floor 8 fp32 roundings of the largest term k * max(w) * max|phi|; a
total that carries other terms adds their files' floors, each times its weight.
Every test prints the distances it observed (`bnd ...` lines; run with -s); profiles/boundary_loss.txt keeps them."""
import contextlib
import io
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_sub
from sdm_reference import boundary_reference, sdm_reference
from test_dice_gpu import ab_floor, ce_floor, ce_reference, gpu, scalar, soft_reference
from test_dice_host import dice_reference
from test_ohem_gpu import ce_floor as mined_floor
from test_ohem_host import ohem_reference

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
SDM_SHAPES = [(2, 1, 1, 1), (1, 1, 9, 2), (1, 9, 1, 2), (2, 5, 7, 3), (2, 40, 300, 4), (1, 70, 33, 21), (1, 33, 65, 64)]
HEADS = [(2, 3, 5, 7, 33, 41), (2, 21, 9, 9, 65, 65)]                       # N, C, H, W -> OH, OW: the two resized heads
FORWARD = HEADS + [(2, 4, 12, 10, 12, 10), (2, 1, 3, 3, 9, 9), (2, 64, 3, 3, 9, 9)]


# ------------------------------------------------------------------------------------------ labels
def blobs(rng, N, H, W, C):
    """random blobs: a coarse random map, each cell 4 rows x 5 columns"""
    coarse = rng.integers(0, C, size=(N, (H + 3) // 4, (W + 4) // 5))
    return np.repeat(np.repeat(coarse, 4, axis=1), 5, axis=2)[:, :H, :W].astype(np.int64).copy()


def label_patterns(N, H, W, C, seed):
    rng = np.random.default_rng(seed)
    out = {"blobs": blobs(rng, N, H, W, C)}
    lab = blobs(rng, N, H, W, C)
    lab[0, 0, 0] = 0
    other = lab[-1]                                                          # class 0 absent from the last sample (N == 1: from the call)
    other[other == 0] = 1 if C > 1 else 255
    out["absent in one sample"] = lab
    lab = blobs(rng, N, H, W, C)
    lab[0] = C - 1
    out["a class fills a sample"] = lab
    lab = np.full((N, H, W), C - 1 if C > 1 else 255, dtype=np.int64)
    lab[0, 0, 0] = 0
    lab[-1, H - 1, W - 1] = 0
    out["one member in a corner"] = lab
    yy, xx = np.indices((H, W))
    out["checkerboard"] = np.broadcast_to((yy + xx) % 2, (N, H, W)).astype(np.int64).copy()       # (C == 1: class 0 and the void id 1)
    lab = blobs(rng, N, H, W, C)
    flat = lab.reshape(-1)
    flat[::5] = 255
    flat[2::7] = -100
    flat[3::9] = C
    flat[4::13] = C + 190
    out["void labels"] = lab
    return out


class Guarded(object):
    """a 256-byte aligned view of `nbytes` between two 64 KiB guards of 0xFF bytes, the view itself pre-filled with `fill`"""

    def __init__(self, nbytes, fill, dev):
        self.g = 65536
        self.buf = torch.full((nbytes + 2 * self.g + 256,), 0xFF, dtype=torch.uint8, device=dev)
        self.off = self.g + (-(self.buf.data_ptr() + self.g)) % 256
        self.n = nbytes
        self.view = self.buf[self.off:self.off + nbytes]
        self.view.fill_(fill)

    def intact(self):
        return bool((self.buf[:self.off] == 0xFF).all()) and bool((self.buf[self.off + self.n:] == 0xFF).all())


def raw_sdm(F, dev, labd, N, H, W, C, fill):
    need = F.lib.sscg_sdm_workspace(N, H, W, C)
    assert need > 0
    out, ws = Guarded(N * H * W * C * 4, fill, dev), Guarded(need, fill, dev)
    rc = F.lib.sscg_sdm(labd.data_ptr(), N, H, W, C, out.view.data_ptr(), ws.view.data_ptr(), need, F._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert out.intact() and ws.intact(), "a guard was written"
    return out.view.clone().view(torch.int32).view(N, H, W, C)


# ------------------------------------------------------------------------------------------ 1. the signed distance maps
@pytest.mark.parametrize("shape", SDM_SHAPES + [(1, 2, 24577, 2)], ids=lambda s: "x".join(map(str, s)))
def test_sdm_equals_the_reference_bit_for_bit(shape, F, dev):
    N, H, W, C = shape
    pats = label_patterns(N, H, W, C, 17 * H + W + C)
    if W > 20000:                                                             # the row wider than the staged limit: read from the workspace
        pats = {k: pats[k] for k in ("blobs", "void labels")}
    for name, lab in pats.items():
        want = torch.from_numpy(sdm_reference(lab, C))
        labd = torch.from_numpy(lab).to(dev)
        got = [raw_sdm(F, dev, labd, N, H, W, C, fill).cpu() for fill in (0xFF, 0x00, 0x5A)]
        assert torch.equal(got[0], want), (shape, name, int((got[0] != want).sum()))
        assert torch.equal(got[1], got[0]) and torch.equal(got[2], got[0]), (shape, name, "depends on what the scratch held")
        assert torch.equal(F.signed_distance_maps(labd, C).cpu(), want)
        live = int((want != 0).any(dim=1).any(dim=1).sum())
        print("bnd sdm %-14s %-24s equal; %d of %d planes have a contour, max |sdm| %d" % (
            "x".join(map(str, shape)), name, live, N * C, int(want.abs().max())))
    if "checkerboard" in pats and H * W > 1 and C >= 2:
        s = sdm_reference(pats["checkerboard"], C)
        assert (np.abs(s[..., :2]) == 1).all()
    if "absent in one sample" in pats and N == 2:
        s = sdm_reference(pats["absent in one sample"], C)
        assert s[0, :, :, 0].any() or H * W == 1
        assert not s[1, :, :, 0].any()                                        # nothing leaks across samples


# ------------------------------------------------------------------------------------------ 2. the loss forward
def make_weights(C, seed):
    g = torch.Generator().manual_seed(seed)
    w = (torch.rand(C, generator=g) + 0.2).float()
    if C > 1:
        w[(C - 1) // 2] = 0.0
    return w


def make_head_case(geom, seed):
    N, C, H, W, OH, OW = geom
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 2
    lab = torch.from_numpy(label_patterns(N, OH, OW, C, seed)["void labels"])
    return x, lab


def bnd_floor(ref, w32):
    return 8 * EPS32 * ref["k"] * (1.0 if w32 is None else float(w32.max())) * float(np.abs(ref["phi"]).max())


def check_grad(tag, grad, ref_grad, floor):
    grad = grad.detach().double().cpu()
    dg, gmax = float((grad - ref_grad).abs().max()), float(ref_grad.abs().max())
    print("bnd %-62s grad max-abs diff %.2e of %.2e rel %.2e (floor %.1e)" % (tag, dg, gmax, dg / max(gmax, 1e-30), floor))
    assert torch.isfinite(grad).all() and dg <= 1e-3 * gmax + floor, (tag, dg, gmax)


@pytest.mark.parametrize("geom", FORWARD, ids=lambda g: "N%d-C%d-%dx%d-%dx%d" % g)
def test_loss_forward(geom, F, dev):
    N, C, H, W, OH, OW = geom
    x, lab = make_head_case(geom, 100 * C + OH)
    xg, labd = gpu(x, dev), lab.to(dev)
    sdm = F.signed_distance_maps(labd, C)
    up = xg if (OH, OW) == (H, W) else F.upsample_bilinear(xg, (OH, OW))
    up64 = up.double().cpu()
    for w32 in (None, make_weights(C, C + 1)):
        wd = None if w32 is None else F.boundary_weight(w32.tolist(), C, dev)
        ref = boundary_reference(x, lab, w32, up64=up64)
        assert torch.equal(sdm.cpu(), torch.from_numpy(ref["sdm"]))
        loss, coef, sums, counted = F.boundary_loss_fwd(xg, labd, (OH, OW), sdm, wd, want_sums=True)
        assert int(counted) == ref["counted"] and 0 < ref["counted"] < N * OH * OW
        assert abs(float(coef) - ref["k"]) <= EPS32 * ref["k"]
        ds = (sums.cpu() - ref["sums"]).abs()
        assert (ds <= 1e-6 * ref["scale"] + 1e-7).all(), (geom, float((ds - 1e-6 * ref["scale"]).max()))
        S = ref["k"] * ref["S"]
        dl = abs(float(loss) - float(ref["loss"]))
        print("bnd fwd N%d C%d %dx%d->%dx%d w=%d: loss %.9g ref %.9g diff %.2e (bound %.2e); sums worst diff / scale %.2e" % (
            N, C, H, W, OH, OW, w32 is not None, float(loss), float(ref["loss"]), dl, 1e-6 * S + 1e-7,
            float((ds / ref["scale"].clamp_min(1e-300)).max())))
        assert math.isfinite(float(loss)) and dl <= 1e-6 * S + 1e-7
        if C == 1:
            # p = 1: the sums are the level set's own sums
            phi = torch.from_numpy(ref["phi"]).double()[..., 0] * ((lab >= 0) & (lab < 1))
            assert (sums.cpu()[:, 0] - phi.sum((1, 2))).abs().max() <= 1e-9 * phi.abs().sum()
        # the resized form = the identity form on the resize's own output, and the same call twice: the same bits
        again = F.boundary_loss_fwd(xg, labd, (OH, OW), sdm, wd, want_sums=True)
        flat = F.boundary_loss_fwd(up, labd, (OH, OW), sdm, wd, want_sums=True)
        for a, b, c in zip((loss, coef, sums, counted), again, flat):
            assert torch.equal(a, b) and torch.equal(a, c)


def test_an_all_void_batch(F, dev):
    N, C, H, W, OH, OW = HEADS[0]
    x, _ = make_head_case(HEADS[0], 5)
    void = torch.full((N, OH, OW), 255, dtype=torch.int64, device=dev)
    void[0, 0, 0] = -100
    void[1, 2, 3] = C
    xg = gpu(x, dev).requires_grad_(True)
    sdm = F.signed_distance_maps(void, C)
    assert torch.count_nonzero(sdm) == 0
    loss, coef, sums, counted = F.boundary_loss_fwd(xg.detach(), void, (OH, OW), sdm, None, want_sums=True)
    assert float(loss) == 0.0 and float(coef) == 0.0 and int(counted) == 0 and torch.count_nonzero(sums) == 0
    out = F.upsample_softmax_losses(xg, (OH, OW), void, want_soft=False, want_ce=False, boundary=F.BoundaryLossOptions())
    assert out[:3] == (None, None, None) and float(out[3].detach()) == 0.0
    out[3].backward()
    assert torch.count_nonzero(xg.grad) == 0 and torch.isfinite(xg.grad).all()
    up = gpu(torch.randn(N, C, OH, OW, dtype=torch.float64), dev).requires_grad_(True)
    b = F.boundary_loss(up, void)
    b.backward()
    assert float(b.detach()) == 0.0 and torch.count_nonzero(up.grad) == 0


# ------------------------------------------------------------------------------------------ 3. the backward
@pytest.mark.parametrize("geom", FORWARD, ids=lambda g: "N%d-C%d-%dx%d-%dx%d" % g)
def test_flat_backward(geom, F, dev):
    """sscg_boundary_loss_bwd on the output-sized logits, through F.boundary_loss and raw on a guarded output"""
    N, C, _, _, OH, OW = geom
    g = torch.Generator().manual_seed(7 * C + OW)
    x = torch.randn(N, C, OH, OW, generator=g, dtype=torch.float64) * 2
    lab = torch.from_numpy(label_patterns(N, OH, OW, C, C + OH)["void labels"])
    labd = lab.to(dev)
    for w32 in (None, make_weights(C, C + 2)):
        wd = None if w32 is None else F.boundary_weight(w32.tolist(), C, dev)
        ref = boundary_reference(x, lab, w32)
        xg = gpu(x, dev).requires_grad_(True)
        b = F.boundary_loss(xg, labd, wd)
        F.weighted_sum([b], [0.37]).backward()
        tag = "flat N%d C%d %dx%d w=%d" % (N, C, OH, OW, w32 is not None)
        check_grad(tag, xg.grad / 0.37, ref["grad"], bnd_floor(ref, w32))
        void = ~((lab >= 0) & (lab < C))
        assert torch.count_nonzero(xg.grad.cpu().permute(0, 2, 3, 1)[void]) == 0          # a zero row for a pixel that is not counted
        # raw, between sentinels
        xh = xg.detach().permute(0, 2, 3, 1)
        assert xh.is_contiguous()
        sdm = F.signed_distance_maps(labd, C)
        _, coef, _, _ = F.boundary_loss_fwd(xg.detach(), labd, (OH, OW), sdm, wd)
        guard = torch.full((N * OH * OW * C + 64,), 7.0, device=dev)
        dx = guard[32:32 + N * OH * OW * C]
        rc = F.lib.sscg_boundary_loss_bwd(xh.data_ptr(), labd.data_ptr(), sdm.data_ptr(), N, OH, OW, C, None if wd is None else wd.data_ptr(),
                                          coef.data_ptr(), None, 0.37, dx.data_ptr(), F._stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert (guard[:32] == 7).all() and (guard[-32:] == 7).all()
        assert torch.equal(dx.view(N, OH, OW, C).permute(0, 3, 1, 2), xg.grad)


@pytest.mark.parametrize("geom", HEADS, ids=lambda g: "N%d-C%d-%dx%d-%dx%d" % g)
def test_fused_head_with_the_boundary_branch(geom, F, dev):
    N, C, H, W, OH, OW = geom
    x, lab = make_head_case(geom, 300 + C)
    labd = lab.to(dev)
    assert F._head_applies(gpu(x, dev), OH, OW)
    g = torch.Generator().manual_seed(9 + C)
    R = torch.randn(N, C, OH, OW, generator=g, dtype=torch.float64)
    Rg = gpu(R, dev)
    soft_grad = soft_reference(x, R, (OH, OW))
    w_b, w_ce, w_d = make_weights(C, C + 3), make_weights(C, C + 4), make_weights(C, C + 5)
    geo = "%dx%dx%d->%dx%d C=%d" % (N, H, W, OH, OW, C)
    th, K, f = 0.5, 0, 0.25
    y_plain = F.upsample_softmax_ce(gpu(x, dev), (OH, OW))[0]
    for wb32 in (None, w_b):
        wbd = None if wb32 is None else F.boundary_weight(wb32.tolist(), C, dev)
        bopt = F.BoundaryLossOptions(weight=wbd)
        ref = boundary_reference(x, lab, wb32, resize=(OH, OW))
        fl = bnd_floor(ref, wb32)
        wtag = " wb=%d" % (wb32 is not None)

        def check_value(tag, b):
            d = abs(float(b) - float(ref["loss"]))
            print("bnd %-62s loss %.9g ref %.9g diff %.2e" % (tag, float(b), float(ref["loss"]), d))
            assert d <= 1e-3 * ref["k"] * ref["S"] + 1e-7          # (against F.interpolate's fp64 resize: the gradient rule's 1e-3 on the scale)

        # the boundary term alone
        xg = gpu(x, dev).requires_grad_(True)
        y, ce, d, b = F.upsample_softmax_losses(xg, (OH, OW), labd, want_soft=False, want_ce=False, boundary=bopt)
        assert y is None and ce is None and d is None
        F.weighted_sum([b], [0.6]).backward()
        check_value("head %s alone%s" % (geo, wtag), b)
        check_grad("head %s alone%s" % (geo, wtag), xg.grad / 0.6, ref["grad"], fl)
        alone = xg.grad / 0.6
        # ... equals the adjoint resize of the flat backward (the separate passes) within the same rule
        was = F.FUSE_HEAD[0]
        F.FUSE_HEAD[0] = False
        try:
            xs = gpu(x, dev).requires_grad_(True)
            bs = F.upsample_softmax_losses(xs, (OH, OW), labd, want_soft=False, want_ce=False, boundary=bopt)[3]
            bs.backward()
        finally:
            F.FUSE_HEAD[0] = was
        assert torch.equal(bs.detach(), b.detach())                 # the resized forward = the flat one on the resize's output
        check_grad("head %s separate passes%s" % (geo, wtag), xs.grad, ref["grad"], fl)
        check_grad("head %s fused vs separate%s" % (geo, wtag), alone, xs.grad.double().cpu(), fl)
        # with the cross entropy: plain, then weighted and smoothed
        for cw, eps in ((None, 0.0), (w_ce, 0.1)):
            cwd = None if cw is None else F.ce_weight(cw.tolist(), C, dev)
            ce_ref = ce_reference(x, lab, cw, eps, resize=(OH, OW))
            xg = gpu(x, dev).requires_grad_(True)
            y, ce, d, b = F.upsample_softmax_losses(xg, (OH, OW), labd, want_soft=False, weight=cwd, label_smoothing=eps, boundary=bopt)
            assert y is None and d is None
            (1.3 * ce + 0.6 * b).backward()
            tag = "head %s +CE(w=%d eps=%g)%s" % (geo, cw is not None, eps, wtag)
            check_grad(tag, xg.grad, 1.3 * ce_ref[1] + 0.6 * ref["grad"], 1.3 * ce_floor(lab, cw, C) + 0.6 * fl)
            plain = F.upsample_softmax_ce(gpu(x, dev), (OH, OW), labd, want_soft=False, weight=cwd, label_smoothing=eps)[1]
            assert torch.equal(ce.detach(), plain) and torch.equal(b.detach(), bs.detach())
            # CE + Dice
            dopts = F.DiceOptions(weight=F.dice_weight(w_d.tolist(), C, dev), smooth=1.0, batch=False)
            dref = dice_reference(x, lab, w_d, 1.0, False, resize=(OH, OW))
            xg = gpu(x, dev).requires_grad_(True)
            y, ce, d, b = F.upsample_softmax_losses(xg, (OH, OW), labd, want_soft=False, weight=cwd, label_smoothing=eps, dice=dopts,
                                                    boundary=bopt)
            (1.3 * ce + 0.7 * d + 0.6 * b).backward()
            check_grad(tag + " +Dice", xg.grad, 1.3 * ce_ref[1] + 0.7 * dref["grad"] + 0.6 * ref["grad"],
                       1.3 * ce_floor(lab, cw, C) + 0.7 * ab_floor(dref) + 0.6 * fl)
            # mined CE + Dice, with the softmax map live
            opt = F.OhemOptions(th, min_kept=K, min_frac=f)
            out = F.ohem_fwd(gpu(x, dev), labd, (OH, OW), opt, cwd, eps)
            mask = (out[2] <= out[3]).cpu()
            mref = ohem_reference(x, lab, cw, eps, th, K, f, resize=(OH, OW), mask=mask)
            xg = gpu(x, dev).requires_grad_(True)
            y, ce, d, b = F.upsample_softmax_losses(xg, (OH, OW), labd, want_soft=True, weight=cwd, label_smoothing=eps, dice=dopts,
                                                    ohem=opt, boundary=bopt)
            (1.3 * ce + 0.7 * d + 0.6 * b + (y * Rg).sum()).backward()
            check_grad(tag + " mined +Dice +soft", xg.grad, 1.3 * mref["grad"] + 0.7 * dref["grad"] + 0.6 * ref["grad"] + soft_grad,
                       1.3 * mined_floor(mref, cw) + 0.7 * ab_floor(dref) + 0.6 * fl)
            assert torch.equal(y.detach(), y_plain) and torch.equal(ce.detach(), out[0]) and torch.equal(b.detach(), bs.detach())
        # dy_soft and the boundary term only
        xg = gpu(x, dev).requires_grad_(True)
        y, ce, d, b = F.upsample_softmax_losses(xg, (OH, OW), labd, want_soft=True, want_ce=False, boundary=bopt)
        assert ce is None and d is None and torch.equal(y.detach(), y_plain)
        (0.6 * b + (y * Rg).sum()).backward()
        check_grad("head %s +soft%s" % (geo, wtag), xg.grad, 0.6 * ref["grad"] + soft_grad, 0.6 * fl)


def test_the_raw_entry_without_sdm_is_the_mined_head_itself(F, dev):
    """sscg_upsample_head_bwd_b with sdm == NULL against sscg_upsample_head_bwd_h: bit for bit, every combination of the three branches"""
    N, C, H, W, OH, OW = HEADS[1]
    x, lab = make_head_case(HEADS[1], 41)
    labd = lab.to(dev)
    xg = gpu(x, dev)
    xh = xg.permute(0, 2, 3, 1)
    wd = F.ce_weight(make_weights(C, 3).tolist(), C, dev)
    out = F.ohem_fwd(xg, labd, (OH, OW), F.OhemOptions(0.5, min_frac=0.25), wd, 0.1)
    _, valid, keys, thr, _ = out
    _, coef, _ = F.dice_fwd(xg, labd, (OH, OW), None, 1.0, True)
    g = torch.Generator().manual_seed(2)
    dyn = gpu(torch.randn(N, C, OH, OW, generator=g, dtype=torch.float64), dev).permute(0, 2, 3, 1).contiguous()
    g_ce, g_dice, junk = scalar(1.3, dev), scalar(0.7, dev), scalar(float("nan"), dev)
    p = lambda t, on: t.data_ptr() if on else None
    for use_ce in (True, False):
        for use_soft in (True, False):
            for use_dice in (True, False):
                if not (use_ce or use_soft or use_dice):
                    continue
                res = []
                for entry in ("h", "b"):
                    guard = torch.full((N * H * W * C + 64,), 7.0, device=dev)
                    dx = guard[32:32 + N * H * W * C]
                    a = (xh.data_ptr(), labd.data_ptr(), p(keys, use_ce), p(thr, use_ce), wd.data_ptr(), 0.1, p(dyn, use_soft), p(g_ce, use_ce),
                         p(valid, use_ce), p(coef, use_dice), p(g_dice, use_dice), 1, dx.data_ptr(), N, H, W, C, OH, OW)
                    if entry == "h":
                        rc = F.lib.sscg_upsample_head_bwd_h(*a, F._stream())
                    else:       # sdm NULL: the three other boundary arguments are not looked at
                        rc = F.lib.sscg_upsample_head_bwd_b(*a, None, junk.data_ptr(), None, junk.data_ptr(), F._stream())
                    assert rc == 0
                    torch.cuda.synchronize()
                    assert (guard[:32] == 7).all() and (guard[-32:] == 7).all()
                    res.append(dx.clone())
                assert torch.equal(res[0], res[1]), (use_ce, use_soft, use_dice)
    # with sdm and every other branch off it is the boundary term alone, on a guarded output
    sdm = F.signed_distance_maps(labd, C)
    _, bcoef, _, _ = F.boundary_loss_fwd(xg, labd, (OH, OW), sdm, None)
    guard = torch.full((N * H * W * C + 64,), 7.0, device=dev)
    dx = guard[32:32 + N * H * W * C]
    rc = F.lib.sscg_upsample_head_bwd_b(xh.data_ptr(), labd.data_ptr(), None, None, None, 0.0, None, None, None, None, None, 0, dx.data_ptr(),
                                        N, H, W, C, OH, OW, sdm.data_ptr(), bcoef.data_ptr(), None, None, F._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert (guard[:32] == 7).all() and (guard[-32:] == 7).all()
    ref = boundary_reference(x, lab, None, resize=(OH, OW))
    check_grad("raw head, boundary only", dx.view(N, H, W, C).permute(0, 3, 1, 2), ref["grad"], bnd_floor(ref, None))


# ------------------------------------------------------------------------------------------ 4. through the model
def _args(dev, tmp_path, **kw):
    FX = __import__("oracle.fixtures", fromlist=["x"])
    return FX.make_args(dataset="acdc", crop_height=64, crop_width=64, batch_size=2, gpu_ids=[dev.index or 0], ngf=8, ndf=8,
                        checkpoint_dir=str(tmp_path / "ckpt"), as_written=True, **kw)


def test_supervised_step_reports_the_boundary_loss(F, dev, tmp_path):
    md, data = load_sub("model"), load_sub("data")
    got = {}
    for tag, kw in (("default", {}), ("zero", dict(boundary_loss=0.0, boundary_loss_skip="0", boundary_loss_ramp=3)),
                    ("on", dict(boundary_loss=0.5, boundary_loss_skip="0", boundary_loss_ramp=2, dice_weight=0.5))):
        args = _args(dev, tmp_path, model="supervised_model", **kw)
        torch.manual_seed(21)
        with contextlib.redirect_stdout(io.StringIO()):
            m = md.supervised_model(args)
            loader = data.synthetic_loaders(args, 4, steps=2)[0]
        l_img, l_gt, _ = next(iter(loader))
        l_img, l_gt = l_img.to(dev), l_gt.to(dev)
        if tag == "on":
            assert m.boundary_w == 0.5 and m.boundary_loss_options.weight.tolist() == [0.0, 1.0, 1.0, 1.0] and m._boundary_b == 0.0
            assert m.set_boundary_epoch(1) == 0.25
            with torch.no_grad():
                logits = m.Gsi(l_img).float().cpu()
        else:
            assert m.boundary_loss_options is None
        before = [p.detach().clone() for p in m.Gsi.parameters()]
        ce = float(m.step(l_img, l_gt))
        F.flush_side_work()
        torch.cuda.synchronize()
        got[tag] = (ce, [p.detach().clone() for p in m.Gsi.parameters()], dict(getattr(m, "extras", None) or {}))
        assert any(not torch.equal(a, b) for a, b in zip(before, m.Gsi.parameters()))            # the update was applied
    # the flag absent or 0: the losses and the trained weights are the default run's, bit for bit, and there is no new key
    assert got["zero"][0] == got["default"][0] and all(torch.equal(a, b) for a, b in zip(got["zero"][1], got["default"][1]))
    assert set(got["zero"][2]) == set(got["default"][2]) and "boundary_loss" not in got["default"][2]
    ce, _, extras = got["on"]
    bnd = float(extras["boundary_loss"])
    lab = l_gt.cpu().squeeze(1)
    ref = boundary_reference(logits.double(), lab, torch.tensor([0.0, 1.0, 1.0, 1.0]), resize=(64, 64))
    ce_ref = float(ce_reference(logits.double(), lab, None, 0.0, resize=(64, 64))[0])
    print("bnd supervised step: CE %.9g ref %.9g; boundary %.9g ref %.9g (scale %.3g); keys %s" % (
        ce, ce_ref, bnd, float(ref["loss"]), ref["k"] * ref["S"], sorted(extras)))
    assert set(extras) == {"boundary_loss", "dice_loss"} and math.isfinite(bnd)
    assert abs(ce - ce_ref) <= 1e-3 * abs(ce_ref) and abs(bnd - float(ref["loss"])) <= 1e-3 * ref["k"] * ref["S"] + 1e-7
    assert ce == pytest.approx(got["default"][0], rel=1e-3)         # the first forward does not depend on the loss flags


def test_semisupervised_step_takes_the_flag(F, dev, tmp_path):
    md, data = load_sub("model"), load_sub("data")
    got, weights = {}, {}
    for tag, kw in (("default", {}), ("zero", dict(boundary_loss=0.0)), ("on", dict(boundary_loss=0.5))):
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
        weights[tag] = [p.detach().clone() for net in (m.Gsi, m.Gis) for p in net.parameters()]
    assert set(got["default"]) == set(md.LOSS_KEYS) and got["zero"] == got["default"]
    assert all(torch.equal(a, b) for a, b in zip(weights["zero"], weights["default"]))
    assert set(got["on"]) - set(got["default"]) == {"lab_loss_boundary", "gt_cycle_boundary"}
    print("bnd semisupervised step: lab_loss_boundary %.6g, gt_cycle_boundary %.6g; lab_loss_CE %.6g / %.6g, lab_loss_MSE %.6g / %.6g" % (
        got["on"]["lab_loss_boundary"], got["on"]["gt_cycle_boundary"], got["on"]["lab_loss_CE"], got["default"]["lab_loss_CE"],
        got["on"]["lab_loss_MSE"], got["default"]["lab_loss_MSE"]))
    # the networks' first forward does not depend on the loss flags: the terms the flag cannot reach agree
    for k in md.LOSS_KEYS:
        assert got["on"][k] == pytest.approx(got["default"][k], rel=1e-3), k
    assert any(not torch.equal(a, b) for a, b in zip(weights["on"], weights["default"]))


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
for tag, kw in (("sup off", dict(model="supervised_model")), ("sup on", dict(model="supervised_model", boundary_loss=0.5)), ("semi off", {})):
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
    new = {"sscg_sdm_workspace", "sscg_sdm", "sscg_boundary_loss_workspace", "sscg_boundary_loss_fwd", "sscg_boundary_loss_bwd",
           "sscg_upsample_head_bwd_b"}
    calls = {}
    for tag in ("sup off", "sup on", "semi off"):
        body = r.stderr[r.stderr.index("[census] begin " + tag):r.stderr.index("[census] end " + tag)]
        names = [line[7:].split("(")[0] for line in body.splitlines() if line.startswith("[sscg] ")]
        calls[tag] = {n: names.count(n) for n in set(names)}
    assert calls["sup off"].get("sscg_upsample_head_fwd") == 1 and calls["sup off"].get("sscg_upsample_head_bwd") == 1
    assert not new & set(calls["sup off"]) and not new & set(calls["semi off"]), calls
    assert calls["semi off"].get("sscg_upsample_head_fwd") == 3 and calls["semi off"].get("sscg_upsample_head_bwd") == 3
    # the control: with the flag the log does name them - the existing forward entry, one sdm, one loss forward, ONE stencil launch backward
    on = calls["sup on"]
    assert on.get("sscg_sdm") == 1 and on.get("sscg_boundary_loss_fwd") == 1 and on.get("sscg_upsample_head_bwd_b") == 1
    assert on.get("sscg_upsample_head_fwd") == 1 and "sscg_upsample_head_bwd" not in on and "sscg_boundary_loss_bwd" not in on
    # every other launch of the step is the one it was (host-side size / applies queries are cached per process: left out)
    def launches(c):
        return {k: v for k, v in c.items() if k not in new and k not in ("sscg_upsample_head_bwd", "sscg_weighted_sum")
                and not k.endswith(("_workspace", "_bytes", "_applies"))}
    assert launches(on) == launches(calls["sup off"]), (launches(on), launches(calls["sup off"]))
