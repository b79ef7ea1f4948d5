"""Lovasz-softmax loss on the MI355X: sscg_lovasz_fwd (keys, loss, coefficient map), its backward through the existing entries
(the fused head's stencil, sscg_softmax_bwd in the flat form), composition with the other branches of the label head, determinism,
isolation, and one training step of either model - against tests/lovasz_reference.py in fp64 on the CPU.

Tolerances are those of the named existing tests:
  keys          tests/test_ohem_gpu.py: |device - fp64| <= 4 e, e = the CPU fp32 arithmetic's own distance from fp64 on these keys;
  loss          tests/test_dice_gpu.py: 1e-3 |ref| + 1e-7;
  gradient      tests/test_dice_gpu.py / test_boundary_loss_gpu.py: max-abs difference <= 1e-3 max|ref| + floor, the floor 8 fp32
                roundings of the largest term of a gradient entry - here the largest coefficient d loss / d p (a logit's gradient is a
                sum of products p (coef - sum p coef), none larger), times the weight the term has in the total.
Every test prints the distances it observed (`lovasz ...` lines; run with -s)."""
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
from lovasz_reference import EPS32, GEOMS, LABELS, OPTIONS, end_to_end, errors, lovasz_reference, make_case, probabilities

pytestmark = pytest.mark.gpu

CL = torch.channels_last
IDS = [g[0] for g in GEOMS]


def gpu(t, dev):
    return t.float().to(dev).contiguous(memory_format=CL)


def otag(o):
    return "%s%s skip=%s" % (o["classes"], " per_image" if o["per_image"] else "", list(o["skip"]))


def keys_nchw(keys, N, C, OH, OW, per_image):
    """the entry's class-major planes [segments][C][pixels] as int64 [N, C, OH, OW]"""
    k = keys.cpu().numpy().view(np.uint32).astype(np.int64)
    return k.reshape(N, C, OH, OW) if per_image else k.reshape(C, N, OH, OW).transpose(1, 0, 2, 3)


def check_loss(tag, loss, ref):
    loss, ref = float(loss), float(ref)
    d = abs(loss - ref)
    print("lovasz %-70s loss %.9g ref %.9g rel %.2e" % (tag, loss, ref, d / max(abs(ref), 1e-30)))
    assert math.isfinite(loss) and d <= 1e-3 * abs(ref) + 1e-7, (tag, loss, ref)


def check_grad(tag, grad, ref, floor):
    grad = grad.detach().double().cpu()
    dg, gmax = float((grad - ref).abs().max()), float(ref.abs().max())
    print("lovasz %-70s grad max-abs diff %.2e of %.2e rel %.2e (floor %.1e)" % (tag, dg, gmax, dg / max(gmax, 1e-30), floor))
    assert torch.isfinite(grad).all() and dg <= 1e-3 * gmax + floor, (tag, dg, gmax)


def coef_reference(p64, lab, o, keys=None):
    """(loss, d loss / d p [N, C, OH, OW]) of the reference, g held constant"""
    p = p64.clone().requires_grad_(True)
    loss = lovasz_reference(p, lab, keys=keys, **o)
    grad = torch.autograd.grad(loss, p)[0] if loss.requires_grad else torch.zeros_like(p64)
    return float(loss.detach()), grad


def head(F, xg, OH, OW, labd, opt, want_soft=False, want_ce=False, dice=None, ohem=None, boundary=None):
    """the fused node itself (functional._label_head takes it only where the resize grows the map 16-fold)"""
    return F.LabelHeadFn.apply(xg, OH, OW, labd, want_soft, want_ce, None, 0.0, dice, ohem, boundary, opt)


# ------------------------------------------------------------------------------------------ (a), (b): keys, loss and coefficient map
@pytest.mark.parametrize("labels", LABELS)
@pytest.mark.parametrize("geom", GEOMS, ids=IDS)
def test_keys_loss_and_coefficients(geom, labels, F, dev):
    name, N, C, H, W, OH, OW = geom
    x, lab = make_case(geom, labels)
    rs = None if (OH, OW) == (H, W) else (OH, OW)
    xg, labd = gpu(x, dev), lab.to(dev)
    counted = (lab >= 0) & (lab < C)
    cm = counted.unsqueeze(1).expand(N, C, OH, OW)
    fg = torch.zeros(N, C, OH, OW, dtype=torch.bool)
    fg.scatter_(1, torch.where(counted, lab, torch.zeros_like(lab)).unsqueeze(1), True)
    fg &= cm
    e64 = errors(probabilities(x, rs), lab)
    e32 = errors(probabilities(x.float(), rs), lab)
    e = float((e32.double() - e64).abs().max())
    first = None
    for o in OPTIONS:
        tag = "%s %s %s" % (name, labels, otag(o))
        loss, coef, keys, per_class = F.lovasz_fwd(xg, labd, (OH, OW), F.LovaszOptions(**o), want_class=True)
        k = keys_nchw(keys, N, C, OH, OW, o["per_image"])
        # (a) 0 at ignored pixels, bits(e) + 1 at counted ones, within the key tolerance of the mined cross entropy
        assert (k[~cm.numpy()] == 0).all() and (k[cm.numpy()] >= 1).all() and (k[cm.numpy()] <= 0x3F800001).all(), tag
        e_dev = torch.from_numpy(((k - 1) * cm.numpy()).astype(np.uint32).view(np.float32).astype(np.float64)) * cm
        dk = float((e_dev - e64).abs().max())
        assert dk <= 4 * e, (tag, dk, e)
        if first is None:
            first = k
            print("lovasz %-70s keys max |fp32 - fp64| %.2e (e %.2e)" % (tag, dk, e))
        assert np.array_equal(k, first), tag                              # the keys depend on no option
        # (b) the reference on the device's own keys: the order is decided bit for bit
        p_dev = torch.where(fg, 1.0 - e_dev, e_dev)
        ref_loss, ref_coef = coef_reference(p_dev, lab, o, keys=k)
        check_loss(tag, loss.cpu(), ref_loss)
        got = coef.cpu().permute(0, 3, 1, 2)
        gmax = float(ref_coef.abs().max())
        check_grad(tag + " coef", got, ref_coef, 8 * EPS32 * gmax)
        assert (got[ref_coef == 0] == 0).all(), tag                       # ignored pixels, skipped and absent classes: exactly 0
        assert (got[~cm] == 0).all() and all((got[:, c] == 0).all() for c in o["skip"]), tag
        assert torch.isfinite(per_class).all()
        if o["classes"] == "all" and not o["per_image"]:                  # the loss is the mean of the per-class values over the classes that take part
            live = [c for c in range(C) if c not in o["skip"]]
            assert abs(float(per_class.cpu()[live].double().mean()) - float(loss)) <= 1e-6 * max(abs(float(loss)), 1e-30) + 1e-7


# ------------------------------------------------------------------------------------------ (c) end to end: fused head and flat form
@pytest.mark.parametrize("labels", LABELS)
@pytest.mark.parametrize("geom", GEOMS, ids=IDS)
def test_end_to_end_loss_and_gradient(geom, labels, F, dev):
    name, N, C, H, W, OH, OW = geom
    x, lab = make_case(geom, labels)
    rs = None if (OH, OW) == (H, W) else (OH, OW)
    labd = lab.to(dev)
    p64 = probabilities(x, rs)
    for o in OPTIONS:
        tag = "%s %s %s" % (name, labels, otag(o))
        opt = F.LovaszOptions(**o)
        ref_loss, ref_grad = end_to_end(x, lab, rs, **o)
        floor = 8 * EPS32 * float(coef_reference(p64, lab, o)[1].abs().max())
        if rs is not None:
            xg = gpu(x, dev).requires_grad_(True)
            out = head(F, xg, OH, OW, labd, opt)
            assert len(out) == 4 and out[0] is None and out[1] is None and out[2] is None
            F.weighted_sum([out[3]], [0.6]).backward()
            check_loss(tag + " fused", out[3].detach().cpu(), ref_loss)
            check_grad(tag + " fused", xg.grad / 0.6, ref_grad, floor)
        # the public entry: the separate passes at these sizes (resize, then the flat form), the flat form itself on "flat4"
        xs = gpu(x, dev).requires_grad_(True)
        if rs is None:
            ls = F.lovasz_softmax(xs, labd, opt)
        else:
            res = F.upsample_softmax_losses(xs, (OH, OW), labd, want_soft=False, want_ce=False, lovasz=o)
            assert len(res) == 5 and all(r is None for r in res[:4])
            ls = res[4]
            assert torch.equal(ls.detach(), out[3].detach()), tag          # the resized forward = the flat one on the resize's output
        ls.backward()
        check_loss(tag + " flat", ls.detach().cpu(), ref_loss)
        check_grad(tag + " flat", xs.grad, ref_grad, floor)


# ------------------------------------------------------------------------------------------ (d) composition with every other branch
@pytest.mark.parametrize("geom", GEOMS[:2], ids=IDS[:2])
def test_composition_with_dice_ohem_boundary_and_the_softmax_map(geom, F, dev):
    name, N, C, H, W, OH, OW = geom
    x, lab = make_case(geom, "mixed")
    labd = lab.to(dev)
    g = torch.Generator().manual_seed(9 + C)
    Rg = gpu(torch.randn(N, C, OH, OW, generator=g, dtype=torch.float64), dev)
    dopts = F.DiceOptions(weight=None, smooth=1.0, batch=False)
    ohem = F.OhemOptions(0.5, min_kept=0, min_frac=0.25)
    bopt = F.BoundaryLossOptions(weight=None)
    for o in (OPTIONS[0], OPTIONS[3]):
        opt = F.LovaszOptions(**o)
        xa = gpu(x, dev).requires_grad_(True)
        y, ce, d, b, l = head(F, xa, OH, OW, labd, opt, True, True, dopts, ohem, bopt)
        (1.3 * ce + 0.7 * d + 0.6 * b + 0.9 * l + (y * Rg).sum()).backward()
        xr = gpu(x, dev).requires_grad_(True)
        y2, ce2, d2, b2 = F.LabelHeadFn.apply(xr, OH, OW, labd, True, True, None, 0.0, dopts, ohem, bopt)
        (1.3 * ce2 + 0.7 * d2 + 0.6 * b2 + (y2 * Rg).sum()).backward()
        xl = gpu(x, dev).requires_grad_(True)
        l3 = head(F, xl, OH, OW, labd, opt)[3]
        (0.9 * l3).backward()
        for u, v in ((y, y2), (ce, ce2), (d, d2), (b, b2), (l, l3)):
            assert torch.equal(u.detach(), v.detach())                     # no branch's forward sees the others
        parts = xr.grad.double().cpu() + xl.grad.double().cpu()
        check_grad("%s all branches %s" % (name, otag(o)), xa.grad, parts, 8 * EPS32 * float(parts.abs().max()))
        # without the boundary branch (the mined + Dice entry), and the softmax map alone beside the Lovasz term
        xa = gpu(x, dev).requires_grad_(True)
        y, ce, d, l = head(F, xa, OH, OW, labd, opt, True, True, dopts, ohem)
        (1.3 * ce + 0.7 * d + 0.9 * l + (y * Rg).sum()).backward()
        xr = gpu(x, dev).requires_grad_(True)
        y2, ce2, d2 = F.LabelHeadFn.apply(xr, OH, OW, labd, True, True, None, 0.0, dopts, ohem)
        (1.3 * ce2 + 0.7 * d2 + (y2 * Rg).sum()).backward()
        parts = xr.grad.double().cpu() + xl.grad.double().cpu()
        check_grad("%s mined + Dice + soft %s" % (name, otag(o)), xa.grad, parts, 8 * EPS32 * float(parts.abs().max()))
        xa = gpu(x, dev).requires_grad_(True)
        y, _, _, l = head(F, xa, OH, OW, labd, opt, True)
        (0.9 * l + (y * Rg).sum()).backward()
        xr = gpu(x, dev).requires_grad_(True)
        (F.LabelHeadFn.apply(xr, OH, OW, labd, True, False, None, 0.0, None, None)[0] * Rg).sum().backward()
        parts = xr.grad.double().cpu() + xl.grad.double().cpu()
        check_grad("%s soft only %s" % (name, otag(o)), xa.grad, parts, 8 * EPS32 * float(parts.abs().max()))


# ------------------------------------------------------------------------------------------ (e) determinism and isolation
def test_same_bits_twice_and_nothing_moves_without_the_option(F, dev):
    geom = GEOMS[1]
    name, N, C, H, W, OH, OW = geom
    x, lab = make_case(geom, "mixed")
    labd = lab.to(dev)
    opt = F.LovaszOptions(classes="present", per_image=True)
    runs = []
    for _ in range(2):
        xg = gpu(x, dev).requires_grad_(True)
        loss, coef, keys, pc = F.lovasz_fwd(xg.detach(), labd, (OH, OW), opt, want_class=True)
        l = head(F, xg, OH, OW, labd, opt)[3]
        l.backward()
        runs.append((loss, coef, keys, pc, l.detach(), xg.grad))
    for u, v in zip(*runs):
        assert torch.equal(u, v)
    # lovasz=None: the same values as the call that does not name it
    a = F.upsample_softmax_losses(gpu(x, dev), (OH, OW), labd, dice=F.DiceOptions())
    b = F.upsample_softmax_losses(gpu(x, dev), (OH, OW), labd, dice=F.DiceOptions(), lovasz=None)
    assert len(a) == len(b) == 4 and all((u is None and v is None) or torch.equal(u, v) for u, v in zip(a, b))
    # a Lovasz term nothing differentiates leaves the other branches' gradient bit for bit
    g = torch.Generator().manual_seed(4)
    Rg = gpu(torch.randn(N, C, OH, OW, generator=g, dtype=torch.float64), dev)
    grads = []
    for with_l in (False, True):
        xg = gpu(x, dev).requires_grad_(True)
        if with_l:
            y, ce, d, l = head(F, xg, OH, OW, labd, opt, True, True, F.DiceOptions())
        else:
            y, ce, d = F.LabelHeadFn.apply(xg, OH, OW, labd, True, True, None, 0.0, F.DiceOptions(), None)
        (1.3 * ce + 0.7 * d + (y * Rg).sum()).backward()
        grads.append((y.detach(), ce.detach(), d.detach(), xg.grad))
    for u, v in zip(*grads):
        assert torch.equal(u, v)


def test_all_void_call(F, dev):
    geom = GEOMS[0]
    name, N, C, H, W, OH, OW = geom
    x, _ = make_case(geom, "mixed")
    labd = torch.full((N, OH, OW), 255, dtype=torch.int64, device=dev)
    for o in OPTIONS:
        xg = gpu(x, dev).requires_grad_(True)
        l = head(F, xg, OH, OW, labd, F.LovaszOptions(**o))[3]
        l.backward()
        assert float(l) == 0.0 and torch.count_nonzero(xg.grad) == 0, otag(o)


# ------------------------------------------------------------------------------------------ (f) through the models
def _args(dev, tmp_path, **kw):
    FX = __import__("oracle.fixtures", fromlist=["x"])
    return FX.make_args(dataset="acdc", crop_height=64, crop_width=64, batch_size=2, gpu_ids=[dev.index or 0], ngf=8, ndf=8,
                        checkpoint_dir=str(tmp_path / "ckpt"), as_written=True, **kw)


def test_supervised_step_reports_the_lovasz_loss(F, dev, tmp_path):
    md, data = load_sub("model"), load_sub("data")
    got = {}
    for tag, kw in (("default", {}), ("zero", dict(lovasz_weight=0.0, lovasz_skip="0", lovasz_per_image=True)),
                    ("on", dict(lovasz_weight=0.5, lovasz_skip="0", lovasz_classes="all"))):
        args = _args(dev, tmp_path, model="supervised_model", **kw)
        torch.manual_seed(21)
        with contextlib.redirect_stdout(io.StringIO()):
            m = md.supervised_model(args)
            loader = data.synthetic_loaders(args, 4, steps=2)[0]
        l_img, l_gt, _ = next(iter(loader))
        l_img, l_gt = l_img.to(dev), l_gt.to(dev)
        if tag == "on":
            assert m.lovasz_w == 0.5 and (m.lovasz_options.classes, m.lovasz_options.per_image, m.lovasz_options.skip) == ("all", False, (0,))
            with torch.no_grad():
                logits = m.Gsi(l_img).float().cpu()
        else:
            assert m.lovasz_options is None
        ce = float(m.step(l_img, l_gt))
        F.flush_side_work()
        torch.cuda.synchronize()
        got[tag] = (ce, [p.detach().clone() for p in m.Gsi.parameters()], dict(getattr(m, "extras", None) or {}))
    # the flag absent or 0: the loss and the trained weights are the default run's, bit for bit, and there is no new key
    assert got["zero"][0] == got["default"][0] and all(torch.equal(a, b) for a, b in zip(got["zero"][1], got["default"][1]))
    assert set(got["zero"][2]) == set(got["default"][2]) and "lovasz_loss" not in got["default"][2]
    ce, weights, extras = got["on"]
    lov = float(extras["lovasz_loss"])
    ref = end_to_end(logits.double(), l_gt.cpu().squeeze(1), (64, 64), classes="all", per_image=False, skip=(0,))[0]
    print("lovasz supervised step: CE %.9g; lovasz %.9g ref %.9g; keys %s" % (ce, lov, ref, sorted(extras)))
    assert set(extras) == {"lovasz_loss"} and math.isfinite(lov) and abs(lov - ref) <= 1e-3 * abs(ref) + 1e-7
    assert ce == pytest.approx(got["default"][0], rel=1e-3)               # the first forward does not depend on the loss flags
    assert any(not torch.equal(a, b) for a, b in zip(weights, got["default"][1]))


def test_semisupervised_step_takes_the_flag(F, dev, tmp_path):
    md, data = load_sub("model"), load_sub("data")
    got, weights = {}, {}
    for tag, kw in (("default", {}), ("zero", dict(lovasz_weight=0.0)), ("on", dict(lovasz_weight=0.5, lovasz_per_image=True))):
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
    assert set(got["on"]) - set(got["default"]) == {"lab_loss_lovasz", "gt_cycle_lovasz"}
    print("lovasz semisupervised step: lab_loss_lovasz %.6g, gt_cycle_lovasz %.6g" % (got["on"]["lab_loss_lovasz"], got["on"]["gt_cycle_lovasz"]))
    assert 0.0 < got["on"]["lab_loss_lovasz"] <= 1.0 and 0.0 < got["on"]["gt_cycle_lovasz"] <= 1.0
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
for tag, kw in (("sup off", dict(model="supervised_model")), ("sup on", dict(model="supervised_model", lovasz_weight=0.5)), ("semi off", {})):
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
    new = {"sscg_sort_chunk", "sscg_sort_ws_bytes", "sscg_sort_u32_desc", "sscg_lovasz_workspace", "sscg_lovasz_fwd", "sscg_lovasz_scale_add"}
    calls = {}
    for tag in ("sup off", "sup on", "semi off"):
        body = r.stderr[r.stderr.index("[census] begin " + tag):r.stderr.index("[census] end " + tag)]
        names = [line[7:].split("(")[0] for line in body.splitlines() if line.startswith("[sscg] ")]
        calls[tag] = {n: names.count(n) for n in set(names)}
    assert calls["sup off"].get("sscg_upsample_head_fwd") == 1 and calls["sup off"].get("sscg_upsample_head_bwd") == 1
    assert not new & set(calls["sup off"]) and not new & set(calls["semi off"]), calls
    assert calls["semi off"].get("sscg_upsample_head_fwd") == 3 and calls["semi off"].get("sscg_upsample_head_bwd") == 3
    # the control: with the flag the log does name them - one loss forward, one scale-add, and still ONE stencil launch backward
    on = calls["sup on"]
    assert on.get("sscg_lovasz_fwd") == 1 and on.get("sscg_lovasz_scale_add") == 1
    assert on.get("sscg_upsample_head_fwd") == 1 and on.get("sscg_upsample_head_bwd") == 1

    def launches(c):
        return {k: v for k, v in c.items() if k not in new and k != "sscg_weighted_sum" and not k.endswith(("_workspace", "_bytes", "_applies"))}
    assert launches(on) == launches(calls["sup off"]), (launches(on), launches(calls["sup off"]))
