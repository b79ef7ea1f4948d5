"""The structural-similarity loss fused with the L1 terms on the MI355X: sscg_l1_ssim_fwd / _bwd against the fp64 restatement
(tests/ssim_reference.py), the autograd node, and one step of the semi-supervised driver with --ssim_weight.

Tolerances.  The yardstick is the fp32 twin of the reference on the same inputs, never the kernel: a loss or a per-sample mean is held
to 4 |ref32 - ref64| + 2^-20 (the floor: about 8 fp32 roundings at the loss's scale of 1; the factor: another, equally valid summation
order), a gradient to max|got - ref64| <= 4 max|ref32 - ref64| + 2^-20 max|ref64|, the L1 mean to 1e-6 relative (an fp64 sum of fp32
differences, rounded once).  The flat inputs are the cancellation regime of E[a^2] - mu_a^2: they are held to the same rule.
Every test prints what it measured (`ssim ...` lines; run with -s); profiles/ssim.txt keeps them."""
import contextlib
import io
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, load_sub
from ssim_reference import make_inputs, ssim_reference

pytestmark = pytest.mark.gpu

CL = torch.channels_last
FLOOR = 2.0 ** -20
TILE = 16                                                                   # csrc/ssim.hip: SSIM_T
# N, C, H, W, k: one output pixel; the smallest window; a 2-row map; odd sizes over several tiles; a 7-pixel window; a map of 65 x 66,
# past any tile side <= 64; and H' = TILE + 1
SHAPES = [(2, 3, 11, 11, 11), (1, 1, 3, 3, 3), (1, 3, 12, 45, 11), (2, 3, 43, 37, 11), (2, 3, 40, 70, 7), (1, 3, 75, 76, 11),
          (1, 3, TILE + 1 + 10, TILE + 2 + 10, 11)]
KINDS = ["noise", "near", "flat"]
SIGMA = {11: 1.5, 7: 1.0, 3: 0.75}
G_L1, W_L1, G_SSIM, W_SSIM = 0.7, 0.5, 1.3, 2.0

_REF = {}


def reference(shape, kind):
    """(a, b, fp64 reference, fp32 twin) of a case: computed once, shared, never modified"""
    key = (shape, kind)
    if key not in _REF:
        N, C, H, W, k = shape
        a, b = make_inputs(kind, N, C, H, W, 1000 + 7 * H + W + KINDS.index(kind))
        _REF[key] = (a, b, ssim_reference(a, b, k, SIGMA[k]), ssim_reference(a, b, k, SIGMA[k], dtype=torch.float32))
    return _REF[key]


class Guarded(object):
    """a 256-byte aligned view of `nbytes` between two 4 KiB guards of 0xFF bytes, the view itself pre-filled with `fill`"""

    def __init__(self, nbytes, fill, dev):
        self.g = 4096
        self.buf = torch.full((nbytes + 2 * self.g + 256,), 0xFF, dtype=torch.uint8, device=dev)
        self.off = self.g + (-(self.buf.data_ptr() + self.g)) % 256
        self.n = nbytes
        self.view = self.buf[self.off:self.off + nbytes]
        self.view.fill_(fill)

    def ptr(self):
        return self.view.data_ptr()

    def f32(self):
        return self.view.clone().view(torch.float32)

    def intact(self):
        return bool((self.buf[:self.off] == 0xFF).all()) and bool((self.buf[self.off + self.n:] == 0xFF).all())


def gpu(t, dev):
    return t.float().to(dev).contiguous(memory_format=CL)


def scalar(v, dev):
    return torch.full((), float(v), device=dev)


def raw_fwd(F, dev, ag, bg, shape, fill, want=(True, True, True), ws=None):
    """sscg_l1_ssim_fwd between guards -> (l1, loss, per_sample, coef) as fp32 tensors (None where not asked), the workspace"""
    N, C, H, W, k = shape
    M = N * C * (H - k + 1) * (W - k + 1)
    need = F.lib.sscg_ssim_workspace(N, H, W, C, k)
    assert need > 0
    o = F.SsimOptions(window=k, sigma=SIGMA[k])
    out = [Guarded(4, fill, dev) if want[0] else None, Guarded(4, fill, dev), Guarded(4 * N, fill, dev) if want[1] else None,
           Guarded(12 * M, fill, dev) if want[2] else None]
    ws = ws or Guarded(need, fill, dev)
    p = lambda g: None if g is None else g.ptr()
    rc = F.lib.sscg_l1_ssim_fwd(ag.data_ptr(), bg.data_ptr(), N, H, W, C, k, o.sigma, o.c1, o.c2, p(out[0]), p(out[1]), p(out[2]), p(out[3]),
                                ws.ptr(), need, F._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert all(g.intact() for g in out if g is not None) and ws.intact(), "a guard was written"
    return [None if g is None else g.f32() for g in out], ws


def raw_bwd(F, dev, ag, bg, coef, shape, g_l1, g_ssim):
    """sscg_l1_ssim_bwd into a guarded da pre-filled with 0xFF bytes (NaN as fp32): every element must be written"""
    N, C, H, W, k = shape
    da = Guarded(4 * N * C * H * W, 0xFF, dev)
    p = lambda t: None if t is None else t.data_ptr()
    rc = F.lib.sscg_l1_ssim_bwd(ag.data_ptr(), bg.data_ptr(), p(coef), N, H, W, C, k, SIGMA[k], p(g_l1), W_L1, p(g_ssim), W_SSIM, da.ptr(),
                                F._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert da.intact(), "a guard was written"
    out = da.f32()
    assert not torch.isnan(out).any(), "an element of da was not written"
    return out.view(N, H, W, C).permute(0, 3, 1, 2)


def within(tag, got, r64, r32):
    """the rule for a loss or a per-sample mean, element by element"""
    got, r64, r32 = (torch.as_tensor(t).double().cpu().reshape(-1) for t in (got, r64, r32))
    err, twin = (got - r64).abs(), (r32 - r64).abs()
    print("ssim %-44s err %.2e twin %.2e ratio %.2f bound %.2e" % (tag, float(err.max()), float(twin.max()),
                                                                  float((err / twin.clamp_min(1e-30)).max()), float((4 * twin + FLOOR).min())))
    assert torch.isfinite(got).all() and (err <= 4 * twin + FLOOR).all(), (tag, err.tolist(), twin.tolist())


def grad_within(tag, got, r64, r32):
    got, r64, r32 = got.double().cpu(), r64.double(), r32.double()
    err, twin, gmax = float((got - r64).abs().max()), float((r32 - r64).abs().max()), float(r64.abs().max())
    print("ssim %-44s grad err %.2e twin %.2e ratio %.2f of max %.2e (err/max %.2e, bound/max %.2e)" % (
        tag, err, twin, err / max(twin, 1e-30), gmax, err / gmax, (4 * twin + FLOOR * gmax) / gmax))
    assert torch.isfinite(got).all() and err <= 4 * twin + FLOOR * gmax, (tag, err, twin, gmax)


# ------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_entries_against_the_reference(shape, kind, F, dev):
    N, C, H, W, k = shape
    a, b, r64, r32 = reference(shape, kind)
    ag, bg = gpu(a, dev), gpu(b, dev)
    assert ag.permute(0, 2, 3, 1).is_contiguous()
    tag = "%-14s %-5s" % ("x".join(map(str, shape)), kind)
    # 1. forward, 4. between guards, 5. whatever the workspace and the outputs held, and twice on one workspace
    (l1, loss, per, coef), ws = raw_fwd(F, dev, ag, bg, shape, 0xFF)
    within(tag + " loss", loss, r64["loss"], r32["loss"])
    within(tag + " per_sample", per, r64["per_sample"], r32["per_sample"])
    rel = abs(float(l1) - float(r64["l1"])) / float(r64["l1"])
    print("ssim %-44s rel %.2e" % (tag + " l1", rel))
    assert rel <= 1e-6
    again, _ = raw_fwd(F, dev, ag, bg, shape, 0x00)
    third, _ = raw_fwd(F, dev, ag, bg, shape, 0x5A, ws=ws)
    for x, y, z in zip((l1, loss, per, coef), again, third):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and torch.equal(x.view(torch.int32), z.view(torch.int32))
    (_, alone, _, _), _ = raw_fwd(F, dev, ag, bg, shape, 0x11, want=(False, False, False))
    assert torch.equal(alone, loss)                                        # the optional outputs change nothing
    assert abs(float(loss) - (1.0 - float(per.double().mean()))) <= 2.0 ** -22      # (samples have one size: the loss is 1 - their mean)
    # 2. backward: the L1 term alone, the SSIM term alone, both
    coef_d = coef.to(dev)
    g1, g2 = scalar(G_L1, dev), scalar(G_SSIM, dev)
    parts = {}
    for name, (u1, u2) in (("l1", (True, False)), ("ssim", (False, True)), ("both", (True, True))):
        got = raw_bwd(F, dev, ag, bg, coef_d if u2 else None, shape, g1 if u1 else None, g2 if u2 else None)
        want = [u1 * G_L1 * W_L1 * r["grad_l1"].double() + u2 * G_SSIM * W_SSIM * r["grad_ssim"].double() for r in (r64, r32)]
        grad_within(tag + " da " + name, got, want[0], want[1])
        parts[name] = got
    # 3. without g_ssim: sscg_l1_bwd's bits
    plain = torch.full((N * C * H * W,), float("nan"), device=dev)
    assert F.lib.sscg_l1_bwd(ag.data_ptr(), bg.data_ptr(), N * C * H * W, g1.data_ptr(), W_L1, plain.data_ptr(), F._stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(parts["l1"], plain.view(N, H, W, C).permute(0, 3, 1, 2))
    # 6. the autograd node: the raw entries' bits
    o = F.SsimOptions(window=k, sigma=SIGMA[k])
    av = ag.clone().requires_grad_(True)
    t1, t2 = F.l1_ssim_loss(av, bg, o)
    assert torch.equal(t1.detach().cpu().view(1), l1.cpu()) and torch.equal(t2.detach().cpu().view(1), loss.cpu())
    F.backward(F.weighted_sum([t1, t2], [G_L1, G_SSIM]))
    got = []
    for w1, w2 in ((W_L1, W_SSIM), (1.0, 1.0)):
        da = torch.empty_like(ag, memory_format=CL)
        assert F.lib.sscg_l1_ssim_bwd(ag.data_ptr(), bg.data_ptr(), coef_d.data_ptr(), N, H, W, C, k, SIGMA[k], g1.data_ptr(), w1, g2.data_ptr(), w2,
                                      da.data_ptr(), F._stream()) == 0
        got.append(da)
    torch.cuda.synchronize()
    assert torch.equal(got[0], parts["both"]) and torch.equal(av.grad, got[1])
    av = ag.clone().requires_grad_(True)
    s = F.ssim_loss(av, bg, o)
    assert torch.equal(s.detach(), t2.detach())
    s.backward()
    grad_within(tag + " F.ssim_loss", av.grad, r64["grad_ssim"], r32["grad_ssim"])
    av = ag.clone().requires_grad_(True)
    t1, t2 = F.l1_ssim_loss(av, bg, o)
    (3.0 * t1).backward()                                                  # the SSIM output unused: its gradient arrives as NULL
    torch.cuda.synchronize()
    ref = ag.clone().requires_grad_(True)
    (3.0 * F.l1_loss(ref, bg)).backward()
    assert torch.equal(av.grad, ref.grad)
    assert torch.equal(F.ssim(ag, bg, o).cpu(), per.cpu()) and not F.ssim(av, bg, o).requires_grad


def test_default_options_and_identical_images(F, dev):
    a, _, _, _ = reference(SHAPES[3], "noise")
    ag = gpu(a, dev)
    l1, s = F.l1_ssim_loss(ag, ag.clone())
    assert float(l1) == 0.0 and abs(float(s)) <= FLOOR and (F.ssim(ag, ag.clone()) - 1.0).abs().max() <= FLOOR
    with pytest.raises(load_sub("_lib").SscgError):
        F.ssim_loss(ag[:, :, :10], ag[:, :, :10])                          # smaller than the window


# ------------------------------------------------------------------------------------------ 2. through the model
def _args(dev, tmp_path, **kw):
    FX = __import__("oracle.fixtures", fromlist=["x"])
    return FX.make_args(dataset="acdc", crop_height=64, crop_width=64, batch_size=2, gpu_ids=[dev.index or 0], ngf=8, ndf=8,
                        checkpoint_dir=str(tmp_path / "ckpt"), as_written=True, **kw)


def _one_step(F, dev, tmp_path, monkeypatch, kw):
    md, data = load_sub("model"), load_sub("data")
    args = _args(dev, tmp_path, **kw)
    torch.manual_seed(22)
    with contextlib.redirect_stdout(io.StringIO()):
        m = md.semisuper_cycleGAN(args)
        labeled, unlabeled, _ = data.synthetic_loaders(args, 4, steps=1)
    (l_img, l_gt, _), (unl_img, _, _) = next(iter(labeled)), next(iter(unlabeled))
    seen = []
    orig = F.l1_ssim_loss
    monkeypatch.setattr(F, "l1_ssim_loss", lambda a, b, o: seen.append((a.detach().float().cpu(), b.detach().float().cpu(), o)) or orig(a, b, o))
    torch.manual_seed(23)
    losses = m.step(l_img.to(dev), l_gt.to(dev), unl_img.to(dev))
    m.sync_losses()
    monkeypatch.undo()
    got = {k: float(v) for k, v in losses.items()}
    assert all(math.isfinite(v) for v in got.values()), got
    F.flush_side_work()
    torch.cuda.synchronize()
    return got, [p.detach().clone() for net in (m.Gsi, m.Gis) for p in net.parameters()], seen, m


def _check_term(tag, value, pair):
    a, b, o = pair
    r64 = ssim_reference(a, b, o.window, o.sigma, o.data_range)
    r32 = ssim_reference(a, b, o.window, o.sigma, o.data_range, dtype=torch.float32)
    within(tag, value, r64["loss"], r32["loss"])


def test_semisupervised_step_takes_the_flag(F, dev, tmp_path, monkeypatch):
    md = load_sub("model")
    got, weights = {}, {}
    for tag, kw in (("default", {}), ("zero", dict(ssim_weight=0.0, ssim_window=7)), ("on", dict(ssim_weight=0.5))):
        got[tag], weights[tag], seen, m = _one_step(F, dev, tmp_path, monkeypatch, kw)
        assert (m.ssim_options is not None) == (tag == "on") and len(seen) == (tag == "on")
    assert set(got["default"]) == set(md.LOSS_KEYS) and got["zero"] == got["default"]
    assert all(torch.equal(a, b) for a, b in zip(weights["zero"], weights["default"]))
    assert set(got["on"]) - set(got["default"]) == {"lab_loss_ssim"}
    print("ssim semisupervised step: lab_loss_ssim %.6g; lab_loss_MSE %.6g / %.6g" % (
        got["on"]["lab_loss_ssim"], got["on"]["lab_loss_MSE"], got["default"]["lab_loss_MSE"]))
    for k in md.LOSS_KEYS:          # the networks' first forward does not depend on the loss flags
        assert got["on"][k] == pytest.approx(got["default"][k], rel=1e-3), k
    assert any(not torch.equal(a, b) for a, b in zip(weights["on"], weights["default"]))
    assert seen[0][0].shape == (2, 3, 64, 64) and 0.0 < got["on"]["lab_loss_ssim"] < 2.0
    _check_term("step lab_loss_ssim", got["on"]["lab_loss_ssim"], seen[0])


def test_the_l1_cycle_variant_takes_the_flag(F, dev, tmp_path, monkeypatch):
    md = load_sub("model")
    off, w_off, seen, _ = _one_step(F, dev, tmp_path, monkeypatch, dict(variants="l1_cycle"))
    assert not seen and set(off) == set(md.LOSS_KEYS) | {"img_cycle_l1"}
    on, w_on, seen, _ = _one_step(F, dev, tmp_path, monkeypatch, dict(variants="l1_cycle", ssim_weight=0.5, ssim_window=7, ssim_sigma=1.0))
    assert set(on) - set(off) == {"lab_loss_ssim", "img_cycle_ssim"} and len(seen) == 2
    for k in off:
        assert on[k] == pytest.approx(off[k], rel=1e-3), k
    assert any(not torch.equal(a, b) for a, b in zip(w_on, w_off))
    assert all(o.window == 7 and o.sigma == 1.0 for _, _, o in seen)
    _check_term("step img_cycle_ssim (l1_cycle)", on["img_cycle_ssim"], seen[0])
    _check_term("step lab_loss_ssim (l1_cycle)", on["lab_loss_ssim"], seen[1])


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
for tag, kw in (("semi off", {}), ("semi on", dict(ssim_weight=0.5)), ("cycle off", dict(variants="l1_cycle")),
                ("cycle on", dict(variants="l1_cycle", ssim_weight=0.5))):
    a = args(**kw)
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        m = md.semisuper_cycleGAN(a)
    labeled, unlabeled, _ = data.synthetic_loaders(a, 4, steps=1)
    (l_img, l_gt, _), (unl_img, _, _) = next(iter(labeled)), next(iter(unlabeled))
    l_img, l_gt, unl_img = l_img.to(dev), l_gt.to(dev), unl_img.to(dev)
    torch.cuda.synchronize()
    sys.stderr.write("[census] begin %%s\n" %% tag)
    m.step(l_img, l_gt, unl_img)
    m.sync_losses()
    load_sub("functional").flush_side_work()
    torch.cuda.synchronize()
    sys.stderr.write("[census] end %%s\n" %% tag)
"""


def test_launch_census_of_a_step(tmp_path):
    env = dict(os.environ, SSCG_TRACE="1")
    for k in ("SSCG_RACECHECK", "SSCG_FUZZ", "SSCG_FUSE_HEAD"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", CENSUS % (ROOT, os.path.join(ROOT, "tests"), str(tmp_path / "ckpt"))], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    new = {"sscg_ssim_workspace", "sscg_l1_ssim_fwd", "sscg_l1_ssim_bwd"}
    calls = {}
    for tag in ("semi off", "semi on", "cycle off", "cycle on"):
        body = r.stderr[r.stderr.index("[census] begin " + tag):r.stderr.index("[census] end " + tag)]
        names = [line[7:].split("(")[0] for line in body.splitlines() if line.startswith("[sscg] ")]
        calls[tag] = {n: names.count(n) for n in set(names)}

    def launches(c):        # (host-side size / applies queries are cached per process: left out)
        return {k: v for k, v in c.items() if k not in new and k not in ("sscg_l1_fwd", "sscg_l1_bwd", "sscg_weighted_sum")
                and not k.endswith(("_workspace", "_bytes", "_applies"))}

    for off, on, fused in (("semi off", "semi on", 1), ("cycle off", "cycle on", 2)):
        assert not new & set(calls[off]), calls[off]
        assert calls[off].get("sscg_l1_fwd") == fused and calls[off].get("sscg_l1_bwd") == fused
        assert calls[on].get("sscg_l1_ssim_fwd") == fused and calls[on].get("sscg_l1_ssim_bwd") == fused
        assert calls[on].get("sscg_l1_fwd", 0) == 0 and calls[on].get("sscg_l1_bwd", 0) == 0
        assert launches(calls[on]) == launches(calls[off]), (launches(calls[on]), launches(calls[off]))
