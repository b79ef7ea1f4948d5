"""Optimiser options of the flat-arena Adam on the MI355X: sscg_grad_norm, sscg_adam_step_ex, FusedAdam's clip / decay / EMA and the
two models' steps with them.

Launch geometry (csrc/optim_ex.hip): sscg_adam_step_ex caps its grid like the plain launch (16384 blocks of 256, one element per
thread and pass); sscg_grad_norm caps at 2048 blocks of 256 threads with four elements per thread and pass.  Both are run beyond one
pass.  Every size runs from a 16-byte-aligned pointer and from one that is a float further.

Tolerances: the norm within 2^-22 relative of numpy's fp64 norm of the fp32-rounded grad * grad_scale (one fp32 rounding of the
square root plus margin); the arithmetic within test_kernels_gpu.py::test_adam_matches_torch's 1e-6; everything else is equality
of bits."""
import contextlib
import io

import numpy as np
import pytest
import torch

from conftest import load_sub

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
ADAM_PASS = 16384 * 256
NORM_PASS = 2048 * 256 * 4
SIZES = [1, 3, 63, 64, 65, 257, 10007, NORM_PASS + 1031, ADAM_PASS + 1031]
SCALES = [1e-3, 1.0, 1e3]
NORM_TOL = 2.0 ** -22
TOL = 1e-6


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def bits(t):
    """fp32 / bf16 values as integers (equality of bits: -0 != +0, NaN == NaN); integer tensors (a norm layer's step counter) as they are."""
    t = t.detach()
    return t.view(torch.int16 if t.dtype == BF else torch.int32) if t.is_floating_point() else t


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def split3_ref(x):
    """sscg_split3 (csrc/common.h) on the CPU: h = bf16(x), m = bf16(x - h), l = bf16((x - h) - m)."""
    h = x.to(BF)
    r1 = x - h.float()
    m = r1.to(BF)
    return torch.stack([h, m, (r1 - m.float()).to(BF)])


def at(dev, values, off, dtype=torch.float32):
    """`values` on the device, `off` elements into a larger buffer (off = 1: a pointer that is not 16-byte aligned)."""
    buf = torch.zeros(values.numel() + 8, dtype=dtype, device=dev)
    v = buf[off:off + values.numel()]
    v.copy_(values)
    return v


# ------------------------------------------------------------------------------------------ sscg_grad_norm
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_grad_norm(F, dev, n, off):
    gen = torch.Generator().manual_seed(n + off)
    base = torch.randn(n, generator=gen)
    worst = 0.0
    for si, scale in enumerate(SCALES):
        g_cpu = base * scale
        g = at(dev, g_cpu, off)
        assert g.data_ptr() % 16 == 4 * off
        for gs in (1.0, 0.125):
            t = (g_cpu.numpy() * np.float32(gs)).astype(np.float32)
            ref = float(np.sqrt(np.sum(t.astype(np.float64) ** 2)))
            for factor in (0.5, 2.0):           # max_norm below the norm (clips) and above it (does not)
                max_norm = float(np.float32(ref * factor))
                norm, clip = F.grad_norm(g, max_norm, gs)
                norm2, clip2 = F.grad_norm(g, max_norm, gs)
                got, c = norm.cpu().numpy(), clip.cpu().numpy()
                err = abs(float(got) - ref) / ref
                worst = max(worst, err)
                assert err < NORM_TOL, (n, off, scale, gs, err)
                want = np.minimum(np.float32(1.0), np.float32(max_norm) / (got + np.float32(1e-6)))
                assert c.dtype == np.float32 and c.tobytes() == np.float32(want).tobytes(), (n, off, scale, gs, factor, c, want)
                assert (float(c) < 1.0) == (factor < 1.0)
                assert same(norm, norm2) and same(clip, clip2)
    print("grad_norm n=%d off=%d: worst relative distance from the fp64 norm %.3e (bound %.3e)" % (n, off, worst, NORM_TOL))


def test_grad_norm_non_finite_propagates_as_in_torch(F, dev):
    g = torch.randn(1000, generator=torch.Generator().manual_seed(0))
    for bad, want_norm in ((float("inf"), float("inf")), (float("nan"), float("nan"))):
        gb = g.clone()
        gb[517] = bad
        p = torch.nn.Parameter(torch.zeros(1000))
        p.grad = gb.clone()
        torch.nn.utils.clip_grad_norm_([p], 1.0)         # torch: coefficient 0 for an inf norm, NaN for a NaN norm
        norm, clip = F.grad_norm(gb.to(dev), 1.0)
        ref_clip = 0.0 if bad == float("inf") else float("nan")
        assert str(float(norm)) == str(want_norm) and str(float(clip)) == str(ref_clip)
        assert torch.isnan(p.grad).any()
    print("grad_norm: inf -> (inf, 0), nan -> (nan, nan)")


# ------------------------------------------------------------------------------------------ sscg_adam_step_ex: bit contracts
HYPER = dict(lr=1e-2, beta1=0.5, beta2=0.999, eps=1e-8)


def _state(n, seed):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen) * 0.05
    grads = [torch.randn(n, generator=gen) * SCALES[(seed + s) % 3] for s in range(3)]
    lo, hi = n // 2, min(n, n // 2 + 64)           # a stretch of arena padding: zero parameter, zero gradient
    p[lo:hi] = 0.0
    for g in grads:
        g[lo:hi] = 0.0
    return p, grads, (lo, hi)


def _run(F, dev, p0, grads, off, shadow, gs=1.0, **opt):
    """Three steps from p0 with the gradients `grads` (device tensors, already at their offset); opt: plain (sscg_adam_step itself),
    clip (a float), weight_decay, decoupled, ema_decay.  Returns p, m, v, shadow, ema."""
    n = p0.numel()
    p, m, v = at(dev, p0, off), at(dev, p0, off).zero_(), at(dev, p0, off).zero_()
    sh16 = torch.zeros(n + 8, dtype=BF, device=dev)[off:off + n] if shadow == "bf16" else None
    sh3 = torch.zeros(3 * n + 8, dtype=BF, device=dev)[off:off + 3 * n] if shadow == "split" else None
    ema = at(dev, p0, off) if opt.get("ema_decay") is not None else None
    clip = torch.full((), opt["clip"], dtype=torch.float32, device=dev) if opt.get("clip") is not None else None
    for s, gd in enumerate(grads):
        if opt.get("plain"):
            F.adam_step(p, gd, m, v, HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], s + 1, gs, shadow_bf16=sh16, shadow_split=sh3)
        else:
            F.adam_step_ex(p, gd, m, v, HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], s + 1, gs, shadow_bf16=sh16,
                           shadow_split=sh3, clip=clip, weight_decay=opt.get("weight_decay", 0.0), decoupled=opt.get("decoupled", False),
                           ema=ema, ema_decay=opt.get("ema_decay") or 0.0)
    return p, m, v, (sh16 if sh16 is not None else sh3), ema


@pytest.mark.parametrize("shadow", [None, "bf16", "split"])
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_bit_contracts(F, dev, n, off, shadow):
    p0, grads, (lo, hi) = _state(n, n + off)
    p0, grads = p0.to(dev), [at(dev, g, off) for g in grads]
    for gs in (1.0, 1.0 / 3.0):       # 1/3: grad * grad_scale is inexact, the plain kernel feeds the first moment the unrounded product
        plain = _run(F, dev, p0, grads, off, shadow, gs, plain=True)
        # (a) no option: the plain launch itself
        # (b) a clip of exactly 1.0 and / or an EMA nobody reads: the plain launch's bits
        for opt in ({}, dict(clip=1.0), dict(ema_decay=0.9), dict(clip=1.0, ema_decay=0.9)):
            got = _run(F, dev, p0, grads, off, shadow, gs, **opt)
            for name, a, b in zip(("param", "exp_avg", "exp_avg_sq", "shadow"), got[:4], plain[:4]):
                assert (a is None and b is None) or same(a, b), (n, off, shadow, gs, opt, name)
    # (c) padding stays exactly zero under every option, in param and in ema
    for opt in (dict(clip=0.5, ema_decay=0.9), dict(weight_decay=0.1, ema_decay=0.9), dict(weight_decay=0.1, decoupled=True, ema_decay=0.9),
                dict(clip=0.5, weight_decay=0.1, decoupled=True, ema_decay=0.9), dict(clip=0.5, weight_decay=0.1, ema_decay=0.9)):
        p, m, v, sh, ema = _run(F, dev, p0, grads, off, shadow, 1.0, **opt)
        for t in (p, ema, m, v):
            assert not bool(bits(t[lo:hi]).any()), (n, off, shadow, opt)
        if hi - lo < n:
            assert bool(torch.isfinite(p).all()) and bool((p != p0).any())
    print("adam_step_ex n=%d off=%d shadow=%s: distance 0 bits from sscg_adam_step in (a), (b); padding [%d, %d) exactly zero" % (
        n, off, shadow, lo, hi))


# ------------------------------------------------------------------------------------------ sscg_adam_step_ex: arithmetic
def _reference(p0, grads, weight_decay=0.0, decoupled=False, max_norm=None, ema_decay=None):
    """Three steps of torch on the CPU in fp64: Adam(weight_decay=) / AdamW, clip_grad_norm_ in front, ema.lerp_(p, 1 - decay)."""
    p = torch.nn.Parameter(p0.double().clone())
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([p], lr=HYPER["lr"], betas=(HYPER["beta1"], HYPER["beta2"]), eps=HYPER["eps"], weight_decay=weight_decay)
    ema = p0.double().clone()
    for g in grads:
        p.grad = g.double().clone()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_([p], max_norm)
        opt.step()
        if ema_decay is not None:
            ema.lerp_(p.detach(), 1.0 - ema_decay)
    return p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], ema


ARITH = {"l2": (dict(weight_decay=0.1), "param"), "adamw": (dict(weight_decay=0.1, decoupled=True), "param"),
         "clip": (dict(max_norm=5.0), "exp_avg"), "ema": (dict(ema_decay=0.9), "ema"),
         "all_l2": (dict(weight_decay=0.1, max_norm=5.0, ema_decay=0.9), "param"),
         "all_adamw": (dict(weight_decay=0.1, decoupled=True, max_norm=5.0, ema_decay=0.9), "param")}


@pytest.mark.parametrize("shadow", ["bf16", "split"])
@pytest.mark.parametrize("which", sorted(ARITH))
def test_arithmetic_matches_torch(F, dev, which, shadow):
    """lr 1e-2, weight_decay 0.1, ema_decay 0.9, max_norm 5 against gradient norms of ~100 (randn, n = 10007).  The reference
    without the option must be > 100 tolerances from the one with it in the quantity the option acts on (decay: param; clip: the
    first moment - Adam's update direction is nearly invariant to a gradient scale; ema: the EMA against the parameter it would be
    without averaging), so a dropped option cannot pass."""
    opt, target = ARITH[which]
    n, off = 10007, 1
    gen = torch.Generator().manual_seed(77)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) for _ in range(3)]
    ref = dict(zip(("param", "exp_avg", "exp_avg_sq", "ema"), _reference(p0, grads, **opt)))
    without = dict(zip(("param", "exp_avg", "exp_avg_sq", "ema"), _reference(p0, grads)))
    without["ema"] = ref["param"]
    apart = rel_err(without[target], ref[target])
    assert apart > 100 * TOL, (which, target, apart)

    p, m, v = at(dev, p0, off), at(dev, torch.zeros(n), off), at(dev, torch.zeros(n), off)
    sh16 = torch.zeros(n + 8, dtype=BF, device=dev)[off:off + n] if shadow == "bf16" else None
    sh3 = torch.zeros(3 * n + 8, dtype=BF, device=dev)[off:off + 3 * n] if shadow == "split" else None
    ema = at(dev, p0, off) if "ema_decay" in opt else None
    clip = None
    for s, g in enumerate(grads):
        gd = at(dev, g, off)
        if "max_norm" in opt:
            _, clip = F.grad_norm(gd, opt["max_norm"])
            assert float(clip) < 0.1
        F.adam_step_ex(p, gd, m, v, HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], s + 1, 1.0, shadow_bf16=sh16,
                       shadow_split=sh3, clip=clip, weight_decay=opt.get("weight_decay", 0.0), decoupled=opt.get("decoupled", False),
                       ema=ema, ema_decay=opt.get("ema_decay", 0.0))
    got = dict(param=p, exp_avg=m, exp_avg_sq=v, ema=ema)
    dist = {k: rel_err(got[k], ref[k]) for k in got if got[k] is not None}
    print("adam_step_ex %s (%s shadow): distances from torch fp64 %s (bound %.0e); the reference without the option is %.3e away in %s" % (
        which, shadow, ", ".join("%s %.3e" % kv for kv in dist.items()), TOL, apart, target))
    assert all(d < TOL for d in dist.values()), dist
    # the written shadow is the cast / the split of the new param, bit for bit
    if shadow == "bf16":
        assert same(sh16.cpu(), p.cpu().to(BF))
    else:
        assert same(torch.as_strided(sh3, (3, n), (n, 1)).cpu(), split3_ref(p.cpu()))


# ------------------------------------------------------------------------------------------ FusedAdam
SHAPES = [(1,), (63,), (64,), (65,), (1000,), (64, 3, 3, 64)]       # the last: a conv weight [K, R, S, C] as arch.ops.Conv2d keeps it
                                                                    # (64 channels: the narrowest the bf16 conv kernels take)


def _params(dev, seed):
    gen = torch.Generator().manual_seed(seed)
    ps = []
    for s in SHAPES:
        w = torch.randn(*s, generator=gen) * 0.1
        if len(s) == 4:
            w = w.permute(0, 3, 1, 2)          # logical [K, C, R, S], channels-last memory
        ps.append(torch.nn.Parameter(w.to(dev)))
    return ps


def _fused(dev, seed=5, **kw):
    optim = load_sub("optim")
    ps = _params(dev, seed)
    start = [p.detach().cpu().clone() for p in ps]
    return optim.FusedAdam(ps, lr=1e-2, betas=(0.5, 0.999), **kw), ps, start


def test_fused_adam_all_options_match_torch(F, dev):
    kw = dict(weight_decay=0.1, decoupled=True, max_grad_norm=1.0, ema_decay=0.9)
    opt, ps, start = _fused(dev, **kw)
    plain_keys = _fused(dev)[0].state_dict()
    ref_p = [torch.nn.Parameter(s.double().clone()) for s in start]
    ref = torch.optim.AdamW(ref_p, lr=1e-2, betas=(0.5, 0.999), weight_decay=0.1)
    ref_ema = [s.double().clone() for s in start]
    gen = torch.Generator().manual_seed(6)
    for step in range(3):
        opt.zero_grad()
        for p, r in zip(ps, ref_p):
            g = torch.randn(r.shape, generator=gen)
            p.grad.copy_(g.to(dev))
            r.grad = g.double()
        total = torch.nn.utils.clip_grad_norm_(ref_p, 1.0)
        opt.step()
        ref.step()
        for e, r in zip(ref_ema, ref_p):
            e.lerp_(r.detach(), 1.0 - 0.9)
        nerr = abs(float(opt.last_grad_norm) - float(total)) / float(total)
        assert nerr < NORM_TOL and float(total) > 1.0
    names = [("p%d" % i, p) for i, p in enumerate(ps)]
    ema_sd = opt.ema_state_dict(names)
    d_p = max(rel_err(p, r) for p, r in zip(ps, ref_p))
    d_e = max(rel_err(ema_sd["p%d" % i], e) for i, e in enumerate(ref_ema))
    d_m = max(rel_err(opt._view(opt.exp_avg, p, opt.slices[p][0]), ref.state[r]["exp_avg"]) for p, r in zip(ps, ref_p))
    d_v = max(rel_err(opt._view(opt.exp_avg_sq, p, opt.slices[p][0]), ref.state[r]["exp_avg_sq"]) for p, r in zip(ps, ref_p))
    print("FusedAdam, all options, against clip_grad_norm_ + AdamW in fp64: param %.3e, exp_avg %.3e, exp_avg_sq %.3e, ema %.3e (bound %.0e); "
          "norm %.3e (bound %.3e)" % (d_p, d_m, d_v, d_e, TOL, nerr, NORM_TOL))
    assert max(d_p, d_m, d_v, d_e) < TOL
    # the padding between the slices is still exactly zero, in the arena and in the EMA
    pad = torch.ones(opt.arena.numel(), dtype=torch.bool, device=dev)
    for off, n in opt.slices.values():
        pad[off:off + n] = False
    assert int(pad.sum()) > 0 and not bool(bits(opt.arena[pad]).any()) and not bool(bits(opt.ema[pad]).any())
    # state_dict(): torch.optim.Adam's format, the keys of an optimiser without options
    sd = opt.state_dict()
    assert set(sd) == set(plain_keys) and set(sd["param_groups"][0]) == set(plain_keys["param_groups"][0]) == {"lr", "betas", "eps", "params"}
    assert len(sd["state"]) == len(ps) and all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in sd["state"].values())
    # the EMA round-trips through a second optimiser
    opt2, ps2, _ = _fused(dev, seed=9, ema_decay=0.5)
    names2 = [("p%d" % i, p) for i, p in enumerate(ps2)]
    opt2.load_ema_state_dict(names2, {k: v.cpu() for k, v in ema_sd.items()})
    back = opt2.ema_state_dict(names2)
    assert list(back) == list(ema_sd) and all(same(back[k], ema_sd[k]) for k in back)
    assert same(opt2.ema, opt.ema)


def test_fused_adam_without_options_makes_the_plain_call(F, dev, monkeypatch):
    calls = []
    monkeypatch.setattr(F, "adam_step_ex", lambda *a, **k: calls.append("ex"))
    monkeypatch.setattr(F, "grad_norm", lambda *a, **k: calls.append("norm"))
    real = F.adam_step
    monkeypatch.setattr(F, "adam_step", lambda *a, **k: (calls.append("plain"), real(*a, **k)))
    opt, ps, _ = _fused(dev)
    assert opt.ema is None and opt.last_grad_norm is None
    ps[0].grad.fill_(1.0)
    opt.step()
    assert calls == ["plain"]
    with opt.ema_weights():            # no EMA: nothing changes
        pass
    assert opt.ema is None


@pytest.mark.parametrize("mode", ["f32s", "bf16"])
def test_ema_weights_swaps_values_and_operand_copies(F, dev, mode):
    prev = F.get_conv_precision()
    F.set_conv_precision(mode)
    try:
        opt, ps, _ = _fused(dev, ema_decay=0.9)
        w = ps[-1]
        gen = torch.Generator().manual_seed(3)
        x = (torch.randn(2, 64, 9, 11, generator=gen)).to(dev).contiguous(memory_format=torch.channels_last)
        x = F.cast(x, BF) if mode == "bf16" else x
        with torch.no_grad():
            F.conv2d(x, w, None, 1, 1, 1)          # first use builds the operand copies of this mode
            opt.ensure_operand_copies()
            for _ in range(2):
                opt.zero_grad()
                for p in ps:
                    p.grad.copy_(torch.randn(p.shape, generator=gen).to(dev))
                opt.step()
            y_trained = F.conv2d(x, w, None, 1, 1, 1)
            n = opt.arena.numel()
            copy = lambda: (opt.arena_x3 if mode == "f32s" else opt.arena16).clone()
            arena0, copy0, ema0 = opt.arena.clone(), copy(), opt.ema.clone()
            assert not same(arena0, ema0)
            with opt.ema_weights():
                assert same(opt.arena, ema0) and same(opt.ema, ema0)
                for p in ps:
                    off, k = opt.slices[p]
                    assert same(p.detach().reshape(-1) if p.dim() == 1 else p.detach().permute(0, 2, 3, 1).reshape(-1), ema0[off:off + k])
                if mode == "f32s":         # the copies equal a fresh sscg_split3 / sscg_cast of the EMA values
                    fresh = torch.empty(3 * n, dtype=BF, device=dev)
                    F.check(F.lib.sscg_split3(ema0.data_ptr(), fresh.data_ptr(), n, n, F._stream()), "sscg_split3")
                    assert same(opt.arena_x3, fresh) and same(fresh.view(3, n).cpu(), split3_ref(ema0.cpu()))
                else:
                    assert same(opt.arena16, F.cast(ema0, BF)) and same(opt.arena16.cpu(), ema0.cpu().to(BF))
                y_ema = F.conv2d(x, w, None, 1, 1, 1)
                with opt.ema_weights():        # nested: no second swap
                    assert same(opt.arena, ema0)
                assert same(opt.arena, ema0)
                with pytest.raises(RuntimeError):
                    opt.step()
            # after exit: the old bits, in the arena and in the copies
            assert same(opt.arena, arena0) and same(copy(), copy0) and same(opt.ema, ema0)
            assert same(F.conv2d(x, w, None, 1, 1, 1), y_trained)
            # the forward inside the block is the forward of a weight holding those values, written in by hand
            off, k = opt.slices[w]
            hand = torch.nn.Parameter(torch.empty(64, 3, 3, 64, device=dev).permute(0, 3, 1, 2))
            hand.data.permute(0, 2, 3, 1).reshape(-1).copy_(ema0[off:off + k])
            y_hand = F.conv2d(x, hand, None, 1, 1, 1)
            assert same(y_ema, y_hand) and not same(y_ema, y_trained)
            print("ema_weights (%s): copies and forward equal the hand-written EMA weights bit for bit; relative distance of the EMA "
                  "forward from the trained one %.3e" % (mode, rel_err(y_ema.float(), y_trained.float())))
    finally:
        F.set_conv_precision(prev)


# ------------------------------------------------------------------------------------------ the two models' steps
def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _weights(nets):
    return {"%s.%s" % (k, n): t.detach().clone() for k, net in nets.items() for n, t in net.state_dict().items()}


def _host_norm(opt):
    t = (opt.grad.cpu().numpy() * np.float32(1.0 / opt.world_size)).astype(np.float32)
    return float(np.sqrt(np.sum(t.astype(np.float64) ** 2)))


def _same_iou(a, b):
    return list(a) == list(b) and np.array_equal(np.array(list(a.values()), dtype=np.float64), np.array(list(b.values()), dtype=np.float64),
                                                 equal_nan=True)


def _val_batches(C, H, W, seed):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(2, 3, H, W, generator=gen), torch.randint(0, C, (2, 1, H, W), generator=gen), ["v"] * 2) for _ in range(2)]


def test_semisupervised_step_with_options(F, dev, tmp_path):
    from oracle import fixtures as FX
    md = load_sub("model")
    C, H = 21, 64

    def build(tag, **kw):
        args = FX.make_args(dataset="voc2012", crop_height=H, crop_width=H, batch_size=2, gpu_ids=[dev.index or 0],
                            checkpoint_dir=str(tmp_path / tag), as_written=True, no_dropout=True, **kw)
        return _quiet(md.semisuper_cycleGAN, args)
    nets = lambda m: {k: getattr(m, k) for k in ("Gis", "Gsi", "Di", "Ds", "old_Gis", "old_Gsi", "old_Di")}
    torch.manual_seed(31)
    a = build("a")
    b = build("b", clip_grad_norm=1e30, ema_decay=0.9)
    assert b.g_optimizer.ema_decay == 0.9 and b.d_optimizer.ema_decay is None and b.d_optimizer.max_grad_norm == 1e30
    for k, net in nets(a).items():
        nets(b)[k].load_state_dict(net.state_dict())
    batch = [t.to(dev) for t in FX.step_batch("opt", 0, C, H, H, 2)]
    out = {}
    for tag, m in (("a", a), ("b", b)):
        np.random.seed(0)
        torch.manual_seed(32)
        losses = []
        for _ in range(2):
            r = m.step(*batch)
            m.sync_losses()
            losses.append({k: v.detach().clone() for k, v in r.items()})
        torch.cuda.synchronize()
        out[tag] = (losses, _weights(nets(m)))
    for la, lb in zip(out["a"][0], out["b"][0]):
        assert all(same(la[k], lb[k]) for k in la), "a clip that does not trigger and an unread EMA changed a loss"
    assert all(same(out["a"][1][k], out["b"][1][k]) for k in out["a"][1]), "... changed a weight"
    assert not same(b.g_optimizer.ema, b.g_optimizer.arena)
    print("semisuper_cycleGAN, 2 steps, clip 1e30 + EMA: 9 losses x 2 and %d tensors equal the plain run bit for bit" % len(out["a"][1]))
    # a clip that triggers: the norm the step found is the norm of the gradient arena
    for o in (b.g_optimizer, b.d_optimizer):
        o.max_grad_norm = 1e-3
    np.random.seed(0)
    b.step(*batch)
    b.sync_losses()
    torch.cuda.synchronize()
    for name, o in (("G", b.g_optimizer), ("D", b.d_optimizer)):
        ref, got = _host_norm(o), float(o.last_grad_norm)
        print("semisuper_cycleGAN %s: last_grad_norm %.9e, fp64 norm of the arena %.9e, relative distance %.3e (bound %.3e); clip %.3e" % (
            name, got, ref, abs(got - ref) / ref, NORM_TOL, float(o._clip)))
        assert abs(got - ref) / ref < NORM_TOL and float(o._clip) < 1.0
    # evaluate() with an EMA = evaluate() of a model whose weights were set to the EMA values by hand
    val = _val_batches(C, H, H, 33)
    miou_b, iou_b = b.evaluate(val)
    conf_b = b.running_metrics_val.confusion_matrix.copy()
    for k in ("Gis", "Gsi"):
        sd = {n: t.clone() for n, t in getattr(b, k).state_dict().items()}
        sd.update(b.g_optimizer.ema_state_dict(getattr(b, k)))
        getattr(a, k).load_state_dict(sd)
    miou_a, iou_a = a.evaluate(val)
    print("semisuper_cycleGAN evaluate: mIoU with EMA %.6f, by hand %.6f" % (miou_b, miou_a))
    assert miou_a == miou_b and _same_iou(iou_a, iou_b) and np.array_equal(conf_b, a.running_metrics_val.confusion_matrix)
    assert conf_b.sum() > 0


def test_supervised_step_with_options(F, dev, tmp_path):
    from oracle import fixtures as FX
    md = load_sub("model")
    C, H = 4, 65

    def build(tag, **kw):
        args = FX.make_args(dataset="acdc", crop_height=H, crop_width=H, batch_size=2, gpu_ids=[dev.index or 0], ngf=8,
                            model="supervised_model", checkpoint_dir=str(tmp_path / tag), as_written=True, no_dropout=True, **kw)
        return _quiet(md.supervised_model, args)
    torch.manual_seed(41)
    a = build("a")
    b = build("b", clip_grad_norm=1e30, ema_decay=0.9)
    b.Gsi.load_state_dict(a.Gsi.state_dict())
    gen = torch.Generator().manual_seed(42)
    img, gt = torch.randn(2, 3, H, H, generator=gen).to(dev), torch.randint(0, C, (2, 1, H, H), generator=gen).to(dev)
    la = [a.step(img, gt).clone() for _ in range(2)]
    lb = [b.step(img, gt).clone() for _ in range(2)]
    torch.cuda.synchronize()
    wa, wb = _weights({"Gsi": a.Gsi}), _weights({"Gsi": b.Gsi})
    assert all(same(x, y) for x, y in zip(la, lb)) and all(same(wa[k], wb[k]) for k in wa)
    print("supervised_model, 2 steps, clip 1e30 + EMA: losses and %d tensors equal the plain run bit for bit" % len(wa))
    b.gsi_optimizer.max_grad_norm = 1e-3
    b.step(img, gt)
    torch.cuda.synchronize()
    ref, got = _host_norm(b.gsi_optimizer), float(b.gsi_optimizer.last_grad_norm)
    print("supervised_model: last_grad_norm %.9e, fp64 norm of the arena %.9e, relative distance %.3e (bound %.3e)" % (
        got, ref, abs(got - ref) / ref, NORM_TOL))
    assert abs(got - ref) / ref < NORM_TOL and float(b.gsi_optimizer._clip) < 1.0
    val = _val_batches(C, H, H, 43)
    miou_b, iou_b = b.evaluate(val)
    trained = _weights({"Gsi": b.Gsi})
    sd = {n: t.clone() for n, t in b.Gsi.state_dict().items()}
    ema_sd = b.gsi_optimizer.ema_state_dict(b.Gsi)
    assert set(ema_sd) == {n for n, _ in b.Gsi.named_parameters()} and set(ema_sd) <= set(sd)    # parameters only: buffers are not averaged
    sd.update(ema_sd)
    a.Gsi.load_state_dict(sd)
    miou_a, iou_a = a.evaluate(val)
    print("supervised_model evaluate: mIoU with EMA %.6f, by hand %.6f" % (miou_b, miou_a))
    assert miou_a == miou_b and _same_iou(iou_a, iou_b)
    after = _weights({"Gsi": b.Gsi})
    assert all(same(trained[k], after[k]) for k in trained)
    assert any(not same(ema_sd[k], trained["Gsi." + k]) for k in ema_sd)
