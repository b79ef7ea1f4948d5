"""The losses of the unlabelled head on the MI355X: sscg_unl_fwd / sscg_unl_bwd (flat), the resized statistics and
sscg_upsample_head_bwd_u (the fused head with the UNL term), against the definitions written with torch ops in fp64 on the CPU
(tests/unl_reference.py: F.interpolate(align_corners=True) -> log_softmax -> the three losses, gradient by autograd).

Tolerances (tests/test_dice_gpu.py's header): a loss within 1e-3 |ref| + 1e-7; a gradient's max-abs distance within 1e-3 max|ref| +
floor, floor = 8 fp32 roundings of the largest term of an entry,
    8 * 2^-23 * (|g_e| max|u| / (V ln C) + |g_m| / V + |g_p| / max(K, 1) + max|dy|),
which covers C = 1, where every reference entry is exactly 0.  K and the pseudo-label map are EXACT (torch.equal), which only makes
sense where fp32 cannot flip a decision: every input here keeps, in fp64, |conf - tau| >= 1e-4 and a top-two probability gap >= 1e-4
at every output pixel (about 100x the fp32 error of a probability from logits of this size), and for C > 1 on a source map larger than
1x1 a kept share in [0.1, 0.9]; tests/test_unl_host.py asserts that on the CPU for the SEEDS below.  The 1x1 -> 5x5 geometry has a
constant map - kept entirely or not at all - and runs with one tau below and one above its confidence.  The fp64 sums carry no bound of
their own: their relative distances are printed.
Every test prints the distances it observed (`unl ...` lines; run with -s); profiles/unl.txt keeps them."""
import contextlib
import functools
import io
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, load_sub
from test_dice_host import CLASSES, GEOMS
from unl_reference import MARGIN, TAU, make_logits, unl_reference

pytestmark = pytest.mark.gpu

CL = torch.channels_last
EPS32 = 2.0 ** -23
# (index into GEOMS, C) -> the seed of make_logits: the first of 0..13 whose input meets the margin and kept-share conditions
SEEDS = {(0, 1): 0, (0, 4): 0, (0, 20): 0, (0, 21): 0, (0, 64): 0, (1, 1): 0, (1, 4): 0, (1, 20): 0, (1, 21): 0, (1, 64): 0,
         (2, 1): 0, (2, 4): 1, (2, 20): 1, (2, 21): 1, (2, 64): 1, (3, 1): 0, (3, 4): 1, (3, 20): 0, (3, 21): 0, (3, 64): 1}
G3 = (0.37, 1.9, 0.61)          # distinct upstream scales of (entropy, max-squares, pseudo-label cross entropy)


def case_inputs(gi, C):
    """(logits fp64 [N, C, H, W], the thresholds to run) of a geometry and class count; the all-or-none geometry takes one threshold
    halfway below its constant confidence and one halfway between it and 1 (C == 1: the confidence is 1, nothing lies above it)"""
    N, H, W, OH, OW = GEOMS[gi]
    x = make_logits(SEEDS[(gi, C)], N, C, H, W)
    if H * W > 1:
        return x, [TAU[C]]
    conf = float(torch.softmax(x, 1).max())
    return x, [0.5 * conf] + ([0.5 * (conf + 1.0)] if C > 1 else [])


@functools.lru_cache(maxsize=None)
def reference(gi, C, tau, g=(1.0, 1.0, 1.0), soft_seed=None):
    """unl_reference of a case, computed once and shared (left unchanged by its readers); soft_seed: the seed of the upstream gradient R
    of the softmax map (None: none)"""
    N, H, W, OH, OW = GEOMS[gi]
    x, _ = case_inputs(gi, C)
    R = soft_upstream(soft_seed, N, C, OH, OW) if soft_seed is not None else None
    return unl_reference(x, tau, (OH, OW), g, R)


def soft_upstream(seed, N, C, OH, OW):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, C, OH, OW, generator=g, dtype=torch.float32) * 0.01).double()


def gpu(t, dev):
    return t.float().to(dev).contiguous(memory_format=CL) if t.dim() == 4 else t.float().to(dev)


def grad_floor(ref, g, C, max_dy=0.0):
    lnc = math.log(C) if C > 1 else 1.0
    return 8 * EPS32 * (abs(g[0]) * ref["max_u"] / (ref["V"] * lnc) + abs(g[1]) / ref["V"] + abs(g[2]) / max(ref["K"], 1) + max_dy)


def check_loss(tag, loss, ref_loss):
    loss, ref_loss = float(loss.detach()), float(ref_loss)
    d = abs(loss - ref_loss)
    print("unl %-62s loss %.9g ref %.9g rel %.2e" % (tag, loss, ref_loss, d / max(abs(ref_loss), 1e-30)))
    assert math.isfinite(loss) and d <= 1e-3 * abs(ref_loss) + 1e-7, (tag, loss, ref_loss)


def check_grad(tag, grad, ref_grad, floor):
    grad = grad.detach().double().cpu()
    dg, gmax = float((grad - ref_grad).abs().max()), float(ref_grad.abs().max())
    print("unl %-62s grad max-abs diff %.2e of %.2e rel %.2e (floor %.1e)" % (tag, dg, gmax, dg / max(gmax, 1e-30), floor))
    assert torch.isfinite(grad).all() and dg <= 1e-3 * gmax + floor, (tag, dg, gmax)


def check_forward(tag, losses, sums, pseudo, ref):
    """the three losses to tolerance; K and the map exactly; the sums' distances printed"""
    for k, name in enumerate(("ent", "msq", "pl")):
        check_loss(tag + " " + name, losses[k], ref[name])
    s = sums.cpu()
    assert s.dtype == torch.float64 and s.shape == (4,)
    assert float(s[3]) == ref["K"], (tag, float(s[3]), ref["K"])
    rel = [abs(float(s[k]) - float(ref["sums"][k])) / max(abs(float(ref["sums"][k])), 1e-30) for k in range(3)]
    print("unl %-62s K %d of %d exact; sums rel %.2e %.2e %.2e" % (tag, ref["K"], ref["V"], rel[0], rel[1], rel[2]))
    if pseudo is not None:
        assert pseudo.dtype == torch.uint8 and torch.equal(pseudo.cpu(), ref["pseudo"]), tag


def run_head(F, dev, x64, size, tau, g, R64=None, want_soft=True, want_pseudo=True):
    """upsample_softmax_unl + backward of g . losses + sum(soft * R): (soft, losses, stats, gradient with respect to the logits)"""
    xg = gpu(x64, dev).requires_grad_(True)
    live = [k for k in range(3) if g[k] != 0.0]
    opts = F.UnlabelledOptions(entropy=1.0, maxsq=1.0, pseudo=1.0, thresh=tau)
    soft, l_ent, l_msq, l_pl, stats = F.upsample_softmax_unl(xg, size, opts, want_soft=want_soft, want_pseudo=want_pseudo)
    losses = (l_ent, l_msq, l_pl)
    total = F.weighted_sum([losses[k] for k in live], [g[k] for k in live]) if live else None
    if R64 is not None:
        t = (soft * gpu(R64, dev)).sum()
        total = t if total is None else total + t
    total.backward()
    return soft, losses, stats, xg.grad


# ------------------------------------------------------------------------------------------ 1. the fused head
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("gi", range(len(GEOMS)))
def test_fused_head_value_map_gradient(gi, C, F, dev):
    N, H, W, OH, OW = GEOMS[gi]
    x, taus = case_inputs(gi, C)
    assert F._head_applies(gpu(x, dev), OH, OW)
    plain = F.upsample_softmax_ce(gpu(x, dev), (OH, OW))[0]
    for tau in taus:
        tag = "head %dx%dx%d->%dx%d C=%d tau=%.3f" % (N, H, W, OH, OW, C, tau)
        # all three terms with distinct scales, with and without an upstream gradient on the softmax map
        for seed in (5, None):
            ref = reference(gi, C, tau, G3, seed)
            assert ref["K"] in (0, ref["V"]) or H * W > 1
            R = soft_upstream(seed, N, C, OH, OW) if seed is not None else None
            soft, losses, stats, grad = run_head(F, dev, x, (OH, OW), tau, G3, R)
            assert torch.equal(soft, plain)
            check_forward(tag + (" +dy" if R is not None else ""), losses, stats["sums"], stats["pseudo"], ref)
            check_grad(tag + (" +dy" if R is not None else "") + " all", grad, ref["grad"],
                       grad_floor(ref, G3, C, 0.0 if R is None else float(R.abs().max())))
        # each term alone
        for k in range(3):
            g = tuple(G3[j] if j == k else 0.0 for j in range(3))
            ref = reference(gi, C, tau, g)
            _, _, _, grad = run_head(F, dev, x, (OH, OW), tau, g)
            check_grad(tag + " only " + ("ent", "msq", "pl")[k], grad, ref["grad"], grad_floor(ref, g, C))
            if k == 2 and ref["K"] == 0:
                assert torch.count_nonzero(grad) == 0            # nothing kept: loss 0, gradient 0
        # without the softmax map
        ref = reference(gi, C, tau, G3)
        soft, losses, stats, grad = run_head(F, dev, x, (OH, OW), tau, G3, want_soft=False, want_pseudo=False)
        assert soft is None and stats["pseudo"] is None
        check_forward(tag + " no soft", losses, stats["sums"], None, ref)
        check_grad(tag + " no soft", grad, ref["grad"], grad_floor(ref, G3, C))


# ------------------------------------------------------------------------------------------ 2. the raw ABI
def raw_fwd(F, dev, xh, OH, OW, tau, want_map=True):
    """sscg_unl_fwd on sentinel-guarded outputs, the workspace followed by a guard region: (losses [3], sums [4], map or None)"""
    lib = F.lib
    N, H, W, C = xh.shape
    need = lib.sscg_unl_workspace(N, OH, OW)
    assert need == N * 4 * (min((OH * OW + 255) // 256, 256) + 1) * 8
    ws = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device=dev)
    lo = torch.full((3 + 64,), 7.0, device=dev)
    su = torch.full((4 + 64,), 7.0, dtype=torch.float64, device=dev)
    pm = torch.full((N * OH * OW + 128,), 0xEE, dtype=torch.uint8, device=dev)
    losses, sums, pmap = lo[32:35], su[32:36], pm[64:64 + N * OH * OW]
    assert lib.sscg_unl_fwd(xh.data_ptr(), N, H, W, C, OH, OW, tau, losses.data_ptr(), sums.data_ptr(), None, ws.data_ptr(), need - 1,
                            F._stream()) == -3                                               # one byte short
    rc = lib.sscg_unl_fwd(xh.data_ptr(), N, H, W, C, OH, OW, tau, losses.data_ptr(), sums.data_ptr(), pmap.data_ptr() if want_map else None,
                          ws.data_ptr(), need, F._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert (ws[need:] == 0x5A).all() and (lo[:32] == 7).all() and (lo[35:] == 7).all() and (su[:32] == 7).all() and (su[36:] == 7).all()
    assert (pm[:64] == 0xEE).all() and (pm[64 + N * OH * OW:] == 0xEE).all() and (want_map or (pm == 0xEE).all())
    return losses.clone(), sums.clone(), pmap.clone().view(N, OH, OW) if want_map else None


def raw_bwd_u(F, dev, xh, pmap, dy, g, sums, OH, OW):
    """sscg_upsample_head_bwd_u on a sentinel-guarded dx; g: three device scalars or None"""
    N, H, W, C = xh.shape
    guard = torch.full((xh.numel() + 64,), 7.0, device=dev)
    dx = guard[32:32 + xh.numel()]
    rc = F.lib.sscg_upsample_head_bwd_u(xh.data_ptr(), None if pmap is None else pmap.data_ptr(), None if dy is None else dy.data_ptr(),
                                        *[None if t is None else t.data_ptr() for t in g], sums.data_ptr(), dx.data_ptr(),
                                        N, H, W, C, OH, OW, F._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert (guard[:32] == 7).all() and (guard[-32:] == 7).all()
    return dx.clone().view(N, H, W, C).permute(0, 3, 1, 2)


@pytest.mark.parametrize("C", CLASSES)
def test_raw_abi_every_live_branch_combination(C, F, dev):
    gi = 2
    N, H, W, OH, OW = GEOMS[gi]
    x, (tau,) = case_inputs(gi, C)
    xh = gpu(x, dev).permute(0, 2, 3, 1)
    assert xh.is_contiguous()
    ref0 = reference(gi, C, tau)
    losses, sums, pmap = raw_fwd(F, dev, xh, OH, OW, tau)
    check_forward("raw C=%d" % C, losses, sums, pmap, ref0)
    l2, s2, none = raw_fwd(F, dev, xh, OH, OW, tau, want_map=False)
    assert none is None and torch.equal(l2, losses) and torch.equal(s2, sums)
    R = soft_upstream(9, N, C, OH, OW)
    dy = gpu(R, dev).permute(0, 2, 3, 1).contiguous()
    scal = [torch.tensor(v, device=dev) for v in G3]
    for mask in range(8):
        for with_dy in (False, True):
            g = tuple(G3[k] if mask >> k & 1 else 0.0 for k in range(3))
            gp = [scal[k] if mask >> k & 1 else None for k in range(3)]
            if mask == 0 and not with_dy:
                assert F.lib.sscg_upsample_head_bwd_u(xh.data_ptr(), None, None, None, None, None, sums.data_ptr(), xh.data_ptr(),
                                                      N, H, W, C, OH, OW, F._stream()) == -1      # nothing to differentiate
                continue
            dx = raw_bwd_u(F, dev, xh, pmap if mask & 4 else None, dy if with_dy else None, gp, sums, OH, OW)
            if mask == 0:       # no loss gradient: the plain head's backward, bit for bit
                plain = torch.empty_like(xh)
                assert F.lib.sscg_upsample_head_bwd(xh.data_ptr(), dy.data_ptr(), None, None, None, plain.data_ptr(), N, H, W, C, OH, OW,
                                                    F._stream()) == 0
                assert torch.equal(dx, plain.permute(0, 3, 1, 2))
            ref = reference(gi, C, tau, g, 9 if with_dy else None)
            check_grad("raw C=%d mask %d dy %d" % (C, mask, with_dy), dx, ref["grad"],
                       grad_floor(ref, g, C, float(R.abs().max()) if with_dy else 0.0))


# ------------------------------------------------------------------------------------------ 3. fused against flat
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("gi", range(len(GEOMS)))
def test_fused_equals_flat(gi, C, F, dev):
    N, H, W, OH, OW = GEOMS[gi]
    x, taus = case_inputs(gi, C)
    xg = gpu(x, dev)
    xh = xg.permute(0, 2, 3, 1)
    up = F.upsample_bilinear(xg, (OH, OW))                   # the stored resize
    uph = up.permute(0, 2, 3, 1)
    assert xh.is_contiguous() and uph.is_contiguous()
    for tau in taus:
        a = raw_fwd(F, dev, xh, OH, OW, tau)
        b = raw_fwd(F, dev, uph, OH, OW, tau)               # the identity call: the same kernel without the stencil
        assert all(torch.equal(p, q) for p, q in zip(a, b)), (gi, C, tau)
        ref = reference(gi, C, tau, G3)
        fused = run_head(F, dev, x, (OH, OW), tau, G3)[3]
        was = F.FUSE_HEAD[0]
        F.FUSE_HEAD[0] = False
        try:
            soft, losses, stats, flat = run_head(F, dev, x, (OH, OW), tau, G3)
        finally:
            F.FUSE_HEAD[0] = was
        tag = "flat %dx%dx%d->%dx%d C=%d tau=%.3f" % (N, H, W, OH, OW, C, tau)
        check_forward(tag, losses, stats["sums"], stats["pseudo"], ref)
        floor = grad_floor(ref, G3, C)
        check_grad(tag, flat, ref["grad"], floor)
        check_grad(tag + " fused - flat", fused, flat.detach().double().cpu(), floor)


# ------------------------------------------------------------------------------------------ 4. hand cases
@pytest.mark.parametrize("C", [4, 21])
def test_hand_cases(C, F, dev):
    N, H, W, OH, OW = GEOMS[0]
    V = N * OH * OW
    zero = torch.zeros(N, C, H, W, dtype=torch.float64)
    for tau, want_k in ((0.5 / C, V), (1.0, 0)):
        soft, losses, stats, grad = run_head(F, dev, zero, (OH, OW), tau, G3)
        check_loss("hand zeros C=%d tau=%g ent" % (C, tau), losses[0], 1.0)
        check_loss("hand zeros C=%d tau=%g msq" % (C, tau), losses[1], -0.5 / C)
        check_loss("hand zeros C=%d tau=%g pl" % (C, tau), losses[2], math.log(C) if want_k else 0.0)
        assert float(stats["sums"][3]) == want_k
        assert (stats["pseudo"] == (0 if want_k else 255)).all()             # the first maximum of a tie is class 0
        ref = unl_reference(zero, tau, (OH, OW), G3)
        assert ref["K"] == want_k
        check_grad("hand zeros C=%d tau=%g" % (C, tau), grad, ref["grad"], grad_floor(ref, G3, C))
    soft, losses, stats, grad = run_head(F, dev, zero, (OH, OW), 1.0, (0.0, 0.0, G3[2]))
    assert float(losses[2].detach()) == 0.0 and torch.count_nonzero(grad) == 0       # nothing kept: loss 0, gradient 0
    # one logit at +200, the rest at -200: exp(-400) vanishes, and 0 * u must stay 0
    peak = torch.full((N, C, H, W), -200.0, dtype=torch.float64)
    peak[:, C // 2] = 200.0
    soft, losses, stats, grad = run_head(F, dev, peak, (OH, OW), 0.9, G3)
    vals = [float(v.detach()) for v in losses]
    print("unl hand peak C=%d: ent %.3g msq %.9g pl %.3g, max |grad| %.3g" % (C, vals[0], vals[1], vals[2], float(grad.abs().max())))
    assert vals[0] == 0.0 and vals[2] == 0.0 and abs(vals[1] + 0.5) <= 1e-6 and float(stats["sums"][0]) == 0.0
    assert float(stats["sums"][3]) == V and (stats["pseudo"] == C // 2).all()
    ref = unl_reference(peak, 0.9, (OH, OW), G3)
    assert torch.isfinite(grad).all()
    check_grad("hand peak C=%d" % C, grad, ref["grad"], grad_floor(ref, G3, C))


# ------------------------------------------------------------------------------------------ 5. determinism
def test_the_same_call_twice_gives_the_same_bits(F, dev):
    N, C, H, W, OH, OW = 2, 21, 9, 11, 67, 83
    assert (OH * OW) % 256 and OH * OW > 256
    x = make_logits(77, N, C, H, W)
    R = soft_upstream(78, N, C, OH, OW)
    runs = []
    for _ in range(2):
        soft, losses, stats, grad = run_head(F, dev, x, (OH, OW), TAU[C], G3, R)
        runs.append([soft, torch.stack(losses), stats["sums"], stats["pseudo"], grad])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    ref = unl_reference(x, TAU[C], (OH, OW), G3, R)
    for k, name in enumerate(("ent", "msq", "pl")):
        check_loss("twice " + name, runs[0][1][k], ref[name])
    check_grad("twice", runs[0][4], ref["grad"], grad_floor(ref, G3, C, float(R.abs().max())))


# ------------------------------------------------------------------------------------------ 6. past the caps
@pytest.mark.parametrize("case", ["grid cap", "finish block", "backward cap"])
def test_past_the_caps(case, F, dev):
    """C = 4, flat, ragged tails (the sizes of tests/test_dice_gpu.py::test_past_the_caps):
      grid cap:      363 x 363 pixels > 2 * 256 blocks * 256 threads: every statistics thread takes 2 pixels, 697 of them a third
      finish block:  3 samples x 89 blocks = 267 records, 89 > the 64 row lanes of the per-sample reduction; 150 x 151 % 256 = 122
      backward cap:  1449 x 1449 pixels > the flat backward's 8192 blocks * 256 threads (and 33 pixels per statistics thread)
    Millions of random pixels cannot all keep the 1e-4 margins, so the logits come from nine levels: the confidences then take finitely
    many values, the threshold sits in a gap between them (asserted), and a tie of the top two is an exact tie of equal logits, which
    fp32 resolves as fp64 does - by the first maximum."""
    C, tau = 4, 0.6
    N, H, W = {"grid cap": (1, 363, 363), "finish block": (3, 150, 151), "backward cap": (1, 1449, 1449)}[case]
    if case == "grid cap":
        assert H * W > 2 * 256 * 256 and (H * W) % 256
    if case == "finish block":
        assert (H * W + 255) // 256 > 64 and N * ((H * W + 255) // 256) > 256 and (H * W) % 256
    if case == "backward cap":
        assert H * W > 8192 * 256 and (H * W) % 256
    g = torch.Generator().manual_seed(len(case))
    x = (torch.randint(-4, 5, (N, C, H, W), generator=g).float() * 0.75).double()
    ref = unl_reference(x, tau, None, G3)
    p = torch.softmax(x, 1)
    top2 = p.topk(2, dim=1).values
    gap = top2[:, 0] - top2[:, 1]
    assert ref["conf_margin"] >= MARGIN and bool(((gap == 0) | (gap >= MARGIN)).all()) and 0.1 <= ref["kept_share"] <= 0.9
    xh = gpu(x, dev).permute(0, 2, 3, 1)
    tag = "caps %s %dx%dx%d" % (case, N, H, W)
    losses, sums, pmap = raw_fwd(F, dev, xh, H, W, tau)
    check_forward(tag, losses, sums, pmap, ref)
    rows = N * H * W
    guard = torch.full((rows * C + 64,), 7.0, device=dev)
    dx = guard[32:32 + rows * C]
    scal = [torch.tensor(v, device=dev) for v in G3]
    rc = F.lib.sscg_unl_bwd(xh.data_ptr(), pmap.data_ptr(), N, H, W, C, scal[0].data_ptr(), scal[1].data_ptr(), scal[2].data_ptr(),
                            sums.data_ptr(), dx.data_ptr(), F._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert (guard[:32] == 7).all() and (guard[-32:] == 7).all()
    check_grad(tag, dx.view(N, H, W, C).permute(0, 3, 1, 2), ref["grad"], grad_floor(ref, G3, C))


# ------------------------------------------------------------------------------------------ 7. through the model
def _args(dev, tmp_path, **kw):
    FX = __import__("oracle.fixtures", fromlist=["x"])
    return FX.make_args(dataset="acdc", crop_height=64, crop_width=64, batch_size=2, gpu_ids=[dev.index or 0], ngf=8, ndf=8,
                        checkpoint_dir=str(tmp_path / "ckpt"), as_written=True, **kw)


FLAG_KEYS = {"unl_entropy": {"unl_entropy"}, "unl_maxsq": {"unl_maxsq"}, "unl_pseudo": {"unl_pseudo_ce", "unl_pseudo_kept"}}


def test_semisupervised_step_takes_each_flag(F, dev, tmp_path, monkeypatch):
    md, data = load_sub("model"), load_sub("data")
    seen = []
    inner = F.upsample_softmax_unl

    def spy(x, size, unl=None, **k):
        seen.append((x.detach().float().cpu(), tuple(size), unl))
        return inner(x, size, unl, **k)
    monkeypatch.setattr(F, "upsample_softmax_unl", spy)
    got = {}
    runs = [("default", {})] + [(k, {k: 0.3}) for k in FLAG_KEYS] + [("all", dict(unl_entropy=0.2, unl_maxsq=0.3, unl_pseudo=0.4,
                                                                                   unl_pseudo_thresh=0.4, unl_ramp=2))]
    for tag, kw in runs:
        args = _args(dev, tmp_path, **kw)
        torch.manual_seed(22)
        with contextlib.redirect_stdout(io.StringIO()):
            m = md.semisuper_cycleGAN(args)
            labeled, unlabeled, _ = data.synthetic_loaders(args, 4, steps=1)
        (l_img, l_gt, _), (unl_img, _, _) = next(iter(labeled)), next(iter(unlabeled))
        if tag == "all":
            assert m.set_unl_epoch(1) == 0.5
        torch.manual_seed(23)
        del seen[:]
        losses = m.step(l_img.to(dev), l_gt.to(dev), unl_img.to(dev))
        m.sync_losses()
        got[tag] = {k: float(v) for k, v in losses.items()}
        assert all(math.isfinite(v) for v in got[tag].values()), got[tag]
        F.flush_side_work()
        torch.cuda.synchronize()
        want = set() if tag == "default" else set().union(*FLAG_KEYS.values()) if tag == "all" else FLAG_KEYS[tag]
        assert set(got[tag]) - set(md.LOSS_KEYS) == want, (tag, set(got[tag]))
        assert len(seen) == (0 if tag == "default" else 1)
        if tag == "default":
            continue
        logits, size, opts = seen[0]
        assert size == (64, 64)
        ref = unl_reference(logits.double(), opts.thresh, size)
        for key, name in (("unl_entropy", "ent"), ("unl_maxsq", "msq"), ("unl_pseudo_ce", "pl")):
            if key in got[tag]:
                print("unl step %-12s %-14s %.9g ref %.9g" % (tag, key, got[tag][key], float(ref[name])))
                assert abs(got[tag][key] - float(ref[name])) <= 1e-3 * abs(float(ref[name])) + 1e-7, (tag, key)
        if "unl_pseudo_kept" in got[tag]:
            near = int(((ref["conf"] - opts.thresh).abs() < MARGIN).sum())        # the pixels fp32 may decide the other way
            print("unl step %-12s kept %.9g ref %.9g (%d of %d pixels inside the margin)" % (
                tag, got[tag]["unl_pseudo_kept"], ref["kept_share"], near, ref["V"]))
            assert abs(got[tag]["unl_pseudo_kept"] * ref["V"] - ref["K"]) <= near + 1e-3          # (+ the fp32 rounding of the share)
        # the networks' first forward does not depend on the loss flags and the head hands the step the same softmax map: none of the
        # step's own losses can be reached by the flags in a first step (the D step reads no generator weight), so all of them agree
        for key in md.LOSS_KEYS:
            assert got[tag][key] == pytest.approx(got["default"][key], rel=1e-3), (tag, key)


def test_supervised_step_ignores_the_flags(F, dev, tmp_path):
    """The supervised model has no unlabelled batch: with the flags set its step returns the loss, records the extras and applies the
    update of a model built without them - bit for bit."""
    md, data = load_sub("model"), load_sub("data")
    got = {}
    for tag, kw in (("off", {}), ("on", dict(unl_entropy=0.5, unl_maxsq=0.5, unl_pseudo=0.5))):
        args = _args(dev, tmp_path, model="supervised_model", **kw)
        torch.manual_seed(21)
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            m = md.supervised_model(args)
            loader = data.synthetic_loaders(args, 4, steps=2)[0]
        assert ("are ignored" in out.getvalue()) == (tag == "on") and not hasattr(m, "unl_options")
        l_img, l_gt, _ = next(iter(loader))
        torch.manual_seed(24)
        loss = m.step(l_img.to(dev), l_gt.to(dev))
        F.flush_side_work()
        torch.cuda.synchronize()
        got[tag] = (loss.detach().clone(), dict(vars(m).get("extras", {})), [p.detach().clone() for p in m.Gsi.parameters()])
    assert math.isfinite(float(got["on"][0])) and torch.equal(got["on"][0], got["off"][0])
    assert got["on"][1] == got["off"][1] == {}                                # what the step records beside its loss: nothing new
    assert all(torch.equal(a, b) for a, b in zip(got["on"][2], got["off"][2]))


# ------------------------------------------------------------------------------------------ 8. the launch census
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
ON = dict(unl_entropy=0.2, unl_maxsq=0.3, unl_pseudo=0.4)
for tag, kw in (("off", {}), ("on", ON), ("sup on", dict(model="supervised_model", **ON))):
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


def test_launch_census(tmp_path):
    env = dict(os.environ, SSCG_TRACE="1")
    for k in ("SSCG_RACECHECK", "SSCG_FUZZ", "SSCG_FUSE_HEAD"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", CENSUS % (ROOT, os.path.join(ROOT, "tests"), str(tmp_path / "ckpt"))], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    new = {"sscg_unl_workspace", "sscg_unl_fwd", "sscg_unl_bwd", "sscg_upsample_head_bwd_u"}
    calls = {}
    for tag in ("off", "on", "sup on"):
        body = r.stderr[r.stderr.index("[census] begin " + tag):r.stderr.index("[census] end " + tag)]
        names = [line[7:].split("(")[0] for line in body.splitlines() if line.startswith("[sscg] ")]
        calls[tag] = {n: names.count(n) for n in set(names)}
    off, on = calls["off"], calls["on"]
    assert not new & set(off), off
    # the supervised model has no unlabelled batch: with the flags set its step names none of the entries either
    assert not new & set(calls["sup on"]) and calls["sup on"].get("sscg_upsample_head_fwd") == 1, calls["sup on"]
    assert off.get("sscg_upsample_head_fwd") == 3 and off.get("sscg_upsample_head_bwd") == 3
    # on: one statistics entry forward; the unlabelled head's ONE backward launch is now the _u entry - it gains none
    assert on.get("sscg_unl_fwd") == 1 and on.get("sscg_upsample_head_bwd_u") == 1 and "sscg_unl_bwd" not in on
    assert on.get("sscg_upsample_head_fwd") == 3 and on.get("sscg_upsample_head_bwd") == 2

    def launches(c):
        return {k: v for k, v in c.items() if k not in new and k not in ("sscg_upsample_head_bwd", "sscg_weighted_sum")
                and not k.endswith(("_workspace", "_bytes", "_applies"))}
    assert launches(on) == launches(off), (launches(on), launches(off))
