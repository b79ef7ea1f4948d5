#!/usr/bin/env python
"""The gated CRF loss (`--unl_crf`, sscg_crf_loss_fwd) on the MI355X at the training step's sizes (8 x 21 x 256 x 256 and
16 x 20 x 256 x 512), HIP events around --reps back-to-back calls, the variants interleaved sample by sample, medians:

  crf_loss fwd+bwd   F.crf_loss on a softmax map that needs a gradient, then backward: the stencil launch with its one-block finish
                     and ONE sscg_lovasz_scale_add - what the step adds with the flag on
  torch ops          the same maths from torch ops: per tap a shifted slice of the zero-padded map and image, the pairwise weight,
                     k * (1 - p(i) . p(j)); autograd backward
  crf_iter step      one mean-field step of sscg_crf_head (one crf_iter_kernel launch) on the same map and image: (1 + K iterations - 1
                     iteration) / K - the kernel this one shares its tap walk with
and the parts on their own: the forward with and without coef, the scale launch.

  --step    also the whole training step (voc2012, 256x256, batch 8) with --unl_crf on against off: two models in one process, timed
            alternately (bench.py takes no loss flags, so tools/ab.sh cannot switch this one; tools/ab.sh in this tree and in a
            checkout of the parent commit gives the flag-off pair)

usage: python tools/crf_loss_bench.py [--samples 20] [--reps 10] [--step] [--crf SPEC] [--out FILE]
(needs the GPU: there is no CPU path)"""
import argparse
import contextlib
import importlib
import io
import math
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "semi-supervised-segmentation-cyclegan_amd"
SHAPES = [(8, 21, 256, 256), (16, 20, 256, 512)]          # batch, classes, map
EXTRA = 5                                                  # iterations between the two timed variants of the mean-field step


def interleaved(torch, variants, samples, reps, warmup=2):
    for _ in range(warmup):
        for _, fn, _ in variants:
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name, _, _ in variants}
    for _ in range(samples):
        for name, fn, scale in variants:
            n = max(1, reps // scale)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e3 / n)          # us per call
    return out


def torch_ops_loss(torch, p, img, crf):
    """The definition from torch ops on [N,C,H,W] / [N,IC,H,W]: taps in row-major order, a tap outside the map skipped."""
    import torch.nn.functional as TF
    N, C, H, W = p.shape
    r, d = crf.radius, crf.dilation
    R = r * d
    ia, ib, ig = (1.0 / (2.0 * t * t) for t in (crf.theta_alpha, crf.theta_beta, crf.theta_gamma))
    pp, ip = TF.pad(p, (R, R, R, R)), TF.pad(img, (R, R, R, R))
    mask = TF.pad(torch.ones(1, H, W, device=p.device), (R, R, R, R))
    total = p.new_zeros(())
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dy == 0 and dx == 0:
                continue
            ys, xs = slice(R + dy * d, R + dy * d + H), slice(R + dx * d, R + dx * d + W)
            with torch.no_grad():
                d2 = float((dy * d) ** 2 + (dx * d) ** 2)
                c2 = ((img - ip[:, :, ys, xs]) ** 2).sum(1)
                k = (crf.w_bilateral * torch.exp(-(d2 * ia + c2 * ib)) + crf.w_spatial * math.exp(-d2 * ig)) * mask[:, ys, xs]
            total = total + (k * (1.0 - (p * pp[:, :, ys, xs]).sum(1))).sum()
    return total / (N * H * W)


def kernels(torch, F, shape, crf, samples, reps, emit):
    B, C, H, W = shape
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    low = (torch.randn(B, C, H // 8 + 1, W // 8 + 1, generator=g) * 2).to(dev)
    with torch.no_grad():
        soft = F.upsample_softmax_ce(low, (H, W))[0]                  # channels-last [B,C,H,W]: the map the step hands the loss
    image = torch.randn(B, 3, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    p = soft.detach().clone().requires_grad_(True)
    gup = torch.tensor(0.1, device=dev)
    coef_keep = F.crf_loss_fwd(soft, image, crf, True)[2]
    kw = {k: getattr(crf, k) for k in crf.__slots__ if k != "iterations"}

    def both():
        p.grad = None
        F.crf_loss(p, image, crf).backward(gup)

    pt = soft.detach().contiguous().requires_grad_(True)              # NCHW memory for the torch ops
    it = image.contiguous()

    def unfused():
        pt.grad = None
        torch_ops_loss(torch, pt, it, crf).backward(gup)

    def iters(n):
        opts = F.CrfOptions(iterations=n, **kw)
        return lambda: F.crf_labels(soft, image, (H, W), opts, probs=True, want_u8=True)

    both()
    unfused()
    torch.cuda.synchronize()
    l_hip, l_ref = float(F.crf_loss(soft, image, crf)), float(torch_ops_loss(torch, pt.detach(), it, crf))
    agree = float((pt.grad - p.grad).abs().max() / pt.grad.abs().max())
    tag = "%dx%dx%dx%d r%d d%d" % (B, C, H, W, crf.radius, crf.dilation)
    emit("%s  loss %.6f (torch ops: %.6f); gradients agree to %.1e of the largest" % (tag, l_hip, l_ref, agree))
    variants = [("crf_loss fwd+bwd", both, 1), ("torch ops fwd+bwd", unfused, 10), ("fwd, value only", lambda: F.crf_loss_fwd(soft, image, crf, False), 1),
                ("fwd with coef", lambda: F.crf_loss_fwd(soft, image, crf, True), 1), ("scale_add alone", lambda: F._lovasz_upstream(coef_keep, gup, None), 1),
                ("crf_head 1 iteration", iters(1), 1), ("crf_head %d iterations" % (1 + EXTRA), iters(1 + EXTRA), 1)]
    us = interleaved(torch, variants, samples, reps)
    med = {}
    for name, _, _ in variants:
        v = us[name]
        med[name] = statistics.median(v)
        emit("%s  %-22s median %9.1f us (range %.1f .. %.1f over %d samples)" % (tag, name, med[name], min(v), max(v), samples))
    step = (med["crf_head %d iterations" % (1 + EXTRA)] - med["crf_head 1 iteration"]) / EXTRA
    must = B * H * W * (2 * C + 3) * 4
    emit("%s  one crf_iter_kernel step %.1f us; fwd with coef / that step: %.2fx; fwd+bwd / that step: %.2fx; torch ops / crf_loss: %.1fx; "
         "the forward must move %.1f MB (p read, coef written, image): %.1f us at 8 TB/s" % (
             tag, step, med["fwd with coef"] / step, med["crf_loss fwd+bwd"] / step, med["torch ops fwd+bwd"] / med["crf_loss fwd+bwd"],
             must / 1e6, must / 8e12 * 1e6))


def whole_step(torch, F, emit, rounds=3, steps=8):
    md, data = importlib.import_module(PKG + ".model"), importlib.import_module(PKG + ".data")
    import main as cli
    dev = torch.device("cuda:0")
    on_flags = ["--unl_crf", "0.1"]
    models = {}
    ckpt = tempfile.TemporaryDirectory(prefix="sscg_crf_loss_bench_")          # removed when the function returns
    for tag, extra in (("off", []), ("on", on_flags)):
        args = cli.get_args(["--model", "semisupervised_cycleGAN", "--dataset", "voc2012", "--crop_height", "256", "--crop_width", "256",
                             "--batch_size", "8", "--checkpoint_dir", ckpt.name] + extra)
        args.gpu_ids, args.as_written, args.overlap_d = [0], True, False
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            models[tag] = md.semisuper_cycleGAN(args)
    lab = list(data.SyntheticLoader(8, 21, 256, 256, 4, 3, device=dev))
    unl = list(data.SyntheticLoader(8, 21, 256, 256, 4, 4, device=dev))
    times = {tag: [] for tag in models}
    for r in range(rounds + 1):                     # round 0 warms both up
        for tag, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                m.step(lab[i % 4][0], lab[i % 4][1], unl[i % 4][0])
            m.sync_losses()
            F.flush_side_work()
            torch.cuda.synchronize()
            if r:
                times[tag].append((time.perf_counter() - t0) * 1e3 / steps)
    off, on = statistics.median(times["off"]), statistics.median(times["on"])
    emit("whole step voc2012 256x256 batch 8: flag off %.2f ms (%s), %s %.2f ms (%s): %+.2f ms, %+.2f %% (alternating, %d rounds of %d steps)" % (
        off, " ".join("%.2f" % t for t in times["off"]), " ".join(on_flags), on, " ".join("%.2f" % t for t in times["on"]), on - off,
        100 * (on - off) / off, rounds, steps))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--crf", type=str, default="on")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/crf_loss_bench.py measures on the MI355X: no GPU here, nothing measured")
    F = importlib.import_module(PKG + ".functional")
    crf = importlib.import_module(PKG + ".utils").parse_unl_crf_kernel(a.crf)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit("device: %s; kernel: %r (untuned defaults unless --crf says otherwise)" % (torch.cuda.get_device_name(0), crf))
    for shape in SHAPES:
        kernels(torch, F, shape, crf, a.samples, a.reps, emit)
    if a.step:
        whole_step(torch, F, emit)


if __name__ == "__main__":
    main()
