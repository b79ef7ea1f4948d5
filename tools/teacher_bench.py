#!/usr/bin/env python
"""Mean-teacher consistency of the unlabelled head (`--unl_teacher`, sscg_teacher_fwd) on the MI355X at the training step's sizes,
forward + backward, HIP events around --reps back-to-back calls, the variants interleaved sample by sample, medians:

  fused     sscg_upsample_head_fwd (softmax map) + sscg_teacher_fwd, then sscg_lovasz_scale_add (g_mse * coef + the map's upstream
            gradient) and ONE sscg_upsample_head_bwd_u whose pseudo-label slot is the teacher's - what the step runs with mse and ce on
  unfused   the same maths from torch ops on the materialised resizes: F.interpolate(align_corners=True) of both logit maps, the
            per-sample flip, softmax, the two losses and the softmax map, autograd backward
  plain     sscg_upsample_head_fwd + sscg_upsample_head_bwd - the unlabelled head of the step with the flag off
and the parts on their own: sscg_teacher_fwd, the scale-add, and the two stencil backwards.

  --step    also the whole training step (voc2012, 256x256, batch 8, --ema_decay 0.999) with `--unl_teacher mse=1,ce=0.5,thresh=0.35,flip`
            against the flag off: two models in one process, timed alternately; and, on the model with the flag on, the teacher's part
            on its own - the mirrored view, the two arena swaps of ema_weights() with nothing between them, and the swaps with the
            evaluation forward inside

usage: python tools/teacher_bench.py [--samples 30] [--reps 20] [--step] [--out FILE]
(needs the GPU: there is no CPU path)"""
import argparse
import contextlib
import importlib
import io
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "semi-supervised-segmentation-cyclegan_amd"
# batch, classes, logit map, crop: VOC at batch 8; the Cityscapes configuration's low-resolution logits at batch 16
SHAPES = [(8, 21, (33, 33), (256, 256)), (16, 20, (33, 65), (256, 512))]
TAU = 0.35
G_MSE, G_CE = 0.37, 1.9


def interleaved(torch, variants, samples, reps, warmup=3):
    for _ in range(warmup):
        for _, fn in variants:
            for _ in range(reps):
                fn()
    torch.cuda.synchronize()
    out = {name: [] for name, _ in variants}
    for _ in range(samples):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e3 / reps)          # us per call
    return out


def kernels(torch, F, shape, samples, reps, emit):
    import torch.nn.functional as TF
    B, C, (H, W), (OH, OW) = shape
    dev = torch.device("cuda:0")
    lib, st = F.lib, F._stream()
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(B, H, W, C, generator=g) * 3).to(dev)
    t = (x.cpu() + torch.randn(B, H, W, C, generator=g) * 1.5).to(dev)
    flips = [n % 2 == 0 for n in range(B)]
    flip = torch.tensor(flips, dtype=torch.uint8, device=dev)
    dy = (torch.randn(B, OH, OW, C, generator=g) * 0.01).to(dev)
    y, dx, up_dy = torch.empty(B, OH, OW, C, device=dev), torch.empty(B, H, W, C, device=dev), torch.empty(B, OH, OW, C, device=dev)
    coef = torch.empty(B, OH, OW, C, device=dev)
    losses, sums = torch.empty(2, device=dev), torch.empty(4, dtype=torch.float64, device=dev)
    pmap = torch.empty(B, OH, OW, dtype=torch.uint8, device=dev)
    ws = torch.empty(lib.sscg_teacher_workspace(B, OH, OW), dtype=torch.uint8, device=dev)
    g_mse, g_ce = torch.tensor(G_MSE, device=dev), torch.tensor(G_CE, device=dev)

    def head_fwd():
        assert lib.sscg_upsample_head_fwd(x.data_ptr(), None, y.data_ptr(), None, None, None, B, H, W, C, OH, OW, None, 0, st) == 0

    def teacher_fwd():
        assert lib.sscg_teacher_fwd(x.data_ptr(), t.data_ptr(), flip.data_ptr(), B, H, W, C, OH, OW, 1.0, TAU, losses.data_ptr(),
                                    sums.data_ptr(), pmap.data_ptr(), coef.data_ptr(), ws.data_ptr(), ws.numel(), st) == 0

    def scale_add():
        assert lib.sscg_lovasz_scale_add(coef.data_ptr(), g_mse.data_ptr(), dy.data_ptr(), up_dy.data_ptr(), coef.numel(), st) == 0

    def bwd_u():
        assert lib.sscg_upsample_head_bwd_u(x.data_ptr(), pmap.data_ptr(), up_dy.data_ptr(), None, None, g_ce.data_ptr(), sums.data_ptr(),
                                            dx.data_ptr(), B, H, W, C, OH, OW, st) == 0

    def bwd_plain():
        assert lib.sscg_upsample_head_bwd(x.data_ptr(), dy.data_ptr(), None, None, None, dx.data_ptr(), B, H, W, C, OH, OW, st) == 0

    def fused():
        head_fwd()
        teacher_fwd()
        scale_add()
        bwd_u()

    def plain():
        head_fwd()
        bwd_plain()

    xt = x.permute(0, 3, 1, 2).detach().requires_grad_(True)          # [B, C, H, W] views of the same logits
    tt = t.permute(0, 3, 1, 2)
    dyt = dy.permute(0, 3, 1, 2)
    mask = torch.tensor(flips, device=dev).view(B, 1, 1, 1)
    V = B * OH * OW

    def unfused():
        xt.grad = None
        up = TF.interpolate(xt, size=(OH, OW), mode="bilinear", align_corners=True)
        with torch.no_grad():
            tup = TF.interpolate(tt, size=(OH, OW), mode="bilinear", align_corners=True)
            q = torch.softmax(torch.where(mask, tup.flip(-1), tup), 1)
            conf, lab = q.max(1)
            kept = conf >= TAU
        logp = torch.log_softmax(up, 1)
        p = logp.exp()
        mse = (((p - q) ** 2).sum(1) * kept).sum() / (C * V)
        ce = -(logp.gather(1, lab.unsqueeze(1)).squeeze(1) * kept).sum() / kept.sum().clamp(min=1)
        (G_MSE * mse + G_CE * ce + (p * dyt).sum()).backward()
        return mse.detach(), ce.detach()

    fused()
    torch.cuda.synchronize()
    first = [v.clone() for v in (losses, sums, pmap, coef, dx)]
    fused()
    torch.cuda.synchronize()
    same = all(torch.equal(p, q) for p, q in zip(first, (losses, sums, pmap, coef, dx)))
    ref = [float(v) for v in unfused()]
    agree = float((xt.grad - dx.permute(0, 3, 1, 2)).abs().max() / xt.grad.abs().max())
    tag = "%dx%dx%dx%d -> %dx%d" % (B, C, H, W, OH, OW)
    emit("%s  fused twice bit-identical: %s; losses %.6g %.6g (torch ops: %.6g %.6g); kept %.3f agree %.3f; gradients agree to %.1e of the largest" % (
        tag, same, float(losses[0]), float(losses[1]), ref[0], ref[1], float(sums[3]) / V, float(sums[1]) / max(float(sums[3]), 1.0), agree))
    if not same:
        raise SystemExit("the fused path is not deterministic: nothing timed")
    variants = [("fused", fused), ("unfused", unfused), ("plain", plain), ("teacher_fwd alone", teacher_fwd), ("scale_add alone", scale_add),
                ("head_bwd_u alone", bwd_u), ("head_bwd alone", bwd_plain), ("head_fwd alone", head_fwd)]
    us = interleaved(torch, variants, samples, reps)
    med = {}
    for name, _ in variants:
        v = us[name]
        med[name] = statistics.median(v)
        emit("%s  %-18s median %9.1f us (range %.1f .. %.1f over %d samples of %d)" % (tag, name, med[name], min(v), max(v), samples, reps))
    emit("%s  fused - plain: %+.1f us per step (x%.2f); unfused / fused: %.2fx" % (
        tag, med["fused"] - med["plain"], med["fused"] / med["plain"], med["unfused"] / med["fused"]))


def whole_step(torch, F, emit, rounds=3, steps=8):
    md, data = importlib.import_module(PKG + ".model"), importlib.import_module(PKG + ".data")
    import main as cli
    dev = torch.device("cuda:0")
    on_flags = ["--unl_teacher", "mse=1,ce=0.5,thresh=%g,flip" % TAU]
    models = {}
    for tag, extra in (("off", []), ("on", on_flags)):
        args = cli.get_args(["--model", "semisupervised_cycleGAN", "--dataset", "voc2012", "--crop_height", "256", "--crop_width", "256",
                             "--batch_size", "8", "--checkpoint_dir", "/tmp/sscg_teacher_bench_ckpt", "--ema_decay", "0.999"] + extra)
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
    emit("whole step voc2012 256x256 batch 8 --ema_decay 0.999: flag off %.2f ms (%s), %s %.2f ms (%s): %+.2f ms, %+.2f %% (alternating, %d rounds of %d steps)" % (
        off, " ".join("%.2f" % v for v in times["off"]), " ".join(on_flags), on, " ".join("%.2f" % v for v in times["on"]), on - off,
        100 * (on - off) / off, rounds, steps))
    # ---- the teacher's part on its own, on the model with the flag on: host clock around synchronised repetitions
    m = models["on"]
    img = unl[0][0]

    def view():
        m._teacher_view(img)

    def swaps():
        with m.g_optimizer.ema_weights():
            pass

    def teacher():
        m._teacher_logits(img)
    parts = {}
    for name, fn in (("mirrored view", view), ("two arena swaps", swaps), ("swaps + evaluation forward", teacher)):
        fn()
        torch.cuda.synchronize()
        v = []
        for _ in range(7):
            t0 = time.perf_counter()
            for _ in range(4):
                fn()
            F.flush_side_work()
            torch.cuda.synchronize()
            v.append((time.perf_counter() - t0) * 1e3 / 4)
        parts[name] = statistics.median(v)
        emit("teacher part: %-28s median %.3f ms (range %.3f .. %.3f, 7 samples of 4)" % (name, parts[name], min(v), max(v)))
    emit("teacher part: the evaluation forward %.3f ms, the swaps %.3f ms: %.1f %% / %.1f %% of the step with the flag on" % (
        parts["swaps + evaluation forward"] - parts["two arena swaps"], parts["two arena swaps"],
        100 * (parts["swaps + evaluation forward"] - parts["two arena swaps"]) / on, 100 * parts["two arena swaps"] / on))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/teacher_bench.py measures on the MI355X: no GPU here, nothing measured")
    F = importlib.import_module(PKG + ".functional")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit("device: %s" % torch.cuda.get_device_name(0))
    for shape in SHAPES:
        kernels(torch, F, shape, a.samples, a.reps, emit)
    if a.step:
        whole_step(torch, F, emit)


if __name__ == "__main__":
    main()
