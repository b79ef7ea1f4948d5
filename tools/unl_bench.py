#!/usr/bin/env python
"""The losses of the unlabelled head (entropy, max-squares, thresholded pseudo-label cross entropy) on the MI355X at the training step's
sizes, forward + backward, HIP events around --reps back-to-back pairs, the variants interleaved sample by sample, medians:

  fused     sscg_upsample_head_fwd (softmax map) + sscg_unl_fwd, then ONE sscg_upsample_head_bwd_u with the map's upstream gradient and
            all three loss gradients - what the step runs with the flags on
  unfused   the same maths from torch ops on the materialised resize: F.interpolate(align_corners=True) -> log_softmax -> the three
            losses and the softmax map, autograd backward
  plain     sscg_upsample_head_fwd (softmax map) + sscg_upsample_head_bwd with the map's upstream gradient - the unlabelled head of the
            step with the flags off
and the parts on their own: sscg_unl_fwd, and the two stencil backwards (the SOFT + UNL instantiation against the SOFT-only one).

  --step    also the whole training step (voc2012, 256x256, batch 8) with the three flags on against off: two models in one process,
            timed alternately (bench.py takes no loss flags, so tools/ab.sh cannot switch this one)

  --one-step on|off [--root DIR]
            nothing but the whole step of ONE model in this process, flags on or off, from the tree at DIR (default: this one) - for a
            pair across two trees, such as the flags on here against a checkout of the parent commit with them off, run alternately

usage: python tools/unl_bench.py [--samples 30] [--reps 20] [--step] [--one-step on|off [--root DIR]] [--out FILE]
(needs the GPU: there is no CPU path)"""
import argparse
import contextlib
import importlib
import io
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv[1:-1]:          # the tree whose package and main.py are imported: decided before anything is
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
PKG = "semi-supervised-segmentation-cyclegan_amd"
# batch, classes, logit map, crop: VOC at batch 8; the Cityscapes configuration's low-resolution logits at batch 16
SHAPES = [(8, 21, (33, 33), (256, 256)), (16, 20, (33, 65), (256, 512))]
TAU = 0.35


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
    dy = (torch.randn(B, OH, OW, C, generator=g) * 0.01).to(dev)
    y, dx = torch.empty(B, OH, OW, C, device=dev), torch.empty(B, H, W, C, device=dev)
    losses, sums = torch.empty(3, device=dev), torch.empty(4, dtype=torch.float64, device=dev)
    pmap = torch.empty(B, OH, OW, dtype=torch.uint8, device=dev)
    ws = torch.empty(lib.sscg_unl_workspace(B, OH, OW), dtype=torch.uint8, device=dev)
    gs = [torch.tensor(v, device=dev) for v in (0.37, 1.9, 0.61)]

    def head_fwd():
        assert lib.sscg_upsample_head_fwd(x.data_ptr(), None, y.data_ptr(), None, None, None, B, H, W, C, OH, OW, None, 0, st) == 0

    def unl_fwd():
        assert lib.sscg_unl_fwd(x.data_ptr(), B, H, W, C, OH, OW, TAU, losses.data_ptr(), sums.data_ptr(), pmap.data_ptr(), ws.data_ptr(),
                                ws.numel(), st) == 0

    def bwd_u():
        assert lib.sscg_upsample_head_bwd_u(x.data_ptr(), pmap.data_ptr(), dy.data_ptr(), gs[0].data_ptr(), gs[1].data_ptr(), gs[2].data_ptr(),
                                            sums.data_ptr(), dx.data_ptr(), B, H, W, C, OH, OW, st) == 0

    def bwd_plain():
        assert lib.sscg_upsample_head_bwd(x.data_ptr(), dy.data_ptr(), None, None, None, dx.data_ptr(), B, H, W, C, OH, OW, st) == 0

    def fused():
        head_fwd()
        unl_fwd()
        bwd_u()

    def plain():
        head_fwd()
        bwd_plain()

    xt = x.permute(0, 3, 1, 2).detach().requires_grad_(True)          # [B, C, H, W] view of the same logits
    dyt = dy.permute(0, 3, 1, 2)
    V = B * OH * OW

    def unfused():
        xt.grad = None
        up = TF.interpolate(xt, size=(OH, OW), mode="bilinear", align_corners=True)
        logp = torch.log_softmax(up, 1)
        p = logp.exp()
        ent = -(p * logp).sum() / (V * math.log(C))
        msq = -(p * p).sum() / (2.0 * V)
        conf, lab = p.detach().max(1)
        kept = conf >= TAU
        pl = -(logp.gather(1, lab.unsqueeze(1)).squeeze(1) * kept).sum() / kept.sum().clamp(min=1)
        (0.37 * ent + 1.9 * msq + 0.61 * pl + (p * dyt).sum()).backward()
        return ent.detach(), msq.detach(), pl.detach()

    fused()
    torch.cuda.synchronize()
    first = [t.clone() for t in (losses, sums, pmap, dx)]
    fused()
    torch.cuda.synchronize()
    same = all(torch.equal(p, q) for p, q in zip(first, (losses, sums, pmap, dx)))
    ref = [float(v) for v in unfused()]
    agree = float((xt.grad - dx.permute(0, 3, 1, 2)).abs().max() / xt.grad.abs().max())
    tag = "%dx%dx%dx%d -> %dx%d" % (B, C, H, W, OH, OW)
    emit("%s  fused twice bit-identical: %s; losses %.6f %.6f %.6f (torch ops: %.6f %.6f %.6f); kept %.3f; gradients agree to %.1e of the largest" % (
        tag, same, float(losses[0]), float(losses[1]), float(losses[2]), ref[0], ref[1], ref[2], float(sums[3]) / V, agree))
    if not same:
        raise SystemExit("the fused path is not deterministic: nothing timed")
    variants = [("fused", fused), ("unfused", unfused), ("plain", plain), ("unl_fwd alone", unl_fwd), ("head_bwd_u alone", bwd_u),
                ("head_bwd alone", bwd_plain), ("head_fwd alone", head_fwd)]
    us = interleaved(torch, variants, samples, reps)
    med = {}
    for name, _ in variants:
        v = us[name]
        med[name] = statistics.median(v)
        emit("%s  %-17s median %9.1f us (range %.1f .. %.1f over %d samples of %d)" % (tag, name, med[name], min(v), max(v), samples, reps))
    emit("%s  fused - plain: %+.1f us per step (x%.2f); unfused / fused: %.2fx; head_bwd_u / head_bwd: %.3fx" % (
        tag, med["fused"] - med["plain"], med["fused"] / med["plain"], med["unfused"] / med["fused"],
        med["head_bwd_u alone"] / med["head_bwd alone"]))


def whole_step(torch, F, emit, rounds=3, steps=8, only=None):
    md, data = importlib.import_module(PKG + ".model"), importlib.import_module(PKG + ".data")
    import main as cli
    dev = torch.device("cuda:0")
    on_flags = ["--unl_entropy", "0.1", "--unl_maxsq", "0.1", "--unl_pseudo", "0.1", "--unl_pseudo_thresh", "0.35"]
    models = {}
    for tag, extra in (("off", []), ("on", on_flags)):
        if only not in (None, tag):
            continue
        args = cli.get_args(["--model", "semisupervised_cycleGAN", "--dataset", "voc2012", "--crop_height", "256", "--crop_width", "256",
                             "--batch_size", "8", "--checkpoint_dir", "/tmp/sscg_unl_bench_ckpt"] + extra)
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
    if only is not None:
        emit("whole step voc2012 256x256 batch 8, tree %s, flags %s: %.2f ms (%s) (%d rounds of %d steps)" % (
            os.path.relpath(ROOT), only, statistics.median(times[only]), " ".join("%.2f" % t for t in times[only]), rounds, steps))
        return
    off, on = statistics.median(times["off"]), statistics.median(times["on"])
    emit("whole step voc2012 256x256 batch 8: flags off %.2f ms (%s), %s %.2f ms (%s): %+.2f ms, %+.2f %% (alternating, %d rounds of %d steps)" % (
        off, " ".join("%.2f" % t for t in times["off"]), " ".join(on_flags), on, " ".join("%.2f" % t for t in times["on"]), on - off,
        100 * (on - off) / off, rounds, steps))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--one-step", choices=["on", "off"], default=None)
    ap.add_argument("--root", type=str, default=None)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/unl_bench.py measures on the MI355X: no GPU here, nothing measured")
    F = importlib.import_module(PKG + ".functional")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    if a.one_step:
        return whole_step(torch, F, emit, only=a.one_step)
    emit("device: %s" % torch.cuda.get_device_name(0))
    for shape in SHAPES:
        kernels(torch, F, shape, a.samples, a.reps, emit)
    if a.step:
        whole_step(torch, F, emit)


if __name__ == "__main__":
    main()
