#!/usr/bin/env python
"""Times the fused L1 + SSIM image loss on the MI355X (include/sscg.h: sscg_l1_ssim_fwd / _bwd) at 8x3x256x256 and 16x3x256x512:

  fused     sscg_l1_ssim_fwd (with the coefficient maps) + sscg_l1_ssim_bwd (both terms)
  l1        sscg_l1_fwd + sscg_l1_bwd alone: what the same term costs without --ssim_weight
  unfused   the same maths composed from torch ops on the device (grouped separable conv2d over the five moment maps, autograd
            backward), plus torch's L1

Each sample is the device time of REPS back-to-back forward + backward pairs between two events, divided by REPS, after a warm-up;
the line gives the median of the samples and their range.  The achieved bytes/s of the fused pair is taken against the traffic it
cannot avoid: read a and b, write and read the three coefficient maps, write da.

  --step    also the whole training step (acdc, 256x256, batch 8) with --ssim_weight 0.5 against the flag off: two models in one
            process, timed alternately (bench.py takes no loss flags, so tools/ab.sh cannot switch this one)

usage: python tools/ssim_bench.py [--samples 30] [--reps 20] [--step] [--out FILE]   (needs the GPU: there is no CPU path)"""
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
SHAPES = [(8, 3, 256, 256), (16, 3, 256, 512)]


def timed(torch, fn, samples, reps, warmup=3):
    for _ in range(warmup * reps):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(samples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / reps)          # us per pair
    return statistics.median(out), min(out), max(out)


def kernels(torch, F, shape, samples, reps, emit):
    import torch.nn.functional as TF
    n, c, h, w = shape
    dev = torch.device("cuda:0")
    opts = F.SsimOptions()
    k = opts.window
    gen = torch.Generator().manual_seed(1)
    a = torch.tanh(torch.randn(n, c, h, w, generator=gen)).to(dev).contiguous(memory_format=torch.channels_last)
    b = torch.tanh(torch.randn(n, c, h, w, generator=gen)).to(dev).contiguous(memory_format=torch.channels_last)
    m = n * c * (h - k + 1) * (w - k + 1)
    numel = a.numel()
    lib, st = F.lib, F._stream()
    l1, loss = torch.empty((), device=dev), torch.empty((), device=dev)
    coef = torch.empty(3 * m, device=dev)
    da = torch.empty_like(a)
    g1, g2 = torch.full((), 1.0, device=dev), torch.full((), 0.5, device=dev)
    need = lib.sscg_ssim_workspace(n, h, w, c, k)
    ws = torch.empty(max(need, lib.sscg_loss_workspace(numel)), dtype=torch.uint8, device=dev)

    def fused():
        F.check(lib.sscg_l1_ssim_fwd(a.data_ptr(), b.data_ptr(), n, h, w, c, k, opts.sigma, opts.c1, opts.c2, l1.data_ptr(), loss.data_ptr(), None,
                                     coef.data_ptr(), ws.data_ptr(), ws.numel(), st), "sscg_l1_ssim_fwd")
        F.check(lib.sscg_l1_ssim_bwd(a.data_ptr(), b.data_ptr(), coef.data_ptr(), n, h, w, c, k, opts.sigma, g1.data_ptr(), 1.0, g2.data_ptr(), 1.0,
                                     da.data_ptr(), st), "sscg_l1_ssim_bwd")

    def plain():
        F.check(lib.sscg_l1_fwd(a.data_ptr(), b.data_ptr(), numel, l1.data_ptr(), ws.data_ptr(), ws.numel(), st), "sscg_l1_fwd")
        F.check(lib.sscg_l1_bwd(a.data_ptr(), b.data_ptr(), numel, g1.data_ptr(), 1.0, da.data_ptr(), st), "sscg_l1_bwd")

    d = torch.arange(k, dtype=torch.float64) - (k - 1) / 2
    g = torch.exp(-d * d / (2 * opts.sigma ** 2))
    g = (g / g.sum()).float().to(dev)
    wr, wc = g.view(1, 1, 1, -1).expand(c, 1, 1, -1).contiguous(), g.view(1, 1, -1, 1).expand(c, 1, -1, 1).contiguous()
    av = a.clone().requires_grad_(True)

    def filt(x):
        return TF.conv2d(TF.conv2d(x, wr, groups=c), wc, groups=c)

    def unfused():
        av.grad = None
        mua, mub = filt(av), filt(b)
        va, vb, cov = filt(av * av) - mua * mua, filt(b * b) - mub * mub, filt(av * b) - mua * mub
        s = (2 * mua * mub + opts.c1) * (2 * cov + opts.c2) / ((mua * mua + mub * mub + opts.c1) * (va + vb + opts.c2))
        ((av - b).abs().mean() + 0.5 * (1 - s.mean())).backward()

    tag = "%dx%dx%dx%d" % shape
    byts = 4 * (2 * numel + 6 * m + numel)
    res = {}
    for name, fn in (("fused", fused), ("l1", plain), ("unfused", unfused)):
        try:
            res[name] = timed(torch, fn, samples, reps)
            emit("%-13s %-8s median %9.1f us per forward + backward (range %.1f .. %.1f over %d samples of %d)" % (
                (tag, name) + res[name] + (samples, reps)))
        except Exception as e:                      # one leg must not take the others with it; the line says what happened
            emit("%-13s %-8s could not be run: %s: %s" % (tag, name, type(e).__name__, str(e).splitlines()[0] if str(e) else ""))
    if "fused" in res:
        emit("%-13s fused    compulsory traffic %.1f MB (a, b read; coef written and read; da written) -> %.2f TB/s achieved" % (
            tag, byts / 1e6, byts / res["fused"][0] / 1e6))
    if "fused" in res and "l1" in res:
        emit("%-13s fused / l1 alone: %.2fx (+%.1f us per step and term)" % (tag, res["fused"][0] / res["l1"][0], res["fused"][0] - res["l1"][0]))
    if "fused" in res and "unfused" in res:
        emit("%-13s unfused / fused: %.2fx" % (tag, res["unfused"][0] / res["fused"][0]))
        # faster and different is not faster: the two agree on the seeded input
        fused()
        torch.cuda.synchronize()
        unfused()
        err = float((av.grad - da).abs().max()) / float(av.grad.abs().max())
        emit("%-13s gradients of the two agree to %.1e of the largest" % (tag, err))


def whole_step(torch, F, emit, rounds=3, steps=8):
    md, data = importlib.import_module(PKG + ".model"), importlib.import_module(PKG + ".data")
    import main as cli
    dev = torch.device("cuda:0")
    models = {}
    for tag, extra in (("off", []), ("--ssim_weight 0.5", ["--ssim_weight", "0.5"])):
        args = cli.get_args(["--model", "semisupervised_cycleGAN", "--dataset", "acdc", "--crop_height", "256", "--crop_width", "256",
                             "--batch_size", "8", "--checkpoint_dir", "/tmp/sscg_ssim_bench_ckpt"] + extra)
        args.gpu_ids, args.as_written, args.overlap_d = [0], True, False
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            models[tag] = md.semisuper_cycleGAN(args)
    lab = list(data.SyntheticLoader(8, 4, 256, 256, 4, 3, device=dev))
    unl = list(data.SyntheticLoader(8, 4, 256, 256, 4, 4, device=dev))
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
    off, on = statistics.median(times["off"]), statistics.median(times["--ssim_weight 0.5"])
    emit("whole step acdc 256x256 batch 8: flag off %.2f ms (%s), --ssim_weight 0.5 %.2f ms (%s): %+.2f ms, %+.2f %% (alternating, %d rounds of %d steps)" % (
        off, " ".join("%.2f" % t for t in times["off"]), on, " ".join("%.2f" % t for t in times["--ssim_weight 0.5"]), on - off,
        100 * (on - off) / off, rounds, steps))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/ssim_bench.py measures on the MI355X: no GPU here, nothing measured")
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
