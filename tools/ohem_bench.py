#!/usr/bin/env python
"""Forward + backward of the label head with a mined (OHEM) cross entropy, timed with HIP events on the MI355X at the two head shapes of
the training step (DeepLab's stride-8 logit map -> the crop):
  fused     : functional.upsample_softmax_ce(..., ohem=) - sscg_ohem_fwd, then ONE stencil launch backward (sscg_upsample_head_bwd_h);
  separate  : the composition a user has without it - upsample_bilinear -> softmax2d -> gather of p[y] -> torch.kthvalue (its rank
              needs the counted pixels on the host: one sync) -> cross_entropy of the resized logits with every pixel that is not kept
              mapped to the void id - and its backward through the resized [B, C, crop] maps;
  plain     : the fused head without mining (sscg_upsample_head_fwd / _bwd): what the option costs.
Each figure is the time of --burst forward + backward passes divided by --burst, launch path included (the composition's sync is part of
what it costs); the variants are interleaved repetition by repetition and medians are reported.  Before anything is timed the fused
and the separate form are compared: same threshold up to fp32 rounding, same kept count up to the pixels at the threshold.
usage: python tools/ohem_bench.py [--reps 30] [--warmup 3] [--burst 10] [--configs voc,cityscapes] [--out FILE]"""
import argparse
import importlib
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from predict_bench import PKG, interleaved, row  # noqa: E402

# dataset, classes, batch, logit map, crop
CONFIGS = {"voc": ("voc2012", 21, 8, (33, 33), (256, 256)), "cityscapes": ("cityscapes", 20, 16, (33, 65), (256, 512))}
THRESH, MIN_KEPT, MIN_FRAC = 0.7, 100000, 0.0625


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--configs", default="voc,cityscapes")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ohem_bench.py measures on the MI355X: no GPU here, nothing is reported")
    F = importlib.import_module(PKG + ".functional")
    dev = torch.device("cuda", 0)
    opt = F.OhemOptions(THRESH, min_kept=MIN_KEPT, min_frac=MIN_FRAC)
    lines = ["device: %s; %d repetitions after %d warm-up rounds, variants interleaved, HIP events around %d forward + backward passes each" % (
        torch.cuda.get_device_name(0), a.reps, a.warmup, a.burst),
        "OHEM: thresh %g, min_kept %d, min_frac %g" % (THRESH, MIN_KEPT, MIN_FRAC)]
    for key in a.configs.split(","):
        dataset, C, B, (H, W), (OH, OW) = CONFIGS[key]
        g = torch.Generator().manual_seed(5)
        x = (torch.randn(B, C, H, W, generator=g) * 3).to(dev).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            guess = F.predict_labels(x, (OH, OW), want_index=True, want_u8=False)[1].cpu()
        lab = torch.randint(0, C, (B, OH, OW), generator=g)
        lab = torch.where(torch.rand(lab.shape, generator=g) < 0.7, guess, lab)      # most labels agree with the net, as in training
        lab.view(-1)[::9] = 255
        lab = lab.to(dev)
        state = {}

        def fused():
            for _ in range(a.burst):
                xg = x.detach().requires_grad_(True)
                loss = F.upsample_softmax_ce(xg, (OH, OW), lab, want_soft=False, ohem=opt)[1]
                loss.backward()
            state["fused"] = (loss.detach(), xg.grad) + F.ohem_stats()

        def separate():
            for _ in range(a.burst):
                xg = x.detach().requires_grad_(True)
                up = F.upsample_bilinear(xg, (OH, OW))
                p = F.softmax2d(up).detach()
                counted = (lab >= 0) & (lab < C)
                k = p.gather(1, torch.where(counted, lab, torch.zeros_like(lab)).unsqueeze(1)).squeeze(1)
                kc = k[counted]                                                   # (a sync: the number of counted pixels shapes it)
                V = kc.numel()
                r = min(max(MIN_KEPT, int(math.ceil(MIN_FRAC * V)), 1), V)
                tau = torch.clamp(torch.kthvalue(kc, r).values, min=THRESH)
                mined = torch.where(counted & (k <= tau), lab, torch.full_like(lab, 255))
                loss = F.cross_entropy(up, mined)
                loss.backward()
            state["separate"] = (loss.detach(), xg.grad, tau, (mined != 255).sum(), torch.tensor(V))

        def plain():
            for _ in range(a.burst):
                xg = x.detach().requires_grad_(True)
                loss = F.upsample_softmax_ce(xg, (OH, OW), lab, want_soft=False)[1]
                loss.backward()

        fused(), separate()
        torch.cuda.synchronize()
        fl, fg, fthr, fkept, fV = state["fused"]
        sl, sg, sthr, skept, sV = state["separate"]
        lines.append("")
        lines.append("== %s: B = %d, %d classes, logits %dx%d -> %dx%d" % (dataset, B, C, H, W, OH, OW))
        lines.append("  fused:    loss %.7f  thr %.9g  kept %d of %d (share %.4f)" % (float(fl), float(fthr), int(fkept), int(fV), int(fkept) / max(int(fV), 1)))
        lines.append("  separate: loss %.7f  thr %.9g  kept %d of %d;  gradient max-abs difference %.2e of %.2e" % (
            float(sl), float(sthr), int(skept), int(sV), float((fg - sg).abs().max()), float(sg.abs().max())))
        variants = [("fused OHEM head", fused), ("separate passes + kthvalue", separate), ("plain fused head (no mining)", plain)]
        ms = interleaved(variants, a.reps, a.warmup)
        base = statistics.median(ms["fused OHEM head"])
        for name, _ in variants:
            lines.append("    " + row(name, [v / a.burst for v in ms[name]]) + "   x%.3f of the fused OHEM head" % (statistics.median(ms[name]) / base))
        med = {name: statistics.median(ms[name]) for name, _ in variants}
        lines.append("  fused against separate: x%.2f %s; the option costs x%.2f of the plain fused head" % (
            med["separate passes + kthvalue"] / base, "faster" if med["separate passes + kthvalue"] > base else "SLOWER - the fused form loses here",
            base / med["plain fused head (no mining)"]))
        del x, lab
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
