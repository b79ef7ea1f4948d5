#!/usr/bin/env python
"""The fused label head with the class-weighted / label-smoothed cross entropy against the plain one, timed with HIP events on the
MI355X at the training step's sizes (DeepLab's stride-8 logit map -> the crop).
  forward : sscg_upsample_head_fwd            vs  sscg_upsample_head_fwd_w with weights, with smoothing, with both
            (each with and without the softmax output: the lab_loss_CE and the gt_cycle_loss call sites)
  backward: sscg_upsample_head_bwd - the same entry for all of them (scale of the gradient the forward left, or the softmax backward
            plus that scale)
Each figure is the time of --burst back-to-back launches of one entry divided by --burst (the kernels, not the launch path); the
variants are interleaved repetition by repetition and medians are reported.  Before anything is timed, the weighted entry with NULL
weights and smoothing 0 is compared with the plain entry bit for bit.
usage: python tools/ce_bench.py [--reps 30] [--warmup 3] [--burst 20] [--configs voc,cityscapes] [--out FILE]"""
import argparse
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from predict_bench import PKG, interleaved, row  # noqa: E402

# dataset, classes, batch, logit map, crop
CONFIGS = {"voc": ("voc2012", 21, 8, (33, 33), (256, 256)), "cityscapes": ("cityscapes", 20, 16, (33, 65), (256, 512)),
           "acdc": ("acdc", 4, 8, (33, 33), (256, 256))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--configs", default="voc,cityscapes,acdc")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ce_bench.py measures on the MI355X: no GPU here, nothing is reported")
    F = importlib.import_module(PKG + ".functional")
    lib, dev = F.lib, torch.device("cuda", 0)
    lines = ["device: %s; %d repetitions after %d warm-up rounds, variants interleaved, HIP events around %d launches each" % (
        torch.cuda.get_device_name(0), a.reps, a.warmup, a.burst)]
    for key in a.configs.split(","):
        dataset, C, B, (H, W), (OH, OW) = CONFIGS[key]
        g = torch.Generator().manual_seed(5)
        x = (torch.randn(B, H, W, C, generator=g) * 3).to(dev)
        lab = torch.randint(0, C, (B, OH, OW), generator=g)
        lab.view(-1)[::9] = 255
        lab = lab.to(dev)
        w = F.ce_weight((torch.rand(C, generator=g) + 0.2).tolist(), C, dev)
        loss, valid, one = torch.zeros(1, device=dev), torch.zeros(1, device=dev), torch.ones(1, device=dev)
        dl, dx = torch.empty(B, H, W, C, device=dev), torch.empty(B, H, W, C, device=dev)
        y, dy = torch.empty(B, OH, OW, C, device=dev), torch.randn(B, OH, OW, C, generator=g).to(dev)
        ws = torch.empty(lib.sscg_upsample_head_workspace(B, H, W), dtype=torch.uint8, device=dev)

        def fwd(weight, eps, soft, plain=False):
            def run():
                for _ in range(a.burst):
                    if plain:
                        rc = lib.sscg_upsample_head_fwd(x.data_ptr(), lab.data_ptr(), y.data_ptr() if soft else None, loss.data_ptr(),
                                                        valid.data_ptr(), dl.data_ptr(), B, H, W, C, OH, OW, ws.data_ptr(), ws.numel(), F._stream())
                    else:
                        rc = lib.sscg_upsample_head_fwd_w(x.data_ptr(), lab.data_ptr(), None if weight is None else weight.data_ptr(), eps,
                                                          y.data_ptr() if soft else None, loss.data_ptr(), valid.data_ptr(), dl.data_ptr(),
                                                          B, H, W, C, OH, OW, ws.data_ptr(), ws.numel(), F._stream())
                    assert rc == 0
            return run

        def bwd(soft):
            def run():
                for _ in range(a.burst):
                    assert lib.sscg_upsample_head_bwd(x.data_ptr(), dy.data_ptr() if soft else None, dl.data_ptr(), one.data_ptr(),
                                                      valid.data_ptr(), dx.data_ptr(), B, H, W, C, OH, OW, F._stream()) == 0
            return run

        def outputs(run):
            for t in (loss, valid, dl, y):
                t.fill_(7.0)
            run()
            torch.cuda.synchronize()
            return [t.clone() for t in (loss, valid, dl, y)]

        same = all(torch.equal(p, q) for p, q in zip(outputs(fwd(None, 0.0, True, plain=True)), outputs(fwd(None, 0.0, True))))
        lines.append("")
        lines.append("== %s: B = %d, %d classes, logits %dx%d -> %dx%d; _w entry with NULL weights and smoothing 0 bit-identical to the "
                     "plain entry: %s" % (dataset, B, C, H, W, OH, OW, same))
        if not same:
            sys.exit("\n".join(lines + ["the dispatch of the _w entry does not reproduce the plain entry: nothing timed"]))
        for soft in (True, False):
            lines.append("  forward, %s" % ("loss + softmax output (lab_loss_CE site)" if soft else "loss only (gt_cycle_loss / supervised site)"))
            variants = [("plain", fwd(None, 0.0, soft, plain=True)), ("weights", fwd(w, 0.0, soft)), ("smoothing 0.1", fwd(None, 0.1, soft)),
                        ("weights + smoothing 0.1", fwd(w, 0.1, soft))]
            ms = interleaved(variants, a.reps, a.warmup)
            base = statistics.median(ms["plain"])
            for name, _ in variants:
                per = [v / a.burst for v in ms[name]]
                lines.append("    " + row(name, per) + "   x%.3f of plain" % (statistics.median(ms[name]) / base))
        ms = interleaved([("backward: scale only", bwd(False)), ("backward: softmax + scale", bwd(True))], a.reps, a.warmup)
        lines.append("  backward (sscg_upsample_head_bwd, shared by every variant)")
        for name in ms:
            lines.append("    " + row(name, [v / a.burst for v in ms[name]]))
        del x, lab, y, dy, dl, dx
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
