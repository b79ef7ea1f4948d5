#!/usr/bin/env python
"""The Dice branch of the fused label head against the head's own passes, timed with HIP events on the MI355X at the training step's
sizes (DeepLab's stride-8 logit map -> the crop).
  forward : sscg_dice_fwd (statistics + finish, per-sample and batch groups)   vs  sscg_upsample_head_fwd (the cross-entropy forward
            of the same tree: the 4x-redundant stencil pass), loss only and loss + softmax output
  backward: sscg_upsample_head_bwd_d (Dice only; Dice + CE; Dice + CE + dy_soft)  vs  sscg_upsample_head_bwd with dy_soft - the
            comparable stencil pass - and its scale-only form
  flat    : sscg_dice_fwd / sscg_dice_bwd on the materialised crop-size logits (the path taken where the head is not fused)
Each figure is the time of --burst back-to-back launches of one entry divided by --burst (the kernels, not the launch path); the
variants are interleaved repetition by repetition and medians are reported.  Before anything is timed, sscg_dice_fwd is run twice and
its outputs compared bit for bit.
usage: python tools/dice_bench.py [--reps 30] [--warmup 3] [--burst 20] [--configs voc,cityscapes] [--out FILE]"""
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
    ap.add_argument("--configs", default="voc,cityscapes")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dice_bench.py measures on the MI355X: no GPU here, nothing is reported")
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
        loss, valid, one = torch.zeros(1, device=dev), torch.zeros(1, device=dev), torch.ones(1, device=dev)
        dl, dx = torch.empty(B, H, W, C, device=dev), torch.empty(B, H, W, C, device=dev)
        y, dy = torch.empty(B, OH, OW, C, device=dev), torch.randn(B, OH, OW, C, generator=g).to(dev)
        ws = torch.empty(lib.sscg_upsample_head_workspace(B, H, W), dtype=torch.uint8, device=dev)
        dws = torch.empty(lib.sscg_dice_workspace(B, OH, OW, C), dtype=torch.uint8, device=dev)
        dloss, sums, coef = torch.zeros(1, device=dev), torch.zeros(B, C, 3, device=dev, dtype=torch.float64), torch.zeros(B, C, 2, device=dev)
        up = torch.empty(B, OH, OW, C, device=dev)
        assert lib.sscg_upsample_bilinear_fwd(x.data_ptr(), up.data_ptr(), B, H, W, C, OH, OW, F._stream()) == 0
        dup = torch.empty(B, OH, OW, C, device=dev)

        def ce_fwd(soft):
            def run():
                for _ in range(a.burst):
                    assert lib.sscg_upsample_head_fwd(x.data_ptr(), lab.data_ptr(), y.data_ptr() if soft else None, loss.data_ptr(),
                                                      valid.data_ptr(), dl.data_ptr(), B, H, W, C, OH, OW, ws.data_ptr(), ws.numel(), F._stream()) == 0
            return run

        def dice_fwd(batch, flat=False):
            def run():
                for _ in range(a.burst):
                    src, h, w = (up, OH, OW) if flat else (x, H, W)
                    assert lib.sscg_dice_fwd(src.data_ptr(), lab.data_ptr(), B, h, w, C, OH, OW, None, 1.0, batch, dloss.data_ptr(), sums.data_ptr(),
                                             coef.data_ptr(), dws.data_ptr(), dws.numel(), F._stream()) == 0
            return run

        def head_bwd(soft):
            def run():
                for _ in range(a.burst):
                    assert lib.sscg_upsample_head_bwd(x.data_ptr(), dy.data_ptr() if soft else None, dl.data_ptr(), one.data_ptr(),
                                                      valid.data_ptr(), dx.data_ptr(), B, H, W, C, OH, OW, F._stream()) == 0
            return run

        def head_bwd_d(soft, ce):
            def run():
                for _ in range(a.burst):
                    assert lib.sscg_upsample_head_bwd_d(x.data_ptr(), lab.data_ptr(), dy.data_ptr() if soft else None, dl.data_ptr() if ce else None,
                                                        one.data_ptr() if ce else None, valid.data_ptr() if ce else None, coef.data_ptr(),
                                                        one.data_ptr(), 0, dx.data_ptr(), B, H, W, C, OH, OW, F._stream()) == 0
            return run

        def flat_bwd():
            for _ in range(a.burst):
                assert lib.sscg_dice_bwd(up.data_ptr(), lab.data_ptr(), B, OH, OW, C, coef.data_ptr(), 0, one.data_ptr(), 1.0, dup.data_ptr(),
                                         F._stream()) == 0

        def outputs():
            for t in (dloss, sums, coef):
                t.fill_(7.0)
            dice_fwd(0)()
            torch.cuda.synchronize()
            return [t.clone() for t in (dloss, sums, coef)]

        ce_fwd(True)()                    # dl / valid for the backward variants
        same = all(torch.equal(p, q) for p, q in zip(outputs(), outputs()))
        lines.append("")
        lines.append("== %s: B = %d, %d classes, logits %dx%d -> %dx%d; sscg_dice_fwd twice bit-identical: %s; Dice loss %.6f" % (
            dataset, B, C, H, W, OH, OW, same, float(dloss)))
        if not same:
            sys.exit("\n".join(lines + ["sscg_dice_fwd is not deterministic: nothing timed"]))
        variants = [("CE forward, loss only", ce_fwd(False)), ("CE forward, loss + softmax", ce_fwd(True)),
                    ("Dice stats + finish, per sample", dice_fwd(0)), ("Dice stats + finish, batch", dice_fwd(1)),
                    ("Dice stats + finish, flat (materialised)", dice_fwd(0, flat=True))]
        ms = interleaved(variants, a.reps, a.warmup)
        base = statistics.median(ms["CE forward, loss only"])
        lines.append("  forward")
        for name, _ in variants:
            lines.append("    " + row(name, [v / a.burst for v in ms[name]]) + "   x%.3f of the CE forward (loss only)" % (statistics.median(ms[name]) / base))
        variants = [("head_bwd: scale only", head_bwd(False)), ("head_bwd: dy_soft + CE", head_bwd(True)),
                    ("head_bwd_d: Dice only", head_bwd_d(False, False)), ("head_bwd_d: Dice + CE", head_bwd_d(False, True)),
                    ("head_bwd_d: Dice + CE + dy_soft", head_bwd_d(True, True)), ("flat dice_bwd (materialised)", flat_bwd)]
        ms = interleaved(variants, a.reps, a.warmup)
        base = statistics.median(ms["head_bwd: dy_soft + CE"])
        lines.append("  backward")
        for name, _ in variants:
            lines.append("    " + row(name, [v / a.burst for v in ms[name]]) + "   x%.3f of head_bwd with dy_soft" % (statistics.median(ms[name]) / base))
        del x, lab, y, dy, dl, dx, up, dup
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
