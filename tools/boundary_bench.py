#!/usr/bin/env python
"""Contour scores of the evaluation (`--boundary`, sscg_boundary_counts) timed with HIP events on the MI355X.
  (a) the kernel alone on synthetic region maps (a coarse random label grid blown up to blocks, the prediction the same map moved by a
      few pixels, a void strip) at the widths the published ratio 0.02 gives: VOC B = 8, 256 x 256, d = 7; Cityscapes B = 16, 256 x 512,
      d = 11; and 16 x 512 x 1024, d = 23.  Beside the time: the bytes it has to read at least (8 B of ground truth and 1 B of
      prediction per pixel) and the effective bandwidth that makes, so the distance to the HBM bound is visible.  The confusion
      histogram on the same maps (sscg_confusion_hist, 16 B per pixel) runs beside it as a yardstick of a pure streaming count;
  (b) one evaluate() pass over a synthetic loader of --batches batches without and with the option.
Same process, warm-up first, the variants interleaved repetition by repetition, medians reported.  Nothing is promised or gated: the
cost of the option is whatever this prints.
usage: python tools/boundary_bench.py [--reps 30] [--warmup 3] [--batches 16] [--configs voc,cityscapes,full] [--out FILE]"""
import argparse
import contextlib
import importlib
import io
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from predict_bench import PKG, interleaved, row  # noqa: E402

# dataset, classes, batch, map size, whether evaluate() is timed at this size too
CONFIGS = {"voc": ("voc2012", 21, 8, (256, 256), True), "cityscapes": ("cityscapes", 20, 16, (256, 512), True),
           "full": ("cityscapes", 20, 16, (512, 1024), False)}
HBM_PEAK = 8.0e12          # bytes / s, the MI355X's specified peak
BLOCK = 48                 # side of the label blocks of the synthetic maps


def region_maps(B, C, H, W, g, dev):
    grid = torch.randint(0, C, (B, H // BLOCK + 2, W // BLOCK + 2), generator=g)
    gt = grid.repeat_interleave(BLOCK, 1).repeat_interleave(BLOCK, 2)[:, 11:11 + H, 5:5 + W].contiguous()
    pred = torch.roll(gt, (3, 5), (1, 2)).to(torch.uint8)
    gt[:, :, :2] = 255
    return gt.to(dev), pred.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--configs", default="voc,cityscapes,full")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("boundary_bench.py measures on the MI355X: no GPU here, nothing is reported")
    F = importlib.import_module(PKG + ".functional")
    md = importlib.import_module(PKG + ".model")
    from oracle import fixtures as FX
    dev = torch.device("cuda", 0)
    opt = F.BoundaryOptions()
    lines = ["device: %s; %d repetitions after %d warm-up rounds, variants interleaved, HIP events" % (
        torch.cuda.get_device_name(0), a.reps, a.warmup), "boundary: %r" % (opt,)]
    for key in a.configs.split(","):
        dataset, C, B, (H, W), with_eval = CONFIGS[key]
        d = opt.width(H, W)
        g = torch.Generator().manual_seed(5)
        gt, pred = region_maps(B, C, H, W, g, dev)
        pred64 = pred.to(torch.int64)
        counts = F.boundary_counts(gt, pred, C, d)
        hist = F.confusion_hist(gt, pred64, C)
        bt = counts[:C].sum().item()
        lines.append("")
        lines.append("== %s: B = %d, %d classes, %d x %d, d = %d (%.1f %% of the valid pixels in E_t)" % (
            dataset, B, C, H, W, d, 100.0 * bt / max(1, int((gt != 255).sum()))))
        names = ["boundary_counts, d = %d" % d, "boundary_counts, d = 1", "confusion_hist (16 B / pixel)"]
        ms = interleaved([(names[0], lambda: F.boundary_counts(gt, pred, C, d, counts)),
                          (names[1], lambda: F.boundary_counts(gt, pred, C, 1, counts)),
                          (names[2], lambda: F.confusion_hist(gt, pred64, C, hist))], a.reps, a.warmup)
        for name in names:
            lines.append("    " + row(name, ms[name]))
        t = statistics.median(ms[names[0]])
        must = B * H * W * 9
        lines.append("(a) the kernel must read %.1f MB (9 B per pixel): %.3f ms is %.2f TB/s effective, %.1fx the time at the %.1f TB/s HBM peak "
                     "(HIP events around one launch: launch overhead included)" % (must / 1e6, t, must / (t * 1e-3) / 1e12,
                                                                                 t / (1e3 * must / HBM_PEAK), HBM_PEAK / 1e12))
        if with_eval and a.batches > 0:
            args = FX.make_args(dataset=dataset, crop_height=H, crop_width=W, batch_size=B, gpu_ids=[0], checkpoint_dir="/tmp/sscg_boundary_bench",
                                as_written=True)
            with contextlib.redirect_stdout(io.StringIO()):
                m = md.supervised_model(args)
            loader = [(torch.randn(B, 3, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last), gt.unsqueeze(1), ["s"] * B)
                      for _ in range(a.batches)]
            ev = lambda o: (lambda: m.evaluate(loader, boundary=o)[0])
            lines.append("(b) evaluate() over %d batches (one DeepLab forward per batch + head + host mIoU)" % a.batches)
            ms = interleaved([("evaluate()", ev(None)), ("evaluate(boundary=on)", ev(opt))], max(a.reps // 3, 5), 1)
            for name in ms:
                lines.append("    " + row(name, ms[name]))
            u, f = statistics.median(ms["evaluate()"]), statistics.median(ms["evaluate(boundary=on)"])
            lines.append("    with / without = %.4f (%+.2f %%, %+.3f ms per batch)" % (f / u, 100.0 * (f - u) / u, (f - u) / a.batches))
            del m, loader
        del gt, pred, pred64
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
