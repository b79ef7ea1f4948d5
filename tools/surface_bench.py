#!/usr/bin/env python
"""Surface distances of the evaluation (`--surface`, sscg_surface_stats) timed with HIP events on the MI355X.
  (a) one call on synthetic region maps (a coarse random label grid blown up to blocks, the prediction the same map moved by a few
      pixels) at ACDC B = 8, 4 classes, 256 x 256; VOC B = 8, 21 classes, 256 x 256 with a void ring; Cityscapes B = 16, 20 classes,
      256 x 512.  Beside the time: the launches of a call, the share of the pixels that lie on a surface, the cases that are defined,
      the workspace, and the confusion histogram and the contour counts (`--boundary`) on the same maps as yardsticks;
  (b) one evaluate() pass over a synthetic loader of --batches batches without and with the option (VOC and Cityscapes sizes with
      the datasets' own models; ACDC at its size).
Same process, warm-up first, the variants interleaved repetition by repetition, medians reported.  Nothing is promised or gated: the
cost of the option is whatever this prints.
usage: python tools/surface_bench.py [--reps 30] [--warmup 3] [--batches 16] [--configs acdc,voc,cityscapes] [--out FILE]"""
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

# dataset, classes, batch, map size, void ring
CONFIGS = {"acdc": ("acdc", 4, 8, (256, 256), False), "voc": ("voc2012", 21, 8, (256, 256), True),
           "cityscapes": ("cityscapes", 20, 16, (256, 512), False)}
BLOCK = 48                 # side of the label blocks of the synthetic maps


def region_maps(B, C, H, W, ring, g, dev):
    grid = torch.randint(0, C, (B, H // BLOCK + 2, W // BLOCK + 2), generator=g)
    gt = grid.repeat_interleave(BLOCK, 1).repeat_interleave(BLOCK, 2)[:, 11:11 + H, 5:5 + W].contiguous()
    pred = torch.roll(gt, (3, 5), (1, 2)).to(torch.uint8)
    if ring:
        gt[:, 0, :] = gt[:, -1, :] = gt[:, :, 0] = gt[:, :, -1] = 255
    return gt.to(dev), pred.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--configs", default="acdc,voc,cityscapes")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("surface_bench.py measures on the MI355X: no GPU here, nothing is reported")
    F = importlib.import_module(PKG + ".functional")
    L = importlib.import_module(PKG + "._lib")
    md = importlib.import_module(PKG + ".model")
    from oracle import fixtures as FX
    dev = torch.device("cuda", 0)
    opt, bopt = F.SurfaceOptions(), F.BoundaryOptions()
    lines = ["device: %s; %d repetitions after %d warm-up rounds, variants interleaved, HIP events" % (
        torch.cuda.get_device_name(0), a.reps, a.warmup), "surface: %r" % (opt,)]
    for key in a.configs.split(","):
        dataset, C, B, (H, W), ring = CONFIGS[key]
        g = torch.Generator().manual_seed(5)
        gt, pred = region_maps(B, C, H, W, ring, g, dev)
        pred64 = pred.to(torch.int64)
        stats, sums = F.surface_stats(gt, pred, C, opt)
        d = bopt.width(H, W)
        counts = F.boundary_counts(gt, pred, C, d)
        hist = F.confusion_hist(gt, pred64, C)
        cnt = stats[..., 0]
        defined = int(((cnt[0] > 0) & (cnt[1] > 0)).sum())
        chunks = -(-C // 8)
        lines.append("")
        lines.append("== %s: B = %d, %d classes, %d x %d: %.1f %% / %.1f %% of the pixels on a true / predicted surface, %d of %d cases defined, "
                     "workspace %.1f MB, %d launches per call" % (
                         dataset, B, C, H, W, 100.0 * int(cnt[0].sum()) / (B * H * W), 100.0 * int(cnt[1].sum()) / (B * H * W), defined,
                         B * C, L.lib.sscg_surface_workspace(B, H, W, C) / 1e6, 10 + 2 * chunks))
        names = ["surface_stats", "boundary_counts, d = %d" % d, "confusion_hist (16 B / pixel)"]
        ms = interleaved([(names[0], lambda: F.surface_stats(gt, pred, C, opt, stats=stats, sums=sums)),
                          (names[1], lambda: F.boundary_counts(gt, pred, C, d, counts)),
                          (names[2], lambda: F.confusion_hist(gt, pred64, C, hist))], a.reps, a.warmup)
        for name in names:
            lines.append("    " + row(name, ms[name]))
        if a.batches > 0:
            args = FX.make_args(dataset=dataset, crop_height=H, crop_width=W, batch_size=B, gpu_ids=[0], checkpoint_dir="/tmp/sscg_surface_bench",
                                as_written=True)
            with contextlib.redirect_stdout(io.StringIO()):
                m = md.supervised_model(args)
            loader = [(torch.randn(B, 3, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last), gt.unsqueeze(1), ["s"] * B)
                      for _ in range(a.batches)]

            def ev(o):
                def run():
                    m.set_surface(o)
                    return m.evaluate(loader)[0]
                return run

            lines.append("(b) evaluate() over %d batches (one DeepLab forward per batch + head + host scores)" % a.batches)
            ms = interleaved([("evaluate()", ev(None)), ("evaluate(), set_surface(on)", ev(opt))], max(a.reps // 3, 5), 1)
            for name in ms:
                lines.append("    " + row(name, ms[name]))
            u, f = statistics.median(ms["evaluate()"]), statistics.median(ms["evaluate(), set_surface(on)"])
            lines.append("    with / without = %.4f (%+.2f %%, %+.3f ms per batch)" % (f / u, 100.0 * (f - u) / u, (f - u) / a.batches))
            m.set_surface(None)
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
