#!/usr/bin/env python
"""Connected-component filtering of predicted label maps (`--components`, sscg_components_filter) timed with HIP events on the MI355X
against the path a user has without it, at the evaluation's sizes: VOC B = 8, 21 classes, 320 x 320; Cityscapes B = 16, 20 classes,
512 x 1024; ACDC B = 8, 4 classes, 256 x 256.
  device: F.component_filter on the uint8 map the head wrote, with the ground truth and the confusion matrix (what the score keeper
          calls), and without them (what validation.py / testing.py call);
  host:   the device-to-host copy of the map, scipy.ndimage.label plus np.bincount per sample and class, the relabelling, and the
          host-to-device copy back (tests/components_reference.py's arithmetic without its bookkeeping); its three parts are also timed
          on their own;
  beside them the confusion histogram on the same maps as a yardstick of one pass over 16 B per pixel.
The maps are block label maps (a coarse random grid blown up) with 3 % of the pixels replaced by a random class, so that small islands
exist.  Same process, warm-up first, the device variants interleaved repetition by repetition, medians reported; the host path runs
--host_reps times (it takes seconds at the Cityscapes size).  Nothing is promised or gated: the cost is whatever this prints.
usage: python tools/components_bench.py [--reps 30] [--warmup 3] [--host_reps 3] [--configs acdc,voc,cityscapes] [--out FILE]"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np
import torch
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from predict_bench import PKG, interleaved, row, timed  # noqa: E402

# dataset, classes, batch, map size, void ring
CONFIGS = {"acdc": ("acdc", 4, 8, (256, 256), False), "voc": ("voc2012", 21, 8, (320, 320), True),
           "cityscapes": ("cityscapes", 20, 16, (512, 1024), False)}
BLOCK = 48                 # side of the label blocks of the synthetic maps
SPECKLE = 0.03             # share of the pixels replaced by a random class
FULL = ndimage.generate_binary_structure(2, 2)


def speckled_maps(B, C, H, W, ring, g, dev):
    grid = torch.randint(0, C, (B, H // BLOCK + 2, W // BLOCK + 2), generator=g)
    gt = grid.repeat_interleave(BLOCK, 1).repeat_interleave(BLOCK, 2)[:, 11:11 + H, 5:5 + W].contiguous()
    pred = torch.roll(gt, (3, 5), (1, 2))
    hit = torch.rand((B, H, W), generator=g) < SPECKLE
    pred = torch.where(hit, torch.randint(0, C, (B, H, W), generator=g), pred).to(torch.uint8)
    if ring:
        gt[:, 0, :] = gt[:, -1, :] = gt[:, :, 0] = gt[:, :, -1] = 255
    return gt.to(dev), pred.to(dev)


def host_filter(maps, C, min_area, fill):
    """What a user does today with the map on the host: per sample and class label, bincount, relabel the small ones."""
    out = maps.copy()
    for n in range(maps.shape[0]):
        for c in range(C):
            if c == fill:
                continue
            ids, count = ndimage.label(maps[n] == c, structure=FULL)
            if count:
                small = np.bincount(ids.ravel(), minlength=count + 1) < min_area
                small[0] = False
                out[n][small[ids]] = fill
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host_reps", type=int, default=3)
    ap.add_argument("--configs", default="acdc,voc,cityscapes")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("components_bench.py measures on the MI355X: no GPU here, nothing is reported")
    F = importlib.import_module(PKG + ".functional")
    L = importlib.import_module(PKG + "._lib")
    U = importlib.import_module(PKG + ".utils")
    dev = torch.device("cuda", 0)
    opt = U.parse_components("on")
    big = F.ComponentOptions(largest=True)
    lines = ["device: %s; %d repetitions after %d warm-up rounds, device variants interleaved, HIP events; host path %d repetitions" % (
        torch.cuda.get_device_name(0), a.reps, a.warmup, a.host_reps), "components: %r (--components on) and %r" % (opt, big)]
    for key in a.configs.split(","):
        dataset, C, B, (H, W), ring = CONFIGS[key]
        g = torch.Generator().manual_seed(5)
        gt, pred = speckled_maps(B, C, H, W, ring, g, dev)
        pred64 = pred.to(torch.int64)
        out, hist, stats = F.component_filter(pred, C, opt, label_true=gt, stats=True)
        want = host_filter(pred.cpu().numpy(), C, opt.min_area, opt.fill)
        if not np.array_equal(out.cpu().numpy(), want):
            sys.exit("components_bench.py: the device and the host path disagree at %s" % key)
        st = stats.sum(dim=0).cpu().numpy()
        pix = B * H * W
        lines.append("")
        lines.append("== %s: B = %d, %d classes, %d x %d: %d components, %d kept, %.2f %% of the pixels relabelled (the host path gives the "
                     "same bytes), workspace %.1f MB, 5 launches per call" % (
                         dataset, B, C, H, W, int(st[:, 0].sum()), int(st[:, 1].sum()), 100.0 * float((out != pred).sum()) / pix,
                         L.lib.sscg_components_workspace(B, H, W, C) / 1e6))
        hist2 = F.confusion_hist(gt, pred64, C)
        names = ["component_filter + hist + stats", "component_filter, largest", "component_filter, map only", "confusion_hist (16 B / pixel)"]
        ms = interleaved([(names[0], lambda: F.component_filter(pred, C, opt, label_true=gt, hist=hist, out=out, stats=stats)),
                          (names[1], lambda: F.component_filter(pred, C, big, label_true=gt, hist=hist, out=out, stats=stats)),
                          (names[2], lambda: F.component_filter(pred, C, opt, out=out)),
                          (names[3], lambda: F.confusion_hist(gt, pred64, C, hist2))], a.reps, a.warmup)
        for name in names:
            lines.append("    " + row(name, ms[name]))
        dev_ms = statistics.median(ms[names[2]])
        lines.append("    map only: %.3f ns per pixel, %.0f GB/s over the 8 + 2 B per pixel of workspace writes, map read and map write it cannot "
                     "avoid" % (1e6 * dev_ms / pix, 10.0 * pix / (dev_ms * 1e6)))

        def host_path():
            return host_filter(pred.cpu().numpy(), C, opt.min_area, opt.fill)

        def host_round_trip():
            return torch.from_numpy(host_path()).to(dev)

        host = [timed(host_round_trip)[0] for _ in range(a.host_reps)]
        lines.append("    " + row("host: copy, scipy label, copy back", host))
        parts = {"d2h copy of the map": [], "scipy label + bincount + relabel": [], "h2d copy back": []}
        for _ in range(a.host_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            np_map = pred.cpu().numpy()
            t1 = time.perf_counter()
            res = host_filter(np_map, C, opt.min_area, opt.fill)
            t2 = time.perf_counter()
            torch.from_numpy(res).to(dev)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            for k, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2)):
                parts[k].append(1e3 * v)
        for k, v in parts.items():
            lines.append("        " + row(k + " (host clock)", v))
        lines.append("    host / device (map only) = %.0f x" % (statistics.median(host) / dev_ms))
        del gt, pred, pred64, out
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
