#!/usr/bin/env python
"""The fused augmenting batch finish (sscg_augment_u8) against what it replaces, on one MI355X.
  (a) the fused launch with identity matrices                       HIP events
  (b) the fused launch with a drawn rotate + scale batch            HIP events
  (c) sscg_image_u8_to_f32 + sscg_label_lut on the same bytes       HIP events   (writes the bytes (a) writes)
  (d) the PIL path (Compose.__call__) over the same batch            host wall time, one process, no workers
and the colour table of sscg_augment_colour_u8 against the plain launch, all three at the drawn maps of (b), interleaved among themselves:
  (e) the plain fused launch                                         HIP events
  (f) the colour launch, table without a contrast (no mean)          HIP events
  (g) the colour launch with the image mean (clear + sum pass + launch)   HIP events
Same process, warm-up first, the variants interleaved repetition by repetition, medians reported, with bytes written over kernel time
beside the device figures.  (a) is compared with (c), and the colour launch with the identity table with (e), bit for bit before anything is timed.
usage: python tools/augment_bench.py [--reps 30] [--warmup 3] [--configs voc,cityscapes] [--spec rotate=10,scale=0.5:2]
                                     [--colour brightness=0.4,contrast=0.4,saturation=0.4,hue=0.1] [--out FILE]"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "semi-supervised-segmentation-cyclegan_amd"
CONFIGS = {"voc": ("voc2012", 8, 320, 320), "cityscapes": ("cityscapes", 16, 512, 1024)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def row(name, v, nbytes=None):
    v = sorted(v)
    med = statistics.median(v)
    tail = "   %7.1f GB/s written" % (nbytes / med / 1e6) if nbytes else ""
    return "%-46s median %9.4f ms   min %9.4f   p90 %9.4f   (n = %d)%s" % (name, med, v[0], v[int(0.9 * (len(v) - 1))], len(v), tail)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="voc,cityscapes")
    ap.add_argument("--spec", default="rotate=10,scale=0.5:2")
    ap.add_argument("--colour", default="brightness=0.4,contrast=0.4,saturation=0.4,hue=0.1")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("augment_bench.py measures on the MI355X: no GPU here, nothing is reported")
    F = importlib.import_module(PKG + ".functional")
    du = importlib.import_module(PKG + ".data_utils")
    dev = torch.device("cuda", 0)
    lines = ["device: %s; %d repetitions after %d warm-up rounds, variants interleaved; (a)-(c) HIP events, (d) host wall time" % (
        torch.cuda.get_device_name(0), a.reps, a.warmup)]
    for key in a.configs.split(","):
        dataset, B, H, W = CONFIGS[key]
        rng = np.random.RandomState(7)
        img = rng.randint(0, 256, (B, H, W, 3), dtype=np.uint8)
        gt = rng.randint(0, 21, (B, H, W)).astype(np.uint8)
        comp = du.augmentations.from_spec(a.spec, (H, W), label_fill=du.LABEL_FILL[dataset], out_size=(H, W), seed=11)
        drawn = torch.from_numpy(comp.matrices(np.random.RandomState(11), B, W, H)).to(dev)
        ident = torch.tensor([65536, 0, 0, 0, 65536, 0], dtype=torch.int32).repeat(B, 1).to(dev)
        d_img, d_gt = torch.from_numpy(img).to(dev), torch.from_numpy(gt).to(dev)
        lut = du.label_table(dataset).to(dev)
        mean, std = torch.full((3,), .5, device=dev), torch.full((3,), .5, device=dev)
        pil = [(Image.fromarray(img[i]), Image.fromarray(gt[i])) for i in range(B)]
        nbytes = B * H * W * (3 * 4 + 8)

        fused = lambda m: F.augment_batch(d_img, d_gt, m, (H, W), mean, std, lut, label_fill=comp.label_fill)
        unfused = lambda: (F.image_u8_to_f32(d_img, mean, std), F.label_lut(d_gt, lut))
        host = lambda: [comp(i, g) for i, g in pil]
        (i0, g0), (i1, g1) = fused(ident), unfused()
        same = torch.equal(i0, i1) and torch.equal(g0, g1)
        lines += ["", "== %s: B = %d, %d x %d x 3 uint8 + labels -> fp32 + int64 (%.1f MB written); --augment %s" % (
            dataset, B, H, W, nbytes / 1e6, a.spec), "(a) bit-identical to (c): %s" % same]
        if not same:
            sys.exit("\n".join(lines + ["the fused launch with identity maps does not reproduce the two passes: nothing timed"]))
        variants = [("(a) fused, identity maps", lambda: fused(ident), timed), ("(b) fused, drawn maps", lambda: fused(drawn), timed),
                    ("(c) image_u8_to_f32 + label_lut", unfused, timed), ("(d) PIL Compose.__call__ per sample (host)", host, wall)]
        for _ in range(a.warmup):
            for _, fn, _ in variants:
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _, _ in variants}
        for _ in range(a.reps):
            for name, fn, clock in variants:
                ms[name].append(clock(fn))
        for name, _, clock in variants:
            lines.append("    " + row(name, ms[name], nbytes if clock is timed else None))
        med = {n: statistics.median(v) for n, v in ms.items()}
        lines.append("    (a) / (c) = %.2f    (b) / (c) = %.2f    (d) / (b) = %.0fx" % (
            med["(a) fused, identity maps"] / med["(c) image_u8_to_f32 + label_lut"],
            med["(b) fused, drawn maps"] / med["(c) image_u8_to_f32 + label_lut"],
            med["(d) PIL Compose.__call__ per sample (host)"] / med["(b) fused, drawn maps"]))
        # ---- the colour table, at the same maps
        ccomp = du.augmentations.from_spec(a.colour, (H, W))
        table = torch.from_numpy(ccomp.colours(np.random.RandomState(511), B, 3)[0]).to(dev)
        eye = torch.tensor([1, 0, 0, 0, 1, 0, 0, 0, 1] + [0] * 12, dtype=torch.float32).repeat(B, 1).to(dev)
        colour = lambda t, m: F.augment_batch(d_img, d_gt, drawn, (H, W), mean, std, lut, label_fill=comp.label_fill, colour=t, need_mean=m)
        (i0, g0) = fused(drawn)
        same = all(torch.equal(i0, i) and torch.equal(g0, g) for i, g in (colour(eye, False), colour(eye, True)))
        lines += ["    colour table %s; the identity table bit-identical to (e): %s" % (a.colour, same)]
        if not same:
            sys.exit("\n".join(lines + ["the colour launch with the identity table does not reproduce the plain launch: nothing timed"]))
        variants = [("(e) fused, drawn maps, plain entry", lambda: fused(drawn)), ("(f) colour table, no mean", lambda: colour(table, False)),
                    ("(g) colour table + mean (clear, sum pass)", lambda: colour(table, True))]
        for _ in range(a.warmup):
            for _, fn in variants:
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in variants}
        for _ in range(a.reps):
            for name, fn in variants:
                ms[name].append(timed(fn))
        for name, _ in variants:
            lines.append("    " + row(name, ms[name], nbytes))
        med = {n: statistics.median(v) for n, v in ms.items()}
        lines.append("    (f) / (e) = %.2f    (g) / (e) = %.2f" % (med["(f) colour table, no mean"] / med["(e) fused, drawn maps, plain entry"],
                                                               med["(g) colour table + mean (clear, sum pass)"] / med["(e) fused, drawn maps, plain entry"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
