#!/usr/bin/env python
"""The mix launch of the augmenting batch finish (sscg_augment_mix_u8) on one MI355X, at B x 3 x H x W uint8 with labels, for each of
three pipelines - affine only, + colour (a contrast item, so with the sum pass), + elastic:
  (a) the unmixed launch (sscg_augment_u8 / _colour_u8 / _elastic_u8)                                        HIP events
  (b) the mix launch with a drawn box per sample (cutmix at p = 1, classes = 0)                              HIP events
  (c) the mix launch with box and classes (cutmix and classmix at p = 1)                                     HIP events
  (d) the unfused composition of (c): (a), then the pasted mask from torch ops on the finished batch (the box from two aranges, the
      class rule as a shift of the partner's class map), then two torch.where                                HIP events
Same process, warm-up first, the variants interleaved repetition by repetition, medians with minimum and 90th percentile reported,
with the bytes a launch must move (source pixels and labels read once, outputs written) over the time beside them.  Before anything
is timed (c) is compared with (d) and an all-unmixed table with (a), bit for bit.
usage: python tools/augment_mix_bench.py [--reps 200] [--warmup 20] [--batch 8] [--size 256] [--out FILE]"""
import argparse
import importlib
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "semi-supervised-segmentation-cyclegan_amd"
PIPELINES = (("affine only", "rotate=10,scale=0.5:2"), ("+ colour", "rotate=10,scale=0.5:2,brightness=0.3,contrast=0.3"),
             ("+ elastic", "rotate=10,scale=0.5:2,elastic=12:32"))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def row(name, v, nbytes):
    v = sorted(v)
    med = statistics.median(v)
    return "%-52s median %9.4f ms   min %9.4f   p90 %9.4f   (n = %d)   %7.1f GB/s moved" % (
        name, med, v[0], v[int(0.9 * (len(v) - 1))], len(v), nbytes / med / 1e6)


def unfused(plain, table):
    """(d): the rule of sscg_augment_mix_u8 from torch ops on the finished batch of `plain()` (the class map is the finished label)."""
    partner = table[:, 0].long()
    x0, y0, x1, y1 = (table[:, k, None, None] for k in (1, 2, 3, 4))
    bits = (table[:, 6].long() << 32) | (table[:, 5].long() & 0xFFFFFFFF)

    def run():
        img, gt = plain()
        n, _, oh, ow = img.shape
        ys = torch.arange(oh, device=img.device)[None, :, None]
        xs = torch.arange(ow, device=img.device)[None, None, :]
        pasted = (xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)
        cls = gt[partner, 0]
        pasted = pasted | (((cls >= 0) & (cls < 64)) & (((bits[:, None, None] >> cls.clamp(0, 63)) & 1) != 0))
        pasted = pasted[:, None]
        return torch.where(pasted, img[partner], img), torch.where(pasted, gt[partner], gt)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("augment_mix_bench.py measures on the MI355X: no GPU here, nothing is reported")
    F = importlib.import_module(PKG + ".functional")
    du = importlib.import_module(PKG + ".data_utils")
    dev = torch.device("cuda", 0)
    B, H, W = a.batch, a.size, a.size
    rng = np.random.RandomState(7)
    d_img = torch.from_numpy(rng.randint(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
    d_gt = torch.from_numpy(rng.randint(0, 21, (B, H, W)).astype(np.uint8)).to(dev)
    lut = du.label_table("voc2012").to(dev)
    mean, std = torch.full((3,), .5, device=dev), torch.full((3,), .5, device=dev)
    moved = B * H * W * (3 + 1) + B * H * W * (3 * 4 + 8)
    lines = ["device: %s; %d repetitions after %d warm-up rounds, variants interleaved, HIP events around the call (the outputs' allocation "
             "included)" % (torch.cuda.get_device_name(0), a.reps, a.warmup),
             "B = %d, %d x %d x 3 uint8 + labels -> fp32 + int64; bytes a launch must move: %.2f MB (%.2f MB read once, %.2f MB written); "
             "tables drawn by Compose.mixes with cutmix=1 (b) and cutmix=1,classmix=1:0 (c, d)" % (
                 B, H, W, moved / 1e6, B * H * W * 4 / 1e6, B * H * W * 20 / 1e6)]
    for title, spec in PIPELINES:
        comp = du.augmentations.from_spec(spec + ",cutmix=1,classmix=1:0", (H, W), label_fill=255, out_size=(H, W))
        drawn = comp.matrices(np.random.RandomState(11), B, W, H)
        kw = {}
        if comp.colour_ops:
            table, need_mean = comp.colours(np.random.RandomState(13), B, 3)
            kw.update(colour=torch.from_numpy(table).to(dev), need_mean=need_mean)
        if comp.elastic_ops:
            lattice, grid = comp.fields(np.random.RandomState(12), B, W, H, drawn)
            kw.update(elastic=(torch.from_numpy(lattice).to(dev), grid))
        mats = torch.from_numpy(drawn).to(dev)
        both, _ = comp.mixes(np.random.RandomState(14), B, W, H)
        box = both.copy()
        box[:, 5:7] = 0
        off = both.copy()
        off[:, 0] = np.arange(B)
        t_both, t_box, t_off = (torch.from_numpy(t).to(dev) for t in (both, box, off))
        call = lambda mix=None: F.augment_batch(d_img, d_gt, mats, (H, W), mean, std, lut, label_fill=255, mix=mix, **kw)
        variants = [("(a) unmixed launch", call), ("(b) mix launch, box", lambda: call((t_box, 0))),
                    ("(c) mix launch, box and classes", lambda: call((t_both, 1))),
                    ("(d) (a) + mask from torch ops + 2 x torch.where", unfused(call, t_both))]
        (i0, g0), (i1, g1), (i2, g2), (i3, g3) = call(), call((t_off, 1)), variants[2][1](), variants[3][1]()
        same = torch.equal(i0, i1) and torch.equal(g0, g1)
        agree = torch.equal(i2, i3) and torch.equal(g2, g3)
        share = float((g2 != g0).float().mean())
        lines += ["", "%s: --augment %s" % (title, spec),
                  "an all-unmixed table bit-identical to (a): %s; (c) bit-identical to (d): %s; labels changed by (c): %.1f %% of the pixels" % (
                      same, agree, 100 * share)]
        if not (same and agree):
            sys.exit("\n".join(lines + ["the launches do not agree: nothing timed"]))
        for _ in range(a.warmup):
            for _, fn in variants:
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in variants}
        for _ in range(a.reps):
            for name, fn in variants:
                ms[name].append(timed(fn))
        for name, _ in variants:
            lines.append("    " + row(name, ms[name], moved))
        med = [statistics.median(ms[name]) for name, _ in variants]
        lines.append("    (b) / (a) = %.2f    (c) / (a) = %.2f    (d) / (c) = %.2f" % (med[1] / med[0], med[2] / med[0], med[3] / med[2]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
