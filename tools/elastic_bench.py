#!/usr/bin/env python
"""The elastic launch of the augmenting batch finish (sscg_augment_elastic_u8) on one MI355X, at B x 3 x H x W uint8 with labels:
  (a) the elastic launch, drawn maps and a drawn lattice                          HIP events
  (b) the affine launch (sscg_augment_u8) on the same inputs and maps              HIP events
  (c) the same maths from torch ops: the lattice upsampled to a displacement per pixel (bicubic interpolate), added to the affine
      sampling grid, grid_sample bilinear for the image and nearest for the labels, then the normalisation and the label table
                                                                                  HIP events
Same process, warm-up first, the variants interleaved repetition by repetition, medians reported, with the bytes moved (source
pixels and labels read once, nodes, maps, outputs written) over kernel time beside them.  Before anything is timed the elastic launch
with an all-zero lattice is compared with (b) bit for bit.  (c) is a timing yardstick, not a reference: its arithmetic is float.
usage: python tools/elastic_bench.py [--reps 50] [--warmup 5] [--batch 8] [--size 256] [--grid 32] [--alpha 12]
                                     [--spec rotate=10,scale=0.5:2] [--out FILE]"""
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
    return "%-44s median %9.4f ms   min %9.4f   p90 %9.4f   (n = %d)   %7.1f GB/s moved" % (
        name, med, v[0], v[int(0.9 * (len(v) - 1))], len(v), nbytes / med / 1e6)


def torch_path(d_img, d_gt, mats, nodes, grid, mean, std, lut):
    """(c): float coordinates from the same Q16 numbers, torch ops only."""
    import torch.nn.functional as TF
    B, H, W, _ = d_img.shape
    dev = d_img.device
    m = mats.to(torch.float32) / 65536.0
    oy, ox = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")

    def run():
        # the lattice covers cells -1 .. (size - 1) / grid + 2: upsample it and cut the output's window out of it
        disp = TF.interpolate(nodes.permute(0, 3, 1, 2).to(torch.float32) / 65536.0, scale_factor=grid, mode="bicubic", align_corners=False)
        disp = disp[:, :, grid + grid // 2:grid + grid // 2 + H, grid + grid // 2:grid + grid // 2 + W]
        sx = m[:, 0, None, None] * ox + m[:, 1, None, None] * oy + m[:, 2, None, None] + disp[:, 0]
        sy = m[:, 3, None, None] * ox + m[:, 4, None, None] * oy + m[:, 5, None, None] + disp[:, 1]
        g = torch.stack([(2 * sx + 1) / W - 1, (2 * sy + 1) / H - 1], dim=-1)
        x = d_img.permute(0, 3, 1, 2).to(torch.float32) / 255
        img = TF.grid_sample(x, g, mode="bilinear", padding_mode="zeros", align_corners=False)
        lab = TF.grid_sample(d_gt[:, None].to(torch.float32), g, mode="nearest", padding_mode="zeros", align_corners=False)
        return (img - mean[None, :, None, None]) / std[None, :, None, None], lut[lab.to(torch.int64)]
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--alpha", type=float, default=12.0)
    ap.add_argument("--spec", default="rotate=10,scale=0.5:2")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("elastic_bench.py measures on the MI355X: no GPU here, nothing is reported")
    F = importlib.import_module(PKG + ".functional")
    du = importlib.import_module(PKG + ".data_utils")
    dev = torch.device("cuda", 0)
    B, H, W = a.batch, a.size, a.size
    rng = np.random.RandomState(7)
    img = rng.randint(0, 256, (B, H, W, 3), dtype=np.uint8)
    gt = rng.randint(0, 21, (B, H, W)).astype(np.uint8)
    spec = "%s,elastic=%g:%d" % (a.spec, a.alpha, a.grid)
    comp = du.augmentations.from_spec(spec, (H, W), label_fill=255, out_size=(H, W))
    drawn = comp.matrices(np.random.RandomState(11), B, W, H)
    lattice, grid = comp.fields(np.random.RandomState(12), B, W, H, drawn)
    mats, nodes = torch.from_numpy(drawn).to(dev), torch.from_numpy(lattice).to(dev)
    zero = torch.zeros_like(nodes)
    d_img, d_gt = torch.from_numpy(img).to(dev), torch.from_numpy(gt).to(dev)
    lut = du.label_table("voc2012").to(dev)
    mean, std = torch.full((3,), .5, device=dev), torch.full((3,), .5, device=dev)
    moved = B * H * W * (3 + 1) + B * H * W * (3 * 4 + 8) + mats.numel() * 4
    affine = lambda: F.augment_batch(d_img, d_gt, mats, (H, W), mean, std, lut, label_fill=255)
    elastic = lambda n: F.augment_batch(d_img, d_gt, mats, (H, W), mean, std, lut, label_fill=255, elastic=(n, grid))
    (i0, g0), (i1, g1) = affine(), elastic(zero)
    same = torch.equal(i0, i1) and torch.equal(g0, g1)
    lines = ["device: %s; %d repetitions after %d warm-up rounds, variants interleaved, HIP events" % (torch.cuda.get_device_name(0), a.reps, a.warmup),
             "B = %d, %d x %d x 3 uint8 + labels -> fp32 + int64; --augment %s; lattice %s int32 (%d bytes)" % (
                 B, H, W, spec, tuple(nodes.shape), nodes.numel() * 4),
             "bytes moved per launch: %.2f MB (%.2f MB read once, %.2f MB written), the lattice on top for (a) and (c)" % (
                 moved / 1e6, B * H * W * 4 / 1e6, B * H * W * 20 / 1e6),
             "the elastic launch with an all-zero lattice bit-identical to the affine launch: %s" % same]
    if not same:
        sys.exit("\n".join(lines + ["the zero lattice does not reproduce the affine launch: nothing timed"]))
    variants = [("(a) elastic launch", lambda: elastic(nodes), moved + nodes.numel() * 4), ("(b) affine launch", affine, moved),
                ("(c) torch: interpolate + grid_sample x 2", torch_path(d_img, d_gt, mats, nodes, grid, mean, std, lut), moved + nodes.numel() * 4)]
    for _ in range(a.warmup):
        for _, fn, _ in variants:
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in variants}
    for _ in range(a.reps):
        for name, fn, _ in variants:
            ms[name].append(timed(fn))
    for name, _, nbytes in variants:
        lines.append("    " + row(name, ms[name], nbytes))
    med = {n: statistics.median(v) for n, v in ms.items()}
    lines.append("    (a) / (b) = %.2f    (c) / (a) = %.1f" % (med["(a) elastic launch"] / med["(b) affine launch"],
                                                              med["(c) torch: interpolate + grid_sample x 2"] / med["(a) elastic launch"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
