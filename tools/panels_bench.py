#!/usr/bin/env python
"""The per-epoch image panels, timed with HIP events on the MI355X.
  (a) semisuper_cycleGAN.panels() on one validation batch: the default (sscg_panel_labels / _range / _grid on the device) against
      SSCG_FUSE_PANELS=0 (predict_labels -> label_onehot -> host: colorize_mask, PIL_to_tensor, make_grid, grid_to_u8), with the
      host's wall clock beside the device time of each, and the bytes each path copies to the host;
  (b) the three new launches on their own, on the maps of that batch.
Same process, warm-up first, the variants interleaved repetition by repetition, medians with the p90 - min spread.  The five arrays
of both paths are compared byte for byte before anything is timed.
usage: python tools/panels_bench.py [--reps 30] [--warmup 3] [--configs voc,cityscapes] [--out FILE]"""
import argparse
import contextlib
import importlib
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "semi-supervised-segmentation-cyclegan_amd"
CONFIGS = {"voc": ("voc2012", 21, 8, 256, 256), "cityscapes": ("cityscapes", 20, 16, 256, 512)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def interleaved(variants, reps, warmup):
    """{name: ([event ms, ...], [host wall ms, ...])} with the variants run in turn inside every repetition"""
    for _ in range(warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    ms = {name: ([], []) for name, _ in variants}
    for _ in range(reps):
        for name, fn in variants:
            ev, wall = timed(fn)
            ms[name][0].append(ev)
            ms[name][1].append(wall)
    return ms


def row(name, v):
    v = sorted(v)
    p90 = v[int(0.9 * (len(v) - 1))]
    return "%-40s median %9.3f ms   min %9.3f   p90 %9.3f   spread (p90 - min) %7.3f   (n = %d)" % (
        name, statistics.median(v), v[0], p90, p90 - v[0], len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="voc,cityscapes")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("panels_bench.py measures on the MI355X: no GPU here, nothing is reported")
    F = importlib.import_module(PKG + ".functional")
    md = importlib.import_module(PKG + ".model")
    utils = importlib.import_module(PKG + ".utils")
    from oracle import fixtures as FX
    dev = torch.device("cuda", 0)
    lines = ["device: %s; %d repetitions after %d warm-up rounds, variants interleaved, HIP events" % (
        torch.cuda.get_device_name(0), a.reps, a.warmup)]
    for key in a.configs.split(","):
        dataset, C, B, H, W = CONFIGS[key]
        args = FX.make_args(dataset=dataset, crop_height=H, crop_width=W, batch_size=B, gpu_ids=[0], checkpoint_dir="/tmp/sscg_panels_bench",
                            as_written=True)
        with contextlib.redirect_stdout(io.StringIO()):
            m = md.semisuper_cycleGAN(args)
        g = torch.Generator().manual_seed(5)
        img = torch.randn(B, 3, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        gt = torch.randint(0, C, (B, 1, H, W), generator=g).to(dev)
        lines.append("")
        lines.append("== %s: B = %d, %d x %d, %d classes" % (dataset, B, H, W, C))

        def panels(flag):
            def run():
                was = F.FUSE_PANELS[0]
                F.FUSE_PANELS[0] = flag
                try:
                    return m.panels(img, gt)
                finally:
                    F.FUSE_PANELS[0] = was
            return run

        fused, plain = panels(True)(), panels(False)()
        same = list(fused) == list(plain) and all(np.array_equal(fused[t], plain[t]) for t in fused)
        lines.append("(a) panels(): five grids of %s bytes; both paths byte-identical: %s" % ("x".join(map(str, fused[md.PANEL_TAGS[0]].shape)), same))
        if not same:
            sys.exit("\n".join(lines + ["the fused panels do not reproduce the separate passes: nothing timed"]))
        grid_bytes = sum(v.size for v in fused.values())
        # what the separate path copies to the host: three int64 label maps (two predictions, the ground truth), two fp32 images
        host_bytes = 3 * B * H * W * 8 + 2 * B * 3 * H * W * 4
        lines.append("    device -> host: %.2f MB (fused: the five grids) against %.2f MB (separate: 3 int64 maps + 2 fp32 images)" % (
            grid_bytes / 1e6, host_bytes / 1e6))
        ms = interleaved([("SSCG_FUSE_PANELS=0", panels(False)), ("default (fused)", panels(True))], a.reps, a.warmup)
        for name in ms:
            lines.append("    " + row(name + ", stream time", ms[name][0]))
            lines.append("    " + row(name + ", host wall clock", ms[name][1]))

        # the four generator forwards both paths share (eval mode, the chain of panels() without its tail)
        def forwards():
            with torch.no_grad():
                m.Gsi.eval()
                m.Gis.eval()
                x = m.Gsi(img)
                oh = utils.make_one_hot(gt, dataset)
                y = m.interp(m.Gis(oh))
                m.Gis(oh)
                m.Gsi(y)
                m.Gsi.train()
                m.Gis.train()
                return x
        fw = interleaved([("four generator forwards alone", forwards)], a.reps, a.warmup)["four generator forwards alone"]
        lines.append("    " + row("four generator forwards, stream time", fw[0]))
        lines.append("    " + row("four generator forwards, host wall", fw[1]))
        f_wall = statistics.median(fw[1])
        lines.append("    host time outside the forwards: separate %.3f ms, fused %.3f ms" % (
            statistics.median(ms["SSCG_FUSE_PANELS=0"][1]) - f_wall, statistics.median(ms["default (fused)"][1]) - f_wall))

        # (b) the launches on their own
        with torch.no_grad():
            m.Gsi.eval()
            logits = F.to_nhwc(m.Gsi(img).detach())
            m.Gsi.train()
            logits = F.to_nhwc(logits * (4.0 / float(logits.std())) + torch.randn(logits.shape, generator=g).to(dev))
            ids, onehot = F.panel_labels(logits, (H, W))
            image = torch.randn(B, 3, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
            pal = utils.palette_tensor(dataset, dev)
            rng_i = F.panel_range(image, F.PANEL_IMAGE, 0.5, 0.5)
            rng_c = F.panel_range(ids, F.PANEL_COLOUR, palette=pal)
            rng_g = F.panel_range(gt, F.PANEL_GREY)
        lines.append("(b) the launches alone; logits %s -> %d x %d" % ("x".join(map(str, logits.shape)), H, W))

        def ng(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run
        variants = [
            ("panel_labels: ids + one-hot", ng(lambda: F.panel_labels(logits, (H, W)))),
            ("panel_labels: ids only", ng(lambda: F.panel_labels(logits, (H, W), want_onehot=False))),
            ("predict_labels(index) + label_onehot", ng(lambda: F.label_onehot(F.predict_labels(logits, (H, W), want_index=True, want_u8=False)[1].unsqueeze(1), C))),
            ("panel_range: image", ng(lambda: F.panel_range(image, F.PANEL_IMAGE, 0.5, 0.5))),
            ("panel_range: colour", ng(lambda: F.panel_range(ids, F.PANEL_COLOUR, palette=pal))),
            ("panel_range: grey", ng(lambda: F.panel_range(gt, F.PANEL_GREY))),
            ("panel_grid: image", ng(lambda: F.panel_grid(image, F.PANEL_IMAGE, rng_i, 2, 2, 0.5, 0.5))),
            ("panel_grid: colour", ng(lambda: F.panel_grid(ids, F.PANEL_COLOUR, rng_c, 2, 2, palette=pal))),
            ("panel_grid: grey", ng(lambda: F.panel_grid(gt, F.PANEL_GREY, rng_g, 2, 2))),
        ]
        ms = interleaved(variants, a.reps, a.warmup)
        for name in ms:
            lines.append("    " + row(name, ms[name][0]))
        lab = statistics.median(ms["panel_labels: ids + one-hot"][0])
        lines.append("    one-hot store: %.1f MB in %.3f ms = %.0f GB/s" % (onehot.numel() * 4 / 1e6, lab, onehot.numel() * 4 / 1e6 / lab))
        del m
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
