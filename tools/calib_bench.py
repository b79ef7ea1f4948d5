#!/usr/bin/env python
"""Calibration counts of the evaluation (`--calibration`, sscg_calib_stats) timed with HIP events on the MI355X.
  (a) one call at the evaluation's own size - logits 8 x 21 x 33 x 33 resized to 256 x 256, 15 bins - at one temperature and at eight,
      against the same maths from torch ops on the separate passes' probability map (resize, multiply, softmax, then max / bucketize /
      bincount / gather / log / squares per temperature), and against the label head (sscg_predict_head) as a yardstick;
  (b) one evaluate() pass over a synthetic loader of --batches batches with the option off, on, and on with the temperature grid.
Same process, warm-up first, the variants interleaved repetition by repetition, medians reported.  Nothing is promised or gated: the
cost of the option is whatever this prints.
usage: python tools/calib_bench.py [--reps 30] [--warmup 3] [--batches 16] [--out FILE]"""
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

N, C, H, W, OH, OW, BINS = 8, 21, 33, 33, 256, 256, 15


def torch_counts(F, logits, size, lt, inv_temps, bins):
    """The same counts from torch ops on the probability map of the separate passes: what the fused entry replaces."""
    z = F.upsample_bilinear(logits, size)
    keep = (lt >= 0) & (lt < C)
    lab = lt.clamp(0, C - 1)
    out = []
    for it in inv_temps:
        p = F.softmax2d(z * it)                                       # [N, C, OH, OW], channels last
        conf, pred = p.max(1)
        hit = (pred == lt) & keep
        b = (conf * float(bins)).to(torch.int64).clamp_(max=bins - 1)
        q = (conf * 16777216.0).to(torch.int64)
        tab = []
        for key, size_ in ((b, bins), (pred, C)):
            k = key[keep]
            tab.append(torch.stack([torch.bincount(k, minlength=size_), torch.bincount(key[hit], minlength=size_),
                                    torch.zeros(size_, dtype=torch.int64, device=k.device).index_add_(0, k, q[keep])], 1))
        py = p.gather(1, lab.unsqueeze(1)).squeeze(1).double().clamp_min(2.0 ** -126)
        nll = -(py.log() * keep).sum()
        p64 = p.double()
        brier = (((p64 * p64).sum(1) - 2.0 * p64.gather(1, lab.unsqueeze(1)).squeeze(1) + 1.0) * keep).sum()
        out.append((tab[0], tab[1], nll, brier))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("calib_bench.py measures on the MI355X: no GPU here, nothing is reported")
    F = importlib.import_module(PKG + ".functional")
    L = importlib.import_module(PKG + "._lib")
    U = importlib.import_module(PKG + ".utils")
    md = importlib.import_module(PKG + ".model")
    from oracle import fixtures as FX
    dev = torch.device("cuda", 0)
    one, grid = U.parse_calibration("on"), U.parse_calibration("fit")
    g = torch.Generator().manual_seed(5)
    logits = (torch.randn(N, C, H, W, generator=g) * 3).to(dev).contiguous(memory_format=torch.channels_last)
    gt = torch.randint(0, C, (N, OH, OW), generator=g)
    gt[:, 0, :] = gt[:, -1, :] = gt[:, :, 0] = gt[:, :, -1] = 255
    gt = gt.to(dev)
    lines = ["device: %s; %d repetitions after %d warm-up rounds, variants interleaved, HIP events" % (
        torch.cuda.get_device_name(0), a.reps, a.warmup),
        "logits %d x %d x %d x %d -> %d x %d, %d bins; workspace %d B at one temperature, %d B at eight; two launches per call" % (
            N, C, H, W, OH, OW, BINS, L.lib.sscg_calib_workspace(N, OH, OW, 1), L.lib.sscg_calib_workspace(N, OH, OW, 8)), ""]
    with torch.no_grad():
        s1 = F.calibration_stats(logits, (OH, OW), gt, one)
        s8 = F.calibration_stats(logits, (OH, OW), gt, grid)
        ref = torch_counts(F, logits, (OH, OW), gt, grid.inv_temps, BINS)
        assert all(torch.equal(s8[0][t], r[0]) and torch.equal(s8[1][t], r[1]) for t, r in enumerate(ref)), "the torch chain counts differently"
        hist = F.predict_labels(logits, (OH, OW), want_u8=False, label_true=gt)[2]
        names = ["calibration_stats, NT = 1", "torch ops on the map, NT = 1", "calibration_stats, NT = 8", "torch ops on the map, NT = 8",
                 "predict_labels (label head + hist)"]
        ms = interleaved([(names[0], lambda: F.calibration_stats(logits, (OH, OW), gt, one, state=s1)),
                          (names[1], lambda: torch_counts(F, logits, (OH, OW), gt, one.inv_temps, BINS)),
                          (names[2], lambda: F.calibration_stats(logits, (OH, OW), gt, grid, state=s8)),
                          (names[3], lambda: torch_counts(F, logits, (OH, OW), gt, grid.inv_temps, BINS)),
                          (names[4], lambda: F.predict_labels(logits, (OH, OW), want_u8=False, label_true=gt, hist=hist))], a.reps, a.warmup)
    lines.append("(a) one call")
    for name in names:
        lines.append("    " + row(name, ms[name]))
    med = {k: statistics.median(v) for k, v in ms.items()}
    lines.append("    torch ops / fused entry: %.1fx at NT = 1, %.1fx at NT = 8" % (med[names[1]] / med[names[0]], med[names[3]] / med[names[2]]))
    if a.batches > 0:
        args = FX.make_args(dataset="voc2012", crop_height=OH, crop_width=OW, batch_size=N, gpu_ids=[0], checkpoint_dir="/tmp/sscg_calib_bench",
                            as_written=True)
        with contextlib.redirect_stdout(io.StringIO()):
            m = md.supervised_model(args)
        loader = [(torch.randn(N, 3, OH, OW, generator=g).to(dev).contiguous(memory_format=torch.channels_last), gt.unsqueeze(1), ["s"] * N)
                  for _ in range(a.batches)]

        def ev(o):
            def run():
                m.set_calibration(o)
                return m.evaluate(loader)[0]
            return run

        lines.append("(b) evaluate() over %d batches of %d x 3 x %d x %d (one DeepLab forward per batch + head + host scores)" % (a.batches, N, OH, OW))
        tags = ["evaluate()", "evaluate(), calibration on", "evaluate(), calibration fit (8 T)"]
        ms = interleaved([(tags[0], ev(None)), (tags[1], ev(one)), (tags[2], ev(grid))], max(a.reps // 3, 5), 1)
        for name in tags:
            lines.append("    " + row(name, ms[name]))
        u = statistics.median(ms[tags[0]])
        for name in tags[1:]:
            f = statistics.median(ms[name])
            lines.append("    %s / without = %.4f (%+.2f %%, %+.3f ms per batch)" % (name, f / u, 100.0 * (f - u) / u, (f - u) / a.batches))
        m.set_calibration(None)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
