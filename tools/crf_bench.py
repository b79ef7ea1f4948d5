#!/usr/bin/env python
"""Windowed dense-CRF refinement (`--crf`, sscg_crf_head) timed with HIP events on the MI355X.
  (a) the head alone on synthetic logits and a synthetic guide image at the VOC (B = 8, 21 x 256 x 256) and Cityscapes (B = 16,
      20 x 256 x 512) evaluation sizes: the plain fused head (F.predict_labels), the CRF with 1 and with 1 + K iterations - their
      difference over K is the time of ONE mean-field step (one crf_iter_kernel launch) - and the default 5 iterations.  Beside the
      step's time: the bytes it has to move at least (u read, Q read, Q written, the guide image read, once each) and that over the HBM
      peak, so the distance to the bandwidth bound is visible;
  (b) one evaluate() pass over a synthetic loader of --batches batches without and with the CRF.
Same process, warm-up first, the variants interleaved repetition by repetition, medians reported.
usage: python tools/crf_bench.py [--reps 30] [--warmup 3] [--batches 8] [--configs voc,cityscapes] [--crf on] [--out FILE]"""
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

# dataset, classes, batch, output size, DeepLab's stride-8 logit map
CONFIGS = {"voc": ("voc2012", 21, 8, (256, 256), (33, 33)), "cityscapes": ("cityscapes", 20, 16, (256, 512), (33, 65))}
HBM_PEAK = 8.0e12          # bytes / s, the MI355X's specified peak
EXTRA = 5                  # iterations between the two timed variants of (a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--configs", default="voc,cityscapes")
    ap.add_argument("--crf", default="on")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("crf_bench.py measures on the MI355X: no GPU here, nothing is reported")
    F = importlib.import_module(PKG + ".functional")
    md = importlib.import_module(PKG + ".model")
    utils = importlib.import_module(PKG + ".utils")
    from oracle import fixtures as FX
    dev = torch.device("cuda", 0)
    crf = utils.parse_crf(a.crf)
    kw = {k: getattr(crf, k) for k in crf.__slots__ if k != "iterations"}
    lines = ["device: %s; %d repetitions after %d warm-up rounds, variants interleaved, HIP events" % (
        torch.cuda.get_device_name(0), a.reps, a.warmup), "crf: %r" % (crf,)]
    for key in a.configs.split(","):
        dataset, C, B, (H, W), (h, w) = CONFIGS[key]
        g = torch.Generator().manual_seed(5)
        logits = F.to_nhwc((torch.randn(B, C, h, w, generator=g) * 2).to(dev))
        image = torch.randn(B, 3, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        lab = torch.randint(0, C, (B, H, W), generator=g).to(dev)
        lines.append("")
        lines.append("== %s: B = %d, %d classes, logits %dx%d -> %d x %d, radius %d, dilation %d" % (dataset, B, C, h, w, H, W, crf.radius,
                                                                                                  crf.dilation))
        with torch.no_grad():
            plain = lambda: F.predict_labels(logits, (H, W), want_u8=False, label_true=lab)[2]
            run = lambda it: (lambda: F.crf_labels(logits, image, (H, W), F.CrfOptions(iterations=it, **kw), want_u8=False, label_true=lab)[2])
            moved = float((F.crf_labels(logits, image, (H, W), crf, want_index=True)[1] != F.predict_labels(logits, (H, W), want_index=True)[1])
                          .float().mean())
            same = torch.equal(run(0)(), plain())
            lines.append("(a) confusion matrix of 0 iterations equals the plain head's: %s; labels moved by %d iterations: %.1f %%" % (
                same, crf.iterations, 100 * moved))
            if not same:
                sys.exit("\n".join(lines + ["0 iterations do not reproduce the plain head: nothing timed"]))
            names = ["plain head (predict_labels)", "crf, 1 iteration", "crf, %d iterations" % (1 + EXTRA), "crf, %d iterations" % crf.iterations]
            ms = interleaved([(names[0], plain), (names[1], run(1)), (names[2], run(1 + EXTRA)), (names[3], run(crf.iterations))], a.reps, a.warmup)
        for name in dict.fromkeys(names):
            lines.append("    " + row(name, ms[name]))
        step = (statistics.median(ms[names[2]]) - statistics.median(ms[names[1]])) / EXTRA
        must = B * H * W * (3 * C + 3) * 4
        lines.append("    one mean-field step: %.3f ms; it must move %.1f MB (u, Q read, Q written, image), %.3f ms at the %.1f TB/s HBM peak: "
                     "%.1fx the bandwidth bound" % (step, must / 1e6, 1e3 * must / HBM_PEAK, HBM_PEAK / 1e12, step / (1e3 * must / HBM_PEAK)))
        lines.append("    workspace: %.1f MB (u and two Q buffers)" % (F.lib.sscg_crf_workspace(B, C, H, W, crf.iterations) / 1e6))
        if a.batches > 0:
            args = FX.make_args(dataset=dataset, crop_height=H, crop_width=W, batch_size=B, gpu_ids=[0], checkpoint_dir="/tmp/sscg_crf_bench",
                                as_written=True)
            with contextlib.redirect_stdout(io.StringIO()):
                m = md.supervised_model(args)
            loader = [(torch.randn(B, 3, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last),
                       torch.randint(0, C, (B, 1, H, W), generator=g).to(dev), ["s"] * B) for _ in range(a.batches)]
            ev = lambda opt: (lambda: m.evaluate(loader, crf=opt)[0])
            lines.append("(b) evaluate() over %d batches (one DeepLab forward per batch + head + host mIoU)" % a.batches)
            ms = interleaved([("evaluate()", ev(None)), ("evaluate(crf=%s)" % a.crf, ev(crf))], max(a.reps // 3, 5), 1)
            for name in ms:
                lines.append("    " + row(name, ms[name]))
            u, f = statistics.median(ms["evaluate()"]), statistics.median(ms["evaluate(crf=%s)" % a.crf])
            lines.append("    with / without = %.4f (%+.2f %%, %+.3f ms per batch)" % (f / u, 100.0 * (f - u) / u, (f - u) / a.batches))
            del m, loader
        del logits, image, lab
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
