#!/usr/bin/env python
"""Multi-scale / mirrored inference: the fused head of all views against the chain of separate passes, timed with HIP events on the
MI355X.
  (a) the head alone on synthetic logit maps of 3 views (three scales) and 6 views (each with its mirrored twin):
      per view upsample -> flip -> softmax -> add, then argmax_index -> confusion_hist   vs   one sscg_predict_head_ms launch
  (b) one evaluate(tta=...) pass over a synthetic loader of --batches batches, SSCG_FUSE_TTA=0's path vs the default.
Same process, warm-up first, the two variants interleaved repetition by repetition, medians reported.  The outputs of both variants are
compared bit for bit before anything is timed.
usage: python tools/tta_bench.py [--reps 30] [--warmup 3] [--batches 16] [--configs voc,cityscapes] [--tta 0.5,0.75,1.0:flip] [--out FILE]"""
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

# dataset, classes, batch, output size, the views' logit map sizes (DeepLab's stride-8 maps of the 0.5 / 0.75 / 1.0 inputs)
CONFIGS = {"voc": ("voc2012", 21, 8, (256, 256), [(17, 17), (25, 25), (33, 33)]),
           "cityscapes": ("cityscapes", 20, 16, (256, 512), [(17, 33), (25, 49), (33, 65)])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--configs", default="voc,cityscapes")
    ap.add_argument("--tta", default="0.5,0.75,1.0:flip")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tta_bench.py measures on the MI355X: no GPU here, nothing is reported")
    F = importlib.import_module(PKG + ".functional")
    md = importlib.import_module(PKG + ".model")
    utils = importlib.import_module(PKG + ".utils")
    from oracle import fixtures as FX
    dev = torch.device("cuda", 0)
    lines = ["device: %s; %d repetitions after %d warm-up rounds, variants interleaved, HIP events" % (
        torch.cuda.get_device_name(0), a.reps, a.warmup)]

    def with_switch(flag, fn):
        def run():
            was = F.FUSE_TTA[0]
            F.FUSE_TTA[0] = flag
            try:
                with torch.no_grad():
                    return fn()
            finally:
                F.FUSE_TTA[0] = was
        return run

    for key in a.configs.split(","):
        dataset, C, B, (H, W), sizes = CONFIGS[key]
        g = torch.Generator().manual_seed(5)
        lab = torch.randint(0, C, (B, H, W), generator=g).to(dev)
        lines.append("")
        lines.append("== %s: B = %d, %d classes, logit maps %s -> %d x %d" % (dataset, B, C, " ".join("%dx%d" % s for s in sizes), H, W))
        for twins in (False, True):
            shapes = [s for s in sizes for _ in range(2 if twins else 1)]
            flips = [twins and i % 2 == 1 for i in range(len(shapes))]
            xs = [F.to_nhwc((torch.randn(B, C, h, w, generator=g) * 4).to(dev)) for h, w in shapes]
            both = lambda: F.predict_labels_ms(xs, flips, (H, W), want_u8=False, want_index=True, label_true=lab)
            counts = lambda: F.predict_labels_ms(xs, flips, (H, W), want_u8=False, label_true=lab)[2]
            u8 = lambda: F.predict_labels_ms(xs, flips, (H, W))[0]
            sep, fus = with_switch(False, both)(), with_switch(True, both)()
            same = torch.equal(sep[1], fus[1]) and torch.equal(sep[2], fus[2]) and torch.equal(with_switch(True, counts)(), sep[2]) \
                and torch.equal(with_switch(True, u8)(), sep[1].to(torch.uint8))
            lines.append("(a) %d views%s; outputs bit-identical: %s; classes predicted: %d of %d" % (
                len(xs), " (mirrored twins)" if twins else "", same, int(sep[1].unique().numel()), C))
            if not same:
                sys.exit("\n".join(lines + ["the fused head does not reproduce the chain: nothing timed"]))
            base_name = "separate: %d passes + fill" % (sum(3 + int(f) for f in flips) + 2)
            ms = interleaved([(base_name, with_switch(False, both)), ("fused: index + confusion matrix", with_switch(True, both)),
                              ("fused: confusion matrix only", with_switch(True, counts)), ("fused: uint8 map only", with_switch(True, u8))],
                             a.reps, a.warmup)
            for name in ms:
                lines.append("    " + row(name, ms[name]))
            base = statistics.median(ms[base_name])
            lines.append("    speed-up over the separate passes: %.1fx (index + matrix), %.1fx (matrix only), %.1fx (uint8 only)" % (
                base / statistics.median(ms["fused: index + confusion matrix"]), base / statistics.median(ms["fused: confusion matrix only"]),
                base / statistics.median(ms["fused: uint8 map only"])))
            del xs
        if a.batches > 0:
            args = FX.make_args(dataset=dataset, crop_height=H, crop_width=W, batch_size=B, gpu_ids=[0], checkpoint_dir="/tmp/sscg_tta_bench",
                                as_written=True)
            with contextlib.redirect_stdout(io.StringIO()):
                m = md.supervised_model(args)
            loader = [(torch.randn(B, 3, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last),
                       torch.randint(0, C, (B, 1, H, W), generator=g).to(dev), ["s"] * B) for _ in range(a.batches)]
            views = utils.parse_tta(a.tta)
            ev = lambda flag: with_switch(flag, lambda: m.evaluate(loader, tta=views)[0])
            same = ev(False)() == ev(True)()
            lines.append("(b) evaluate(tta=%r) over %d batches (%d DeepLab forwards per batch + head + host mIoU); equal mIoU: %s" % (
                a.tta, a.batches, len(views), same))
            ms = interleaved([("SSCG_FUSE_TTA=0", ev(False)), ("default (fused)", ev(True))], max(a.reps // 3, 5), 1)
            for name in ms:
                lines.append("    " + row(name, ms[name]))
            u, f = statistics.median(ms["SSCG_FUSE_TTA=0"]), statistics.median(ms["default (fused)"])
            lines.append("    fused / separate = %.4f (%+.2f %%)" % (f / u, 100.0 * (f - u) / u))
            del m, loader
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
