#!/usr/bin/env python
"""The inference heads against the chain of separate passes they replace, timed with HIP events on the MI355X.
  (a) the label chain alone on recorded logits (one eval-mode DeepLab forward of the configuration's batch):
      upsample_bilinear -> softmax2d -> argmax_index -> confusion_hist   vs   one sscg_predict_head launch
  (b) one evaluate() pass over a synthetic loader of --batches batches, SSCG_FUSE_PREDICT=0's path vs the default.
Same process, warm-up first, the two variants interleaved repetition by repetition, medians reported.  The outputs of both variants are
compared bit for bit before anything is timed.
usage: python tools/predict_bench.py [--reps 30] [--warmup 3] [--batches 16] [--configs voc,cityscapes] [--out FILE]"""
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
PKG = "semi-supervised-segmentation-cyclegan_amd"
CONFIGS = {"voc": ("voc2012", 21, 8, 256, 256), "cityscapes": ("cityscapes", 20, 16, 256, 512)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def interleaved(variants, reps, warmup):
    """{name: [ms, ...]} with the variants run in turn inside every repetition"""
    for _ in range(warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in variants}
    for _ in range(reps):
        for name, fn in variants:
            ms[name].append(timed(fn)[0])
    return ms


def row(name, v):
    v = sorted(v)
    return "%-34s median %9.3f ms   min %9.3f   p90 %9.3f   (n = %d)" % (name, statistics.median(v), v[0], v[int(0.9 * (len(v) - 1))], len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--configs", default="voc,cityscapes")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("predict_bench.py measures on the MI355X: no GPU here, nothing is reported")
    F = importlib.import_module(PKG + ".functional")
    md = importlib.import_module(PKG + ".model")
    utils = importlib.import_module(PKG + ".utils")
    from oracle import fixtures as FX
    dev = torch.device("cuda", 0)
    lines = ["device: %s; %d repetitions after %d warm-up rounds, variants interleaved, HIP events" % (
        torch.cuda.get_device_name(0), a.reps, a.warmup)]
    for key in a.configs.split(","):
        dataset, C, B, H, W = CONFIGS[key]
        args = FX.make_args(dataset=dataset, crop_height=H, crop_width=W, batch_size=B, gpu_ids=[0], checkpoint_dir="/tmp/sscg_predict_bench",
                            as_written=True)
        with contextlib.redirect_stdout(io.StringIO()):
            m = md.supervised_model(args)
        g = torch.Generator().manual_seed(5)
        loader = [(torch.randn(B, 3, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last),
                   torch.randint(0, C, (B, 1, H, W), generator=g).to(dev), ["s"] * B) for _ in range(a.batches)]
        m.Gsi.eval()
        with torch.no_grad():
            logits = m.Gsi(loader[0][0]).detach()
            # logits of an untrained net are nearly flat: spread them so that every class wins somewhere, as a trained head's do
            logits = F.to_nhwc(logits * (4.0 / float(logits.std())) + torch.randn(logits.shape, generator=g).to(dev))
        m.Gsi.train()
        lab = loader[0][1].squeeze(1).contiguous()
        n, c, h, w = logits.shape
        lines.append("")
        lines.append("== %s: B = %d, logits %d x %d x %d -> %d x %d" % (dataset, B, c, h, w, H, W))

        def unfused():
            with torch.no_grad():
                idx = F.argmax_index(F.softmax2d(F.upsample_bilinear(logits, (H, W))))
                return idx, F.confusion_hist(lab, idx, C)

        def fused():
            with torch.no_grad():
                _, idx, hist = F.predict_labels(logits, (H, W), want_u8=False, want_index=True, label_true=lab)
                return idx, hist

        def fused_eval():          # what evaluate() launches: the counts alone
            with torch.no_grad():
                return F.predict_labels(logits, (H, W), want_u8=False, label_true=lab)[2]

        def fused_u8():            # what the drivers launch: the uint8 map alone
            with torch.no_grad():
                return F.predict_labels(logits, (H, W))[0]

        (i0, h0), (i1, h1) = unfused(), fused()
        same = torch.equal(i0, i1) and torch.equal(h0, h1) and torch.equal(fused_eval(), h0) and torch.equal(fused_u8(), i0.to(torch.uint8))
        lines.append("(a) label chain on recorded logits; outputs bit-identical: %s; classes predicted: %d of %d" % (
            same, int(i0.unique().numel()), C))
        if not same:
            sys.exit("\n".join(lines + ["the fused head does not reproduce the chain: nothing timed"]))
        ms = interleaved([("unfused: 4 passes + fill", unfused), ("fused: index + confusion matrix", fused),
                          ("fused: confusion matrix only", fused_eval), ("fused: uint8 map only", fused_u8)], a.reps, a.warmup)
        for name in ms:
            lines.append("    " + row(name, ms[name]))
        base = statistics.median(ms["unfused: 4 passes + fill"])
        lines.append("    speed-up over the unfused chain: %.1fx (index + matrix), %.1fx (matrix only), %.1fx (uint8 only)" % (
            base / statistics.median(ms["fused: index + confusion matrix"]), base / statistics.median(ms["fused: confusion matrix only"]),
            base / statistics.median(ms["fused: uint8 map only"])))

        def evaluate(flag):
            def run():
                was = F.FUSE_PREDICT[0]
                F.FUSE_PREDICT[0] = flag
                try:
                    return m.evaluate(loader)[0]
                finally:
                    F.FUSE_PREDICT[0] = was
            return run

        same = evaluate(False)() == evaluate(True)()
        lines.append("(b) evaluate() over %d batches (DeepLab forward + head + host mIoU); equal mIoU: %s" % (a.batches, same))
        ms = interleaved([("SSCG_FUSE_PREDICT=0", evaluate(False)), ("default (fused)", evaluate(True))], max(a.reps // 2, 10), 2)
        for name in ms:
            lines.append("    " + row(name, ms[name]))
        u, f = statistics.median(ms["SSCG_FUSE_PREDICT=0"]), statistics.median(ms["default (fused)"])
        lines.append("    fused / unfused = %.4f (%+.2f %%)" % (f / u, 100.0 * (f - u) / u))
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
