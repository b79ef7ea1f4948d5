#!/usr/bin/env python
"""Sliding-window inference: the fused head of all windows against the chain of separate passes, timed with HIP events on the MI355X.
  (a) the head alone on synthetic logit maps of every window of a batch:
      per window upsample -> softmax -> (flip) -> mul -> add_, then argmax_index -> confusion_hist (-> mul)   vs   one
      sscg_predict_head_sw launch; the chain is the kernels that existed before plus torch ops, a baseline independent of the new kernel
  (b) the gather alone: torch slicing + stack against one sscg_window_gather launch
  (c) one evaluate() pass with set_sliding(...) over a synthetic loader of --batches batches, SSCG_FUSE_SLIDING=0's path vs the default, and
      beside them the whole-image evaluate() of a model whose crop IS the evaluation size (one forward per batch on the full image)
Same process, warm-up first, the variants interleaved repetition by repetition, medians reported.  The outputs of both variants are
compared bit for bit before anything is timed.
usage: python tools/sliding_bench.py [--reps 30] [--warmup 3] [--batches 4] [--configs cityscapes,voc] [--out FILE]"""
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

# dataset, classes, batch, window (the crop), evaluation size, the windows' logit map size (DeepLab's stride-8 map of the crop)
CONFIGS = {"cityscapes": ("cityscapes", 20, 2, (256, 512), (512, 1024), (33, 65)),
           "voc": ("voc2012", 21, 2, (256, 256), (512, 512), (33, 33))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--configs", default="cityscapes,voc")
    ap.add_argument("--overlap", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sliding_bench.py measures on the MI355X: no GPU here, nothing is reported")
    F = importlib.import_module(PKG + ".functional")
    md = importlib.import_module(PKG + ".model")
    from oracle import fixtures as FX
    dev = torch.device("cuda", 0)
    lines = ["device: %s; %d repetitions after %d warm-up rounds, variants interleaved, HIP events" % (
        torch.cuda.get_device_name(0), a.reps, a.warmup)]

    def with_switch(flag, fn):
        def run():
            was = F.FUSE_SLIDING[0]
            F.FUSE_SLIDING[0] = flag
            try:
                with torch.no_grad():
                    return fn()
            finally:
                F.FUSE_SLIDING[0] = was
        return run

    for key in a.configs.split(","):
        dataset, C, B, win, size, (h, w) = CONFIGS[key]
        g = torch.Generator().manual_seed(5)
        lab = torch.randint(0, C, (B,) + size, generator=g).to(dev)
        lines.append("")
        for flip in (False, True):
            opts = F.SlidingOptions(win, size, overlap=a.overlap, flip=flip)
            plan = F.sliding_plan(size[0], size[1], opts, dev)
            lines.append("== %s: B = %d, %d classes, %d x %d windows of %dx%d%s (logits %dx%d) -> %d x %d, overlap %g" % (
                dataset, B, C, plan.ky, plan.kx, win[0], win[1], ", each mirrored" if flip else "", h, w, size[0], size[1], a.overlap))
            x = F.to_nhwc((torch.randn(B * plan.views, C, h, w, generator=g) * 4).to(dev))
            both = lambda: F.predict_labels_sw(x, plan, want_u8=False, want_index=True, label_true=lab)
            full = lambda: F.predict_labels_sw(x, plan, want_prob=True, want_index=True, label_true=lab)
            u8 = lambda: F.predict_labels_sw(x, plan)[0]
            sep, fus = with_switch(False, full)(), with_switch(True, full)()
            same = torch.equal(sep[1], fus[1]) and torch.equal(sep[2], fus[2]) and torch.equal(sep[3], fus[3]) \
                and torch.equal(with_switch(True, u8)(), sep[1].to(torch.uint8))
            lines.append("(a) %d windows per sample; outputs bit-identical: %s; classes predicted: %d of %d" % (
                plan.views, same, int(sep[1].unique().numel()), C))
            if not same:
                sys.exit("\n".join(lines + ["the fused head does not reproduce the chain: nothing timed"]))
            ms = interleaved([("separate: index + matrix", with_switch(False, both)), ("fused: index + matrix", with_switch(True, both)),
                              ("separate: + probabilities", with_switch(False, full)), ("fused: + probabilities", with_switch(True, full)),
                              ("fused: uint8 map only", with_switch(True, u8))], a.reps, a.warmup)
            for name in ms:
                lines.append("    " + row(name, ms[name]))
            med = {k: statistics.median(v) for k, v in ms.items()}
            lines.append("    speed-up over the separate passes: %.1fx (index + matrix), %.1fx (+ probabilities)" % (
                med["separate: index + matrix"] / med["fused: index + matrix"], med["separate: + probabilities"] / med["fused: + probabilities"]))
            img = torch.randn(B, 3, *size, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
            gather = lambda: F.window_gather(img, plan)
            same = torch.equal(with_switch(False, gather)(), with_switch(True, gather)())
            lines.append("(b) window_gather of %d x 3 x %d x %d; outputs bit-identical: %s" % (B, size[0], size[1], same))
            ms = interleaved([("separate: slicing + stack", with_switch(False, gather)), ("fused: one launch", with_switch(True, gather))],
                             a.reps, a.warmup)
            for name in ms:
                lines.append("    " + row(name, ms[name]))
            del x, img
        if a.batches > 0:
            mk = lambda crop: FX.make_args(dataset=dataset, crop_height=crop[0], crop_width=crop[1], batch_size=B, gpu_ids=[0],
                                           checkpoint_dir="/tmp/sscg_sliding_bench", as_written=True, model="supervised_model")
            with contextlib.redirect_stdout(io.StringIO()):
                m, whole = md.supervised_model(mk(win)), md.supervised_model(mk(size))
            loader = [(torch.randn(B, 3, *size, generator=g).to(dev).contiguous(memory_format=torch.channels_last),
                       torch.randint(0, C, (B, 1) + size, generator=g).to(dev), ["s"] * B) for _ in range(a.batches)]
            opts = F.SlidingOptions(win, size, overlap=a.overlap)
            plan = F.sliding_plan(size[0], size[1], opts, dev)
            m.set_sliding(opts)
            ev = lambda flag: with_switch(flag, lambda: m.evaluate(loader)[0])
            plain = with_switch(True, lambda: whole.evaluate(loader)[0])
            same = ev(False)() == ev(True)()
            lines.append("(c) evaluate() with set_sliding() over %d batches (%d DeepLab forwards of %d windows per batch + gather + head + host mIoU); "
                         "equal mIoU: %s" % (a.batches, -(-B * plan.views // B), B, same))
            ms = interleaved([("SSCG_FUSE_SLIDING=0", ev(False)), ("default (fused)", ev(True)),
                              ("whole image, crop = %dx%d" % size, plain)], max(a.reps // 3, 5), 1)
            for name in ms:
                lines.append("    " + row(name, ms[name]))
            u, f, p = (statistics.median(ms[k]) for k in ms)
            lines.append("    fused / separate = %.4f (%+.2f %%); sliding (fused) / whole image = %.2f" % (f / u, 100.0 * (f - u) / u, f / p))
            del m, whole, loader
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
