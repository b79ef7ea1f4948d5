#!/usr/bin/env python
"""The optimiser options of the flat-arena Adam against the plain launch, timed with HIP events on the MI355X at the generators'
arena size (--n, default 85.7 M floats), in both shadow modes (three split planes / one bf16 arena):
  sscg_adam_step               vs  sscg_adam_step_ex with a clip coefficient, with L2 decay, with decoupled decay, with an EMA, with all
  sscg_grad_norm alone, with the bandwidth it reaches on its one read of the gradient arena
Each figure is the time of --burst back-to-back launches of one entry divided by --burst; the variants are interleaved repetition by
repetition and medians are reported.  The byte counts are the streams an element crosses (4-byte reads of param / grad / both moments,
4-byte writes of param / both moments, 2 or 6 bytes of shadow, 8 more with an EMA).
usage: python tools/optim_bench.py [--reps 20] [--warmup 3] [--burst 5] [--n 85700000] [--out FILE]"""
import argparse
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from predict_bench import PKG, interleaved, row  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--burst", type=int, default=5)
    ap.add_argument("--n", type=int, default=85_700_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("optim_bench.py measures on the MI355X: no GPU here, nothing is reported")
    F = importlib.import_module(PKG + ".functional")
    dev, n = torch.device("cuda", 0), a.n
    lines = ["device: %s; n = %d floats; %d repetitions after %d warm-up rounds, variants interleaved, HIP events around %d launches each" % (
        torch.cuda.get_device_name(0), n, a.reps, a.warmup, a.burst)]
    g = torch.Generator(device=dev).manual_seed(1)
    p = torch.randn(n, generator=g, device=dev) * 0.05
    grad = torch.randn(n, generator=g, device=dev) * 1e-3
    m, v, ema = torch.zeros(n, device=dev), torch.zeros(n, device=dev), p.clone()
    clip = torch.full((), 0.5, device=dev)
    hyper = (2e-4, 0.5, 0.999, 1e-8, 1)

    norm_run = lambda: [F.grad_norm(grad, 1.0) for _ in range(a.burst)]
    ms = interleaved([("sscg_grad_norm", norm_run)], a.reps, a.warmup)["sscg_grad_norm"]
    per = [t / a.burst for t in ms]
    lines += ["", "== gradient norm (one read of the arena, two launches)",
              "    " + row("sscg_grad_norm", per) + "   %.0f GB/s" % (4.0 * n / (statistics.median(per) * 1e-3) / 1e9)]

    for mode, bytes_sh in (("split", 6), ("bf16", 2)):
        sh = torch.zeros((3 if mode == "split" else 1) * n, dtype=torch.bfloat16, device=dev)
        kw = dict(shadow_split=sh) if mode == "split" else dict(shadow_bf16=sh)

        def ex(**opt):
            return lambda: [F.adam_step_ex(p, grad, m, v, *hyper, 1.0, **kw, **opt) for _ in range(a.burst)]
        variants = [("plain (sscg_adam_step)", (lambda: [F.adam_step(p, grad, m, v, *hyper, 1.0, **kw) for _ in range(a.burst)]), 0),
                    ("ex: clip", ex(clip=clip), 0), ("ex: weight decay (L2)", ex(weight_decay=1e-4), 0),
                    ("ex: weight decay (decoupled)", ex(weight_decay=1e-4, decoupled=True), 0), ("ex: EMA", ex(ema=ema, ema_decay=0.999), 8),
                    ("ex: clip + decoupled + EMA", ex(clip=clip, weight_decay=1e-4, decoupled=True, ema=ema, ema_decay=0.999), 8)]
        ms = interleaved([(k, fn) for k, fn, _ in variants], a.reps, a.warmup)
        base = statistics.median(ms[variants[0][0]])
        lines += ["", "== Adam launch, %s shadow" % mode]
        for k, _, extra in variants:
            per = [t / a.burst for t in ms[k]]
            lines.append("    " + row(k, per) + "   x%.3f of plain   %.0f GB/s" % (
                statistics.median(ms[k]) / base, (28.0 + bytes_sh + extra) * n / (statistics.median(per) * 1e-3) / 1e9))
        del sh
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
