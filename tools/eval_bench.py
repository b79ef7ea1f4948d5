#!/usr/bin/env python
"""Eval-mode BatchNorm folded into the conv (sscg_conv2d_fwd_affine) against the separate passes, timed with HIP events on the MI355X.
  (a) the DeepLab eval forward of the configuration's batch (VOC B=8 256x256, Cityscapes B=16 256x512), fp32 (split) and bf16 modes;
  (b) one evaluate() pass over a synthetic loader of --batches batches (fp32 mode, as the drivers run it).
Fused (the default) against F.FUSE_EVAL_NORM = False - the parent path: conv, sscg_rstd_from_var, sscg_norm_apply per unit - in the
same process, warm-up first, the two variants interleaved repetition by repetition, medians and spread reported.  The outputs of both
variants are compared bit for bit before anything is timed.  Every configuration runs in a child process under a time limit of its own.
usage: python tools/eval_bench.py [--reps 20] [--warmup 3] [--batches 16] [--configs voc,cityscapes] [--modes f32s,bf16] [--out FILE]"""
import argparse
import contextlib
import importlib
import io
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "semi-supervised-segmentation-cyclegan_amd"
CONFIGS = {"voc": ("voc2012", 21, 8, 256, 256), "cityscapes": ("cityscapes", 20, 16, 256, 512)}


def row(name, v):
    v = sorted(v)
    return "%-28s median %9.3f ms   min %9.3f   p90 %9.3f   (n = %d)" % (name, statistics.median(v), v[0], v[int(0.9 * (len(v) - 1))], len(v))


def child(key, mode, reps, warmup, batches):
    import torch
    F = importlib.import_module(PKG + ".functional")
    md = importlib.import_module(PKG + ".model")
    from oracle import fixtures as FX
    dev = torch.device("cuda", 0)
    dataset, C, B, H, W = CONFIGS[key]
    F.set_conv_precision(mode)
    args = FX.make_args(dataset=dataset, crop_height=H, crop_width=W, batch_size=B, gpu_ids=[0], checkpoint_dir="/tmp/sscg_eval_bench",
                        as_written=True)
    with contextlib.redirect_stdout(io.StringIO()):
        m = md.supervised_model(args)
    g = torch.Generator().manual_seed(5)
    loader = [(torch.randn(B, 3, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last),
               torch.randint(0, C, (B, 1, H, W), generator=g).to(dev), ["s"] * B) for _ in range(batches)]
    m.Gsi.eval()
    x = loader[0][0]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    def interleaved(variants, n, w):
        for _ in range(w):
            for _, fn in variants:
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in variants}
        for _ in range(n):
            for name, fn in variants:
                ms[name].append(timed(fn)[0])
        return ms

    def with_flag(flag, fn):
        def run():
            was = F.FUSE_EVAL_NORM[0]
            F.FUSE_EVAL_NORM[0] = flag
            try:
                with torch.no_grad():
                    return fn()
            finally:
                F.FUSE_EVAL_NORM[0] = was
        return run

    def report(title, ms):
        print(title)
        for name in ms:
            print("    " + row(name, ms[name]))
        u, f = statistics.median(ms["SSCG_FUSE_EVAL_NORM=0"]), statistics.median(ms["default (fused)"])
        su, sf = sorted(ms["SSCG_FUSE_EVAL_NORM=0"]), sorted(ms["default (fused)"])
        spread = max(su[int(0.9 * (len(su) - 1))] - su[0], sf[int(0.9 * (len(sf) - 1))] - sf[0])
        print("    fused / separate = %.4f (%+.2f %%); repetition spread (p90 - min) %.3f ms = %.2f %%" % (
            f / u, 100.0 * (f - u) / u, spread, 100.0 * spread / u))

    print("== %s, %s: B = %d, %d x %d (%s)" % (dataset, mode, B, H, W, torch.cuda.get_device_name(0)))
    fwd = lambda: m.Gsi(x)
    a, b = with_flag(True, fwd)(), with_flag(False, fwd)()
    same = torch.equal(a, b)
    print("(a) DeepLab eval forward; logits bit-identical: %s" % same)
    if not same:
        sys.exit("the fused forward does not reproduce the separate passes: nothing timed")
    report("", interleaved([("SSCG_FUSE_EVAL_NORM=0", with_flag(False, fwd)), ("default (fused)", with_flag(True, fwd))], reps, warmup))
    if mode == "f32s" and batches > 0:
        ev = lambda: m.evaluate(loader)[0]
        same = with_flag(False, ev)() == with_flag(True, ev)()
        m.Gsi.eval()
        report("(b) evaluate() over %d batches (forward + predict head + host mIoU); equal mIoU: %s" % (batches, same),
               interleaved([("SSCG_FUSE_EVAL_NORM=0", with_flag(False, ev)), ("default (fused)", with_flag(True, ev))], max(reps // 2, 6), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--configs", default="voc,cityscapes")
    ap.add_argument("--modes", default="f32s,bf16")
    ap.add_argument("--timeout", type=int, default=280, help="seconds per configuration (a child process each)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.reps, a.warmup, a.batches)
    import torch
    if not torch.cuda.is_available():
        sys.exit("eval_bench.py measures on the MI355X: no GPU here, nothing is reported")
    lines = ["%d repetitions after %d warm-up rounds, variants interleaved, HIP events" % (a.reps, a.warmup)]
    for key in a.configs.split(","):
        for mode in a.modes.split(","):
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", key, mode, "--reps", str(a.reps),
                   "--warmup", str(a.warmup), "--batches", str(a.batches)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            lines += ["", r.stdout.rstrip()]
            if r.returncode != 0:       # a fault, an abort or the time limit: nothing more is started on the device
                lines.append("child exited with status %d: stopping here\n%s" % (r.returncode, r.stderr[-2000:]))
                break
        else:
            continue
        break
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
