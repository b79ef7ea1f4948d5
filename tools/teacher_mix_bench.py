#!/usr/bin/env python
"""CutMix consistency for the mean teacher (`--unl_cutmix`: sscg_teacher_fwd_mix, sscg_mix_boxes) on the MI355X at the training step's
sizes, HIP events around --reps back-to-back calls, the variants interleaved sample by sample (tools/ab.sh's order: a b a b ...),
medians and ranges:

  (a) mix vs plain   sscg_teacher_fwd_mix with interior boxes (every sample mixes, a box of 3/8 of the area, the partner the next
                     sample) against sscg_teacher_fwd on the same inputs: what the lookup and the per-thread source rows cost
  (b) fused vs       the fused route - ONE sscg_teacher_fwd_mix on the low-resolution teacher - against the separate passes:
      separate       sscg_upsample_bilinear_fwd of the teacher's logits (the [N, OH, OW, C] map the fused route never writes), a per-sample
                     flip and torch.where with the pasted mask, then the identity-size sscg_teacher_fwd; outputs compared bit for bit
  (c) mix_boxes      sscg_mix_boxes on the image batch [N, OH, OW, 3] against torch.where on the same mask, and its achieved bandwidth
                     (bytes = one read and one write of the batch; the partner's pixels replace the sample's own reads)
  (d) --step         the whole training step (voc2012, 256x256, batch 8, --ema_decay 0.999, --unl_teacher mse=1,ce=0.5,thresh=0.35,flip)
                     with and without `--unl_cutmix 1`: two models in one process, timed alternately, the spread of both arms

usage: python tools/teacher_mix_bench.py [--samples 30] [--reps 20] [--step | --step-only] [--rounds 5] [--out FILE]
(needs the GPU: there is no CPU path)"""
import argparse
import contextlib
import importlib
import io
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
PKG = "semi-supervised-segmentation-cyclegan_amd"
from teacher_bench import SHAPES, TAU, interleaved  # noqa: E402  (the shapes, the threshold and the timing loop of the plain entry's bench)


def interior_table(torch, B, OH, OW):
    """every sample takes a box of 3/4 of the height by 1/2 of the width (3/8 of the area, the middle of --unl_cutmix's default
    0.25..0.5) from the next sample, off centre"""
    rows = torch.zeros(B, 8, dtype=torch.int32)
    for n in range(B):
        x0, y0 = OW // 8 + (n * 7) % (OW // 4), OH // 16 + (n * 5) % (OH // 8)
        rows[n, :5] = torch.tensor([(n + 1) % B, x0, y0, x0 + OW // 2, y0 + (3 * OH) // 4])
    return rows


def pasted_mask(torch, rows, OH, OW, dev):
    ys = torch.arange(OH, device=dev).view(1, OH, 1)
    xs = torch.arange(OW, device=dev).view(1, 1, OW)
    r = rows.to(dev).long()
    return ((xs >= r[:, 1].view(-1, 1, 1)) & (xs < r[:, 3].view(-1, 1, 1)) & (ys >= r[:, 2].view(-1, 1, 1)) & (ys < r[:, 4].view(-1, 1, 1)))


def report(emit, tag, us, samples, reps):
    med = {}
    for name, v in us.items():
        med[name] = statistics.median(v)
        emit("%s  %-26s median %9.1f us (range %.1f .. %.1f over %d samples of %d)" % (tag, name, med[name], min(v), max(v), samples, reps))
    return med


def kernels(torch, F, shape, samples, reps, emit):
    B, C, (H, W), (OH, OW) = shape
    dev = torch.device("cuda:0")
    lib, st = F.lib, F._stream()
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(B, H, W, C, generator=g) * 3).to(dev)
    t = (x.cpu() + torch.randn(B, H, W, C, generator=g) * 1.5).to(dev)
    flips = [n % 2 == 0 for n in range(B)]
    flip = torch.tensor(flips, dtype=torch.uint8, device=dev)
    rows = interior_table(torch, B, OH, OW)
    table = rows.to(dev)
    mask = pasted_mask(torch, rows, OH, OW, dev)                       # [B, OH, OW]
    partner = rows[:, 0].long().to(dev)
    share = float(mask.float().mean())
    tag = "%dx%dx%dx%d -> %dx%d" % (B, C, H, W, OH, OW)

    def outputs():
        return (torch.empty(2, device=dev), torch.empty(4, dtype=torch.float64, device=dev), torch.empty(B, OH, OW, dtype=torch.uint8, device=dev),
                torch.empty(B, OH, OW, C, device=dev))
    out_mix, out_plain, out_sep = outputs(), outputs(), outputs()
    ws = torch.empty(lib.sscg_teacher_workspace(B, OH, OW), dtype=torch.uint8, device=dev)
    up_x, up_t = torch.empty(B, OH, OW, C, device=dev), torch.empty(B, OH, OW, C, device=dev)
    assert lib.sscg_upsample_bilinear_fwd(x.data_ptr(), up_x.data_ptr(), B, H, W, C, OH, OW, st) == 0
    fmask, m4 = flip.bool().view(B, 1, 1, 1), mask.unsqueeze(-1)

    def tail(o):
        return (1.0, TAU, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), ws.data_ptr(), ws.numel(), st)

    def mix():
        assert lib.sscg_teacher_fwd_mix(x.data_ptr(), t.data_ptr(), flip.data_ptr(), table.data_ptr(), B, H, W, C, OH, OW, *tail(out_mix)) == 0

    def plain():
        assert lib.sscg_teacher_fwd(x.data_ptr(), t.data_ptr(), flip.data_ptr(), B, H, W, C, OH, OW, *tail(out_plain)) == 0

    def separate():
        # the teacher's side of the separate passes: resize (written), un-mirror, select, then the identity-size plain entry.  That entry
        # needs the student at the output size too: `up_x` is resized once, OUTSIDE the timed region - the separate route gets it free
        assert lib.sscg_upsample_bilinear_fwd(t.data_ptr(), up_t.data_ptr(), B, H, W, C, OH, OW, st) == 0
        a = torch.where(fmask, up_t.flip(2), up_t)
        mixed = torch.where(m4, a[partner], a)
        assert lib.sscg_teacher_fwd(up_x.data_ptr(), mixed.data_ptr(), None, B, OH, OW, C, OH, OW, *tail(out_sep)) == 0

    mix()
    separate()
    torch.cuda.synchronize()
    same = all(torch.equal(p, q) for p, q in zip(out_mix, out_sep))
    V = B * OH * OW
    emit("%s  boxes: %.3f of the pixels pasted; fused = separate passes bit for bit: %s; kept %.3f agree %.3f (plain entry on the same inputs: "
         "see below)" % (tag, share, same, float(out_mix[1][3]) / V, float(out_mix[1][1]) / max(float(out_mix[1][3]), 1.0)))
    if not same:
        raise SystemExit("the fused route and the separate passes differ: nothing timed")
    us = interleaved(torch, [("teacher_fwd_mix (fused)", mix), ("teacher_fwd (plain)", plain), ("separate passes", separate)], samples, reps)
    med = report(emit, tag, us, samples, reps)
    emit("%s  (a) mix / plain: x%.3f (%+.1f us);  (b) separate / fused: x%.2f (%+.1f us; the separate passes write and read the resized "
         "teacher, %.1f MB)" % (tag, med["teacher_fwd_mix (fused)"] / med["teacher_fwd (plain)"],
                                med["teacher_fwd_mix (fused)"] - med["teacher_fwd (plain)"], med["separate passes"] / med["teacher_fwd_mix (fused)"],
                                med["separate passes"] - med["teacher_fwd_mix (fused)"], B * OH * OW * C * 4 / 1e6))
    # ---- (c) the student's input: the image batch at the output size, 3 channels
    img = torch.randn(B, OH, OW, 3, generator=g).to(dev)
    y = torch.empty_like(img)

    def boxes():
        assert lib.sscg_mix_boxes(img.data_ptr(), y.data_ptr(), table.data_ptr(), B, OH, OW, 3, st) == 0

    def where():
        return torch.where(m4, img[partner], img)

    boxes()
    torch.cuda.synchronize()
    if not torch.equal(y, where()):
        raise SystemExit("sscg_mix_boxes differs from torch.where: nothing timed")
    us = interleaved(torch, [("mix_boxes", boxes), ("torch.where (+ gather)", where)], samples, reps)
    med = report(emit, tag + " image", us, samples, reps)
    nbytes = 2 * img.numel() * 4
    emit("%s image  (c) torch.where / mix_boxes: x%.2f; mix_boxes moves %.2f MB in %.1f us: %.0f GB/s achieved (read + write of the batch)" % (
        tag, med["torch.where (+ gather)"] / med["mix_boxes"], nbytes / 1e6, med["mix_boxes"], nbytes / med["mix_boxes"] / 1e3))


def whole_step(torch, F, emit, rounds=5, steps=8):
    md, data = importlib.import_module(PKG + ".model"), importlib.import_module(PKG + ".data")
    import main as cli
    dev = torch.device("cuda:0")
    base = ["--unl_teacher", "mse=1,ce=0.5,thresh=%g,flip" % TAU]
    models = {}
    for tag, extra in (("teacher", base), ("teacher + cutmix", base + ["--unl_cutmix", "1"])):
        args = cli.get_args(["--model", "semisupervised_cycleGAN", "--dataset", "voc2012", "--crop_height", "256", "--crop_width", "256",
                             "--batch_size", "8", "--checkpoint_dir", "/tmp/sscg_teacher_mix_bench_ckpt", "--ema_decay", "0.999"] + extra)
        args.gpu_ids, args.as_written, args.overlap_d = [0], True, False
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            models[tag] = md.semisuper_cycleGAN(args)
    lab = list(data.SyntheticLoader(8, 21, 256, 256, 4, 3, device=dev))
    unl = list(data.SyntheticLoader(8, 21, 256, 256, 4, 4, device=dev))
    times = {tag: [] for tag in models}
    for r in range(rounds + 1):                     # round 0 warms both up
        for tag, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                m.step(lab[i % 4][0], lab[i % 4][1], unl[i % 4][0])
            m.sync_losses()
            F.flush_side_work()
            torch.cuda.synchronize()
            if r:
                times[tag].append((time.perf_counter() - t0) * 1e3 / steps)
    a, b = statistics.median(times["teacher"]), statistics.median(times["teacher + cutmix"])
    emit("(d) whole step voc2012 256x256 batch 8 --ema_decay 0.999 %s: without --unl_cutmix %.2f ms (%s; spread %.2f), with --unl_cutmix 1 "
         "%.2f ms (%s; spread %.2f): %+.2f ms, %+.2f %% (alternating, %d rounds of %d steps)" % (
             " ".join(base), a, " ".join("%.2f" % v for v in times["teacher"]), max(times["teacher"]) - min(times["teacher"]), b,
             " ".join("%.2f" % v for v in times["teacher + cutmix"]), max(times["teacher + cutmix"]) - min(times["teacher + cutmix"]),
             b - a, 100 * (b - a) / a, rounds, steps))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--step-only", action="store_true", help="(d) alone")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds of (d)")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/teacher_mix_bench.py measures on the MI355X: no GPU here, nothing measured")
    F = importlib.import_module(PKG + ".functional")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit("device: %s" % torch.cuda.get_device_name(0))
    for shape in ([] if a.step_only else SHAPES):
        kernels(torch, F, shape, a.samples, a.reps, emit)
    if a.step or a.step_only:
        whole_step(torch, F, emit, rounds=a.rounds)


if __name__ == "__main__":
    main()
