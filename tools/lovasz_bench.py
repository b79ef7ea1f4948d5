#!/usr/bin/env python
"""The Lovasz-softmax loss and its segmented sort on the MI355X at the training step's size (8 x 21 x 33 x 33 -> 256 x 256), HIP
events around --reps back-to-back calls, the variants interleaved sample by sample, medians:

  sort          sscg_sort_u32_desc alone: 21 segments of 8 * 256 * 256 keys below 2^30 (the loss's planes)
  torch.sort    torch.sort(descending=True) of the same planes, for scale
  fused         sscg_lovasz_fwd + sscg_lovasz_scale_add + ONE sscg_upsample_head_bwd - what the step adds with --lovasz_weight
  lovasz_fwd    the forward alone
  torch ops     the same maths from torch ops on the device: F.interpolate(align_corners=True) -> softmax -> |f - p| -> torch.sort ->
                cumsum -> the Jaccard differences -> the dot product, autograd backward (the authors' formulation, all classes at once)

  --step        also the whole training step (voc2012, 256x256, batch 8) with --lovasz_weight 0.5 against off: two models in one
                process, timed alternately (bench.py takes no loss flags)

usage: python tools/lovasz_bench.py [--samples 20] [--reps 5] [--step] [--out FILE]      (needs the GPU: there is no CPU path)"""
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
PKG = "semi-supervised-segmentation-cyclegan_amd"
SHAPE = (8, 21, (33, 33), (256, 256))


def interleaved(torch, variants, samples, reps, warmup=2):
    for _ in range(warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name, _ in variants}
    for _ in range(samples):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e3 / reps)          # us per call
    return out


def kernels(torch, F, samples, reps, emit):
    import torch.nn.functional as TF
    B, C, (H, W), (OH, OW) = SHAPE
    dev = torch.device("cuda:0")
    lib, st = F.lib, F._stream()
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(B, H, W, C, generator=g) * 3).to(dev)
    lab = torch.randint(0, C - 1, (B, OH, OW), generator=g)            # class C - 1 is absent
    lab[torch.rand(B, OH, OW, generator=g) < 0.1] = 255
    lab = lab.to(dev)
    L = B * OH * OW
    keys = torch.empty(C * L, dtype=torch.int32, device=dev)
    coef, up = torch.empty(B, OH, OW, C, device=dev), torch.empty(B, OH, OW, C, device=dev)
    dx, loss, gl = torch.empty(B, H, W, C, device=dev), torch.empty((), device=dev), torch.tensor(0.5, device=dev)
    ws = torch.empty(lib.sscg_lovasz_workspace(B, OH, OW, C, 0), dtype=torch.uint8, device=dev)
    skeys, sidx = torch.empty(C, L, dtype=torch.int32, device=dev), torch.empty(C, L, dtype=torch.int32, device=dev)
    sws = torch.empty(lib.sscg_sort_ws_bytes(C, L), dtype=torch.uint8, device=dev)

    def lovasz_fwd():
        assert lib.sscg_lovasz_fwd(x.data_ptr(), lab.data_ptr(), B, H, W, C, OH, OW, 0, 0, 0, keys.data_ptr(), coef.data_ptr(), loss.data_ptr(),
                                   None, ws.data_ptr(), ws.numel(), st) == 0

    def fused():
        lovasz_fwd()
        assert lib.sscg_lovasz_scale_add(coef.data_ptr(), gl.data_ptr(), None, up.data_ptr(), coef.numel(), st) == 0
        assert lib.sscg_upsample_head_bwd(x.data_ptr(), up.data_ptr(), None, None, None, dx.data_ptr(), B, H, W, C, OH, OW, st) == 0

    def sort():
        assert lib.sscg_sort_u32_desc(keys.data_ptr(), C, L, 0x3F800002, skeys.data_ptr(), sidx.data_ptr(), sws.data_ptr(), sws.numel(), st) == 0

    k2 = keys.view(C, L)

    def torch_sort():
        return torch.sort(k2, 1, descending=True)

    xt = x.permute(0, 3, 1, 2).detach().requires_grad_(True)
    valid = (lab.reshape(-1) >= 0) & (lab.reshape(-1) < C)
    fg = (lab.reshape(-1)[valid].unsqueeze(0) == torch.arange(C, device=dev).unsqueeze(1)).float()      # [C, V]
    G = fg.sum(1, keepdim=True)
    present = (G.squeeze(1) > 0).float()

    def torch_ops():
        xt.grad = None
        p = torch.softmax(TF.interpolate(xt, size=(OH, OW), mode="bilinear", align_corners=True), 1)
        e = (fg - p.permute(1, 0, 2, 3).reshape(C, -1)[:, valid]).abs()
        es, perm = torch.sort(e, 1, descending=True)
        fs = fg.gather(1, perm)
        J = 1.0 - (G - fs.cumsum(1)) / (G + (1.0 - fs).cumsum(1))
        gj = torch.cat([J[:, :1], J[:, 1:] - J[:, :-1]], 1)
        out = ((es * gj.detach()).sum(1) * present).sum() / present.sum()
        (0.5 * out).backward()
        return out.detach()

    fused()
    torch.cuda.synchronize()
    first = [t.clone() for t in (loss, coef, keys, dx)]
    fused()
    torch.cuda.synchronize()
    same = all(torch.equal(p, q) for p, q in zip(first, (loss, coef, keys, dx)))
    ref = float(torch_ops())
    agree = float((xt.grad - dx.permute(0, 3, 1, 2)).abs().max() / xt.grad.abs().max())
    sort()
    tk, _ = torch_sort()
    tag = "%dx%dx%dx%d -> %dx%d" % (B, C, H, W, OH, OW)
    emit("%s  fused twice bit-identical: %s; loss %.7f (torch ops: %.7f); gradients agree to %.1e of the largest; sorted keys equal "
         "torch.sort's: %s" % (tag, same, float(loss), ref, agree, bool(torch.equal(tk, skeys))))
    emit("%s  workspace %.1f MB + keys %.1f MB + coefficient map %.1f MB" % (tag, ws.numel() / 1e6, keys.numel() * 4 / 1e6, coef.numel() * 4 / 1e6))
    if not same:
        raise SystemExit("the fused path is not deterministic: nothing timed")
    variants = [("sort", sort), ("torch.sort", torch_sort), ("fused", fused), ("lovasz_fwd", lovasz_fwd), ("torch ops", torch_ops)]
    us = interleaved(torch, variants, samples, reps)
    med = {}
    for name, _ in variants:
        v = us[name]
        med[name] = statistics.median(v)
        emit("%s  %-11s median %9.1f us (range %.1f .. %.1f over %d samples of %d)" % (tag, name, med[name], min(v), max(v), samples, reps))
    emit("%s  torch ops / fused: %.2fx; torch.sort / sort: %.2fx; the sort is %.0f %% of the forward" % (
        tag, med["torch ops"] / med["fused"], med["torch.sort"] / med["sort"], 100 * med["sort"] / med["lovasz_fwd"]))


def whole_step(torch, F, emit, rounds=3, steps=8):
    md, data = importlib.import_module(PKG + ".model"), importlib.import_module(PKG + ".data")
    import main as cli
    dev = torch.device("cuda:0")
    on_flags = ["--lovasz_weight", "0.5"]
    models = {}
    for tag, extra in (("off", []), ("on", on_flags)):
        args = cli.get_args(["--model", "semisupervised_cycleGAN", "--dataset", "voc2012", "--crop_height", "256", "--crop_width", "256",
                             "--batch_size", "8", "--checkpoint_dir", "/tmp/sscg_lovasz_bench_ckpt"] + extra)
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
    off, on = statistics.median(times["off"]), statistics.median(times["on"])
    emit("whole step voc2012 256x256 batch 8: flags off %.2f ms (%s), %s %.2f ms (%s): %+.2f ms, %+.2f %% (alternating, %d rounds of %d steps)" % (
        off, " ".join("%.2f" % t for t in times["off"]), " ".join(on_flags), on, " ".join("%.2f" % t for t in times["on"]), on - off,
        100 * (on - off) / off, rounds, steps))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/lovasz_bench.py measures on the MI355X: no GPU here, nothing measured")
    F = importlib.import_module(PKG + ".functional")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit("device: %s" % torch.cuda.get_device_name(0))
    kernels(torch, F, a.samples, a.reps, emit)
    if a.step:
        whole_step(torch, F, emit)


if __name__ == "__main__":
    main()
