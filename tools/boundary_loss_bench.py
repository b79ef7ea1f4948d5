#!/usr/bin/env python
"""The boundary loss of the fused label head, timed with HIP events on the MI355X at the training step's sizes (DeepLab's stride-8
logit map -> the crop), on labels made of blobs (a coarse random map, 16 x 16 pixel cells - per-pixel noise would make every distance 1):
  sdm     : sscg_sdm (counts, then a column and a row pass per chunk of 16 classes)
  forward : sscg_boundary_loss_fwd (statistics + reduce + finish), resized and flat (on the materialised crop-size logits)
  backward: sscg_upsample_head_bwd_b with the boundary term (alone; + CE; + CE + Dice; + CE + Dice + dy_soft)  vs  the same entry with
            sdm == NULL (= sscg_upsample_head_bwd_h: mined CE; + Dice; + Dice + dy_soft) and sscg_upsample_head_bwd_d (Dice + CE), and
            the flat sscg_boundary_loss_bwd
  host    : what the device path replaces - scipy.ndimage.distance_transform_edt per sample and class on the host (Kervadec's
            one_hot2dist) plus the copy of the C-channel fp32 map to the device; wall clock, synchronised
  step    : --step: supervised_model.step with --boundary_loss 0.5 against the same tree with the flag off, interleaved
Each device figure is the time of --burst back-to-back launches of one entry divided by --burst; the variants are interleaved
repetition by repetition and medians are reported.  Before anything is timed, sscg_sdm and the loss forward are run twice and their
outputs compared bit for bit.
usage: python tools/boundary_loss_bench.py [--reps 20] [--warmup 3] [--burst 10] [--configs acdc,voc,cityscapes] [--step] [--out FILE]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from predict_bench import PKG, interleaved, row  # noqa: E402

# dataset, classes, batch, logit map, crop
CONFIGS = {"acdc": ("acdc", 4, 8, (33, 33), (256, 256)), "voc": ("voc2012", 21, 8, (33, 33), (256, 256)),
           "cityscapes": ("cityscapes", 20, 16, (33, 65), (256, 512))}


def blob_labels(g, B, OH, OW, C, cell=16):
    coarse = torch.randint(0, C, (B, (OH + cell - 1) // cell, (OW + cell - 1) // cell), generator=g)
    lab = coarse.repeat_interleave(cell, 1).repeat_interleave(cell, 2)[:, :OH, :OW].contiguous()
    lab.view(-1)[::97] = 255
    return lab


def host_path(lab, C, dev):
    """Kervadec's one_hot2dist per sample and class with scipy, then the copy: seconds"""
    from scipy.ndimage import distance_transform_edt as edt
    lab = lab.numpy()
    t0 = time.perf_counter()
    out = np.zeros((lab.shape[0], C) + lab.shape[1:], dtype=np.float32)
    for n in range(lab.shape[0]):
        for c in range(C):
            pos = lab[n] == c
            if pos.any():
                neg = ~pos
                out[n, c] = edt(neg) * neg - (edt(pos) - 1) * pos
    t1 = time.perf_counter()
    d = torch.from_numpy(out).to(dev)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    del d
    return t1 - t0, t2 - t1


def step_times(md, data, F, dataset, B, crop, reps, warmup, dev):
    """{flag off, flag on}: ms per supervised_model.step, the two models interleaved"""
    from oracle import fixtures as FX
    models = {}
    for tag, kw in (("flag off", {}), ("--boundary_loss 0.5", dict(boundary_loss=0.5))):
        args = FX.make_args(dataset=dataset, crop_height=crop[0], crop_width=crop[1], batch_size=B, gpu_ids=[0], model="supervised_model",
                            checkpoint_dir="/tmp/sscg_bnd_bench_ckpt", as_written=True, **kw)
        torch.manual_seed(1)
        with contextlib.redirect_stdout(io.StringIO()):
            m = md.supervised_model(args)
            loader = data.synthetic_loaders(args, m.n_channels, steps=1)[0]
        l_img, l_gt, _ = next(iter(loader))
        models[tag] = (m, l_img.to(dev), l_gt.to(dev))

    def stepper(tag):
        m, l_img, l_gt = models[tag]

        def run():
            m.step(l_img, l_gt)
            F.flush_side_work()
        return run
    return interleaved([(tag, stepper(tag)) for tag in models], reps, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--configs", default="acdc,voc,cityscapes")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("boundary_loss_bench.py measures on the MI355X: no GPU here, nothing is reported")
    F = importlib.import_module(PKG + ".functional")
    lib, dev = F.lib, torch.device("cuda", 0)
    lines = ["device: %s; %d repetitions after %d warm-up rounds, variants interleaved, HIP events around %d launches each" % (
        torch.cuda.get_device_name(0), a.reps, a.warmup, a.burst)]
    for key in a.configs.split(","):
        dataset, C, B, (H, W), (OH, OW) = CONFIGS[key]
        g = torch.Generator().manual_seed(5)
        x = (torch.randn(B, H, W, C, generator=g) * 3).to(dev)
        lab_cpu = blob_labels(g, B, OH, OW, C)
        lab = lab_cpu.to(dev)
        one = torch.ones(1, device=dev)
        dx = torch.empty(B, H, W, C, device=dev)
        dy = torch.randn(B, OH, OW, C, generator=g).to(dev)
        sdm = torch.empty(B, OH, OW, C, dtype=torch.int32, device=dev)
        sws = torch.empty(lib.sscg_sdm_workspace(B, OH, OW, C), dtype=torch.uint8, device=dev)
        bws = torch.empty(lib.sscg_boundary_loss_workspace(B, OH, OW, C), dtype=torch.uint8, device=dev)
        bloss, bcoef = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
        sums, counted = torch.zeros(B, C, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        up, dup = torch.empty(B, OH, OW, C, device=dev), torch.empty(B, OH, OW, C, device=dev)
        assert lib.sscg_upsample_bilinear_fwd(x.data_ptr(), up.data_ptr(), B, H, W, C, OH, OW, F._stream()) == 0
        xn = x.permute(0, 3, 1, 2)                                   # the NCHW view of the channels-last logits
        _, valid, keys, thr, _ = F.ohem_fwd(xn, lab, (OH, OW), F.OhemOptions(0.7, min_frac=0.0625))
        _, coef, _ = F.dice_fwd(xn, lab, (OH, OW))
        ploss, pvalid, dl = torch.zeros(1, device=dev), torch.zeros(1, device=dev), torch.empty(B, H, W, C, device=dev)
        hws = torch.empty(lib.sscg_upsample_head_workspace(B, H, W), dtype=torch.uint8, device=dev)
        assert lib.sscg_upsample_head_fwd(x.data_ptr(), lab.data_ptr(), None, ploss.data_ptr(), pvalid.data_ptr(), dl.data_ptr(), B, H, W, C,
                                          OH, OW, hws.data_ptr(), hws.numel(), F._stream()) == 0

        def sdm_run():
            for _ in range(a.burst):
                assert lib.sscg_sdm(lab.data_ptr(), B, OH, OW, C, sdm.data_ptr(), sws.data_ptr(), sws.numel(), F._stream()) == 0

        def loss_fwd(flat):
            def run():
                src, h, w = (up, OH, OW) if flat else (x, H, W)
                for _ in range(a.burst):
                    assert lib.sscg_boundary_loss_fwd(src.data_ptr(), lab.data_ptr(), sdm.data_ptr(), B, h, w, C, OH, OW, None, bloss.data_ptr(),
                                                      sums.data_ptr(), counted.data_ptr(), bcoef.data_ptr(), bws.data_ptr(), bws.numel(),
                                                      F._stream()) == 0
            return run

        def head_b(bnd, ce, dice, soft, mined=False):
            def run():
                for _ in range(a.burst):
                    assert lib.sscg_upsample_head_bwd_b(
                        x.data_ptr(), lab.data_ptr(), keys.data_ptr() if (ce and mined) else None, thr.data_ptr() if (ce and mined) else None,
                        None, 0.0, dy.data_ptr() if soft else None, one.data_ptr() if ce else None,
                        (valid if mined else pvalid).data_ptr() if ce else None, coef.data_ptr() if dice else None,
                        one.data_ptr() if dice else None, 0, dx.data_ptr(), B, H, W, C, OH, OW, sdm.data_ptr() if bnd else None,
                        bcoef.data_ptr(), None, one.data_ptr(), F._stream()) == 0
            return run

        def head_d():
            for _ in range(a.burst):
                assert lib.sscg_upsample_head_bwd_d(x.data_ptr(), lab.data_ptr(), None, dl.data_ptr(), one.data_ptr(), pvalid.data_ptr(),
                                                    coef.data_ptr(), one.data_ptr(), 0, dx.data_ptr(), B, H, W, C, OH, OW, F._stream()) == 0

        def flat_bwd():
            for _ in range(a.burst):
                assert lib.sscg_boundary_loss_bwd(up.data_ptr(), lab.data_ptr(), sdm.data_ptr(), B, OH, OW, C, None, bcoef.data_ptr(), one.data_ptr(),
                                                  1.0, dup.data_ptr(), F._stream()) == 0

        def outputs():
            sdm.fill_(7)
            sws.fill_(0x5A)
            for t in (bloss, bcoef, sums):
                t.fill_(7.0)
            assert lib.sscg_sdm(lab.data_ptr(), B, OH, OW, C, sdm.data_ptr(), sws.data_ptr(), sws.numel(), F._stream()) == 0
            assert lib.sscg_boundary_loss_fwd(x.data_ptr(), lab.data_ptr(), sdm.data_ptr(), B, H, W, C, OH, OW, None, bloss.data_ptr(),
                                              sums.data_ptr(), counted.data_ptr(), bcoef.data_ptr(), bws.data_ptr(), bws.numel(), F._stream()) == 0
            torch.cuda.synchronize()
            return [t.clone() for t in (sdm, bloss, bcoef, sums, counted)]

        same = all(torch.equal(p, q) for p, q in zip(outputs(), outputs()))
        lines.append("")
        lines.append("== %s: B = %d, %d classes, logits %dx%d -> %dx%d; sdm %.1f MB, max |sdm| %d; sscg_sdm + loss forward twice bit-identical: %s; "
                     "loss %.6f" % (dataset, B, C, H, W, OH, OW, sdm.numel() * 4 / 1e6, int(sdm.abs().max()), same, float(bloss)))
        if not same:
            sys.exit("\n".join(lines + ["the forward is not deterministic: nothing timed"]))
        variants = [("sscg_sdm", sdm_run), ("boundary_loss_fwd, resized", loss_fwd(False)), ("boundary_loss_fwd, flat (materialised)", loss_fwd(True))]
        ms = interleaved(variants, a.reps, a.warmup)
        lines.append("  forward")
        for name, _ in variants:
            lines.append("    " + row(name, [v / a.burst for v in ms[name]]))
        variants = [("bwd_b sdm=NULL: mined CE", head_b(False, True, False, False, True)),
                    ("bwd_b sdm=NULL: mined CE + Dice", head_b(False, True, True, False, True)),
                    ("bwd_b sdm=NULL: mined CE+Dice+soft", head_b(False, True, True, True, True)),
                    ("bwd_d: CE + Dice", head_d),
                    ("bwd_b: boundary only", head_b(True, False, False, False)),
                    ("bwd_b: boundary + CE", head_b(True, True, False, False)),
                    ("bwd_b: boundary + CE + Dice", head_b(True, True, True, False)),
                    ("bwd_b: boundary + mined CE + Dice", head_b(True, True, True, False, True)),
                    ("bwd_b: boundary+mined CE+Dice+soft", head_b(True, True, True, True, True)),
                    ("flat boundary_loss_bwd", flat_bwd)]
        ms = interleaved(variants, a.reps, a.warmup)
        base = statistics.median(ms["bwd_b sdm=NULL: mined CE + Dice"])
        lines.append("  backward")
        for name, _ in variants:
            lines.append("    " + row(name, [v / a.burst for v in ms[name]]) + "   x%.3f of the mined CE + Dice head" % (statistics.median(ms[name]) / base))
        host = [host_path(lab_cpu, C, dev) for _ in range(3)]
        lines.append("  host path it replaces (scipy per sample and class, then the copy of %.1f MB): edt median %.1f ms, copy median %.2f ms" % (
            B * C * OH * OW * 4 / 1e6, 1e3 * statistics.median(h[0] for h in host), 1e3 * statistics.median(h[1] for h in host)))
        del x, lab, dy, dx, up, dup, sdm, sws
        torch.cuda.empty_cache()
        if a.step:
            md, data = importlib.import_module(PKG + ".model"), importlib.import_module(PKG + ".data")
            ms = step_times(md, data, F, dataset, B, (OH, OW), max(a.reps // 2, 5), a.warmup, dev)
            lines.append("  supervised_model.step, B = %d, crop %dx%d" % (B, OH, OW))
            for name in ms:
                lines.append("    " + row(name, ms[name]))
            torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
