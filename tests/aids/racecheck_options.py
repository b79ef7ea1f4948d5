"""racecheck_step.py's `options=<name>` scenario (see its docstring): the semi-supervised step with a set of opt-in options on, fed by
augmenting DeviceLoaders, an evaluation under the EMA weights between two steps, then two supervised steps - all under the
stream-ordering checker, with no host synchronisation the product would not make."""
import contextlib
import importlib
import io
import itertools
import os
import sys
import tempfile

import torch

import step_options as SO

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden"))
from data_trees import data_trees  # noqa: E402
from oracle import fixtures as FX  # noqa: E402


def _floats(rec):
    return {k: float(v) for k, v in rec.items()}


def _norm_rows(pairs):
    rows = []
    for who, opt in pairs:
        if opt.last_grad_norm is not None:
            rows.append((who, float(opt.last_grad_norm), opt.max_grad_norm))
            print("%s: last_grad_norm %.6g (clip %.6g)" % rows[-1])
    return rows


def run(name, md, F, rc, dp, dev, steps, size, batch, overlap):
    du = importlib.import_module(md.__name__.rsplit(".", 1)[0] + ".data_utils")
    opts = SO.OPTIONS[name]
    lib = F.lib
    bad, vacuous = 0, False
    with tempfile.TemporaryDirectory(prefix="sscg_rc_") as tmp:
        args = FX.make_args(dataset="voc2012", crop_height=size, crop_width=size, batch_size=batch, gpu_ids=[0],
                            checkpoint_dir=os.path.join(tmp, "ckpt"), as_written=True, augment=SO.AUGMENT, **opts)
        args.overlap_d = overlap
        torch.manual_seed(0)                                    # the networks' initial weights and the loaders' shuffles
        with contextlib.redirect_stdout(io.StringIO()):
            roots = data_trees(os.path.join(tmp, "data"))
            m = md.semisuper_cycleGAN(args, data_parallel=dp)
            lab, unl, val = du.build_loaders(args, roots=roots, device=dev)
        torch.cuda.synchronize()
        outs = []
        for s, ((l_img, l_gt, _), (unl_img, _, _)) in enumerate(itertools.islice(zip(lab, unl), steps)):
            outs.append(m.step(l_img, l_gt, unl_img))
            rc.name_streams(F, dev)
            print("step %d issued: %d launches, %d reports so far" % (s, rc.CORE.launches, len(rc.CORE.reports)), flush=True)
            if s == 1:      # train()'s end of an epoch: sync_losses(), then the evaluation under the averaged weights
                m.sync_losses()
                with m.g_optimizer.ema_weights(), contextlib.redirect_stdout(io.StringIO()):
                    miou, _ = m.evaluate(itertools.islice(val, 2))
                print("evaluated 2 batches under the EMA weights: mIoU %.6g, %d launches, %d reports so far" % (
                    miou, rc.CORE.launches, len(rc.CORE.reports)), flush=True)
        assert len(outs) == steps, "the loaders gave %d batches, %d steps were asked for" % (len(outs), steps)
        m.sync_losses()
        torch.cuda.synchronize()
        recs = [_floats(o) for o in outs]
        print("losses finite:", all(v == v and abs(v) != float("inf") for rec in recs for v in rec.values()))
        for s, rec in enumerate(recs):
            print("step %d: %s" % (s, " ".join("%s=%.6g" % (k, rec[k]) for k in sorted(rec) if k not in md.LOSS_KEYS)))
        norms = _norm_rows((("G", m.g_optimizer), ("D", m.d_optimizer)))
        counts = dict(lib.counts)
        print("census: %s" % " ".join("%s=%d" % (e, counts.get(e, 0)) for e in SO.ENTRIES[name] + SO.AUGMENT_ENTRIES))
        print("semi-supervised phase:")
        core = rc.report(sys.stdout)
        bad += len(core.reports)
        try:
            SO.check_not_vacuous(name, recs, counts, norms, entries=SO.ENTRIES[name] + SO.AUGMENT_ENTRIES)
        except AssertionError as e:
            print(e, flush=True)
            vacuous = True

        # ---- two supervised steps with the same flags, in the same process
        before, launched, seen = len(core.order), core.launches, dict(lib.counts)
        sargs = FX.make_args(dataset="voc2012", crop_height=size, crop_width=size, batch_size=batch, gpu_ids=[0], model="supervised_model",
                             checkpoint_dir=os.path.join(tmp, "ckpt_sup"), **SO.supervised(opts))
        with contextlib.redirect_stdout(io.StringIO()):
            sm = md.supervised_model(sargs, data_parallel=None)
        srecs = []
        for s, (l_img, l_gt, _) in enumerate(itertools.islice(lab, 2)):
            loss = sm.step(l_img, l_gt)
            srecs.append(dict(getattr(sm, "extras", {}), loss=loss))
            print("supervised step %d issued: %d launches, %d reports so far" % (s, rc.CORE.launches, len(rc.CORE.reports)), flush=True)
        torch.cuda.synchronize()
        srecs = [_floats(r) for r in srecs]
        print("supervised losses finite:", all(v == v and abs(v) != float("inf") for rec in srecs for v in rec.values()))
        for s, rec in enumerate(srecs):
            print("supervised step %d: %s" % (s, " ".join("%s=%.6g" % (k, rec[k]) for k in sorted(rec))))
        snorms = _norm_rows((("supervised Gsi", sm.gsi_optimizer),))
        scounts = {k: v - seen.get(k, 0) for k, v in lib.counts.items()}
        sentries = tuple(e for e in SO.ENTRIES[name] if e not in SO.UNLABELLED_ENTRIES)
        print("supervised census: %s" % " ".join("%s=%d" % (e, scounts.get(e, 0)) for e in sentries))
        print("supervised phase:")
        print("racecheck: %d launches, %d streams, %d distinct reports" % (core.launches - launched, len(core.vc), len(core.order) - before))
        print("\n".join(core.summary().split("\n")[1 + before:]))
        bad += len(core.order) - before
        try:
            skeys = SO.SUPERVISED_EXTRAS if SO.EXTRA_KEYS[name] else ()
            SO.check_not_vacuous(name, srecs, scounts, snorms, entries=sentries, keys=skeys, shares=("ohem_kept",))
        except AssertionError as e:
            print(e, flush=True)
            vacuous = True
        if not vacuous:
            print("options %s: not vacuous" % name, flush=True)
    return 1 if bad else 2 if vacuous else 0
