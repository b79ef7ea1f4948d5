#!/usr/bin/env python
"""Training steps with --unl_teacher mse=1,ce=0.5,thresh=T,flip --unl_cutmix 1 under --ema_decay 0.9 (tests/aids/teacher_step.py's shape:
ACDC's 4 classes, 64x64, batch 2, ngf = ndf = 8, seeded initial weights, synthetic batches, WARM + STEPS steps).
usage: python tests/aids/teacher_mix_step.py <mode> [checkpoint dir]
  check     overlapped steps under the stream-ordering checker (SSCG_RACECHECK=1): the report is clean; sscg_mix_boxes and
            sscg_teacher_fwd_mix are launched once per step and sscg_teacher_fwd never; the teacher (_teacher_logits) saw the UNMIXED
            batch - mirrored by the step's flip draws - and every later reader (Gsi, the frozen old_Gsi, the D step) saw
            data_utils.augmentations.mix_batch of it under the step's table; every extra key is present and finite and
            unl_cutmix_share lies strictly inside (0, 1);
  fuzz      the serial one-stream run against one fuzzed multi-stream schedule (SSCG_FUZZ=1, racecheck.fuzz(seed)): the same bits on
            every loss of every step, on both arenas, the EMA arena and the BatchNorm state;
  identity  the draw replaced by the identity table (every sample its own partner): the steps give the bits of the same steps with
            --unl_teacher alone, on every loss and on the trained weights - through sscg_teacher_fwd_mix, which is still launched.
Prints `teacher mix step: ok` and exits 0, or exits 1 with what failed."""
import contextlib
import importlib
import io
import math
import os
import sys

MODE = sys.argv[1] if len(sys.argv) > 1 else "check"
if MODE == "check":
    os.environ["SSCG_RACECHECK"] = "1"
elif MODE == "fuzz":
    os.environ.setdefault("SSCG_FUZZ", "1")
import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import PKG_NAME  # noqa: E402
from oracle import fixtures as FX  # noqa: E402

md = importlib.import_module(PKG_NAME + ".model")
F = importlib.import_module(PKG_NAME + ".functional")
A = importlib.import_module(PKG_NAME + ".data_utils.augmentations")
rc = importlib.import_module(PKG_NAME + "._lib").dev_tool("racecheck")
CKPT = sys.argv[2] if len(sys.argv) > 2 else "/tmp/sscg_teacher_mix_step"
T = 0.5                 # tests/aids/teacher_step.py's threshold
SPEC = "mse=1,ce=0.5,thresh=%g,flip" % T
WARM, STEPS, SIZE, BATCH = 1, 3, 64, 2
EXTRA = ("unl_teacher_mse", "unl_teacher_ce", "unl_teacher_kept", "unl_teacher_agree", "unl_cutmix_share")
dev = torch.device("cuda", 0)
data = importlib.import_module(PKG_NAME + ".data")


def make_args(cutmix="1"):
    kw = {"unl_cutmix": cutmix} if cutmix else {}
    return FX.make_args(dataset="acdc", crop_height=SIZE, crop_width=SIZE, batch_size=BATCH, gpu_ids=[0], ngf=8, ndf=8, checkpoint_dir=CKPT,
                        as_written=True, ema_decay=0.9, unl_teacher=SPEC, **kw)


def make_batches():
    torch.manual_seed(23)
    with contextlib.redirect_stdout(io.StringIO()):
        labeled, unlabeled, _ = data.synthetic_loaders(make_args(), 4, steps=4)
    return [(l_img.to(dev), l_gt.to(dev), unl_img.to(dev)) for (l_img, l_gt, _), (unl_img, _, _) in zip(labeled, unlabeled)]


batches = make_batches()


def build(serial=False, cutmix="1"):
    args = make_args(cutmix)
    args.overlap_d = not serial
    args.fork_forward = not serial
    F.SideStream.enabled = not serial
    torch.manual_seed(22)                # the networks' initial weights
    with contextlib.redirect_stdout(io.StringIO()):
        m = md.semisuper_cycleGAN(args)
    np.random.seed(0)
    torch.manual_seed(0)
    torch.cuda.synchronize()
    return m


def fail(msg):
    print("teacher mix step: FAILED: " + msg, flush=True)
    sys.exit(1)


def check_extras(outs, share_inside=True):
    recs = [{k: float(v) for k, v in o.items()} for o in outs]
    for s, rec in enumerate(recs):
        print("step %d: %s" % (s, " ".join("%s=%.6g" % (k, rec[k]) for k in sorted(rec) if k not in md.LOSS_KEYS)), flush=True)
        for k in EXTRA:
            if k not in rec or not math.isfinite(rec[k]):
                fail("step %d: %s is missing or not finite: %r" % (s, k, rec.get(k)))
        if not all(math.isfinite(v) for v in rec.values()):
            fail("step %d: a loss is not finite: %r" % (s, rec))
        if share_inside and not 0.0 < rec["unl_cutmix_share"] < 1.0:
            fail("step %d: unl_cutmix_share = %r is not strictly inside (0, 1)" % (s, rec["unl_cutmix_share"]))


def launches(name, seen):
    return F.lib.counts.get(name, 0) - seen.get(name, 0)


def mode_check():
    m = build()
    n = BATCH
    seen_views, seen_gsi, seen_old, seen_d, tables = [], [], [], [], []
    inner_logits, inner_table, inner_d = m._teacher_logits, m._cutmix_table, m._d_step
    gsi_forward, old_forward = m.Gsi.forward, m.old_Gsi.forward

    def spy_logits(view):
        seen_views.append(view.detach().clone())
        spy_logits.inside = True
        try:
            return inner_logits(view)
        finally:
            spy_logits.inside = False
    spy_logits.inside = False

    def spy_table(k):
        tables.append(inner_table(k).copy())
        return tables[-1]

    def spy_gsi(x, *a, **k):
        if not spy_logits.inside:                  # (the teacher's own pass goes through Gsi too)
            seen_gsi.append(x.detach()[:n].clone())
        return gsi_forward(x, *a, **k)

    def spy_old(x, *a, **k):
        seen_old.append(x.detach()[:n].clone())
        return old_forward(x, *a, **k)

    def spy_d(a, recon_img, fake_img, fake_gt, unl_img, *rest, **k):
        seen_d.append(unl_img.detach().clone())
        return inner_d(a, recon_img, fake_img, fake_gt, unl_img, *rest, **k)
    m._teacher_logits, m._cutmix_table, m._d_step = spy_logits, spy_table, spy_d
    m.Gsi.forward, m.old_Gsi.forward = spy_gsi, spy_old
    seen = dict(F.lib.counts)
    outs = []
    for s in range(WARM + STEPS):
        outs.append(m.step(*batches[s % len(batches)]))
        rc.name_streams(F, dev)
        print("step %d issued: %d launches, %d reports so far" % (s, rc.CORE.launches, len(rc.CORE.reports)), flush=True)
    m.sync_losses()
    F.flush_side_work()
    torch.cuda.synchronize()
    check_extras(outs)
    steps = WARM + STEPS
    for name, want in (("sscg_mix_boxes", steps), ("sscg_teacher_fwd_mix", steps), ("sscg_teacher_fwd", 0)):
        if launches(name, seen) != want:
            fail("%s was launched %d times in %d steps, expected %d" % (name, launches(name, seen), steps, want))
    # what the teacher and the student saw: the flip draws and the tables of the steps, replayed on the host
    rng = torch.Generator().manual_seed(md._UnlabelledLosses.TEACHER_SEED)
    if not (len(seen_views) == len(tables) == len(seen_d) == steps and len(seen_old) >= steps):
        fail("spies: %d teacher passes, %d tables, %d frozen passes, %d D steps in %d steps" % (len(seen_views), len(tables), len(seen_old),
                                                                                          len(seen_d), steps))
    gsi_unl = [g for g in seen_gsi if tuple(g.shape) == (n, 3 if g.shape[1] == 3 else g.shape[1], SIZE, SIZE)]
    for s in range(steps):
        unl = batches[s % len(batches)][2]
        draws = (torch.rand(n, generator=rng) < 0.5).tolist()
        view = torch.stack([unl[i].flip(-1) if draws[i] else unl[i] for i in range(n)])
        if not torch.equal(seen_views[s], view):
            fail("step %d: the teacher did not see the UNMIXED batch (mirrored by the step's flip draws %r)" % (s, draws))
        mixed = torch.from_numpy(A.mix_batch(unl.cpu().numpy(), None, tables[s], False)[0]).to(dev)
        if torch.equal(mixed, unl):
            fail("step %d: the table %r mixes nothing" % (s, tables[s].tolist()))
        share = float(outs[s]["unl_cutmix_share"])
        want_share = float((mixed != unl).any(1).sum()) / (n * SIZE * SIZE)
        if share < want_share or share > 1.0:       # (pixels the two samples share by chance do not count as changed)
            fail("step %d: unl_cutmix_share %r, %r of the pixels changed" % (s, share, want_share))
        hits = [g for g in gsi_unl if torch.equal(g, mixed)]
        if not hits or any(torch.equal(g, unl) for g in gsi_unl):
            fail("step %d: Gsi saw the mixed batch %d times (and the unmixed one %d times)" % (s, len(hits), sum(torch.equal(g, unl) for g in gsi_unl)))
        if not any(torch.equal(g, mixed) for g in seen_old) or any(torch.equal(g, unl) for g in seen_old):
            fail("step %d: the frozen generator did not see the mixed batch" % s)
        if not torch.equal(seen_d[s], mixed):
            fail("step %d: the D step did not see the mixed batch" % s)
    print("spies: the teacher saw the unmixed batch, Gsi / old_Gsi / the D step the mixed one, in %d steps" % steps, flush=True)
    core = rc.report(sys.stdout)
    if core.reports:
        fail("the stream-ordering checker reported %d conflicts" % len(core.reports))


def record(m, outs):
    keys = sorted(outs[0])
    rec = {"loss " + k: torch.stack([o[k].float().to(dev) for o in outs]).view(torch.int32).cpu() for k in keys}
    rec["G arena"] = m.g_optimizer.arena.view(torch.int32).clone()
    rec["D arena"] = m.d_optimizer.arena.view(torch.int32).clone()
    rec["EMA arena"] = m.g_optimizer.ema.view(torch.int32).clone()
    rec["BN state"] = torch.cat([b.detach().float().reshape(-1) for net in (m.Gis, m.Gsi) for b in net.buffers()
                                 if b.dtype.is_floating_point]).view(torch.int32).clone()
    return rec


def run_steps(serial, seed, cutmix="1", identity=False, fuzzing=False):
    m = build(serial, cutmix)
    if identity:
        m._cutmix_table = lambda k: np.concatenate([np.arange(k, dtype=np.int32)[:, None], np.zeros((k, 7), dtype=np.int32)], 1)
    before = dict(getattr(F.lib, "counts", {}))
    if fuzzing:
        rc.fuzz(seed, busy=seed is not None)
    outs = [m.step(*batches[s % len(batches)]) for s in range(WARM + STEPS)]
    if fuzzing:
        rc.fuzz(None)
    m.sync_losses()
    F.flush_side_work()
    torch.cuda.synchronize()
    F.SideStream.enabled = True
    return m, outs, before


def mode_fuzz():
    m, outs, before = run_steps(True, None, fuzzing=True)
    check_extras(outs)
    for name, want in (("sscg_mix_boxes", WARM + STEPS), ("sscg_teacher_fwd_mix", WARM + STEPS), ("sscg_teacher_fwd", 0)):
        if launches(name, before) != want:
            fail("the serial run launched %s %d times" % (name, launches(name, before)))
    ref = record(m, outs)
    rc.FUZZ["sleeps"] = 0
    m, outs, _ = run_steps(False, 3, fuzzing=True)
    got = record(m, outs)
    diff = [k for k in ref if k not in got or not torch.equal(ref[k], got[k])]
    print("fuzzed schedule (seed 3, %d sleeps): %d records, %s" % (rc.FUZZ["sleeps"], len(ref), "same" if not diff else "DIFFER: " + ", ".join(diff)),
          flush=True)
    if diff:
        fail("the fuzzed schedule differs from the serial run on " + ", ".join(diff))
    if not rc.FUZZ["sleeps"]:
        fail("the fuzzer queued no sleep: the schedule was not fuzzed")


class _Counting(object):
    """functional.lib with every call counted by name"""

    def __init__(self, inner):
        self._inner, self.counts = inner, {}

    def __getattr__(self, name):
        fn = getattr(self._inner, name)

        def call(*a):
            self.counts[name] = self.counts.get(name, 0) + 1
            return fn(*a)
        return call


def mode_identity():
    if not hasattr(F.lib, "counts"):
        F.lib = _Counting(F.lib)
    m, outs, _ = run_steps(True, None, cutmix="")
    plain = record(m, outs)
    seen = dict(F.lib.counts)
    m, outs, _ = run_steps(True, None, cutmix="1", identity=True)
    check_extras(outs, share_inside=False)
    got = record(m, outs)
    if launches("sscg_teacher_fwd_mix", seen) != WARM + STEPS or launches("sscg_teacher_fwd", seen) != 0 or launches("sscg_mix_boxes", seen) != 0:
        fail("the identity draw launched sscg_teacher_fwd_mix %d, sscg_teacher_fwd %d, sscg_mix_boxes %d times"
             % tuple(launches(k, seen) for k in ("sscg_teacher_fwd_mix", "sscg_teacher_fwd", "sscg_mix_boxes")))
    extra = sorted(set(got) - set(plain))
    if extra != ["loss unl_cutmix_share"] or set(plain) - set(got):
        fail("the records differ in their keys: %r / %r" % (extra, sorted(set(plain) - set(got))))
    if int(got["loss unl_cutmix_share"].abs().max()) != 0:
        fail("the identity draw reports a pasted share")
    diff = [k for k in plain if not torch.equal(plain[k], got[k])]
    print("identity draw against --unl_teacher alone: %d records, %s" % (len(plain), "same" if not diff else "DIFFER: " + ", ".join(diff)), flush=True)
    if diff:
        fail("the identity draw differs from --unl_teacher alone on " + ", ".join(diff))


{"check": mode_check, "fuzz": mode_fuzz, "identity": mode_identity}[MODE]()
print("teacher mix step: ok", flush=True)
