#!/usr/bin/env python
"""Training steps with --unl_teacher (mse=1,ce=0.5,thresh=T,flip under --ema_decay 0.9; ACDC's 4 classes, 64x64, batch 2, ngf = ndf = 8,
seeded initial weights, synthetic batches).
usage: python tests/aids/teacher_step.py <mode> [checkpoint dir]
  check  three overlapped steps under the stream-ordering checker (SSCG_RACECHECK=1): every extra key present and finite at every step,
         unl_teacher_kept and unl_teacher_agree strictly inside (0, 1), sscg_teacher_fwd launched once per step, _teacher_logits leaves
         every parameter, buffer, EMA value and operand copy bit-identical and equals a separately computed Gsi.eval() forward under
         ema_weights(), and the checker's report is clean;
  fuzz   the serial one-stream run against one fuzzed multi-stream schedule (SSCG_FUZZ=1, racecheck.fuzz(seed)): the same bits on
         every loss of every step, on the trained weights, the BatchNorm state and the EMA arena;
  grid   what T was read off: per step the kept share and the agreement at a grid of thresholds, from the step's own logits.
Every mode runs WARM steps before the STEPS = 3 steps whose shares are checked: a freshly initialised teacher in evaluation mode
normalises with BatchNorm's initial running statistics and predicts near-uniform maps (every confidence below 0.26 of 4 classes at the
first step), and two steps later its least confident pixel is above 0.32 - no one threshold keeps a share strictly inside (0, 1) on
all of the first three steps, with these weights or with the 21-class keyed ones (profiles/unl_teacher.txt has both grids).  After the
warm-up the confidences spread and T is read off the grid of the three steps that follow.  The keys must be present and finite at
every step, the warm-up included.  Prints `teacher step: ok` and exits 0, or exits 1 with what failed."""
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
rc = importlib.import_module(PKG_NAME + "._lib").dev_tool("racecheck")
CKPT = sys.argv[2] if len(sys.argv) > 2 else "/tmp/sscg_teacher_step"
T = 0.5                 # the teacher's confidence threshold: read off `grid`, see the docstring
SPEC = "mse=1,ce=0.5,thresh=%g,flip" % T
WARM, STEPS, SIZE, BATCH = 1, 3, 64, 2
EXTRA = ("unl_teacher_mse", "unl_teacher_ce", "unl_teacher_kept", "unl_teacher_agree")
dev = torch.device("cuda", 0)
data = importlib.import_module(PKG_NAME + ".data")


def make_args():
    return FX.make_args(dataset="acdc", crop_height=SIZE, crop_width=SIZE, batch_size=BATCH, gpu_ids=[0], ngf=8, ndf=8, checkpoint_dir=CKPT,
                        as_written=True, ema_decay=0.9, unl_teacher=SPEC)


def make_batches():
    torch.manual_seed(23)
    with contextlib.redirect_stdout(io.StringIO()):
        labeled, unlabeled, _ = data.synthetic_loaders(make_args(), 4, steps=4)
    return [(l_img.to(dev), l_gt.to(dev), unl_img.to(dev)) for (l_img, l_gt, _), (unl_img, _, _) in zip(labeled, unlabeled)]


batches = make_batches()


def build(serial=False):
    args = make_args()
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
    print("teacher step: FAILED: " + msg, flush=True)
    sys.exit(1)


def state_of(m):
    """clones of everything _teacher_logits must leave alone"""
    o = m.g_optimizer
    out = {"arena": o.arena.clone(), "ema": o.ema.clone() if o.ema is not None else None,
           "bf16 shadow": o.arena16.clone() if o.arena16 is not None else None,
           "split planes": o.arena_x3.clone() if o.arena_x3 is not None else None}
    for net_name in ("Gsi", "Gis"):
        net = getattr(m, net_name)
        for k, p in net.named_parameters():
            out["%s.%s" % (net_name, k)] = p.detach().clone()
        for k, b in net.named_buffers():
            out["%s.%s (buffer)" % (net_name, k)] = b.detach().clone()
    return out


def check_extras(outs):
    """every step: the keys, finite; the STEPS steps after the warm-up: the shares strictly inside (0, 1)"""
    recs = [{k: float(v) for k, v in o.items()} for o in outs]
    for s, rec in enumerate(recs):
        print("step %d: %s" % (s, " ".join("%s=%.6g" % (k, rec[k]) for k in sorted(rec) if k not in md.LOSS_KEYS)), flush=True)
        for k in EXTRA:
            if k not in rec or not math.isfinite(rec[k]):
                fail("step %d: %s is missing or not finite: %r" % (s, k, rec.get(k)))
        if not all(math.isfinite(v) for v in rec.values()):
            fail("step %d: a loss is not finite: %r" % (s, rec))
        for k in ("unl_teacher_kept", "unl_teacher_agree"):
            if s >= WARM and not 0.0 < rec[k] < 1.0:
                fail("step %d: %s = %r is not strictly inside (0, 1) at thresh %g" % (s, k, rec[k], T))


def mode_check():
    m = build()
    # ---- _teacher_logits on its own: it changes nothing and equals the plain evaluation forward under the averaged weights
    unl_img = batches[0][2]
    m.g_optimizer.ensure_operand_copies()
    m.g_optimizer._ema_sync()            # (the EMA arena exists from the first look at it: a copy of the weights)
    torch.cuda.synchronize()
    before = state_of(m)
    was_training = m.Gsi.training
    got = m._teacher_logits(unl_img)
    F.flush_side_work()
    torch.cuda.synchronize()
    after = state_of(m)
    if m.Gsi.training != was_training or not was_training:
        fail("_teacher_logits left Gsi in %s mode" % ("training" if m.Gsi.training else "evaluation"))
    if got.requires_grad or got.dtype != torch.float32:
        fail("_teacher_logits returned %s, requires_grad=%s" % (got.dtype, got.requires_grad))
    for k in before:
        a, b = before[k], after[k]
        if (a is None) != (b is None) or (a is not None and not torch.equal(a, b)):
            fail("_teacher_logits changed %s" % k)
    with m.g_optimizer.ema_weights(), torch.no_grad():
        m.Gsi.eval()
        want = m.Gsi(unl_img).float()
        m.Gsi.train()
    if not torch.equal(got, want):
        fail("_teacher_logits differs from the evaluation forward under ema_weights(): max-abs %g" % float((got - want).abs().max()))
    print("_teacher_logits: %d tensors unchanged, equal to the evaluation forward under the EMA weights" % len(before), flush=True)
    # ---- three steps, no host synchronisation between them
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
    n = F.lib.counts.get("sscg_teacher_fwd", 0) - seen.get("sscg_teacher_fwd", 0)
    if n != WARM + STEPS:
        fail("sscg_teacher_fwd was launched %d times in %d steps" % (n, WARM + STEPS))
    core = rc.report(sys.stdout)
    if core.reports:
        fail("the stream-ordering checker reported %d conflicts" % len(core.reports))


def run_fuzz(serial, seed):
    m = build(serial)
    rc.fuzz(seed, busy=seed is not None)
    outs = [m.step(*batches[s % len(batches)]) for s in range(WARM + STEPS)]
    rc.fuzz(None)
    m.sync_losses()
    F.flush_side_work()
    torch.cuda.synchronize()
    F.SideStream.enabled = True
    keys = sorted(outs[0])
    rec = {"loss " + k: torch.stack([o[k].float() for o in outs]).view(torch.int32).cpu() for k in keys}
    rec["G arena"] = m.g_optimizer.arena.view(torch.int32).clone()
    rec["D arena"] = m.d_optimizer.arena.view(torch.int32).clone()
    rec["EMA arena"] = m.g_optimizer.ema.view(torch.int32).clone()
    rec["BN state"] = torch.cat([b.detach().float().reshape(-1) for net in (m.Gis, m.Gsi) for b in net.buffers()
                                 if b.dtype.is_floating_point]).view(torch.int32).clone()
    if serial:
        check_extras(outs)
        if F.lib.counts.get("sscg_teacher_fwd", 0) != WARM + STEPS:
            fail("the serial run launched sscg_teacher_fwd %d times" % F.lib.counts.get("sscg_teacher_fwd", 0))
    return rec


def mode_fuzz():
    ref = run_fuzz(True, None)
    rc.FUZZ["sleeps"] = 0
    got = run_fuzz(False, 3)
    diff = [k for k in ref if k not in got or not torch.equal(ref[k], got[k])]
    print("fuzzed schedule (seed 3, %d sleeps): %d records, %s" % (rc.FUZZ["sleeps"], len(ref), "same" if not diff else "DIFFER: " + ", ".join(diff)),
          flush=True)
    if diff:
        fail("the fuzzed schedule differs from the serial run on " + ", ".join(diff))
    if not rc.FUZZ["sleeps"]:
        fail("the fuzzer queued no sleep: the schedule was not fuzzed")


def mode_grid():
    m = build(serial=True)
    inner = F.upsample_softmax_teacher
    grid = (0.26, 0.28, 0.3, 0.32, 0.34, 0.36, 0.38, 0.4, 0.45, 0.5, 0.6, 0.7, 0.8, 0.9)
    rows = []

    def spy(x, size, t, teacher, unl=None, flip=None, **k):
        row = []
        for tau in grid:
            sums = F.teacher_fwd(F.to_nhwc(x.detach()), F.to_nhwc(t), flip, size, teacher.inv_temp, tau, False, False)[1].cpu()
            row.append((float(sums[3]) / (x.shape[0] * size[0] * size[1]), float(sums[1]) / max(float(sums[3]), 1.0)))
        rows.append(row)
        return inner(x, size, t, teacher, unl, flip=flip, **k)
    F.upsample_softmax_teacher = spy
    outs = [m.step(*batches[s % len(batches)]) for s in range(WARM + STEPS)]
    m.sync_losses()
    torch.cuda.synchronize()
    print("thresh  " + "  ".join("step %d kept / agree" % s for s in range(WARM + STEPS)))
    for i, tau in enumerate(grid):
        print("%-6g  " % tau + "  ".join("%10.4f / %-6.4f" % rows[s][i] for s in range(WARM + STEPS)))
    check_extras(outs)


{"check": mode_check, "fuzz": mode_fuzz, "grid": mode_grid}[MODE]()
print("teacher step: ok", flush=True)
