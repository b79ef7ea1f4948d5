"""A run stopped at a checkpoint and started again continues the run that was never stopped.

The state that has to survive a resume is spread over the flat parameter arenas, both moment arenas and the step counter, the EMA
arena, the bf16 shadow / split planes, the cached transposed copies, the BatchNorm running statistics and the optimisers'
`param_groups`.  Two instances in one process compute the same bits (test_semisupervised_step_with_options and the schedule tests
rely on it), so every comparison of a resumed run R with the uninterrupted run U is equality of bits.  The uninterrupted run itself
is held against torch's Adam / AdamW in fp64 restored from the same file, within test_optim_options_gpu.py's TOL, and the same fp64
reference restored WRONGLY (step counter restarted, moments zeroed) has to end at least 100 TOL away: the check can see a wrong
restore.

C1 / C2 / C3 run on the small two-net Rig of test_operand_copies_gpu.py (every kind of operand copy, well under a second per step);
C4 / C5 run the two trainers through their own constructors and train().  Host-side file format: tests/test_checkpoint_host.py."""
import contextlib
import io
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import load_sub
from test_operand_copies_gpu import Rig, _mode
from test_optim_options_gpu import TOL

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
LR = 5e-3           # of the Rig's two FusedAdams here: see test_rig_run_is_adams_and_a_wrong_restore_would_show
OPTION_SETS = {
    "plain": (dict(lr=LR), dict(lr=LR)),
    # decoupled weight decay, EMA, and a clip far below the gradient norms of the Rig's two losses (asserted: _clip < 1)
    "all": (dict(lr=LR, weight_decay=0.1, decoupled=True, max_grad_norm=1e-4, ema_decay=0.9),
            dict(lr=LR, weight_decay=0.1, decoupled=True, max_grad_norm=1e-4, ema_decay=0.9)),
}


def bits(t):
    t = t.detach()
    return t.view(torch.int16 if t.dtype == BF else torch.int32) if t.is_floating_point() else t


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _capture(fn, *a, **k):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        r = fn(*a, **k)
    return r, out.getvalue()


def first_difference(a, b):
    """The first key of two {name: tensor-or-number} snapshots whose values differ in a bit (None: they are equal)."""
    assert list(a) == list(b), (list(a), list(b))
    for k in a:
        x, y = a[k], b[k]
        if torch.is_tensor(x) != torch.is_tensor(y) or (not same(x, y) if torch.is_tensor(x) else x != y):
            return k
    return None


# ------------------------------------------------------------------------------------------ the Rig: snapshots, files
def rig_inputs(n_steps, seed=1234):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(2, 21, 16, 16, generator=g) for _ in range(2 * n_steps)]


def _opt_state(name, opt, out, lr=True):
    for a in ("arena", "exp_avg", "exp_avg_sq", "ema"):
        t = getattr(opt, a)
        if t is not None:
            out["%s.%s" % (name, a)] = t.detach().clone()           # the WHOLE arena: the padding between the slices included
    out[name + "._steps"] = opt._steps
    if lr:
        out[name + ".lr"] = opt.param_groups[0]["lr"]


def rig_snapshot(rig):
    torch.cuda.synchronize()
    out = {"w." + n: w.detach().clone() for n, w in rig.weights().items()}
    for tag, net in (("g", rig.g), ("d", rig.d), ("stock", rig.stock)):
        out.update({"sd.%s.%s" % (tag, k): v.detach().clone() for k, v in net.state_dict().items()})
    _opt_state("g_opt", rig.g_opt, out)
    _opt_state("d_opt", rig.d_opt, out)
    for i, st in enumerate(rig.s_opt.state.values()):
        out.update({"s_opt.%d.%s" % (i, k): v.detach().clone() for k, v in st.items()})
    return out


def rig_save(utils, rig, path):
    """The three nets' and the three optimisers' state_dict()s and the EMA dicts, through utils.save_checkpoint.  The frozen conv goes
    into the file too: the models' frozen networks (old_*) come from a file of their own, the Rig's has no other source."""
    ck = {"g": rig.g.state_dict(), "d": rig.d.state_dict(), "stock": rig.stock.state_dict(), "frozen": rig.frozen.state_dict(),
          "g_opt": rig.g_opt.state_dict(), "d_opt": rig.d_opt.state_dict(), "s_opt": rig.s_opt.state_dict()}
    if rig.g_opt.ema_decay is not None:
        ck["g_ema"], ck["d_ema"] = rig.g_opt.ema_state_dict(rig.g), rig.d_opt.ema_state_dict(rig.d)
    utils.save_checkpoint(ck, path)


def rig_load(utils, rig, path):
    ck, printed = _capture(utils.load_checkpoint, path)
    assert "succeed" in printed
    for k in ("g", "d", "stock", "frozen"):
        getattr(rig, k).load_state_dict(ck[k], strict=True)
    rig.g_opt.load_state_dict(ck["g_opt"])
    rig.d_opt.load_state_dict(ck["d_opt"])
    rig.s_opt.load_state_dict(ck["s_opt"])
    if rig.g_opt.ema_decay is not None:
        rig.g_opt.load_ema_state_dict(rig.g, ck["g_ema"])
        rig.d_opt.load_ema_state_dict(rig.d, ck["d_ema"])
    return ck


def record_gradients(opt, grads, states, net):
    """Wrap opt.step(): the gradient arena's slices are cloned before every update, parameters / moments / EMA after it."""
    real = opt.step
    named = list(net.named_parameters())

    def step():
        torch.cuda.synchronize()
        grads.append([opt._view(opt.grad, p, opt.slices[p][0]).detach().clone().cpu() for _, p in named])
        real()
        torch.cuda.synchronize()
        states.append({"param": [p.detach().clone().cpu() for _, p in named],
                       "exp_avg": [opt._view(opt.exp_avg, p, opt.slices[p][0]).clone().cpu() for _, p in named],
                       "exp_avg_sq": [opt._view(opt.exp_avg_sq, p, opt.slices[p][0]).clone().cpu() for _, p in named],
                       "ema": [opt._view(opt.ema, p, opt.slices[p][0]).clone().cpu() for _, p in named] if opt.ema is not None else None,
                       "clip": None if opt._clip is None else float(opt._clip)})
    opt.step = step


# ------------------------------------------------------------------------------------------ the fp64 reference of C2
def reference_run(net_sd, opt_sd, ema_sd, names, grads, kw, wrong=None):
    """torch.optim.Adam / AdamW in fp64 on the host, restored from the FILE's stock-format optimiser state, fed the gradients the fused
    optimiser used; clip_grad_norm_ in front and ema.lerp_ behind, as test_fused_adam_all_options_match_torch does.
    wrong = "step0": the step counter restarted at 0; "moments0": both moments zeroed - what a broken restore would compute.
    Returns per step {param, exp_avg, exp_avg_sq, ema} as lists in `names` order."""
    ps = [torch.nn.Parameter(net_sd[n].detach().double().cpu().clone()) for n in names]
    cls = torch.optim.AdamW if kw.get("decoupled") else torch.optim.Adam
    ref = cls(ps, lr=1.0, betas=(0.5, 0.999), weight_decay=kw.get("weight_decay", 0.0))
    group = dict(ref.param_groups[0])
    group.update(opt_sd["param_groups"][0])                 # lr, betas, eps of the file (FusedAdam keeps its options out of the groups)
    group["params"] = list(range(len(ps)))
    state = {i: {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in st.items()} for i, st in opt_sd["state"].items()}
    assert sorted(state) == list(range(len(ps)))            # every parameter of the Rig's nets has received a gradient
    for st in state.values():
        if wrong == "step0":
            st["step"] = torch.zeros_like(st["step"])
        elif wrong == "moments0":
            st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(st["exp_avg"]), torch.zeros_like(st["exp_avg_sq"])
    ref.load_state_dict({"state": state, "param_groups": [group]})
    assert all(ref.state[p]["exp_avg"].dtype == torch.float64 for p in ps)
    ema = [ema_sd[n].detach().double().cpu().clone() for n in names] if ema_sd is not None else None
    out = []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.double().clone()
        if kw.get("max_grad_norm") is not None:
            torch.nn.utils.clip_grad_norm_(ps, kw["max_grad_norm"])
        ref.step()
        if ema is not None:
            for e, p in zip(ema, ps):
                e.lerp_(p.detach(), 1.0 - kw["ema_decay"])
        out.append({"param": [p.detach().clone() for p in ps], "exp_avg": [ref.state[p]["exp_avg"].clone() for p in ps],
                    "exp_avg_sq": [ref.state[p]["exp_avg_sq"].clone() for p in ps],
                    "ema": [e.clone() for e in ema] if ema is not None else None})
    return out


def _distance(a, b, key):
    return max(rel_err(x, y) for x, y in zip(a[key], b[key]))


# ------------------------------------------------------------------------------------------ C1 + C2
class _Runs(object):
    pass


@pytest.fixture(scope="module", params=[(m, o) for m in ("f32s", "bf16", "f32x") for o in ("plain", "all")], ids=lambda p: "%s-%s" % p)
def rig_runs(request, F, dev, tmp_path_factory):
    """The runs C1 and C2 look at, made once per (mode, option set).  Run U: 4 steps.  Run R: 2 steps, save through
    utils.save_checkpoint, a NEW Rig from another seed (every initial value differs), load through utils.load_checkpoint, 2 more steps
    on inputs 3 and 4 - the gradients the fused optimisers used there and the state after each update are recorded.  The Rig's own
    coherence checks run after the load and around each step (they raise); nothing else is asserted here."""
    mode, options = request.param
    utils = load_sub("utils")
    g_kw, d_kw = OPTION_SETS[options]
    inputs = rig_inputs(4)
    path = str(tmp_path_factory.mktemp("rig") / "rig.ckpt")
    x = _Runs()
    x.mode, x.options, x.g_kw, x.d_kw = mode, options, g_kw, d_kw
    with _mode(F, mode):
        u = Rig(F, dev, seed=0, g_kw=g_kw, d_kw=d_kw, inputs=inputs)
        x.u_after = {}
        for s in range(4):
            u.step()
            x.u_after[s + 1] = rig_snapshot(u)
        x.u_clips = [None if o._clip is None else float(o._clip) for o in (u.g_opt, u.d_opt)]
        r0 = Rig(F, dev, seed=0, g_kw=g_kw, d_kw=d_kw, inputs=inputs)
        r0.step()
        r0.step()
        x.at_save = rig_snapshot(r0)
        rig_save(utils, r0, path)
        r = Rig(F, dev, seed=1, g_kw=g_kw, d_kw=d_kw, inputs=inputs)
        x.fresh = rig_snapshot(r)
        x.n_weights = len(r.weights())
        x.ck = rig_load(utils, r, path)
        x.state_left = bool(r.g_opt.state) or bool(r.d_opt.state)
        r.replay(2)
        r.check()
        x.loaded = rig_snapshot(r)
        x.rec = {}
        for name, opt, net in (("g", r.g_opt, r.g), ("d", r.d_opt, r.d)):
            x.rec[name] = ([], [])
            record_gradients(opt, x.rec[name][0], x.rec[name][1], net)
        x.r_after = {}
        for s in (3, 4):
            r.step()
            x.r_after[s] = rig_snapshot(r)
        r.refresh()
        x.names = {name: [n for n, _ in getattr(r, name).named_parameters()] for name in ("g", "d")}
    return x


def test_rig_resume_continues_the_uninterrupted_run(rig_runs):
    """C1.  R equals U bit for bit in every weight, the whole arena / exp_avg / exp_avg_sq / ema of both optimisers (padding
    included), `_steps`, `param_groups[0]["lr"]` and the stock Adam's state - right after the load (against the first Rig at its
    save), after step 3 and after step 4.  If they differ, the first unequal item - after the load, then after one step - names what
    was not restored."""
    x = rig_runs
    tag = "rig %s/%s" % (x.mode, x.options)
    assert first_difference(x.at_save, x.u_after[2]) is None        # (two instances, same bits: the premise of everything below)
    differing = [k for k in x.fresh if k.startswith("w.") and not same(x.fresh[k], x.at_save[k])]
    assert len(differing) == x.n_weights                            # the second Rig started from other values everywhere
    n_t = sum(torch.is_tensor(v) for v in x.loaded.values())
    diff = first_difference(x.loaded, x.at_save)
    print("%s: after the load %d tensors + 4 numbers compared with the run at its save: first difference %r" % (tag, n_t, diff))
    assert diff is None, "right after the load: %s" % diff
    assert x.loaded["g_opt._steps"] == 2 and x.loaded["d_opt._steps"] == 2 and x.loaded["g_opt.lr"] == LR and x.loaded["d_opt.lr"] == LR
    assert not x.state_left                                         # no second device copy of the moments is left behind
    for s in (3, 4):
        diff = first_difference(x.r_after[s], x.u_after[s])
        print("%s: after step %d first difference from the uninterrupted run: %r" % (tag, s, diff))
        assert diff is None, "after step %d: %s" % (s, diff)
    if x.options == "all":
        clips = [st["clip"] for name in x.rec for st in x.rec[name][1]]
        print("%s: clip coefficients of steps 3, 4 (G, D): %s; of the uninterrupted run's step 4: %s" % (tag, clips, x.u_clips))
        assert all(c < 1.0 for c in clips + x.u_clips)


def test_rig_run_is_adams_and_a_wrong_restore_would_show(rig_runs):
    """C2.  The stock-format optimiser state of the SAME file goes into torch's Adam / AdamW in fp64, which is fed the gradients the
    fused optimisers used at steps 3 and 4; parameters, both moments and the EMA agree within test_optim_options_gpu.py's TOL after
    each step.  Then the power of that check, on the host: the same reference restored with the step counter at 0, and with zeroed
    moments, must end >= 100 TOL from the correct one in the parameters.  Why lr = 5e-3 and not the Rig's 2e-4: with betas (0.5,
    0.999) the bias corrections of step 3 and of step 1 nearly cancel ((0.875 / 0.5) * sqrt(0.001 / 0.002997) = 1.011) and those of
    step 4 and step 2 differ by 12 %.  A restarted counter therefore moves a parameter by about a tenth of the two updates, each ~lr:
    at 2e-4 that is ~2e-5, which against weights of ~0.1 is only of the order of 100 TOL; at 5e-3 the margin no longer hangs on the
    weights' scale (measured: 3e4 TOL and more for the counter, 3e5 TOL and more for the moments)."""
    x = rig_runs
    tag = "rig %s/%s" % (x.mode, x.options)
    for name, kw in (("g", x.g_kw), ("d", x.d_kw)):
        grads, got = x.rec[name]
        names, ck = x.names[name], x.ck
        args = (ck[name], ck[name + "_opt"], ck.get(name + "_ema"), names, grads, kw)
        ref = reference_run(*args)
        keys = ["param", "exp_avg", "exp_avg_sq"] + (["ema"] if kw.get("ema_decay") is not None else [])
        for s in range(2):
            dist = {k: _distance(got[s], ref[s], k) for k in keys}
            print("%s %s_opt step %d against torch fp64 restored from the file, %d tensors each: %s (bound %.0e)" % (
                tag, name, s + 3, len(names), ", ".join("%s %.3e" % kv for kv in dist.items()), TOL))
            assert all(d < TOL for d in dist.values()), (name, s + 3, dist)
        for wrong in ("step0", "moments0"):
            bad = reference_run(*args, wrong=wrong)
            apart = {k: _distance(bad[1], ref[1], k) for k in keys}
            print("%s %s_opt restored wrongly (%s): after step 4 the fp64 reference is %s from the correct one = %.0f x the "
                  "bound in the parameters" % (tag, name, wrong, ", ".join("%s %.3e" % kv for kv in apart.items()), apart["param"] / TOL))
            assert apart["param"] >= 100 * TOL, (name, wrong, apart)


# ------------------------------------------------------------------------------------------ C3
@pytest.mark.parametrize("mode", ["f32s", "bf16"])
def test_rig_reads_between_steps_leave_no_trace(F, dev, mode):
    """C3.  Between the steps of a 3-step run: state_dict() of both optimisers (it clears and refills self.state and synchronises),
    ema_state_dict, a no_grad forward inside `with g_opt.ema_weights():`, the Rig's getter checks.  The trajectory equals the plain
    3-step run (no checks, nothing in between) bit for bit."""
    g_kw, d_kw = OPTION_SETS["all"]
    inputs = rig_inputs(3)
    probe = torch.randn(2, 21, 16, 16, generator=torch.Generator().manual_seed(99)).to(dev).contiguous(memory_format=torch.channels_last)
    with _mode(F, mode):
        plain = Rig(F, dev, seed=0, g_kw=g_kw, d_kw=d_kw, inputs=inputs)
        plain_after = []
        for _ in range(3):
            plain.step(check=False)
            plain_after.append(rig_snapshot(plain))
        busy = Rig(F, dev, seed=0, g_kw=g_kw, d_kw=d_kw, inputs=inputs)
        outs = []
        for s in range(3):
            busy.step()
            g_sd, d_sd = busy.g_opt.state_dict(), busy.d_opt.state_dict()
            assert len(g_sd["state"]) == len(list(busy.g.parameters())) and len(d_sd["state"]) == len(list(busy.d.parameters()))
            ema_sd = busy.g_opt.ema_state_dict(busy.g)
            busy.d_opt.ema_state_dict(busy.d)
            with torch.no_grad(), busy.g_opt.ema_weights():
                g = busy.g
                assert same(g["mid"].weight.detach(), ema_sd["mid.weight"])
                h = busy.stock(busy.frozen(g["mid"](g["stem"](probe))))
                outs.append(g["ragged"](g["head"](g["up"](h))).float().clone())
            busy.check()
            diff = first_difference(rig_snapshot(busy), plain_after[s])
            print("rig %s: after step %d with state_dict / ema_state_dict / EMA forward / getter checks in between, first difference "
                  "from the plain run: %r (%d entries compared)" % (mode, s + 1, diff, len(plain_after[s])))
            assert diff is None, "after step %d: %s" % (s + 1, diff)
        assert bool(torch.isfinite(torch.stack(outs)).all()) and not same(outs[0], outs[2])


# ------------------------------------------------------------------------------------------ C4: the trainers, through their own code
@pytest.fixture()
def bf16_mode():
    F = load_sub("functional")
    F.set_conv_precision("bf16")
    yield F
    F.set_conv_precision("f32")


def _batches(C, H, seed, n=2, names="b"):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(2, 3, H, H, generator=gen), torch.randint(0, C, (2, 1, H, H), generator=gen), [names] * 2) for _ in range(n)]


def _model_snapshot(nets, opts):
    torch.cuda.synchronize()
    out = {"%s.%s" % (k, n): t.detach().clone() for k, net in nets.items() for n, t in net.state_dict().items()}
    for name, opt in opts.items():
        _opt_state(name, opt, out, lr=False)        # (what train() leaves in `lr` is the schedule's position: see the semi-supervised case)
    return out


def _copy_aside(monkeypatch, utils, aside):
    """utils.save_checkpoint also copies each file it writes to `aside`/epoch<N>.ckpt."""
    real = utils.save_checkpoint
    os.makedirs(aside, exist_ok=True)

    def save(state, path):
        real(state, path)
        shutil.copy(path, os.path.join(aside, "epoch%d.ckpt" % state["epoch"]))
    monkeypatch.setattr(utils, "save_checkpoint", save)


def _resume_case(monkeypatch, tmp_path, build, ckpt_name, nets_of, opts_of, loaders, seed):
    """Run U: train() over both epochs, every checkpoint copied aside.  Run R: a fresh model whose checkpoint_dir holds the epoch-1
    file, then train().  Returns what the two runs are compared in."""
    utils = load_sub("utils")
    assert utils.LambdaLR(2, 0, 1).step(0) == 1.0 and utils.LambdaLR(2, 0, 1).step(1) == 1.0       # both epochs at the same rate
    aside = str(tmp_path / "aside")
    _copy_aside(monkeypatch, utils, aside)
    torch.manual_seed(seed)
    (u, args_u), printed = _capture(build, str(tmp_path / "u"))
    assert "No checkpoint!" in printed and u.start_epoch == 0 and u.best_iou == -100
    hist_u, _ = _capture(u.train, args_u, loaders=loaders)
    snap_u = _model_snapshot(nets_of(u), opts_of(u))
    assert os.path.isfile(os.path.join(aside, "epoch1.ckpt")) and len(hist_u) == 4
    saved = torch.load(os.path.join(aside, "epoch1.ckpt"), map_location="cpu", weights_only=True)     # torch's default, no allow-list
    assert saved["epoch"] == 1 and type(saved["best_iou"]) is float and np.isfinite(saved["best_iou"])
    assert all(type(k) is int and type(v) is float for k, v in saved["class_iou"].items())
    os.makedirs(str(tmp_path / "r"))
    shutil.copy(os.path.join(aside, "epoch1.ckpt"), str(tmp_path / "r" / ckpt_name))
    torch.manual_seed(seed)
    (r, args_r), printed = _capture(build, str(tmp_path / "r"))
    assert "succeed!" in printed and "No checkpoint!" not in printed, printed
    assert r.start_epoch == 1 and type(r.best_iou) is float and r.best_iou == saved["best_iou"]
    assert all(not opt.state for opt in opts_of(r).values())
    hist_r, _ = _capture(r.train, args_r, loaders=loaders)
    snap_r = _model_snapshot(nets_of(r), opts_of(r))
    return u, r, hist_u, hist_r, snap_u, snap_r, saved


def _assert_resumed(tag, hist_u, hist_r, snap_u, snap_r):
    n_t = sum(torch.is_tensor(v) for v in snap_u.values())
    diff = first_difference(snap_r, snap_u)
    print("%s: resumed at epoch 1 against the uninterrupted run: %d tensors (weights, running statistics, num_batches_tracked, arenas, "
          "moments, EMA) + %d numbers, first difference %r; epoch-1 loss records %d, equal %s" % (
              tag, n_t, len(snap_u) - n_t, diff, len(hist_r), hist_r == hist_u[2:]))
    assert len(hist_r) == 2 and hist_r == hist_u[2:], (hist_r, hist_u[2:])
    assert diff is None, diff


def test_semisupervised_trainer_resumes_bit_for_bit(F, dev, tmp_path, monkeypatch):
    """C4, semisuper_cycleGAN: VOC, 64x64, batch 2, the default arithmetic (`f32`), overlap_d, --ema_decay, AdamW decay and a clip
    that triggers; two epochs of two steps (the three history pools never fill and stay stateless), a two-batch validation list.
    R (constructed over the epoch-1 file, then train()) equals U (train() over both epochs) bit for bit in the four trained networks'
    state_dict()s, both optimisers' arenas, moments and `_steps`, the EMA, and the loss records of epoch 1.  No test-side copying of
    state: torch.manual_seed before each construction makes the initial networks identical, the frozen old_* (which no checkpoint
    holds) included; no_dropout, because the dropout seeds depend on construction order.
    Out of scope: the schedule position is not checkpointed, here or in the reference - after a resume LambdaLR restarts
    at epoch 0; with make_args' epochs=2, decay_epoch=1 both epochs run at lam = 1 (asserted), so it does not act on a step.  It
    shows in the rate train() leaves behind (U ends at lam(2) = 0, R at lam(1) = 1), which is therefore not compared here; the
    restored `lr` itself is compared in the Rig test above."""
    from oracle import fixtures as FX
    md = load_sub("model")
    C, H = 21, 64

    def build(ckpt_dir):
        args = FX.make_args(dataset="voc2012", crop_height=H, crop_width=H, batch_size=2, gpu_ids=[dev.index or 0], checkpoint_dir=ckpt_dir,
                            as_written=True, no_dropout=True, overlap_d=True, ema_decay=0.9, weight_decay=0.1, adamw=True,
                            clip_grad_norm=1e-3)
        return md.semisuper_cycleGAN(args), args
    loaders = (_batches(C, H, 51), _batches(C, H, 52), _batches(C, H, 53))
    nets_of = lambda m: {k: getattr(m, k) for k in ("Gis", "Gsi", "Di", "Ds")}
    opts_of = lambda m: {"g_optimizer": m.g_optimizer, "d_optimizer": m.d_optimizer}
    np.random.seed(0)
    u, r, hist_u, hist_r, snap_u, snap_r, saved = _resume_case(monkeypatch, tmp_path, build, "latest_semisuper_cycleGAN.ckpt", nets_of,
                                                               opts_of, loaders, 61)
    assert "Gis_ema" in saved and "Gsi_ema" in saved and u.g_optimizer.ema is not None and u.overlap_d
    assert all(float(o._clip) < 1.0 for m in (u, r) for o in (m.g_optimizer, m.d_optimizer))
    assert u.g_optimizer._steps == 4 and r.g_optimizer._steps == 4 and r.d_optimizer._steps == 4
    assert all(p.cur_elements < p.max_elements for p in u.pools)
    frozen = [k for k in ("old_Gis", "old_Gsi", "old_Di") for a, b in zip(getattr(u, k).state_dict().values(), getattr(r, k).state_dict().values())
              if not same(a, b)]
    assert not frozen
    _assert_resumed("semisuper_cycleGAN", hist_u, hist_r, snap_u, snap_r)


def test_supervised_trainer_resumes_bit_for_bit(dev, tmp_path, monkeypatch, bf16_mode):
    """C4, supervised_model: ACDC, 65x65, as in test_supervised_step_with_options, in bf16 mode (which refuses --ngf 8: ngf is 64
    here, the DeepLab generator does not read it), with --ema_decay and a clip that triggers.  The BatchNorm running statistics and
    num_batches_tracked are part of the compared state_dict."""
    from oracle import fixtures as FX
    md = load_sub("model")
    C, H = 4, 65

    def build(ckpt_dir):
        args = FX.make_args(dataset="acdc", crop_height=H, crop_width=H, batch_size=2, gpu_ids=[dev.index or 0], ngf=64,
                            model="supervised_model", checkpoint_dir=ckpt_dir, as_written=True, no_dropout=True, ema_decay=0.9,
                            clip_grad_norm=1e-3)
        return md.supervised_model(args), args
    loaders = (_batches(C, H, 71), None, _batches(C, H, 73))
    u, r, hist_u, hist_r, snap_u, snap_r, saved = _resume_case(monkeypatch, tmp_path, build, "latest_supervised_model.ckpt",
                                                               lambda m: {"Gsi": m.Gsi}, lambda m: {"gsi_optimizer": m.gsi_optimizer}, loaders, 62)
    assert "Gsi_ema" in saved and float(u.gsi_optimizer._clip) < 1.0 and float(r.gsi_optimizer._clip) < 1.0
    assert r.gsi_optimizer._steps == 4 and int(snap_r["Gsi.bn1.num_batches_tracked"]) == 4
    moved = [k for k in snap_u if k.endswith("running_mean")]
    assert moved and all(bool(snap_u[k].abs().max() > 0) for k in moved)
    _assert_resumed("supervised_model (bf16)", hist_u, hist_r, snap_u, snap_r)


# ------------------------------------------------------------------------------------------ C5: failure behaviour
def test_supervised_constructor_on_missing_broken_and_old_files(dev, tmp_path):
    """C5.  No file: start_epoch 0, best_iou -100, "No checkpoint!".  A file whose `Gsi` lacks a key: the constructor raises (it must
    not go on and train over the file).  A file in the old format (numpy.float64 scores): it resumes."""
    from oracle import fixtures as FX
    md, utils = load_sub("model"), load_sub("utils")

    def build(ckpt_dir):
        args = FX.make_args(dataset="acdc", crop_height=65, crop_width=65, batch_size=2, gpu_ids=[dev.index or 0], ngf=8,
                            model="supervised_model", checkpoint_dir=ckpt_dir, as_written=True, no_dropout=True)
        return md.supervised_model(args)
    torch.manual_seed(81)
    a, printed = _capture(build, str(tmp_path / "none"))
    assert "No checkpoint!" in printed and a.start_epoch == 0 and a.best_iou == -100
    sd = {k: v.detach().cpu().clone() for k, v in a.Gsi.state_dict().items()}
    ck = {"epoch": 1, "Gsi": sd, "gsi_optimizer": a.gsi_optimizer.state_dict(), "best_iou": np.float64(0.25),
          "class_iou": {k: np.float64(v) for k, v in enumerate((0.5, float("nan"), 0.25, 0.0))}}
    # ---- a key of Gsi removed
    os.makedirs(str(tmp_path / "broken"))
    gone = "layer1.0.conv1.weight"
    assert gone in sd
    _capture(utils.save_checkpoint, dict(ck, best_iou=0.25, class_iou={}, Gsi={k: v for k, v in sd.items() if k != gone}),
             str(tmp_path / "broken" / "latest_supervised_model.ckpt"))
    with pytest.raises(RuntimeError, match=gone.replace(".", r"\.")):
        _capture(build, str(tmp_path / "broken"))
    # ---- the old numpy format
    os.makedirs(str(tmp_path / "old"))
    torch.save(ck, str(tmp_path / "old" / "latest_supervised_model.ckpt"))
    torch.manual_seed(82)               # other initial weights: what the model holds afterwards came from the file
    b, printed = _capture(build, str(tmp_path / "old"))
    assert "succeed!" in printed and "No checkpoint!" not in printed
    assert b.start_epoch == 1 and type(b.best_iou) is float and b.best_iou == 0.25
    got = b.Gsi.state_dict()
    assert all(same(got[k].cpu(), sd[k]) for k in sd)
    print("supervised_model constructor: no file -> epoch 0; Gsi without %s -> RuntimeError; numpy-format file -> epoch %d, best_iou %r, "
          "%d tensors restored" % (gone, b.start_epoch, b.best_iou, len(sd)))
