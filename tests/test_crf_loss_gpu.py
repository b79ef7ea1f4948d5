"""The gated CRF loss on the MI355X: sscg_crf_loss_fwd (csrc/crf_loss.hip) against the fp64 numpy restatement of its definition
(tests/crf_loss_reference.py, checked on its own in tests/test_crf_loss_host.py), the exact cases, the bit identities inside this
build, the autograd node and the training step, at the shapes of tests/test_crf_gpu.py's CASES.

Accuracy.  The reference has no such loss, so the outputs are held to the fp64 restatement.  Per case the same restatement also runs in
numpy fp32, and e32, its distance from fp64 for the same output, scales the bound, in test_crf_gpu.py's form  gpu <= 8 * e32 + floor
(the operations are the same: expf plus compiler-formed FMAs):
  coef    e32 = max |coef_np32 - coef_fp64| over the elements; floor 2e-6 * min(1, |s| * max ksum), 2e-6 of the output's full scale.
  loss    e32 = |loss_np32 - loss_fp64|; floor 2e-6 * min(1, mean ksum) (the loss lies in [0, mean ksum]).
  sums    fp64 [2]: e32 = |sum_np32 - sum_fp64| of the per-pixel e and ksum; the loss's floor times M.
The test prints e32, the GPU's distance and their ratio per case and output; profiles/crf_loss.txt keeps the figures of the first
MI355X run with these distances (the largest ratios: see section 4 there); the factor 8 stands as test_crf_gpu.py has it."""
import contextlib
import ctypes as C
import functools
import io
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import crf_loss_reference as LR
import crf_reference as R
from conftest import ROOT, load_sub
from test_crf_gpu import CASES, SETS

pytestmark = pytest.mark.gpu
GUARD = 64
SENT = {torch.float32: float("nan"), torch.float64: float("nan"), torch.uint8: 0xEE}


@functools.lru_cache(maxsize=None)
def reference(case, pset):
    """Inputs and the fp64 / fp32 restatements of one case, computed once and shared (read-only) by the tests that need them."""
    (N, H, W, Cn, OH, OW, r, d, _), seed, IC = CASES[case]
    p, img = LR.case_inputs(seed, N, H, W, Cn, OH, OW, IC)
    r64 = LR.crf_loss(p, img, r, d, np.float64, **SETS[pset])
    r32 = LR.crf_loss(p, img, r, d, np.float32, **SETS[pset])
    for a in (p, img) + tuple(v for v in r64.values() if isinstance(v, np.ndarray)):
        a.setflags(write=False)
    M = r64["M"]
    kbar, kmax = r64["sums"][1] / M, float(r64["ksum"].max())
    s = abs(float(np.float32(-2.0 / M)))
    e32 = dict(coef=float(np.abs(r32["coef"].astype(np.float64) - r64["coef"]).max()),
               loss=abs(float(r32["loss"]) - float(r64["loss"])), sum_e=abs(r32["sums"][0] - r64["sums"][0]),
               sum_k=abs(r32["sums"][1] - r64["sums"][1]),
               s_ksum=float(np.abs((np.float32(-2.0 / M) * r32["ksum"]).astype(np.float64) - float(np.float32(-2.0 / M)) * r64["ksum"]).max()))
    floor = dict(coef=2e-6 * min(1.0, s * kmax), loss=2e-6 * min(1.0, kbar), sum_e=2e-6 * min(1.0, kbar) * M, sum_k=2e-6 * min(1.0, kbar) * M)
    return dict(p=p, img=img, r=r, d=d, ref=r64, e32=e32, floor=floor, M=M, s=np.float32(-2.0 / M))


def options(F, ref, pset, **over):
    return F.CrfOptions(**dict(dict(radius=ref["r"], dilation=ref["d"], **SETS[pset]), **over))


def guarded(n, dtype, dev, fill=None):
    """(buffer, view of n elements GUARD elements into it): the guard bands hold the sentinel of the dtype, the view `fill` (or it too)."""
    buf = torch.full((n + 2 * GUARD,), SENT[dtype], dtype=dtype, device=dev)
    if fill is not None:
        buf[GUARD:GUARD + n] = fill
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf):
    g = torch.cat([buf[:GUARD], buf[-GUARD:]])
    return bool(torch.isnan(g).all()) if buf.is_floating_point() else bool((g == SENT[buf.dtype]).all())


def raw(L, p, img, opts, dev, *, want_coef=True, ws_byte=0xFF):
    """sscg_crf_loss_fwd itself on p [N,OH,OW,C] / img [N,OH,OW,IC] device tensors: every output and the workspace are views into
    sentinel-filled buffers whose guard bands must survive (coef starts as NaN: an element the kernel skips stays one); the workspace's
    own bytes are pre-filled with `ws_byte`.  Returns (loss fp32 0-dim, sums fp64 [2], coef [N,OH,OW,C] | None)."""
    N, oh, ow, Cn = p.shape
    need = L.lib.sscg_crf_loss_workspace(N, oh, ow)
    assert need == N * ((oh + 15) // 16) * ((ow + 15) // 16) * 16
    wb, ws = guarded(need, torch.uint8, dev, fill=ws_byte)
    lb, loss = guarded(1, torch.float32, dev)
    sb, sums = guarded(2, torch.float64, dev)
    bufs = [wb, lb, sb]
    coef = None
    if want_coef:
        cb, coef = guarded(N * oh * ow * Cn, torch.float32, dev)
        bufs.append(cb)
    args = (p.data_ptr(), N, oh, ow, Cn, img.data_ptr(), img.shape[3], C.byref(opts.params()), loss.data_ptr(), sums.data_ptr(),
            None if coef is None else coef.data_ptr(), ws.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    assert L.lib.sscg_crf_loss_fwd(*args, need - 1, stream) == -3                      # a workspace one byte short is refused
    rc = L.lib.sscg_crf_loss_fwd(*args, need, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for b in bufs:
        assert guards_intact(b), "a store outside the %s buffer" % b.dtype
    return loss.view(()).clone(), sums.clone(), None if coef is None else coef.view(N, oh, ow, Cn).clone()


def to_dev(ref, dev):
    p, img = torch.tensor(ref["p"], device=dev), torch.tensor(ref["img"], device=dev)          # (copies: the shared arrays are read-only)
    assert p.is_contiguous() and img.is_contiguous()                                       # raw() hands the entry their pointers
    return p, img


# ------------------------------------------------------------------------------------------ 1. loss and coef against fp64
@pytest.mark.parametrize("pset", ["strong", "gentle"])
@pytest.mark.parametrize("case", list(CASES))
def test_loss_and_coef_against_the_fp64_restatement(F, dev, case, pset):
    L = load_sub("_lib")
    ref = reference(case, pset)
    p, img = to_dev(ref, dev)
    loss, sums, coef = raw(L, p, img, options(F, ref, pset), dev)
    r64 = ref["ref"]
    assert not bool(torch.isnan(coef).any()), "a coef element was not written"
    got = dict(coef=float(np.abs(coef.cpu().numpy().astype(np.float64) - r64["coef"]).max()), loss=abs(float(loss) - float(r64["loss"])),
               sum_e=abs(float(sums[0]) - r64["sums"][0]), sum_k=abs(float(sums[1]) - r64["sums"][1]))
    bad = []
    for key in ("coef", "loss", "sum_e", "sum_k"):
        e32, bound = ref["e32"][key], 8.0 * ref["e32"][key] + ref["floor"][key]
        print("[crf_loss] %-28s %-5s e32 %.3e  gpu %.3e  ratio %6.2f  bound %.3e" % ("%s/%s" % (case, pset), key, e32, got[key],
                                                                                      got[key] / e32 if e32 else float("inf"), bound))
        if not got[key] <= bound:
            bad.append("%s: gpu distance %.3e > 8 * e32 + floor = %.3e (e32 %.3e)" % (key, got[key], bound, e32))
    print("[crf_loss] %-28s loss %.9g (fp64 %.9g), mean ksum %.6g" % ("%s/%s" % (case, pset), float(loss), float(r64["loss"]), r64["sums"][1] / ref["M"]))
    assert not bad, "%s/%s: %s" % (case, pset, "; ".join(bad))
    assert float(loss) == float(np.float32(float(sums[0]) / ref["M"]))                  # the loss is the stored sum's quotient, rounded once
    assert float(loss) >= 0.0 and bool((coef <= 0).all())


# ------------------------------------------------------------------------------------------ 2. exact cases
@pytest.mark.parametrize("case", list(CASES))
def test_a_constant_one_hot_map_costs_exactly_nothing(F, dev, case):
    L = load_sub("_lib")
    ref = reference(case, "strong")
    opts = options(F, ref, "strong")
    _, img = to_dev(ref, dev)
    N, oh, ow, Cn = ref["p"].shape
    # ksum of every pixel, from the kernel's own weights: a one-class map of ones has msg = ksum (the run-time class arm).  The entry
    # never hands out ksum per pixel, so the bit equality below holds between two arms of THIS build only (loss == 0 is what pins the hot
    # class's msg to ksum); against the restatement s * ksum is held within tolerance, further down
    _, sums1, coef1 = raw(L, torch.ones(N, oh, ow, 1, device=dev), img, opts, dev)
    s = torch.tensor(ref["s"], device=dev)
    for hot in sorted({0, Cn // 2, Cn - 1}):
        one = torch.zeros(N, oh, ow, Cn, device=dev)
        one[..., hot] = 1.0
        loss, sums, coef = raw(L, one, img, opts, dev)
        assert float(loss) == 0.0 and float(sums[0]) == 0.0 and float(sums[1]) > 0.0
        assert torch.equal(sums[1], sums1[1])
        assert torch.equal(coef[..., hot], coef1[..., 0]), "coef at the hot class is not s * ksum"
        rest = torch.cat([coef[..., :hot], coef[..., hot + 1:]], dim=3)
        assert not bool(rest.any()) and not bool(torch.isnan(rest).any())
    # s * ksum it is: against the restatement's within coef's form of bound (e32 = the numpy-fp32 s * ksum's distance from fp64), and
    # the fp64 sum of coef / s is sums[1]
    err = float(np.abs(coef1[..., 0].cpu().numpy().astype(np.float64) - float(ref["s"]) * ref["ref"]["ksum"]).max())
    print("[crf_loss] %-28s s*ksum e32 %.3e  gpu %.3e  ratio %6.2f" % (case, ref["e32"]["s_ksum"], err, err / ref["e32"]["s_ksum"]))
    assert err <= 8.0 * ref["e32"]["s_ksum"] + ref["floor"]["coef"], err
    assert float((coef1.double() / s.double()).sum()) == pytest.approx(float(sums1[1]), rel=1e-6)


# ------------------------------------------------------------------------------------------ 3. bit identities inside this build
@pytest.mark.parametrize("case", list(CASES))
def test_outputs_agree_with_each_other_bit_for_bit(F, dev, case):
    L = load_sub("_lib")
    ref = reference(case, "strong")
    opts = options(F, ref, "strong")
    p, img = to_dev(ref, dev)
    loss, sums, coef = raw(L, p, img, opts, dev)
    assert not bool(torch.isnan(coef).any())                                 # every element is written (the buffer started as NaN)
    # the value-only call, the same call again, a zeroed workspace in place of one full of 0xFF bytes (NaNs): the same bits
    loss_v, sums_v, none = raw(L, p, img, opts, dev, want_coef=False)
    assert none is None and torch.equal(loss_v, loss) and torch.equal(sums_v, sums)
    loss_2, sums_2, coef_2 = raw(L, p, img, opts, dev)
    assert torch.equal(loss_2, loss) and torch.equal(sums_2, sums) and torch.equal(coef_2, coef)
    loss_z, sums_z, coef_z = raw(L, p, img, opts, dev, ws_byte=0)
    assert torch.equal(loss_z, loss) and torch.equal(sums_z, sums) and torch.equal(coef_z, coef)
    # `iterations` is ignored
    loss_i, _, coef_i = raw(L, p, img, options(F, ref, "strong", iterations=0), dev)
    assert torch.equal(loss_i, loss) and torch.equal(coef_i, coef)
    # a sample's coefficients depend on the batch through s only: msg is the sample's own
    N = p.shape[0]
    if N > 1:
        for n in range(N):
            _, _, c1 = raw(L, p[n:n + 1].contiguous(), img[n:n + 1].contiguous(), opts, dev)
            s1, sN = np.float32(-2.0 / (ref["M"] // N)), ref["s"]          # (one fp32 rounding of each product: 2 * 2^-24 apart)
            assert torch.allclose(c1[0].double() / float(s1), coef[n].double() / float(sN), rtol=2.5e-7, atol=0.0), (case, n)
    # coef / s is the message of one mean-field step of sscg_crf_head on Q = p: softmax(log p + msg) is its Q.  msg <= ksum (at most a
    # few hundred with these weights) comes back from coef / s within 2^-23 relative, some 5e-5 in the exponent: Q within 5e-4
    q = F.crf_labels(p.permute(0, 3, 1, 2), img.permute(0, 3, 1, 2), p.shape[1:3], options(F, ref, "strong", iterations=1), probs=True,
                     want_q=True, want_u8=False)[3].permute(0, 2, 3, 1)
    msg = coef.double() / float(ref["s"])
    want = torch.softmax(torch.log(p.double().clamp_min(1.17549435e-38)) + msg, dim=3)
    assert float((q.double() - want).abs().max()) <= 5e-4
    # the Python entry returns the same bits
    py_loss, py_sums, py_coef = F.crf_loss_fwd(p.permute(0, 3, 1, 2), img.permute(0, 3, 1, 2), opts, True)
    assert torch.equal(py_loss, loss) and torch.equal(py_sums, sums) and torch.equal(py_coef, coef)
    assert F.crf_loss_fwd(p.permute(0, 3, 1, 2), img.permute(0, 3, 1, 2), opts, False)[2] is None


# ------------------------------------------------------------------------------------------ 4. autograd
@pytest.mark.parametrize("case", ["voc21_r3", "acdc4_r3d2_grey", "c33_identity_one_step"])
def test_backward_is_g_times_coef(F, dev, case):
    L = load_sub("_lib")
    ref = reference(case, "strong")
    opts = options(F, ref, "strong")
    p, img = to_dev(ref, dev)
    loss, _, coef = raw(L, p, img, opts, dev)
    probs = p.permute(0, 3, 1, 2).clone().requires_grad_(True)               # logical NCHW, channels-last memory
    image = img.permute(0, 3, 1, 2).clone().requires_grad_(True)
    out = F.crf_loss(probs, image, opts)
    assert out.shape == () and torch.equal(out.detach(), loss)
    g = torch.tensor(0.37, device=dev)
    out.backward(g)
    assert image.grad is None                                                # the image gets no gradient
    assert torch.equal(probs.grad.permute(0, 2, 3, 1), g * coef)
    # a dict of options and a map in NCHW memory give the same bits; no gradient asked for: no coef is kept
    again = F.crf_loss(p.permute(0, 3, 1, 2).contiguous(), image.detach(), dict(radius=ref["r"], dilation=ref["d"], **SETS["strong"]))
    assert torch.equal(again, loss) and not again.requires_grad
    # the defaults (UNTUNED) are CrfOptions()
    assert torch.equal(F.crf_loss(probs.detach(), image.detach()), F.crf_loss(probs.detach(), image.detach(), F.CrfOptions()))


def test_through_the_unlabelled_head_the_gradient_is_the_head_backward_of_g_times_coef(F, dev):
    L = load_sub("_lib")
    (N, H, W, Cn, OH, OW, r, d, _), seed, IC = CASES["voc21_r3"]
    x_np, img_np = R.make_inputs(seed, N, H, W, Cn, OH, OW, IC)
    x = torch.tensor(x_np, device=dev).permute(0, 3, 1, 2).requires_grad_(True)
    image = torch.tensor(img_np, device=dev).permute(0, 3, 1, 2)
    opts = F.CrfOptions(radius=r, dilation=d, **SETS["strong"])
    assert F._head_applies(x, OH, OW)
    soft = F.upsample_softmax_unl(x, (OH, OW))[0]
    loss = F.crf_loss(soft, image, opts)
    g = torch.tensor(1.5, device=dev)
    loss.backward(g)
    # by hand: the head's map, the forward's coef, dy = g * coef, the unlabelled head's backward entry with no loss gradient
    with torch.no_grad():
        xs = F.to_nhwc(x.detach())
        soft2 = F.upsample_softmax_unl(x.detach(), (OH, OW))[0]
        assert torch.equal(soft2, soft.detach())
        _, _, coef = F.crf_loss_fwd(F.to_nhwc(soft2), F.to_nhwc(image), opts, True)
        dy = F._lovasz_upstream(coef, g, None)
        _, sums, _ = F.unl_fwd(xs, (OH, OW), 0.9, False)
        dx = F.empty_nhwc(N, Cn, H, W, dev)
        assert L.lib.sscg_upsample_head_bwd_u(xs.data_ptr(), None, dy.data_ptr(), None, None, None, sums.data_ptr(), dx.data_ptr(), N, H, W,
                                              Cn, OH, OW, F._stream()) == 0
    torch.cuda.synchronize()
    assert float(x.grad.abs().max()) > 0.0 and torch.equal(x.grad, dx)


# ------------------------------------------------------------------------------------------ 5. through the model
def _args(dev, tmp_path, **kw):
    FX = __import__("oracle.fixtures", fromlist=["x"])
    return FX.make_args(dataset="acdc", crop_height=64, crop_width=64, batch_size=2, gpu_ids=[dev.index or 0], ngf=8, ndf=8,
                        checkpoint_dir=str(tmp_path / "ckpt"), as_written=True, **kw)


def test_semisupervised_step_takes_the_flag(F, dev, tmp_path, monkeypatch):
    md, data = load_sub("model"), load_sub("data")
    gen, seen = [], []
    inner_sum, inner_loss = F.weighted_sum, F.crf_loss

    def sum_spy(terms, weights, *a, **k):
        out = inner_sum(terms, weights, *a, **k)
        if len(terms) >= md.GEN_LOSS_BASE_TERMS:
            gen.append((out.detach().clone(), list(weights)))
        return out

    def loss_spy(probs, image, crf=None):
        seen.append((probs.detach().clone(), image.detach().clone(), crf))
        return inner_loss(probs, image, crf)
    monkeypatch.setattr(F, "weighted_sum", sum_spy)
    monkeypatch.setattr(F, "crf_loss", loss_spy)
    got = {}
    for tag, kw in (("off", {}), ("on", dict(unl_crf=0.1, unl_crf_kernel="radius=2,dilation=2")), ("ramp", dict(unl_crf=0.1, unl_ramp=2)),
                    ("with", dict(unl_crf=0.1, unl_entropy=0.2, unl_pseudo=0.3))):
        args = _args(dev, tmp_path, **kw)
        torch.manual_seed(22)
        with contextlib.redirect_stdout(io.StringIO()):
            m = md.semisuper_cycleGAN(args)
            labeled, unlabeled, _ = data.synthetic_loaders(args, 4, steps=1)
        (l_img, l_gt, _), (unl_img, _, _) = next(iter(labeled)), next(iter(unlabeled))
        assert m._unl_scale == (0.0 if tag == "ramp" else 1.0)                 # epoch 0 of a ramp: weight 0
        torch.manual_seed(23)
        del gen[:], seen[:]
        losses = m.step(l_img.to(dev), l_gt.to(dev), unl_img.to(dev))
        m.sync_losses()
        F.flush_side_work()
        torch.cuda.synchronize()
        vals = {k: float(v) for k, v in losses.items()}
        assert all(math.isfinite(v) for v in vals.values()), vals
        assert len(gen) == 1 and len(seen) == (0 if tag == "off" else 1)
        weights = {net + "." + k: v.detach().clone() for net in ("Gis", "Gsi", "Di", "Ds") for k, v in getattr(m, net).state_dict().items()}
        got[tag] = (vals, gen[0], weights, seen[0] if seen else None)
    off, on, ramp, both = got["off"], got["on"], got["ramp"], got["with"]
    assert set(off[0]) == set(md.LOSS_KEYS)                                          # off: the loss keys of before
    assert set(on[0]) - set(md.LOSS_KEYS) == {"unl_crf"} == set(ramp[0]) - set(md.LOSS_KEYS)
    assert set(both[0]) - set(md.LOSS_KEYS) == {"unl_crf", "unl_entropy", "unl_pseudo_ce", "unl_pseudo_kept"}
    assert on[0]["unl_crf"] > 0.0 and ramp[0]["unl_crf"] > 0.0
    # the step handed the loss the head's softmax map, the unlabelled image and the parsed kernel; the key holds its value
    probs, image, crf = on[3]
    assert tuple(probs.shape) == (2, 4, 64, 64) and tuple(image.shape) == (2, 3, 64, 64) and (crf.radius, crf.dilation) == (2, 2)
    assert float(F.crf_loss(probs, image, crf)) == on[0]["unl_crf"] and ramp[3][2] == F.CrfOptions()
    # the term is in the generator loss with weight F * scale: the sum moves by 0.1 * unl_crf when on, by nothing at weight 0
    assert on[1][1][-1] == 0.1 and ramp[1][1][-1] == 0.0 and len(on[1][1]) == len(off[1][1]) + 1 and both[1][1][-3:] == [0.2, 0.3, 0.1]
    assert float(on[1][0]) != float(off[1][0])
    assert float(on[1][0]) - float(off[1][0]) == pytest.approx(0.1 * on[0]["unl_crf"], rel=1e-3)
    assert torch.equal(ramp[1][0], off[1][0])
    # weight 0 (the first epoch of a ramp): every weight after the step equals the flag-off step's, bit for bit; on: Gsi's moved
    assert set(ramp[2]) == set(off[2]) and all(torch.equal(ramp[2][k], off[2][k]) for k in off[2])
    assert any(not torch.equal(on[2][k], off[2][k]) for k in off[2] if k.startswith("Gsi."))


def test_supervised_model_ignores_the_flag(F, dev, tmp_path):
    md = load_sub("model")
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        m = md.supervised_model(_args(dev, tmp_path, model="supervised_model", unl_crf=0.5))
    assert "--unl_crf is ignored" in out.getvalue() and not hasattr(m, "unl_crf")
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        md.supervised_model(_args(dev, tmp_path, model="supervised_model"))
    assert "ignored" not in out.getvalue()


SCRIPT = r"""
import contextlib, io, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
from conftest import load_sub
md, data, F, L = load_sub("model"), load_sub("data"), load_sub("functional"), load_sub("_lib")
FX = __import__("oracle.fixtures", fromlist=["x"])
dev = torch.device("cuda:0")
for tag, kw in (("off", {}), ("on", dict(unl_crf=0.1))):
    a = FX.make_args(dataset="acdc", crop_height=64, crop_width=64, batch_size=2, gpu_ids=[0], ngf=8, ndf=8, checkpoint_dir=%r,
                     as_written=True, **kw)
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        m = md.semisuper_cycleGAN(a)
        labeled, unlabeled, _ = data.synthetic_loaders(a, 4, steps=1)
    (l_img, l_gt, _), (unl_img, _, _) = next(iter(labeled)), next(iter(unlabeled))
    l_img, l_gt, unl_img = l_img.to(dev), l_gt.to(dev), unl_img.to(dev)
    torch.cuda.synchronize()
    sys.stderr.write("[census] begin %%s\n" %% tag)
    for _ in range(%d):
        m.step(l_img, l_gt, unl_img)
    m.sync_losses()
    F.flush_side_work()
    torch.cuda.synchronize()
    sys.stderr.write("[census] end %%s\n" %% tag)
if %d:
    rc = L.dev_tool("racecheck")
    core = rc.report(sys.stdout)
    sys.stderr.write("[racecheck] %%d reports, %%d crf_loss launches\n" %% (len(core.reports), L.lib.counts.get("sscg_crf_loss_fwd", 0)))
"""


def _run(tmp_path, env, steps, racecheck):
    for k in ("SSCG_RACECHECK", "SSCG_FUZZ", "SSCG_FUSE_HEAD", "SSCG_TRACE"):
        env.pop(k, None)
    env.update(racecheck and {"SSCG_RACECHECK": "1"} or {"SSCG_TRACE": "1"})
    code = SCRIPT % (ROOT, os.path.join(ROOT, "tests"), str(tmp_path / "ckpt"), steps, 1 if racecheck else 0)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def test_launch_census(dev, tmp_path):
    r = _run(tmp_path, dict(os.environ), 1, False)
    calls = {}
    for tag in ("off", "on"):
        body = r.stderr[r.stderr.index("[census] begin " + tag):r.stderr.index("[census] end " + tag)]
        names = [line[7:].split("(")[0] for line in body.splitlines() if line.startswith("[sscg] ")]
        calls[tag] = {n: names.count(n) for n in set(names)}
    off, on = calls["off"], calls["on"]
    assert not any(n.startswith("sscg_crf") for n in off), off
    # on: ONE forward entry, and the existing scale launch backward; no other launch is added or lost
    assert on.get("sscg_crf_loss_fwd") == 1 and on.get("sscg_lovasz_scale_add") == 1 and "sscg_lovasz_scale_add" not in off
    assert "sscg_crf_head" not in on and "sscg_unl_fwd" not in on
    # (a guide batch in NCHW memory, as these loaders give it, is brought to channels-last once more)
    assert on.get("sscg_nchw_to_nhwc", 0) - off.get("sscg_nchw_to_nhwc", 0) in (0, 1)

    def launches(c):
        return {k: v for k, v in c.items() if not k.startswith("sscg_crf_loss") and k not in ("sscg_lovasz_scale_add", "sscg_weighted_sum", "sscg_nchw_to_nhwc")
                and not k.endswith(("_workspace", "_bytes", "_applies"))}
    assert launches(on) == launches(off), (launches(on), launches(off))


def test_the_step_with_the_flag_is_clean_under_the_stream_ordering_checker(dev, tmp_path):
    r = _run(tmp_path, dict(os.environ), 2, True)
    line = [ln for ln in r.stderr.splitlines() if ln.startswith("[racecheck] ")]
    assert line == ["[racecheck] 0 reports, 2 crf_loss launches"], (line, r.stdout[-3000:])
