"""Mean-teacher consistency on the MI355X: sscg_teacher_fwd (csrc/teacher.hip) and the nodes built on it (functional.TeacherHeadFn,
the flat TeacherLossFn) against the definition written with torch ops in fp64 on the CPU (tests/teacher_reference.py:
F.interpolate(align_corners=True), a per-sample flip of the resized teacher, * float32(1 / temp), softmax; the gradient by autograd
with the teacher detached).

Tolerances (tests/test_unl_gpu.py's header): a loss within 1e-3 |ref| + 1e-7; coef and the logits' gradient within a max-abs distance of
1e-3 max|ref| + floor, floor = 8 fp32 roundings of the largest term of an entry,
    8 * 2^-23 * (2 |g_mse| / (C V) + |g_ce| / max(K, 1) + max|dy|)        (+ test_unl_gpu.grad_floor's terms where --unl_* terms ride).
K, A and the label map are EXACT (torch.equal), which only makes sense where fp32 cannot flip a decision: every input keeps, in fp64,
|conf - tau| >= 1e-4 and top-two gaps >= 1e-4 of both the teacher and the student at every output pixel, and for C > 1 on a source map
larger than 1x1 a kept share and an agreement share in [0.1, 0.9]; tests/test_teacher_host.py asserts that on the CPU for the seeds
teacher_reference.SEEDS pins.  Two settings run: teacher_reference.CONFIGS' thresholds at temperature 1 and at 0.5.
Every test prints the distances it observed (`teacher ...` lines; run with -s); profiles/unl_teacher.txt keeps them."""
import collections
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, load_sub
from test_dice_host import CLASSES, GEOMS
from teacher_reference import CONFIGS, case_inputs, inv_temp32, mirror_where, reference, soft_upstream, teacher_reference, unl_reference
from unl_reference import TAU, make_logits

pytestmark = pytest.mark.gpu

CL = torch.channels_last
EPS32 = 2.0 ** -23
G2 = (0.37, 1.9)                # distinct upstream scales of (L_mse, L_ce)
GU = (0.53, 1.3, 0.61)          # ... of the unlabelled head's own (entropy, max-squares, pseudo-label cross entropy)
CASES = [(cfg, gi, C) for cfg in sorted(CONFIGS) for gi in range(len(GEOMS)) for C in CLASSES]


def gpu(t, dev):
    return t.float().to(dev).contiguous(memory_format=CL) if t.dim() == 4 else t.float().to(dev)


def flip_bytes(flip, dev):
    return None if flip is None else torch.tensor(list(flip), dtype=torch.uint8, device=dev)


def floor_of(ref, C, g, max_dy=0.0):
    return 8 * EPS32 * (2 * abs(g[0]) / (C * ref["V"]) + abs(g[1]) / max(ref["K"], 1) + max_dy)


def check_loss(tag, loss, ref_loss):
    loss, ref_loss = float(loss.detach()), float(ref_loss)
    d = abs(loss - ref_loss)
    print("teacher %-58s loss %.9g ref %.9g rel %.2e" % (tag, loss, ref_loss, d / max(abs(ref_loss), 1e-30)))
    assert math.isfinite(loss) and d <= 1e-3 * abs(ref_loss) + 1e-7, (tag, loss, ref_loss)


def check_close(tag, got, want, floor):
    got = got.detach().double().cpu()
    d, m = float((got - want).abs().max()), float(want.abs().max())
    print("teacher %-58s max-abs diff %.2e of %.2e rel %.2e (floor %.1e)" % (tag, d, m, d / max(m, 1e-30), floor))
    assert torch.isfinite(got).all() and d <= 1e-3 * m + floor, (tag, d, m)


def raw_fwd(F, dev, xh, th, flip, OH, OW, inv_temp, tau, want_map=True, want_coef=True, fill=0x5A):
    """sscg_teacher_fwd on sentinel-guarded outputs, the workspace pre-filled and followed by a guard region: (losses [2], sums [4], map
    or None, coef or None)"""
    lib = F.lib
    N, H, W, C = xh.shape
    need = lib.sscg_teacher_workspace(N, OH, OW)
    assert need == N * 4 * (min((OH * OW + 255) // 256, 256) + 1) * 8
    V = N * OH * OW
    ws = torch.full((need + 256,), fill, dtype=torch.uint8, device=dev)
    lo = torch.full((2 + 64,), 7.0, device=dev)
    su = torch.full((4 + 64,), 7.0, dtype=torch.float64, device=dev)
    pm = torch.full((V + 128,), 0xEE, dtype=torch.uint8, device=dev)
    cf = torch.full((V * C + 128,), 7.0, device=dev)
    losses, sums, pmap, coef = lo[32:34], su[32:36], pm[64:64 + V], cf[64:64 + V * C]
    fp = None if flip is None else flip.data_ptr()
    assert lib.sscg_teacher_fwd(xh.data_ptr(), th.data_ptr(), fp, N, H, W, C, OH, OW, inv_temp, tau, losses.data_ptr(), sums.data_ptr(), None,
                                None, ws.data_ptr(), need - 1, F._stream()) == -3                # one byte short
    rc = lib.sscg_teacher_fwd(xh.data_ptr(), th.data_ptr(), fp, N, H, W, C, OH, OW, inv_temp, tau, losses.data_ptr(), sums.data_ptr(),
                              pmap.data_ptr() if want_map else None, coef.data_ptr() if want_coef else None, ws.data_ptr(), need, F._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert (ws[need:] == fill).all() and (lo[:32] == 7).all() and (lo[34:] == 7).all() and (su[:32] == 7).all() and (su[36:] == 7).all()
    assert (pm[:64] == 0xEE).all() and (pm[64 + V:] == 0xEE).all() and (want_map or (pm == 0xEE).all())
    assert (cf[:64] == 7).all() and (cf[64 + V * C:] == 7).all() and (want_coef or (cf == 7).all())
    return (losses.clone(), sums.clone(), pmap.clone().view(N, OH, OW) if want_map else None,
            coef.clone().view(N, OH, OW, C) if want_coef else None)


def check_forward(tag, C, out, ref):
    losses, sums, pmap, coef = out
    check_loss(tag + " mse", losses[0], ref["mse"])
    check_loss(tag + " ce", losses[1], ref["ce"])
    s = sums.cpu()
    assert s.dtype == torch.float64 and s.shape == (4,)
    assert float(s[3]) == ref["K"] and float(s[1]) == ref["A"], (tag, s, ref["K"], ref["A"])
    rel = [abs(float(s[k]) - float(ref["sums"][k])) / max(abs(float(ref["sums"][k])), 1e-30) for k in (0, 2)]
    print("teacher %-58s K %d A %d of %d exact; sums rel %.2e %.2e" % (tag, ref["K"], ref["A"], ref["V"], rel[0], rel[1]))
    if pmap is not None:
        assert pmap.dtype == torch.uint8 and torch.equal(pmap.cpu(), ref["pseudo"]), tag
    if coef is not None:
        check_close(tag + " coef", coef, ref["coef"], floor_of(ref, C, (1.0, 0.0)))
        dropped = ~ref["kept"].unsqueeze(-1).expand_as(ref["coef"])
        bits = coef.cpu().view(torch.int32)
        assert (bits[dropped] == 0).all(), tag                     # bitwise +0 at every dropped pixel


# ------------------------------------------------------------------------------------------ 1. the raw entry against the definition
@pytest.mark.parametrize("cfg,gi,C", CASES)
def test_raw_forward_values_counts_map_coef(cfg, gi, C, F, dev):
    N, H, W, OH, OW = GEOMS[gi]
    x, t, flip, tau, temp = case_inputs(cfg, gi, C)
    ref = reference(cfg, gi, C)
    it = F.TeacherOptions(temp=temp).inv_temp
    assert it == inv_temp32(temp)
    xh, th = gpu(x, dev).permute(0, 2, 3, 1), gpu(t, dev).permute(0, 2, 3, 1)
    assert xh.is_contiguous() and th.is_contiguous()
    tag = "raw %s %dx%dx%d->%dx%d C=%d" % (cfg, N, H, W, OH, OW, C)
    out = raw_fwd(F, dev, xh, th, flip_bytes(flip, dev), OH, OW, it, tau)
    check_forward(tag, C, out, ref)
    # the optional outputs change nothing else
    bare = raw_fwd(F, dev, xh, th, flip_bytes(flip, dev), OH, OW, it, tau, want_map=False, want_coef=False)
    assert bare[2] is None and bare[3] is None and torch.equal(bare[0], out[0]) and torch.equal(bare[1], out[1])
    # the resized form equals the identity form on upsample_bilinear's output - the teacher's mirrored by torch.flip where flip is set
    up = F.upsample_bilinear(gpu(x, dev), (OH, OW))
    tup = F.upsample_bilinear(gpu(t, dev), (OH, OW))
    flat_flip = raw_fwd(F, dev, up.permute(0, 2, 3, 1), tup.permute(0, 2, 3, 1), flip_bytes(flip, dev), OH, OW, it, tau)
    assert all(torch.equal(a, b) for a, b in zip(out, flat_flip)), tag
    if flip is not None:
        mirrored = mirror_where(tup, flip).contiguous(memory_format=CL)
        flat = raw_fwd(F, dev, up.permute(0, 2, 3, 1), mirrored.permute(0, 2, 3, 1), None, OH, OW, it, tau)
        assert all(torch.equal(a, b) for a, b in zip(out, flat)), tag


# ------------------------------------------------------------------------------------------ 2. the teacher equal to the student
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("gi", range(len(GEOMS)))
def test_self_consistency_with_the_unlabelled_head(gi, C, F, dev):
    """t = x, flip = NULL, inv_temp = 1: the map, K and the kept cross entropies are sscg_unl_fwd's bit for bit, the distance is 0,
    every kept pixel agrees and coef is all zeros"""
    N, H, W, OH, OW = GEOMS[gi]
    x, _, _, tau, _ = case_inputs("t1", gi, C)
    xh = gpu(x, dev).permute(0, 2, 3, 1)
    for size in ((OH, OW), (H, W)):
        losses, sums, pmap, coef = raw_fwd(F, dev, xh, xh, None, size[0], size[1], 1.0, tau)
        u_losses, u_sums, u_map = F.unl_fwd(gpu(x, dev), size, tau, True)
        assert torch.equal(pmap, u_map) and torch.equal(sums[3], u_sums[3]) and torch.equal(sums[2], u_sums[2]), (gi, C, size)
        assert torch.equal(losses[1], u_losses[2])
        assert float(sums[0]) == 0.0 and float(losses[0]) == 0.0 and torch.equal(sums[1], sums[3])
        assert torch.count_nonzero(coef.view(torch.int32)) == 0


# ------------------------------------------------------------------------------------------ 3. determinism
def test_the_same_call_twice_gives_the_same_bits(F, dev):
    N, C, H, W, OH, OW = 2, 21, 9, 11, 67, 83
    assert (OH * OW) % 256 and OH * OW > 256
    x = make_logits(77, N, C, H, W)
    t = (x.float() + make_logits(177, N, C, H, W, scale=1.5).float()).double()
    xh, th = gpu(x, dev).permute(0, 2, 3, 1), gpu(t, dev).permute(0, 2, 3, 1)
    flip = flip_bytes((0, 1), dev)
    runs = [raw_fwd(F, dev, xh, th, flip, OH, OW, 1.0, 0.35, fill=fill) for fill in (0xFF, 0xFF, 0x00)]
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1])) and all(torch.equal(a, b) for a, b in zip(runs[0], runs[2]))
    ref = teacher_reference(x, t, (0, 1), 0.35, 1.0, (OH, OW))
    check_loss("twice mse", runs[0][0][0], ref["mse"])
    check_loss("twice ce", runs[0][0][1], ref["ce"])


# ------------------------------------------------------------------------------------------ 4. through autograd
# (tag, teacher weights that are on, the unlabelled head's own weights that are on)
COMBOS = [("mse", (1, 0), None), ("ce", (0, 1), None), ("both", (1, 1), None), ("both+ent+msq", (1, 1), (1, 1, 0)), ("mse+pseudo", (1, 0), (0, 0, 1))]


def run_head(F, dev, x64, t64, flip, size, tau, temp, on, unl_on, tau_u, R64, counts=None):
    """upsample_softmax_teacher + backward of the weighted live losses + sum(soft * R): (soft, the five losses, stats, gradient)"""
    xg = gpu(x64, dev).requires_grad_(True)
    teacher = F.TeacherOptions(mse=float(on[0]), ce=float(on[1]), thresh=tau, temp=temp)
    unl = None if unl_on is None else F.UnlabelledOptions(entropy=float(unl_on[0]), maxsq=float(unl_on[1]), pseudo=float(unl_on[2]), thresh=tau_u)
    soft, l_mse, l_ce, l_ent, l_msq, l_pl, stats = F.upsample_softmax_teacher(xg, size, gpu(t64, dev), teacher, unl, flip=flip_bytes(flip, dev))
    terms, weights = [], []
    for term, live, w in ((l_mse, on[0], G2[0]), (l_ce, on[1], G2[1])) + (() if unl_on is None else tuple(zip((l_ent, l_msq, l_pl), unl_on, GU))):
        if live:
            terms.append(term)
            weights.append(w)
    total = F.weighted_sum(terms, weights) + (soft * gpu(R64, dev)).sum()
    if counts is not None:
        counts.clear()
    total.backward()
    return soft, (l_mse, l_ce, l_ent, l_msq, l_pl), stats, xg.grad


class _Counting(object):
    """functional.lib with every call counted by name"""

    def __init__(self, inner, counts):
        self._inner, self._counts = inner, counts

    def __getattr__(self, name):
        fn = getattr(self._inner, name)

        def call(*a):
            self._counts[name] += 1
            return fn(*a)
        return call


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("gi", [0, 2, 3])
def test_autograd_every_combination_of_live_terms(gi, C, F, dev, monkeypatch):
    N, H, W, OH, OW = GEOMS[gi]
    cfg = "t05" if gi == 2 else "t1"
    x, t, flip, tau, temp = case_inputs(cfg, gi, C)
    tau_u = TAU[C]
    R = soft_upstream(5, N, C, OH, OW)
    assert F._head_applies(gpu(x, dev), OH, OW)
    plain = F.upsample_softmax_ce(gpu(x, dev), (OH, OW))[0]
    counts = collections.Counter()
    monkeypatch.setattr(F, "lib", _Counting(F.lib, counts))
    for name, on, unl_on in COMBOS:
        g = tuple(G2[k] * on[k] for k in range(2))
        ref = teacher_reference(x, t, flip, tau, temp, (OH, OW), g, R)
        want, floor = ref["grad"], floor_of(ref, C, g, float(R.abs().max()))
        uref = None
        if unl_on is not None:
            gu = tuple(GU[k] * unl_on[k] for k in range(3))
            uref = unl_reference(x, tau_u, (OH, OW), gu)
            want = want + uref["grad"]
            lnc = math.log(C) if C > 1 else 1.0
            floor += 8 * EPS32 * (abs(gu[0]) * uref["max_u"] / (uref["V"] * lnc) + abs(gu[1]) / uref["V"] + abs(gu[2]) / max(uref["K"], 1))
        tag = "head %s %dx%dx%d->%dx%d C=%d %s" % (cfg, N, H, W, OH, OW, C, name)
        for fused in (True, False):
            was = F.FUSE_HEAD[0]
            F.FUSE_HEAD[0] = fused
            try:
                soft, losses, stats, grad = run_head(F, dev, x, t, flip, (OH, OW), tau, temp, on, unl_on, tau_u, R, counts)
            finally:
                F.FUSE_HEAD[0] = was
            back = dict(counts)
            kind = tag + (" fused" if fused else " flat")
            assert torch.equal(soft, plain) if fused else torch.allclose(soft, plain, rtol=0, atol=1e-6)
            check_loss(kind + " mse", losses[0], ref["mse"])
            check_loss(kind + " ce", losses[1], ref["ce"])
            assert float(stats["sums"][3]) == ref["K"] and float(stats["sums"][1]) == ref["A"]
            assert torch.equal(stats["pseudo"].cpu(), ref["pseudo"])
            if uref is not None:
                for k, key in enumerate(("ent", "msq", "pl")):
                    check_loss(kind + " " + key, losses[2 + k], uref[key])
                assert float(stats["unl_sums"][3]) == uref["K"]
            else:
                assert losses[2] is None and losses[3] is None and losses[4] is None and stats["unl_sums"] is None
            check_close(kind + " grad", grad, want, floor)
            # the launch census of the backward: the squared distance is one scale-add into the map's upstream gradient, everything
            # else rides in ONE stencil launch (flat: one sscg_unl_bwd beside the softmax's own backward)
            assert back.get("sscg_lovasz_scale_add", 0) == (1 if on[0] else 0), (kind, back)
            if fused:
                assert back.get("sscg_upsample_head_bwd_u") == 1 and "sscg_unl_bwd" not in back and "sscg_upsample_head_bwd" not in back, (kind, back)
            else:
                assert back.get("sscg_unl_bwd", 0) == (1 if on[1] or unl_on is not None else 0) and back.get("sscg_softmax_bwd") == 1, (kind, back)
                assert "sscg_upsample_head_bwd_u" not in back, (kind, back)


def test_the_teacher_gets_no_gradient_and_both_pseudo_terms_are_refused(F, dev):
    N, H, W, OH, OW = GEOMS[0]
    x, t, flip, tau, temp = case_inputs("t1", 0, 4)
    xg, tg = gpu(x, dev).requires_grad_(True), gpu(t, dev).requires_grad_(True)
    soft, l_mse, l_ce, _, _, _, stats = F.upsample_softmax_teacher(xg, (OH, OW), tg, F.TeacherOptions(mse=1.0, ce=1.0, thresh=tau),
                                                                   flip=flip_bytes(flip, dev))
    (l_mse + l_ce + soft.sum()).backward()
    assert tg.grad is None and xg.grad is not None and not stats["sums"].requires_grad
    # with the squared distance off its value is still returned, as a constant
    out = F.upsample_softmax_teacher(gpu(x, dev).requires_grad_(True), (OH, OW), gpu(t, dev), F.TeacherOptions(ce=1.0, thresh=tau))
    assert not out[1].requires_grad and out[2].requires_grad
    with pytest.raises(ValueError):
        F.upsample_softmax_teacher(xg, (OH, OW), tg, F.TeacherOptions(ce=1.0), F.UnlabelledOptions(pseudo=1.0))
    with pytest.raises(load_sub("_lib").SscgError):
        F.teacher_fwd(gpu(x, dev), gpu(t, dev)[:, :3], None, (OH, OW), 1.0, 0.5)


@pytest.mark.parametrize("C", [21, 64])
@pytest.mark.parametrize("temp", [3.0, 0.7])
def test_inexact_inverse_temperatures(temp, C, F, dev):
    """1 / temp = 1/3 or 1/0.7 rounds: zt * inv_temp is then a rounded product, and an instance that fused it into the softmax's
    subtraction would differ from one that did not.  The resized and the identity instances (compile-time arm at 21 classes, run-time
    arm at 64) must give the same bits, the product taken with torch on the stored resize as well, and the values the definition's."""
    gi = 2
    N, H, W, OH, OW = GEOMS[gi]
    x, t, flip, tau, _ = case_inputs("t1", gi, C)
    it = F.TeacherOptions(temp=temp).inv_temp
    assert it == inv_temp32(temp) and it != 1.0 / temp              # not exactly representable
    ref = teacher_reference(x, t, flip, tau, temp, (OH, OW))
    near = int(((ref["conf"] - tau).abs() < 1e-4).sum())            # the pixels fp32 may decide the other way
    xh, th = gpu(x, dev).permute(0, 2, 3, 1), gpu(t, dev).permute(0, 2, 3, 1)
    out = raw_fwd(F, dev, xh, th, flip_bytes(flip, dev), OH, OW, it, tau)
    up = F.upsample_bilinear(gpu(x, dev), (OH, OW)).permute(0, 2, 3, 1)
    tup = F.upsample_bilinear(gpu(t, dev), (OH, OW))
    flat = raw_fwd(F, dev, up, tup.permute(0, 2, 3, 1), flip_bytes(flip, dev), OH, OW, it, tau)
    assert all(torch.equal(a, b) for a, b in zip(out, flat)), (temp, C)
    # the product formed outside the kernel, one rounding per element, then the kernel at temperature 1
    scaled = (mirror_where(tup, flip) * torch.tensor(it, dtype=torch.float32, device=dev)).contiguous(memory_format=CL)
    outside = raw_fwd(F, dev, up, scaled.permute(0, 2, 3, 1), None, OH, OW, 1.0, tau)
    assert all(torch.equal(a, b) for a, b in zip(out, outside)), (temp, C)
    tag = "temp %g C=%d" % (temp, C)
    print("teacher %-58s K %d ref %d A %d ref %d (%d pixels inside the margin)" % (tag, int(out[1][3]), ref["K"], int(out[1][1]), ref["A"], near))
    assert abs(float(out[1][3]) - ref["K"]) <= near
    if near == 0 and ref["gap_margin"] >= 1e-4:         # no decision fp32 could take the other way: everything as in the raw test
        check_forward(tag, C, out, ref)


def test_mirror_samples_equals_torch_flip(F, dev):
    g = torch.Generator().manual_seed(9)
    x = torch.randn(5, 3, 7, 10, generator=g).to(dev)
    for flags in ([0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [1, 0, 0, 1, 1], [0, 1, 0, 1, 0]):
        got = F.mirror_samples(x, flags)
        assert torch.equal(got, mirror_where(x, flags)) and (any(flags) or got is x), flags
        assert not any(flags) or got.is_contiguous(memory_format=CL)
    with pytest.raises(ValueError):
        F.mirror_samples(x, [1, 0])


# ------------------------------------------------------------------------------------------ 5. the training step
@pytest.mark.parametrize("mode", ["check", "fuzz"])
def test_training_steps_with_the_teacher(mode, tmp_path):
    """tests/aids/teacher_step.py in a fresh process: three steps under the stream-ordering checker (check), and the serial run against
    one fuzzed schedule, bit for bit (fuzz)"""
    env = dict(os.environ)
    for k in ("SSCG_TRACE", "SSCG_RACECHECK", "SSCG_FUZZ", "SSCG_FUSE_HEAD"):
        env.pop(k, None)
    r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.join(ROOT, "tests", "aids", "teacher_step.py"), mode,
                        str(tmp_path / "ckpt")], env=env, capture_output=True, text=True)
    sys.stdout.write(r.stdout[-6000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "teacher step: ok" in r.stdout
