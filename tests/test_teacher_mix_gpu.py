"""CutMix consistency for the mean teacher on the MI355X: sscg_mix_boxes (csrc/mix_boxes.hip) against
data_utils.augmentations.mix_batch, sscg_teacher_fwd_mix (csrc/teacher.hip) against sscg_teacher_fwd on inputs mixed with torch, and
against the definition in fp64 on the CPU (tests/teacher_mix_reference.py: un-mirror, F.interpolate(align_corners=True), where(pasted,
a[p], a[n]), then tests/teacher_reference.py's arithmetic), the autograd nodes with `mix=`, and the training step with --unl_cutmix.

Tolerances: tests/test_teacher_gpu.py's, imported - the quantities and the arithmetic are the same: a loss within 1e-3 |ref| + 1e-7;
coef and the logits' gradient within 1e-3 max|ref| + floor_of(...); K, A and the label map EXACT, which the margins of the inputs make
meaningful (tests/test_teacher_mix_host.py asserts them on the CPU for the seeds teacher_mix_reference.SEEDS pins).  Everything that
compares two GPU results is bit for bit.  The tests print the distances they observed (`teacher ...` lines; run with -s)."""
import collections
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_sub
from teacher_mix_reference import (CLASSES, DET_CLASSES, DET_FLIPS, DET_GEOM, GEOMS, NOTHING, TAU, case_inputs, mix_closed_form_grad,
                                   mix_inputs_of, mix_teacher_reference, pasted, reference, tables_of)
from teacher_reference import mirror_where, soft_upstream, unl_reference
from test_teacher_gpu import COMBOS, EPS32, G2, GU, _Counting, check_close, check_forward, check_loss, flip_bytes, floor_of, gpu, raw_fwd

pytestmark = pytest.mark.gpu

CL = torch.channels_last


def dev_table(table, dev):
    return None if table is None else torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).to(dev)


def raw_mix(F, dev, xh, th, flip, table, OH, OW, inv_temp, tau, want_map=True, want_coef=True, fill=0x5A):
    """sscg_teacher_fwd_mix on sentinel-guarded outputs, the workspace pre-filled and followed by a guard region (test_teacher_gpu's
    raw_fwd with the table): (losses [2], sums [4], map or None, coef or None).  table: int32 [N, 8] on the device, or None = NULL"""
    lib = F.lib
    N, H, W, C = xh.shape
    need = lib.sscg_teacher_workspace(N, OH, OW)
    V = N * OH * OW
    ws = torch.full((need + 256,), fill, dtype=torch.uint8, device=dev)
    lo = torch.full((2 + 64,), 7.0, device=dev)
    su = torch.full((4 + 64,), 7.0, dtype=torch.float64, device=dev)
    pm = torch.full((V + 128,), 0xEE, dtype=torch.uint8, device=dev)
    cf = torch.full((V * C + 128,), 7.0, device=dev)
    losses, sums, pmap, coef = lo[32:34], su[32:36], pm[64:64 + V], cf[64:64 + V * C]
    fp = None if flip is None else flip.data_ptr()
    tp = None if table is None else table.data_ptr()
    assert table is None or (table.dtype == torch.int32 and tuple(table.shape) == (N, 8) and table.is_contiguous())
    assert lib.sscg_teacher_fwd_mix(xh.data_ptr(), th.data_ptr(), fp, tp, N, H, W, C, OH, OW, inv_temp, tau, losses.data_ptr(), sums.data_ptr(),
                                    None, None, ws.data_ptr(), need - 1, F._stream()) == -3          # one byte short
    rc = lib.sscg_teacher_fwd_mix(xh.data_ptr(), th.data_ptr(), fp, tp, N, H, W, C, OH, OW, inv_temp, tau, losses.data_ptr(), sums.data_ptr(),
                                  pmap.data_ptr() if want_map else None, coef.data_ptr() if want_coef else None, ws.data_ptr(), need,
                                  F._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert (ws[need:] == fill).all() and (lo[:32] == 7).all() and (lo[34:] == 7).all() and (su[:32] == 7).all() and (su[36:] == 7).all()
    assert (pm[:64] == 0xEE).all() and (pm[64 + V:] == 0xEE).all() and (want_map or (pm == 0xEE).all())
    assert (cf[:64] == 7).all() and (cf[64 + V * C:] == 7).all() and (want_coef or (cf == 7).all())
    return (losses.clone(), sums.clone(), pmap.clone().view(N, OH, OW) if want_map else None,
            coef.clone().view(N, OH, OW, C) if want_coef else None)


def same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


def nhwc(t, dev):
    h = gpu(t, dev).permute(0, 2, 3, 1)
    assert h.is_contiguous()
    return h


def mixed_on_device(tup, flip, table, OH, OW):
    """the teacher's full-resolution map [N, C, OH, OW] on the device, un-mirrored where flip and mixed with torch.where"""
    a = mirror_where(tup, flip)
    mask, partner = pasted(table, OH, OW)
    out = torch.where(mask.to(tup.device).unsqueeze(1), a[torch.as_tensor(partner, device=tup.device)], a)
    return out.contiguous(memory_format=CL)


# ------------------------------------------------------------------------------------------ 1. sscg_mix_boxes
# 5 x 7, 13 x 17 and 21 x 23 have an odd number of elements per sample at C = 1 and 3: one float per thread.  4 x 8 and 6 x 10 make
# H*W*C a multiple of 4 at every C: four floats per thread, spanning four pixels at C = 1 and parts of two at C = 3.
MIX_SIZES = [(5, 7), (13, 17), (21, 23), (4, 8), (6, 10)]


def raw_mix_boxes(F, dev, x_nhwc, table, shift=0):
    """sscg_mix_boxes into a buffer of 0xFF bytes: the output between its guards.  shift: floats by which both tensors are moved off
    their 16-byte alignment"""
    N, H, W, C = x_nhwc.shape
    total = N * H * W * C
    src = torch.empty(total + 8, device=dev)[shift:shift + total].view(N, H, W, C)
    src.copy_(x_nhwc)
    buf = torch.full(((total + 128 + 8) * 4,), 0xFF, dtype=torch.uint8, device=dev)
    words = buf.view(torch.int32)
    y = words[64 + shift:64 + shift + total]
    assert (src.data_ptr() % 16 == 0) == (shift % 4 == 0) and (y.data_ptr() % 16 == 0) == (shift % 4 == 0)
    assert F.lib.sscg_mix_boxes(src.data_ptr(), y.data_ptr(), table.data_ptr(), N, H, W, C, F._stream()) == 0
    torch.cuda.synchronize()
    assert (words[:64 + shift] == -1).all() and (words[64 + shift + total:] == -1).all()
    return y.clone().view(torch.float32).view(N, H, W, C)


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("size", MIX_SIZES)
def test_mix_boxes_equals_mix_batch(size, C, F, dev):
    A = load_sub("data_utils.augmentations")
    H, W = size
    for N in (3, 2, 1):
        g = torch.Generator().manual_seed(100 * H + 10 * C + N)
        x = torch.randn(N, C, H, W, generator=g)                   # finite, so a 0xFF word left in the output cannot equal its reference
        xh = x.to(dev).permute(0, 2, 3, 1).contiguous()
        for name, table in tables_of((N, 0, 0, H, W)).items():
            want = torch.from_numpy(A.mix_batch(x.numpy(), None, table, False)[0]).permute(0, 2, 3, 1).contiguous()
            for shift in (0, 1):
                got = raw_mix_boxes(F, dev, xh, dev_table(table, dev), shift)
                assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)), (size, C, N, name, shift)
    # y == x is refused before anything is launched
    t = dev_table(tables_of((3, 0, 0, H, W))["whole"], dev)
    assert F.lib.sscg_mix_boxes(xh.data_ptr(), xh.data_ptr(), t.data_ptr(), 1, H, W, C, F._stream()) == -1


def test_mix_boxes_wrapper(F, dev):
    A, L = load_sub("data_utils.augmentations"), load_sub("_lib")
    g = torch.Generator().manual_seed(3)
    for C, H, W in ((3, 8, 12), (1, 5, 7), (4, 13, 17)):
        x = torch.randn(3, C, H, W, generator=g)
        tabs = tables_of((3, 0, 0, H, W))
        for layout in (x.to(dev), x.to(dev).contiguous(memory_format=CL)):
            for name, table in tabs.items():
                got = F.mix_boxes(layout, table)
                want = torch.from_numpy(A.mix_batch(x.numpy(), None, table, False)[0])
                assert torch.equal(got.cpu(), want), (C, H, W, name)
                assert (got is layout) == (name in NOTHING), name                   # the batch itself when no row mixes
                assert torch.equal(F.mix_boxes(layout, torch.from_numpy(table)).cpu(), want)
        assert torch.equal(layout.cpu(), x)                                          # the input is left alone
    with pytest.raises(L.SscgError):
        F.mix_boxes(x.to(dev).requires_grad_(True), tabs["whole"])                   # no autograd
    with torch.no_grad():
        assert torch.equal(F.mix_boxes(x.to(dev).requires_grad_(True), tabs["whole"]).cpu(), x[[1, 2, 0]])


# ------------------------------------------------------------------------------------------ 2.-5. the mix entry against the plain one
_OUTS = {}


def entry_outputs(F, dev, gi, C):
    """per table of a case: the outputs of the RESIZED mix entry, computed once and shared (left unchanged by their readers)"""
    if (gi, C) not in _OUTS:
        N, H, W, OH, OW = GEOMS[gi]
        x, t, flip, tau, temp = case_inputs(gi, C)
        xh, th, fb = nhwc(x, dev), nhwc(t, dev), flip_bytes(flip, dev)
        _OUTS[(gi, C)] = {name: raw_mix(F, dev, xh, th, fb, dev_table(table, dev), OH, OW, 1.0, tau) for name, table in tables_of(gi).items()}
    return _OUTS[(gi, C)]


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("gi", range(len(GEOMS)))
def test_a_table_that_mixes_nothing_gives_the_plain_entry(gi, C, F, dev):
    N, H, W, OH, OW = GEOMS[gi]
    x, t, flip, tau, temp = case_inputs(gi, C)
    xh, th, fb = nhwc(x, dev), nhwc(t, dev), flip_bytes(flip, dev)
    outs = entry_outputs(F, dev, gi, C)
    plain = raw_fwd(F, dev, xh, th, fb, OH, OW, 1.0, tau)
    assert same(raw_mix(F, dev, xh, th, fb, None, OH, OW, 1.0, tau), plain), (gi, C, "NULL")
    for name in outs:
        if name in NOTHING or N == 1:
            assert same(outs[name], plain), (gi, C, name)
    # the identity-size instances, and the optional outputs
    up, tup = F.upsample_bilinear(gpu(x, dev), (OH, OW)).permute(0, 2, 3, 1), F.upsample_bilinear(gpu(t, dev), (OH, OW)).permute(0, 2, 3, 1)
    flat = raw_fwd(F, dev, up, tup, fb, OH, OW, 1.0, tau)
    tabs = tables_of(gi)
    for name in (None,) + NOTHING:
        table = dev_table(tabs[name], dev) if name else None
        assert same(raw_mix(F, dev, up, tup, fb, table, OH, OW, 1.0, tau), flat), (gi, C, name)
        bare = raw_mix(F, dev, xh, th, fb, table, OH, OW, 1.0, tau, want_map=False, want_coef=False)
        assert bare[2] is None and bare[3] is None and torch.equal(bare[0], plain[0]) and torch.equal(bare[1], plain[1])
    assert same(raw_mix(F, dev, xh, th, None, dev_table(tabs["identity"], dev), OH, OW, 1.0, tau), raw_fwd(F, dev, xh, th, None, OH, OW, 1.0, tau))


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("gi", range(len(GEOMS)))
def test_the_identity_size_form_and_the_resized_form(gi, C, F, dev):
    """3. OH == H: the mix entry equals sscg_teacher_fwd with flip = NULL on the teacher map mixed with torch.where after un-mirroring;
    4. the resized form equals that identity-size form on sscg_upsample_bilinear_fwd's outputs of x and t - every table, bit for bit"""
    N, H, W, OH, OW = GEOMS[gi]
    x, t, flip, tau, temp = case_inputs(gi, C)
    fb = flip_bytes(flip, dev)
    outs = entry_outputs(F, dev, gi, C)
    up, tup = F.upsample_bilinear(gpu(x, dev), (OH, OW)), F.upsample_bilinear(gpu(t, dev), (OH, OW))
    uph, tuph = up.permute(0, 2, 3, 1), tup.permute(0, 2, 3, 1)
    assert uph.is_contiguous() and tuph.is_contiguous()
    for name, table in tables_of(gi).items():
        flat_mix = raw_mix(F, dev, uph, tuph, fb, dev_table(table, dev), OH, OW, 1.0, tau)
        by_torch = raw_fwd(F, dev, uph, mixed_on_device(tup, flip, table, OH, OW).permute(0, 2, 3, 1), None, OH, OW, 1.0, tau)
        assert same(flat_mix, by_torch), (gi, C, name, "identity size")
        assert same(outs[name], flat_mix), (gi, C, name, "resized")
        # without flip bytes the partner is read as it lies
        if name in ("interior", "cycle_a"):
            nf = raw_mix(F, dev, uph, tuph, None, dev_table(table, dev), OH, OW, 1.0, tau)
            assert same(nf, raw_fwd(F, dev, uph, mixed_on_device(tup, None, table, OH, OW).permute(0, 2, 3, 1), None, OH, OW, 1.0, tau))


@pytest.mark.parametrize("C", CLASSES)
def test_the_whole_map_cycle_is_the_permuted_batch(C, F, dev):
    gi = 0
    N, H, W, OH, OW = GEOMS[gi]
    x, t, flip, tau, temp = case_inputs(gi, C)
    outs = entry_outputs(F, dev, gi, C)
    for name, perm in (("cycle_a_whole", [1, 2, 0]), ("cycle_b_whole", [2, 0, 1])):
        want = raw_fwd(F, dev, nhwc(x, dev), nhwc(t[perm], dev), flip_bytes(tuple(flip[p] for p in perm), dev), OH, OW, 1.0, tau)
        assert same(outs[name], want), (C, name)
    # N = 2: the whole map with the next sample is the swapped batch
    gi = 1
    N, H, W, OH, OW = GEOMS[gi]
    x, t, flip, tau, temp = case_inputs(gi, C)
    want = raw_fwd(F, dev, nhwc(x, dev), nhwc(t[[1, 0]], dev), flip_bytes((flip[1], flip[0]), dev), OH, OW, 1.0, tau)
    assert same(entry_outputs(F, dev, gi, C)["whole"], want), C


# ------------------------------------------------------------------------------------------ 6. against the definition
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("gi", range(len(GEOMS)))
def test_values_against_the_fp64_reference(gi, C, F, dev):
    N, H, W, OH, OW = GEOMS[gi]
    outs = entry_outputs(F, dev, gi, C)
    for name in tables_of(gi):
        check_forward("mix %dx%dx%d->%dx%d C=%d %s" % (N, H, W, OH, OW, C, name), C, outs[name], reference(gi, C, name))


# ------------------------------------------------------------------------------------------ 7. through autograd
def run_head_mix(F, dev, x64, t64, flip, table, size, tau, temp, on, unl_on, tau_u, R64, counts=None):
    """test_teacher_gpu.run_head with `mix=`: (soft, the five losses, stats, the gradient on x, the teacher's gradient)"""
    xg = gpu(x64, dev).requires_grad_(True)
    tg = gpu(t64, dev).requires_grad_(True)
    teacher = F.TeacherOptions(mse=float(on[0]), ce=float(on[1]), thresh=tau, temp=temp)
    unl = None if unl_on is None else F.UnlabelledOptions(entropy=float(unl_on[0]), maxsq=float(unl_on[1]), pseudo=float(unl_on[2]), thresh=tau_u)
    soft, l_mse, l_ce, l_ent, l_msq, l_pl, stats = F.upsample_softmax_teacher(xg, size, tg, teacher, unl, flip=flip_bytes(flip, dev),
                                                                              mix=dev_table(table, dev))
    terms, weights = [], []
    for term, live, w in ((l_mse, on[0], G2[0]), (l_ce, on[1], G2[1])) + (() if unl_on is None else tuple(zip((l_ent, l_msq, l_pl), unl_on, GU))):
        if live:
            terms.append(term)
            weights.append(w)
    total = F.weighted_sum(terms, weights) + (soft * gpu(R64, dev)).sum()
    if counts is not None:
        counts.clear()
    total.backward()
    return soft, (l_mse, l_ce, l_ent, l_msq, l_pl), stats, xg.grad, tg.grad


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("gi,name", [(0, "cycle_a"), (0, "outside"), (1, "interior")])
def test_autograd_every_combination_of_live_terms(gi, name, C, F, dev, monkeypatch):
    N, H, W, OH, OW = GEOMS[gi]
    x, t, flip, tau, temp = case_inputs(gi, C)
    table = tables_of(gi)[name]
    tau_u = TAU[C]
    R = soft_upstream(5, N, C, OH, OW)
    assert F._head_applies(gpu(x, dev), OH, OW)
    plain = F.upsample_softmax_ce(gpu(x, dev), (OH, OW))[0]
    counts = collections.Counter()
    monkeypatch.setattr(F, "lib", _Counting(F.lib, counts))
    for combo, on, unl_on in COMBOS:
        g = tuple(G2[k] * on[k] for k in range(2))
        ref = mix_teacher_reference(x, t, flip, table, tau, temp, (OH, OW), g, R)
        want, floor = mix_closed_form_grad(x, t, flip, table, tau, temp, (OH, OW), g, R), floor_of(ref, C, g, float(R.abs().max()))
        uref = None
        if unl_on is not None:
            gu = tuple(GU[k] * unl_on[k] for k in range(3))
            uref = unl_reference(x, tau_u, (OH, OW), gu)
            want = want + uref["grad"]
            lnc = math.log(C) if C > 1 else 1.0
            floor += 8 * EPS32 * (abs(gu[0]) * uref["max_u"] / (uref["V"] * lnc) + abs(gu[1]) / uref["V"] + abs(gu[2]) / max(uref["K"], 1))
        tag = "mix head %dx%dx%d->%dx%d C=%d %s %s" % (N, H, W, OH, OW, C, name, combo)
        for fused in (True, False):
            was = F.FUSE_HEAD[0]
            F.FUSE_HEAD[0] = fused
            try:
                counts.clear()
                soft, losses, stats, grad, tgrad = run_head_mix(F, dev, x, t, flip, table, (OH, OW), tau, temp, on, unl_on, tau_u, R, counts)
            finally:
                F.FUSE_HEAD[0] = was
            back = dict(counts)
            kind = tag + (" fused" if fused else " flat")
            assert tgrad is None, kind                                              # the teacher gets no gradient
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
            # the backward is the plain node's: one scale-add for the squared distance, ONE stencil launch (flat: one sscg_unl_bwd)
            assert back.get("sscg_lovasz_scale_add", 0) == (1 if on[0] else 0), (kind, back)
            assert "sscg_teacher_fwd_mix" not in back and "sscg_teacher_fwd" not in back, (kind, back)
            if fused:
                assert back.get("sscg_upsample_head_bwd_u") == 1 and "sscg_unl_bwd" not in back and "sscg_upsample_head_bwd" not in back, (kind, back)
            else:
                assert back.get("sscg_unl_bwd", 0) == (1 if on[1] or unl_on is not None else 0) and back.get("sscg_softmax_bwd") == 1, (kind, back)
                assert "sscg_upsample_head_bwd_u" not in back, (kind, back)


def test_the_forward_of_the_node_is_the_mix_entry_once(F, dev, monkeypatch):
    gi, C = 0, 4
    N, H, W, OH, OW = GEOMS[gi]
    x, t, flip, tau, temp = case_inputs(gi, C)
    counts = collections.Counter()
    monkeypatch.setattr(F, "lib", _Counting(F.lib, counts))
    table = dev_table(tables_of(gi)["cycle_a"], dev)
    for fused in (True, False):
        was = F.FUSE_HEAD[0]
        F.FUSE_HEAD[0] = fused
        try:
            counts.clear()
            out = F.upsample_softmax_teacher(gpu(x, dev).requires_grad_(True), (OH, OW), gpu(t, dev), F.TeacherOptions(mse=1.0, ce=1.0, thresh=tau),
                                             flip=flip_bytes(flip, dev), mix=table)
            assert counts["sscg_teacher_fwd_mix"] == 1 and counts["sscg_teacher_fwd"] == 0, dict(counts)
            counts.clear()
            F.upsample_softmax_teacher(gpu(x, dev).requires_grad_(True), (OH, OW), gpu(t, dev), F.TeacherOptions(mse=1.0, ce=1.0, thresh=tau),
                                       flip=flip_bytes(flip, dev))
            assert counts["sscg_teacher_fwd_mix"] == 0 and counts["sscg_teacher_fwd"] == 1, dict(counts)
        finally:
            F.FUSE_HEAD[0] = was
        ref = reference(gi, C, "cycle_a")
        assert float(out[6]["sums"][3]) == ref["K"] and torch.equal(out[6]["pseudo"].cpu(), ref["pseudo"])
    with pytest.raises(load_sub("_lib").SscgError):
        F.teacher_fwd(gpu(x, dev), gpu(t, dev), None, (OH, OW), 1.0, 0.5, table=table[:2])
    with pytest.raises(load_sub("_lib").SscgError):
        F.teacher_fwd(gpu(x, dev), gpu(t, dev), None, (OH, OW), 1.0, 0.5, table=table.cpu())


# ------------------------------------------------------------------------------------------ 8. determinism
def test_the_same_call_twice_gives_the_same_bits(F, dev):
    N, H, W, OH, OW = DET_GEOM
    C = DET_CLASSES
    assert (OH * OW) % 256 and OH * OW > 256
    x, t = mix_inputs_of(77, DET_GEOM, C, DET_FLIPS)
    xh, th, fb = nhwc(x, dev), nhwc(t, dev), flip_bytes(DET_FLIPS, dev)
    table = tables_of(DET_GEOM)["interior"]
    runs = [raw_mix(F, dev, xh, th, fb, dev_table(table, dev), OH, OW, 1.0, 0.35, fill=fill) for fill in (0xFF, 0xFF, 0x00)]
    assert same(runs[0], runs[1]) and same(runs[0], runs[2])
    ref = mix_teacher_reference(x, t, DET_FLIPS, table, 0.35, 1.0, (OH, OW))
    check_loss("mix twice mse", runs[0][0][0], ref["mse"])
    check_loss("mix twice ce", runs[0][0][1], ref["ce"])
    # and it is not the plain entry's result: the box changed something
    assert not torch.equal(runs[0][2], raw_fwd(F, dev, xh, th, fb, OH, OW, 1.0, 0.35)[2])


# ------------------------------------------------------------------------------------------ 9. the training step
@pytest.mark.parametrize("mode", ["check", "fuzz", "identity"])
def test_training_steps_with_cutmix_consistency(mode, tmp_path):
    """tests/aids/teacher_mix_step.py in a fresh process: steps under the stream-ordering checker with spies on what the teacher and
    the student saw (check), the serial run against one fuzzed schedule, bit for bit (fuzz), and the identity draw against
    --unl_teacher alone, bit for bit (identity)"""
    env = dict(os.environ)
    for k in ("SSCG_TRACE", "SSCG_RACECHECK", "SSCG_FUZZ", "SSCG_FUSE_HEAD"):
        env.pop(k, None)
    r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.join(ROOT, "tests", "aids", "teacher_mix_step.py"), mode,
                        str(tmp_path / "ckpt")], env=env, capture_output=True, text=True)
    sys.stdout.write(r.stdout[-6000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "teacher mix step: ok" in r.stdout
