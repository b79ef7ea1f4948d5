"""Sliding-window inference on the MI355X: sscg_predict_head_sw (the windows of one batch blended into one label map in one launch) and
sscg_window_gather (the network input of every window).  The contract is BIT IDENTITY with the chain of separate passes - per window
sscg_upsample_bilinear_fwd, sscg_softmax_fwd, a mirror of the W axis for a mirrored window, an fp32 multiply by the outer product of the
weight tables, an fp32 add into the window's place of a zeroed accumulator; then sscg_argmax_onehot's index, sscg_confusion_hist and an
fp32 multiply by the outer product of the normalisation tables - so every comparison with them is torch.equal.  The fp64 restatement of
tests/sliding_reference.py, which shares no code with either path, guards the meaning (window order, mirror, weights, normalisation).

fp64 figures of test 4 (C = 21, N = 2, 23 x 29 from 12 x 16 windows, logits randn * 4): the test prints them before it asserts."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sliding_reference as R
from conftest import ROOT, load_sub

pytestmark = pytest.mark.gpu
CL = torch.channels_last
GUARD = 64
SENT = {torch.float32: float("nan"), torch.int64: -7777, torch.uint8: 0xEE}

# (OH, OW, wh, ww, h, w, overlap, blend, flip)
CASES = [(23, 29, 12, 16, 5, 7, 0.5, "gauss", False),          # the last window flush with the edge, coverage 1..3 per axis
         (23, 29, 12, 16, 5, 7, 0.75, "gauss", True),          # coverage up to 5 per axis, both views
         (23, 29, 12, 16, 5, 7, 0.0, "const", False),
         (23, 29, 12, 16, 12, 16, 0.5, "gauss", True),         # identity resize
         (12, 16, 12, 16, 5, 7, 0.5, "gauss", False)]          # one window
CASE_IDS = ["flush_last_window", "overlap_075_flip", "const_no_overlap", "identity_resize_flip", "one_window"]


def guarded(n, dtype, dev):
    """(buffer, view of n elements GUARD elements into it): the whole buffer holds the sentinel of its dtype."""
    buf = torch.full((n + 2 * GUARD,), SENT[dtype], dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


def is_sentinel(t):
    return torch.isnan(t) if t.is_floating_point() else t == SENT[t.dtype]


def guards_intact(buf):
    return bool(is_sentinel(torch.cat([buf[:GUARD], buf[-GUARD:]])).all())


def make_plan(F, dev, OH, OW, wh, ww, overlap, blend, flip):
    return F.sliding_plan(OH, OW, F.SlidingOptions((wh, ww), (OH, OW), overlap=overlap, blend=blend, flip=flip), dev)


def make_logits(Cn, N, plan, h, w, seed, dev, scale=3.0):
    """The windows' logit maps [N * views, Cn, h, w] (channels-last memory), `randn * scale`."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N * plan.views, Cn, h, w, generator=g) * scale).to(dev).contiguous(memory_format=CL)


def make_labels(Cn, N, oh, ow, seed, dev):
    g = torch.Generator().manual_seed(seed + 1000)
    lt = torch.randint(0, Cn, (N, oh, ow), generator=g)
    flat = lt.view(-1)
    flat[0::7] = -1
    flat[3::11] = 255
    flat[5::13] = Cn
    return lt.to(dev)


def hist_pattern(Cn, dev):
    return (torch.arange(Cn * Cn, dtype=torch.int64, device=dev) * 3 + 1).view(Cn, Cn)


def separate(F, x, plan, lt=None, hist=None):
    """The chain of separate passes, written here from entries that existed before (the resize also at the identity size) and torch
    element-wise ops.  Returns (acc [N,C,OH,OW], index, prob)."""
    nv, Cn = x.shape[:2]
    N = nv // plan.views
    Fv = 2 if plan.flip else 1
    acc = torch.zeros(N, Cn, plan.OH, plan.OW, device=x.device)
    g = plan.wy_dev[:, None] * plan.wx_dev[None, :]
    xs = x.view(N, plan.ky, plan.kx, Fv, Cn, *x.shape[2:])
    for iy, py in enumerate(plan.pos_y):
        for ix, px in enumerate(plan.pos_x):
            for f in range(Fv):
                xk = xs[:, iy, ix, f].contiguous(memory_format=CL)
                p = F.softmax_fwd(F.upsample_fwd(xk, plan.wh, plan.ww))
                if f:
                    p = torch.flip(p, dims=(3,))
                acc[:, :, py:py + plan.wh, px:px + plan.ww] += p * g
    idx = F.argmax_index(acc)
    if lt is not None:
        F.confusion_hist(lt, idx, Cn, hist)
    return acc, idx, acc * (plan.ry_dev[:, None] * plan.rx_dev[None, :])


def fused_raw(L, x, plan, lt, hist_init, dev, outputs=("prob", "index", "u8", "hist")):
    """sscg_predict_head_sw itself, every output a view into a sentinel-filled buffer; the outputs not named get a null pointer.
    Returns {name: tensor} for all four buffers (the ones not asked for must come back untouched)."""
    nv, Cn, h, w = x.shape
    N, oh, ow = nv // plan.views, plan.OH, plan.OW
    pb, prob = guarded(N * oh * ow * Cn, torch.float32, dev)
    ib, index = guarded(N * oh * ow, torch.int64, dev)
    ub, u8 = guarded(N * oh * ow, torch.uint8, dev)
    hb, hist = guarded(Cn * Cn, torch.int64, dev)
    if "hist" in outputs:
        hist.copy_(hist_init.view(-1))
    ptr = lambda name, t: t.data_ptr() if name in outputs else None
    rc = L.lib.sscg_predict_head_sw(x.data_ptr(), N, h, w, Cn, plan.wh, plan.ww, plan.sy, plan.sx, plan.ky, plan.kx, 1 if plan.flip else 0,
                                    oh, ow, plan.wy_dev.data_ptr(), plan.wx_dev.data_ptr(), plan.ry_dev.data_ptr(), plan.rx_dev.data_ptr(),
                                    ptr("prob", prob), ptr("index", index), ptr("u8", u8), lt.data_ptr() if "hist" in outputs else None,
                                    ptr("hist", hist), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for b in (pb, ib, ub, hb):
        assert guards_intact(b), "a store outside the %s output" % b.dtype
    out = {"prob": prob.view(N, oh, ow, Cn), "index": index.view(N, oh, ow), "u8": u8.view(N, oh, ow), "hist": hist.view(Cn, Cn)}
    for name, t in out.items():
        if name in outputs:
            assert not bool(is_sentinel(t).any()), "%s: an element was not written" % name
        else:
            assert bool(is_sentinel(t).all()), "%s was not asked for and was written" % name
    return out


# ------------------------------------------------------------------------------------------ 1. the head against the separate passes
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("Cn", [4, 20, 21, 5])
def test_head_equals_the_separate_passes(F, dev, Cn, case):
    L = load_sub("_lib")
    OH, OW, wh, ww, h, w, overlap, blend, flip = case
    N = 2
    plan = make_plan(F, dev, OH, OW, wh, ww, overlap, blend, flip)
    x = make_logits(Cn, N, plan, h, w, 100 * Cn + CASES.index(case), dev)
    lt = make_labels(Cn, N, OH, OW, Cn, dev)
    assert bool((lt == 255).any()) and bool((lt >= Cn).any())
    want_hist = hist_pattern(Cn, dev).clone()
    acc, idx, prob = separate(F, x, plan, lt, want_hist)
    got = fused_raw(L, x, plan, lt, hist_pattern(Cn, dev), dev)
    what = "C=%d %s" % (Cn, CASE_IDS[CASES.index(case)])
    assert torch.equal(got["prob"], prob.permute(0, 2, 3, 1)), "%s: %d of %d probabilities differ" % (
        what, int((got["prob"] != prob.permute(0, 2, 3, 1)).sum()), prob.numel())
    assert torch.equal(got["index"], idx), "%s: %d labels differ" % (what, int((got["index"] != idx).sum()))
    assert torch.equal(got["u8"].to(torch.int64), idx), what
    assert torch.equal(got["hist"], want_hist), what
    assert int((got["hist"] - hist_pattern(Cn, dev)).sum()) == int(((lt >= 0) & (lt < Cn)).sum())
    # a subset of the outputs: the same bits, and the buffers not asked for stay as they were
    part = fused_raw(L, x, plan, lt, hist_pattern(Cn, dev), dev, outputs=("u8", "hist"))
    assert torch.equal(part["u8"], got["u8"]) and torch.equal(part["hist"], got["hist"])
    part = fused_raw(L, x, plan, lt, hist_pattern(Cn, dev), dev, outputs=("prob",))
    assert torch.equal(part["prob"], got["prob"])
    # the Python entry: the fused launch and the chain behind SSCG_FUSE_SLIDING=0 return the same objects
    outs = []
    try:
        for fuse in (True, False):
            F.FUSE_SLIDING[0] = fuse
            outs.append(F.predict_labels_sw(x, plan, want_prob=True, want_index=True, label_true=lt, hist=hist_pattern(Cn, dev).clone()))
    finally:
        F.FUSE_SLIDING[0] = True
    for a, b in zip(*outs):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    assert torch.equal(outs[0][0], got["u8"]) and torch.equal(outs[0][1], got["index"]) and torch.equal(outs[0][2], got["hist"])
    assert torch.equal(outs[0][3].permute(0, 2, 3, 1), got["prob"]) and outs[0][3].is_contiguous(memory_format=CL)


# ------------------------------------------------------------------------------------------ 2. one window = sscg_predict_head
@pytest.mark.parametrize("Cn", [4, 20, 21, 5])
def test_one_const_window_equals_predict_head(F, dev, Cn):
    L = load_sub("_lib")
    N, wh, ww = 2, 12, 16
    plan = make_plan(F, dev, wh, ww, wh, ww, 0.5, "const", False)
    assert plan.views == 1
    for h, w in ((5, 7), (12, 16)):
        x = make_logits(Cn, N, plan, h, w, Cn + h, dev)
        lt = make_labels(Cn, N, wh, ww, Cn, dev)
        u8, idx, hist = F.predict_labels(x, (wh, ww), want_index=True, label_true=lt, hist=hist_pattern(Cn, dev).clone())
        soft = F.softmax_fwd(F.upsample_fwd(x, wh, ww))
        got = fused_raw(L, x, plan, lt, hist_pattern(Cn, dev), dev)
        assert torch.equal(got["index"], idx) and torch.equal(got["u8"], u8) and torch.equal(got["hist"], hist)
        assert torch.equal(got["prob"], soft.permute(0, 2, 3, 1))          # weight 1.0, normaliser 1.0


# ------------------------------------------------------------------------------------------ 3. past the grid cap
def test_more_pixels_than_the_grid_holds(F, dev):
    L = load_sub("_lib")
    N, Cn = 1, 4
    plan = make_plan(F, dev, 600, 900, 320, 480, 0.5, "gauss", False)      # 540 000 pixels > 2048 workgroups x 256 threads
    assert (plan.ky, plan.kx) == (3, 3)
    x = make_logits(Cn, N, plan, 41, 61, 4, dev)
    lt = make_labels(Cn, N, 600, 900, 4, dev)
    want_hist = torch.zeros(Cn, Cn, dtype=torch.int64, device=dev)
    _, idx, prob = separate(F, x, plan, lt, want_hist)
    got = fused_raw(L, x, plan, lt, torch.zeros(Cn, Cn, dtype=torch.int64, device=dev), dev)
    assert torch.equal(got["index"], idx) and torch.equal(got["u8"].to(torch.int64), idx) and torch.equal(got["hist"], want_hist)
    assert torch.equal(got["prob"], prob.permute(0, 2, 3, 1))
    assert int(got["hist"].sum()) == int(((lt >= 0) & (lt < Cn)).sum())


# ------------------------------------------------------------------------------------------ 4. an independent check against fp64
def test_probabilities_and_labels_agree_with_the_fp64_restatement(F, dev):
    """Figures of the first MI355X run are printed below; the bounds are the issue's (1e-5 absolute on the probabilities; labels equal
    wherever the fp64 top two are 1e-4 apart; at most 1 % of the pixels left out by that margin)."""
    L = load_sub("_lib")
    Cn, N = 21, 2
    OH, OW, wh, ww, h, w, overlap, blend, flip = CASES[0]
    for (overlap, blend, flip) in ((overlap, blend, flip), (0.75, "gauss", True), (0.0, "const", False)):
        plan = make_plan(F, dev, OH, OW, wh, ww, overlap, blend, flip)
        x = make_logits(Cn, N, plan, h, w, 2100, dev, scale=4.0)
        lt = make_labels(Cn, N, OH, OW, Cn, dev)
        ref, ref_labels = R.blend64(x.permute(0, 2, 3, 1).cpu().numpy(), N, OH, OW, wh, ww, overlap, blend, plan.options.sigma, flip)
        got = fused_raw(L, x, plan, lt, hist_pattern(Cn, dev), dev)
        top2 = np.sort(ref, axis=3)[..., -2:]
        clear = (top2[..., 1] - top2[..., 0]) >= 1e-4
        err = float(np.abs(got["prob"].double().cpu().numpy() - ref).max())
        print("overlap %.2f %s flip=%s: max |prob - fp64| %.3e; %d of %d pixels within 1e-4 of a tie" % (
            overlap, blend, flip, err, int((~clear).sum()), clear.size))
        assert 1.0 - clear.mean() <= 0.01
        assert (got["index"].cpu().numpy()[clear] == ref_labels[clear]).all()
        assert err <= 1e-5, err
        assert float(np.abs(ref.sum(axis=3) - 1).max()) < 1e-12          # the reference's normalisation is one


# ------------------------------------------------------------------------------------------ 5. window_gather
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("Cn", [3, 1])
def test_window_gather_equals_slicing(F, dev, Cn, flip):
    L = load_sub("_lib")
    for (OH, OW, wh, ww, overlap) in ((23, 29, 12, 16, 0.5), (23, 29, 12, 16, 0.75), (97, 113, 65, 65, 0.5)):
        plan = make_plan(F, dev, OH, OW, wh, ww, overlap, "gauss", flip)
        N = 2
        g = torch.Generator().manual_seed(OH + Cn)
        img = torch.randn(N, Cn, OH, OW, generator=g).to(dev).contiguous(memory_format=CL)
        wins = []
        for n in range(N):
            for py in plan.pos_y:
                for px in plan.pos_x:
                    t = img[n, :, py:py + wh, px:px + ww]
                    wins.append(t)
                    if flip:
                        wins.append(torch.flip(t, dims=(2,)))
        want = torch.stack(wins)
        buf, y = guarded(want.numel(), torch.float32, dev)
        rc = L.lib.sscg_window_gather(img.data_ptr(), y.data_ptr(), N, OH, OW, Cn, wh, ww, plan.sy, plan.sx, plan.ky, plan.kx, int(flip),
                                      torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert guards_intact(buf) and not bool(torch.isnan(y).any())
        assert torch.equal(y.view(N * plan.views, wh, ww, Cn), want.permute(0, 2, 3, 1))
        outs = []
        try:
            for fuse in (True, False):
                F.FUSE_SLIDING[0] = fuse
                outs.append(F.window_gather(img, plan))
        finally:
            F.FUSE_SLIDING[0] = True
        for got in outs:
            assert got.shape == want.shape and torch.equal(got, want) and got.is_contiguous(memory_format=CL)
    one = make_plan(F, dev, 12, 16, 12, 16, 0.5, "gauss", False)
    img = torch.randn(2, Cn, 12, 16).to(dev)
    assert F.window_gather(img, one) is img                              # one unmirrored window: the batch itself, no launch
    mirrored = make_plan(F, dev, 12, 16, 12, 16, 0.5, "gauss", True)
    got = F.window_gather(img, mirrored)
    assert torch.equal(got[0::2], img) and torch.equal(got[1::2], torch.flip(img, dims=(3,)))


# ------------------------------------------------------------------------------------------ 6. network level
def _model(dev, tmp_path, size=(97, 113)):
    FX = __import__("oracle.fixtures", fromlist=["x"])
    md = load_sub("model")
    args = FX.make_args(dataset="acdc", crop_height=65, crop_width=65, batch_size=2, gpu_ids=[dev.index or 0], ngf=8,
                        model="supervised_model", checkpoint_dir=str(tmp_path / "ckpt"), as_written=True)
    torch.manual_seed(12)
    with contextlib.redirect_stdout(io.StringIO()):
        m = md.supervised_model(args)                # Gsi = define_Gen(3, 4, 8, 'deeplab', ...)
    g = torch.Generator().manual_seed(13)
    gt = torch.randint(0, 4, (2, 1) + size, generator=g)
    gt.view(-1)[::9] = 255
    return m, [(torch.randn(2, 3, *size, generator=g), gt, ["a", "b"])]


def _evaluate(m, batches, **kw):
    """(confusion matrix, mIoU) of one evaluate(); supervised_model.evaluate() resets the matrix after get_scores(), so keep it."""
    score, conf = m.running_metrics_val, []
    fold = score._fold_device

    def keep():
        fold()
        conf[:] = [score.confusion_matrix.copy()]

    score._fold_device = keep
    m.set_sliding(kw.pop("sliding", None))           # the option is state of the model: evaluate()'s parameter list stays
    try:
        miou, _ = m.evaluate(batches, **kw)
    finally:
        del score._fold_device
        m.set_sliding(None)
    return conf[0], miou


def test_evaluate_with_windows_fused_equals_the_separate_passes(F, dev, tmp_path):
    U = load_sub("utils")
    m, batches = _model(dev, tmp_path)
    before = {k: v.clone() for k, v in m.Gsi.state_dict().items()}
    opts = U.parse_sliding("size=97x113,overlap=0.5,flip", (65, 65))
    try:
        F.FUSE_SLIDING[0] = True
        conf_f, miou_f = _evaluate(m, batches, sliding=opts)
        assert m.Gsi.training
        F.FUSE_SLIDING[0] = False
        conf_s, miou_s = _evaluate(m, batches, sliding=opts)
    finally:
        F.FUSE_SLIDING[0] = True
    counted = sum(int((gt != 255).sum()) for _, gt, _ in batches)
    assert conf_f.sum() == counted and (conf_f == conf_s).all() and miou_f == miou_s
    assert m.Gsi.training
    after = m.Gsi.state_dict()
    assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)
    # the evaluation size == the crop, constant blend, no mirror: one window, the plain evaluation
    g = torch.Generator().manual_seed(17)
    gt = torch.randint(0, 4, (2, 1, 65, 65), generator=g)
    gt.view(-1)[::9] = 255
    small = [(torch.randn(2, 3, 65, 65, generator=g), gt, ["a", "b"])]
    conf_1, miou_1 = _evaluate(m, small, sliding=U.parse_sliding("scale=1,blend=const", (65, 65)))
    conf_0, miou_0 = _evaluate(m, small)
    assert (conf_1 == conf_0).all() and miou_1 == miou_0
    m.set_sliding(opts)
    with pytest.raises(ValueError):
        m.evaluate(small, tta=U.parse_tta("0.5,1.0"))
    m.set_sliding(None)
    assert m.Gsi.training
    with pytest.raises(ValueError):
        m.set_sliding(U.parse_sliding("scale=2", (64, 64)))               # another window than the crop


CENSUS = r"""
import contextlib, io, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
from conftest import load_sub
from oracle import fixtures as FX
md, U = load_sub("model"), load_sub("utils")
args = FX.make_args(dataset="acdc", crop_height=65, crop_width=65, batch_size=2, gpu_ids=[0], ngf=8, model="supervised_model",
                    checkpoint_dir=%r, as_written=True)
with contextlib.redirect_stdout(io.StringIO()):
    m = md.supervised_model(args)
g = torch.Generator().manual_seed(1)
batches = [(torch.randn(2, 3, 97, 113, generator=g), torch.randint(0, 4, (2, 1, 97, 113), generator=g), ["a", "b"]) for _ in range(2)]
opts = U.parse_sliding("size=97x113,overlap=0.5,flip", (65, 65))
calls = [0]
m.Gsi.register_forward_hook(lambda *a: calls.__setitem__(0, calls[0] + 1))
m.set_sliding(opts)
m.evaluate(batches[:1])          # operand copies are made here
torch.cuda.synchronize()
calls[0] = 0
sys.stderr.write("[census] begin\n")
m.evaluate(batches)
torch.cuda.synchronize()
sys.stderr.write("[census] end\n")
sys.stderr.write("[census] forwards %%d\n" %% calls[0])
"""


def test_launch_census_of_an_evaluation_with_windows(tmp_path):
    counts, forwards = {}, {}
    for fuse in ("1", "0"):
        env = dict(os.environ, SSCG_TRACE="1", SSCG_FUSE_SLIDING=fuse)
        r = subprocess.run([sys.executable, "-c", CENSUS % (ROOT, os.path.join(ROOT, "tests"), str(tmp_path / "ckpt"))], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        body = r.stderr[r.stderr.index("[census] begin"):r.stderr.index("[census] end")]
        calls = {}
        for line in body.splitlines():
            if line.startswith("[sscg] "):
                name = line[7:].split("(")[0]
                calls[name] = calls.get(name, 0) + 1
        counts[fuse] = calls
        forwards[fuse] = int(r.stderr.rsplit("[census] forwards ", 1)[1].split()[0])
    fused, plain = counts["1"], counts["0"]
    # two batches of 2 samples x (2 x 3 windows) x 2 views = 24 windows each, 2 per forward
    assert forwards["1"] == 2 * 12 and forwards["0"] == 2 * 12, forwards
    assert fused.get("sscg_window_gather", 0) == 2 and fused.get("sscg_predict_head_sw", 0) == 2, fused
    assert fused.get("sscg_softmax_fwd", 0) == 0 and fused.get("sscg_upsample_bilinear_fwd", 0) == 0, fused
    assert fused.get("sscg_argmax_onehot", 0) == 0 and fused.get("sscg_confusion_hist", 0) == 0, fused
    assert plain.get("sscg_window_gather", 0) == 0 and plain.get("sscg_predict_head_sw", 0) == 0, plain
    assert plain.get("sscg_softmax_fwd", 0) == 2 * 12 and plain.get("sscg_confusion_hist", 0) == 2, plain


# ------------------------------------------------------------------------------------------ 8. with the other evaluation options
def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(p, q) for p, q in zip(a, b))
    try:
        return bool(np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True))
    except TypeError:           # not numbers
        return a == b


def test_windows_combine_with_the_other_evaluation_options(F, dev, tmp_path):
    U = load_sub("utils")
    m, batches = _model(dev, tmp_path)
    opts = U.parse_sliding("size=97x113,overlap=0.5", (65, 65))
    crf = U.parse_crf("iters=2,radius=1")
    m.set_surface(U.parse_surface("on"))
    m.set_components(U.parse_components("on"))
    m.set_calibration(U.parse_calibration("on"), crf=crf, sliding=opts)
    records = []
    try:
        for fuse in (True, False):
            F.FUSE_SLIDING[0] = fuse
            for use_crf in (crf, None):
                conf, miou = _evaluate(m, batches, sliding=opts, crf=use_crf, boundary=U.parse_boundary("on"))
                records.append((conf, miou, dict(m.eval_boundary), dict(m.eval_surface), dict(m.eval_components), dict(m.eval_calibration)))
    finally:
        F.FUSE_SLIDING[0] = True
    counted = sum(int((gt != 255).sum()) for _, gt, _ in batches)
    for fused, chain in ((records[0], records[2]), (records[1], records[3])):
        assert fused[0].sum() == counted and (fused[0] == chain[0]).all() and fused[1] == chain[1]
        for a, b in zip(fused[2:], chain[2:]):
            assert _same(a, b)
    assert records[0][5]["counted"] == counted and records[1][5]["counted"] == counted
    with pytest.raises(ValueError):
        m.set_calibration(U.parse_calibration("fit"), sliding=opts)          # a temperature grid has no logits to rescale here


# ------------------------------------------------------------------------------------------ 9. drivers
def test_validation_driver_writes_the_same_label_bytes_either_way(F, dev, tmp_path):
    sys.path.insert(0, ROOT)
    import validation as vdrv
    FX = __import__("oracle.fixtures", fromlist=["x"])
    arch, U = load_sub("arch"), load_sub("utils")
    torch.manual_seed(21)
    with contextlib.redirect_stdout(io.StringIO()):
        net = arch.define_Gen(3, 4, 8, "deeplab", "instance", False, [dev.index or 0])
    ck = tmp_path / "ckpt"
    os.makedirs(ck)
    U.save_checkpoint({"epoch": 1, "Gsi": net.state_dict(), "best_iou": 0.25}, str(ck / "latest_supervised_model.ckpt"))
    g = torch.Generator().manual_seed(22)
    batches = [(torch.randn(2, 3, 97, 113, generator=g), torch.randint(0, 4, (2, 1, 97, 113), generator=g), ["s0", "s1"])]
    png = {}
    try:
        for fuse in (True, False):
            F.FUSE_SLIDING[0] = fuse
            args = FX.make_args(dataset="acdc", crop_height=65, crop_width=65, batch_size=2, gpu_ids=[dev.index or 0], ngf=8,
                                model="supervised_model", checkpoint_dir=str(ck), validation_dir=str(tmp_path / ("val%d" % fuse)),
                                sliding="size=97x113,overlap=0.5,flip")
            with contextlib.redirect_stdout(io.StringIO()):
                assert vdrv.validation(args, batches) == 0.25
            png[fuse] = [open(os.path.join(args.validation_dir, "supervised", n + ".png"), "rb").read() for n in ("s0", "s1")]
    finally:
        F.FUSE_SLIDING[0] = True
    assert png[True] == png[False] and all(len(b) > 0 for b in png[True])
    from PIL import Image
    im = Image.open(os.path.join(str(tmp_path / "val1"), "supervised", "s0.png"))
    assert im.mode == "P" and im.size == (113, 97) and int(np.asarray(im).max()) < 4
