"""Multi-scale / mirrored inference on the MI355X: sscg_predict_head_ms (the views of one batch fused into one label map in one
launch) and sscg_resize_flip (the network input of a view).  The contract is BIT IDENTITY with the chain of separate passes - per view
sscg_upsample_bilinear_fwd, a mirror of the W axis where flagged, sscg_softmax_fwd, an fp32 add into the accumulator; then
sscg_argmax_onehot's index and sscg_confusion_hist - so every comparison with them is torch.equal.  An fp64 restatement in numpy, which
shares no code with either path, guards the meaning of the mirror and of the view order.

fp64 figures of test 5 (the six-view inputs, C in {4, 7, 20, 21, 64}): the test prints them; PROB_SUM_MEASURED below and
profiles/tta.txt take the figure of the first MI355X run (not made yet: until then the bound is its ceiling, 1e-5 x S)."""
import contextlib
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_sub

pytestmark = pytest.mark.gpu
CL = torch.channels_last
GUARD = 64
SENT = {torch.float32: float("nan"), torch.int64: -7777, torch.uint8: 0xEE}
OH = 17
SIZES = lambda ow: [(17, ow), (3, 5), (1, 1), (5, 9), (17, 1), (9, 17)]      # the first is the identity-size member


def guarded(n, dtype, dev):
    """(buffer, view of n elements GUARD elements into it): the whole buffer holds the sentinel of its dtype."""
    buf = torch.full((n + 2 * GUARD,), SENT[dtype], dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf):
    g = torch.cat([buf[:GUARD], buf[-GUARD:]])
    return bool(torch.isnan(g).all()) if buf.is_floating_point() else bool((g == SENT[buf.dtype]).all())


def make_views(Cn, S, N, ow, seed, dev):
    """S logit maps [N, Cn, h, w] (channels-last memory), `randn * 3`, sizes cycling through SIZES(ow)."""
    g = torch.Generator().manual_seed(seed)
    sizes = SIZES(ow)
    return [(torch.randn(N, Cn, *sizes[s % len(sizes)], generator=g) * 3).to(dev).contiguous(memory_format=CL) for s in range(S)]


def make_labels(Cn, N, oh, ow, seed, dev):
    g = torch.Generator().manual_seed(seed + 1000)
    lt = torch.randint(0, Cn, (N, oh, ow), generator=g)
    flat = lt.view(-1)
    flat[0::7] = -1
    flat[3::11] = 255
    flat[5::13] = Cn
    return lt.to(dev)


def flip_list(kind, S):
    return [kind == "all" or (kind == "alt" and s % 2 == 1) for s in range(S)]


def separate(F, xs, flips, size, lt=None, hist=None):
    """The chain of separate passes, every pass a launch of an entry that existed before (the resize also at the identity size)."""
    acc = None
    for x, flip in zip(xs, flips):
        p = F.softmax_fwd(F.upsample_fwd(F.to_nhwc(x), size[0], size[1]))
        if flip:
            p = torch.flip(p, dims=(3,))
        acc = p if acc is None else acc + p
    idx = F.argmax_index(acc)
    if lt is not None:
        F.confusion_hist(lt, idx, xs[0].shape[1], hist)
    return acc, idx


def fused_raw(L, xs, flips, size, lt, hist_init, dev):
    """sscg_predict_head_ms itself, every output a view into a sentinel-filled buffer.  Returns (prob [N,OH,OW,C], index, u8, hist)."""
    N, Cn = xs[0].shape[:2]
    oh, ow = size
    S = len(xs)
    pb, prob = guarded(N * oh * ow * Cn, torch.float32, dev)
    ib, index = guarded(N * oh * ow, torch.int64, dev)
    ub, u8 = guarded(N * oh * ow, torch.uint8, dev)
    hb, hist = guarded(Cn * Cn, torch.int64, dev)
    hist.copy_(hist_init.view(-1))
    mask = sum(1 << s for s, f in enumerate(flips) if f)
    ptrs = (C.c_void_p * S)(*[x.data_ptr() for x in xs])
    hs = (C.c_int * S)(*[x.shape[2] for x in xs])
    ws = (C.c_int * S)(*[x.shape[3] for x in xs])
    rc = L.lib.sscg_predict_head_ms(ptrs, hs, ws, S, mask, N, Cn, oh, ow, prob.data_ptr(), index.data_ptr(), u8.data_ptr(),
                                    lt.data_ptr(), hist.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for b in (pb, ib, ub, hb):
        assert guards_intact(b), "a store outside the %s output" % b.dtype
    return prob.view(N, oh, ow, Cn), index.view(N, oh, ow), u8.view(N, oh, ow), hist.view(Cn, Cn)


def hist_pattern(Cn, dev):
    return (torch.arange(Cn * Cn, dtype=torch.int64, device=dev) * 3 + 1).view(Cn, Cn)


# ------------------------------------------------------------------------------------------ 1. the head against the separate passes
@pytest.mark.parametrize("ow", [33, 32])
@pytest.mark.parametrize("Cn", [4, 20, 21, 7, 64])
def test_head_equals_the_separate_passes(F, dev, Cn, ow):
    L = load_sub("_lib")
    for N in (1, 2):
        lt = make_labels(Cn, N, OH, ow, Cn + N, dev)
        for S in (1, 2, 3, 6, 8):
            xs = make_views(Cn, S, N, ow, 100 * Cn + 10 * S + N, dev)
            for kind in ("none", "all", "alt"):
                flips = flip_list(kind, S)
                what = "C=%d OW=%d N=%d S=%d flips=%s" % (Cn, ow, N, S, kind)
                want_hist = hist_pattern(Cn, dev).clone()
                acc, idx = separate(F, xs, flips, (OH, ow), lt, want_hist)
                prob, index, u8, hist = fused_raw(L, xs, flips, (OH, ow), lt, hist_pattern(Cn, dev), dev)
                assert torch.equal(prob, acc.permute(0, 2, 3, 1)), "%s: %d of %d summed probabilities differ" % (
                    what, int((prob != acc.permute(0, 2, 3, 1)).sum()), prob.numel())
                assert torch.equal(index, idx), "%s: %d labels differ" % (what, int((index != idx).sum()))
                assert torch.equal(u8.to(torch.int64), idx), what
                assert torch.equal(hist, want_hist), what
    # the Python entry: the fused launch and the chain behind SSCG_FUSE_TTA=0 return the same objects
    outs = []
    try:
        for fuse in (True, False):
            F.FUSE_TTA[0] = fuse
            outs.append(F.predict_labels_ms(xs, flips, (OH, ow), want_prob=True, want_index=True, label_true=lt, hist=hist_pattern(Cn, dev).clone()))
    finally:
        F.FUSE_TTA[0] = True
    for a, b in zip(*outs):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    assert torch.equal(outs[0][1], index) and torch.equal(outs[0][2], hist) and torch.equal(outs[0][3].permute(0, 2, 3, 1), prob)
    assert outs[0][3].is_contiguous(memory_format=CL)


# ------------------------------------------------------------------------------------------ 2. one view = sscg_predict_head
@pytest.mark.parametrize("Cn", [4, 20, 21, 7, 64])
def test_one_unmirrored_view_equals_predict_head(F, dev, Cn):
    L = load_sub("_lib")
    for N, (h, w) in ((2, (5, 9)), (1, (OH, 33)), (2, (1, 1))):
        g = torch.Generator().manual_seed(Cn + h)
        x = (torch.randn(N, Cn, h, w, generator=g) * 3).to(dev).contiguous(memory_format=CL)
        lt = make_labels(Cn, N, OH, 33, Cn, dev)
        u8, idx, hist = F.predict_labels(x, (OH, 33), want_index=True, label_true=lt, hist=hist_pattern(Cn, dev).clone())
        _, index, label, got_hist = fused_raw(L, [x], [False], (OH, 33), lt, hist_pattern(Cn, dev), dev)
        assert torch.equal(index, idx) and torch.equal(label, u8) and torch.equal(got_hist, hist)


# ------------------------------------------------------------------------------------------ 3. forced ties
def test_forced_ties_name_the_first_maximum(F, dev):
    L = load_sub("_lib")
    Cn, N = 7, 2
    xs = make_views(Cn, 3, N, 33, 77, dev)
    for x in xs:
        x[:, 2] += 10.0
        x[:, 5] = x[:, 2]               # classes 2 and 5 carry the same logits everywhere: the summed probabilities tie exactly
    lt = make_labels(Cn, N, OH, 33, 7, dev)
    flips = [False, True, False]
    acc, idx = separate(F, xs, flips, (OH, 33))
    _, index, u8, _ = fused_raw(L, xs, flips, (OH, 33), lt, hist_pattern(Cn, dev), dev)
    assert bool((acc[:, 2] == acc[:, 5]).all())
    assert bool((idx == 2).all()) and bool((index == 2).all()) and bool((u8 == 2).all())
    # a tie that exists only in the SUM: view 0 favours class 1 by exactly what view 1 favours class 3, on constant maps
    Cn = 5
    a = torch.full((N, Cn, 5, 9), -1.0)
    b = a.clone()
    a[:, 1], a[:, 3] = 2.0, 0.0
    b[:, 1], b[:, 3] = 0.0, 2.0
    xs = [t.to(dev).contiguous(memory_format=CL) for t in (a, b)]
    lt = make_labels(Cn, N, OH, 33, 9, dev)
    for flips in ([False, False], [False, True]):
        want_hist = hist_pattern(Cn, dev).clone()
        acc, idx = separate(F, xs, flips, (OH, 33), lt, want_hist)
        prob, index, u8, hist = fused_raw(L, xs, flips, (OH, 33), lt, hist_pattern(Cn, dev), dev)
        assert torch.equal(prob, acc.permute(0, 2, 3, 1)) and torch.equal(index, idx) and torch.equal(hist, want_hist)
        assert bool(((index == 1) | (index == 3)).all())
        assert float((acc[:, 1] - acc[:, 3]).abs().max()) < 1e-6          # the two classes do meet in the sum


# ------------------------------------------------------------------------------------------ 4. past the grid cap
def test_more_pixels_than_the_grid_holds(F, dev):
    L = load_sub("_lib")
    N, Cn, oh, ow = 2, 4, 600, 450           # 540 000 pixels > 2048 workgroups x 256 threads: the grid-stride loop runs twice
    g = torch.Generator().manual_seed(4)
    xs = [(torch.randn(N, Cn, h, w, generator=g) * 3).to(dev).contiguous(memory_format=CL) for h, w in ((9, 7), (5, 5))]
    lt = make_labels(Cn, N, oh, ow, 4, dev)
    flips = [False, True]
    want_hist = torch.zeros(Cn, Cn, dtype=torch.int64, device=dev)
    _, idx = separate(F, xs, flips, (oh, ow), lt, want_hist)
    _, index, u8, hist = fused_raw(L, xs, flips, (oh, ow), lt, torch.zeros(Cn, Cn, dtype=torch.int64, device=dev), dev)
    assert torch.equal(index, idx) and torch.equal(u8.to(torch.int64), idx) and torch.equal(hist, want_hist)
    assert int(hist.sum()) == int(((lt >= 0) & (lt < Cn)).sum())


# ------------------------------------------------------------------------------------------ 5. an independent check against fp64
def resize64(x, oh, ow):
    """Bilinear resize with align_corners=True of a [N, H, W, C] float64 array."""
    N, H, W, Cn = x.shape
    fy = np.arange(oh, dtype=np.float64) * ((H - 1) / (oh - 1) if oh > 1 else 0.0)
    fx = np.arange(ow, dtype=np.float64) * ((W - 1) / (ow - 1) if ow > 1 else 0.0)
    y0, x0 = np.minimum(np.floor(fy).astype(int), H - 1), np.minimum(np.floor(fx).astype(int), W - 1)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    ly, lx = (fy - y0)[None, :, None, None], (fx - x0)[None, None, :, None]
    top = x[:, y0][:, :, x0] * (1 - lx) + x[:, y0][:, :, x1] * lx
    bot = x[:, y1][:, :, x0] * (1 - lx) + x[:, y1][:, :, x1] * lx
    return top * (1 - ly) + bot * ly


def fused64(xs, flips, oh, ow):
    total = 0.0
    for x, flip in zip(xs, flips):
        r = resize64(x.permute(0, 2, 3, 1).double().cpu().numpy(), oh, ow)
        if flip:
            r = r[:, :, ::-1]
        e = np.exp(r - r.max(axis=3, keepdims=True))
        total = total + e / e.sum(axis=3, keepdims=True)
    return total


# Largest |prob_sum - fp64 sum| over the five class counts on the first MI355X run (profiles/tta.txt; the separate passes' own
# distance on the same inputs is printed beside it).  The bound is 4x that, for expf differences between ROCm versions, and never
# looser than 1e-5 x S.  None = not measured yet: the ceiling alone holds (torch's CPU fp32 chain is 3.6e-7 .. 6.9e-7 from the
# same restatement on these inputs).
PROB_SUM_MEASURED = None
S5 = 6


@pytest.mark.parametrize("Cn", [4, 7, 20, 21, 64])
def test_labels_and_sums_agree_with_an_fp64_restatement(F, dev, Cn):
    L = load_sub("_lib")
    N, ow = 2, 33
    xs = make_views(Cn, S5, N, ow, 100 * Cn + 10 * S5 + N, dev)          # test 1's six-view inputs
    flips = flip_list("alt", S5)
    lt = make_labels(Cn, N, OH, ow, Cn + N, dev)
    ref = fused64(xs, flips, OH, ow)
    prob, index, _, _ = fused_raw(L, xs, flips, (OH, ow), lt, hist_pattern(Cn, dev), dev)
    acc, _ = separate(F, xs, flips, (OH, ow))
    top2 = np.sort(ref, axis=3)[..., -2:]
    clear = (top2[..., 1] - top2[..., 0]) >= 1e-4
    left_out = 1.0 - clear.mean()
    err = float(np.abs(prob.double().cpu().numpy() - ref).max())
    err_sep = float(np.abs(acc.permute(0, 2, 3, 1).double().cpu().numpy() - ref).max())
    print("C=%d: max |prob_sum - fp64| fused %.3e, separate passes %.3e; %d of %d pixels within 1e-4 of a tie" % (
        Cn, err, err_sep, int((~clear).sum()), clear.size))
    assert left_out <= 0.01
    assert (index.cpu().numpy()[clear] == ref.argmax(axis=3)[clear]).all()
    bound = 1e-5 * S5 if PROB_SUM_MEASURED is None else min(4 * PROB_SUM_MEASURED, 1e-5 * S5)
    assert err <= bound, (err, bound)


# ------------------------------------------------------------------------------------------ 6. resize_flip
@pytest.mark.parametrize("geom", [((9, 17), (5, 9)), ((5, 9), (9, 17)), ((7, 7), (7, 7)), ((4, 1), (8, 1)), ((6, 6), (1, 1))],
                         ids=["minify", "magnify", "mirror_only", "one_column", "to_one_pixel"])
def test_resize_flip_equals_upsample_then_flip(F, dev, geom):
    L = load_sub("_lib")
    (h, w), (oh, ow) = geom
    for Cn in (1, 3, 4):
        for N in (1, 3):
            g = torch.Generator().manual_seed(h * 100 + w * 10 + Cn + N)
            x = torch.randn(N, Cn, h, w, generator=g).to(dev).contiguous(memory_format=CL)
            up = F.upsample_fwd(x, oh, ow)                       # sscg_upsample_bilinear_fwd itself, also at the identity size
            for flip in (0, 1):
                buf, y = guarded(N * oh * ow * Cn, torch.float32, dev)
                rc = L.lib.sscg_resize_flip(x.data_ptr(), y.data_ptr(), N, h, w, Cn, oh, ow, flip, torch.cuda.current_stream().cuda_stream)
                assert rc == 0
                torch.cuda.synchronize()
                want = torch.flip(up, dims=(3,)) if flip else up
                assert guards_intact(buf)
                assert torch.equal(y.view(N, oh, ow, Cn), want.permute(0, 2, 3, 1)), (geom, Cn, N, flip)
                got = F.resize_flip(x, (oh, ow), bool(flip))
                assert torch.equal(got, want) and got.shape == want.shape
                if not flip and (oh, ow) == (h, w):
                    assert got is x                              # nothing to do: the batch itself, no launch


# ------------------------------------------------------------------------------------------ 7. network level
def _model(dev, tmp_path):
    FX = __import__("oracle.fixtures", fromlist=["x"])
    md = load_sub("model")
    args = FX.make_args(dataset="acdc", crop_height=65, crop_width=65, batch_size=2, gpu_ids=[dev.index or 0], ngf=8,
                        model="supervised_model", checkpoint_dir=str(tmp_path / "ckpt"), as_written=True)
    torch.manual_seed(12)
    with contextlib.redirect_stdout(io.StringIO()):
        m = md.supervised_model(args)                # Gsi = define_Gen(3, 4, 8, 'deeplab', ...)
    g = torch.Generator().manual_seed(13)
    batches = []
    for _ in range(2):
        gt = torch.randint(0, 4, (2, 1, 65, 65), generator=g)
        gt.view(-1)[::9] = 255
        batches.append((torch.randn(2, 3, 65, 65, generator=g), gt, ["a", "b"]))
    return m, batches


def _evaluate(m, batches, **kw):
    """(confusion matrix, mIoU) of one evaluate(); supervised_model.evaluate() resets the matrix after get_scores(), so keep it."""
    score, conf = m.running_metrics_val, []
    fold = score._fold_device

    def keep():
        fold()
        conf[:] = [score.confusion_matrix.copy()]

    score._fold_device = keep
    try:
        miou, _ = m.evaluate(batches, **kw)
    finally:
        del score._fold_device
    return conf[0], miou


def test_evaluate_with_views_fused_equals_the_separate_passes(F, dev, tmp_path):
    U = load_sub("utils")
    m, batches = _model(dev, tmp_path)
    before = {k: v.clone() for k, v in m.Gsi.state_dict().items()}
    views = U.parse_tta("0.5,1.0:flip")
    try:
        F.FUSE_TTA[0] = True
        conf_f, miou_f = _evaluate(m, batches, tta=views)
        assert m.Gsi.training
        F.FUSE_TTA[0] = False
        conf_s, miou_s = _evaluate(m, batches, tta=views)
    finally:
        F.FUSE_TTA[0] = True
    counted = sum(int((gt != 255).sum()) for _, gt, _ in batches)
    assert conf_f.sum() == counted and (conf_f == conf_s).all() and miou_f == miou_s
    conf_1, miou_1 = _evaluate(m, batches, tta=U.parse_tta("1.0"))
    conf_0, miou_0 = _evaluate(m, batches)
    assert (conf_1 == conf_0).all() and miou_1 == miou_0          # one unscaled view is the plain evaluation
    assert m.Gsi.training
    after = m.Gsi.state_dict()
    assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)


def test_semisupervised_evaluate_takes_the_views(F, dev, tmp_path):
    FX = __import__("oracle.fixtures", fromlist=["x"])
    md, U = load_sub("model"), load_sub("utils")
    args = FX.make_args(dataset="acdc", crop_height=65, crop_width=65, batch_size=2, gpu_ids=[dev.index or 0], ngf=8,
                        checkpoint_dir=str(tmp_path / "ckpt"), as_written=True)
    torch.manual_seed(14)
    with contextlib.redirect_stdout(io.StringIO()):
        m = md.semisuper_cycleGAN(args)
    g = torch.Generator().manual_seed(15)
    gt = torch.randint(0, 4, (2, 1, 65, 65), generator=g)
    gt.view(-1)[::5] = 255
    batches = [(torch.randn(2, 3, 65, 65, generator=g), gt, ["a", "b"])]
    before = {k: v.clone() for k, v in m.Gsi.state_dict().items()}
    views = U.parse_tta("0.5,1.0:flip")
    confs = []
    try:
        for fuse in (True, False):
            F.FUSE_TTA[0] = fuse
            miou, _ = m.evaluate(batches, tta=views)
            confs.append((m.running_metrics_val.confusion_matrix.copy(), miou))
            assert m.Gsi.training and m.Gis.training
    finally:
        F.FUSE_TTA[0] = True
    assert confs[0][0].sum() == int((gt != 255).sum()) and (confs[0][0] == confs[1][0]).all() and confs[0][1] == confs[1][1]
    after = m.Gsi.state_dict()
    assert all(torch.equal(after[k], before[k]) for k in before)


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
batches = [(torch.randn(2, 3, 65, 65, generator=g), torch.randint(0, 4, (2, 1, 65, 65), generator=g), ["a", "b"]) for _ in range(2)]
views = U.parse_tta("0.5,1.0:flip")
m.evaluate(batches[:1], tta=views)          # operand copies are made here
torch.cuda.synchronize()
sys.stderr.write("[census] begin\n")
m.evaluate(batches, tta=views)
torch.cuda.synchronize()
sys.stderr.write("[census] end\n")
"""


def test_launch_census_of_an_evaluation_with_views(tmp_path):
    counts = {}
    for fuse in ("1", "0"):
        env = dict(os.environ, SSCG_TRACE="1", SSCG_FUSE_TTA=fuse)
        r = subprocess.run([sys.executable, "-c", CENSUS % (ROOT, os.path.join(ROOT, "tests"), str(tmp_path / "ckpt"))], env=env,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        body = r.stderr[r.stderr.index("[census] begin"):r.stderr.index("[census] end")]
        calls = {}
        for line in body.splitlines():
            if line.startswith("[sscg] "):
                name = line[7:].split("(")[0]
                calls[name] = calls.get(name, 0) + 1
        counts[fuse] = calls
    fused, plain = counts["1"], counts["0"]
    # two batches of four views: (0.5, 0.5 mirrored, 1.0, 1.0 mirrored) - the unmirrored 1.0 view is the batch itself
    assert fused.get("sscg_predict_head_ms", 0) == 2 and fused.get("sscg_resize_flip", 0) == 2 * 3, fused
    assert fused.get("sscg_softmax_fwd", 0) == 0 and fused.get("sscg_upsample_bilinear_fwd", 0) == 0, fused
    assert fused.get("sscg_argmax_onehot", 0) == 0 and fused.get("sscg_confusion_hist", 0) == 0, fused
    assert plain.get("sscg_predict_head_ms", 0) == 0 and plain.get("sscg_softmax_fwd", 0) == 2 * 4, plain
    assert plain.get("sscg_upsample_bilinear_fwd", 0) == 2 * 4 and plain.get("sscg_confusion_hist", 0) == 2, plain


# ------------------------------------------------------------------------------------------ 8. drivers
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
    batches = [(torch.randn(2, 3, 64, 96, generator=g), torch.randint(0, 4, (2, 1, 64, 96), generator=g), ["s0", "s1"])]
    png = {}
    try:
        for fuse in (True, False):
            F.FUSE_TTA[0] = fuse
            args = FX.make_args(dataset="acdc", crop_height=64, crop_width=96, batch_size=2, gpu_ids=[dev.index or 0], ngf=8,
                                model="supervised_model", checkpoint_dir=str(ck), validation_dir=str(tmp_path / ("val%d" % fuse)),
                                tta="0.75,1.0:flip")
            with contextlib.redirect_stdout(io.StringIO()):
                assert vdrv.validation(args, batches) == 0.25
            png[fuse] = [open(os.path.join(args.validation_dir, "supervised", n + ".png"), "rb").read() for n in ("s0", "s1")]
    finally:
        F.FUSE_TTA[0] = True
    assert png[True] == png[False] and all(len(b) > 0 for b in png[True])
    from PIL import Image
    im = Image.open(os.path.join(str(tmp_path / "val1"), "supervised", "s0.png"))
    assert im.mode == "P" and im.size == (96, 64) and int(np.asarray(im).max()) < 4
