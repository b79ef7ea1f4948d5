"""Class-weighted, label-smoothed cross entropy on the MI355X: sscg_ce_fwd_w / _bwd_w (flat), sscg_upsample_head_fwd_w (the fused
label head: resize -> softmax -> loss, the forward leaves the gradient) and sscg_label_hist, against torch on the CPU in fp64 -
F.cross_entropy(weight=w, label_smoothing=eps) with every label outside [0, C) mapped to the ignore index.

Tolerance (README): 1e-3 relative for an fp32 result against the fp64 reference; for a gradient the max-abs difference
over the max-abs of the reference gradient.  Two absolute floors cover references that are exactly zero (C = 1: p = 1, every term and
every gradient entry vanishes): 1e-7 on a loss (below fp32's resolution of an O(1) loss), and 8 fp32 roundings of the largest term of a
gradient entry, max(w) / D, on a gradient.  Every test prints the distances it observed (`weighted_ce ...` lines; run with -s).

D == 0 (no counted pixel, or every counted pixel in a weight-0 class): the library's rule is a NaN loss and an all-zero gradient, with
or without smoothing.  torch's loss is NaN in these cases too; torch's gradient is NaN where the library writes zeros (the rule
sscg_ce_fwd always had for "no counted pixel")."""
import contextlib
import io
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from conftest import load_sub

pytestmark = pytest.mark.gpu

CL = torch.channels_last
EPS32 = 2.0 ** -23
GEOMS = [(2, 3, 4, 13, 17), (1, 1, 1, 5, 5), (2, 5, 5, 21, 23), (1, 2, 7, 9, 28)]       # N, H, W -> OH, OW; each OH*OW >= 16*H*W
HEAD_CLASSES = [4, 20, 21, 64]


def gpu(t, dev):
    return t.float().to(dev).contiguous(memory_format=CL) if t.dim() == 4 else t.float().to(dev)


def make_labels(g, shape, C, absent=True):
    """ids in [0, C) - the last class never occurs when `absent` - with the void id 255 and torch's -100 sprinkled in"""
    lab = torch.randint(0, C - 1 if (absent and C > 1) else C, shape, generator=g)
    flat = lab.view(-1)
    flat[::7] = 255
    flat[3::11] = -100
    return lab


def make_weights(g, C):
    """fp32 weights in [0.2, 1.2) with one class at 0"""
    w = (torch.rand(C, generator=g) * 1.0 + 0.2).float()
    w[(C - 1) // 2] = 0.0
    return w


def reference(logits64, lab, w32, eps, resize=None):
    """(loss, gradient with respect to logits64, D) of torch's cross entropy in fp64 on the CPU"""
    C = logits64.shape[1]
    x = logits64.clone().requires_grad_(True)
    up = x if resize is None else TF.interpolate(x, size=resize, mode="bilinear", align_corners=True)
    ref_lab = lab.clone()
    ref_lab[(lab < 0) | (lab >= C)] = -100
    loss = TF.cross_entropy(up, ref_lab, weight=None if w32 is None else w32.double(), label_smoothing=eps, ignore_index=-100)
    counted = ref_lab[ref_lab >= 0]
    D = float(counted.numel()) if w32 is None else float(w32.double()[counted].sum())
    grad = torch.autograd.grad(loss, x)[0] if D > 0 else torch.zeros_like(x)
    return loss.detach(), grad, D


def check(tag, loss, valid, grad, ref, w32):
    """the 1e-3 rule against `ref` = reference(...); returns the two observed distances"""
    ref_loss, ref_grad, D = ref
    loss, grad = float(loss.detach()), grad.detach().double().cpu()
    if valid is not None:
        assert abs(float(valid) - D) <= 1e-6 * D, (tag, float(valid), D)
    if D == 0:
        assert math.isnan(loss) and math.isnan(float(ref_loss)), (tag, loss, float(ref_loss))
        assert torch.count_nonzero(grad) == 0, tag
        return 0.0, 0.0
    wmax = 1.0 if w32 is None else float(w32.max())
    dl, dg = abs(loss - float(ref_loss)), float((grad - ref_grad).abs().max())
    gmax = float(ref_grad.abs().max())
    rl, rg = dl / max(abs(float(ref_loss)), 1e-30), dg / max(gmax, 1e-30)
    print("weighted_ce %-46s loss %.9g ref %.9g rel %.2e | grad max-abs diff %.2e of %.2e rel %.2e" % (tag, loss, float(ref_loss), rl, dg, gmax, rg))
    assert dl <= 1e-3 * abs(float(ref_loss)) + 1e-7, (tag, loss, float(ref_loss))
    assert dg <= 1e-3 * gmax + 8 * EPS32 * wmax / D, (tag, dg, gmax)
    return rl, rg


SETTINGS = [("w", 0.0), (None, 0.1), ("w", 0.1)]


# ------------------------------------------------------------------------------------------ 1. flat cross entropy
@pytest.mark.parametrize("C", [1, 4, 21, 64])
def test_flat_ce_value_and_gradient(C, F, dev):
    g = torch.Generator().manual_seed(100 + C)
    x = torch.randn(2, C, 7, 9, generator=g, dtype=torch.float64) * 2
    lab = make_labels(g, (2, 7, 9), C)
    assert (lab == 255).any() and (lab == -100).any()
    w = make_weights(g, C)
    for wk, eps in [(None, 0.0)] + SETTINGS:
        w32 = w if wk else None
        ref = reference(x, lab, w32, eps)
        xg = gpu(x, dev).requires_grad_(True)
        loss = F.cross_entropy(xg, lab.to(dev), weight=None if w32 is None else F.ce_weight(w32.tolist(), C, dev), label_smoothing=eps)
        valid = loss.grad_fn.saved_tensors[2]              # (read before the backward frees it)
        loss.backward()
        check("flat C=%d w=%s eps=%g" % (C, wk, eps), loss, valid, xg.grad, ref, w32)
        # the upstream gradient scales it
        xg2 = gpu(x, dev).requires_grad_(True)
        F.weighted_sum([F.cross_entropy(xg2, lab.to(dev), weight=None if w32 is None else gpu(w32, dev), label_smoothing=eps)], [0.37]).backward()
        check("flat C=%d w=%s eps=%g x0.37" % (C, wk, eps), loss, None, xg2.grad / 0.37, ref, w32)


# ------------------------------------------------------------------------------------------ 2. the fused head
def run_head(F, dev, x, size, lab, w32, eps, want_soft, fused=True):
    """(y_soft, loss, valid, d loss / d x) of UpsampleHeadFn (fused) or of the three separate passes"""
    C = x.shape[1]
    was = F.FUSE_HEAD[0]
    F.FUSE_HEAD[0] = fused
    try:
        xg = gpu(x, dev).requires_grad_(True)
        assert F._head_applies(xg, *size) == fused
        wd = None if w32 is None else F.ce_weight(w32.tolist(), C, dev)
        if fused:
            y, loss = F.UpsampleHeadFn.apply(xg, size[0], size[1], lab.to(dev), want_soft, wd, eps)
        else:
            y, loss = F.upsample_softmax_ce(xg, size, lab.to(dev), want_soft=want_soft, weight=wd, label_smoothing=eps)
        assert (y is not None) == want_soft
        valid = loss.grad_fn.saved_tensors[2]              # (read before the backward frees it)
        loss.backward()
        return y, loss.detach(), valid, xg.grad
    finally:
        F.FUSE_HEAD[0] = was


@pytest.mark.parametrize("C", HEAD_CLASSES)
@pytest.mark.parametrize("geom", GEOMS)
def test_fused_head_loss_valid_gradient(geom, C, F, dev):
    N, H, W, OH, OW = geom
    g = torch.Generator().manual_seed(1000 * C + H * W)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 2
    lab = make_labels(g, (N, OH, OW), C)                       # class C-1 is absent from the labels
    assert not (lab == C - 1).any()
    w = make_weights(g, C)
    xg = gpu(x, dev)
    y_plain = F.UpsampleHeadFn.apply(xg, OH, OW, lab.to(dev), True)[0]
    assert torch.equal(y_plain, F.UpsampleHeadFn.apply(xg, OH, OW, None, True)[0])
    for wk, eps in SETTINGS:
        w32 = w if wk else None
        ref = reference(x, lab, w32, eps, resize=(OH, OW))
        for want_soft in (True, False):
            y, loss, valid, dx = run_head(F, dev, x, (OH, OW), lab, w32, eps, want_soft)
            check("head %dx%dx%d->%dx%d C=%d w=%s eps=%g soft=%d" % (N, H, W, OH, OW, C, wk, eps, want_soft), loss, valid, dx, ref, w32)
            if want_soft:
                assert torch.equal(y, y_plain)                  # the softmax branch is untouched: the same bits


def test_fused_head_edge_cases(F, dev):
    N, H, W, OH, OW, C = 2, 3, 4, 13, 17, 4
    g = torch.Generator().manual_seed(77)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 2
    w = torch.tensor([0.7, 0.0, 1.1, 0.4])
    # a sample with no counted pixel: it adds nothing, and its logits get a zero gradient
    lab = make_labels(g, (N, OH, OW), C, absent=False)
    lab[1] = 255
    for fused in (True, False):
        for wk, eps in SETTINGS:
            w32 = w if wk else None
            _, loss, valid, dx = run_head(F, dev, x, (OH, OW), lab, w32, eps, False, fused=fused)
            check("edge empty sample fused=%d w=%s eps=%g" % (fused, wk, eps), loss, valid, dx, reference(x, lab, w32, eps, resize=(OH, OW)), w32)
            assert torch.count_nonzero(dx[1]) == 0
    # every counted pixel in the weight-0 class: D == 0.  eps = 0: NaN loss, all-zero gradient.  eps = 0.1: the sum of the smoothing
    # parts is positive and D is still 0 - torch's loss is NaN (its weighted-mean part is 0 / 0); the rule of D == 0 holds: NaN, zeros.
    lab0 = torch.full((N, OH, OW), 1, dtype=torch.int64)
    lab0[0, :2] = 255
    lab0[1, 5, :] = -100
    for fused in (True, False):
        for eps in (0.0, 0.1):
            y, loss, valid, dx = run_head(F, dev, x, (OH, OW), lab0, w, eps, True, fused=fused)
            ref = reference(x, lab0, w, eps, resize=(OH, OW))
            assert ref[2] == 0.0 and math.isnan(float(ref[0]))                 # torch: NaN as well
            assert math.isnan(float(loss)) and float(valid) == 0.0 and torch.count_nonzero(dx) == 0, (fused, eps)
            assert torch.isfinite(y).all()                                     # the softmax map is served all the same
        # no counted pixel at all
        _, loss, valid, dx = run_head(F, dev, x, (OH, OW), torch.full((N, OH, OW), 255, dtype=torch.int64), w, 0.1, False, fused=fused)
        assert math.isnan(float(loss)) and float(valid) == 0.0 and torch.count_nonzero(dx) == 0


# ------------------------------------------------------------------------------------------ 3. fused against separate
@pytest.mark.parametrize("C", [4, 21])
@pytest.mark.parametrize("geom", [GEOMS[0], GEOMS[2]])
def test_fused_equals_separate(geom, C, F, dev):
    N, H, W, OH, OW = geom
    g = torch.Generator().manual_seed(31 * C + H)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 2
    lab = make_labels(g, (N, OH, OW), C)
    w = make_weights(g, C)
    for wk, eps in SETTINGS:
        w32 = w if wk else None
        ref = reference(x, lab, w32, eps, resize=(OH, OW))
        yf, lf, vf, dxf = run_head(F, dev, x, (OH, OW), lab, w32, eps, True, fused=True)
        ys, ls, vs, dxs = run_head(F, dev, x, (OH, OW), lab, w32, eps, True, fused=False)
        check("separate C=%d %dx%d w=%s eps=%g" % (C, H, W, wk, eps), ls, vs, dxs, ref, w32)
        check("fused    C=%d %dx%d w=%s eps=%g" % (C, H, W, wk, eps), lf, vf, dxf, ref, w32)
        dl, dg = abs(float(lf) - float(ls)), float((dxf - dxs).abs().max())
        print("weighted_ce fused vs separate C=%d %dx%d w=%s eps=%g: loss rel %.2e, grad rel %.2e" % (
            C, H, W, wk, eps, dl / abs(float(ls)), dg / float(dxs.abs().max())))
        assert dl <= 1e-3 * abs(float(ls)) and dg <= 1e-3 * float(dxs.abs().max())
        assert float(vf) == float(vs)                              # D: the same fp32 weights summed in fp64


# ------------------------------------------------------------------------------------------ 4. no change when off
def raw_head(F, dev, entry_w, x_nhwc, lab, w, eps, OH, OW, want_soft):
    """the C entry itself on fresh, sentinel-filled outputs: (loss, valid, dlogits, y_soft)"""
    lib = F.lib
    N, H, W, C = x_nhwc.shape
    loss, valid = torch.full((1,), 7.0, device=dev), torch.full((1,), 7.0, device=dev)
    dl = torch.full((N, H, W, C), 7.0, device=dev)
    y = torch.full((N, OH, OW, C), 7.0, device=dev) if want_soft else None
    ws = torch.zeros(lib.sscg_upsample_head_workspace(N, H, W), dtype=torch.uint8, device=dev)
    yp = y.data_ptr() if want_soft else None
    if entry_w:
        rc = lib.sscg_upsample_head_fwd_w(x_nhwc.data_ptr(), lab.data_ptr(), None if w is None else w.data_ptr(), eps, yp, loss.data_ptr(),
                                          valid.data_ptr(), dl.data_ptr(), N, H, W, C, OH, OW, ws.data_ptr(), ws.numel(), F._stream())
    else:
        rc = lib.sscg_upsample_head_fwd(x_nhwc.data_ptr(), lab.data_ptr(), yp, loss.data_ptr(), valid.data_ptr(), dl.data_ptr(), N, H, W, C,
                                        OH, OW, ws.data_ptr(), ws.numel(), F._stream())
    assert rc == 0
    torch.cuda.synchronize()
    return loss, valid, dl, y


def raw_flat(F, dev, entry_w, x, lab, w, eps):
    """sscg_ce_fwd[_w] + sscg_ce_bwd[_w] on [rows][C] logits: (loss, valid, dx)"""
    lib = F.lib
    rows, C = x.shape
    loss, valid, dx = torch.full((1,), 7.0, device=dev), torch.full((1,), 7.0, device=dev), torch.full((rows, C), 7.0, device=dev)
    ws = torch.zeros(lib.sscg_loss_workspace(rows), dtype=torch.uint8, device=dev)
    wp = None if w is None else w.data_ptr()
    if entry_w:
        rc = lib.sscg_ce_fwd_w(x.data_ptr(), lab.data_ptr(), rows, C, wp, eps, loss.data_ptr(), valid.data_ptr(), ws.data_ptr(), ws.numel(), F._stream())
        rc |= lib.sscg_ce_bwd_w(x.data_ptr(), lab.data_ptr(), rows, C, wp, eps, None, 0.37, valid.data_ptr(), dx.data_ptr(), F._stream())
    else:
        rc = lib.sscg_ce_fwd(x.data_ptr(), lab.data_ptr(), rows, C, loss.data_ptr(), valid.data_ptr(), ws.data_ptr(), ws.numel(), F._stream())
        rc |= lib.sscg_ce_bwd(x.data_ptr(), lab.data_ptr(), rows, C, None, 0.37, valid.data_ptr(), dx.data_ptr(), F._stream())
    assert rc == 0
    torch.cuda.synchronize()
    return loss, valid, dx


@pytest.mark.parametrize("C", HEAD_CLASSES)
@pytest.mark.parametrize("geom", GEOMS)
def test_no_change_when_off(geom, C, F, dev):
    N, H, W, OH, OW = geom
    g = torch.Generator().manual_seed(7 * C + OH)
    x = (torch.randn(N, H, W, C, generator=g) * 2).to(dev)
    lab = make_labels(g, (N, OH, OW), C).to(dev)
    count = int(((lab >= 0) & (lab < C)).sum())
    for want_soft in (True, False):
        plain = raw_head(F, dev, False, x, lab, None, 0.0, OH, OW, want_soft)
        off = raw_head(F, dev, True, x, lab, None, 0.0, OH, OW, want_soft)
        assert float(plain[0]) != 7.0 and float(plain[1]) == count
        for a, b in zip(plain, off):
            assert (a is None and b is None) or torch.equal(a, b)           # loss, valid, dlogits, y_soft: bit-identical
    # all-ones weights, eps = 0: the weighted instantiation computes the plain loss - D is the pixel count exactly
    ones = torch.ones(C, device=dev)
    lw, vw, dw, yw = raw_head(F, dev, True, x, lab, ones, 0.0, OH, OW, True)
    assert float(vw) == count and torch.equal(yw, plain_soft(F, dev, x, lab, OH, OW))
    lp, vp, dp, _ = raw_head(F, dev, False, x, lab, None, 0.0, OH, OW, False)
    dl, dg, gmax = abs(float(lw) - float(lp)), float((dw - dp).abs().max()), float(dp.abs().max())
    print("weighted_ce ones-vs-plain head %dx%dx%d->%dx%d C=%d: loss bit-equal %s (rel %.2e), dlogits bit-equal %s (rel %.2e)" % (
        N, H, W, OH, OW, C, torch.equal(lw, lp), dl / abs(float(lp)), torch.equal(dw, dp), dg / gmax))
    assert dl <= 1e-3 * abs(float(lp)) and dg <= 1e-3 * gmax
    # the flat entries, on as many rows as the head has output pixels
    xf = (torch.randn(N * OH * OW, C, generator=g) * 2).to(dev)
    labf = lab.reshape(-1)
    plain, off = raw_flat(F, dev, False, xf, labf, None, 0.0), raw_flat(F, dev, True, xf, labf, None, 0.0)
    assert float(plain[0]) != 7.0 and float(plain[1]) == count and all(torch.equal(a, b) for a, b in zip(plain, off))
    lw, vw, dw = raw_flat(F, dev, True, xf, labf, ones, 0.0)
    assert float(vw) == count
    dl, dg, gmax = abs(float(lw) - float(plain[0])), float((dw - plain[2]).abs().max()), float(plain[2].abs().max())
    print("weighted_ce ones-vs-plain flat rows=%d C=%d: loss bit-equal %s (rel %.2e), dx bit-equal %s (rel %.2e)" % (
        xf.shape[0], C, torch.equal(lw, plain[0]), dl / max(abs(float(plain[0])), 1e-30), torch.equal(dw, plain[2]), dg / max(gmax, 1e-30)))
    assert dl <= 1e-3 * abs(float(plain[0])) + 1e-7 and dg <= 1e-3 * gmax + 8 * EPS32 / count


def plain_soft(F, dev, x, lab, OH, OW):
    return raw_head(F, dev, False, x, lab, None, 0.0, OH, OW, True)[3]


# ------------------------------------------------------------------------------------------ 5. label_hist
@pytest.mark.parametrize("C", [1, 21, 64])
def test_label_hist_equals_bincount(C, F, dev):
    g = torch.Generator().manual_seed(C)
    lab = torch.randint(-3, C + 5, (1 << 20,), generator=g)
    lab[::13] = 255
    lab[5::17] = -100
    inside = lab[(lab >= 0) & (lab < C)].numpy()
    want = np.bincount(inside, minlength=C)
    assert 0 < inside.size < lab.numel()
    got = F.label_hist(lab.to(dev), C)
    assert got.dtype == torch.int64 and got.shape == (C,) and (got.cpu().numpy() == want).all()
    start = torch.arange(C, dtype=torch.int64) * 1000 + 5
    acc = F.label_hist(lab.view(4, 1, 512, 512).to(dev), C, start.to(dev))           # accumulates into non-zero counts; any shape
    assert (acc.cpu().numpy() == want + start.numpy()).all()
    assert (F.label_hist(lab.to(torch.int32).to(dev), C).cpu().numpy() == want).all()  # other integer dtypes are widened


# ------------------------------------------------------------------------------------------ 6. through the model
def _args(dev, tmp_path, **kw):
    FX = __import__("oracle.fixtures", fromlist=["x"])
    return FX.make_args(dataset="acdc", crop_height=64, crop_width=64, batch_size=2, gpu_ids=[dev.index or 0], ngf=8, ndf=8,
                        checkpoint_dir=str(tmp_path / "ckpt"), as_written=True, **kw)


def test_supervised_step_returns_torchs_weighted_loss(F, dev, tmp_path, monkeypatch):
    md, U, data = load_sub("model"), load_sub("utils"), load_sub("data")
    args = _args(dev, tmp_path, model="supervised_model", ce_weights="median", label_smoothing=0.1)
    torch.manual_seed(21)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        m = md.supervised_model(args)
        loader = data.synthetic_loaders(args, 4, steps=2)[0]
        with pytest.raises(RuntimeError):                       # a rule is not trained on before it is resolved
            m.step(*[t.to(dev) for t in next(iter(loader))[:2]])
        w = m.resolve_ce_weights(loader)
        assert m.resolve_ce_weights(None) is w                  # resolved once
    counts = np.bincount(np.concatenate([gt.numpy().ravel() for _, gt, _ in loader]), minlength=4)
    want_w = U.ce_weights_from_counts(("median",), counts.tolist())
    assert w.dtype == torch.float32 and w.device == dev and w.cpu().tolist() == torch.tensor(want_w).float().tolist()
    assert out.getvalue().count("cross-entropy class weights") == 1
    l_img, l_gt, _ = next(iter(loader))
    l_img, l_gt = l_img.to(dev), l_gt.to(dev)
    with torch.no_grad():
        logits = m.Gsi(l_img).float().cpu()
    loss = float(m.step(l_img, l_gt))
    ref = float(reference(logits.double(), l_gt.cpu().squeeze(1), w.cpu(), 0.1, resize=(64, 64))[0])
    plain = float(reference(logits.double(), l_gt.cpu().squeeze(1), None, 0.0, resize=(64, 64))[0])
    print("weighted_ce supervised step: loss %.9g, torch fp64 on the same logits %.9g (rel %.2e); unweighted %.9g" % (
        loss, ref, abs(loss - ref) / abs(ref), plain))
    assert abs(loss - ref) <= 1e-3 * abs(ref)
    assert abs(plain - ref) > 2e-3 * abs(ref)                   # (the unweighted loss of these logits is out of the tolerance's reach)
    # the defaults never count labels, and take the plain entries
    def refuse(*a, **k):
        raise AssertionError("label_hist was called")
    monkeypatch.setattr(F, "label_hist", refuse)
    torch.manual_seed(21)
    with contextlib.redirect_stdout(io.StringIO()):
        m0 = md.supervised_model(_args(dev, tmp_path, model="supervised_model"))
        m0.resolve_ce_weights(loader)
        with torch.no_grad():
            logits0 = m0.Gsi(l_img).float().cpu()
        loss0 = float(m0.step(l_img, l_gt))
    assert m0.ce_weight is None and m0._ce_kwargs() == {}
    ref0 = float(reference(logits0.double(), l_gt.cpu().squeeze(1), None, 0.0, resize=(64, 64))[0])
    assert abs(loss0 - ref0) <= 1e-3 * abs(ref0)


def test_semisupervised_step_takes_the_flags(F, dev, tmp_path):
    md, data = load_sub("model"), load_sub("data")
    got = {}
    # (a list of clearly unequal weights: the synthetic label maps hold the four classes in nearly equal shares, for which a frequency
    # rule gives nearly equal weights - a weighted mean close to the plain one; the rules are resolved in the supervised test above)
    for tag, kw in (("default", {}), ("weighted", dict(ce_weights="0,0.2,1,5", label_smoothing=0.1))):
        args = _args(dev, tmp_path, **kw)
        torch.manual_seed(22)
        with contextlib.redirect_stdout(io.StringIO()):
            m = md.semisuper_cycleGAN(args)
            labeled, unlabeled, _ = data.synthetic_loaders(args, 4, steps=1)
            m.resolve_ce_weights(labeled)
        (l_img, l_gt, _), (unl_img, _, _) = next(iter(labeled)), next(iter(unlabeled))
        torch.manual_seed(23)
        losses = m.step(l_img.to(dev), l_gt.to(dev), unl_img.to(dev))
        m.sync_losses()
        got[tag] = {k: float(v) for k, v in losses.items()}
        assert all(math.isfinite(v) for v in got[tag].values()), got[tag]
        assert (m.ce_weight is None) == (tag == "default")
        F.flush_side_work()
        torch.cuda.synchronize()
    print("weighted_ce semisupervised lab_loss_CE: default %.6g, weights 0,0.2,1,5 + smoothing 0.1 %.6g; gt_cycle_loss %.6g / %.6g" % (
        got["default"]["lab_loss_CE"], got["weighted"]["lab_loss_CE"], got["default"]["gt_cycle_loss"], got["weighted"]["gt_cycle_loss"]))
    assert abs(got["weighted"]["lab_loss_CE"] - got["default"]["lab_loss_CE"]) > 1e-3 * abs(got["default"]["lab_loss_CE"])
    assert got["weighted"]["gt_cycle_loss"] != got["default"]["gt_cycle_loss"]
    # the networks' first forward does not depend on the loss flags: the terms that do not use them agree
    assert got["weighted"]["lab_loss_MSE"] == pytest.approx(got["default"]["lab_loss_MSE"], rel=1e-3)
