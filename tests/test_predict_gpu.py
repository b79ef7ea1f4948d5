"""The inference heads (sscg_predict_head / sscg_image_head, ABI v18) on the MI355X.  The contract is BIT IDENTITY with the chain of
separate passes they replace (upsample_bilinear -> softmax2d -> argmax_index -> confusion_hist; upsample_bilinear -> to_nhwc ->
act_fwd(TANH) -> host un-normalise + save_image), so every comparison is torch.equal."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_sub

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CL = torch.channels_last

# (H, W, OH, OW): DeepLab's 33x33 -> the VOC crop, 33x65 -> the Cityscapes crop, a smaller square, a non-square odd target, identity
GEOMS = [(33, 33, 256, 256), (33, 65, 256, 512), (17, 17, 128, 128), (9, 13, 50, 71), (24, 40, 24, 40)]
GEOM_IDS = ["33x33-256x256", "33x65-256x512", "17x17-128x128", "9x13-50x71", "identity"]


def gpu(x, dev):
    x = x.to(dev)
    return x.contiguous(memory_format=CL) if x.dim() == 4 else x


def unfused_index(F, xg, size):
    return F.argmax_index(F.softmax2d(F.upsample_bilinear(xg, size)))


# ------------------------------------------------------------------------------------------ 1. labels vs the unfused chain
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
@pytest.mark.parametrize("C", [4, 20, 21, 7])
def test_labels_equal_the_unfused_chain(F, dev, C, geom, N):
    H, W, OH, OW = geom
    g = torch.Generator().manual_seed(1000 * C + 10 * H + N)
    # seeded normal logits
    x = torch.randn(N, C, H, W, generator=g) * 3.0
    # forced ties (a): one class's low-resolution plane copied onto another - interpolation of equal planes is equal, the softmax ties
    lo, hi = 1, C - 1
    xa = torch.randn(N, C, H, W, generator=g)
    xa[:, lo] += 2.5
    xa[:, hi] = xa[:, lo]
    # forced ties (b): two planes ONE ULP apart that tower over the rest; the higher class holds the greater logit.  The values lie
    # in [1/16, 1/8), where one ulp is 2^-27: exp(-2^-27) = 1 - 2^-27 + ... rounds to 1.0f, so both probabilities are equal and the
    # LOWER index wins although argmax of the logits would name the higher one
    xb = torch.randn(N, C, H, W, generator=g) - 12.0
    base = torch.rand(N, H, W, generator=g) * 0.0624 + 0.0625
    xb[:, lo] = base
    xb[:, hi] = torch.nextafter(base, torch.full_like(base, 1.0))
    assert bool((xb[:, hi] > xb[:, lo]).all()) and float((xb[:, hi] - xb[:, lo]).max()) <= 2.0 ** -27
    with torch.no_grad():
        for name, t in (("normal", x), ("copied plane", xa), ("one ulp apart", xb)):
            xg = gpu(t, dev)
            want = unfused_index(F, xg, (OH, OW))
            u8, idx, hist = F.predict_labels(xg, (OH, OW), want_index=True)
            assert hist is None and u8.dtype == torch.uint8 and idx.dtype == torch.int64
            assert tuple(u8.shape) == tuple(idx.shape) == (N, OH, OW)
            assert torch.equal(idx, want), name
            assert torch.equal(u8, want.to(torch.uint8)), name
            only_u8 = F.predict_labels(xg, (OH, OW))
            assert only_u8[1] is None and torch.equal(only_u8[0], u8)
            if name == "copied plane":
                assert not bool((idx == hi).any()) and bool((idx == lo).any())          # as test_argmax_onehot_bit_exact: lower index wins
            if name == "one ulp apart":
                # output pixel (0, 0) is source pixel (0, 0) exactly (weights 1 and 0): the probabilities tie there
                assert bool((idx[:, 0, 0] == lo).all())


def test_predict_labels_is_not_an_autograd_node(F, dev):
    L = load_sub("_lib")
    x = torch.randn(1, 21, 9, 9).to(dev).requires_grad_(True)
    with pytest.raises(L.SscgError):
        F.predict_labels(x, (32, 32))
    with pytest.raises(L.SscgError):
        F.predict_image(torch.randn(1, 3, 9, 9).to(dev).requires_grad_(True), (32, 32))
    with torch.no_grad():
        assert F.predict_labels(x, (32, 32))[0].shape == (1, 32, 32)
    with pytest.raises(L.SscgError):
        F.predict_labels(x.detach(), (32, 32), num_classes=20)


# ------------------------------------------------------------------------------------------ 2. histogram
@pytest.mark.parametrize("C,geom", [(21, GEOMS[0]), (20, GEOMS[1]), (7, GEOMS[3]), (4, GEOMS[4]), (64, GEOMS[3])],
                         ids=["voc", "cityscapes", "generic", "identity", "C64"])
def test_histogram_equals_confusion_hist_and_bincount(F, dev, C, geom):
    H, W, OH, OW = geom
    N = 3
    g = torch.Generator().manual_seed(77 + C)
    x1, x2 = (gpu(torch.randn(N, C, H, W, generator=g) * 2.0, dev) for _ in range(2))
    labs = []
    for _ in range(2):
        lab = torch.randint(0, C, (N, OH, OW), generator=g)
        lab[0, :3] = 255                     # the "void" label of VOC
        lab[-1, OH // 2, :] = -1
        lab[1, 5, 7] = C                     # first id outside the range
        labs.append(lab)

    def host(lab, idx):
        lt, lp = lab.numpy().ravel(), idx.cpu().numpy().ravel()
        keep = (lt >= 0) & (lt < C)
        return np.bincount(C * lt[keep].astype(int) + lp[keep], minlength=C * C).reshape(C, C)

    with torch.no_grad():
        u8, idx, hist = F.predict_labels(x1, (OH, OW), want_index=True, label_true=labs[0].to(dev), num_classes=C)
        assert hist.dtype == torch.int64 and tuple(hist.shape) == (C, C)
        assert torch.equal(hist, F.confusion_hist(labs[0].to(dev), idx, C))
        h1 = host(labs[0], idx)
        assert np.array_equal(hist.cpu().numpy(), h1)
        assert int(h1.sum()) == int(((labs[0] >= 0) & (labs[0] < C)).sum())
        # accumulation over two calls into one matrix; histogram alone (no label map asked for)
        first = hist.clone()
        none_u8, none_idx, hist2 = F.predict_labels(x2, (OH, OW), want_u8=False, label_true=labs[1].to(dev), hist=hist)
        assert none_u8 is None and none_idx is None and hist2 is hist
        idx2 = unfused_index(F, x2, (OH, OW))
        assert np.array_equal(hist.cpu().numpy(), first.cpu().numpy() + host(labs[1], idx2))
    # runningScore.update_logits == update_device on the unfused predictions
    utils = load_sub("utils")
    a, b = utils.runningScore(C, "acdc"), utils.runningScore(C, "acdc")
    with torch.no_grad():
        for xg, lab in ((x1, labs[0]), (x2, labs[1])):
            a.update_logits(lab.to(dev), xg, (OH, OW))
            b.update_device(lab.to(dev), unfused_index(F, xg, (OH, OW)))
    sa, sb = a.get_scores(), b.get_scores()
    assert np.array_equal(a.confusion_matrix, b.confusion_matrix) and a.confusion_matrix.sum() > 0
    assert np.array_equal(np.float64(sa[0]["Mean IoU : \t"]), np.float64(sb[0]["Mean IoU : \t"]), equal_nan=True)


# ------------------------------------------------------------------------------------------ 3 / 5. evaluate() in processes of its own
def _evaluate_child(env, kind="semi"):
    e = dict(os.environ)
    for k in ("SSCG_FUSE_PREDICT", "SSCG_TRACE", "SSCG_RACECHECK", "SSCG_FUZZ", "SSCG_FORCE_DP"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(HERE, "aids", "predict_eval.py"), kind], env=e, capture_output=True, text=True,
                       timeout=1100)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line), r


@pytest.mark.parametrize("kind", ["semi", "sup"])
def test_evaluate_fused_equals_unfused_on_the_reference_configuration(kind):
    """The g5_eval configuration (the one test_evaluation_matches_the_references_label_maps holds against the reference's label
    maps): evaluate() with SSCG_FUSE_PREDICT unset and = 0, a fresh process each, gives the same confusion matrix and mIoU - and the
    default really runs the fused entry, the switch really the separate passes (SSCG_TRACE lists every C-ABI call)."""
    meta = json.load(open(os.path.join(HERE, "golden", "meta.json")))["g5_eval"]
    fused, rf = _evaluate_child({"SSCG_TRACE": "1"}, kind)
    plain, rp = _evaluate_child({"SSCG_TRACE": "1", "SSCG_FUSE_PREDICT": "0"}, kind)
    assert fused["fused"] is True and plain["fused"] is False
    assert "sscg_predict_head" in rf.stderr and "sscg_confusion_hist" not in rf.stderr and "sscg_softmax_fwd" not in rf.stderr
    assert "sscg_predict_head" not in rp.stderr and "sscg_confusion_hist" in rp.stderr and "sscg_softmax_fwd" in rp.stderr
    assert fused["confusion"] == plain["confusion"]
    assert fused["miou"] == plain["miou"] and fused["class_iou"] == plain["class_iou"]
    cfg = meta["config"]
    assert int(np.sum(fused["confusion"])) > 0 and int(np.sum(fused["confusion"])) <= cfg["batches"] * cfg["B"] * cfg["H"] * cfg["W"]
    assert abs(fused["miou"] - meta["miou"]) < 1e-3          # and both are the reference's figure (tests/test_parity_gpu.py's bound)


def test_evaluate_under_the_ordering_checker_reports_no_race():
    out, r = _evaluate_child({"SSCG_RACECHECK": "1"})
    assert out["fused"] is True
    assert "0 distinct reports" in r.stdout, (r.stdout[-3000:], r.stderr[-2000:])


# ------------------------------------------------------------------------------------------ 4. images
def _special_image_values():
    """fp32 inputs whose tanh is exactly +-1, and inputs whose byte arithmetic lands next to an integer: px = (t * 0.5 + 0.5) * 255 + 0.5
    close to m  <=>  t close to (2 * m - 1) / 255 - 1.  Checked here, on the CPU, that the set holds such values."""
    m = np.arange(1, 256, dtype=np.float64)
    t = (2.0 * m - 1.0) / 255.0 - 1.0
    x = np.arctanh(np.clip(t, -1 + 1e-12, 1 - 1e-12)).astype(np.float32)
    x = np.concatenate([x, np.nextafter(x, np.float32(10)), np.nextafter(x, np.float32(-10)),
                        np.array([20.0, -20.0, 10.0, -10.0, 0.0, 9.2, -9.2], dtype=np.float32)])
    xt = torch.from_numpy(x)
    th = torch.tanh(xt)
    assert bool((th == 1.0).any()) and bool((th == -1.0).any())
    px = (th * 0.5 + 0.5) * 255 + 0.5
    ulp = torch.nextafter(px, torch.full_like(px, 1e9)) - px
    near = (px - px.round()).abs() <= ulp
    assert int(near.sum()) > 0, "no value next to an integer in the constructed set"
    assert float(th.min()) == -1.0 and float(th.max()) == 1.0 and int((th.abs() < 0.5).sum()) > 50       # tanh covers (-1, 1)
    return xt


def _host_bytes(y):
    """validation.py + utils.save_image on the host: `y.cpu() * 0.5 + 0.5`, then `.mul(255).add_(0.5).clamp_(0, 255)` -> uint8, HWC"""
    t = y.detach().float().cpu().contiguous() * 0.5 + 0.5
    return t.mul(255).add_(0.5).clamp_(0, 255).permute(0, 2, 3, 1).to(torch.uint8).contiguous()


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("C", [3, 1, 4])
@pytest.mark.parametrize("geom", [GEOMS[0], GEOMS[3], (64, 48, 64, 48), (9, 9, 17, 17)], ids=["33x33-256x256", "9x13-50x71", "identity", "9x9-17x17"])
def test_images_equal_the_unfused_chain_and_the_host_bytes(F, dev, geom, C, N):
    H, W, OH, OW = geom
    g = torch.Generator().manual_seed(31 * H + 7 * C + N)
    x = torch.randn(N, C, H, W, generator=g) * 2.0
    sp = _special_image_values()
    flat = x.view(-1)
    pos = torch.randperm(flat.numel(), generator=g)[:min(sp.numel(), flat.numel() // 2)]
    flat[pos] = sp[:pos.numel()]            # identity and the 9x9 -> 17x17 grid (scale exactly 1/2) hand many of them through unchanged
    with torch.no_grad():
        xg = gpu(x, dev)
        want = F.act_fwd(F.to_nhwc(F.upsample_bilinear(xg, (OH, OW))), F.ACT_TANH)
        y, u8 = F.predict_image(xg, (OH, OW))
        assert tuple(y.shape) == (N, C, OH, OW) and y.is_contiguous(memory_format=CL) and tuple(u8.shape) == (N, OH, OW, C)
        assert torch.equal(y, want)
        hb = _host_bytes(want)
        assert torch.equal(u8.cpu(), hb)
        if (H, W) == (OH, OW):
            assert int((hb == 0).sum()) > 0 and int((hb == 255).sum()) > 0              # the exact -1 / +1 came through
        y_only, none = F.predict_image(xg, (OH, OW), want_u8=False)
        none2, u8_only = F.predict_image(xg, (OH, OW), want_float=False)
        assert none is None and none2 is None and torch.equal(y_only, want) and torch.equal(u8_only, u8)


# ------------------------------------------------------------------------------------------ 5. plumbing
def test_dry_run_leaves_the_outputs_untouched(F, dev):
    lib = load_sub("_lib").lib
    N, C, H, W, OH, OW = 2, 21, 9, 9, 40, 40
    x = gpu(torch.randn(N, C, H, W), dev)
    idx = torch.full((N, OH, OW), -5, dtype=torch.int64, device=dev)
    u8 = torch.full((N, OH, OW), 7, dtype=torch.uint8, device=dev)
    lab = torch.zeros((N, OH, OW), dtype=torch.int64, device=dev)
    hist = torch.full((C, C), 3, dtype=torch.int64, device=dev)
    xi = gpu(torch.randn(N, 3, H, W), dev)
    y = torch.full((N, OH, OW, 3), 9.0, device=dev)
    rgb = torch.full((N, OH, OW, 3), 11, dtype=torch.uint8, device=dev)
    st = F._stream()
    was = lib.sscg_set_dry_run(1)
    try:
        assert lib.sscg_predict_head(x.data_ptr(), N, H, W, C, OH, OW, idx.data_ptr(), u8.data_ptr(), lab.data_ptr(), hist.data_ptr(), st) == 0
        assert lib.sscg_image_head(xi.data_ptr(), N, H, W, 3, OH, OW, y.data_ptr(), rgb.data_ptr(), st) == 0
    finally:
        lib.sscg_set_dry_run(was)
    torch.cuda.synchronize()
    assert bool((idx == -5).all()) and bool((u8 == 7).all()) and bool((hist == 3).all())
    assert bool((y == 9.0).all()) and bool((rgb == 11).all())
    # and with the launches back on, the same calls write every element
    assert lib.sscg_predict_head(x.data_ptr(), N, H, W, C, OH, OW, idx.data_ptr(), u8.data_ptr(), lab.data_ptr(), hist.data_ptr(), st) == 0
    assert lib.sscg_image_head(xi.data_ptr(), N, H, W, 3, OH, OW, y.data_ptr(), rgb.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert bool(((idx >= 0) & (idx < C)).all()) and torch.equal(u8, idx.to(torch.uint8))
    assert int(hist.sum()) == 3 * C * C + N * OH * OW and bool((y.abs() <= 1.0).all())
