"""Contour counts on the MI355X: sscg_boundary_counts (csrc/boundary.hip) against the numpy restatement of its definition
(tests/boundary_reference.py, checked on its own in tests/test_boundary_host.py), then the score keeper and the drivers.

Every comparison is exact (integers), inside an output buffer with guard elements on both sides that must stay intact.  The inputs are
region maps, not noise: each case asserts - on the restatement alone - that between 10 % and 90 % of its valid pixels lie in E_t, so
that both the edge and the non-edge path of the kernel decide counts.  Exempt, each with its reason in EXEMPT: the 5x9 case with
d = 8 and the one-pixel-high / one-pixel-wide maps - there every window leaves the image (H or W is below d), so the share is 100 %
by the definition itself, which is what those cases are for; they assert exactly that."""
import contextlib
import functools
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import boundary_reference as R
from conftest import ROOT, load_sub

pytestmark = pytest.mark.gpu
GUARD = 64
SENT = -7777

# name: (N, H, W, C, d, blob seeds per sample, seed): sizes that are no multiple of the 32 x 32 tile, one-pixel-wide maps, a window
# larger than the map, the maximal halo (larger than a tile: a window crosses several neighbours), N = 1..3, C = 1 / 4 / 20 / 21 / 64
CASES = {
    "37x53_d1_c4": (2, 37, 53, 4, 1, 6, 0),
    "37x53_d3_c21": (3, 37, 53, 21, 3, 6, 1),
    "37x53_d7_c64": (1, 37, 53, 64, 7, 3, 2),
    "70x45_d1_c20": (1, 70, 45, 20, 1, 6, 3),
    "70x45_d3_c1": (2, 70, 45, 1, 3, 4, 4),
    "70x45_d7_c4": (3, 70, 45, 4, 7, 3, 5),
    "5x9_d8_c4": (2, 5, 9, 4, 8, 3, 6),
    "1x40_d3_c4": (2, 1, 40, 4, 3, 3, 7),
    "40x1_d3_c21": (2, 40, 1, 21, 3, 3, 8),
    "97x131_d32_c21": (2, 97, 131, 21, 32, 0, 9),          # 0 seeds: make_case's layout for widths near the map's size
    "97x131_d32_c64": (1, 97, 131, 64, 32, 0, 10),
}
EXEMPT = {"5x9_d8_c4": "every window leaves the 5 x 9 map at d = 8: all valid pixels are in E_t by construction",
          "1x40_d3_c4": "a map one pixel high: every window leaves it",
          "40x1_d3_c21": "a map one pixel wide: every window leaves it"}


@functools.lru_cache(maxsize=None)
def reference(case, pred_over=False):
    """Inputs and the restated counts of one case, computed once and shared (read-only) by the tests that need them."""
    N, H, W, Cn, d, seeds, seed = CASES[case]
    gt, pred = R.make_case(seed, N, H, W, Cn, seeds=seeds, void=True, pred_over=pred_over)
    want = R.counts(gt, pred, Cn, d)
    for a in (gt, pred, want):
        a.setflags(write=False)
    return gt, pred, want, R.edge_share(gt, Cn, d)


def raw(L, lt, lp, Cn, d, dev, init=None):
    """sscg_boundary_counts itself on device tensors: counts is a view into a sentinel-filled buffer whose guard bands must survive."""
    nb = 3 * Cn + Cn * Cn
    buf = torch.full((nb + 2 * GUARD,), SENT, dtype=torch.int64, device=dev)
    counts = buf[GUARD:GUARD + nb]
    counts[:] = 0 if init is None else init
    N, H, W = lt.shape
    rc = L.lib.sscg_boundary_counts(lt.data_ptr(), lp.data_ptr(), N, H, W, Cn, d, counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((torch.cat([buf[:GUARD], buf[-GUARD:]]) == SENT).all()), "a store outside the counts"
    return counts.cpu().numpy()


def to_dev(gt, pred, dev):
    return torch.tensor(gt, device=dev), torch.tensor(pred, device=dev)          # (copies: the shared arrays are read-only)


# ------------------------------------------------------------------------------------------ 1. the kernel against the restatement
@pytest.mark.parametrize("case", list(CASES))
def test_counts_equal_the_restatement(dev, case):
    L = load_sub("_lib")
    gt, pred, want, share = reference(case)
    N, H, W, Cn, d = CASES[case][:5]
    print("[boundary] %-16s %.1f %% of the valid pixels in E_t" % (case, 100 * share))
    if case in EXEMPT:
        assert share == 1.0, EXEMPT[case]
    else:
        assert 0.10 <= share <= 0.90, "%s: %.1f %% of the valid pixels are in E_t" % (case, 100 * share)
    bt, bp, bi, tri = R.split(want, Cn)
    assert bt.sum() > 0 and bp.sum() > 0 and 0 < bi.sum() < bt.sum() and tri.sum() > 0
    assert ((gt < 0) | (gt >= Cn)).any()                                     # void is in the map
    got = raw(L, *to_dev(gt, pred, dev), Cn, d, dev)
    assert np.array_equal(got, want), case
    # a second run gives the same bits
    assert np.array_equal(raw(L, *to_dev(gt, pred, dev), Cn, d, dev), got)
    # a sample's counts do not depend on the batch around it: the batch is the sum of its samples
    if N > 1:
        parts = sum(raw(L, *to_dev(gt[n:n + 1], pred[n:n + 1], dev), Cn, d, dev) for n in range(N))
        assert np.array_equal(parts, want)


@pytest.mark.parametrize("case", ["37x53_d3_c21", "70x45_d7_c4", "97x131_d32_c21"])
def test_predicted_values_at_or_above_the_class_count(dev, case):
    L = load_sub("_lib")
    gt, pred, want, _ = reference(case, pred_over=True)
    Cn, d = CASES[case][3:5]
    assert (pred == 200).any() and (pred == Cn).any() and not np.array_equal(want, reference(case)[2])
    assert np.array_equal(raw(L, *to_dev(gt, pred, dev), Cn, d, dev), want)


def test_calls_accumulate(dev):
    L = load_sub("_lib")
    (gt1, pred1, want1, _), (gt2, pred2, want2, _) = reference("37x53_d3_c21"), reference("97x131_d32_c21")
    init = np.arange(3 * 21 + 21 * 21, dtype=np.int64) * 3 + 1
    got = raw(L, *to_dev(gt1, pred1, dev), 21, 3, dev, init=torch.tensor(init, device=dev))
    assert np.array_equal(got, init + want1)
    both = raw(L, *to_dev(gt2, pred2, dev), 21, 32, dev, init=torch.tensor(got, device=dev))
    assert np.array_equal(both, init + want1 + want2)


def test_wrapper_contiguity_fresh_and_given_buffers_and_refusals(F, dev):
    L = load_sub("_lib")
    gt, pred, want, _ = reference("70x45_d7_c4")
    lt, lp = to_dev(gt, pred, dev)
    got = F.boundary_counts(lt, lp, 4, 7)
    assert got.dtype == torch.int64 and tuple(got.shape) == (3 * 4 + 16,) and np.array_equal(got.cpu().numpy(), want)
    again = F.boundary_counts(lt, lp, 4, 7, got)
    assert again is got and np.array_equal(got.cpu().numpy(), 2 * want)
    # non-contiguous inputs: transposed storage, and a strided slice of a wider map
    lt_t = lt.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    wide = torch.zeros(3, 70, 90, dtype=torch.uint8, device=dev)
    wide[:, :, ::2] = lp
    assert not lt_t.is_contiguous() and not wide[:, :, ::2].is_contiguous()
    assert np.array_equal(F.boundary_counts(lt_t, wide[:, :, ::2], 4, 7).cpu().numpy(), want)
    assert np.array_equal(F.boundary_counts(lt.to(torch.int32), lp, 4, 7).cpu().numpy(), want)          # any integer type of labels
    with pytest.raises(L.SscgError):
        F.boundary_counts(lt, lp[:, :, :44], 4, 7)                                  # a shape mismatch
    with pytest.raises(L.SscgError):
        F.boundary_counts(lt, lp, 4, 7, torch.zeros(27, dtype=torch.int64, device=dev))
    for bad in (0, 33, -1, 2.0):
        with pytest.raises(ValueError):
            F.boundary_counts(lt, lp, 4, bad)
    with pytest.raises(L.SscgError):
        F.boundary_counts(lt, lp, 65, 7)                                            # the entry's own refusal surfaces


# ------------------------------------------------------------------------------------------ 2. the score keeper
def _head_inputs(dev, seed=21, N=2, Cn=4, size=(33, 41)):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(N, Cn, 9, 9, generator=g).to(dev)
    image = torch.randn(N, 3, size[0], size[1], generator=g).to(dev)
    gt, _ = R.make_case(seed, N, size[0], size[1], Cn, seeds=5, void=True)
    return logits, image, torch.tensor(gt, device=dev)


@pytest.mark.parametrize("head", ["logits", "ms", "crf", "crf_probs", "device"])
def test_running_score_counts_the_map_its_head_returns(F, dev, head):
    U = load_sub("utils")
    Cn, size, d = 4, (33, 41), 2
    logits, image, gt = _head_inputs(dev)
    crf = F.CrfOptions(iterations=2, radius=2, dilation=1)
    half = F.resize_flip(logits, (5, 6), True)            # a second "view": any logits of another size, flagged as mirrored
    if head == "logits":
        update = lambda rs: rs.update_logits(gt, logits, size)
        u8 = F.predict_labels(logits, size)[0]
    elif head == "ms":
        update = lambda rs: rs.update_logits_ms(gt, [logits, half], [False, True], size)
        u8 = F.predict_labels_ms([logits, half], [False, True], size)[0]
    elif head == "crf":
        update = lambda rs: rs.update_logits_crf(gt, logits, image, size, crf)
        u8 = F.crf_labels(logits, image, size, crf)[0]
    elif head == "crf_probs":
        prob = F.predict_labels_ms([logits, half], [False, True], size, want_prob=True, want_u8=False)[3]
        update = lambda rs: rs.update_logits_crf(gt, prob, image, size, crf, probs=True)
        u8 = F.crf_labels(prob, image, size, crf, probs=True)[0]
    else:
        idx = F.predict_labels(logits, size, want_u8=False, want_index=True)[1]
        update = lambda rs: rs.update_device(gt, idx)
        u8 = idx.to(torch.uint8)
    off, on = U.runningScore(Cn, "acdc"), U.runningScore(Cn, "acdc")
    on.set_boundary(F.BoundaryOptions(d=d))
    for rs in (off, on):
        update(rs)
        update(rs)
    want = 2 * R.counts(gt.cpu().numpy(), u8.cpu().numpy(), Cn, d)
    assert off._boundary_counts is None and off.get_boundary_scores() is None
    assert np.array_equal(on._boundary_counts.cpu().numpy(), want) and want[:Cn].sum() > 0
    assert torch.equal(on._device_hist, off._device_hist)                          # the confusion matrix: bitwise the one without
    got, ref = on.get_boundary_scores(), U.boundary_scores(want, Cn, "acdc")
    assert got["boundary_iou"] == ref["boundary_iou"] and got["trimap_iou"] == ref["trimap_iou"] and 0 < got["boundary_iou"] < 1
    s_on, s_off = on.get_scores(), off.get_scores()
    assert s_on[0]["Mean IoU : \t"] == s_off[0]["Mean IoU : \t"] and (on.confusion_matrix == off.confusion_matrix).all()
    on.reset()
    assert on._boundary_counts is None and on.get_boundary() == F.BoundaryOptions(d=d)
    # a ratio resolves against the map the head returns: 0.02 of the 33 x 41 diagonal is 1
    on.set_boundary(F.BoundaryOptions())
    update(on)
    assert np.array_equal(on._boundary_counts.cpu().numpy(), R.counts(gt.cpu().numpy(), u8.cpu().numpy(), Cn, 1))


# ------------------------------------------------------------------------------------------ 3. the drivers
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
    for k in range(2):
        gt, _ = R.make_case(30 + k, 2, 65, 65, 4, seeds=6, void=True)
        batches.append((torch.randn(2, 3, 65, 65, generator=g), torch.tensor(gt).unsqueeze(1), ["a", "b"]))
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


def test_evaluate_with_boundary_scores_the_maps_it_predicts(F, dev, tmp_path):
    U = load_sub("utils")
    m, batches = _model(dev, tmp_path)
    conf_off, miou_off = _evaluate(m, batches)
    assert not hasattr(m, "eval_boundary")
    conf_on, miou_on = _evaluate(m, batches, boundary=F.BoundaryOptions(d=3))
    assert miou_on == miou_off and (conf_on == conf_off).all() and m.Gsi.training
    want = np.zeros(3 * 4 + 16, dtype=np.int64)
    m.Gsi.eval()
    with torch.no_grad():
        for image, gt, _ in batches:
            u8 = F.predict_labels(m.Gsi(image.to(dev)), (65, 65))[0]
            want += R.counts(gt.squeeze(1).numpy(), u8.cpu().numpy(), 4, 3)
    m.Gsi.train()
    ref = U.boundary_scores(want, 4, "acdc")
    got = m.eval_boundary
    assert set(got) == {"boundary_iou", "class_boundary_iou", "trimap_iou", "class_trimap_iou"} and want[:4].sum() > 0
    for key in ("boundary_iou", "trimap_iou"):
        assert got[key] == ref[key] or (np.isnan(got[key]) and np.isnan(ref[key])), key
    for key in ("class_boundary_iou", "class_trimap_iou"):
        assert all(got[key][c] == ref[key][c] or (np.isnan(got[key][c]) and np.isnan(ref[key][c])) for c in range(4)), key
    # with the CRF and several views the option rides on their heads; the region scores stay theirs
    crf, views = U.parse_crf("iters=2,radius=2,dilation=1"), U.parse_tta("0.5,1.0:flip")
    conf_c, miou_c = _evaluate(m, batches, crf=crf, tta=views)
    conf_cb, miou_cb = _evaluate(m, batches, crf=crf, tta=views, boundary=U.parse_boundary("on"))
    assert miou_cb == miou_c and (conf_cb == conf_c).all() and np.isfinite(m.eval_boundary["trimap_iou"])
    # switched off again, the attribute goes
    _evaluate(m, batches)
    assert not hasattr(m, "eval_boundary")


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
m.evaluate(batches[:1])          # operand copies are made here
torch.cuda.synchronize()
for tag, kw in (("plain", {}), ("boundary", {"boundary": U.parse_boundary("d=3")}), ("plain again", {}),
                ("crf+boundary", {"crf": U.parse_crf("iters=2"), "boundary": U.parse_boundary("on")})):
    sys.stderr.write("[census] begin %%s\n" %% tag)
    m.evaluate(batches, **kw)
    torch.cuda.synchronize()
    sys.stderr.write("[census] end %%s\n" %% tag)
"""


def test_launch_census_of_an_evaluation_with_and_without_the_option(dev, tmp_path):
    env = dict(os.environ, SSCG_TRACE="1")
    r = subprocess.run([sys.executable, "-c", CENSUS % (ROOT, os.path.join(ROOT, "tests"), str(tmp_path / "ckpt"))], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    counts = {}
    for tag in ("plain", "boundary", "plain again", "crf+boundary"):
        body = r.stderr[r.stderr.index("[census] begin " + tag + "\n"):r.stderr.index("[census] end " + tag + "\n")]
        calls = {}
        for line in body.splitlines():
            if line.startswith("[sscg] "):
                name = line[7:].split("(")[0]
                calls[name] = calls.get(name, 0) + 1
        counts[tag] = calls
    plain, on, again, both = counts["plain"], counts["boundary"], counts["plain again"], counts["crf+boundary"]
    # without the option: the launches of before - one fused head per batch, nothing of the contour scores - also after a run with it
    assert plain.get("sscg_boundary_counts", 0) == 0 and plain.get("sscg_predict_head", 0) == 2, plain
    assert again == plain, (plain, again)
    # with it: one sscg_boundary_counts per batch and one fill for the fresh counts; every other launch as without
    extra = {k: v - plain.get(k, 0) for k, v in on.items() if v != plain.get(k, 0)}
    assert extra == {"sscg_boundary_counts": 2, "sscg_fill": 1} and set(plain) <= set(on), (plain, on)
    assert both.get("sscg_crf_head", 0) == 2 and both.get("sscg_boundary_counts", 0) == 2 and both.get("sscg_predict_head", 0) == 0, both
