"""Windowed dense-CRF refinement on the MI355X: sscg_crf_head (csrc/crf.hip) against the fp64 numpy restatement of its definition
(tests/crf_reference.py, checked on its own in tests/test_crf_host.py), the bit identities inside this build, and the drivers.

Accuracy.  The reference has no CRF, so Q is held to the fp64 restatement.  Per case the same restatement also runs in numpy fp32 and
e32 = max|Q_np32 - Q_fp64| scales the bound: max|Q_gpu - Q_fp64| <= 8 * e32 + 2e-6 (the device's expf and the FMAs the compiler forms
differ from numpy by a few ulp per operation; the amplification through the iterations is the same for both).  The test prints e32, the
GPU's distance and their ratio per case; profiles/crf.txt keeps the figures of the first MI355X run.
Labels equal the fp64 first maximum wherever the fp64 top-two margin is >= 1e-3; at most 1 % of a case's pixels may fall under that
margin (the seeds below were checked on the CPU: the restatement alone excludes at most 0.5 % on the logits cases and 0.8 % on the
two views' flatter summed probabilities), and in every strong case at least 10 % of the labels must differ from the first maximum
of Q0 - otherwise the message path is not being exercised."""
import contextlib
import ctypes as C
import functools
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import crf_reference as R
from conftest import ROOT, load_sub

pytestmark = pytest.mark.gpu
CL = torch.channels_last
GUARD = 64
SENT = {torch.float32: float("nan"), torch.int64: -7777, torch.uint8: 0xEE}

# (N, H, W, C, OH, OW, radius, dilation, iterations), seed, IC: ragged tiles, a window larger than the map, all four borders, every
# dispatch arm (21 / 20 / 4 / run-time C, radius <= 3 and beyond), the identity resize, a single iteration and many
CASES = {
    "voc21_r3": ((2, 9, 11, 21, 37, 45, 3, 1, 5), 0, 3),
    "acdc4_r3d2": ((1, 5, 7, 4, 19, 23, 3, 2, 5), 2, 3),
    "acdc4_r3d2_grey": ((1, 5, 7, 4, 19, 23, 3, 2, 5), 0, 1),
    "city20_r5": ((2, 9, 11, 20, 37, 45, 5, 1, 5), 1, 3),
    "tiny2_window_past_map": ((1, 3, 3, 2, 3, 5, 3, 2, 3), 2, 3),
    "c33_identity_one_step": ((2, 19, 23, 33, 19, 23, 2, 1, 1), 2, 3),
    "voc21_tall_d3": ((1, 2, 2, 21, 70, 18, 2, 3, 4), 0, 3),
}
SETS = {"strong": R.STRONG, "gentle": R.GENTLE}


@functools.lru_cache(maxsize=None)
def reference(case, pset):
    """Inputs and the fp64 / fp32 restatements of one case, computed once and shared (read-only) by the tests that need them."""
    (N, H, W, Cn, OH, OW, r, d, T), seed, IC = CASES[case]
    x, img = R.make_inputs(seed, N, H, W, Cn, OH, OW, IC)
    return _restate(x, R.LOGITS, img, (OH, OW), T, r, d, pset)


def _restate(x, kind, img, size, T, r, d, pset):
    u64, q64 = R.crf(x, kind, img, size, T, r, d, np.float64, **SETS[pset])
    _, q32 = R.crf(x, kind, img, size, T, r, d, np.float32, **SETS[pset])
    for a in (x, img, q64[0], q64[-1]):
        a.setflags(write=False)
    return dict(x=x, img=img, q0=q64[0], q=q64[-1], e32=float(np.abs(q32[-1].astype(np.float64) - q64[-1]).max()),
                size=size, T=T, r=r, d=d, kind=kind)


def options(F, ref, pset, **over):
    return F.CrfOptions(**dict(dict(iterations=ref["T"], radius=ref["r"], dilation=ref["d"], **SETS[pset]), **over))


def guarded(n, dtype, dev, fill=None):
    """(buffer, view of n elements GUARD elements into it): the guard bands hold the sentinel of the dtype, the view `fill` (or it too)."""
    buf = torch.full((n + 2 * GUARD,), SENT[dtype], dtype=dtype, device=dev)
    if fill is not None:
        buf[GUARD:GUARD + n] = fill
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf):
    g = torch.cat([buf[:GUARD], buf[-GUARD:]])
    return bool(torch.isnan(g).all()) if buf.is_floating_point() else bool((g == SENT[buf.dtype]).all())


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


def raw(L, x, kind, img, size, opts, dev, *, want_q=True, want_index=True, want_u8=True, lt=None, hist_init=None, ws_byte=0xFF):
    """sscg_crf_head itself on x [N,H,W,C] / img [N,OH,OW,IC] device tensors: every output and the workspace are views into sentinel-
    filled buffers whose guard bands must survive; the workspace's own bytes are pre-filled with `ws_byte`.
    Returns (q [N,OH,OW,C] | None, index | None, u8 | None, hist | None)."""
    N, H, W, Cn = x.shape
    oh, ow = size
    IC = img.shape[3]
    need = L.lib.sscg_crf_workspace(N, Cn, oh, ow, opts.iterations)
    assert need == (3 * N * Cn * oh * ow * 4 if opts.iterations else 0)
    wb, ws = guarded(max(need, 1), torch.uint8, dev, fill=ws_byte)
    bufs = [wb]
    q = index = u8 = hist = None
    if want_q:
        b, q = guarded(N * oh * ow * Cn, torch.float32, dev)
        bufs.append(b)
    if want_index:
        b, index = guarded(N * oh * ow, torch.int64, dev)
        bufs.append(b)
    if want_u8:
        b, u8 = guarded(N * oh * ow, torch.uint8, dev)
        bufs.append(b)
    if lt is not None:
        b, hist = guarded(Cn * Cn, torch.int64, dev, fill=hist_init.view(-1))
        bufs.append(b)
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = L.lib.sscg_crf_head(x.data_ptr(), kind, N, H, W, Cn, oh, ow, img.data_ptr(), IC, C.byref(opts.params()), ptr(q), ptr(index), ptr(u8),
                             ptr(lt), ptr(hist), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for b in bufs:
        assert guards_intact(b), "a store outside the %s buffer" % b.dtype
    v = lambda t, *s: None if t is None else t.view(*s)
    return v(q, N, oh, ow, Cn), v(index, N, oh, ow), v(u8, N, oh, ow), v(hist, Cn, Cn)


def to_dev(ref, dev):
    return torch.tensor(ref["x"], device=dev), torch.tensor(ref["img"], device=dev)          # (copies: the shared arrays are read-only)


def check_against_fp64(what, ref, q, index, strong):
    """The accuracy and label conditions of the module docstring for one case; prints the figures before it asserts."""
    q64, e32 = ref["q"], ref["e32"]
    got = q.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), what
    err = float(np.abs(got - q64).max())
    bound = 8.0 * e32 + 2e-6
    margin = R.top_two_margin(q64)
    sure = margin >= 1e-3
    excluded = 1.0 - float(sure.mean())
    labels = index.cpu().numpy()
    wrong = int(((labels != R.first_max(q64)) & sure).sum())
    moved = float((labels != R.first_max(ref["q0"])).mean())
    print("[crf] %-34s e32 %.3e  gpu %.3e  ratio %6.2f  bound %.3e | labels: %d wrong of %d sure, %.3f %% excluded, %.1f %% moved from Q0"
          % (what, e32, err, err / e32, bound, wrong, int(sure.sum()), 100 * excluded, 100 * moved))
    assert err <= bound, "%s: max|Q_gpu - Q_fp64| = %.3e > 8 * e32 + 2e-6 = %.3e (e32 %.3e)" % (what, err, bound, e32)
    assert excluded <= 0.01, "%s: %.2f %% of the pixels have an fp64 top-two margin under 1e-3" % (what, 100 * excluded)
    assert wrong == 0, "%s: %d labels differ from the fp64 first maximum at a margin >= 1e-3" % (what, wrong)
    if strong:
        assert moved >= 0.10, "%s: only %.1f %% of the labels differ from the first maximum of Q0" % (what, 100 * moved)


# ------------------------------------------------------------------------------------------ 1. Q and the labels against fp64
@pytest.mark.parametrize("pset", ["strong", "gentle"])
@pytest.mark.parametrize("case", list(CASES))
def test_q_and_labels_against_the_fp64_restatement(F, dev, case, pset):
    L = load_sub("_lib")
    ref = reference(case, pset)
    x, img = to_dev(ref, dev)
    q, index, u8, _ = raw(L, x, L.CRF_LOGITS, img, ref["size"], options(F, ref, pset), dev)
    assert torch.equal(u8.to(torch.int64), index)
    check_against_fp64("%s/%s" % (case, pset), ref, q, index, pset == "strong")


def _two_view_scores(F, dev, seed=12, N=2, Cn=21, size=(37, 45)):
    """prob_sum of a real predict_labels_ms call on two views (the second mirrored), [N,OH,OW,C] contiguous, and a guide image."""
    rs = np.random.RandomState(seed)
    views = [torch.from_numpy((rs.standard_normal((N, h, w, Cn)) * 2.0).astype(np.float32)).to(dev) for h, w in ((9, 11), (19, 23))]
    prob = F.predict_labels_ms([v.permute(0, 3, 1, 2) for v in views], [False, True], size, want_prob=True, want_u8=False)[3]
    _, img = R.make_inputs(seed, N, 2, 2, Cn, size[0], size[1], 3)
    return views, prob.permute(0, 2, 3, 1).contiguous(), torch.from_numpy(img).to(dev)


@pytest.mark.parametrize("pset", ["strong", "gentle"])
def test_scores_of_two_views_against_the_fp64_restatement(F, dev, pset):
    L = load_sub("_lib")
    _, prob, img = _two_view_scores(F, dev)
    assert float(prob.min()) >= 0.0 and abs(float(prob.sum(dim=3).mean()) - 2.0) < 1e-4
    ref = _restate(prob.cpu().numpy(), R.PROBS, img.cpu().numpy(), (37, 45), 5, 3, 2, pset)
    q, index, _, _ = raw(L, prob, L.CRF_PROBS, img, (37, 45), options(F, ref, pset), dev)
    check_against_fp64("two views, scores/%s" % pset, ref, q, index, pset == "strong")


# ------------------------------------------------------------------------------------------ 2. bit identities inside this build
@pytest.mark.parametrize("case", list(CASES))
def test_outputs_agree_with_each_other_bit_for_bit(F, dev, case):
    L = load_sub("_lib")
    ref = reference(case, "strong")
    opts = options(F, ref, "strong")
    x, img = to_dev(ref, dev)
    N, _, _, Cn = x.shape
    oh, ow = ref["size"]
    lt = make_labels(Cn, N, oh, ow, Cn, dev)
    q, index, u8, hist = raw(L, x, L.CRF_LOGITS, img, ref["size"], opts, dev, lt=lt, hist_init=hist_pattern(Cn, dev))
    # the label outputs of a call that writes no Q = the first maximum and the confusion counts of the Q of the call that does
    _, index2, u82, hist2 = raw(L, x, L.CRF_LOGITS, img, ref["size"], opts, dev, want_q=False, lt=lt, hist_init=hist_pattern(Cn, dev))
    first = F.argmax_index(q.permute(0, 3, 1, 2))
    assert torch.equal(index, first) and torch.equal(index2, first) and torch.equal(u8.to(torch.int64), first) and torch.equal(u82, u8)
    want_hist = F.confusion_hist(lt, first, Cn, hist_pattern(Cn, dev).clone())
    assert torch.equal(hist, want_hist) and torch.equal(hist2, want_hist)
    counted = int(((lt >= 0) & (lt < Cn)).sum())
    assert int((hist - hist_pattern(Cn, dev)).sum()) == counted and counted < lt.numel()          # labels outside [0, C) are ignored
    only_hist = raw(L, x, L.CRF_LOGITS, img, ref["size"], opts, dev, want_q=False, want_index=False, want_u8=False, lt=lt,
                    hist_init=torch.zeros(Cn, Cn, dtype=torch.int64, device=dev))[3]
    assert torch.equal(only_hist, want_hist - hist_pattern(Cn, dev))
    # the workspace is written before it is read: the same bits from a zeroed one as from one full of 0xFF bytes (NaNs)
    qz, indexz, _, _ = raw(L, x, L.CRF_LOGITS, img, ref["size"], opts, dev, ws_byte=0)
    assert torch.equal(qz, q) and torch.equal(indexz, index)
    # a sample's result does not depend on the batch around it
    if N > 1:
        for n in range(N):
            q1, index1, _, _ = raw(L, x[n:n + 1].contiguous(), L.CRF_LOGITS, img[n:n + 1].contiguous(), ref["size"], opts, dev)
            assert torch.equal(q1[0], q[n]) and torch.equal(index1[0], index[n]), (case, n)
    # the Python entry returns the same objects
    pu8, pidx, phist, pq = F.crf_labels(x.permute(0, 3, 1, 2), img.permute(0, 3, 1, 2), ref["size"], opts, want_q=True, want_index=True,
                                        label_true=lt, hist=hist_pattern(Cn, dev).clone())
    assert pq.shape == (N, Cn, oh, ow) and pq.is_contiguous(memory_format=CL) and pu8.dtype == torch.uint8 and pidx.dtype == torch.int64
    assert torch.equal(pq.permute(0, 2, 3, 1), q) and torch.equal(pidx, index) and torch.equal(pu8, u8) and torch.equal(phist, hist)
    fresh = F.crf_labels(x.permute(0, 3, 1, 2), img.permute(0, 3, 1, 2), ref["size"], opts, want_u8=False, label_true=lt)
    assert fresh[0] is None and fresh[1] is None and fresh[3] is None and torch.equal(fresh[2], only_hist)


def test_scores_outputs_agree_with_each_other_bit_for_bit(F, dev):
    L = load_sub("_lib")
    _, prob, img = _two_view_scores(F, dev)
    N, oh, ow, Cn = prob.shape
    opts = F.CrfOptions(iterations=3, **R.STRONG)
    lt = make_labels(Cn, N, oh, ow, 5, dev)
    q, index, u8, hist = raw(L, prob, L.CRF_PROBS, img, (oh, ow), opts, dev, lt=lt, hist_init=hist_pattern(Cn, dev))
    _, index2, _, hist2 = raw(L, prob, L.CRF_PROBS, img, (oh, ow), opts, dev, want_q=False, lt=lt, hist_init=hist_pattern(Cn, dev), ws_byte=0)
    first = F.argmax_index(q.permute(0, 3, 1, 2))
    assert torch.equal(index, first) and torch.equal(index2, first) and torch.equal(u8.to(torch.int64), first)
    assert torch.equal(hist, F.confusion_hist(lt, first, Cn, hist_pattern(Cn, dev).clone())) and torch.equal(hist2, hist)
    for n in range(N):
        q1 = raw(L, prob[n:n + 1].contiguous(), L.CRF_PROBS, img[n:n + 1].contiguous(), (oh, ow), opts, dev)[0]
        assert torch.equal(q1[0], q[n])
    pq = F.crf_labels(prob.permute(0, 3, 1, 2), img.permute(0, 3, 1, 2), (oh, ow), opts, probs=True, want_q=True)[3]
    assert torch.equal(pq.permute(0, 2, 3, 1), q)


# ------------------------------------------------------------------------------------------ 3. no iteration: the plain heads
@pytest.mark.parametrize("case", ["voc21_r3", "acdc4_r3d2", "c33_identity_one_step"])
def test_zero_iterations_on_logits_is_predict_labels(F, dev, case):
    L = load_sub("_lib")
    ref = reference(case, "strong")
    x, img = to_dev(ref, dev)
    N, _, _, Cn = x.shape
    oh, ow = ref["size"]
    lt = make_labels(Cn, N, oh, ow, 3, dev)
    opts = options(F, ref, "strong", iterations=0)
    want_u8, want_idx, want_hist = F.predict_labels(x.permute(0, 3, 1, 2), ref["size"], want_index=True, label_true=lt,
                                                    hist=hist_pattern(Cn, dev).clone())
    _, index, u8, hist = raw(L, x, L.CRF_LOGITS, img, ref["size"], opts, dev, want_q=False, lt=lt, hist_init=hist_pattern(Cn, dev))
    assert torch.equal(index, want_idx) and torch.equal(u8, want_u8) and torch.equal(hist, want_hist)
    pu8, pidx, phist, pq = F.crf_labels(x.permute(0, 3, 1, 2), img.permute(0, 3, 1, 2), ref["size"], opts, want_index=True, label_true=lt,
                                        hist=hist_pattern(Cn, dev).clone())
    assert pq is None and torch.equal(pidx, want_idx) and torch.equal(pu8, want_u8) and torch.equal(phist, want_hist)
    with pytest.raises(L.SscgError):
        F.crf_labels(x.permute(0, 3, 1, 2), img.permute(0, 3, 1, 2), ref["size"], opts, want_q=True)


def test_zero_iterations_on_scores_is_the_first_maximum_of_predict_labels_ms(F, dev):
    L = load_sub("_lib")
    views, prob, img = _two_view_scores(F, dev)
    N, oh, ow, Cn = prob.shape
    lt = make_labels(Cn, N, oh, ow, 4, dev)
    want_u8, want_idx, want_hist, _ = F.predict_labels_ms([v.permute(0, 3, 1, 2) for v in views], [False, True], (oh, ow), want_index=True,
                                                          label_true=lt, hist=hist_pattern(Cn, dev).clone())
    opts = F.CrfOptions(iterations=0)
    _, index, u8, hist = raw(L, prob, L.CRF_PROBS, img, (oh, ow), opts, dev, want_q=False, lt=lt, hist_init=hist_pattern(Cn, dev))
    assert torch.equal(index, want_idx) and torch.equal(u8, want_u8) and torch.equal(hist, want_hist)
    # a run-time class count and exact ties: the first maximum wins
    p7 = prob[..., :7].contiguous()
    p7[..., 5] = p7[..., 2]
    index7 = raw(L, p7, L.CRF_PROBS, img, (oh, ow), opts, dev, want_q=False, want_u8=False)[1]
    assert torch.equal(index7, F.argmax_index(p7.permute(0, 3, 1, 2))) and not bool((index7 == 5).any())


# ------------------------------------------------------------------------------------------ 4. the drivers
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


def _confusion(gt, labels, n):
    t, p = gt.reshape(-1).cpu().numpy(), labels.reshape(-1).cpu().numpy()
    keep = (t >= 0) & (t < n)
    return np.bincount(n * t[keep] + p[keep], minlength=n * n).reshape(n, n).astype(np.float64)


def test_evaluate_with_crf_counts_what_crf_labels_gives_per_batch(F, dev, tmp_path):
    U = load_sub("utils")
    m, batches = _model(dev, tmp_path)
    crf = U.parse_crf("iters=2,radius=2,dilation=2,wb=2,ws=1,alpha=6,beta=0.7,gamma=2")
    views = U.parse_tta("0.5,1.0:flip")
    before = {k: v.clone() for k, v in m.Gsi.state_dict().items()}
    conf, miou = _evaluate(m, batches, crf=crf)
    conf_tta, _ = _evaluate(m, batches, crf=crf, tta=views)
    conf_plain, miou_plain = _evaluate(m, batches)
    assert m.Gsi.training
    want, want_tta, moved = np.zeros((4, 4)), np.zeros((4, 4)), 0
    m.Gsi.eval()
    with torch.no_grad():
        for image, gt, _ in batches:
            image, gt = image.to(dev), gt.to(dev)
            logits = m.Gsi(image)
            idx = F.crf_labels(logits, image, (65, 65), crf, want_u8=False, want_index=True)[1]
            want += _confusion(gt, idx, 4)
            moved += int((idx != F.predict_labels(logits, (65, 65), want_u8=False, want_index=True)[1]).sum())
            prob = F.predict_labels_ms(*U.tta_logits(m.Gsi, image, views), (65, 65), want_prob=True, want_u8=False)[3]
            want_tta += _confusion(gt, F.crf_labels(prob, image, (65, 65), crf, probs=True, want_u8=False, want_index=True)[1], 4)
    m.Gsi.train()
    counted = sum(int((gt != 255).sum()) for _, gt, _ in batches)
    assert conf.sum() == counted and (conf == want).all() and (conf_tta == want_tta).all()
    assert moved > 0 and conf_plain.sum() == counted          # the CRF did move labels on these batches
    assert np.isfinite(miou) and np.isfinite(miou_plain)
    after = m.Gsi.state_dict()
    assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)
    # a guide of another size is resized to the crop
    assert U.crf_guide(batches[0][0].to(dev), (65, 65)) is not None and tuple(U.crf_guide(batches[0][0].to(dev), (33, 41)).shape) == (2, 3, 33, 41)


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
for tag, kw in (("plain", {}), ("crf", {"crf": U.parse_crf("iters=3")}), ("crf+tta", {"crf": U.parse_crf("on"), "tta": U.parse_tta("0.5,1.0")})):
    sys.stderr.write("[census] begin %%s\n" %% tag)
    m.evaluate(batches, **kw)
    torch.cuda.synchronize()
    sys.stderr.write("[census] end %%s\n" %% tag)
"""


def test_launch_census_of_an_evaluation_with_and_without_the_crf(dev, tmp_path):
    env = dict(os.environ, SSCG_TRACE="1")
    r = subprocess.run([sys.executable, "-c", CENSUS % (ROOT, os.path.join(ROOT, "tests"), str(tmp_path / "ckpt"))], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    counts = {}
    for tag in ("plain", "crf", "crf+tta"):
        body = r.stderr[r.stderr.index("[census] begin " + tag + "\n"):r.stderr.index("[census] end " + tag + "\n")]
        calls = {}
        for line in body.splitlines():
            if line.startswith("[sscg] "):
                name = line[7:].split("(")[0]
                calls[name] = calls.get(name, 0) + 1
        counts[tag] = calls
    plain, crf, both = counts["plain"], counts["crf"], counts["crf+tta"]
    # without the option: the launches of before - one fused head per batch, nothing of the CRF
    assert not any(name.startswith("sscg_crf") for name in plain), plain
    assert plain.get("sscg_predict_head", 0) == 2 and plain.get("sscg_predict_head_ms", 0) == 0, plain
    # with it: one sscg_crf_head per batch in place of the head (the size query is cached: at most one call)
    assert crf.get("sscg_crf_head", 0) == 2 and crf.get("sscg_predict_head", 0) == 0 and crf.get("sscg_crf_workspace", 0) <= 1, crf
    assert crf.get("sscg_upsample_bilinear_fwd", 0) == 0, crf               # the guide already has the crop's size
    # with views: the multi-scale head emits the summed probabilities, the CRF consumes them
    assert both.get("sscg_predict_head_ms", 0) == 2 and both.get("sscg_crf_head", 0) == 2 and both.get("sscg_resize_flip", 0) == 2, both
    assert both.get("sscg_argmax_onehot", 0) == 0 and both.get("sscg_confusion_hist", 0) == 0, both
