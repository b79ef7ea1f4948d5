"""Surface distances on the MI355X: sscg_surface_stats (csrc/surface.hip) against the numpy / scipy restatement of its definition
(tests/surface_reference.py, checked on its own in tests/test_surface_host.py), then the score keeper and the drivers.

The integer records must match bit for bit; a sum must lie within (cnt + 2) * 2^-52 * sum of the restatement's - the rounding bound of
an fp64 sum of cnt correctly rounded square roots added in another order.  Outputs and workspace are views into sentinel-filled
buffers whose guard bands must survive.  The random maps are smooth label maps (argmax of Gaussian-filtered noise); the module asserts
that at least 60 % of their cases are defined, so that it cannot pass on empty work."""
import contextlib
import functools
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import surface_reference as R
from conftest import ROOT, load_sub

pytestmark = pytest.mark.gpu
GUARD = 4096                  # bytes on either side of every buffer
SENT = 0xA5

# name: (N, H, W, C, seed, void ring): one pixel, one row, one column, smaller than a wave, one past a 32 tile in both axes, several
# blocks of the per-pixel passes, more classes than one chunk of the column / row passes holds (8), N = 1..3, C = 1 / 2 / 4 / 21 / 64
RANDOM = {
    "1x1_c4": (2, 1, 1, 4, 0, False),
    "1x7_c2": (3, 1, 7, 2, 1, False),
    "7x1_c2": (1, 7, 1, 2, 2, False),
    "5x9_c4": (2, 5, 9, 4, 3, False),
    "33x47_c4": (3, 33, 47, 4, 4, False),
    "33x47_c1": (2, 33, 47, 1, 5, False),
    "33x47_c2": (1, 33, 47, 2, 6, False),
    "64x64_c4": (2, 64, 64, 4, 7, False),
    "40x72_c21_void": (2, 40, 72, 21, 8, True),
    "33x47_c64": (1, 33, 47, 64, 9, False),
}
DEFAULT = (4, 95)             # tol2, pct


def _blobs():
    """Blobs of class 1 in opposite corners of 64 x 64: the distance exceeds any tile or halo; class 2 in the ground truth only,
    class 3 in neither."""
    gt = np.zeros((1, 64, 64), dtype=np.int64)
    pred = np.zeros((1, 64, 64), dtype=np.uint8)
    gt[0, 1:6, 2:9] = 1
    pred[0, 55:63, 50:62] = 1
    gt[0, 30:34, 30:40] = 2
    return gt, pred


def _over():
    gt, pred = R.make_case(40, 2, 33, 47, 4, pred_over=True)
    return gt, pred


def _checker():
    y, x = np.arange(17)[:, None], np.arange(23)[None, :]
    gt = np.broadcast_to((y + x) % 2, (2, 17, 23)).astype(np.int64).copy()
    pred = gt.astype(np.uint8).copy()
    pred[1] = 1 - pred[1]                      # sample 0: identical; sample 1: the complementary board, every d^2 = 1
    return gt, pred


def _straddle():
    """Three single pixels against one: d^2 = 5, 72, 6272 - at pct = 50 the ranks are 1 and 2, two values that differ in the selection's
    second digit, so v_hi is the next larger value and not v_lo."""
    gt = np.zeros((1, 64, 64), dtype=np.int64)
    pred = np.zeros((1, 64, 64), dtype=np.uint8)
    gt[0, 2, 3] = gt[0, 10, 10] = gt[0, 60, 60] = 1
    pred[0, 4, 4] = 1
    return gt, pred


# name: (maps, C, tol2, pct)
BUILT = {
    "straddle": (_straddle, 2, 4, 50),
    "corners": (_blobs, 4, 4, 95),
    "pred_over": (_over, 4, 4, 95),
    "checker": (_checker, 2, 0, 95),
    "pct100": (lambda: R.make_case(41, 2, 33, 47, 4), 4, 4, 100),
    "pct1": (lambda: R.make_case(42, 2, 33, 47, 4), 4, 4, 1),
    "pct50_tol0": (lambda: R.make_case(43, 1, 64, 64, 4), 4, 0, 50),
    "tol_large": (lambda: R.make_case(44, 1, 33, 47, 4), 4, 1 << 30, 95),
}


@functools.lru_cache(maxsize=None)
def reference(case):
    """Inputs and the restated records of one case, computed once and shared (read-only) by the tests that need them."""
    if case in RANDOM:
        N, H, W, Cn, seed, ring = RANDOM[case]
        gt, pred = R.make_case(seed, N, H, W, Cn, void_ring=ring)
        tol2, pct = DEFAULT
    else:
        maps, Cn, tol2, pct = BUILT[case]
        gt, pred = maps()
    st, sm = R.stats(gt, pred, Cn, tol2, pct)
    for a in (gt, pred, st, sm):
        a.setflags(write=False)
    return gt, pred, Cn, tol2, pct, st, sm


def _guarded(nbytes, dev, fill):
    buf = torch.full((nbytes + 2 * GUARD,), SENT, dtype=torch.uint8, device=dev)
    buf[GUARD:GUARD + nbytes] = fill
    return buf, buf[GUARD:GUARD + nbytes]


def raw(L, gt, pred, Cn, tol2, pct, dev, fill=0xFF):
    """sscg_surface_stats itself: stats, sums and the workspace (exactly the size the query promises) are views into sentinel-filled
    buffers, pre-filled with `fill`; the guard bands must survive."""
    lt, lp = torch.tensor(gt, device=dev), torch.tensor(pred, device=dev)          # (copies: the shared arrays are read-only)
    N, H, W = lt.shape
    need = L.lib.sscg_surface_workspace(N, H, W, Cn)
    assert need > 0
    bufs = [_guarded(b, dev, fill) for b in (2 * N * Cn * 5 * 8, 2 * N * Cn * 8, need)]
    assert all(v.data_ptr() % 256 == 0 for _, v in bufs)
    (_, st), (_, sm), (_, ws) = bufs
    rc = L.lib.sscg_surface_stats(lt.data_ptr(), lp.data_ptr(), N, H, W, Cn, tol2, pct, st.data_ptr(), sm.data_ptr(), ws.data_ptr(), need,
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for name, (buf, v) in zip(("stats", "sums", "workspace"), bufs):
        assert bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + v.numel():] == SENT).all()), "a store outside the " + name
    return st.view(torch.int64).reshape(2, N, Cn, 5).cpu().numpy(), sm.view(torch.float64).reshape(2, N, Cn).cpu().numpy()


def check(got, want, tag):
    (st, sm), (wst, wsm) = got, want
    assert np.array_equal(st, wst), "%s: records differ at %s" % (tag, np.argwhere(st != wst)[:8].tolist())
    bound = (wst[..., R.CNT] + 2) * 2.0 ** -52 * wsm
    worst = float((np.abs(sm - wsm) - bound).max())
    print("[surface] %-16s %3d defined / %3d missing / %3d empty; max |sum - ref| / bound = %.3f" % (
        (tag,) + R.case_census(wst) + (float((np.abs(sm - wsm) / np.where(bound > 0, bound, 1.0)).max()),)))
    assert worst <= 0.0, "%s: a sum is %.3e beyond its bound" % (tag, worst)
    assert (sm[wsm == 0.0] == 0.0).all()


# ------------------------------------------------------------------------------------------ 1. the kernels against the restatement
def test_random_cases_are_mostly_defined():
    d = m = 0
    for case in RANDOM:
        a, b, _ = R.case_census(reference(case)[5])
        d, m = d + a, m + b
    print("[surface] random cases: %d defined, %d missing" % (d, m))
    assert d >= 0.6 * (d + m) and d >= 40, (d, m)


@pytest.mark.parametrize("case", list(RANDOM) + list(BUILT))
def test_records_equal_the_restatement(dev, case):
    L = load_sub("_lib")
    gt, pred, Cn, tol2, pct, st, sm = reference(case)
    got = raw(L, gt, pred, Cn, tol2, pct, dev)
    check(got, (st, sm), case)
    # the same bits whatever the workspace and the outputs held before
    again = raw(L, gt, pred, Cn, tol2, pct, dev, fill=0x00)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1].view(np.int64), got[1].view(np.int64))
    # a sample's records do not depend on the batch around it
    if gt.shape[0] > 1:
        for n in range(gt.shape[0]):
            one = raw(L, gt[n:n + 1], pred[n:n + 1], Cn, tol2, pct, dev)
            assert np.array_equal(one[0][:, 0], got[0][:, n]) and np.array_equal(one[1][:, 0].view(np.int64), got[1][:, n].view(np.int64)), n


def test_built_cases_hold_what_they_were_built_for():
    gt, pred, Cn, _, _, st, sm = reference("corners")
    assert st[0, 0, 1, R.MAX2] > 48 ** 2 + 48 ** 2 and st[0, 0, 1, R.V_LO] > 32 ** 2          # farther than any tile or halo
    assert st[0, 0, 2].tolist() == [24, 0, -1, -1, -1] and st[1, 0, 2].tolist() == [0, 0, -1, -1, -1]          # one map only
    assert st[:, 0, 3, R.CNT].sum() == 0                                                        # neither
    gt, pred, Cn, _, _, st, _ = reference("pred_over")
    assert (pred == 200).any() and (pred == Cn).any() and R.case_census(st)[0] >= 4
    gt, pred, Cn, _, _, st, _ = reference("checker")
    assert (st[:, :, :, R.CNT].sum(axis=2) == 17 * 23).all()                                   # every pixel is surface
    assert (st[:, 0, :, R.MAX2] == 0).all() and (st[:, 1, :, R.V_LO] == 1).all() and (st[:, 1, :, R.WITHIN] == 0).all()
    st = reference("pct100")[5]
    d = st[..., R.CNT] > 0
    assert np.array_equal(st[..., R.V_LO][d], st[..., R.MAX2][d]) and np.array_equal(st[..., R.V_HI][d], st[..., R.MAX2][d])
    st1, st50 = reference("pct1")[5], reference("pct50_tol0")[5]
    assert (st1[..., R.V_LO] <= st1[..., R.V_HI]).all() and (st50[..., R.V_LO] < st50[..., R.MAX2]).any()
    assert reference("straddle")[5][0, 0, 1].tolist() == [3, 0, 6272, 72, 6272]                 # a rank pair that straddles two values
    big = reference("tol_large")[5]
    assert np.array_equal(big[..., R.WITHIN][big[..., R.MAX2] >= 0], big[..., R.CNT][big[..., R.MAX2] >= 0])


def test_wrapper_contiguity_given_buffers_and_refusals(F, dev):
    L = load_sub("_lib")
    gt, pred, Cn, tol2, pct, st, sm = reference("33x47_c4")
    lt, lp = torch.tensor(gt, device=dev), torch.tensor(pred, device=dev)
    opts = F.SurfaceOptions()
    assert (opts.tol2, opts.pct) == (tol2, pct)
    got = F.surface_stats(lt, lp, Cn, opts)
    assert got[0].dtype == torch.int64 and tuple(got[0].shape) == (2, 3, Cn, 5) and got[1].dtype == torch.float64
    check((got[0].cpu().numpy(), got[1].cpu().numpy()), (st, sm), "wrapper")
    # given outputs are used; non-contiguous inputs and another integer type of labels give the same records
    s2, m2 = torch.empty_like(got[0]), torch.empty_like(got[1])
    lt_t = lt.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    wide = torch.zeros(3, 33, 94, dtype=torch.uint8, device=dev)
    wide[:, :, ::2] = lp
    out = F.surface_stats(lt_t.to(torch.int32), wide[:, :, ::2], Cn, opts, stats=s2, sums=m2)
    assert out[0] is s2 and out[1] is m2 and torch.equal(s2, got[0]) and torch.equal(m2, got[1])
    with pytest.raises(L.SscgError):
        F.surface_stats(lt, lp[:, :, :44], Cn, opts)
    with pytest.raises(L.SscgError):
        F.surface_stats(lt, lp, Cn, opts, stats=torch.empty(2, 3, Cn, 4, dtype=torch.int64, device=dev))
    with pytest.raises(TypeError):
        F.surface_stats(lt, lp, Cn, (2.0, 95))
    with pytest.raises(L.SscgError):
        F.surface_stats(lt, lp, 65, opts)                                           # the entry's own refusal surfaces


# ------------------------------------------------------------------------------------------ 2. the score keeper and the drivers
def _close(got, want):
    assert set(got) == set(want)
    assert got["cases"] == want["cases"] and got["missing"] == want["missing"]
    for key in ("hd", "hd95", "assd", "nsd"):
        for a, b in [(got[key], want[key])] + [(got["class_" + key][c], want["class_" + key][c]) for c in want["class_" + key]]:
            assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-12 * max(1.0, abs(b)), (key, a, b)


@pytest.mark.parametrize("head", ["logits", "ms", "crf", "device"])
def test_running_score_scores_the_map_its_head_returns(F, dev, head):
    U = load_sub("utils")
    Cn, size = 4, (33, 41)
    g = torch.Generator().manual_seed(21)
    logits = torch.randn(2, Cn, 9, 9, generator=g).to(dev)
    image = torch.randn(2, 3, size[0], size[1], generator=g).to(dev)
    gt = torch.tensor(R.make_case(21, 2, size[0], size[1], Cn, void_ring=True)[0], device=dev)
    crf = F.CrfOptions(iterations=2, radius=2, dilation=1)
    half = F.resize_flip(logits, (5, 6), True)
    if head == "logits":
        update = lambda rs: rs.update_logits(gt, logits, size)
        u8 = F.predict_labels(logits, size)[0]
    elif head == "ms":
        update = lambda rs: rs.update_logits_ms(gt, [logits, half], [False, True], size)
        u8 = F.predict_labels_ms([logits, half], [False, True], size)[0]
    elif head == "crf":
        update = lambda rs: rs.update_logits_crf(gt, logits, image, size, crf)
        u8 = F.crf_labels(logits, image, size, crf)[0]
    else:
        idx = F.predict_labels(logits, size, want_u8=False, want_index=True)[1]
        update = lambda rs: rs.update_device(gt, idx)
        u8 = idx.to(torch.uint8)
    opts = F.SurfaceOptions(tol=1.0, pct=90)
    off, on = U.runningScore(Cn, "acdc"), U.runningScore(Cn, "acdc")
    on.set_surface(opts)
    for rs in (off, on):
        update(rs)
        update(rs)
    assert off._surface_records == [] and off.get_surface_scores() is None and len(on._surface_records) == 2
    assert torch.equal(on._device_hist, off._device_hist)                          # the confusion matrix: bitwise the one without
    st, sm = R.stats(gt.cpu().numpy(), u8.cpu().numpy(), Cn, opts.tol2, opts.pct)
    want = R.scores(np.concatenate([st, st], axis=1), np.concatenate([sm, sm], axis=1), Cn, "acdc", opts.pct)
    got = on.get_surface_scores()
    _close(got, want)
    assert sum(got["cases"].values()) >= 4 and np.isfinite(got["hd95"])
    assert on.get_scores()[0]["Mean IoU : \t"] == off.get_scores()[0]["Mean IoU : \t"]
    on.reset()
    assert on._surface_records == [] and on.get_surface() == opts


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
        gt = R.make_case(30 + k, 2, 65, 65, 4, void_ring=True)[0]
        batches.append((torch.randn(2, 3, 65, 65, generator=g), torch.tensor(gt).unsqueeze(1), ["a", "b"]))
    return m, batches


def test_evaluate_with_surface_scores_the_maps_it_predicts(F, dev, tmp_path):
    U = load_sub("utils")
    m, batches = _model(dev, tmp_path)
    miou_off, _ = m.evaluate(batches)
    assert not hasattr(m, "eval_surface") and not hasattr(m, "eval_boundary")
    opts = U.parse_surface("tol=1.5,pct=90")
    m.set_surface(opts)
    miou_on, _ = m.evaluate(batches)
    assert miou_on == miou_off and m.Gsi.training and not hasattr(m, "eval_boundary")
    sts, sms = [], []
    m.Gsi.eval()
    with torch.no_grad():
        for image, gt, _ in batches:
            u8 = F.predict_labels(m.Gsi(image.to(dev)), (65, 65))[0]
            st, sm = R.stats(gt.squeeze(1).numpy(), u8.cpu().numpy(), 4, opts.tol2, opts.pct)
            sts.append(st)
            sms.append(sm)
    m.Gsi.train()
    want = R.scores(np.concatenate(sts, axis=1), np.concatenate(sms, axis=1), 4, "acdc", opts.pct)
    alone = dict(m.eval_surface)
    _close(alone, want)
    assert sum(alone["cases"].values()) + sum(alone["missing"].values()) >= 4
    # with --boundary beside it: both score sets, each equal to its value alone
    boundary = U.parse_boundary("d=3")
    miou_both, _ = m.evaluate(batches, boundary=boundary)
    both_s, both_b = dict(m.eval_surface), dict(m.eval_boundary)
    m.set_surface(None)
    miou_b, _ = m.evaluate(batches, boundary=boundary)
    assert not hasattr(m, "eval_surface") and miou_both == miou_b == miou_off
    same = lambda a, b: a == b or (np.isnan(a) and np.isnan(b))
    for key in ("hd", "hd95", "assd", "nsd"):
        assert same(both_s[key], alone[key]) and all(same(both_s["class_" + key][c], alone["class_" + key][c]) for c in range(4)), key
    assert both_s["cases"] == alone["cases"] and both_s["missing"] == alone["missing"]
    for key in ("boundary_iou", "trimap_iou"):
        assert same(both_b[key], m.eval_boundary[key]), key
    # switched off again, the attribute goes
    m.evaluate(batches)
    assert not hasattr(m, "eval_surface") and not hasattr(m, "eval_boundary")


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
for tag, surface, kw in (("plain", None, {}), ("surface", "on", {}), ("plain again", None, {}),
                         ("surface+boundary", "tol=1", {"boundary": U.parse_boundary("d=3")})):
    m.set_surface(U.parse_surface(surface))
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
    for tag in ("plain", "surface", "plain again", "surface+boundary"):
        body = r.stderr[r.stderr.index("[census] begin " + tag + "\n"):r.stderr.index("[census] end " + tag + "\n")]
        calls = {}
        for line in body.splitlines():
            if line.startswith("[sscg] "):
                name = line[7:].split("(")[0]
                calls[name] = calls.get(name, 0) + 1
        counts[tag] = calls
    plain, on, again, both = counts["plain"], counts["surface"], counts["plain again"], counts["surface+boundary"]
    # without the option: the launches of before - one fused head per batch, nothing of the surface distances - also after a run with it
    assert plain.get("sscg_surface_stats", 0) == 0 and plain.get("sscg_surface_workspace", 0) == 0, plain
    assert plain.get("sscg_predict_head", 0) == 2 and plain.get("sscg_boundary_counts", 0) == 0, plain
    assert again == plain, (plain, again)
    # with it: one sscg_surface_stats per batch and one size query for the shape; every other launch as without
    extra = {k: v - plain.get(k, 0) for k, v in on.items() if v != plain.get(k, 0)}
    assert extra == {"sscg_surface_stats": 2, "sscg_surface_workspace": 1} and set(plain) <= set(on), (plain, on)
    assert both.get("sscg_surface_stats", 0) == 2 and both.get("sscg_boundary_counts", 0) == 2 and both.get("sscg_predict_head", 0) == 2, both
