"""Connected-component filtering on the MI355X: sscg_components_filter (csrc/components.hip) against the numpy / scipy restatement of its
definition (tests/components_reference.py, checked on its own in tests/test_components_host.py), then the score keeper and the drivers.

Everything is an integer and must match bit for bit: the filtered map, the confusion matrix, the stats.  Outputs and workspace are views
of exactly the promised size between 0xA5 guard bands, which must survive.  The random maps are speckled smooth label maps whose seeds
the host test holds to conditions (something removed, something kept, components across tile seams), so that this module cannot pass on
empty work; the built cases are the shapes a block-based union-find can get wrong (tests/components_reference.py: BUILT)."""
import contextlib
import functools
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import components_reference as R
from conftest import ROOT, load_sub

pytestmark = pytest.mark.gpu
GUARD = 4096                  # bytes on either side of every buffer
SENT = 0xA5


def _key(kw):
    return tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(label_true, label_pred, C, settings) of one case, made once and shared read-only."""
    if case in R.RANDOM:
        N, H, W, Cn, seed, ring = R.RANDOM[case]
        gt, pred = R.make_case(seed, N, H, W, Cn, void_ring=ring)
        settings = R.random_settings(Cn)
    else:
        pred, Cn, settings = R.BUILT[case]()
        gt = R.built_truth(pred, Cn)
    gt.setflags(write=False)
    pred.setflags(write=False)
    return gt, pred, Cn, tuple(_key(kw) for kw in settings)


@functools.lru_cache(maxsize=None)
def reference(case, key):
    """The restated (label_out, hist, stats) of one case under one setting, computed once and shared read-only."""
    gt, pred, Cn, _ = inputs(case)
    out = R.filter_maps(pred, Cn, label_true=gt, **dict(key))
    for a in out:
        a.setflags(write=False)
    return out


def _guarded(nbytes, dev, fill):
    buf = torch.full((nbytes + 2 * GUARD,), SENT, dtype=torch.uint8, device=dev)
    buf[GUARD:GUARD + nbytes] = fill
    return buf, buf[GUARD:GUARD + nbytes]


def raw(L, gt, pred, Cn, kw, dev, fill=0xFF, in_place=False, prior=None, want_hist=True, want_stats=True):
    """sscg_components_filter itself: label_out, stats and the workspace (exactly the size the query promises) are views into
    sentinel-filled buffers, pre-filled with `fill`; hist starts from `prior` (zeros when None); the guard bands must survive.
    Returns (label_out, hist, stats) as numpy arrays."""
    lp = torch.tensor(pred, device=dev)                                               # (copies: the shared arrays are read-only)
    lt = torch.tensor(gt, device=dev) if gt is not None else None
    N, H, W = lp.shape
    need = L.lib.sscg_components_workspace(N, H, W, Cn)
    assert need > 0
    bufs = [_guarded(b, dev, fill) for b in (N * H * W, N * Cn * 4 * 8, need, Cn * Cn * 8)]
    assert all(v.data_ptr() % 256 == 0 for _, v in bufs)
    (ob, out), (_, st), (_, ws), (_, hist) = bufs
    if in_place:
        out[:] = lp.reshape(-1)
    hist.view(torch.int64)[:] = (torch.zeros(Cn * Cn, dtype=torch.int64) if prior is None else torch.tensor(prior.reshape(-1))).to(dev)
    kw = dict(dict(conn=8, largest=False, min_area=0, fill=0, skip=()), **kw)
    rc = L.lib.sscg_components_filter(out.data_ptr() if in_place else lp.data_ptr(), lt.data_ptr() if lt is not None else None, N, H, W, Cn,
                                      kw["conn"], int(kw["largest"]), kw["min_area"], kw["fill"], sum(1 << s for s in kw["skip"]),
                                      out.data_ptr(), hist.data_ptr() if want_hist and lt is not None else None,
                                      st.data_ptr() if want_stats else None, ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for name, (buf, v) in zip(("label_out", "stats", "workspace", "hist"), bufs):
        assert bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + v.numel():] == SENT).all()), "a store outside the " + name
    return (out.reshape(N, H, W).cpu().numpy(), hist.view(torch.int64).reshape(Cn, Cn).cpu().numpy(),
            st.view(torch.int64).reshape(N, Cn, 4).cpu().numpy())


def same(got, want, tag):
    for name, a, b in zip(("label_out", "hist", "stats"), got, want):
        assert np.array_equal(a, b), "%s: %s differs at %s (got %s, expected %s)" % (
            tag, name, np.argwhere(a != b)[:6].tolist(), a[a != b][:6].tolist(), b[a != b][:6].tolist())


# ------------------------------------------------------------------------------------------ 1. the kernels against the restatement
@pytest.mark.parametrize("case", list(R.RANDOM) + list(R.BUILT))
def test_filter_equals_the_restatement(dev, case):
    L = load_sub("_lib")
    gt, pred, Cn, settings = inputs(case)
    removed = 0
    for key in settings:
        want = reference(case, key)
        got = raw(L, gt, pred, Cn, dict(key), dev)
        same(got, want, "%s %s" % (case, dict(key)))
        removed += int((want[0] != pred).sum())
    print("[components] %-16s %d settings, %d pixels relabelled in all" % (case, len(settings), removed))


@pytest.mark.parametrize("case", ["33x47_c4", "40x72_c21_void", "65x130_c4", "serpentine", "holes", "sample_border"])
def test_in_place_workspace_contents_reproducibility_and_nullable_outputs(dev, case):
    L = load_sub("_lib")
    gt, pred, Cn, settings = inputs(case)
    for key in settings[:3]:
        kw, want = dict(key), reference(case, key)
        first = raw(L, gt, pred, Cn, kw, dev, fill=0xFF)
        same(first, want, case)
        # the same bits whatever the workspace, label_out and stats held before, and on a second call
        same(raw(L, gt, pred, Cn, kw, dev, fill=0x00), first, case + " (workspace of zeros)")
        same(raw(L, gt, pred, Cn, kw, dev, fill=0xFF), first, case + " (again)")
        # label_out aliasing label_pred
        same(raw(L, gt, pred, Cn, kw, dev, in_place=True), first, case + " (in place)")
        # hist accumulates onto what it held; without label_true / hist / stats the map is the same and the buffers stay untouched
        prior = np.arange(Cn * Cn, dtype=np.int64).reshape(Cn, Cn) * 1000003
        got = raw(L, gt, pred, Cn, kw, dev, prior=prior)
        assert np.array_equal(got[1], prior + want[1]) and np.array_equal(got[0], want[0])
        bare = raw(L, None, pred, Cn, kw, dev, fill=0x5C, want_stats=False)
        assert np.array_equal(bare[0], want[0]) and not bare[1].any() and (bare[2].view(np.uint8) == 0x5C).all()
        nohist = raw(L, gt, pred, Cn, kw, dev, fill=0x5C, want_hist=False)
        assert np.array_equal(nohist[0], want[0]) and not nohist[1].any() and np.array_equal(nohist[2], want[2])


def test_a_sample_does_not_depend_on_the_batch_around_it(dev):
    L = load_sub("_lib")
    gt, pred, Cn, settings = inputs("33x47_c4")
    for key in settings[:2]:
        whole = reference("33x47_c4", key)
        for n in range(pred.shape[0]):
            one = raw(L, gt[n:n + 1], pred[n:n + 1], Cn, dict(key), dev)
            assert np.array_equal(one[0][0], whole[0][n]) and np.array_equal(one[2][0], whole[2][n]), n


def test_wrapper_hist_given_buffers_and_refusals(F, dev):
    L = load_sub("_lib")
    case, key = "33x47_c4", _key(dict(largest=True, min_area=8, skip=(1,)))
    gt, pred, Cn, settings = inputs(case)
    assert key in settings
    want = reference(case, key)
    opts = F.ComponentOptions(largest=True, min_area=8, skip=(1,))
    lt, lp = torch.tensor(gt, device=dev), torch.tensor(pred, device=dev)
    u8, hist, stats = F.component_filter(lp, Cn, opts, label_true=lt, stats=True)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == lp.shape and hist.dtype == torch.int64 and tuple(stats.shape) == (3, Cn, 4)
    same((u8.cpu().numpy(), hist.cpu().numpy(), stats.cpu().numpy()), want, "wrapper")
    assert torch.equal(lp, torch.tensor(pred, device=dev))                                  # the input is not written
    # hist is sscg_confusion_hist's of the filtered map, and accumulates
    assert torch.equal(hist, F.confusion_hist(lt, u8, Cn))
    u8b, hist2, none = F.component_filter(lp, Cn, opts, label_true=lt, hist=hist)
    assert hist2 is hist and none is None and torch.equal(hist, 2 * torch.tensor(want[1], device=dev)) and torch.equal(u8b, u8)
    # without a ground truth: the map alone
    only, h0, s0 = F.component_filter(lp, Cn, opts)
    assert h0 is None and s0 is None and torch.equal(only, u8)
    # given outputs are used (in place too); int64 class ids and non-contiguous inputs give the same bytes
    out, st = torch.empty_like(lp), torch.empty(3, Cn, 4, dtype=torch.int64, device=dev)
    wide = torch.zeros(3, 33, 94, dtype=torch.int64, device=dev)
    wide[:, :, ::2] = lp
    got = F.component_filter(wide[:, :, ::2], Cn, opts, label_true=lt.to(torch.int32), out=out, stats=st)
    assert got[0] is out and got[2] is st and torch.equal(out, u8) and torch.equal(st, stats) and torch.equal(got[1], torch.tensor(want[1], device=dev))
    work = lp.clone()
    assert F.component_filter(work, Cn, opts, out=work)[0] is work and torch.equal(work, u8)
    with pytest.raises(L.SscgError):
        F.component_filter(lp, Cn, opts, label_true=lt[:, :, :44])
    with pytest.raises(L.SscgError):
        F.component_filter(lp, Cn, opts, hist=hist)                                         # a confusion matrix needs label_true
    with pytest.raises(L.SscgError):
        F.component_filter(lp, Cn, opts, stats=torch.empty(3, Cn, 5, dtype=torch.int64, device=dev))
    with pytest.raises(L.SscgError):
        F.component_filter(lp, Cn, opts, out=torch.empty(3, 33, 47, dtype=torch.int64, device=dev))
    with pytest.raises(L.SscgError):
        F.component_filter(lp[0], Cn, opts)
    with pytest.raises(TypeError):
        F.component_filter(lp, Cn, "largest")
    with pytest.raises(L.SscgError):
        F.component_filter(lp, Cn, F.ComponentOptions(largest=True, fill=Cn))               # not a class


# ------------------------------------------------------------------------------------------ 2. the score keeper and the drivers
@pytest.mark.parametrize("head", ["logits", "ms", "crf", "device"])
def test_running_score_scores_the_filtered_map(F, dev, head):
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
    opts = F.ComponentOptions(largest=True, fill=0, skip=(3,))
    want_u8, want_hist, want_st = R.filter_maps(u8.cpu().numpy(), Cn, label_true=gt.cpu().numpy(), largest=True, skip=(3,))
    assert (want_u8 != u8.cpu().numpy()).sum() >= 1, "the head's map has nothing to remove: the test would show nothing"
    filtered = torch.tensor(want_u8, device=dev)
    surface, boundary = F.SurfaceOptions(tol=1.0, pct=90), F.BoundaryOptions(d=2)
    off, on = U.runningScore(Cn, "acdc"), U.runningScore(Cn, "acdc")
    on.set_components(opts)
    for rs in (off, on):
        rs.set_surface(surface)
        rs.set_boundary(boundary)
        update(rs)
        update(rs)
    assert off._component_stats == [] and off.get_component_scores() is None and len(on._component_stats) == 2
    # the confusion matrix, the contour counts and the surface records are those of the restatement's filtered map
    assert np.array_equal(on._device_hist.cpu().numpy(), 2 * want_hist) and not torch.equal(on._device_hist, off._device_hist)
    assert torch.equal(on._boundary_counts, 2 * F.boundary_counts(gt, filtered, Cn, 2))
    st, sm = F.surface_stats(gt, filtered, Cn, surface)
    for rec in on._surface_records:
        assert torch.equal(rec[0], st) and torch.equal(rec[1], sm)
    assert not torch.equal(on._boundary_counts, off._boundary_counts)
    got = on.get_component_scores()
    tot = 2 * want_st.sum(axis=0)
    assert got["components"] == int(tot[:, 0].sum()) and got["kept_components"] == int(tot[:, 1].sum())
    assert got["removed_pixels"] == 2 * int((want_u8 != u8.cpu().numpy()).sum()) > 0
    assert got["class_removed_pixels"] == {c: (0 if c == 0 else int(tot[c, 2] - tot[c, 3])) for c in range(Cn)}
    assert got["class_components"][3] == got["class_kept_components"][3] and got["class_removed_pixels"][3] == 0        # skipped
    h = 2.0 * want_hist
    assert on.get_scores()[0]["Mean IoU : \t"] == np.nanmean(U.kept_iou(h, Cn, "acdc"))
    on.reset()
    assert on._component_stats == [] and on.get_components() == opts and on.get_component_scores()["components"] == 0


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


def test_evaluate_with_components_scores_the_filtered_maps(F, dev, tmp_path):
    U = load_sub("utils")
    m, batches = _model(dev, tmp_path)
    rs = m.running_metrics_val
    seen = []                                          # the confusion matrix of each evaluation, taken when evaluate() clears it
    plain_reset = rs.reset
    rs.reset = lambda: (seen.append(rs.confusion_matrix.copy()), plain_reset())[1]
    last = lambda: [h for h in seen if h.sum() > 0][-1]
    miou_off, iou_off = m.evaluate(batches)
    assert not hasattr(m, "eval_components")
    h_off = last()
    # min_area = 1 without `largest` filters nothing: the same scores, and the attribute is there
    m.set_components(U.parse_components("min_area=1"))
    miou_one, iou_one = m.evaluate(batches)
    assert miou_one == miou_off and iou_one == iou_off and np.array_equal(last(), h_off) and m.Gsi.training
    assert m.eval_components["removed_pixels"] == 0 and m.eval_components["components"] == m.eval_components["kept_components"] > 0
    # under `largest`: another confusion matrix, the restatement's
    m.set_components(U.parse_components("largest"))
    miou_on, iou_on = m.evaluate(batches)
    h_on = last()
    want, removed, comps = np.zeros((4, 4), dtype=np.int64), 0, 0
    m.Gsi.eval()
    with torch.no_grad():
        for image, gt, _ in batches:
            u8 = F.predict_labels(m.Gsi(image.to(dev)), (65, 65))[0].cpu().numpy()
            out, hist, st = R.filter_maps(u8, 4, label_true=gt.squeeze(1).numpy(), largest=True)
            want, removed, comps = want + hist, removed + int((out != u8).sum()), comps + int(st[..., 0].sum())
    m.Gsi.train()
    assert removed > 0 and not np.array_equal(h_on, h_off), "the maps this model predicts have nothing to remove"
    assert np.array_equal(h_on, want.astype(np.float64))
    assert miou_on == np.nanmean(U.kept_iou(want.astype(np.float64), 4, "acdc"))
    assert m.eval_components["removed_pixels"] == removed and m.eval_components["components"] == comps
    # with --surface and --boundary beside it: the same filtering and confusion matrix; what the contour options score is pinned in
    # test_running_score_scores_the_filtered_map
    m.set_surface(U.parse_surface("on"))
    m.evaluate(batches, boundary=U.parse_boundary("d=3"))
    assert hasattr(m, "eval_surface") and hasattr(m, "eval_boundary") and m.eval_components["removed_pixels"] == removed
    assert np.array_equal(last(), h_on)
    # switched off again, the attribute goes and the scores are the plain ones
    m.set_surface(None)
    m.set_components(None)
    miou_again, _ = m.evaluate(batches)
    assert miou_again == miou_off and not hasattr(m, "eval_components") and np.array_equal(last(), h_off)


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
for tag, components, surface, kw in (("plain", None, None, {}), ("components", "largest,min_area=8", None, {}), ("plain again", None, None, {}),
                                     ("contours", None, "tol=1", {"boundary": U.parse_boundary("d=3")}),
                                     ("all", "on", "tol=1", {"boundary": U.parse_boundary("d=3")})):
    m.set_components(U.parse_components(components))
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
    for tag in ("plain", "components", "plain again", "all", "contours"):
        body = r.stderr[r.stderr.index("[census] begin " + tag + "\n"):r.stderr.index("[census] end " + tag + "\n")]
        calls = {}
        for line in body.splitlines():
            if line.startswith("[sscg] "):
                name = line[7:].split("(")[0]
                calls[name] = calls.get(name, 0) + 1
        counts[tag] = calls
    plain, on, again, both, contours = (counts[k] for k in ("plain", "components", "plain again", "all", "contours"))
    # without the option: the launches of before - one fused head per batch, nothing of the filter - also after a run with it
    assert plain.get("sscg_components_filter", 0) == 0 and plain.get("sscg_components_workspace", 0) == 0, plain
    assert plain.get("sscg_predict_head", 0) == 2 and plain.get("sscg_surface_stats", 0) == 0, plain
    assert again == plain, (plain, again)
    # with it: one sscg_components_filter per batch and one size query for the shape; the head as often as before; at most one fill
    # more (the confusion matrix is zeroed by the filter's wrapper instead of the head's: in fact none)
    extra = {k: v - plain.get(k, 0) for k, v in on.items() if v != plain.get(k, 0)}
    fills = extra.pop("sscg_fill", 0)
    assert extra == {"sscg_components_filter": 2, "sscg_components_workspace": 1} and 0 <= fills <= 1 and set(plain) <= set(on), (plain, on)
    assert on["sscg_predict_head"] == 2
    # beside the contour options: the filter's launches more than the contour options alone (every size was queried before)
    more = {k: v - contours.get(k, 0) for k, v in both.items() if v != contours.get(k, 0)}
    assert 0 <= more.pop("sscg_fill", 0) <= 1 and more == {"sscg_components_filter": 2}, (contours, both)
    assert both["sscg_surface_stats"] == 2 and both["sscg_boundary_counts"] == 2 and both["sscg_predict_head"] == 2, both
