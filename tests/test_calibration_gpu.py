"""Calibration counts on the MI355X: sscg_calib_stats (csrc/calib.hip) against the numpy restatement of its definition
(tests/calibration_reference.py, checked on its own in tests/test_calibration_host.py), then the wrapper, the score keeper and the
drivers.

The oracle probability map of every case comes from the device's SEPARATE passes - F.softmax2d(F.upsample_bilinear(logits, size) *
inv_T) with a torch fp32 multiply, or the given score map times `scale` - copied to the host and fed to the restatement.
  * The integer outputs (pixels, hits, Q24 confidence sums per bin and per predicted class) must be equal bit for bit, no pixel left out.
  * The fp64 sums are held to a relative 1e-9: the only differences are the summation order and the last ulp of the fp64 logarithm;
    n positive terms added in another order differ by less than n * 2^-53 relative, 1.5e-11 at the 2^17 + 1026 pixels of the largest case
    here.  Every test prints the distance it measured before it asserts.
Outputs and workspace are views into 0xFF-filled buffers whose guard bands must survive; the workspace has exactly the size the query
promises and starts as 0xFF bytes (NaNs: a record read before it is written would poison the sums)."""
import contextlib
import functools
import io
import math

import numpy as np
import pytest
import torch

import calibration_reference as R
from conftest import load_sub

pytestmark = pytest.mark.gpu
GUARD = 4096
SENT = 0xFF
Q = 1 << 24
CAP_PIXELS = 512 * 256        # include/sscg.h: "grid-stride over at most 512 workgroups of 256 threads"
GRID8 = (1.0, 0.5, 0.75, 1.5, 2.0, 3.0, 0.9, 1.1)

# name: (N, C, H, W, OH, OW, B, temps, seed)
RANDOM = {
    "c21_ragged_small": (2, 21, 5, 7, 19, 23, 15, (1.0,), 0),               # compile-time C, ragged resize, less than one workgroup
    "c4_ident": (2, 4, 16, 16, 16, 16, 15, (1.0,), 1),                      # the identity resize
    "c20_resize": (2, 20, 6, 5, 16, 18, 10, (1.0, 2.0), 2),
    "c5_b32_nt8": (2, 5, 7, 6, 20, 21, 32, GRID8, 3),                       # the run-time class path, the largest bin table
    "c64_b32_nt8": (2, 64, 4, 5, 12, 13, 32, GRID8, 4),
    "c1": (2, 1, 5, 5, 9, 9, 15, (1.0, 2.0), 5),                            # confidence is always 1
    "c21_many_nt8": (3, 21, 33, 33, 129, 129, 15, GRID8, 6),                # many workgroups
    "c4_past_the_cap": (2, 4, 257, 257, 257, 257, 10, (1.0,), 7),           # more pixels than the capped grid has threads: a second trip
}


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cpu().numpy()


def _labels(rng, N, OH, OW, C):
    lab = rng.randint(0, C, size=(N, OH, OW)).astype(np.int64)
    for value in (-1, 255, C):                                               # not counted: below, the void id, one past the classes
        lab[rng.rand(N, OH, OW) < 0.04] = value
    return lab


def oracle_probs(F, logits, size, inv_temps):
    """The separate passes on the device: resize, one torch fp32 multiply per temperature, softmax -> NT host maps [N, OH, OW, C]."""
    with torch.no_grad():
        z = F.upsample_bilinear(logits, size)
        return [_nhwc(F.softmax2d(z * torch.tensor(it, dtype=torch.float32, device=z.device))) for it in inv_temps]


@functools.lru_cache(maxsize=None)
def reference(case):
    """Inputs and the restated counts of one random case, computed once and shared (read-only) by the tests that need them."""
    F = load_sub("functional")
    N, C, H, W, OH, OW, B, temps, seed = RANDOM[case]
    rng = np.random.RandomState(seed)
    logits = (rng.randn(N, C, H, W) * 3.0).astype(np.float32)
    lab = _labels(rng, N, OH, OW, C)
    opts = F.CalibrationOptions(bins=B, temps=temps)
    probs = oracle_probs(F, torch.tensor(logits, device="cuda:0"), (OH, OW), opts.inv_temps)
    want = R.stats(probs, lab, B)
    for a in (logits, lab) + want:
        a.setflags(write=False)
    return logits, lab, opts, want


def _guarded(nbytes, dev, fill):
    buf = torch.full((nbytes + 2 * GUARD,), SENT, dtype=torch.uint8, device=dev)
    buf[GUARD:GUARD + nbytes] = fill
    return buf, buf[GUARD:GUARD + nbytes]


def raw(L, x_nhwc, kind, scale, geom, lab, inv_temps, B, dev, ws_short=0):
    """sscg_calib_stats itself on a channels-last device tensor: bins, cls, sums (zeroed) and the workspace (exactly the size the query
    promises, 0xFF-filled) are views into sentinel-filled buffers; the guard bands must survive.  Returns (rc, bins, cls, sums)."""
    N, H, W, C, OH, OW = geom
    nt = len(inv_temps)
    lt = torch.tensor(lab, device=dev)
    need = L.lib.sscg_calib_workspace(N, OH, OW, nt)
    assert need == min(-(-(N * OH * OW) // 256), 512) * nt * 16
    bufs = [_guarded(nt * B * 24, dev, 0), _guarded(nt * C * 24, dev, 0), _guarded(nt * 16, dev, 0), _guarded(need, dev, SENT)]
    (_, bn), (_, cl), (_, sm), (_, ws) = bufs
    its = (L.C.c_float * nt)(*inv_temps)
    rc = L.lib.sscg_calib_stats(x_nhwc.data_ptr(), kind, scale, N, H, W, C, OH, OW, lt.data_ptr(), its, nt, B, bn.data_ptr(), cl.data_ptr(),
                                sm.data_ptr(), ws.data_ptr(), need - ws_short, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for name, (buf, v) in zip(("bins", "cls", "sums", "workspace"), bufs):
        assert bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + v.numel():] == SENT).all()), "a store outside the " + name
    return (rc, bn.view(torch.int64).reshape(nt, B, 3).cpu().numpy(), cl.view(torch.int64).reshape(nt, C, 3).cpu().numpy(),
            sm.view(torch.float64).reshape(nt, 2).cpu().numpy())


def raw_logits(F, L, logits, size, lab, opts, dev):
    x = F.to_nhwc(torch.tensor(logits, device=dev))
    N, C, H, W = x.shape
    rc, bn, cl, sm = raw(L, x, 0, 1.0, (N, H, W, C, size[0], size[1]), lab, opts.inv_temps, opts.bins, dev)
    assert rc == 0, rc
    return bn, cl, sm


def check(tag, got, want):
    """Integers bit for bit; the fp64 sums within a relative 1e-9 (the module docstring derives it), the distance printed first."""
    (bn, cl, sm), (wb, wc, ws) = got, want
    with np.errstate(invalid="ignore", divide="ignore"):
        dist = float(np.nanmax(np.where(ws != 0, np.abs(sm - ws) / np.abs(ws), np.abs(sm))))
    print("[calibration] %-24s %8d counted, max |sum - ref| / |ref| = %.3e" % (tag, int(wb[0, :, 0].sum()), dist))
    assert bn.dtype == np.int64 and np.array_equal(bn, wb), tag
    assert cl.dtype == np.int64 and np.array_equal(cl, wc), tag
    assert np.isfinite(sm).all() and dist <= 1e-9, (tag, dist)


# ------------------------------------------------------------------------------------------ the entry against the restatement
@pytest.mark.parametrize("case", sorted(RANDOM))
def test_counts_equal_the_restatement_of_the_separate_passes(F, dev, case):
    L = load_sub("_lib")
    N, C, H, W, OH, OW, B, temps, _ = RANDOM[case]
    logits, lab, opts, want = reference(case)
    if case == "c4_past_the_cap":
        assert N * OH * OW > CAP_PIXELS
    got = raw_logits(F, L, logits, (OH, OW), lab, opts, dev)
    check(case, got, want)
    counted = int(((lab >= 0) & (lab < C)).sum())
    assert 0 < counted < lab.size                                               # some pixels are ignored, and not all
    for t in range(len(temps)):
        assert got[0][t, :, 0].sum() == counted == got[1][t, :, 0].sum() and got[0][t, :, 1].sum() == got[1][t, :, 1].sum()
    if C == 1:
        assert got[0][0, B - 1].tolist() == [counted, counted, counted * Q] and got[2][0, 0] == 0.0 and got[2][0, 1] == 0.0
    else:
        assert (got[0][0, :, 0] > 0).sum() >= 3                                  # the confidences spread over the diagram


@pytest.mark.parametrize("case", ["c21_ragged_small", "c4_ident", "c5_b32_nt8"])
def test_counts_agree_with_the_confusion_matrix_of_the_label_head(F, dev, case):
    L = load_sub("_lib")
    N, C, H, W, OH, OW, B, temps, _ = RANDOM[case]
    logits, lab, opts, _ = reference(case)
    bn, cl, _ = raw_logits(F, L, logits, (OH, OW), lab, opts, dev)
    hist = F.predict_labels(torch.tensor(logits, device=dev), (OH, OW), label_true=torch.tensor(lab, device=dev))[2].cpu().numpy()
    assert bn[0, :, 0].sum() == hist.sum() and bn[0, :, 1].sum() == np.trace(hist)
    assert np.array_equal(cl[0, :, 0], hist.sum(axis=0)) and np.array_equal(cl[0, :, 1], np.diag(hist))


def test_scores_of_several_views_and_of_the_crf(F, dev):
    """kind = 1: prob_sum of F.predict_labels_ms over two views with scale = 0.5, and the Q of F.crf_labels with scale = 1."""
    L = load_sub("_lib")
    C, size, B = 5, (21, 26), 15
    g = torch.Generator().manual_seed(11)
    logits = (torch.randn(2, C, 9, 9, generator=g) * 3).to(dev)
    half = F.resize_flip(logits, (5, 6), True)
    image = torch.randn(2, 3, size[0], size[1], generator=g).to(dev)
    lab = _labels(np.random.RandomState(11), 2, size[0], size[1], C)
    prob = F.predict_labels_ms([logits, half], [False, True], size, want_prob=True)[3]
    q = F.crf_labels(logits, image, size, F.CrfOptions(iterations=2, radius=2, dilation=1), want_q=True)[3]
    for tag, scores, scale in (("two views, scale 0.5", prob, 0.5), ("crf q, scale 1", q, 1.0)):
        x = F.to_nhwc(scores)
        assert x.is_contiguous(memory_format=torch.channels_last)
        rc, bn, cl, sm = raw(L, x, 1, scale, (2, size[0], size[1], C, size[0], size[1]), lab, [1.0], B, dev)
        assert rc == 0, rc
        want = R.stats([_nhwc(scores * torch.tensor(scale, dtype=torch.float32, device=dev))], lab, B)
        check(tag, (bn, cl, sm), want)
    # and through the wrapper, accumulated twice
    opts = F.CalibrationOptions(bins=B)
    lt = torch.tensor(lab, device=dev)
    state = F.calibration_stats(prob, size, lt, opts, probs=True, scale=0.5)
    again = F.calibration_stats(prob, size, lt, opts, probs=True, scale=0.5, state=state)
    assert all(a is b for a, b in zip(state, again))
    want = R.stats([_nhwc(prob * 0.5)], lab, B)
    assert np.array_equal(state[0].cpu().numpy(), 2 * want[0]) and np.array_equal(state[1].cpu().numpy(), 2 * want[1])


# ------------------------------------------------------------------------------------------ planted pixels and maps
def test_planted_pixels(F, dev):
    """Exact ties (the first maximum wins, conf = 1 / C on a bin edge), a logit ahead by 200 (conf == 1.0f), a true class whose
    probability underflows to 0 (the clamp: 126 ln 2, not infinity), and the labels -1, 255 and C, which are ignored."""
    L = load_sub("_lib")
    C, B = 4, 4
    logits = np.zeros((1, C, 2, 4), dtype=np.float32)
    lab = np.zeros((1, 2, 4), dtype=np.int64)
    logits[0, :, 0, 0], lab[0, 0, 0] = 1.5, 0                      # a tie, label 0: the first maximum is a hit, conf 0.25 -> bin 1
    logits[0, :, 0, 1], lab[0, 0, 1] = -7.0, 2                     # a tie, label 2: a miss
    logits[0, 2, 0, 2], lab[0, 0, 2] = 200.0, 2                    # sure and right: bin 3, q = 2^24
    logits[0, 1, 0, 3], lab[0, 0, 3] = 200.0, 3                    # sure and wrong, p[3] = exp(-200) = 0 in fp32: the clamp
    logits[0, :, 1, 0], lab[0, 1, 0] = (0.0, 1.0, 1.0, 0.5), 2     # two equal maxima: class 1 wins, label 2: a miss
    lab[0, 1, 1], lab[0, 1, 2], lab[0, 1, 3] = -1, 255, C          # ignored, whatever the logits
    logits[0, 0, 1, 1:] = 200.0
    opts = F.CalibrationOptions(bins=B)
    bn, cl, sm = raw_logits(F, L, logits, (2, 4), lab, opts, dev)
    probs = oracle_probs(F, torch.tensor(logits, device=dev), (2, 4), [1.0])[0]
    check("planted", (bn, cl, sm), R.stats([probs], lab, B))
    # and by hand: five counted pixels
    two_maxima = probs[0, 1, 0]                                    # softmax(0, 1, 1, 0.5): conf = 0.336 -> bin 1, predicted class 1
    assert two_maxima[1] == two_maxima[2] and R.bin_of(two_maxima[1], B) == 1
    q_two = int(R.q24_of(two_maxima[1]))
    assert bn[0, 0].tolist() == [0, 0, 0] and bn[0, 1].tolist() == [3, 1, 2 * (Q // 4) + q_two] and bn[0, 2].tolist() == [0, 0, 0]
    assert bn[0, 3].tolist() == [2, 1, 2 * Q]
    assert cl[0, 0].tolist() == [2, 1, 2 * (Q // 4)] and cl[0, 1].tolist() == [2, 0, Q + q_two]
    assert cl[0, 2].tolist() == [1, 1, Q] and cl[0, 3].tolist() == [0, 0, 0]
    # the NLL: two ties at ln 4, the sure hit at 0, the clamp at 126 ln 2 (not infinity), the two maxima's own term
    by_hand = 2 * math.log(4.0) + 0.0 + 126 * math.log(2.0) - math.log(float(two_maxima[2]))
    assert np.isfinite(sm).all() and abs(sm[0, 0] - by_hand) <= 1e-9 * by_hand


def test_a_map_of_sure_pixels_carries_the_q24_sums_past_32_bits(F, dev):
    """64 x 64 pixels that are all conf == 1.0f: every workgroup of 256 pixels sums exactly 2^32 in Q24."""
    L = load_sub("_lib")
    C, B, N = 4, 15, 2
    logits = np.zeros((N, C, 64, 64), dtype=np.float32)
    logits[:, 1] = 200.0
    lab = np.ones((N, 64, 64), dtype=np.int64)
    lab[1, ::2] = 3                                                # half of sample 1 is wrong: hits differ from the pixels
    n = N * 64 * 64
    for size, tag in (((64, 64), "sure, identity"), ((96, 80), "sure, resized")):
        labs = lab if size == (64, 64) else np.ones((N,) + size, dtype=np.int64)
        hits = int((labs == 1).sum())
        bn, cl, sm = raw_logits(F, L, logits, size, labs, F.CalibrationOptions(bins=B, temps=(1.0, 2.0)), dev)
        cnt = labs.size
        for t in range(2):
            assert bn[t, B - 1].tolist() == [cnt, hits, cnt * Q] and cl[t, 1].tolist() == [cnt, hits, cnt * Q], (tag, t)
            assert bn[t].sum() == cnt + hits + cnt * Q and cl[t].sum() == cnt + hits + cnt * Q
        assert cnt * Q > 1 << 32 and n * Q == 1 << 37               # a 32-bit bin would have wrapped many times over
        for t in range(2):                                          # a miss: the true class at exp(-200 / T) = 0, the clamp; brier 1 + 1
            assert abs(sm[t, 0] - (cnt - hits) * 126 * math.log(2.0)) <= 1e-9 * max(sm[t, 0], 1.0)
            assert abs(sm[t, 1] - 2.0 * (cnt - hits)) <= 1e-9 * max(sm[t, 1], 1.0)


def test_a_batch_without_a_counted_pixel_leaves_zeros(F, dev):
    L, U = load_sub("_lib"), load_sub("utils")
    logits = np.random.RandomState(3).randn(2, 4, 5, 5).astype(np.float32)
    lab = np.full((2, 9, 9), 255, dtype=np.int64)
    lab[0, :3], lab[1, 4] = -1, 4
    opts = F.CalibrationOptions(bins=5, temps=(1.0, 2.0))
    bn, cl, sm = raw_logits(F, L, logits, (9, 9), lab, opts, dev)
    assert not bn.any() and not cl.any() and not sm.any()
    s = U.calibration_scores(bn, cl, sm, opts.temps, 4, "acdc")
    assert s["counted"] == 0 and np.isnan(s["ece"]) and np.isnan(s["nll"]) and np.isnan(s["temperature"])


# ------------------------------------------------------------------------------------------ accumulation, determinism, the grid's slice 0
def test_accumulation_determinism_and_slice_zero(F, dev):
    L = load_sub("_lib")
    N, C, H, W, OH, OW, B, temps, _ = RANDOM["c5_b32_nt8"]
    logits, lab, opts, want = reference("c5_b32_nt8")
    first = raw_logits(F, L, logits, (OH, OW), lab, opts, dev)
    second = raw_logits(F, L, logits, (OH, OW), lab, opts, dev)
    for a, b in zip(first, second):                                 # the same call twice: the same bits in all three outputs
        assert a.tobytes() == b.tobytes()
    one = raw_logits(F, L, logits, (OH, OW), lab, F.CalibrationOptions(bins=B), dev)
    for a, b in zip(one, first):                                    # inv_temps = [1.0] is slice 0 of the grid's call, bit for bit
        assert a[0].tobytes() == b[0].tobytes()
    # two calls into one state = the sum of two fresh states: the integers exactly, and the fp64 sums too - the finish adds the call's
    # total, formed in a fixed order, to what the state held: (0 + a) + b on the device is a + b on the host
    other = (np.random.RandomState(9).randn(N, C, H, W) * 2).astype(np.float32)
    fresh = raw_logits(F, L, other, (OH, OW), lab, opts, dev)
    lt = torch.tensor(lab, device=dev)
    state = F.calibration_stats(torch.tensor(logits, device=dev), (OH, OW), lt, opts)
    assert all(np.array_equal(s.cpu().numpy(), f) for s, f in zip(state, first))
    state = F.calibration_stats(torch.tensor(other, device=dev), (OH, OW), lt, opts, state=state)
    assert np.array_equal(state[0].cpu().numpy(), first[0] + fresh[0]) and np.array_equal(state[1].cpu().numpy(), first[1] + fresh[1])
    assert state[2].cpu().numpy().tobytes() == (first[2] + fresh[2]).tobytes()


def test_guards_and_refusals_on_the_device(F, dev):
    """A workspace one byte short is refused and nothing is written; the wrapper refuses what does not fit.  (The argument errors are
    checked one by one, without a device, in tests/test_calibration_host.py.)"""
    L = load_sub("_lib")
    N, C, H, W, OH, OW, B, temps, _ = RANDOM["c21_ragged_small"]
    logits, lab, opts, _ = reference("c21_ragged_small")
    x = F.to_nhwc(torch.tensor(logits, device=dev))
    rc, bn, cl, sm = raw(L, x, 0, 1.0, (N, H, W, C, OH, OW), lab, opts.inv_temps, B, dev, ws_short=1)
    assert rc == -3 and not bn.any() and not cl.any() and not sm.any()                      # SSCG_ERR_WORKSPACE, no launch
    rc, bn, cl, sm = raw(L, x, 1, 1.0, (N, H, W, C, OH, OW), lab, opts.inv_temps, B, dev)
    assert rc == -1 and not bn.any()                                                        # scores must have the output size
    lt = torch.tensor(lab, device=dev)
    xt = torch.tensor(logits, device=dev)
    with pytest.raises(L.SscgError):
        F.calibration_stats(xt, (OH, OW + 1), lt, opts)                                     # label_true does not cover the output
    with pytest.raises(L.SscgError):
        F.calibration_stats(xt, (OH, OW), lt, opts, probs=True)                             # scores at another size
    with pytest.raises(ValueError):
        F.calibration_stats(xt, (H, W), lt[:, :H, :W], F.CalibrationOptions(temps=(1.0, 2.0)), probs=True)
    with pytest.raises(L.SscgError):
        F.calibration_stats(xt, (OH, OW), lt, opts, state=F.calibration_stats(xt, (OH, OW), lt, F.CalibrationOptions(bins=B + 1)))
    with pytest.raises(L.SscgError):
        F.calibration_stats(xt.requires_grad_(), (OH, OW), lt, opts)


# ------------------------------------------------------------------------------------------ the score keeper
def _same_scores(got, want, exact=False):
    assert set(got) == set(want), set(got) ^ set(want)
    same = lambda a, b: a == b or (np.isnan(a) and np.isnan(b))
    close = lambda a, b: same(a, b) or (not exact and abs(a - b) <= 1e-9 * abs(b))
    for key in ("counted", "ece", "mce", "accuracy", "confidence"):                         # from integers alone: exact
        assert same(got[key], want[key]), (key, got[key], want[key])
    assert all(same(got["class_gap"][c], want["class_gap"][c]) for c in want["class_gap"]) and len(got["class_gap"]) == len(want["class_gap"])
    assert len(got["bins"]) == len(want["bins"]) and all(all(same(a, b) for a, b in zip(r, w)) for r, w in zip(got["bins"], want["bins"]))
    assert all(all(same(a, b) for a, b in zip(r, w)) for r, w in zip(got["above"], want["above"]))
    for key in ("nll", "brier"):
        assert close(got[key], want[key]), (key, got[key], want[key])
    if "temperature" in want:
        assert got["temperature_at_edge"] == want["temperature_at_edge"] and abs(got["temperature"] - want["temperature"]) <= 1e-6 * want["temperature"]
        assert all(a[0] == b[0] and close(a[1], b[1]) and same(a[2], b[2]) for a, b in zip(got["temperature_grid"], want["temperature_grid"]))


@pytest.mark.parametrize("head", ["logits", "logits_grid", "ms", "crf", "crf0", "probs", "components"])
def test_running_score_scores_what_its_head_takes_the_labels_from(F, dev, head):
    U = load_sub("utils")
    Cn, size = 4, (33, 41)
    g = torch.Generator().manual_seed(21)
    logits = (torch.randn(2, Cn, 9, 9, generator=g) * 2).to(dev)
    image = torch.randn(2, 3, size[0], size[1], generator=g).to(dev)
    lab = _labels(np.random.RandomState(21), 2, size[0], size[1], Cn)
    gt = torch.tensor(lab, device=dev)
    crf = F.CrfOptions(iterations=2 if head == "crf" else 0, radius=2, dilation=1)
    half = F.resize_flip(logits, (5, 6), True)
    opts = U.parse_calibration("bins=10,temps=0.5:3.0:7" if head == "logits_grid" else "bins=10")
    soft = F.softmax2d(F.upsample_bilinear(logits, size))
    if head in ("logits", "logits_grid", "crf0", "components"):
        update = (lambda rs: rs.update_logits_crf(gt, logits, image, size, crf)) if head == "crf0" else (lambda rs: rs.update_logits(gt, logits, size))
        probs = oracle_probs(F, logits, size, opts.inv_temps)
    elif head == "ms":
        update = lambda rs: rs.update_logits_ms(gt, [logits, half], [False, True], size)
        probs = [_nhwc(F.predict_labels_ms([logits, half], [False, True], size, want_prob=True)[3] * 0.5)]
    elif head == "crf":
        update = lambda rs: rs.update_logits_crf(gt, logits, image, size, crf)
        probs = [_nhwc(F.crf_labels(logits, image, size, crf, want_q=True)[3])]
    else:
        idx = F.argmax_index(soft)

        def update(rs):
            rs.update_probs(gt, soft)
            rs.update_device(gt, idx)
        probs = [_nhwc(soft)]
    off, on = U.runningScore(Cn, "acdc"), U.runningScore(Cn, "acdc")
    on.set_calibration(opts)
    if head == "components":                                        # the filter changes label maps, not probabilities
        for rs in (off, on):
            rs.set_components(U.parse_components("min_area=30"))
    for rs in (off, on):
        update(rs)
        update(rs)
    assert off._calibration_state is None and off.get_calibration_scores() is None
    assert torch.equal(on._device_hist, off._device_hist)           # the confusion matrix: bitwise the one without
    bn, cl, sm = R.stats(probs, lab, opts.bins)
    want = U.calibration_scores(2 * bn, 2 * cl, sm + sm, opts.temps, Cn, "acdc")
    got = on.get_calibration_scores()
    _same_scores(got, want)
    assert got["counted"] == 2 * int(((lab >= 0) & (lab < Cn)).sum()) and np.isfinite(got["ece"]) and ("temperature" in got) == (head == "logits_grid")
    assert on.get_scores()[0]["Mean IoU : \t"] == off.get_scores()[0]["Mean IoU : \t"]
    on.reset()
    assert on._calibration_state is None and on.get_calibration() == opts and on.get_calibration_scores()["counted"] == 0
    if head == "logits_grid":                                       # the other heads have no logits to rescale: refused, whenever asked
        with pytest.raises(ValueError):
            on.update_logits_ms(gt, [logits, half], [False, True], size)
        with pytest.raises(ValueError):
            on.update_logits_crf(gt, logits, image, size, F.CrfOptions(iterations=1, radius=1, dilation=1))


# ------------------------------------------------------------------------------------------ end to end
class _Counting(object):
    """A call counter on the binding: every entry point of libsscg.so that functional.py calls, by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return call


def _model(dev, tmp_path):
    FX = __import__("oracle.fixtures", fromlist=["x"])
    md = load_sub("model")
    args = FX.make_args(dataset="acdc", crop_height=64, crop_width=64, batch_size=2, gpu_ids=[dev.index or 0], ngf=8,
                        model="supervised_model", checkpoint_dir=str(tmp_path / "ckpt"), as_written=True)
    torch.manual_seed(12)
    with contextlib.redirect_stdout(io.StringIO()):
        m = md.supervised_model(args)                # Gsi = define_Gen(3, 4, 8, 'deeplab', ...)
    g = torch.Generator().manual_seed(13)
    batches = []
    for k in range(2):
        gt = torch.randint(0, 4, (2, 1, 64, 64), generator=g)
        gt[:, :, :2], gt[:, :, :, -3:] = 255, 255                   # a void band
        batches.append((torch.randn(2, 3, 64, 64, generator=g), gt, ["a", "b"]))
    return m, batches


def _evaluate(m, batches, **kw):
    """evaluate() -> (mIoU, the confusion matrix it was formed from, the binding's call counts)."""
    F = load_sub("functional")
    rs, seen = m.running_metrics_val, []
    inner = rs.get_scores

    def get_scores():
        out = inner()
        seen.append(rs.confusion_matrix.copy())
        return out
    rs.get_scores = get_scores
    counter = _Counting(F.lib)
    F.lib = counter
    try:
        miou, _ = m.evaluate(batches, **kw)
    finally:
        F.lib = counter._lib
        del rs.get_scores
    return miou, seen[0], counter.calls


def _expected(F, U, m, batches, dev, opts, tta=None, crf=None):
    """calibration_scores of the restatement run on the separate passes' probabilities of every batch."""
    total = None
    m.Gsi.eval()
    with torch.no_grad():
        for image, gt, _ in batches:
            image = image.to(dev)
            if crf is not None:
                scores, is_prob = U.crf_scores(m.Gsi, image, (64, 64), tta)
                probs = [_nhwc(F.crf_labels(scores, U.crf_guide(image, (64, 64)), (64, 64), crf, probs=is_prob, want_q=True)[3])]
            elif tta:
                views = U.tta_logits(m.Gsi, image, tta)
                probs = [_nhwc(F.predict_labels_ms(*views, (64, 64), want_prob=True)[3] * torch.tensor(1.0 / len(tta), dtype=torch.float32, device=dev))]
            else:
                probs = oracle_probs(F, m.Gsi(image), (64, 64), opts.inv_temps)
            part = R.stats(probs, gt.squeeze(1).numpy(), opts.bins)
            total = part if total is None else tuple(a + b for a, b in zip(total, part))
    m.Gsi.train()
    return U.calibration_scores(*total, opts.temps, 4, "acdc")


def test_evaluate_with_calibration_scores_the_probabilities_it_predicts_from(F, dev, tmp_path):
    U = load_sub("utils")
    m, batches = _model(dev, tmp_path)
    m.evaluate(batches[:1])                                          # operand copies and size queries are made here, once
    miou_off, hist_off, calls_off = _evaluate(m, batches)
    assert not hasattr(m, "eval_calibration")
    assert not any(name.startswith("sscg_calib") for name in calls_off) and calls_off.get("sscg_predict_head", 0) == 2, calls_off
    opts = F.CalibrationOptions()
    m.set_calibration(opts)
    miou_on, hist_on, calls_on = _evaluate(m, batches)
    assert miou_on == miou_off and hist_on.tobytes() == hist_off.tobytes() and m.Gsi.training
    extra = {k: v - calls_off.get(k, 0) for k, v in calls_on.items() if v != calls_off.get(k, 0)}
    assert extra.pop("sscg_calib_workspace", 1) == 1                 # one size query per shape and process
    assert extra == {"sscg_calib_stats": 2, "sscg_fill": 1} and set(calls_off) <= set(calls_on), (calls_off, calls_on)
    plain = dict(m.eval_calibration)
    _same_scores(plain, _expected(F, U, m, batches, dev, opts))
    assert plain["counted"] == sum(int((gt != 255).sum()) for _, gt, _ in batches) and 0.0 <= plain["ece"] <= plain["mce"] <= 1.0
    # a temperature grid: the same scores at T = 1, and a fitted temperature
    grid = U.parse_calibration("fit")
    m.set_calibration(grid)
    miou_grid, hist_grid, _ = _evaluate(m, batches)
    assert miou_grid == miou_off and hist_grid.tobytes() == hist_off.tobytes()
    fitted = dict(m.eval_calibration)
    _same_scores(fitted, _expected(F, U, m, batches, dev, grid))
    _same_scores({k: fitted[k] for k in plain}, plain, exact=True)
    assert len(fitted["temperature_grid"]) == 8 and 0.5 <= fitted["temperature"] <= 3.0
    # a grid does not combine with several views, the CRF or the chain of separate passes: refused before the first batch
    tta, crf = U.parse_tta("0.75,1.0"), F.CrfOptions(iterations=2, radius=2, dilation=1)
    for kw in ({"tta": tta}, {"crf": crf}):
        with pytest.raises(ValueError):
            m.evaluate(iter(()), **kw)
        with pytest.raises(ValueError):
            m.set_calibration(grid, **kw)
    # temperature 1 alone does: under tta=, crf= and both, the scores of what the labels are taken from; mIoU and matrix as without
    m.set_calibration(opts)
    for kw in ({"tta": tta}, {"crf": crf}, {"tta": tta, "crf": crf}):
        m.set_calibration(None)
        miou_0, hist_0, _ = _evaluate(m, batches, **kw)
        assert not hasattr(m, "eval_calibration")
        m.set_calibration(opts)
        miou_1, hist_1, _ = _evaluate(m, batches, **kw)
        assert miou_1 == miou_0 and hist_1.tobytes() == hist_0.tobytes(), sorted(kw)
        _same_scores(dict(m.eval_calibration), _expected(F, U, m, batches, dev, opts, **kw))
    # SSCG_FUSE_PREDICT=0: the softmax map of the separate passes is scored - the same probabilities, the same scores
    fuse = F.FUSE_PREDICT[0]
    try:
        F.FUSE_PREDICT[0] = False
        miou_sep, hist_sep, calls_sep = _evaluate(m, batches)
        assert miou_sep == miou_off and hist_sep.tobytes() == hist_off.tobytes() and calls_sep["sscg_calib_stats"] == 2
        _same_scores(dict(m.eval_calibration), plain, exact=True)
        with pytest.raises(ValueError):
            m.set_calibration(grid)
    finally:
        F.FUSE_PREDICT[0] = fuse
    # switched off again, the attribute goes and nothing of it is launched
    m.set_calibration(None)
    miou_end, hist_end, calls_end = _evaluate(m, batches)
    assert not hasattr(m, "eval_calibration") and miou_end == miou_off and hist_end.tobytes() == hist_off.tobytes() and calls_end == calls_off
