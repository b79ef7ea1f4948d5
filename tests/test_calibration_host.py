"""Calibration scores of the evaluation (sscg_calib_stats, `--calibration`) on a GPU-less host: the spec parser, the scores formed
from hand-made counts (utils.calibration_scores), the numpy restatement's bin and Q24 rules on planted confidences
(tests/calibration_reference.py, the pin of tests/test_calibration_gpu.py), the argument checks of the entry, the command line and
the score keeper's option state.  Nothing here launches a kernel."""
import ctypes as C
import inspect
import math
import os
import sys

import numpy as np
import pytest
import torch

import calibration_reference as R
from conftest import ROOT, load_sub

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
ONE = C.c_void_p(16)                      # a non-null pointer that is never dereferenced
Q = 1 << 24


# ------------------------------------------------------------------------------------------ the spec
def test_parse_calibration_table():
    F, U = load_sub("functional"), load_sub("utils")
    assert U.parse_calibration("") is None and U.parse_calibration(None) is None and U.parse_calibration("  ") is None
    on = U.parse_calibration("on")
    assert on == F.CalibrationOptions() and on.bins == 15 and on.temps == (1.0,) and U.parse_calibration(" on ") == on
    fit = U.parse_calibration("fit")
    assert fit == U.parse_calibration("bins=15,temps=0.5:3.0:7") and fit.bins == 15 and len(fit.temps) == 8
    assert fit.temps[0] == 1.0 and fit.temps[1] == 0.5 and fit.temps[-1] == 3.0
    ratios = [fit.temps[k + 1] / fit.temps[k] for k in range(1, 7)]
    assert max(ratios) / min(ratios) < 1 + 1e-12 and abs(ratios[0] - 6.0 ** (1.0 / 6.0)) < 1e-12            # log-spaced
    assert U.parse_calibration("bins=10") == F.CalibrationOptions(bins=10)
    assert U.parse_calibration("temps=0.5/2") == F.CalibrationOptions(temps=(0.5, 2.0)) and U.parse_calibration("temps=2").temps == (1.0, 2.0)
    assert U.parse_calibration("temps=1/2/4, bins=32") == F.CalibrationOptions(bins=32, temps=(1.0, 2.0, 4.0))      # 1.0 is not doubled
    assert U.parse_calibration("temps=0.5:2:3").temps == (1.0, 0.5, 2.0)                # the grid's own 1.0 is the leading one
    for spec, token in (("bins=1", "bins=1"), ("bins=33", "bins=33"), ("temps=0.5:3:8", "temps=0.5:3:8"), ("temps=0:1:3", "temps=0:1:3"),
                        ("temps=.2/.3/.4/.5/.6/.7/.8/.9", "temps="), ("bins=x", "bins=x"), ("zap", "zap"), ("bins=4,bins=5", "bins=5"),
                        ("temps=-1", "temps=-1"), ("temps=a/b", "temps=a/b"), ("temps=3:1:4", "temps=3:1:4"), ("temps=1:2", "temps=1:2"),
                        ("temps=2/2", "temps=2/2"), ("temps=inf", "temps=inf")):
        with pytest.raises(ValueError) as e:
            U.parse_calibration(spec)
        assert token in str(e.value) and "--calibration" in str(e.value), (spec, str(e.value))


def test_calibration_options():
    F = load_sub("functional")
    o = F.CalibrationOptions()
    assert (o.bins, o.temps) == (15, (1.0,)) and o.inv_temps == [1.0]
    g = F.CalibrationOptions(bins=4, temps=(2.0, 0.75))
    assert g.temps == (1.0, 2.0, 0.75) and g.inv_temps == [1.0, 0.5, float(np.float32(1) / np.float32(0.75))]
    assert g == F.CalibrationOptions(4, [1, 2, 0.75]) and g != o and hash(g) == hash(F.CalibrationOptions(4, (1.0, 2.0, 0.75)))
    assert len({o, F.CalibrationOptions(15), g}) == 2 and "bins=4" in repr(g)
    for bad in ({"bins": 1}, {"bins": 33}, {"bins": 15.0}, {"bins": True}, {"temps": (0.0,)}, {"temps": (float("nan"),)},
                {"temps": (float("inf"),)}, {"temps": ("2",)}, {"temps": (1e-60,)}, {"temps": tuple(range(2, 10))}, {"temps": (2.0, 2.0)}):
        with pytest.raises(ValueError):
            F.CalibrationOptions(**bad)
    assert len(F.CalibrationOptions(temps=tuple(range(2, 9))).temps) == 8


# ------------------------------------------------------------------------------------------ the scores of hand-made counts
def _tables(rows, C_=3, cls=None):
    """bins [1, B, 3] from (n, hits, mean confidence as a multiple of 2^-24) rows, with a matching one-class cls table and zero sums."""
    bins = np.array([[(n, h, q) for n, h, q in rows]], dtype=np.int64)
    if cls is None:
        cls = np.zeros((1, C_, 3), dtype=np.int64)
        cls[0, 0] = bins[0].sum(axis=0)
    return bins, cls, np.zeros((1, 2))


def test_a_perfectly_calibrated_table_has_no_error():
    U = load_sub("utils")
    # four bins: the accuracy of every bin is exactly its mean confidence (1/8, 3/8, 5/8, 7/8)
    rows = [(8, 1, 8 * Q // 8), (16, 6, 16 * 3 * Q // 8), (8, 5, 8 * 5 * Q // 8), (32, 28, 32 * 7 * Q // 8)]
    s = U.calibration_scores(*_tables(rows), (1.0,), 3, "acdc")
    assert s["ece"] == 0.0 and s["mce"] == 0.0 and s["counted"] == 64
    assert s["accuracy"] == 40 / 64 and s["confidence"] == (1 + 6 + 5 + 28) / 64 and s["class_gap"][0] == 0.0
    assert np.isnan(s["class_gap"][1]) and np.isnan(s["class_gap"][2])              # never predicted
    assert "temperature" not in s and "temperature_grid" not in s
    assert s["bins"][1] == (0.25, 0.5, 16, 6 / 16, 3 / 8)


def test_a_two_bin_table_by_hand():
    U = load_sub("utils")
    # bin 0: 10 pixels, 2 hits, mean confidence 0.25 -> gap 0.05; bin 1: 30 pixels, 27 hits, mean confidence 0.75 -> gap 0.15
    bins = np.array([[(10, 2, 10 * Q // 4), (30, 27, 30 * 3 * Q // 4)]], dtype=np.int64)
    # predicted class 0: 20 pixels, 18 hits, mean confidence 0.75; class 1: 20 pixels, 11 hits, mean confidence 0.5; class 2: never
    cls = np.array([[(20, 18, 20 * 3 * Q // 4), (20, 11, 20 * Q // 2), (0, 0, 0)]], dtype=np.int64)
    sums = np.array([[20.0, 10.0]])
    s = U.calibration_scores(bins, cls, sums, (1.0,), 3, "acdc")
    assert abs(s["ece"] - (10 / 40 * 0.05 + 30 / 40 * 0.15)) < 1e-15 and abs(s["ece"] - 0.125) < 1e-15
    assert abs(s["mce"] - 0.15) < 1e-15 and s["nll"] == 0.5 and s["brier"] == 0.25 and s["counted"] == 40
    assert s["accuracy"] == 29 / 40 and s["confidence"] == (2.5 + 22.5) / 40
    assert abs(s["class_gap"][0] - (0.75 - 0.9)) < 1e-15 and abs(s["class_gap"][1] - (0.5 - 0.55)) < 1e-15 and np.isnan(s["class_gap"][2])
    assert (s["ece"], s["mce"]) == pytest.approx(R.ece_by_hand(bins[0]), abs=1e-15)
    # the threshold table: everything at or above 0, the upper bin at or above 0.5
    assert s["above"] == [(0.0, 1.0, 29 / 40), (0.5, 0.75, 0.9)]
    # VOC drops class 0, Cityscapes the last class
    assert set(U.calibration_scores(bins, cls, sums, (1.0,), 3, "voc2012")["class_gap"]) == {0, 1}
    v = U.calibration_scores(bins, cls, sums, (1.0,), 3, "voc2012")["class_gap"]
    assert abs(v[0] - (0.5 - 0.55)) < 1e-15 and np.isnan(v[1])
    with pytest.raises(ValueError):
        U.calibration_scores(bins, cls[:, :2], sums, (1.0,), 3, "acdc")
    with pytest.raises(ValueError):
        U.calibration_scores(bins, cls, sums, (1.0, 2.0), 3, "acdc")


def test_above_is_monotone_in_coverage():
    U = load_sub("utils")
    rng = np.random.RandomState(0)
    n = rng.randint(0, 50, size=15)
    n[3] = n[9] = 0
    rows = [(int(k), int(rng.randint(0, k + 1)), int(k) * Q // 2) for k in n]
    s = U.calibration_scores(*_tables(rows), (1.0,), 3, "acdc")
    cov = [c for _, c, _ in s["above"]]
    assert len(cov) == 15 and cov[0] == 1.0 and all(a >= b for a, b in zip(cov, cov[1:])) and cov[-1] == n[-1] / n.sum()
    assert [e for e, _, _ in s["above"]] == [b / 15 for b in range(15)]
    tail_hits = sum(r[1] for r in rows[10:])
    assert s["above"][10][2] == tail_hits / n[10:].sum()


def test_empty_counts_give_nans_and_no_exception():
    U = load_sub("utils")
    z = (np.zeros((2, 5, 3), dtype=np.int64), np.zeros((2, 4, 3), dtype=np.int64), np.zeros((2, 2)))
    s = U.calibration_scores(*z, (1.0, 2.0), 4, "acdc")
    assert s["counted"] == 0
    for key in ("ece", "mce", "nll", "brier", "accuracy", "confidence", "temperature"):
        assert np.isnan(s[key]), key
    assert all(np.isnan(v) for v in s["class_gap"].values()) and len(s["class_gap"]) == 4
    assert all(np.isnan(c) and np.isnan(a) for _, c, a in s["above"]) and all(r[2] == 0 and np.isnan(r[3]) for r in s["bins"])
    assert s["temperature_at_edge"] is False and len(s["temperature_grid"]) == 2


def _grid_state(temps, nll_of):
    nt = len(temps)
    bins = np.zeros((nt, 4, 3), dtype=np.int64)
    bins[:, 3] = (100, 90, 100 * 7 * Q // 8)
    cls = np.zeros((nt, 3, 3), dtype=np.int64)
    cls[:, 1] = bins[:, 3]
    sums = np.array([[100.0 * nll_of(t), 1.0] for t in temps])
    return bins, cls, sums


def test_the_fitted_temperature_is_the_vertex_of_an_exact_parabola_in_log_t():
    U = load_sub("utils")
    best = 1.7
    nll = lambda t: 0.25 + 3.0 * (math.log(t) - math.log(best)) ** 2
    temps = (1.0, 0.5, 0.8, 1.3, 2.2, 3.0)                              # 1.0 in front, the rest in any order
    s = U.calibration_scores(*_grid_state(temps, nll), temps, 3, "acdc")
    assert abs(s["temperature"] - best) < 1e-9 and s["temperature_at_edge"] is False
    assert [g[0] for g in s["temperature_grid"]] == sorted(temps)
    assert all(abs(g[1] - nll(g[0])) < 1e-12 for g in s["temperature_grid"]) and abs(s["nll"] - nll(1.0)) < 1e-12
    assert all(abs(g[2] - (0.9 - 0.875)) < 1e-15 for g in s["temperature_grid"])


def test_the_edge_flag_is_set_at_either_end_of_the_grid():
    U = load_sub("utils")
    temps = (1.0, 2.0, 3.0)
    rising = U.calibration_scores(*_grid_state(temps, lambda t: t), temps, 3, "acdc")
    assert rising["temperature"] == 1.0 and rising["temperature_at_edge"] is True
    falling = U.calibration_scores(*_grid_state(temps, lambda t: -t), temps, 3, "acdc")
    assert falling["temperature"] == 3.0 and falling["temperature_at_edge"] is True
    inner = U.calibration_scores(*_grid_state(temps, lambda t: (t - 2.1) ** 2), temps, 3, "acdc")
    assert inner["temperature_at_edge"] is False and 1.0 < inner["temperature"] < 3.0


# ------------------------------------------------------------------------------------------ the restatement's own rules
def test_reference_bin_and_q24_rules_on_planted_confidences():
    assert R.bin_of(np.float32(1.0), 15) == 14 and R.bin_of(np.float32(1.0), 2) == 1 and R.q24_of(np.float32(1.0)) == Q
    assert R.bin_of(np.float32(0.25), 4) == 1 and R.q24_of(np.float32(0.25)) == Q // 4            # an edge opens its bin
    assert R.bin_of(np.float32(0.2), 15) == 3                       # fp32(0.2) * 15 rounds to 3.0 in fp32 (in fp64 it stays above)
    assert float(np.float32(0.2)) * 15 > 3.0 and np.float32(0.2) * np.float32(15) == np.float32(3.0)
    below = np.nextafter(np.float32(0.25), np.float32(0))
    assert R.bin_of(below, 4) == 0 and R.q24_of(below) == Q // 4 - 1                              # truncation, not rounding
    assert R.bin_of(np.float32(0.0), 32) == 0 and R.q24_of(np.float32(0.0)) == 0
    assert R.bin_of(np.float32(1.0000001), 15) == 14                                              # a sum of views a hair above 1


def test_reference_counts_a_small_map_by_hand():
    p = np.array([[0.5, 0.5, 0.0, 0.0],            # a tie: the first maximum, class 0; label 1 -> a miss
                  [0.0, 0.0, 1.0, 0.0],            # sure and right
                  [1.0, 0.0, 0.0, 0.0],            # sure and wrong, the true class at 0: the clamp
                  [0.25, 0.25, 0.25, 0.25],        # ignored: label 255
                  [0.1, 0.2, 0.3, 0.4]], dtype=np.float32)       # label -1: ignored
    lab = np.array([1, 2, 3, 255, -1])
    bins, cls, sums = R.stats_one(p, lab, 4)
    assert bins.tolist() == [[0, 0, 0], [0, 0, 0], [1, 0, Q // 2], [2, 1, 2 * Q]]
    assert cls.tolist() == [[2, 0, Q // 2 + Q], [0, 0, 0], [1, 1, Q], [0, 0, 0]]
    assert abs(sums[0] - (math.log(2) + 0.0 + 126 * math.log(2))) < 1e-12 and abs(sums[1] - (0.5 + 0.0 + 2.0)) < 1e-15
    none = R.stats_one(p, np.full(5, 4), 4)
    assert not none[0].any() and not none[1].any() and not none[2].any()
    b3, c3, s3 = R.stats([p, p], lab, 4)
    assert b3.shape == (2, 4, 3) and c3.shape == (2, 4, 3) and s3.shape == (2, 2) and (b3[1] == bins).all()


# ------------------------------------------------------------------------------------------ the entries, the wrapper, the drivers
def test_entries_are_exported_declared_and_bound():
    L = load_sub("_lib")
    hdr = open(os.path.join(ROOT, "include", "sscg.h")).read()
    assert "size_t sscg_calib_workspace(int N, int OH, int OW, int NT);" in hdr
    assert "int sscg_calib_stats(const float* x, int kind, float scale, int N, int H, int W, int C, int OH, int OW," in hdr
    block = hdr[hdr.index("calibration scores of the evaluation"):hdr.index("size_t sscg_calib_workspace(")]
    for word in ("Q24", "0x1p-126", "AFTER the resize", "min(B - 1, (int)(conf * (float)B))", "ACCUMULATED"):
        assert word in block, word
    assert len(L.SIGNATURES["sscg_calib_stats"][1]) == 19 and len(L.SIGNATURES["sscg_calib_workspace"][1]) == 4
    assert callable(L.lib.sscg_calib_stats) and callable(L.lib.sscg_calib_workspace)
    assert L.ABI_VERSION == 18 and L.lib.sscg_abi_version() == 18 and "#define SSCG_ABI_VERSION 18" in hdr          # an addition
    assert "calib.hip" in open(os.path.join(ROOT, "semi-supervised-segmentation-cyclegan_amd", "csrc", "Makefile")).read()


def test_workspace_size_follows_the_documented_formula():
    lib = load_sub("_lib").lib
    for (N, OH, OW, NT) in ((1, 1, 1, 1), (2, 19, 23, 1), (3, 129, 129, 8), (8, 256, 256, 8), (2, 257, 257, 3), (1, 32768, 65535, 1)):
        want = min(-(-(N * OH * OW) // 256), 512) * NT * 2 * 8
        assert lib.sscg_calib_workspace(N, OH, OW, NT) == want, (N, OH, OW, NT)
    assert lib.sscg_calib_workspace(0, 5, 5, 1) == 0 and lib.sscg_calib_workspace(1, 5, 5, 0) == 0 and lib.sscg_calib_workspace(1, 5, 5, 9) == 0
    assert lib.sscg_calib_workspace(2, 32768, 32768, 1) == 0


def test_argument_errors_are_returned_before_any_launch():
    lib = load_sub("_lib").lib

    def call(x=ONE, kind=0, scale=1.0, N=1, H=5, W=5, Cn=4, OH=9, OW=9, lt=ONE, temps=(1.0,), NT=None, B=15, bins=ONE, cls=ONE,
             sums=ONE, ws=ONE, ws_bytes=1 << 40):
        its = None if temps is None else (C.c_float * len(temps))(*temps)
        return lib.sscg_calib_stats(x, kind, scale, N, H, W, Cn, OH, OW, lt, its, len(temps) if NT is None else NT, B, bins, cls, sums,
                                    ws, ws_bytes, None)

    for ptr in ("x", "lt", "bins", "cls", "sums"):
        assert call(**{ptr: None}) == BAD_ARG, ptr
    assert call(temps=None, NT=1) == BAD_ARG
    for size in ("N", "H", "W", "OH", "OW"):
        assert call(**{size: 0}) == BAD_ARG and call(**{size: -3}) == BAD_ARG, size
    assert call(Cn=0) == BAD_ARG and call(Cn=65) == BAD_ARG
    assert call(B=1) == BAD_ARG and call(B=33) == BAD_ARG and call(B=2, ws=None) == WORKSPACE and call(B=32, ws=None) == WORKSPACE
    assert call(NT=0) == BAD_ARG and call(temps=(1.0,) * 9) == BAD_ARG and call(temps=(1.0,) * 8, ws=None) == WORKSPACE
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(temps=(1.0, bad)) == BAD_ARG, bad
    assert call(kind=2) == BAD_ARG and call(kind=-1) == BAD_ARG
    ident = dict(kind=1, H=9, W=9)
    assert call(ws=None, **ident) == WORKSPACE                                      # accepted up to the workspace
    assert call(kind=1, H=5, W=9) == BAD_ARG and call(kind=1, H=9, W=5) == BAD_ARG
    assert call(temps=(1.0, 1.0), **ident) == BAD_ARG and call(temps=(0.5,), **ident) == BAD_ARG
    assert call(N=2, H=9, W=9, OH=32768, OW=32768) == UNSUPPORTED and call(N=1 << 30, OH=1 << 30, OW=1 << 30) == UNSUPPORTED
    assert call(N=2, H=32768, W=32768, B=1) == BAD_ARG                              # the argument errors come first
    need = lib.sscg_calib_workspace(1, 9, 9, 1)
    assert need == 16 and call(ws_bytes=need - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE


def test_wrapper_refuses_cpu_tensors_and_the_drivers_take_the_option():
    F, L, U, md = load_sub("functional"), load_sub("_lib"), load_sub("utils"), load_sub("model")
    x, lt = torch.zeros(1, 4, 5, 5), torch.zeros(1, 9, 9, dtype=torch.int64)
    with pytest.raises(L.SscgError):
        F.calibration_stats(x, (9, 9), lt, F.CalibrationOptions())
    with pytest.raises(TypeError):
        F.calibration_stats(x, (9, 9), lt, (15, (1.0,)))
    assert list(inspect.signature(F.calibration_stats).parameters) == ["x", "size", "label_true", "options", "probs", "scale", "state"]
    for cls in (md.semisuper_cycleGAN, md.supervised_model):
        assert list(inspect.signature(cls.evaluate).parameters) == ["self", "val_loader", "first_batch", "tta", "crf", "boundary"]
        assert callable(cls.set_calibration) and list(inspect.signature(cls.set_calibration).parameters)[:2] == ["self", "opts"]
        assert callable(cls._calibration_scores)
    for name in ("set_calibration", "get_calibration", "get_calibration_scores", "update_probs"):
        assert callable(getattr(U.runningScore, name)), name


def test_running_score_holds_the_option_as_state_and_refuses_what_cannot_be_scored():
    F, U = load_sub("functional"), load_sub("utils")
    rs = U.runningScore(4, "acdc")
    assert rs.get_calibration() is None and rs.get_calibration_scores() is None
    opts = F.CalibrationOptions(bins=10)
    rs.set_calibration(opts)
    assert rs.get_calibration() == opts
    s = rs.get_calibration_scores()                              # nothing scored yet
    assert s["counted"] == 0 and np.isnan(s["ece"]) and len(s["bins"]) == 10 and "temperature" not in s
    rs.reset()
    assert rs.get_calibration() == opts                          # reset() clears the counts, not the option
    for bad in (3, "on", (15, (1.0,)), F.SurfaceOptions()):
        with pytest.raises(TypeError):
            rs.set_calibration(bad)
    grid = U.parse_calibration("fit")
    tta, crf = U.parse_tta("0.5,1.0:flip"), F.CrfOptions()
    for kw in ({"tta": tta}, {"crf": crf}, {"tta": tta, "crf": crf}):
        with pytest.raises(ValueError):
            rs.set_calibration(grid, **kw)
        rs.set_calibration(opts, **kw)                           # temperature 1 alone combines with both
    assert rs.get_calibration() == opts                          # a refused option is not set
    rs.set_calibration(grid)
    assert "temperature" in rs.get_calibration_scores()
    with pytest.raises(ValueError):
        rs.check_calibration(tta=tta)                            # what evaluate() asks before its first batch
    with pytest.raises(ValueError):
        rs.check_calibration(crf=crf)
    rs.check_calibration()
    fuse = F.FUSE_PREDICT[0]
    try:
        F.FUSE_PREDICT[0] = False                                # the chain of separate passes has no logits to rescale either
        with pytest.raises(ValueError):
            rs.check_calibration()
        with pytest.raises(ValueError):
            U.runningScore(4, "acdc").set_calibration(grid)
        U.runningScore(4, "acdc").set_calibration(opts)
    finally:
        F.FUSE_PREDICT[0] = fuse
    rs.set_calibration(None)
    assert rs.get_calibration() is None and rs.get_calibration_scores() is None and rs.get_surface() is None
    rs.update([np.array([[0, 1], [2, 255]])], [np.array([[0, 1], [1, 3]])])        # the host path is as it was
    assert rs.confusion_matrix.sum() == 3


def test_main_takes_calibration_and_moves_no_other_default():
    sys.path.insert(0, ROOT)
    import main
    a = main.get_args([])
    assert a.calibration == "" and "calibration" not in vars(a)         # an absent flag leaves the namespace as it always was
    b = main.get_args(["--calibration", "fit"])
    assert b.calibration == "fit" and set(vars(b)) - set(vars(a)) == {"calibration"}
    rest = dict(vars(b))
    del rest["calibration"]
    assert rest == vars(a)
    assert main.get_args(["--calibration", "on"]).calibration == "on"
    assert main.get_args(["--calibration", "bins=20,temps=0.5/2"]).calibration == "bins=20,temps=0.5/2"
    old = ["--dataset", "acdc", "--tta", "0.5,1.0:flip", "--crf", "on", "--boundary", "on", "--surface", "on", "--batch_size", "4"]
    assert vars(main.get_args(old + ["--calibration", "on"])).items() >= vars(main.get_args(old)).items()
    for bad in ("zap", "bins=1", "bins=33", "temps=0:1:3", "temps=.2/.3/.4/.5/.6/.7/.8/.9", "bins=x"):
        with pytest.raises(SystemExit):
            main.get_args(["--calibration", bad])
    for combo in (["--tta", "0.5,1.0"], ["--crf", "on"]):               # a grid with --tta / --crf exits at parse time too
        with pytest.raises(SystemExit):
            main.get_args(combo + ["--calibration", "fit"])
    text = open(os.path.join(ROOT, "main.py")).read()
    assert "--calibration" in text[:text.index("import importlib")] and "untuned" in text[text.index('"--calibration"'):][:1500]
