"""Class-weighted, label-smoothed cross entropy (sscg_ce_fwd_w / sscg_ce_bwd_w / sscg_upsample_head_fwd_w / sscg_label_hist) on a
GPU-less host: the four entries are declared, exported and bound, the C entries return every argument error before any HIP call, the
weight-spec parser, the two frequency rules and the driver flags behave as documented, and a model built with the defaults takes none
of the new paths."""
import ctypes as C
import math
import os
import sys
import types

import pytest
import torch

from conftest import ROOT, load_sub

BAD_ARG, WORKSPACE = -1, -3
ONE = C.c_void_p(16)          # never dereferenced
NEW = ("sscg_ce_fwd_w", "sscg_ce_bwd_w", "sscg_upsample_head_fwd_w", "sscg_label_hist")


def test_the_four_entries_are_declared_exported_and_bound():
    import re
    import subprocess
    L = load_sub("_lib")
    hdr = open(os.path.join(ROOT, "include", "sscg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert ("int sscg_ce_fwd_w(const float* logits, const int64_t* labels, int64_t rows, int C, const float* class_w, float smoothing, "
            "float* loss,") in code
    assert "int sscg_ce_bwd_w(const float* logits, const int64_t* labels, int64_t rows, int C, const float* class_w, float smoothing," in code
    assert ("int sscg_upsample_head_fwd_w(const float* x, const int64_t* labels, const float* class_w, float smoothing, float* y_soft, "
            "float* loss,") in code
    assert "int sscg_label_hist(const int64_t* labels, int64_t n, int C, int64_t* counts, void* stream);" in code
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sscg_[a-z0-9_]+)", out))
    for name in NEW:
        assert name in exported and name in L.SIGNATURES and callable(getattr(L.lib, name)), name
    assert [len(L.SIGNATURES[n][1]) for n in NEW] == [11, 11, 17, 5]
    assert L.SIGNATURES["sscg_ce_fwd_w"][1][5] is C.c_float and L.SIGNATURES["sscg_upsample_head_fwd_w"][1][3] is C.c_float
    assert L.ABI_VERSION == 18 and L.lib.sscg_abi_version() == 18 and "#define SSCG_ABI_VERSION 18" in hdr      # additions only
    assert "It serves sscg_upsample_head_fwd_w unchanged" in hdr            # the backward is reused as it stands, and says so


def test_argument_errors_are_returned_before_any_launch():
    lib = load_sub("_lib").lib
    big = 1 << 20

    def fwd(x=ONE, lab=ONE, rows=9, Cn=4, w=ONE, eps=0.1, loss=ONE, valid=ONE, ws=ONE, wsb=big):
        return lib.sscg_ce_fwd_w(x, lab, rows, Cn, w, eps, loss, valid, ws, wsb, None)

    def bwd(x=ONE, lab=ONE, rows=9, Cn=4, w=ONE, eps=0.1, g=None, valid=ONE, dx=ONE):
        return lib.sscg_ce_bwd_w(x, lab, rows, Cn, w, eps, g, 1.0, valid, dx, None)

    def head(x=ONE, lab=ONE, w=ONE, eps=0.1, y=None, loss=ONE, valid=ONE, dl=ONE, N=1, H=3, W=3, Cn=4, OH=12, OW=12, ws=ONE, wsb=big):
        return lib.sscg_upsample_head_fwd_w(x, lab, w, eps, y, loss, valid, dl, N, H, W, Cn, OH, OW, ws, wsb, None)

    for call in (fwd, bwd, head):
        for eps in (-0.1, 1.0, 1.5, float("nan"), float("inf")):          # smoothing outside [0, 1): first of all
            assert call(eps=eps) == BAD_ARG, (call.__name__, eps)
            assert call(eps=eps, w=None) == BAD_ARG
        assert call(x=None) == BAD_ARG and call(Cn=0) == BAD_ARG and call(Cn=65) == BAD_ARG
        assert call(x=None, w=None, eps=0.0) == BAD_ARG                   # the plain entries' own rules behind the dispatch
        assert call(Cn=65, w=None, eps=0.0) == BAD_ARG
    assert fwd(lab=None) == BAD_ARG and fwd(loss=None) == BAD_ARG and fwd(rows=0) == BAD_ARG
    assert fwd(ws=None) == WORKSPACE and fwd(wsb=8) == WORKSPACE and fwd(ws=None, w=None, eps=0.0) == WORKSPACE
    assert bwd(lab=None) == BAD_ARG and bwd(dx=None) == BAD_ARG and bwd(rows=-1) == BAD_ARG
    assert head(loss=None) == BAD_ARG and head(valid=None) == BAD_ARG and head(dl=None) == BAD_ARG
    assert head(lab=None, y=None) == BAD_ARG                              # neither branch
    assert head(N=0) == BAD_ARG and head(OH=0) == BAD_ARG and head(H=-1) == BAD_ARG
    assert head(ws=None) == WORKSPACE and head(wsb=8) == WORKSPACE
    assert lib.sscg_label_hist(None, 10, 4, ONE, None) == BAD_ARG and lib.sscg_label_hist(ONE, 10, 4, None, None) == BAD_ARG
    assert lib.sscg_label_hist(ONE, -1, 4, ONE, None) == BAD_ARG
    assert lib.sscg_label_hist(ONE, 10, 0, ONE, None) == BAD_ARG and lib.sscg_label_hist(ONE, 10, 65, ONE, None) == BAD_ARG
    assert lib.sscg_label_hist(ONE, 0, 4, ONE, None) == 0                 # nothing to count: no launch


def test_parse_ce_weights():
    U = load_sub("utils")
    assert U.parse_ce_weights("", 4) is None and U.parse_ce_weights(None, 4) is None and U.parse_ce_weights("  ", 21) is None
    assert U.parse_ce_weights("1,2.5,0,1e-1", 4) == [1.0, 2.5, 0.0, 0.1]
    assert U.parse_ce_weights("3", 1) == [3.0]
    assert U.parse_ce_weights("median", 4) == ("median",)
    assert U.parse_ce_weights("invlog", 21) == ("invlog", 1.02) and U.CE_INVLOG_K == 1.02
    assert U.parse_ce_weights("invlog:1.1", 21) == ("invlog", 1.1)
    for bad, token in (("1,2,3", "1,2,3"), ("1,2,3,4,5", "1,2,3,4,5"),           # a wrong length: the whole list is named
                       ("1,-2,3,4", "-2"), ("1,nan,3,4", "nan"), ("1,2,inf,4", "inf"), ("1,2,,4", "''"),
                       ("garbage", "garbage"), ("1,two,3,4", "two"), ("median:3", "median:3"), ("invlog:abc", "abc"),
                       ("invlog:1.0", "1.0"), ("invlog:0.5", "0.5"), ("invlog:nan", "nan"), ("invlog:", "''")):
        with pytest.raises(ValueError) as e:
            U.parse_ce_weights(bad, 4)
        assert token in str(e.value), (bad, str(e.value))


def test_ce_weights_from_counts_by_hand():
    U = load_sub("utils")
    counts = [10, 30, 0, 60]                    # f = 0.1, 0.3, -, 0.6; the classes present: 0, 1, 3; their median frequency 0.3
    med = U.ce_weights_from_counts(("median",), counts)
    assert med[2] == 0.0 and med == pytest.approx([3.0, 1.0, 0.0, 0.5], rel=1e-12)
    inv = U.ce_weights_from_counts(("invlog", 1.02), counts)
    assert inv[2] == 0.0 and inv == pytest.approx([1 / math.log(1.12), 1 / math.log(1.32), 0.0, 1 / math.log(1.62)], rel=1e-12)
    inv = U.ce_weights_from_counts(U.parse_ce_weights("invlog:1.1", 4), counts)
    assert inv == pytest.approx([1 / math.log(1.2), 1 / math.log(1.4), 0.0, 1 / math.log(1.7)], rel=1e-12)
    # an even number of classes present: the median is the mean of the middle two frequencies
    assert U.ce_weights_from_counts(("median",), [1, 3, 0, 0]) == pytest.approx([0.5 / 0.25, 0.5 / 0.75, 0.0, 0.0], rel=1e-12)
    assert U.ce_weights_from_counts(("median",), torch.tensor([5, 5]).tolist()) == [1.0, 1.0]
    for bad in ([0, 0, 0, 0], [1, -1, 3, 4]):
        with pytest.raises(ValueError):
            U.ce_weights_from_counts(("median",), bad)
    with pytest.raises(ValueError):
        U.ce_weights_from_counts(("other",), counts)


def test_main_takes_both_flags_and_moves_no_default():
    sys.path.insert(0, ROOT)
    import main
    a = main.get_args([])
    assert a.ce_weights == "" and a.label_smoothing == 0.0 and isinstance(a.label_smoothing, float)
    before = dict(vars(a))
    assert "ce_weights" not in before and "label_smoothing" not in before     # a default run parses to the namespace it always did
    assert before["tta"] == "" and before["augment"] == "" and before["panels"] is None and before["lab_CE_weight"] == 1
    b = main.get_args(["--ce_weights", "median", "--label_smoothing", "0.1"])
    assert b.ce_weights == "median" and b.label_smoothing == 0.1
    rest = dict(vars(b))
    del rest["ce_weights"], rest["label_smoothing"]
    assert rest == before
    assert main.get_args(["--ce_weights", "1,2,3,4"]).ce_weights == "1,2,3,4"


def test_weight_tensor_is_checked_once_on_the_host_and_cpu_tensors_are_refused():
    F, L = load_sub("functional"), load_sub("_lib")
    w = F.ce_weight([0.5, 0, 2, 1], 4, torch.device("cpu"))
    assert w.dtype == torch.float32 and w.tolist() == [0.5, 0.0, 2.0, 1.0]
    for bad in ([1, 2, 3], [1, 2, 3, 4, 5], [1, -1, 1, 1], [1, float("nan"), 1, 1], [1, float("inf"), 1, 1]):
        with pytest.raises(ValueError):
            F.ce_weight(bad, 4, torch.device("cpu"))
    x, lab = torch.zeros(1, 4, 3, 3), torch.zeros(1, 3, 3, dtype=torch.int64)
    with pytest.raises(L.SscgError):                                      # no CPU fallback for the weighted loss either
        F.cross_entropy(x, lab, weight=w, label_smoothing=0.1)
    with pytest.raises(L.SscgError):
        F.upsample_softmax_ce(x, (12, 12), torch.zeros(1, 12, 12, dtype=torch.int64), weight=w)
    with pytest.raises(L.SscgError):
        F.label_hist(lab, 4)
    for eps in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            F._ce_options(None, eps, 4, torch.device("cpu"))
    with pytest.raises(L.SscgError):                                      # a weight tensor of the wrong length / dtype
        F._ce_options(w, 0.0, 5, torch.device("cpu"))
    with pytest.raises(L.SscgError):
        F._ce_options(w.double(), 0.0, 4, torch.device("cpu"))
    assert F._ce_options(None, 0.0, 4, torch.device("cpu")) == (None, 0.0, False)
    assert F._ce_options(w, 0.0, 4, torch.device("cpu"))[2] and F._ce_options(None, 0.1, 4, torch.device("cpu"))[2]


class _Driver(object):
    """The loss-option part of both drivers (model._WeightedCE) without their networks, which need the GPU."""

    def __new__(cls, md, **kw):
        kind = type("Driver", (md._WeightedCE,), {})
        d = kind()
        d.args = types.SimpleNamespace(gpu_ids=[], **kw)
        d.dp, d.n_channels = None, 4
        d._init_ce(d.args, 4)
        return d


def test_the_defaults_never_count_labels(monkeypatch, capsys):
    md, F = load_sub("model"), load_sub("functional")
    assert issubclass(md.supervised_model, md._WeightedCE) and issubclass(md.semisuper_cycleGAN, md._WeightedCE)

    def refuse(*a, **k):
        raise AssertionError("label_hist was called")

    class Untouchable(object):
        def __iter__(self):
            raise AssertionError("the labelled loader was read")

    monkeypatch.setattr(F, "label_hist", refuse)
    for kw in ({}, {"ce_weights": "", "label_smoothing": 0.0}):
        d = _Driver(md, **kw)
        assert d.resolve_ce_weights(Untouchable()) is None and d._ce_kwargs() == {} and d.ce_weight is None and d.ce_smoothing == 0.0
    assert capsys.readouterr().out == ""                      # nothing is printed either
    d = _Driver(md, ce_weights="", label_smoothing=0.1)
    assert d.resolve_ce_weights(Untouchable()) is None and d._ce_kwargs() == {"weight": None, "label_smoothing": 0.1}
    d = _Driver(md, ce_weights="1,0,2,0.5", label_smoothing=0.0)         # a list needs no pass over the data
    assert d.resolve_ce_weights(Untouchable()).tolist() == [1.0, 0.0, 2.0, 0.5] and d._ce_kwargs()["label_smoothing"] == 0.0
    assert "1, 0, 2, 0.5" in capsys.readouterr().out          # the resolved weights are printed once
    d = _Driver(md, ce_weights="median")
    with pytest.raises(RuntimeError):                         # a rule that was never resolved must not train unweighted in silence
        d._ce_kwargs()
    with pytest.raises(AssertionError, match="the labelled loader was read"):
        d.resolve_ce_weights(Untouchable())
    for bad in ({"label_smoothing": 1.0}, {"label_smoothing": -0.5}, {"ce_weights": "1,2,3"}, {"ce_weights": "bogus"}):
        with pytest.raises(ValueError):
            _Driver(md, **bad)
