"""Mean-teacher consistency on the unlabelled head (sscg_teacher_workspace / sscg_teacher_fwd; --unl_teacher) on a GPU-less host: the
two entries are declared, exported and bound, the C entry returns every argument error before any HIP call, the flag parses and
validates, a model built with the defaults takes no teacher path, the closed form the kernels implement equals torch's autograd of the
definition in fp64 - and the inputs of tests/test_teacher_gpu.py keep the margins that make its exact comparisons meaningful."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
import types

import pytest
import torch

from conftest import ROOT, load_sub
from test_dice_host import CLASSES, GEOMS
from teacher_reference import (CONFIGS, FLIPS, MARGIN, SEEDS, case_inputs, closed_form_grad, input_ok, inputs_of, reference, soft_upstream,
                               teacher_reference)

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
ONE = C.c_void_p(16)          # never dereferenced
NEW = ("sscg_teacher_workspace", "sscg_teacher_fwd")


# ------------------------------------------------------------------------------------------ 1. the ABI
def test_the_entries_are_declared_exported_and_bound():
    L = load_sub("_lib")
    hdr = open(os.path.join(ROOT, "include", "sscg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "size_t sscg_teacher_workspace(int N, int OH, int OW);" in code
    assert ("int sscg_teacher_fwd(const float* x, const float* t, const uint8_t* flip, int N, int H, int W, int C, int OH, int OW, "
            "float inv_temp,") in code
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sscg_[a-z0-9_]+)", out))
    for name in NEW:
        assert name in exported and name in L.SIGNATURES and callable(getattr(L.lib, name)), name
    assert [len(L.SIGNATURES[n][1]) for n in NEW] == [3, 18]
    fwd = L.SIGNATURES["sscg_teacher_fwd"][1]
    assert fwd[9] is C.c_float and fwd[10] is C.c_float and fwd[16] is C.c_size_t            # inv_temp, thresh, ws_bytes
    assert L.SIGNATURES["sscg_teacher_workspace"][0] is C.c_size_t
    assert L.ABI_VERSION == 18 and L.lib.sscg_abi_version() == 18 and "#define SSCG_ABI_VERSION 18" in hdr      # additions only
    # the workspace is sscg_unl_workspace's: one fp64 record of four per statistics block, at most 256 per sample, and one per sample
    ws = L.lib.sscg_teacher_workspace
    assert ws(2, 13, 17) == 2 * (1 + 1) * 4 * 8 and ws(8, 256, 256) == 8 * (256 + 1) * 4 * 8 and ws(3, 150, 151) == 3 * (89 + 1) * 4 * 8
    assert ws(0, 5, 5) == 0 and ws(1, 0, 5) == 0 and ws(1, 5, -1) == 0 and ws(1, 46341, 46341) == 0
    # the stream-ordering checker reads the header: the entry is in its table with the kinds of its pointers
    table = L.dev_tool("racecheck").parse_header(os.path.join(ROOT, "include", "sscg.h"))
    kinds = dict(table["sscg_teacher_fwd"])
    assert [kinds[a] for a in ("x", "t", "flip")] == ["r"] * 3
    assert [kinds[a] for a in ("losses", "sums", "pseudo", "coef", "ws")] == ["w"] * 5 and kinds["stream"] == "stream"


def test_argument_errors_are_returned_before_any_launch():
    lib = load_sub("_lib").lib
    big = 1 << 30

    def fwd(x=ONE, t=ONE, flip=ONE, N=2, H=3, W=4, Cn=4, OH=13, OW=17, it=1.0, tau=0.5, losses=ONE, sums=ONE, pm=ONE, coef=ONE, ws=ONE,
            wsb=big):
        return lib.sscg_teacher_fwd(x, t, flip, N, H, W, Cn, OH, OW, it, tau, losses, sums, pm, coef, ws, wsb, None)

    assert fwd(x=None) == BAD_ARG and fwd(t=None) == BAD_ARG and fwd(losses=None) == BAD_ARG and fwd(sums=None) == BAD_ARG
    assert fwd(Cn=0) == BAD_ARG and fwd(Cn=65) == BAD_ARG and fwd(Cn=-1) == BAD_ARG
    assert fwd(N=0) == BAD_ARG and fwd(H=0) == BAD_ARG and fwd(W=-3) == BAD_ARG and fwd(OH=0) == BAD_ARG and fwd(OW=-1) == BAD_ARG
    for tau in (-0.01, 1.01, float("nan"), float("inf"), -float("inf")):
        assert fwd(tau=tau) == BAD_ARG, tau
    for it in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert fwd(it=it) == BAD_ARG, it
    # the optional operands are no error of their own: the next check answers
    assert fwd(flip=None, pm=None, coef=None, ws=None) == WORKSPACE
    assert fwd(ws=None) == WORKSPACE and fwd(wsb=2 * 2 * 4 * 8 - 1) == WORKSPACE
    assert fwd(N=1, H=1, W=1, OH=46341, OW=46341) == UNSUPPORTED                   # N * OH * OW >= 2^31
    assert fwd(N=1, H=46341, W=46341, OH=46341, OW=46340) == UNSUPPORTED           # N * H * W >= 2^31
    assert fwd(N=1, H=1, W=1, OH=46341, OW=46341, ws=None) == UNSUPPORTED          # ... before the workspace is looked at
    assert fwd(N=1, H=1, W=1, OH=46341, OW=46341, tau=2.0) == BAD_ARG              # ... after the arguments
    assert fwd(N=1, H=1, W=1, OH=46341, OW=46341, it=0.0) == BAD_ARG


# ------------------------------------------------------------------------------------------ 2. the flag and the options
def test_main_takes_the_flag_and_moves_no_default(capsys):
    sys.path.insert(0, ROOT)
    import main
    a = main.get_args([])
    assert a.unl_teacher == ""
    before = dict(vars(a))
    assert "unl_teacher" not in before                             # a default run parses to the namespace it always did
    old = ["--dataset", "acdc", "--ce_weights", "median", "--ema_decay", "0.99", "--unl_entropy", "0.5", "--unl_crf", "0.1"]
    assert "unl_teacher" not in vars(main.get_args(old))
    b = main.get_args(["--ema_decay", "0.99", "--unl_teacher", "mse=1,ce=0.5,thresh=0.6,flip"])
    assert b.unl_teacher == "mse=1,ce=0.5,thresh=0.6,flip" and b.ema_decay == 0.99
    assert {k: v for k, v in vars(b).items() if k not in ("unl_teacher", "ema_decay")} == before
    assert main.get_args(["--ema_decay", "0.9", "--unl_teacher", "on"]).unl_teacher == "on"
    assert main.get_args(["--ema_decay", "0.9", "--unl_teacher", "mse=1", "--unl_pseudo", "0.5"]).unl_pseudo == 0.5      # mse rides beside it
    for bad in (["--unl_teacher", "on"],                                               # no --ema_decay
                ["--ema_decay", "0.9", "--unl_teacher", "ce=1", "--unl_pseudo", "0.5"],   # one pseudo-label slot
                ["--ema_decay", "0.9", "--unl_teacher", "mse=-1"], ["--ema_decay", "0.9", "--unl_teacher", "thresh=1.5"],
                ["--ema_decay", "0.9", "--unl_teacher", "mse=0"], ["--ema_decay", "0.9", "--unl_teacher", "bogus=1"]):
        with pytest.raises(SystemExit):
            main.get_args(bad)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        main.get_args(["--help"])
    assert "--unl_teacher" in capsys.readouterr().out and "--unl_teacher" in main.__doc__


def test_parse_unl_teacher_accepts_and_refuses():
    U, F = load_sub("utils"), load_sub("functional")
    assert U.parse_unl_teacher("") is None and U.parse_unl_teacher(None) is None and U.parse_unl_teacher("  ") is None
    o = U.parse_unl_teacher("on")
    assert isinstance(o, F.TeacherOptions) and (o.mse, o.ce, o.thresh, o.temp, o.flip) == (1.0, 0.0, 0.0, 1.0, False)
    o = U.parse_unl_teacher("mse=1,ce=0.5,thresh=0.6,temp=0.5,flip")
    assert (o.mse, o.ce, o.thresh, o.temp, o.flip) == (1.0, 0.5, 0.6, 0.5, True) and o.inv_temp == 2.0
    o = U.parse_unl_teacher(" flip , ce=2 ")
    assert (o.mse, o.ce, o.thresh, o.temp, o.flip) == (0.0, 2.0, 0.0, 1.0, True)
    assert U.parse_unl_teacher("mse=1,thresh=0").thresh == 0.0 and U.parse_unl_teacher("mse=1,thresh=1").thresh == 1.0
    assert U.parse_unl_teacher("mse=1,temp=3").inv_temp == float(torch.tensor(1.0 / 3.0, dtype=torch.float32))      # rounded to fp32 once
    for bad in ("mse", "mse=", "mse=x", "mse=-1", "mse=nan", "mse=inf", "ce=-0.5", "thresh=-0.1", "thresh=1.1", "thresh=nan", "temp=0",
                "temp=-1", "temp=inf", "temp=nan", "flip=1", "flip,flip", "mse=1,mse=2", "iters=3", "mse=1,,ce=1", "mse=0", "mse=0,ce=0",
                "flip", "thresh=0.5", "On"):
        with pytest.raises(ValueError) as e:
            U.parse_unl_teacher(bad)
        assert "--unl_teacher" in str(e.value), bad


def test_options_validate_on_the_host():
    F, L = load_sub("functional"), load_sub("_lib")
    o = F.TeacherOptions()
    assert (o.mse, o.ce, o.thresh, o.temp, o.flip, o.any) == (0.0, 0.0, 0.0, 1.0, False, False)
    o = F.TeacherOptions(mse=1, ce=0.5, thresh=1, temp=2, flip=1)
    assert (o.mse, o.ce, o.thresh, o.temp, o.flip, o.any, o.inv_temp) == (1.0, 0.5, 1.0, 2.0, True, True, 0.5)
    assert F._teacher_options({"ce": 1.0}).ce == 1.0
    for bad in (dict(mse=-1), dict(mse=float("nan")), dict(ce=float("inf")), dict(ce=-0.5), dict(thresh=-0.1), dict(thresh=1.1),
                dict(thresh=float("nan")), dict(temp=0), dict(temp=-2), dict(temp=float("inf")), dict(temp=float("nan"))):
        with pytest.raises(ValueError):
            F.TeacherOptions(**bad)
    with pytest.raises(TypeError):
        F._teacher_options(0.5)
    with pytest.raises(TypeError):
        F._teacher_options(None)
    x = torch.zeros(1, 4, 3, 3)
    # both pseudo-label terms at once are refused before anything runs; no CPU fallback
    with pytest.raises(ValueError):
        F.upsample_softmax_teacher(x, (12, 12), x, F.TeacherOptions(ce=1.0), F.UnlabelledOptions(pseudo=1.0))
    with pytest.raises(L.SscgError):
        F.upsample_softmax_teacher(x, (12, 12), x, F.TeacherOptions(mse=1.0))
    with pytest.raises(L.SscgError):
        F.upsample_softmax_teacher(x, (3, 3), x, F.TeacherOptions(mse=1.0))
    assert F.upsample_softmax_unl.__defaults__ == (None, True, False) and F.upsample_softmax_ce.__defaults__ == (None, True, None, 0.0)


class _Driver(object):
    """The unlabelled-loss part of the semi-supervised driver (model._UnlabelledLosses) without its networks, which need the GPU."""

    def __new__(cls, md, **kw):
        kind = type("Driver", (md._UnlabelledLosses,), {})
        d = kind()
        d.args = types.SimpleNamespace(gpu_ids=[], **kw)
        d.crop = (12, 12)
        d._init_unl(d.args)
        return d


def test_the_option_matrix():
    md = load_sub("model")
    d = _Driver(md, ema_decay=0.9, unl_teacher="mse=1,ce=0.5,thresh=0.6,flip", unl_ramp=4)
    t = d.unl_teacher
    assert (t.mse, t.ce, t.thresh, t.temp, t.flip) == (1.0, 0.5, 0.6, 1.0, True) and d.unl_options is None
    assert d.unl_ramp == 4 and d._unl_scale == 0.0 and [d.set_unl_epoch(e) for e in (1, 2, 4, 9)] == [0.25, 0.5, 1.0, 1.0]      # it rides --unl_ramp
    assert isinstance(d._teacher_rng, torch.Generator)
    assert _Driver(md, ema_decay=0.9, unl_teacher="on")._teacher_rng is None
    d = _Driver(md, ema_decay=0.0, unl_teacher="mse=2", unl_pseudo=0.5, unl_entropy=0.1)            # mse rides beside --unl_pseudo
    assert d.unl_teacher.mse == 2.0 and d.unl_options.pseudo == 0.5
    for bad in (dict(unl_teacher="on"), dict(unl_teacher="on", ema_decay=None),                   # no --ema_decay
                dict(unl_teacher="ce=1", ema_decay=0.9, unl_pseudo=0.5),                          # ce with --unl_pseudo
                dict(unl_teacher="mse=1,ce=0.1", ema_decay=0.9, unl_pseudo=0.5),
                dict(unl_teacher="mse=-1", ema_decay=0.9), dict(unl_teacher="thresh=0.5", ema_decay=0.9)):
        with pytest.raises(ValueError):
            _Driver(md, **bad)
    # the generator-loss term count follows the live weights
    base = md.gen_loss_terms_of(types.SimpleNamespace())
    for spec, n in (("", 0), ("on", 1), ("ce=1", 1), ("mse=1,ce=0.5,flip", 2), ("mse=0,ce=2", 1)):
        assert md.gen_loss_terms_of(types.SimpleNamespace(unl_teacher=spec, ema_decay=0.9)) == base + n, spec
    assert md.gen_loss_terms_of(types.SimpleNamespace(unl_teacher="mse=1,ce=1", unl_entropy=0.1, unl_crf=0.2)) == base + 4


def test_the_flip_draws_come_from_a_generator_of_their_own():
    md = load_sub("model")
    img = torch.zeros(64, 3, 4, 4)
    runs = []
    for other_seed in (1, 2):
        torch.manual_seed(other_seed)
        d = _Driver(md, ema_decay=0.9, unl_teacher="mse=1,flip")
        before = torch.get_rng_state()
        # (all 64 draws equal would need no launch; the view itself needs the GPU, the bytes do not: draw as _teacher_view does)
        draws = torch.rand(img.shape[0], generator=d._teacher_rng) < 0.5
        assert torch.equal(torch.get_rng_state(), before)          # torch's global stream did not move
        runs.append(draws)
    assert torch.equal(runs[0], runs[1]) and 0 < int(runs[0].sum()) < 64


def test_the_defaults_take_no_teacher_path(monkeypatch):
    md, F = load_sub("model"), load_sub("functional")
    seen = []
    boom = lambda what: (lambda *a, **k: (_ for _ in ()).throw(AssertionError(what + " was called")))
    monkeypatch.setattr(F, "upsample_softmax_ce", lambda *a, **k: seen.append((a, k)) or ("soft", None))
    monkeypatch.setattr(F, "upsample_softmax_teacher", boom("the teacher head"))
    monkeypatch.setattr(F, "teacher_fwd", boom("teacher_fwd"))
    monkeypatch.setattr(md._UnlabelledLosses, "_teacher_logits", boom("_teacher_logits"))
    for kw in ({}, dict(unl_teacher=""), dict(unl_teacher="", ema_decay=0.9, unl_ramp=3)):
        d = _Driver(md, **kw)
        assert d.unl_teacher is None and d._teacher_rng is None
        extras, terms, weights = {}, [], []
        assert d._unl_head("x", extras, terms, weights) == "soft" and seen[-1] == (("x", (12, 12)), {})
        assert extras == {} and terms == [] and weights == []
    # on: the plain heads are not called; the terms join the extras under their own keys with their own ramped weights
    sums = torch.tensor([3.0, 54.0, 5.0, 72.0], dtype=torch.float64)
    usums = torch.tensor([0.0, 0.0, 0.0, 36.0], dtype=torch.float64)
    soft = torch.zeros(2, 4, 12, 12)
    calls = []
    monkeypatch.setattr(F, "upsample_softmax_ce", boom("the plain head"))
    monkeypatch.setattr(F, "upsample_softmax_unl", boom("the unlabelled head"))
    monkeypatch.setattr(F, "upsample_softmax_teacher",
                        lambda *a, **k: calls.append((a, k)) or (soft, "MSE", "CE", "E", "M", "P", {"sums": sums, "pseudo": None, "unl_sums": usums}))
    d = _Driver(md, ema_decay=0.9, unl_teacher="mse=1,ce=0.5,thresh=0.6", unl_ramp=4)
    d.set_unl_epoch(1)
    extras, terms, weights = {}, [], []
    with pytest.raises(ValueError):
        d._unl_head("x", extras, terms, weights)                   # the step must hand the teacher's logits over
    assert d._unl_head("x", extras, terms, weights, None, ("T", "FLIP")) is soft
    assert calls[-1] == (("x", (12, 12), "T", d.unl_teacher, None), {"flip": "FLIP"})
    assert terms == ["MSE", "CE"] and weights == [1.0 * 0.25, 0.5 * 0.25]
    assert set(extras) == {"unl_teacher_mse", "unl_teacher_ce", "unl_teacher_kept", "unl_teacher_agree"}
    assert extras["unl_teacher_kept"].dtype == torch.float32 and float(extras["unl_teacher_kept"]) == 72.0 / (2 * 12 * 12)
    assert extras["unl_teacher_agree"].dtype == torch.float32 and float(extras["unl_teacher_agree"]) == 0.75
    d = _Driver(md, ema_decay=0.9, unl_teacher="mse=2", unl_entropy=0.4, unl_pseudo=0.2)
    extras, terms, weights = {}, [], []
    d._unl_head("x", extras, terms, weights, None, ("T", None))
    assert calls[-1] == (("x", (12, 12), "T", d.unl_teacher, d.unl_options), {"flip": None})
    assert terms == ["E", "P", "MSE"] and weights == [0.4, 0.2, 2.0]
    assert set(extras) == {"unl_entropy", "unl_pseudo_ce", "unl_pseudo_kept", "unl_teacher_mse", "unl_teacher_kept", "unl_teacher_agree"}
    assert float(extras["unl_pseudo_kept"]) == 36.0 / (2 * 12 * 12)
    # nothing kept: the agreement share is 0 / 1, not NaN
    sums[1], sums[3] = 0.0, 0.0
    extras = {}
    d._unl_head("x", extras, [], [], None, ("T", None))
    assert float(extras["unl_teacher_agree"]) == 0.0 and float(extras["unl_teacher_kept"]) == 0.0


# ------------------------------------------------------------------------------------------ 3. the closed form
@pytest.mark.parametrize("C", [1, 4, 21])
def test_closed_form_equals_autograd_of_the_definition(C):
    """dy = R + g_mse coef with coef = 2 (p - q) [kept] / (C V); d_c = p_c (dy_c - sum p dy) + [kept] (g_ce / max(K, 1)) (p_c - [c ==
    y*]); then F.interpolate's adjoint - what sscg_lovasz_scale_add and the stencil's pseudo-label slot compute - against torch's
    autograd of the definition, both in fp64."""
    gi = 2
    N, H, W, OH, OW = GEOMS[gi]
    x, t, flip = inputs_of(40 + C, gi, C)
    R = soft_upstream(50 + C, N, C, OH, OW)
    worst = 0.0
    for cfg, (taus, temp) in CONFIGS.items():
        for gs in ((1.0, 0.0), (0.0, 1.0), (0.37, 1.9)):
            for r in (None, R):
                for resize in ((OH, OW), None):
                    if resize is None and r is not None:
                        continue
                    ref = teacher_reference(x, t, flip, taus[C], temp, resize, gs, r)
                    got = closed_form_grad(x, t, flip, taus[C], temp, resize, gs, r)
                    worst = max(worst, float((got - ref["grad"]).abs().max()))
    print("teacher closed form C=%d: max-abs distance %.2e" % (C, worst))
    assert worst <= 1e-15
    ref = teacher_reference(x, t, flip, CONFIGS["t1"][0][C], 1.0, (OH, OW))
    assert 0.0 <= float(ref["mse"]) <= 2.0 / C and float(ref["ce"]) >= 0.0 and ref["A"] <= ref["K"] <= ref["V"]
    # the teacher equal to the student: distance 0, every kept pixel agrees, and the cross entropy is the unlabelled head's own
    same = teacher_reference(x, x, None, CONFIGS["t1"][0][C], 1.0, (OH, OW), (1.0, 0.0))
    assert float(same["mse"]) == 0.0 and same["A"] == same["K"] and float(same["grad"].abs().max()) == 0.0
    # nothing kept: both losses and the gradient are 0
    if C > 1:
        none = teacher_reference(x, t, flip, 1.0, 1.0, (OH, OW))
        assert none["K"] == 0 and float(none["mse"]) == 0.0 and float(none["ce"]) == 0.0 and float(none["grad"].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ 4. the GPU tests' inputs
def test_the_seed_table_is_the_first_passing_seed():
    """SEEDS pins, per case, the first seed of 0..39 that meets input_ok: every earlier one fails it (the table is not hand-picked)."""
    assert set(SEEDS) == {(cfg, gi, C) for cfg in CONFIGS for gi in range(len(GEOMS)) for C in CLASSES}
    for (cfg, gi, C), seed in SEEDS.items():
        N, H, W, OH, OW = GEOMS[gi]
        taus, temp = CONFIGS[cfg]
        assert 0 <= seed < 40
        for s in range(seed):
            x, t, flip = inputs_of(s, gi, C)
            assert not input_ok(teacher_reference(x, t, flip, taus[C], temp, (OH, OW)), C, H, W), (cfg, gi, C, s)


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("gi", range(len(GEOMS)))
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_the_gpu_inputs_keep_their_margins(cfg, gi, C):
    N, H, W, OH, OW = GEOMS[gi]
    x, t, flip, tau, temp = case_inputs(cfg, gi, C)
    assert torch.equal(x, x.float().double()) and torch.equal(t, t.float().double())       # fp32-representable
    assert flip == FLIPS[gi] and (flip is None or len(flip) == N)
    assert FLIPS[0] == (1, 0) and FLIPS[2] == (1, 0)               # mirrored and plain samples meet in one call
    ref = reference(cfg, gi, C)
    assert input_ok(ref, C, H, W)
    assert ref["conf_margin"] >= MARGIN and ref["gap_margin"] >= MARGIN, (cfg, gi, C, ref["conf_margin"], ref["gap_margin"])
    if C > 1 and H * W > 1:
        assert 0.1 <= ref["kept_share"] <= 0.9 and 0.1 <= ref["agree_share"] <= 0.9, (cfg, gi, C, ref["kept_share"], ref["agree_share"])
    assert math.isfinite(float(ref["mse"])) and math.isfinite(float(ref["ce"]))
