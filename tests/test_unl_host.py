"""The losses of the unlabelled head (sscg_unl_workspace / sscg_unl_fwd / sscg_unl_bwd / sscg_upsample_head_bwd_u; --unl_entropy,
--unl_maxsq, --unl_pseudo, --unl_pseudo_thresh, --unl_ramp) on a GPU-less host: the four entries are declared, exported and bound, the
C entries return every argument error before any HIP call, the flags parse and validate, the ramp is the documented schedule, a model
built with the defaults takes none of the new paths, the closed form the kernels implement equals torch's autograd of the definitions
in fp64 - and the inputs of tests/test_unl_gpu.py keep the margins that make its exact comparisons meaningful."""
import ctypes as C
import os
import re
import subprocess
import sys
import types

import pytest
import torch

from conftest import ROOT, load_sub
from test_dice_host import CLASSES, GEOMS
from test_unl_gpu import SEEDS, case_inputs
from unl_reference import MARGIN, TAU, closed_form_grad, make_logits, unl_reference

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
ONE = C.c_void_p(16)          # never dereferenced
NEW = ("sscg_unl_workspace", "sscg_unl_fwd", "sscg_unl_bwd", "sscg_upsample_head_bwd_u")
FLAGS = ("unl_entropy", "unl_maxsq", "unl_pseudo", "unl_pseudo_thresh", "unl_ramp")


# ------------------------------------------------------------------------------------------ 1. the ABI
def test_the_four_entries_are_declared_exported_and_bound():
    L = load_sub("_lib")
    hdr = open(os.path.join(ROOT, "include", "sscg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "size_t sscg_unl_workspace(int N, int OH, int OW);" in code
    assert ("int sscg_unl_fwd(const float* x, int N, int H, int W, int C, int OH, int OW, float thresh, float* losses, double* sums, "
            "uint8_t* pseudo,") in code
    assert "int sscg_unl_bwd(const float* x, const uint8_t* pseudo, int N, int H, int W, int C, const float* g_ent, const float* g_msq," in code
    assert ("int sscg_upsample_head_bwd_u(const float* x, const uint8_t* pseudo, const float* dy_soft, const float* g_ent, "
            "const float* g_msq,") in code
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sscg_[a-z0-9_]+)", out))
    for name in NEW:
        assert name in exported and name in L.SIGNATURES and callable(getattr(L.lib, name)), name
    assert [len(L.SIGNATURES[n][1]) for n in NEW] == [3, 14, 12, 15]
    fwd = L.SIGNATURES["sscg_unl_fwd"][1]
    assert fwd[7] is C.c_float and fwd[12] is C.c_size_t                                 # thresh, ws_bytes
    assert L.SIGNATURES["sscg_unl_workspace"][0] is C.c_size_t
    assert L.ABI_VERSION == 18 and L.lib.sscg_abi_version() == 18 and "#define SSCG_ABI_VERSION 18" in hdr      # additions only
    # the workspace: one fp64 record of four per statistics block, at most 256 blocks per sample, and one per sample
    ws = L.lib.sscg_unl_workspace
    assert ws(2, 13, 17) == 2 * (1 + 1) * 4 * 8 and ws(8, 256, 256) == 8 * (256 + 1) * 4 * 8
    assert ws(1, 363, 363) == (256 + 1) * 4 * 8 and ws(3, 150, 151) == 3 * (89 + 1) * 4 * 8
    assert ws(0, 5, 5) == 0 and ws(1, 0, 5) == 0 and ws(1, 5, -1) == 0


def test_argument_errors_are_returned_before_any_launch():
    lib = load_sub("_lib").lib
    big = 1 << 30

    def fwd(x=ONE, N=2, H=3, W=4, Cn=4, OH=13, OW=17, tau=0.5, losses=ONE, sums=ONE, pm=ONE, ws=ONE, wsb=big):
        return lib.sscg_unl_fwd(x, N, H, W, Cn, OH, OW, tau, losses, sums, pm, ws, wsb, None)

    def bwd(x=ONE, pm=ONE, N=2, H=3, W=4, Cn=4, ge=ONE, gm=ONE, gp=ONE, sums=ONE, dx=ONE):
        return lib.sscg_unl_bwd(x, pm, N, H, W, Cn, ge, gm, gp, sums, dx, None)

    def head(x=ONE, pm=ONE, dy=ONE, ge=ONE, gm=ONE, gp=ONE, sums=ONE, dx=ONE, N=2, H=3, W=4, Cn=4, OH=13, OW=17):
        return lib.sscg_upsample_head_bwd_u(x, pm, dy, ge, gm, gp, sums, dx, N, H, W, Cn, OH, OW, None)

    for call in (fwd, bwd, head):
        assert call(x=None) == BAD_ARG and call(sums=None) == BAD_ARG, call.__name__
        assert call(Cn=0) == BAD_ARG and call(Cn=65) == BAD_ARG and call(Cn=-1) == BAD_ARG
        assert call(N=0) == BAD_ARG and call(H=0) == BAD_ARG and call(W=-3) == BAD_ARG
    for tau in (-0.01, 1.01, float("nan"), float("inf"), -float("inf")):
        assert fwd(tau=tau) == BAD_ARG, tau
    assert fwd(losses=None) == BAD_ARG and fwd(OH=0) == BAD_ARG and fwd(OW=-1) == BAD_ARG
    assert fwd(ws=None) == WORKSPACE and fwd(wsb=2 * 2 * 4 * 8 - 1) == WORKSPACE
    assert fwd(pm=None, ws=None) == WORKSPACE                                       # the map is optional: the error is not its
    assert fwd(N=1, H=1, W=1, OH=46341, OW=46341) == UNSUPPORTED                   # N * OH * OW >= 2^31
    assert fwd(N=1, H=1, W=1, OH=46341, OW=46341, ws=None) == UNSUPPORTED          # ... before the workspace is looked at
    assert fwd(N=1, H=1, W=1, OH=46341, OW=46341, tau=2.0) == BAD_ARG              # ... after the arguments
    assert bwd(dx=None) == BAD_ARG and bwd(N=1, H=46341, W=46341) == UNSUPPORTED
    assert bwd(ge=None, gm=None, gp=None) == BAD_ARG                                # nothing to differentiate
    assert bwd(pm=None) == BAD_ARG and head(pm=None) == BAD_ARG                     # the pseudo-label gradient without its labels
    assert head(dx=None) == BAD_ARG and head(OH=0) == BAD_ARG
    assert head(N=1, H=1, W=1, OH=46341, OW=46341) == UNSUPPORTED
    # no loss gradient: the plain head's entry decides - it refuses a call without dy_soft too
    assert head(ge=None, gm=None, gp=None, dy=None) == BAD_ARG and head(ge=None, gm=None, gp=None, x=None) == BAD_ARG


# ------------------------------------------------------------------------------------------ 2. flags, options, schedule
def test_main_takes_the_flags_and_moves_no_default(capsys):
    sys.path.insert(0, ROOT)
    import main
    a = main.get_args([])
    assert (a.unl_entropy, a.unl_maxsq, a.unl_pseudo, a.unl_pseudo_thresh, a.unl_ramp) == (0.0, 0.0, 0.0, None, 0)
    before = dict(vars(a))
    assert not any(k.startswith("unl") for k in before)            # a default run parses to the namespace it always did
    old = ["--dataset", "acdc", "--ce_weights", "median", "--tta", "0.5,1.0:flip", "--batch_size", "4", "--ssim_weight", "0.5"]
    assert not any(k.startswith("unl") for k in vars(main.get_args(old)))
    b = main.get_args(["--unl_entropy", "0.1", "--unl_maxsq", "0.2", "--unl_pseudo", "0.3", "--unl_pseudo_thresh", "0.8", "--unl_ramp", "5"])
    assert (b.unl_entropy, b.unl_maxsq, b.unl_pseudo, b.unl_pseudo_thresh, b.unl_ramp) == (0.1, 0.2, 0.3, 0.8, 5)
    assert {k: v for k, v in vars(b).items() if not k.startswith("unl")} == before
    assert main.get_args(["--unl_entropy", "0"]).unl_entropy == 0.0               # 0 means off
    assert main.get_args(["--unl_pseudo", "1", "--unl_pseudo_thresh", "0"]).unl_pseudo_thresh == 0.0
    for bad in (["--unl_entropy", "-0.1"], ["--unl_entropy", "nan"], ["--unl_entropy", "inf"], ["--unl_entropy", "x"],
                ["--unl_maxsq", "-1"], ["--unl_maxsq", "nan"], ["--unl_pseudo", "-1"], ["--unl_pseudo", "inf"],
                ["--unl_pseudo_thresh", "0.5"], ["--unl_pseudo", "0", "--unl_pseudo_thresh", "0.5"],
                ["--unl_pseudo", "1", "--unl_pseudo_thresh", "1.5"], ["--unl_pseudo", "1", "--unl_pseudo_thresh", "-0.1"],
                ["--unl_pseudo", "1", "--unl_pseudo_thresh", "nan"], ["--unl_ramp", "-1"], ["--unl_ramp", "1.5"]):
        with pytest.raises(SystemExit):
            main.get_args(bad)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        main.get_args(["--help"])
    out = capsys.readouterr().out
    for flag in FLAGS:
        assert "--" + flag in out and "--" + flag in main.__doc__, flag


def test_options_validate_on_the_host():
    F, L = load_sub("functional"), load_sub("_lib")
    o = F.UnlabelledOptions()
    assert (o.entropy, o.maxsq, o.pseudo, o.thresh, o.any) == (0.0, 0.0, 0.0, 0.9, False)
    o = F.UnlabelledOptions(entropy=1, maxsq=0.5, pseudo=2, thresh=0)
    assert (o.entropy, o.maxsq, o.pseudo, o.thresh, o.any) == (1.0, 0.5, 2.0, 0.0, True)
    assert F.UnlabelledOptions(thresh=1).thresh == 1.0 and F._unl_options({"pseudo": 1.0}).pseudo == 1.0 and F._unl_options(None).thresh == 0.9
    for bad in (dict(entropy=-1), dict(entropy=float("nan")), dict(maxsq=float("inf")), dict(pseudo=-0.5), dict(thresh=-0.1),
                dict(thresh=1.1), dict(thresh=float("nan"))):
        with pytest.raises(ValueError):
            F.UnlabelledOptions(**bad)
    with pytest.raises(TypeError):
        F._unl_options(0.5)
    # no CPU fallback
    x = torch.zeros(1, 4, 3, 3)
    with pytest.raises(L.SscgError):
        F.unlabelled_losses(x)
    with pytest.raises(L.SscgError):
        F.upsample_softmax_unl(x, (12, 12), o)
    assert F.upsample_softmax_ce.__defaults__ == (None, True, None, 0.0)        # the plain head keeps its signature


class _Driver(object):
    """The unlabelled-loss part of the semi-supervised driver (model._UnlabelledLosses) without its networks, which need the GPU."""

    def __new__(cls, md, **kw):
        kind = type("Driver", (md._UnlabelledLosses,), {})
        d = kind()
        d.args = types.SimpleNamespace(gpu_ids=[], **kw)
        d.crop = (12, 12)
        d._init_unl(d.args)
        return d


def test_the_ramp_schedule():
    md, U = load_sub("model"), load_sub("utils")
    assert issubclass(md.semisuper_cycleGAN, md._UnlabelledLosses) and not issubclass(md.supervised_model, md._UnlabelledLosses)
    d = _Driver(md, unl_entropy=0.4, unl_ramp=4)
    assert d.unl_ramp == 4 and d._unl_scale == 0.0
    assert [d.set_unl_epoch(e) for e in (0, 1, 2, 4, 5, 400)] == [0.0, 0.25, 0.5, 1.0, 1.0, 1.0]
    assert [0.4 * d.set_unl_epoch(e) for e in (1, 3, 9)] == [U.boundary_loss_schedule(0.4, 4, e) for e in (1, 3, 9)]
    d = _Driver(md, unl_maxsq=0.4)
    assert d.unl_ramp == 0 and [d.set_unl_epoch(e) for e in (0, 7)] == [1.0, 1.0]
    off = _Driver(md, unl_ramp=3)
    assert off.unl_options is None and off.set_unl_epoch(1) == 1.0             # off: nothing changes
    # the weights reach the weighted sum ramped, each term under its own key
    d = _Driver(md, unl_entropy=0.4, unl_pseudo=0.2, unl_pseudo_thresh=0.7, unl_ramp=4)
    o = d.unl_options
    assert (o.entropy, o.maxsq, o.pseudo, o.thresh) == (0.4, 0.0, 0.2, 0.7)
    assert _Driver(md, unl_pseudo=1.0).unl_options.thresh == 0.9
    for bad in (dict(unl_entropy=-1.0), dict(unl_maxsq=float("nan")), dict(unl_pseudo=float("inf")), dict(unl_pseudo_thresh=0.5),
                dict(unl_pseudo=1.0, unl_pseudo_thresh=1.5), dict(unl_entropy=1.0, unl_ramp=-1), dict(unl_entropy=1.0, unl_ramp=1.5)):
        with pytest.raises(ValueError):
            _Driver(md, **bad)


def test_the_defaults_take_no_unlabelled_path(monkeypatch):
    md, F = load_sub("model"), load_sub("functional")
    seen = []
    monkeypatch.setattr(F, "upsample_softmax_ce", lambda *a, **k: seen.append((a, k)) or ("soft", None))
    monkeypatch.setattr(F, "upsample_softmax_unl", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the unlabelled losses were called")))
    for kw in ({}, dict(unl_entropy=0.0), dict(unl_entropy=0, unl_maxsq=0.0, unl_pseudo=0, unl_ramp=3)):
        d = _Driver(md, **kw)
        assert d.unl_options is None
        extras, terms, weights = {}, [], []
        assert d._unl_head("x", extras, terms, weights) == "soft" and seen[-1] == (("x", (12, 12)), {})
        assert extras == {} and terms == [] and weights == []
    # on: the enabled terms join the extras under their own keys with their own ramped weights
    sums = torch.tensor([0.0, 0.0, 0.0, 72.0], dtype=torch.float64)
    soft = torch.zeros(2, 4, 12, 12)
    calls = []
    monkeypatch.setattr(F, "upsample_softmax_ce", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the plain head was called")))
    monkeypatch.setattr(F, "upsample_softmax_unl", lambda *a, **k: calls.append((a, k)) or (soft, "E", "M", "P", {"sums": sums, "pseudo": None}))
    d = _Driver(md, unl_entropy=0.4, unl_pseudo=0.2, unl_ramp=4)
    d.set_unl_epoch(1)
    extras, terms, weights = {}, [], []
    assert d._unl_head("x", extras, terms, weights) is soft and calls[-1] == (("x", (12, 12), d.unl_options), {})
    assert terms == ["E", "P"] and weights == [0.4 * 0.25, 0.2 * 0.25]
    assert set(extras) == {"unl_entropy", "unl_pseudo_ce", "unl_pseudo_kept"} and extras["unl_entropy"] == "E" and extras["unl_pseudo_ce"] == "P"
    assert extras["unl_pseudo_kept"].dtype == torch.float32 and float(extras["unl_pseudo_kept"]) == 72.0 / (2 * 12 * 12)
    d = _Driver(md, unl_maxsq=1.5)
    extras, terms, weights = {}, [], []
    d._unl_head("x", extras, terms, weights)
    assert terms == ["M"] and weights == [1.5] and set(extras) == {"unl_maxsq"}


# ------------------------------------------------------------------------------------------ 3. the closed form
@pytest.mark.parametrize("C", [1, 4, 21])
def test_closed_form_equals_autograd_of_the_definition(C):
    """q_c = dy_c - (g_e / (V ln C)) u_c - (g_m / V) p_c, d_c = p_c (q_c - sum p q) + [kept] (g_p / max(K, 1)) (p_c - [c == y*]), then
    F.interpolate's adjoint - what the kernels compute - against torch's autograd of the definitions, both in fp64."""
    x = make_logits(40 + C, 2, C, 5, 5)
    g = torch.Generator().manual_seed(50 + C)
    R = torch.randn(2, C, 21, 23, generator=g, dtype=torch.float64) * 0.01
    worst = 0.0
    for gs in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.37, 1.9, 0.61)):
        for r in (None, R):
            for resize in ((21, 23), None):
                if resize is None and r is not None:
                    continue
                ref = unl_reference(x, TAU[C], resize, gs, r)
                got = closed_form_grad(x, TAU[C], resize, gs, r)
                worst = max(worst, float((got - ref["grad"]).abs().max()))
                assert C == 1 or resize is None or 0 < ref["K"] < ref["V"]
    print("unl closed form C=%d: max-abs distance %.2e" % (C, worst))
    assert worst <= 1e-15
    # the value ranges of the definitions
    ref = unl_reference(x, TAU[C], (21, 23))
    assert 0.0 <= float(ref["ent"]) <= 1.0 and -0.5 - 1e-15 <= float(ref["msq"]) <= -0.5 / C + 1e-15
    if C == 1:
        assert float(ref["ent"]) == 0.0 and float(ref["pl"]) == 0.0 and float(ref["grad"].abs().max()) == 0.0
    none = unl_reference(x, 1.0, (21, 23), (0.0, 0.0, 1.0)) if C > 1 else None
    assert none is None or (none["K"] == 0 and float(none["pl"]) == 0.0 and float(none["grad"].abs().max()) == 0.0)


# ------------------------------------------------------------------------------------------ 4. the GPU tests' inputs
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("gi", range(len(GEOMS)))
def test_the_gpu_inputs_keep_their_margins(gi, C):
    N, H, W, OH, OW = GEOMS[gi]
    assert 0 <= SEEDS[(gi, C)] < 14
    x, taus = case_inputs(gi, C)
    assert torch.equal(x, x.float().double())                  # fp32-representable
    assert len(taus) == (1 if H * W > 1 or C == 1 else 2)
    shares = []
    for tau in taus:
        ref = unl_reference(x, tau, (OH, OW))
        assert ref["conf_margin"] >= MARGIN and ref["gap_margin"] >= MARGIN, (gi, C, tau, ref["conf_margin"], ref["gap_margin"])
        shares.append(ref["kept_share"])
        if C > 1 and H * W > 1:
            assert 0.1 <= ref["kept_share"] <= 0.9, (gi, C, ref["kept_share"])
    if H * W == 1:                                             # the all-or-none case: K = V and (C > 1) K = 0
        assert shares == ([1.0] if C == 1 else [1.0, 0.0])
