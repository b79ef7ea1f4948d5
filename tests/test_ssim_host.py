"""The structural-similarity loss without a GPU: the fp64 restatement (tests/ssim_reference.py) against values known by hand, the closed-form
gradient of include/sscg.h against autograd, the adjoint identity of the filter, the three entries in header, library and bindings,
their refusals (before any HIP call: pointers that are never dereferenced), the workspace query, the flags and the model's options."""
import ctypes as C
import os
import re
import subprocess
import sys
import types

import pytest
import torch

from conftest import ROOT, load_sub
from ssim_reference import closed_form_gradient, constants, gadjoint, gfilter, make_inputs, ssim_map, ssim_reference, window

NEW = ("sscg_ssim_workspace", "sscg_l1_ssim_fwd", "sscg_l1_ssim_bwd")
BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
ONE = C.c_void_p(16)                                                        # never dereferenced
SHAPES = [(2, 3, 11, 11, 11), (1, 3, 12, 45, 11), (2, 3, 43, 37, 11), (1, 1, 3, 3, 3), (2, 3, 40, 70, 7)]


# ------------------------------------------------------------------------------------------ 1. the reference
def test_the_window():
    for k, sigma in ((11, 1.5), (7, 1.0), (3, 0.5), (5, 2.25)):
        g = window(k, sigma)
        assert g.dtype == torch.float32 and g.numel() == k and abs(float(g.double().sum()) - 1.0) < 1e-6
        assert torch.equal(g, g.flip(0)) and int(g.argmax()) == k // 2
        d = torch.arange(k, dtype=torch.float64) - (k - 1) / 2
        e = torch.exp(-d * d / (2 * sigma * sigma))
        assert (g.double() - e / e.sum()).abs().max() < 2.0 ** -24


def test_reference_against_literals():
    c1, c2 = constants(2.0)
    assert c1 == (0.02) ** 2 and c2 == (0.06) ** 2
    # identical images: S == 1 everywhere, loss 0, gradient 0
    a, _ = make_inputs("noise", 2, 3, 14, 17, 1)
    r = ssim_reference(a, a.clone())
    assert (r["S"] - 1.0).abs().max() < 1e-12 and abs(float(r["loss"])) < 1e-12 and float(r["l1"]) == 0.0
    assert r["grad_ssim"].abs().max() < 1e-12 and torch.count_nonzero(r["grad_l1"]) == 0
    assert (r["per_sample"] - 1.0).abs().max() < 1e-12
    # a = -b constant: mu_a = -mu_b = m, no variance: S = (-2 m^2 + C1) / (2 m^2 + C1)
    m = 0.75
    a = torch.full((1, 2, 13, 12), m)
    r = ssim_reference(a, -a)
    # ... for weights that sum to 1.  The fp32 weights sum to s = 1 + O(2^-24) per axis, which leaves a "variance" m^2 s (1 - s):
    s = float(window(11, 1.5).double().sum()) ** 2
    q = m * m * s * (1 - s)
    want = (-2 * m * m * s * s + c1) * (-2 * q + c2) / ((2 * m * m * s * s + c1) * (2 * q + c2))
    assert (r["S"] - want).abs().max() < 1e-12 and abs(float(r["loss"]) - (1 - want)) < 1e-12 and abs(float(r["l1"]) - 2 * m) < 1e-15
    ideal = (-2 * m * m + c1) / (2 * m * m + c1)
    assert abs(s - 1) < 2.0 ** -21 and abs(want - ideal) < 8 * m * m * abs(s - 1) / c2      # (d S / d q = -4 S / c2 at q = 0, plus slack)
    # one window, H = W = k: the map is one number per (n, c), the moments are plain weighted sums
    for k, sigma in ((11, 1.5), (3, 0.8)):
        a, b = make_inputs("noise", 2, 3, k, k, 5 + k)
        S = ssim_map(a.double(), b.double(), k, sigma)
        assert S.shape == (2, 3, 1, 1)
        g = window(k, sigma).double()
        w2 = g[:, None] * g[None, :]
        x, y = a.double()[1, 2], b.double()[1, 2]
        mx, my = (w2 * x).sum(), (w2 * y).sum()
        vx, vy, cxy = (w2 * x * x).sum() - mx * mx, (w2 * y * y).sum() - my * my, (w2 * x * y).sum() - mx * my
        want = (2 * mx * my + c1) * (2 * cxy + c2) / ((mx * mx + my * my + c1) * (vx + vy + c2))
        assert abs(float(S[1, 2, 0, 0]) - float(want)) < 1e-13
        r = ssim_reference(a, b, k, sigma)
        assert torch.equal(r["per_sample"], S.mean(dim=(1, 2, 3))) and abs(float(r["loss"]) - (1 - float(S.mean()))) < 1e-15


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["noise", "near", "flat"])
def test_closed_form_gradient_against_autograd(shape, kind):
    N, Cn, H, W, k = shape
    a, b = make_inputs(kind, N, Cn, H, W, 100 + H + W)
    sigma = 1.5 if k == 11 else 1.0
    r = ssim_reference(a, b, k, sigma)
    got = closed_form_gradient(a.double(), b.double(), k, sigma)
    d, gmax = float((got - r["grad_ssim"]).abs().max()), float(r["grad_ssim"].abs().max())
    print("ssim closed form %-16s %-5s max-abs diff %.2e of %.2e rel %.2e" % ("x".join(map(str, shape)), kind, d, gmax, d / gmax))
    assert gmax > 0 and d <= 1e-12 * gmax


def test_the_adjoint_identity():
    gen = torch.Generator().manual_seed(3)
    for k, sigma, H, W in ((11, 1.5, 19, 23), (3, 0.7, 3, 8), (7, 1.0, 7, 7)):
        g = window(k, sigma).double()
        x = torch.randn(2, 3, H, W, generator=gen, dtype=torch.float64)
        y = torch.randn(2, 3, H - k + 1, W - k + 1, generator=gen, dtype=torch.float64)
        gy = gadjoint(y, g)
        assert gy.shape == x.shape
        lhs, rhs = float((gfilter(x, g) * y).sum()), float((x * gy).sum())
        assert abs(lhs - rhs) <= 1e-13 * max(1.0, abs(lhs))


# ------------------------------------------------------------------------------------------ 2. the ABI
def test_the_entries_are_declared_exported_and_bound():
    L = load_sub("_lib")
    hdr = open(os.path.join(ROOT, "include", "sscg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "size_t sscg_ssim_workspace(int N, int H, int W, int C, int win);" in code
    assert "int sscg_l1_ssim_fwd(const float* a, const float* b, int N, int H, int W, int C, int win, float sigma, float c1, float c2, float* l1," in code
    assert "int sscg_l1_ssim_bwd(const float* a, const float* b, const float* coef, int N, int H, int W, int C, int win, float sigma," in code
    assert "the reference has no such term" in hdr
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sscg_[a-z0-9_]+)", out))
    for name in NEW:
        assert name in exported and name in L.SIGNATURES and callable(getattr(L.lib, name)), name
    assert [len(L.SIGNATURES[n][1]) for n in NEW] == [5, 17, 15]
    assert L.ABI_VERSION == 18 and L.lib.sscg_abi_version() == 18 and "#define SSCG_ABI_VERSION 18" in hdr      # additions only


def test_argument_errors_are_returned_before_any_launch():
    lib = load_sub("_lib").lib
    big = 1 << 40

    def fwd(a=ONE, b=ONE, N=2, H=20, W=30, Cn=3, win=11, sigma=1.5, c1=4e-4, c2=3.6e-3, l1=ONE, loss=ONE, per=ONE, coef=ONE, ws=ONE, wsb=big):
        return lib.sscg_l1_ssim_fwd(a, b, N, H, W, Cn, win, sigma, c1, c2, l1, loss, per, coef, ws, wsb, None)

    def bwd(a=ONE, b=ONE, coef=ONE, N=2, H=20, W=30, Cn=3, win=11, sigma=1.5, g_l1=ONE, g_ssim=ONE, da=ONE):
        return lib.sscg_l1_ssim_bwd(a, b, coef, N, H, W, Cn, win, sigma, g_l1, 1.0, g_ssim, 1.0, da, None)

    for call in (fwd, bwd):
        assert call(a=None) == BAD_ARG and call(b=None) == BAD_ARG, call.__name__
        assert call(N=0) == BAD_ARG and call(H=0) == BAD_ARG and call(W=-3) == BAD_ARG, call.__name__
        for win in (10, 4, 1, 2, 13, 12, 0, -3):                                # even, or outside 3..11
            assert call(win=win, H=64, W=64) == BAD_ARG, (call.__name__, win)
        assert call(sigma=0.0) == BAD_ARG and call(sigma=-1.0) == BAD_ARG and call(sigma=float("nan")) == BAD_ARG, call.__name__
        assert call(H=10) == BAD_ARG and call(W=10) == BAD_ARG and call(win=7, H=6) == BAD_ARG, call.__name__      # smaller than the window
        assert call(Cn=0) == UNSUPPORTED and call(Cn=5) == UNSUPPORTED and call(Cn=-1) == UNSUPPORTED, call.__name__
        assert call(N=1, H=46341, W=46341, Cn=1) == UNSUPPORTED and call(N=2, H=16384, W=16384, Cn=4) == UNSUPPORTED, call.__name__
        assert call(N=1 << 30, H=1 << 30, W=1 << 30, Cn=4) == UNSUPPORTED, call.__name__                           # no wrap-around
        assert call(N=1, H=46341, W=46341, Cn=1, a=None) == BAD_ARG, call.__name__                                 # ... after the arguments
    assert fwd(loss=None) == BAD_ARG and fwd(c1=-1e-9) == BAD_ARG and fwd(c2=-1.0) == BAD_ARG and fwd(c1=float("nan")) == BAD_ARG
    assert bwd(da=None) == BAD_ARG and bwd(coef=None) == BAD_ARG and bwd(g_l1=None, g_ssim=None) == BAD_ARG
    # the workspace: missing, one byte short
    need = lib.sscg_ssim_workspace(2, 20, 30, 3, 11)
    assert need > 0 and fwd(ws=None) == WORKSPACE and fwd(wsb=need - 1) == WORKSPACE and fwd(wsb=0) == WORKSPACE
    assert fwd(N=1, H=46341, W=46341, Cn=1, ws=None) == UNSUPPORTED                                                # sizes before the workspace
    # l1, per_sample and coef are optional: the error (if any) is not theirs
    assert fwd(l1=None, per=None, coef=None, ws=None) == WORKSPACE


def test_workspace_sizes():
    ws = load_sub("_lib").lib.sscg_ssim_workspace
    # two fp64 records per forward block, one block per (sample, 16 x 16 tile of the map)
    assert ws(2, 11, 11, 3, 11) == 2 * 2 * 8 and ws(1, 3, 3, 1, 3) == 2 * 8
    assert ws(8, 256, 256, 3, 11) == 2 * 8 * 16 * 16 * 8 and ws(1, 27, 28, 3, 11) == 2 * 2 * 2 * 8 and ws(2, 40, 70, 4, 7) == 2 * 2 * 3 * 4 * 8
    sizes = [ws(n, h, w, 3, 11) for n, h, w in ((1, 11, 11), (1, 26, 26), (1, 27, 26), (1, 27, 27), (2, 27, 27), (2, 64, 64), (3, 64, 200))]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0                  # monotone in every extent
    assert ws(1, 30, 30, 3, 11) <= ws(1, 30, 30, 3, 9) <= ws(1, 30, 30, 3, 3)              # a smaller window leaves a larger map
    for bad in ((0, 20, 20, 3, 11), (1, 0, 20, 3, 11), (1, 20, -1, 3, 11), (1, 20, 20, 0, 11), (1, 20, 20, 5, 11), (1, 20, 20, 3, 10),
                (1, 20, 20, 3, 13), (1, 20, 20, 3, 1), (1, 10, 20, 3, 11), (1, 20, 10, 3, 11), (1, 46341, 46341, 1, 11),
                (1 << 30, 1 << 30, 1 << 30, 4, 11)):
        assert ws(*bad) == 0, bad


# ------------------------------------------------------------------------------------------ 3. flags, options, the model
def test_main_takes_the_flags_and_moves_no_default(capsys):
    sys.path.insert(0, ROOT)
    import main
    a = main.get_args([])
    assert a.ssim_weight == 0.0 and a.ssim_window == 11 and a.ssim_sigma == 1.5
    before = dict(vars(a))
    assert not any(k.startswith("ssim") for k in before)                   # a default run parses to the namespace it always did
    old = ["--dataset", "acdc", "--dice_weight", "0.5", "--boundary_loss", "0.1", "--batch_size", "4"]
    assert not any(k.startswith("ssim") for k in vars(main.get_args(old)))
    b = main.get_args(["--ssim_weight", "0.5", "--ssim_window", "7", "--ssim_sigma", "1.0"])
    assert b.ssim_weight == 0.5 and b.ssim_window == 7 and b.ssim_sigma == 1.0
    assert {k: v for k, v in vars(b).items() if not k.startswith("ssim")} == before
    assert main.get_args(["--ssim_weight", "0"]).ssim_weight == 0.0        # 0 means off
    for bad in (["--ssim_weight", "-0.1"], ["--ssim_weight", "nan"], ["--ssim_weight", "inf"], ["--ssim_weight", "x"],
                ["--ssim_window", "10"], ["--ssim_window", "1"], ["--ssim_window", "13"], ["--ssim_window", "5.0"],
                ["--ssim_sigma", "0"], ["--ssim_sigma", "-1"], ["--ssim_sigma", "nan"], ["--ssim_sigma", "inf"]):
        with pytest.raises(SystemExit):
            main.get_args(bad)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        main.get_args(["--help"])
    out = capsys.readouterr().out
    for flag in ("--ssim_weight", "--ssim_window", "--ssim_sigma"):
        assert flag in out and flag in main.__doc__


def test_options():
    F = load_sub("functional")
    o = F.SsimOptions()
    assert (o.window, o.sigma, o.data_range) == (11, 1.5, 2.0) and (o.c1, o.c2) == constants(2.0)
    o = F.SsimOptions(window=7, sigma=1, data_range=1.0)
    assert (o.window, o.sigma) == (7, 1.0) and o.c1 == pytest.approx(1e-4, rel=1e-15) and o.c2 == pytest.approx(9e-4, rel=1e-15)
    for bad in (dict(window=10), dict(window=1), dict(window=13), dict(window=5.5), dict(window=True), dict(sigma=0.0), dict(sigma=-2.0),
                dict(sigma=float("nan")), dict(sigma=float("inf")), dict(data_range=0.0), dict(data_range=float("nan"))):
        with pytest.raises(ValueError):
            F.SsimOptions(**bad)
    assert F._ssim_options(None).window == 11 and F._ssim_options({"window": 5}).window == 5 and F._ssim_options(o) is o
    with pytest.raises(TypeError):
        F._ssim_options(0.5)
    # no CPU fallback
    L = load_sub("_lib")
    x = torch.zeros(1, 3, 16, 16)
    for fn in (F.l1_ssim_loss, F.ssim_loss, F.ssim):
        with pytest.raises(L.SscgError):
            fn(x, x)


class _Driver(object):
    """semisuper_cycleGAN's image-loss options without its networks, which need the GPU."""

    def __new__(cls, md, crop=(64, 64), **kw):
        kind = type("Driver", (md.semisuper_cycleGAN,), {"__init__": lambda self: None})
        d = kind()
        d.args = types.SimpleNamespace(gpu_ids=[], **kw)
        d.crop = crop
        d._init_ssim(d.args)
        return d


def test_the_defaults_take_no_ssim_path(monkeypatch):
    md, F = load_sub("model"), load_sub("functional")
    assert md.LOSS_KEYS == ("img_dis_loss", "gt_dis_loss", "cycle_img_dis_loss", "img_gen_loss", "gt_gen_loss", "img_cycle_loss",
                            "gt_cycle_loss", "lab_loss_CE", "lab_loss_MSE")
    assert md.semisuper_cycleGAN.ssim_w == 0.0 and md.semisuper_cycleGAN.ssim_options is None
    monkeypatch.setattr(F, "l1_loss", lambda a, b: ("l1", a, b))
    monkeypatch.setattr(F, "l1_ssim_loss", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the fused term was called")))
    for kw in ({}, {"ssim_weight": 0.0}, {"ssim_weight": 0, "ssim_window": 7, "ssim_sigma": 1.0}, {"ssim_weight": None}):
        d = _Driver(md, **kw)
        assert d.ssim_options is None and d.ssim_w == 0.0
        extras, terms, weights = {}, [], []
        assert d._image_l1("p", "i", extras, "lab_loss_ssim", 1.0, terms, weights) == ("l1", "p", "i")
        assert extras == {} and terms == [] and weights == []
    monkeypatch.undo()
    # on
    d = _Driver(md, ssim_weight=0.5)
    assert d.ssim_w == 0.5 and (d.ssim_options.window, d.ssim_options.sigma, d.ssim_options.data_range) == (11, 1.5, 2.0)
    d = _Driver(md, crop=(9, 64), ssim_weight=2, ssim_window=9, ssim_sigma=2.0)
    assert d.ssim_w == 2.0 and (d.ssim_options.window, d.ssim_options.sigma) == (9, 2.0)
    seen = []
    monkeypatch.setattr(F, "l1_ssim_loss", lambda a, b, o: seen.append((a, b, o)) or ("l1", "ssim"))
    extras, terms, weights = {}, ["t"], [1.0]
    assert d._image_l1("p", "i", extras, "img_cycle_ssim", 0.5, terms, weights) == "l1"
    assert extras == {"img_cycle_ssim": "ssim"} and terms == ["t", "ssim"] and weights == [1.0, 1.0] and seen == [("p", "i", d.ssim_options)]
    for bad in (dict(ssim_weight=-1.0), dict(ssim_weight=float("nan")), dict(ssim_weight=float("inf")), dict(ssim_weight=1.0, ssim_window=8),
                dict(ssim_weight=1.0, ssim_window=13), dict(ssim_weight=1.0, ssim_window=1), dict(ssim_weight=1.0, ssim_sigma=0.0),
                dict(ssim_weight=1.0, ssim_sigma=-1.0)):
        with pytest.raises(ValueError):
            _Driver(md, **bad)
    with pytest.raises(ValueError) as e:
        _Driver(md, crop=(64, 8), ssim_weight=1.0, ssim_window=9)
    assert "crop" in str(e.value)
