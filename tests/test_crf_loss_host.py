"""The gated CRF loss (sscg_crf_loss_workspace / sscg_crf_loss_fwd; --unl_crf, --unl_crf_kernel) on a GPU-less host: the numpy
restatement (tests/crf_loss_reference.py) has the properties of the definition - the contract's gradient -2/M * msg equals the gradient
formed by scattering without any symmetry assumption and a central difference of the loss, the loss is >= 0 on rows that sum to 1,
exactly 0 on a constant one-hot map and does not depend on the order of the classes - the two entries are declared, exported and
bound, the C entry returns every argument error before any HIP call, the flags parse and refuse, the driver adds the term under the
ramp and the generator loss counts it."""
import ctypes as C
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import crf_loss_reference as LR
import crf_reference as R
from conftest import ROOT, load_sub

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
ONE = C.c_void_p(16)          # never dereferenced
NEW = ("sscg_crf_loss_workspace", "sscg_crf_loss_fwd")

# (N, OH, OW, C, IC, radius, dilation), seed: a window larger than the map among them
SMALL = [((2, 13, 17, 5, 3, 2, 1), 0), ((1, 9, 7, 3, 1, 3, 2), 1), ((1, 3, 5, 2, 3, 3, 2), 2), ((1, 12, 6, 4, 3, 5, 1), 3)]


def _inputs(geom, seed):
    N, OH, OW, Cn, IC, r, d = geom
    p, img = LR.case_inputs(seed, N, max(2, OH // 3), max(2, OW // 3), Cn, OH, OW, IC)
    return p, img, r, d


# ------------------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("pset", [R.STRONG, R.GENTLE], ids=["strong", "gentle"])
@pytest.mark.parametrize("geom,seed", SMALL)
def test_the_gradient_is_minus_two_over_m_times_the_message(geom, seed, pset):
    p, img, r, d = _inputs(geom, seed)
    ref = LR.crf_loss(p, img, r, d, np.float64, **pset)
    want = -2.0 / ref["M"] * ref["msg"]
    got = LR.scatter_grad(p, img, r, d, dt=np.float64, **pset)
    scale = float(np.abs(want).max())
    assert scale > 0 and float(np.abs(got - want).max()) <= 1e-12 * scale
    # the restatement's own weights agree with crf_reference's message (the gather half alone is msg)
    assert float(np.abs(ref["coef"] - want).max()) <= 1e-7 * scale          # coef carries s rounded to fp32
    # a central difference of the restated loss: the loss is quadratic in p, so the difference quotient is exact up to rounding
    rs = np.random.RandomState(seed + 50)
    h = 1e-3
    for _ in range(6):
        at = tuple(int(rs.randint(0, n)) for n in p.shape)
        lo, hi = p.astype(np.float64), p.astype(np.float64)
        lo[at] -= h
        hi[at] += h
        f = lambda q: LR.crf_loss(q, img, r, d, np.float64, **pset)["sums"][0] / ref["M"]
        cd = (f(hi) - f(lo)) / (2 * h)
        assert abs(cd - want[at]) <= 1e-9 * scale, (at, cd, want[at])


@pytest.mark.parametrize("geom,seed", SMALL)
def test_value_properties(geom, seed):
    p, img, r, d = _inputs(geom, seed)
    N, OH, OW, Cn = p.shape
    p64 = p.astype(np.float64)
    p64 /= p64.sum(axis=3, keepdims=True)
    ref = LR.crf_loss(p64, img, r, d, np.float64, **R.STRONG)
    # rows that sum to 1: e(i) = sum_j k(i, j) (1 - p(i) . p(j)) >= 0, pixel by pixel
    assert float(ref["e"].min()) >= -1e-12 * float(ref["ksum"].max()) and float(ref["loss"]) > 0.0
    assert 0.0 < ref["sums"][0] <= ref["sums"][1]
    # a constant one-hot map: exactly 0, in fp64 and in fp32 (k * 1 accumulated in the same order on both sides of the subtraction)
    for dt in (np.float64, np.float32):
        for hot in range(Cn):
            one = np.zeros((N, OH, OW, Cn), dtype=np.float32)
            one[..., hot] = 1.0
            z = LR.crf_loss(one, img, r, d, dt, **R.STRONG)
            assert float(z["loss"]) == 0.0 and z["sums"][0] == 0.0 and not z["e"].any()
            assert np.array_equal(z["msg"][..., hot], z["ksum"]) and not np.delete(z["msg"], hot, axis=3).any()
    # the order of the classes does not matter
    perm = np.random.RandomState(seed).permutation(Cn)
    alt = LR.crf_loss(p64[..., perm], img, r, d, np.float64, **R.STRONG)
    assert abs(alt["sums"][0] - ref["sums"][0]) <= 1e-12 * ref["sums"][1] and alt["sums"][1] == ref["sums"][1]
    assert float(np.abs(alt["coef"] - ref["coef"][..., perm]).max()) == 0.0
    # a uniform map under a single-colour image: e = ksum (1 - 1/C)
    flat = LR.crf_loss(np.full((N, OH, OW, Cn), 1.0 / Cn), np.zeros_like(img), r, d, np.float64, **R.STRONG)
    assert flat["sums"][0] == pytest.approx(flat["sums"][1] * (1.0 - 1.0 / Cn), rel=1e-12)


# ------------------------------------------------------------------------------------------ 2. the ABI
def test_the_entries_are_declared_exported_and_bound():
    L = load_sub("_lib")
    hdr = open(os.path.join(ROOT, "include", "sscg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "size_t sscg_crf_loss_workspace(int N, int OH, int OW);" in code
    assert ("int sscg_crf_loss_fwd(const float* p, int N, int OH, int OW, int C, const float* img, int IC, const sscg_crf_params* prm, "
            "float* loss,") in code
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sscg_[a-z0-9_]+)", out))
    for name in NEW:
        assert name in exported and name in L.SIGNATURES and callable(getattr(L.lib, name)), name
    assert [len(L.SIGNATURES[n][1]) for n in NEW] == [3, 14]
    fwd = L.SIGNATURES["sscg_crf_loss_fwd"][1]
    assert fwd[7] is C.POINTER(L.CrfParams) and fwd[12] is C.c_size_t and L.SIGNATURES["sscg_crf_loss_workspace"][0] is C.c_size_t
    assert L.ABI_VERSION == 18 and L.lib.sscg_abi_version() == 18 and "#define SSCG_ABI_VERSION 18" in hdr      # additions only
    # one record of two doubles per 16 x 16 tile
    ws = L.lib.sscg_crf_loss_workspace
    assert ws(2, 37, 45) == 2 * 3 * 3 * 16 and ws(1, 3, 5) == 16 and ws(8, 256, 256) == 8 * 256 * 16 and ws(1, 16, 17) == 2 * 16
    assert ws(0, 5, 5) == 0 and ws(1, 0, 5) == 0 and ws(1, 5, -1) == 0
    # the stream-ordering checker reads the header: the new entry is in its table with the kinds of its pointers
    table = L.dev_tool("racecheck").parse_header(os.path.join(ROOT, "include", "sscg.h"))
    kinds = dict(table["sscg_crf_loss_fwd"])
    assert [kinds[a] for a in ("p", "img", "prm")] == ["r"] * 3 and [kinds[a] for a in ("loss", "sums", "coef", "ws")] == ["w"] * 4
    assert kinds["stream"] == "stream" and len(table["sscg_crf_loss_fwd"]) == 14


def test_argument_errors_are_returned_before_any_launch():
    L = load_sub("_lib")
    lib = L.lib
    big = 1 << 30

    def prm(radius=3, dilation=2, iterations=5, wb=4.0, ws=3.0, ta=8.0, tb=0.5, tg=3.0):
        return L.CrfParams(radius, dilation, iterations, wb, ws, ta, tb, tg)

    def fwd(p=ONE, N=2, OH=13, OW=17, Cn=4, img=ONE, IC=3, pr=None, loss=ONE, sums=ONE, coef=ONE, ws=ONE, wsb=big, null_prm=False):
        pr = prm() if pr is None else pr
        return lib.sscg_crf_loss_fwd(p, N, OH, OW, Cn, img, IC, None if null_prm else C.byref(pr), loss, sums, coef, ws, wsb, None)

    assert fwd(p=None) == BAD_ARG and fwd(img=None) == BAD_ARG and fwd(null_prm=True) == BAD_ARG
    assert fwd(loss=None) == BAD_ARG and fwd(sums=None) == BAD_ARG
    assert fwd(N=0) == BAD_ARG and fwd(OH=0) == BAD_ARG and fwd(OW=-3) == BAD_ARG
    assert fwd(Cn=0) == BAD_ARG and fwd(Cn=65) == BAD_ARG and fwd(Cn=-1) == BAD_ARG and fwd(IC=0) == BAD_ARG and fwd(IC=5) == BAD_ARG
    assert fwd(pr=prm(radius=0)) == BAD_ARG and fwd(pr=prm(radius=6)) == BAD_ARG and fwd(pr=prm(dilation=0)) == BAD_ARG
    for w in (-0.5, float("nan"), float("inf")):
        assert fwd(pr=prm(wb=w)) == BAD_ARG and fwd(pr=prm(ws=w)) == BAD_ARG, w
    for t in (0.0, -1.0, float("nan"), 1e-30):                                       # 1 / (2 theta^2) must be a finite fp32 number
        assert fwd(pr=prm(ta=t)) == BAD_ARG and fwd(pr=prm(tb=t)) == BAD_ARG and fwd(pr=prm(tg=t)) == BAD_ARG, t
    assert fwd(pr=prm(radius=5, dilation=4)) == UNSUPPORTED and fwd(pr=prm(radius=4, dilation=4), ws=None) == WORKSPACE
    assert fwd(N=1, OH=46341, OW=46341, Cn=1) == UNSUPPORTED and fwd(N=1, OH=32768, OW=16384, Cn=4) == UNSUPPORTED     # N*OH*OW*C >= 2^31
    assert fwd(N=1, OH=46341, OW=46341, Cn=1, ws=None) == UNSUPPORTED               # ... before the workspace is looked at
    assert fwd(N=1, OH=46341, OW=46341, Cn=1, pr=prm(wb=-1.0)) == BAD_ARG           # ... after the arguments
    # the size is 2 * 1 * 2 tiles of 16 bytes; one byte short is refused, a null coef is the value-only call and no error of its own
    assert fwd(ws=None) == WORKSPACE and fwd(wsb=2 * 2 * 16 - 1) == WORKSPACE and fwd(coef=None, ws=None) == WORKSPACE
    for it in (-3, 0, 1 << 30):                                                     # iterations is ignored: never the reason of a refusal
        assert fwd(pr=prm(iterations=it), ws=None) == WORKSPACE


# ------------------------------------------------------------------------------------------ 3. flags, options, the driver
def test_main_takes_the_flags_and_moves_no_default(capsys):
    sys.path.insert(0, ROOT)
    import main
    F = load_sub("functional")
    a = main.get_args([])
    assert (a.unl_crf, a.unl_crf_kernel) == (0.0, "")
    before = dict(vars(a))
    assert not any(k.startswith("unl") for k in before)            # a default run parses to the namespace it always did
    b = main.get_args(["--unl_crf", "0.1", "--unl_crf_kernel", "iters=9,radius=2,dilation=3,wb=1,ws=0.5,alpha=4,beta=0.3,gamma=2"])
    assert b.unl_crf == 0.1 and {k: v for k, v in vars(b).items() if not k.startswith("unl")} == before
    U = load_sub("utils")
    o = U.parse_unl_crf_kernel(b.unl_crf_kernel)
    assert (o.radius, o.dilation, o.w_bilateral, o.w_spatial, o.theta_alpha, o.theta_beta, o.theta_gamma) == (2, 3, 1.0, 0.5, 4.0, 0.3, 2.0)
    assert U.parse_unl_crf_kernel("") == F.CrfOptions() and U.parse_unl_crf_kernel("on") == F.CrfOptions()
    assert main.get_args(["--unl_crf", "0"]).unl_crf == 0.0               # 0 means off
    assert main.get_args(["--unl_crf", "1", "--unl_ramp", "3", "--unl_entropy", "0.2"]).unl_ramp == 3
    for bad in (["--unl_crf", "-0.1"], ["--unl_crf", "nan"], ["--unl_crf", "inf"], ["--unl_crf", "x"], ["--unl_crf_kernel", "radius=2"],
                ["--unl_crf", "0", "--unl_crf_kernel", "on"], ["--unl_crf", "1", "--unl_crf_kernel", "radius=6"],
                ["--unl_crf", "1", "--unl_crf_kernel", "radius=5,dilation=4"], ["--unl_crf", "1", "--unl_crf_kernel", "wb=-1"],
                ["--unl_crf", "1", "--unl_crf_kernel", "beta=0"], ["--unl_crf", "1", "--unl_crf_kernel", "colour=3"]):
        with pytest.raises(SystemExit):
            main.get_args(bad)
    assert "--unl_crf_kernel" in capsys.readouterr().err               # the refusal names this flag, not --crf
    with pytest.raises(ValueError, match="--unl_crf_kernel"):
        U.parse_unl_crf_kernel("radius=9")
    with pytest.raises(SystemExit):
        main.get_args(["--help"])
    out = capsys.readouterr().out
    for flag in ("--unl_crf", "--unl_crf_kernel"):
        assert flag in out and flag in main.__doc__, flag
    assert "untuned" in out and "untuned" in F.crf_loss.__doc__.lower()


def test_crf_loss_validates_on_the_host():
    F, L = load_sub("functional"), load_sub("_lib")
    assert F._crf_loss_options(None) == F.CrfOptions() and F._crf_loss_options({"radius": 2}).radius == 2
    with pytest.raises(TypeError):
        F._crf_loss_options("on")
    with pytest.raises(ValueError):
        F._crf_loss_options({"radius": 7})
    with pytest.raises(L.SscgError):                                    # no CPU fallback
        F.crf_loss(torch.zeros(1, 4, 8, 8), torch.zeros(1, 3, 8, 8))


class _Driver(object):
    """The unlabelled-loss part of the semi-supervised driver (model._UnlabelledLosses) without its networks, which need the GPU."""

    def __new__(cls, md, **kw):
        d = type("Driver", (md._UnlabelledLosses,), {})()
        d.args = types.SimpleNamespace(gpu_ids=[], **kw)
        d.crop = (12, 12)
        d._init_unl(d.args)
        return d


def test_the_driver_adds_the_term_under_the_ramp(monkeypatch):
    md, F = load_sub("model"), load_sub("functional")
    soft, image = torch.zeros(2, 4, 12, 12), torch.zeros(2, 3, 12, 12)
    calls = []
    monkeypatch.setattr(F, "upsample_softmax_ce", lambda *a, **k: (soft, None))
    monkeypatch.setattr(F, "upsample_softmax_unl", lambda *a, **k: (soft, "E", "M", "P", {"sums": torch.zeros(4, dtype=torch.float64), "pseudo": None}))
    monkeypatch.setattr(F, "crf_loss", lambda *a, **k: calls.append((a, k)) or "CRF")
    # off: no call, no key, no term - and the kernel flag alone is refused
    for kw in ({}, dict(unl_crf=0.0), dict(unl_crf=0, unl_ramp=3)):
        d = _Driver(md, **kw)
        extras, terms, weights = {}, [], []
        assert d.unl_crf == 0.0 and d.unl_crf_options is None and d._unl_head("x", extras, terms, weights, image) is soft
        assert calls == [] and extras == {} and terms == [] and weights == [] and d.set_unl_epoch(1) == 1.0
    for bad in (dict(unl_crf=-1.0), dict(unl_crf=float("nan")), dict(unl_crf=float("inf")), dict(unl_crf_kernel="on"),
                dict(unl_crf=0.0, unl_crf_kernel="radius=2"), dict(unl_crf=1.0, unl_crf_kernel="radius=6"),
                dict(unl_crf=1.0, unl_ramp=-1)):
        with pytest.raises(ValueError):
            _Driver(md, **bad)
    # on, alone: the plain head, then the loss on its map under the unlabelled image, weight F * min(1, epoch / ramp)
    d = _Driver(md, unl_crf=0.4, unl_ramp=4, unl_crf_kernel="iters=7,radius=2,dilation=3")
    assert d.unl_options is None and d.unl_crf == 0.4 and d._unl_scale == 0.0
    assert (d.unl_crf_options.radius, d.unl_crf_options.dilation) == (2, 3)
    assert [d.set_unl_epoch(e) for e in (0, 1, 2, 4, 9)] == [0.0, 0.25, 0.5, 1.0, 1.0]
    d.set_unl_epoch(1)
    extras, terms, weights = {}, [], []
    assert d._unl_head("x", extras, terms, weights, image) is soft
    (a, k), = calls
    assert a[0] is soft and a[1] is image and a[2] is d.unl_crf_options and k == {}
    assert extras == {"unl_crf": "CRF"} and terms == ["CRF"] and weights == [0.4 * 0.25]
    assert _Driver(md, unl_crf=1.0).unl_crf_options == F.CrfOptions()
    with pytest.raises(ValueError, match="unlabelled image"):                # on, and no guide handed over: said in so many words
        d._unl_head("x", {}, [], [])
    # on, beside the other three: their terms first, each under its own key
    d = _Driver(md, unl_crf=0.5, unl_entropy=0.2, unl_pseudo=0.3)
    extras, terms, weights = {}, [], []
    d._unl_head("x", extras, terms, weights, image)
    assert terms == ["E", "P", "CRF"] and weights == [0.2, 0.3, 0.5]
    assert set(extras) == {"unl_entropy", "unl_pseudo_ce", "unl_pseudo_kept", "unl_crf"}
    assert issubclass(md.semisuper_cycleGAN, md._UnlabelledLosses) and not hasattr(md.supervised_model, "unl_crf")


def test_gen_loss_terms_counts_the_term():
    sys.path.insert(0, ROOT)
    import main
    md = load_sub("model")
    base = md.gen_loss_terms_of(main.get_args([]))
    assert base == md.GEN_LOSS_BASE_TERMS == 6
    assert md.gen_loss_terms_of(main.get_args(["--unl_crf", "0.1"])) == base + 1
    assert md.gen_loss_terms_of(main.get_args(["--unl_crf", "0"])) == base
    assert md.gen_loss_terms_of(main.get_args(["--unl_crf", "0.1", "--unl_crf_kernel", "radius=2", "--unl_ramp", "3"])) == base + 1
    every = ["--unl_entropy", "0.1", "--unl_maxsq", "0.1", "--unl_pseudo", "0.1"]
    assert md.gen_loss_terms_of(main.get_args(every)) == base + 3 and md.gen_loss_terms_of(main.get_args(every + ["--unl_crf", "2"])) == base + 4
    assert md.gen_loss_terms_of(types.SimpleNamespace(unl_crf=0.3, variants="l1_cycle", dice_weight=0.5)) == base + 1 + 1 + 2
    assert md.gen_loss_terms(unl=4) == base + 4
