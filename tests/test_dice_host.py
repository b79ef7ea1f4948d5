"""Soft Dice loss (sscg_dice_workspace / sscg_dice_fwd / sscg_dice_bwd / sscg_upsample_head_bwd_d, --dice_weight) on a GPU-less host:
the four entries are declared, exported and bound, the C entries return every argument error before any HIP call, the driver flags and
utils.dice_scores behave as documented, a model built with the defaults takes none of the new paths - and the closed form the kernels
implement (the (A, B) table, the softmax backward, the adjoint of the resize) equals torch's autograd of the definition in fp64.

`dice_reference` is the definition written with torch ops in fp64; tests/test_dice_gpu.py holds the kernels to it."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from conftest import ROOT, load_sub

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
ONE = C.c_void_p(16)          # never dereferenced
NEW = ("sscg_dice_workspace", "sscg_dice_fwd", "sscg_dice_bwd", "sscg_upsample_head_bwd_d")
GEOMS = [(2, 3, 4, 13, 17), (1, 1, 1, 5, 5), (2, 5, 5, 21, 23), (1, 2, 7, 9, 28)]       # N, H, W -> OH, OW; each OH*OW >= 16*H*W
CLASSES = [1, 4, 20, 21, 64]


def make_labels(g, shape, C, absent=True):
    """tests/test_weighted_ce_gpu.py's: ids in [0, C) - the last class never occurs when `absent` - with the void id 255 and torch's
    -100 sprinkled in; and, for a batch of two, sample 1 entirely void"""
    lab = torch.randint(0, C - 1 if (absent and C > 1) else C, shape, generator=g)
    flat = lab.view(-1)
    flat[::7] = 255
    flat[3::11] = -100
    if shape[0] == 2:
        lab[1] = 255
    return lab


def make_weights(g, C):
    """fp32 weights in [0.2, 1.2) with one class at 0 (C == 1: the one class keeps its weight - all-zero weights are refused)"""
    w = (torch.rand(C, generator=g) * 1.0 + 0.2).float()
    if C > 1:
        w[(C - 1) // 2] = 0.0
    return w


def dice_sums(p, lab):
    """(I, P, T, counted) per sample: [N, C] each, from probabilities p [N, C, H, W] and labels [N, H, W]"""
    C = p.shape[1]
    counted = ((lab >= 0) & (lab < C))
    onehot = TF.one_hot(torch.where(counted, lab, torch.zeros_like(lab)), C).permute(0, 3, 1, 2).to(p.dtype) * counted.unsqueeze(1)
    m = counted.unsqueeze(1).to(p.dtype)
    return (p * onehot).sum((2, 3)), (p * m).sum((2, 3)), onehot.sum((2, 3)), onehot


def dice_reference(x64, lab, w32=None, smooth=1.0, batch=False, resize=None):
    """The definition in fp64 on the CPU: F.interpolate(align_corners=True) -> softmax -> sums -> loss, gradient by autograd.
    Returns dict(loss, grad, sums [G, C, 3] = (I, P, T), dice [G, C], A, B [G, C])."""
    C = x64.shape[1]
    x = x64.clone().requires_grad_(True)
    up = x if resize is None else TF.interpolate(x, size=resize, mode="bilinear", align_corners=True)
    p = torch.softmax(up, 1)
    I, P, T, _ = dice_sums(p, lab)
    if batch:
        I, P, T = I.sum(0, keepdim=True), P.sum(0, keepdim=True), T.sum(0, keepdim=True)
    G = I.shape[0]
    w = torch.ones(C, dtype=torch.float64) if w32 is None else w32.double()
    num, den = 2 * I + smooth, P + T + smooth
    dice = num / den
    loss = 1 - (w * dice).sum() / (G * w.sum())
    grad = torch.autograd.grad(loss, x)[0]
    k = w / (G * w.sum())
    return dict(loss=loss.detach(), grad=grad, sums=torch.stack([I, P, T], 2).detach(), dice=dice.detach(),
                A=(-2 * k / den).detach(), B=(k * num / den ** 2).detach())


# ------------------------------------------------------------------------------------------ 1. the ABI
def test_the_four_entries_are_declared_exported_and_bound():
    import re
    import subprocess
    L = load_sub("_lib")
    hdr = open(os.path.join(ROOT, "include", "sscg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "size_t sscg_dice_workspace(int N, int OH, int OW, int C);" in code
    assert ("int sscg_dice_fwd(const float* x, const int64_t* labels, int N, int H, int W, int C, int OH, int OW, const float* class_w, "
            "float smooth,") in code
    assert "int sscg_dice_bwd(const float* x, const int64_t* labels, int N, int H, int W, int C, const float* coef, int batch, const float* g," in code
    assert ("int sscg_upsample_head_bwd_d(const float* x, const int64_t* labels, const float* dy_soft, const float* dlogits, "
            "const float* g_ce,") in code
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sscg_[a-z0-9_]+)", out))
    for name in NEW:
        assert name in exported and name in L.SIGNATURES and callable(getattr(L.lib, name)), name
    assert [len(L.SIGNATURES[n][1]) for n in NEW] == [4, 17, 12, 17]
    fwd = L.SIGNATURES["sscg_dice_fwd"][1]
    assert fwd[9] is C.c_float and fwd[10] is C.c_int and fwd[15] is C.c_size_t          # smooth, batch, ws_bytes
    assert L.SIGNATURES["sscg_dice_bwd"][1][7] is C.c_int and L.SIGNATURES["sscg_dice_bwd"][1][9] is C.c_float      # batch, w
    assert L.SIGNATURES["sscg_upsample_head_bwd_d"][1][8] is C.c_int                     # batch
    assert L.SIGNATURES["sscg_dice_workspace"][0] is C.c_size_t
    assert L.ABI_VERSION == 18 and L.lib.sscg_abi_version() == 18 and "#define SSCG_ABI_VERSION 18" in hdr      # additions only
    # the workspace: one fp64 record [C][3] per statistics block, at most 256 blocks per sample, and one per sample
    ws = L.lib.sscg_dice_workspace
    assert ws(2, 13, 17, 4) == 2 * (1 + 1) * 4 * 3 * 8 and ws(8, 256, 256, 21) == 8 * (256 + 1) * 21 * 3 * 8
    assert ws(1, 363, 363, 4) == (256 + 1) * 4 * 3 * 8 and ws(3, 150, 151, 4) == 3 * (89 + 1) * 4 * 3 * 8
    assert ws(0, 5, 5, 4) == 0 and ws(1, 5, 5, 0) == 0


def test_argument_errors_are_returned_before_any_launch():
    lib = load_sub("_lib").lib
    big = 1 << 30

    def fwd(x=ONE, lab=ONE, N=2, H=3, W=4, Cn=4, OH=13, OW=17, w=ONE, s=1.0, batch=0, loss=ONE, sums=ONE, coef=ONE, ws=ONE, wsb=big):
        return lib.sscg_dice_fwd(x, lab, N, H, W, Cn, OH, OW, w, s, batch, loss, sums, coef, ws, wsb, None)

    def bwd(x=ONE, lab=ONE, N=2, H=3, W=4, Cn=4, coef=ONE, batch=0, g=None, dx=ONE):
        return lib.sscg_dice_bwd(x, lab, N, H, W, Cn, coef, batch, g, 1.0, dx, None)

    def head(x=ONE, lab=ONE, dy=ONE, dl=ONE, g_ce=None, valid=ONE, coef=ONE, g_dice=None, batch=0, dx=ONE, N=2, H=3, W=4, Cn=4, OH=13, OW=17):
        return lib.sscg_upsample_head_bwd_d(x, lab, dy, dl, g_ce, valid, coef, g_dice, batch, dx, N, H, W, Cn, OH, OW, None)

    for call in (fwd, bwd, head):
        assert call(x=None) == BAD_ARG and call(lab=None) == BAD_ARG and call(coef=None) == BAD_ARG, call.__name__
        assert call(Cn=0) == BAD_ARG and call(Cn=65) == BAD_ARG and call(Cn=-1) == BAD_ARG
        assert call(N=0) == BAD_ARG and call(H=0) == BAD_ARG and call(W=-3) == BAD_ARG
        assert call(batch=2) == BAD_ARG and call(batch=-1) == BAD_ARG
    for s in (0.0, -1.0, float("nan"), float("inf")):
        assert fwd(s=s) == BAD_ARG, s
    assert fwd(loss=None) == BAD_ARG and fwd(OH=0) == BAD_ARG and fwd(OW=-1) == BAD_ARG
    assert fwd(ws=None) == WORKSPACE and fwd(wsb=2 * 2 * 4 * 3 * 8 - 1) == WORKSPACE
    assert fwd(N=1, H=1, W=1, OH=46341, OW=46341) == UNSUPPORTED                   # N * OH * OW >= 2^31
    assert fwd(N=1, H=1, W=1, OH=46341, OW=46341, ws=None) == UNSUPPORTED          # ... before the workspace is looked at
    assert fwd(N=1, H=1, W=1, OH=46341, OW=46341, s=0.0) == BAD_ARG                # ... after the arguments
    assert bwd(dx=None) == BAD_ARG and bwd(N=1, H=46341, W=46341) == UNSUPPORTED
    assert head(dx=None) == BAD_ARG and head(OH=0) == BAD_ARG
    assert head(valid=None) == BAD_ARG                                              # dlogits without valid
    assert head(N=1, H=1, W=1, OH=46341, OW=46341) == UNSUPPORTED
    # sums, class weights, the upstream scalars and the two other branches of the head are optional: the error (if any) is not theirs
    assert fwd(sums=None, w=None, ws=None) == WORKSPACE and head(dy=None, dl=None, valid=None, x=None) == BAD_ARG


# ------------------------------------------------------------------------------------------ 2. flags, scores, options
def test_main_takes_the_dice_flags_and_moves_no_default(capsys):
    sys.path.insert(0, ROOT)
    import main
    a = main.get_args([])
    assert a.dice_weight == 0.0 and a.dice_smooth == 1.0 and a.dice_skip == "" and a.dice_batch is False
    before = dict(vars(a))
    assert not any(k.startswith("dice") for k in before)          # a default run parses to the namespace it always did
    old = ["--dataset", "acdc", "--ce_weights", "median", "--tta", "0.5,1.0:flip", "--batch_size", "4"]
    assert not any(k.startswith("dice") for k in vars(main.get_args(old)))
    b = main.get_args(["--dice_weight", "0.5", "--dice_smooth", "1e-5", "--dice_skip", "0, 3", "--dice_batch"])
    assert b.dice_weight == 0.5 and b.dice_smooth == 1e-5 and b.dice_skip == "0, 3" and b.dice_batch is True
    rest = {k: v for k, v in vars(b).items() if not k.startswith("dice")}
    assert rest == before
    assert main.get_args(["--dice_weight", "0"]).dice_weight == 0.0            # 0 means off
    for bad in (["--dice_weight", "-0.1"], ["--dice_weight", "nan"], ["--dice_weight", "inf"], ["--dice_weight", "x"],
                ["--dice_smooth", "0"], ["--dice_smooth", "-1"], ["--dice_smooth", "nan"], ["--dice_smooth", "inf"],
                ["--dice_skip", "21"], ["--dice_skip", "-1"], ["--dice_skip", "a"], ["--dice_skip", "0,,1"],
                ["--dataset", "acdc", "--dice_skip", "4"], ["--dataset", "acdc", "--dice_skip", "0,1,2,3"]):
        with pytest.raises(SystemExit):
            main.get_args(bad)
    capsys.readouterr()
    assert main.get_args(["--dataset", "cityscapes", "--dice_skip", "19"]).dice_skip == "19"
    for flag in ("--dice_weight", "--dice_smooth", "--dice_skip", "--dice_batch"):
        with pytest.raises(SystemExit):
            main.get_args(["--help"])
        assert flag in capsys.readouterr().out


def test_dice_skip_gives_the_weight_list():
    U, F = load_sub("utils"), load_sub("functional")
    assert U.parse_dice_skip("", 4) == [] and U.parse_dice_skip(None, 21) == [] and U.parse_dice_skip("  ", 4) == []
    assert U.parse_dice_skip("0", 21) == [0] and U.parse_dice_skip("19", 20) == [19] and U.parse_dice_skip("3, 0,3", 4) == [0, 3]
    for bad, token in (("4", "'4'"), ("-1", "'-1'"), ("a", "'a'"), ("0,,1", "''"), ("1.5", "'1.5'"), ("0,1,2,3", "every class")):
        with pytest.raises(ValueError) as e:
            U.parse_dice_skip(bad, 4)
        assert token in str(e.value), (bad, str(e.value))
    cpu = torch.device("cpu")
    w = F.dice_weight([0.0 if c in U.parse_dice_skip("0,3", 4) else 1.0 for c in range(4)], 4, cpu)
    assert w.dtype == torch.float32 and w.tolist() == [0.0, 1.0, 1.0, 0.0]
    for bad in ([1, 2, 3], [1, -1, 1, 1], [1, float("nan"), 1, 1], [1, float("inf"), 1, 1], [0, 0, 0, 0]):
        with pytest.raises(ValueError):
            F.dice_weight(bad, 4, cpu)


def test_dice_scores_by_hand():
    U = load_sub("utils")
    h = np.array([[5, 1, 0, 0],          # rows: true class, columns: predicted
                  [2, 3, 0, 0],
                  [0, 0, 0, 0],          # class 2: in neither the labels nor the predictions
                  [1, 0, 0, 0]])         # class 3: labelled, never predicted
    got = U.dice_scores(h)
    tp, fp, fn = np.diag(h), h.sum(0) - np.diag(h), h.sum(1) - np.diag(h)
    with np.errstate(invalid="ignore"):
        want = 2.0 * tp / (2.0 * tp + fp + fn)
    assert got.shape == (4,) and np.isnan(got[2]) and np.isnan(want[2]) and got[3] == 0.0
    assert got[[0, 1, 3]] == pytest.approx([10 / 14, 6 / 9, 0.0], rel=1e-15) and np.allclose(got, want, rtol=1e-15, atol=0, equal_nan=True)
    # through runningScore: the class dropping of get_scores()
    for dataset, keep in (("acdc", [0, 1, 2, 3]), ("voc2012", [1, 2, 3]), ("cityscapes", [0, 1, 2])):
        rs = U.runningScore(4, dataset)
        rs.confusion_matrix += h
        d = rs.get_dice()
        sub = h[np.ix_(keep, keep)]
        want = U.dice_scores(sub)
        assert list(d["class_dice"]) == list(range(len(keep)))
        assert np.allclose(list(d["class_dice"].values()), want, equal_nan=True) and d["mean_dice"] == pytest.approx(np.nanmean(want))
        assert len(rs.get_scores()[1]) == len(keep)                     # the same classes as the IoU


class _Driver(object):
    """The loss-option part of both drivers (model._WeightedCE) without their networks, which need the GPU."""

    def __new__(cls, md, **kw):
        kind = type("Driver", (md._WeightedCE,), {})
        d = kind()
        d.args = types.SimpleNamespace(gpu_ids=[], **kw)
        d.dp, d.n_channels, d.crop = None, 4, (12, 12)
        d._init_ce(d.args, 4)
        return d


def test_the_defaults_take_no_dice_path(monkeypatch, capsys):
    md, F, L = load_sub("model"), load_sub("functional"), load_sub("_lib")
    seen = []
    monkeypatch.setattr(F, "upsample_softmax_ce", lambda *a, **k: seen.append((a, k)) or ("soft", "ce"))
    monkeypatch.setattr(F, "upsample_softmax_ce_dice", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the Dice head was called")))
    for kw in ({}, {"dice_weight": 0.0}, {"dice_weight": 0, "dice_skip": "0", "dice_batch": True, "dice_smooth": 1e-5}):
        d = _Driver(md, **kw)
        assert d.dice_options is None and d.dice_w == 0.0
        assert d._head("x", "lab", False) == ("soft", "ce", None) and seen[-1] == (("x", (12, 12), "lab"), {"want_soft": False})
        d._dice_scores(None)
        assert not hasattr(d, "eval_dice")
    assert capsys.readouterr().out == ""
    monkeypatch.undo()
    d = _Driver(md, dice_weight=0.5, dice_skip="0,3", dice_smooth=0.25, dice_batch=True)
    o = d.dice_options
    assert d.dice_w == 0.5 and o.weight.tolist() == [0.0, 1.0, 1.0, 0.0] and o.smooth == 0.25 and o.batch is True and o.ce is True
    o = _Driver(md, dice_weight=2).dice_options
    assert o.weight is None and o.smooth == 1.0 and o.batch is False
    for bad in ({"dice_weight": -1.0}, {"dice_weight": float("nan")}, {"dice_weight": 1.0, "dice_smooth": 0.0},
                {"dice_weight": 1.0, "dice_smooth": float("nan")}, {"dice_weight": 1.0, "dice_skip": "4"},
                {"dice_weight": 1.0, "dice_skip": "0,1,2,3"}):
        with pytest.raises(ValueError):
            _Driver(md, **bad)
    # no CPU fallback
    x, lab = torch.zeros(1, 4, 3, 3), torch.zeros(1, 3, 3, dtype=torch.int64)
    with pytest.raises(L.SscgError):
        F.dice_loss(x, lab)
    with pytest.raises(L.SscgError):
        F.upsample_softmax_ce_dice(x, (12, 12), torch.zeros(1, 12, 12, dtype=torch.int64))
    cpu = torch.device("cpu")
    for s in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            F._dice_options(None, s, False, 4, cpu)
    w = F.dice_weight([1, 0, 2, 1], 4, cpu)
    assert F._dice_options(w, 1e-5, True, 4, cpu) == (w, 1e-5, 1) and F._dice_options(None, 1, False, 4, cpu) == (None, 1.0, 0)
    with pytest.raises(L.SscgError):
        F._dice_options(w, 1.0, False, 5, cpu)
    with pytest.raises(L.SscgError):
        F._dice_options(w.double(), 1.0, False, 4, cpu)
    assert F.upsample_softmax_ce.__defaults__ == (None, True, None, 0.0)        # the plain head keeps its signature


# ------------------------------------------------------------------------------------------ 3. the closed form
@pytest.mark.parametrize("C", CLASSES)
def test_closed_form_equals_autograd_of_the_definition(C):
    """g_c = A [y == c] + B on the counted pixels, dz = p (g - sum p g), then F.interpolate's adjoint - what the kernels compute - against
    torch's autograd of the definition, both in fp64."""
    worst = 0.0
    for (N, H, W, OH, OW) in GEOMS:
        g = torch.Generator().manual_seed(50 * C + H * W)
        x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 2
        lab = make_labels(g, (N, OH, OW), C)
        assert (lab == 255).any() and (C == 1 or not (lab == C - 1).any())
        wts = make_weights(g, C)
        for batch in (False, True):
            for s in (1.0, 1e-5):
                for w32 in (None, wts):
                    ref = dice_reference(x, lab, w32, s, batch, resize=(OH, OW))
                    xr = x.clone().requires_grad_(True)
                    up = TF.interpolate(xr, size=(OH, OW), mode="bilinear", align_corners=True)
                    p = torch.softmax(up.detach(), 1)
                    _, _, _, onehot = dice_sums(p, lab)
                    counted = ((lab >= 0) & (lab < C)).unsqueeze(1).double()
                    A = ref["A"].expand(N, C)[:, :, None, None]
                    B = ref["B"].expand(N, C)[:, :, None, None]
                    gp = (A * onehot + B) * counted
                    dz = p * (gp - (p * gp).sum(1, keepdim=True))
                    dx = torch.autograd.grad(up, xr, grad_outputs=dz)[0]
                    worst = max(worst, float((dx - ref["grad"]).abs().max()))
                    if N == 2:                                              # the void-only sample
                        assert torch.count_nonzero(ref["grad"][1]) == 0 and torch.count_nonzero(dx[1]) == 0
                        if not batch:
                            assert torch.equal(ref["dice"][1], torch.ones(C, dtype=torch.float64))
                    assert torch.isfinite(ref["loss"]) and (ref["sums"][:, :, 1] + ref["sums"][:, :, 2] + s > 0).all()
    print("dice closed form C=%d: max |closed form - autograd| %.2e" % (C, worst))
    assert worst <= 1e-12
