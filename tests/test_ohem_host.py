"""Hard-pixel mining (OHEM) cross entropy (sscg_ohem_workspace / sscg_ohem_fwd / sscg_ce_bwd_ohem / sscg_upsample_head_bwd_h,
--ohem_thresh) on a GPU-less host: the four entries are declared, exported and bound with the const-ness the stream checker reads, the
C entries return every argument error before any HIP call, the options and driver flags behave as documented, a model built with the
defaults takes none of the new paths - and `ohem_reference`, the definition written with torch ops in fp64 (F.interpolate(align_corners=
True) -> softmax -> kthvalue -> masked loss, gradient by autograd with the mask held constant), agrees with a sort and with torch's own
cross entropy once every pixel that is not kept is mapped to the ignore index.  tests/test_ohem_gpu.py holds the kernels to it."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from conftest import ROOT, load_sub

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
ONE = C.c_void_p(16)          # never dereferenced
NEW = ("sscg_ohem_workspace", "sscg_ohem_fwd", "sscg_ce_bwd_ohem", "sscg_upsample_head_bwd_h")
GEOMS = [(2, 5, 7, 40, 56), (2, 9, 9, 65, 65), (2, 24, 24, 24, 24)]          # N, H, W -> OH, OW; the last one is flat
CLASSES = [4, 21, 64]
SELECT = [(0.7, 1, 0.0), (0.05, 1000, 0.0), (0.3, 0, 0.5)]                    # (thresh, min_kept, min_frac); the first is thresh-dominated
# With logits randn * 2 a key is of the order of a few / C: at C = 21 and 64 the threshold 0.7 lies above 93 % .. 99.97 % of the keys, so
# there SELECT[0] is thresh-dominated but keeps nearly everything.  Those class counts get one more thresh-dominated selection, at the
# scale of their keys, so that every C has one whose kept share lies in (0.1, 0.9).
THETA_MID = {4: 0.7, 21: 0.2, 64: 0.1}


def selections(Cn):
    return SELECT + ([] if THETA_MID[Cn] == SELECT[0][0] else [(THETA_MID[Cn], 1, 0.0)])


HEAD_BYTES = 3 * 1024 * 4 + 256 + 3 * 1024 * 8                               # tables, state, records: what the workspace holds beside `term`


def f32(v):
    return float(np.float32(v))


def make_case(seed, N, C, H, W, OH, OW):
    """logits randn * 2 (fp64); labels = the argmax of the fp64 resized logits on ~70 % of the pixels, random elsewhere, ~10 % void (255
    and -100)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 2
    up = x if (OH, OW) == (H, W) else TF.interpolate(x, size=(OH, OW), mode="bilinear", align_corners=True)
    lab = up.argmax(1)
    rnd = torch.randint(0, C, lab.shape, generator=g)
    u = torch.rand(lab.shape, generator=g)
    lab = torch.where(u < 0.3, rnd, lab)
    v = torch.rand(lab.shape, generator=g)
    lab = torch.where(v < 0.05, torch.full_like(lab, 255), lab)
    lab = torch.where((v >= 0.05) & (v < 0.10), torch.full_like(lab, -100), lab)
    return x, lab


def make_weights(seed, C):
    """fp32 weights in [0.2, 1.2) with one class at 0"""
    g = torch.Generator().manual_seed(seed)
    w = (torch.rand(C, generator=g) + 0.2).float()
    if C > 1:
        w[(C - 1) // 2] = 0.0
    return w


def ohem_rank(V, K, f):
    """r = clamp(max(K, ceil(f * V)), 1, V), the product in fp64 from the fp32 f"""
    return min(max(int(K), int(math.ceil(f32(f) * V)), 1), V)


def ohem_reference(x64, lab, w32=None, eps=0.0, thresh=0.7, min_kept=0, min_frac=0.0, resize=None, mask=None):
    """The definition (include/sscg.h, sscg_ohem_fwd) in fp64 on the CPU.  mask: evaluate loss and gradient with THIS keep mask (teacher
    forcing) instead of the reference's own.  Returns dict(loss, grad, keys [N, OH, OW] (2.0 where not counted), counted, V, r, m, tau,
    mask, kept, D).  thresh and min_frac are the fp32 values the C entry receives."""
    Cn = x64.shape[1]
    x = x64.clone().requires_grad_(True)
    up = x if resize is None else TF.interpolate(x, size=resize, mode="bilinear", align_corners=True)
    logp = torch.log_softmax(up, 1)
    counted = (lab >= 0) & (lab < Cn)
    safe = torch.where(counted, lab, torch.zeros_like(lab))
    lp_y = logp.gather(1, safe.unsqueeze(1)).squeeze(1)
    k = torch.softmax(up.detach(), 1).gather(1, safe.unsqueeze(1)).squeeze(1)
    keys = torch.where(counted, k, torch.full_like(k, 2.0))
    V = int(counted.sum())
    r = m = None
    tau = f32(thresh)
    if V:
        r = ohem_rank(V, min_kept, min_frac)
        m = float(torch.kthvalue(k[counted], r).values)
        tau = max(m, tau)
    own = counted & (k <= tau)
    keep = own if mask is None else (mask & counted)
    w = torch.ones(Cn, dtype=torch.float64) if w32 is None else w32.double()
    term = (1 - eps) * w[safe] * (-lp_y) + (eps / Cn) * (w.view(1, Cn, 1, 1) * (-logp)).sum(1)
    D = float((w[safe] * keep).sum())
    if D > 0:
        loss = (term * keep).sum() / D
        grad = torch.autograd.grad(loss, x)[0]
        loss = loss.detach()
    else:
        loss, grad = torch.tensor(float("nan"), dtype=torch.float64), torch.zeros_like(x64)
    return dict(loss=loss, grad=grad, keys=keys, counted=counted, V=V, r=r, m=m, tau=tau, mask=own, kept=int(keep.sum()), D=D)


# ------------------------------------------------------------------------------------------ 1. the ABI
def test_the_four_entries_are_declared_exported_and_bound():
    L = load_sub("_lib")
    hdr = open(os.path.join(ROOT, "include", "sscg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "size_t sscg_ohem_workspace(int N, int OH, int OW);" in code
    assert ("int sscg_ohem_fwd(const float* x, const int64_t* labels, int N, int H, int W, int C, int OH, int OW, const float* class_w, "
            "float smoothing,") in code
    assert "float thresh, int64_t min_kept, float min_frac, float* keys, float* loss, float* valid, float* thr, int64_t* counts," in code
    assert "int sscg_ce_bwd_ohem(const float* logits, const int64_t* labels, const float* keys, const float* thr, int64_t rows, int C," in code
    assert "int sscg_upsample_head_bwd_h(const float* x, const int64_t* labels, const float* keys, const float* thr, const float* class_w," in code
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sscg_[a-z0-9_]+)", out))
    for name in NEW:
        assert name in exported and name in L.SIGNATURES and callable(getattr(L.lib, name)), name
    assert [len(L.SIGNATURES[n][1]) for n in NEW] == [3, 21, 13, 20]
    fwd = L.SIGNATURES["sscg_ohem_fwd"][1]
    assert fwd[9] is C.c_float and fwd[10] is C.c_float and fwd[11] is C.c_int64 and fwd[12] is C.c_float and fwd[19] is C.c_size_t
    assert L.SIGNATURES["sscg_ce_bwd_ohem"][1][4] is C.c_int64 and L.SIGNATURES["sscg_ce_bwd_ohem"][1][7] is C.c_float
    assert L.SIGNATURES["sscg_upsample_head_bwd_h"][1][5] is C.c_float and L.SIGNATURES["sscg_upsample_head_bwd_h"][1][11] is C.c_int
    assert L.SIGNATURES["sscg_ohem_workspace"][0] is C.c_size_t
    assert L.ABI_VERSION == 18 and L.lib.sscg_abi_version() == 18 and "#define SSCG_ABI_VERSION 18" in hdr      # additions only
    # the workspace: the tables, the state, the loss records, and ONE fp32 per output pixel (term) - keys is the caller's other map
    ws = L.lib.sscg_ohem_workspace
    assert ws(2, 40, 56) == HEAD_BYTES + 2 * 40 * 56 * 4 and ws(8, 256, 256) == HEAD_BYTES + 8 * 256 * 256 * 4
    assert ws(0, 5, 5) == 0 and ws(1, 0, 5) == 0 and ws(1, 5, -1) == 0
    # the header says why the comparison is <= where HRNet's and mmsegmentation's is <
    assert "<= on purpose" in hdr and "HRNet" in hdr and "0 / 0" in hdr


def test_the_stream_checker_reads_the_const_qualifiers():
    """tools/racecheck.py derives reads / writes from the header: inputs (keys and thr in the backwards) read, outputs written."""
    rc = load_sub("_lib").dev_tool("racecheck")
    tab = rc.parse_header(os.path.join(ROOT, "include", "sscg.h"))
    for name in NEW:
        assert name in tab and len(tab[name]) == len(load_sub("_lib").SIGNATURES[name][1]), name
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sscg.h")).read(), flags=re.S)

    def params(name):
        body = re.search(r"\b%s\((.*?)\);" % name, hdr, flags=re.S).group(1)
        return {p.split()[-1].lstrip("*"): p for p in (" ".join(q.split()) for q in body.split(","))}
    p = params("sscg_ohem_fwd")
    assert all(p[k].startswith("const ") for k in ("x", "labels", "class_w"))
    assert all(not p[k].startswith("const ") and "*" in p[k] for k in ("keys", "loss", "valid", "thr", "counts", "ws"))
    for name, outs in (("sscg_ce_bwd_ohem", ("dx",)), ("sscg_upsample_head_bwd_h", ("dx",))):
        p = params(name)
        for k, decl in p.items():
            if "*" in decl and k != "stream":
                assert decl.startswith("const ") == (k not in outs), (name, decl)


def test_argument_errors_are_returned_before_any_launch():
    lib = load_sub("_lib").lib
    big = 1 << 40
    nan = float("nan")

    def fwd(x=ONE, lab=ONE, N=2, H=5, W=7, Cn=4, OH=40, OW=56, w=ONE, eps=0.0, th=0.7, K=0, f=0.0, keys=ONE, loss=ONE, valid=ONE, thr=ONE,
            counts=ONE, ws=ONE, wsb=big):
        return lib.sscg_ohem_fwd(x, lab, N, H, W, Cn, OH, OW, w, eps, th, K, f, keys, loss, valid, thr, counts, ws, wsb, None)

    def bwd(x=ONE, lab=ONE, keys=ONE, thr=ONE, rows=100, Cn=4, w=ONE, eps=0.0, g=None, valid=ONE, dx=ONE):
        return lib.sscg_ce_bwd_ohem(x, lab, keys, thr, rows, Cn, w, eps, g, 1.0, valid, dx, None)

    def head(x=ONE, lab=ONE, keys=ONE, thr=ONE, w=ONE, eps=0.0, dy=ONE, g_ce=None, valid=ONE, coef=ONE, g_dice=None, batch=0, dx=ONE, N=2, H=5,
             W=7, Cn=4, OH=40, OW=56):
        return lib.sscg_upsample_head_bwd_h(x, lab, keys, thr, w, eps, dy, g_ce, valid, coef, g_dice, batch, dx, N, H, W, Cn, OH, OW, None)

    for call in (fwd, bwd, head):
        assert call(x=None) == BAD_ARG and call(lab=None) == BAD_ARG, call.__name__
        assert call(Cn=0) == BAD_ARG and call(Cn=65) == BAD_ARG and call(Cn=-1) == BAD_ARG
        for eps in (-0.1, 1.0, 1.5, nan):
            assert call(eps=eps) == BAD_ARG, (call.__name__, eps)
    for kw in (dict(N=0), dict(H=0), dict(W=-3), dict(OH=0), dict(OW=-1)):
        assert fwd(**kw) == BAD_ARG and head(**kw) == BAD_ARG, kw
    for out in ("keys", "loss", "valid", "thr", "counts"):
        assert fwd(**{out: None}) == BAD_ARG, out
    for th in (0.0, -0.5, 1.0000001, 2.0, nan, float("inf")):
        assert fwd(th=th) == BAD_ARG, th
    assert fwd(th=1.0, ws=None) == WORKSPACE and fwd(th=1e-6, ws=None) == WORKSPACE          # the ends of (0, 1]
    for K in (-1, -(1 << 40)):
        assert fwd(K=K) == BAD_ARG, K
    assert fwd(K=1 << 40, ws=None) == WORKSPACE                                                 # any K >= 0 is clamped on the device
    for f in (-0.01, 1.01, nan, float("inf")):
        assert fwd(f=f) == BAD_ARG, f
    assert fwd(f=0.0, ws=None) == WORKSPACE and fwd(f=1.0, ws=None) == WORKSPACE
    assert fwd(w=None, ws=None) == WORKSPACE                                                    # class weights are optional
    assert fwd(ws=None) == WORKSPACE and fwd(wsb=HEAD_BYTES + 2 * 40 * 56 * 4 - 1) == WORKSPACE
    assert fwd(N=1, H=1, W=1, OH=46341, OW=46341) == UNSUPPORTED                   # N * OH * OW >= 2^31
    assert fwd(N=1, H=1, W=1, OH=46341, OW=46341, ws=None) == UNSUPPORTED          # ... before the workspace is looked at
    assert fwd(N=1, H=1, W=1, OH=46341, OW=46341, th=0.0) == BAD_ARG               # ... after the arguments
    assert bwd(keys=None) == BAD_ARG and bwd(thr=None) == BAD_ARG and bwd(valid=None) == BAD_ARG and bwd(dx=None) == BAD_ARG
    assert bwd(rows=0) == BAD_ARG and bwd(rows=-5) == BAD_ARG and bwd(rows=1 << 31) == UNSUPPORTED
    assert head(dx=None) == BAD_ARG and head(batch=2) == BAD_ARG and head(batch=-1) == BAD_ARG
    assert head(thr=None) == BAD_ARG and head(valid=None) == BAD_ARG              # keys without thr / valid
    assert head(keys=None, dy=None, coef=None) == BAD_ARG                         # no live branch
    assert head(N=1, H=1, W=1, OH=46341, OW=46341) == UNSUPPORTED
    # each branch alone is a legal call: the error (if any) is not theirs
    assert head(keys=None, thr=None, valid=None, coef=None, lab=None, x=None) == BAD_ARG
    assert head(keys=None, thr=None, valid=None, dy=None, dx=None) == BAD_ARG and head(dy=None, coef=None, dx=None) == BAD_ARG


# ------------------------------------------------------------------------------------------ 2. options and flags
def test_ohem_options_check_their_arguments():
    F, L = load_sub("functional"), load_sub("_lib")
    o = F.OhemOptions(0.7)
    assert (o.thresh, o.min_kept, o.min_frac) == (0.7, 0, 0.0)
    o = F.OhemOptions(1, min_kept=100000, min_frac=1)
    assert (o.thresh, o.min_kept, o.min_frac) == (1.0, 100000, 1.0) and isinstance(o.min_kept, int)
    assert F.OhemOptions(0.5, 3.0).min_kept == 3
    for bad in (dict(thresh=0.0), dict(thresh=-1.0), dict(thresh=1.5), dict(thresh=float("nan")), dict(thresh=0.5, min_kept=-1),
                dict(thresh=0.5, min_kept=2.5), dict(thresh=0.5, min_kept=1 << 63), dict(thresh=0.5, min_frac=-0.1),
                dict(thresh=0.5, min_frac=1.1), dict(thresh=0.5, min_frac=float("nan"))):
        with pytest.raises(ValueError):
            F.OhemOptions(**bad)
    assert F._ohem_options({"thresh": 0.25, "min_frac": 0.5}).min_frac == 0.5 and F._ohem_options(o) is o
    with pytest.raises(TypeError):
        F._ohem_options(0.7)
    # the option is keyword-only everywhere: every positional signature is the one it was
    assert F.upsample_softmax_ce.__defaults__ == (None, True, None, 0.0) and F.upsample_softmax_ce.__kwdefaults__ == {"ohem": None}
    assert F.upsample_softmax_ce_dice.__kwdefaults__ == {"ohem": None} and F.cross_entropy.__kwdefaults__ == {"ohem": None}
    assert F.ohem_stats() is None or len(F.ohem_stats()) == 3
    # no CPU fallback
    x, lab = torch.zeros(1, 4, 3, 3), torch.zeros(1, 3, 3, dtype=torch.int64)
    with pytest.raises(L.SscgError):
        F.cross_entropy(x, lab, ohem=o)
    with pytest.raises(L.SscgError):
        F.upsample_softmax_ce(x, (12, 12), torch.zeros(1, 12, 12, dtype=torch.int64), ohem=o)
    with pytest.raises(ValueError):
        F.upsample_softmax_ce_dice(x, (12, 12), torch.zeros(1, 12, 12, dtype=torch.int64), dice=F.DiceOptions(ce=False), ohem=o)


def test_main_takes_the_ohem_flags_and_moves_no_default(capsys):
    sys.path.insert(0, ROOT)
    import main
    a = main.get_args([])
    assert a.ohem_thresh is None and a.ohem_min_kept == 0 and a.ohem_min_frac == 0.0625
    before = dict(vars(a))
    assert not any(k.startswith("ohem") for k in before)          # a default run parses to the namespace it always did
    old = ["--dataset", "acdc", "--ce_weights", "median", "--dice_weight", "0.5", "--batch_size", "4"]
    assert not any(k.startswith("ohem") for k in vars(main.get_args(old)))
    b = main.get_args(["--ohem_thresh", "0.7", "--ohem_min_kept", "100000", "--ohem_min_frac", "0.25"])
    assert b.ohem_thresh == 0.7 and b.ohem_min_kept == 100000 and b.ohem_min_frac == 0.25
    assert {k: v for k, v in vars(b).items() if not k.startswith("ohem")} == before
    c = main.get_args(["--ohem_thresh", "1.0"])
    assert c.ohem_thresh == 1.0 and c.ohem_min_kept == 0 and c.ohem_min_frac == 0.0625
    for bad in (["--ohem_thresh", "0"], ["--ohem_thresh", "-0.1"], ["--ohem_thresh", "1.01"], ["--ohem_thresh", "nan"], ["--ohem_thresh", "x"],
                ["--ohem_thresh", "0.7", "--ohem_min_kept", "-1"], ["--ohem_thresh", "0.7", "--ohem_min_kept", "1.5"],
                ["--ohem_thresh", "0.7", "--ohem_min_frac", "-0.1"], ["--ohem_thresh", "0.7", "--ohem_min_frac", "1.5"],
                ["--ohem_thresh", "0.7", "--ohem_min_frac", "nan"], ["--ohem_min_kept", "10"], ["--ohem_min_frac", "0.5"]):
        with pytest.raises(SystemExit):
            main.get_args(bad)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        main.get_args(["--help"])
    out = capsys.readouterr().out
    for flag in ("--ohem_thresh", "--ohem_min_kept", "--ohem_min_frac"):
        assert flag in out


class _Driver(object):
    """The loss-option part of both drivers (model._WeightedCE) without their networks, which need the GPU."""

    def __new__(cls, md, **kw):
        kind = type("Driver", (md._WeightedCE,), {})
        d = kind()
        d.args = types.SimpleNamespace(gpu_ids=[], **kw)
        d.dp, d.n_channels, d.crop = None, 4, (12, 12)
        d._init_ce(d.args, 4)
        return d


def test_the_drivers_pass_the_option_and_the_defaults_do_not(monkeypatch):
    md, F = load_sub("model"), load_sub("functional")
    seen = []
    monkeypatch.setattr(F, "upsample_softmax_ce", lambda *a, **k: seen.append(("ce", a, k)) or ("soft", "ce"))
    monkeypatch.setattr(F, "upsample_softmax_ce_dice", lambda *a, **k: seen.append(("dice", a, k)) or ("soft", "ce", "dice"))
    monkeypatch.setattr(F, "ohem_stats", lambda: (torch.tensor(0.7), torch.tensor(3), torch.tensor(12)))
    for kw in ({}, {"ohem_min_kept": 5, "ohem_min_frac": 0.5}, {"ohem_thresh": None}):
        d = _Driver(md, **kw)
        kept = {}
        assert d.ohem_options is None and d._head("x", "lab", False, kept) == ("soft", "ce", None) and not kept
        assert seen[-1] == ("ce", ("x", (12, 12), "lab"), {"want_soft": False})
    d = _Driver(md, ohem_thresh=0.7)
    o = d.ohem_options
    assert (o.thresh, o.min_kept, o.min_frac) == (0.7, 0, 0.0625)
    kept = {}
    assert d._head("x", "lab", True, kept) == ("soft", "ce", None)
    assert seen[-1] == ("ce", ("x", (12, 12), "lab"), {"want_soft": True, "ohem": o}) and float(kept["ohem_kept"]) == 0.25
    d = _Driver(md, ohem_thresh=0.3, ohem_min_kept=1000, ohem_min_frac=0.0, dice_weight=0.5, label_smoothing=0.1)
    o = d.ohem_options
    assert (o.thresh, o.min_kept, o.min_frac) == (0.3, 1000, 0.0)
    assert d._head("x", "lab", False) == ("soft", "ce", "dice")
    assert seen[-1][0] == "dice" and seen[-1][2] == {"want_soft": False, "dice": d.dice_options, "ohem": o, "weight": None, "label_smoothing": 0.1}
    for bad in ({"ohem_thresh": 0.0}, {"ohem_thresh": 1.5}, {"ohem_thresh": 0.5, "ohem_min_kept": -1}, {"ohem_thresh": 0.5, "ohem_min_frac": 2.0}):
        with pytest.raises(ValueError):
            _Driver(md, **bad)


# ------------------------------------------------------------------------------------------ 3. the reference
def test_the_reference_is_the_definition():
    """Against a sort, on every geometry / class count / selection of the GPU tests: the mask keeps at least r pixels, every pixel at or
    below the r-th smallest key and every pixel at or below thresh, nothing else; a thresh-dominated case keeps a share in (0.1, 0.9);
    loss and gradient equal torch's cross entropy with every pixel that is not kept mapped to the ignore index."""
    worst = 0.0
    for gi, (N, H, W, OH, OW) in enumerate(GEOMS):
        for Cn in CLASSES:
            x, lab = make_case(1000 * gi + Cn, N, Cn, H, W, OH, OW)
            rs = None if (OH, OW) == (H, W) else (OH, OW)
            share_void = float(((lab < 0) | (lab >= Cn)).double().mean())
            assert 0.05 < share_void < 0.15
            for si, (th, K, f) in enumerate(selections(Cn)):
                for w32, eps in ((None, 0.0), (make_weights(Cn, Cn), 0.1)):
                    ref = ohem_reference(x, lab, w32, eps, th, K, f, resize=rs)
                    V = ref["V"]
                    assert V == int(ref["counted"].sum()) and ref["r"] == min(max(K, math.ceil(f * V), 1), V)
                    srt = torch.sort(ref["keys"][ref["counted"]]).values
                    m = float(srt[ref["r"] - 1])
                    assert ref["m"] == m and ref["tau"] == max(m, f32(th))
                    want = ref["counted"] & (ref["keys"] <= max(m, f32(th)))
                    assert torch.equal(ref["mask"], want) and ref["kept"] == int(want.sum()) >= ref["r"]
                    assert (ref["keys"][~ref["counted"]] == 2.0).all()
                    if si in (0, 3):
                        assert ref["tau"] == f32(th)                                               # thresh-dominated
                    if th == THETA_MID[Cn]:
                        assert 0.1 < ref["kept"] / V < 0.9, (Cn, ref["kept"] / V)
                    elif si == 1:
                        assert ref["kept"] >= min(1000, V)
                    xr = x.clone().requires_grad_(True)
                    up = xr if rs is None else TF.interpolate(xr, size=rs, mode="bilinear", align_corners=True)
                    tl = torch.where(ref["mask"], lab, torch.full_like(lab, -100))
                    loss = TF.cross_entropy(up, tl, weight=None if w32 is None else w32.double(), label_smoothing=eps, ignore_index=-100)
                    grad = torch.autograd.grad(loss, xr)[0]
                    worst = max(worst, abs(float(loss.detach()) - float(ref["loss"])) / abs(float(loss.detach())),
                                float((grad - ref["grad"]).abs().max() / grad.abs().max()))
    print("ohem reference against torch's masked cross entropy: worst relative distance %.2e" % worst)
    assert worst <= 1e-12


def test_the_reference_on_ties_empty_and_teacher_forced_masks():
    x = torch.zeros(1, 2, 3, 3, dtype=torch.float64)                       # every key is 0.5
    lab = torch.tensor([[[0, 1, 0], [1, 255, 0], [1, 1, -100]]])
    ref = ohem_reference(x, lab, None, 0.0, 0.1, 1, 0.0)
    assert ref["V"] == 7 and ref["r"] == 1 and ref["m"] == 0.5 and ref["kept"] == 7          # <=: every tie at m is kept
    assert float(ref["loss"]) == pytest.approx(math.log(2.0), rel=1e-15)
    none = ohem_reference(x, torch.full((1, 3, 3), 255), None, 0.0, 0.5, 3, 0.5)
    assert none["V"] == 0 and none["kept"] == 0 and math.isnan(float(none["loss"])) and torch.count_nonzero(none["grad"]) == 0
    w0 = torch.tensor([0.0, 1.0])
    zero_d = ohem_reference(x, torch.zeros(1, 3, 3, dtype=torch.int64), w0, 0.0, 1.0, 0, 0.0)
    assert zero_d["V"] == 9 and zero_d["kept"] == 9 and zero_d["D"] == 0 and math.isnan(float(zero_d["loss"]))
    forced = torch.zeros(1, 3, 3, dtype=torch.bool)
    forced[0, 0, 0] = forced[0, 1, 1] = True                                # (1, 1) is void: a forced mask cannot keep it
    tf = ohem_reference(x, lab, None, 0.0, 0.1, 1, 0.0, mask=forced)
    assert tf["kept"] == 1 and torch.count_nonzero(tf["grad"][0, :, 0, 0]) == 2 and torch.count_nonzero(tf["grad"]) == 2
    assert ohem_rank(10, 0, 0.0) == 1 and ohem_rank(10, 1000, 0.0) == 10 and ohem_rank(11, 0, 0.5) == 6 and ohem_rank(10, 3, 0.25) == 3
