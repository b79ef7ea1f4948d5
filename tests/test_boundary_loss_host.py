"""Boundary loss on signed distance maps (sscg_sdm, sscg_boundary_loss_fwd / _bwd, sscg_upsample_head_bwd_b, --boundary_loss) on a
GPU-less host: tests/sdm_reference.py against literals, an O(P^2) brute force and Kervadec's two-transform formula; the level set's bits;
every argument error of the new entries before any HIP call; the driver flags, the ramp schedule, and a model built with the defaults
taking none of the new paths."""
import ctypes as C
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT, load_sub
from sdm_reference import boundary_reference, kervadec_phi, phi_reference, sdm_brute, sdm_reference

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
ONE = C.c_void_p(16)          # never dereferenced
NEW = ("sscg_sdm_workspace", "sscg_sdm", "sscg_boundary_loss_workspace", "sscg_boundary_loss_fwd", "sscg_boundary_loss_bwd",
       "sscg_upsample_head_bwd_b")


# ------------------------------------------------------------------------------------------ 1. the reference
def test_reference_against_literals():
    lab = np.array([[[0, 0, 0, 0, 0],
                     [0, 1, 1, 0, 0],
                     [0, 1, 1, 0, 255],
                     [0, 0, 0, 0, -100]]], dtype=np.int64)
    s = sdm_reference(lab, 3)
    assert s.dtype == np.int32 and s.shape == (1, 4, 5, 3)
    assert s[0, :, :, 1].tolist() == [[2, 1, 1, 2, 5],
                                      [1, -1, -1, 1, 4],
                                      [1, -1, -1, 1, 4],
                                      [2, 1, 1, 2, 5]]
    # class 0: its non-members are the four 1s and the two void pixels
    assert s[0, :, :, 0].tolist() == [[-2, -1, -1, -2, -4],
                                      [-1, 1, 1, -1, -1],
                                      [-1, 1, 1, -1, 1],
                                      [-2, -1, -1, -1, 1]]
    assert not s[0, :, :, 2].any()                                    # absent class: a zero plane
    full = np.zeros((2, 3, 3), dtype=np.int64)
    full[1, 1, 1] = 1
    s = sdm_reference(full, 2)
    assert not s[0].any()                                             # sample 0: class 0 fills it, class 1 is absent
    assert s[1, :, :, 1].tolist() == [[2, 1, 2], [1, -1, 1], [2, 1, 2]] and s[1, :, :, 0].tolist() == [[-2, -1, -2], [-1, 1, -1], [-2, -1, -2]]
    void = np.full((1, 2, 2), 255, dtype=np.int64)
    assert not sdm_reference(void, 4).any()
    phi = phi_reference(np.array([0, 1, -1, 4, -4, 2, -2], dtype=np.int32))
    assert phi.dtype == np.float32 and phi.tolist()[:5] == [0.0, 1.0, 0.0, 2.0, -1.0]
    assert phi[5] == np.float32(np.sqrt(np.float32(2))) and phi[6] == np.float32(1) - np.float32(np.sqrt(np.float32(2)))


@pytest.mark.parametrize("shape,Cn", [((2, 1, 1), 1), ((1, 1, 9), 2), ((1, 9, 1), 2), ((2, 5, 7), 3), ((2, 9, 11), 4), ((1, 8, 8), 6)])
def test_reference_against_brute_force(shape, Cn):
    g = np.random.default_rng(7 * Cn + shape[1] * shape[2])
    for trial in range(6):
        lab = g.integers(0, Cn, size=shape).astype(np.int64)
        if trial == 1:
            lab[0] = 0                                                # a class filling a sample
        if trial == 2:
            lab[:] = Cn - 1
            lab[0, 0, 0] = 0                                          # one member pixel in a corner
        if trial == 3:
            yy, xx = np.indices(shape[1:])
            lab[:] = (yy + xx) % 2                                    # checkerboard (class ids 0 / 1; C == 1: class 0 and void)
        if trial >= 4:
            flat = lab.reshape(-1)
            flat[::5] = 255
            flat[2::7] = -100
            flat[3::9] = Cn + 3                                       # an id >= C is void as well
        assert np.array_equal(sdm_reference(lab, Cn), sdm_brute(lab, Cn)), (shape, Cn, trial)
    if shape[1] * shape[2] > 1 and Cn >= 2:
        yy, xx = np.indices(shape[1:])
        board = np.broadcast_to((yy + xx) % 2, shape).astype(np.int64)
        s = sdm_reference(board, Cn)
        assert (np.abs(s[..., :2]) == 1).all() and not s[..., 2:].any()


def test_reference_against_kervadecs_formula():
    g = np.random.default_rng(11)
    for shape, Cn in (((2, 9, 11), 4), ((1, 17, 13), 3), ((1, 1, 9), 2)):
        lab = g.integers(0, Cn, size=shape).astype(np.int64)
        lab.reshape(-1)[::6] = 255
        want = kervadec_phi(lab, Cn)
        phi = phi_reference(sdm_reference(lab, Cn))
        assert np.abs(phi.astype(np.float64) - want).max() <= 2.0 ** -23 * max(1.0, np.abs(want).max())
        # the squares are exact: the integers are the squares of the transform's distances
        s = sdm_reference(lab, Cn).astype(np.float64)
        pos = lab[..., None] == np.arange(Cn)
        d = np.where(pos, 1.0 - want, want)
        assert np.array_equal((np.rint(d * d) * (s != 0)), np.abs(s)) and ((s < 0) == (pos & (s != 0))).all()


def test_phi_bits_are_the_fp64_root_rounded_once():
    s = np.concatenate([np.arange(-5000, 5001), np.array([2 ** 24 + 1, -(2 ** 24 + 3), 2 ** 30 - 1, -(2 ** 30 - 1), 123456789])]).astype(np.int32)
    phi = phi_reference(s)
    f = np.abs(s).astype(np.float32)                                  # the cast is the definition's first rounding
    root = np.sqrt(f.astype(np.float64)).astype(np.float32)           # fp64 sqrt of an fp32 value, rounded once: correctly rounded
    want = np.where(s > 0, root, np.where(s < 0, (np.float32(1) - root).astype(np.float32), np.float32(0))).astype(np.float32)
    assert np.array_equal(phi.view(np.int32), want.view(np.int32))
    assert phi[s == 0].view(np.int32).tolist() == [0] and (phi[s > 0] > 0).all() and (phi[s < 0] <= 0).all()


def test_loss_reference_by_hand():
    lab = torch.tensor([[[0, 1], [1, 255]]])
    x = torch.zeros(1, 2, 2, 2, dtype=torch.float64)                  # p = 1/2 everywhere
    ref = boundary_reference(x, lab)
    # class 0: member (0,0) phi = 1 - 1 = 0; (0,1), (1,0) non-members at distance 1; class 1: (0,0) at 1, members phi = 0.  void: not counted
    assert ref["counted"] == 3 and ref["k"] == 1.0 / 6.0
    assert ref["sums"].tolist() == [[1.0, 0.5]] and float(ref["loss"]) == pytest.approx(0.25)
    w = torch.tensor([0.0, 2.0])
    assert float(boundary_reference(x, lab, w)["loss"]) == pytest.approx(2.0 * 0.5 / (3 * 2.0))
    allvoid = boundary_reference(x, torch.full((1, 2, 2), 255))
    assert float(allvoid["loss"]) == 0.0 and not allvoid["grad"].any() and allvoid["k"] == 0.0
    # the gradient with respect to the probabilities is k w_c phi_c: through the softmax, d_c = p_c (q_c - sum_k p_k q_k)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 4, 5, generator=g, dtype=torch.float64)
    lab = torch.randint(0, 3, (2, 4, 5), generator=g)
    lab[0, 0, 0] = 255
    w = torch.tensor([1.0, 0.0, 0.5])
    ref = boundary_reference(x, lab, w)
    p = torch.softmax(x, 1)
    q = ref["k"] * w.double()[None, :, None, None] * torch.from_numpy(ref["phi"]).double().permute(0, 3, 1, 2)
    q = q * ((lab >= 0) & (lab < 3)).unsqueeze(1)
    d = p * (q - (p * q).sum(1, keepdim=True))
    assert (d - ref["grad"]).abs().max() <= 1e-14


# ------------------------------------------------------------------------------------------ 2. the ABI
def test_the_entries_are_declared_exported_and_bound():
    L = load_sub("_lib")
    hdr = open(os.path.join(ROOT, "include", "sscg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "size_t sscg_sdm_workspace(int N, int H, int W, int C);" in code
    assert "int sscg_sdm(const int64_t* labels, int N, int H, int W, int C, int32_t* sdm, void* ws, size_t ws_bytes, void* stream);" in code
    assert "size_t sscg_boundary_loss_workspace(int N, int OH, int OW, int C);" in code
    assert "int sscg_boundary_loss_fwd(const float* x, const int64_t* labels, const int32_t* sdm, int N, int H, int W, int C, int OH, int OW," in code
    assert "int sscg_boundary_loss_bwd(const float* x, const int64_t* labels, const int32_t* sdm, int N, int H, int W, int C, const float* class_w," in code
    assert "const int32_t* sdm,\n                             const float* bnd_coef, const float* bnd_w, const float* g_bnd, void* stream);" in code
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sscg_[a-z0-9_]+)", out))
    for name in NEW:
        assert name in exported and name in L.SIGNATURES and callable(getattr(L.lib, name)), name
    assert [len(L.SIGNATURES[n][1]) for n in NEW] == [4, 9, 4, 17, 13, 24]
    # _bwd_b = the arguments of _bwd_h, then four pointers, then the stream
    h, b = L.SIGNATURES["sscg_upsample_head_bwd_h"][1], L.SIGNATURES["sscg_upsample_head_bwd_b"][1]
    assert b[:len(h) - 1] == h[:-1] and b[len(h) - 1:] == [C.c_void_p] * 5
    assert L.ABI_VERSION == 18 and L.lib.sscg_abi_version() == 18 and "#define SSCG_ABI_VERSION 18" in hdr      # additions only


def test_workspace_sizes():
    lib = load_sub("_lib").lib
    up = lambda b: (b + 255) // 256 * 256
    ws = lib.sscg_sdm_workspace
    # the counts [N][C] uint32, then min(C, 16) uint16 planes of column distances
    assert ws(2, 5, 7, 3) == up(2 * 3 * 4) + up(3 * 2 * 5 * 7 * 2)
    assert ws(1, 70, 33, 21) == up(21 * 4) + up(16 * 70 * 33 * 2) and ws(8, 256, 256, 4) == up(8 * 4 * 4) + 4 * 8 * 256 * 256 * 2
    assert ws(0, 5, 5, 4) == 0 and ws(1, 5, 5, 0) == 0 and ws(1, 5, 5, 65) == 0 and ws(1, -1, 5, 4) == 0
    assert ws(1, 46341, 46341, 1) == 0 and ws(1, 32769, 1, 1) == 0 and ws(1, 23172, 23172, 2) == 0 and ws(1, 23171, 23171, 2) > 0       # sizes sscg_sdm refuses
    assert ws(1, 32768, 1, 1) > 0
    bl = lib.sscg_boundary_loss_workspace
    # one fp64 record [C + 1] per statistics block, at most 256 blocks per sample, and one per sample
    assert bl(2, 13, 17, 4) == 2 * 5 * (1 + 1) * 8 and bl(8, 256, 256, 21) == 8 * 22 * (256 + 1) * 8 and bl(3, 150, 151, 4) == 3 * 5 * (89 + 1) * 8
    assert bl(0, 5, 5, 4) == 0 and bl(1, 5, 5, 0) == 0 and bl(1, 5, 5, 65) == 0 and bl(1, 46341, 46341, 1) == 0 and bl(1, 32769, 1, 1) == 0


def test_argument_errors_are_returned_before_any_launch():
    lib = load_sub("_lib").lib
    big = 1 << 40

    def sdm(lab=ONE, N=2, H=5, W=7, Cn=3, out=ONE, ws=ONE, wsb=big):
        return lib.sscg_sdm(lab, N, H, W, Cn, out, ws, wsb, None)

    def fwd(x=ONE, lab=ONE, sdm=ONE, N=2, H=3, W=4, Cn=4, OH=13, OW=17, w=ONE, loss=ONE, sums=ONE, counted=ONE, coef=ONE, ws=ONE, wsb=big):
        return lib.sscg_boundary_loss_fwd(x, lab, sdm, N, H, W, Cn, OH, OW, w, loss, sums, counted, coef, ws, wsb, None)

    def bwd(x=ONE, lab=ONE, sdm=ONE, N=2, H=3, W=4, Cn=4, w=ONE, coef=ONE, g=None, dx=ONE):
        return lib.sscg_boundary_loss_bwd(x, lab, sdm, N, H, W, Cn, w, coef, g, 1.0, dx, None)

    def head(x=ONE, lab=ONE, keys=ONE, thr=ONE, w=ONE, eps=0.0, dy=ONE, g_ce=None, valid=ONE, coef=ONE, g_dice=None, batch=0, dx=ONE,
             N=2, H=3, W=4, Cn=4, OH=13, OW=17, sdm=ONE, bcoef=ONE, bw=ONE, g_bnd=None):
        return lib.sscg_upsample_head_bwd_b(x, lab, keys, thr, w, eps, dy, g_ce, valid, coef, g_dice, batch, dx, N, H, W, Cn, OH, OW,
                                            sdm, bcoef, bw, g_bnd, None)

    assert sdm(lab=None) == BAD_ARG and sdm(out=None) == BAD_ARG
    for call in (sdm, fwd, bwd, head):
        assert call(Cn=0) == BAD_ARG and call(Cn=65) == BAD_ARG and call(Cn=-1) == BAD_ARG, call.__name__
        assert call(N=0) == BAD_ARG and call(H=0) == BAD_ARG and call(W=-3) == BAD_ARG, call.__name__
    for call in (fwd, bwd, head):
        assert call(x=None) == BAD_ARG and call(lab=None) == BAD_ARG, call.__name__
    assert fwd(sdm=None) == BAD_ARG and fwd(loss=None) == BAD_ARG and fwd(coef=None) == BAD_ARG and fwd(OH=0) == BAD_ARG and fwd(OW=-1) == BAD_ARG
    assert bwd(sdm=None) == BAD_ARG and bwd(coef=None) == BAD_ARG and bwd(dx=None) == BAD_ARG
    assert head(dx=None) == BAD_ARG and head(bcoef=None) == BAD_ARG and head(OH=0) == BAD_ARG
    assert head(thr=None) == BAD_ARG and head(valid=None) == BAD_ARG                    # keys without thr / valid
    assert head(eps=1.0) == BAD_ARG and head(eps=float("nan")) == BAD_ARG and head(batch=2) == BAD_ARG
    # sdm == NULL: sscg_upsample_head_bwd_h's own checks answer ...
    assert head(sdm=None, x=None) == BAD_ARG and head(sdm=None, keys=None, dy=None, coef=None, valid=None) == BAD_ARG       # no branch at all
    assert head(sdm=None, lab=None) == BAD_ARG and head(sdm=None, N=1, H=1, W=1, OH=46341, OW=46341) == UNSUPPORTED
    assert head(sdm=None, keys=None, thr=None) == BAD_ARG                               # ... and valid without keys is refused, not dropped
    # sizes
    assert sdm(N=1, H=46341, W=46341) == UNSUPPORTED and sdm(N=1, H=46341, W=46341, ws=None) == UNSUPPORTED
    assert sdm(N=1, H=23172, W=23172) == UNSUPPORTED and sdm(N=1, H=32769, W=1) == UNSUPPORTED          # (H-1)^2 + (W-1)^2 >= 2^30
    assert sdm(N=1, H=46341, W=46341, out=None) == BAD_ARG                              # ... after the arguments
    assert fwd(N=1, H=1, W=1, OH=46341, OW=46341) == UNSUPPORTED and fwd(N=1, H=1, W=1, OH=32769, OW=1) == UNSUPPORTED
    assert fwd(N=1, H=46341, W=46341, OH=2, OW=2) == UNSUPPORTED and fwd(N=1, H=1, W=1, OH=46341, OW=46341, ws=None) == UNSUPPORTED
    assert bwd(N=1, H=46341, W=46341) == UNSUPPORTED and bwd(N=1, H=32769, W=1) == UNSUPPORTED
    assert head(N=1, H=1, W=1, OH=46341, OW=46341) == UNSUPPORTED and head(N=1, H=1, W=1, OH=32769, OW=1) == UNSUPPORTED
    # the workspaces: one byte short
    need = lib.sscg_sdm_workspace(2, 5, 7, 3)
    assert need > 0 and sdm(ws=None) == WORKSPACE and sdm(wsb=need - 1) == WORKSPACE and sdm(wsb=0) == WORKSPACE
    need = lib.sscg_boundary_loss_workspace(2, 13, 17, 4)
    assert need > 0 and fwd(ws=None) == WORKSPACE and fwd(wsb=need - 1) == WORKSPACE
    # sums, counted, class weights and the upstream scalars are optional: the error (if any) is not theirs
    assert fwd(sums=None, counted=None, w=None, ws=None) == WORKSPACE and bwd(w=None, g=None, x=None) == BAD_ARG
    assert head(keys=None, thr=None, valid=None, dy=None, coef=None, w=None, bw=None, x=None) == BAD_ARG


# ------------------------------------------------------------------------------------------ 3. flags, options, schedule
def test_main_takes_the_flags_and_moves_no_default(capsys):
    sys.path.insert(0, ROOT)
    import main
    a = main.get_args([])
    assert a.boundary_loss == 0.0 and a.boundary_loss_skip == "" and a.boundary_loss_ramp == 0
    before = dict(vars(a))
    assert not any(k.startswith("boundary_loss") for k in before)          # a default run parses to the namespace it always did
    old = ["--dataset", "acdc", "--dice_weight", "0.5", "--boundary", "on", "--batch_size", "4"]
    assert not any(k.startswith("boundary_loss") for k in vars(main.get_args(old)))
    b = main.get_args(["--boundary_loss", "0.01", "--boundary_loss_skip", "0, 3", "--boundary_loss_ramp", "20"])
    assert b.boundary_loss == 0.01 and b.boundary_loss_skip == "0, 3" and b.boundary_loss_ramp == 20
    assert {k: v for k, v in vars(b).items() if not k.startswith("boundary_loss")} == before
    assert main.get_args(["--boundary_loss", "0"]).boundary_loss == 0.0                     # 0 means off
    c = main.get_args(["--dataset", "acdc", "--boundary_loss", "1", "--ce_weights", "median", "--label_smoothing", "0.1", "--dice_weight", "0.5",
                       "--ohem_thresh", "0.7"])
    assert c.boundary_loss == 1.0 and c.dice_weight == 0.5 and c.ohem_thresh == 0.7          # it combines with the other loss flags
    for bad in (["--boundary_loss", "-0.1"], ["--boundary_loss", "nan"], ["--boundary_loss", "inf"], ["--boundary_loss", "x"],
                ["--boundary_loss_ramp", "-1"], ["--boundary_loss_ramp", "1.5"], ["--boundary_loss_ramp", "x"],
                ["--boundary_loss_skip", "21"], ["--boundary_loss_skip", "-1"], ["--boundary_loss_skip", "a"], ["--boundary_loss_skip", "0,,1"],
                ["--dataset", "acdc", "--boundary_loss_skip", "4"], ["--dataset", "acdc", "--boundary_loss_skip", "0,1,2,3"]):
        with pytest.raises(SystemExit):
            main.get_args(bad)
    capsys.readouterr()
    assert main.get_args(["--dataset", "cityscapes", "--boundary_loss_skip", "19"]).boundary_loss_skip == "19"
    with pytest.raises(SystemExit):
        main.get_args(["--help"])
    out = capsys.readouterr().out
    for flag in ("--boundary_loss", "--boundary_loss_skip", "--boundary_loss_ramp"):
        assert flag in out and flag in main.__doc__


def test_skip_list_and_weights():
    U, F = load_sub("utils"), load_sub("functional")
    P = U.parse_boundary_loss_skip
    assert P("", 4) == [] and P(None, 21) == [] and P("  ", 4) == []
    assert P("0", 21) == [0] and P("19", 20) == [19] and P("3, 0,3", 4) == [0, 3]
    for bad, token in (("4", "'4'"), ("-1", "'-1'"), ("a", "'a'"), ("0,,1", "''"), ("1.5", "'1.5'"), ("0,1,2,3", "every class")):
        with pytest.raises(ValueError) as e:
            P(bad, 4)
        assert token in str(e.value) and "--boundary_loss_skip" in str(e.value), (bad, str(e.value))
    cpu = torch.device("cpu")
    w = F.boundary_weight([0.0 if c in P("0,3", 4) else 1.0 for c in range(4)], 4, cpu)
    assert w.dtype == torch.float32 and w.tolist() == [0.0, 1.0, 1.0, 0.0]
    for bad in ([1, 2, 3], [1, -1, 1, 1], [1, float("nan"), 1, 1], [1, float("inf"), 1, 1], [0, 0, 0, 0]):
        with pytest.raises(ValueError):
            F.boundary_weight(bad, 4, cpu)
    assert F.BoundaryLossOptions().weight is None and F.BoundaryLossOptions(weight=w).weight is w
    assert F._boundary_options({"weight": w}).weight is w
    with pytest.raises(TypeError):
        F._boundary_options(0.5)


def test_the_ramp_schedule():
    U = load_sub("utils")
    S = U.boundary_loss_schedule
    assert [S(0.5, 0, e) for e in (0, 1, 100)] == [0.5, 0.5, 0.5]                             # no ramp: constant
    assert [S(2.0, 4, e) for e in range(7)] == [0.0, 0.5, 1.0, 1.5, 2.0, 2.0, 2.0]            # F * min(1, epoch / N)
    assert S(0.01, 1, 0) == 0.0 and S(0.01, 1, 1) == 0.01 and S(0.0, 5, 3) == 0.0
    assert S(1.0, 3, 1) == pytest.approx(1.0 / 3.0, rel=1e-15)


class _Driver(object):
    """The loss-option part of both drivers (model._WeightedCE) without their networks, which need the GPU."""

    def __new__(cls, md, **kw):
        kind = type("Driver", (md._WeightedCE,), {})
        d = kind()
        d.args = types.SimpleNamespace(gpu_ids=[], **kw)
        d.dp, d.n_channels, d.crop = None, 4, (12, 12)
        d._init_ce(d.args, 4)
        return d


def test_the_defaults_take_no_boundary_path(monkeypatch):
    md, F, L = load_sub("model"), load_sub("functional"), load_sub("_lib")
    seen = []
    monkeypatch.setattr(F, "upsample_softmax_ce", lambda *a, **k: seen.append((a, k)) or ("soft", "ce"))
    monkeypatch.setattr(F, "upsample_softmax_losses", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the boundary head was called")))
    for kw in ({}, {"boundary_loss": 0.0}, {"boundary_loss": 0, "boundary_loss_skip": "0", "boundary_loss_ramp": 5}):
        d = _Driver(md, **kw)
        assert d.boundary_loss_options is None and d.boundary_w == 0.0 and d._boundary_b == 0.0 and d.set_boundary_epoch(7) == 0.0
        kept = {}
        assert d._head("x", "lab", False, kept) == ("soft", "ce", None) and kept == {}
        assert seen[-1] == (("x", (12, 12), "lab"), {"want_soft": False})
    monkeypatch.undo()
    assert "lab_loss_boundary" not in md.LOSS_KEYS and "gt_cycle_boundary" not in md.LOSS_KEYS
    # on: the options, the ramp per epoch, and the term through _head's dict
    d = _Driver(md, boundary_loss=0.5, boundary_loss_skip="0,3", boundary_loss_ramp=4)
    assert d.boundary_w == 0.5 and d.boundary_ramp == 4 and d.boundary_loss_options.weight.tolist() == [0.0, 1.0, 1.0, 0.0]
    assert d._boundary_b == 0.0 and d.set_boundary_epoch(2) == 0.25 and d._boundary_b == 0.25 and d.set_boundary_epoch(9) == 0.5
    d = _Driver(md, boundary_loss=2)
    assert d.boundary_loss_options.weight is None and d.boundary_ramp == 0 and d._boundary_b == 2.0
    calls = []
    monkeypatch.setattr(F, "upsample_softmax_losses", lambda *a, **k: calls.append((a, k)) or ("soft", "ce", None, "bnd"))
    kept = {}
    assert d._head("x", "lab", True, kept) == ("soft", "ce", None) and kept == {"boundary": "bnd"}
    assert calls[-1][0] == ("x", (12, 12), "lab") and calls[-1][1]["boundary"] is d.boundary_loss_options and calls[-1][1]["dice"] is None
    monkeypatch.undo()
    for bad in ({"boundary_loss": -1.0}, {"boundary_loss": float("nan")}, {"boundary_loss": float("inf")},
                {"boundary_loss": 1.0, "boundary_loss_skip": "4"}, {"boundary_loss": 1.0, "boundary_loss_skip": "0,1,2,3"},
                {"boundary_loss": 1.0, "boundary_loss_ramp": -1}, {"boundary_loss": 1.0, "boundary_loss_ramp": 1.5}):
        with pytest.raises(ValueError):
            _Driver(md, **bad)
    # no CPU fallback
    x, lab = torch.zeros(1, 4, 3, 3), torch.zeros(1, 3, 3, dtype=torch.int64)
    with pytest.raises(L.SscgError):
        F.boundary_loss(x, lab)
    with pytest.raises(L.SscgError):
        F.signed_distance_maps(lab, 4)
    with pytest.raises(L.SscgError):
        F.upsample_softmax_losses(x, (12, 12), torch.zeros(1, 12, 12, dtype=torch.int64), boundary=F.BoundaryLossOptions())
    # the existing heads keep their signatures
    assert F.upsample_softmax_ce.__defaults__ == (None, True, None, 0.0) and F.upsample_softmax_ce_dice.__defaults__ == (True, None, 0.0, None)
