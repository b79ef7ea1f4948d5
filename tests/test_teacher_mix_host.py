"""CutMix consistency for the mean teacher (sscg_mix_boxes / sscg_teacher_fwd_mix; --unl_cutmix) on a GPU-less host: the two entries are
declared, exported and bound, the C entries return every argument error before any HIP call, the flag parses and is refused without
its teacher, a default run parses to the namespace it always did, the boxes' generator leaves the flip draws of a seed where they
were, functional.mix_boxes refuses class-mask words - and the inputs of tests/test_teacher_mix_gpu.py keep the margins that make its
exact comparisons meaningful."""
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
from teacher_mix_reference import (CLASSES, FLIPS, GEOMS, INTERIOR, MARGIN, NOTHING, SEEDS, TAU, TEMP, case_inputs,
                                   mix_teacher_reference, mixed_teacher, pasted, reference, seed_ok, tables_of)
from teacher_reference import mirror_where, teacher_reference

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
ONE, TWO = C.c_void_p(16), C.c_void_p(4096)          # never dereferenced
NEW = ("sscg_mix_boxes", "sscg_teacher_fwd_mix")


# ------------------------------------------------------------------------------------------ 1. the ABI
def test_the_entries_are_declared_exported_and_bound():
    L = load_sub("_lib")
    hdr = open(os.path.join(ROOT, "include", "sscg.h")).read()
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "int sscg_mix_boxes(const float* x, float* y, const int32_t* table, int N, int H, int W, int C, void* stream);" in code
    assert ("int sscg_teacher_fwd_mix(const float* x, const float* t, const uint8_t* flip, const int32_t* table, int N, int H, int W, int C, "
            "int OH, int OW, float inv_temp, float thresh, float* losses, double* sums, uint8_t* pseudo, float* coef, void* ws, "
            "size_t ws_bytes, void* stream);") in code
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sscg_[a-z0-9_]+)", out))
    for name in NEW:
        assert name in exported and name in L.SIGNATURES and callable(getattr(L.lib, name)), name
    assert [len(L.SIGNATURES[n][1]) for n in NEW] == [8, 19]
    # the mix entry is the plain one with `table` behind `flip`
    plain, mix = L.SIGNATURES["sscg_teacher_fwd"][1], L.SIGNATURES["sscg_teacher_fwd_mix"][1]
    assert mix[:3] == plain[:3] and mix[3] is C.c_void_p and mix[4:] == plain[3:]
    assert L.ABI_VERSION == 18 and L.lib.sscg_abi_version() == 18 and "#define SSCG_ABI_VERSION 18" in hdr      # additions only
    # the stream-ordering checker reads the header: the kinds of the pointers
    table = L.dev_tool("racecheck").parse_header(os.path.join(ROOT, "include", "sscg.h"))
    kinds = dict(table["sscg_teacher_fwd_mix"])
    assert [kinds[a] for a in ("x", "t", "flip", "table")] == ["r"] * 4
    assert [kinds[a] for a in ("losses", "sums", "pseudo", "coef", "ws")] == ["w"] * 5 and kinds["stream"] == "stream"
    assert [k for _, k in table["sscg_teacher_fwd_mix"]].count("-") == 9      # N, H, W, C, OH, OW, inv_temp, thresh, ws_bytes
    kinds = dict(table["sscg_mix_boxes"])
    assert kinds["x"] == "r" and kinds["table"] == "r" and kinds["y"] == "w" and kinds["stream"] == "stream"
    assert table["sscg_teacher_fwd"] == [r for r in table["sscg_teacher_fwd_mix"] if r[0] != "table"]        # the plain entry is unmoved


def test_argument_errors_are_returned_before_any_launch():
    lib = load_sub("_lib").lib
    big = 1 << 30

    def fwd(x=ONE, t=ONE, flip=ONE, table=ONE, N=2, H=3, W=4, Cn=4, OH=13, OW=17, it=1.0, tau=0.5, losses=ONE, sums=ONE, pm=ONE, coef=ONE,
            ws=ONE, wsb=big):
        return lib.sscg_teacher_fwd_mix(x, t, flip, table, N, H, W, Cn, OH, OW, it, tau, losses, sums, pm, coef, ws, wsb, None)

    # sscg_teacher_fwd's errors, with and without a table
    for table in (ONE, None):
        assert fwd(x=None, table=table) == BAD_ARG and fwd(t=None, table=table) == BAD_ARG
        assert fwd(losses=None, table=table) == BAD_ARG and fwd(sums=None, table=table) == BAD_ARG
        assert fwd(Cn=0, table=table) == BAD_ARG and fwd(Cn=65, table=table) == BAD_ARG
        assert fwd(N=0, table=table) == BAD_ARG and fwd(H=0, table=table) == BAD_ARG and fwd(W=-3, table=table) == BAD_ARG
        assert fwd(OH=0, table=table) == BAD_ARG and fwd(OW=-1, table=table) == BAD_ARG
        for tau in (-0.01, 1.01, float("nan"), float("inf")):
            assert fwd(tau=tau, table=table) == BAD_ARG, tau
        for it in (0.0, -1.0, float("nan"), float("inf")):
            assert fwd(it=it, table=table) == BAD_ARG, it
        assert fwd(flip=None, pm=None, coef=None, ws=None, table=table) == WORKSPACE
        assert fwd(wsb=2 * 2 * 4 * 8 - 1, table=table) == WORKSPACE
        assert fwd(N=1, H=1, W=1, OH=46341, OW=46341, table=table) == UNSUPPORTED                   # N * OH * OW >= 2^31
        assert fwd(N=1, H=46341, W=46341, OH=46341, OW=46340, table=table) == UNSUPPORTED           # N * H * W >= 2^31
        assert fwd(N=1, H=1, W=1, OH=46341, OW=46341, ws=None, table=table) == UNSUPPORTED          # ... before the workspace
        assert fwd(N=1, H=1, W=1, OH=46341, OW=46341, tau=2.0, table=table) == BAD_ARG              # ... after the arguments

    def mix(x=ONE, y=TWO, table=ONE, N=2, H=5, W=7, Cn=3):
        return lib.sscg_mix_boxes(x, y, table, N, H, W, Cn, None)

    assert mix(x=None) == BAD_ARG and mix(y=None) == BAD_ARG and mix(table=None) == BAD_ARG
    assert mix(y=ONE) == BAD_ARG                                                    # y == x: a partner's pixel is its pixel before mixing
    assert mix(N=0) == BAD_ARG and mix(H=0) == BAD_ARG and mix(W=-1) == BAD_ARG and mix(Cn=0) == BAD_ARG and mix(N=-2) == BAD_ARG
    assert mix(N=1, H=46341, W=46341, Cn=1) == UNSUPPORTED                          # N*H*W*C >= 2^31
    assert mix(N=2, H=32768, W=32768, Cn=1) == UNSUPPORTED                          # exactly 2^31
    assert mix(N=1, H=32768, W=32768, Cn=2) == UNSUPPORTED
    assert mix(N=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1, Cn=2 ** 31 - 1) == UNSUPPORTED      # no product wraps on the way
    assert mix(N=1, H=46341, W=46341, Cn=1, y=ONE) == BAD_ARG                       # the arguments first


# ------------------------------------------------------------------------------------------ 2. the flag
def test_main_takes_the_flag_and_moves_no_default(capsys):
    sys.path.insert(0, ROOT)
    import main
    a = main.get_args([])
    assert a.unl_cutmix == ""
    before = dict(vars(a))
    assert "unl_cutmix" not in before                              # a default run parses to the namespace it always did
    old = ["--ema_decay", "0.99", "--unl_teacher", "mse=1,flip"]
    with_teacher = dict(vars(main.get_args(old)))
    assert "unl_cutmix" not in with_teacher
    b = main.get_args(old + ["--unl_cutmix", "0.5:0.1:0.3"])
    assert b.unl_cutmix == "0.5:0.1:0.3"
    assert {k: v for k, v in vars(b).items() if k != "unl_cutmix"} == with_teacher
    assert main.get_args(old + ["--unl_cutmix", "1"]).unl_cutmix == "1"
    for bad in (["--unl_cutmix", "1"],                                              # no teacher
                ["--ema_decay", "0.9", "--unl_cutmix", "1"],                        # no teacher
                ["--unl_teacher", "on", "--unl_cutmix", "1"],                       # no --ema_decay
                old + ["--unl_cutmix", "0"], old + ["--unl_cutmix", "1.5"], old + ["--unl_cutmix", "0.5:0.3"],
                old + ["--unl_cutmix", "0.5:0.6:0.3"], old + ["--unl_cutmix", "x"], old + ["--unl_cutmix", "0.5:0:0.5"]):
        with pytest.raises(SystemExit):
            main.get_args(bad)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        main.get_args(["--help"])
    assert "--unl_cutmix" in capsys.readouterr().out and "--unl_cutmix" in main.__doc__


def test_parse_unl_cutmix_accepts_and_refuses():
    U = load_sub("utils")
    assert U.parse_unl_cutmix("") is None and U.parse_unl_cutmix(None) is None and U.parse_unl_cutmix("  ") is None
    assert U.parse_unl_cutmix("1") == (1.0, 0.25, 0.5) and U.parse_unl_cutmix(" 0.5 ") == (0.5, 0.25, 0.5)      # --augment cutmix='s defaults
    assert U.parse_unl_cutmix("0.5:0.1:0.3") == (0.5, 0.1, 0.3) and U.parse_unl_cutmix("1:1:1") == (1.0, 1.0, 1.0)
    assert U.parse_unl_cutmix("0.5:0.2:0.2") == (0.5, 0.2, 0.2)
    for bad, token in (("0", "'0'"), ("-0.1", "'-0.1'"), ("1.01", "'1.01'"), ("nan", "'nan'"), ("inf", "'inf'"), ("p", "'p'"),
                       ("0.5:0.3", "'0.5:0.3'"), ("0.5:0.1:0.2:0.3", "'0.5:0.1:0.2:0.3'"), ("0.5:0:0.5", "'0'"), ("0.5:0.2:1.5", "'1.5'"),
                       ("0.5:0.6:0.3", "'0.6'"), ("0.5::0.3", "''"), ("cutmix=0.5", "'cutmix=0.5'"), ("on", "'on'")):
        with pytest.raises(ValueError) as e:
            U.parse_unl_cutmix(bad)
        assert "--unl_cutmix" in str(e.value) and token in str(e.value), (bad, str(e.value))
    # the parser of --unl_teacher and its options are as they were
    F = load_sub("functional")
    assert F.TeacherOptions.__slots__ == ("mse", "ce", "thresh", "temp", "flip") and U._TEACHER_KEYS == ("mse", "ce", "thresh", "temp")


class _Driver(object):
    """The unlabelled-loss part of the semi-supervised driver (model._UnlabelledLosses) without its networks, which need the GPU."""

    def __new__(cls, md, crop=(12, 12), **kw):
        kind = type("Driver", (md._UnlabelledLosses,), {})
        d = kind()
        d.args = types.SimpleNamespace(gpu_ids=[], **kw)
        d.crop = crop
        d._init_unl(d.args)
        return d


def test_the_option_matrix_and_the_draw():
    md, A = load_sub("model"), load_sub("data_utils.augmentations")
    for kw in ({}, dict(unl_cutmix=""), dict(ema_decay=0.9, unl_teacher="mse=1,flip"), dict(ema_decay=0.9, unl_teacher="on", unl_cutmix="  ")):
        d = _Driver(md, **kw)
        assert d.unl_cutmix is None and d._cutmix_rng is None
    for bad in (dict(unl_cutmix="1"), dict(unl_cutmix="1", ema_decay=0.9), dict(unl_cutmix="1", unl_teacher="on"),
                dict(unl_cutmix="0", ema_decay=0.9, unl_teacher="on"), dict(unl_cutmix="0.5:0.3", ema_decay=0.9, unl_teacher="on")):
        with pytest.raises(ValueError):
            _Driver(md, **bad)
    d = _Driver(md, crop=(24, 40), ema_decay=0.9, unl_teacher="mse=1", unl_cutmix="1:0.1:0.3")
    op, = d.unl_cutmix.mix_ops
    assert isinstance(op, A.RandomCutMix) and (op.p, op.lo, op.hi) == (1.0, 0.1, 0.3)
    assert md._UnlabelledLosses.CUTMIX_SEED != md._UnlabelledLosses.TEACHER_SEED
    # the draw is Compose.mixes' with a generator of the constant seed, at the head's output size (width 40, height 24)
    want = A.Compose([A.RandomCutMix(1.0, 0.1, 0.3)]).mixes(np.random.RandomState(md._UnlabelledLosses.CUTMIX_SEED), 5, 40, 24)[0]
    got = d._cutmix_table(5)
    assert got.dtype == np.int32 and got.shape == (5, 8) and np.array_equal(got, want)
    assert (got[:, 5:] == 0).all() and all(0 <= got[n, 0] < 5 and got[n, 0] != n for n in range(5))          # p = 1: every sample mixes
    assert (got[:, 1] >= 0).all() and (got[:, 3] <= 40).all() and (got[:, 2] >= 0).all() and (got[:, 4] <= 24).all()
    area = (got[:, 3] - got[:, 1]) * (got[:, 4] - got[:, 2]) / (24.0 * 40.0)
    assert (area > 0.08).all() and (area < 0.32).all()
    assert not np.array_equal(d._cutmix_table(5), got)                                                      # the generator moves on
    # a batch of one keeps its own index: not mixed
    one = _Driver(md, ema_decay=0.9, unl_teacher="mse=1", unl_cutmix="1")._cutmix_table(1)
    assert one[0, 0] == 0


def test_the_boxes_come_from_a_generator_of_their_own():
    """the flip draws of a seed are what they were without the flag; numpy's and torch's global streams do not move"""
    md = load_sub("model")
    runs = []
    for cutmix in ("", "1", "0.5:0.1:0.2"):
        torch.manual_seed(7)
        np.random.seed(7)
        d = _Driver(md, ema_decay=0.9, unl_teacher="mse=1,flip", unl_cutmix=cutmix)
        before_t, before_n = torch.get_rng_state(), np.random.get_state()[1].copy()
        draws = []
        for _ in range(3):                                         # the order of a step: the flip draw, then the table
            draws.append(torch.rand(64, generator=d._teacher_rng) < 0.5)
            if cutmix:
                d._cutmix_table(4)
        assert torch.equal(torch.get_rng_state(), before_t) and np.array_equal(np.random.get_state()[1], before_n)
        runs.append(torch.stack(draws))
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2]) and 0 < int(runs[0].sum()) < 3 * 64


def test_the_step_side_of_the_draw(monkeypatch, capsys):
    """_cutmix_unl: the size check, the share from the host's table, a batch of one is left alone; _unl_head hands the table on"""
    md, F = load_sub("model"), load_sub("functional")
    d = _Driver(md, crop=(12, 16), ema_decay=0.9, unl_teacher="mse=1", unl_cutmix="1")
    with pytest.raises(ValueError) as e:
        d._cutmix_unl(torch.zeros(2, 3, 12, 12), {})
    assert "--unl_cutmix" in str(e.value)
    calls = []
    monkeypatch.setattr(F, "upload_mix_table", lambda rows, device: ("DEV", rows.clone()))
    monkeypatch.setattr(F, "mix_boxes", lambda x, rows, dt=None: calls.append((x, rows, dt)) or "MIXED")
    img = torch.zeros(3, 3, 12, 16)
    table = np.array([[1, 2, 3, 10, 9, 0, 0, 0], [1, 0, 0, 16, 12, 0, 0, 0], [0, -4, 6, 40, 30, 0, 0, 0]], dtype=np.int32)
    monkeypatch.setattr(d, "_cutmix_table", lambda n: table)
    extras = {}
    mixed, dev_table = d._cutmix_unl(img, extras)
    assert mixed == "MIXED" and dev_table[0] == "DEV" and torch.equal(dev_table[1], torch.from_numpy(table))
    assert calls[-1][0] is img and torch.equal(calls[-1][1], torch.from_numpy(table)) and calls[-1][2] is dev_table
    # sample 0: 8 x 6; sample 1 is its own partner; sample 2: the box clipped to the map, 16 x 6
    share = extras["unl_cutmix_share"]
    assert share.dtype == torch.float32 and not share.is_cuda and float(share) == np.float32((48 + 96) / (3 * 12 * 16.0))
    # nothing mixes: functional.mix_boxes decides (it returns the batch itself), the table still goes to the head, the share is 0
    calls.clear()
    monkeypatch.setattr(F, "mix_boxes", lambda x, rows, dt=None: calls.append((x, rows, dt)) or x)
    monkeypatch.setattr(d, "_cutmix_table", lambda n: np.array([[0, 0, 0, 9, 9, 0, 0, 0], [0, 4, 4, 4, 9, 0, 0, 0], [7, 0, 0, 9, 9, 0, 0, 0]],
                                                               dtype=np.int32))
    extras = {}
    mixed, dev_table = d._cutmix_unl(img, extras)
    assert mixed is img and dev_table[0] == "DEV" and len(calls) == 1 and float(extras["unl_cutmix_share"]) == 0.0
    calls.clear()
    # a batch of one is never mixed, and says so once
    capsys.readouterr()
    one = torch.zeros(1, 3, 12, 16)
    monkeypatch.setattr(d, "_cutmix_table", lambda n: np.zeros((1, 8), dtype=np.int32))
    assert d._cutmix_unl(one, {}) == (one, None) and d._cutmix_unl(one, {}) == (one, None) and calls == []
    assert capsys.readouterr().out.count("batch of one") == 1
    # the head: the table rides as `mix=`; without one the call is what it was
    seen = []
    sums = torch.tensor([3.0, 54.0, 5.0, 72.0], dtype=torch.float64)
    monkeypatch.setattr(F, "upsample_softmax_teacher",
                        lambda *a, **k: seen.append((a, k)) or (torch.zeros(2, 4, 12, 16), "MSE", "CE", None, None, None,
                                                                {"sums": sums, "pseudo": None, "unl_sums": None}))
    d._unl_head("x", {}, [], [], None, ("T", "FLIP"), "TABLE")
    assert seen[-1] == (("x", (12, 16), "T", d.unl_teacher, None), {"flip": "FLIP", "mix": "TABLE"})
    d._unl_head("x", {}, [], [], None, ("T", "FLIP"))
    assert seen[-1] == (("x", (12, 16), "T", d.unl_teacher, None), {"flip": "FLIP"})
    # the supervised model names the flag it ignores
    import inspect
    assert "--unl_cutmix is ignored" in inspect.getsource(md.supervised_model)


def test_mix_boxes_refuses_mask_words_and_bad_tables():
    F, L = load_sub("functional"), load_sub("_lib")
    x = torch.zeros(2, 3, 5, 7)
    ok = np.array([[1, 0, 0, 3, 3, 0, 0, 0], [0, 1, 1, 4, 4, 0, 0, 0]], dtype=np.int32)
    for word in (5, 6):
        t = ok.copy()
        t[1, word] = 1
        with pytest.raises(ValueError) as e:
            F.mix_boxes(x, t)
        assert "class mask" in str(e.value)
        with pytest.raises(ValueError):
            F.mix_boxes(x, torch.from_numpy(t))
    for bad in (ok.astype(np.int64), ok[:1], ok[:, :5], ok.reshape(-1)):
        with pytest.raises(L.SscgError):
            F.mix_boxes(x, bad)
    with pytest.raises(L.SscgError):
        F.mix_boxes(x, ok)                                          # a good table on a CPU batch: no CPU fallback
    with pytest.raises(L.SscgError):
        F.mix_boxes(x[0], ok)
    live = F.mix_rows_live(torch.tensor([[1, 0, 0, 3, 3, 0, 0, 0], [1, 0, 0, 3, 3, 0, 0, 0], [-1, 0, 0, 3, 3, 0, 0, 0], [6, 0, 0, 3, 3, 0, 0, 0],
                                         [0, 3, 0, 3, 3, 0, 0, 0], [0, 0, 2, 3, 1, 0, 0, 0]], dtype=torch.int32))
    assert live.tolist() == [True, False, False, False, False, False]
    # all existing call signatures stay valid
    import inspect
    assert list(inspect.signature(F.teacher_fwd).parameters)[-1] == "table" and inspect.signature(F.teacher_fwd).parameters["table"].default is None
    p = inspect.signature(F.upsample_softmax_teacher).parameters
    assert list(p)[:7] == ["x", "size", "teacher_logits", "teacher", "unl", "flip", "want_soft"] and p["mix"].default is None


# ------------------------------------------------------------------------------------------ 3. the reference and the GPU tests' inputs
def test_the_tables_cover_what_they_name():
    for gi, (N, H, W, OH, OW) in enumerate(GEOMS):
        tabs = tables_of(gi)
        for name, t in tabs.items():
            assert t.dtype == np.int32 and t.shape == (N, 8) and (t[:, 5:] == 0).all(), name
            mask, partner = pasted(t, OH, OW)
            count = int(mask.sum())
            if name in NOTHING or N == 1:
                assert count == 0, (gi, name)
            elif name.startswith("corner"):
                assert count == N and all(int(mask[n].sum()) == 1 for n in range(N)), (gi, name)
            elif name.endswith("whole"):
                assert count == N * OH * OW, (gi, name)
        if N > 1:
            corners = {tuple(int(v) for v in pasted(tabs[k], OH, OW)[0][0].nonzero()[0]) for k in tabs if k.startswith("corner")}
            assert corners == {(0, 0), (0, OW - 1), (OH - 1, 0), (OH - 1, OW - 1)}
            assert int(pasted(tabs["outside"], OH, OW)[0].sum()) == N * OW * (OH - 4)
            assert tabs["outside"][0, 1] < 0 and tabs["outside"][0, 3] > OW
            assert set(tabs["bad_partner"][:2, 0]) == {-1, N}
        if N == 3:
            assert list(tabs["cycle_a"][:, 0]) == [1, 2, 0] and list(tabs["cycle_b"][:, 0]) == [2, 0, 1]
            assert {FLIPS[gi][p] for p in tabs["cycle_a"][:, 0]} == {0, 1}                  # a cycle meets both flip values
    # 21 x 23: a sample spans two 256-thread blocks and the interior box crosses the seam
    N, H, W, OH, OW = GEOMS[1]
    m = pasted(tables_of(1)["interior"], OH, OW)[0][0].reshape(-1)
    assert OH * OW > 256 and bool(m[:256].any()) and bool(m[256:].any())


def test_the_reference_states_the_mix():
    """a table that mixes nothing is teacher_reference itself, and the whole-map cycle is teacher_reference on the permuted teachers"""
    gi, Cn = 0, 4
    N, H, W, OH, OW = GEOMS[gi]
    x, t, flip, tau, temp = case_inputs(gi, Cn)
    tabs = tables_of(gi)
    plain = teacher_reference(x, t, flip, tau, temp, (OH, OW))
    for name in NOTHING:
        r = mix_teacher_reference(x, t, flip, tabs[name], tau, temp, (OH, OW))
        assert r["K"] == plain["K"] and r["A"] == plain["A"] and torch.equal(r["pseudo"], plain["pseudo"]), name
        assert abs(float(r["mse"]) - float(plain["mse"])) <= 1e-12 and abs(float(r["ce"]) - float(plain["ce"])) <= 1e-12
    for name, perm in (("cycle_a_whole", [1, 2, 0]), ("cycle_b_whole", [2, 0, 1])):
        r = mix_teacher_reference(x, t, flip, tabs[name], tau, temp, (OH, OW))
        want = teacher_reference(x, t[perm], tuple(flip[p] for p in perm), tau, temp, (OH, OW))
        assert r["K"] == want["K"] and r["A"] == want["A"] and torch.equal(r["pseudo"], want["pseudo"]), name
        assert abs(float(r["mse"]) - float(want["mse"])) <= 1e-12 and float((r["grad"] - want["grad"]).abs().max()) <= 1e-12
    # inside the box the map is the partner's aligned, resized map; outside it the sample's own
    m = mixed_teacher(t, flip, tabs["cycle_a"], (OH, OW))
    a = torch.nn.functional.interpolate(mirror_where(t, flip), size=(OH, OW), mode="bilinear", align_corners=True)
    mask = pasted(tabs["cycle_a"], OH, OW)[0]
    for n, p in enumerate([1, 2, 0]):
        assert torch.equal(m[n][:, mask[n]], a[p][:, mask[n]]) and torch.equal(m[n][:, ~mask[n]], a[n][:, ~mask[n]])


def test_the_seed_table_is_the_first_passing_seed():
    assert set(SEEDS) == {(gi, Cn) for gi in range(len(GEOMS)) for Cn in CLASSES}
    for (gi, Cn), seed in SEEDS.items():
        assert 0 <= seed < 40 and seed_ok(seed, gi, Cn), (gi, Cn, seed)
        for s in range(seed):
            assert not seed_ok(s, gi, Cn), (gi, Cn, s)


@pytest.mark.parametrize("Cn", CLASSES)
@pytest.mark.parametrize("gi", range(len(GEOMS)))
def test_the_gpu_inputs_keep_their_margins(gi, Cn):
    """per sample, once: they then hold for every table - checked here for every table all the same"""
    N, H, W, OH, OW = GEOMS[gi]
    x, t, flip, tau, temp = case_inputs(gi, Cn)
    assert torch.equal(x, x.float().double()) and torch.equal(t, t.float().double())       # fp32-representable
    assert tau == TAU[Cn] and temp == TEMP and len(flip) == N
    for name in tables_of(gi):
        ref = reference(gi, Cn, name)
        assert ref["conf_margin"] >= MARGIN and ref["gap_margin"] >= MARGIN, (gi, Cn, name, ref["conf_margin"], ref["gap_margin"])
        if Cn > 1 and name in INTERIOR:
            assert 0.1 <= ref["kept_share"] <= 0.9 and 0.1 <= ref["agree_share"] <= 0.9, (gi, Cn, name, ref["kept_share"], ref["agree_share"])
