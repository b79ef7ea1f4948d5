"""Optimiser options (gradient-norm clip, weight decay, EMA) without a GPU: the argument errors of sscg_grad_norm and
sscg_adam_step_ex come back before any HIP call, the command-line flags parse and leave the defaults alone."""
import ctypes as C
import inspect
import os
import sys

import pytest

from conftest import ROOT, load_sub

BAD_ARG, WORKSPACE = -1, -3
NAN, INF = float("nan"), float("inf")


def _adam_ex(lib, one, **kw):
    a = dict(param=one, grad=one, exp_avg=one, exp_avg_sq=one, shadow=None, shadow_dtype=0, ema=None, n=100, lr=1e-3, beta1=0.9,
             beta2=0.999, eps=1e-8, step=1, grad_scale=1.0, clip=None, weight_decay=0.0, decoupled=0, ema_decay=0.0, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return lib.sscg_adam_step_ex(*a.values())


def test_bindings_and_read_write_table():
    L = load_sub("_lib")
    assert {"sscg_grad_norm_workspace", "sscg_grad_norm", "sscg_adam_step_ex"} <= set(L.SIGNATURES)
    table = L.dev_tool("racecheck").parse_header(os.path.join(ROOT, "include", "sscg.h"))
    kinds = dict(table["sscg_grad_norm"])
    assert kinds["grad"] == "r" and kinds["norm"] == "w" and kinds["clip"] == "w" and kinds["ws"] == "w" and kinds["stream"] == "stream"
    kinds = dict(table["sscg_adam_step_ex"])
    assert kinds["grad"] == "r" and kinds["clip"] == "r"
    assert all(kinds[k] == "w" for k in ("param", "exp_avg", "exp_avg_sq", "shadow", "ema"))
    assert L.lib.sscg_grad_norm_workspace(1) > 0 and L.lib.sscg_grad_norm_workspace(1 << 30) == L.lib.sscg_grad_norm_workspace(1)


def test_grad_norm_argument_errors_are_returned_before_any_launch():
    lib = load_sub("_lib").lib
    one = C.c_void_p(16)          # never dereferenced
    ws = lib.sscg_grad_norm_workspace(100)
    assert lib.sscg_grad_norm(None, 100, 1.0, 1.0, one, one, one, ws, None) == BAD_ARG            # null gradient
    assert lib.sscg_grad_norm(one, 0, 1.0, 1.0, one, one, one, ws, None) == BAD_ARG               # n < 1
    for bad in (0.0, -1.0, NAN):
        assert lib.sscg_grad_norm(one, 100, 1.0, bad, one, one, one, ws, None) == BAD_ARG         # max_norm <= 0 or NaN
    assert lib.sscg_grad_norm(one, 100, 1.0, 1.0, None, None, one, ws, None) == BAD_ARG           # nowhere to write
    assert lib.sscg_grad_norm(C.c_void_p(18), 100, 1.0, 1.0, one, one, one, ws, None) == BAD_ARG  # not 4-byte aligned
    assert lib.sscg_grad_norm(one, 100, 1.0, 1.0, one, one, None, ws, None) == WORKSPACE
    assert lib.sscg_grad_norm(one, 100, 1.0, 1.0, one, one, one, ws - 1, None) == WORKSPACE


def test_adam_step_ex_argument_errors_are_returned_before_any_launch():
    lib = load_sub("_lib").lib
    one = C.c_void_p(16)          # never dereferenced
    # sscg_adam_step's own rules
    for k in ("param", "grad", "exp_avg", "exp_avg_sq"):
        assert _adam_ex(lib, one, **{k: None}) == BAD_ARG
        assert _adam_ex(lib, one, weight_decay=0.1, **{k: None}) == BAD_ARG
    assert _adam_ex(lib, one, n=0, ema=one) == BAD_ARG
    assert _adam_ex(lib, one, step=0, clip=one) == BAD_ARG
    assert _adam_ex(lib, one, shadow=one, shadow_dtype=7, weight_decay=0.1) == BAD_ARG
    # the options' rules
    for bad in (-0.1, NAN, INF, -INF):
        assert _adam_ex(lib, one, weight_decay=bad) == BAD_ARG
        assert _adam_ex(lib, one, weight_decay=bad, decoupled=1) == BAD_ARG
    for bad in (1.0, 1.5, -0.01, NAN, INF):
        assert _adam_ex(lib, one, ema=one, ema_decay=bad) == BAD_ARG


ARGV0 = ["--dataset", "voc2012"]


def _main():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import main
    return main


def test_flags_parse_and_defaults_stay():
    main = _main()
    args = main.get_args(ARGV0)
    assert not {"clip_grad_norm", "weight_decay", "adamw", "ema_decay"} & set(vars(args))       # nothing stored for an absent flag
    assert args.clip_grad_norm is None and args.weight_decay == 0.0 and args.adamw is False and args.ema_decay is None
    md = load_sub("model")
    sig = inspect.signature(load_sub("optim").FusedAdam.__init__).parameters
    for ema in (True, False):
        kw = md._optim_options(args, ema=ema)
        assert kw == {k: sig[k].default for k in ("weight_decay", "decoupled", "max_grad_norm", "ema_decay")}
        assert kw == dict(weight_decay=0.0, decoupled=False, max_grad_norm=None, ema_decay=None)
    args = main.get_args(ARGV0 + ["--clip_grad_norm", "2.5", "--weight_decay", "1e-4", "--adamw", "--ema_decay", "0.999"])
    assert md._optim_options(args, ema=True) == dict(weight_decay=1e-4, decoupled=True, max_grad_norm=2.5, ema_decay=0.999)
    assert md._optim_options(args, ema=False) == dict(weight_decay=1e-4, decoupled=True, max_grad_norm=2.5, ema_decay=None)
    # a namespace of an existing caller (no such attribute at all) gives the defaults too
    assert md._optim_options(object(), ema=True) == dict(weight_decay=0.0, decoupled=False, max_grad_norm=None, ema_decay=None)


@pytest.mark.parametrize("argv, word", [(["--adamw"], "--weight_decay"), (["--adamw", "--weight_decay", "0"], "--weight_decay"),
                                        (["--weight_decay", "-1"], "--weight_decay"), (["--clip_grad_norm", "0"], "--clip_grad_norm"),
                                        (["--ema_decay", "1.0"], "--ema_decay")])
def test_bad_flag_values_are_rejected_with_a_clear_message(argv, word, capsys):
    with pytest.raises(SystemExit) as e:
        _main().get_args(ARGV0 + argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "error:" in err and word in err
    if argv == ["--adamw"]:
        assert "--adamw" in err and "needs --weight_decay" in err
