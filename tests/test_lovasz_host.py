"""Lovasz-softmax loss, host side (no GPU): the options and the command line parse and validate, the entries refuse bad arguments
before any HIP call, the reference's closed-form Lovasz gradient equals the difference form, the loss does not depend on how tied
errors are ordered, and on every input the GPU end-to-end test uses the fp32 order of the errors is the fp64 order."""
import ctypes as C
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_sub
from lovasz_reference import (GEOMS, LABELS, OPTIONS, errors, lovasz_grad_closed, lovasz_grad_diff, lovasz_reference, make_case,
                              probabilities, sort_u32_desc_reference, stable_desc_argsort)


def test_options_parse_and_validate():
    F = load_sub("functional")
    o = F.LovaszOptions()
    assert (o.classes, o.per_image, o.skip) == ("present", False, ())
    o = F.LovaszOptions(classes="all", per_image=1, skip=[3, 0])
    assert (o.classes, o.per_image, o.skip) == ("all", True, (0, 3)) and o.skip_mask(4) == 0b1001
    assert F._lovasz_options(dict(classes="all")).classes == "all" and F._lovasz_options(None).classes == "present"
    for bad in (dict(classes="some"), dict(skip=(1, 1)), dict(skip=(-1,)), dict(skip=(64,)), dict(skip=(1.5,)), dict(skip=(True,))):
        with pytest.raises(ValueError):
            F.LovaszOptions(**bad)
    with pytest.raises(ValueError):
        F.LovaszOptions(skip=(4,)).skip_mask(4)                                   # a class id past the class count
    with pytest.raises(ValueError):
        F.LovaszOptions(classes="all", skip=(0, 1, 2, 3)).skip_mask(4)            # nothing left to average
    assert F.LovaszOptions(classes="present", skip=(0, 1, 2, 3)).skip_mask(4) == 15   # "present" may be empty: the loss is 0
    with pytest.raises(TypeError):
        F._lovasz_options("present")


def test_command_line():
    sys.path.insert(0, ROOT)
    import main
    a = main.get_args([])
    assert (a.lovasz_weight, a.lovasz_per_image, a.lovasz_classes, a.lovasz_skip) == (0.0, False, "present", "")
    assert not any(k.startswith("lovasz") for k in vars(a))                       # SUPPRESS: a run without the flags parses as it did
    a = main.get_args(["--lovasz_weight", "0.5", "--lovasz_per_image", "--lovasz_classes", "all", "--lovasz_skip", "0, 20"])
    assert (a.lovasz_weight, a.lovasz_per_image, a.lovasz_classes, a.lovasz_skip) == (0.5, True, "all", "0, 20")
    for bad in (["--lovasz_weight", "-1"], ["--lovasz_weight", "inf"], ["--lovasz_weight", "nan"], ["--lovasz_classes", "some"],
                ["--lovasz_skip", "21"], ["--lovasz_skip", "a"], ["--dataset", "acdc", "--lovasz_skip", "0,1,2,3"]):
        with pytest.raises(SystemExit):
            main.get_args(bad)
    U = load_sub("utils")
    assert U.parse_lovasz_skip("", 4) == () and U.parse_lovasz_skip(" 3,0 ,3", 4) == (0, 3)
    for bad in ("4", "x", "0,1,2,3", "1,,2"):
        with pytest.raises(ValueError):
            U.parse_lovasz_skip(bad, 4)


def test_entries_refuse_bad_arguments_before_any_hip_call():
    L = load_sub("_lib")
    F = load_sub("functional")
    lib = L.lib
    BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
    one = C.c_void_p(16)                                                          # never dereferenced
    # the sort
    assert lib.sscg_sort_chunk() > 0 and lib.sscg_sort_ws_bytes(5, 257) > 0
    assert lib.sscg_sort_ws_bytes(0, 4) == 0 and lib.sscg_sort_ws_bytes(1 << 16, 1 << 15) == 0
    ws = lib.sscg_sort_ws_bytes(5, 257)
    assert lib.sscg_sort_u32_desc(None, 5, 257, 0, one, one, one, ws, None) == BAD_ARG
    assert lib.sscg_sort_u32_desc(one, 5, 257, 0, one, one, one, ws, None) == BAD_ARG                 # out == in
    assert lib.sscg_sort_u32_desc(one, 0, 257, 0, C.c_void_p(32), one, one, ws, None) == BAD_ARG
    assert lib.sscg_sort_u32_desc(one, 1 << 16, 1 << 15, 0, C.c_void_p(32), one, one, 1 << 40, None) == UNSUPPORTED
    assert lib.sscg_sort_u32_desc(one, 5, 257, 0, C.c_void_p(32), one, one, ws - 1, None) == WORKSPACE  # one byte short
    assert lib.sscg_sort_u32_desc(one, 5, 257, 0, C.c_void_p(32), one, None, ws, None) == WORKSPACE
    # the loss
    n = lib.sscg_lovasz_workspace(2, 13, 19, 4, 0)
    assert n > 0 and lib.sscg_lovasz_workspace(2, 13, 19, 65, 0) == 0 and lib.sscg_lovasz_workspace(64, 2048, 2048, 21, 1) == 0
    a = (2, 5, 7, 4, 13, 19)
    assert lib.sscg_lovasz_fwd(None, one, *a, 0, 0, 0, one, one, one, None, one, n, None) == BAD_ARG
    assert lib.sscg_lovasz_fwd(one, one, *a, 2, 0, 0, one, one, one, None, one, n, None) == BAD_ARG       # classes flag outside {0, 1}
    assert lib.sscg_lovasz_fwd(one, one, *a, 0, 0, 1 << 4, one, one, one, None, one, n, None) == BAD_ARG  # a skip bit at class 4 of 4
    assert lib.sscg_lovasz_fwd(one, one, *a, 1, 0, 15, one, one, one, None, one, n, None) == BAD_ARG      # "all" with every class skipped
    assert lib.sscg_lovasz_fwd(one, one, 2, 5, 7, 65, 13, 19, 0, 0, 0, one, one, one, None, one, n, None) == BAD_ARG
    assert lib.sscg_lovasz_fwd(one, one, 64, 33, 33, 21, 2048, 2048, 0, 0, 0, one, one, one, None, one, 1 << 40, None) == UNSUPPORTED
    assert lib.sscg_lovasz_fwd(one, one, *a, 0, 0, 0, one, one, one, None, one, n - 1, None) == WORKSPACE
    assert lib.sscg_lovasz_scale_add(None, one, None, one, 8, None) == BAD_ARG
    assert lib.sscg_lovasz_scale_add(one, one, None, one, 0, None) == BAD_ARG
    # the operators: no CPU fallback, fp32 only, the option checks come first
    x, lab = torch.zeros(2, 4, 13, 19), torch.zeros(2, 13, 19, dtype=torch.int64)
    with pytest.raises(L.SscgError):
        F.lovasz_softmax(x, lab)
    with pytest.raises(L.SscgError):
        F.sort_u32_desc(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(TypeError):
        F.lovasz_softmax(x, lab, "all")
    with pytest.raises(ValueError):
        F.upsample_softmax_losses(x, (13, 19), lab, lovasz=dict(classes="none"))
    if torch.cuda.is_available():
        with pytest.raises(L.SscgError):
            F.lovasz_softmax(x.cuda().half(), lab.cuda())                                               # a non-fp32 input
        with pytest.raises(ValueError):
            F.lovasz_softmax(x.cuda(), lab.cuda(), F.LovaszOptions(classes="all", skip=(0, 1, 2, 3)))


def test_closed_form_gradient_equals_the_difference_form():
    rng = np.random.RandomState(5)
    worst = 0.0
    for V in (1, 2, 3, 17, 494, 5000):
        for mode in ("none", "all", "random", "sparse", "first", "last"):
            f = {"none": np.zeros(V, bool), "all": np.ones(V, bool), "random": rng.rand(V) < 0.5, "sparse": rng.rand(V) < 0.02,
                 "first": np.arange(V) == 0, "last": np.arange(V) == V - 1}[mode]
            a, b = lovasz_grad_closed(f), lovasz_grad_diff(f)
            # the difference form cancels: each J = 1 - I / U carries two roundings of numbers <= 1 (2^-54 each), their difference
            # one more, the closed form three roundings of a g <= 1: below 8 * 2^-53 in all
            assert np.abs(a - b).max() <= 8 * 2.0 ** -53, (V, mode, np.abs(a - b).max())
            assert abs(a.sum() - (1.0 if V else 0.0)) <= 1e-12 * V                 # J_V = 1: the gradient sums to 1
            assert (a >= 0).all()
            worst = max(worst, float(np.abs(a - b).max()))
    # an absent class (G = 0): J_1 = 1, so g = (1, 0, 0, ...); a full class (G = V): g_j = 1 / V
    assert lovasz_grad_closed(np.zeros(5, bool)).tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
    assert lovasz_grad_closed(np.ones(4, bool)).tolist() == [0.25] * 4
    print("lovasz closed vs difference form: max |diff| %.2e" % worst)


def test_the_loss_does_not_depend_on_the_order_of_tied_errors():
    rng = np.random.RandomState(11)
    N, Cn, H, W = 1, 3, 6, 8
    lab = torch.from_numpy(rng.randint(0, Cn, size=(N, H, W)).astype(np.int64))
    vals = np.asarray([0.125, 0.25, 0.5])                                          # few distinct probabilities: heavy ties
    p = torch.from_numpy(vals[rng.randint(0, 3, size=(N, Cn, H, W))])
    base = float(lovasz_reference(p, lab, classes="all"))
    e = errors(p, lab).numpy()
    for trial in range(5):
        # keys that keep the order of distinct errors and permute the tied ones
        keys = (e * 1024).astype(np.int64) * 1000 + rng.permutation(N * Cn * H * W).reshape(e.shape) % 1000
        assert abs(float(lovasz_reference(p, lab, classes="all", keys=keys)) - base) <= 1e-13      # (48 terms per class, a rounding of 2^-53 each: 1e-13 is generous)


def test_stable_sort_reference():
    k = np.asarray([[3, 1, 3, 0, 1, 0xFFFFFFFF]], dtype=np.uint32)
    s, i = sort_u32_desc_reference(k)
    assert s.tolist() == [[0xFFFFFFFF, 3, 3, 1, 1, 0]] and i.tolist() == [[5, 0, 2, 1, 4, 3]]


@pytest.mark.parametrize("labels", LABELS)
@pytest.mark.parametrize("geom", GEOMS, ids=[g[0] for g in GEOMS])
def test_fp32_and_fp64_orders_agree_on_the_committed_seeds(geom, labels):
    """Every segment and class of every input tests/test_lovasz_gpu.py feeds end to end: the descending stable order of the errors
    computed in fp32 on the CPU is the order in fp64 - no pixel and no class is left out."""
    name, N, Cn, H, W, OH, OW = geom
    x, lab = make_case(geom, labels)
    rs = None if (OH, OW) == (H, W) else (OH, OW)
    e64 = errors(probabilities(x, rs), lab).numpy()
    e32 = errors(probabilities(x.float(), rs), lab).numpy()
    assert e32.dtype == np.float32
    counted = ((lab >= 0) & (lab < Cn)).numpy()
    for seg in [[n] for n in range(N)] + [list(range(N))]:
        m = counted[seg].reshape(-1)
        for c in range(Cn):
            a, b = e32[seg, c].reshape(-1)[m], e64[seg, c].reshape(-1)[m]
            assert np.array_equal(stable_desc_argsort(a), stable_desc_argsort(b)), (name, labels, seg, c)
