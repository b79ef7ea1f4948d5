"""Eval-mode BatchNorm folded into the conv (sscg_conv2d_fwd_affine) on the MI355X.  The contract is BIT IDENTITY with the
separate passes it replaces (sscg_conv2d_fwd -> sscg_rstd_from_var -> sscg_norm_apply), so every comparison is torch.equal."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, load_sub

pytestmark = pytest.mark.gpu
CL = torch.channels_last
RELU, LRELU, NONE = 1, 2, 0

# (name, N, H, W, C, K, ksize, stride, pad, dil, activation, residual)
GEOMS = [
    ("1x1_64_256_res_relu", 8, 33, 33, 64, 256, 1, 1, 0, 1, RELU, True),          # bn3 + shortcut -> ReLU
    ("1x1_256_64_relu", 8, 33, 33, 256, 64, 1, 1, 0, 1, RELU, False),
    ("3x3_d2_256_relu", 8, 33, 33, 256, 256, 3, 1, 2, 2, RELU, False),
    ("3x3_d4_512_relu", 8, 33, 33, 512, 512, 3, 1, 4, 4, RELU, False),
    ("3x3_d4_256_relu", 8, 33, 33, 256, 256, 3, 1, 4, 4, RELU, False),
    ("3x3_d2_512_relu", 8, 33, 33, 512, 512, 3, 1, 2, 2, RELU, False),
    ("1x1_s2_256_512_none", 8, 65, 65, 256, 512, 1, 2, 0, 1, NONE, False),        # the downsample pair
    ("1x1_1024_2048_none", 8, 33, 33, 1024, 2048, 1, 1, 0, 1, NONE, False),
    ("one_tile", 1, 8, 8, 64, 64, 1, 1, 0, 1, RELU, True),
    ("3x3_d2_256_big_lrelu", 16, 65, 65, 256, 256, 3, 1, 2, 2, LRELU, True),      # 67600 rows: the 128x128 class
    ("1x1_256_1024_res_relu", 8, 33, 33, 256, 1024, 1, 1, 0, 1, RELU, True),
]


def make(dev, mode, N, H, W, C, K, k, seed):
    g = torch.Generator().manual_seed(seed)
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    x = torch.randn(N, C, H, W, generator=g).to(dev).contiguous(memory_format=CL).to(dt)
    w = (torch.randn(K, C, k, k, generator=g) * (1.0 / (C * k * k) ** 0.5)).to(dev).contiguous(memory_format=CL)
    bias = (torch.randn(K, generator=g) * 0.1).to(dev)
    rm = (torch.randn(K, generator=g) * 0.3).to(dev)
    rv = (torch.rand(K, generator=g) * 1.5 + 0.25).to(dev)
    ga = (torch.randn(K, generator=g) * 0.2 + 1.0).to(dev)
    be = (torch.randn(K, generator=g) * 0.2).to(dev)
    return x, w, bias, rm, rv, ga, be, g, dt


@pytest.fixture
def mode(request, F):
    F.set_conv_precision(request.param)
    yield request.param
    F.set_conv_precision("f32")


def separate(F, x, w, bias, rm, rv, ga, be, res, stride, pad, dil, eps, act, slope):
    y = F.conv2d(x, w, bias, stride, pad, dil, 0, 0, 0.0, out_f32=False)
    return F.batch_norm_act(y, ga, be, rm, rv, False, 0.1, eps, act, slope, res)


# ------------------------------------------------------------------------------------------ 1. unit parity
@pytest.mark.parametrize("mode", ["f32s", "bf16"], indirect=True)
@pytest.mark.parametrize("geom", GEOMS, ids=[g[0] for g in GEOMS])
def test_fused_unit_equals_the_separate_passes(F, dev, geom, mode):
    name, N, H, W, C, K, k, stride, pad, dil, act, with_res = geom
    x, w, bias, rm, rv, ga, be, g, dt = make(dev, mode, N, H, W, C, K, k, 17 * C + K + H)
    P = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
    Q = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    res = torch.randn(N, K, P, Q, generator=g).to(dev).contiguous(memory_format=CL).to(dt) if with_res else None
    slope = 0.2 if act == LRELU else 0.0
    with torch.no_grad():
        assert F.conv_bn_eval_applies(x, w, stride, pad, dil, 0, act, slope)
        if name == "3x3_d2_256_relu" and mode == "f32s":
            # the plan of this launch cuts its tail along K: the reduction carries the affine
            d = F.make_desc(x.shape, w.shape, stride, pad, dil, 0, act, slope, 0, 2, 0, 0, F.weight_split(w)[1])
            assert F._ws_bytes(d, "fwd") > 0
        for gamma, beta, b in ((ga, be, None), (None, None, None), (ga, be, bias)):
            want = separate(F, x, w, b, rm, rv, gamma, beta, res, stride, pad, dil, 1e-5, act, slope)
            got = F.conv_bn_eval_act(x, w, b, rm, rv, gamma, beta, res, stride, pad, dil, 0, 1e-5, act, slope)
            assert got.dtype == want.dtype and got.shape == want.shape
            assert torch.isfinite(got.float()).all()
            assert torch.equal(got, want), "%s %s: %d of %d elements differ, max |d| %.3e" % (
                name, mode, int((got != want).sum()), got.numel(), float((got.float() - want.float()).abs().max()))
        if act == RELU:
            assert float(got.float().min()) == 0.0 and float(got.float().max()) > 0.0


@pytest.mark.parametrize("mode", ["f32s", "bf16"], indirect=True)
def test_unserved_geometries_fall_back_to_the_separate_passes(F, dev, mode):
    """21 output channels (the heads' 32-column class) and - in fp32 - a 3-channel stem: `_applies` is 0, the function still answers,
    with the separate passes' bits."""
    cases = [(2, 17, 17, 64, 21, 3, 1, 1, 1)]
    if mode == "f32s":
        cases.append((2, 32, 32, 3, 64, 7, 2, 3, 1))
    for (N, H, W, C, K, k, stride, pad, dil) in cases:
        x, w, bias, rm, rv, ga, be, g, dt = make(dev, mode, N, H, W, C, K, k, 5)
        with torch.no_grad():
            assert not F.conv_bn_eval_applies(x, w, stride, pad, dil, 0, RELU, 0.0)
            want = separate(F, x, w, None, rm, rv, ga, be, None, stride, pad, dil, 1e-5, RELU, 0.0)
            got = F.conv_bn_eval_act(x, w, None, rm, rv, ga, be, None, stride, pad, dil, 0, 1e-5, RELU, 0.0)
            assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------ 2. network parity
def deeplab(dev, seed=3, classes=21):
    import contextlib
    import io
    gen = load_sub("arch.generators")
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        net = gen.define_Gen(3, classes, 64, "deeplab", gpu_ids=[0])
    g = torch.Generator().manual_seed(seed + 1)
    ops = load_sub("arch.ops")
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, ops.BatchNorm2d):
                m.running_mean.copy_((torch.randn(m.num_features, generator=g) * 0.05).to(dev))
                m.running_var.copy_((torch.rand(m.num_features, generator=g) * 0.5 + 0.75).to(dev))
    return net


@pytest.mark.parametrize("mode", ["f32s", "bf16"], indirect=True)
def test_deeplab_eval_logits_are_the_same_bits(F, dev, mode):
    net = deeplab(dev).eval()
    ops = load_sub("arch.ops")
    tracked = [m.batches_tracked() for m in net.modules() if isinstance(m, ops.BatchNorm2d)]
    g = torch.Generator().manual_seed(11)
    try:
        for (H, W) in ((256, 256), (256, 512)):
            x = torch.randn(2, 3, H, W, generator=g).to(dev)
            with torch.no_grad():
                F.FUSE_EVAL_NORM[0] = True
                a = net(x)
                F.FUSE_EVAL_NORM[0] = False
                b = net(x)
            assert a.shape == b.shape and torch.isfinite(a).all() and float(a.abs().max()) > 0
            assert torch.equal(a, b), "%dx%d %s: %d logits differ" % (H, W, mode, int((a != b).sum()))
    finally:
        F.FUSE_EVAL_NORM[0] = True
    assert tracked == [m.batches_tracked() for m in net.modules() if isinstance(m, ops.BatchNorm2d)]      # eval forwards count no batch


def test_evaluate_confusion_matrices_are_equal(F, dev):
    utils = load_sub("utils")
    net = deeplab(dev).eval()
    g = torch.Generator().manual_seed(5)
    batches = [(torch.randn(2, 3, 128, 128, generator=g).to(dev), torch.randint(0, 21, (2, 128, 128), generator=g).to(dev)) for _ in range(2)]
    conf = []
    try:
        for fused in (True, False):
            F.FUSE_EVAL_NORM[0] = fused
            score = utils.runningScore(21, "voc2012")
            with torch.no_grad():
                for img, gt in batches:
                    score.update_logits(gt, net(img), (128, 128))
            score.get_scores()
            conf.append(score.confusion_matrix.copy())
    finally:
        F.FUSE_EVAL_NORM[0] = True
    assert conf[0].sum() == 2 * 2 * 128 * 128 and (conf[0] == conf[1]).all()


# ------------------------------------------------------------------------------------------ 3. launch census
CENSUS = r"""
import contextlib, io, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
from conftest import load_sub
gen, ops = load_sub("arch.generators"), load_sub("arch.ops")
with contextlib.redirect_stdout(io.StringIO()):
    net = gen.define_Gen(3, 21, 64, "deeplab", gpu_ids=[0]).eval()
units = thin = 0
for m in net.modules():
    if isinstance(m, ops.BatchNorm2d):
        units += 1
for m in net.modules():
    if isinstance(m, ops.Conv2d) and m.in_channels < 32:
        thin += 1
x = torch.randn(1, 3, 128, 128).cuda()
with torch.no_grad():
    net(x)                      # operand copies are made here
    torch.cuda.synchronize()
    sys.stderr.write("[census] begin\n")
    net(x)
    torch.cuda.synchronize()
    sys.stderr.write("[census] end\n")
print("units", units, "thin", thin)
"""


def census(env_extra):
    env = dict(os.environ, SSCG_TRACE="1")
    env.pop("SSCG_FUSE_EVAL_NORM", None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", CENSUS % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    err = r.stderr
    body = err[err.index("[census] begin"):err.index("[census] end")]
    calls = {}
    for line in body.splitlines():
        if line.startswith("[sscg] "):
            name = line[7:].split("(")[0]
            calls[name] = calls.get(name, 0) + 1
    words = r.stdout.split()
    return calls, int(words[words.index("units") + 1]), int(words[words.index("thin") + 1])


def test_launch_census_of_one_deeplab_eval_forward():
    calls, units, thin = census({})
    assert units >= 100 and thin == 1          # DeepLab-ResNet101: 104 conv -> BN units, one of them behind the 3-channel stem
    assert calls.get("sscg_norm_apply", 0) <= thin and calls.get("sscg_rstd_from_var", 0) <= thin, calls
    assert calls.get("sscg_conv2d_fwd_affine", 0) == units - thin, calls
    plain, _, _ = census({"SSCG_FUSE_EVAL_NORM": "0"})
    assert plain.get("sscg_conv2d_fwd_affine", 0) == 0 and plain.get("sscg_norm_apply", 0) == units, plain


# ------------------------------------------------------------------------------------------ 4. guards
def test_an_input_that_requires_grad_is_refused(F, dev):
    L = load_sub("_lib")
    x, w, bias, rm, rv, ga, be, g, dt = make(dev, "f32", 1, 8, 8, 64, 64, 1, 9)
    x.requires_grad_(True)
    with pytest.raises(L.SscgError):
        F.conv_bn_eval_act(x, w, None, rm, rv, ga, be)
    with torch.no_grad():
        F.conv_bn_eval_act(x, w, None, rm, rv, ga, be)


def test_a_train_forward_after_an_eval_forward_is_unchanged(F, dev):
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(2)).to(dev)
    outs = []
    for with_eval in (False, True):
        net = deeplab(dev, seed=8)
        if with_eval:
            net.eval()
            with torch.no_grad():
                net(x)
        net.train()
        with torch.no_grad():
            outs.append(net(x))
        outs.append(torch.cat([m.running_mean for m in net.modules() if hasattr(m, "running_mean")]))
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])
