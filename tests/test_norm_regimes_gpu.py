"""csrc/norm.hip in the regimes the training step runs it in: many reduce chunks per group (the finalize kernels' lanes take a second
chunk), several rounds of a slab kernel's row loop per block, ragged last chunks, the flat kernels on millions of vectors, and the
column sum on hundreds of thousands of rows.  The other kernel-level tests stop at maps of 19x23 pixels: one round, at most 6 chunks.

Every (group, channel) has its own mean and standard deviation, and gamma / beta differ per channel, so a kernel that reads a
neighbouring channel's or group's parameters is wrong by tens of percent, not by the 2 / sqrt(L) that separates two sample means of
one distribution.

References are closed-form fp64 tensor expressions on the CPU, evaluated on the values the device tensors hold (bf16 tensors:
rounded first).  Every test prints its figures (`norm_regimes ...`, shown by `pytest -s`) before it asserts; profiles/norm_regimes.txt
holds the distance of a plain-fp32 evaluation of the same expressions from the reference, the yardstick of the bounds.

The regimes beside each case were read off a Python mirror of plan_reduce / plan_slab (csrc/norm.hip).  A change of either planner
has to revisit them: the cases are the smallest shapes that reach each regime, not shapes that reach them whatever the plan."""
import functools
import os

import pytest
import torch

from conftest import load_sub

pytestmark = pytest.mark.gpu
CL = torch.channels_last
F32 = torch.float32
BF = torch.bfloat16
EPS16 = 2.0 ** -8          # one bf16 rounding: relative error <= 2^-9 of the value, compared against the tensor's max
EPS = 1e-5
SLOPE = 0.2
MOMENTUM = 0.1
# Inputs keep every pre-activation value at least GUARD away from zero (see _inputs): the derivative of ReLU / LeakyReLU jumps there,
# and a kernel whose fp32 pre-activation (error ~1e-6 at these magnitudes) falls on the other side is not wrong.
GUARD = 1e-4

# fp32 bounds: those of test_norm_act; bf16: those of test_norm_act_bf16 (the fp32 outputs of bf16 runs - mean, rstd, dgamma,
# dbeta - take the fp32 bounds).  profiles/norm_regimes.txt: a plain-fp32 CPU evaluation of the reference's expressions at these sizes
# is 60-100x (fp32) and 1.2-2.7x (bf16, one rounding of the result) inside them.
TOL = {F32: dict(y=1e-5, dx=2e-5, dres=1e-6), BF: dict(y=EPS16, dx=2 * EPS16, dres=EPS16)}
TOL_STAT = 1e-5            # mean, rstd, running statistics, dgamma, dbeta

# id: dtype, NCHW shape, per_sample (True InstanceNorm, False BatchNorm, k BatchNorm over k stacked batches) -> (G, L, C)
CASES = {
    # (2, 40000, 16): reduce CW=4, 79 chunks by rows (a finalize lane takes chunks k and k + 64), last chunk 454 of 507 rows;
    # slab <4,4> with cw=4 (64 row lanes), 157 chunks of one round, last 64 of 256 rows
    "A": (F32, (2, 16, 200, 200), True),
    # (1, 33800, 64): DeepLab layer1 BatchNorm of the step: 128 chunks by budget, last chunk 145 of 265 rows; slab 529 chunks of one
    # round, last 8 of 64 rows
    "B": (F32, (8, 64, 65, 65), False),
    # (8, 33000, 64): slab <4,4> limited by the block budget: 258 chunks of 128 rows = 2 rounds each, last 104 of 128; reduce 128
    # chunks, last 234 of 258 rows; eight groups
    "C": (F32, (8, 64, 150, 220), True),
    # (2, 65536, 21) and (2, 65536, 3): no slab plan (VEC=1): the flat kernels on 2.7 M / 0.4 M vectors, fd_div on row indices up to
    # 131071; VEC=1 reduce with ragged column groups (21 of 32, 3 of 4 lanes), 128 chunks of 512 rows
    "D21": (F32, (2, 21, 256, 256), True),
    "D3": (F32, (2, 3, 256, 256), True),
    # (1, 8712, 2048): DeepLab layer4: slab cw=256 (one row lane), two channel slabs, 1089 chunks of 8 rows = 2 rounds; reduce 32
    # channel slabs x 64 chunks, last 81 of 137 rows
    "G": (F32, (8, 2048, 33, 33), False),
    # (3, 5000, 72): 18 column groups, not a power of two: VEC=4 flat kernels; reduce 2 slabs, the second ragged (2 of 16 lanes), 40
    # chunks of 125 rows; three BatchNorm groups (running statistics advance three times)
    "H": (F32, (6, 72, 50, 50), 3),
    # (16, 16500, 64) bf16: slab <8,2> 129 chunks of 128 rows = 2 rounds (last 116), backward slab <8,1> 172 chunks of 96 rows = 3
    # rounds (last 84); reduce VEC=8, 65 chunks of 254 rows (last 244)
    "E": (BF, (16, 64, 100, 165), True),
    # (1, 34320, 256) bf16: config-3 BatchNorm: reduce 2 channel slabs x 128 chunks, last 157 of 269 rows; slab apply 2145 chunks of
    # one round (16 rows), backward slab 2 rounds of 8
    "I": (BF, (16, 256, 33, 65), False),
    # (2, 20000, 132) bf16, 132 % 8 != 0: VEC=4, 33 column groups: flat kernels on bf16; reduce 3 slabs, the last ragged (1 of 16
    # lanes), 128 chunks of 157 rows (last 61); two BatchNorm groups
    "J": (BF, (4, 132, 100, 100), 2),
    # (1, 8712, 2048) bf16: slab cw=256: apply <8,2> 2178 chunks of 4 rows = 2 rounds, backward <8,1> 2904 chunks of 3 rows = 3
    # rounds; reduce 16 slabs x 69 chunks, last 76 of 127 rows
    "K": (BF, (8, 2048, 33, 33), False),
}
# rows per chunk and per round of the slab kernels (apply, backward) for the cases whose blocks run more than one round
SLAB_ROWS = {"C": ((128, 64), (128, 64)), "G": ((8, 4), (8, 4)), "E": ((128, 64), (96, 32)), "K": ((4, 2), (3, 1))}


def _frac(t):
    return t - t.floor()


def _rnd(t, dtype):
    """fp32 copy of t rounded to dtype (what a tensor of that dtype holds)."""
    return t.float().to(dtype).float()


def _table(G, L, C, dtype, seed, col_shift=0.0):
    """[G][L][C] values, rounded to dtype: group g, channel c has mean 0.5 (c % 7) - 1.5 + 0.75 g (+ col_shift c) and standard deviation
    0.5 + 0.25 (c % 5)."""
    gen = torch.Generator().manual_seed(seed)
    ch = torch.arange(C, dtype=torch.float32)
    mu = 0.5 * (ch % 7) - 1.5 + col_shift * ch + 0.75 * torch.arange(G, dtype=torch.float32)[:, None]
    sd = 0.5 + 0.25 * (ch % 5)
    x = torch.randn(G, L, C, generator=gen)
    x.mul_(sd).add_(mu[:, None, :])
    return _rnd(x, dtype)


def _affine(C):
    """gamma in [0.75, 1.25), beta in [-0.4, 0.4): low-discrepancy sequences, distinct per channel, neighbours 0.1 - 0.3 apart."""
    ch = torch.arange(C, dtype=torch.float64)
    return (0.75 + 0.5 * _frac(ch * 0.6180339887498949)).float(), (-0.4 + 0.8 * _frac(ch * 0.7548776662466927)).float()


def _glc_of(shape, per):
    n, c, h, w = shape
    G = n if per is True else (1 if per is False else int(per))
    return G, n * h * w // G, c


@functools.lru_cache(maxsize=2)
def _inputs(cid):
    """The one input builder: x, dy, residual as [G][L][C] fp32 CPU tensors holding values of the case's dtype, gamma / beta, and the
    fp64 statistics of x.  `affine`: the case is a BatchNorm (the autograd unit applies gamma and beta).  Where the unit's
    pre-activation gamma * xhat + beta + residual is within GUARD of zero the residual is moved by 0.5."""
    dtype, shape, per = CASES[cid]
    G, L, C = _glc_of(shape, per)
    seed = 100 + sorted(CASES).index(cid)
    x = _table(G, L, C, dtype, seed)
    gen = torch.Generator().manual_seed(seed + 50)
    dy = _rnd(torch.randn(G, L, C, generator=gen), dtype)
    res = _rnd(torch.randn(G, L, C, generator=gen), dtype)
    gamma, beta = _affine(C)
    affine = per is not True
    xd = x.double()
    mean = xd.mean(1)
    var = (xd - mean[:, None, :]).square_().mean(1)
    rstd = (var + EPS).rsqrt()
    z = xd.sub_(mean[:, None, :]).mul_(rstd[:, None, :])
    if affine:
        z.mul_(gamma.double()).add_(beta.double())
    z.add_(res)
    near = z.abs() < GUARD
    if near.any():
        moved = _rnd(res[near] + 0.5, dtype)
        assert float((z[near] + (moved.double() - res[near].double())).abs().min()) > GUARD
        res[near] = moved
    return dict(cid=cid, dtype=dtype, shape=shape, per=per, G=G, L=L, C=C, affine=affine, x=x, dy=dy, res=res, gamma=gamma, beta=beta,
                mean=mean, var=var, rstd=rstd)


def _act(z, act):
    if act == "relu":
        return z.clamp_min(0)
    if act == "lrelu":
        return torch.where(z > 0, z, z * SLOPE)
    return z


def _reference(inp, act, dt=torch.float64):
    """y = act(gamma * xhat + beta + res) and its backward in closed form.  dt = float64: the reference.  dt = float32: the same
    expressions in plain fp32 with fp64 accumulation of the sums, as the kernels have them (the yardstick for a bound, see TOL)."""
    L = inp["L"]
    x, dy, res = inp["x"].to(dt), inp["dy"].to(dt), inp["res"].to(dt)
    mean, rstd = inp["mean"].to(dt)[:, None, :], inp["rstd"].to(dt)[:, None, :]
    xhat = (x - mean) * rstd
    z = xhat
    ga = None
    if inp["affine"]:
        ga = inp["gamma"].to(dt)
        z = z * ga + inp["beta"].to(dt)
    z = z + res
    y = _act(z, act)
    if act == "relu":
        g = dy * (z > 0)
    elif act == "lrelu":
        g = torch.where(z > 0, dy, dy * SLOPE)
    else:
        g = dy
    gx = g.double() * xhat.double()
    sg, sgx = g.double().sum(1), gx.sum(1)
    c1, c2 = (sg / L).to(dt)[:, None, :], (sgx / L).to(dt)[:, None, :]
    dx = (g - c1 - xhat * c2) * rstd
    if ga is not None:
        dx = dx * ga
    return dict(y=y, dx=dx, dres=g, dgamma=sgx.sum(0), dbeta=sg.sum(0), dgamma_scale=gx.abs().sum((0, 1)),
                dbeta_scale=g.double().abs().sum((0, 1)))


def _dev(inp, t, dev):
    """[G][L][C] CPU tensor -> the case's NCHW-shaped channels-last device tensor of its dtype."""
    n, c, h, w = inp["shape"]
    return t.to(dev).to(inp["dtype"]).view(n, h, w, c).permute(0, 3, 1, 2)


def _glc(t, inp):
    return t.detach().permute(0, 2, 3, 1).reshape(inp["G"], inp["L"], inp["C"])


def _maxnorm(got, ref, dev):
    """max |got - ref| / max |ref| (the measure of test_norm_act), evaluated on the device."""
    r = ref.to(dev).double()
    return float((got.double() - r).abs().max() / r.abs().max())


def _per_element(got, ref, scale=None):
    """max over a small table of |got - ref| / |ref| (or / scale), element by element."""
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.double()
    return float(((got - ref).abs() / (ref.abs() if scale is None else scale)).max())


class _Figures:
    """Prints every figure when it is taken; asserts them all at the end, so that one run shows the whole case."""

    def __init__(self, label):
        self.label, self.bad = label, []

    def add(self, name, err, bound):
        print("norm_regimes %s %s err %.3e bound %.3e" % (self.label, name, err, bound))
        if not err < bound:         # (a NaN fails)
            self.bad.append((name, err, bound))

    def check(self):
        assert not self.bad, (self.label, self.bad)


def _act_code(F, act):
    return {"none": F.ACT_NONE, "relu": F.ACT_RELU, "lrelu": F.ACT_LRELU}[act]


@pytest.mark.parametrize("cid", list(CASES))
def test_statistics_per_group_and_channel(cid, F, dev):
    """sscg_norm_stats: mean and rstd of every (group, channel) against fp64, each relative to ITSELF; BatchNorm cases: the running
    mean / variance after the G updates with momentum 0.1 and the unbiased-variance factor L / (L - 1)."""
    inp = _inputs(cid)
    G, L, C = inp["G"], inp["L"], inp["C"]
    fig = _Figures("%s stats" % cid)
    rm = rv = None
    if inp["affine"]:
        ch = torch.arange(C, dtype=torch.float32)
        rm0, rv0 = 0.1 * (ch % 9) - 0.45, 0.5 + 0.125 * (ch % 6)
        rm, rv = rm0.to(dev), rv0.to(dev)
    mean, rstd = F.norm_stats(_dev(inp, inp["x"], dev), inp["per"], EPS, rm, rv, MOMENTUM)
    fig.add("mean", _per_element(mean, inp["mean"]), TOL_STAT)
    fig.add("rstd", _per_element(rstd, inp["rstd"]), TOL_STAT)
    if rm is not None:
        rmr, rvr = rm0.double(), rv0.double()
        for g in range(G):
            rmr = (1 - MOMENTUM) * rmr + MOMENTUM * inp["mean"][g]
            rvr = (1 - MOMENTUM) * rvr + MOMENTUM * inp["var"][g] * L / (L - 1)
        fig.add("running_mean", _per_element(rm, rmr), TOL_STAT)
        fig.add("running_var", _per_element(rv, rvr), TOL_STAT)
    fig.check()


# ReLU everywhere; LeakyReLU and no activation on one case per kernel family (fp32 slab, fp32 BatchNorm, bf16 slab, bf16 flat)
_UNIT_CASES = [(c, "relu") for c in CASES] + [(c, a) for c in ("A", "B", "E", "J") for a in ("lrelu", "none")]


@pytest.mark.parametrize("cid,act", _UNIT_CASES)
def test_norm_act_unit_forward_backward(cid, act, F, dev):
    """instance_norm_act / batch_norm_act (trainable gamma, beta; `groups` stacked batches) with a residual: y, dx, dres in the
    max-norm measure of test_norm_act; dgamma / dbeta per channel, relative to the sum of the |terms| of that channel's sum (a sum of
    terms of either sign can be arbitrarily small: it is no scale)."""
    inp = _inputs(cid)
    ref = _reference(inp, act)
    tol = TOL[inp["dtype"]]
    fig = _Figures("%s unit %s" % (cid, act))
    xg = _dev(inp, inp["x"], dev).requires_grad_(True)
    rg = _dev(inp, inp["res"], dev).requires_grad_(True)
    code = _act_code(F, act)
    if inp["affine"]:
        C = inp["C"]
        gg, bg = inp["gamma"].to(dev).requires_grad_(True), inp["beta"].to(dev).requires_grad_(True)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        y = F.batch_norm_act(xg, gg, bg, rm, rv, True, MOMENTUM, EPS, code, SLOPE, residual=rg,
                             groups=1 if inp["per"] is False else inp["per"])
    else:
        y = F.instance_norm_act(xg, code, SLOPE, residual=rg, eps=EPS)
    assert y.dtype == inp["dtype"]
    fig.add("y", _maxnorm(_glc(y, inp), ref["y"], dev), tol["y"])
    y.backward(_dev(inp, inp["dy"], dev))
    assert xg.grad.dtype == inp["dtype"]
    fig.add("dx", _maxnorm(_glc(xg.grad, inp), ref["dx"], dev), tol["dx"])
    fig.add("dres", _maxnorm(_glc(rg.grad, inp), ref["dres"], dev), tol["dres"])
    if inp["affine"]:
        fig.add("dgamma", _per_element(gg.grad, ref["dgamma"], ref["dgamma_scale"]), TOL_STAT)
        fig.add("dbeta", _per_element(bg.grad, ref["dbeta"], ref["dbeta_scale"]), TOL_STAT)
    fig.check()


@pytest.mark.parametrize("act", ["relu", "lrelu"])
@pytest.mark.parametrize("cid", ["C", "E", "K"])
def test_mask_recomputed_from_x_in_the_multi_round_regime(cid, act, F, dev):
    """sscg_norm_bwd with y == NULL where the backward slab kernels run several rounds per block (and the reduce many chunks): dx,
    dgamma, dbeta bitwise those of the call that reads y (test_norm_bwd_mask_recomputed_from_x_equals_mask_from_y, one round)."""
    inp = _inputs(cid)
    C, per = inp["C"], inp["per"]
    code = _act_code(F, act)
    x, dy = _dev(inp, inp["x"], dev), _dev(inp, inp["dy"], dev)
    gamma, beta = inp["gamma"].to(dev), inp["beta"].to(dev)
    mean, rstd = F.norm_stats(x, per, EPS)
    y = F.norm_apply(x, mean, rstd, gamma, beta, None, per, code, SLOPE)
    outs = []
    for yy in (y, None):
        dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        dx, _ = F.norm_bwd(dy, x, yy, mean, rstd, gamma, per, code, SLOPE, True, False, dg, db, beta=beta)
        outs.append((dx, dg, db))
    assert float(outs[0][0].float().abs().max()) > 0 and float(outs[0][1].abs().max()) > 0
    for a, b, name in zip(outs[0], outs[1], ("dx", "dgamma", "dbeta")):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("act", ["relu", "lrelu"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [64, 24, 21])
def test_mask_recomputed_from_x_in_the_slab_flat_and_scalar_kernels(C, dtype, act, F, dev):
    """[G][L][C] = (2, 1031, C): 64 channels run the slab kernels, 24 the flat kernels on vectors (six fp32 / three bf16 column groups:
    no power of two), 21 the flat kernels element by element.  The backward's recomputed pre-activation and the forward's are one
    function (csrc/norm_expr.h): dx, dgamma, dbeta with y == NULL are bitwise those of the call that reads y."""
    G, L = 2, 1031
    # the regime, from a mirror of vec_for / plan_slab (csrc/norm.hip): vectors of 8 (bf16, C % 8 == 0), 4 (C % 4 == 0) or 1; the slab
    # kernels where the vectors per row are a power of two and SSCG_NORM_SLAB does not switch them off
    vec = 8 if (dtype == BF and C % 8 == 0) else (4 if C % 4 == 0 else 1)
    groups = C // vec
    slab = vec >= 4 and groups & (groups - 1) == 0 and os.environ.get("SSCG_NORM_SLAB", "1").strip() != "0"
    assert (vec, slab) == {(64, F32): (4, True), (64, BF): (8, True), (24, F32): (4, False), (24, BF): (8, False), (21, F32): (1, False),
                           (21, BF): (1, False)}[(C, dtype)]
    code = _act_code(F, act)
    x = _table(G, L, C, dtype, 700 + C).to(dev).to(dtype).view(G, L, 1, C).permute(0, 3, 1, 2)
    dy = _rnd(torch.randn(G, L, C, generator=torch.Generator().manual_seed(800 + C)), dtype).to(dev).to(dtype).view(G, L, 1, C).permute(0, 3, 1, 2)
    gamma, beta = (t.to(dev) for t in _affine(C))
    mean, rstd = F.norm_stats(x, True, EPS)
    y = F.norm_apply(x, mean, rstd, gamma, beta, None, True, code, SLOPE)
    outs = []
    for yy in (y, None):
        dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        dx, _ = F.norm_bwd(dy, x, yy, mean, rstd, gamma, True, code, SLOPE, True, False, dg, db, beta=beta)
        outs.append((dx, dg, db))
    assert outs[0][0].dtype == dtype and float(outs[0][0].float().abs().max()) > 0 and float(outs[0][1].abs().max()) > 0
    masked = float((y.float() <= 0).float().mean())
    assert 0.05 < masked < 0.95, masked
    for a, b, name in zip(outs[0], outs[1], ("dx", "dgamma", "dbeta")):
        assert torch.equal(a, b), (name, int((a != b).sum()))


def _row_ranges(L, rows_per_chunk, round_rows):
    """(start, count), at most 64 rows each: the first rows, rows on both sides of the first chunk boundary, rows of the second
    chunk's later rounds, the last rows."""
    return [(0, min(64, L)), (max(0, rows_per_chunk - 32), 64), (rows_per_chunk + round_rows, min(64, rows_per_chunk - round_rows)),
            (L - 64, 64)]


def _slice_nchw(t_glc, g, a, n):
    """rows [a, a + n) of group g as a small contiguous (1, C, n, 1) channels-last tensor of its own."""
    return t_glc[g, a:a + n].clone().view(1, n, 1, -1).permute(0, 3, 1, 2)


@pytest.mark.parametrize("cid", list(SLAB_ROWS))
def test_rows_of_the_large_call_equal_small_calls_bitwise(cid, F, dev):
    """With mean and rstd given, sscg_norm_apply and the frozen-statistics sscg_norm_bwd are independent per row, by one per-element
    expression: rows cut out of the large tensor and run as tensors of their own (one round per block: the regime the small tests
    pin) give bitwise the rows of the large call.  A failure names the rows."""
    inp = _inputs(cid)
    G, L, per = inp["G"], inp["L"], inp["per"]
    x, dy, res = (_dev(inp, inp[k], dev) for k in ("x", "dy", "res"))
    gamma, beta = inp["gamma"].to(dev), inp["beta"].to(dev)
    mean, rstd = F.norm_stats(x, per, EPS)
    y = F.norm_apply(x, mean, rstd, gamma, beta, res, per, F.ACT_RELU, 0.0)
    dx, dres = F.norm_bwd(dy, x, y, mean, rstd, gamma, per, F.ACT_RELU, 0.0, stats_grad=False, want_dres=True)
    big = {k: _glc(t, inp) for k, t in (("x", x), ("dy", dy), ("res", res), ("y", y), ("dx", dx), ("dres", dres))}
    g = G - 1
    mg, rg = mean[g:g + 1].contiguous(), rstd[g:g + 1].contiguous()
    bad = []
    for kind, (rpc, rnd) in zip(("apply", "bwd"), SLAB_ROWS[cid]):
        for a, n in _row_ranges(L, rpc, rnd):
            xs, ds, rs, ys = (_slice_nchw(big[k], g, a, n) for k in ("x", "dy", "res", "y"))
            if kind == "apply":
                got = {"y": F.norm_apply(xs, mg, rg, gamma, beta, rs, False, F.ACT_RELU, 0.0)}
            else:
                sdx, sdres = F.norm_bwd(ds, xs, ys, mg, rg, gamma, False, F.ACT_RELU, 0.0, stats_grad=False, want_dres=True)
                got = {"dx": sdx, "dres": sdres}
            for k, t in got.items():
                want = big[k][g, a:a + n]
                t = t.permute(0, 2, 3, 1).reshape(n, -1)
                if not torch.equal(t, want):
                    rows = (t != want).any(1).nonzero().flatten() + a
                    bad.append((k, "group %d rows %d..%d" % (g, a, a + n - 1), "first differing rows", rows[:8].tolist()))
    assert float(big["y"].float().abs().max()) > 0 and float(big["dx"].float().abs().max()) > 0
    assert not bad, bad


@pytest.mark.parametrize("cols,dtype", [(1, F32), (3, F32), (21, F32), (64, F32), (64, BF)], ids=lambda v: str(v).replace("torch.", ""))
def test_colsum_at_step_row_counts(cols, dtype, F, dev):
    """sscg_colsum (the bias gradients) on 300000 rows: 128 chunks of 2344 rows, the last 2312 (two lane rounds in finalize_sum_kernel;
    VEC = 1 / 4 / 8 column groups), written and then accumulated into a prefilled vector.  Per column against the fp64 sum,
    relative to the column's sum of |x|.  Bound: the fp64 accumulation is exact at this scale, the sum is rounded to fp32 once
    (2^-24) and added to the prefill in fp32 once more (2^-24 of the result): 2^-22 leaves a factor two."""
    rows = 300000
    x = _table(1, rows, cols, dtype, 7 + cols, col_shift=0.03125)[0]       # distinct column means
    xd = x.double()
    ref, scale = xd.sum(0), xd.abs().sum(0)
    assert cols == 1 or float((ref / rows).sort().values.diff().min()) > 0.02
    xg = x.to(dev).to(dtype)
    fig = _Figures("colsum cols=%d %s" % (cols, str(dtype).replace("torch.", "")))
    out = F.colsum(rows, cols, xg)
    fig.add("written", _per_element(out, ref, scale), 2.0 ** -22)
    pre = (1000.0 * (torch.arange(cols, dtype=torch.float32) + 1))
    out = pre.to(dev)
    F.colsum(rows, cols, xg, out=out, accumulate=True)
    fig.add("accumulated", _per_element(out, ref + pre.double(), scale + pre.double()), 2.0 ** -22)
    fig.check()


def _torch_pixel_discriminator(net, norm):
    """The reference's PixelDiscriminator as stock torch modules in fp64 holding `net`'s weights (as in test_kernels_gpu.py)."""
    from torch import nn
    convs = [m for m in net.dis_model if hasattr(m, "kernel_size")]
    c1, c2, c3 = convs
    nl = nn.BatchNorm2d(c2.out_channels) if norm == "batch" else nn.InstanceNorm2d(c2.out_channels)
    ref = nn.Sequential(nn.Conv2d(c1.in_channels, c1.out_channels, 1), nn.LeakyReLU(0.2), nn.Conv2d(c2.in_channels, c2.out_channels, 1, bias=c2.bias is not None),
                        nl, nn.LeakyReLU(0.2), nn.Conv2d(c3.in_channels, 1, 1, bias=c3.bias is not None))
    with torch.no_grad():
        for r, m in zip((ref[0], ref[2], ref[5]), convs):
            r.weight.copy_(m.weight.detach().cpu())
            if m.bias is not None:
                r.bias.copy_(m.bias.detach().cpu())
        if norm == "batch":
            ours = [m for m in net.dis_model if getattr(m, "running_mean", None) is not None][0]
            nl.weight.copy_(ours.weight.detach().cpu())
            nl.bias.copy_(ours.bias.detach().cpu())
    return ref.double()


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("norm", ["instance", "batch"])
@pytest.mark.parametrize("geom", [(2, 3, 16, 192, 192), (2, 3, 128, 90, 100)], ids=lambda g: "n%d_cin%d_c%d_%dx%d" % g)
def test_fused_pixel_discriminator_tail_with_many_chunks(geom, norm, F, dev):
    """test_fused_pixel_discriminator_tail's comparisons where the tail's backward reduce (RM_BWD_HEAD: two rounds through the LDS)
    has 72 chunks of 512 rows (C = 16) and 2 slabs x 71 chunks (C = 128) per image under InstanceNorm, 128 under BatchNorm - the
    existing geometries give at most 3 - so that finalize_bwd_kernel's and finalize_head_kernel's lanes take a second chunk."""
    ops = load_sub("arch.ops")
    disc = load_sub("arch.discriminators")
    N, Cin, C, H, W = geom
    torch.manual_seed(sum(geom))
    net = disc.PixelDiscriminator(Cin, C // 2, norm_layer=ops.get_norm_layer(norm), use_bias=(norm == "instance")).to(dev)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape) * (0.5 if p.dim() == 1 else 1.0 / p.shape[1] ** 0.5))
    ref = _torch_pixel_discriminator(net, norm)
    x0 = torch.randn(N, Cin, H, W)
    g0 = torch.randn(N, 1, H, W)
    xr = x0.double().requires_grad_(True)
    yr = ref(xr)
    (yr * g0.double()).sum().backward()
    want = [yr, xr.grad] + [p.grad for p in ref.parameters() if p.grad is not None]
    # The one departure from the small test: dx is compared on the pixels whose every channel has its fp64 pre-activation (the norm
    # layer's output, magnitude ~1, fp32 error ~1e-6) at least 1e-5 away from the LeakyReLU's kink.  A pixel on the kink gets a dx
    # off by tens of percent from a correct kernel; at 1.2 M / 2.3 M pre-activations some ~20 pixels of 36864 / 18000 x 2 are that close (the small
    # geometries have 2e5 values at most and have not met one).  Sums over pixels (the weight gradients) move by < 1e-5 of a term.
    with torch.no_grad():
        keep = ~(ref[:4](x0.double()).abs() < 1e-5).any(1, keepdim=True)
    print("norm_regimes tail %s c=%d pixels left out of dx: %d of %d" % (norm, geom[2], int((~keep).sum()), keep.numel()))
    assert float(keep.double().mean()) > 0.99
    got = {}
    for fused in (True, False):
        ops.FUSE_HEAD[0] = fused
        try:
            for p in net.parameters():
                p.grad = None
            x = x0.to(dev).contiguous(memory_format=CL).requires_grad_(True)
            y = net(x)
            F.backward((y * g0.to(dev).contiguous(memory_format=CL)).sum())
            F.SideStream.join(dev)
            torch.cuda.synchronize()
            convs = [m for m in net.dis_model if hasattr(m, "kernel_size")]
            norms = [m for m in net.dis_model if isinstance(m, ops.BatchNorm2d)]
            grads = []
            for m in convs:
                grads.append(m.weight.grad)
                if m.bias is not None:
                    grads.append(m.bias.grad)
            got[fused] = [y.detach(), x.grad] + grads + ([norms[0].weight.grad, norms[0].bias.grad] if norms else [])
        finally:
            ops.FUSE_HEAD[0] = True
    # the reference's parameter order: conv1 (w, b), conv2 (w[, b]), norm (w, b) for batch, conv3 (w[, b])
    inst, bat = norm == "instance", norm == "batch"
    names = ["y", "dx", "w1", "b1", "w2"] + ["b2"] * inst + ["gamma", "beta"] * bat + ["w3"] + ["b3"] * inst
    refs = dict(zip(names, want))
    ours_names = ["y", "dx", "w1", "b1", "w2"] + ["b2"] * inst + ["w3"] + ["b3"] * inst + ["gamma", "beta"] * bat
    fig = _Figures("tail %s c=%d" % (norm, C))
    for fused in (True, False):
        vals = dict(zip(ours_names, got[fused]))
        for k in names:
            if k == "b2":
                continue        # a bias in front of InstanceNorm has zero gradient: nothing to compare against but roundoff
            m = keep if k == "dx" else 1.0
            fig.add("%s %s" % ("fused" if fused else "unfused", k), _rel(vals[k].reshape(refs[k].shape).cpu() * m, refs[k] * m), 3e-5)
    a, b = dict(zip(ours_names, got[True])), dict(zip(ours_names, got[False]))
    for k in ("y", "dx", "w2", "w3"):
        m = keep if k == "dx" else 1.0
        fig.add("fused vs unfused %s" % k, _rel(a[k].cpu() * m, b[k].cpu() * m), 1e-5)
    fig.check()
