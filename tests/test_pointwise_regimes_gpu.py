"""csrc/pointwise.hip and the class-axis / loss half of csrc/loss_optim.hip in the regimes the training step runs them in and at their
geometry edges.  The other kernel-level tests stop far below the grid caps (6,144 elements for the scalar losses, 2,048 rows for the
class axis, 274,560 elements for the bf16 pointwise kernels); the step runs L1 / MSE over 1.57 M elements, cross entropy over 524,288
rows and activations and adds over tens of millions of elements.

The constants every regime below is derived from (a change of one has to revisit the cases: they are the smallest shapes that reach
each regime, not shapes that reach it whatever the constant):
  CAP  = 8192 blocks x 256 threads = 2,097,152: the grid of every grid-stride kernel (`ew_blocks`); element CAP + k is handled in a
         SECOND round by the thread that handled element k.  N2 = CAP + 257: a second round that 257 threads (one block and one thread
         of the next) take and the other 8190 blocks do not.
  LCAP = 1024 blocks (`LOSS_BLOCKS`) x 256 = 262,144: the grid of the loss forwards, one fp64 partial per block, summed by one block.
  HCAP = 1024 blocks x 256 threads x 16 labels = 4,194,304: the block count of `sscg_confusion_hist` stops growing there.
  sscg_add: 16-byte vectors (V = 4 fp32 / 8 bf16 elements) when n % V == 0 and all three pointers are 16-byte aligned, else the scalar
         kernel; the vector kernel's grid is ew_blocks(ceil(nv / 2)), its loop `for (; i + stride < nv; i += 2 * stride)` keeps two
         vectors in flight and a tail `if (i < nv)` takes the odd one.

Every element is distinguishable: inputs are a saw-tooth of the flat index (period 8191; 2^21 = 256 mod 8191, so elements one grid
stride apart differ by 256 / 8191 of the range) plus seeded noise, never noise alone.  Outputs start as NaN (0xEE.. for integers):
either the test allocates them itself, as a view into a larger sentinel-filled buffer whose head and tail must still hold the sentinel
afterwards (calls through F._lib.lib), or the wrappers' allocations are poisoned (`_nan_outputs`).

References are plain torch expressions on the CPU, in fp64 where there is arithmetic, evaluated on the values the device tensors hold
(bf16: rounded first).  A selection, a copy or a single correctly rounded fp32 operation is held to torch.equal.  Every numeric bound is
one the project already uses for the same kernel at a small shape (named beside it).  Each test prints its figures
(`pointwise_regimes ...`, shown by `pytest -s`) before it asserts; profiles/pointwise_regimes.txt holds the distance of a plain-fp32
CPU evaluation of the same references (`dt=torch.float32`) from the fp64 ones, the yardstick of the bounds."""
import contextlib
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from conftest import load_sub

pytestmark = pytest.mark.gpu
CL = torch.channels_last
F32 = torch.float32
BF = torch.bfloat16
F64 = torch.float64
EPS16 = 2.0 ** -8           # one bf16 rounding: relative error <= 2^-9 of the value, compared against the tensor's max (test_pointwise_bf16)
CAP = 8192 * 256
LCAP = 1024 * 256
HCAP = 1024 * 256 * 16
N2 = CAP + 257
EDGES = (1, 255, 256, 257)  # one thread; one block less a thread; one full block; a block and one thread of the second
SLOPE = 0.2
GUARD = 64                  # sentinel elements before and after a guarded view (256 / 128 bytes: the view stays 16-byte aligned)
SENT = {F32: float("nan"), BF: float("nan"), torch.int64: -7777, torch.uint8: 0xEE}
DTYPES = pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])

# fp32 tanhf: the HIP / OpenCL device library documents <= 5 ulp; |tanh| <= 1, so <= 5 * 2^-24 = 3e-7 of the maximum; the backward
# dy * (1 - y * y) is three fp32 roundings (<= 2e-7 of the maximum).  1e-6 is the project's bound for its fp32 pointwise results
# (test_mse_l1_weighted, test_maxpool); bf16 results: one rounding (test_pointwise_bf16).
TOL_POINT = {F32: 1e-6, BF: EPS16}


# ----------------------------------------------------------------------------------------------------------------- helpers
def _saw(n, lo, hi, period=8191):
    i = torch.arange(n, dtype=F64)
    return lo + (hi - lo) * (i % period) / period


def _table(shape, seed, dtype=F32, lo=-2.0, hi=2.0, noise=0.25, period=8191):
    """CPU fp32 tensor of `shape` holding values of `dtype`: saw-tooth of the flat index in [lo, hi) + noise * N(0, 1) (seeded)."""
    n = math.prod(shape)
    g = torch.Generator().manual_seed(seed)
    x = _saw(n, lo, hi, period).float() + noise * torch.randn(n, generator=g)
    return x.to(dtype).float().view(shape)


def _dev4(t, dev, dtype=F32):
    """NCHW CPU tensor -> channels-last device tensor of dtype (the values are representable: no rounding happens here)."""
    return t.to(dev).to(dtype).contiguous(memory_format=CL)


def _rows_dev(t2d, shape, dev):
    """[rows, C] CPU table -> the logical (N, C, H, W) channels-last device tensor whose memory it is."""
    n, c, h, w = shape
    return t2d.to(dev).view(n, h, w, c).permute(0, 3, 1, 2)


def _rows_cpu(t4):
    n, c, h, w = t4.shape
    return t4.detach().permute(0, 2, 3, 1).reshape(n * h * w, c).cpu()


def _guarded(n, dtype, dev, shift=0):
    """(buffer, view of n elements GUARD (+ shift) elements into it): the whole buffer holds the sentinel."""
    buf = torch.full((n + 2 * GUARD + shift,), SENT[dtype], dtype=dtype, device=dev)
    return buf, buf[GUARD + shift:GUARD + shift + n]


def _guards_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    g = torch.cat((buf[:lo], buf[lo + view.numel():]))
    return bool(torch.isnan(g).all()) if buf.is_floating_point() else bool((g == SENT[buf.dtype]).all())


@contextlib.contextmanager
def _nan_outputs():
    """The allocation hook: every device tensor that torch.empty / torch.empty_like hand out while this is active (the wrappers of
    functional.py allocate their outputs, index maps, loss scalars and workspaces through them) starts as the sentinel of its dtype,
    so an element no kernel writes is a NaN in the comparison, whatever the caching allocator left in that memory."""
    real_empty, real_like = torch.empty, torch.empty_like

    def poison(t):
        if t.is_cuda and t.numel():
            t.fill_(SENT.get(t.dtype, 0))
        return t

    torch.empty = lambda *a, **k: poison(real_empty(*a, **k))
    torch.empty_like = lambda *a, **k: poison(real_like(*a, **k))
    try:
        yield
    finally:
        torch.empty, torch.empty_like = real_empty, real_like


def _maxnorm(got, ref):
    """max |got - ref| / max |ref| (the measure of test_kernels_gpu.rel_err)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got.reshape(ref.shape) - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _maxabs(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got.reshape(ref.shape) - ref).abs().max())


class _Figures:
    """Prints every figure when it is taken; asserts them all at the end, so that one run shows the whole case."""

    def __init__(self, label):
        self.label, self.bad = label, []

    def add(self, name, err, bound):
        print("pointwise_regimes %s %s err %.3e bound %.3e" % (self.label, name, err, bound))
        if not err < bound:         # (a NaN fails)
            self.bad.append((name, err, bound))

    def exact(self, name, got, ref):
        """torch.equal; the figure is the number of elements that differ (an unwritten element is a NaN: it differs)."""
        got, ref = got.detach().cpu(), ref.detach().cpu()
        got = got.reshape(ref.shape)
        ok = got.dtype == ref.dtype and torch.equal(got, ref)
        bad = 0 if ok else max(int((got != ref).sum()), 1)
        print("pointwise_regimes %s %s differing %d of %d" % (self.label, name, bad, ref.numel()))
        if not ok:
            self.bad.append((name, bad, 0))

    def true(self, name, ok, detail=""):
        print("pointwise_regimes %s %s %s %s" % (self.label, name, "ok" if ok else "FAILED", detail))
        if not ok:
            self.bad.append((name, detail))

    def check(self):
        assert not self.bad, (self.label, self.bad)


def _dt_code(F, dtype):
    return {F32: F.F32, BF: F.BF16}[dtype]


def _name(dtype):
    return {F32: "f32", BF: "bf16"}[dtype]


# ----------------------------------------------------------------------------------------------------------------- references
# dt = torch.float64: the reference.  dt = torch.float32: the same expressions in plain fp32, the yardstick of a bound.
def ref_act_fwd(x, act, dt=F64):
    x = x.to(dt)
    if act == 1:
        return torch.where(x > 0, x, torch.zeros_like(x))
    if act == 2:
        return torch.where(x > 0, x, x * torch.tensor(SLOPE, dtype=F32).to(dt))      # the kernel's slope is the fp32 0.2
    if act == 3:
        return torch.tanh(x)
    return x


def ref_act_bwd(dy, y, act, dt=F64):
    dy, y = dy.to(dt), y.to(dt)
    if act == 1:
        return torch.where(y > 0, dy, torch.zeros_like(dy))
    if act == 2:
        return torch.where(y > 0, dy, dy * torch.tensor(SLOPE, dtype=F32).to(dt))
    if act == 3:
        return dy * (1 - y * y)
    return dy


def ref_reflect_bwd(xshape, gy, pad, dt=F64):
    if pad == 0:
        return gy.to(dt)
    xr = torch.zeros(xshape, dtype=dt, requires_grad=True)
    TF.pad(xr, (pad, pad, pad, pad), mode="reflect").backward(gy.to(dt))
    return xr.grad


def ref_pool(x, gy, k, dt=F64):
    """k = 3: MaxPool2d(3, 2, 1, ceil_mode=True); k = 2: MaxPool2d(2, 2).  gy: a function of the output shape."""
    xr = x.detach().to(dt, copy=True).requires_grad_(True)
    y = TF.max_pool2d(xr, 3, 2, 1, ceil_mode=True) if k == 3 else TF.max_pool2d(xr, 2, 2)
    g = gy(tuple(y.shape))
    y.backward(g.to(dt))
    return y.detach(), xr.grad, g


def ref_upsample(x, gy, size, dt=F64):
    xr = x.detach().to(dt, copy=True).requires_grad_(True)
    y = TF.interpolate(xr, size=size, mode="bilinear", align_corners=True)
    y.backward(gy.to(dt))
    return y.detach(), xr.grad


def ref_softmax(x2d, gy2d, dt=F64):
    xr = x2d.detach().to(dt, copy=True).requires_grad_(True)
    s = torch.softmax(xr, 1)
    s.backward(gy2d.to(dt))
    return s.detach(), xr.grad


def ref_ce(x2d, lab, scale, dt=F64):
    """nn.CrossEntropyLoss with every label outside [0, C) ignored; the gradient of scale * loss."""
    C = x2d.shape[1]
    rl = lab.clone()
    rl[(lab < 0) | (lab >= C)] = -100
    xr = x2d.detach().to(dt, copy=True).requires_grad_(True)
    loss = TF.cross_entropy(xr, rl, ignore_index=-100)
    (loss * scale).backward()
    return loss.detach(), xr.grad


LOSS_W = (1.0, 0.5, 2.0, 0.75)      # weighted_sum weights of (l1, mse_const vs 1, mse_const vs 0, mse)
LOSS_G = 1.7                        # the upstream gradient of the weighted sum


def ref_losses(t, dt=F64):
    a1, d, a2, b2 = (t[k].detach().to(dt, copy=True).requires_grad_(True) for k in ("a1", "d", "a2", "b2"))
    b1 = t["b1"].to(dt)
    l1 = (a1 - b1).abs().mean()
    m1 = ((d - 1.0) ** 2).mean()
    m0 = (d ** 2).mean()
    ms = ((a2 - b2) ** 2).mean()
    tot = LOSS_W[0] * l1 + LOSS_W[1] * m1 + LOSS_W[2] * m0 + LOSS_W[3] * ms
    tot.backward(torch.tensor(LOSS_G, dtype=dt))
    return dict(l1=l1.detach(), m1=m1.detach(), m0=m0.detach(), mse=ms.detach(), tot=tot.detach(), da1=a1.grad, dd=d.grad, da2=a2.grad,
                db2=b2.grad)


# ----------------------------------------------------------------------------------------------------------------- input builders
def act_inputs(n, dtype):
    """x (exact zeros at every 7th element from the 4th, negatives, positives), the activation output y the backward is given
    (|y| <= 0.96875 so that it is a value tanh can produce; the zeros stay zeros) and dy."""
    x = _table((n,), 11, dtype)
    x[3::7] = 0.0
    y = (x * 0.45).clamp(-0.96875, 0.96875).to(dtype).float()
    dy = _table((n,), 12, dtype, -1.0, 1.0, 0.5)
    return x, y, dy


def class_inputs(shape, seed):
    """[rows, C] logits (fp32 values), labels, softmax upstream gradient.  Rows r % 29 == 0: magnitudes of +-80, every second of them
    +-90 (e^90 = 1.2e39 is beyond fp32: a softmax without the max subtraction overflows there, and at +-80 it has lost the small
    classes); rows r % 31 == 1: all classes equal; argmax ties: class 5 copies class 3 on every third row (C >= 6), class 1 copies class 0 on rows r % 5 == 2
    (C >= 2).  Labels: ~5 % 255, ~1 % negative (-1 / -100)."""
    n, C, h, w = shape
    rows = n * h * w
    g = torch.Generator().manual_seed(seed)
    x = 3.0 * torch.randn(rows, C, generator=g) + _saw(rows * C, -1.0, 1.0).float().view(rows, C)
    r = torch.arange(rows)
    big = r % 29 == 0
    sign = torch.where(torch.rand(int(big.sum()), C, generator=g) < 0.5, -1.0, 1.0)
    x[big] = sign * torch.where((r[big] % 58 == 0)[:, None], 90.0, 80.0) + torch.randn(int(big.sum()), C, generator=g)
    flat = r % 31 == 1
    x[flat] = x[flat][:, :1].expand(-1, C).clone()
    if C >= 6:
        x[::3, 5] = x[::3, 3]
    if C >= 2:
        x[2::5, 1] = x[2::5, 0]
    lab = torch.randint(0, C, (rows,), generator=g)
    u = torch.rand(rows, generator=g)
    lab[u < 0.05] = 255
    lab[(u >= 0.05) & (u < 0.055)] = -1
    lab[(u >= 0.055) & (u < 0.06)] = -100
    gy = torch.randn(rows, C, generator=g)
    return x, lab, gy


def loss_inputs(n):
    """Means far from zero (a, b ~ 100): a sum of squares or of differences formed carelessly in fp32 loses digits there.  L1: every
    10th pair is an exact tie."""
    a1 = _table((n,), 31, lo=99.0, hi=101.0)
    b1 = _table((n,), 32, lo=99.0, hi=101.0)
    b1[3::10] = a1[3::10]
    d = _table((n,), 33, lo=99.0, hi=101.0)
    a2 = _table((n,), 34, lo=99.0, hi=101.0)
    b2 = _table((n,), 35, lo=99.0, hi=101.0)
    return dict(a1=a1, b1=b1, d=d, a2=a2, b2=b2)


def add_size(case, V):
    """sscg_add cases of a dtype with V elements per 16-byte vector -> (n, which operand is misaligned or None)."""
    return {
        # nv = 1537 vectors: grid ew_blocks(769) = 4 blocks, stride 1024: threads 0..512 run the loop once (i, i + 1024) and no tail;
        # threads 513..1023 fail the loop condition at once and run the tail branch only
        "a": (V * (2 * 256 * 3 + 1), None),
        # nv = 3 CAP + 5 vectors: the grid is capped (stride = CAP vectors): every thread runs the loop once (i, i + CAP) and then the
        # tail at i + 2 CAP, except threads 0..4, which run the loop twice (i + 2 CAP, i + 3 CAP).  25.2 M fp32 / 50.3 M bf16 elements
        "b": (V * (3 * CAP + 5), None),
        # n % V == 3: the scalar kernel
        "c": (V * (2 * 256 * 3 + 1) + 3, None),
        # n % V == 0, but one operand starts one element (4 / 2 bytes) into its buffer: the scalar kernel
        "d_a": (V * (2 * 256 * 3 + 1), "a"), "d_b": (V * (2 * 256 * 3 + 1), "b"), "d_y": (V * (2 * 256 * 3 + 1), "y"),
        # CAP + 257 is odd: the scalar kernel, whose second round 257 threads take
        "e": (N2, None),
    }[case]


# ----------------------------------------------------------------------------------------------------------------- 1. grid-stride rounds
@DTYPES
@pytest.mark.parametrize("n", EDGES + (N2,))
def test_activation_forward_and_backward(n, dtype, F, dev):
    """sscg_act_fwd / sscg_act_bwd, every activation code: the block edges and N2 (second round of 257 threads).  none / relu (and
    lrelu in fp32: one correctly rounded product) are torch.equal; tanh and the bf16 lrelu take TOL_POINT."""
    lib, dt = F._lib.lib, _dt_code(F, dtype)
    fig = _Figures("act %s n=%d" % (_name(dtype), n))
    x, yv, dy = act_inputs(n, dtype)
    xg, yg, dyg = (t.to(dev).to(dtype) for t in (x, yv, dy))
    for act, an in ((F.ACT_NONE, "none"), (F.ACT_RELU, "relu"), (F.ACT_LRELU, "lrelu"), (F.ACT_TANH, "tanh")):
        exact = an in ("none", "relu") or (an == "lrelu" and dtype == F32)
        buf, out = _guarded(n, dtype, dev)
        F.check(lib.sscg_act_fwd(xg.data_ptr(), out.data_ptr(), dt, n, act, SLOPE, F._stream()), "sscg_act_fwd")
        if exact:
            fig.exact("fwd_" + an, out.float(), ref_act_fwd(x, act, F32))
        else:
            fig.add("fwd_" + an, _maxnorm(out, ref_act_fwd(x, act)), TOL_POINT[dtype])
        fig.true("fwd_%s_guards" % an, _guards_intact(buf, out))
        buf, out = _guarded(n, dtype, dev)
        F.check(lib.sscg_act_bwd(dyg.data_ptr(), yg.data_ptr(), out.data_ptr(), dt, n, act, SLOPE, F._stream()), "sscg_act_bwd")
        if exact:
            fig.exact("bwd_" + an, out.float(), ref_act_bwd(dy, yv, act, F32))
        else:
            fig.add("bwd_" + an, _maxnorm(out, ref_act_bwd(dy, yv, act)), TOL_POINT[dtype])
        fig.true("bwd_%s_guards" % an, _guards_intact(buf, out))
    fig.check()


@pytest.mark.parametrize("n", EDGES + (N2,))
def test_cast_all_dtype_pairs(n, F, dev):
    """sscg_cast fp32 <-> bf16 and the two copies: torch.equal with torch's round-to-nearest-even.  Every 9th fp32 source value is an
    exact tie between two bf16 neighbours (1 + an odd multiple of 2^-8, times a power of two)."""
    lib = F._lib.lib
    fig = _Figures("cast n=%d" % n)
    x = _table((n,), 13)
    k = torch.arange(n)[2::9]
    x[2::9] = ((1.0 + (2 * (k % 64) + 1) * 2.0 ** -8) * 2.0 ** (k % 5).double()).float() * torch.where(k % 2 == 0, 1.0, -1.0)
    for sd in (F32, BF):
        src = x.to(sd)
        sg = src.to(dev)
        for dd in (F32, BF):
            buf, out = _guarded(n, dd, dev)
            F.check(lib.sscg_cast(sg.data_ptr(), _dt_code(F, sd), out.data_ptr(), _dt_code(F, dd), n, F._stream()), "sscg_cast")
            fig.exact("%s_to_%s" % (_name(sd), _name(dd)), out, src.to(dd))
            fig.true("%s_to_%s_guards" % (_name(sd), _name(dd)), _guards_intact(buf, out))
    fig.check()


def test_fill(F, dev):
    """sscg_fill at the block edges and N2; F.fill_ of a bf16 tensor (zero only: pairs of elements written as fp32 zeros)."""
    lib = F._lib.lib
    fig = _Figures("fill")
    for n in EDGES + (N2,):
        buf, out = _guarded(n, F32, dev)
        F.check(lib.sscg_fill(out.data_ptr(), n, 1.25, F._stream()), "sscg_fill")
        fig.exact("n=%d" % n, out, torch.full((n,), 1.25))
        fig.true("n=%d_guards" % n, _guards_intact(buf, out))
    buf, out = _guarded(2 * N2, BF, dev)        # 2 N2 bf16 = N2 fp32 words
    F.fill_(out, 0.0)
    fig.exact("bf16_zero n=%d" % (2 * N2), out, torch.zeros(2 * N2, dtype=BF))
    fig.true("bf16_zero_guards", _guards_intact(buf, out))
    fig.check()


@DTYPES
def test_dropout_mask_is_a_function_of_seed_and_index(dtype, F, dev):
    """sscg_dropout: kept elements are x / (1 - p) exactly (p = 0.5: a doubling), dropped ones 0; the call over n elements equals the
    first n elements of the call over N2 (n = 4096 and the block edges): the hash sees the element index, not the thread; the second
    round's 257 masks are not the first round's; keep rates within 5 sigma of the binomial (sigma = sqrt(p (1 - p) / n): a correct
    kernel misses with probability 6e-7, and the seed is fixed)."""
    lib, dt = F._lib.lib, _dt_code(F, dtype)
    fig = _Figures("dropout %s" % _name(dtype))
    x = _table((N2,), 14, dtype, 1.0, 2.0, 0.0)          # [1, 2): never zero, so a zero output is a dropped element
    xg = x.to(dev).to(dtype)

    def run(n, p, seed=1234):
        buf, out = _guarded(n, dtype, dev)
        F.check(lib.sscg_dropout(xg.data_ptr(), out.data_ptr(), dt, n, p, seed, F._stream()), "sscg_dropout")
        fig.true("n=%d p=%.2f guards" % (n, p), _guards_intact(buf, out))
        return out.float().cpu()

    full = run(N2, 0.5)
    keep = full != 0
    fig.exact("n=%d kept_values" % N2, full, torch.where(keep, x * 2.0, torch.zeros_like(x)))
    for n in EDGES + (4096,):
        fig.exact("n=%d equals_prefix_of_n=%d" % (n, N2), run(n, 0.5), full[:n])
    fig.true("second_round_mask_differs", not torch.equal(keep[CAP:CAP + 257], keep[:257]),
             "%d of 257 masks differ" % int((keep[CAP:CAP + 257] != keep[:257]).sum()))
    fig.true("other_seed_differs", not torch.equal(run(4096, 0.5, 1235) != 0, keep[:4096]))
    fig.add("keep_rate_all", abs(float(keep.double().mean()) - 0.5), 5 * math.sqrt(0.25 / N2))
    fig.add("keep_rate_second_round", abs(float(keep[CAP:].double().mean()) - 0.5), 5 * math.sqrt(0.25 / 257))
    if dtype == F32:
        q = run(N2, 0.25)
        kq = q != 0
        scale = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(0.25))        # the entry point's 1.f / (1.f - p)
        fig.exact("p=0.25 kept_values", q, torch.where(kq, x * scale, torch.zeros_like(x)))
        fig.add("p=0.25 keep_rate_all", abs(float(kq.double().mean()) - 0.75), 5 * math.sqrt(0.25 * 0.75 / N2))
        fig.add("p=0.25 keep_rate_second_round", abs(float(kq[CAP:].double().mean()) - 0.75), 5 * math.sqrt(0.25 * 0.75 / 257))
    fig.check()


def test_gauss_noise_is_a_function_of_seed_and_index(F, dev):
    """sscg_gauss_noise (y = x + sigma x z): a call over n elements equals the first n of the call over N2; the second round's z are
    not the first round's; z has zero mean and unit variance over all N2 elements (test_gauss_noise_statistics' bounds, 0.02) and over
    the 257 of the second round (5 sigma: 5 / sqrt(257) for the mean, 5 / sqrt(2 * 257) for the standard deviation)."""
    lib = F._lib.lib
    fig = _Figures("gauss_noise")
    sigma = 0.2
    x = _table((N2,), 15, F32, 1.0, 2.0, 0.0)
    xg = x.to(dev)

    def run(n, seed=77):
        buf, out = _guarded(n, F32, dev)
        F.check(lib.sscg_gauss_noise(xg.data_ptr(), out.data_ptr(), n, sigma, seed, F._stream()), "sscg_gauss_noise")
        fig.true("n=%d guards" % n, _guards_intact(buf, out))
        return out.cpu()

    full = run(N2)
    for n in EDGES + (4096,):
        fig.exact("n=%d equals_prefix_of_n=%d" % (n, N2), run(n), full[:n])
    z = (full.double() - x.double()) / (sigma * x.double())
    fig.true("all_finite", bool(torch.isfinite(z).all()))
    fig.true("second_round_differs", float((z[CAP:CAP + 257] - z[:257]).abs().max()) > 0.1,
             "max |z[CAP + k] - z[k]| = %.3f" % float((z[CAP:CAP + 257] - z[:257]).abs().max()))
    fig.true("other_seed_differs", not torch.equal(run(4096, 78), full[:4096]))
    fig.add("mean_all", abs(float(z.mean())), 0.02)
    fig.add("std_all", abs(float(z.std()) - 1.0), 0.02)
    fig.add("mean_second_round", abs(float(z[CAP:].mean())), 5 / math.sqrt(257))
    fig.add("std_second_round", abs(float(z[CAP:].std()) - 1.0), 5 / math.sqrt(2 * 257))
    fig.check()


# ----------------------------------------------------------------------------------------------------------------- 2. sscg_add
@DTYPES
@pytest.mark.parametrize("case", ["a", "b", "c", "d_a", "d_b", "d_y", "e"])
def test_add_dispatch_paths(case, dtype, F, dev):
    """The four kernels of sscg_add (see add_size for the path each case takes).  fp32: the CPU's a + b bit for bit; bf16: the fp32 sum
    rounded once."""
    lib, dt = F._lib.lib, _dt_code(F, dtype)
    n, mis = add_size(case, 4 if dtype == F32 else 8)
    fig = _Figures("add %s %s n=%d" % (_name(dtype), case, n))
    g = torch.Generator(device=dev).manual_seed(16)
    i = torch.arange(n + 1, device=dev)

    def operand(k):
        t = (-2.0 + 4.0 * ((i + 977 * k) % 8191).float() / 8191) + 0.25 * torch.randn(n + 1, device=dev, generator=g)
        t = t.to(dtype)
        return t[1:] if mis == "ab"[k] else t[:n]

    a, b = operand(0), operand(1)
    buf, out = _guarded(n, dtype, dev, shift=1 if mis == "y" else 0)
    ptrs = (a.data_ptr(), b.data_ptr(), out.data_ptr())
    fig.true("alignment", all(p % 16 == 0 for p in ptrs) == (mis is None), "pointers mod 16: %s" % [p % 16 for p in ptrs])
    F.check(lib.sscg_add(ptrs[0], ptrs[1], ptrs[2], dt, n, F._stream()), "sscg_add")
    fig.exact("sum", out, (a.cpu().float() + b.cpu().float()).to(dtype))
    fig.true("guards", _guards_intact(buf, out))
    fig.check()


# ----------------------------------------------------------------------------------------------------------------- 3. reflection pad
PAD_CASES = {
    "pad1": (2, 5, 2, 7, 1),            # the ResNet blocks' pad = 1, on H = 2 (pad = H - 1: both rows mirror onto each other)
    "pad_h_minus_1": (1, 3, 4, 9, 3),   # the largest legal pad: every row but the mirror row itself is read twice
    "pad0": (2, 3, 5, 6, 0),            # a copy
    "odd": (3, 7, 11, 6, 2),            # H != W, odd C
    # padded 2 x 64 x 136 x 132 = 2,297,856 > CAP: the forward's second round covers 200,704 elements (the adjoint's 2,096,640 source
    # elements stay 512 below the cap)
    "beyond_cap": (2, 64, 130, 126, 3),
}


@DTYPES
@pytest.mark.parametrize("cid", list(PAD_CASES))
def test_reflect_pad_forward_and_adjoint(cid, dtype, F, dev):
    """sscg_reflect_pad is torch.equal to TF.pad(mode="reflect"); sscg_reflect_pad_bwd against autograd in fp64: fp32 within
    test_reflect_pad_adjoint's 1e-5 (absolute; dy of the same magnitude as there), bf16 within one rounding of the result."""
    N, C, H, W, pad = PAD_CASES[cid]
    fig = _Figures("reflect_pad %s %s" % (cid, _name(dtype)))
    x = _table((N, C, H, W), 17, dtype)
    gy = _table((N, C, H + 2 * pad, W + 2 * pad), 18, dtype, -1.0, 1.0, 0.5)
    with _nan_outputs():
        y = F.reflect_pad(_dev4(x, dev, dtype), pad)
        dx = F.reflect_pad_bwd(_dev4(gy, dev, dtype), pad)
    fig.true("dtype_and_shape", y.dtype == dtype and dx.dtype == dtype and tuple(dx.shape) == (N, C, H, W))
    fig.exact("forward", y.float(), TF.pad(x, (pad, pad, pad, pad), mode="reflect") if pad else x)
    ref = ref_reflect_bwd((N, C, H, W), gy, pad)
    if dtype == F32:
        fig.add("adjoint_abs", _maxabs(dx, ref), 1e-5)
    else:
        fig.add("adjoint", _maxnorm(dx, ref), EPS16)
    fig.check()


def test_reflect_pad_refuses_a_pad_of_the_map_size(F, dev):
    """pad = H and pad = W have no mirror image (TF.pad refuses them too): SSCG_ERR_BAD_ARG, forward and adjoint."""
    for shape, pad in (((1, 3, 4, 9), 4), ((1, 3, 9, 4), 4)):
        x = torch.zeros(shape, device=dev).contiguous(memory_format=CL)
        dy = torch.zeros((shape[0], shape[1], shape[2] + 2 * pad, shape[3] + 2 * pad), device=dev).contiguous(memory_format=CL)
        with pytest.raises(F._lib.SscgError):
            F.reflect_pad(x, pad)
        with pytest.raises(F._lib.SscgError):
            F.reflect_pad_bwd(dy, pad)
        with pytest.raises(RuntimeError):
            TF.pad(x.cpu(), (pad, pad, pad, pad), mode="reflect")
    torch.cuda.synchronize()
    print("pointwise_regimes reflect_pad refusals ok")


# ----------------------------------------------------------------------------------------------------------------- 4. layout transposes
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("C", [1, 3, 33, 65, 2048])
def test_layout_transposes(C, N, F, dev):
    """sscg_nchw_to_nhwc / sscg_nhwc_to_nchw (32x32 LDS tiles): C = 33, 65, 2048 are 2, 3 and 64 tile rows (65: a last tile of one
    row), C = 1, 3 a ragged single one; 33 x 31 = 1023 pixels is one short of 32 tile columns; a 1x1 map is one ragged tile.  Called on
    guarded buffers (the wrappers skip the kernel when C = 1 or the map is 1x1: the memory is the same either way)."""
    lib = F._lib.lib
    for H, W in ((33, 31), (1, 1)):
        fig = _Figures("transpose N=%d C=%d %dx%d" % (N, C, H, W))
        x = _table((N, C, H, W), 19)
        xg = x.to(dev)
        buf, nhwc = _guarded(x.numel(), F32, dev)
        F.check(lib.sscg_nchw_to_nhwc(xg.data_ptr(), nhwc.data_ptr(), N, C, H, W, F._stream()), "sscg_nchw_to_nhwc")
        fig.exact("to_nhwc", nhwc, x.permute(0, 2, 3, 1).contiguous().flatten())
        fig.true("to_nhwc_guards", _guards_intact(buf, nhwc))
        buf2, nchw = _guarded(x.numel(), F32, dev)
        F.check(lib.sscg_nhwc_to_nchw(nhwc.data_ptr(), nchw.data_ptr(), N, C, H, W, F._stream()), "sscg_nhwc_to_nchw")
        fig.exact("to_nchw", nchw, x.flatten())
        fig.true("to_nchw_guards", _guards_intact(buf2, nchw))
        with _nan_outputs():
            y = F.to_nhwc(xg)
            z = F.to_nchw(y)
        fig.true("wrapper_layouts", y.is_contiguous(memory_format=CL) and z.is_contiguous())
        fig.exact("wrapper_to_nhwc", y, x)
        fig.exact("wrapper_round_trip", z, x)
        fig.check()


# ----------------------------------------------------------------------------------------------------------------- 5. max pools
def _pool_input(shape, seed, dtype):
    """Many exact ties: values on a grid of 0.25 (bf16-exact), the negative half clipped to 0 (as test_maxpool's relu).  The saw-tooth
    has a period of 7 elements here, so that a map of a few pixels spans the whole range as well (2^21 = 1 mod 7)."""
    x = _table(shape, seed, dtype, -2.0, 2.0, 0.5, period=7)
    return (x * 4).round().div(4).clamp_min(0.0)


def _pool3(shape, dtype, F, dev, fig):
    x = _pool_input(shape, 20, dtype)
    yr, dxr, gy = ref_pool(x, lambda s: _table(s, 21, dtype, -1.0, 1.0, 0.5), 3)
    xg = _dev4(x, dev, dtype).requires_grad_(True)
    with _nan_outputs():
        yg = F.MaxPoolFn.apply(xg)
        fig.true("shape", tuple(yg.shape) == tuple(yr.shape) and yg.dtype == dtype, str(tuple(yg.shape)))
        yg.backward(_dev4(gy, dev, dtype))
    fig.exact("forward", yg.float(), yr.float())
    # fp32: test_maxpool's bound; bf16: test_pointwise_bf16's (an element's gradient is a sum of up to four dy, rounded once)
    fig.add("backward", _maxnorm(xg.grad, dxr), TOL_POINT[dtype])


@DTYPES
def test_maxpool3x3_small_maps(dtype, F, dev):
    """MaxPoolFn (3x3, stride 2, pad 1, ceil mode) on every map of 1..5 x 1..5 pixels (N = 3, C = 5): windows that hold one to nine
    pixels, output sizes where the ceil-mode rule drops the last window (H = 1: one window that starts in the padding)."""
    fig = _Figures("maxpool3 %s" % _name(dtype))
    for H in range(1, 6):
        for W in range(1, 6):
            fig.label = "maxpool3 %s %dx%d" % (_name(dtype), H, W)
            _pool3((3, 5, H, W), dtype, F, dev, fig)
    fig.check()


@DTYPES
def test_maxpool3x3_beyond_the_cap(dtype, F, dev):
    """(4, 64, 259, 131) -> 130 x 66: 2,196,480 outputs (a second round of 99,328) and 8,686,592 input gradients (4.1 rounds)."""
    fig = _Figures("maxpool3 %s beyond_cap" % _name(dtype))
    _pool3((4, 64, 259, 131), dtype, F, dev, fig)
    fig.check()


def _pool2(shape, dtype, F, dev, fig):
    x = _pool_input(shape, 22, dtype)
    yr, dxr, gy = ref_pool(x, lambda s: _table(s, 23, dtype, -1.0, 1.0, 0.5), 2)
    xg = _dev4(x, dev, dtype).requires_grad_(True)
    with _nan_outputs():
        yg = F.maxpool2x2(xg)
        fig.true("shape", tuple(yg.shape) == tuple(yr.shape) and yg.dtype == dtype, str(tuple(yg.shape)))
        yg.backward(_dev4(gy, dev, dtype))
    fig.exact("forward", yg.float(), yr.float())
    fig.exact("backward", xg.grad.float(), dxr.float())         # windows do not overlap: a gradient is one dy or zero, a copy
    P, Q = shape[2] // 2, shape[3] // 2
    g = xg.grad.float().cpu()
    fig.true("zero_past_2P_2Q", bool((g[:, :, 2 * P:, :] == 0).all()) and bool((g[:, :, :, 2 * Q:] == 0).all()))


@DTYPES
def test_maxpool2x2_odd_and_even_maps(dtype, F, dev):
    """maxpool2x2 (floor mode) on H, W in {2, 3, 4, 7}: the odd sizes leave a last row / column that no window covers."""
    fig = _Figures("maxpool2 %s" % _name(dtype))
    for H in (2, 3, 4, 7):
        for W in (2, 3, 4, 7):
            fig.label = "maxpool2 %s %dx%d" % (_name(dtype), H, W)
            _pool2((3, 5, H, W), dtype, F, dev, fig)
    fig.check()


@DTYPES
def test_maxpool2x2_beyond_the_cap(dtype, F, dev):
    """(4, 64, 183, 183) -> 91 x 91: 2,119,936 outputs (a second round of 22,784; a 181 x 181 map stays below the cap), 8,573,184 input
    gradients, a last row and column without a window."""
    fig = _Figures("maxpool2 %s beyond_cap" % _name(dtype))
    _pool2((4, 64, 183, 183), dtype, F, dev, fig)
    fig.check()


# ----------------------------------------------------------------------------------------------------------------- 6. bilinear resize
RESIZE_CASES = {
    "down": ((2, 4, 65, 33), (17, 9)),                  # scale 4: three of four source rows / columns get no gradient
    "to_one_row": ((1, 3, 9, 9), (1, 5)),               # OH = 1: scale 0, every output row reads source row 0 only
    "from_one_row": ((1, 3, 1, 7), (6, 7)),             # H = 1; W unchanged (scale exactly 1)
    "near_integer": ((1, 2, 33, 33), (257, 255)),       # 32 / 256 = 1 / 8 exactly beside 32 / 254: source positions next to integers
    # 32 x 64 x 33 x 33 = 2,230,272 source elements > CAP: the backward's second round covers 133,120 (and the forward's 2,652,160
    # outputs a second round of 555,008).  The map is test_upsample's 33 x 33, not a large one with few channels: a source position is
    # scale * index in fp32, off by up to 2^-24 of its size, so the bound of 1e-5 that holds at 33 pixels cannot hold at 513, where
    # torch's own fp32 arithmetic is 3e-5 from fp64 (profiles/pointwise_regimes.txt)
    "backward_beyond_cap": ((32, 64, 33, 33), (35, 37)),
}


@pytest.mark.parametrize("cid", list(RESIZE_CASES))
def test_bilinear_resize_forward_and_backward(cid, F, dev):
    """upsample_bilinear against TF.interpolate(align_corners=True) in fp64, test_upsample's bounds (1e-5, forward and backward)."""
    shape, size = RESIZE_CASES[cid]
    fig = _Figures("resize %s" % cid)
    x = _table(shape, 24)
    gy = _table(shape[:2] + size, 25, F32, -1.0, 1.0, 0.5)
    yr, dxr = ref_upsample(x, gy, size)
    xg = _dev4(x, dev).requires_grad_(True)
    with _nan_outputs():
        yg = F.upsample_bilinear(xg, size)
        yg.backward(_dev4(gy, dev))
    fig.true("shape", tuple(yg.shape) == tuple(yr.shape))
    fig.add("forward", _maxnorm(yg, yr), 1e-5)
    fig.add("backward", _maxnorm(xg.grad, dxr), 1e-5)
    fig.check()


# ----------------------------------------------------------------------------------------------------------------- 7. resize_channels
@pytest.mark.parametrize("rows", [1, 255, 257, 70001])
def test_resize_channels(rows, F, dev):
    """sscg_resize_channels: pad (Cd > Cs), slice (Cd < Cs) and copy, on the f32x4 store path (Cd % 4 == 0: 24, 32, 8, 4) and the scalar
    one (21, 3, 5, 1).  One thread per 4 destination channels: rows * ceil(Cd / 4) is no multiple of 256 at any of these row counts
    (the last block is ragged); 70001 rows are 274 to 2,188 blocks.  Nothing past rows * Cd is written."""
    lib = F._lib.lib
    fig = _Figures("resize_channels rows=%d" % rows)
    for Cs, Cd in ((21, 24), (20, 32), (3, 8), (24, 21), (8, 3), (21, 21), (3, 5), (5, 3), (1, 4), (4, 1)):
        src = _table((rows, Cs), 26, F32, 1.0, 3.0)           # never zero: a padded zero is not a copied value
        sg = src.to(dev)
        buf, dst = _guarded(rows * Cd, F32, dev)
        F.check(lib.sscg_resize_channels(sg.data_ptr(), dst.data_ptr(), rows, Cs, Cd, F._stream()), "sscg_resize_channels")
        ref = torch.zeros(rows, Cd)
        ref[:, :min(Cs, Cd)] = src[:, :min(Cs, Cd)]
        fig.exact("%d_to_%d" % (Cs, Cd), dst, ref)
        fig.true("%d_to_%d_guards" % (Cs, Cd), _guards_intact(buf, dst))
    fig.check()


# ----------------------------------------------------------------------------------------------------------------- 8. class axis
def _class_axis(shape, seed, F, dev, fig, softmax=True):
    """softmax2d forward / backward (test_softmax_ce_losses: 1e-6 / 1e-5), argmax_onehot and label_onehot (torch.equal), cross_entropy
    with out-of-range labels and its gradient under a weight of 0.37 (test_softmax_ce_losses and
    test_cross_entropy_ignores_out_of_range_labels: 1e-6 / 1e-5; ignored rows get exactly zero)."""
    n, C, h, w = shape
    x, lab, gy = class_inputs(shape, seed)
    valid = (lab >= 0) & (lab < C)
    with _nan_outputs():
        xg = _rows_dev(x, shape, dev)
        if softmax:
            sr, dsr = ref_softmax(x, gy)
            sg = F.softmax_fwd(xg)
            dsg = F.softmax_bwd(_rows_dev(gy, shape, dev), sg)
            fig.add("softmax", _maxnorm(_rows_cpu(sg), sr), 1e-6)
            fig.add("softmax_bwd", _maxnorm(_rows_cpu(dsg), dsr), 1e-5)
            del sg, dsg
            idx_r = x.max(1)[1]
            oh, idx = F.argmax_onehot(xg, want_index=True)
            fig.exact("argmax_index", idx.flatten(), idx_r)
            fig.exact("argmax_onehot", _rows_cpu(oh), torch.zeros_like(x).scatter_(1, idx_r[:, None], 1.0))
            fig.exact("argmax_index_alone", F.argmax_index(xg).flatten(), idx_r)
            del oh, idx
            lo = F.label_onehot(lab.view(n, 1, h, w).to(dev), C)
            ref = torch.zeros_like(x)
            ref[valid] = ref[valid].scatter_(1, lab[valid][:, None], 1.0)
            fig.exact("label_onehot", _rows_cpu(lo), ref)
            del lo
        lr, dxr = ref_ce(x, lab, 0.37)
        xl = xg.detach().requires_grad_(True)
        lg = F.cross_entropy(xl, lab.view(n, h, w).to(dev))
        F.weighted_sum([lg], [0.37]).backward()
    fig.add("ce_loss", _maxnorm(lg, lr), 1e-6)
    got = _rows_cpu(xl.grad)
    fig.add("ce_grad", _maxnorm(got, dxr), 1e-5)
    fig.true("ce_grad_zero_on_ignored_rows", bool((got[~valid] == 0).all()), "%d ignored rows" % int((~valid).sum()))


@pytest.mark.parametrize("C", [1, 2, 21, 64])
def test_class_axis_class_counts(C, F, dev):
    """C = 1 (softmax 1, loss 0, gradients 0), 2, 21 and 64 = MAXC (the full per-thread array) on 3 x 17 x 19 = 969 rows: four blocks,
    the last of 201 rows."""
    fig = _Figures("class_axis C=%d" % C)
    _class_axis((3, C, 17, 19), 40 + C, F, dev, fig)
    fig.check()


def test_class_axis_rows_beyond_the_cap(F, dev):
    """(2, 4, 1025, 1025): 2,101,250 rows > CAP: the row loops of softmax, argmax, one-hot and the cross-entropy backward take a second
    round of 4,098 rows; the cross-entropy forward (LCAP) runs eight full rounds and a ninth of 4,098."""
    fig = _Figures("class_axis rows_beyond_cap")
    _class_axis((2, 4, 1025, 1025), 50, F, dev, fig)
    fig.check()


def test_cross_entropy_loss_grid_rounds(F, dev):
    """3 x 419 x 419 = 526,683 rows at C = 21: two full rounds of the 1024-block loss grid (524,288) and a third of 2,395 rows (ten
    blocks, the last of 91), all 1024 partials summed by finish_ce_kernel; ~5 % void and ~1 % negative labels."""
    fig = _Figures("class_axis ce_rounds")
    _class_axis((3, 21, 419, 419), 51, F, dev, fig, softmax=False)
    fig.check()


def test_class_axis_refuses_65_classes(F, dev):
    """C = 65 > MAXC: softmax (forward, backward) and cross entropy (forward, backward) are refused, not run on a short array."""
    lib = F._lib.lib
    x = torch.zeros(1, 65, 3, 3, device=dev).contiguous(memory_format=CL)
    lab = torch.zeros(1, 3, 3, dtype=torch.int64, device=dev)
    with pytest.raises(F._lib.SscgError):
        F.softmax2d(x)
    with pytest.raises(F._lib.SscgError):
        F.softmax_bwd(x, x)
    with pytest.raises(F._lib.SscgError):
        F.cross_entropy(x, lab)
    dx = torch.zeros_like(x)
    assert lib.sscg_ce_bwd(x.data_ptr(), lab.data_ptr(), 9, 65, None, 1.0, None, dx.data_ptr(), F._stream()) != 0
    torch.cuda.synchronize()
    print("pointwise_regimes class_axis C=65 refusals ok")


# ----------------------------------------------------------------------------------------------------------------- 9. scalar losses
@pytest.mark.parametrize("n", [1, 255, 257, 2 * LCAP + 77, N2])
def test_scalar_losses_and_weighted_sum(n, F, dev):
    """l1_loss, mse_const (targets 1 and 0), mse_loss and their gradients through weighted_sum under an upstream gradient of 1.7,
    test_mse_l1_weighted's bound (1e-6) throughout (test_maxpool2x2_and_mse_between_tensors has the same for mse_loss).
    2 LCAP + 77: every forward thread sums two elements, 77 threads a third (1024 partials); N2 = 8 LCAP + 257: the forwards run nine
    rounds, the backward kernels (CAP) a second one of 257.  Exact ties of the L1 pair get a gradient of exactly 0."""
    fig = _Figures("losses n=%d" % n)
    t = loss_inputs(n)
    r = ref_losses(t)
    dv = {k: v.view(1, 1, 1, n).to(dev).requires_grad_(k != "b1") for k, v in t.items()}
    with _nan_outputs():
        l1 = F.l1_loss(dv["a1"], dv["b1"])
        m1 = F.mse_const(dv["d"], 1.0)
        m0 = F.mse_const(dv["d"], 0.0)
        ms = F.mse_loss(dv["a2"], dv["b2"])
        tot = F.weighted_sum([l1, m1, m0, ms], LOSS_W)
        tot.backward(torch.tensor(LOSS_G, device=dev))
    for name, got in (("l1", l1), ("m1", m1), ("m0", m0), ("mse", ms), ("tot", tot)):
        fig.add(name, _maxnorm(got, r[name]), 1e-6)
    for name, key in (("da1", "a1"), ("dd", "d"), ("da2", "a2"), ("db2", "b2")):
        fig.add(name, _maxnorm(dv[key].grad, r[name]), 1e-6)
    tie = (t["a1"] == t["b1"])
    fig.true("l1_ties_zero_gradient", bool((dv["a1"].grad.flatten().cpu()[tie] == 0).all()) and (n < 4 or int(tie.sum()) > 0),
             "%d ties" % int(tie.sum()))
    fig.check()


def test_weighted_sum_of_16_terms_and_refusal_of_17(F, dev):
    """sscg_weighted_sum at its limit of 16 terms (terms and weights positive: a sum that cancels has no scale to be relative to),
    gradients w_i * g, and the RAW entry's refusal of 17 (functional.weighted_sum folds beyond 16: the test below)."""
    import ctypes as C
    fig = _Figures("weighted_sum")
    vals = [1.0 + 0.37 * k for k in range(17)]
    ws = [0.25 + 0.11 * ((7 * k) % 17) for k in range(17)]
    terms = [torch.tensor(v, device=dev, requires_grad=True) for v in vals]
    with _nan_outputs():
        out = F.weighted_sum(terms[:16], ws[:16])
        out.backward(torch.tensor(LOSS_G, device=dev))
    v32 = [float(torch.tensor(v)) for v in vals]
    w32 = [float(torch.tensor(w)) for w in ws]
    fig.add("sum16", abs(float(out) - sum(a * b for a, b in zip(v32[:16], w32[:16]))) / sum(a * b for a, b in zip(v32[:16], w32[:16])), 1e-6)
    fig.add("grads16", max(abs(float(t.grad) - w * float(torch.tensor(LOSS_G))) / (w * LOSS_G) for t, w in zip(terms[:16], w32)), 1e-6)
    raw = torch.full((), 7.0, device=dev)
    rc = F.lib.sscg_weighted_sum((C.c_void_p * 17)(*[t.data_ptr() for t in terms]), (C.c_float * 17)(*ws), 17, raw.data_ptr(), F._stream())
    torch.cuda.synchronize()
    fig.true("raw_entry_refuses_17", rc != 0 and float(raw) == 7.0, "rc %d" % rc)
    fig.check()


def _wsum_case(n):
    """n terms of mixed sign over seven decades, weights of mixed sign: (terms, weights) as python floats that are fp32 values."""
    vals = [(-1.0) ** (k // 2) * (1.0 + 0.37 * k) * 10.0 ** ((5 * k) % 7 - 3) for k in range(n)]
    ws = [(-1.0) ** (k % 3 == 1) * (0.25 + 0.11 * ((7 * k) % 17)) for k in range(n)]
    return [float(torch.tensor(v)) for v in vals], [float(torch.tensor(w)) for w in ws]


@pytest.mark.parametrize("n", [16, 17, 31, 32, 40])
def test_weighted_sum_of_any_number_of_terms(n, F, dev, monkeypatch):
    """functional.weighted_sum beyond the raw entry's 16 terms (every loss flag plus --variants l1_cycle is 18): up to 16 it is ONE
    launch with the raw entry's own bits; beyond, the first launch sums terms 0..15 and each later one takes the running partial
    sum with weight 1 plus the next 15 terms, in index order (17 and 32: a last launch of the partial and ONE term; 31: exactly full).
    Value against the fp64 sum of the same fp32 terms and weights within n * 2^-24 * sum_i |w_i t_i| - each product and each add
    rounds once in fp32, the partial never exceeds sum |w_i t_i|; a fused multiply-add only rounds less - and every term's gradient
    is fl(w_i * g), bit for bit."""
    import ctypes as C
    fig = _Figures("weighted_sum n=%d" % n)
    vals, ws = _wsum_case(n)
    terms = [torch.tensor(v, device=dev, requires_grad=True) for v in vals]
    calls = []
    real = F.lib.sscg_weighted_sum

    def counted(tab, w, k, out, stream):
        calls.append((k, tab[0], w[0], out))
        return real(tab, w, k, out, stream)
    monkeypatch.setattr(F.lib, "sscg_weighted_sum", counted)
    with _nan_outputs():
        out = F.weighted_sum(terms, ws)
        fwd = list(calls)
        out.backward(torch.tensor(LOSS_G, device=dev))
    monkeypatch.undo()
    want = F.weighted_sum_launches(n)
    fig.true("forward_launches", len(fwd) == want == (1 if n <= 16 else 1 + -(-(n - 16) // 15)), "%d launches, %d expected" % (len(fwd), want))
    sizes = [16] + [min(16, n - i + 1) for i in range(16, n, 15)] if n > 16 else [n]
    chained = all(c[0] == k and (j == 0 or (c[1] == fwd[j - 1][3] and c[2] == 1.0)) for j, (c, k) in enumerate(zip(fwd, sizes)))
    fig.true("fold_in_index_order", chained and fwd[0][1] == terms[0].data_ptr() and fwd[-1][3] == out.data_ptr(), "sizes %s" % [c[0] for c in fwd])
    fig.true("backward_one_launch_per_term", len(calls) - len(fwd) == n, "%d launches" % (len(calls) - len(fwd)))
    ref = sum(np.float64(a) * np.float64(b) for a, b in zip(vals, ws))
    scale = sum(abs(np.float64(a) * np.float64(b)) for a, b in zip(vals, ws))
    fig.add("value_vs_fp64", abs(float(out) - ref), n * 2.0 ** -24 * scale)
    g32 = torch.tensor(LOSS_G, dtype=F32)
    wrong = [i for i, (t, w) in enumerate(zip(terms, ws)) if t.grad is None or not torch.equal(t.grad.cpu(), torch.tensor(w, dtype=F32) * g32)]
    fig.true("grads_exactly_w_times_g", not wrong, "terms %s differ" % wrong)
    if n <= 16:     # today's path is one raw launch: the same bits
        raw = torch.zeros((), device=dev)
        rc = real((C.c_void_p * n)(*[t.data_ptr() for t in terms]), (C.c_float * n)(*ws), n, raw.data_ptr(), F._stream())
        fig.true("one_launch_bits", rc == 0 and torch.equal(raw.cpu().view(torch.int32), out.detach().cpu().view(torch.int32)))
    fig.check()


# ----------------------------------------------------------------------------------------------------------------- 10. confusion matrix
@pytest.mark.parametrize("C", [21, 64])
def test_confusion_hist_beyond_its_block_cap(C, F, dev):
    """n = HCAP + 4099: 1024 blocks, every thread counts 16 labels and 4,099 threads a 17th.  Void (255) and negative true labels,
    predictions >= C and negative (pairs that must be skipped, not folded into a neighbouring bin), accumulation into a non-zero
    matrix; C = 64: the largest LDS histogram (4096 bins, 16 per thread).  np.array_equal against np.bincount."""
    n = HCAP + 4099
    g = torch.Generator().manual_seed(60 + C)
    lt = torch.randint(0, C, (n,), generator=g, dtype=torch.int64)
    lp = (lt + torch.randint(0, 3, (n,), generator=g)) % C          # a strong diagonal: bins differ by orders of magnitude
    u = torch.rand(n, generator=g)
    lt[u < 0.05] = 255
    lt[(u >= 0.05) & (u < 0.06)] = -1
    lp[(u >= 0.04) & (u < 0.045)] = -3              # inside the void range of lt: both labels out of range on these pixels
    lp[(u >= 0.06) & (u < 0.07)] = C
    lp[(u >= 0.07) & (u < 0.075)] = 255
    lp[(u >= 0.075) & (u < 0.08)] = C * C + 1
    keep = (lt >= 0) & (lt < C) & (lp >= 0) & (lp < C)
    ref = np.bincount((C * lt[keep] + lp[keep]).numpy(), minlength=C * C).reshape(C, C)
    start = (torch.arange(C * C, dtype=torch.int64) * 3 + 1).view(C, C)
    h = start.clone().to(dev)
    out = F.confusion_hist(lt.to(dev), lp.to(dev), C, h)
    got = out.cpu().numpy()
    print("pointwise_regimes confusion_hist C=%d n=%d counted %d skipped %d differing bins %d of %d" % (
        C, n, int(keep.sum()), n - int(keep.sum()), int((got != start.numpy() + ref).sum()), C * C))
    assert out.data_ptr() == h.data_ptr()
    assert np.array_equal(got, start.numpy() + ref)
    with _nan_outputs():
        fresh = F.confusion_hist(lt.to(dev), lp.to(dev), C)
    assert np.array_equal(fresh.cpu().numpy(), ref)
