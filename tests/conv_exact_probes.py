"""Convolution inputs whose mathematically exact result is an fp32 (or bf16) number, and that result.

Every other convolution check of the suite carries a tolerance of 1e-5 or more; the low piece of the split contraction (csrc/common.h,
sscg_split3: x = h + m + l in bfloat16) weighs 2^-16 of its operand and the product m*m 2^-16 of the product: a kernel that loses
one of them in one region of the operand space passes those checks.  On the probes built here every summation order, tile class and
split-K plan has to return the same bits as the fp64 reference (tests/test_conv_exact_gpu.py); tests/test_conv_exact_host.py proves,
without a GPU, that the reference is exact and that the probes reach what they are for.  Shares no code with the library.

A probe is built for a shape (N, H, W, C, K, R, stride, pad, dil) and an entry: "fwd" (x, w -> y), "dgrad" (gy, w -> dx), "wgrad"
(x, gy -> dw).  Kinds:
  dense    small integers on both sides (|x|, |gy| <= 8, |w| <= 4, integer bias / addend / accumulate target): every partial sum in
           any order is an integer below 2^24 and every value is exact in bfloat16;
  carry-a  the FIRST operand of the entry (x, gy, x) holds values whose significand is WIDTH["carry"] bits wide with the lowest kept
           bit set (all three pieces needed), the other one is zero but for values +-2^j placed so that every output element
           receives at most one nonzero product: the result is +-2^j * a;
  carry-b  the roles exchanged: the SECOND operand (w, w, gy) carries, the first one is sparse;
  pair     carry-b's placement, both sides with significands of WIDTH["pair"] bits (l = 0, h and m nonzero for most values): the one
           product per output is h*h + h*m + m*h + m*m, at most 2 * WIDTH["pair"] bits wide.
bf16 tensors: the significands are WIDTH16 wide (carry: 8 bits, one bfloat16; pair: 4 + 4 bits, the product one bfloat16) - a pure
routing check.

Placement of the sparse side (what test_conv_exact_host.py asserts about it: at most one term per output; every tap, every filter,
the first, the last and one channel of every block of 64 in a nonzero product over the instances of a probe):
  sparse w   one (c, r, s) per filter (forward) / one (k, r, s) per channel (data gradient);
  sparse x   forward: a lattice of pixels, no two of them under one filter window, one channel per lattice point;
             weight gradient: one pixel per channel;
  sparse gy  data gradient: a lattice of output pixels no two of which reach one input pixel, one filter per lattice point;
             weight gradient: one pixel per filter.
Where one instance does not cover everything, further instances (other lattice origins and directions, the next taps / channels /
filters of the round-robin) are added until it does: `instances`."""
import functools
import math
import zlib

import torch
import torch.nn.functional as TF

F32, BF, F64 = torch.float32, torch.bfloat16, torch.float64
KINDS = ("dense", "carry-a", "carry-b", "pair")
WIDTH = {"carry": 23, "pair": 11}       # significand bits, fp32 tensors (24 bits: the orders h,l,m and l,h,m of the piece sums round)
WIDTH16 = {"carry": 8, "pair": 4}       # bf16 tensors
EXPONENTS = (-6, 6)                     # of the wide values
POWERS = (-3, 3)                        # j of the sparse side's +-2^j
DENSE_X, DENSE_W, DENSE_B = 8, 4, 16    # |x|, |gy|, addend, accumulate target <= 8; |w| <= 4; |bias| <= 16
SLOPE = 0.25                            # LeakyReLU slope of every epilogue run on a probe: exact
MAX_INSTANCES = 32
ENTRY_OPERANDS = {"fwd": ("x", "w"), "dgrad": ("gy", "w"), "wgrad": ("x", "gy")}


def split3(x):
    """sscg_split3 (csrc/common.h) in torch on the CPU: h = bf16(x), m = bf16(x - h), l = bf16((x - h) - m), as fp32 tensors"""
    h = x.to(BF).float()
    r1 = x - h
    m = r1.to(BF).float()
    return h, m, (r1 - m).to(BF).float()


def out_size(h, r, s, p, d):
    return (h + 2 * p - d * (r - 1) - 1) // s + 1


def tensor_shapes(shape):
    N, H, W, C, K, R, st, pad, d = shape
    return dict(x=(N, C, H, W), w=(K, C, R, R), gy=(N, K, out_size(H, R, st, pad, d), out_size(W, R, st, pad, d)))


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


def wide_values(shape, width, gen):
    """sign * (2^(width-1) + 2 r + 1) * 2^(e - width + 1): a significand exactly `width` bits wide (the lowest of them set), e uniform
    in EXPONENTS"""
    n = math.prod(shape)
    mant = torch.full((n,), 1, dtype=torch.int64)
    if width >= 2:
        mant = 2 ** (width - 1) + 1 + 2 * torch.randint(0, 2 ** (width - 2), (n,), generator=gen, dtype=torch.int64)
    e = torch.randint(EXPONENTS[0], EXPONENTS[1] + 1, (n,), generator=gen, dtype=torch.int64)
    sign = 2 * torch.randint(0, 2, (n,), generator=gen, dtype=torch.int64) - 1
    v = (sign * mant).double() * torch.pow(torch.tensor(2.0, dtype=F64), (e - (width - 1)).double())
    out = v.float()
    assert torch.equal(out.double(), v)
    return out.view(shape)


def power_values(n, gen):
    j = torch.randint(POWERS[0], POWERS[1] + 1, (n,), generator=gen, dtype=torch.int64)
    sign = 2 * torch.randint(0, 2, (n,), generator=gen, dtype=torch.int64) - 1
    return (sign.double() * torch.pow(torch.tensor(2.0, dtype=F64), j.double())).float()


def integer_values(shape, bound, gen):
    return torch.randint(-bound, bound + 1, shape, generator=gen, dtype=torch.int64).float()


def required_channels(C):
    """the first, the last and one channel of every block of 64"""
    req = {0, C - 1}
    for b in range(-(-C // 64)):
        req.add(64 * b + (17 * b + 5) % min(64, C - 64 * b))
    return sorted(req)


# ----------------------------------------------------------------------------------------------------------------- the reference
def reference(entry, shape, x=None, w=None, gy=None, dtype=F64, reflect=False):
    """the entry's result by torch's CPU convolution in `dtype` (fp64: the reference; fp32: what the host file compares with it).
    reflect (forward only): reflection padding in front of an unpadded convolution"""
    N, H, W, C, K, R, st, pad, d = shape
    if entry == "fwd":
        xin = x.to(dtype)
        if reflect:
            return TF.conv2d(TF.pad(xin, (pad, pad, pad, pad), mode="reflect"), w.to(dtype), None, st, 0, d)
        return TF.conv2d(xin, w.to(dtype), None, st, pad, d)
    if entry == "dgrad":
        return torch.nn.grad.conv2d_input((N, C, H, W), w.to(dtype), gy.to(dtype), st, pad, d)
    return torch.nn.grad.conv2d_weight(x.to(dtype), (K, C, R, R), gy.to(dtype), st, pad, d)


# ----------------------------------------------------------------------------------------------------------------- placement
def _axis_points(n, conflict, reverse, start):
    """greedy subset of range(n), visited from `start` upwards (downwards: reverse), no two members at a distance `conflict` rejects"""
    order = [(start + i) % n for i in range(n)]
    if reverse:
        order = [n - 1 - y for y in order]
    chosen = []
    for y in order:
        if all(not conflict(abs(y - c)) for c in chosen):
            chosen.append(y)
    return sorted(chosen)


def _lattice(N, n_y, n_x, conflict, inst):
    """[L, 3] (n, y, x): the product of two greedy axis sets in every image; the instance picks directions and origin"""
    ys = _axis_points(n_y, conflict, bool(inst & 1), inst >> 2)
    xs = _axis_points(n_x, conflict, bool(inst & 2), inst >> 2)
    g = torch.cartesian_prod(torch.arange(N), torch.tensor(ys), torch.tensor(xs))
    return g.view(-1, 3)


def _round_robin(count, inst, required, modulus, gen):
    """index j of instance `inst` stands for the global index jj = inst * count + j: required[jj] while the list lasts, then random"""
    jj = inst * count + torch.arange(count)
    rnd = torch.randint(0, modulus, (count,), generator=gen, dtype=torch.int64)
    req = torch.tensor(required, dtype=torch.int64)
    return torch.where(jj < len(required), req[jj.clamp_max(len(required) - 1)], rnd), jj


def _sparse_operand(entry, shape, which, inst, values, gen):
    """the sparse operand `which` ("w" / "x" / "gy") of an entry: zeros but for values(count) at the placement of the module docstring"""
    N, H, W, C, K, R, st, pad, d = shape
    shp = tensor_shapes(shape)
    P, Q = shp["gy"][2:]
    t = torch.zeros(shp[which])
    if which == "w" and entry == "fwd":                 # one (c, r, s) per filter
        c, jj = _round_robin(K, inst, required_channels(C), C, gen)
        tap = jj % (R * R)
        t[torch.arange(K), c, tap // R, tap % R] = values(K)
    elif which == "w":                                  # data gradient: one (k, r, s) per channel
        jj = inst * C + torch.arange(C)
        tap = jj % (R * R)
        t[jj % K, torch.arange(C), tap // R, tap % R] = values(C)
    elif which == "x" and entry == "fwd":               # two pixels under one window: a multiple of dil apart, at most R - 1 of them
        g = _lattice(N, H, W, lambda dl: dl % d == 0 and dl // d <= R - 1, inst)
        c, _ = _round_robin(len(g), inst, required_channels(C), C, gen)
        t[g[:, 0], c, g[:, 1], g[:, 2]] = values(len(g))
    elif which == "gy" and entry == "dgrad":            # two output pixels reach one input pixel: dp * stride = m * dil, |m| <= R - 1
        g = _lattice(N, P, Q, lambda dl: (dl * st) % d == 0 and dl * st // d <= R - 1, inst)
        k = (inst * len(g) + torch.arange(len(g))) % K
        t[g[:, 0], k, g[:, 1], g[:, 2]] = values(len(g))
    elif which == "gy":                                 # weight gradient: one pixel per filter
        n, p, q = (torch.randint(0, m, (K,), generator=gen, dtype=torch.int64) for m in (N, P, Q))
        t[n, torch.arange(K), p, q] = values(K)
    else:                                               # weight gradient: one pixel per channel
        n, y, xx = (torch.randint(0, m, (C,), generator=gen, dtype=torch.int64) for m in (N, H, W))
        t[n, torch.arange(C), y, xx] = values(C)
    return t


# ----------------------------------------------------------------------------------------------------------------- probes
def build(entry, shape, kind, bf16=False, inst=0):
    """one probe instance: dict(entry, kind, shape, inst, sparse = name of the sparse operand or None, full = name of the operand that
    carries, the entry's two operands by name, bias / addend / old (integers for dense, zeros elsewhere), exact = the fp64 result)"""
    shp = tensor_shapes(shape)
    a, b = ENTRY_OPERANDS[entry]
    gen = _gen(entry, shape, kind, bf16, inst)
    p = dict(entry=entry, kind=kind, shape=shape, inst=inst, sparse=None, full=None, bf16=bf16)
    out_shape = shp[{"fwd": "gy", "dgrad": "x", "wgrad": "w"}[entry]]
    if kind == "dense":
        for name in (a, b):
            p[name] = integer_values(shp[name], DENSE_W if name == "w" else DENSE_X, gen)
        p["bias"] = integer_values((out_shape[1],), DENSE_B, gen)
        p["addend"] = integer_values(out_shape, DENSE_X, gen)
        p["old"] = integer_values(out_shape, DENSE_X, gen)
    else:
        widths = WIDTH16 if bf16 else WIDTH
        full, sparse = (a, b) if kind == "carry-a" else (b, a)
        wd = widths["pair" if kind == "pair" else "carry"]
        p[full] = wide_values(shp[full], wd, gen)
        values = (lambda n: wide_values((n,), wd, gen)) if kind == "pair" else (lambda n: power_values(n, gen))
        p[sparse] = _sparse_operand(entry, shape, sparse, inst, values, gen)
        p.update(sparse=sparse, full=full, width=wd, bias=torch.zeros(out_shape[1]), addend=torch.zeros(out_shape), old=torch.zeros(out_shape))
    p["exact"] = reference(entry, shape, x=p.get("x"), w=p.get("w"), gy=p.get("gy"))
    return p


def _taps_any(n_in, n_out, R, st, pad, d):
    """[R] bool: tap r reaches inside the input from some output position"""
    pos = torch.arange(n_out).view(-1, 1) * st - pad + torch.arange(R).view(1, -1) * d
    return ((pos >= 0) & (pos < n_in)).any(0)


def _taps_of_output(p0, n_in, R, st, pad, d):
    """[L, R] bool: tap r of output position p0 lies inside the input"""
    pos = p0.view(-1, 1) * st - pad + torch.arange(R).view(1, -1) * d
    return (pos >= 0) & (pos < n_in)


def _taps_of_input(y0, n_out, R, st, pad, d):
    """[L, R] bool: input position y0 is tap r of some output position"""
    t = y0.view(-1, 1) + pad - torch.arange(R).view(1, -1) * d
    return (t % st == 0) & (t >= 0) & (t // st < n_out)


def coverage(p):
    """(taps [R, R] bool, set of filters, set of channels) that occur in a nonzero product of a carry / pair probe: derived from the
    nonzero elements of the sparse operand (the other operand has no zero)"""
    N, H, W, C, K, R, st, pad, d = p["shape"]
    P, Q = tensor_shapes(p["shape"])["gy"][2:]
    nz = p[p["sparse"]].nonzero()
    if p["sparse"] == "w":
        ok = _taps_any(H, P, R, st, pad, d)[nz[:, 2]] & _taps_any(W, Q, R, st, pad, d)[nz[:, 3]]
        nz = nz[ok]
        taps = torch.zeros(R, R, dtype=torch.bool)
        taps[nz[:, 2], nz[:, 3]] = True
        return taps, set(nz[:, 0].tolist()), set(nz[:, 1].tolist())
    if p["sparse"] == "x":
        ty, tx = _taps_of_input(nz[:, 2], P, R, st, pad, d), _taps_of_input(nz[:, 3], Q, R, st, pad, d)
    else:
        ty, tx = _taps_of_output(nz[:, 2], H, R, st, pad, d), _taps_of_output(nz[:, 3], W, R, st, pad, d)
    taps = (ty.float().t() @ tx.float()) > 0
    hit = set(nz[ty.any(1) & tx.any(1), 1].tolist())
    return (taps, set(range(K)), hit) if p["sparse"] == "x" else (taps, hit, set(range(C)))


def covered(probes):
    """dict(taps, filters, channels, nonzero): the union over the instances of a probe; nonzero = share of the result's elements that are
    nonzero in at least one instance"""
    taps, filters, channels, nzero = None, set(), set(), None
    for p in probes:
        t, f, c = coverage(p)
        taps = t if taps is None else taps | t
        filters |= f
        channels |= c
        nzero = (p["exact"] != 0) if nzero is None else nzero | (p["exact"] != 0)
    return dict(taps=taps, filters=filters, channels=channels, nonzero=float(nzero.double().mean()))


def complete(probes):
    """what the host file asks of the instances of a carry / pair probe together"""
    C, K = probes[0]["shape"][3:5]
    cov = covered(probes)
    ok = bool(cov["taps"].all()) and cov["filters"] == set(range(K)) and set(required_channels(C)) <= cov["channels"]
    if probes[0]["entry"] == "wgrad" and probes[0]["kind"] == "carry-a":
        ok = ok and cov["nonzero"] >= 0.5
    return ok


@functools.lru_cache(maxsize=16)
def instances(entry, shape, kind, bf16=False):
    """the instances of one probe, built once (a bounded cache: the families of a case run one after the other)"""
    out = [build(entry, shape, kind, bf16, 0)]
    while kind != "dense" and not complete(out) and len(out) < MAX_INSTANCES:
        out.append(build(entry, shape, kind, bf16, len(out)))
    return tuple(out)


# ----------------------------------------------------------------------------------------------------------------- expected values
def activation(z, act):
    """0 none, 1 ReLU, 2 LeakyReLU with SLOPE, on the fp64 pre-activation"""
    if act == 1:
        return z.clamp_min(0)
    if act == 2:
        return torch.where(z > 0, z, z * SLOPE)
    return z


def stored(z, dtype):
    """the exact fp64 value as the tensor of `dtype` holds it: fp32 unchanged (asserted), bf16 rounded once to nearest even"""
    f = z.float()
    assert torch.equal(f.double(), z), "the expected value is no fp32 number"
    return f.to(dtype).float()


def two_roundings(dgrad, addend):
    """bf16 data gradient with a joined addend: bf16(bf16(dgrad) + addend), the sum formed in fp32"""
    return (stored(dgrad, BF) + addend.to(BF).float()).to(BF).float()


# ----------------------------------------------------------------------------------------------------------------- the PixelDiscriminator front
FRONT_X, FRONT_W1, FRONT_B1, FRONT_W2, FRONT_B2 = 8, 4, 16, 4, 16


@functools.lru_cache(maxsize=4)
def front_probe(shape, cin):
    """dense probe of conv2d_front_fwd: y = conv1x1(lrelu(conv1x1(x, w1) + b1, SLOPE), w2) + b2; h1 holds multiples of SLOPE"""
    N, H, W, mid, K = shape[:5]
    gen = _gen("front", shape, cin)
    x, w1, b1 = integer_values((N, cin, H, W), FRONT_X, gen), integer_values((mid, cin, 1, 1), FRONT_W1, gen), integer_values((mid,), FRONT_B1, gen)
    w2, b2 = integer_values((K, mid, 1, 1), FRONT_W2, gen), integer_values((K,), FRONT_B2, gen)
    h1 = activation(TF.conv2d(x.double(), w1.double(), b1.double()), 2)
    y = TF.conv2d(h1, w2.double(), b2.double())
    return dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, h1=h1, y=y)


# ----------------------------------------------------------------------------------------------------------------- reporting a mismatch
def mismatch(got, exp, names):
    """'' when got == exp element for element (no NaN; the sign of a zero does not count), else: the count of differing elements, the
    first differing index by `names`, and the error there against 2^-8, 2^-16, 2^-24 of the expected value (which names the lost piece)"""
    got, exp = got.detach().float().cpu(), exp.float()
    if tuple(got.shape) != tuple(exp.shape):
        return "shape %s, expected %s" % (tuple(got.shape), tuple(exp.shape))
    bad = ~(got == exp)
    if not bool(bad.any()):
        return ""
    idx = bad.nonzero()[0].tolist()
    g, e = float(got[tuple(idx)]), float(exp[tuple(idx)])
    err, ref = abs(g - e), abs(e) if e != 0 else float(exp.abs().max())
    return "%d of %d elements differ (%d NaN); first at (%s): got %r expected %r; error / (|expected| * 2^-8, 2^-16, 2^-24) = %.3g, %.3g, %.3g" % (
        int(bad.sum()), bad.numel(), int(torch.isnan(got).sum()), ", ".join("%s=%d" % (n, i) for n, i in zip(names, idx)), g, e,
        err / (ref * 2.0 ** -8 + 1e-300), err / (ref * 2.0 ** -16 + 1e-300), err / (ref * 2.0 ** -24 + 1e-300))
