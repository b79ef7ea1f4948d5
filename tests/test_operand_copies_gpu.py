"""Every cached operand copy of a weight equals a fresh one, bit for bit.

In the split mode (`--dtype f32`) and in bf16 mode no convolution reads the fp32 master weights: the kernels read copies - the
split planes / bf16 shadow of an optimiser arena (rewritten by the Adam kernel), transposed copies cached on the weight
(`_sscg_wt`, `_sscg_wt16`, `_sscg_wtx3`), plain copies of weights no arena owns (`_sscg_w16`, `_sscg_wx3`), and the 32-channel
paddings of 21 / 20-channel stems and heads (`_sscg_wpad`, `_sscg_wpadk`) with second-level copies cached on the padded tensor.
A stale copy neither crashes nor produces garbage - it is a step computed with weights one update (~lr) old, which is what the
multi-step tolerances are built to accept.  So this file checks the one property all the invalidation mechanisms exist for: at the
moment a convolution reads a copy, the copy is what one gets by deriving it NOW from the current fp32 weight.

Every comparison is equality of bits (int16 / int32 views), except the fp64 Adam comparison, which reuses the 1e-6 of
test_kernels_gpu.py::test_adam_matches_torch.

Launch geometry of the kernels involved (csrc/): `sscg_split3` has one thread per 8 elements and NO cap on its grid (no grid-stride
loop: the grid grows with n; a block covers 2048 elements); `sscg_cast` caps its grid at 8192 blocks of 256 and `sscg_adam_step`
at 16384 blocks of 256 - both loop beyond that, and both are run here at lengths beyond one pass."""
import collections
import contextlib
import io

import pytest
import torch

from conftest import load_sub

CL = torch.channels_last
BF = torch.bfloat16
CAST_PASS = 8192 * 256          # elements one grid pass of sscg_cast covers
ADAM_PASS = 16384 * 256         # ... of sscg_adam_step


# ------------------------------------------------------------------------------------------ the CPU restatement of common.h
def split3_ref(x):
    """sscg_split3 (csrc/common.h) in plain torch on the CPU: h = bf16(x), m = bf16(x - h), l = bf16((x - h) - m); fp32
    subtractions, round-to-nearest-even casts.  Returns the three bf16 planes."""
    assert x.dtype == torch.float32 and x.device.type == "cpu"
    h = x.to(BF)
    r1 = x - h.float()
    m = r1.to(BF)
    r2 = r1 - m.float()
    return h, m, r2.to(BF)


def _bits_to_f32(v):
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32).view(torch.float32)


def split_inputs(n, seed):
    """n fp32 values where a split can go wrong: weight-scale normals, tiny normals, wide uniforms, rounding ties of the bf16 cast
    (low 16 bits 0x8000), magnitudes log-uniform over 2^-100 ... 2^100 and exact +-0 - shuffled, so that a ragged tail holds all
    kinds.  Magnitudes stay inside [2^-100, 2^100] (or are exactly 0): see test_split3_emulation_reconstructs_exactly."""
    g = torch.Generator().manual_seed(seed)
    k = n // 6 + 1

    def bits(sign, ex, man, low):
        return _bits_to_f32((sign << 31) | (ex << 23) | (man << 16) | low)
    ri = lambda lo, hi: torch.randint(lo, hi, (k,), generator=g, dtype=torch.int64)
    parts = [torch.randn(k, generator=g) * 0.05,
             torch.randn(k, generator=g) * 1e-6,
             (torch.rand(k, generator=g) * 2 - 1) * 1e4,
             bits(ri(0, 2), ri(27, 227), ri(0, 128), 0x8000),                                       # ties
             bits(ri(0, 2), ri(27, 227), ri(0, 128), ri(0, 65536)),                                 # any mantissa, 2^-100 ... 2^100
             torch.zeros(k) * (ri(0, 2).float() * 2 - 1)]                                           # +0 and -0
    x = torch.cat(parts)
    tiny = (x != 0) & (x.abs() < 2.0 ** -100)          # (a normal draw may land below the range: lift it to the edge)
    x = torch.where(tiny, torch.full_like(x, 2.0 ** -100), x)
    return x[torch.randperm(x.numel(), generator=g)][:n].contiguous()


def test_split3_emulation_reconstructs_exactly():
    """h + m + l == x EXACTLY (in fp64) on weight-scale normals, 1e-6-scale normals, uniforms in +-1e4, rounding ties, magnitudes
    over 2^-100 ... 2^100 and +-0: three 8-bit pieces hold the 24-bit significand whenever no residual is subnormal.
    Out of scope: inputs whose residuals fall into the fp32 subnormal range (first failures at |x| ~ 1.2e-38) and inf / nan -
    no weight lives there."""
    x = split_inputs(3_000_000, 1)
    assert bool(((x == 0) | ((x.abs() >= 2.0 ** -100) & (x.abs() <= 2.0 ** 100))).all())
    assert int(((x.view(torch.int32) & 0xFFFF) == 0x8000).sum()) > 400_000            # the ties are in there
    h, m, l = split3_ref(x)
    assert torch.equal(h.double() + m.double() + l.double(), x.double())
    assert torch.equal(h, x.bfloat16())
    # -0 keeps its sign in the leading piece, the residuals of an exactly representable value are zero
    z = x == 0
    assert torch.equal(h[z].view(torch.int16), x[z].bfloat16().view(torch.int16)) and not bool(m[z].float().any()) and not bool(l[z].float().any())


# ------------------------------------------------------------------------------------------ helpers
def _bits(t):
    return t.detach().view(torch.int16 if t.dtype == BF else torch.int32)


def _mem(t):
    """The elements of t in memory order (channels-last for a 4-D tensor), as integers."""
    t = _bits(t)
    if t.dim() == 4:
        t = t.permute(0, 2, 3, 1)
    return t.contiguous().reshape(-1)


def _same(a, b):
    return a.dtype == b.dtype and a.numel() == b.numel() and torch.equal(_mem(a), _mem(b))


def _planes(flat, plane, n):
    """[3, n] view of three planes `plane` elements apart that start at flat's first element (flat may be a slice of an arena)."""
    return torch.as_strided(flat, (3, n), (plane, 1))


def _split3_gpu(F, x, plane=None):
    n = x.numel()
    plane = n if plane is None else plane
    out = torch.empty(3 * plane, dtype=BF, device=x.device)
    F.check(F.lib.sscg_split3(x.data_ptr(), out.data_ptr(), n, plane, F._stream()), "sscg_split3")
    return out


def _ref_planes(x_cpu):
    return torch.stack(split3_ref(x_cpu.reshape(-1).contiguous()))


@contextlib.contextmanager
def _mode(F, mode, batch=None):
    was = F.BATCH_TRANSPOSES[0]
    F.set_conv_precision(mode)
    if batch is not None:
        F.BATCH_TRANSPOSES[0] = batch
    try:
        yield
    finally:
        F.BATCH_TRANSPOSES[0] = was
        F.set_conv_precision("f32")


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


# ------------------------------------------------------------------------------------------ 1. the derivations themselves
@pytest.mark.gpu
@pytest.mark.parametrize("n", [10007, 3 * 2048 + 5, ADAM_PASS + 1031], ids=lambda n: "n%d" % n)
def test_split3_kernel_equals_emulation(F, dev, n):
    """lib.sscg_split3 against the CPU restatement: n not a multiple of 256 (nor of the 8 elements a thread takes), one block, a
    few blocks, two thousand blocks."""
    x = split_inputs(n, 2)
    got = _split3_gpu(F, x.to(dev)).cpu().view(3, n)
    assert torch.equal(_bits(got), _bits(_ref_planes(x)))


@pytest.mark.gpu
def test_split3_with_plane_stride_leaves_the_gaps_alone(F, dev):
    """The form FusedAdam.split_view uses: source and destination are a slice at an offset inside an arena, the plane stride is the
    ARENA's length - everything outside the three slices keeps its sentinel."""
    arena_n, off, n = 64 * 700, 64 * 3, 10007
    x = split_inputs(n, 3)
    src = torch.zeros(arena_n, device=dev)
    src[off:off + n] = x.to(dev)
    dst = torch.full((3 * arena_n,), -1.75, dtype=BF, device=dev)
    F.check(F.lib.sscg_split3(src[off:off + n].data_ptr(), dst[off:off + n].data_ptr(), n, arena_n, F._stream()), "sscg_split3")
    got = dst.cpu().view(3, arena_n)
    assert torch.equal(_bits(got[:, off:off + n]), _bits(_ref_planes(x)))
    untouched = torch.ones(3, arena_n, dtype=torch.bool)
    untouched[:, off:off + n] = False
    assert bool((got[untouched].float() == -1.75).all())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [10007, CAST_PASS + 777], ids=lambda n: "n%d" % n)
def test_cast_to_bf16_rounds_to_nearest_even(F, dev, n):
    """sscg_cast f32 -> bf16 (FusedAdam.refresh_shadow, the cached casts of frozen weights) == torch's cast, ties included; the
    longer length runs the kernel's grid-stride loop."""
    x = split_inputs(n, 4)
    got = F.cast(x.to(dev), BF).cpu()
    assert torch.equal(_bits(got), _bits(x.bfloat16()))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(40, 24, 3, 3), (64, 64, 3, 3)], ids=["ragged", "aligned"])
def test_transposed_split_copy_equals_emulation_of_the_permuted_weight(F, dev, shape):
    """weight_transposed(w, "x3"): [K][R][S][C] fp32 -> three planes of [C][R][S][K] bf16, the same split as everywhere."""
    k, c, r, s = shape
    w = split_inputs(k * c * r * s, 5).view(k, c, r, s).contiguous(memory_format=CL)
    got = F.weight_transposed(w.to(dev), "x3").cpu().view(3, w.numel())
    want = _ref_planes(w.permute(1, 2, 3, 0))          # logical [C][R][S][K], flattened in that order
    assert torch.equal(_bits(got), _bits(want))


# ------------------------------------------------------------------------------------------ 2. the Adam kernel's in-pass copies
@pytest.mark.gpu
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("n", [10007, ADAM_PASS + 1031], ids=lambda n: "n%d" % n)
def test_adam_kernel_writes_current_copies(F, dev, n, grad_scale):
    """F.adam_step with a split / bf16 / no shadow: the copy written in the pass is the split / cast of the NEW p; p, m, v do not
    depend on which copy was asked for; elements whose gradient has always been zero (arena padding, never-used parameters) do not
    move; and the update is torch.optim.Adam's (fp64, gradient pre-multiplied by grad_scale) to test_adam_matches_torch's 1e-6."""
    g = torch.Generator().manual_seed(11)
    p0 = torch.randn(n, generator=g) * 0.05
    idle = torch.zeros(n, dtype=torch.bool)
    idle[-64:] = True           # "padding": zero weight, zero gradient
    idle[100:164] = True        # a never-used parameter: non-zero weight, zero gradient
    p0[-64:] = 0.0
    grads = [torch.randn(n, generator=g).masked_fill_(idle, 0.0) for _ in range(3)]
    pr = p0.double().clone().requires_grad_(True)
    ref = torch.optim.Adam([pr], lr=2e-4, betas=(0.5, 0.999), eps=1e-8)
    runs = {}
    for kind in ("none", "bf16", "split"):
        p = p0.to(dev)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        sh = {"none": None, "bf16": torch.empty(n, dtype=BF, device=dev), "split": torch.empty(3 * n, dtype=BF, device=dev)}[kind]
        for step in range(1, 4):
            F.adam_step(p, grads[step - 1].to(dev), m, v, 2e-4, 0.5, 0.999, 1e-8, step, grad_scale,
                        shadow_bf16=sh if kind == "bf16" else None, shadow_split=sh if kind == "split" else None)
            torch.cuda.synchronize()
            if kind == "bf16":
                assert torch.equal(_bits(sh), _bits(p.to(BF))), step
                assert torch.equal(_bits(sh.cpu()), _bits(p.cpu().bfloat16())), step
            elif kind == "split":
                assert torch.equal(_bits(sh), _bits(_split3_gpu(F, p))), step
                assert torch.equal(_bits(sh.cpu().view(3, n)), _bits(_ref_planes(p.cpu()))), step
            if kind == "none":
                pr.grad = grads[step - 1].double() * grad_scale
                ref.step()
        runs[kind] = (p.cpu(), m.cpu(), v.cpu())
    for kind in ("bf16", "split"):
        for a, b in zip(runs[kind], runs["none"]):
            assert torch.equal(_bits(a), _bits(b)), kind
    p, m, v = runs["none"]
    assert torch.equal(_bits(p[idle]), _bits(p0[idle]))
    assert not bool(m[idle].any()) and not bool(v[idle].any())
    assert not torch.equal(p[~idle], p0[~idle])

    def rel_err(a, b):
        return float((a.double() - b.detach().double()).abs().max() / b.detach().double().abs().max().clamp_min(1e-30))
    assert rel_err(p, pr) < 1e-6
    assert rel_err(m, ref.state[pr]["exp_avg"]) < 1e-6
    assert rel_err(v, ref.state[pr]["exp_avg_sq"]) < 1e-6


# ------------------------------------------------------------------------------------------ 3. the checker
class Incoherent(AssertionError):
    """A copy under a CURRENT tag (or handed out by a getter) differs from a fresh derivation; `.what` lists (weight, form)."""

    def __init__(self, what):
        self.what = list(what)
        super().__init__("stale operand copies: " + ", ".join("%s: %s" % w for w in self.what[:12]) +
                         (" ... (%d in all)" % len(self.what) if len(self.what) > 12 else ""))

    def forms(self):
        return {f for _, f in self.what}


_STORED = {"_sscg_wt": "t32", "_sscg_wt16": "t16", "_sscg_wtx3": "tx3", "_sscg_w16": "w16", "_sscg_wx3": "wx3",
           "_sscg_wpad": "wpad", "_sscg_wpadk": "wpadk"}
_WT_DTYPE = {"t32": torch.float32, "t16": BF, "tx3": "x3"}


class _Fresh:
    """Every form of one weight derived now, from a private clone of its current fp32 data, with the standalone entry points."""

    def __init__(self, F, w):
        self.F = F
        w = w.detach().clone(memory_format=torch.preserve_format)
        self.w = w if w.is_contiguous(memory_format=CL) else w.contiguous(memory_format=CL)
        self.made = {}

    def get(self, form, size=32):
        F = self.F
        if form not in self.made:
            if "." in form:
                base, inner = form.split(".")
                pad = self.get(base, size)
                t = F._split3_copy(pad) if inner == "wx3" else F.weight_transposed(pad, "x3")
            elif form == "w16":
                t = F.cast(self.w, BF)
            elif form == "wx3":
                t = F._split3_copy(self.w)
            elif form in _WT_DTYPE:         # (the bf16 form: the clone belongs to no optimiser, its bf16 source is a cast of its own)
                t = F.weight_transposed(self.w, _WT_DTYPE[form])
            elif form == "wpad":
                t = F.resize_channels(self.w, size)
            elif form == "wpadk":
                t = F._pad_filters(self.w, size)
            else:
                raise KeyError(form)
            self.made[form] = t
        return self.made[form]


def _owner(w):
    opt = getattr(w, "_sscg_opt", None)
    return opt() if opt is not None else None


def _check_arena(F, opt, fails, seen):
    """The bf16 shadow / the three split planes of an optimiser arena against a fresh cast / split of the whole arena (padding
    included) - or, while torch has written a parameter and the optimiser has not re-derived its slice yet (`_shadow_ver` /
    `_split_ver` behind `_version`: the slice is rebuilt on its next use), of the slices that are recorded as current."""
    n_all = opt.arena.numel()
    for name, copy, vers, planes in (("arena16", opt.arena16, opt._shadow_ver, 1), ("arena_x3", opt.arena_x3, opt._split_ver, 3)):
        if copy is None:
            continue
        fresh = F.cast(opt.arena, BF) if planes == 1 else _split3_gpu(F, opt.arena)
        assert copy.numel() == planes * n_all
        got, want = _bits(copy).view(planes, n_all), _bits(fresh).view(planes, n_all)
        if all(vers.get(p) == p._version for p in opt.trainable):
            seen["stored:" + name] += 1
            if not torch.equal(got, want):
                fails.append(("optimiser arena", "stored " + name))
            continue
        for p in opt.trainable:
            if vers.get(p) == p._version:
                off, n = opt.slices[p]
                seen["stored:" + name + " slice"] += 1
                if not torch.equal(got[:, off:off + n], want[:, off:off + n]):
                    fails.append(("optimiser arena slice at %d" % off, "stored " + name))
            else:
                seen["behind:" + name] += 1


def _check_stored(F, name, w, fresh, fails, seen):
    tag = F._wtag(w)
    for attr, form in _STORED.items():
        ent = getattr(w, attr, None)
        if ent is None:
            continue
        if ent.tag != tag:
            seen["stale-tag:" + attr] += 1          # legitimately stale: rebuilt on its next use
            continue
        seen["stored:" + attr] += 1
        size = ent.t.shape[1] if form == "wpad" else ent.t.shape[0]
        if not _same(ent.t, fresh.get(form, size)):
            fails.append((name, "stored " + attr))
        if form in ("wpad", "wpadk"):
            for attr2, form2 in (("_sscg_wx3", "wx3"), ("_sscg_wtx3", "tx3")):
                ent2 = getattr(ent.t, attr2, None)
                if ent2 is not None and ent2.tag == F._wtag(ent.t):
                    seen["stored:%s.%s" % (attr, attr2)] += 1
                    if not _same(ent2.t, fresh.get(form + "." + form2, size)):
                        fails.append((name, "stored %s.%s" % (attr, attr2)))


def _check_split_getter(F, name, w, what, fresh3, fails):
    flat, plane = F.weight_split(w)
    n = w.numel()
    if not torch.equal(_bits(_planes(flat, plane, n)), _bits(fresh3).view(3, n)):
        fails.append((name, what))


def _check_getters(F, name, w, fresh, fails, seen):
    """What a convolution would be handed now, for every kind of copy a pass has asked for in the current mode."""
    ent = F._WT_USERS.get(id(w))
    for kind in sorted(ent[1]) if ent is not None else ():
        seen["getter:" + kind] += 1
        if kind == "w16":
            if not _same(F.weight_bf16(w), fresh.get("w16")):
                fails.append((name, "weight_bf16"))
        elif kind == "wx3":
            _check_split_getter(F, name, w, "weight_split", fresh.get("wx3"), fails)
        else:
            if not _same(F._cached_wt(w, _WT_DTYPE[kind]), fresh.get(kind)):
                fails.append((name, "_cached_wt " + kind))
    if F.get_conv_precision() != "f32s":
        return
    if getattr(w, "_sscg_wpad", None) is not None:          # a 21 / 20-channel stem: source channels padded
        cp = w._sscg_wpad.t.shape[1]
        wp = F._padded_weight(w, cp)
        seen["getter:wpad"] += 1
        if not _same(wp, fresh.get("wpad", cp)):
            fails.append((name, "_padded_weight"))
        _check_split_getter(F, name, wp, "weight_split(padded)", fresh.get("wpad.wx3", cp), fails)
        if not _same(F._cached_wt(wp, "x3"), fresh.get("wpad.tx3", cp)):
            fails.append((name, "_cached_wt(padded) tx3"))
    if getattr(w, "_sscg_wpadk", None) is not None:         # a 21 / 20-channel head: filters padded (conv2d_dgrad_param's own lines)
        kp = w._sscg_wpadk.t.shape[0]
        wp = F._cached_copy(w, "_sscg_wpadk", lambda: F._pad_filters(w.detach(), kp))
        seen["getter:wpadk"] += 1
        if not _same(wp, fresh.get("wpadk", kp)):
            fails.append((name, "padded filters"))
        if not _same(F._cached_wt(wp, "x3"), fresh.get("wpadk.tx3", kp)):
            fails.append((name, "_cached_wt(padded filters) tx3"))


def dgrad_operand_taken(F, w, xshape, stride, pad, dil):
    """The operand copy conv2d_dgrad_param hands to the data-gradient launch of weight w (an fp32 output gradient): the launch
    itself is replaced by a recorder."""
    k, _, r, _ = w.shape
    p, q = F.conv_out_size(xshape[2], r, stride, pad, dil), F.conv_out_size(xshape[3], r, stride, pad, dil)
    dy = F.empty_nhwc(xshape[0], k, p, q, w.device)
    F.fill_(dy, 0.0)
    taken = []
    real = F.conv2d_dgrad

    def recorder(dy_, wt, xs, *a, **kw):
        taken.append(wt)
        return F.empty_nhwc(xs[0], xs[1], xs[2], xs[3], dy_.device)
    F.conv2d_dgrad = recorder
    try:
        F.conv2d_dgrad_param(dy, w, tuple(xshape), tuple(w.shape), stride, pad, dil)
    finally:
        F.conv2d_dgrad = real
    assert len(taken) == 1
    return taken[0]


def assert_coherent(F, weights, getters=True, heads=()):
    """weights: {name: 4-D weight}.  Stored copies under a current tag, the optimisers' arena copies and (getters=True) whatever the
    getters hand out must equal fresh derivations bit for bit.  heads: (name, xshape, stride, pad, dil, form) - the operand
    conv2d_dgrad_param takes for that layer must be the fresh `form`.  Returns a counter of what was compared."""
    torch.cuda.synchronize()
    fails, seen = [], collections.Counter()
    opts = []
    for name, w in weights.items():
        assert w.dim() == 4
        fresh = _Fresh(F, w)
        _check_stored(F, name, w, fresh, fails, seen)
        if getters:
            _check_getters(F, name, w, fresh, fails, seen)
            _check_stored(F, name, w, fresh, fails, seen)         # ... and what the getters left behind for the next reader
            for hname, xshape, stride, pad, dil, form in heads:
                if hname == name:
                    seen["taken:" + form] += 1
                    if not _same(dgrad_operand_taken(F, w, xshape, stride, pad, dil), fresh.get(form)):
                        fails.append((name, "operand taken by conv2d_dgrad_param (%s)" % form))
        opt = _owner(w)
        if opt is not None and all(opt is not o for o in opts):
            opts.append(opt)
    for opt in opts:
        _check_arena(F, opt, fails, seen)
    torch.cuda.synchronize()
    if fails:
        raise Incoherent(fails)
    return seen


# ------------------------------------------------------------------------------------------ the fixture nets
class Rig:
    """Two small nets of arch.ops layers in which every kind of copy occurs.
    G (optim.FusedAdam): 7x7 21->64 stem (padded-stem path) -> 3x3 64->64 -> a FROZEN 3x3 64->64 (no optimiser) -> a 3x3 64->64
    under a stock torch.optim.Adam -> ConvTranspose2d 64->64 -> 3x3 64->21 head (padded-head data gradient) -> 1x1 21->5 (ragged
    channel counts: the exact fp32 kernels in every mode).  D (a second FusedAdam): 3x3 21->64 -> 3x3 64->64 -> 1x1 64->1.
    g_kw / d_kw: keyword options of the two FusedAdams (lr, weight_decay, decoupled, max_grad_norm, ema_decay).  inputs: a list of
    [2,21,16,16] CPU tensors the phases consume in order (two per step: G, then D) in place of draws from the rig's own generator -
    `replay(k)` points at the inputs of step k, so that a second rig can continue where a first one stopped."""

    def __init__(self, F, dev, seed=0, g_kw=None, d_kw=None, inputs=None):
        ops, optim = load_sub("arch.ops"), load_sub("optim")
        self.F, self.dev = F, dev
        torch.manual_seed(seed)
        mk = ops.Conv2d
        self.g = torch.nn.ModuleDict(dict(stem=mk(21, 64, 7, 1, 3), mid=mk(64, 64, 3, 1, 1, bias=False),
                                          up=ops.ConvTranspose2d(64, 64, 3, 2, 1, 1, bias=False), head=mk(64, 21, 3, 1, 1),
                                          ragged=mk(21, 5, 1, bias=False))).to(dev)
        self.frozen = mk(64, 64, 3, 1, 1, bias=False).to(dev)
        self.stock = mk(64, 64, 3, 1, 1, bias=False).to(dev)
        self.d = torch.nn.ModuleDict(dict(stem=mk(21, 64, 3, 1, 1), mid=mk(64, 64, 3, 1, 1, bias=False), head=mk(64, 1, 1))).to(dev)
        for m in (self.g["head"], self.g["ragged"], self.d["head"]):
            m.head = True                   # fp32 output in bf16 mode, as the networks' last convs
        self.frozen.weight.requires_grad_(False)
        self.g_opt = optim.FusedAdam(self.g.parameters(), **dict(dict(lr=2e-4), **(g_kw or {})))
        self.d_opt = optim.FusedAdam(self.d.parameters(), **dict(dict(lr=2e-4), **(d_kw or {})))
        self.s_opt = torch.optim.Adam(self.stock.parameters(), lr=2e-4, betas=(0.5, 0.999))
        self.gen = torch.Generator().manual_seed(seed + 1)
        self.inputs, self.next_input = inputs, 0
        self.steps = 0
        self.ptrs = []          # after every refresh: {(weight, attribute): data_ptr of the transposed copy}
        self.checks = collections.Counter()
        # (layer, input shape, stride, pad, dil, the form its data gradient must take in the split mode)
        self.heads = (("g.stem", (2, 21, 16, 16), 1, 3, 1, "wpad.tx3"), ("g.mid", (2, 64, 16, 16), 1, 1, 1, "tx3"),
                      ("g.head", (2, 64, 32, 32), 1, 1, 1, "wpadk.tx3"), ("g.ragged", (2, 21, 32, 32), 1, 0, 1, "t32"),
                      ("d.stem", (2, 21, 16, 16), 1, 1, 1, "wpad.tx3"), ("frozen", (2, 64, 16, 16), 1, 1, 1, "tx3"),
                      ("stock", (2, 64, 16, 16), 1, 1, 1, "tx3"))

    def g_weights(self):
        return {"g." + k: m.weight for k, m in self.g.items()}

    def d_weights(self):
        return {"d." + k: m.weight for k, m in self.d.items()}

    def weights(self):
        w = dict(self.g_weights(), **self.d_weights())
        w.update(frozen=self.frozen.weight, stock=self.stock.weight)
        return w

    def replay(self, step):
        """The next phases read the fixed inputs of step `step` (0-based) onwards."""
        self.next_input = 2 * step

    def _input(self):
        if self.inputs is not None:
            x, self.next_input = self.inputs[self.next_input], self.next_input + 1
        else:
            x = torch.randn(2, 21, 16, 16, generator=self.gen)
        x = x.to(self.dev).contiguous(memory_format=CL)
        return x.requires_grad_(True)       # (the stems' data gradients run too: Gis(fake_gt) in the real step)

    def check(self, getters=True, weights=None):
        F = self.F
        heads = self.heads if (getters and F.get_conv_precision() == "f32s") else ()
        seen = assert_coherent(F, self.weights() if weights is None else weights, getters, heads)
        self.checks.update(seen)
        return seen

    def refresh(self, check=True):
        """What model.py does before a pass reads the copies: the arena copies of the mode, then the transposed copies in the two
        forms the step uses (every registered user / the generators' weights only), in alternating order."""
        F = self.F
        self.g_opt.ensure_operand_copies()
        self.d_opt.ensure_operand_copies()
        gw = list(self.g_weights().values())
        if self.steps % 2 == 0:
            F.refresh_transposed_weights()
            F.refresh_transposed_weights(gw, all_users=False)
        else:
            F.refresh_transposed_weights(gw, all_users=False)
            F.refresh_transposed_weights()
        torch.cuda.synchronize()
        self.ptrs.append({(n, a): getattr(w, a).t.data_ptr() for n, w in self.weights().items() for a in F._WT_ATTR.values()
                          if getattr(w, a, None) is not None and getattr(w, a).tag == F._wtag(w)})
        if check:
            self.check()

    def g_phase(self):
        F, g = self.F, self.g
        self.g_opt.zero_grad()
        self.s_opt.zero_grad(set_to_none=True)
        h = self.stock(self.frozen(g["mid"](g["stem"](self._input()))))
        loss = F.mse_const(g["ragged"](g["head"](g["up"](h))), 1.0)
        F.backward(loss)
        F.SideStream.join(self.dev)
        self.g_opt.step()
        self.s_opt.step()

    def d_phase(self):
        F, d = self.F, self.d
        self.d_opt.zero_grad()
        loss = F.mse_const(d["head"](d["mid"](d["stem"](self._input()))), 0.0)
        F.backward(loss)
        F.SideStream.join(self.dev)
        self.d_opt.step()

    def step(self, check=True):
        """One training step, coherence checked where the copies are read (after the refresh, getters included) and where they
        were just invalidated (after the updates: stored copies and arena copies only - a getter would rebuild lazily and take the
        next refresh off the in-place path)."""
        self.refresh(check)
        before = {n: w.detach().clone() for n, w in self.weights().items()}
        self.g_phase()
        self.d_phase()
        self.steps += 1
        torch.cuda.synchronize()
        for n, w in self.weights().items():         # the step is a real one: every trained weight moved
            assert (n == "frozen") == torch.equal(before[n], w.detach()), n
        if check:
            self.check(getters=False)


def _covered(seen, *keys):
    missing = [k for k in keys if seen[k] == 0]
    assert not missing, "the scenario never compared %s (compared: %s)" % (missing, dict(seen))


# ------------------------------------------------------------------------------------------ 3. scenarios
_MODE_COVER = {
    "f32s": ("stored:arena_x3", "stored:_sscg_wtx3", "stored:_sscg_wt", "stored:_sscg_wx3", "stored:_sscg_wpad", "stored:_sscg_wpadk",
             "stored:_sscg_wpad._sscg_wx3", "stored:_sscg_wpad._sscg_wtx3", "stored:_sscg_wpadk._sscg_wtx3",
             "getter:wx3", "getter:tx3", "getter:t32", "getter:wpad", "getter:wpadk", "taken:wpad.tx3", "taken:wpadk.tx3", "taken:tx3",
             "stale-tag:_sscg_wtx3", "stale-tag:_sscg_wpad"),
    "bf16": ("stored:arena16", "stored:_sscg_wt16", "stored:_sscg_wt", "stored:_sscg_w16", "getter:w16", "getter:t16", "getter:t32",
             "stale-tag:_sscg_wt16"),
    "f32x": ("stored:_sscg_wt", "getter:t32", "stale-tag:_sscg_wt"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [True, False], ids=["batch_transposes", "per_weight_transposes"])
@pytest.mark.parametrize("mode", ["f32s", "bf16", "f32x"])
def test_three_steps_keep_every_copy_coherent(F, dev, mode, batch):
    """Scenario 1.  The second refresh rebuilds the lazily built copies of the first step; from then on `_transpose_batch` rewrites
    them in place from its cached job table: the pointers must not change any more (so the test is known to be on that path)."""
    with _mode(F, mode, batch):
        rig = Rig(F, dev)
        for _ in range(3):
            rig.step()
        rig.refresh()
        _covered(rig.checks, *_MODE_COVER[mode])
        if batch:
            base = rig.ptrs[1]
            assert len(base) >= 6, base
            for later in rig.ptrs[2:]:
                assert {k: later.get(k) for k in base} == base


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32s", "bf16"])
def test_torch_writes_between_steps(F, dev, mode):
    """Scenario 2: p.copy_() under no_grad, net.load_state_dict, opt.load_state_dict followed by a step."""
    with _mode(F, mode):
        rig = Rig(F, dev)
        sd_g = {k: v.detach().clone() for k, v in rig.g.state_dict().items()}
        sd_d = {k: v.detach().clone() for k, v in rig.d.state_dict().items()}
        rig.step()
        osd = rig.g_opt.state_dict()
        osd = {"state": {k: {a: (b.detach().clone() if torch.is_tensor(b) else b) for a, b in st.items()} for k, st in osd["state"].items()},
               "param_groups": osd["param_groups"]}
        with torch.no_grad():
            for w in (rig.g["mid"].weight, rig.g["stem"].weight, rig.g["head"].weight, rig.d["mid"].weight, rig.frozen.weight):
                w.copy_(w * 1.5 + 0.01)
        seen = rig.check(getters=False)         # the slices torch wrote are recorded as behind, their cached copies carry old tags
        _covered(seen, "behind:arena_x3" if mode == "f32s" else "behind:arena16")
        rig.check()                             # ... and a getter re-derives them on use
        rig.step()
        rig.g.load_state_dict(sd_g, strict=True)
        rig.d.load_state_dict(sd_d, strict=True)
        rig.check(getters=False)
        rig.check()
        rig.step()
        rig.g_opt.load_state_dict(osd)
        rig.check()
        rig.step()
        rig.refresh()


@pytest.mark.gpu
@pytest.mark.parametrize("other", ["bf16", "f32x"])
def test_mode_changes_between_steps(F, dev, other):
    """Scenario 3: f32s -> other -> f32s, a step in each.  The arena copy step() drops for the inactive mode comes back rebuilt from
    the current arena; no copy made for the earlier mode is served with old data under a current tag."""
    try:
        F.set_conv_precision("f32s")
        rig = Rig(F, dev)
        rig.step()
        rig.refresh()
        assert rig.g_opt.arena_x3 is not None
        F.set_conv_precision(other)
        rig.step()
        assert rig.g_opt.arena_x3 is None and rig.d_opt.arena_x3 is None        # dropped by step(), not left to go stale
        assert (rig.g_opt.arena16 is not None) == (other == "bf16")
        rig.refresh()
        F.set_conv_precision("f32s")
        rig.refresh()
        assert rig.g_opt.arena_x3 is not None
        rig.step()
        assert rig.g_opt.arena16 is None and rig.d_opt.arena16 is None
        rig.refresh()
        _covered(rig.checks, *_MODE_COVER["f32s"])
    finally:
        F.set_conv_precision("f32")


def _entries(F, weights):
    """Every cached copy object of `weights`, second level included: {(weight, attr[, attr2]): (object, data_ptr, current?)}."""
    out = {}
    for n, w in weights.items():
        for attr in _STORED:
            ent = getattr(w, attr, None)
            if ent is None:
                continue
            out[(n, attr)] = (ent, ent.t.data_ptr(), ent.tag == F._wtag(w))
            if attr in ("_sscg_wpad", "_sscg_wpadk"):
                for attr2 in ("_sscg_wx3", "_sscg_wtx3"):
                    e2 = getattr(ent.t, attr2, None)
                    if e2 is not None:
                        out[(n, attr, attr2)] = (e2, e2.t.data_ptr(), ent.tag == F._wtag(w) and e2.tag == F._wtag(ent.t))
    return out


@contextlib.contextmanager
def _count_transposes(F):
    """Rows rebuilt by the two transpose entry points while the block runs."""
    lib, count = F.lib, [0]
    one, many = lib.sscg_weight_krsc_to_crsk, lib.sscg_weight_krsc_to_crsk_batch

    def one_(*a):
        count[0] += 1
        return one(*a)

    def many_(table, rows, blocks, stream):
        count[0] += rows
        return many(table, rows, blocks, stream)
    lib.sscg_weight_krsc_to_crsk, lib.sscg_weight_krsc_to_crsk_batch = one_, many_
    try:
        yield count
    finally:
        lib.sscg_weight_krsc_to_crsk, lib.sscg_weight_krsc_to_crsk_batch = one, many


@pytest.mark.gpu
def test_an_update_invalidates_its_own_optimisers_copies_only(F, dev):
    """Scenario 4.  The second optimiser's update leaves the first one's copies untouched AND valid (same objects, same pointers,
    current tags, no transpose launched for them); the first one's update invalidates all of its own - the padded weights and the
    copies cached on them included - and none of the second's."""
    with _mode(F, "f32s", True):
        rig = Rig(F, dev)
        rig.step()
        rig.step()
        rig.refresh()
        gw, dw = rig.g_weights(), rig.d_weights()
        others = {"frozen": rig.frozen.weight, "stock": rig.stock.weight}
        g0, d0, o0 = _entries(F, gw), _entries(F, dw), _entries(F, others)
        assert all(cur for _, _, cur in list(g0.values()) + list(d0.values()) + list(o0.values()))
        assert ("g.stem", "_sscg_wpad", "_sscg_wtx3") in g0 and ("g.head", "_sscg_wpadk", "_sscg_wtx3") in g0
        # ---- the discriminator's update
        rig.d_phase()
        torch.cuda.synchronize()
        for before, weights in ((g0, gw), (o0, others)):
            now = _entries(F, weights)
            assert now.keys() == before.keys()
            for k, (ent, ptr, _) in before.items():
                assert now[k][0] is ent and now[k][1] == ptr and now[k][2], k
        seen = assert_coherent(F, gw, getters=False)
        _covered(seen, "stored:_sscg_wtx3", "stored:_sscg_wpad", "stored:_sscg_wpadk", "stored:_sscg_wpad._sscg_wtx3", "stored:arena_x3")
        d1 = _entries(F, dw)
        assert not any(cur for _, _, cur in d1.values())
        stale_transposed = [k for k in d1 if len(k) == 2 and k[1] in F._WT_ATTR.values()]
        assert len(stale_transposed) >= 2
        with _count_transposes(F) as count:
            F.refresh_transposed_weights()
        assert count[0] == len(stale_transposed), (count[0], stale_transposed)      # the generators' copies were not rebuilt
        now = _entries(F, gw)
        assert all(now[k][0] is ent and now[k][1] == ptr for k, (ent, ptr, _) in g0.items())
        rig.check()
        # ---- the generators' update
        d2 = _entries(F, dw)
        rig.g_phase()
        torch.cuda.synchronize()
        assert not any(cur for _, _, cur in _entries(F, gw).values())
        now = _entries(F, dw)
        assert all(now[k][0] is ent and now[k][1] == ptr and now[k][2] for k, (ent, ptr, _) in d2.items())
        old_pad, old_padk = g0[("g.stem", "_sscg_wpad")][0].t, g0[("g.head", "_sscg_wpadk")][0].t
        rig.check()                                 # the getters rebuild: new padded tensors, new second-level copies
        assert rig.g["stem"].weight._sscg_wpad.t is not old_pad and rig.g["head"].weight._sscg_wpadk.t is not old_padk
        assert rig.g["stem"].weight._sscg_wpad.t._sscg_wtx3 is not g0[("g.stem", "_sscg_wpad", "_sscg_wtx3")][0]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32s", "bf16"])
def test_raw_arena_write_then_refresh_operand_copies(F, dev, mode):
    """Scenario 5: what DataParallel.attach() does after broadcast_flat - the arena is rewritten through a raw view (no `_version`
    moves), then parallel._refresh_operand_copies(opt) - with transposed and padded copies already built (a model that ran a pass
    before it was attached).  The broadcast is emulated by an in-place scale of opt.arena: no process group needed.
    (This pins the epoch bump in `_refresh_operand_copies`: without it every transposed and padded copy keeps a current tag and the
    weights from before the broadcast.)"""
    parallel = load_sub("parallel")
    with _mode(F, mode):
        rig = Rig(F, dev)
        rig.step()
        rig.refresh()
        before = {n: w.detach().clone() for n, w in rig.weights().items()}
        for opt in (rig.g_opt, rig.d_opt):
            opt.arena.mul_(1.0 + 2.0 ** -6)
            parallel._refresh_operand_copies(opt)
        torch.cuda.synchronize()
        assert all((n in ("frozen", "stock")) == torch.equal(before[n], w.detach()) for n, w in rig.weights().items())
        rig.check(getters=False)
        rig.check()
        rig.step()
        rig.refresh()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32s", "bf16"])
def test_weights_no_arena_owns(F, dev, mode):
    """Scenario 6: the weight under a stock torch.optim.Adam and the frozen weight are invalidated by `_version`; a raw write (no
    version moves) is announced with bump_weight_epoch() - no cell -, which must not touch the arena optimisers' copies."""
    with _mode(F, mode):
        rig = Rig(F, dev)
        rig.step()
        rig.refresh()
        own = {"frozen": rig.frozen.weight, "stock": rig.stock.weight}
        plain = "_sscg_wx3" if mode == "f32s" else "_sscg_w16"
        trans = "_sscg_wtx3" if mode == "f32s" else "_sscg_wt16"
        e0 = _entries(F, own)
        assert all(e0[(n, a)][2] for n in own for a in (plain, trans))
        with torch.no_grad():
            rig.frozen.weight.mul_(1.5)             # torch writes: a new version
        e1 = _entries(F, own)
        assert not any(e1[("frozen", a)][2] for a in (plain, trans)) and all(e1[("stock", a)][2] for a in (plain, trans))
        rig.check(getters=False)
        ver = rig.stock.weight._version
        rig.g_phase()                               # the pass re-derives the frozen weight's copies; then the stock optimiser's
        assert rig.stock.weight._version > ver      # update: a new version, too
        torch.cuda.synchronize()
        e1 = _entries(F, own)
        assert all(e1[("frozen", a)][2] for a in (plain, trans)) and not any(e1[("stock", a)][2] for a in (plain, trans))
        seen = rig.check(getters=False)
        _covered(seen, "stored:" + plain, "stored:" + trans, "stale-tag:" + plain, "stale-tag:" + trans)
        rig.check()
        rig.refresh()
        # a raw write
        g0 = _entries(F, dict(rig.g_weights(), **rig.d_weights()))
        for w in own.values():
            v = w._version
            w.data.mul_(0.75)
            assert w._version == v
        F.bump_weight_epoch()
        e2 = _entries(F, own)
        assert not any(e2[(n, a)][2] for n in own for a in (plain, trans))
        now = _entries(F, dict(rig.g_weights(), **rig.d_weights()))
        for k, (ent, ptr, cur) in g0.items():
            if len(k) == 2:                         # (the copies ON a padded tensor follow the global epoch: rebuilt, from the same data)
                assert now[k][0] is ent and now[k][1] == ptr and now[k][2] == cur, k
        rig.check(getters=False)
        rig.check()
        rig.step()
        rig.refresh()


@pytest.mark.gpu
def test_shipped_step_keeps_every_copy_coherent(F, dev):
    """Scenario 7: semisuper_cycleGAN at 64x64 (built as tests/test_nets_gpu.py::_make_model builds it, keyed weights `s64`), two
    m.step() calls in the split mode - the shipped call order, lanes and events included - then every 4-D parameter of the four
    trained nets (and of the frozen ones) after each."""
    import numpy as np
    from oracle import fixtures as FX
    with _mode(F, "f32s"):
        C, dataset, H, Wd, B, _ = FX.STEP_CONFIGS["s64"]
        md = load_sub("model")
        args = FX.make_args(dataset=dataset, crop_height=H, crop_width=Wd, batch_size=B, gpu_ids=[dev.index or 0],
                            checkpoint_dir="/tmp/sscg_test_ckpt_none", as_written=True)
        m = _quiet(md.semisuper_cycleGAN, args)
        for k, sd in FX.semisup_state_dicts(C, torch.float32, "s64").items():
            getattr(m, k).load_state_dict(sd, strict=True)
        nets = [k for k in ("Gis", "Gsi", "Di", "Ds", "old_Gis", "old_Gsi", "old_Di") if hasattr(m, k)]
        assert nets[:4] == ["Gis", "Gsi", "Di", "Ds"]
        weights = {"%s.%s" % (k, n): p for k in nets for n, p in getattr(m, k).named_parameters() if p.dim() == 4}
        np.random.seed(0)
        total = collections.Counter()
        for s in range(2):
            l_img, l_gt, unl_img = FX.step_batch("s64", s, C, H, Wd, B)
            m.step(l_img.to(dev), l_gt.to(dev), unl_img.to(dev))
            m.sync_losses()
            F.flush_side_work()
            torch.cuda.synchronize()
            total.update(assert_coherent(F, weights, getters=False))
            total.update(assert_coherent(F, weights))
        _covered(total, "stored:arena_x3", "stored:_sscg_wtx3", "stored:_sscg_wx3", "stored:_sscg_wpad", "getter:wx3", "getter:tx3",
                 "getter:wpad", "stale-tag:_sscg_wtx3")
        assert total["stored:_sscg_wtx3"] > 50         # the generators' copies, rebuilt beside the discriminator step


# ------------------------------------------------------------------------------------------ 4. the checker can fail
@pytest.mark.gpu
def test_checker_sees_a_missing_epoch_bump(F, dev):
    """Negative control: one update whose bump_weight_epoch is lost leaves the transposed (and padded) copies with a current tag and
    the previous weights - assert_coherent must raise on them."""
    with _mode(F, "f32s"):
        rig = Rig(F, dev)
        rig.step()
        rig.refresh()
        real = F.bump_weight_epoch
        F.bump_weight_epoch = lambda cell=None: None
        try:
            rig.g_phase()
        finally:
            F.bump_weight_epoch = real
        with pytest.raises(Incoherent) as e:
            assert_coherent(F, rig.g_weights(), getters=False)
        forms = e.value.forms()
        assert "stored _sscg_wtx3" in forms and "stored _sscg_wpad" in forms and "stored _sscg_wpadk" in forms, forms
        assert "stored arena_x3" not in forms               # (the Adam kernel rewrote the planes itself)
        with pytest.raises(Incoherent) as e:
            assert_coherent(F, rig.g_weights(), getters=True)
        assert "_cached_wt tx3" in e.value.forms()
        assert_coherent(F, rig.d_weights())                 # the other optimiser's copies are what they should be


@pytest.mark.gpu
def test_checker_sees_planes_the_adam_kernel_did_not_write(F, dev):
    """Negative control: adam_step called with both shadows None while arena_x3 exists leaves the split planes one update old."""
    with _mode(F, "f32s"):
        rig = Rig(F, dev)
        rig.step()
        rig.refresh()
        real = F.adam_step

        def no_shadow(*a, **kw):
            kw["shadow_bf16"] = kw["shadow_split"] = None
            return real(*a, **kw)
        F.adam_step = no_shadow
        try:
            rig.g_phase()
        finally:
            F.adam_step = real
        assert rig.g_opt.arena_x3 is not None
        with pytest.raises(Incoherent) as e:
            assert_coherent(F, rig.g_weights(), getters=False)
        assert e.value.forms() == {"stored arena_x3"}, e.value.forms()
        with pytest.raises(Incoherent) as e:
            assert_coherent(F, rig.g_weights(), getters=True)
        assert "weight_split" in e.value.forms()
