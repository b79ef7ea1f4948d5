"""The convolution and normalisation entries stay inside their outputs, records and workspaces.

The wrappers of functional.py hand the kernels outputs from torch.empty and a workspace that is 1.25x the largest request so far, and
they report that oversized figure as `ws_bytes`: a store past a ragged last tile, or past the bytes a *_workspace() query promised,
lands in slack or in a neighbouring allocation, and the fp64 comparisons of the other files look inside the tensor only.  Here every
device tensor the wrappers allocate while `_Guarded` is active (torch.empty, torch.empty_like, functional.empty_nhwc, functional._WS.get)
is a 256-byte aligned view into a larger buffer of 0xFF bytes - a NaN in fp32, bf16 and fp64 - with at least max(64 KiB, size of the
view) of guard on either side, and a workspace view has exactly the size the wrapper asked for, max(nbytes, 16): the entries' own
SSCG_ERR_WORKSPACE check sees the size the query promised.  The operands sit between NaN guards too: a read past one that reaches a result
is a NaN in the comparison.

Every call is checked four ways (`_Run`):
  1. every guard of every allocation still holds its sentinel (first / last damaged byte relative to the view are reported);
  2. no element of a result is still the sentinel;
  3. the result agrees with fp64 within the bound the suite already uses for that kernel (named beside each constant below);
  4. the results are torch.equal across three runs: exact workspace pre-filled with 0xFF, exact workspace pre-filled with 0x00, the
     product's own oversized workspace - they depend neither on stale scratch nor on slack.

Cases, kernel families and the regime each case reaches: tests/test_conv_extents_host.py (which asserts those regimes from the size
queries).  Each case runs under tuning 0, every forced tile class of the family and forced split 3.  Where a family does not serve an
entry the entry is dropped for it and the printed line says so: bf16 tensors need 64-channel multiples on the operand side
(functional._fwd_operands / conv2d_dgrad_param: stems and heads run on fp32 tensors in that mode, covered under f32x); the masked store
of the backward sums is fp32 ReLU only; a forced tile class the exact family has no instance of for ragged channels answers
SSCG_ERR_UNSUPPORTED before any launch.  Inputs are the saw-tooth-plus-noise tables of test_pointwise_regimes_gpu._table (every element
distinguishable).  Forward activations are continuous, so their pre-activations need no margin; where a ReLU / LeakyReLU MASK is formed
(backward sums, norm backward) the pre-activations are kept 1e-4 away from zero the way test_norm_regimes_gpu does it.
Figures are printed before they are asserted (`conv_extents ...`, shown by pytest -s; profiles/conv_extents.txt)."""
import contextlib
import functools
import math

import pytest
import torch
import torch.nn.functional as TF

from conftest import load_sub
import test_conv_extents_host as H
import test_norm_regimes_gpu as NR
from test_pointwise_regimes_gpu import _table

pytestmark = pytest.mark.gpu
CL = torch.channels_last
F32, BF, F64 = torch.float32, torch.bfloat16, torch.float64
EPS16 = 2.0 ** -8           # one bf16 rounding, against the tensor's max (test_conv_bf16_tensors)
TOL_FWD = 2e-5              # forward / data gradient, fp32 results (test_conv_fwd_bwd, test_conv_bf16_tensors)
TOL_WGRAD = {"f32x": 5e-5, "f32s": 5e-5, "bf16": 2e-5, "bf16c": 5e-5}     # test_conv_fwd_bwd; test_conv_bf16_tensors (bf16-rounded operands)
TOL_WACC = 2e-4             # accumulating weight gradient (test_conv_bf16_tensors)
TOL_STATS = {"f32x": 2e-5, "f32s": 2e-5, "bf16": 1e-4, "bf16c": 1e-4}    # of scale (test_norm_statistics_fused_into_the_conv_epilogue)
TOL_SUMS = 1e-5             # fused backward sums against the reduction-pass route (test_norm_backward_sums_fused_into_the_data_gradient)
TOL_HEAD = 3e-5             # norm head (test_fused_pixel_discriminator_tail)
SLOPE = 0.2
EPS = 1e-5
MARGIN = 1e-4               # distance of a mask's pre-activation from zero (test_norm_regimes_gpu.GUARD)
MIN_GUARD = 64 * 1024
ALIGN = 256


# ----------------------------------------------------------------------------------------------------------------- the guard
class _Guarded:
    """Context manager: see the module docstring.  ws = "ff" / "00": exact workspace views pre-filled with that byte; "own": the
    product's own _Workspace (its buffer is still carved from a guarded allocation when it grows)."""

    def __init__(self, F, ws="ff", shrink_ws=0):
        self.F, self.ws, self.shrink_ws = F, ws, shrink_ws
        self.allocs = []        # (buffer, offset of the view, bytes of the view, label)

    def carve(self, shape, stride, dtype, device, label, fill=None):
        esz = self._empty((), dtype=dtype).element_size()
        numel = math.prod(shape)
        n_el = 0 if numel == 0 else 1 + sum((s - 1) * st for s, st in zip(shape, stride))
        nbytes = n_el * esz
        g = -(-max(MIN_GUARD, nbytes) // ALIGN) * ALIGN
        buf = self._empty(g + nbytes + g + ALIGN, dtype=torch.uint8, device=device)
        buf.fill_(0xFF)
        off = g + (-(buf.data_ptr() + g)) % ALIGN
        view = buf[off:off + nbytes]
        if fill is not None:
            view.fill_(fill)
        self.allocs.append((buf, off, nbytes, "%s %s %s" % (label, tuple(shape), str(dtype).replace("torch.", ""))))
        t = view.view(dtype).as_strided(tuple(shape), tuple(stride))
        assert t.data_ptr() % ALIGN == 0
        return t

    def _on_device(self, dv):
        return dv is not None and torch.device(dv).type == "cuda"

    def __enter__(self):
        self._empty, self._like, self._ws = torch.empty, torch.empty_like, self.F._WS
        guard = self

        def empty(*a, **k):
            if not guard._on_device(k.get("device")):
                return guard._empty(*a, **k)
            m = guard._empty(*a, **dict(k, device="meta"))
            return guard.carve(m.shape, m.stride(), m.dtype, k["device"], "empty")

        def empty_like(x, **k):
            if not guard._on_device(x.device) or "device" in k:
                return guard._like(x, **k)
            m = guard._like(torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device="meta"), **k)
            return guard.carve(m.shape, m.stride(), m.dtype, x.device, "empty_like")

        class ExactWorkspace:
            def get(self, nbytes, device):
                nbytes = max(int(nbytes), 16) - guard.shrink_ws
                return guard.carve((nbytes,), (1,), torch.uint8, device, "workspace", fill=0xFF if guard.ws == "ff" else 0x00)

        torch.empty, torch.empty_like = empty, empty_like
        if self.ws != "own":
            self.F._WS = ExactWorkspace()
        return self

    def __exit__(self, *exc):
        torch.empty, torch.empty_like, self.F._WS = self._empty, self._like, self._ws
        return False

    def put(self, t, dtype=F32):
        """CPU tensor (NCHW shaped: channels-last memory) -> guarded device tensor of dtype holding its values"""
        assert torch.empty is not self._empty, "inside the context only"
        dev = torch.device("cuda:0")
        if t.dim() == 4:
            d = torch.empty(tuple(t.shape), dtype=dtype, device=dev, memory_format=CL)
        else:
            d = torch.empty(tuple(t.shape), dtype=dtype, device=dev)
        d.copy_(t.to(dtype))
        return d

    def damage(self):
        """[] when every guard holds its sentinel, else one line per damaged allocation"""
        torch.cuda.synchronize()
        if not self.allocs:
            return []
        flags = torch.stack([(b[:off] != 0xFF).any() | (b[off + n:] != 0xFF).any() for b, off, n, _ in self.allocs]).cpu()
        out = []
        for hit, (b, off, n, label) in zip(flags.tolist(), self.allocs):
            if hit:
                bad = (b != 0xFF)
                bad[off:off + n] = False
                idx = bad.nonzero().flatten()
                out.append("%s (%d bytes): %d guard bytes damaged, first at %+d, last at %+d relative to the view" % (
                    label, n, idx.numel(), int(idx[0]) - off, int(idx[-1]) - off))
        return out


class _Run:
    """One (case, family, tuning) of one test: collects figures, prints them, asserts at the end."""

    def __init__(self, label):
        self.label, self.bad, self.lines = label, [], []

    def say(self, text):
        if text not in self.lines:      # (a call runs three times: its remarks are printed once)
            self.lines.append(text)
            print("conv_extents %s %s" % (self.label, text))

    def add(self, name, err, bound):
        self.say("%s err %.3e bound %.3e" % (name, err, bound))
        if not err < bound:         # (a NaN fails)
            self.bad.append((name, err, bound))

    def true(self, name, ok, detail=""):
        if not ok:
            self.say("%s FAILED %s" % (name, detail))
            self.bad.append((name, detail))

    def check(self):
        assert not self.bad, (self.label, self.bad)


def _rel(got, ref):
    """max |got - ref| / max |ref| (test_kernels_gpu.rel_err)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got.reshape(ref.shape) - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _three_runs(F, run, call, refs, shrink_ws=0):
    """call(g) -> {name: device tensor}, run under the three workspace regimes; refs: {name: (fp64 reference, bound)} or
    {name: (None, None)} for results that are compared between the runs only.  Returns the first run's results."""
    outs = {}
    for ws in ("ff", "00", "own"):
        with _Guarded(F, ws, shrink_ws) as g:
            res = call(g)
            dmg = g.damage()
        run.true("guards[%s]" % ws, not dmg, "; ".join(dmg))
        outs[ws] = res
    first = outs["ff"]
    for name, t in first.items():
        if t is None:
            continue
        if t.is_floating_point():
            run.true("written:" + name, not bool(torch.isnan(t).any()), "%d elements still hold the sentinel" % int(torch.isnan(t).sum()))
        for ws in ("00", "own"):
            run.true("equal[%s]:%s" % (ws, name), torch.equal(t, outs[ws][name]), "differs from the 0xFF-workspace run")
        ref, bound = refs.get(name, (None, None))
        if ref is not None:
            if callable(bound):
                bound(run, name, t, ref)
            else:
                run.add(name, _rel(t, ref), bound)
    run.say("guards ok: %s" % ("yes" if not any(b[0].startswith("guards") for b in run.bad) else "NO"))
    return first


@contextlib.contextmanager
def _mode(F, fam, **tuning):
    F.set_conv_precision(fam)
    old = F.tuning(**tuning)
    try:
        yield
    finally:
        F.TUNING[0], F.WGRAD_TUNING[0] = old
        F.set_conv_precision("f32")


def _tunings(fam, K=64, thin=False):
    """(label, functional.tuning arguments): the library's plan, every forced tile class of the family, forced split 3 (the thin 1x1
    kernels of conv_thin.hip have no tile classes and take no workspace: the plan alone)"""
    if thin:
        return [("plan", {})]
    classes = list(H.TILE_CLASSES[fam])
    if fam == "f32x" and K <= 4:
        classes.append(8)
    return [("plan", {})] + [("class%d" % c, dict(tile_class=c)) for c in classes] + [("split3", dict(split=3))]


def _unsupported(F, fn):
    """fn(), or None when the library answers SSCG_ERR_UNSUPPORTED (before any launch: a forced class the family has no instance of)"""
    try:
        return fn()
    except F._lib.SscgError as e:
        if "SSCG_ERR_UNSUPPORTED" in str(e):
            return None
        raise


# ----------------------------------------------------------------------------------------------------------------- inputs, references
def _rnd(t, fam):
    return t.to(BF).float() if fam in ("bf16", "bf16c") else t


@functools.lru_cache(maxsize=None)
def _case(cid, rounded, reflect=False):
    """inputs (fp32 CPU tensors holding the operand values) and fp64 results of one case, computed once: pre = conv + bias, dx, dw"""
    N, Hh, W, Cin, K, R, s, p, d = H.CASES[cid]["shape"]
    seed = 1000 + 10 * list(H.CASES).index(cid)
    fam = "bf16" if rounded else "f32x"
    x = _rnd(_table((N, Cin, Hh, W), seed), fam)
    w = _rnd(_table((K, Cin, R, R), seed + 1, lo=-1.0, hi=1.0, noise=0.1, period=257) / (Cin * R * R) ** 0.5, fam)
    b = _table((K,), seed + 2, lo=-0.5, hi=0.5, noise=0.1, period=7)
    _, _, P, Q = H.geometry(H.CASES[cid]["shape"])
    gy = _rnd(_table((N, K, P, Q), seed + 3, lo=-1.0, hi=1.0, noise=0.25, period=4093), fam)
    xr, wr = x.double().requires_grad_(not reflect), w.double().requires_grad_(True)
    xin = TF.pad(xr, (p, p, p, p), mode="reflect") if reflect else xr
    conv = TF.conv2d(xin, wr, None, s, 0 if reflect else p, d)
    conv.backward(gy.double())
    conv = conv.detach()
    return dict(x=x, w=w, b=b, gy=gy, conv=conv, pre=conv + b.double().view(1, K, 1, 1), dx=None if reflect else xr.grad, dw=wr.grad,
                shape=H.CASES[cid]["shape"], P=P, Q=Q)


def _act64(z, act):
    if act == 1:
        return z.clamp_min(0)
    if act == 2:
        return torch.where(z > 0, z, z * float(torch.tensor(SLOPE, dtype=F32)))
    if act == 3:
        return torch.tanh(z)
    return z


def _tdt(fam):
    return BF if fam == "bf16" else F32


def _tol(fam, dtype):
    return EPS16 if dtype == BF else TOL_FWD


def _fams(cid):
    return list(H.FAMILIES) + (["bf16c"] if cid == H.BF16C_CASE else [])


def _case_fams(entry=None):
    out = []
    for cid in H.CASE_IDS:
        for fam in _fams(cid):
            Cin, K = H.CASES[cid]["shape"][3], H.CASES[cid]["shape"][4]
            if fam == "bf16" and ((entry in ("fwd", "wgrad") and Cin % 64) or (entry in ("dgrad", "wgrad") and K % 64)):
                continue        # bf16 tensors need 64-channel multiples on the operand side: dropped for the family
            out.append(pytest.param(cid, fam, id="%s-%s" % (cid, fam)))
    return out


# ----------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("cid,fam", _case_fams("fwd"))
def test_forward_entries_stay_inside_their_outputs_records_and_workspace(cid, fam, F, dev):
    """conv2d_fwd (bias x act none / ReLU / LeakyReLU; tanh and reflection padding on the stem / head cases), conv2d_fwd_norm (the fused
    statistics, G = 1 and G = N) and conv_bn_eval_act (the eval fold, on the cases sscg_conv2d_fwd_affine_applies accepts)."""
    case = H.CASES[cid]
    N, Hh, W, Cin, K, R, s, p, d = case["shape"]
    c = _case(cid, fam in ("bf16", "bf16c"))
    dt = _tdt(fam)
    small = cid in ("head3", "stem3", "stem20", "stem21")
    cr = _case(cid, fam in ("bf16", "bf16c"), True) if small else None
    M, L1 = N * c["P"] * c["Q"], c["P"] * c["Q"]
    fold = cid in H.AFFINE_CASES and fam in ("f32s", "bf16")
    ch = torch.arange(K, dtype=F32)
    rm0, rv0 = 0.1 * (ch % 9) - 0.45, 0.5 + 0.125 * (ch % 6)
    gamma, beta = NR._affine(K)
    res = _rnd(_table((N, K, c["P"], c["Q"]), 77, lo=-1.0, hi=1.0, noise=0.1), fam)
    failures = []
    for tname, tkw in _tunings(fam, K, case.get("thin")):
        run = _Run("fwd %s %s %s" % (cid, fam, tname))
        refs = {}

        def call(g):
            x, w, b = g.put(c["x"], dt), g.put(c["w"]), g.put(c["b"])
            out = {}
            for bias in (0, 1):
                for act in (0, 1, 2) + ((3,) if small else ()):
                    name = "y_bias%d_act%d" % (bias, act)
                    y = _unsupported(F, lambda: F.conv2d_fwd(x, w, b if bias else None, s, p, d, F.PAD_ZEROS, act, SLOPE, out_f32=False))
                    out[name] = y
                    if y is None:
                        run.say("forced class: SSCG_ERR_UNSUPPORTED before any launch")
                    else:
                        refs[name] = (_act64(c["pre"] if bias else c["conv"], act), _tol(fam, y.dtype))
            if small:
                y = _unsupported(F, lambda: F.conv2d_fwd(x, w, b, s, p, d, F.PAD_REFLECT, 3 if K <= 4 else 0, SLOPE, out_f32=False))
                out["y_reflect"] = y
                refs["y_reflect"] = (_act64(cr["pre"], 3 if K <= 4 else 0), _tol(fam, dt))
            if fam == "bf16":
                out["y_f32out"] = F.conv2d_fwd(x, w, b, s, p, d, out_f32=True)
                refs["y_f32out"] = (c["pre"], TOL_FWD)
            for G in (1, N):
                L = M // G
                rm, rv = (g.put(rm0), g.put(rv0)) if G == 1 else (None, None)
                r3 = _unsupported(F, lambda: F.conv2d_fwd_norm(x, w, b, s, p, d, F.PAD_ZEROS, False, (G, L, K), EPS, rm, rv, 0.1))
                if r3 is None or r3[1] is None:
                    run.say("fused statistics G=%d: not fused for this plan" % G)
                    continue
                y, mean, rstd = r3
                yv = c["pre"].view(G, N // G, K, L1)
                mu = yv.mean((1, 3))
                var = ((yv - mu.view(G, 1, K, 1)) ** 2).mean((1, 3))
                scale = float(mu.abs().max() + var.sqrt().max())
                out.update({"stats%d_y" % G: y, "stats%d_mean" % G: mean, "stats%d_rstd" % G: rstd})
                refs["stats%d_y" % G] = (c["pre"], _tol(fam, y.dtype))
                refs["stats%d_mean" % G] = (mu, lambda r, n, t, ref, sc=scale: r.add(n, float((t.double().cpu() - ref).abs().max()) / sc, TOL_STATS[fam]))
                refs["stats%d_rstd" % G] = (1.0 / torch.sqrt(var + EPS), TOL_STATS[fam])
                if G == 1:
                    out.update(running_mean=rm, running_var=rv)
                    refs["running_mean"] = (0.9 * rm0.double() + 0.1 * mu[0], TOL_STATS[fam])
                    refs["running_var"] = (0.9 * rv0.double() + 0.1 * var[0] * L / (L - 1), TOL_STATS[fam])
            if fold:
                a = [g.put(rm0), g.put(rv0), g.put(gamma), g.put(beta)]
                r = g.put(res, dt)
                with torch.no_grad():
                    if F.conv_bn_eval_applies(x, w, s, p, d, F.PAD_ZEROS, F.ACT_RELU, 0.0, False):
                        out["fold"] = F.conv_bn_eval_act(x, w, b, a[0], a[1], a[2], a[3], r, s, p, d, F.PAD_ZEROS, EPS, F.ACT_RELU, 0.0, False)
                        y0 = F.conv2d_fwd(x, w, b, s, p, d, F.PAD_ZEROS, 0, 0.0, out_f32=False)
                        out["fold_separate"] = F.batch_norm_act(y0, a[2], a[3], a[0], a[1], False, 0.1, EPS, F.ACT_RELU, 0.0, r)
                    else:
                        run.say("eval fold: not served under this tuning")
            return out

        with _mode(F, fam, **tkw):
            first = _three_runs(F, run, call, refs)
        if "fold" in first:     # bit for bit the three separate launches (include/sscg.h, sscg_conv2d_fwd_affine)
            run.true("fold == separate passes", torch.equal(first["fold"], first["fold_separate"]))
            rstd = 1.0 / torch.sqrt(rv0.double() + EPS)
            ref = _act64((c["pre"] - rm0.double().view(1, K, 1, 1)) * (rstd * gamma.double()).view(1, K, 1, 1) + beta.double().view(1, K, 1, 1)
                         + res.double(), 1)
            # fp32 tensors: the forward's bound too.  (bf16 tensors round the conv's map in front of the affine, as the stored map of
            # the separate passes is: held to the bit-for-bit contract above alone.)
            if dt == F32:
                run.add("fold vs fp64", _rel(first["fold"], ref), TOL_FWD)
        failures += run.bad
    assert not failures, failures


# ----------------------------------------------------------------------------------------------------------------- data gradient
def _norm_inputs(cid, fam, G):
    """nx (the normalisation layer's input, the shape of dx), its fp64 statistics per (group, channel) as fp32 tables, gamma / beta for
    G = 1, an addend; nx is moved where the mask's pre-activation gamma * xhat + beta comes within MARGIN of zero"""
    N, Hh, W, Cin = H.CASES[cid]["shape"][:4]
    nx = _rnd(_table((N, Cin, Hh, W), 501, lo=-1.5, hi=2.5, noise=0.5, period=1021), fam)
    add = _rnd(_table((N, Cin, Hh, W), 502, lo=-1.0, hi=1.0, noise=0.25, period=2039), fam)
    v = nx.double().view(G, N // G, Cin, Hh * W)
    mean = v.mean((1, 3)).float()
    rstd = (1.0 / torch.sqrt(((v - mean.double().view(G, 1, Cin, 1)) ** 2).mean((1, 3)) + EPS)).float()
    gamma, beta = NR._affine(Cin) if G == 1 else (None, None)

    def z_of(t):
        z = (t.double().view(G, N // G, Cin, Hh * W) - mean.double().view(G, 1, Cin, 1)) * rstd.double().view(G, 1, Cin, 1)
        if gamma is not None:
            z = z * gamma.double().view(1, 1, Cin, 1) + beta.double().view(1, 1, Cin, 1)
        return z.view(N, Cin, Hh, W)

    near = z_of(nx).abs() < MARGIN
    if near.any():
        nx[near] = _rnd(nx[near] + 0.5, fam)
    z = z_of(nx)
    assert float(z.abs().min()) > MARGIN
    return dict(nx=nx, add=add, mean=mean, rstd=rstd, gamma=gamma, beta=beta, z=z)


def _two_roundings(d64):
    """bf16 tensors, addend joined: dx = bf16(bf16(dgrad) + addend), bit-identical to the separate passes it replaces - two roundings to
    nearest, each at most 2^-9 of its value (2^-8 of the binade's lower end), + the fp32 accumulation's noise: the measure and the bound
    of test_fused_fan_in_against_fp64_at_bench_size_bf16"""
    def check(run, name, t, ref):
        err = (t.double().cpu() - ref).abs()
        run.add(name + " excess over two roundings", float((err - (d64.abs() + ref.abs()) * (2.0 ** -8)).max()), 2e-5)
    return check


@pytest.mark.parametrize("cid,fam", _case_fams("dgrad"))
def test_data_gradient_entries_stay_inside_their_outputs_records_and_workspace(cid, fam, F, dev):
    """conv2d_dgrad plain; with bias + activation (the ConvTranspose route's epilogue); with the backward sums of the normalisation
    layer in front (unmasked for ReLU / LeakyReLU / none, masked for ReLU on fp32 tensors, G = 1 with gamma / beta and G = N without),
    with and without a joined addend; the addend alone."""
    case = H.CASES[cid]
    N, Hh, W, Cin, K, R, s, p, d = case["shape"]
    c = _case(cid, fam in ("bf16", "bf16c"))
    dt = _tdt(fam)
    xshape, wshape = (N, Cin, Hh, W), (K, Cin, R, R)
    bc = _table((Cin,), 31, lo=-0.5, hi=0.5, noise=0.1, period=7)
    ni = {G: _norm_inputs(cid, fam, G) for G in sorted({1, N})}
    failures = []
    for tname, tkw in _tunings(fam, Cin, case.get("thin")):
        run = _Run("dgrad %s %s %s" % (cid, fam, tname))
        refs = {}

        def call(g):
            gy, w = g.put(c["gy"], dt), g.put(c["w"])
            wt = F.dgrad_operand(w, xshape, s, p, d, dy_dtype=dt)
            out = {}
            dx = _unsupported(F, lambda: F.conv2d_dgrad(gy, wt, xshape, wshape, s, p, d, out_dtype=dt))
            if dx is None:
                run.say("forced class: SSCG_ERR_UNSUPPORTED before any launch")
                return out
            out["dx"] = dx
            refs["dx"] = (c["dx"], _tol(fam, dt))
            if fam == "bf16":
                out["dx_f32out"] = F.conv2d_dgrad(gy, wt, xshape, wshape, s, p, d, out_dtype=F32)
                refs["dx_f32out"] = (c["dx"], TOL_FWD)
            b = g.put(bc)
            for act in (1, 2):
                out["dx_bias_act%d" % act] = F.conv2d_dgrad(gy, wt, xshape, wshape, s, p, d, bias=b, act=act, slope=SLOPE, out_dtype=dt)
                refs["dx_bias_act%d" % act] = (_act64(c["dx"] + bc.double().view(1, Cin, 1, 1), act), _tol(fam, dt))
            for G, v in ni.items():
                L = N * Hh * W // G
                nx, add = g.put(v["nx"], dt), g.put(v["add"], dt)
                mean, rstd = g.put(v["mean"]), g.put(v["rstd"])
                ga, be = (g.put(v["gamma"]), g.put(v["beta"])) if G == 1 else (None, None)
                per = False if G == 1 else True
                for nact, masked, joined in ((1, False, False), (2, False, False), (0, False, False), (1, True, False), (1, False, True),
                                             (1, True, True)):
                    if masked and dt != F32:
                        continue
                    tag = "sums_G%d_act%d%s%s" % (G, nact, "_masked" if masked else "", "_add" if joined else "")
                    dxs, rec, did = F.conv2d_dgrad(gy, wt, xshape, wshape, s, p, d, out_dtype=dt,
                                                   bsums=(nx, mean, rstd, ga, be, (G, L, Cin), nact, SLOPE), addend=add if joined else None,
                                                   premask=masked)
                    if rec is None:
                        if nact == 1 and not masked:
                            run.say("%s: backward sums not fused for this plan (addend joined: %s)" % (tag, did))
                        if joined and did and not masked:
                            out["dx_add_G%d" % G] = dxs
                            refs["dx_add_G%d" % G] = (c["dx"] + v["add"].double(), _two_roundings(c["dx"]) if dt == BF else TOL_FWD)
                        continue
                    total = c["dx"] + (v["add"].double() if (joined and did) else 0.0)
                    out[tag + "_dx"] = dxs
                    refs[tag + "_dx"] = (torch.where(v["z"] > 0, total, torch.zeros_like(total)) if masked else total, _tol(fam, dt))
                    dg, db = (torch.empty(Cin, dtype=F32, device=dev), torch.empty(Cin, dtype=F32, device=dev)) if G == 1 else (None, None)
                    if masked:
                        dnx, _ = F.norm_bwd_from_sums(rec, dxs, nx, mean, rstd, ga, be, per, F.ACT_NONE, 0.0, dg, db)
                    else:
                        dnx, _ = F.norm_bwd_from_sums(rec, dxs, nx, mean, rstd, ga, be, per, nact, SLOPE, dg, db)
                    # the reduction-pass route on the same total
                    tot = dx if not (joined and did) else F.add(dx, add)
                    dg0, db0 = (torch.empty(Cin, dtype=F32, device=dev), torch.empty(Cin, dtype=F32, device=dev)) if G == 1 else (None, None)
                    dnx0, _ = F.norm_bwd(tot, nx, None, mean, rstd, ga, per, nact, SLOPE, True, dgamma=dg0, dbeta=db0, beta=be, overwrite=True)
                    out.update({tag + "_dnx": dnx, tag + "_dnx_passes": dnx0, tag + "_dgamma": dg, tag + "_dgamma_passes": dg0,
                                tag + "_dbeta": db, tag + "_dbeta_passes": db0})
            return out

        with _mode(F, fam, **tkw):
            first = _three_runs(F, run, call, refs)
        for name, t in first.items():       # the fused-sums route against the reduction-pass route, of the tensor's scale
            if name.endswith("_passes") or t is None or name + "_passes" not in first:
                continue
            u = first[name + "_passes"].double()
            err = float((t.double() - u).abs().max()) / (float(u.abs().max()) + 1e-30)
            # bf16 tensors: the reduction pass reads the bf16-rounded dz, the fused sums the fp32 accumulators
            # (test_norm_backward_sums_fused_into_the_bf16_data_gradient: 2e-2 on dx, 5e-3 on the parameter gradients)
            bound = TOL_SUMS + 1e-9 if dt == F32 else (2e-2 if name.endswith("_dnx") else 5e-3)
            run.add(name + " vs reduction pass", err, bound)
        failures += run.bad
    assert not failures, failures


@pytest.mark.parametrize("fam", ["f32x", "f32s", "bf16"])
@pytest.mark.parametrize("geom", [(3, 1, 1), (4, 1, 0)], ids=["3x3_s2_p1_op1", "4x4_s2_p1_op0"])
def test_conv_transpose_route_stays_inside_its_output(geom, fam, F, dev):
    """conv_transpose2d (the data gradient with bias + activation as a forward) on an odd map, 64 -> 128 channels"""
    r, pad, op = geom
    N, Cin, Hh, W, Cout = 2, 128, 9, 7, 64
    dt = _tdt(fam)
    x = _rnd(_table((N, Cin, Hh, W), 41), fam)
    w = _rnd(_table((Cin, Cout, r, r), 42, lo=-1.0, hi=1.0, noise=0.1, period=257) / (Cin * r * r) ** 0.5, fam)
    b = _table((Cout,), 43, lo=-0.5, hi=0.5, noise=0.1, period=7)
    failures = []
    for tname, tkw in _tunings(fam, Cout):
        run = _Run("conv_transpose %dx%d %s %s" % (r, r, fam, tname))
        refs = {}

        def call(g):
            xg, wg, bg = g.put(x, dt), g.put(w), g.put(b)
            out = {}
            with torch.no_grad():
                for act in (0, 1, 2):
                    y = _unsupported(F, lambda: F.conv_transpose2d(xg, wg, bg, 2, pad, op, act, SLOPE, out_f32=False))
                    out["y_act%d" % act] = y
                    if y is not None:
                        refs["y_act%d" % act] = (_act64(TF.conv_transpose2d(x.double(), w.double(), b.double(), 2, pad, op), act), _tol(fam, y.dtype))
            return out

        with _mode(F, fam, **tkw):
            _three_runs(F, run, call, refs)
        failures += run.bad
    assert not failures, failures


# ----------------------------------------------------------------------------------------------------------------- weight gradient
_WGRAD_VARIANTS = {
    # test_split_weight_gradient_variants' routes, and forced pixel splits 1 and 3 of both tile classes
    "f32s": [("plan", {}), ("fly", dict(wgrad_class=2)), ("planes", dict(wgrad_class=3)), ("planes_2stage", dict(wgrad_class=3, wgrad_flags=1)),
             ("planes_split3", dict(wgrad_class=3, wgrad_splits=3)), ("fly_64x64", dict(wgrad_class=1, wgrad_splits=2)),
             ("c0_splits1", dict(wgrad_class=0, wgrad_splits=1)), ("c0_splits3", dict(wgrad_class=0, wgrad_splits=3)),
             ("c1_splits1", dict(wgrad_class=1, wgrad_splits=1)), ("c1_splits3", dict(wgrad_class=1, wgrad_splits=3))],
    "f32x": [("plan", {}), ("c0_splits1", dict(wgrad_class=0, wgrad_splits=1)), ("c0_splits3", dict(wgrad_class=0, wgrad_splits=3)),
             ("c1_splits1", dict(wgrad_class=1, wgrad_splits=1)), ("c1_splits3", dict(wgrad_class=1, wgrad_splits=3))],
    # test_wgrad_bf16_every_kernel's switches, and forced pixel splits
    "bf16": [("plan", {}), ("flags2", dict(wgrad_flags=2)), ("c0_splits1", dict(wgrad_class=0, wgrad_splits=1)),
             ("c0_splits3", dict(wgrad_class=0, wgrad_splits=3))],
    "bf16c": [("plan", {})],
}


@pytest.mark.parametrize("cid,fam", _case_fams("wgrad"))
def test_weight_gradient_stays_inside_dw_and_its_partial_copies(cid, fam, F, dev):
    """conv2d_wgrad with out=None, and accumulating into a guarded tensor holding known values, under every wgrad_class / wgrad_flags
    variant the suite names and forced wgrad_splits 1 and 3"""
    case = H.CASES[cid]
    N, Hh, W, Cin, K, R, s, p, d = case["shape"]
    c = _case(cid, fam in ("bf16", "bf16c"))
    dt = _tdt(fam)
    old = _table((K, Cin, R, R), 61, lo=-1.0, hi=1.0, noise=0.25, period=509)
    failures = []
    # forced classes and pixel splits where both GEMM sides fill a tile, as in the tests that name the variants (K >= 64 filters, a
    # reduction of >= 64); the few-channel heads and the streaming 1x1 kernel run their own plan
    variants = _WGRAD_VARIANTS[fam] if (K >= 64 and Cin * R * R >= 64) else _WGRAD_VARIANTS[fam][:1]
    for vname, vkw in variants:
        run = _Run("wgrad %s %s %s" % (cid, fam, vname))
        refs = {}

        def call(g):
            x, gy = g.put(c["x"], dt), g.put(c["gy"], dt)
            out = {}
            dw = _unsupported(F, lambda: F.conv2d_wgrad(x, gy, (K, Cin, R, R), s, p, d))
            if dw is None:
                run.say("SSCG_ERR_UNSUPPORTED before any launch")
                return out
            run.say("workspace query %d bytes (dw %d bytes)" % (F._ws_bytes(F.make_desc(x.shape, (K, Cin, R, R), s, p, d, F.PAD_ZEROS, xdt=F._dt(x),
                                                                                     ydt=F._dt(gy), prec=F._prec("wgrad")), "wgrad"), dw.numel() * 4))
            out["dw"] = dw
            refs["dw"] = (c["dw"], TOL_WGRAD[fam])
            acc = g.put(old)
            F.conv2d_wgrad(x, gy, (K, Cin, R, R), s, p, d, out=acc, accumulate=True)
            out["acc"] = acc
            refs["acc"] = (c["dw"], lambda r, n, t, ref: r.add(n + " - old", _rel(t.double().cpu() - old.double(), ref), TOL_WACC))
            return out

        with _mode(F, fam, **vkw):
            _three_runs(F, run, call, refs)
        failures += run.bad
    assert not failures, failures


@pytest.mark.parametrize("fam", ["f32x", "f32s", "bf16"])
def test_a_workspace_one_byte_short_of_the_query_is_refused_through_the_wrappers(fam, F, dev):
    """The split-K tail case with every workspace view one byte shorter than the wrapper asked for: the wrappers pass the view's size, so
    the entries' own check answers SSCG_ERR_WORKSPACE before any launch (with the product's 1.25x buffer it never sees the promised
    size).  Forward, data gradient, weight gradient."""
    cid = "tail91"
    N, Hh, W, Cin, K, R, s, p, d = H.CASES[cid]["shape"]
    c = _case(cid, fam == "bf16")
    dt = _tdt(fam)
    refused = []
    with _mode(F, fam):
        with _Guarded(F, "ff", shrink_ws=1) as g:
            x, w, gy = g.put(c["x"], dt), g.put(c["w"]), g.put(c["gy"], dt)
            wt = F.dgrad_operand(w, (N, Cin, Hh, W), s, p, d, dy_dtype=dt)
            for name, fn in (("fwd", lambda: F.conv2d_fwd(x, w, None, s, p, d, out_f32=False)),
                             ("dgrad", lambda: F.conv2d_dgrad(gy, wt, (N, Cin, Hh, W), (K, Cin, R, R), s, p, d, out_dtype=dt)),
                             ("wgrad", lambda: F.conv2d_wgrad(x, gy, (K, Cin, R, R), s, p, d))):
                with pytest.raises(F._lib.SscgError, match="SSCG_ERR_WORKSPACE"):
                    fn()
                refused.append(name)
            assert g.damage() == []
    assert refused == ["fwd", "dgrad", "wgrad"]


# ----------------------------------------------------------------------------------------------------------------- PixelDiscriminator front
@pytest.mark.parametrize("cin", H.CASES["front"]["front"])
def test_pixel_discriminator_front_stays_inside_its_outputs_and_records(cin, F, dev):
    """conv2d_front_fwd: Conv2d(cin, 64, 1x1) -> LeakyReLU -> Conv2d(64, 128, 1x1) in one launch on an odd map, with the 64-channel map
    written and the statistics records of the norm layer behind it (G = N and G = 1), under the plan and both tile classes that carry
    the fused prologue"""
    N, Hh, W, _, K = H.CASES["front"]["shape"][:5]
    x = _table((N, cin, Hh, W), 71)
    w1 = _table((64, cin, 1, 1), 72, lo=-1.0, hi=1.0, noise=0.1, period=61) / cin ** 0.5
    b1 = _table((64,), 73, lo=-0.5, hi=0.5, noise=0.1, period=7)
    w2 = _table((K, 64, 1, 1), 74, lo=-1.0, hi=1.0, noise=0.1, period=257) / 8.0
    b2 = _table((K,), 75, lo=-0.5, hi=0.5, noise=0.1, period=7)
    h1 = _act64(TF.conv2d(x.double(), w1.double(), b1.double()), 2)
    yr = TF.conv2d(h1, w2.double(), b2.double())
    failures = []
    for tname, tkw in (("plan", {}), ("class0", dict(tile_class=0)), ("class1", dict(tile_class=1))):
        run = _Run("front cin%d %s" % (cin, tname))
        refs = {}

        def call(g):
            xg, w1g, b1g, w2g, b2g = g.put(x), g.put(w1), g.put(b1), g.put(w2), g.put(b2)
            out = {}
            if not F.conv2d_front_applies(xg, w1g, w2g, 1, 0, 1, F.PAD_ZEROS):
                run.say("not served under this tuning")
                return out
            for G in (N, 1):
                L = N * Hh * W // G
                y, h, cs = F.conv2d_front_fwd(xg, w1g, b1g, SLOPE, w2g, b2g, glc=(G, L, K), want_h1=True)
                mean, rstd = F.norm_stats_from_conv(cs, (G, L, K), EPS)
                yv = yr.view(G, N // G, K, Hh * W)
                mu = yv.mean((1, 3))
                var = ((yv - mu.view(G, 1, K, 1)) ** 2).mean((1, 3))
                scale = float(mu.abs().max() + var.sqrt().max())
                out.update({"y_G%d" % G: y, "h1_G%d" % G: h, "mean_G%d" % G: mean, "rstd_G%d" % G: rstd})
                refs["y_G%d" % G] = (yr, TOL_FWD)
                refs["h1_G%d" % G] = (h1, TOL_FWD)
                refs["mean_G%d" % G] = (mu, lambda r, n, t, ref, sc=scale: r.add(n, float((t.double().cpu() - ref).abs().max()) / sc, TOL_STATS["f32s"]))
                refs["rstd_G%d" % G] = (1.0 / torch.sqrt(var + EPS), TOL_STATS["f32s"])
            y, h, cs = F.conv2d_front_fwd(xg, w1g, b1g, SLOPE, w2g, b2g)
            out["y_alone"] = y
            refs["y_alone"] = (yr, TOL_FWD)
            return out

        with _mode(F, "f32s", **tkw):
            first = _three_runs(F, run, call, refs)
        if tname == "plan":
            run.true("served", "y_alone" in first)
        failures += run.bad
    assert not failures, failures


# ----------------------------------------------------------------------------------------------------------------- normalisation entries
def _norm_case(glc, dtype):
    G, L, Cn = glc
    x = NR._table(G, L, Cn, dtype, 900 + Cn)
    gen = torch.Generator().manual_seed(950 + Cn)
    dy = NR._rnd(torch.randn(G, L, Cn, generator=gen), dtype)
    gamma, beta = NR._affine(Cn)
    xd = x.double()
    mean = xd.mean(1)
    var = (xd - mean[:, None, :]).square().mean(1)
    rstd = (var + EPS).rsqrt()
    z = (xd - mean[:, None, :]) * rstd[:, None, :] * gamma.double() + beta.double()
    near = z.abs() < MARGIN
    if near.any():      # (the statistics stay the tables they are: the entries take them as inputs)
        x[near] = NR._rnd(x[near] + 0.5, dtype)
        z = (x.double() - mean[:, None, :]) * rstd[:, None, :] * gamma.double() + beta.double()
    assert float(z.abs().min()) > MARGIN
    return dict(G=G, L=L, C=Cn, x=x, dy=dy, res=torch.zeros_like(x), gamma=gamma, beta=beta, mean=mean, var=var, rstd=rstd, affine=True)


def _nchw(t):
    """[G][L][C] CPU table -> the (G, C, L, 1) NCHW-shaped tensor whose channels-last memory it is"""
    return t.permute(0, 2, 1).unsqueeze(-1)


def _glc_of(t, G, L, Cn):
    return t.detach().permute(0, 2, 3, 1).reshape(G, L, Cn)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("glc", H.NORM_SHAPES, ids=lambda s: "g%d_l%d_c%d" % s)
def test_norm_entries_stay_inside_their_outputs_and_workspace(glc, dtype, F, dev):
    """colsum, norm_stats (without and with running statistics, grouped), norm_bwd (ReLU / LeakyReLU / none, the mask recomputed from
    x, gamma / beta gradients written) on [G][L][C]: bounds of test_norm_regimes_gpu (TOL, TOL_STAT, 2^-22 of the column's sum of |x|)"""
    G, L, Cn = glc
    inp = _norm_case(glc, dtype)
    tol = NR.TOL[dtype]
    run = _Run("norm g%d l%d c%d %s" % (G, L, Cn, "f32" if dtype == F32 else "bf16"))
    refs = {}
    ch = torch.arange(Cn, dtype=F32)
    rm0, rv0 = 0.1 * (ch % 9) - 0.45, 0.5 + 0.125 * (ch % 6)
    xd = inp["x"].double()
    # (the statistics of the moved x: what norm_stats must find)
    mu = xd.mean(1)
    var = (xd - mu[:, None, :]).square().mean(1)
    per = True if G > 1 else False

    def per_element(scale=None, bound=NR.TOL_STAT):
        return lambda r, n, t, ref: r.add(n, NR._per_element(t, ref, scale), bound)

    def maxnorm(bound):
        return lambda r, n, t, ref: r.add(n, NR._maxnorm(_glc_of(t, G, L, Cn), ref, dev), bound)

    def call(g):
        x, dy = g.put(_nchw(inp["x"]), dtype), g.put(_nchw(inp["dy"]), dtype)
        out = {}
        out["colsum"] = F.colsum(G * L, Cn, x)
        refs["colsum"] = (xd.sum((0, 1)), per_element(xd.abs().sum((0, 1)), 2.0 ** -22))
        pre = g.put(rm0)
        F.colsum(G * L, Cn, x, out=pre, accumulate=True)
        out["colsum_acc"] = pre
        refs["colsum_acc"] = (xd.sum((0, 1)) + rm0.double(), per_element(xd.abs().sum((0, 1)) + rm0.double().abs(), 2.0 ** -22))
        out["mean"], out["rstd"] = F.norm_stats(x, per, EPS)
        refs["mean"], refs["rstd"] = (mu, per_element()), ((var + EPS).rsqrt(), per_element())
        rm, rv = g.put(rm0), g.put(rv0)
        out["mean_grouped"], out["rstd_grouped"] = F.norm_stats(x, G if G > 1 else False, EPS, rm, rv, 0.1)
        refs["mean_grouped"], refs["rstd_grouped"] = (mu, per_element()), ((var + EPS).rsqrt(), per_element())
        # (the running mean is a sum of terms of either sign - with 2048 channels one of them cancels to 1e-4 of its terms: relative to
        # the sum of the |terms|, as test_norm_regimes_gpu measures dgamma / dbeta; the running variance's terms are positive)
        rmr, rvr, rms = rm0.double(), rv0.double(), rm0.double().abs()
        for gi in range(G):
            rmr, rms = 0.9 * rmr + 0.1 * mu[gi], 0.9 * rms + 0.1 * mu[gi].abs()
            rvr = 0.9 * rvr + 0.1 * var[gi] * L / (L - 1)
        out["running_mean"], out["running_var"] = rm, rv
        refs["running_mean"], refs["running_var"] = (rmr, per_element(rms)), (rvr, per_element())
        mean, rstd, ga, be = g.put(inp["mean"].float()), g.put(inp["rstd"].float()), g.put(inp["gamma"]), g.put(inp["beta"])
        inp32 = dict(inp, mean=inp["mean"].float().double(), rstd=inp["rstd"].float().double())
        for act, code in (("relu", F.ACT_RELU), ("lrelu", F.ACT_LRELU), ("none", F.ACT_NONE)):
            ref = NR._reference(inp32, act)
            dg, db = torch.empty(Cn, dtype=F32, device=dev), torch.empty(Cn, dtype=F32, device=dev)
            dx, _ = F.norm_bwd(dy, x, None, mean, rstd, ga, per, code, SLOPE, True, dgamma=dg, dbeta=db, beta=be, overwrite=True)
            out.update({"dx_" + act: dx, "dgamma_" + act: dg, "dbeta_" + act: db})
            refs["dx_" + act] = (ref["dx"], maxnorm(tol["dx"]))
            refs["dgamma_" + act] = (ref["dgamma"], per_element(ref["dgamma_scale"]))
            refs["dbeta_" + act] = (ref["dbeta"], per_element(ref["dbeta_scale"]))
        return out

    _three_runs(F, run, call, refs)
    run.check()


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("Cn", [16, 256])
@pytest.mark.parametrize("gl", [(3, 143), (2, 4097), (1, 8712)], ids=lambda s: "g%d_l%d" % s)
def test_norm_head_stays_inside_its_outputs_and_workspace(gl, Cn, dtype, F, dev):
    """norm_head_fwd / norm_head_bwd (norm -> LeakyReLU -> 1x1 single-channel conv in one pass) at the limits of sscg_norm_head_applies"""
    G, L = gl
    assert F.norm_head_applies(Cn)
    inp = _norm_case((G, L, Cn), dtype)
    run = _Run("norm_head g%d l%d c%d %s" % (G, L, Cn, "f32" if dtype == F32 else "bf16"))
    w = _table((Cn,), 81, lo=-1.0, hi=1.0, noise=0.1, period=13) / Cn ** 0.5
    bias = torch.tensor([0.3])
    dout = _table((G, L), 82, lo=-1.0, hi=1.0, noise=0.25, period=1021)
    mean, rstd = inp["mean"].float().double(), inp["rstd"].float().double()
    xr = inp["x"].double().requires_grad_(True)
    ga, be, wr = (inp["gamma"].double().requires_grad_(True), inp["beta"].double().requires_grad_(True), w.double().requires_grad_(True))
    # statistics as constants (flags bit 0 clear): the entry takes mean / rstd as they are
    z = (xr - mean[:, None, :]) * rstd[:, None, :] * ga + be
    outr = (torch.where(z > 0, z, z * float(torch.tensor(SLOPE, dtype=F32))) * wr).sum(2) + bias.double()
    outr.backward(dout.double())
    refs = {}

    def call(g):
        x = g.put(_nchw(inp["x"]), dtype)
        m, r, gam, bet, wg, bg = g.put(mean.float()), g.put(rstd.float()), g.put(inp["gamma"]), g.put(inp["beta"]), g.put(w), g.put(bias)
        do = g.put(dout.view(G, 1, L, 1))
        per = True if G > 1 else False
        out = {}
        out["out"] = F.norm_head_fwd(x, m, r, gam, bet, wg, bg, per, F.ACT_LRELU, SLOPE)
        refs["out"] = (outr.detach().view(G, 1, L, 1), TOL_HEAD)
        dwb = torch.empty(Cn + 1, dtype=F32, device=dev)
        dg, db = torch.empty(Cn, dtype=F32, device=dev), torch.empty(Cn, dtype=F32, device=dev)
        dx = F.norm_head_bwd(do, wg, x, m, r, gam, bet, per, F.ACT_LRELU, SLOPE, False, dwb, dg, db)
        out.update(dx=dx, dwb=dwb, dgamma=dg, dbeta=db)
        refs["dx"] = (_nchw(xr.grad), TOL_HEAD if dtype == F32 else 2 * EPS16)
        refs["dwb"] = (torch.cat((wr.grad, dout.double().sum().view(1))), TOL_HEAD)
        refs["dgamma"], refs["dbeta"] = (ga.grad, TOL_HEAD), (be.grad, TOL_HEAD)
        return out

    _three_runs(F, run, call, refs)
    run.check()
