"""The convolution entries against the exact result of exactly representable inputs: torch.equal, no tolerance.

Every other convolution check carries a tolerance of 1e-5 or more and runs on random tables; the l piece of the split contraction
(`--dtype f32`: each fp32 operand as three bfloat16 pieces h + m + l, six of the nine piece products) weighs 2^-16 of its operand and
the product m*m 2^-16 of the product, so a kernel that loses one of them in one region of the operand space - a ragged last k-tile, the
channels a stem is padded to, the tail rows behind the last whole round of workgroups, one parity class of a stride-2 data gradient,
one split-K piece - passes them.  The probes of tests/conv_exact_probes.py (dense small integers; carry-a / carry-b: one operand with
23-bit significands against +-2^j placed so that every output receives at most one product; pair: 11-bit significands on both sides)
have results that are fp32 numbers whatever the summation order: tests/test_conv_exact_host.py proves that without a GPU, and that the
probes put a nonzero product on every tap, filter and channel block.  bf16 tensors: significands of 8 (carry) and 4 + 4 (pair) bits,
a routing check; a bf16 result of the dense probe is the exact integer rounded once (twice with a joined addend: two_roundings).

Cases, families, tunings and weight-gradient variants are those of tests/test_conv_extents_gpu.py: every case of
test_conv_extents_host.CASES under the library's plan, every forced tile class of the family and forced split 3 (a forced class the
family has no instance of answers SSCG_ERR_UNSUPPORTED before any launch and is counted as skipped; the plan never is), the weight
gradient under every variant of _WGRAD_VARIANTS.  A mismatch is reported with the count of differing elements, the first differing
index and the error against 2^-8, 2^-16 and 2^-24 of the expected value - which names the lost piece.
Figures: `conv_exact ...` lines (pytest -s; profiles/conv_exact.txt)."""
import time

import pytest
import torch

import conv_exact_probes as X
import test_conv_exact_host as XH
import test_conv_extents_gpu as E
import test_conv_extents_host as H

pytestmark = pytest.mark.gpu
CL = torch.channels_last
F32, BF = torch.float32, torch.bfloat16
EPS = 1e-5
SMALL = ("head3", "stem3", "stem20", "stem21")      # the cases the extents file runs with reflection padding
NAMES = {"fwd": ("n", "k", "y", "x"), "dgrad": ("n", "c", "y", "x"), "wgrad": ("k", "c", "r", "s")}


def _kinds(fam):
    return ("dense",) if fam == "bf16c" else X.KINDS


def _put(t, dev, dtype=F32):
    d = t.to(dev)
    if d.dim() == 4:
        d = d.contiguous(memory_format=CL)
    return d.to(dtype)


class _Tally:
    """what ran, what was skipped, what differed, for one test"""

    def __init__(self, label, dev):
        self.label, self.dev, self.ran, self.skipped, self.compared, self.bad, self.t0 = label, dev, 0, 0, 0, [], time.time()
        self.notes, self.joined = [], [0, 0]

    def expect(self, exp64, dtype):
        """(the expected values as the tensor of `dtype` holds them, on the device; the same on the CPU)"""
        e = X.stored(exp64, dtype)
        return e.to(self.dev), e

    def same(self, where, got, exp, names):
        self.compared += 1
        e_dev, e_cpu = exp
        if tuple(got.shape) == tuple(e_dev.shape) and bool((got.float() == e_dev).all()):
            return
        if len(self.bad) < 12:
            self.bad.append("%s: %s" % (where, X.mismatch(got, e_cpu, names)))
        else:
            self.bad.append(where)

    def note(self, text):
        if text not in self.notes:
            self.notes.append(text)

    def variant(self, ran):
        if ran:
            self.ran += 1
        else:
            self.skipped += 1

    def check(self):
        torch.cuda.synchronize()
        if self.joined[1]:
            self.note("addend joined in %d of %d variants" % tuple(self.joined))
        print("conv_exact %s: %d variants ran, %d skipped (SSCG_ERR_UNSUPPORTED), %d comparisons, %d differ, %.2f s%s" % (
            self.label, self.ran, self.skipped, self.compared, len(self.bad), time.time() - self.t0,
            "".join("; " + n for n in self.notes)))
        assert self.ran > 0
        assert not self.bad, "%s: %d comparisons differ:\n%s" % (self.label, len(self.bad), "\n".join(self.bad[:12]))


def _probes(entry, shape, fam):
    for kind in _kinds(fam):
        for p in X.instances(entry, shape, kind, fam == "bf16"):
            yield kind, p, "%s#%d" % (kind, p["inst"])


# ----------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("cid,fam", E._case_fams("fwd"))
def test_forward_entries_return_the_exact_result(cid, fam, F, dev):
    """conv2d_fwd plain, with bias, bias + ReLU, bias + LeakyReLU 0.25, with reflection padding (stem / head cases; dense and carry-a:
    a sparse x would meet its own mirror image), and the y of conv2d_fwd_norm"""
    case = H.CASES[cid]
    shape = case["shape"]
    N, Hh, W, Cin, K, R, s, p, d = shape
    dt = E._tdt(fam)
    tally = _Tally("fwd %s %s" % (cid, fam), dev)
    for kind, pr, tag in _probes("fwd", shape, fam):
        x, w, b = _put(pr["x"], dev, dt), _put(pr["w"], dev), _put(pr["bias"], dev)
        pre = pr["exact"] + pr["bias"].double().view(1, K, 1, 1)
        M = pre.numel() // K
        exp = {"plain": tally.expect(pr["exact"], dt)}
        for act in (0, 1, 2):
            exp["bias_act%d" % act] = tally.expect(X.activation(pre, act), dt)
        reflect = cid in SMALL and kind in ("dense", "carry-a")
        if reflect:
            ops = dict(x=pr["x"], w=pr["w"])
            exp["reflect"] = tally.expect(X.reference("fwd", shape, reflect=True, **ops) + pr["bias"].double().view(1, K, 1, 1), dt)
        for tname, tkw in E._tunings(fam, K, case.get("thin")):
            where = "%s %s " % (tag, tname)
            with E._mode(F, fam, **tkw):
                y = E._unsupported(F, lambda: F.conv2d_fwd(x, w, None, s, p, d, F.PAD_ZEROS, 0, 0.0, out_f32=False))
                tally.variant(y is not None)
                if y is None:
                    assert tname != "plan", "the library's own plan is never unsupported"
                    continue
                tally.same(where + "plain", y, exp["plain"], NAMES["fwd"])
                for act in (0, 1, 2):
                    y = F.conv2d_fwd(x, w, b, s, p, d, F.PAD_ZEROS, act, X.SLOPE, out_f32=False)
                    tally.same(where + "bias_act%d" % act, y, exp["bias_act%d" % act], NAMES["fwd"])
                if reflect:
                    y = E._unsupported(F, lambda: F.conv2d_fwd(x, w, b, s, p, d, F.PAD_REFLECT, 0, 0.0, out_f32=False))
                    if y is None:
                        tally.note("reflection padding unsupported under %s" % tname)
                    else:
                        tally.same(where + "reflect", y, exp["reflect"], NAMES["fwd"])
                r3 = E._unsupported(F, lambda: F.conv2d_fwd_norm(x, w, b, s, p, d, F.PAD_ZEROS, False, (1, M, K), EPS, None, None, 0.1))
                if r3 is not None:
                    tally.same(where + "fwd_norm y (statistics %s)" % ("fused" if r3[1] is not None else "not fused"), r3[0],
                               exp["bias_act0"], NAMES["fwd"])
    tally.check()


def test_a_contraction_that_rounds_its_operands_is_seen(F, dev):
    """The probes against real kernels that lose pieces by design: the "bf16c" mode (fp32 tensors, operands rounded to bfloat16 between
    LDS and the matrix cores) on the carry probes returns the exact result of the ROUNDED operand bit for bit - and that differs from
    the reference in nearly every element, by at most the 2^-8 the message then names."""
    cid = H.BF16C_CASE
    shape = H.CASES[cid]["shape"]
    N, Hh, W, Cin, K, R, s, p, d = shape
    for kind in ("carry-a", "carry-b"):
        pr = X.instances("fwd", shape, kind)[0]
        with E._mode(F, "bf16c"):
            y = F.conv2d_fwd(_put(pr["x"], dev), _put(pr["w"], dev), None, s, p, d, F.PAD_ZEROS, 0, 0.0, out_f32=False)
        rounded = X.reference("fwd", shape, x=pr["x"].to(BF).float(), w=pr["w"].to(BF).float())
        assert X.mismatch(y, X.stored(rounded, F32), NAMES["fwd"]) == ""
        text = X.mismatch(y, X.stored(pr["exact"], F32), NAMES["fwd"])
        print("conv_exact lossy bf16c %s %s: %s" % (cid, kind, text))
        differ = float((y.cpu().double() != pr["exact"]).sum()) / float((pr["exact"] != 0).sum())
        rel = ((y.cpu().double() - pr["exact"]).abs() / pr["exact"].abs().clamp_min(1e-300)).max()
        assert text != "" and differ > 0.9 and 2.0 ** -16 < float(rel) <= 2.0 ** -8, (kind, differ, float(rel))


# ----------------------------------------------------------------------------------------------------------------- data gradient
def _dgrad_calls(F, tally, where, pr, shape, gy, w, b, add, dt, exp):
    """the data-gradient entries of one probe under the current mode and tuning; False when the forced class is unsupported"""
    N, Hh, W, Cin, K, R, s, p, d = shape
    xshape, wshape = (N, Cin, Hh, W), (K, Cin, R, R)
    names = NAMES["dgrad"]
    wt = F.dgrad_operand(w, xshape, s, p, d, dy_dtype=dt)
    dx = E._unsupported(F, lambda: F.conv2d_dgrad(gy, wt, xshape, wshape, s, p, d, out_dtype=dt))
    if dx is None:
        return False
    tally.same(where + "dgrad", dx, exp["plain"], names)
    dxp = E._unsupported(F, lambda: F.conv2d_dgrad_param(gy, w, xshape, wshape, s, p, d, out_dtype=dt))
    if dxp is None:
        tally.note("conv2d_dgrad_param unsupported under a forced class")
    else:
        tally.same(where + "dgrad_param", dxp, exp["plain"], names)
    for act in (1, 2):
        y = F.conv2d_dgrad(gy, wt, xshape, wshape, s, p, d, bias=b, act=act, slope=X.SLOPE, out_dtype=dt)
        tally.same(where + "dgrad bias_act%d" % act, y, exp["bias_act%d" % act], names)
        y = E._unsupported(F, lambda: F.conv2d_dgrad_param(gy, w, xshape, wshape, s, p, d, bias=b, act=act, slope=X.SLOPE, out_dtype=dt))
        if y is not None:
            tally.same(where + "dgrad_param bias_act%d" % act, y, exp["bias_act%d" % act], names)
    dxa, _, joined = F.conv2d_dgrad(gy, wt, xshape, wshape, s, p, d, out_dtype=dt, addend=add)
    tally.joined[1] += 1
    if joined:      # (elsewhere sscg_conv2d_dgrad_add_applies declines and the caller adds)
        tally.joined[0] += 1
        tally.same(where + "dgrad + addend", dxa, exp["joined"], names)
    return True


def _dgrad_expectations(tally, pr, dt):
    Cin = pr["shape"][3]
    pre = pr["exact"] + pr["bias"].double().view(1, Cin, 1, 1)
    exp = {"plain": tally.expect(pr["exact"], dt)}
    for act in (0, 1, 2):
        exp["bias_act%d" % act] = tally.expect(X.activation(pre, act), dt)
    if dt == BF:
        j = X.two_roundings(pr["exact"], pr["addend"])
        exp["joined"] = (j.to(tally.dev), j)
    else:
        exp["joined"] = tally.expect(pr["exact"] + pr["addend"].double(), dt)
    return exp


@pytest.mark.parametrize("cid,fam", E._case_fams("dgrad"))
def test_data_gradient_entries_return_the_exact_result(cid, fam, F, dev):
    """conv2d_dgrad and conv2d_dgrad_param plain and with bias + ReLU / LeakyReLU 0.25 (the ConvTranspose route's epilogue);
    conv2d_dgrad with the joined addend where the library joins it (integers for dense, zeros elsewhere)"""
    case = H.CASES[cid]
    shape = case["shape"]
    Cin = shape[3]
    dt = E._tdt(fam)
    tally = _Tally("dgrad %s %s" % (cid, fam), dev)
    for kind, pr, tag in _probes("dgrad", shape, fam):
        gy, w, b, add = _put(pr["gy"], dev, dt), _put(pr["w"], dev), _put(pr["bias"], dev), _put(pr["addend"], dev, dt)
        exp = _dgrad_expectations(tally, pr, dt)
        for tname, tkw in E._tunings(fam, Cin, case.get("thin")):
            with E._mode(F, fam, **tkw):
                ran = _dgrad_calls(F, tally, "%s %s " % (tag, tname), pr, shape, gy, w, b, add, dt, exp)
            tally.variant(ran)
            assert ran or tname != "plan", "the library's own plan is never unsupported"
    tally.check()


@pytest.mark.parametrize("fam", ["f32x", "f32s", "bf16"])
@pytest.mark.parametrize("tid", list(XH.TRANSPOSED))
def test_conv_transpose_returns_the_exact_result(tid, fam, F, dev):
    """conv_transpose2d (the data gradient with bias + activation as a forward) on the two geometries of
    test_conv_transpose_route_stays_inside_its_output: x = the probe's gy, w [Cin, Cout, r, r] = the mirrored convolution's [K, C, r, r]"""
    shape, op = XH.TRANSPOSED[tid]
    Cout, pad = shape[3], shape[7]
    dt = E._tdt(fam)
    tally = _Tally("conv_transpose %s %s" % (tid, fam), dev)
    for kind, pr, tag in _probes("dgrad", shape, fam):
        x, w, b = _put(pr["gy"], dev, dt), _put(pr["w"], dev), _put(pr["bias"], dev)
        exp = _dgrad_expectations(tally, pr, dt)
        for tname, tkw in E._tunings(fam, Cout):
            with E._mode(F, fam, **tkw), torch.no_grad():
                ran = False
                for act in (0, 1, 2):
                    y = E._unsupported(F, lambda: F.conv_transpose2d(x, w, b, 2, pad, op, act, X.SLOPE, out_f32=False))
                    if y is not None:
                        ran = True
                        tally.same("%s %s act%d" % (tag, tname, act), y, exp["bias_act%d" % act], NAMES["dgrad"])
            tally.variant(ran)
            assert ran or tname != "plan", "the library's own plan is never unsupported"
    tally.check()


# ----------------------------------------------------------------------------------------------------------------- weight gradient
@pytest.mark.parametrize("cid,fam", E._case_fams("wgrad"))
def test_weight_gradient_returns_the_exact_result(cid, fam, F, dev):
    """conv2d_wgrad fresh, and accumulating into a tensor of small integers (dense; zeros elsewhere), under every variant of
    test_weight_gradient_stays_inside_dw_and_its_partial_copies; the whole of dw is compared"""
    shape = H.CASES[cid]["shape"]
    N, Hh, W, Cin, K, R, s, p, d = shape
    dt = E._tdt(fam)
    variants = E._WGRAD_VARIANTS[fam] if (K >= 64 and Cin * R * R >= 64) else E._WGRAD_VARIANTS[fam][:1]
    tally = _Tally("wgrad %s %s" % (cid, fam), dev)
    for kind, pr, tag in _probes("wgrad", shape, fam):
        x, gy, old = _put(pr["x"], dev, dt), _put(pr["gy"], dev, dt), _put(pr["old"], dev)
        exp_dw, exp_acc = tally.expect(pr["exact"], F32), tally.expect(pr["exact"] + pr["old"].double(), F32)
        for vname, vkw in variants:
            with E._mode(F, fam, **vkw):
                dw = E._unsupported(F, lambda: F.conv2d_wgrad(x, gy, (K, Cin, R, R), s, p, d))
                tally.variant(dw is not None)
                if dw is None:
                    assert vname != "plan", "the library's own plan is never unsupported"
                    continue
                tally.same("%s %s dw" % (tag, vname), dw, exp_dw, NAMES["wgrad"])
                acc = old.clone(memory_format=torch.preserve_format)
                F.conv2d_wgrad(x, gy, (K, Cin, R, R), s, p, d, out=acc, accumulate=True)
                tally.same("%s %s accumulated" % (tag, vname), acc, exp_acc, NAMES["wgrad"])
    tally.check()


# ----------------------------------------------------------------------------------------------------------------- PixelDiscriminator front
@pytest.mark.parametrize("cin", H.CASES["front"]["front"])
def test_pixel_discriminator_front_returns_the_exact_result(cin, F, dev):
    """conv2d_front_fwd on the dense probe (slope 0.25: h1 holds multiples of 0.25; test_front_probe_stays_below_two_to_the_24): y and
    the 64-channel map, with and without the statistics records, under the plan and both tile classes that carry the fused prologue"""
    shape = H.CASES["front"]["shape"]
    N, Hh, W, _, K = shape[:5]
    pr = X.front_probe(shape, cin)
    tally = _Tally("front cin%d" % cin, dev)
    x, w1, b1, w2, b2 = (_put(pr[n], dev) for n in ("x", "w1", "b1", "w2", "b2"))
    exp_y, exp_h = tally.expect(pr["y"], F32), tally.expect(pr["h1"], F32)
    for tname, tkw in (("plan", {}), ("class0", dict(tile_class=0)), ("class1", dict(tile_class=1))):
        with E._mode(F, "f32s", **tkw):
            served = F.conv2d_front_applies(x, w1, w2, 1, 0, 1, F.PAD_ZEROS)
            tally.variant(served)
            assert served or tname != "plan", "the library's own plan serves the front"
            if not served:
                continue
            for G in (N, 1):
                y, h, _ = F.conv2d_front_fwd(x, w1, b1, X.SLOPE, w2, b2, glc=(G, N * Hh * W // G, K), want_h1=True)
                tally.same("%s G%d y" % (tname, G), y, exp_y, NAMES["fwd"])
                tally.same("%s G%d h1" % (tname, G), h, exp_h, NAMES["fwd"])
            y, _, _ = F.conv2d_front_fwd(x, w1, b1, X.SLOPE, w2, b2)
            tally.same("%s y alone" % tname, y, exp_y, NAMES["fwd"])
    tally.check()
