"""The probes of tests/conv_exact_probes.py are exact, and they reach what they are for (no GPU).

tests/test_conv_exact_gpu.py compares the convolution entries with the fp64 result of these probes at zero tolerance.  That is only
a fair demand where the exact result is a number of the output's format and where NO summation order of the partial sums a kernel may
form rounds; and it only closes the gap it is meant to close where the probes put a nonzero product on every tap, filter and channel
block with all the pieces of the split contraction (csrc/common.h sscg_split3: x = h + m + l) in play.  Asserted here, for every case
of test_conv_extents_host.CASES and the two ConvTranspose geometries, per entry and probe kind:
  * dense: reduction length x magnitudes (+ bias, addend, accumulate target) < 2^24;
  * carry / pair: at most one nonzero term per output element (an indicator convolution of the nonzero patterns);
  * carry / pair: the pieces of both factors of every such term sum to the factor exactly, and every order of the fp32 partial sums
    of the piece products the library forms (a0 b0, a0 b1, a1 b0, a0 b2, a1 b1, a2 b0) gives the exact product - all permutations of
    the nonzero ones, which includes the leading product in an accumulator of its own (KS_ACC2 of conv_split.hip: the others first, the
    leading one last), and the two-by-two pairings;
  * carry: at least 90 % of the wide values have l != 0;
  * coverage over the instances: every tap, every filter, the first, the last and one channel of every block of 64 in a nonzero
    product; weight gradient, carry-a: at least half of dw nonzero;
  * torch's CPU fp32 convolution of every probe equals the fp64 one;
  * a deliberately wrong CPU emulation of the split contraction (the l piece of one operand dropped; m*m omitted) differs from the
    reference on the carry / pair probes while it stays inside the 2e-5 the tolerance tests allow.
Figures are printed (`conv_exact host ...`, shown by pytest -s; profiles/conv_exact.txt)."""
import itertools

import pytest
import torch

import conv_exact_probes as X
import test_conv_extents_host as H

F32, F64 = torch.float32, torch.float64
# the mirrored convolutions of test_conv_transpose_route_stays_inside_its_output (x 2 x 128 x 9 x 7 -> 64 channels, stride 2): the data
# gradient of (N, H, W, C, K, R, stride, pad, dil)
TRANSPOSED = {"t3x3_s2_p1_op1": ((2, 18, 14, 64, 128, 3, 2, 1, 1), 1), "t4x4_s2_p1_op0": ((2, 18, 14, 64, 128, 4, 2, 1, 1), 0)}
ENTRIES = ("fwd", "dgrad", "wgrad")
SHAPES = [(cid, H.CASES[cid]["shape"], ENTRIES) for cid in H.CASE_IDS] + [(tid, TRANSPOSED[tid][0], ("dgrad",)) for tid in TRANSPOSED]
LIMIT = 2 ** 24
SIX = ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))      # the piece products of the split contraction (csrc/common.h)


def _params():
    return [pytest.param(shape, entries, id=cid) for cid, shape, entries in SHAPES]


def _factors(p):
    """(a, b): the two factors of the one term each output element receives, as tensors of the output's shape (0 where there is none);
    a from the operand that carries, b from the sparse one"""
    ops = {n: p[n] for n in X.ENTRY_OPERANDS[p["entry"]]}
    ind = dict(ops)
    ind[p["sparse"]] = (ops[p["sparse"]] != 0).float()
    a = X.reference(p["entry"], p["shape"], **ind)
    one = dict(ops)
    one[p["full"]] = torch.ones_like(ops[p["full"]])
    b = X.reference(p["entry"], p["shape"], **one)
    return a.float(), torch.where(a != 0, b, torch.zeros_like(b)).float()


def _orders(products):
    """every way the suite admits of summing `products` (fp32 tensors) in fp32: all sequential orders; two-by-two pairings of four"""
    n = len(products)
    for perm in itertools.permutations(range(n)):
        acc = products[perm[0]]
        for i in perm[1:]:
            acc = acc + products[i]
        yield perm, acc
    if n == 4:
        for pair in ((0, 1, 2, 3), (0, 2, 1, 3), (0, 3, 1, 2)):
            yield pair, (products[pair[0]] + products[pair[1]]) + (products[pair[2]] + products[pair[3]])


@pytest.mark.parametrize("shape,entries", _params())
def test_dense_probe_stays_below_two_to_the_24(shape, entries):
    N, Hh, W, Cin, K, R, s, p, d = shape
    _, _, P, Q = H.geometry(shape)
    bound = {"fwd": Cin * R * R * X.DENSE_X * X.DENSE_W + X.DENSE_B,
             "dgrad": K * R * R * X.DENSE_X * X.DENSE_W + X.DENSE_B + X.DENSE_X,        # + bias, + the joined addend
             "wgrad": N * P * Q * X.DENSE_X * X.DENSE_X + X.DENSE_X}                    # over N * P * Q, + the accumulate target
    for entry in entries:
        assert bound[entry] < LIMIT, (entry, bound[entry])
        pr = X.instances(entry, shape, "dense")[0]
        for name in X.ENTRY_OPERANDS[entry]:
            t = pr[name]
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= (X.DENSE_W if name == "w" else X.DENSE_X)
            assert torch.equal(t.to(torch.bfloat16).float(), t)
        for name, top in (("bias", X.DENSE_B), ("addend", X.DENSE_X), ("old", X.DENSE_X)):
            assert torch.equal(pr[name], pr[name].round()) and float(pr[name].abs().max()) <= top
        assert float(pr["exact"].abs().max()) + X.DENSE_B + X.DENSE_X < LIMIT and torch.equal(pr["exact"], pr["exact"].round())


def test_front_probe_stays_below_two_to_the_24():
    """conv2d_front_fwd: h1 = lrelu(conv(x, w1) + b1, 0.25) holds multiples of 0.25; the second reduction in units of 0.25"""
    shape = H.CASES["front"]["shape"]
    for cin in H.CASES["front"]["front"]:
        h1max = cin * X.FRONT_X * X.FRONT_W1 + X.FRONT_B1
        assert (64 * h1max * X.FRONT_W2 + X.FRONT_B2) / X.SLOPE < LIMIT
        pr = X.front_probe(shape, cin)
        assert float(pr["h1"].abs().max()) <= h1max and torch.equal(pr["h1"] * 4, (pr["h1"] * 4).round())
        assert torch.equal(pr["y"].float().double(), pr["y"]) and torch.equal(pr["h1"].float().double(), pr["h1"])
        y32 = torch.nn.functional.conv2d(X.activation(torch.nn.functional.conv2d(pr["x"], pr["w1"], pr["b1"]).double(), 2).float(), pr["w2"], pr["b2"])
        assert torch.equal(y32.double(), pr["y"])


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape,entries", _params())
def test_sparse_probes_have_one_term_per_output_and_every_piece_order_is_exact(shape, entries, bf16):
    for entry in entries:
        for kind in X.KINDS[1:]:
            low, count = 0, 0
            for p in X.instances(entry, shape, kind, bf16):
                ind = {n: (p[n] != 0).float() for n in X.ENTRY_OPERANDS[entry]}
                terms = X.reference(entry, shape, **ind)
                assert float(terms.max()) <= 1.0, (entry, kind, p["inst"], "more than one nonzero term in an output element")
                a, b = _factors(p)
                assert torch.equal(a.double() * b.double(), p["exact"]), (entry, kind, p["inst"])
                pa, pb = X.split3(a), X.split3(b)
                for t, pieces in ((a, pa), (b, pb)):
                    assert torch.equal(pieces[0] + pieces[1] + pieces[2], t)
                    assert torch.equal(pieces[0].double() + pieces[1].double() + pieces[2].double(), t.double())
                if bf16:
                    assert not pa[1].any() and not pb[1].any(), "bf16 tensors: every value is one bfloat16"
                    assert torch.equal(p["exact"].float().to(torch.bfloat16).double(), p["exact"]), "the product is one bfloat16"
                products = [pa[i] * pb[j] for i, j in SIX]
                assert all(torch.equal(q.double(), pa[i].double() * pb[j].double()) for q, (i, j) in zip(products, SIX))
                live = [q for q in products if bool(q.any())]
                if not bf16:
                    if kind == "pair":
                        assert not pa[2].any() and not pb[2].any() and len(live) == 4, (entry, kind, len(live))
                    else:
                        assert not pb[1].any() and len(live) == 3, (entry, kind, len(live))
                exact = p["exact"].float()
                for order, acc in _orders(live):
                    assert torch.equal(acc, exact), (entry, kind, p["inst"], "order", order)
                if kind != "pair":
                    h, m, l = X.split3(p[p["full"]])
                    low += int((l != 0).sum())
                    count += l.numel()
            if kind != "pair" and not bf16:
                print("conv_exact host %s %s %s: width %d, l != 0 in %.1f %% of %d wide values" % (
                    shape, entry, kind, X.WIDTH["carry"], 100.0 * low / count, count))
                assert low >= 0.9 * count, (entry, kind, low, count)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape,entries", _params())
def test_probe_instances_cover_every_tap_filter_and_channel_block(shape, entries, bf16):
    Cin, K, R = shape[3], shape[4], shape[5]
    for entry in entries:
        for kind in X.KINDS[1:]:
            ps = X.instances(entry, shape, kind, bf16)
            cov = X.covered(ps)
            print("conv_exact host %s %s %s %s: %d instance(s), nonzero share of the result %.2f" % (
                shape, entry, kind, "bf16" if bf16 else "f32", len(ps), cov["nonzero"]))
            assert bool(cov["taps"].all()), (entry, kind, cov["taps"])
            assert cov["filters"] == set(range(K)), (entry, kind)
            assert {0, Cin - 1} <= cov["channels"], (entry, kind)
            for blk in range(-(-Cin // 64)):
                assert cov["channels"] & set(range(64 * blk, min(Cin, 64 * blk + 64))), (entry, kind, blk)
            if entry == "wgrad":
                assert all(tuple(p["exact"].shape) == (K, Cin, R, R) and not torch.isnan(p["exact"]).any() for p in ps)
                if kind == "carry-a":
                    assert cov["nonzero"] >= 0.5, (kind, cov["nonzero"])


@pytest.mark.parametrize("cid", ["head3", "s2even", "head21", "stem3"])
def test_coverage_agrees_with_indicator_convolutions_tap_by_tap(cid):
    """coverage() derives the taps from the sparse operand's nonzero positions; here each tap is asked of torch's convolution instead"""
    shape = H.CASES[cid]["shape"]
    K, Cin, R = shape[4], shape[3], shape[5]
    for entry in ENTRIES:
        for kind in ("carry-a", "carry-b"):
            p = X.instances(entry, shape, kind)[0]
            taps = X.coverage(p)[0]
            ind = {n: (p[n] != 0).double() for n in X.ENTRY_OPERANDS[entry]}
            for r in range(R):
                for s in range(R):
                    if entry == "wgrad":
                        hit = bool(X.reference(entry, shape, **ind)[:, :, r, s].any())
                    else:
                        one = dict(ind)
                        one["w"] = torch.zeros_like(ind["w"])
                        one["w"][:, :, r, s] = ind["w"][:, :, r, s]
                        hit = bool(X.reference(entry, shape, **one).any())
                    assert hit == bool(taps[r, s]), (cid, entry, kind, r, s)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape,entries", _params())
def test_fp32_convolution_of_every_probe_equals_the_fp64_one(shape, entries, bf16):
    small = shape[3] <= 64 and shape[5] == 7        # the stem / head cases the extents file runs with reflection padding
    for entry in entries:
        for kind in X.KINDS:
            for p in X.instances(entry, shape, kind, bf16):
                ops = {n: p[n] for n in X.ENTRY_OPERANDS[entry]}
                got = X.reference(entry, shape, dtype=F32, **ops)
                assert torch.equal(got.double(), p["exact"]), (entry, kind, p["inst"])
                assert torch.equal(X.stored(p["exact"], F32).double(), p["exact"])
                if entry == "fwd" and small and kind in ("dense", "carry-a"):
                    r64 = X.reference(entry, shape, reflect=True, **ops)
                    assert torch.equal(X.reference(entry, shape, dtype=F32, reflect=True, **ops).double(), r64)
                    if kind != "dense":
                        terms = X.reference(entry, shape, reflect=True, **{n: (t != 0).float() for n, t in ops.items()})
                        assert float(terms.max()) <= 1.0


def _emulated(p, drop=()):
    """the split contraction on the CPU: the sum over SIX of the entry applied to piece i of the first operand and piece j of the second,
    each exact in fp64; `drop`: piece products left out, or ("l", operand index) = that operand's l piece lost"""
    a, b = X.ENTRY_OPERANDS[p["entry"]]
    pieces = [list(X.split3(p[a])), list(X.split3(p[b]))]
    for d in drop:
        if d[0] == "l":
            pieces[d[1]][2] = torch.zeros_like(pieces[d[1]][2])
    total = torch.zeros_like(p["exact"])
    for i, j in SIX:
        if (i, j) not in drop:
            total = total + X.reference(p["entry"], p["shape"], **{a: pieces[0][i], b: pieces[1][j]})
    return total


@pytest.mark.parametrize("cid", ["k192", "s2odd", "p1x1"])
def test_a_wrong_emulation_passes_the_tolerance_and_fails_the_probe(cid):
    """self-check of the probes (not of the library): with every piece product the emulation equals the reference; with the l piece of
    the carrying operand lost (carry) or m*m left out (pair) it differs, by less than the 2e-5 of the max-norm tests"""
    shape = H.CASES[cid]["shape"]
    for entry in ENTRIES:
        for kind, drop in (("carry-a", (("l", 0),)), ("carry-b", (("l", 1),)), ("pair", ((1, 1),))):
            p = X.instances(entry, shape, kind)[0]
            assert torch.equal(_emulated(p), p["exact"]), (entry, kind)
            wrong = _emulated(p, drop)
            rel = float((wrong - p["exact"]).abs().max() / p["exact"].abs().max())
            share = float((wrong != p["exact"]).sum()) / float((p["exact"] != 0).sum())
            print("conv_exact host %s %s %s: wrong emulation %s differs in %.1f %% of the nonzero elements, max-norm error %.2e" % (
                cid, entry, kind, drop, 100 * share, rel))
            assert 0 < rel < 2e-5 and share > 0.5, (entry, kind, rel, share)
            assert X.mismatch(wrong, p["exact"], "abcd") != "" and X.mismatch(p["exact"], p["exact"], "abcd") == ""


@pytest.mark.parametrize("tid", list(TRANSPOSED))
def test_transposed_convolution_is_the_data_gradient_of_the_mirrored_shape(tid):
    """torch's conv_transpose2d of (the probe's gy, its w read as [Cin, Cout, r, r]) is the probe's exact data gradient"""
    shape, op = TRANSPOSED[tid]
    for kind in X.KINDS:
        p = X.instances("dgrad", shape, kind)[0]
        y = torch.nn.functional.conv_transpose2d(p["gy"].double(), p["w"].double(), None, shape[6], shape[7], op)
        assert torch.equal(y, p["exact"]), (tid, kind)
