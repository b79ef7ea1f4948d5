#!/usr/bin/env python
"""Golden answers of the convolution families' host-side plans (tests/golden/g10_conv_plans.json, read by tests/test_conv_plan_host.py).

Needs no GPU and no reference: it asks a built libsscg.so the size and applicability queries of include/sscg.h - workspace bytes, record
bytes of the fused statistics / backward sums, which fusions apply - for every convolution shape of the three bench shape lists and a few
small edge shapes, under every weight / tensor dtype combination and every forced tile class and forced split of `tuning`.  These queries
make no HIP call.  Where a workspace query is positive the matching compute entry is called with a NULL workspace and never-dereferenced
pointers: it must refuse before any launch - SSCG_ERR_WORKSPACE, or SSCG_ERR_UNSUPPORTED where no family computes that dtype
combination (the query then answered for the exact family's plan).  No other compute entry is called, and none for the 1x1 shapes
with a handful of channels on one side: the streaming kernels that serve them take no workspace and would launch.

The fixture pins the plans across a change of the host code: generate it with SSCG_LIB pointing at a library built from the commit
whose decisions are to be kept (and the SSCG_KS_* tuning variables unset).
Usage: SSCG_LIB=/path/to/libsscg.so python tests/golden/gen_conv_plans.py
"""
import ctypes as C
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

SHAPE_FILES = ("bench_conv_shapes.txt", "bench_conv_shapes_c3.txt", "bench_conv_shapes_c5.txt")
# (N, H, W, C, K, R, stride, pad, dil): odd stride-2 maps (a parity class with a different extent per axis, one with a single tap), a
# 4x4 stride-2 kernel, the split tail of a dilated 3x3, a 21-channel head on a long reduction, a short 1x1
EDGE_SHAPES = ((2, 17, 15, 64, 64, 3, 2, 1, 1), (2, 16, 16, 64, 128, 4, 2, 1, 1), (8, 33, 33, 256, 256, 3, 1, 2, 2),
               (2, 33, 33, 2048, 21, 3, 1, 12, 12), (1, 64, 64, 64, 32, 1, 1, 0, 1))
F32, BF16, BF16X3 = 0, 1, 2
# (family that serves the dtype triple, (x, w, y) dtypes, number of tile classes `tuning` can force)
FAMILIES = (("exact", (F32, F32, F32), 9), ("split", (F32, BF16X3, F32), 4), ("bf16", (BF16, BF16, BF16), 6), ("bf16", (BF16, BF16, F32), 6))
QUERIES = ("fwd_workspace", "dgrad_workspace", "fwd_stats_bytes_GN", "fwd_stats_bytes_G1", "dgrad_bsums_bytes_GN", "dgrad_bsums_bytes_G1",
           "split_applies_fwd", "split_applies_dgrad", "fwd_affine_applies", "front_applies_3", "front_applies_4", "front_applies_20",
           "front_applies_21", "dgrad_add_applies")
# the families a query can answer differently for (split_applies looks at the geometry alone)
SERVED = {q: ("exact", "split", "bf16") for q in QUERIES}
for _q in ("dgrad_bsums_bytes_GN", "dgrad_bsums_bytes_G1", "fwd_affine_applies", "dgrad_add_applies"):
    SERVED[_q] = ("split", "bf16")
for _q in ("front_applies_3", "front_applies_4", "front_applies_20", "front_applies_21"):
    SERVED[_q] = ("split",)
REFUSALS = ("fwd", "dgrad", "fwd_affine")       # compute entries called without the workspace their plan needs
ERR_UNSUPPORTED, ERR_WORKSPACE = -2, -3


def tunings(n_classes):
    """the library's own plan, every forced tile class, never split, every tile cut in three"""
    return [0] + list(range(1, n_classes + 1)) + [0x100, 0x300]


def shapes():
    out = set(EDGE_SHAPES)
    for name in SHAPE_FILES:
        for line in open(os.path.join(HERE, name)):
            m = re.match(r"(\d+)x(\d+)x(\d+) c(\d+) k(\d+) r(\d+) s(\d+) p(\d+) d(\d+)", line.strip())
            if m:
                out.add(tuple(int(v) for v in m.groups()))
    return sorted(out)


def desc(L, shape, dtypes, tuning):
    N, H, W, Cin, K, R, s, p, d = shape
    P = (H + 2 * p - d * (R - 1) - 1) // s + 1
    Q = (W + 2 * p - d * (R - 1) - 1) // s + 1
    return L.ConvDesc(N=N, H=H, W=W, C=Cin, K=K, R=R, S=R, P=P, Q=Q, stride=s, pad=p, dil=d, pad_mode=0, act=0, slope=0.0,
                      x_dtype=dtypes[0], w_dtype=dtypes[1], y_dtype=dtypes[2], precision=0, tuning=tuning)


def ask(L, d):
    """-> (answers in QUERIES order, {entry: return code} of the compute entries that had to refuse a NULL workspace)"""
    lib, r = L.lib, C.byref(d)
    a = [lib.sscg_conv2d_fwd_workspace(r), lib.sscg_conv2d_dgrad_workspace(r),
         lib.sscg_conv2d_fwd_stats_bytes(r, d.N, d.P * d.Q), lib.sscg_conv2d_fwd_stats_bytes(r, 1, d.N * d.P * d.Q),
         lib.sscg_conv2d_dgrad_bsums_bytes(r, d.N, d.H * d.W), lib.sscg_conv2d_dgrad_bsums_bytes(r, 1, d.N * d.H * d.W),
         lib.sscg_conv2d_split_applies(r, 0), lib.sscg_conv2d_split_applies(r, 1), lib.sscg_conv2d_fwd_affine_applies(r)]
    a += [lib.sscg_conv2d_front_applies(r, cin) for cin in (3, 4, 20, 21)]
    a.append(lib.sscg_conv2d_dgrad_add_applies(r))
    one = C.c_void_p(16)        # never dereferenced
    rc = {}
    if d.R == 1 and (d.K <= 4 or d.C <= 32):        # conv_thin.hip's territory: no workspace check in front of its launch
        return a, rc
    if a[0] > 0:
        rc["fwd"] = lib.sscg_conv2d_fwd(r, one, one, None, one, None, 0, None)
        if a[8]:                # the folded forward runs the plain forward's plan
            rc["fwd_affine"] = lib.sscg_conv2d_fwd_affine(r, one, one, None, one, one, 1e-5, None, None, None, one, None, 0, None)
    if a[1] > 0:
        rc["dgrad"] = lib.sscg_conv2d_dgrad(r, one, one, None, one, 0, 0.0, None, 0, None)
    return a, rc


def collect(L, all_shapes):
    """answers[family entry][tuning][query] = one value per shape; refusals[...][entry] = [[shape index, return code], ...]"""
    answers, refusals = [], []
    for _, dtypes, n_classes in FAMILIES:
        fa, fr = [], []
        for t in tunings(n_classes):
            cols = [[] for _ in QUERIES]
            ref = {e: [] for e in REFUSALS}
            for i, shape in enumerate(all_shapes):
                a, rc = ask(L, desc(L, shape, dtypes, t))
                for col, v in zip(cols, a):
                    col.append(int(v))
                for e, v in rc.items():
                    ref[e].append([i, int(v)])
            fa.append(cols)
            fr.append(ref)
        answers.append(fa)
        refusals.append(fr)
    return answers, refusals


def vacuous(answers):
    """queries with one distinct answer over all descriptors of a family that serves them"""
    seen = {}
    for (family, _, _), fa in zip(FAMILIES, answers):
        for cols in fa:
            for q, col in zip(QUERIES, cols):
                if family in SERVED[q]:
                    seen.setdefault((q, family), set()).update(col)
    return sorted(k for k, v in seen.items() if len(v) < 2)


def main():
    assert not [k for k in os.environ if k.startswith("SSCG_KS_")], "unset the SSCG_KS_* tuning variables"
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import importlib
    L = importlib.import_module("semi-supervised-segmentation-cyclegan_amd._lib")
    all_shapes = shapes()
    answers, refusals = collect(L, all_shapes)
    dull = vacuous(answers)
    assert not dull, "one distinct answer only: %s" % dull
    n_ref = 0
    for fr in refusals:
        for ref in fr:
            for e, pairs in ref.items():
                bad = [p for p in pairs if p[1] not in (ERR_WORKSPACE, ERR_UNSUPPORTED)]
                assert not bad, "%s did not refuse a NULL workspace: %s" % (e, bad)
                n_ref += sum(p[1] == ERR_WORKSPACE for p in pairs)
    assert n_ref > 0
    out = {"library": os.path.basename(L.LIB_PATH), "shapes": [list(s) for s in all_shapes],
           "families": [[f, list(dt), tunings(n)] for f, dt, n in FAMILIES], "queries": list(QUERIES), "answers": answers,
           "refusals": refusals}
    path = os.path.join(HERE, "g10_conv_plans.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s (%d bytes): %d shapes, %d descriptors, %d calls refused for their workspace, library %s" % (
        path, os.path.getsize(path), len(all_shapes), len(all_shapes) * sum(len(tunings(n)) for _, _, n in FAMILIES), n_ref, L.LIB_PATH))


if __name__ == "__main__":
    main()
