"""Connected-component filtering of predicted label maps (sscg_components_filter, `--components`) on a GPU-less host: the numpy / scipy
restatement the GPU test is pinned to (tests/components_reference.py) against literals worked by hand and against an independent
queue-based flood fill; the conditions on the GPU test's random inputs (they must give the filter something to remove, to keep, and
components that cross tile seams); the built cases hold what they were built for; the entries are exported, declared and bound and
return every argument error before any HIP call; the options object, the spec parser, the score keeper's state, the command line."""
import collections
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import components_reference as R
from conftest import ROOT, load_sub

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
ONE = C.c_void_p(16)          # never dereferenced


def u8(rows):
    return np.array(rows, dtype=np.uint8)[None]


# ------------------------------------------------------------------------------------------ the restatement against literals
def test_an_l_shaped_blob_is_one_component_and_a_speck_goes():
    pred = u8([[1, 0, 0, 0, 0],
               [1, 0, 0, 0, 1],
               [1, 1, 1, 0, 0],
               [0, 0, 0, 0, 0]])
    for conn in (4, 8):
        for kw in (dict(min_area=2), dict(largest=True), dict(largest=True, min_area=5)):
            out, hist, st = R.filter_maps(pred, 2, conn=conn, **kw)
            assert hist is None and out[0].tolist() == [[1, 0, 0, 0, 0], [1, 0, 0, 0, 0], [1, 1, 1, 0, 0], [0, 0, 0, 0, 0]]
            assert st[0].tolist() == [[1, 1, 14, 15], [2, 1, 6, 5]]
        assert not R.filter_maps(pred, 2, conn=conn, min_area=6)[0].any()


def test_two_diagonal_pixels_under_both_connectivities():
    pred = u8([[0, 0, 0],
               [0, 1, 0],
               [0, 0, 1]])
    out, _, st = R.filter_maps(pred, 2, conn=4, min_area=2)
    assert not out.any() and st[0].tolist() == [[1, 1, 7, 9], [2, 0, 2, 0]]
    out, _, st = R.filter_maps(pred, 2, conn=8, min_area=2)
    assert np.array_equal(out, pred) and st[0].tolist() == [[1, 1, 7, 7], [1, 1, 2, 2]]
    # under conn 4 `largest` keeps the first of the two single pixels, under conn 8 the pair
    assert R.filter_maps(pred, 2, conn=4, largest=True)[0][0].tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 0]]
    assert np.array_equal(R.filter_maps(pred, 2, conn=8, largest=True)[0], pred)


def test_an_equal_area_tie_goes_to_the_smallest_anchor():
    pred = u8([[0, 0, 0, 2, 2],
               [2, 2, 0, 0, 0],
               [0, 0, 0, 2, 0]])
    out, _, st = R.filter_maps(pred, 3, largest=True)
    assert out[0].tolist() == [[0, 0, 0, 2, 2], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]                 # anchor 3 precedes anchor 5
    assert st[0].tolist() == [[1, 1, 10, 13], [0, 0, 0, 0], [3, 1, 5, 2]]


def test_area_equal_to_min_area_is_kept():
    pred = u8([[1, 1, 1, 0, 1, 1]])
    assert np.array_equal(R.filter_maps(pred, 2, min_area=3)[0], u8([[1, 1, 1, 0, 0, 0]]))
    assert np.array_equal(R.filter_maps(pred, 2, min_area=2)[0], pred)
    assert not R.filter_maps(pred, 2, min_area=4)[0].any()
    assert np.array_equal(R.filter_maps(pred, 2, min_area=0)[0], pred)
    assert np.array_equal(R.filter_maps(pred, 2, largest=True, min_area=4)[0], u8([[0] * 6]))       # the largest is too small: both rules


def test_a_byte_255_passes_through_and_joins_nothing():
    pred = u8([[1, 255, 1, 1],
               [0, 2, 0, 0]])
    out, _, st = R.filter_maps(pred, 2, conn=8, largest=True)
    assert out[0].tolist() == [[0, 255, 1, 1], [0, 2, 0, 0]]                      # 255 and 2 (= C) stay, they split the run of ones
    assert st[0].tolist() == [[2, 2, 3, 4], [2, 1, 3, 2]]


def test_a_void_true_label_is_left_out_of_the_confusion_matrix():
    pred = u8([[1, 1, 0, 1],
               [0, 0, 0, 2]])
    gt = np.array([[[1, 255, 0, 1], [-1, 0, 1, 0]]], dtype=np.int64)
    out, hist, _ = R.filter_maps(pred, 2, conn=4, largest=True, label_true=gt)
    assert out[0].tolist() == [[1, 1, 0, 0], [0, 0, 0, 2]]
    assert hist.tolist() == [[2, 0], [2, 1]] and hist.sum() == 5                  # 8 pixels - 2 void truths - 1 byte >= C
    assert np.array_equal(hist, R.confusion(gt, out, 2))


def test_exempt_classes_and_the_fill_class_are_never_filtered():
    pred = u8([[1, 0, 2, 0, 1, 1, 0, 2, 2]])
    out, _, st = R.filter_maps(pred, 3, largest=True, fill=0, skip=(2,))
    assert out[0, 0].tolist() == [0, 0, 2, 0, 1, 1, 0, 2, 2] and st[0, 2].tolist() == [2, 2, 3, 3]
    out, _, st = R.filter_maps(pred, 3, largest=True, fill=2)
    assert out[0, 0].tolist() == [2, 0, 2, 2, 1, 1, 2, 2, 2]                          # the fill class 2 keeps both of its components
    assert st[0].tolist() == [[3, 1, 3, 1], [2, 1, 3, 2], [2, 2, 3, 6]]
    assert R.exempt_mask(3, 0, (2,)) == 0b101 and R.exempt_mask(64, 63) == 1 << 63


# ------------------------------------------------------------------------------------------ ... and against an independent flood fill
def flood_filter(pred, Cn, conn, largest, min_area, fill, skip):
    out = pred.copy()
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn == 8 else [])
    N, H, W = pred.shape
    for n in range(N):
        seen = np.zeros((H, W), dtype=bool)
        found = collections.defaultdict(list)                                   # class -> [pixels of a component] in anchor order
        for y in range(H):
            for x in range(W):
                if seen[y, x] or pred[n, y, x] >= Cn:
                    continue
                c, queue, comp = pred[n, y, x], collections.deque([(y, x)]), []
                seen[y, x] = True
                while queue:
                    py, px = queue.popleft()
                    comp.append((py, px))
                    for dy, dx in steps:
                        qy, qx = py + dy, px + dx
                        if 0 <= qy < H and 0 <= qx < W and not seen[qy, qx] and pred[n, qy, qx] == c:
                            seen[qy, qx] = True
                            queue.append((qy, qx))
                found[int(c)].append(comp)
        for c, comps in found.items():
            if c == fill or c in skip:
                continue
            best = max(range(len(comps)), key=lambda k: (len(comps[k]), -k))
            for k, comp in enumerate(comps):
                if len(comp) < min_area or (largest and k != best):
                    for py, px in comp:
                        out[n, py, px] = fill
    return out


@pytest.mark.parametrize("case", ["1x1_c4", "1x7_c2", "7x1_c2", "5x9_c4", "33x47_c4", "33x47_c64"])
def test_restatement_equals_a_flood_fill(case):
    N, H, W, Cn, seed, ring = R.RANDOM[case]
    gt, pred = R.make_case(seed, N, H, W, Cn, void_ring=ring)
    pred = pred.copy()
    pred.reshape(-1)[::37] = 255                                                  # and some bytes that belong to no class
    for kw in R.random_settings(Cn):
        full = dict(dict(conn=8, largest=False, min_area=0, fill=0, skip=()), **kw)
        want = flood_filter(pred, Cn, **full)
        got, hist, st = R.filter_maps(pred, Cn, label_true=gt, **kw)
        assert np.array_equal(got, want), (case, kw)
        assert np.array_equal(st[..., R.AFTER], np.stack([[(want[n] == c).sum() for c in range(Cn)] for n in range(N)]))
        assert np.array_equal(hist, R.confusion(gt, want, Cn)) and (got == 255).sum() == (pred == 255).sum()
        assert st[..., R.BEFORE].sum() == (pred < Cn).sum() == st[..., R.AFTER].sum() and (st[..., R.KEPT] <= st[..., R.COMPONENTS]).all()


# ------------------------------------------------------------------------------------------ the GPU test's inputs
BIG = [k for k, v in R.RANDOM.items() if v[0] * v[1] * v[2] >= 1000]


def test_random_cases_cover_the_listed_shapes():
    assert sorted(v[:4] for v in R.RANDOM.values()) == sorted([(2, 1, 1, 4), (3, 1, 7, 2), (1, 7, 1, 2), (2, 5, 9, 4), (3, 33, 47, 4),
                                                               (2, 33, 47, 1), (2, 64, 64, 4), (2, 40, 72, 21), (1, 33, 47, 64),
                                                               (1, 65, 130, 4)])
    assert R.RANDOM["40x72_c21_void"][5] and len(BIG) == 6
    for Cn in (1, 2, 4, 21, 64):
        s = R.random_settings(Cn)
        assert any(k.get("largest") and not k.get("min_area") for k in s) and any(k.get("min_area") == 8 and not k.get("largest") for k in s)
        assert any(k.get("largest") and k.get("min_area") for k in s) and {k.get("conn", 8) for k in s} == {4, 8}
        assert any(k.get("fill", 0) == 0 for k in s) and (Cn == 1 or (any(k.get("fill", 0) > 0 for k in s) and any(k.get("skip") for k in s)))


@pytest.mark.parametrize("case", BIG)
def test_random_cases_do_real_work(case):
    """A condition on the inputs, met by the restatement alone: under `largest` and under min_area = 8 some component is removed and
    some is kept, and some removed and some kept component each have pixels on both sides of a tile seam, for tile edges 16 and 32.
    (With one class, that class is the fill class and nothing can ever be removed: the condition there is that nothing is.)"""
    N, H, W, Cn, seed, ring = R.RANDOM[case]
    pred = R.make_case(seed, N, H, W, Cn, void_ring=ring)[1]
    for kw in (dict(largest=True), dict(min_area=8)):
        if Cn == 1:
            out, _, st = R.filter_maps(pred, Cn, **kw)
            assert np.array_equal(out, pred) and np.array_equal(st[..., R.KEPT], st[..., R.COMPONENTS])
            continue
        for conn in (4, 8):
            for tile in (16, 32):
                got = R.census(pred, Cn, tile, conn=conn, **kw)
                assert min(got.values()) >= 1, (case, kw, conn, tile, got)


def test_built_cases_hold_what_they_were_built_for():
    f = lambda name, k: R.filter_maps(*R.BUILT[name]()[:2], **R.BUILT[name]()[2][k])
    pred, Cn, sets = R.BUILT["serpentine"]()
    assert pred.shape == (2, 70, 70) and np.array_equal(pred[1], pred[0].T)
    for conn in (4, 8):
        for n in (0, 1):
            ids, areas = R.components(pred[n], 1, conn)
            assert areas.tolist() == [35 * 70 + 35]                                      # one component ...
            for edge in (16, 32, 64):                                                    # ... with pixels in every tile
                ty, tx = np.nonzero(ids)[0] // edge, np.nonzero(ids)[1] // edge
                assert len(set(zip(ty.tolist(), tx.tolist()))) == (-(-70 // edge)) ** 2
            assert R.components(pred[n], 0, conn)[1].tolist() == [69] * 35
    out, _, st = f("serpentine", 0)
    assert st[:, 0].tolist() == [[35, 1, 2415, 69]] * 2 and (out[0, 1, :69] == 0).all() and (out[0, 3, 1:] == 2).all()      # first strip
    assert (f("serpentine", 3)[0] == 1).sum() == 2 * 2485 and not (f("serpentine", 4)[0] == 1).any()
    pred, Cn, sets = R.BUILT["u_shape"]()
    for c in (1, 2):
        top = pred[0, :32, :32] if c == 1 else pred[0, 32:, :32]
        assert R.components(top, c, 8)[1].tolist() == ([22, 22] if c == 1 else [22, 22, 1])          # two arms on this side of the seam
        assert sorted(R.components(pred[0], c, 4)[1].tolist()) == [1, 65]                # joined in the whole map
    assert (f("u_shape", 0)[2][0, 1:] == [[2, 1, 66, 65]] * 2).all() and (f("u_shape", 3)[2][0, 1:, R.KEPT] == 0).all()
    pred, Cn, sets = R.BUILT["corners"]()
    for c in (1, 2):
        assert R.components(pred[0], c, 4)[1].tolist() == [1] * 6 and R.components(pred[0], c, 8)[1].tolist() == [2] * 3
    assert np.array_equal(f("corners", 0)[0], pred) and (f("corners", 1)[0] == 0).all()
    keep8, keep4 = f("corners", 2)[0], f("corners", 3)[0]
    assert sorted(zip(*[a.tolist() for a in np.nonzero(keep8[0])])) == [(15, 15), (15, 16), (16, 15), (16, 16)]
    assert sorted(zip(*[a.tolist() for a in np.nonzero(keep4[0])])) == [(15, 15), (15, 16)]
    pred, Cn, sets = R.BUILT["checker"]()
    out4, _, st4 = f("checker", 0)
    assert st4[0].tolist() == [[196, 1, 196, 1], [195, 1, 195, 1], [0, 0, 0, 389]] and out4[0, 0, :3].tolist() == [0, 1, 2]
    assert (out4 == 2).sum() == 389 and np.array_equal(f("checker", 1)[0], pred) and (f("checker", 2)[0] == 2).all()
    assert f("one_class", 0)[2][0, 1].tolist() == [1, 1, 8450, 8450] and not f("one_class", 2)[0].any()
    assert np.array_equal(f("one_class", 1)[0], R.BUILT["one_class"]()[0])
    pred = R.BUILT["sample_border"]()[0]
    assert (pred.reshape(-1)[4 * 40:6 * 40] == 1).all()                                   # 80 contiguous bytes of class 1 ...
    assert np.array_equal(f("sample_border", 1)[0], pred) and not f("sample_border", 2)[0].any()      # ... and two components of 40
    assert f("sample_border", 0)[2][:, 1].tolist() == [[1, 1, 40, 40]] * 2
    out = f("equal_blobs", 0)[0]
    assert (out[0, 6:9, 30:33] == 1).all() and (out == 1).sum() == 9 and (f("equal_blobs", 2)[0] == 1).sum() == 18
    assert not f("equal_blobs", 3)[0].any()
    pred = R.BUILT["holes"]()[0]
    assert R.components(pred[0], 1, 8)[1].tolist() == [98, 98]
    for k in range(5):
        out = f("holes", k)[0]
        assert np.array_equal(out[pred >= 2], pred[pred >= 2]) and (pred == 255).sum() == 13 and (pred == 2).sum() == 2
    assert (f("holes", 0)[0][0, 5:15, 4:14] > 0).all() and not (f("holes", 0)[0][0, 5:15, 15:25] == 1).any()
    assert np.array_equal(f("holes", 2)[0], pred) and not (f("holes", 3)[0] == 1).any()


# ------------------------------------------------------------------------------------------ options, parser, state
def test_component_options():
    F = load_sub("functional")
    o = F.ComponentOptions()
    assert (o.largest, o.min_area, o.conn, o.fill, o.skip) == (False, 0, 8, 0, ())
    assert F.ComponentOptions(largest=True, skip=[3, 1, 3]) == F.ComponentOptions(True, 0, 8, 0, (1, 3))
    assert F.ComponentOptions(min_area=8) != F.ComponentOptions(min_area=9) and F.ComponentOptions() != F.ComponentOptions(conn=4)
    assert F.ComponentOptions(fill=1) != F.ComponentOptions() and F.ComponentOptions(largest=True) != F.ComponentOptions()
    assert F.ComponentOptions() != None and "min_area=8" in repr(F.ComponentOptions(min_area=8))          # noqa: E711
    assert F.ComponentOptions(fill=2, skip=(0, 5)).exempt_mask(21) == 0b100101 and F.ComponentOptions().exempt_mask(4) == 1
    assert F.ComponentOptions(fill=63).exempt_mask(64) == 1 << 63
    for bad in (dict(largest=2), dict(largest="yes"), dict(min_area=-1), dict(min_area=1.5), dict(min_area=True), dict(min_area=2 ** 31),
                dict(conn=6), dict(conn=True), dict(conn="8"), dict(fill=-1), dict(fill=64), dict(fill=1.0), dict(skip=(64,)),
                dict(skip=(-1,)), dict(skip=(1.5,)), dict(skip=3)):
        with pytest.raises(ValueError):
            F.ComponentOptions(**bad)
    for Cn, o in ((4, F.ComponentOptions(fill=4)), (4, F.ComponentOptions(skip=(4,))), (0, F.ComponentOptions()), (65, F.ComponentOptions())):
        with pytest.raises(ValueError):
            o.exempt_mask(Cn)


def test_parse_components_table():
    F, U = load_sub("functional"), load_sub("utils")
    P, O = U.parse_components, F.ComponentOptions
    assert P("") is None and P(None) is None and P("  ") is None
    assert P("on") == O(min_area=64) and P(" on ") == O(False, 64, 8, 0, ())
    assert P("largest") == O(largest=True) and P("min_area=8") == O(min_area=8) and P("largest,min_area=16") == O(True, 16)
    assert P("min_area=8, conn=4 ,fill=3,skip=1:2") == O(False, 8, 4, 3, (1, 2)) and P("skip=7,largest") == O(largest=True, skip=(7,))
    assert P("largest,min_area=0") == O(largest=True)
    for spec, token in (("off", "off"), ("largest=1", "largest=1"), ("min_area", "min_area"), ("min_area=", "min_area="),
                        ("min_area=x", "min_area=x"), ("min_area=-1", "min_area=-1"), ("min_area=2.5", "min_area=2.5"),
                        ("largest,conn=6", "conn=6"), ("largest,fill=64", "fill=64"), ("largest,fill=-1", "fill=-1"),
                        ("largest,skip=a", "skip=a"), ("largest,skip=1:", "skip=1:"), ("largest,skip=64", "skip=64"),
                        ("largest,largest", "largest"), ("min_area=2,min_area=3", "min_area=3"), ("on,largest", "on"),
                        ("LARGEST", "LARGEST"), ("largest,", ""), ("conn=4", "conn=4"), ("fill=1,skip=2", "fill=1,skip=2")):
        with pytest.raises(ValueError) as e:
            P(spec)
        assert repr(token) in str(e.value) and "--components" in str(e.value), (spec, str(e.value))
    assert "untuned" in P.__doc__


def test_running_score_holds_the_option_as_state():
    F, U = load_sub("functional"), load_sub("utils")
    rs = U.runningScore(4, "acdc")
    assert rs.get_components() is None and rs.get_component_scores() is None
    opts = F.ComponentOptions(largest=True, skip=(3,))
    rs.set_components(opts)
    assert rs.get_components() == opts
    s = rs.get_component_scores()                               # nothing filtered yet
    assert s["components"] == s["kept_components"] == s["removed_pixels"] == 0 and s["class_components"] == {0: 0, 1: 0, 2: 0, 3: 0}
    assert set(s) == {"components", "kept_components", "removed_pixels", "class_components", "class_kept_components", "class_removed_pixels"}
    rs.reset()
    assert rs.get_components() == opts                          # reset() clears the kept stats, not the option
    with pytest.raises(TypeError):
        rs.set_components("largest")
    with pytest.raises(ValueError):
        rs.set_components(F.ComponentOptions(largest=True, fill=4))              # not a class of this score keeper
    with pytest.raises(ValueError):
        rs.set_components(F.ComponentOptions(largest=True, skip=(9,)))
    assert rs.get_components() == opts
    rs.set_components(None)
    assert rs.get_components() is None and rs.get_component_scores() is None and rs.get_surface() is None and rs.get_boundary() is None
    rs.update([np.array([[0, 1], [2, 255]])], [np.array([[0, 1], [1, 3]])])        # the host path is as it was
    assert rs.confusion_matrix.sum() == 3


# ------------------------------------------------------------------------------------------ the entries, the wrapper, the drivers
def test_entries_are_exported_declared_and_bound():
    L = load_sub("_lib")
    hdr = open(os.path.join(ROOT, "include", "sscg.h")).read()
    flat = " ".join(hdr.split())
    assert "size_t sscg_components_workspace(int N, int H, int W, int C);" in flat
    assert ("int sscg_components_filter(const uint8_t* label_pred, const int64_t* label_true /*nullable*/, int N, int H, int W, int C, "
            "int conn, int largest, int min_area, int fill, uint64_t exempt_mask, uint8_t* label_out, int64_t* hist /*nullable, "
            "accumulated*/, int64_t* stats /*nullable, overwritten*/, void* ws, size_t ws_bytes, void* stream);") in flat
    block = hdr[hdr.index("connected-component filtering of predicted label maps"):hdr.index("size_t sscg_components_workspace(")]
    assert "the reference has no such step" in block and "SSCG_ABI_VERSION stays 18" in " ".join(block.replace(" * ", " ").split())
    assert len(L.SIGNATURES["sscg_components_filter"][1]) == 17 and len(L.SIGNATURES["sscg_components_workspace"][1]) == 4
    assert L.SIGNATURES["sscg_components_filter"][1][10] is C.c_uint64 and L.SIGNATURES["sscg_components_workspace"][0] is C.c_size_t
    assert callable(L.lib.sscg_components_filter) and callable(L.lib.sscg_components_workspace)
    assert L.ABI_VERSION == 18 and L.lib.sscg_abi_version() == 18 and "#define SSCG_ABI_VERSION 18" in hdr          # an addition
    mk = open(os.path.join(ROOT, "semi-supervised-segmentation-cyclegan_amd", "csrc", "Makefile")).read()
    assert "components.hip" in [l for l in mk.splitlines() if l.startswith("SRCS")][0].split()


def test_workspace_size_follows_the_documented_layout():
    lib = load_sub("_lib").lib
    up = lambda b: -(-b // 256) * 256
    for (N, H, W, Cn) in ((1, 1, 1, 1), (2, 33, 47, 4), (8, 256, 256, 21), (16, 512, 1024, 20), (1, 7, 5, 64)):
        pix = N * H * W
        assert lib.sscg_components_workspace(N, H, W, Cn) == 2 * up(4 * pix) + up(8 * N * Cn), (N, H, W, Cn)
    for refused in ((0, 5, 5, 4), (1, 0, 5, 4), (1, 5, -1, 4), (1, 5, 5, 0), (1, 5, 5, 65), (1, 32768, 65536, 4), (2, 32768, 32768, 4),
                    (1 << 30, 1 << 30, 1 << 30, 4)):
        assert lib.sscg_components_workspace(*refused) == 0, refused
    assert lib.sscg_components_workspace(1, 32768, 65535, 4) > 0                      # 2^31 - 2^15 pixels: the last size accepted


def test_argument_errors_are_returned_before_any_launch():
    lib = load_sub("_lib").lib

    def call(lp=ONE, lt=ONE, N=1, H=5, W=5, Cn=4, conn=8, largest=1, min_area=0, fill=0, mask=0, out=ONE, hist=ONE, stats=ONE, ws=ONE,
             ws_bytes=1 << 40):
        return lib.sscg_components_filter(lp, lt, N, H, W, Cn, conn, largest, min_area, fill, mask, out, hist, stats, ws, ws_bytes, None)

    for ptr in ("lp", "out", "ws"):
        assert call(**{ptr: None}) == BAD_ARG, ptr
    assert call(lt=None) == BAD_ARG                                                    # hist without label_true
    for size in ("N", "H", "W"):
        assert call(**{size: 0}) == BAD_ARG and call(**{size: -3}) == BAD_ARG, size
    assert call(Cn=0) == BAD_ARG and call(Cn=65) == BAD_ARG and call(Cn=-4) == BAD_ARG
    assert call(conn=0) == BAD_ARG and call(conn=6) == BAD_ARG and call(conn=-8) == BAD_ARG and call(conn=12) == BAD_ARG
    assert call(largest=2) == BAD_ARG and call(largest=-1) == BAD_ARG
    assert call(min_area=-1) == BAD_ARG and call(fill=-1) == BAD_ARG and call(fill=4) == BAD_ARG and call(Cn=64, fill=64) == BAD_ARG
    assert call(mask=1 << 4) == BAD_ARG and call(mask=1 << 63) == BAD_ARG and call(Cn=63, mask=1 << 63) == BAD_ARG
    assert call(N=2, H=32768, W=32768) == UNSUPPORTED and call(N=1, H=1 << 16, W=1 << 15) == UNSUPPORTED          # N*H*W >= 2^31
    assert call(N=1 << 30, H=1 << 30, W=1 << 30) == UNSUPPORTED                                                    # and no overflow on the way
    assert call(N=2, H=32768, W=32768, conn=5) == BAD_ARG and call(N=2, H=32768, W=32768, mask=16) == BAD_ARG      # argument errors first
    need = lib.sscg_components_workspace(1, 5, 5, 4)
    assert need > 0 and call(ws_bytes=need - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE                     # one byte short
    need = lib.sscg_components_workspace(3, 33, 47, 21)
    assert call(N=3, H=33, W=47, Cn=21, ws_bytes=need - 1) == WORKSPACE
    # what is allowed reaches the workspace check: the nullable pointers, every bit below C, C = 64 with the top bit, min_area at its top
    assert call(lt=None, hist=None, ws_bytes=0) == WORKSPACE and call(hist=None, ws_bytes=0) == WORKSPACE and call(stats=None, ws_bytes=0) == WORKSPACE
    assert call(mask=0b1111, ws_bytes=0) == WORKSPACE and call(Cn=64, mask=(1 << 64) - 1, fill=63, ws_bytes=0) == WORKSPACE
    assert call(conn=4, largest=0, min_area=2 ** 31 - 1, fill=3, ws_bytes=0) == WORKSPACE


def test_wrapper_refuses_cpu_tensors_and_the_drivers_take_the_option():
    F, L, U, md = load_sub("functional"), load_sub("_lib"), load_sub("utils"), load_sub("model")
    lt, lp = torch.zeros(1, 5, 5, dtype=torch.int64), torch.zeros(1, 5, 5, dtype=torch.uint8)
    with pytest.raises(L.SscgError):
        F.component_filter(lp, 4, F.ComponentOptions(largest=True))                         # no CPU fallback
    with pytest.raises(L.SscgError):
        F.component_filter(lp, 4, F.ComponentOptions(largest=True), label_true=lt)
    sig = inspect.signature(F.component_filter)
    assert list(sig.parameters) == ["label_pred", "num_classes", "options", "label_true", "hist", "out", "stats"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("label_true", "hist", "out", "stats"))
    for cls in (md.semisuper_cycleGAN, md.supervised_model):
        assert list(inspect.signature(cls.evaluate).parameters) == ["self", "val_loader", "first_batch", "tta", "crf", "boundary"]
        assert callable(cls.set_components) and list(inspect.signature(cls.set_components).parameters) == ["self", "opts"]
    for name in ("set_components", "get_components", "get_component_scores"):
        assert callable(getattr(U.runningScore, name))


def test_main_takes_components_and_moves_no_other_default(capsys):
    sys.path.insert(0, ROOT)
    import main
    a = main.get_args([])
    assert a.components == "" and "components" not in vars(a)           # an absent flag leaves the namespace as it always was
    b = main.get_args(["--components", "largest"])
    assert b.components == "largest" and set(vars(b)) - set(vars(a)) == {"components"}
    rest = dict(vars(b))
    del rest["components"]
    assert rest == vars(a)
    assert main.get_args(["--components", "on"]).components == "on"
    old = ["--dataset", "acdc", "--tta", "0.5,1.0:flip", "--crf", "on", "--boundary", "on", "--surface", "on", "--batch_size", "4"]
    assert vars(main.get_args(old + ["--components", "largest,min_area=8,fill=0,skip=3"])).items() >= vars(main.get_args(old)).items()
    assert "components" not in vars(main.get_args(old))
    for bad in ("zap", "min_area=-1", "conn=4", "largest,conn=5", "largest,skip=x", "fill=2"):
        with pytest.raises(SystemExit):
            main.get_args(["--components", bad])
    # fill and skip are checked against the dataset's class count: 4 (acdc), 20 (cityscapes), 21 (voc2012, the default)
    for dataset, ok, bad in (("acdc", "3", "4"), ("cityscapes", "19", "20"), ("voc2012", "20", "21")):
        for key in ("fill=", "skip=0:"):
            assert main.get_args(["--dataset", dataset, "--components", "largest," + key + ok]).components.endswith(ok)
            with pytest.raises(SystemExit):
                main.get_args(["--dataset", dataset, "--components", "largest," + key + bad])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        main.get_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--components SPEC" in text
    assert "combines with --tta, --crf, --boundary, --surface and --ema_decay" in text[text.index("--components SPEC"):]
