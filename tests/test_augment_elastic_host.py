"""Elastic deformation in the device batch finish, the parts that need no GPU: the B-spline numerators, the lattices `Compose.fields`
draws, the `--augment elastic=` item, the host path (`Compose.__call__`, the integer definition in numpy) against the restatement
of tests/elastic_reference.py, the C entry's declaration and argument checks, and the wrapper's."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import ROOT, load_sub
from elastic_reference import D, coordinates, displacement, elastic_reference, integers, lattice_shape, numerators
from test_augment_colour_host import colour_reference
from test_augment_host import warp_reference


def _aug():
    return load_sub("data_utils.augmentations")


class _Fixed:
    """A generator whose every draw is the given value."""

    def __init__(self, v):
        self.v = v

    def uniform(self, lo, hi, size=None):
        return self.v if size is None else np.full(size, self.v, dtype=np.float64)

    def random_sample(self):
        return self.v


# ------------------------------------------------------------------------------------------------ the weights
def test_numerators_sum_to_the_denominator_are_non_negative_and_mirror():
    t = np.arange(256, dtype=np.int64)
    for n in (numerators(t), list(_aug().bspline_numerators(t))):
        assert D == 6 * 2 ** 24 == _aug().BSPLINE_DENOM
        assert (n[0] + n[1] + n[2] + n[3] == D).all()
        assert all((k >= 0).all() and int(k.max()) < 2 ** 31 for k in n)
        for k in range(4):
            assert np.array_equal(n[k][1:], n[3 - k][256 - t[1:]])           # n_k(t) == n_{3-k}(256 - t), t in 1..255
    assert [int(k[0]) for k in numerators(t)] == [2 ** 24, 4 * 2 ** 24, 2 ** 24, 0]     # t = 0: (1, 4, 1, 0) / 6


def test_restatement_of_a_zero_and_a_constant_lattice():
    """The two properties of the definition, on the restatement itself: a zero lattice displaces nothing, a constant one by the constant
    (the weights sum to D exactly, whatever the sign), and a lattice linear in the node index gives a displacement linear in the pixel."""
    OH, OW, grid = 17, 21, 7
    gh, gw = lattice_shape(grid, OH, OW)
    assert (gh, gw) == (6, 6)
    dx, dy = displacement(np.zeros((gh, gw, 2), dtype=np.int32), grid, OH, OW)
    assert not dx.any() and not dy.any()
    const = np.empty((gh, gw, 2), dtype=np.int32)
    const[..., 0], const[..., 1] = 3 * 65536 + 1234, -70000
    dx, dy = displacement(const, grid, OH, OW)
    assert (dx == 3 * 65536 + 1234).all() and (dy == -70000).all()
    # node value 6 * 256 * 7 * (index - 1): a cubic B-spline reproduces linear functions, here exactly (every product is a multiple of D)
    ramp = np.zeros((gh, gw, 2), dtype=np.int64)
    ramp[..., 0] = 6 * 256 * 7 * (np.arange(gw) - 1)[None, :]
    dx, dy = displacement(ramp, grid, OH, OW)
    ox = np.arange(OW)
    assert np.array_equal(dx[0], 6 * 256 * 7 * (ox // grid) + 6 * 7 * (((ox % grid) * 256) // grid)) and not dy.any()


def test_restatement_with_a_zero_lattice_equals_the_affine_restatements():
    rng = np.random.RandomState(70)
    img, gt = rng.randint(0, 256, (2, 11, 13, 3), dtype=np.uint8), rng.randint(0, 34, (2, 11, 13)).astype(np.uint8)
    mats = np.array([[65536, 0, 0, 0, 65536, 0], [40000, -9000, 3 * 65536 + 77, 9000, 40000, -65536]], dtype=np.int32)
    lut = load_sub("data_utils").label_table("cityscapes").numpy()
    mean, std = [0.4, 0.5, 0.6], [0.2, 0.5, 0.3]
    zero = np.zeros((2,) + lattice_shape(4, 7, 9) + (2,), dtype=np.int32)
    want, wl = warp_reference(img, gt, mats, (7, 9), mean, std, lut, 77, 250)
    for nodes in (None, zero):
        got, gl = elastic_reference(img, gt, mats, nodes, 4, (7, 9), mean, std, lut, 77, 250)
        assert np.array_equal(got, want) and np.array_equal(gl, wl)
    tables = np.random.RandomState(71).uniform(-0.5, 1.2, (2, 21)).astype(np.float32)
    for need_mean in (False, True):
        want, wl = colour_reference(img, gt, mats, tables, need_mean, (7, 9), mean, std, lut, 77, 250)
        got, gl = elastic_reference(img, gt, mats, zero, 4, (7, 9), mean, std, lut, 77, 250, colours=tables, need_mean=need_mean)
        assert np.array_equal(got, want) and np.array_equal(gl, wl)
    only, none = elastic_reference(img, None, mats, zero, 4, (7, 9), mean, std, None, 77, 250)
    assert none is None and np.array_equal(only, warp_reference(img, None, mats, (7, 9), mean, std, None, 77, 250)[0])


def test_product_displacement_equals_the_restatement():
    A = _aug()
    rng = np.random.RandomState(3)
    for grid, (OH, OW) in ((4, (17, 21)), (7, (17, 21)), (64, (17, 21)), (16, (40, 50))):
        gh, gw = lattice_shape(grid, OH, OW)
        assert A.lattice_shape(grid, OH, OW) == (gh, gw)
        nodes = rng.randint(-6 * 65536, 6 * 65536 + 1, (gh, gw, 2)).astype(np.int32)
        dx, dy = displacement(nodes, grid, OH, OW)
        d = A.elastic_displacement(nodes, grid, OH, OW)
        assert d.dtype == np.int64 and np.array_equal(d[..., 0], dx) and np.array_equal(d[..., 1], dy)
        assert np.abs(d).max() <= np.abs(nodes).max()                         # a convex combination, rounded to nearest


# ------------------------------------------------------------------------------------------------ fields
def test_fields_shape_range_and_none_without_an_elastic_op():
    A = _aug()
    plain = A.from_spec("hflip,rotate=10", (24, 32), out_size=(24, 32))
    mats = plain.matrices(np.random.RandomState(1), 3, 50, 40)
    assert plain.fields(np.random.RandomState(2), 3, 50, 40, mats) is None
    for spec, grid, (oh, ow) in (("elastic=6:16", 16, (24, 32)), ("elastic=1.5:4", 4, (17, 21)), ("elastic=2:7", 7, (17, 21)),
                                 ("elastic=12", 32, (65, 64))):
        comp = A.from_spec(spec, (oh, ow), out_size=(oh, ow))
        ident = comp.matrices(np.random.RandomState(1), 3, ow, oh)
        assert ident.tolist() == [[65536, 0, 0, 0, 65536, 0]] * 3
        nodes, g = comp.fields(np.random.RandomState(2), 3, ow, oh, ident)
        gh, gw = (oh - 1) // grid + 4, (ow - 1) // grid + 4
        assert g == grid and nodes.dtype == np.int32 and nodes.shape == (3, gh, gw, 2)
        alpha = comp.elastic_ops[0].alpha
        assert np.abs(nodes).max() <= alpha * 65536 and np.abs(nodes).max() > 0.8 * alpha * 65536
        assert len({r.tobytes() for r in nodes}) == 3                         # one lattice per sample
        again, _ = comp.fields(np.random.RandomState(2), 3, ow, oh, ident)
        assert np.array_equal(nodes, again)
    # without an out_size the lattice lies over the input's size
    nodes, _ = A.from_spec("elastic=2:8", (24, 32)).fields(np.random.RandomState(2), 1, 32, 24, ident[:1])
    assert nodes.shape == (1, 23 // 8 + 4, 31 // 8 + 4, 2)


def test_fields_fold_the_linear_part_of_each_map():
    """Offsets of +alpha in x and y (output pixels) under a flip and under a map that zooms by 2 (source = 2 x output)."""
    A = _aug()
    comp = A.Compose([A.RandomElastic(3.0, 8)], out_size=(16, 24))
    flip = A.to_q16(A.RandomHorizontallyFlip(1.0).matrix(np.random.RandomState(0), 24, 16)[0])
    zoom = A.to_q16(A.Scale(24).matrix(np.random.RandomState(0), 48, 32)[0])
    shear = np.array([65536, 16384, 0, -32768, 65536, 0], dtype=np.int32)
    assert flip.tolist()[:2] == [-65536, 0] and zoom.tolist()[0] == zoom.tolist()[4] == 2 * 65536
    nodes, grid = comp.fields(_Fixed(3.0), 3, 24, 16, np.stack([flip, zoom, shear]))
    assert grid == 8 and nodes.shape == (3, 5, 6, 2)
    assert (nodes[0, ..., 0] == -3 * 65536).all() and (nodes[0, ..., 1] == 3 * 65536).all()
    assert (nodes[1] == 6 * 65536).all()
    assert (nodes[2, ..., 0] == 3 * 65536 + 3 * 16384).all() and (nodes[2, ..., 1] == -3 * 32768 + 3 * 65536).all()
    # rounding to nearest of the float64 product
    odd = np.array([[21845, 0, 0, 0, 21846, 0]], dtype=np.int32)
    nodes, _ = comp.fields(_Fixed(0.5), 1, 24, 16, odd)
    assert (nodes[0, ..., 0] == int(np.rint(21845 * 0.5))).all() and (nodes[0, ..., 1] == 10923).all()


def test_fields_refuse_nodes_beyond_the_lattice_range():
    A = _aug()
    comp = A.Compose([A.RandomElastic(12.0, 32)], out_size=(16, 24))
    big = np.array([[90 * 65536, 0, 0, 0, 65536, 0]], dtype=np.int32)         # 12 output pixels = 1080 source pixels >= 2^26 / 2^16
    with pytest.raises(ValueError):
        comp.fields(_Fixed(12.0), 1, 24, 16, big)
    ok = np.array([[85 * 65536, 0, 0, 0, 65536, 0]], dtype=np.int32)          # 1020 source pixels
    nodes, _ = comp.fields(_Fixed(12.0), 1, 24, 16, ok)
    assert int(nodes.max()) == 1020 * 65536 < 2 ** 26


def test_elastic_draws_leave_the_matrix_and_colour_streams_alone():
    A = _aug()
    assert A.ELASTIC_SEED_OFFSET != A.COLOUR_SEED_OFFSET == 500 and A.ELASTIC_SEED_OFFSET != 0
    plain = A.from_spec("hflip,rotate=10,scale=0.5:2,brightness=0.4,contrast=0.3", (24, 32), out_size=(24, 32))
    for spec in ("elastic=6:16,hflip,rotate=10,scale=0.5:2,brightness=0.4,contrast=0.3", "hflip,rotate=10,elastic=6:16,scale=0.5:2,brightness=0.4,contrast=0.3",
                 "hflip,rotate=10,scale=0.5:2,brightness=0.4,contrast=0.3,elastic=6:16"):
        mixed = A.from_spec(spec, (24, 32), out_size=(24, 32))
        a, b = plain.matrices(np.random.RandomState(5), 6, 50, 40), mixed.matrices(np.random.RandomState(5), 6, 50, 40)
        assert np.array_equal(a, b) and len({tuple(r) for r in a.tolist()}) == 6
        ta, tb = plain.colours(np.random.RandomState(505), 6, 3), mixed.colours(np.random.RandomState(505), 6, 3)
        assert np.array_equal(ta[0], tb[0]) and ta[1] == tb[1]
        assert [type(o).__name__ for o in mixed.geometric_ops] == ["RandomHorizontallyFlip", "RandomRotate", "RandomScale"]
    # the host path seeds three generators
    one = A.from_spec("rotate=10,brightness=0.4,elastic=3:8", (24, 32), seed=5)
    off = A.ELASTIC_SEED_OFFSET
    assert one.rng.uniform() == np.random.RandomState(5).uniform() and one.colour_rng.uniform() == np.random.RandomState(505).uniform()
    assert one.elastic_rng.uniform() == np.random.RandomState(5 + off).uniform()


# ------------------------------------------------------------------------------------------------ the spec
def test_from_spec_takes_the_elastic_item_and_refuses_bad_ones():
    A = _aug()
    comp = A.from_spec("hflip, elastic=6:16 ,rotate=10", (32, 48), out_size=(32, 48))
    assert [type(o).__name__ for o in comp.ops] == ["RandomHorizontallyFlip", "RandomElastic", "RandomRotate"]
    (op,) = comp.elastic_ops
    assert (op.alpha, op.grid) == (6.0, 16) and comp.colour_ops == []
    assert A.ELASTIC_DEFAULT_GRID == 32
    (op,) = A.from_spec("elastic=12.8", (32, 48)).elastic_ops                # the default spacing; 12.8 = 0.4 * 32, the bound itself
    assert (op.alpha, op.grid) == (12.8, 32)
    (op,) = A.from_spec("elastic=0:4", (32, 48)).elastic_ops                 # nothing moves; the minimum spacing
    assert (op.alpha, op.grid) == (0.0, 4)
    assert A.from_spec("elastic=1.6:4", (32, 48)).elastic_ops[0].alpha == 1.6
    for bad in ("elastic", "elastic=", "elastic=-1", "elastic=-0.5:16", "elastic=nan", "elastic=nan:16", "elastic=2:3", "elastic=1:0",
                "elastic=1:-8", "elastic=6:16,hflip,elastic=6:16", "elastic=3,elastic=2:8", "elastic=12.9", "elastic=6.5:16",
                "elastic=1.7:4", "elastic=2:8:3", "elastic=2:8.5", "elastic=x", "gamma=2"):
        with pytest.raises(ValueError):
            A.from_spec(bad, (32, 48))
    with pytest.raises(ValueError):                                          # ... and the classes refuse what the spec refuses
        A.Compose([A.RandomElastic(2, 8), A.RandomElastic(2, 8)])
    for alpha, grid in ((-1, 8), (float("nan"), 8), (1, 3)):
        with pytest.raises(ValueError):
            A.RandomElastic(alpha, grid)


def test_main_help_names_the_item():
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    main = importlib.import_module("main")
    assert main.get_args(["--augment", "hflip,elastic=6:16"]).augment == "hflip,elastic=6:16"
    src = open(os.path.join(ROOT, "main.py")).read()
    assert "elastic=<alpha>[:<grid>]" in src


# ------------------------------------------------------------------------------------------------ the host path
def _rgb_and_mask(h=40, w=50, seed=11):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (1, h, w, 3), dtype=np.uint8), rng.randint(0, 34, (1, h, w)).astype(np.uint8)


def _host_want(A, comp_ops, seed, img, gt, out_size, image_fill, label_fill):
    """What the host path must return, from the restatement fed the generators of the seed: uint8 (v + 0x8000) >> 16 and the raw ids."""
    h, w = img.shape[1:3]
    M, (ow, oh) = A.Compose(comp_ops, out_size=out_size).matrix(np.random.RandomState(seed), w, h)
    mats = A.to_q16(M)[None]
    nodes, grid = A.Compose(comp_ops, out_size=(oh, ow)).fields(np.random.RandomState(seed + A.ELASTIC_SEED_OFFSET), 1, w, h, mats)
    sx, sy = coordinates(mats, nodes, grid, (oh, ow))
    v, ids = integers(img, gt, sx, sy, image_fill, label_fill)
    return ((v + 0x8000) >> 16).astype(np.uint8), ids.astype(np.uint8), mats, nodes, grid, (oh, ow)


def test_call_path_equals_the_restatement_on_an_rgb_image_with_a_mask():
    A = _aug()
    img, gt = _rgb_and_mask()
    ops = [A.RandomHorizontallyFlip(0.5), A.RandomRotate(10), A.RandomElastic(6.0, 16), A.RandomScale(0.8, 1.25)]
    comp = A.Compose(ops, image_fill=77, label_fill=250, seed=9)
    out_img, out_gt = comp(Image.fromarray(img[0]), Image.fromarray(gt[0]))
    px, ids, mats, nodes, grid, (oh, ow) = _host_want(A, ops, 9, img, gt, None, 77, 250)
    assert (oh, ow) == (40, 50) and grid == 16 and np.abs(nodes).max() > 3 * 65536 and mats[0, 1] != 0
    assert out_img.mode == "RGB" and out_img.size == (50, 40) and out_gt.mode == "L" and out_gt.size == (50, 40)
    assert np.array_equal(np.asarray(out_img), px[0]) and np.array_equal(np.asarray(out_gt), ids[0])
    assert (ids[0] == 250).any() and (px[0] == 77).all(axis=-1).any()         # both fills show (the rotation leaves the source)
    # the same pixels as the device entry's definition: t = (v * 2^-16) / 255 of the float restatement, rounded
    t, lab = elastic_reference(img, gt, mats, nodes, grid, (oh, ow), [0.0] * 3, [1.0] * 3, np.arange(256), 77, 250)
    assert np.abs(np.asarray(out_img).astype(np.float64) - 255.0 * t[0]).max() <= 0.5 + 1e-4 and np.array_equal(lab[0], ids[0])
    # the lattice did move pixels: the affine part alone, by the same integer definition, gives another image
    v, _ = integers(img, gt, *coordinates(mats, None, 0, (oh, ow)), image_fill=77, label_fill=250)
    assert not np.array_equal(((v[0] + 0x8000) >> 16).astype(np.uint8), px[0])
    # the one-argument form of the 'test' split, and a second object of the same seed
    only = A.Compose(ops, image_fill=77, label_fill=250, seed=9)(Image.fromarray(img[0]))
    assert np.array_equal(np.asarray(only), np.asarray(out_img))


def test_call_path_with_out_size_a_grey_image_a_palette_mask_and_colour_ops():
    A = _aug()
    rng = np.random.RandomState(12)
    img, gt = rng.randint(0, 256, (1, 40, 50, 1), dtype=np.uint8), rng.randint(0, 21, (1, 40, 50)).astype(np.uint8)
    mask = Image.fromarray(gt[0])
    mask.putpalette([(i * 7) % 256 for i in range(768)])
    assert mask.mode == "P"
    ops = [A.RandomElastic(2.0, 7), A.RandomRotate(20), A.RandomBrightness(0.3)]
    comp = A.Compose(ops, out_size=(17, 21), image_fill=9, label_fill=255, seed=4)
    out_img, out_gt = comp(Image.fromarray(img[0][:, :, 0]), mask)
    px, ids, _, nodes, grid, out = _host_want(A, ops, 4, img, gt, (17, 21), 9, 255)
    assert out == (17, 21) and grid == 7 and nodes.shape == (1, 6, 6, 2)
    assert out_gt.mode == "P" and out_gt.getpalette() == mask.getpalette() and np.array_equal(np.asarray(out_gt), ids[0])
    row = A.colour_table_row(*A.Compose(ops).colour_state(np.random.RandomState(4 + 500), 1))
    assert out_img.mode == "L" and np.array_equal(np.asarray(out_img), A.apply_colour(px[0], row, False)[:, :, 0])
    with pytest.raises(ValueError):                                          # 8-bit images only
        comp(Image.fromarray(img[0][:, :, 0]).convert("I"), mask)


def test_zero_alpha_equals_the_affine_integer_definition():
    A = _aug()
    img, gt = _rgb_and_mask(seed=13)
    ops = [A.RandomRotate(15), A.RandomScale(0.7, 1.4)]
    comp = A.Compose(ops + [A.RandomElastic(0.0, 8)], out_size=(33, 41), image_fill=77, label_fill=250, seed=6)
    out_img, out_gt = comp(Image.fromarray(img[0]), Image.fromarray(gt[0]))
    M, _ = A.Compose(ops, out_size=(33, 41)).matrix(np.random.RandomState(6), 50, 40)
    mats = A.to_q16(M)[None]
    want, lab = warp_reference(img, gt, mats, (33, 41), [0.0] * 3, [1.0] * 3, np.arange(256, dtype=np.int64), 77, 250)
    v, ids = integers(img, gt, *coordinates(mats, None, 0, (33, 41)), image_fill=77, label_fill=250)
    assert np.array_equal((v.astype(np.float32) * np.float32(2.0 ** -16)) / np.float32(255), want)   # the affine definition's t
    assert np.array_equal(np.asarray(out_img), ((v[0] + 0x8000) >> 16).astype(np.uint8))
    assert np.array_equal(np.asarray(out_gt).astype(np.int64), lab[0]) and np.array_equal(lab[0], ids[0])


def test_without_an_elastic_op_the_call_path_is_the_pil_one():
    A = _aug()
    img, gt = _rgb_and_mask(seed=14)
    comp = A.Compose([A.RandomRotate(15)], image_fill=77, label_fill=250, seed=3)
    assert comp.elastic_ops == []
    out_img, out_gt = comp(Image.fromarray(img[0]), Image.fromarray(gt[0]))
    M, out = A.Compose([A.RandomRotate(15)]).matrix(np.random.RandomState(3), 50, 40)
    coef = tuple(float(v) for v in M[:2].reshape(-1))
    assert np.array_equal(np.asarray(out_img), np.asarray(Image.fromarray(img[0]).transform(out, Image.AFFINE, coef, Image.BILINEAR, fillcolor=(77,) * 3)))
    assert np.array_equal(np.asarray(out_gt), np.asarray(Image.fromarray(gt[0]).transform(out, Image.AFFINE, coef, Image.NEAREST, fillcolor=250)))


def test_build_loaders_in_host_mode_feed_the_integer_path_to_the_usual_transforms(tmp_path):
    from test_data_utils import _voc_tree
    from types import SimpleNamespace
    du, A = load_sub("data_utils"), _aug()
    root = str(tmp_path / "VOC2012")
    _voc_tree(root)
    args = SimpleNamespace(dataset="voc2012", crop_height=32, crop_width=48, batch_size=2, augment="hflip,rotate=10,elastic=3:8,brightness=0.2")
    lab, unl, val = du.build_loaders(args, roots={"voc2012": root})
    assert len(lab.dataset.augmentation.elastic_ops) == 1 and len(unl.dataset.augmentation.elastic_ops) == 1 and val.dataset.augmentation is None
    img, gt, _ = next(iter(lab))
    assert tuple(img.shape) == (2, 3, 32, 48) and tuple(gt.shape) == (2, 1, 32, 48) and int(gt.max()) <= 20 and int(gt.min()) >= 0
    img, _ = next(iter(unl))[:2]
    assert tuple(img.shape) == (2, 3, 32, 48) and bool(torch.isfinite(img).all())


# ------------------------------------------------------------------------------------------------ the C entry and the wrapper
def test_symbol_is_declared_exported_and_bound_and_the_abi_version_stays():
    L = load_sub("_lib")
    src = open(os.path.join(ROOT, "include", "sscg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint sscg_augment_elastic_u8\s*\(", code)
    sig = L.SIGNATURES["sscg_augment_elastic_u8"][1]
    assert len(sig) == 24 and sig[:19] == L.SIGNATURES["sscg_augment_colour_u8"][1][:19] and sig[23] == C.c_void_p
    assert L.lib.sscg_augment_elastic_u8 is not None
    assert "#define SSCG_ABI_VERSION 18" in src and L.ABI_VERSION == 18 and L.lib.sscg_abi_version() == 18
    comment = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int sscg_augment_elastic_u8", src, flags=re.S).group(1)
    assert "SSCG_ABI_VERSION stays 18" in comment and "6 * 2^24" in comment and "floor" in comment
    kinds = dict(L.dev_tool("racecheck").parse_header(os.path.join(ROOT, "include", "sscg.h"))["sscg_augment_elastic_u8"])
    assert kinds["nodes"] == "r" and kinds["colour"] == "r" and kinds["ws"] == "w" and kinds["grid"] == "-" and kinds["stream"] == "stream"
    assert kinds["img"] == "r" and kinds["mats"] == "r" and kinds["out_img"] == "w" and kinds["out_gt"] == "w"
    # the existing entries keep their signatures
    assert len(L.SIGNATURES["sscg_augment_u8"][1]) == 17 and len(L.SIGNATURES["sscg_augment_colour_u8"][1]) == 20


def test_argument_errors_are_returned_before_any_hip_call():
    lib = load_sub("_lib").lib
    BAD_ARG, UNSUPPORTED = -1, -2
    one = C.c_void_p(16)                                                     # never dereferenced

    def call(img=one, gt=one, mats=one, out=one, out_gt=one, N=2, H=8, W=8, Cc=3, OH=8, OW=8, mean=one, std=one, lut=one, ifill=0, lfill=0,
             colour=one, need_mean=0, ws=one, nodes=one, grid=4, GH=5, GW=5):
        return lib.sscg_augment_elastic_u8(img, gt, mats, out, out_gt, N, H, W, Cc, OH, OW, mean, std, lut, ifill, lfill, colour, need_mean, ws,
                                           nodes, grid, GH, GW, None)
    # its own
    assert call(nodes=None) == BAD_ARG
    assert call(grid=3, GH=6, GW=6) == BAD_ARG and call(grid=0) == BAD_ARG and call(grid=-4) == BAD_ARG
    assert call(GH=4) == BAD_ARG and call(GH=6) == BAD_ARG and call(GW=4) == BAD_ARG and call(GW=6) == BAD_ARG
    assert call(OH=9, GH=5) == BAD_ARG                                       # (9 - 1) / 4 + 4 = 6
    assert call(grid=8, GH=5, GW=5) == BAD_ARG                               # (8 - 1) / 8 + 4 = 4
    # every SSCG_ERR_BAD_ARG case of sscg_augment_u8 and of the colour entry
    for null in ("img", "mats", "out", "mean", "std"):
        assert call(**{null: None}) == BAD_ARG, null
    assert call(Cc=0) == BAD_ARG and call(Cc=5) == BAD_ARG
    for size in ("N", "H", "W", "OH", "OW"):
        assert call(**{size: 0}) == BAD_ARG and call(**{size: -3}) == BAD_ARG, size
    assert call(ifill=256) == BAD_ARG and call(ifill=-1) == BAD_ARG and call(lfill=256) == BAD_ARG and call(lfill=-1) == BAD_ARG
    assert call(lut=None) == BAD_ARG and call(out_gt=None) == BAD_ARG and call(gt=None, lut=None) == BAD_ARG
    assert call(need_mean=1, ws=None) == BAD_ARG and call(need_mean=1, ws=C.c_void_p(20)) == BAD_ARG
    # unsupported: the size limits; C of 2 or 4 only together with a colour table
    assert call(Cc=2) == UNSUPPORTED and call(Cc=4) == UNSUPPORTED
    assert call(Cc=2, nodes=None) == BAD_ARG                                 # a bad argument is reported first
    assert call(N=2, OH=32768, OW=32768, GH=8195, GW=8195) == UNSUPPORTED    # N * OH * OW = 2^31
    assert call(H=32768) == UNSUPPORTED and call(W=32768) == UNSUPPORTED
    assert call(N=65536, OH=1, OW=1, GH=4, GW=4, need_mean=1) == UNSUPPORTED
    assert call(grid=2 ** 22 + 1, GH=4, GW=4) == UNSUPPORTED                 # (position in a cell) * 256 must stay an int


def test_wrapper_refuses_cpu_tensors_and_wrong_nodes():
    F, L = load_sub("functional"), load_sub("_lib")
    img, mats = torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.zeros(1, 6, dtype=torch.int32)
    nodes = torch.zeros(1, 4, 4, 2, dtype=torch.int32)
    with pytest.raises(L.SscgError):
        F.augment_batch(img, None, mats, (4, 4), torch.zeros(3), torch.ones(3), None, elastic=(nodes, 4))
    # the node checks do not depend on where the image lives: stand-ins that claim to be on the device
    class OnDevice:
        def __init__(self, t):
            self.t = t
            self.is_cuda, self.dtype, self.shape = True, t.dtype, t.shape

        def dim(self):
            return self.t.dim()
    for bad, grid in ((nodes, 4), (torch.zeros(1, 5, 4, 2, dtype=torch.int32), 4), (torch.zeros(1, 4, 4, 2, dtype=torch.int64), 4),
                      (torch.zeros(2, 4, 4, 2, dtype=torch.int32), 4), (torch.zeros(1, 4, 4, dtype=torch.int32), 4), (nodes, 3), (None, 4)):
        with pytest.raises(L.SscgError, match="elastic"):
            F.augment_batch(OnDevice(img), None, OnDevice(mats), (4, 4), torch.zeros(3), torch.ones(3), None, elastic=(bad, grid))
