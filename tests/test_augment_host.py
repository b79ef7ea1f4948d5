"""Batched affine augmentation, the parts that need no GPU: the C entry's declaration and argument checks, the Q16 coefficients, the
ops' draws, and the integer definition of the warp - restated here in numpy (`warp_reference`, which tests/test_augment_gpu.py
compares the kernel against bit for bit) and checked against hand-computable cases and against the PIL host path of the same maps."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import ROOT, load_sub


def warp_reference(img, gt, mats, out_size, mean, std, lut, image_fill=0, label_fill=0):
    """include/sscg.h, sscg_augment_u8, in numpy: img uint8 [N,H,W,C], gt uint8 [N,H,W] or None, mats int [N,6] ->
    (float32 [N,OH,OW,C], int64 [N,OH,OW] or None).  Integers up to v; then float32 (v * 2^-16) / 255, (t - mean) / std - IEEE
    round-to-nearest operations, one rounding each, like the kernel's."""
    N, H, W, Cc = img.shape
    OH, OW = out_size
    oy, ox = np.meshgrid(np.arange(OH, dtype=np.int64), np.arange(OW, dtype=np.int64), indexing="ij")
    mean, std = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    out = np.empty((N, OH, OW, Cc), dtype=np.float32)
    lab = np.empty((N, OH, OW), dtype=np.int64) if gt is not None else None
    for n in range(N):
        m = [int(v) for v in mats[n]]
        sx, sy = m[0] * ox + m[1] * oy + m[2], m[3] * ox + m[4] * oy + m[5]
        x0, y0 = sx >> 16, sy >> 16
        fx, fy = ((sx & 0xFFFF) >> 8)[..., None], ((sy & 0xFFFF) >> 8)[..., None]

        def tap(y, x):
            inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            px = img[n][np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)].astype(np.int64)
            return np.where(inside[..., None], px, image_fill)
        top = tap(y0, x0) * (256 - fx) + tap(y0, x0 + 1) * fx
        bot = tap(y0 + 1, x0) * (256 - fx) + tap(y0 + 1, x0 + 1) * fx
        v = top * (256 - fy) + bot * fy
        assert int(v.max()) < 2 ** 24
        t = (v.astype(np.float32) * np.float32(2.0 ** -16)) / np.float32(255)
        out[n] = (t - mean) / std
        if gt is not None:
            ix, iy = (sx + 0x8000) >> 16, (sy + 0x8000) >> 16
            inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
            ids = np.where(inside, gt[n][np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)], label_fill)
            lab[n] = np.asarray(lut, dtype=np.int64)[ids]
    return out, lab


def finish_reference(img, mean, std):
    """image_u8_to_f32: ((u / 255) - mean) / std in float32."""
    return (img.astype(np.float32) / np.float32(255) - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)


def _aug():
    return load_sub("data_utils.augmentations")


# ------------------------------------------------------------------------------------------------ the C entry
def test_symbol_is_declared_exported_and_bound_and_the_abi_version_stays():
    L = load_sub("_lib")
    src = open(os.path.join(ROOT, "include", "sscg.h")).read()
    assert re.search(r"\bint sscg_augment_u8\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert "sscg_augment_u8" in L.SIGNATURES and len(L.SIGNATURES["sscg_augment_u8"][1]) == 17
    assert L.lib.sscg_augment_u8 is not None
    assert "#define SSCG_ABI_VERSION 18" in src and L.ABI_VERSION == 18 and L.lib.sscg_abi_version() == 18


def test_argument_errors_are_returned_before_any_hip_call():
    lib = load_sub("_lib").lib
    BAD_ARG, UNSUPPORTED = -1, -2
    one = C.c_void_p(16)                                                     # never dereferenced

    def call(img=one, gt=one, mats=one, out=one, out_gt=one, N=2, H=8, W=8, Cc=3, OH=8, OW=8, mean=one, std=one, lut=one, ifill=0, lfill=0):
        return lib.sscg_augment_u8(img, gt, mats, out, out_gt, N, H, W, Cc, OH, OW, mean, std, lut, ifill, lfill, None)
    for null in ("img", "mats", "out", "mean", "std"):
        assert call(**{null: None}) == BAD_ARG, null
    assert call(Cc=0) == BAD_ARG and call(Cc=5) == BAD_ARG
    for size in ("N", "H", "W", "OH", "OW"):
        assert call(**{size: 0}) == BAD_ARG and call(**{size: -3}) == BAD_ARG, size
    assert call(ifill=256) == BAD_ARG and call(ifill=-1) == BAD_ARG and call(lfill=256) == BAD_ARG and call(lfill=-1) == BAD_ARG
    assert call(lut=None) == BAD_ARG                                         # a label input without a table
    assert call(out_gt=None) == BAD_ARG                                      # ... or without a label output
    assert call(gt=None, lut=None) == BAD_ARG                                # a label output without a label input
    assert call(N=2, OH=32768, OW=32768) == UNSUPPORTED                      # N * OH * OW = 2^31
    assert call(H=32768) == UNSUPPORTED and call(W=32768) == UNSUPPORTED


def test_cpu_tensors_are_refused():
    F, L = load_sub("functional"), load_sub("_lib")
    with pytest.raises(L.SscgError):
        F.augment_batch(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), None, torch.zeros(1, 6, dtype=torch.int32), (4, 4),
                        torch.zeros(3), torch.ones(3), None)


# ------------------------------------------------------------------------------------------------ Q16 coefficients
def test_to_q16_of_identity_hflip_and_integer_translation():
    A = _aug()
    W, H = 13, 11
    rng = np.random.RandomState(0)
    assert A.to_q16(np.eye(3)).tolist() == [65536, 0, 0, 0, 65536, 0] and A.to_q16(np.eye(3)).dtype == np.int32
    M, size = A.RandomHorizontallyFlip(1.0).matrix(rng, W, H)
    assert size == (W, H) and A.to_q16(M).tolist() == [-65536, 0, (W - 1) * 65536, 0, 65536, 0]
    M, size = A.RandomHorizontallyFlip(0.0).matrix(rng, W, H)
    assert A.to_q16(M).tolist() == [65536, 0, 0, 0, 65536, 0]
    M, size = A.CenterCrop((15, 9)).matrix(rng, W, H)                        # x offset round(4 / 2) = 2, y offset round(-4 / 2) = -2
    assert size == (9, 15) and A.to_q16(M).tolist() == [65536, 0, 2 * 65536, 0, 65536, -2 * 65536]
    # a 2x minification samples between the pixel pairs: output index 0 reads source index 0.5
    M, size = A.Scale(6).matrix(rng, 12, 8)
    assert size == (6, 4) and A.to_q16(M).tolist() == [2 * 65536, 0, 32768, 0, 2 * 65536, 32768]


# ------------------------------------------------------------------------------------------------ the integer definition
def _sample(c=3, seed=3, h=11, w=13):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (1, h, w, c), dtype=np.uint8), rng.randint(0, 34, (1, h, w)).astype(np.uint8)


def _three_maps(A, w, h):
    rng = np.random.RandomState(0)
    return [("identity", np.eye(3), (w, h))] + [(name,) + op.matrix(rng, w, h) for name, op in
                                                 (("hflip", A.RandomHorizontallyFlip(1.0)), ("padded crop", A.CenterCrop((h + 4, w - 4))))]


@pytest.mark.parametrize("c", [1, 3])
def test_restatement_reproduces_identity_hflip_and_padded_crop_exactly(c):
    A = _aug()
    img, gt = _sample(c)
    H, W = img.shape[1:3]
    lut = load_sub("data_utils").label_table("cityscapes").numpy()
    mean, std = [0.4, 0.5, 0.6][:c], [0.2, 0.5, 0.3][:c]
    ifill, lfill = 77, 250
    for name, M, (w2, h2) in _three_maps(A, W, H):
        got, lab = warp_reference(img, gt, A.to_q16(M)[None], (h2, w2), mean, std, lut, ifill, lfill)
        if name == "identity":
            want_img, want_gt = img[0], gt[0]
        elif name == "hflip":
            want_img, want_gt = img[0][:, ::-1], gt[0][:, ::-1]
        else:                                                                  # rows -2..H+1, columns 2..W-3: two fill rows on both sides
            want_img = np.full((H + 4, W - 4, c), ifill, dtype=np.uint8)
            want_gt = np.full((H + 4, W - 4), lfill, dtype=np.uint8)
            want_img[2:H + 2], want_gt[2:H + 2] = img[0][:, 2:W - 2], gt[0][:, 2:W - 2]
        assert np.array_equal(got[0], finish_reference(want_img, mean, std)), name
        assert np.array_equal(lab[0], lut[want_gt]), name


@pytest.mark.parametrize("c", [1, 3])
def test_pil_call_path_equals_the_restatement_on_pixel_aligned_maps(c):
    """`Compose.__call__` (Image.transform, AFFINE) and the integer definition agree exactly where the map lands on pixel centres."""
    A = _aug()
    img, gt = _sample(c)
    H, W = img.shape[1:3]
    ident = np.arange(256, dtype=np.int64)
    pil_img = Image.fromarray(img[0] if c == 3 else img[0][:, :, 0])
    pil_gt = Image.fromarray(gt[0])
    for name, op in (("identity", None), ("hflip", A.RandomHorizontallyFlip(1.0)), ("padded crop", A.CenterCrop((H + 4, W - 4)))):
        comp = A.Compose([op] if op is not None else [], image_fill=77, label_fill=250, seed=0)
        out_img, out_gt = comp(pil_img, pil_gt)
        M, (w2, h2) = comp.matrix(np.random.RandomState(0), W, H)
        want, lab = warp_reference(img, gt, A.to_q16(M)[None], (h2, w2), [0.0] * c, [1.0] * c, ident, 77, 250)
        got = np.asarray(out_img).reshape(h2, w2, c)
        assert np.array_equal(finish_reference(got, [0.0] * c, [1.0] * c), want[0]), name
        assert np.array_equal(np.asarray(out_gt).astype(np.int64), lab[0]), name
        only = comp(pil_img)                                                  # the one-argument form of the 'test' split
        assert np.array_equal(np.asarray(only), np.asarray(out_img)), name


# ------------------------------------------------------------------------------------------------ draws
def _pipeline(A):
    return A.Compose([A.RandomHorizontallyFlip(0.5), A.RandomRotate(10), A.RandomScale(0.5, 2.0), A.RandomSizedCrop((24, 32))],
                     out_size=(24, 32))


def test_draws_are_deterministic_for_a_seed():
    A = _aug()
    a = _pipeline(A).matrices(np.random.RandomState(5), 6, 50, 40)
    b = _pipeline(A).matrices(np.random.RandomState(5), 6, 50, 40)
    c = _pipeline(A).matrices(np.random.RandomState(6), 6, 50, 40)
    assert a.dtype == np.int32 and a.shape == (6, 6) and np.array_equal(a, b) and not np.array_equal(a, c)
    assert len({tuple(r) for r in a.tolist()}) == 6                          # one map per sample
    one, two = A.Compose([A.RandomRotate(10)], seed=9), A.Compose([A.RandomRotate(10)], seed=9)
    im = Image.fromarray(_sample(3)[0][0])
    assert np.array_equal(np.asarray(one(im)), np.asarray(two(im)))


def test_crop_rectangles_lie_inside_the_view():
    A = _aug()
    rng = np.random.RandomState(1)
    w, h = 50, 40
    for op in (A.RandomCrop((24, 32)), A.RandomCrop(40), A.RandomSizedCrop(24), A.RandomSizedCrop((24, 32)), A.RandomSized(24)):
        for _ in range(200):
            M, (w2, h2) = op.matrix(rng, w, h)
            corners = M.dot(np.array([[0, w2, 0, w2], [0, 0, h2, h2], [1, 1, 1, 1]], dtype=np.float64))
            assert corners[0].min() >= -1e-9 and corners[0].max() <= w + 1e-9, (op, M)
            assert corners[1].min() >= -1e-9 and corners[1].max() <= h + 1e-9, (op, M)
    # a view smaller than the window is resized to it, not cropped
    M, size = A.RandomCrop((24, 32)).matrix(rng, 16, 12)
    assert size == (32, 24) and np.allclose(M, [[0.5, 0, 0], [0, 0.5, 0], [0, 0, 1]])
    # RandomSizedCrop: the window holds 45..100 % of the area (up to the rounding of its sides)
    for _ in range(100):
        M, _ = A.RandomSizedCrop(24).matrix(rng, w, h)
        frac = (M[0, 0] * 24) * (M[1, 1] * 24) / (w * h)
        assert 0.40 <= frac <= 1.0 + 1e-9


def test_ops_end_at_their_sizes_and_compose_ends_at_out_size():
    A = _aug()
    rng = np.random.RandomState(2)
    assert A.Scale(20).matrix(rng, 50, 40)[1] == (20, 16) and A.Scale(20).matrix(rng, 40, 50)[1] == (16, 20)
    assert A.Scale(50).matrix(rng, 50, 40)[1] == (50, 40)
    assert A.CenterCrop((10, 30)).matrix(rng, 50, 40)[1] == (30, 10)
    assert A.RandomRotate(30).matrix(rng, 50, 40)[1] == (50, 40)
    # a rotation keeps the centre where it is
    M, _ = A.RandomRotate(30).matrix(rng, 50, 40)
    assert np.allclose(M.dot([25.0, 20.0, 1.0]), [25.0, 20.0, 1.0]) and math.isclose(np.linalg.det(M[:2, :2]), 1.0, rel_tol=1e-12)
    for ops in ([], [A.RandomSized(24)], [A.RandomSizedCrop(48)], [A.Scale(20), A.RandomRotate(5)], [A.RandomCrop((24, 32))]):
        for _ in range(20):
            assert A.Compose(ops, out_size=(24, 32)).matrix(rng, 50, 40)[1] == (32, 24)
    assert A.Compose([A.Scale(20)]).matrix(rng, 50, 40)[1] == (20, 16)        # no out_size: wherever the ops end
    im, gt = Image.fromarray(_sample(3, h=40, w=50)[0][0]), Image.fromarray(_sample(3, h=40, w=50)[1][0])
    a, b = A.Compose([A.RandomSized(24)], out_size=(24, 32), seed=0)(im, gt)
    assert a.size == b.size == (32, 24) and a.mode == "RGB" and b.mode == gt.mode


# ------------------------------------------------------------------------------------------------ wiring
def test_from_spec_and_build_loaders_augment_only_the_training_sets(tmp_path):
    from test_data_utils import _voc_tree
    from types import SimpleNamespace
    du, A = load_sub("data_utils"), _aug()
    assert A.from_spec("", (32, 48)) is None and A.from_spec(None, (32, 48)) is None
    comp = A.from_spec("hflip, rotate=10,scale=0.5:2,sizedcrop", (32, 48), label_fill=255, out_size=(32, 48))
    assert [type(o).__name__ for o in comp.ops] == ["RandomHorizontallyFlip", "RandomRotate", "RandomScale", "RandomSizedCrop"]
    assert comp.label_fill == 255 and comp.image_fill == 0 and comp.out_size == (32, 48)
    for bad in ("flip", "rotate", "scale=2", "scale=2:1", "hflip=1"):
        with pytest.raises(ValueError):
            A.from_spec(bad, (32, 48))
    root = str(tmp_path / "VOC2012")
    _voc_tree(root)
    args = SimpleNamespace(dataset="voc2012", crop_height=32, crop_width=48, batch_size=2)          # no `augment` attribute at all
    for ld in du.build_loaders(args, roots={"voc2012": root}):
        assert ld.dataset.augmentation is None
    args.augment = ""
    for ld in du.build_loaders(args, roots={"voc2012": root}):
        assert ld.dataset.augmentation is None
    args.augment = "hflip,rotate=10"
    lab, unl, val = du.build_loaders(args, roots={"voc2012": root})
    assert isinstance(lab.dataset.augmentation, A.Compose) and isinstance(unl.dataset.augmentation, A.Compose)
    assert val.dataset.augmentation is None
    assert lab.dataset.augmentation.label_fill == 255 and du.LABEL_FILL == {"voc2012": 255, "cityscapes": 250, "acdc": 0}
    assert int(du.label_table("voc2012")[255]) == 0 and int(du.label_table("cityscapes")[250]) == 19
    img, gt, _ = next(iter(lab))                                                # host mode: the PIL path feeds the usual transforms
    assert tuple(img.shape) == (2, 3, 32, 48) and tuple(gt.shape) == (2, 1, 32, 48) and int(gt.max()) <= 20
    (test,) = du.build_loaders(args, roots={"voc2012": root}, sets=("test",))
    assert test.dataset.augmentation is None


def test_main_augment_flag_defaults_to_none():
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    main = importlib.import_module("main")
    assert main.get_args([]).augment == ""
    assert main.get_args(["--augment", "hflip,rotate=10"]).augment == "hflip,rotate=10"
