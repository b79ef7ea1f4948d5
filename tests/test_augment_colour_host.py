"""Per-sample colour jitter in the device batch finish, the parts that need no GPU: the C entry's declaration and argument checks, the
colour ops and their composition into one (A, B, b) state, the `--augment` items, the independence of the geometric draws, the host
path - and the definition of sscg_augment_colour_u8 (include/sscg.h) restated in numpy (`colour_reference`, which
tests/test_augment_colour_gpu.py compares the kernels against bit for bit)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import ROOT, load_sub
from test_augment_host import warp_reference

W_LUMA = np.array([0.299, 0.587, 0.114])


def warp_integers(img, mats, out_size, image_fill=0):
    """The integer part of warp_reference (tests/test_augment_host.py) on its own: int64 [N,OH,OW,C], the values v < 2^24 of
    include/sscg.h, sscg_augment_u8."""
    N, H, W, Cc = img.shape
    OH, OW = out_size
    oy, ox = np.meshgrid(np.arange(OH, dtype=np.int64), np.arange(OW, dtype=np.int64), indexing="ij")
    out = np.empty((N, OH, OW, Cc), dtype=np.int64)
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
        out[n] = top * (256 - fy) + bot * fy
    return out


def colour_reference(img, gt, mats, colours, need_mean, out_size, mean, std, lut, image_fill=0, label_fill=0, clamped=True):
    """include/sscg.h, sscg_augment_colour_u8, in numpy: img uint8 [N,H,W,C] (C of 1 or 3), gt uint8 [N,H,W] or None, mats int [N,6],
    colours float32 [N,21] -> (float32 [N,OH,OW,C], int64 [N,OH,OW] or None).  The warp, t and the labels are warp_reference's; the mean
    is an int64 sum and three float64 operations; every float32 product and sum is one numpy operation, so one rounding.
    `clamped=False` leaves out the clamp and the normalisation (what the host tests look at)."""
    f = np.float32
    N, H, W, Cc = img.shape
    OH, OW = out_size
    assert Cc in (1, 3) and colours.dtype == np.float32 and colours.shape == (N, 21)
    v = warp_integers(img, mats, out_size, image_fill)
    t, lab = warp_reference(img, gt, mats, out_size, [0.0] * Cc, [1.0] * Cc, lut, image_fill, label_fill)
    assert t.dtype == np.float32 and np.array_equal(t, (v.astype(f) * f(2.0 ** -16)) / f(255))      # (t - 0) / 1 is exact
    mean, std = np.asarray(mean, dtype=f), np.asarray(std, dtype=f)
    out = np.empty((N, OH, OW, Cc), dtype=f)
    for n in range(N):
        A, B, b = colours[n, :9].reshape(3, 3), colours[n, 9:18].reshape(3, 3), colours[n, 18:]
        mu = np.zeros(Cc, dtype=f)
        if need_mean:
            S = v[n].reshape(-1, Cc).sum(axis=0, dtype=np.int64)
            mu = (S.astype(np.float64) / (np.float64(OH * OW) * np.float64(16711680.0))).astype(f)
        for c in range(Cc):
            if Cc == 3:
                o = ((B[c, 0] * mu[0] + B[c, 1] * mu[1]) + B[c, 2] * mu[2]) + b[c]
                u = ((A[c, 0] * t[n, ..., 0] + A[c, 1] * t[n, ..., 1]) + A[c, 2] * t[n, ..., 2]) + o
            else:
                o = B[0, 0] * mu[0] + b[0]
                u = A[0, 0] * t[n, ..., 0] + o
            assert u.dtype == np.float32 and np.asarray(o).dtype == np.float32
            out[n, ..., c] = (np.minimum(np.maximum(u, f(0)), f(1)) - mean[c]) / std[c] if clamped else u
    return out, lab


def identity_table(n):
    return np.tile(np.concatenate([np.eye(3).reshape(-1), np.zeros(12)]).astype(np.float32), (n, 1))


def _aug():
    return load_sub("data_utils.augmentations")


class _Fixed:
    """A generator whose every draw is the given value."""

    def __init__(self, v):
        self.v = v

    def uniform(self, lo, hi):
        return self.v

    def random_sample(self):
        return self.v


# ------------------------------------------------------------------------------------------------ the C entry
def test_symbols_are_declared_exported_and_bound_and_the_abi_version_stays():
    L = load_sub("_lib")
    src = open(os.path.join(ROOT, "include", "sscg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint sscg_augment_colour_u8\s*\(", code) and re.search(r"\bsize_t sscg_augment_colour_workspace\s*\(int N\)", code)
    assert len(L.SIGNATURES["sscg_augment_colour_u8"][1]) == 20 and L.SIGNATURES["sscg_augment_colour_u8"][1][:16] == L.SIGNATURES["sscg_augment_u8"][1][:16]
    assert L.SIGNATURES["sscg_augment_colour_workspace"] == (C.c_size_t, [C.c_int])
    assert L.lib.sscg_augment_colour_u8 is not None and len(L.SIGNATURES["sscg_augment_u8"][1]) == 17
    assert "#define SSCG_ABI_VERSION 18" in src and L.ABI_VERSION == 18 and L.lib.sscg_abi_version() == 18
    assert L.lib.sscg_augment_colour_workspace(5) == 5 * 3 * 8 and L.lib.sscg_augment_colour_workspace(0) == 0
    # the stream-ordering checker's read / write table: the table is read, the workspace written
    kinds = dict(L.dev_tool("racecheck").parse_header(os.path.join(ROOT, "include", "sscg.h"))["sscg_augment_colour_u8"])
    assert kinds["colour"] == "r" and kinds["ws"] == "w" and kinds["need_mean"] == "-" and kinds["stream"] == "stream"
    assert kinds["img"] == "r" and kinds["mats"] == "r" and kinds["out_img"] == "w" and kinds["out_gt"] == "w"


def test_argument_errors_are_returned_before_any_hip_call():
    lib = load_sub("_lib").lib
    BAD_ARG, UNSUPPORTED = -1, -2
    one = C.c_void_p(16)                                                     # never dereferenced

    def call(img=one, gt=one, mats=one, out=one, out_gt=one, N=2, H=8, W=8, Cc=3, OH=8, OW=8, mean=one, std=one, lut=one, ifill=0, lfill=0,
             colour=one, need_mean=0, ws=one):
        return lib.sscg_augment_colour_u8(img, gt, mats, out, out_gt, N, H, W, Cc, OH, OW, mean, std, lut, ifill, lfill, colour, need_mean, ws, None)
    # every SSCG_ERR_BAD_ARG case of sscg_augment_u8
    for null in ("img", "mats", "out", "mean", "std"):
        assert call(**{null: None}) == BAD_ARG, null
    assert call(Cc=0) == BAD_ARG and call(Cc=5) == BAD_ARG
    for size in ("N", "H", "W", "OH", "OW"):
        assert call(**{size: 0}) == BAD_ARG and call(**{size: -3}) == BAD_ARG, size
    assert call(ifill=256) == BAD_ARG and call(ifill=-1) == BAD_ARG and call(lfill=256) == BAD_ARG and call(lfill=-1) == BAD_ARG
    assert call(lut=None) == BAD_ARG and call(out_gt=None) == BAD_ARG and call(gt=None, lut=None) == BAD_ARG
    # its own
    assert call(colour=None) == BAD_ARG
    assert call(need_mean=1, ws=None) == BAD_ARG
    assert call(need_mean=1, ws=C.c_void_p(20)) == BAD_ARG                   # int64 sums: 8-byte aligned
    assert call(Cc=2) == UNSUPPORTED and call(Cc=4) == UNSUPPORTED
    assert call(Cc=2, colour=None) == BAD_ARG                                # a bad argument is reported first
    assert call(N=2, OH=32768, OW=32768) == UNSUPPORTED                      # N * OH * OW = 2^31
    assert call(H=32768) == UNSUPPORTED and call(W=32768) == UNSUPPORTED
    assert call(N=65536, OH=1, OW=1, need_mean=1) == UNSUPPORTED             # the sum pass takes the sample from the grid's y index


def test_cpu_tensors_are_refused():
    F, L = load_sub("functional"), load_sub("_lib")
    with pytest.raises(L.SscgError):
        F.augment_batch(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), None, torch.zeros(1, 6, dtype=torch.int32), (4, 4),
                        torch.zeros(3), torch.ones(3), None, colour=torch.zeros(1, 21), need_mean=True)


# ------------------------------------------------------------------------------------------------ the ops
def test_factor_zero_ranges_give_the_identity_state():
    A = _aug()
    rng = np.random.RandomState(0)
    for ch in (1, 3):
        comp = A.Compose([A.RandomBrightness(0), A.RandomContrast(0), A.RandomSaturation(0), A.RandomHue(0), A.RandomGrayscale(0)])
        a, b, v = comp.colour_state(rng, ch)
        assert np.allclose(a, np.eye(ch), atol=1e-15) and np.allclose(b, 0, atol=1e-15) and np.allclose(v, 0, atol=1e-15)
        table, need_mean = comp.colours(rng, 4, ch)
        assert need_mean and table.dtype == np.float32 and table.shape == (4, 21)
        assert np.allclose(table, identity_table(4), rtol=0, atol=1e-15)       # (a zero hue turn is inv(T).T: the identity to rounding)
    table, need_mean = A.Compose([A.RandomBrightness(0)]).colours(rng, 2, 3)
    assert not need_mean and np.array_equal(table, identity_table(2))


def test_hue_keeps_luma_and_grey_and_is_a_rotation():
    A = _aug()
    rng = np.random.RandomState(1)
    assert np.allclose(A.YIQ_INV.dot(A.YIQ), np.eye(3), atol=1e-14) and tuple(A.YIQ[0]) == A.LUMA
    for _ in range(50):
        M, c = A.RandomHue(0.5).colour(rng, 3)
        assert c is None and np.abs(W_LUMA.dot(M) - W_LUMA).max() < 1e-12 and np.abs(M.dot(np.ones(3)) - 1).max() < 1e-12
    half, _ = A.RandomHue(0.5).colour(_Fixed(0.5), 3)                        # half a turn twice is a whole one
    assert np.allclose(half.dot(half), np.eye(3), atol=1e-12) and not np.allclose(half, np.eye(3), atol=0.1)
    none, _ = A.RandomHue(0.5).colour(_Fixed(0.0), 3)
    assert np.allclose(none, np.eye(3), atol=1e-15)


def test_grey_saturation_and_one_channel_states():
    A = _aug()
    grey, _ = A.RandomGrayscale(1.0).colour(np.random.RandomState(2), 3)
    assert np.array_equal(grey, np.outer(np.ones(3), W_LUMA))
    keep, _ = A.RandomGrayscale(0.0).colour(np.random.RandomState(2), 3)
    assert np.array_equal(keep, np.eye(3))
    sat0, _ = A.RandomSaturation(1.0).colour(_Fixed(0.0), 3)                 # factor 0 = grey
    assert np.allclose(sat0, grey, atol=1e-15)
    sat1, _ = A.RandomSaturation(1.0).colour(_Fixed(1.0), 3)
    assert np.allclose(sat1, np.eye(3), atol=1e-15)
    # one channel: saturation, hue and grey are the identity; brightness and contrast are scalars with w = (1)
    rng = np.random.RandomState(3)
    for op in (A.RandomSaturation(0.9), A.RandomHue(0.5), A.RandomGrayscale(1.0)):
        M, c = op.colour(rng, 1)
        assert c is None and np.array_equal(M, np.eye(1))
    a, b, v = A.Compose([A.RandomBrightness(0.5), A.RandomContrast(0.5)]).colour_state(_Fixed(1.5), 1)
    assert np.allclose(a, [[2.25]]) and np.allclose(b, [[-0.5 * 1.5]]) and np.allclose(v, [0.0])
    row = A.colour_table_row(a, b, v)
    want = identity_table(1)[0]
    want[0], want[9] = 2.25, -0.75
    assert np.array_equal(row, want)                                         # the layout does not change: [0][0] and [0]


def test_draw_ranges_hold():
    A = _aug()
    rng = np.random.RandomState(4)
    for x, lo, hi in ((0.4, 0.6, 1.4), (1.5, 0.0, 2.5)):
        fs = [A.RandomBrightness(x).colour(rng, 3)[0][0, 0] for _ in range(200)]
        cs = [A.RandomContrast(x).colour(rng, 3)[1] for _ in range(200)]
        ss = [A.RandomSaturation(x).colour(rng, 3)[0] for _ in range(200)]
        ss = [(M[0, 0] - 0.299) / (1 - 0.299) for M in ss]                    # M00 = f + (1 - f) * 0.299
        for vals in (fs, cs, ss):
            assert lo - 1e-12 <= min(vals) and max(vals) <= hi + 1e-12 and max(vals) - min(vals) > 0.8 * (hi - lo)
    hs = []
    for _ in range(200):
        M, _ = A.RandomHue(0.1).colour(rng, 3)
        R = A.YIQ.dot(M).dot(A.YIQ_INV)
        hs.append(np.arctan2(R[2, 1], R[1, 1]) / (2 * np.pi))
    assert -0.1 - 1e-12 <= min(hs) and max(hs) <= 0.1 + 1e-12 and max(hs) - min(hs) > 0.16
    greys = sum(A.RandomGrayscale(0.3).colour(rng, 3)[0][0, 1] != 0 for _ in range(200))
    assert 30 <= greys <= 90


def test_composed_state_equals_op_by_op_application_without_clamps():
    A = _aug()
    ops = [A.RandomBrightness(0.4), A.RandomContrast(0.6), A.RandomSaturation(0.7), A.RandomContrast(0.3), A.RandomHue(0.2)]
    comp = A.Compose(ops)
    v = np.random.RandomState(5).rand(37, 3)
    for seed in range(5):
        a, b, off = comp.colour_state(np.random.RandomState(seed), 3)
        got = v.dot(a.T) + b.dot(v.mean(axis=0)) + off
        rng, x = np.random.RandomState(seed), v.copy()
        for op in ops:
            M, c = op.colour(rng, 3)
            x = x.dot(M.T) if M is not None else c * x + (1 - c) * x.dot(W_LUMA).mean()
        assert np.abs(got - x).max() < 1e-12
        assert np.abs(b).max() > 1e-3                                        # the contrasts did put the mean in


# ------------------------------------------------------------------------------------------------ draws and the spec
def test_geometric_draws_do_not_depend_on_colour_items():
    A = _aug()
    plain = A.from_spec("hflip,rotate=10,scale=0.5:2", (24, 32), out_size=(24, 32))
    mixed = A.from_spec("brightness=0.4,hflip,contrast=0.4,rotate=10,gray=0.2,scale=0.5:2,hue=0.1", (24, 32), out_size=(24, 32))
    a, b = plain.matrices(np.random.RandomState(5), 6, 50, 40), mixed.matrices(np.random.RandomState(5), 6, 50, 40)
    assert np.array_equal(a, b) and len({tuple(r) for r in a.tolist()}) == 6
    # colour draws are deterministic for a seed and differ per sample
    t1, _ = mixed.colours(np.random.RandomState(505), 6, 3)
    t2, _ = mixed.colours(np.random.RandomState(505), 6, 3)
    assert np.array_equal(t1, t2) and len({tuple(r) for r in t1.tolist()}) == 6
    # the host path: the colour generator is seeded with seed + 500 beside the geometric one
    one = A.from_spec("rotate=10,brightness=0.4", (24, 32), seed=9)
    assert A.COLOUR_SEED_OFFSET == 500
    assert one.colour_rng.uniform() == np.random.RandomState(509).uniform() and one.rng.uniform() == np.random.RandomState(9).uniform()


def test_from_spec_takes_the_colour_items_and_refuses_bad_ones():
    A = _aug()
    comp = A.from_spec("hflip, brightness=0.4,contrast=0.3,saturation=0.2,hue=0.1,gray=0.25,rotate=10", (32, 48), out_size=(32, 48))
    assert [type(o).__name__ for o in comp.geometric_ops] == ["RandomHorizontallyFlip", "RandomRotate"]
    assert [type(o).__name__ for o in comp.colour_ops] == ["RandomBrightness", "RandomContrast", "RandomSaturation", "RandomHue",
                                                           "RandomGrayscale"]
    assert [o.x for o in comp.colour_ops[:4]] == [0.4, 0.3, 0.2, 0.1] and comp.colour_ops[4].p == 0.25 and comp.need_mean
    assert not A.from_spec("brightness=0.4,hue=0.5,gray=1", (32, 48)).need_mean
    for bad in ("hue=0.6", "brightness=-1", "gray=2", "contrast", "saturation=-0.1", "gray=-0.5", "hue=-0.1", "brightness=nan", "gamma=2",
                "flip", "rotate", "scale=2", "scale=2:1", "hflip=1"):
        with pytest.raises(ValueError):
            A.from_spec(bad, (32, 48))
    # colour items alone: no geometric op, identity maps plus the out_size crop
    only = A.from_spec("brightness=0.4,contrast=0.4", (32, 48), out_size=(7, 9))
    assert only.geometric_ops == [] and len(only.colour_ops) == 2
    M, size = only.matrix(np.random.RandomState(0), 13, 11)
    assert size == (9, 7) and A.to_q16(M).tolist() == [65536, 0, 2 * 65536, 0, 65536, 2 * 65536]
    M, size = A.from_spec("gray=0.5", (32, 48)).matrix(np.random.RandomState(0), 13, 11)
    assert size == (13, 11) and A.to_q16(M).tolist() == [65536, 0, 0, 0, 65536, 0]


# ------------------------------------------------------------------------------------------------ the host path
HOST_SEEDS = {1: 0, 3: 3}        # per channel count: a seed whose 255 * u stays clear of the half-integers (checked below)


@pytest.mark.parametrize("c", [1, 3])
def test_call_path_equals_the_restatement_on_the_identity_map(c):
    A = _aug()
    rng = np.random.RandomState(60 + c)
    img, gt = rng.randint(0, 256, (1, 11, 13, c), dtype=np.uint8), rng.randint(0, 34, (1, 11, 13)).astype(np.uint8)
    ops = [A.RandomBrightness(0.4), A.RandomContrast(0.4), A.RandomSaturation(0.4), A.RandomHue(0.1)]
    seed = HOST_SEEDS[c]
    comp = A.Compose(ops, seed=seed)
    table, need_mean = A.Compose(ops).colours(np.random.RandomState(seed + 500), 1, c)
    assert need_mean and not np.array_equal(table, identity_table(1))
    ident = np.array([[65536, 0, 0, 0, 65536, 0]], dtype=np.int32)
    u, lab = colour_reference(img, gt, ident, table, True, (11, 13), [0.0] * c, [1.0] * c, np.arange(256, dtype=np.int64))
    scaled = np.float64(255) * u.astype(np.float64)
    assert np.abs(scaled - np.floor(scaled) - 0.5).min() > 1e-3               # no rounding tie in reach of the last bits
    pil = Image.fromarray(img[0] if c == 3 else img[0][:, :, 0])
    out_img, out_gt = comp(pil, Image.fromarray(gt[0]))
    assert out_img.mode == pil.mode and out_img.size == pil.size
    assert np.array_equal(np.asarray(out_img).reshape(11, 13, c), np.rint(np.float32(255) * u[0]).astype(np.uint8))
    assert np.array_equal(np.asarray(out_gt), gt[0]) and np.array_equal(lab[0], gt[0])        # labels are untouched
    only = A.Compose(ops, seed=seed)(pil)                                     # the one-argument form of the 'test' split
    assert np.array_equal(np.asarray(only), np.asarray(out_img))
    assert not np.array_equal(np.asarray(out_img), np.asarray(pil))           # and the jitter did something


def test_restatement_with_the_identity_table_is_the_plain_warp():
    rng = np.random.RandomState(70)
    img, gt = rng.randint(0, 256, (2, 11, 13, 3), dtype=np.uint8), rng.randint(0, 34, (2, 11, 13)).astype(np.uint8)
    mats = np.array([[65536, 0, 0, 0, 65536, 0], [40000, -9000, 3 * 65536 + 77, 9000, 40000, -65536]], dtype=np.int32)
    lut = np.arange(256, dtype=np.int64)
    want, wl = warp_reference(img, gt, mats, (7, 9), [0.4, 0.5, 0.6], [0.2, 0.5, 0.3], lut, 77, 250)
    for need_mean in (False, True):
        got, gl = colour_reference(img, gt, mats, identity_table(2), need_mean, (7, 9), [0.4, 0.5, 0.6], [0.2, 0.5, 0.3], lut, 77, 250)
        assert np.array_equal(got, want) and np.array_equal(gl, wl)
