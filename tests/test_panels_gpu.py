"""The per-epoch image panels on the MI355X: sscg_panel_labels against the inference head and label_onehot, sscg_panel_range against
torch.min / torch.max of the restated values, sscg_panel_grid against the numpy restatement of tests/test_panels_host.py (`ref_grid`),
model.panels() fused against SSCG_FUSE_PANELS=0, and train() with a recording writer.  The contract is bit identity: every comparison
is equality."""
import contextlib
import io

import numpy as np
import pytest
import torch

from conftest import load_sub
from oracle import fixtures as FX
from test_panels_host import COLOUR, GREY, IMAGE, panel_case, panel_values, ref_grid, ref_range

pytestmark = pytest.mark.gpu
CL = torch.channels_last

GEOMS = [(9, 13, 50, 71), (17, 17, 128, 128), (33, 65, 64, 130), (24, 40, 24, 40)]
GEOM_IDS = ["9x13-50x71", "17x17-128x128", "33x65-64x130", "identity"]


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def gpu(x, dev):
    x = x.to(dev)
    return x.contiguous(memory_format=CL) if x.dim() == 4 else x


# ------------------------------------------------------------------------------------------ 1. labels
def tie_logits(N, C, H, W, g):
    """the three constructions of tests/test_predict_gpu.py: normal logits, one plane copied onto another, two planes one ulp apart"""
    x = torch.randn(N, C, H, W, generator=g) * 3.0
    lo, hi = 1, C - 1
    xa = torch.randn(N, C, H, W, generator=g)
    xa[:, lo] += 2.5
    xa[:, hi] = xa[:, lo]
    xb = torch.randn(N, C, H, W, generator=g) - 12.0
    base = torch.rand(N, H, W, generator=g) * 0.0624 + 0.0625
    xb[:, lo] = base
    xb[:, hi] = torch.nextafter(base, torch.full_like(base, 1.0))
    assert bool((xb[:, hi] > xb[:, lo]).all()) and float((xb[:, hi] - xb[:, lo]).max()) <= 2.0 ** -27
    return (("normal", x), ("copied plane", xa), ("one ulp apart", xb)), lo, hi


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
@pytest.mark.parametrize("C", [4, 20, 21, 7])
def test_labels_equal_the_predict_head_and_label_onehot(F, dev, C, geom, N):
    lib = load_sub("_lib").lib
    H, W, OH, OW = geom
    cases, lo, hi = tie_logits(N, C, H, W, torch.Generator().manual_seed(1000 * C + 10 * H + N))
    with torch.no_grad():
        for name, t in cases:
            xg = gpu(t, dev)
            want_u8, want_idx, _ = F.predict_labels(xg, (OH, OW), want_index=True)
            want_onehot = F.label_onehot(want_idx.unsqueeze(1), C)
            u8, onehot = F.panel_labels(xg, (OH, OW))
            assert u8.dtype == torch.uint8 and tuple(u8.shape) == (N, OH, OW)
            assert tuple(onehot.shape) == (N, C, OH, OW) and onehot.is_contiguous(memory_format=CL)
            assert torch.equal(u8, want_u8), name
            assert torch.equal(onehot, want_onehot), name
            only_u8, none = F.panel_labels(xg, (OH, OW), want_onehot=False)
            assert none is None and torch.equal(only_u8, want_u8)
            if name == "copied plane":
                assert not bool((u8 == hi).any()) and bool((u8 == lo).any())            # the lower index wins
            if name == "one ulp apart":
                assert bool((u8[:, 0, 0] == lo).all())
            # every element of the one-hot map is written: the entry itself on NaN-filled memory, once on a 16-byte aligned base
            # and once on a base one float behind it (scalar head and tail in every chunk)
            x = F.to_nhwc(xg)
            for off in (0, 1):
                buf = torch.full((N * OH * OW * C + 4,), float("nan"), device=dev)
                ids = torch.full((N * OH * OW,), 255, dtype=torch.uint8, device=dev)
                assert lib.sscg_panel_labels(x.data_ptr(), N, H, W, C, OH, OW, ids.data_ptr(), buf.data_ptr() + 4 * off, F._stream()) == 0
                body = buf[off:off + N * OH * OW * C]
                assert torch.equal(body.view(N, OH, OW, C), want_onehot.permute(0, 2, 3, 1)), (name, off)
                assert torch.equal(ids.view(N, OH, OW), want_u8)
                rest = torch.cat([buf[:off], buf[off + N * OH * OW * C:]])
                assert bool(torch.isnan(rest).all())                                    # and nothing beside it


def test_panel_labels_is_not_an_autograd_node(F, dev):
    L = load_sub("_lib")
    x = torch.randn(1, 21, 9, 9).to(dev).requires_grad_(True)
    with pytest.raises(L.SscgError):
        F.panel_labels(x, (32, 32))
    with torch.no_grad():
        assert F.panel_labels(x, (32, 32))[0].shape == (1, 32, 32)


# ------------------------------------------------------------------------------------------ 2. range
def range_sources(kind, pixels, variant, seed):
    """(host source shaped [1, (C,) 1, pixels], scale, shift, palette) with the extremes where `variant` wants them"""
    src, scale, shift, pal = panel_case(kind, 1, 1, pixels, seed, 3, "voc2012", "constant" if variant == "all equal" else "random")
    if variant == "extremes at the ends":          # the minimum at the last element, the maximum at the first
        if kind == IMAGE:
            src[0, 0, 0, 0], src[0, -1, 0, -1] = 50.0, -50.0
        elif kind == GREY:
            src[src == 255] = 9
            src[0, 0, 0], src[0, 0, -1] = 255, 0
            src[0, 0, 1:-1] += 1
        else:
            src[:] = 7                             # VOC palette: (128, 128, 128)
            src[0, 0, 0], src[0, 0, -1] = 15, 14   # (192, 128, 128) first, (64, 128, 128) last
    if variant == "negative":
        if kind == IMAGE:
            src = (-np.abs(src) - np.float32(3.0)).astype(np.float32)
        elif kind == GREY:
            src = -src - 1
    return src, scale, shift, pal


# (a palette holds no negative value: that variant is an image's and a label map's)
RANGE_CASES = [(k, v) for k in (IMAGE, COLOUR, GREY) for v in ("random", "extremes at the ends", "all equal", "negative")
               if not (k == COLOUR and v == "negative")]


@pytest.mark.parametrize("pixels", [1, 63, 65, 4097, (1 << 20) + 37])
@pytest.mark.parametrize("kind,variant", RANGE_CASES, ids=["%s-%s" % (("image", "colour", "grey")[k], v) for k, v in RANGE_CASES])
def test_range_equals_torch_min_max(F, dev, kind, pixels, variant):
    src, scale, shift, pal = range_sources(kind, pixels, variant, 7 * pixels + kind)
    pal_g = torch.from_numpy(pal).to(dev) if pal is not None else None
    v = torch.from_numpy(panel_values(src, kind, scale, shift, pal))
    want = torch.stack([v.min(), v.max()])
    with torch.no_grad():
        got = F.panel_range(gpu(torch.from_numpy(src), dev), kind, scale, shift, pal_g)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2,)
    assert torch.equal(got.cpu(), want), (got.cpu().tolist(), want.tolist())
    assert np.array_equal(got.cpu().numpy(), ref_range(src, kind, scale, shift, pal))
    if variant == "all equal":
        assert float(got[0]) == float(got[1])
    if variant == "negative":
        assert float(got[1]) < 0


@pytest.mark.parametrize("pixels", [65, 4097])
def test_range_of_colour_panels_with_few_classes(F, dev, pixels):
    utils = load_sub("utils")
    pal = torch.tensor(utils.PALETTES["voc2012"], dtype=torch.uint8).reshape(256, 3)
    one = torch.full((1, 1, pixels), 11, dtype=torch.uint8)                         # a single class: (192, 128, 0)
    black = torch.randint(21, 256, (1, 1, pixels), generator=torch.Generator().manual_seed(pixels)).to(torch.uint8)
    black[0, 0, ::3] = 0                                                            # only classes whose palette rows are all zero
    assert not pal[black.long()].any()
    with torch.no_grad():
        assert F.panel_range(one.to(dev), F.PANEL_COLOUR, palette=pal.to(dev)).tolist() == [0.0, 192.0]
        assert F.panel_range(black.to(dev), F.PANEL_COLOUR, palette=pal.to(dev)).tolist() == [0.0, 0.0]


def test_range_of_an_unaligned_source(F, dev):
    """the entry itself on sources that start 1..3 elements behind a 16-byte boundary: scalar head, vector body, scalar tail"""
    lib = load_sub("_lib").lib
    n = 4097 * 3
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n + 8, generator=g)
    xg = x.to(dev)
    ids = torch.randint(0, 200, (n + 24,), generator=g)
    ids64, ids8 = ids.to(dev), ids.to(torch.uint8).to(dev)
    pal = torch.arange(768, dtype=torch.int64).remainder(251).to(torch.uint8).to(dev)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=dev)
    out = torch.empty(2, device=dev)
    st = F._stream()
    for off in (1, 2, 3):
        assert lib.sscg_panel_range(xg.data_ptr() + 4 * off, IMAGE, n // 3, 3, 0.5, 0.5, None, out.data_ptr(), ws.data_ptr(), ws.numel(), st) == 0
        v = x[off:off + n] * 0.5 + 0.5
        assert out.tolist() == [float(v.min()), float(v.max())]
        assert lib.sscg_panel_range(ids64.data_ptr() + 8 * off, GREY, n, 1, 1.0, 0.0, None, out.data_ptr(), ws.data_ptr(), ws.numel(), st) == 0
        assert out.tolist() == [float(ids[off:off + n].min()), float(ids[off:off + n].max())]
        assert lib.sscg_panel_range(ids8.data_ptr() + 5 * off, COLOUR, n, 1, 1.0, 0.0, pal.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), st) == 0
        pv = pal.cpu().view(256, 3)[ids[5 * off:5 * off + n]]
        assert out.tolist() == [float(pv.min()), float(pv.max())]


# ------------------------------------------------------------------------------------------ 3. grid
def run_grid(F, dev, src, kind, rng, nrow, padding, scale, shift, pal, offset=0):
    """sscg_panel_grid through the binding on a 0xAA-filled allocation with a 256-byte guard band on either side of the grid
    (`offset` moves the grid off its 16-byte alignment).  Returns the grid as numpy; asserts that the guards are untouched."""
    lib = load_sub("_lib").lib
    t = gpu(torch.from_numpy(src), dev)
    if kind == IMAGE:
        t = F.to_nhwc(t)
        n, c, h, w = t.shape
    else:
        (n, h, w), c = t.shape, 1
    shape = F.panel_grid_shape(n, h, w, nrow, padding)
    total = shape[0] * shape[1] * shape[2]
    buf = torch.full((256 + offset + total + 256,), 0xAA, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    pal_g = torch.from_numpy(pal).to(dev) if pal is not None else None
    rng_g = torch.from_numpy(np.asarray(rng, dtype=np.float32)).to(dev)
    rc = lib.sscg_panel_grid(t.data_ptr(), kind, n, h, w, c, scale, shift, pal_g.data_ptr() if pal_g is not None else None,
                             rng_g.data_ptr(), nrow, padding, buf.data_ptr() + 256 + offset, F._stream())
    assert rc == 0
    host = buf.cpu().numpy()
    assert (host[:256 + offset] == 0xAA).all() and (host[256 + offset + total:] == 0xAA).all(), "a guard band was written"
    return host[256 + offset:256 + offset + total].reshape(shape)


@pytest.mark.parametrize("padding", [2, 0])
@pytest.mark.parametrize("tile", [(5, 7), (16, 13), (64, 128)], ids=["5x7", "16x13", "64x128"])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
@pytest.mark.parametrize("kind,c", [(IMAGE, 3), (IMAGE, 1), (COLOUR, 1), (GREY, 1)], ids=["image3", "image1", "colour", "grey"])
def test_grid_equals_the_restatement(F, dev, kind, c, n, tile, padding):
    h, w = tile
    src, scale, shift, pal = panel_case(kind, n, h, w, 1000 * kind + 100 * n + h + padding, c, "cityscapes")
    rng = ref_range(src, kind, scale, shift, pal)
    want = ref_grid(src, kind, rng, 2, padding, scale, shift, pal)
    got = run_grid(F, dev, src, kind, rng, 2, padding, scale, shift, pal)
    assert np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())
    assert got.min() == 0 and got.max() == 255          # a value exactly at lo and one exactly at hi
    # 0xAA is no valid border value: a byte outside a tile that was never written would show here as well
    if n > 1 and padding:
        assert not got[:, :padding].any() and not got[:, :, :padding].any() and not got[:, -padding:].any() and not got[:, :, -padding:].any()
    # off the 16-byte alignment: scalar head and tail
    got = run_grid(F, dev, src, kind, rng, 2, padding, scale, shift, pal, offset=3)
    assert np.array_equal(got, want)
    # and through the wrappers, the range taken on the device
    with torch.no_grad():
        t = gpu(torch.from_numpy(src), dev)
        pal_g = torch.from_numpy(pal).to(dev) if pal is not None else None
        r = F.panel_range(t, kind, scale, shift, pal_g)
        g = F.panel_grid(t, kind, r, 2, padding, scale, shift, pal_g)
    assert np.array_equal(r.cpu().numpy(), rng) and np.array_equal(g.cpu().numpy(), want)


@pytest.mark.parametrize("kind", [IMAGE, COLOUR, GREY], ids=["image", "colour", "grey"])
def test_grid_of_a_constant_panel_is_zero_and_a_foreign_range_clamps(F, dev, kind):
    src, scale, shift, pal = panel_case(kind, 3, 16, 13, 5, 3, "voc2012", "constant")
    rng = ref_range(src, kind, scale, shift, pal)
    assert rng[0] == rng[1]
    got = run_grid(F, dev, src, kind, rng, 2, 2, scale, shift, pal)
    assert np.array_equal(got, ref_grid(src, kind, rng, 2, 2, scale, shift, pal)) and not got.any()
    # a range that does not cover the values: the bytes clamp to 0 and 255 as the restatement's do
    src, scale, shift, pal = panel_case(kind, 3, 16, 13, 6, 3, "voc2012")
    lo, hi = ref_range(src, kind, scale, shift, pal)
    inner = np.array([lo + (hi - lo) * 0.25, lo + (hi - lo) * 0.75], dtype=np.float32)
    got = run_grid(F, dev, src, kind, inner, 2, 2, scale, shift, pal)
    assert np.array_equal(got, ref_grid(src, kind, inner, 2, 2, scale, shift, pal)) and got.max() == 255


# ------------------------------------------------------------------------------------------ 4. models
H = 64
_MODELS = {}


def semi_model(dev, tmp):
    if "semi" not in _MODELS:
        md = load_sub("model")
        args = FX.make_args(dataset="voc2012", crop_height=H, crop_width=H, batch_size=2, gpu_ids=[dev.index or 0],
                            checkpoint_dir=str(tmp), as_written=True)
        m = quiet(md.semisuper_cycleGAN, args)
        for k, sd in FX.semisup_state_dicts(21, torch.float32, "smoke").items():
            getattr(m, k).load_state_dict(sd, strict=True)
        _MODELS["semi"] = (m, args)
    return _MODELS["semi"]


def val_batch(dev, B, C=21):
    smp = [FX.synth_sample("panels/val", i, C, H, H) for i in range(B)]
    gt = torch.stack([g for _, g in smp])
    gt[0, 0, :3] = 255                                   # the "void" label: the ground-truth panel's maximum
    return torch.stack([a for a, _ in smp]).to(dev), gt.to(dev)


def snapshot(nets, optimisers):
    sd = [{k: v.clone() for k, v in net.state_dict().items()} for net in nets]
    opt = [{i: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()} for i, st in o.state_dict()["state"].items()}
           for o in optimisers]
    return sd, opt, [net.training for net in nets]


def same_snapshot(a, b):
    for x, y in zip(a[0], b[0]):
        assert x.keys() == y.keys() and all(torch.equal(x[k], y[k]) for k in x)
    for x, y in zip(a[1], b[1]):
        assert x.keys() == y.keys()
        for i in x:
            assert all(torch.equal(x[i][k], y[i][k]) if torch.is_tensor(x[i][k]) else x[i][k] == y[i][k] for k in x[i])
    assert a[2] == b[2]


def both_paths(F, m, img, gt):
    was = F.FUSE_PANELS[0]
    try:
        F.FUSE_PANELS[0] = True
        fused = m.panels(img, gt)
        F.FUSE_PANELS[0] = False
        plain = m.panels(img, gt)
    finally:
        F.FUSE_PANELS[0] = was
    return fused, plain


@pytest.mark.parametrize("B", [2, 3])
def test_semisupervised_panels_fused_equal_the_separate_passes(F, dev, B, tmp_path_factory):
    md = load_sub("model")
    m, args = semi_model(dev, tmp_path_factory.mktemp("panels_ckpt"))
    nets, opts = [m.Gis, m.Gsi, m.Di, m.Ds, m.old_Gis, m.old_Gsi, m.old_Di], [m.g_optimizer, m.d_optimizer]
    if B == 2:                                           # optimiser state worth comparing: one step first
        np.random.seed(0)
        m.step(*[t.to(dev) for t in FX.step_batch("smoke", 0, 21, H, H, 2)])
        m.sync_losses()
        F.flush_side_work()
        torch.cuda.synchronize()
    img, gt = val_batch(dev, B)
    for mode in (True, False):
        m.Gsi.train(mode)
        m.Gis.train(not mode)
        before = snapshot(nets, opts)
        fused, plain = both_paths(F, m, img, gt)
        torch.cuda.synchronize()
        same_snapshot(before, snapshot(nets, opts))      # parameters, buffers, optimiser state and train / eval modes
    m.Gsi.train()
    m.Gis.train()
    assert tuple(fused.keys()) == tuple(plain.keys()) == md.PANEL_TAGS
    shape = F.panel_grid_shape(B, H, H, 2, 2)
    for tag in md.PANEL_TAGS:
        a, b = fused[tag], plain[tag]
        assert isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.shape == shape and b.dtype == np.uint8
        assert np.array_equal(a, b), "%r: %d bytes differ" % (tag, int((a != b).sum()))
        assert a.max() == 255 and a.min() == 0
    # the ground-truth panel is the restatement of the batch's labels
    gth = gt.cpu().numpy()[:, 0]
    assert np.array_equal(fused[md.PANEL_TAGS[2]], ref_grid(gth, GREY, ref_range(gth, GREY), 2, 2))


@pytest.mark.parametrize("B", [2, 3])
def test_supervised_panels_fused_equal_the_separate_passes(F, dev, B, tmp_path):
    md = load_sub("model")
    if "sup" not in _MODELS:
        args = FX.make_args(dataset="cityscapes", crop_height=H, crop_width=H, batch_size=2, gpu_ids=[dev.index or 0],
                            checkpoint_dir=str(tmp_path), as_written=True)
        torch.manual_seed(4)
        _MODELS["sup"] = quiet(md.supervised_model, args)
    m = _MODELS["sup"]
    img, gt = val_batch(dev, B, 20)
    before = snapshot([m.Gsi], [m.gsi_optimizer])
    fused, plain = both_paths(F, m, img, gt)
    same_snapshot(before, snapshot([m.Gsi], [m.gsi_optimizer]))
    assert tuple(fused.keys()) == tuple(plain.keys()) == md.SUPERVISED_PANEL_TAGS
    for tag in fused:
        assert fused[tag].shape == F.panel_grid_shape(B, H, H, 2, 2) and np.array_equal(fused[tag], plain[tag]), tag


# ------------------------------------------------------------------------------------------ 5. train()
class Recorder:
    def __init__(self):
        self.images, self.scalars = [], []

    def add_scalars(self, tag, d, step):
        self.scalars.append((tag, dict(d), step))

    def add_image(self, tag, arr, step):
        self.images.append((tag, np.array(arr), step))


def test_train_sends_five_panels_per_epoch_and_the_losses_do_not_change(F, dev, tmp_path):
    md = load_sub("model")
    data = load_sub("data")
    sds = FX.semisup_state_dicts(21, torch.float32, "smoke")
    runs = []
    for writer in (Recorder(), None):
        args = FX.make_args(dataset="voc2012", crop_height=H, crop_width=H, batch_size=2, gpu_ids=[dev.index or 0], epochs=2,
                            checkpoint_dir=str(tmp_path / ("w" if writer else "n")), as_written=True)
        m = quiet(md.semisuper_cycleGAN, args)
        for k, sd in sds.items():
            getattr(m, k).load_state_dict(sd, strict=True)
        torch.manual_seed(0)
        np.random.seed(0)
        pdir = str(tmp_path / "png") if writer else None
        runs.append(quiet(m.train, args, loaders=data.synthetic_loaders(args, 21, steps=1), writer=writer, panel_dir=pdir))
        if writer is not None:
            assert [(t, s) for t, _, s in writer.images] == [(t, e) for e in (0, 1) for t in md.PANEL_TAGS]
            for _, arr, _ in writer.images:
                assert arr.dtype == np.uint8 and arr.shape == F.panel_grid_shape(2, H, H, 2, 2)
            assert len(writer.scalars) == 6
            from PIL import Image
            for e in (0, 1):
                for i in range(5):
                    png = np.asarray(Image.open(str(tmp_path / "png" / ("epoch%03d_%d.png" % (e, i + 1)))))
                    assert np.array_equal(png.transpose(2, 0, 1), writer.images[5 * e + i][1])
            assert m.Gsi.training and m.Gis.training
        del m
    assert len(runs[0]) == 2 and runs[0] == runs[1]                     # the nine losses of both steps, bit for bit
