"""sscg_augment_colour_u8 / functional.augment_batch(colour=) / DeviceLoader with colour items on the MI355X against the numpy restatement
of the definition (tests/test_augment_colour_host.py: colour_reference).  The definition is integers for the warp and the mean's sum, three
fp64 operations for the mean and fp32 operations rounded one by one behind them, which the kernels perform without contraction, so the
contract is equality (torch.equal), not a tolerance."""
import numpy as np
import pytest
import torch

from conftest import load_sub
from test_augment_colour_host import colour_reference, identity_table
from test_augment_gpu import IMAGE_FILL, LABEL_FILL, MEAN, STD, _batch, _six_maps

pytestmark = pytest.mark.gpu


def _run(F, dev, img, gt, mats, colours, need_mean, out_size, c, lut):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    mean, std = torch.tensor(MEAN[:c], device=dev), torch.tensor(STD[:c], device=dev)
    return F.augment_batch(t(img), t(gt) if gt is not None else None, t(mats), out_size, mean, std, lut.to(dev) if lut is not None else None,
                           image_fill=IMAGE_FILL, label_fill=LABEL_FILL, colour=t(colours) if colours is not None else None,
                           need_mean=need_mean)


def _check(F, dev, img, gt, mats, colours, need_mean, out_size, c):
    lut = load_sub("data_utils").label_table("cityscapes")
    got_img, got_gt = _run(F, dev, img, gt, mats, colours, need_mean, out_size, c, lut if gt is not None else None)
    want_img, want_gt = colour_reference(img, gt, mats, colours, need_mean, out_size, MEAN[:c], STD[:c], lut.numpy(), IMAGE_FILL, LABEL_FILL)
    n = img.shape[0]
    assert got_img.dtype == torch.float32 and tuple(got_img.shape) == (n, c) + tuple(out_size)
    assert got_img.permute(0, 2, 3, 1).is_contiguous()                       # channels-last memory, as the plain entry returns
    assert torch.equal(got_img.permute(0, 2, 3, 1).cpu(), torch.from_numpy(want_img))
    if gt is None:
        assert got_gt is None
    else:
        assert got_gt.dtype == torch.int64 and tuple(got_gt.shape) == (n, 1) + tuple(out_size)
        assert torch.equal(got_gt[:, 0].cpu(), torch.from_numpy(want_gt))
    return want_img


def _three_tables(A, c):
    """Three different colour tables: every entry in use (a dense random one, negative entries included); a contrast of 2.5 behind a
    brightness of 1.2 with an offset of -0.5, which leaves [0, 1] at both ends; a drawn brightness / contrast / saturation / hue / grey pipeline."""
    rng = np.random.RandomState(77)
    dense = np.concatenate([rng.uniform(-0.6, 1.2, 9), rng.uniform(-0.5, 0.5, 9), rng.uniform(-0.2, 0.3, 3)]).astype(np.float32)
    steep = A.Compose([A.RandomBrightness(0.5), A.RandomContrast(2.0)])
    steep = A.colour_table_row(*steep.colour_state(_Seq([1.2, 2.5]), c))
    steep[18:] = -0.5                                                        # u = 3 t - 0.5 without the mean: both ends there too
    drawn, need_mean = A.Compose([A.RandomBrightness(0.4), A.RandomContrast(0.4), A.RandomSaturation(0.4), A.RandomHue(0.1),
                                  A.RandomGrayscale(1.0), A.RandomContrast(0.2)]).colours(rng, 1, c)
    assert need_mean
    tables = np.stack([dense, steep, drawn[0]])
    assert tables.dtype == np.float32 and len({tuple(r) for r in tables.tolist()}) == 3 and (tables[1:, 9:18] != 0).any(axis=1).all()
    return tables


class _Seq:
    """A generator that answers the given values in turn."""

    def __init__(self, vals):
        self.vals = list(vals)

    def uniform(self, lo, hi):
        return self.vals.pop(0)


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("need_mean", [0, 1])
def test_small_odd_batch_equals_the_definition(F, dev, c, need_mean):
    """11 x 13 -> 7 x 9, N = 3: 189 pixels = 47 groups of four that straddle rows and samples (the table is reloaded inside a group) +
    a scalar tail of one; zoom 0.5, zoom 2 and the shift that is half outside the source (fill pixels enter the mean), three tables."""
    A = load_sub("data_utils.augmentations")
    mats = _six_maps(A, 13, 11, (7, 9))[3:6]
    assert len({tuple(m) for m in mats.tolist()}) == 3
    tables = _three_tables(A, c)
    img, gt = _batch(3, 11, 13, c, seed=50 + c)
    want = _check(F, dev, img, gt, mats, tables, need_mean, (7, 9), c)
    lo, hi = [(np.float32(e) - np.float32(MEAN[0])) / np.float32(STD[0]) for e in (0, 1)]
    assert (want[1, ..., 0] == lo).any() and (want[1, ..., 0] == hi).any()   # the steep sample clamps at both ends
    if need_mean:                                                            # and the mean does reach the output
        other = colour_reference(img, gt, mats, tables, 0, (7, 9), MEAN[:c], STD[:c], np.arange(256), IMAGE_FILL, LABEL_FILL)[0]
        assert not np.array_equal(other[1], want[1]) and not np.array_equal(other[2], want[2])


@pytest.mark.parametrize("c", [1, 3])
def test_identity_table_equals_the_plain_entry(F, dev, c):
    A = load_sub("data_utils.augmentations")
    lut = load_sub("data_utils").label_table("cityscapes")
    mats = _six_maps(A, 13, 11, (7, 9))[[2, 4, 5]]
    img, gt = _batch(3, 11, 13, c, seed=60 + c)
    want_img, want_gt = _run(F, dev, img, gt, mats, None, False, (7, 9), c, lut)
    for need_mean in (False, True):
        got_img, got_gt = _run(F, dev, img, gt, mats, identity_table(3), need_mean, (7, 9), c, lut)
        assert torch.equal(got_img, want_img) and got_img.stride() == want_img.stride() and torch.equal(got_gt, want_gt)


@pytest.mark.parametrize("c", [1, 3])
def test_image_only(F, dev, c):
    A = load_sub("data_utils.augmentations")
    mats = _six_maps(A, 13, 11, (7, 9))[3:6]
    img, _ = _batch(3, 11, 13, c, seed=70 + c)
    _check(F, dev, img, None, mats, _three_tables(A, c), True, (7, 9), c)


def test_colour_table_is_checked(F, dev):
    L = load_sub("_lib")
    img, _ = _batch(2, 11, 13, 3, seed=80)
    mats = np.tile(np.array([65536, 0, 0, 0, 65536, 0], dtype=np.int32), (2, 1))
    t = lambda a: torch.from_numpy(a).to(dev)
    mean, std = torch.tensor(MEAN, device=dev), torch.tensor(STD, device=dev)
    for bad in (torch.from_numpy(identity_table(2)), t(identity_table(3)), t(identity_table(2)).double(), t(identity_table(2))[:, :20]):
        with pytest.raises(L.SscgError):
            F.augment_batch(t(img), None, t(mats), (11, 13), mean, std, None, colour=bad)
    with pytest.raises(L.SscgError):                                         # two channels: SSCG_ERR_UNSUPPORTED
        F.augment_batch(t(img[..., :2].copy()), None, t(mats), (11, 13), mean[:2], std[:2], None, colour=t(identity_table(2)))


def test_several_sum_blocks_per_sample(F, dev):
    """N = 2, 64 x 96 -> 64 x 96: 6144 pixels per sample.  A block of the sum pass covers 256 consecutive pixels of its sample per round
    and the grid gives a sample one block per 1024 pixels (four rounds), here 6 blocks - six 64-bit atomics per channel meet in a
    sample's sum.  Integer sums: two runs give the same bits."""
    A = load_sub("data_utils.augmentations")
    comp = A.from_spec("rotate=10,scale=0.5:2,brightness=0.4,contrast=0.4,saturation=0.4,hue=0.1", (64, 96), out_size=(64, 96))
    mats = comp.matrices(np.random.RandomState(4), 2, 96, 64)
    tables, need_mean = comp.colours(np.random.RandomState(504), 2, 3)
    assert need_mean and not np.array_equal(mats[0], mats[1]) and (mats[:, 1] != 0).all()
    img, gt = _batch(2, 64, 96, 3, seed=90)
    _check(F, dev, img, gt, mats, tables, True, (64, 96), 3)
    lut = load_sub("data_utils").label_table("cityscapes")
    a = _run(F, dev, img, gt, mats, tables, True, (64, 96), 3, lut)
    b = _run(F, dev, img, gt, mats, tables, True, (64, 96), 3, lut)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_grid_stride_loop_with_mean(F, dev):
    """N = 4, 512 x 512, C = 3: 2^18 groups of four on a grid of 768 x 256 = 196608 threads, so a third of the threads take a second
    group; the sum pass runs 256 blocks per sample, four rounds each."""
    A = load_sub("data_utils.augmentations")
    comp = A.from_spec("rotate=10,scale=0.5:2,brightness=0.4,contrast=0.4,saturation=0.4,hue=0.1", (512, 512), out_size=(512, 512))
    mats = comp.matrices(np.random.RandomState(6), 4, 512, 512)
    tables, need_mean = comp.colours(np.random.RandomState(506), 4, 3)
    assert need_mean and 4 * 512 * 512 // 4 > 768 * 256
    img, gt = _batch(4, 512, 512, 3, seed=100)
    _check(F, dev, img, gt, mats, tables, True, (512, 512), 3)


def test_device_loader_draws_maps_and_tables_from_their_own_generators(F, dev, monkeypatch):
    from torch.utils.data import DataLoader
    du, A = load_sub("data_utils"), load_sub("data_utils.augmentations")
    h, w, n, bs, seed = 11, 13, 6, 3, 123
    img, gt = _batch(n, h, w, 3, seed=40)
    items = [(torch.from_numpy(img[i]), torch.from_numpy(gt[i]), "s%d" % i) for i in range(n)]
    tr = du.get_transformation((h, w), dataset="cityscapes", device_finish=True)
    spec = "hflip,rotate=10,brightness=0.4,contrast=0.4,saturation=0.4,hue=0.1"
    comp = A.from_spec(spec, (h, w), image_fill=IMAGE_FILL, label_fill=LABEL_FILL, out_size=(7, 9))
    calls = {"colour": 0, "plain": 0}
    real_colour, real_plain = F.lib.sscg_augment_colour_u8, F.lib.sscg_augment_u8

    def spy(key, fn):
        def call(*a):
            calls[key] += 1
            return fn(*a)
        return call
    monkeypatch.setattr(F.lib, "sscg_augment_colour_u8", spy("colour", real_colour))
    monkeypatch.setattr(F.lib, "sscg_augment_u8", spy("plain", real_plain))
    loader = du.DeviceLoader(DataLoader(items, batch_size=bs, shuffle=False), tr, dev, augmentation=comp, seed=seed)
    rng, crng = np.random.RandomState(seed), np.random.RandomState(seed + 500)
    plain = A.from_spec("hflip,rotate=10", (h, w), image_fill=IMAGE_FILL, label_fill=LABEL_FILL, out_size=(7, 9))
    prng = np.random.RandomState(seed)
    seen = 0
    for k, (bi, bg, names) in enumerate(loader):
        mats = comp.matrices(rng, bs, w, h)
        assert np.array_equal(mats, plain.matrices(prng, bs, w, h))           # the geometry of the seed, colour items or not
        tables, need_mean = comp.colours(crng, bs, 3)
        sl = slice(k * bs, (k + 1) * bs)
        ri, rg = colour_reference(img[sl], gt[sl], mats, tables, need_mean, (7, 9), tr["mean"], tr["std"], tr["lut"].numpy(), IMAGE_FILL,
                                  LABEL_FILL)
        assert need_mean and tuple(bi.shape) == (bs, 3, 7, 9) and list(names) == ["s%d" % i for i in range(sl.start, sl.stop)]
        assert torch.equal(bi.permute(0, 2, 3, 1).cpu(), torch.from_numpy(ri)) and torch.equal(bg[:, 0].cpu(), torch.from_numpy(rg))
        seen += 1
    assert seen == 2 and calls == {"colour": 2, "plain": 0}
    # a spec without colour items never reaches the new entry
    for _ in du.DeviceLoader(DataLoader(items, batch_size=bs, shuffle=False), tr, dev, augmentation=plain, seed=seed):
        pass
    assert calls == {"colour": 2, "plain": 2}
