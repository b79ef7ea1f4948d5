"""sscg_augment_elastic_u8 / functional.augment_batch(elastic=) / DeviceLoader with an elastic item on the MI355X against the numpy
restatement of the definition (tests/elastic_reference.py).  The definition is integers up to the float operations it shares with the
affine entries, which the kernels round one by one, so the contract is equality (torch.equal), not a tolerance."""
import numpy as np
import pytest
import torch

from conftest import load_sub
from elastic_reference import elastic_reference, lattice_shape
from test_augment_colour_gpu import _three_tables
from test_augment_gpu import IMAGE_FILL, LABEL_FILL, MEAN, STD, _batch, _six_maps

pytestmark = pytest.mark.gpu

H, W, OUT = 19, 23, (17, 21)          # case A: N = 3 of 19 x 23 -> 17 x 21, 1071 pixels = 267 groups of four + a scalar tail of three


def _run(F, dev, img, gt, mats, nodes, grid, out_size, c, lut, colours=None, need_mean=False):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    mean, std = torch.tensor(MEAN[:c], device=dev), torch.tensor(STD[:c], device=dev)
    return F.augment_batch(t(img), t(gt) if gt is not None else None, t(mats), out_size, mean, std, lut.to(dev) if lut is not None else None,
                           image_fill=IMAGE_FILL, label_fill=LABEL_FILL, colour=t(colours) if colours is not None else None,
                           need_mean=need_mean, elastic=(t(nodes), grid) if nodes is not None else None)


def _check(F, dev, img, gt, mats, nodes, grid, out_size, c, colours=None, need_mean=False):
    lut = load_sub("data_utils").label_table("cityscapes")
    got_img, got_gt = _run(F, dev, img, gt, mats, nodes, grid, out_size, c, lut if gt is not None else None, colours, need_mean)
    want_img, want_gt = elastic_reference(img, gt, mats, nodes, grid, out_size, MEAN[:c], STD[:c], lut.numpy(), IMAGE_FILL, LABEL_FILL,
                                          colours=colours, need_mean=need_mean)
    n = img.shape[0]
    assert got_img.dtype == torch.float32 and tuple(got_img.shape) == (n, c) + tuple(out_size)
    assert got_img.permute(0, 2, 3, 1).is_contiguous()                       # channels-last memory, as the affine entries return
    assert torch.equal(got_img.permute(0, 2, 3, 1).cpu(), torch.from_numpy(want_img))
    if gt is None:
        assert got_gt is None
    else:
        assert got_gt.dtype == torch.int64 and tuple(got_gt.shape) == (n, 1) + tuple(out_size)
        assert torch.equal(got_gt[:, 0].cpu(), torch.from_numpy(want_gt))
    return want_img, want_gt


def _nodes(n, grid, out_size, seed, reach=6):
    """Random nodes up to +-reach source pixels."""
    gh, gw = lattice_shape(grid, *out_size)
    return np.random.RandomState(seed).randint(-reach * 65536, reach * 65536 + 1, (n, gh, gw, 2)).astype(np.int32)


def _case_a(c, half, seed):
    A = load_sub("data_utils.augmentations")
    mats = _six_maps(A, W, H, OUT)[3 * half:3 * half + 3]
    assert len({tuple(m) for m in mats.tolist()}) == 3 and (3 * OUT[0] * OUT[1]) % 4 == 3 and OUT[1] % 4 != 0
    return _batch(3, H, W, c, seed=seed) + (mats,)


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("grid", [4, 7, 64])
def test_small_odd_batch_equals_the_definition(F, dev, c, half, grid):
    """Case A with the six map kinds cycled over the samples (three per case) and nodes up to +-6 source pixels: groups straddle rows
    and samples, the scalar tail runs.  grid 4: the minimum spacing, a group of four always crosses into the next cell, the last cell of
    a row is partial; 7: no power of two, does not divide the output; 64: the whole output in one cell."""
    img, gt, mats = _case_a(c, half, seed=110 + c)
    nodes = _nodes(3, grid, OUT, seed=120 + grid)
    want_img, want_gt = _check(F, dev, img, gt, mats, nodes, grid, OUT, c)
    fill = ((np.float32(IMAGE_FILL) / np.float32(255) - np.float32(MEAN[0])) / np.float32(STD[0]))
    assert (want_img[..., 0] == fill).any() and (want_gt == 19).any()          # taps and labels leave the source and take the fills
    plain = elastic_reference(img, gt, mats, None, grid, OUT, MEAN[:c], STD[:c], np.arange(256), IMAGE_FILL, LABEL_FILL)[0]
    assert all(not np.array_equal(plain[n], want_img[n]) for n in range(3))   # and the lattice moved every sample


@pytest.mark.parametrize("c", [1, 3])
def test_zero_lattice_equals_the_affine_entries(F, dev, c):
    A = load_sub("data_utils.augmentations")
    lut = load_sub("data_utils").label_table("cityscapes")
    img, gt, mats = _case_a(c, 1, seed=130 + c)
    zero = np.zeros((3,) + lattice_shape(7, *OUT) + (2,), dtype=np.int32)
    want_img, want_gt = _run(F, dev, img, gt, mats, None, 7, OUT, c, lut)
    got_img, got_gt = _run(F, dev, img, gt, mats, zero, 7, OUT, c, lut)
    assert torch.equal(got_img, want_img) and got_img.stride() == want_img.stride() and torch.equal(got_gt, want_gt)
    tables = _three_tables(A, c)
    want_img, want_gt = _run(F, dev, img, gt, mats, None, 7, OUT, c, lut, tables, True)
    got_img, got_gt = _run(F, dev, img, gt, mats, zero, 7, OUT, c, lut, tables, True)
    assert torch.equal(got_img, want_img) and got_img.stride() == want_img.stride() and torch.equal(got_gt, want_gt)


@pytest.mark.parametrize("c", [1, 3])
def test_constant_lattice_equals_the_affine_entry_with_shifted_translations(F, dev, c):
    lut = load_sub("data_utils").label_table("cityscapes")
    img, gt, mats = _case_a(c, 0, seed=140 + c)
    a, b = 3 * 65536 + 1234, -70000
    for grid in (4, 7):
        const = np.empty((3,) + lattice_shape(grid, *OUT) + (2,), dtype=np.int32)
        const[..., 0], const[..., 1] = a, b
        shifted = mats.copy()
        shifted[:, 2] += a
        shifted[:, 5] += b
        want_img, want_gt = _run(F, dev, img, gt, shifted, None, grid, OUT, c, lut)
        got_img, got_gt = _run(F, dev, img, gt, mats, const, grid, OUT, c, lut)
        assert torch.equal(got_img, want_img) and torch.equal(got_gt, want_gt)
        assert not torch.equal(got_img, _run(F, dev, img, gt, mats, None, grid, OUT, c, lut)[0])


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("labels", [1, 0])
def test_colour_with_a_contrast_sees_the_displaced_pixels(F, dev, c, labels):
    """Case A at grid 7 with three colour tables that use the image mean: equal to the restatement, whose sum runs over the displaced
    pixels - and different from what the mean of the undisplaced ones would give."""
    A = load_sub("data_utils.augmentations")
    img, gt, mats = _case_a(c, 1, seed=150 + c)
    nodes = _nodes(3, 7, OUT, seed=151)
    tables = _three_tables(A, c)
    want, _ = _check(F, dev, img, gt if labels else None, mats, nodes, 7, OUT, c, colours=tables, need_mean=True)
    no_mean = elastic_reference(img, None, mats, nodes, 7, OUT, MEAN[:c], STD[:c], None, IMAGE_FILL, LABEL_FILL, colours=tables)[0]
    assert not np.array_equal(no_mean[1], want[1]) and not np.array_equal(no_mean[2], want[2])
    _check(F, dev, img, gt if labels else None, mats, nodes, 7, OUT, c, colours=tables, need_mean=False)


def test_second_round_of_the_grid_stride_loop(F, dev):
    """N = 13 of 256 x 256 x 3 with labels, grid 32: 212992 groups of four on the apply kernel's grid cap of 768 blocks x 256 threads =
    196608, so 16384 threads take a second group; drawn maps and nodes."""
    A = load_sub("data_utils.augmentations")
    comp = A.from_spec("hflip,rotate=10,scale=0.5:2,elastic=12:32", (256, 256), out_size=(256, 256))
    mats = comp.matrices(np.random.RandomState(7), 13, 256, 256)
    nodes, grid = comp.fields(np.random.RandomState(8), 13, 256, 256, mats)
    assert grid == 32 and nodes.shape == (13, 11, 11, 2) and 13 * 256 * 256 // 4 > 768 * 256 and np.abs(nodes).max() > 6 * 65536
    img, gt = _batch(13, 256, 256, 3, seed=160)
    _check(F, dev, img, gt, mats, nodes, grid, (256, 256), 3)


def test_device_loader_draws_from_three_generators_and_repeats_for_a_seed(F, dev):
    from torch.utils.data import DataLoader
    du, A = load_sub("data_utils"), load_sub("data_utils.augmentations")
    h, w, n, bs, seed = 40, 50, 6, 3, 123
    img, gt = _batch(n, h, w, 3, seed=170)
    items = [(torch.from_numpy(img[i]), torch.from_numpy(gt[i]), "s%d" % i) for i in range(n)]
    tr = du.get_transformation((h, w), dataset="cityscapes", device_finish=True)
    spec = "hflip,rotate=10,elastic=6:16,brightness=0.3"
    comp = A.from_spec(spec, (h, w), image_fill=IMAGE_FILL, label_fill=LABEL_FILL, out_size=(33, 41))
    loader = du.DeviceLoader(DataLoader(items, batch_size=bs, shuffle=False), tr, dev, augmentation=comp, seed=seed)
    rng, crng, erng = (np.random.RandomState(seed + off) for off in (0, A.COLOUR_SEED_OFFSET, A.ELASTIC_SEED_OFFSET))
    first = []
    for k, (bi, bg, names) in enumerate(loader):
        mats = comp.matrices(rng, bs, w, h)
        tables, need_mean = comp.colours(crng, bs, 3)
        nodes, grid = comp.fields(erng, bs, w, h, mats)
        sl = slice(k * bs, (k + 1) * bs)
        ri, rg = elastic_reference(img[sl], gt[sl], mats, nodes, grid, (33, 41), tr["mean"], tr["std"], tr["lut"].numpy(), IMAGE_FILL,
                                   LABEL_FILL, colours=tables, need_mean=need_mean)
        assert not need_mean and grid == 16 and tuple(bi.shape) == (bs, 3, 33, 41) and list(names) == ["s%d" % i for i in range(sl.start, sl.stop)]
        assert torch.equal(bi.permute(0, 2, 3, 1).cpu(), torch.from_numpy(ri)) and torch.equal(bg[:, 0].cpu(), torch.from_numpy(rg))
        first.append((bi, bg))
    assert len(first) == 2
    again = list(du.DeviceLoader(DataLoader(items, batch_size=bs, shuffle=False), tr, dev, augmentation=comp, seed=seed))
    assert len(again) == 2 and all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(first, again))
    other = next(iter(du.DeviceLoader(DataLoader(items, batch_size=bs, shuffle=False), tr, dev, augmentation=comp, seed=seed + 1)))
    assert not torch.equal(other[0], first[0][0])


def test_without_an_elastic_item_the_new_entry_is_never_reached(F, dev, monkeypatch):
    from torch.utils.data import DataLoader
    du, A = load_sub("data_utils"), load_sub("data_utils.augmentations")
    img, gt = _batch(3, 11, 13, 3, seed=180)
    items = [(torch.from_numpy(img[i]), torch.from_numpy(gt[i]), "s%d" % i) for i in range(3)]
    tr = du.get_transformation((11, 13), dataset="cityscapes", device_finish=True)
    calls = []
    real = F.lib.sscg_augment_elastic_u8
    monkeypatch.setattr(F.lib, "sscg_augment_elastic_u8", lambda *a: calls.append(1) or real(*a))
    for spec in ("hflip,rotate=10", "hflip,rotate=10,contrast=0.3"):
        comp = A.from_spec(spec, (11, 13), out_size=(7, 9))
        for _ in du.DeviceLoader(DataLoader(items, batch_size=3, shuffle=False), tr, dev, augmentation=comp, seed=1):
            pass
    assert calls == []
    comp = A.from_spec("hflip,elastic=1:4", (11, 13), out_size=(7, 9))
    for _ in du.DeviceLoader(DataLoader(items, batch_size=3, shuffle=False), tr, dev, augmentation=comp, seed=1):
        pass
    assert calls == [1]


def test_node_tensors_are_checked(F, dev):
    L = load_sub("_lib")
    img, _ = _batch(2, 11, 13, 3, seed=190)
    mats = np.tile(np.array([65536, 0, 0, 0, 65536, 0], dtype=np.int32), (2, 1))
    t = lambda a: torch.from_numpy(a).to(dev)
    mean, std = torch.tensor(MEAN, device=dev), torch.tensor(STD, device=dev)
    good = np.zeros((2,) + lattice_shape(4, 11, 13) + (2,), dtype=np.int32)
    for bad, grid in ((torch.from_numpy(good), 4), (t(good)[:1], 4), (t(good).long(), 4), (t(good)[:, :-1], 4), (t(good), 5), (t(good), 3)):
        with pytest.raises(L.SscgError):
            F.augment_batch(t(img), None, t(mats), (11, 13), mean, std, None, elastic=(bad, grid))
    with pytest.raises(L.SscgError):                                         # two channels with a colour table: SSCG_ERR_UNSUPPORTED
        F.augment_batch(t(img[..., :2].copy()), None, t(mats), (11, 13), mean[:2], std[:2], None, elastic=(t(good), 4),
                        colour=t(np.zeros((2, 21), dtype=np.float32)))
    out, none = F.augment_batch(t(img[..., :2].copy()), None, t(mats), (11, 13), mean[:2], std[:2], None, elastic=(t(good), 4))
    assert none is None and tuple(out.shape) == (2, 2, 11, 13)               # ... without one every C in 1..4 runs
