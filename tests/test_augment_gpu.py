"""sscg_augment_u8 / functional.augment_batch / DeviceLoader(augmentation=) on the MI355X against the numpy restatement of the integer
definition (tests/test_augment_host.py: warp_reference).  The definition is integers up to two IEEE float32 divisions, which the kernel
performs with round-to-nearest intrinsics, so the contract is equality (torch.equal), not a tolerance."""
import numpy as np
import pytest
import torch

from conftest import load_sub
from test_augment_host import warp_reference

pytestmark = pytest.mark.gpu

MEAN, STD = [0.4, 0.5, 0.6], [0.2, 0.5, 0.3]
IMAGE_FILL, LABEL_FILL = 77, 250


class _Fixed:
    """A generator whose every draw is the given value."""

    def __init__(self, v):
        self.v = v

    def uniform(self, lo, hi):
        return self.v

    def random_sample(self):
        return self.v


def _batch(n, h, w, c, seed):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (n, h, w, c), dtype=np.uint8), rng.randint(0, 34, (n, h, w)).astype(np.uint8)


def _run(F, dev, img, gt, mats, out_size, c, lut):
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    mean, std = torch.tensor(MEAN[:c], device=dev), torch.tensor(STD[:c], device=dev)
    return F.augment_batch(t(img), t(gt) if gt is not None else None, t(mats), out_size, mean, std, lut.to(dev) if lut is not None else None,
                           image_fill=IMAGE_FILL, label_fill=LABEL_FILL)


def _check(F, dev, img, gt, mats, out_size, c):
    lut = load_sub("data_utils").label_table("cityscapes")
    got_img, got_gt = _run(F, dev, img, gt, mats, out_size, c, lut)
    want_img, want_gt = warp_reference(img, gt, mats, out_size, MEAN[:c], STD[:c], lut.numpy(), IMAGE_FILL, LABEL_FILL)
    n = img.shape[0]
    assert got_img.dtype == torch.float32 and tuple(got_img.shape) == (n, c) + tuple(out_size)
    assert got_img.permute(0, 2, 3, 1).is_contiguous()                       # channels-last memory, as image_u8_to_f32 returns
    assert torch.equal(got_img.permute(0, 2, 3, 1).cpu(), torch.from_numpy(want_img))
    assert got_gt.dtype == torch.int64 and tuple(got_gt.shape) == (n, 1) + tuple(out_size)
    assert torch.equal(got_gt[:, 0].cpu(), torch.from_numpy(want_gt))
    return want_img, want_gt


def _six_maps(A, w, h, out_size):
    """One float map per kind, each ending at out_size: crop, hflip, 17 degrees, zoom 0.5, zoom 2.0, a shift half out of the source."""
    shift = np.array([[1.0, 0.0, -3.5], [0.0, 1.0, 4.25], [0.0, 0.0, 1.0]])

    class Shift:
        def matrix(self, rng, w, h):
            return shift, (w, h)
    rng = np.random.RandomState(0)
    kinds = [([], rng), ([A.RandomHorizontallyFlip(1.0)], rng), ([A.RandomRotate(30)], _Fixed(17.0)),
             ([A.RandomScale(0.5, 0.5)], rng), ([A.RandomScale(2.0, 2.0)], rng), ([Shift()], rng)]
    return np.stack([A.to_q16(A.Compose(ops, out_size=out_size).matrix(r, w, h)[0]) for ops, r in kinds])


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("half", [0, 1])
def test_small_odd_batch_equals_the_integer_definition(F, dev, c, half):
    """11 x 13 -> 7 x 9, N = 3: 189 pixels = 47 groups of four that straddle rows and samples + a scalar tail of one; a different map
    per sample, both fills non-zero, the Cityscapes table."""
    A = load_sub("data_utils.augmentations")
    mats = _six_maps(A, 13, 11, (7, 9))[3 * half:3 * half + 3]
    assert len({tuple(m) for m in mats.tolist()}) == 3
    img, gt = _batch(3, 11, 13, c, seed=10 + c)
    want_img, want_gt = _check(F, dev, img, gt, mats, (7, 9), c)
    if half == 1:                                                            # the shifted sample shows both fills
        fill = ((np.float32(IMAGE_FILL) / np.float32(255) - np.float32(MEAN[0])) / np.float32(STD[0]))
        assert (want_img[2, ..., 0] == fill).any() and (want_gt[2] == 19).any()


@pytest.mark.parametrize("c", [1, 3])
def test_identity_equals_the_two_unfused_passes(F, dev, c):
    du = load_sub("data_utils")
    img, gt = _batch(3, 11, 13, c, seed=20 + c)
    mats = np.tile(np.array([65536, 0, 0, 0, 65536, 0], dtype=np.int32), (3, 1))
    lut = du.label_table("cityscapes")
    mean, std = torch.tensor(MEAN[:c], device=dev), torch.tensor(STD[:c], device=dev)
    want_img = F.image_u8_to_f32(torch.from_numpy(img).to(dev), mean, std)
    want_gt = F.label_lut(torch.from_numpy(gt).to(dev), lut.to(dev))
    got_img, got_gt = _run(F, dev, img, gt, mats, (11, 13), c, lut)
    assert torch.equal(got_img, want_img) and got_img.stride() == want_img.stride()
    assert torch.equal(got_gt, want_gt)
    only_img, none = _run(F, dev, img, None, mats, (11, 13), c, None)       # the 'test' split: no labels, no table
    assert none is None and torch.equal(only_img, want_img)


def test_full_size_batch_with_drawn_maps(F, dev):
    """N = 2, 512 x 1024, C = 3: 2^18 groups of four on a grid of fewer threads (several rounds of the grid-stride loop), Q16 coordinates
    beyond 2^25 (int64 products), maps drawn from rotate=10, scale=0.5:2."""
    A = load_sub("data_utils.augmentations")
    comp = A.from_spec("rotate=10,scale=0.5:2", (512, 1024), out_size=(512, 1024))
    mats = comp.matrices(np.random.RandomState(4), 2, 1024, 512)
    assert not np.array_equal(mats[0], mats[1]) and (mats[:, 1] != 0).all()
    img, gt = _batch(2, 512, 1024, 3, seed=30)
    _check(F, dev, img, gt, mats, (512, 1024), 3)


def test_device_loader_applies_the_seeded_maps_of_each_batch(F, dev):
    from torch.utils.data import DataLoader
    du, A = load_sub("data_utils"), load_sub("data_utils.augmentations")
    h, w, n, bs, seed = 11, 13, 6, 3, 123
    img, gt = _batch(n, h, w, 3, seed=40)
    items = [(torch.from_numpy(img[i]), torch.from_numpy(gt[i]), "s%d" % i) for i in range(n)]
    tr = du.get_transformation((h, w), dataset="cityscapes", device_finish=True)
    comp = A.from_spec("hflip,rotate=10,scale=0.5:2", (h, w), image_fill=IMAGE_FILL, label_fill=LABEL_FILL, out_size=(7, 9))
    loader = du.DeviceLoader(DataLoader(items, batch_size=bs, shuffle=False), tr, dev, augmentation=comp, seed=seed)
    rng = np.random.RandomState(seed)
    mean, std = torch.tensor(tr["mean"], device=dev), torch.tensor(tr["std"], device=dev)
    seen = 0
    for k, (bi, bg, names) in enumerate(loader):
        mats = comp.matrices(rng, bs, w, h)
        sl = slice(k * bs, (k + 1) * bs)
        wi, wg = F.augment_batch(torch.from_numpy(img[sl]).to(dev), torch.from_numpy(gt[sl]).to(dev), torch.from_numpy(mats).to(dev), (7, 9),
                                 mean, std, tr["lut"].to(dev), image_fill=IMAGE_FILL, label_fill=LABEL_FILL)
        assert tuple(bi.shape) == (bs, 3, 7, 9) and torch.equal(bi, wi) and torch.equal(bg, wg) and list(names) == ["s%d" % i for i in range(sl.start, sl.stop)]
        ri, rg = warp_reference(img[sl], gt[sl], mats, (7, 9), tr["mean"], tr["std"], tr["lut"].numpy(), IMAGE_FILL, LABEL_FILL)
        assert torch.equal(bi.permute(0, 2, 3, 1).cpu(), torch.from_numpy(ri)) and torch.equal(bg[:, 0].cpu(), torch.from_numpy(rg))
        seen += 1
    assert seen == 2
    # the 'test' split's (img, name) batches go through the same launch, without labels
    pairs = [(it[0], it[2]) for it in items]
    bi, names = next(iter(du.DeviceLoader(DataLoader(pairs, batch_size=bs, shuffle=False), tr, dev, augmentation=comp, seed=seed)))
    mats = comp.matrices(np.random.RandomState(seed), bs, w, h)
    ri, _ = warp_reference(img[:bs], None, mats, (7, 9), tr["mean"], tr["std"], None, IMAGE_FILL, LABEL_FILL)
    assert torch.equal(bi.permute(0, 2, 3, 1).cpu(), torch.from_numpy(ri)) and list(names) == ["s0", "s1", "s2"]
    # augmentation=None: the unaugmented bits, from the two unfused passes
    bi, bg, _ = next(iter(du.DeviceLoader(DataLoader(items, batch_size=bs, shuffle=False), tr, dev)))
    assert torch.equal(bi, F.image_u8_to_f32(torch.from_numpy(img[:bs]).to(dev), mean, std))
    assert torch.equal(bg, F.label_lut(torch.from_numpy(gt[:bs]).to(dev), tr["lut"].to(dev)))
