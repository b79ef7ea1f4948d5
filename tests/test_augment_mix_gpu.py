"""sscg_augment_mix_u8 / functional.augment_batch(mix=) / DeviceLoader with cutmix / classmix items on the MI355X against the numpy
restatement of the definition (tests/mix_reference.py over tests/elastic_reference.py).  out[n] = where(pasted, plain[p], plain[n])
is a selection among bits the other entries already pin, so the contract is equality (torch.equal) everywhere, no tolerance."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_sub
from elastic_reference import elastic_reference, lattice_shape
from mix_reference import mix_reference
from test_augment_colour_gpu import _three_tables
from test_augment_elastic_gpu import H, OUT, W, _case_a, _nodes
from test_augment_gpu import IMAGE_FILL, LABEL_FILL, MEAN, STD, _batch

pytestmark = pytest.mark.gpu

OH, OW = OUT
VARIANTS = ("plain", "colour", "elastic", "both")
BITS = sum(1 << b for b in (0, 2, 3, 5, 8, 11, 13, 17, 31, 40, 63))          # bit 31 and bit 63: both table words negative as int32


def _words(mask):
    """(mask_lo, mask_hi) as the int32 values with these bits."""
    return [int(np.array(w, dtype=np.uint32).view(np.int32)) for w in (mask & 0xFFFFFFFF, mask >> 32)]


def _lut(name):
    return load_sub("data_utils").label_table(name)


def _pipeline(variant, c, n=3, out=OUT, grid=7, seed=230):
    """(nodes, grid, colours, need_mean) of a pipeline variant."""
    A = load_sub("data_utils.augmentations")
    nodes = _nodes(n, grid, out, seed=seed) if variant in ("elastic", "both") else None
    colours = _three_tables(A, c) if variant in ("colour", "both") else None
    return nodes, grid, colours, colours is not None


def _tables(fill_class):
    """The two tables of case A, both the chain 0 <- 1 <- 2 with sample 2 unmixed.  First: an interior box that cuts groups of four
    (x0 = 1, x1 = OW - 1), a box sticking out of the output on two sides, and - on the unmixed sample, where it must do nothing - an
    empty box with a nonzero mask.  Second: the empty box with a nonzero mask on a mixed sample (the class rule alone), the interior
    box, and a partner of -1.  Every mask has bit 63 and, where it is below 64, the class of label_fill."""
    mask = BITS | (1 << fill_class if fill_class < 64 else 0)
    lo, hi = _words(mask)
    olo, ohi = _words(mask ^ 0x0F0F)
    first = [[1, 1, 3, OW - 1, 9, lo, hi, 0], [2, -5, -3, 6, 5, olo, ohi, 0], [2, 5, 5, 5, 9, lo, hi, 0]]
    second = [[1, 4, 2, 4, 11, lo, hi, 0], [2, 1, 3, OW - 1, 9, olo, ohi, 0], [-1, 0, 0, OW, OH, lo, hi, 0]]
    return np.array(first, dtype=np.int32), np.array(second, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def case_one(c, lut_name, variant):
    """Inputs and expected outputs of test 1, computed once: case A (N = 3 of 19 x 23 -> 17 x 21, the second three of the six map
    kinds: zoom 0.5, zoom 2, a shift half out of the source) under the two tables.  The conditions that keep the test honest are
    asserted here, on the reference alone (tests/test_augment_mix_host.py runs this without a GPU)."""
    img, gt, mats = _case_a(c, 1, seed=200 + c)
    lut = _lut(lut_name).numpy()
    if lut_name == "voc2012":                            # raw ids whose classes are >= 64 and alias set bits modulo 64: 127 -> 63, 128 -> 0, 200 -> 8
        gt = gt.copy()
        for raw, high in ((31, 127), (32, 128), (33, 200)):
            gt[gt == raw] = high
        assert all(int(lut[v]) == v for v in (127, 128, 200)) and all(BITS >> (v % 64) & 1 for v in (127, 128, 200))
    nodes, grid, colours, need_mean = _pipeline(variant, c)
    plain = elastic_reference(img, gt, mats, nodes, grid, OUT, MEAN[:c], STD[:c], lut, IMAGE_FILL, LABEL_FILL, colours=colours, need_mean=need_mean)
    raw = elastic_reference(img, gt, mats, nodes, grid, OUT, MEAN[:c], STD[:c], np.arange(256), IMAGE_FILL, LABEL_FILL)[1]
    fill = raw == LABEL_FILL                             # the pixels whose label left the source (no raw id of the batch is 250)
    assert not (gt == LABEL_FILL).any() and fill[2].any() and not fill.all(axis=(1, 2)).any()
    wants = []
    for k, table in enumerate(_tables(int(lut[LABEL_FILL]))):
        want_img, want_gt, pasted, _ = mix_reference(img, gt, mats, nodes, grid, OUT, MEAN[:c], STD[:c], lut, table, 1, IMAGE_FILL, LABEL_FILL,
                                                     colours=colours, need_mean=need_mean, plain=plain)
        box = mix_reference(img, gt, mats, nodes, grid, OUT, MEAN[:c], STD[:c], lut, table, 0, IMAGE_FILL, LABEL_FILL, plain=plain)[2]
        for n in (0, 1):                                 # both kinds of pixel on every mixed sample, and the result is not the unmixed one
            assert pasted[n].any() and not pasted[n].all()
            assert not np.array_equal(want_img[n], plain[0][n]) and not np.array_equal(want_gt[n], plain[1][n])
        assert not pasted[2].any() and np.array_equal(want_img[2], plain[0][2])
        assert (pasted & ~box).any()                     # pasted by the class rule alone
        assert (pasted[1] & fill[2]).any()               # a partner pixel inside the fill region is pasted
        assert not (pasted & ~box & (plain[1][[1, 2, 2]] >= 64)).any()       # the partner's class >= 64 pastes only inside a box
        # chains do not propagate: where sample 0 takes from sample 1 it shows sample 1's UNMIXED pixel, also where sample 1 itself
        # was pasted over with something else
        both = pasted[0] & pasted[1] & (plain[1][1] != plain[1][2])
        assert both.any() and np.array_equal(want_gt[0][both], plain[1][1][both]) and not np.array_equal(want_gt[0][both], want_gt[1][both])
        if k == 0:
            assert box[0].sum() == (OW - 2) * 6 and 0 < box[1].sum() == 6 * 5 and not box[2].any()
        else:
            assert not box[0].any() and pasted[0].any()  # the empty box: the class rule alone
        wants.append((table, want_img, want_gt))
    if lut_name == "voc2012":
        assert (plain[1] >= 64).any()
    return img, gt, mats, nodes, grid, colours, need_mean, plain, wants


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(F, dev, img, gt, mats, out_size, c, lut, table=None, classes=0, nodes=None, grid=7, colours=None, need_mean=False):
    mean, std = torch.tensor(MEAN[:c], device=dev), torch.tensor(STD[:c], device=dev)
    return F.augment_batch(_t(dev, img), _t(dev, gt) if gt is not None else None, _t(dev, mats), out_size, mean, std,
                           lut.to(dev) if gt is not None else None, image_fill=IMAGE_FILL, label_fill=LABEL_FILL,
                           colour=_t(dev, colours) if colours is not None else None, need_mean=need_mean,
                           elastic=(_t(dev, nodes), grid) if nodes is not None else None,
                           mix=(_t(dev, table), classes) if table is not None else None)


def _equal(got, want_img, want_gt):
    got_img, got_gt = got
    assert got_img.dtype == torch.float32 and got_img.permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(got_img.permute(0, 2, 3, 1).cpu(), torch.from_numpy(want_img))
    if want_gt is None:
        assert got_gt is None
    else:
        assert got_gt.dtype == torch.int64 and torch.equal(got_gt[:, 0].cpu(), torch.from_numpy(want_gt))


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("lut_name", ["cityscapes", "voc2012"])
@pytest.mark.parametrize("c", [1, 3])
def test_small_odd_batch_equals_the_definition(F, dev, c, lut_name, variant):
    """1071 pixels: 267 groups of four that straddle rows and samples (the mix row and the partner's matrix and colour table are
    reloaded inside a group) and a scalar tail of three; boxes that cut groups, leave the output or are empty; masks whose words are
    negative; VOC's classes >= 64, which alias set bits modulo 64 and must not paste."""
    img, gt, mats, nodes, grid, colours, need_mean, _, wants = case_one(c, lut_name, variant)
    for table, want_img, want_gt in wants:
        _equal(_run(F, dev, img, gt, mats, OUT, c, _lut(lut_name), table, 1, nodes, grid, colours, need_mean), want_img, want_gt)


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("c", [1, 3])
def test_identities(F, dev, c, variant):
    img, gt, mats, nodes, grid, colours, need_mean, _, _ = case_one(c, "cityscapes", variant)
    lut = _lut("cityscapes")
    kw = dict(nodes=nodes, grid=grid, colours=colours, need_mean=need_mean)
    plain_img, plain_gt = _run(F, dev, img, gt, mats, OUT, c, lut, **kw)         # the existing entry that fits the variant
    lo, hi = _words(BITS | 1 << 19)
    # an all-unmixed table: the partner is the sample itself, -1 or N - whatever box and mask the row holds
    for partners in ([0, 1, 2], [-1, -1, -1], [3, 3, 3], [0, -7, 2 ** 31 - 1]):
        table = np.array([[p, -3, -3, OW + 3, OH + 3, lo, hi, 0] for p in partners], dtype=np.int32)
        for classes in (0, 1):
            got_img, got_gt = _run(F, dev, img, gt, mats, OUT, c, lut, table, classes, **kw)
            assert torch.equal(got_img, plain_img) and got_img.stride() == plain_img.stride()
            assert torch.equal(got_gt, plain_gt) and got_gt.stride() == plain_gt.stride()
    # a box that covers the whole output (exactly, and reaching far beyond it): the partner's batch entry, labels included
    for box in ((0, 0, OW, OH), (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1)):
        table = np.array([[(n + 1) % 3, *box, 0, 0, 0] for n in range(3)], dtype=np.int32)
        got_img, got_gt = _run(F, dev, img, gt, mats, OUT, c, lut, table, 1, **kw)
        assert torch.equal(got_img, plain_img[[1, 2, 0]]) and torch.equal(got_gt, plain_gt[[1, 2, 0]])
    # a 1 x 1 box at the last pixel of the last sample - the scalar tail - changes exactly that pixel
    # (from sample 1: samples 0 and 2 both show the fill there)
    table = np.array([[0, 0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0], [1, OW - 1, OH - 1, OW, OH, 0, 0, 0]], dtype=np.int32)
    got_img, got_gt = _run(F, dev, img, gt, mats, OUT, c, lut, table, 1, **kw)
    want_img, want_gt = plain_img.clone(), plain_gt.clone()
    want_img[2, :, -1, -1], want_gt[2, :, -1, -1] = plain_img[1, :, -1, -1], plain_gt[1, :, -1, -1]
    assert not torch.equal(want_img, plain_img)
    assert torch.equal(got_img, want_img) and torch.equal(got_gt, want_gt)


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("variant", VARIANTS)
def test_labels_absent(F, dev, variant):
    L = load_sub("_lib")
    img, gt, mats, nodes, grid, colours, need_mean, plain, wants = case_one(3, "cityscapes", variant)
    table = wants[0][0]
    want_img, none, pasted, _ = mix_reference(img, None, mats, nodes, grid, OUT, MEAN, STD, None, table, 0, IMAGE_FILL, LABEL_FILL,
                                              colours=colours, need_mean=need_mean, plain=(plain[0], None))
    assert none is None and pasted[:2].any() and not np.array_equal(want_img, plain[0])
    _equal(_run(F, dev, img, None, mats, OUT, 3, None, table, 0, nodes, grid, colours, need_mean), want_img, None)
    with pytest.raises(L.SscgError, match="sscg_augment_mix_u8"):               # the class rule reads labels: SSCG_ERR_BAD_ARG
        _run(F, dev, img, None, mats, OUT, 3, None, table, 1, nodes, grid, colours, need_mean)


# ------------------------------------------------------------------------------------------------ 4
def test_second_round_of_the_grid_stride_loop(F, dev):
    """N = 13 of 256 x 256 x 3 with labels: 212992 groups of four on the apply kernel's grid cap of 768 blocks x 256 threads = 196608,
    so 16384 threads take a second group; drawn maps, a drawn lattice at grid 32 and a table drawn with both ops at p = 1."""
    A = load_sub("data_utils.augmentations")
    comp = A.from_spec("hflip,rotate=10,scale=0.5:2,elastic=12:32,cutmix=1,classmix=1:19", (256, 256), out_size=(256, 256))
    mats = comp.matrices(np.random.RandomState(7), 13, 256, 256)
    nodes, grid = comp.fields(np.random.RandomState(8), 13, 256, 256, mats)
    table, classes = comp.mixes(np.random.RandomState(9), 13, 256, 256)
    assert grid == 32 and classes and 13 * 256 * 256 // 4 > 768 * 256 and (table[:, 0] != np.arange(13)).all() and (table[:, 5:7] != 0).all()
    img, gt = _batch(13, 256, 256, 3, seed=260)
    lut = _lut("cityscapes")
    want_img, want_gt, pasted, plain = mix_reference(img, gt, mats, nodes, grid, (256, 256), MEAN, STD, lut.numpy(), table, classes,
                                                     IMAGE_FILL, LABEL_FILL)
    assert pasted.reshape(13, -1).any(axis=1).all() and not pasted.reshape(13, -1).all(axis=1).any() and pasted[12, 128:].any()
    _equal(_run(F, dev, img, gt, mats, (256, 256), 3, lut, table, classes, nodes, grid), want_img, want_gt)


# ------------------------------------------------------------------------------------------------ 5
def test_second_round_of_the_scalar_path(F, dev):
    """Outputs that start one element behind a 16-byte boundary: no group of four, every pixel goes down the scalar path.  N = 3 of
    257 x 257, C = 1: 198147 pixels on 196608 threads, so 1539 threads take a second pixel.  augment_batch allocates its outputs, so
    the entry is called through F.lib with views of larger buffers; the elements around the views stay as they were."""
    A = load_sub("data_utils.augmentations")
    n, s, grid = 3, 257, 32
    comp = A.from_spec("hflip,rotate=10,scale=0.5:2,elastic=12:32", (s, s), out_size=(s, s))
    mats = comp.matrices(np.random.RandomState(17), n, s, s)
    nodes, _ = comp.fields(np.random.RandomState(18), n, s, s, mats)
    lo, hi = _words(BITS | 1 << 19)
    table = np.array([[1, 40, 30, 200, 120, lo, hi, 0], [2, -9, 100, 90, 300, hi, lo, 0], [0, 255, 255, 257, 257, lo, lo, 0]], dtype=np.int32)
    img, gt = _batch(n, s, s, 1, seed=270)
    lut = _lut("cityscapes")
    want_img, want_gt, pasted, _ = mix_reference(img, gt, mats, nodes, grid, (s, s), MEAN[:1], STD[:1], lut.numpy(), table, 1, IMAGE_FILL,
                                                 LABEL_FILL)
    assert n * s * s == 198147 > 768 * 256 and pasted[2, -1, -1] and not pasted.reshape(n, -1).all(axis=1).any()
    total = n * s * s
    buf_img = torch.full((total + 8,), -7.0, dtype=torch.float32, device=dev)
    buf_gt = torch.full((total + 8,), -7, dtype=torch.int64, device=dev)
    out_img, out_gt = buf_img[5:5 + total], buf_gt[3:3 + total]
    assert out_img.data_ptr() % 16 == 4 and out_gt.data_ptr() % 16 == 8
    d = [_t(dev, a) for a in (img, gt, mats, nodes, table)]
    mean, std, dlut = torch.tensor(MEAN[:1], device=dev), torch.tensor(STD[:1], device=dev), lut.to(dev)
    gh, gw = lattice_shape(grid, s, s)
    rc = F.lib.sscg_augment_mix_u8(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out_img.data_ptr(), out_gt.data_ptr(), n, s, s, 1, s, s,
                                   mean.data_ptr(), std.data_ptr(), dlut.data_ptr(), IMAGE_FILL, LABEL_FILL, None, 0, None, d[3].data_ptr(), grid,
                                   gh, gw, d[4].data_ptr(), 1, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(out_img.cpu().reshape(n, s, s, 1), torch.from_numpy(want_img))
    assert torch.equal(out_gt.cpu().reshape(n, s, s), torch.from_numpy(want_gt))
    assert bool((buf_img[:5] == -7).all()) and bool((buf_img[5 + total:] == -7).all())
    assert bool((buf_gt[:3] == -7).all()) and bool((buf_gt[3 + total:] == -7).all())


# ------------------------------------------------------------------------------------------------ 6
def test_device_loader_draws_from_four_generators_and_repeats_for_a_seed(F, dev):
    from torch.utils.data import DataLoader
    du, A = load_sub("data_utils"), load_sub("data_utils.augmentations")
    h, w, n, bs, seed = 40, 50, 6, 3, 123
    img, gt = _batch(n, h, w, 3, seed=170)
    items = [(torch.from_numpy(img[i]), torch.from_numpy(gt[i]), "s%d" % i) for i in range(n)]
    tr = du.get_transformation((h, w), dataset="cityscapes", device_finish=True)
    spec = "hflip,rotate=10,elastic=6:16,brightness=0.3"
    make = lambda sp: A.from_spec(sp, (h, w), image_fill=IMAGE_FILL, label_fill=LABEL_FILL, out_size=(33, 41))
    comp, bare = make(spec + ",cutmix=1,classmix=1:19"), make(spec)
    load = lambda cm, sd: du.DeviceLoader(DataLoader(items, batch_size=bs, shuffle=False), tr, dev, augmentation=cm, seed=sd)
    rng, crng, erng, mrng = (np.random.RandomState(seed + off) for off in (0, A.COLOUR_SEED_OFFSET, A.ELASTIC_SEED_OFFSET, A.MIX_SEED_OFFSET))
    first, plains = [], []
    for k, (bi, bg, names) in enumerate(load(comp, seed)):
        mats = comp.matrices(rng, bs, w, h)
        tables, need_mean = comp.colours(crng, bs, 3)
        nodes, grid = comp.fields(erng, bs, w, h, mats)
        table, classes = comp.mixes(mrng, bs, 41, 33)
        sl = slice(k * bs, (k + 1) * bs)
        ri, rg, pasted, plain = mix_reference(img[sl], gt[sl], mats, nodes, grid, (33, 41), tr["mean"], tr["std"], tr["lut"].numpy(), table,
                                              classes, IMAGE_FILL, LABEL_FILL, colours=tables, need_mean=need_mean)
        assert classes and not (table[:, 5] & (1 << 19)).any() and pasted.reshape(bs, -1).any(axis=1).all()
        assert tuple(bi.shape) == (bs, 3, 33, 41) and list(names) == ["s%d" % i for i in range(sl.start, sl.stop)]
        assert torch.equal(bi.permute(0, 2, 3, 1).cpu(), torch.from_numpy(ri)) and torch.equal(bg[:, 0].cpu(), torch.from_numpy(rg))
        first.append((bi, bg))
        plains.append(plain)
    assert len(first) == 2
    # the same loader without the mix items yields exactly the unmixed batches: the other three generators are untouched
    for (bi, bg, _), (pi, pg) in zip(load(bare, seed), plains):
        assert torch.equal(bi.permute(0, 2, 3, 1).cpu(), torch.from_numpy(pi)) and torch.equal(bg[:, 0].cpu(), torch.from_numpy(pg))
    again = list(load(comp, seed))
    assert len(again) == 2 and all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(first, again))
    other = next(iter(load(comp, seed + 1)))
    assert not torch.equal(other[0], first[0][0])


# ------------------------------------------------------------------------------------------------ 7
def test_without_a_mix_item_the_new_entry_is_never_reached(F, dev, monkeypatch):
    from torch.utils.data import DataLoader
    du, A = load_sub("data_utils"), load_sub("data_utils.augmentations")
    img, gt = _batch(6, 11, 13, 3, seed=180)
    items = [(torch.from_numpy(img[i]), torch.from_numpy(gt[i]), "s%d" % i) for i in range(6)]
    tr = du.get_transformation((11, 13), dataset="cityscapes", device_finish=True)
    calls = []
    for name in ("sscg_augment_u8", "sscg_augment_colour_u8", "sscg_augment_elastic_u8", "sscg_augment_mix_u8"):
        real = getattr(F.lib, name)
        monkeypatch.setattr(F.lib, name, lambda *a, _real=real, _name=name: calls.append(_name) or _real(*a))

    def run(spec):
        del calls[:]
        comp = A.from_spec(spec, (11, 13), out_size=(7, 9))
        for _ in du.DeviceLoader(DataLoader(items, batch_size=3, shuffle=False), tr, dev, augmentation=comp, seed=1):
            pass
        return list(calls)
    assert run("hflip,rotate=10") == ["sscg_augment_u8"] * 2
    assert run("hflip,contrast=0.3") == ["sscg_augment_colour_u8"] * 2
    assert run("hflip,elastic=1:4,contrast=0.3") == ["sscg_augment_elastic_u8"] * 2
    for spec in ("hflip,cutmix=0.5", "classmix=0.5:19,contrast=0.3", "hflip,elastic=1:4,contrast=0.3,cutmix=0,classmix=0"):
        assert run(spec) == ["sscg_augment_mix_u8"] * 2, spec


# ------------------------------------------------------------------------------------------------ 8
def test_table_tensors_are_checked(F, dev):
    L = load_sub("_lib")
    img, _ = _batch(2, 11, 13, 3, seed=190)
    mats = np.tile(np.array([65536, 0, 0, 0, 65536, 0], dtype=np.int32), (2, 1))
    mean, std = torch.tensor(MEAN, device=dev), torch.tensor(STD, device=dev)
    good = np.zeros((2, 8), dtype=np.int32)
    t = lambda a: _t(dev, a)
    for bad in (torch.from_numpy(good), t(good).long(), t(good)[:1], t(good)[:, :7], t(good).reshape(16), good):
        with pytest.raises(L.SscgError, match="mix table"):
            F.augment_batch(t(img), None, t(mats), (11, 13), mean, std, None, mix=(bad, 0))
    with pytest.raises(L.SscgError):                                         # two channels: SSCG_ERR_UNSUPPORTED, with or without a colour table
        F.augment_batch(t(img[..., :2].copy()), None, t(mats), (11, 13), mean[:2], std[:2], None, mix=(t(good), 0))
    out, none = F.augment_batch(t(img), None, t(mats), (11, 13), mean, std, None, mix=(t(good), 0))
    assert none is None and tuple(out.shape) == (2, 3, 11, 13)
