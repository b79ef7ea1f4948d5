"""Input pipeline with the wire format of the reference's `data_utils`:
img f32 [B,3|1,H,W] = Normalize(.5,.5)(ToTensor(CenterCrop(Resize(PIL)))), gt int64 [B,1,H,W], name str
(data_utils/__init__.py:117-187, dataloader.py:15-393).

Two modes of `get_transformation`:
  * host (default; drop-in): every transform runs on the CPU and returns what the reference's returns;
  * `device_finish=True` (what `main.py` uses): the PIL part (decode, Resize, CenterCrop - the same PIL calls
    torchvision's PIL backend makes) stays on the host, the sample crosses PCIe as uint8, and ToTensor + Normalize /
    ToLabel + Relabel / Cityscapes encode_segmap run batched on the MI355X (`sscg_image_u8_to_f32`,
    `sscg_label_lut`): a quarter of the host->device bytes and no per-sample float work on the host cores.
torchvision is not a dependency: Resize / CenterCrop / ToTensor / Normalize are restated below on PIL + numpy.

Augmentation (`augmentations.py`; the reference has the module and never uses it) is opt-in - `main.py --augment`,
`build_loaders` reading `args.augment` - and only for the 'label' and 'unlabel' sets.  Its ops are affine maps, not pixel
code: in `device_finish` mode `DeviceLoader(..., augmentation=)` draws one map per sample on the host, uploads the int32
matrices with the batch and finishes the batch with ONE `sscg_augment_u8` launch (warp + ToTensor + Normalize + label table)
instead of the two passes above; in host mode the same maps go through PIL as the datasets' `augmentation=`.  Colour items
(brightness, contrast, saturation, hue, gray) compose into one small table per sample that the same launch applies
(`sscg_augment_colour_u8`; a contrast item adds a sum pass for the image mean).  An `elastic=` item adds a non-rigid warp to the same
launch (`sscg_augment_elastic_u8`): a coarse lattice of control nodes per sample, drawn on the host, interpolated per output pixel on
the device; in host mode the same integer definition runs in numpy instead of PIL.  `cutmix=` / `classmix=` items combine two
samples of a batch, labels with pixels, inside that launch too (`sscg_augment_mix_u8`) - for the 'label' set only and in
`device_finish` mode only: there is no per-sample host path for a batch operation.  Without an augmentation nothing changes: the
same two launches as before."""
import numpy as np
import torch
from PIL import Image

from . import augmentations
from .dataloader import VOCDataset, CityscapesDataset, ACDCDataset   # noqa: F401  (reference: `from data_utils import ...`)

BILINEAR, NEAREST = 2, 0     # PIL.Image filter ids (torchvision's `interpolation=` ints)


class Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


class Resize:
    """torchvision.transforms.Resize on a PIL image with an (h, w) size: `img.resize((w, h), interpolation)`."""

    def __init__(self, size, interpolation=BILINEAR):
        self.size, self.interpolation = size, interpolation

    def __call__(self, img):
        if isinstance(self.size, int):                    # shorter side -> size, aspect kept
            w, h = img.size
            if (w <= h and w == self.size) or (h <= w and h == self.size):
                return img
            if w < h:
                return img.resize((self.size, int(self.size * h / w)), self.interpolation)
            return img.resize((int(self.size * w / h), self.size), self.interpolation)
        return img.resize(tuple(self.size[::-1]), self.interpolation)


class CenterCrop:
    """torchvision.transforms.CenterCrop on a PIL image: zero-pad if smaller, then crop at round((dim - crop) / 2)."""

    def __init__(self, size):
        self.size = (size, size) if isinstance(size, int) else tuple(size)

    def __call__(self, img):
        ch, cw = self.size
        w, h = img.size
        if cw > w or ch > h:
            left, top = (cw - w) // 2 if cw > w else 0, (ch - h) // 2 if ch > h else 0
            right, bottom = (cw - w + 1) // 2 if cw > w else 0, (ch - h + 1) // 2 if ch > h else 0
            padded = Image.new(img.mode, (w + left + right, h + top + bottom), 0)
            if img.mode == "P":
                padded.putpalette(img.getpalette())
            padded.paste(img, (left, top))
            img = padded
            w, h = img.size
            if cw == w and ch == h:
                return img
        top, left = int(round((h - ch) / 2.0)), int(round((w - cw) / 2.0))
        return img.crop((left, top, left + cw, top + ch))


def _hwc_u8(pic):
    a = np.array(pic)
    if a.dtype != np.uint8:
        raise TypeError("8-bit images expected (mode %s)" % pic.mode)
    return a[:, :, None] if a.ndim == 2 else a


class ToTensor:
    """PIL (uint8) -> float32 CHW in [0, 1]."""

    def __call__(self, pic):
        return torch.from_numpy(np.ascontiguousarray(_hwc_u8(pic).transpose(2, 0, 1))).to(torch.float32).div(255)


class Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, t):
        m = torch.tensor(self.mean, dtype=t.dtype).view(-1, 1, 1)
        s = torch.tensor(self.std, dtype=t.dtype).view(-1, 1, 1)
        return t.sub(m).div(s)


class ToU8:
    """device_finish mode: PIL -> uint8 HWC tensor (ToTensor + Normalize happen on the MI355X)."""

    def __call__(self, pic):
        return torch.from_numpy(np.ascontiguousarray(_hwc_u8(pic)))


class ToLabel:
    """PIL label map -> int64 [1, H, W] (data_utils/__init__.py:52-58)."""

    def __call__(self, image):
        return torch.from_numpy(np.array(image)).long().unsqueeze(0)


class ToLabelU8:
    def __call__(self, image):
        a = np.array(image)
        if a.dtype != np.uint8:
            raise TypeError("8-bit label maps expected (mode %s)" % image.mode)
        return torch.from_numpy(np.ascontiguousarray(a))


class Relabel:
    """tensor[tensor == olabel] = nlabel (data_utils/__init__.py:34-50)."""

    def __init__(self, olabel, nlabel):
        self.olabel, self.nlabel = olabel, nlabel

    def __call__(self, tensor):
        assert tensor.dtype == torch.int64, 'tensor needs to be LongTensor'
        tensor[tensor == self.olabel] = self.nlabel
        return tensor


CITYSCAPES_VOID = [0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30, -1]
CITYSCAPES_VALID = [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33]


def cityscapes_encode(mask):
    """CityscapesDataset.encode_segmap (dataloader.py:260-267): void ids -> 250 -> 19, valid ids -> 0..18, in place and
    in the reference's order (the order matters for an in-place remap; see label_table)."""
    for v in CITYSCAPES_VOID:
        mask[mask == v] = 250
    for i, v in enumerate(CITYSCAPES_VALID):
        mask[mask == v] = i
    mask[mask == 250] = 19
    return mask


def label_table(dataset):
    """The 256-entry table `sscg_label_lut` applies: the host-side label transforms run on every possible uint8 id."""
    t = torch.arange(256, dtype=torch.int64)
    if dataset == 'voc2012':
        t = Relabel(255, 0)(t)
    elif dataset == 'cityscapes':
        t = cityscapes_encode(t)
    return t


def get_transformation(size, resize=False, dataset='voc2012', device_finish=False):
    """data_utils/__init__.py:117-187.  `size` = (height, width)."""
    assert dataset in ['voc2012', 'cityscapes', 'acdc'], 'The dataset name must be set correctly in the get_transformation function'
    nch = 1 if dataset == 'acdc' else 3
    head = [Resize(size), CenterCrop(size)] if resize else [CenterCrop(size)]
    head_gt = [Resize(size, interpolation=NEAREST), CenterCrop(size)] if resize else [CenterCrop(size)]
    if device_finish:
        return {'img': Compose(head + [ToU8()]), 'gt': Compose(head_gt + [ToLabelU8()]), 'device_finish': True,
                'lut': label_table(dataset), 'mean': [.5] * nch, 'std': [.5] * nch}
    tail_gt = [ToLabel()] + ([Relabel(255, 0)] if dataset == 'voc2012' else [])   # 255 (boundaries) -> 0
    return {'img': Compose(head + [ToTensor(), Normalize([.5] * nch, [.5] * nch)]), 'gt': Compose(head_gt + tail_gt)}


class DeviceLoader:
    """Wraps a torch DataLoader over a dataset built with `device_finish=True` transforms and yields what the step
    consumes - (img f32 [B,C,H,W] channels-last on the MI355X, gt int64 [B,1,H,W], names) - or (img, names) for the
    'test' split.  Batches cross PCIe as uint8 from pinned memory; the float conversion is one HIP launch per batch.
    `augmentation` (an `augmentations.Compose`, default None = nothing changes): every sample is warped by an affine map of its own
    inside the finish - the maps of a batch are drawn on the host from `RandomState(seed)`, in batch order, uploaded with the batch
    and applied by one `functional.augment_batch` launch that replaces the two passes.  When the augmentation has colour ops, their
    per-sample table is drawn from a second generator, `RandomState(seed + augmentations.COLOUR_SEED_OFFSET)`, and travels with the
    maps; the geometric draws of a seed do not depend on it.  An elastic op likewise: the control lattices of a batch are drawn from a
    third generator, `RandomState(seed + augmentations.ELASTIC_SEED_OFFSET)`, uploaded with the maps and interpolated inside the same
    launch (`sscg_augment_elastic_u8`); without one there is no further upload and no other launch than before.  Mix ops likewise:
    the table of a batch (partner, box, class mask per sample) is drawn from a fourth generator, `RandomState(seed +
    augmentations.MIX_SEED_OFFSET)`, uploaded with the maps and applied per output pixel inside the same launch
    (`sscg_augment_mix_u8`); without one nothing is drawn, uploaded or launched that was not before."""

    def __init__(self, loader, transformation, device, augmentation=None, seed=0):
        if not transformation.get('device_finish'):
            raise ValueError("DeviceLoader needs get_transformation(..., device_finish=True)")
        self.loader, self.device = loader, device
        self.augmentation, self.rng = augmentation, np.random.RandomState(seed)
        self.colour_rng = np.random.RandomState(seed + augmentations.COLOUR_SEED_OFFSET)
        self.elastic_rng = np.random.RandomState(seed + augmentations.ELASTIC_SEED_OFFSET)
        self.mix_rng = np.random.RandomState(seed + augmentations.MIX_SEED_OFFSET)
        self.lut = transformation['lut'].to(device)
        self.mean = torch.tensor(transformation['mean'], dtype=torch.float32, device=device)
        self.std = torch.tensor(transformation['std'], dtype=torch.float32, device=device)

    def __len__(self):
        return len(self.loader)

    def _up(self, t):
        t = t.contiguous()
        return (t.pin_memory() if self.device.type == "cuda" else t).to(self.device, non_blocking=True)

    def __iter__(self):
        from .. import functional as F
        for batch in self.loader:
            if self.augmentation is not None:
                yield self._augmented(F, batch)
                continue
            img = F.image_u8_to_f32(self._up(batch[0]), self.mean, self.std)
            if len(batch) == 2:
                yield img, batch[1]
            else:
                yield img, F.label_lut(self._up(batch[1]), self.lut), batch[2]


    def _augmented(self, F, batch):
        aug = self.augmentation
        b, h, w, c = batch[0].shape
        drawn = aug.matrices(self.rng, b, w, h)
        mats = self._up(torch.from_numpy(drawn))
        gt = self._up(batch[1]) if len(batch) == 3 else None
        extra = {}
        if aug.colour_ops:
            table, need_mean = aug.colours(self.colour_rng, b, c)
            extra = {"colour": self._up(torch.from_numpy(table)), "need_mean": need_mean}
        if aug.elastic_ops:
            nodes, grid = aug.fields(self.elastic_rng, b, w, h, drawn)
            extra["elastic"] = (self._up(torch.from_numpy(nodes)), grid)
        if aug.mix_ops:
            oh, ow = aug.out_size or (h, w)
            table, classes = aug.mixes(self.mix_rng, b, ow, oh)
            extra["mix"] = (self._up(torch.from_numpy(table)), classes and gt is not None)
        img, gt = F.augment_batch(self._up(batch[0]), gt, mats, aug.out_size or (h, w), self.mean, self.std, self.lut,
                                  image_fill=aug.image_fill, label_fill=aug.label_fill, **extra)
        return (img, batch[1]) if gt is None else (img, gt, batch[2])


LABEL_FILL = {'voc2012': 255, 'cityscapes': 250, 'acdc': 0}   # raw ids: the tables map 255 -> 0 (as boundaries), 250 -> 19 (void)
AUGMENT_SEED = 20261017


def build_loaders(args, roots=None, device=None, sets=('label', 'unlabel', 'val'), rank=0):
    """The datasets and DataLoaders of model.py:315-348 (ratios 0.1/0.1/0.5 for VOC, 0.5 otherwise; batch_size, shuffle and
    drop_last on all three, as written there), finished on `device` when one is given.  `args.augment` (absent or "" = none; the
    comma list of augmentations.from_spec) augments the 'label' and 'unlabel' sets, never 'val' or 'test': inside the device finish
    when there is a device, through the datasets' `augmentation=` (PIL, before Resize / CenterCrop) otherwise; rank r draws from
    `RandomState(AUGMENT_SEED + 1000 * r + <index of the set>)`.  The mix items (`cutmix=`, `classmix=`) go to the 'label' set
    only - the 'unlabel' set is built from the spec without them, its draws unchanged - and need the device finish: in host mode a spec
    with one raises ValueError.  `args.sliding` (absent or "" = off; utils.parse_sliding's grammar): the 'val' and 'test' sets get a
    transformation of their own at the evaluation size (images bilinear, ground truth nearest neighbour); the 'label' / 'unlabel' sets
    keep the crop and their draws."""
    roots = roots or {'voc2012': './data/VOC2012', 'cityscapes': './data/Cityscape', 'acdc': './data/ACDC'}
    from torch.utils.data import DataLoader
    tr = get_transformation((args.crop_height, args.crop_width), resize=True, dataset=args.dataset, device_finish=device is not None)
    cls = {'voc2012': VOCDataset, 'cityscapes': CityscapesDataset, 'acdc': ACDCDataset}[args.dataset]
    out = []
    size = (args.crop_height, args.crop_width)
    tr_eval = tr
    if (getattr(args, 'sliding', '') or '').strip():
        from ..utils import parse_sliding
        tr_eval = get_transformation(parse_sliding(args.sliding, size).size, resize=True, dataset=args.dataset, device_finish=device is not None)
    spec = getattr(args, 'augment', '') or ''
    is_mix = lambda item: item.strip().partition('=')[0] in ('cutmix', 'classmix')
    unmixed = ','.join(item for item in spec.split(',') if not is_mix(item))
    if device is None and any(is_mix(item) for item in spec.split(',')):
        raise ValueError("--augment: cutmix / classmix combine the samples of a batch inside the device finish; there is no host path "
                         "for them (given %r without a device)" % spec)
    for name in sets:
        ratio = 0.5 if (args.dataset != 'voc2012' or name in ('val', 'test')) else 0.1
        seed = AUGMENT_SEED + 1000 * rank + len(out)
        aug = augmentations.from_spec(spec if name == 'label' else unmixed, size, label_fill=LABEL_FILL[args.dataset], seed=seed,
                                      out_size=size if device is not None else None) if name in ('label', 'unlabel') else None
        trn = tr if name in ('label', 'unlabel') else tr_eval
        ds = cls(root_path=roots[args.dataset], name=name, ratio=ratio, transformation=trn, augmentation=aug if device is None else None)
        gen = torch.Generator().manual_seed(20260928 + 1000 * rank + len(out)) if rank else None   # ranks draw different batches
        ld = DataLoader(ds, batch_size=args.batch_size, shuffle=True, drop_last=True, generator=gen)
        out.append(DeviceLoader(ld, trn, device, augmentation=aug, seed=seed) if device is not None else ld)
    return out
