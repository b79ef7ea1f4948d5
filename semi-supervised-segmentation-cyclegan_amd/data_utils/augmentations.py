"""Geometric augmentations as affine maps.  The class names and constructor arguments are those of the reference's
`data_utils/augmentations.py` (RandomCrop, CenterCrop, RandomRotate, Scale, RandomSizedCrop, RandomSized, Compose, plus
RandomHorizontallyFlip and RandomScale); the implementation is not: no op touches a pixel.  Every op only answers

    matrix(rng, w, h) -> (M, (w2, h2))

with M a 3x3 float64 map from CONTINUOUS OUTPUT coordinates to continuous input coordinates of a (w, h) view (pixel x covers
[x, x+1), so its centre is x + .5) and (w2, h2) the size of the view it leaves; `rng` is a numpy.random.RandomState.  `Compose`
multiplies the maps of its ops, so a whole pipeline costs one resampling however long it is, and hands the product to one of two
back ends:

  * the device: `Compose.matrices(rng, n, w, h)` draws a batch and rounds each map to the six int32 Q16 coefficients (`to_q16`)
    that `functional.augment_batch` (sscg_augment_u8, include/sscg.h) applies inside the batch finish - `DeviceLoader(...,
    augmentation=)`;
  * the host: `Compose.__call__(img, mask)` (and the one-argument form of the 'test' split) applies the same float map with
    `PIL.Image.transform(AFFINE)`, bilinear for the image and nearest for the mask - what the datasets' `augmentation=` takes.

The two agree exactly on maps that land on pixel centres (identity, flips, integer crops and pads).  Elsewhere they differ by
design: the device path is bilinear with 8-bit weights, treats every tap outside the source as the fill colour (PIL extends the
edge pixel half a pixel outwards) and, like PIL's AFFINE transform, does not antialias when it minifies.  Labels agree wherever the
nearest source index is not a tie.  There is no photometric jitter here."""
import math

import numpy as np
from PIL import Image

Q16 = 65536


def _pair(size):
    """(height, width), the argument order of the reference's crop ops."""
    return (int(size), int(size)) if isinstance(size, (int, float)) else (int(size[0]), int(size[1]))


def _affine(a=1.0, b=0.0, c=0.0, d=0.0, e=1.0, f=0.0):
    return np.array([[a, b, c], [d, e, f], [0.0, 0.0, 1.0]], dtype=np.float64)


def _resize(w, h, w2, h2):
    """The (w2, h2) view that shows the whole (w, h) one."""
    return _affine(a=w / float(w2), e=h / float(h2)), (w2, h2)


def to_q16(M):
    """The six int32 coefficients of sscg_augment_u8 for the map M: it works on pixel INDICES, so the centre offsets of both grids
    (+.5 on the output side, -.5 on the input side) are folded into the two translations."""
    M = np.asarray(M, dtype=np.float64)
    q = [M[0, 0], M[0, 1], M[0, 0] * .5 + M[0, 1] * .5 + M[0, 2] - .5,
         M[1, 0], M[1, 1], M[1, 0] * .5 + M[1, 1] * .5 + M[1, 2] - .5]
    q = [int(round(v * Q16)) for v in q]
    if max(abs(v) for v in q) >= 2 ** 31:
        raise ValueError("affine map out of the Q16 range of int32: %r" % (q,))
    return np.array(q, dtype=np.int32)


class RandomHorizontallyFlip:
    def __init__(self, p=0.5):
        self.p = p

    def matrix(self, rng, w, h):
        flip = rng.random_sample() < self.p
        return (_affine(a=-1.0, c=float(w)) if flip else _affine()), (w, h)


class RandomRotate:
    """Angle uniform in +-degree, about the centre of the view; the size stays."""

    def __init__(self, degree):
        self.degree = degree

    def matrix(self, rng, w, h):
        t = math.radians(rng.uniform(-self.degree, self.degree))
        co, si = math.cos(t), math.sin(t)
        cx, cy = w / 2.0, h / 2.0
        return _affine(co, -si, cx - co * cx + si * cy, si, co, cy - si * cx - co * cy), (w, h)


class RandomScale:
    """Zoom by a factor uniform in lo..hi about the centre of the view; the size stays (what `--augment scale=lo:hi` builds)."""

    def __init__(self, lo, hi):
        self.lo, self.hi = float(lo), float(hi)

    def matrix(self, rng, w, h):
        s = 1.0 / rng.uniform(self.lo, self.hi)
        return _affine(a=s, c=w / 2.0 * (1.0 - s), e=s, f=h / 2.0 * (1.0 - s)), (w, h)


class RandomCrop:
    """A (th, tw) window at a uniformly drawn integer offset; a view too small for the window is resized to it."""

    def __init__(self, size):
        self.size = _pair(size)

    def matrix(self, rng, w, h):
        th, tw = self.size
        if w == tw and h == th:
            return _affine(), (w, h)
        if w < tw or h < th:
            return _resize(w, h, tw, th)
        x1, y1 = int(rng.randint(0, w - tw + 1)), int(rng.randint(0, h - th + 1))
        return _affine(c=float(x1), f=float(y1)), (tw, th)


class CenterCrop:
    """Offset round((dim - crop) / 2); a negative offset pads with the fill."""

    def __init__(self, size):
        self.size = _pair(size)

    def matrix(self, rng, w, h):
        th, tw = self.size
        x1, y1 = int(round((w - tw) / 2.)), int(round((h - th) / 2.))
        return _affine(c=float(x1), f=float(y1)), (tw, th)


class Scale:
    """Longer side to `size`, the other to int(size * short / long)."""

    def __init__(self, size):
        self.size = int(size)

    def matrix(self, rng, w, h):
        if (w >= h and w == self.size) or (h >= w and h == self.size):
            return _affine(), (w, h)
        if w > h:
            return _resize(w, h, self.size, max(1, int(self.size * h / w)))
        return _resize(w, h, max(1, int(self.size * w / h)), self.size)


class RandomSizedCrop:
    """A window of 45..100 % of the area and aspect 0.5..2 (10 attempts), resized to `size`; fallback Scale + CenterCrop."""

    def __init__(self, size):
        self.size = _pair(size)

    def matrix(self, rng, w, h):
        th, tw = self.size
        for _ in range(10):
            target = rng.uniform(0.45, 1.0) * w * h
            aspect = rng.uniform(0.5, 2.0)
            cw, ch = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
            if rng.random_sample() < 0.5:
                cw, ch = ch, cw
            if 0 < cw <= w and 0 < ch <= h:
                x1, y1 = int(rng.randint(0, w - cw + 1)), int(rng.randint(0, h - ch + 1))
                return _affine(a=cw / float(tw), c=float(x1), e=ch / float(th), f=float(y1)), (tw, th)
        m1, (w1, h1) = Scale(max(th, tw)).matrix(rng, w, h)
        m2, out = CenterCrop(self.size).matrix(rng, w1, h1)
        return m1.dot(m2), out


class RandomSized:
    """Each side times a uniform draw in 0.5..2 (truncated), then Scale(size), then RandomCrop(size)."""

    def __init__(self, size):
        self.size = int(size)
        self.scale, self.crop = Scale(self.size), RandomCrop(self.size)

    def matrix(self, rng, w, h):
        w1, h1 = max(1, int(rng.uniform(0.5, 2) * w)), max(1, int(rng.uniform(0.5, 2) * h))
        m, _ = _resize(w, h, w1, h1)
        m2, (w2, h2) = self.scale.matrix(rng, w1, h1)
        m3, out = self.crop.matrix(rng, w2, h2)
        return m.dot(m2).dot(m3), out


class Compose:
    """The product of the ops' maps.  `out_size` = (height, width): a centre crop (or pad) is appended when the ops end elsewhere,
    so every sample of a batch leaves with the same shape.  `image_fill` / `label_fill` (0..255) colour what lies outside the
    source; the label fill is a raw id (the label transforms behind it see it like any pixel).  `seed` seeds the generator of the
    host path (`__call__`); the device path is handed its generator by the caller."""

    def __init__(self, ops, out_size=None, image_fill=0, label_fill=0, seed=None):
        self.ops = list(ops)
        self.out_size = _pair(out_size) if out_size is not None else None
        self.image_fill, self.label_fill = int(image_fill), int(label_fill)
        self.rng = np.random.RandomState(seed)

    def matrix(self, rng, w, h):
        M = _affine()
        for op in self.ops:
            m, (w, h) = op.matrix(rng, w, h)
            M = M.dot(m)
        if self.out_size is not None and (h, w) != self.out_size:
            m, (w, h) = CenterCrop(self.out_size).matrix(rng, w, h)
            M = M.dot(m)
        return M, (w, h)

    def matrices(self, rng, n, w, h):
        """int32 [n, 6]: one drawn map per sample of a batch of (w, h) images, as sscg_augment_u8 reads them."""
        return np.stack([to_q16(self.matrix(rng, w, h)[0]) for _ in range(n)]).astype(np.int32)

    def __call__(self, img, mask=None):
        w, h = img.size
        assert mask is None or mask.size == img.size
        M, out = self.matrix(self.rng, w, h)
        coef = tuple(float(v) for v in M[:2].reshape(-1))
        fill = self.image_fill if len(img.getbands()) == 1 else (self.image_fill,) * len(img.getbands())
        img = img.transform(out, Image.AFFINE, coef, Image.BILINEAR, fillcolor=fill)
        if mask is None:
            return img
        return img, mask.transform(out, Image.AFFINE, coef, Image.NEAREST, fillcolor=self.label_fill)


def from_spec(spec, size, image_fill=0, label_fill=0, out_size=None, seed=None):
    """The augmentation a `--augment` value names, or None for an empty one: a comma list of `hflip`, `rotate=<deg>`,
    `scale=<lo>:<hi>` and `sizedcrop` (RandomSizedCrop to `size` = (height, width)), applied in the order written."""
    ops = []
    for item in (s.strip() for s in (spec or "").split(",")):
        if not item:
            continue
        key, _, val = item.partition("=")
        if key == "hflip" and not val:
            ops.append(RandomHorizontallyFlip(0.5))
        elif key == "rotate" and val:
            ops.append(RandomRotate(float(val)))
        elif key == "scale" and val.count(":") == 1:
            lo, hi = (float(v) for v in val.split(":"))
            if not 0.0 < lo <= hi:
                raise ValueError("--augment scale=<lo>:<hi> needs 0 < lo <= hi, given %r" % item)
            ops.append(RandomScale(lo, hi))
        elif key == "sizedcrop" and not val:
            ops.append(RandomSizedCrop(size))
        else:
            raise ValueError("--augment: unknown item %r (hflip, rotate=<deg>, scale=<lo>:<hi>, sizedcrop)" % item)
    return Compose(ops, out_size=out_size, image_fill=image_fill, label_fill=label_fill, seed=seed) if ops else None
