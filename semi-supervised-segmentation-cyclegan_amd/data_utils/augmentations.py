"""Geometric and colour augmentations as affine maps.  The class names and constructor arguments are those of the reference's
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
nearest source index is not a tie.

Colour jitter has the same structure.  Brightness, saturation, hue rotation and random grey are linear maps of RGB and contrast is
affine in the pixel and the image mean, so every colour op only answers

    colour(rng, channels) -> (M, None)  a linear map of the channels,  or  (None, c)  a contrast factor

and `Compose` folds the colour ops of a pipeline, in the order written and after the geometry, into one state (A, B, b) per sample:

    x = A.v + B.mu + b          v the warped pixel in [0, 1], mu the mean of v over the sample's whole output (fill included)

`Compose.colours(rng, n, channels)` draws a batch of states as the float32 [n, 21] table that sscg_augment_colour_u8 applies inside
the same launch that warps; `Compose.__call__` applies the same float32 formula in numpy behind the PIL transform.  Not
torchvision's ColorJitter, by design: values are clamped to [0, 1] once, at the end, not after every op, and the ops apply in the
order written, not in a random one.  Colour draws come from a generator of their own (`seed + COLOUR_SEED_OFFSET`), so the geometric
maps of a seed are the same with and without colour items.  One-channel images: the state is scalar (luma = the channel);
saturation, hue and grey are the identity.

Elastic deformation is the one geometric op that is not an affine map, and it keeps the rule all the same: `RandomElastic` touches no
pixel, it only answers

    field(rng, gh, gw) -> float64 [gh, gw, 2]   node offsets (x, y) in OUTPUT pixels, uniform in [-alpha, alpha]

on a coarse control lattice laid over the FINAL output view (wherever the item stands in the list), one node every `grid` output
pixels.  `Compose.fields(rng, n, w, h, mats)` draws a batch of lattices, multiplies each sample's 2x2 linear part into its lattice
(a displacement of the output coordinate is one of L times as much in the source) and rounds to the int32 Q16 nodes that
sscg_augment_elastic_u8 (include/sscg.h) interpolates with a cubic B-spline per output pixel and adds to the affine source
coordinate - still one resampling, in the same launch.  The spline is a convex combination of the nodes, so no pixel moves by more
than alpha.  The definition is integers throughout, so with an elastic op the host path (`Compose.__call__`) does not go through PIL
either: it evaluates the same integer definition in numpy (`elastic_displacement`, `warp_u8`), affine and elastic part together,
and returns the integer pixel value rounded to uint8 - the device's pixels and labels.  Elastic draws come from a third generator
(`seed + ELASTIC_SEED_OFFSET`): the maps and colour tables of a seed are the same with and without the item.

Mixed-sample augmentation (`RandomCutMix`, `RandomClassMix`) combines two samples of a BATCH, labels with pixels, and touches no
pixel either: a mix op only answers

    mix(rng, ow, oh) -> (fires, box or None, mask or None)

and `Compose.mixes(rng, n, ow, oh)` draws the int32 [n, 8] table (partner, x0, y0, x1, y1, mask_lo, mask_hi, 0) that
sscg_augment_mix_u8 (include/sscg.h) reads: inside the one launch every output pixel is decided to be its own sample's or, pasted,
its partner's - in the box, or where the partner shows a class whose bit is set in the mask.  `mix_batch` states the same rule in
numpy on a finished batch.  There is no per-sample host path: `Compose.__call__` raises with a mix op.  Mix draws come from a fourth
generator (`seed + MIX_SEED_OFFSET`): the maps, colour tables and lattices of a seed are the same with and without a mix item."""
import math

import numpy as np
from PIL import Image

Q16 = 65536
LUMA = (0.299, 0.587, 0.114)
YIQ = np.array([[.299, .587, .114], [.596, -.274, -.322], [.211, -.523, .312]], dtype=np.float64)   # NTSC; row 0 is LUMA, rows 1, 2 sum to 0
YIQ_INV = np.linalg.inv(YIQ)
COLOUR_SEED_OFFSET = 500
ELASTIC_SEED_OFFSET = 900
MIX_SEED_OFFSET = 1300
ELASTIC_DEFAULT_GRID = 32          # output pixels between control nodes; an untuned default
ELASTIC_NODE_LIMIT = 2 ** 26       # |node| in Q16 source pixels (include/sscg.h)
BSPLINE_DENOM = 6 * 2 ** 24        # the common denominator of the B-spline numerators at t in 0..255


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


class RandomElastic:
    """Free-form deformation: control nodes every `grid` output pixels (>= 4), each moved by an offset uniform in [-alpha, alpha]
    output pixels per component, interpolated by a uniform cubic B-spline (sscg_augment_elastic_u8).  alpha <= 0.4 * grid is the
    control-point bound below which such a deformation cannot fold (Choi and Lee 2000); `from_spec` enforces it."""

    def __init__(self, alpha, grid=ELASTIC_DEFAULT_GRID):
        self.alpha, self.grid = float(alpha), int(grid)
        if not self.alpha >= 0.0 or self.grid < 4:            # (a NaN fails the first)
            raise ValueError("RandomElastic needs alpha >= 0 and grid >= 4, given %r, %r" % (alpha, grid))

    def field(self, rng, gh, gw):
        return rng.uniform(-self.alpha, self.alpha, (gh, gw, 2))


def _wrap_i32(a):
    """int64 values in [0, 2^32) or [-2^31, 2^31) as the int32 with the same low 32 bits."""
    return (np.asarray(a, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def lattice_shape(grid, oh, ow):
    """(GH, GW) of the control lattice over an (oh, ow) output: the cells the pixels lie in plus the three further nodes of a cubic."""
    return (oh - 1) // grid + 4, (ow - 1) // grid + 4


def bspline_numerators(t):
    """The four uniform cubic B-spline weights at t / 256, t an int64 array in 0..255, as integers over BSPLINE_DENOM: [4, ...]."""
    t = np.asarray(t, dtype=np.int64)
    u = 256 - t
    return np.stack([u * u * u, 3 * t ** 3 - 1536 * t * t + 4 * 256 ** 3, -3 * t ** 3 + 768 * t * t + 196608 * t + 256 ** 3, t ** 3])


def elastic_displacement(nodes, grid, oh, ow):
    """The displacement field of sscg_augment_elastic_u8 for one sample: nodes int [GH, GW, 2] (Q16 source pixels) -> int64
    [oh, ow, 2].  The y pass first, once per output row and node column, then the x pass; both round with floor((s + D/2) / D)."""
    nodes = np.asarray(nodes).astype(np.int64)
    assert nodes.shape == lattice_shape(grid, oh, ow) + (2,)
    D = BSPLINE_DENOM
    oy, ox = np.arange(oh, dtype=np.int64), np.arange(ow, dtype=np.int64)
    cy, cx = oy // grid, ox // grid
    ny, nx = bspline_numerators(((oy - cy * grid) * 256) // grid), bspline_numerators(((ox - cx * grid) * 256) // grid)
    rows = sum(ny[i][:, None, None] * nodes[cy + i] for i in range(4))           # [oh, GW, 2]
    rows = (rows + D // 2) // D                                                  # numpy's // floors, negative values too
    d = sum(nx[j][None, :, None] * rows[:, cx + j] for j in range(4))            # [oh, ow, 2]
    return (d + D // 2) // D


def warp_u8(img, mask, q, d, out, image_fill=0, label_fill=0):
    """The integer definition of sscg_augment_u8 / sscg_augment_elastic_u8 on one sample, in numpy: img uint8 [h, w, c], mask uint8
    [h, w] or None, q the six Q16 coefficients, d int64 [oh, ow, 2] (elastic_displacement) or None, out = (oh, ow) ->
    (uint8 [oh, ow, c], uint8 [oh, ow] or None): the pixel is the integer value v of the definition rounded to 8 bits,
    (v + 0x8000) >> 16, the label the raw id at the nearest source index (no table)."""
    h, w, _ = img.shape
    oh, ow = out
    q = [int(v) for v in q]
    oy, ox = np.meshgrid(np.arange(oh, dtype=np.int64), np.arange(ow, dtype=np.int64), indexing="ij")
    sx, sy = q[0] * ox + q[1] * oy + q[2], q[3] * ox + q[4] * oy + q[5]
    if d is not None:
        sx, sy = sx + d[..., 0], sy + d[..., 1]
    x0, y0 = sx >> 16, sy >> 16
    fx, fy = ((sx & 0xFFFF) >> 8)[..., None], ((sy & 0xFFFF) >> 8)[..., None]

    def tap(y, x):
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        return np.where(inside[..., None], img[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.int64), image_fill)
    top = tap(y0, x0) * (256 - fx) + tap(y0, x0 + 1) * fx
    bot = tap(y0 + 1, x0) * (256 - fx) + tap(y0 + 1, x0 + 1) * fx
    px = ((top * (256 - fy) + bot * fy + 0x8000) >> 16).astype(np.uint8)
    if mask is None:
        return px, None
    ix, iy = (sx + 0x8000) >> 16, (sy + 0x8000) >> 16
    inside = (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
    return px, np.where(inside, mask[np.clip(iy, 0, h - 1), np.clip(ix, 0, w - 1)], label_fill).astype(np.uint8)


class RandomCutMix:
    """With probability p a rectangle of the partner is pasted (CutMix, Yun et al. 2019): area share a uniform in [lo, hi] of the
    output, aspect rho = exp(U[-ln 2, ln 2]), bw = clamp(round(sqrt(a.ow.oh.rho)), 1, ow), bh = clamp(round(a.ow.oh / bw), 1, oh)
    (round = half up; a box too tall for its aspect is cut to the output's height), the corner uniform over the positions that
    keep the box inside.  lo = 0.25, hi = 0.5 are untuned defaults.  Five draws per call, whether or not it fires."""
    classes = False

    def __init__(self, p, lo=0.25, hi=0.5):
        self.p, self.lo, self.hi = float(p), float(lo), float(hi)
        if not 0.0 <= self.p <= 1.0 or not 0.0 < self.lo <= self.hi <= 1.0:        # (false for a NaN)
            raise ValueError("RandomCutMix needs 0 <= p <= 1 and 0 < lo <= hi <= 1, given %r, %r, %r" % (p, lo, hi))

    def mix(self, rng, ow, oh):
        u = rng.random_sample(5)
        area = (self.lo + (self.hi - self.lo) * u[1]) * ow * oh
        rho = math.exp((2.0 * u[2] - 1.0) * math.log(2.0))
        bw = min(max(int(math.floor(math.sqrt(area * rho) + 0.5)), 1), ow)
        bh = min(max(int(math.floor(area / bw + 0.5)), 1), oh)
        x0, y0 = min(int(u[3] * (ow - bw + 1)), ow - bw), min(int(u[4] * (oh - bh + 1)), oh - bh)
        return bool(u[0] < self.p), (x0, y0, x0 + bw, y0 + bh), None


class RandomClassMix:
    """With probability p every pixel of a random half of the partner's classes is pasted (ClassMix, Olsson et al. 2021; copy-paste
    by class): 64 independent fair bits, one per class id, with the bits of `skip` (ids in [0, 64) that are never pasted) cleared.
    Which classes the partner shows is not consulted - that would be a host sync - so a mask may paste nothing.  65 draws per call,
    whether or not it fires."""
    classes = True

    def __init__(self, p, skip=()):
        self.p = float(p)
        if not 0.0 <= self.p <= 1.0:
            raise ValueError("RandomClassMix needs 0 <= p <= 1, given %r" % (p,))
        self.skip = tuple(skip)
        if any(int(c) != c or not 0 <= c < 64 for c in self.skip):
            raise ValueError("RandomClassMix skips class ids in [0, 64), given %r" % (self.skip,))
        self.keep = (1 << 64) - 1 - sum(1 << int(c) for c in set(self.skip))

    def mix(self, rng, ow, oh):
        u = rng.random_sample(65)
        bits = sum(1 << c for c in range(64) if u[1 + c] < 0.5)
        return bool(u[0] < self.p), None, bits & self.keep


def mix_batch(img, gt, table, classes):
    """The rule of sscg_augment_mix_u8 on a FINISHED batch, in numpy: img [n, c, oh, ow], gt integer class maps [n, 1, oh, ow] or
    [n, oh, ow] (or None), table int [n, 8] (`Compose.mixes`), classes a flag -> (img, gt) with out[i] = where(pasted, in[p], in[i]),
    p = table[i][0] (outside [0, n) or i itself: not mixed).  Pasted: inside the half-open box x0 <= x < x1, y0 <= y < y1, or - with
    `classes`, which needs gt - where sample p's class is in [0, 64) and its bit of (mask_hi << 32) | mask_lo is set.  Every partner
    pixel is the partner's pixel before mixing."""
    img, table = np.asarray(img), np.asarray(table).astype(np.int64)
    lab = np.asarray(gt) if gt is not None else None
    n, _, oh, ow = img.shape
    if table.shape != (n, 8) or (classes and lab is None) or (lab is not None and lab.shape not in ((n, 1, oh, ow), (n, oh, ow))):
        raise ValueError("mix_batch: a table [n, 8], and labels [n, 1, oh, ow] or [n, oh, ow] with `classes`, expected")
    ys, xs = np.meshgrid(np.arange(oh), np.arange(ow), indexing="ij")
    out_img, out_lab = img.copy(), (lab.copy() if lab is not None else None)
    for i in range(n):
        p, x0, y0, x1, y1, lo, hi = (int(v) for v in table[i, :7])
        if not 0 <= p < n or p == i:
            continue
        pasted = (xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)
        if classes:
            cls = lab[p].reshape(oh, ow).astype(np.int64)
            mask = ((hi & 0xFFFFFFFF) << 32) | (lo & 0xFFFFFFFF)
            bit = np.array([mask >> c & 1 for c in range(64)], dtype=bool)
            pasted |= (cls >= 0) & (cls < 64) & bit[np.clip(cls, 0, 63)]
        out_img[i] = np.where(pasted[None], img[p], img[i])
        if lab is not None:
            out_lab[i] = np.where(pasted.reshape(lab[i].shape[-2:]), lab[p], lab[i])
    return out_img, out_lab


def _luma(channels):
    return np.array(LUMA if channels == 3 else (1.0,), dtype=np.float64)


def _factor(rng, x):
    return rng.uniform(max(0.0, 1.0 - x), 1.0 + x)


class RandomBrightness:
    """Pixel times a factor uniform in [max(0, 1-x), 1+x]."""

    def __init__(self, x):
        self.x = float(x)

    def colour(self, rng, channels):
        return _factor(rng, self.x) * np.eye(channels), None


class RandomContrast:
    """x' = c.x + (1-c).mean_luma(x), c uniform in [max(0, 1-x), 1+x]: the one op that needs the image mean."""

    def __init__(self, x):
        self.x = float(x)

    def colour(self, rng, channels):
        return None, _factor(rng, self.x)


class RandomSaturation:
    """Blend with the pixel's luma: f.I + (1-f).1w', f uniform in [max(0, 1-x), 1+x]."""

    def __init__(self, x):
        self.x = float(x)

    def colour(self, rng, channels):
        f = _factor(rng, self.x)
        if channels != 3:
            return np.eye(channels), None
        return f * np.eye(3) + (1.0 - f) * np.outer(np.ones(3), _luma(3)), None


class RandomHue:
    """Rotation of the I/Q plane of NTSC YIQ by 2.pi.h, h uniform in [-x, x], 0 <= x <= 0.5: keeps luma and grey pixels."""

    def __init__(self, x):
        self.x = float(x)

    def colour(self, rng, channels):
        t = 2.0 * math.pi * rng.uniform(-self.x, self.x)
        if channels != 3:
            return np.eye(channels), None
        co, si = math.cos(t), math.sin(t)
        R = np.array([[1.0, 0.0, 0.0], [0.0, co, -si], [0.0, si, co]], dtype=np.float64)
        return YIQ_INV.dot(R).dot(YIQ), None


class RandomGrayscale:
    """With probability p every channel becomes the pixel's luma."""

    def __init__(self, p=0.1):
        self.p = float(p)

    def colour(self, rng, channels):
        grey = rng.random_sample() < self.p
        if channels != 3 or not grey:
            return np.eye(channels), None
        return np.outer(np.ones(3), _luma(3)), None


def colour_table_row(A, B, b):
    """One row of the [n, 21] table of sscg_augment_colour_u8: A row-major, B row-major, b, rounded from float64.  A scalar state
    (one channel) sits at [0][0] and [0]; the rest of the row is the identity state."""
    k = A.shape[0]
    fa, fb, fv = np.eye(3), np.zeros((3, 3)), np.zeros(3)
    fa[:k, :k], fb[:k, :k], fv[:k] = A, B, b
    return np.concatenate([fa.reshape(-1), fb.reshape(-1), fv]).astype(np.float32)


def apply_colour(px, row, need_mean):
    """The colour stage of sscg_augment_colour_u8 on uint8 pixels [h, w, channels] of a finished warp, in numpy float32 with one
    rounding per operation: t = px / 255, mu from the integer sum, u = clamp(A.t + (B.mu + b)); -> uint8 rint(255 u)."""
    h, w, k = px.shape
    f = np.float32
    A, B, b = row[:9].reshape(3, 3), row[9:18].reshape(3, 3), row[18:21]
    t = px.astype(f) / f(255)
    mu = np.zeros(k, dtype=f)
    if need_mean:
        S = px.reshape(-1, k).astype(np.int64).sum(axis=0) * Q16
        mu = (S.astype(np.float64) / (np.float64(h * w) * np.float64(16711680.0))).astype(f)
    out = np.empty((h, w, k), dtype=f)
    for c in range(k):
        o, u = B[c, 0] * mu[0], A[c, 0] * t[..., 0]
        for j in range(1, k):
            o, u = o + B[c, j] * mu[j], u + A[c, j] * t[..., j]
        out[..., c] = np.minimum(np.maximum(u + (o + b[c]), f(0)), f(1))
    return np.rint(f(255) * out).astype(np.uint8)


class Compose:
    """The product of the ops' maps.  `out_size` = (height, width): a centre crop (or pad) is appended when the ops end elsewhere,
    so every sample of a batch leaves with the same shape.  `image_fill` / `label_fill` (0..255) colour what lies outside the
    source; the label fill is a raw id (the label transforms behind it see it like any pixel).  `seed` seeds the generators of the
    host path (`__call__`); the device path is handed its generators by the caller.  Geometric ops (those with `.matrix`) and
    colour ops (those with `.colour`) may be mixed in `ops`: each kind keeps its order, the colour runs after the geometry.  At most
    one op may be an elastic one (with `.field`): it deforms the final output view, wherever it stands.  Mix ops (with `.mix`; one
    RandomCutMix and one RandomClassMix at the most) act on a batch behind all of that: the device finish only (`mixes`)."""

    def __init__(self, ops, out_size=None, image_fill=0, label_fill=0, seed=None):
        self.ops = list(ops)
        self.geometric_ops = [op for op in self.ops if hasattr(op, "matrix")]
        self.colour_ops = [op for op in self.ops if hasattr(op, "colour")]
        self.elastic_ops = [op for op in self.ops if hasattr(op, "field")]
        if len(self.elastic_ops) > 1:
            raise ValueError("at most one elastic op in a pipeline, given %d" % len(self.elastic_ops))
        self.elastic_rng = np.random.RandomState(seed + ELASTIC_SEED_OFFSET if seed is not None else None)
        self.mix_ops = [op for op in self.ops if hasattr(op, "mix")]
        if len(self.mix_ops) > len({bool(op.classes) for op in self.mix_ops}):
            raise ValueError("at most one box op and one class op among the mix ops of a pipeline, given %d ops" % len(self.mix_ops))
        self.out_size = _pair(out_size) if out_size is not None else None
        self.image_fill, self.label_fill = int(image_fill), int(label_fill)
        self.rng = np.random.RandomState(seed)
        self.colour_rng = np.random.RandomState(seed + COLOUR_SEED_OFFSET if seed is not None else None)

    def matrix(self, rng, w, h):
        M = _affine()
        for op in self.geometric_ops:
            m, (w, h) = op.matrix(rng, w, h)
            M = M.dot(m)
        if self.out_size is not None and (h, w) != self.out_size:
            m, (w, h) = CenterCrop(self.out_size).matrix(rng, w, h)
            M = M.dot(m)
        return M, (w, h)

    def matrices(self, rng, n, w, h):
        """int32 [n, 6]: one drawn map per sample of a batch of (w, h) images, as sscg_augment_u8 reads them."""
        return np.stack([to_q16(self.matrix(rng, w, h)[0]) for _ in range(n)]).astype(np.int32)

    def colour_state(self, rng, channels):
        """(A, B, b) in float64, [channels, channels] twice and [channels]: the drawn colour ops folded in the order written."""
        w, one = _luma(channels), np.ones(channels)
        A, B, b = np.eye(channels), np.zeros((channels, channels)), np.zeros(channels)
        for op in self.colour_ops:
            M, c = op.colour(rng, channels)
            if M is not None:
                A, B, b = M.dot(A), M.dot(B), M.dot(b)
            else:
                A, B, b = c * A, c * B + (1.0 - c) * np.outer(one, w.dot(A + B)), c * b + (1.0 - c) * one * w.dot(b)
        return A, B, b

    @property
    def need_mean(self):
        return any(isinstance(op, RandomContrast) for op in self.colour_ops)

    def colours(self, rng, n, channels):
        """(float32 [n, 21], need_mean): one drawn colour state per sample as sscg_augment_colour_u8 reads them; need_mean is true
        iff an op is a contrast."""
        return np.stack([colour_table_row(*self.colour_state(rng, channels)) for _ in range(n)]), self.need_mean

    def lattice(self, rng, q, ow, oh):
        """int32 [GH, GW, 2]: one drawn lattice over an (ow, oh) output view for the sample whose Q16 coefficients are `q` - the
        op's offsets (output pixels) times the map's 2x2 linear part (q0 q1; q3 q4, already Q16), in float64, rounded to nearest."""
        op = self.elastic_ops[0]
        u = op.field(rng, *lattice_shape(op.grid, oh, ow))
        q = [float(v) for v in q]
        nodes = np.rint(np.stack([q[0] * u[..., 0] + q[1] * u[..., 1], q[3] * u[..., 0] + q[4] * u[..., 1]], axis=-1))
        if nodes.size and np.abs(nodes).max() >= ELASTIC_NODE_LIMIT:
            raise ValueError("elastic node out of the Q16 range of the lattice (|node| < 2^26 = 1024 source pixels): %g" % np.abs(nodes).max())
        return nodes.astype(np.int32)

    def fields(self, rng, n, w, h, mats):
        """(int32 [n, GH, GW, 2], grid): one drawn lattice per sample of a batch of (w, h) images whose maps are `mats` (int [n, 6],
        what `matrices` drew for them), as sscg_augment_elastic_u8 reads them; None without an elastic op.  The lattice lies over the
        output view: `out_size`, or the input's size without one."""
        if not self.elastic_ops:
            return None
        oh, ow = self.out_size if self.out_size is not None else (h, w)
        assert len(mats) == n
        return np.stack([self.lattice(rng, mats[i], ow, oh) for i in range(n)]), self.elastic_ops[0].grid

    def mixes(self, rng, n, ow, oh):
        """(int32 [n, 8], classes): one drawn row (partner, x0, y0, x1, y1, mask_lo, mask_hi, 0) per sample of a batch of n whose
        output view is (ow, oh), as sscg_augment_mix_u8 reads them; classes is true iff an op is a class op.  Per sample, in batch
        order: one draw for the partner - uniform over the other n - 1 samples - then every op's own draws in the order written.
        Each op fires with its own probability, independently; the number of draws does not depend on what fires, so a seed's
        sequence does not depend on outcomes.  A sample with no firing op - and every sample of a batch of one - keeps its own index
        as the partner: not mixed.  A box op that did not fire leaves the empty box, a class op that did not the zero mask."""
        table = np.zeros((n, 8), dtype=np.int64)
        for i in range(n):
            j = min(int(rng.random_sample() * (n - 1)), max(n - 2, 0))
            partner, fired = j + (j >= i), False
            for op in self.mix_ops:
                fires, box, mask = op.mix(rng, ow, oh)
                if not fires or n == 1:
                    continue
                fired = True
                if box is not None:
                    table[i, 1:5] = box
                if mask is not None:
                    table[i, 5:7] = mask & 0xFFFFFFFF, mask >> 32
            table[i, 0] = partner if fired else i
        return _wrap_i32(table), any(op.classes for op in self.mix_ops)

    def _integer_call(self, img, mask, M, out):
        """The host path with an elastic op: the integer definition in numpy, affine and elastic part in one resampling."""
        bands = len(img.getbands())
        if img.mode not in ("L", "RGB") or (mask is not None and mask.mode not in ("L", "P")):
            raise ValueError("elastic augmentation takes 8-bit images of one or three channels and 8-bit masks, given modes %r, %r"
                             % (img.mode, mask.mode if mask is not None else None))
        q = to_q16(M)
        ow, oh = out
        d = elastic_displacement(self.lattice(self.elastic_rng, q, ow, oh), self.elastic_ops[0].grid, oh, ow)
        src = np.asarray(img).reshape(img.size[1], img.size[0], bands)
        px, lab = warp_u8(src, np.asarray(mask) if mask is not None else None, q, d, (oh, ow), self.image_fill, self.label_fill)
        warped = Image.fromarray(px if bands == 3 else px[:, :, 0])
        if mask is None:
            return warped, None
        warped_mask = Image.fromarray(lab)
        if mask.mode == "P":                                  # (an "L" image that is given a palette becomes a "P" one)
            warped_mask.putpalette(mask.getpalette())
        return warped, warped_mask

    def __call__(self, img, mask=None):
        if self.mix_ops:
            raise ValueError("mix ops (cutmix, classmix) combine the samples of a batch: they run in the device finish only "
                             "(DeviceLoader(..., augmentation=) -> functional.augment_batch(mix=)), not sample by sample on the host")
        w, h = img.size
        assert mask is None or mask.size == img.size
        M, out = self.matrix(self.rng, w, h)
        bands = len(img.getbands())
        if self.elastic_ops:
            img, mask = self._integer_call(img, mask, M, out)
        else:
            coef = tuple(float(v) for v in M[:2].reshape(-1))
            fill = self.image_fill if bands == 1 else (self.image_fill,) * bands
            img = img.transform(out, Image.AFFINE, coef, Image.BILINEAR, fillcolor=fill)
        if self.colour_ops:
            if bands not in (1, 3) or img.mode not in ("L", "RGB"):
                raise ValueError("colour augmentation takes 8-bit images of one or three channels, given mode %r" % img.mode)
            row = colour_table_row(*self.colour_state(self.colour_rng, bands))
            px = apply_colour(np.asarray(img).reshape(out[1], out[0], bands), row, self.need_mean)
            img = Image.fromarray(px if bands == 3 else px[:, :, 0])
        if mask is None:
            return img
        return img, (mask if self.elastic_ops else mask.transform(out, Image.AFFINE, coef, Image.NEAREST, fillcolor=self.label_fill))


COLOUR_ITEMS = {"brightness": RandomBrightness, "contrast": RandomContrast, "saturation": RandomSaturation, "hue": RandomHue,
                "gray": RandomGrayscale}


def from_spec(spec, size, image_fill=0, label_fill=0, out_size=None, seed=None):
    """The augmentation a `--augment` value names, or None for an empty one: a comma list of `hflip`, `rotate=<deg>`,
    `scale=<lo>:<hi>` and `sizedcrop` (RandomSizedCrop to `size` = (height, width)), and of the colour items `brightness=<x>`,
    `contrast=<x>`, `saturation=<x>` (factor in max(0, 1-x)..1+x), `hue=<x>` (0..0.5 of a turn) and `gray=<p>` (a probability) -
    geometry and colour each applied in the order written, colour behind geometry - and at most one `elastic=<alpha>[:<grid>]`
    (RandomElastic: node offsets up to alpha output pixels on a lattice of `grid` output pixels, default 32, an untuned default;
    grid >= 4 and 0 <= alpha <= 0.4 * grid), which deforms the final output view wherever it stands in the list.  Two items mix the
    samples of a batch (device finish only), at most one of each: `cutmix=<p>[:<lo>:<hi>]` (RandomCutMix: with probability p a box of
    lo..hi of the area, default 0.25:0.5, untuned) and `classmix=<p>[:<id>[:<id>...]]` (RandomClassMix: with probability p a random half
    of the classes; the ids, each in [0, 64), are never pasted - `classmix=0.5:0` keeps VOC's background, `classmix=0.5:19` Cityscapes'
    void where it is)."""
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
        elif key in COLOUR_ITEMS and val:
            x = float(val)
            top = {"hue": 0.5, "gray": 1.0}.get(key, float("inf"))
            if not 0.0 <= x <= top:                       # (false for a NaN)
                raise ValueError("--augment %s=<x> needs 0 <= x%s, given %r" % (key, " <= %g" % top if top < float("inf") else "", item))
            ops.append(COLOUR_ITEMS[key](x))
        elif key == "elastic" and val and val.count(":") <= 1:
            alpha, _, grid = val.partition(":")
            alpha, grid = float(alpha), int(grid) if grid else ELASTIC_DEFAULT_GRID
            if any(hasattr(op, "field") for op in ops):
                raise ValueError("--augment: one elastic item at the most, given a second: %r" % item)
            if not 0.0 <= alpha <= 0.4 * grid or grid < 4:        # (false for a NaN)
                raise ValueError("--augment elastic=<alpha>[:<grid>] needs grid >= 4 and 0 <= alpha <= 0.4 * grid (beyond it the "
                                 "deformation can fold), given %r" % item)
            ops.append(RandomElastic(alpha, grid))
        elif key == "cutmix" and val and val.count(":") in (0, 2):
            if any(isinstance(op, RandomCutMix) for op in ops):
                raise ValueError("--augment: one cutmix item at the most, given a second: %r" % item)
            ops.append(RandomCutMix(*(float(v) for v in val.split(":"))))
        elif key == "classmix" and val:
            if any(isinstance(op, RandomClassMix) for op in ops):
                raise ValueError("--augment: one classmix item at the most, given a second: %r" % item)
            p, *ids = val.split(":")
            ops.append(RandomClassMix(float(p), tuple(int(v) for v in ids)))
        else:
            raise ValueError("--augment: unknown item %r (hflip, rotate=<deg>, scale=<lo>:<hi>, sizedcrop, elastic=<alpha>[:<grid>], "
                             "brightness=<x>, contrast=<x>, saturation=<x>, hue=<x>, gray=<p>, cutmix=<p>[:<lo>:<hi>], "
                             "classmix=<p>[:<id>...])" % item)
    return Compose(ops, out_size=out_size, image_fill=image_fill, label_fill=label_fill, seed=seed) if ops else None
