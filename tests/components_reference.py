"""Numpy / scipy restatement of the connected-component filter (include/sscg.h: sscg_components_filter) - the pin of
tests/test_components_gpu.py, checked on its own in tests/test_components_host.py against literals and an independent flood fill.  No
torch, no GPU.  Everything is written as what it is: per sample and class scipy.ndimage.label with the cross (conn 4) or the full 3 x 3
structure (conn 8), areas by bincount, the keep rule in words, a bincount for the confusion matrix.

scipy numbers the components in raster order of their first pixel, which is the order of their anchors: "ties go to the smallest anchor"
is "the lowest label id among the largest", i.e. np.argmax of the areas."""
import numpy as np
from scipy import ndimage

STRUCTURE = {4: ndimage.generate_binary_structure(2, 1), 8: ndimage.generate_binary_structure(2, 2)}
COMPONENTS, KEPT, BEFORE, AFTER = range(4)


def exempt_mask(C, fill, skip=()):
    mask = 1 << fill
    for s in skip:
        assert 0 <= s < C
        mask |= 1 << s
    return mask


def components(sample, c, conn):
    """(ids int32 [H,W] with 0 = not of class c and 1.. = the components in anchor order, areas int64 [count]) of one sample."""
    ids, count = ndimage.label(np.asarray(sample) == c, structure=STRUCTURE[conn])
    return ids, np.bincount(ids.ravel(), minlength=count + 1)[1:].astype(np.int64)


def kept_components(areas, largest, min_area):
    """bool [count]: the keep rule of a non-exempt class."""
    keep = areas >= min_area
    if largest and areas.size:
        only = np.zeros(areas.size, dtype=bool)
        only[int(np.argmax(areas))] = True                  # the first of the largest: the smallest anchor
        keep &= only
    return keep


def confusion(label_true, label_out, C):
    """sscg_confusion_hist's rules: a true label outside [0, C) and a predicted byte >= C are counted nowhere."""
    t, p = np.asarray(label_true).astype(np.int64).ravel(), np.asarray(label_out).astype(np.int64).ravel()
    ok = (t >= 0) & (t < C) & (p < C)
    return np.bincount(C * t[ok] + p[ok], minlength=C * C).reshape(C, C).astype(np.int64)


def filter_maps(label_pred, C, conn=8, largest=False, min_area=0, fill=0, skip=(), label_true=None):
    """(label_out uint8 [N,H,W], hist int64 [C,C] or None, stats int64 [N,C,4]) of a batch."""
    lp = np.asarray(label_pred)
    assert lp.dtype == np.uint8 and lp.ndim == 3 and 1 <= C <= 64 and 0 <= fill < C
    mask = exempt_mask(C, fill, skip)
    out = lp.copy()
    N = lp.shape[0]
    st = np.zeros((N, C, 4), dtype=np.int64)
    for n in range(N):
        for c in range(C):
            ids, areas = components(lp[n], c, conn)
            keep = np.ones(areas.size, dtype=bool) if (mask >> c) & 1 else kept_components(areas, largest, min_area)
            st[n, c, COMPONENTS], st[n, c, KEPT], st[n, c, BEFORE] = areas.size, int(keep.sum()), int(areas.sum())
            gone = np.concatenate([[False], ~keep])[ids]    # id 0 (not of the class) is nobody's to remove
            out[n][gone] = fill
        for c in range(C):
            st[n, c, AFTER] = int((out[n] == c).sum())
    hist = None if label_true is None else confusion(label_true, out, C)
    return out, hist, st


def census(label_pred, C, tile, conn=8, largest=False, min_area=0, fill=0, skip=()):
    """What the filter has to do on a batch, for the conditions the tests put on their random inputs: the numbers of removed and of
    kept components of the non-exempt classes, and how many of each have pixels in more than one tile x tile tile."""
    lp = np.asarray(label_pred)
    mask = exempt_mask(C, fill, skip)
    H, W = lp.shape[1:]
    tiles = (np.arange(H)[:, None] // tile) * ((W + tile - 1) // tile) + np.arange(W)[None, :] // tile
    out = {"removed": 0, "kept": 0, "removed_across": 0, "kept_across": 0}
    for n in range(lp.shape[0]):
        for c in range(C):
            if (mask >> c) & 1:
                continue
            ids, areas = components(lp[n], c, conn)
            keep = kept_components(areas, largest, min_area)
            for k in range(areas.size):
                across = np.unique(tiles[ids == k + 1]).size > 1
                name = "kept" if keep[k] else "removed"
                out[name] += 1
                out[name + "_across"] += int(across)
    return out


# ------------------------------------------------------------------------------------------ inputs
def _speckled(rs, N, H, W, C, sigma, share=0.03):
    """A smooth label map - the argmax over C planes of Gaussian-filtered noise, as surface_reference.make_case makes it - with `share`
    of its pixels replaced by a random class: small islands exist."""
    noise = rs.standard_normal((N, C, H, W))
    lab = np.argmax(ndimage.gaussian_filter(noise, sigma=(0, 0, sigma, sigma), mode="nearest"), axis=1).astype(np.int64)
    hit = rs.random_sample((N, H, W)) < share
    lab[hit] = rs.randint(0, C, size=int(hit.sum()))
    return lab


def make_case(seed, N, H, W, C, void_ring=False):
    """(label_true int64, label_pred uint8): a speckled smooth prediction, and a ground truth made the same way from another draw.
    void_ring: the outermost ring of the ground truth is 255."""
    rs = np.random.RandomState(seed)
    sigma = min(3.0, max(0.6, min(H, W) / 4.0))
    pred = _speckled(rs, N, H, W, C, sigma)
    gt = _speckled(rs, N, H, W, C, sigma)
    if void_ring:
        gt[:, 0, :] = gt[:, -1, :] = gt[:, :, 0] = gt[:, :, -1] = 255
    return gt, pred.astype(np.uint8)


# name: (N, H, W, C, seed, void ring) - the random cases of tests/test_components_gpu.py: one pixel, one row, one column, smaller than a
# wave, one past a 32 tile in both axes (and across 16), exactly 2 x 2 tiles of 32 (one of 64), C = 1 / 2 / 4 / 21 / 64, N = 1..3, and
# 65 x 130: past 64 in both axes.  The seeds of the cases of at least 1000 pixels are chosen so that the restatement alone meets the
# conditions of tests/test_components_host.py::test_random_cases_do_real_work.
RANDOM = {
    "1x1_c4": (2, 1, 1, 4, 0, False),
    "1x7_c2": (3, 1, 7, 2, 1, False),
    "7x1_c2": (1, 7, 1, 2, 2, False),
    "5x9_c4": (2, 5, 9, 4, 3, False),
    "33x47_c4": (3, 33, 47, 4, 1, False),
    "33x47_c1": (2, 33, 47, 1, 5, False),
    "64x64_c4": (2, 64, 64, 4, 5, False),
    "40x72_c21_void": (2, 40, 72, 21, 0, True),
    "33x47_c64": (1, 33, 47, 64, 0, False),
    "65x130_c4": (1, 65, 130, 4, 0, False),
}


def random_settings(C):
    """The settings every random case runs under: largest, min_area = 8, both; conn 4 and 8; fill 0 and the last class; a skip."""
    last = C - 1
    out = [dict(largest=True), dict(min_area=8), dict(largest=True, min_area=8, conn=4), dict(largest=True, conn=4, fill=last),
           dict(min_area=8, conn=4, fill=last), dict(largest=True, min_area=3, fill=last)]
    if C > 1:
        out += [dict(largest=True, min_area=8, skip=(1,)), dict(min_area=8, conn=4, fill=last, skip=(0, min(2, last)))]
    return out


# ------------------------------------------------------------------------------------------ built cases: name -> (label_pred, C, settings)
def _serpentine():
    """70 x 70, three classes: class 1 fills the even rows and one end pixel of every odd row, alternately right and left - ONE
    one-pixel-wide component through every tile that crosses every vertical seam in every even row; the rest of an odd row is a strip
    of class 0, a component of its own, all 35 of equal area.  Sample 1 is the transpose: the same along the other axis."""
    a = np.zeros((70, 70), dtype=np.uint8)
    a[0::2, :] = 1
    a[1::4, 69] = 1
    a[3::4, 0] = 1
    return np.stack([a, a.T.copy()]), 3, [dict(largest=True, fill=2), dict(largest=True, conn=4, fill=2), dict(min_area=70, fill=2),
                                          dict(min_area=35 * 70 + 35, fill=2), dict(min_area=35 * 70 + 36, conn=4, fill=2)]


def _u_shape():
    """64 x 64: a U of class 1 whose arms (columns 5 and 9, rows 10..40) lie in the tile above the seam at 32 (and 16) and meet only in
    row 40; a C of class 2 whose arms (rows 50 and 54, columns 10..40) meet only in column 40.  A lone pixel of each class elsewhere."""
    a = np.zeros((1, 64, 64), dtype=np.uint8)
    a[0, 10:41, 5] = a[0, 10:41, 9] = a[0, 40, 5:10] = 1
    a[0, 50, 10:41] = a[0, 54, 10:41] = a[0, 50:55, 40] = 2
    a[0, 2, 60] = 1
    a[0, 60, 2] = 2
    return a, 3, [dict(largest=True), dict(largest=True, conn=4), dict(min_area=65), dict(min_area=66, conn=4)]


def _corners():
    """70 x 70: at each of 15|16, 31|32 and 63|64 class 1 on the diagonal pair (k, k), (k+1, k+1) and class 2 on the anti-diagonal pair
    (k, k+1), (k+1, k): whatever the tile edge (16, 32 or 64) one quadruple sits on a four-tile corner.  Separate under conn 4, joined
    under conn 8."""
    a = np.zeros((1, 70, 70), dtype=np.uint8)
    for k in (15, 31, 63):
        a[0, k, k] = a[0, k + 1, k + 1] = 1
        a[0, k, k + 1] = a[0, k + 1, k] = 2
    return a, 3, [dict(min_area=2), dict(min_area=2, conn=4), dict(largest=True), dict(largest=True, conn=4)]


def _checker():
    """17 x 23 checkerboard of classes 0 and 1, fill = 2: under conn 4 every pixel is its own component, all tie, the first pixel of
    each class survives `largest`; under conn 8 there is one component per class."""
    y, x = np.arange(17)[:, None], np.arange(23)[None, :]
    a = ((y + x) % 2).astype(np.uint8)[None]
    return a, 3, [dict(largest=True, conn=4, fill=2), dict(largest=True, conn=8, fill=2), dict(min_area=2, conn=4, fill=2),
                  dict(min_area=2, conn=8, fill=2)]


def _one_class():
    """65 x 130 of class 1 only: the largest area and the most contended root."""
    a = np.ones((1, 65, 130), dtype=np.uint8)
    return a, 2, [dict(largest=True), dict(min_area=65 * 130, conn=4), dict(min_area=65 * 130 + 1)]


def _sample_border():
    """N = 2, 5 x 40: class 1 fills the last row of sample 0 and the first row of sample 1 - neighbours in memory, two components."""
    a = np.zeros((2, 5, 40), dtype=np.uint8)
    a[0, 4, :] = 1
    a[1, 0, :] = 1
    return a, 2, [dict(largest=True), dict(min_area=40), dict(min_area=41), dict(largest=True, min_area=41, conn=4)]


def _equal_blobs():
    """Two 3 x 3 blobs of class 1 and a smaller one: under `largest` the first of the two equal ones is kept."""
    a = np.zeros((1, 12, 40), dtype=np.uint8)
    a[0, 6:9, 30:33] = 1            # first in raster order: its anchor (6, 30) precedes (7, 2)
    a[0, 7:10, 2:5] = 1
    a[0, 1:3, 10:12] = 1
    return a, 2, [dict(largest=True), dict(largest=True, conn=4), dict(min_area=9), dict(largest=True, min_area=10)]


def _holes():
    """A 10 x 21 blob of class 1 with a column of bytes 255 through it (it splits the blob into a 10 x 10 and a 10 x 10 half), bytes
    255 and 2 (= C) scattered inside the halves: they join nothing and pass through."""
    a = np.zeros((1, 40, 40), dtype=np.uint8)
    a[0, 5:15, 4:25] = 1
    a[0, 5:15, 14] = 255
    a[0, 7, 6] = a[0, 9, 20] = 255
    a[0, 11, 8] = a[0, 6, 22] = 2
    a[0, 30, 30] = 255
    return a, 2, [dict(largest=True), dict(largest=True, conn=4), dict(min_area=98), dict(min_area=99), dict(min_area=1000)]


BUILT = {"serpentine": _serpentine, "u_shape": _u_shape, "corners": _corners, "checker": _checker, "one_class": _one_class,
         "sample_border": _sample_border, "equal_blobs": _equal_blobs, "holes": _holes}


def built_truth(pred, C, seed=99):
    """A ground truth for a built case: random classes with a tenth of the pixels void (255) or negative."""
    rs = np.random.RandomState(seed)
    gt = rs.randint(0, C, size=pred.shape).astype(np.int64)
    r = rs.random_sample(pred.shape)
    gt[r < 0.05] = 255
    gt[r > 0.95] = -1
    return gt
