"""Numpy restatement of the contour counts (include/sscg.h: sscg_boundary_counts) - the pin of tests/test_boundary_gpu.py, checked on
its own in tests/test_boundary_host.py.  No torch, no GPU.  The window is written as what it is: every one of the (2d+1)^2 shifts
is compared with the centre wherever both pixels are inside the image; the counts are bincounts."""
import numpy as np


def canonical_true(label_true, C):
    """t: the label where it lies in [0, C), else VOID (coded C)."""
    lt = np.asarray(label_true).astype(np.int64)
    return np.where((lt >= 0) & (lt < C), lt, C)


def differs_in_window(a, d):
    """[N,H,W] bool: some q in the (2d+1) x (2d+1) window around p, clipped to the image, has a(q) != a(p)."""
    N, H, W = a.shape
    out = np.zeros(a.shape, dtype=bool)
    for dy in range(-min(d, H - 1), min(d, H - 1) + 1):
        for dx in range(-min(d, W - 1), min(d, W - 1) + 1):
            if dy == 0 and dx == 0:
                continue
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)          # the centres whose shifted twin exists
            out[:, y0:y1, x0:x1] |= a[:, y0:y1, x0:x1] != a[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def window_leaves_image(H, W, d):
    """[H,W] bool: the unclipped window leaves the image."""
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    return (y < d) | (y >= H - d) | (x < d) | (x >= W - d)


def masks(label_true, label_pred, C, d):
    """(t, r, E_t, E_r, band) of the definition."""
    t = canonical_true(label_true, C)
    r = np.asarray(label_pred).astype(np.int64)
    assert t.ndim == 3 and t.shape == r.shape and r.min() >= 0 and r.max() <= 255
    in_t, in_r = differs_in_window(t, d), differs_in_window(r, d)
    out = window_leaves_image(t.shape[1], t.shape[2], d)[None]
    valid = t != C
    return t, r, valid & (in_t | out), valid & (in_r | out), valid & in_t


def counts(label_true, label_pred, C, d):
    """int64 [3 C + C C] = bt | bp | bi | tri of one batch."""
    t, r, e_t, e_r, band = masks(label_true, label_pred, C, d)
    in_c = r < C                                             # a predicted value >= C is counted in no bin
    bt = np.bincount(t[e_t], minlength=C)[:C]
    bp = np.bincount(r[e_r & in_c], minlength=C)[:C]
    bi = np.bincount(t[e_t & e_r & (t == r)], minlength=C)[:C]
    sel = band & in_c
    tri = np.bincount(C * t[sel] + r[sel], minlength=C * C)[:C * C]
    return np.concatenate([bt, bp, bi, tri]).astype(np.int64)


def split(v, C):
    """(bt, bp, bi, tri [C,C]) views of a counts vector."""
    v = np.asarray(v)
    return v[:C], v[C:2 * C], v[2 * C:3 * C], v[3 * C:].reshape(C, C)


def width(h, w, ratio):
    return max(1, int(ratio * np.sqrt(float(h) * h + float(w) * w) + 0.5))


def edge_share(label_true, C, d):
    """The share of the valid pixels that lie in E_t: a case that is to exercise both the edge and the non-edge path keeps it inside
    (0.1, 0.9)."""
    t, _, e_t, _, _ = masks(label_true, np.zeros(np.shape(label_true), dtype=np.uint8), C, d)
    return float(e_t.sum()) / max(1, int((t != C).sum()))


# ------------------------------------------------------------------------------------------ inputs: region maps, not noise
def blobs(rs, N, H, W, n_labels, seeds):
    """[N,H,W] int64 nearest-seed regions: `seeds` random points per sample, each with a random label in [0, n_labels)."""
    y, x = np.arange(H)[:, None, None], np.arange(W)[None, :, None]
    out = np.empty((N, H, W), dtype=np.int64)
    for n in range(N):
        sy, sx = rs.randint(0, H, seeds), rs.randint(0, W, seeds)
        lab = rs.randint(0, n_labels, seeds)
        out[n] = lab[np.argmin((y - sy) ** 2 + (x - sx) ** 2, axis=2)]
    return out


def make_case(seed, N, H, W, C, seeds=4, share=0.3, void=True, pred_over=False):
    """(label_true int64, label_pred uint8): the ground truth is a blob map; the prediction is the ground truth with the pixels of a
    few blobs of a second map (about `share` of them) replaced from a third.  void: two blobs and a border strip of the ground truth
    take the values 255, -1 and C.  pred_over: two blobs of the prediction take values >= C (C and 200).
    seeds == 0 is the layout for widths near the map's size, where blobs would leave no window uniform: one class with a ragged
    band of a second class along the right side, void patches in two corners; the prediction is that map moved by (3, 5) pixels."""
    rs = np.random.RandomState(seed)
    if seeds == 0:
        a = rs.randint(0, C)
        b = (a + 1 + rs.randint(0, max(C - 1, 1))) % C          # another class wherever there is one
        y, x = np.arange(H)[:, None], np.arange(W)[None, :]
        one = np.where(x >= W - 14 + (y % 7), b, a)
        gt = np.broadcast_to(one, (N, H, W)).copy()
        pred = np.roll(gt, (3, 5), axis=(1, 2))
        if pred_over:
            pred[:, H // 2:H // 2 + 9, :12] = C
            pred[:, -6:, W // 2:W // 2 + 9] = 200
        if void:
            gt[:, :10, :15] = 255
            gt[:, -8:, :12] = -1
            gt[:, :, :1] = C
        return gt.astype(np.int64), pred.astype(np.uint8)
    gt = blobs(rs, N, H, W, C, seeds)
    other = blobs(rs, N, H, W, C, seeds)
    pick = blobs(rs, N, H, W, 10, seeds + 2) < int(round(10 * share))
    pred = np.where(pick, other, gt)
    if pred_over:
        over = blobs(rs, N, H, W, 8, seeds + 2)
        pred = np.where(over == 0, C, np.where(over == 1, 200, pred))
    if void:
        holes = blobs(rs, N, H, W, 12, seeds + 3)
        gt = np.where(holes == 0, 255, np.where(holes == 1, -1, gt))
        if W > 1:
            gt[:, :, :1] = C                                 # a border strip: the first column, and the last row of a wide or one-pixel-wide map
        if H > 1 and (W > H or W == 1):
            gt[:, -1:, :] = 255
    return gt.astype(np.int64), pred.astype(np.uint8)
