"""Numpy / scipy restatement of the surface-distance records (include/sscg.h: sscg_surface_stats) and of the scores formed from them
(utils.surface_scores) - the pin of tests/test_surface_gpu.py, checked on its own in tests/test_surface_host.py.  No torch, no GPU.
Everything is written as what it is: the masks, the erosion by the cross, every source surface pixel against every target surface
pixel in integers, a sort for the ranks."""
import numpy as np
from scipy import ndimage

CROSS = ndimage.generate_binary_structure(2, 1)
CNT, WITHIN, MAX2, V_LO, V_HI = range(5)


def surface(mask):
    """S(M): the pixels of M with a 4-neighbour outside M or outside the image."""
    mask = np.asarray(mask, dtype=bool)
    return mask & ~ndimage.binary_erosion(mask, CROSS, border_value=0)


def class_masks(label_true, label_pred, c):
    """(T_c, P_c) of one sample: a true label outside [0, C) and a predicted byte >= C equal no class id, so they are in no mask."""
    return np.asarray(label_true).astype(np.int64) == c, np.asarray(label_pred).astype(np.int64) == c


def directed_d2(src, tgt):
    """int64 [cnt]: for every pixel of the surface `src` (row-major order) the smallest squared distance to a pixel of `tgt`;
    None when either is empty."""
    sy, sx = np.nonzero(src)
    ty, tx = np.nonzero(tgt)
    if sy.size == 0 or ty.size == 0:
        return None
    out = np.empty(sy.size, dtype=np.int64)
    for i in range(0, sy.size, 2048):                 # in slabs: the full table of a checkerboard would be large
        dy = sy[i:i + 2048, None].astype(np.int64) - ty[None, :]
        dx = sx[i:i + 2048, None].astype(np.int64) - tx[None, :]
        out[i:i + 2048] = (dy * dy + dx * dx).min(axis=1)
    return out


def ranks(cnt, pct):
    lo = ((cnt - 1) * pct) // 100
    return lo, min(lo + 1, cnt - 1)


def percentile_by_ranks(d2, pct):
    """The integer-rank form of np.percentile(sqrt(d2), pct) (linear interpolation)."""
    v = np.sort(np.asarray(d2, dtype=np.int64))
    lo, hi = ranks(v.size, pct)
    a, b = np.sqrt(float(v[lo])), np.sqrt(float(v[hi]))
    return a + (b - a) * ((((v.size - 1) * pct) % 100) / 100.0)


def stats(label_true, label_pred, C, tol2, pct):
    """(stats int64 [2, N, C, 5], sums float64 [2, N, C]) of a batch; sums by math.fsum-like exactness is not needed: the roots are
    added in fp64 in row-major order, and the test's bound covers any order."""
    lt, lp = np.asarray(label_true), np.asarray(label_pred)
    N = lt.shape[0]
    st = np.zeros((2, N, C, 5), dtype=np.int64)
    sm = np.zeros((2, N, C), dtype=np.float64)
    for n in range(N):
        for c in range(C):
            t, p = class_masks(lt[n], lp[n], c)
            surf = (surface(t), surface(p))
            for d in (0, 1):
                src, tgt = surf[d], surf[1 - d]
                st[d, n, c, CNT] = int(src.sum())
                d2 = directed_d2(src, tgt)
                if d2 is None:
                    st[d, n, c, MAX2:] = -1
                    continue
                v = np.sort(d2)
                lo, hi = ranks(v.size, pct)
                st[d, n, c, WITHIN] = int((d2 <= tol2).sum())
                st[d, n, c, MAX2], st[d, n, c, V_LO], st[d, n, c, V_HI] = v[-1], v[lo], v[hi]
                sm[d, n, c] = float(np.sqrt(d2.astype(np.float64)).sum())
    return st, sm


def kept(C, dataset):
    return list(range(1, C)) if dataset == "voc2012" else (list(range(C - 1)) if dataset == "cityscapes" else list(range(C)))


def scores(st, sm, C, dataset, pct):
    """utils.surface_scores' arithmetic, case by case in Python floats."""
    M = st.shape[1]
    per = {k: [[] for _ in range(C)] for k in ("hd", "hd95", "assd", "nsd")}
    missing = [0] * C
    for n in range(M):
        for c in range(C):
            c0, c1 = int(st[0, n, c, CNT]), int(st[1, n, c, CNT])
            if (c0 > 0) != (c1 > 0):
                missing[c] += 1
            if not (c0 > 0 and c1 > 0):
                continue
            per["hd"][c].append(float(np.sqrt(float(max(st[0, n, c, MAX2], st[1, n, c, MAX2])))))
            h = []
            for d, cnt in ((0, c0), (1, c1)):
                a, b = float(np.sqrt(float(st[d, n, c, V_LO]))), float(np.sqrt(float(st[d, n, c, V_HI])))
                h.append(a + (b - a) * ((((cnt - 1) * pct) % 100) / 100.0))
            per["hd95"][c].append(max(h))
            per["assd"][c].append((float(sm[0, n, c]) + float(sm[1, n, c])) / float(c0 + c1))
            per["nsd"][c].append(float(int(st[0, n, c, WITHIN]) + int(st[1, n, c, WITHIN])) / float(c0 + c1))
    k = kept(C, dataset)
    out = {}
    for name, lists in per.items():
        cls = [float(np.sum(np.asarray(lists[c], dtype=np.float64)) / len(lists[c])) if lists[c] else float("nan") for c in k]
        fin = [v for v in cls if not np.isnan(v)]
        out[name] = float(np.mean(np.asarray(fin, dtype=np.float64))) if fin else float("nan")
        out["class_" + name] = dict(enumerate(cls))
    out["cases"] = dict(enumerate(len(per["hd"][c]) for c in k))
    out["missing"] = dict(enumerate(missing[c] for c in k))
    return out


def case_census(st):
    """(defined, missing, neither) cases of a stats array."""
    a, b = st[0, ..., CNT] > 0, st[1, ..., CNT] > 0
    return int((a & b).sum()), int((a ^ b).sum()), int((~a & ~b).sum())


# ------------------------------------------------------------------------------------------ inputs
def smooth_labels(rs, N, H, W, C, sigma):
    """[N,H,W] int64: the argmax over C planes of Gaussian-filtered noise - smooth regions with curved contours."""
    noise = rs.standard_normal((N, C, H, W))
    return np.argmax(ndimage.gaussian_filter(noise, sigma=(0, 0, sigma, sigma), mode="nearest"), axis=1).astype(np.int64)


def make_case(seed, N, H, W, C, sigma=3.0, void_ring=False, pred_over=False):
    """(label_true int64, label_pred uint8): two smooth maps from one noise field, the prediction's field perturbed - contours that
    lie near each other without coinciding.  void_ring: the outermost ring of the ground truth is 255.  pred_over: a patch of the
    prediction holds bytes >= C (C and 200)."""
    rs = np.random.RandomState(seed)
    sigma = min(sigma, max(0.6, min(H, W) / 4.0))
    base = rs.standard_normal((N, C, H, W))
    other = rs.standard_normal((N, C, H, W))
    f = lambda z: np.argmax(ndimage.gaussian_filter(z, sigma=(0, 0, sigma, sigma), mode="nearest"), axis=1).astype(np.int64)
    gt, pred = f(base), f(base + 0.6 * other)
    if void_ring:
        gt[:, 0, :] = gt[:, -1, :] = gt[:, :, 0] = gt[:, :, -1] = 255
    if pred_over:
        pred[:, : max(1, H // 4), : max(1, W // 3)] = C
        pred[:, -max(1, H // 5):, -max(1, W // 4):] = 200
    return gt, pred.astype(np.uint8)
