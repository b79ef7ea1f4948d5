"""Sliding-window inference restated in numpy float64, sharing no code with the product: window positions, weight and normalisation
tables, align-corners bilinear resize, softmax, weighted sum over the windows, normalisation, first maximum.  tests/test_sliding_host.py
checks the product's host geometry against it, tests/test_sliding_gpu.py the kernel's meaning."""
import math

import numpy as np


def positions(L, w, overlap):
    """Stride s = max(1, int(w (1 - overlap) + 0.5)); k = 1 if L == w else ceil((L - w) / s) + 1; pos_i = min(i s, L - w)."""
    s = max(1, int(w * (1 - overlap) + 0.5))
    k = 1 if L == w else int(math.ceil((L - w) / float(s))) + 1
    return [min(i * s, L - w) for i in range(k)], s


def weights(w, blend, sigma):
    """float64 weights of one axis of the window."""
    if blend == "const":
        return np.ones(w, dtype=np.float64)
    i = np.arange(w, dtype=np.float64)
    return np.exp(-(i - (w - 1) / 2.0) ** 2 / (2.0 * (sigma * w) ** 2))


def coverage(L, w, pos, wt):
    """Sum over the windows covering o of wt[o - pos_i], float64 [L]; and the number of windows covering o."""
    cov, cnt = np.zeros(L, dtype=np.float64), np.zeros(L, dtype=np.int64)
    for p in pos:
        cov[p:p + w] += wt
        cnt[p:p + w] += 1
    return cov, cnt


def resize64(x, oh, ow):
    """Bilinear resize with align_corners=True of a [H, W, C] float64 array."""
    H, W, _ = x.shape
    fy = np.arange(oh, dtype=np.float64) * ((H - 1) / (oh - 1) if oh > 1 else 0.0)
    fx = np.arange(ow, dtype=np.float64) * ((W - 1) / (ow - 1) if ow > 1 else 0.0)
    y0, x0 = np.minimum(np.floor(fy).astype(int), H - 1), np.minimum(np.floor(fx).astype(int), W - 1)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    ly, lx = (fy - y0)[:, None, None], (fx - x0)[None, :, None]
    top = x[y0][:, x0] * (1 - lx) + x[y0][:, x1] * lx
    bot = x[y1][:, x0] * (1 - lx) + x[y1][:, x1] * lx
    return top * (1 - ly) + bot * ly


def softmax64(x):
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def blend64(logits, N, OH, OW, wh, ww, overlap, blend, sigma, flip):
    """`logits`: [N * ky * kx * F, h, w, C] (any float dtype), window ((n ky + iy) kx + ix) F + f, the f = 1 map computed from the
    window mirrored along W.  Returns (prob float64 [N, OH, OW, C] - the normalised blend - and labels int64 [N, OH, OW], the first
    maximum of the blend)."""
    logits = np.asarray(logits, dtype=np.float64)
    pos_y, _ = positions(OH, wh, overlap)
    pos_x, _ = positions(OW, ww, overlap)
    wy, wx = weights(wh, blend, sigma), weights(ww, blend, sigma)
    F = 2 if flip else 1
    Cn = logits.shape[-1]
    assert logits.shape[0] == N * len(pos_y) * len(pos_x) * F
    acc = np.zeros((N, OH, OW, Cn), dtype=np.float64)
    norm = np.zeros((OH, OW), dtype=np.float64)
    g = wy[:, None] * wx[None, :]
    k = 0
    for n in range(N):
        for py in pos_y:
            for px in pos_x:
                for f in range(F):
                    p = softmax64(resize64(logits[k], wh, ww))
                    if f:
                        p = p[:, ::-1]
                    acc[n, py:py + wh, px:px + ww] += g[:, :, None] * p
                    if n == 0:
                        norm[py:py + wh, px:px + ww] += g
                    k += 1
    prob = acc / norm[None, :, :, None]
    return prob, prob.argmax(axis=-1)
