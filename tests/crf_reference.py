"""The windowed dense CRF of include/sscg.h (sscg_crf_head) restated in numpy, sharing no code with the library: tests/test_crf_host.py
checks the restatement against properties of the definition, tests/test_crf_gpu.py checks the kernels against it.  Every step runs in
the dtype asked for - np.float64 is the reference, np.float32 the same operations at the kernels' precision (its distance from the
fp64 result scales the tolerance of the GPU test) - except the three constants 1 / (2 theta^2), which the contract forms in double and
rounds to fp32 once, in both."""
import numpy as np

LOGITS, PROBS = 0, 1
STRONG = dict(w_bilateral=4.0, w_spatial=3.0, theta_alpha=8.0, theta_beta=0.5, theta_gamma=3.0)
GENTLE = dict(w_bilateral=0.5, w_spatial=0.3, theta_alpha=4.0, theta_beta=0.5, theta_gamma=2.0)
FLT_MIN = np.float32(1.17549435e-38)


def resize(x, oh, ow, dt):
    """Bilinear resize with align_corners=True of a [N, H, W, C] array; src = scale * dst with the scale formed in `dt`."""
    N, H, W, Cn = x.shape
    if (H, W) == (oh, ow):
        return x.astype(dt)
    x = x.astype(dt)
    sh = dt(H - 1) / dt(oh - 1) if oh > 1 else dt(0)
    sw = dt(W - 1) / dt(ow - 1) if ow > 1 else dt(0)
    fy, fx = sh * np.arange(oh, dtype=dt), sw * np.arange(ow, dtype=dt)
    y0, x0 = np.minimum(fy.astype(np.int64), H - 1), np.minimum(fx.astype(np.int64), W - 1)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    ly, lx = (fy - y0.astype(dt))[None, :, None, None], (fx - x0.astype(dt))[None, None, :, None]
    one = dt(1)
    top = x[:, y0][:, :, x0] * (one - lx) + x[:, y0][:, :, x1] * lx
    bot = x[:, y1][:, :, x0] * (one - lx) + x[:, y1][:, :, x1] * lx
    return top * (one - ly) + bot * ly


def softmax(v):
    e = np.exp(v - v.max(axis=3, keepdims=True))
    return e / e.sum(axis=3, keepdims=True)


def unary(x, kind, size, dt):
    """u [N, OH, OW, C]: log-probabilities of the resized logits, or the log of the scores clamped at FLT_MIN."""
    if kind == PROBS:
        assert x.shape[1:3] == tuple(size)
        return np.log(np.maximum(x.astype(dt), dt(FLT_MIN)))
    z = resize(x, size[0], size[1], dt)
    z = z - z.max(axis=3, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=3, keepdims=True))


def taps(radius):
    """The window's offsets in row-major (dy, dx) order, centre excluded."""
    return [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if (dy, dx) != (0, 0)]


def message(q, img, radius, dilation, w_bilateral, w_spatial, theta_alpha, theta_beta, theta_gamma, dt):
    """msg_c(i) = sum over the taps inside the map of k(i, j) Q_c(j), accumulated tap by tap in `dt`."""
    N, OH, OW, Cn = q.shape
    ia, ib, ig = (dt(np.float32(1.0 / (2.0 * float(t) * float(t)))) for t in (theta_alpha, theta_beta, theta_gamma))
    wb, ws = dt(w_bilateral), dt(w_spatial)
    msg = np.zeros_like(q)
    for dy, dx in taps(radius):
        oy, ox = dy * dilation, dx * dilation
        ys, xs = slice(max(0, -oy), min(OH, OH - oy)), slice(max(0, -ox), min(OW, OW - ox))           # pixels i whose tap j is in the map
        yj, xj = slice(ys.start + oy, ys.stop + oy), slice(xs.start + ox, xs.stop + ox)
        if ys.start >= ys.stop or xs.start >= xs.stop:
            continue
        d2 = dt(oy * oy + ox * ox)
        diff = img[:, ys, xs] - img[:, yj, xj]
        c2 = (diff * diff).sum(axis=3)
        k = wb * np.exp(-(d2 * ia + c2 * ib)) + ws * np.exp(-d2 * ig)
        msg[:, ys, xs] += k[..., None] * q[:, yj, xj]
    return msg


def crf(x, kind, img, size, iterations, radius, dilation, dt=np.float64, **weights):
    """(u, [Q0, Q1, ..., Q_iterations]) of scores x [N, H, W, C] and guide img [N, OH, OW, IC], all in `dt`."""
    img = img.astype(dt)
    u = unary(x, kind, size, dt)
    qs = [softmax(u)]
    for _ in range(iterations):
        qs.append(softmax(u + message(qs[-1], img, radius, dilation, dt=dt, **weights)))
    assert all(q.dtype == dt for q in qs)
    return u, qs


def first_max(q):
    return q.argmax(axis=3)


def top_two_margin(q):
    s = np.sort(q, axis=3)
    return s[..., -1] - s[..., -2] if q.shape[3] > 1 else np.ones(q.shape[:3])


def make_inputs(seed, N, H, W, Cn, OH, OW, IC=3):
    """Logits N(0, 2^2) [N, H, W, C] and a guide image [N, OH, OW, IC]: a smooth sin / cos ramp plus N(0, 0.3^2) noise, fp32."""
    rs = np.random.RandomState(seed)
    x = (rs.standard_normal((N, H, W, Cn)) * 2.0).astype(np.float32)
    yy, xx = np.meshgrid(np.arange(OH, dtype=np.float64), np.arange(OW, dtype=np.float64), indexing="ij")
    ramp = np.stack([np.sin(0.21 * yy + 0.13 * xx + 0.9 * ch) + np.cos(0.17 * xx - 0.05 * yy + 0.4 * ch) for ch in range(IC)], axis=2)
    img = (ramp[None] + 0.25 * np.arange(N)[:, None, None, None] + rs.standard_normal((N, OH, OW, IC)) * 0.3).astype(np.float32)
    return x, img
