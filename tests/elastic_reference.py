"""include/sscg.h, sscg_augment_elastic_u8, restated in numpy int64 - what tests/test_augment_elastic_host.py and
tests/test_augment_elastic_gpu.py compare the host path and the kernels against, bit for bit.  Written pixel by pixel (every output
pixel gathers its own 4 x 4 nodes), not row by row like the product's host path (data_utils.augmentations.elastic_displacement).
warp_reference (tests/test_augment_host.py) and colour_reference (tests/test_augment_colour_host.py) take the six coefficients, not
the source coordinates, so what lies behind (sx, sy) is restated here; test_augment_elastic_host.py checks that with a zero lattice
this restatement equals both of them."""
import numpy as np

D = 6 * 2 ** 24


def numerators(t):
    """The four B-spline numerators over D at t (int64 array, 0..255)."""
    t = t.astype(np.int64)
    return [(256 - t) ** 3,
            3 * t ** 3 - 6 * 256 * t ** 2 + 4 * 256 ** 3,
            -3 * t ** 3 + 3 * 256 * t ** 2 + 3 * 256 ** 2 * t + 256 ** 3,
            t ** 3]


def lattice_shape(grid, OH, OW):
    return (OH - 1) // grid + 4, (OW - 1) // grid + 4


def displacement(nodes, grid, OH, OW):
    """nodes int [GH, GW, 2] of one sample -> (d_x, d_y), int64 [OH, OW] each."""
    nodes = np.asarray(nodes).astype(np.int64)
    assert nodes.shape == lattice_shape(grid, OH, OW) + (2,) and grid >= 4 and int(np.abs(nodes).max()) < 2 ** 26
    oy, ox = np.meshgrid(np.arange(OH, dtype=np.int64), np.arange(OW, dtype=np.int64), indexing="ij")
    cx, cy = ox // grid, oy // grid
    tx, ty = ((ox - cx * grid) * 256) // grid, ((oy - cy * grid) * 256) // grid
    nx, ny = numerators(tx), numerators(ty)
    out = []
    for k in (0, 1):
        acc = np.zeros((OH, OW), dtype=np.int64)
        for j in range(4):
            s = np.zeros((OH, OW), dtype=np.int64)
            for i in range(4):
                s += ny[i] * nodes[cy + i, cx + j, k]
            assert int(np.abs(s).max()) < 2 ** 53
            acc += nx[j] * np.floor_divide(s + D // 2, D)
        assert int(np.abs(acc).max()) < 2 ** 53
        out.append(np.floor_divide(acc + D // 2, D))
    return out[0], out[1]


def coordinates(mats, nodes, grid, out_size):
    """(sx, sy), int64 [N, OH, OW] each; nodes None = the affine map alone."""
    OH, OW = out_size
    oy, ox = np.meshgrid(np.arange(OH, dtype=np.int64), np.arange(OW, dtype=np.int64), indexing="ij")
    sx, sy = [], []
    for n in range(len(mats)):
        m = [int(v) for v in mats[n]]
        x, y = m[0] * ox + m[1] * oy + m[2], m[3] * ox + m[4] * oy + m[5]
        if nodes is not None:
            dx, dy = displacement(nodes[n], grid, OH, OW)
            x, y = x + dx, y + dy
        sx.append(x)
        sy.append(y)
    return np.stack(sx), np.stack(sy)


def integers(img, gt, sx, sy, image_fill=0, label_fill=0):
    """Behind (sx, sy), up to the last integer: v int64 [N, OH, OW, C] (< 2^24) and the raw label ids int64 [N, OH, OW] (or None)."""
    N, H, W, _ = img.shape
    x0, y0 = sx >> 16, sy >> 16
    fx, fy = ((sx & 0xFFFF) >> 8)[..., None], ((sy & 0xFFFF) >> 8)[..., None]
    nn = np.arange(N)[:, None, None]

    def tap(y, x):
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        return np.where(inside[..., None], img[nn, np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)].astype(np.int64), image_fill)
    top = tap(y0, x0) * (256 - fx) + tap(y0, x0 + 1) * fx
    bot = tap(y0 + 1, x0) * (256 - fx) + tap(y0 + 1, x0 + 1) * fx
    v = top * (256 - fy) + bot * fy
    assert int(v.max()) < 2 ** 24 and int(v.min()) >= 0
    ids = None
    if gt is not None:
        ix, iy = (sx + 0x8000) >> 16, (sy + 0x8000) >> 16
        inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        ids = np.where(inside, gt[nn, np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)], label_fill).astype(np.int64)
    return v, ids


def elastic_reference(img, gt, mats, nodes, grid, out_size, mean, std, lut, image_fill=0, label_fill=0, colours=None, need_mean=False):
    """img uint8 [N,H,W,C], gt uint8 [N,H,W] or None, mats int [N,6], nodes int [N,GH,GW,2] (None = no lattice), colours float32
    [N,21] or None -> (float32 [N,OH,OW,C], int64 [N,OH,OW] or None).  Every float32 / float64 operation is one numpy operation, so
    one IEEE rounding, in the order of include/sscg.h."""
    f = np.float32
    N, _, _, C = img.shape
    OH, OW = out_size
    sx, sy = coordinates(mats, nodes, grid, out_size)
    v, ids = integers(img, gt, sx, sy, image_fill, label_fill)
    t = (v.astype(f) * f(2.0 ** -16)) / f(255)
    mean, std = np.asarray(mean, dtype=f), np.asarray(std, dtype=f)
    if colours is None:
        out = (t - mean) / std
    else:
        assert C in (1, 3) and colours.dtype == f and colours.shape == (N, 21)
        out = np.empty((N, OH, OW, C), dtype=f)
        for n in range(N):
            A, B, b = colours[n, :9].reshape(3, 3), colours[n, 9:18].reshape(3, 3), colours[n, 18:]
            mu = np.zeros(C, dtype=f)
            if need_mean:
                S = v[n].reshape(-1, C).sum(axis=0, dtype=np.int64)
                mu = (S.astype(np.float64) / (np.float64(OH * OW) * np.float64(16711680.0))).astype(f)
            for c in range(C):
                if C == 3:
                    o = ((B[c, 0] * mu[0] + B[c, 1] * mu[1]) + B[c, 2] * mu[2]) + b[c]
                    u = ((A[c, 0] * t[n, ..., 0] + A[c, 1] * t[n, ..., 1]) + A[c, 2] * t[n, ..., 2]) + o
                else:
                    o = B[0, 0] * mu[0] + b[0]
                    u = A[0, 0] * t[n, ..., 0] + o
                assert u.dtype == f and np.asarray(o).dtype == f
                out[n, ..., c] = (np.minimum(np.maximum(u, f(0)), f(1)) - mean[c]) / std[c]
    assert out.dtype == f
    return out, (np.asarray(lut, dtype=np.int64)[ids] if gt is not None else None)
