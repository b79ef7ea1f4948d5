"""The gated CRF loss of include/sscg.h (sscg_crf_loss_fwd) restated in numpy, sharing no code with the library:
tests/test_crf_loss_host.py checks the restatement against properties of the definition, tests/test_crf_loss_gpu.py checks the kernel
against it.  Every step runs in the dtype asked for - np.float64 is the reference, np.float32 the same operations at the kernel's
precision (its distance from the fp64 result scales the tolerance of the GPU test) - except the three constants 1 / (2 theta^2), which
the contract forms in double and rounds to fp32 once, in both (crf_reference.message does).

Two routes to the gradient: `coef`, the contract's -2/M * msg (which assumes k(i, j) == k(j, i)), and `scatter_grad`, which forms
the pairwise weights tap by tap on its own and scatters k(i, j) p(i) to pixel j - no symmetry assumed."""
import numpy as np

from crf_reference import make_inputs, message, resize, softmax, taps


def probs_of(x, size):
    """The softmax of the logits resized to `size` on the host (fp64), rounded to fp32: the map the tests hand to the loss, C-contiguous
    (the resize's fancy indexing leaves another memory order, which a copy to the device would keep)."""
    return np.ascontiguousarray(softmax(resize(x, size[0], size[1], np.float64)).astype(np.float32))


def case_inputs(seed, N, H, W, Cn, OH, OW, IC):
    """(p fp32 [N, OH, OW, C], img fp32 [N, OH, OW, IC]) from crf_reference.make_inputs."""
    x, img = make_inputs(seed, N, H, W, Cn, OH, OW, IC)
    return probs_of(x, (OH, OW)), img


def crf_loss(p, img, radius, dilation, dt=np.float64, **weights):
    """dict(loss, sums = (sum e, sum ksum) in fp64, coef, msg, ksum, e) of the map p [N, OH, OW, C] under the guide img, in `dt`."""
    p, img = p.astype(dt), img.astype(dt)
    M = p.shape[0] * p.shape[1] * p.shape[2]
    msg = message(p, img, radius, dilation, dt=dt, **weights)
    ksum = message(np.ones(p.shape[:3] + (1,), dtype=dt), img, radius, dilation, dt=dt, **weights)[..., 0]
    dot = np.zeros(p.shape[:3], dtype=dt)
    for c in range(p.shape[3]):
        dot = dot + p[..., c] * msg[..., c]
    e = ksum - dot
    sums = (float(e.astype(np.float64).sum()), float(ksum.astype(np.float64).sum()))
    coef = dt(np.float32(-2.0 / M)) * msg
    assert all(a.dtype == dt for a in (msg, ksum, e, coef))
    return dict(loss=dt(sums[0] / M), sums=sums, coef=coef, msg=msg, ksum=ksum, e=e, M=M)


def scatter_grad(p, img, radius, dilation, w_bilateral, w_spatial, theta_alpha, theta_beta, theta_gamma, dt=np.float64):
    """d loss / d p without assuming symmetry: -(1/M) * (msg + S), S_c(j) = sum over the pixels i that have j as a tap of k(i, j) p_c(i).
    The weights are formed here, pair by pair, from the definition."""
    p, img = p.astype(dt), img.astype(dt)
    N, OH, OW, _ = p.shape
    ia, ib, ig = (dt(np.float32(1.0 / (2.0 * float(t) * float(t)))) for t in (theta_alpha, theta_beta, theta_gamma))
    gather, scatter = np.zeros_like(p), np.zeros_like(p)
    for dy, dx in taps(radius):
        oy, ox = dy * dilation, dx * dilation
        y0, y1, x0, x1 = max(0, -oy), min(OH, OH - oy), max(0, -ox), min(OW, OW - ox)
        if y0 >= y1 or x0 >= x1:
            continue
        pi, pj = p[:, y0:y1, x0:x1], p[:, y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        diff = img[:, y0:y1, x0:x1] - img[:, y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        d2 = dt(oy * oy + ox * ox)
        k = dt(w_bilateral) * np.exp(-(d2 * ia + (diff * diff).sum(axis=3) * ib)) + dt(w_spatial) * np.exp(-d2 * ig)
        gather[:, y0:y1, x0:x1] += k[..., None] * pj
        scatter[:, y0 + oy:y1 + oy, x0 + ox:x1 + ox] += k[..., None] * pi
    return -(gather + scatter) / dt(N * OH * OW)
