"""The structural-similarity term restated in torch on the CPU (include/sscg.h: sscg_l1_ssim_fwd / _bwd): the loss from the map, the
gradient from autograd, in fp64 - and the same code in fp32 (its "twin"), whose distance from the fp64 result is the yardstick of the
kernel tests.  The window's weights are the fp32 values the library uses (fp64 on the host, normalised, rounded once), cast to the
working type."""
import math

import torch
import torch.nn.functional as TF


def f32(v):
    """the value an entry receives for a `float` argument"""
    return float(torch.tensor(float(v), dtype=torch.float32))


def window(k, sigma):
    sigma = f32(sigma)
    t = [math.exp(-((i - (k - 1) / 2.0) ** 2) / (2.0 * sigma * sigma)) for i in range(k)]
    s = 0.0
    for v in t:
        s += v
    return torch.tensor([v / s for v in t], dtype=torch.float64).float()


def gfilter(x, g):
    """the valid separable filter G * x of [N,C,H,W]"""
    C = x.shape[1]
    x = TF.conv2d(x, g.view(1, 1, 1, -1).expand(C, 1, 1, -1), groups=C)
    return TF.conv2d(x, g.view(1, 1, -1, 1).expand(C, 1, -1, 1), groups=C)


def gadjoint(y, g):
    """G^T * y, the full correlation: y padded by k-1 zeros on every side, the flipped window"""
    k = g.numel()
    return gfilter(TF.pad(y, (k - 1, k - 1, k - 1, k - 1)), g.flip(0))


def constants(data_range=2.0):
    return (0.01 * data_range) ** 2, (0.03 * data_range) ** 2


def terms(a, b, g, c1, c2):
    mua, mub = gfilter(a, g), gfilter(b, g)
    va, vb, cov = gfilter(a * a, g) - mua * mua, gfilter(b * b, g) - mub * mub, gfilter(a * b, g) - mua * mub
    A1, A2 = 2 * mua * mub + c1, 2 * cov + c2
    B1, B2 = mua * mua + mub * mub + c1, va + vb + c2
    return mua, mub, A1, A2, B1, B2, A1 * A2 / (B1 * B2)


def ssim_map(a, b, k=11, sigma=1.5, data_range=2.0):
    c1, c2 = constants(data_range)
    return terms(a, b, window(k, sigma).to(a.dtype), c1, c2)[-1]


def ssim_reference(a, b, k=11, sigma=1.5, data_range=2.0, dtype=torch.float64):
    """a, b: [N,C,H,W] CPU tensors holding fp32 values.  -> dict: loss = 1 - mean S, per_sample [N], l1 = mean |a - b|, grad_ssim =
    d loss / d a, grad_l1 = d l1 / d a, all in `dtype`."""
    a = a.detach().to(dtype).clone().requires_grad_(True)
    b = b.detach().to(dtype)
    S = ssim_map(a, b, k, sigma, data_range)
    loss = 1 - S.mean()
    (gs,) = torch.autograd.grad(loss, a)
    l1 = (a - b).abs().mean()
    (gl,) = torch.autograd.grad(l1, a)
    return {"loss": loss.detach(), "per_sample": S.detach().mean(dim=(1, 2, 3)), "l1": l1.detach(), "grad_ssim": gs, "grad_l1": gl,
            "S": S.detach()}


def closed_form_gradient(a, b, k=11, sigma=1.5, data_range=2.0):
    """d (1 - mean S) / d a from the coefficient maps P1, P2, P3 and the adjoint filter, in a's type"""
    g = window(k, sigma).to(a.dtype)
    c1, c2 = constants(data_range)
    mua, mub, A1, A2, B1, B2, S = terms(a, b, g, c1, c2)
    P1 = 2 * mub * (A2 - A1) / (B1 * B2) - 2 * mua * S * (1 / B1 - 1 / B2)
    P2 = -S / B2
    P3 = 2 * A1 / (B1 * B2)
    return -(gadjoint(P1, g) + 2 * a * gadjoint(P2, g) + b * gadjoint(P3, g)) / S.numel()


def make_inputs(kind, N, C, H, W, seed):
    """The three input regimes, as fp32 [N,C,H,W]: noise against noise, a near copy, a flat region (the cancellation regime)."""
    gen = torch.Generator().manual_seed(seed)
    if kind == "noise":
        a, b = torch.tanh(torch.randn(N, C, H, W, generator=gen)), torch.tanh(torch.randn(N, C, H, W, generator=gen))
    elif kind == "near":
        b = torch.tanh(torch.randn(N, C, H, W, generator=gen))
        a = (b + 0.05 * torch.randn(N, C, H, W, generator=gen)).clamp(-1, 1)
    elif kind == "flat":
        a = 0.9 + 1e-3 * torch.randn(N, C, H, W, generator=gen)
        b = 0.9 + 1e-3 * torch.randn(N, C, H, W, generator=gen)
    else:
        raise ValueError(kind)
    return a.float(), b.float()
