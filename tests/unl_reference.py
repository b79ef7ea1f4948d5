"""The losses of the unlabelled head by their definitions, in fp64 torch on the CPU: F.interpolate(align_corners=True) -> log_softmax ->
entropy / max-squares / thresholded pseudo-label cross entropy, the gradient by autograd.  tests/test_unl_host.py and
tests/test_unl_gpu.py share it (not a test module: nothing here is collected)."""
import math

import torch
import torch.nn.functional as TF

TAU = {1: 0.5, 4: 0.6, 20: 0.35, 21: 0.35, 64: 0.2}      # the thresholds the inputs below are chosen for, per class count
MARGIN = 1e-4                                            # fp64 |conf - tau| and top-two gap of every pixel of a test input


def make_logits(seed, N, C, H, W, scale=3.0):
    """fp32-representable logits randn * scale as fp64 [N, C, H, W]"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, C, H, W, generator=g, dtype=torch.float32) * scale).double()


def first_max(p):
    """(value, index) of the first maximum over dim 1 - strict > from class 0 up"""
    C = p.shape[1]
    conf = p.max(1).values
    idx = torch.arange(C).view(1, C, 1, 1).expand_as(p)
    y = torch.where(p == conf.unsqueeze(1), idx, torch.full_like(idx, C)).min(1).values
    return conf, y


def unl_reference(x64, tau, resize=None, g=(1.0, 1.0, 1.0), R64=None):
    """dict(ent, msq, pl: the three losses; sums fp64 [4] = (sum H, sum sum p^2, sum of the kept cross entropies, K); pseudo: uint8
    [N, OH, OW], 255 = dropped; grad: d (g[0] ent + g[1] msq + g[2] pl + sum(softmax * R64)) / dx; conf_margin / gap_margin: the
    smallest |conf - tau| and top-two probability gap over the pixels; kept_share; max_u: max |z_c - max z|; up: the resized logits)."""
    x = x64.clone().requires_grad_(True)
    up = x if resize is None else TF.interpolate(x, size=tuple(resize), mode="bilinear", align_corners=True)
    N, C, OH, OW = up.shape
    V = N * OH * OW
    logp = torch.log_softmax(up, 1)
    p = logp.exp()
    H = -(p * logp).sum(1)                       # (log_softmax stays finite where p vanishes: 0 * -400, not 0 * -inf)
    ent = H.sum() / (V * (math.log(C) if C > 1 else 1.0))
    sq = (p * p).sum()
    msq = -sq / (2.0 * V)
    conf, y = first_max(p.detach())
    kept = conf >= tau
    K = int(kept.sum())
    # = F.cross_entropy(up, y*, ignore_index=dropped, reduction="sum"), written on log_softmax (y* and the selection are constants)
    ce_sum = -(logp.gather(1, y.unsqueeze(1)).squeeze(1) * kept).sum()
    pl = ce_sum / max(K, 1)
    total = g[0] * ent + g[1] * msq + g[2] * pl
    if R64 is not None:
        total = total + (p * R64).sum()
    grad = torch.autograd.grad(total, x)[0]
    top2 = p.detach().topk(2, dim=1).values if C > 1 else None
    pseudo = torch.where(kept, y, torch.full_like(y, 255)).to(torch.uint8)
    upd = up.detach()
    return dict(ent=ent.detach(), msq=msq.detach(), pl=pl.detach(),
                sums=torch.tensor([float(H.sum().detach()), float(sq.detach()), float(ce_sum.detach()), float(K)], dtype=torch.float64),
                pseudo=pseudo, grad=grad, K=K, V=V, conf=conf,
                conf_margin=float((conf - tau).abs().min()),
                gap_margin=float((top2[:, 0] - top2[:, 1]).min()) if C > 1 else float("inf"),
                kept_share=K / float(V), max_u=float((upd - upd.max(1, keepdim=True).values).abs().max()), up=upd)


def closed_form_grad(x64, tau, resize=None, g=(1.0, 1.0, 1.0), R64=None):
    """The gradient the kernels form: q_c = dy_c - (g_e / (V ln C)) u_c - (g_m / V) p_c, d_c = p_c (q_c - sum_k p_k q_k) + [kept]
    (g_p / max(K, 1)) (p_c - [c == y*]) on the resized logits, then the adjoint of the resize (autograd of the LINEAR map only)."""
    x = x64.clone().requires_grad_(True)
    up = x if resize is None else TF.interpolate(x, size=tuple(resize), mode="bilinear", align_corners=True)
    with torch.no_grad():
        N, C, OH, OW = up.shape
        V = N * OH * OW
        u = up - up.max(1, keepdim=True).values
        e = u.exp()
        p = e / e.sum(1, keepdim=True)
        conf, y = first_max(p)
        kept = (conf >= tau).unsqueeze(1).double()      # (a bool times a Python float would round the factor to fp32)
        K = int(kept.sum())
        q = -(g[0] / (V * (math.log(C) if C > 1 else 1.0))) * u - (g[1] / V) * p
        if R64 is not None:
            q = q + R64
        onehot = torch.zeros_like(p).scatter_(1, y.unsqueeze(1), 1.0)
        d = p * (q - (p * q).sum(1, keepdim=True)) + kept * (g[2] / max(K, 1)) * (p - onehot)
    return torch.autograd.grad((up * d).sum(), x)[0]
