"""The boundary loss on signed distance maps (include/sscg.h: sscg_sdm, sscg_boundary_loss_fwd) restated with numpy / scipy / torch on the
CPU: the signed squared distance map, the level set, the loss in fp64 and its gradient by fp64 autograd.  tests/test_boundary_loss_host.py
holds this file to literals, to a brute force and to Kervadec's formula; tests/test_boundary_loss_gpu.py holds the kernels to this file."""
import numpy as np
import torch
import torch.nn.functional as TF
from scipy.ndimage import distance_transform_edt


def _d2(mask):
    """exact squared Euclidean distance of every True pixel of a 2-D mask to the nearest False one (integers; 0 at a False pixel)"""
    ind = distance_transform_edt(mask, return_distances=False, return_indices=True)      # the nearest background pixel's indices
    yy, xx = np.indices(mask.shape)
    return (ind[0] - yy).astype(np.int64) ** 2 + (ind[1] - xx).astype(np.int64) ** 2


def sdm_reference(labels, C):
    """labels int64 [N, H, W] (numpy or torch) -> int32 numpy [N, H, W, C]: +d2 at a non-member of class c, -d2 at a member, d2 the
    squared distance to the nearest pixel of the opposite membership in the sample; a zero plane where the class has no member in the
    sample or nothing but members."""
    lab = np.asarray(labels)
    N, H, W = lab.shape
    out = np.zeros((N, H, W, C), dtype=np.int32)
    for n in range(N):
        for c in range(C):
            pos = lab[n] == c
            if not pos.any() or pos.all():
                continue
            out[n, :, :, c] = np.where(pos, -_d2(pos), _d2(~pos)).astype(np.int32)
    return out


def sdm_brute(labels, C):
    """the same map by the definition: every pair of pixels, O(P^2) - for maps of a hundred pixels"""
    lab = np.asarray(labels)
    N, H, W = lab.shape
    yy, xx = np.indices((H, W))
    yy, xx = yy.reshape(-1).astype(np.int64), xx.reshape(-1).astype(np.int64)
    d2 = (yy[:, None] - yy[None, :]) ** 2 + (xx[:, None] - xx[None, :]) ** 2
    out = np.zeros((N, H, W, C), dtype=np.int32)
    for n in range(N):
        for c in range(C):
            pos = (lab[n] == c).reshape(-1)
            if not pos.any() or pos.all():
                continue
            opposite = pos[:, None] != pos[None, :]
            best = np.where(opposite, d2, np.iinfo(np.int64).max).min(1)
            out[n, :, :, c] = np.where(pos, -best, best).reshape(H, W).astype(np.int32)
    return out


def phi_reference(sdm):
    """the level set, fp32 numpy: sqrt(s) outside, 1 - sqrt(-s) inside, 0 on 0 - the cast, the square root and the subtraction each
    rounded once in fp32"""
    s = np.asarray(sdm)
    root = np.sqrt(np.abs(s).astype(np.float32))
    one = np.float32(1.0)
    return np.where(s > 0, root, np.where(s < 0, one - root, np.float32(0.0))).astype(np.float32)


def kervadec_phi(labels, C):
    """Kervadec's one_hot2dist per sample and class in fp64: distance(neg) * neg - (distance(pos) - 1) * pos, zeros for an absent class
    (and, pinned here, for a class that fills the sample)"""
    lab = np.asarray(labels)
    N, H, W = lab.shape
    out = np.zeros((N, H, W, C), dtype=np.float64)
    for n in range(N):
        for c in range(C):
            pos = lab[n] == c
            if not pos.any() or pos.all():
                continue
            neg = ~pos
            out[n, :, :, c] = distance_transform_edt(neg) * neg - (distance_transform_edt(pos) - 1) * pos
    return out


def boundary_reference(x64, lab, w32=None, resize=None, up64=None):
    """The definition in fp64 on the CPU: F.interpolate(align_corners=True) -> softmax -> sum of w_c p_c phi_c over the counted pixels
    / (V * sum w); gradient by autograd.  up64: resized logits to take instead of interpolating (no gradient then) - the forward
    checks pass the fp32 resize's own output, whose bits the loss is defined on.
    Returns dict(loss, grad, sums [N, C], scale [N, C] = the same sums over |p_c phi_c|, S = their weighted total, counted, k, phi, sdm)."""
    C = x64.shape[1]
    x = x64.clone().requires_grad_(True)
    if up64 is not None:
        up = up64
    else:
        up = x if resize is None else TF.interpolate(x, size=resize, mode="bilinear", align_corners=True)
    p = torch.softmax(up, 1)
    lab = torch.as_tensor(lab)
    sdm = sdm_reference(lab.numpy(), C)
    phi32 = phi_reference(sdm)
    phi = torch.from_numpy(phi32).double().permute(0, 3, 1, 2)
    counted = ((lab >= 0) & (lab < C))
    m = counted.unsqueeze(1).double()
    V = int(counted.sum())
    w = torch.ones(C, dtype=torch.float64) if w32 is None else w32.double()
    sums = (p * phi * m).sum((2, 3))
    scale = (p * phi * m).abs().sum((2, 3))
    k = 1.0 / (V * float(w.sum())) if V > 0 else 0.0
    loss = k * (w * sums.sum(0)).sum()
    grad = torch.autograd.grad(loss, x)[0] if (up64 is None and V > 0) else torch.zeros_like(x64)
    return dict(loss=loss.detach(), grad=grad, sums=sums.detach(), scale=scale.detach(), S=float((w * scale.detach().sum(0)).sum()),
                counted=V, k=k, phi=phi32, sdm=sdm)
