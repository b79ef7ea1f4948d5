"""The Lovasz-softmax loss (Berman, Triki, Blaschko, CVPR 2018) restated in fp64 with numpy / torch on the CPU, from the definition
in include/sscg.h (sscg_lovasz_fwd) and the paper - the reference of tests/test_lovasz_host.py and tests/test_lovasz_gpu.py - and
the inputs those two files share.

For a segment (the call, or one sample) and a class c: f_i = [y_i == c], e_i = |f_i - p_i,c| over the V counted pixels, ordered by e
descending with ties by ascending pixel index; F_j foreground pixels among the first j, I_j = G - F_j, U_j = G + j - F_j,
J_j = 1 - I_j / U_j, J_0 = 0, g_j = J_j - J_{j-1}; loss = sum_j e_(j) g_j.  g is a constant of the backward."""
import numpy as np
import torch
import torch.nn.functional as TF

EPS32 = 2.0 ** -23


def stable_desc_argsort(keys):
    """Positions of `keys` (1-D; unsigned integers or floats) in descending order, equal keys by ascending position."""
    k = np.asarray(keys)
    k = k.astype(np.int64) if k.dtype.kind in "iu" else k.astype(np.float64)
    return np.argsort(-k, kind="stable")


def sort_u32_desc_reference(keys):
    """numpy's answer to functional.sort_u32_desc: (sorted uint32 [S, L], index int32 [S, L])"""
    keys = np.asarray(keys, dtype=np.uint32)
    idx = np.stack([stable_desc_argsort(row) for row in keys]) if keys.shape[0] else np.zeros(keys.shape, np.int64)
    return np.take_along_axis(keys, idx, 1), idx.astype(np.int32)


def lovasz_grad_closed(fg_sorted):
    """g_j in closed form from exact integers, fp64: 1 / U_j at a foreground pixel, I_j / (U_j (U_j - 1)) at a background pixel,
    1 / (G + 1) at a background pixel of rank 1."""
    f = np.asarray(fg_sorted, dtype=bool)
    V = f.size
    G = int(f.sum())
    F = np.cumsum(f.astype(np.int64))
    j = np.arange(1, V + 1, dtype=np.int64)
    inter = (G - F).astype(np.float64)
    U = (G + j - F).astype(np.float64)
    g = np.empty(V, np.float64)
    g[f] = 1.0 / U[f]
    b = ~f
    first = b & (j == 1)
    rest = b & (j > 1)
    g[first] = 1.0 / (G + 1.0)
    g[rest] = inter[rest] / (U[rest] * (U[rest] - 1.0))
    return g


def lovasz_grad_diff(fg_sorted):
    """g_j = J_j - J_{j-1}, J_j = 1 - I_j / U_j, J_0 = 0: the difference form of the paper's Algorithm 1, fp64."""
    f = np.asarray(fg_sorted, dtype=bool)
    V = f.size
    G = int(f.sum())
    F = np.cumsum(f.astype(np.int64))
    j = np.arange(1, V + 1, dtype=np.int64)
    J = 1.0 - (G - F).astype(np.float64) / (G + j - F).astype(np.float64)
    return np.diff(np.concatenate([[0.0], J]))


def lovasz_reference(p, lab, classes="present", per_image=False, skip=(), keys=None):
    """The loss as a torch fp64 scalar, differentiable in p with g held constant.  p: fp64 [N, C, OH, OW] probabilities; lab: int64
    [N, OH, OW]; keys: an integer array [N, C, OH, OW] that decides the order in place of the errors themselves (the device's keys:
    the order is then decided bit for bit), or None.  `skip`ped classes never take part; "present": only classes with a foreground
    pixel in the segment; a segment without a class gives 0; with per_image only samples with a counted pixel enter the mean."""
    N, C = p.shape[:2]
    segs = [[n] for n in range(N)] if per_image else [list(range(N))]
    zero = p.sum() * 0.0
    seg_losses = []
    for seg in segs:
        ps = p[seg].permute(1, 0, 2, 3).reshape(C, -1)                 # [C][pixels of the segment, sample-major]
        ls = lab[seg].reshape(-1)
        counted = (ls >= 0) & (ls < C)
        if per_image and not bool(counted.any()):
            continue
        idx = counted.nonzero().squeeze(1)
        ks = None if keys is None else np.asarray(keys)[seg].transpose(1, 0, 2, 3).reshape(C, -1)
        terms = []
        for c in range(C):
            if c in skip:
                continue
            f = ls[idx] == c
            if classes == "present" and not bool(f.any()):
                continue
            e = (f.double() - ps[c][idx]).abs()
            order = stable_desc_argsort(e.detach().numpy() if ks is None else ks[c][idx.numpy()])
            g = torch.from_numpy(lovasz_grad_closed(f.numpy()[order]))
            terms.append((e[torch.from_numpy(order)] * g).sum())
        seg_losses.append(sum(terms) / len(terms) if terms else zero)
    return sum(seg_losses) / len(seg_losses) if seg_losses else zero


def probabilities(x, resize=None):
    """softmax over C of the logits, resized first (bilinear, align_corners=True) when resize = (OH, OW); in x's dtype"""
    up = x if resize is None else TF.interpolate(x, size=resize, mode="bilinear", align_corners=True)
    return torch.softmax(up, 1)


def errors(p, lab):
    """|f - p| [N, C, OH, OW] in p's dtype (zero where the pixel is ignored)"""
    C = p.shape[1]
    counted = (lab >= 0) & (lab < C)
    f = torch.zeros_like(p)
    f.scatter_(1, torch.where(counted, lab, torch.zeros_like(lab)).unsqueeze(1), 1.0)
    f = f * counted.unsqueeze(1)
    return (f - p).abs() * counted.unsqueeze(1)


def end_to_end(x64, lab, resize=None, **opts):
    """(loss, d loss / d logits) in fp64 by autograd through the resize and the softmax"""
    x = x64.clone().requires_grad_(True)
    loss = lovasz_reference(probabilities(x, resize), lab, **opts)
    if not loss.requires_grad:
        return float(loss), torch.zeros_like(x64)
    return float(loss.detach()), torch.autograd.grad(loss, x)[0]


# ---- the inputs the host and the GPU tests share: (name, N, C, H, W, OH, OW)
GEOMS = [("head4", 2, 4, 5, 7, 13, 19), ("head21", 2, 21, 5, 7, 13, 19), ("flat4", 2, 4, 13, 19, 13, 19)]
LABELS = ["mixed", "void_sample", "single"]
OPTIONS = [dict(classes="present", per_image=False, skip=()), dict(classes="all", per_image=False, skip=()),
           dict(classes="present", per_image=True, skip=()), dict(classes="all", per_image=True, skip=()),
           dict(classes="all", per_image=False, skip=(0, 2)), dict(classes="present", per_image=True, skip=(1,))]
ABSENT = {4: 2, 21: 7}            # the class no label carries
# one seed per (geometry, labels): tests/test_lovasz_host.py checks that on each the fp32 and the fp64 order of the errors agree
SEEDS = {(g[0], l): 100 * gi + li for gi, g in enumerate(GEOMS) for li, l in enumerate(LABELS)}


def make_case(geom, labels, seed=None):
    """(logits fp64 [N, C, H, W], labels int64 [N, OH, OW]): 255s, one class absent everywhere; "void_sample": sample 1 ignored
    entirely; "single": every counted pixel carries class 1."""
    name, N, C, H, W, OH, OW = geom
    rng = np.random.RandomState(SEEDS[(name, labels)] if seed is None else seed)
    x = torch.from_numpy(rng.randn(N, C, H, W) * 2.0)
    present = [c for c in range(C) if c != ABSENT[C]]
    lab = np.asarray(present)[rng.randint(0, len(present), size=(N, OH, OW))].astype(np.int64)
    if labels == "single":
        lab[:] = 1
    lab[rng.rand(N, OH, OW) < 0.15] = 255
    if labels == "void_sample":
        lab[1] = 255
    return x, torch.from_numpy(lab)
