"""CutMix consistency for the mean teacher (include/sscg.h: sscg_mix_boxes, sscg_teacher_fwd_mix) by its definition, in fp64 torch /
numpy on the CPU: the teacher's maps are aligned per sample (un-mirrored where flip is set), resized with
F.interpolate(align_corners=True), mixed with where(pasted, a[p], a[n]) at the output resolution, and tests/teacher_reference.py's
arithmetic - unchanged, imported - runs on the mixed map with flip=None.  tests/test_teacher_mix_host.py and
tests/test_teacher_mix_gpu.py share it (not a test module: nothing here is collected)."""
import functools

import numpy as np
import torch
import torch.nn.functional as TF

from teacher_reference import MARGIN, closed_form_grad, mirror_where, soft_upstream, teacher_reference
from unl_reference import TAU, make_logits

CLASSES = [1, 4, 20, 21, 64]            # the compile-time arms (4, 20, 21) and the run-time arm (1, 64)
# (N, H, W, OH, OW) and which samples' teacher saw the mirrored image
GEOMS = [(3, 3, 4, 13, 17),             # three samples: a partner cycle meets both flip values; one block per sample
         (2, 5, 5, 21, 23),             # 483 output pixels: a sample spans two 256-thread blocks, the interior box crosses the seam
         (1, 2, 7, 9, 28)]              # a batch of one: any table is the identity
FLIPS = [(1, 0, 1), (1, 0), (1,)]
DET_GEOM, DET_CLASSES, DET_FLIPS = (2, 9, 11, 67, 83), 21, (0, 1)       # the determinism case only
TEMP = 1.0                              # the thresholds are unl_reference.TAU's, chosen for temperature 1
# (index into GEOMS, C) -> the seed of mix_inputs_of: the first of 0..39 that meets the conditions of seed_ok (search_seeds)
SEEDS = {
    (0, 1): 0, (0, 4): 0, (0, 20): 0, (0, 21): 1, (0, 64): 1,
    (1, 1): 0, (1, 4): 4, (1, 20): 0, (1, 21): 0, (1, 64): 19,
    (2, 1): 0, (2, 4): 0, (2, 20): 0, (2, 21): 0, (2, 64): 0,
}


def interior_box(OH, OW):
    """(x0, y0, x1, y1): half the height by half the width, off centre; at 21 x 23 rows 7..16 - the block seam is pixel 256, row 11"""
    return OW // 4, OH // 3, OW // 4 + OW // 2, OH // 3 + OH // 2


def tables_of(gi_or_geom):
    """name -> int32 [N, 8] rows (partner, x0, y0, x1, y1, 0, 0, 0) of a geometry, in a fixed order.  The partner is the next sample
    unless the name says otherwise: in a batch of one that is the sample itself, and every table is the identity."""
    N, H, W, OH, OW = GEOMS[gi_or_geom] if isinstance(gi_or_geom, int) else gi_or_geom
    nxt = [(n + 1) % N for n in range(N)]

    def rows(partners, box):
        t = np.zeros((N, 8), dtype=np.int32)
        for n in range(N):
            t[n, 0] = partners[n]
            t[n, 1:5] = box[n] if isinstance(box, list) else box
        return t
    inner = interior_box(OH, OW)
    out = {
        "identity": rows(list(range(N)), (0, 0, OW, OH)),                  # the partner is the sample: not mixed, whatever the box
        "empty": rows(nxt, (3, 3, 3, 3)),
        "empty_rev": rows(nxt, (OW - 2, 4, 2, OH)),                        # x1 < x0
        "whole": rows(nxt, (0, 0, OW, OH)),
        "corner_tl": rows(nxt, (0, 0, 1, 1)),
        "corner_tr": rows(nxt, (OW - 1, 0, OW, 1)),
        "corner_bl": rows(nxt, (0, OH - 1, 1, OH)),
        "corner_br": rows(nxt, (OW - 1, OH - 1, OW, OH)),
        "interior": rows(nxt, inner),
        "outside": rows(nxt, (-5, 2, OW + 7, OH - 2)),                     # negative x0, x1 > OW: plain compares, no clamping
        "bad_partner": rows([-1, N] + [N + 5] * max(N - 2, 0), (0, 0, OW, OH)),
        "mixed_rows": rows(nxt, [inner if n % 2 == 0 else (3, 3, 3, 3) for n in range(N)]),      # a mixing and a plain sample in one call
    }
    if N == 3:
        out["cycle_a"] = rows([1, 2, 0], inner)
        out["cycle_b"] = rows([2, 0, 1], inner)
        out["cycle_a_whole"] = rows([1, 2, 0], (0, 0, OW, OH))
        out["cycle_b_whole"] = rows([2, 0, 1], (0, 0, OW, OH))
    return out


INTERIOR = ("interior", "mixed_rows", "cycle_a", "cycle_b")       # the tables whose kept and agreement shares seed_ok bounds
NOTHING = ("identity", "empty", "empty_rev", "bad_partner")       # the tables that mix nothing


def pasted(table, OH, OW):
    """(bool [N, OH, OW], partner per sample) by the rule of the entries: 0 <= p < N, p != n, x0 <= x < x1, y0 <= y < y1"""
    table = np.asarray(table).astype(np.int64)
    N = table.shape[0]
    ys, xs = np.meshgrid(np.arange(OH), np.arange(OW), indexing="ij")
    mask, partner = np.zeros((N, OH, OW), dtype=bool), np.arange(N)
    for n in range(N):
        p, x0, y0, x1, y1 = (int(v) for v in table[n, :5])
        if 0 <= p < N and p != n:
            partner[n] = p
            mask[n] = (xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)
    return torch.from_numpy(mask), partner


def mixed_teacher(t64, flip, table, size):
    """The teacher's map the student is held to, [N, C, OH, OW]: 1. align per sample (un-mirror where flip), 2. resize, 3. where(pasted,
    a[p], a[n]).  t64: the teacher's logits as the entry receives them (sample n mirrored where flip[n])."""
    a = mirror_where(t64, flip)
    if tuple(a.shape[2:]) != tuple(size):
        a = TF.interpolate(a, size=tuple(size), mode="bilinear", align_corners=True)
    mask, partner = pasted(table, size[0], size[1])
    return torch.where(mask.unsqueeze(1), a[torch.as_tensor(partner)], a)


def mix_teacher_reference(x64, t64, flip, table, tau, temp, size, g=(1.0, 1.0), R64=None):
    """teacher_reference's dict for the mix entry: its arithmetic, flip=None, on the mixed map (F.interpolate with align_corners=True
    to the size a map already has is the identity, so the mixed map passes through teacher_reference's own resize unchanged)"""
    return teacher_reference(x64, mixed_teacher(t64, flip, table, size), None, tau, temp, tuple(size), g, R64)


def mix_closed_form_grad(x64, t64, flip, table, tau, temp, size, g=(1.0, 1.0), R64=None):
    return closed_form_grad(x64, mixed_teacher(t64, flip, table, size), None, tau, temp, tuple(size), g, R64)


def mix_inputs_of(seed, geom, C, flips):
    """(student logits, teacher logits as the kernel receives them): teacher_reference.inputs_of's construction on a geometry of this
    module - the ALIGNED teacher is the student plus noise, and sample n of the teacher's map is that, mirrored where flips[n]"""
    N, H, W, OH, OW = geom
    xs = make_logits(seed, N, C, H, W)
    aligned = (xs.float() + make_logits(100 + seed, N, C, H, W, scale=1.5).float()).double()
    return xs, mirror_where(aligned, flips)


def case_inputs(gi, C):
    """(student logits, teacher logits, flip, tau, temp) of a GPU test case"""
    return mix_inputs_of(SEEDS[(gi, C)], GEOMS[gi], C, FLIPS[gi]) + (FLIPS[gi], TAU[C], TEMP)


def seed_ok(seed, gi, C):
    """The conditions on a GPU test's input (not measurements).  The margins - in fp64 |conf - tau| and both top-two gaps at least
    MARGIN - are properties of each sample's own pixels, so they are checked once, on the unmixed batch, and then hold for every
    table.  For C > 1 the kept share and the agreement share lie in [0.1, 0.9] under every interior-box table."""
    N, H, W, OH, OW = GEOMS[gi]
    x, t = mix_inputs_of(seed, GEOMS[gi], C, FLIPS[gi])
    tabs = tables_of(gi)
    plain = mix_teacher_reference(x, t, FLIPS[gi], tabs["identity"], TAU[C], TEMP, (OH, OW))
    if plain["conf_margin"] < MARGIN or plain["gap_margin"] < MARGIN:
        return False
    if C > 1:
        for name in INTERIOR:
            if name in tabs:
                r = mix_teacher_reference(x, t, FLIPS[gi], tabs[name], TAU[C], TEMP, (OH, OW))
                if not (0.1 <= r["kept_share"] <= 0.9 and 0.1 <= r["agree_share"] <= 0.9):
                    return False
    return True


def search_seeds(limit=40):
    """The table above, recomputed: per case the first seed below `limit` that passes seed_ok (None: none does)"""
    return {(gi, C): next((s for s in range(limit) if seed_ok(s, gi, C)), None) for gi in range(len(GEOMS)) for C in CLASSES}


@functools.lru_cache(maxsize=None)
def reference(gi, C, name, g=(1.0, 1.0), soft_seed=None):
    """mix_teacher_reference of a case and a table, computed once and shared (left unchanged by its readers)"""
    N, H, W, OH, OW = GEOMS[gi]
    x, t, flip, tau, temp = case_inputs(gi, C)
    R = soft_upstream(soft_seed, N, C, OH, OW) if soft_seed is not None else None
    return mix_teacher_reference(x, t, flip, tables_of(gi)[name], tau, temp, (OH, OW), g, R)


__all__ = ["CLASSES", "DET_CLASSES", "DET_FLIPS", "DET_GEOM", "FLIPS", "GEOMS", "INTERIOR", "MARGIN", "NOTHING", "SEEDS", "TAU", "TEMP",
           "case_inputs", "interior_box", "mix_closed_form_grad", "mix_inputs_of", "mix_teacher_reference", "mixed_teacher", "pasted",
           "reference", "search_seeds", "seed_ok", "tables_of"]
