"""include/sscg.h, sscg_augment_mix_u8, restated in numpy - what tests/test_augment_mix_host.py and tests/test_augment_mix_gpu.py
compare the product against, bit for bit.  The unmixed batch is elastic_reference's (tests/elastic_reference.py: the affine, colour
and elastic pipeline, with or without a lattice); on top of it this file states only the mixing rule, pixel list by pixel list, and
does not call the product's own statement of it (data_utils.augmentations.mix_batch)."""
import numpy as np

from elastic_reference import elastic_reference


def pasted_mask(table, classes, cls_maps, out_size):
    """bool [N, OH, OW] and the partner per sample (-1 = not mixed): table int [N, 8] = (partner, x0, y0, x1, y1, mask_lo, mask_hi,
    0); cls_maps int64 [N, OH, OW] = every sample's UNMIXED class map (lut256[raw id], the fill included), needed with `classes`."""
    OH, OW = out_size
    N = len(table)
    mask = np.zeros((N, OH, OW), dtype=bool)
    partner = np.full(N, -1, dtype=np.int64)
    for n in range(N):
        p, x0, y0, x1, y1, lo, hi = (int(v) for v in table[n][:7])
        if p < 0 or p >= N or p == n:
            continue
        partner[n] = p
        bits = ((hi % 2 ** 32) << 32) | (lo % 2 ** 32)                       # the two int32 words as unsigned
        oy, ox = np.meshgrid(np.arange(OH), np.arange(OW), indexing="ij")
        mask[n] = (x0 <= ox) & (ox < x1) & (y0 <= oy) & (oy < y1)
        if classes:
            c = np.asarray(cls_maps[p], dtype=np.int64)
            small = (c >= 0) & (c < 64)
            shift = np.where(small, c, 0).astype(np.uint64)
            mask[n] |= small & (((np.uint64(bits) >> shift) & np.uint64(1)) == np.uint64(1))
    return mask, partner


def mix_reference(img, gt, mats, nodes, grid, out_size, mean, std, lut, table, classes, image_fill=0, label_fill=0, colours=None,
                  need_mean=False, plain=None):
    """-> (float32 [N,OH,OW,C], int64 [N,OH,OW] or None, pasted bool [N,OH,OW], plain): where(pasted, plain[p], plain[n]) with plain =
    elastic_reference(...) of the same batch (`plain`: one computed before, to share it among tests)."""
    if plain is None:
        plain = elastic_reference(img, gt, mats, nodes, grid, out_size, mean, std, lut, image_fill, label_fill, colours=colours,
                                  need_mean=need_mean)
    ref_img, ref_gt = plain
    assert not classes or ref_gt is not None
    mask, partner = pasted_mask(table, classes, ref_gt, out_size)
    out_img, out_gt = ref_img.copy(), (ref_gt.copy() if ref_gt is not None else None)
    for n in range(len(table)):
        if partner[n] < 0:
            assert not mask[n].any()
            continue
        out_img[n] = np.where(mask[n][..., None], ref_img[partner[n]], ref_img[n])
        if ref_gt is not None:
            out_gt[n] = np.where(mask[n], ref_gt[partner[n]], ref_gt[n])
    return out_img, out_gt, mask, plain
