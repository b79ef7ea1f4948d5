"""Numpy restatement of the calibration counts (include/sscg.h: sscg_calib_stats) - the pin of tests/test_calibration_gpu.py, checked
on its own in tests/test_calibration_host.py.  No torch, no GPU.

It takes the fp32 PROBABILITY map of one temperature, [N, OH, OW, C], and the labels, and forms bins, cls and sums by the entry's own
fp32 and fp64 expressions: np.float32 multiplies for the bin and for Q24, truncation, the first maximum via argmax, the fp64 log of
the clamped fp32 value.  The probabilities themselves are the device's separate passes' (the GPU test makes them); nothing here
resizes or exponentiates."""
import numpy as np

Q24 = np.float32(16777216.0)
TINY = np.float64(2.0) ** -126          # 0x1p-126: the clamp under the logarithm


def bin_of(conf, B):
    """min(B - 1, (int)(conf * (float)B)) for fp32 confidences: one fp32 multiply, truncation."""
    conf = np.asarray(conf, dtype=np.float32)
    prod = conf * np.float32(B)
    assert prod.dtype == np.float32
    return np.minimum(B - 1, prod.astype(np.int64))


def q24_of(conf):
    """(int64)(conf * 2^24) for fp32 confidences: the multiply is exact, the conversion truncates."""
    conf = np.asarray(conf, dtype=np.float32)
    prod = conf * Q24
    assert prod.dtype == np.float32
    return prod.astype(np.int64)


def stats_one(probs, labels, B):
    """One temperature: probs fp32 [N, OH, OW, C] (or [pixels, C]), labels integers of as many pixels -> bins int64 [B, 3], cls int64
    [C, 3], sums float64 [2].  A pixel is counted when its label is in [0, C)."""
    p = np.asarray(probs)
    assert p.dtype == np.float32
    C = p.shape[-1]
    p = p.reshape(-1, C)
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    assert lab.size == p.shape[0]
    keep = (lab >= 0) & (lab < C)
    p, lab = p[keep], lab[keep]
    bins, cls, sums = np.zeros((B, 3), dtype=np.int64), np.zeros((C, 3), dtype=np.int64), np.zeros(2, dtype=np.float64)
    if lab.size == 0:
        return bins, cls, sums
    rows = np.arange(lab.size)
    pred = np.argmax(p, axis=1)                       # the first maximum
    conf = p[rows, pred]
    hit = (pred == lab).astype(np.int64)
    b, q = bin_of(conf, B), q24_of(conf)
    for table, key, size in ((bins, b, B), (cls, pred, C)):
        table[:, 0] = np.bincount(key, minlength=size)
        table[:, 1] = np.bincount(key, weights=hit, minlength=size).astype(np.int64)
        np.add.at(table[:, 2], key, q)                # integer adds: exact in any order
    p64 = p.astype(np.float64)
    sums[0] = np.sum(-np.log(np.maximum(p64[rows, lab], TINY)))
    onehot = np.zeros_like(p64)
    onehot[rows, lab] = 1.0
    sums[1] = np.sum((p64 - onehot) ** 2)
    return bins, cls, sums


def stats(prob_maps, labels, B):
    """A list of NT probability maps (one per temperature) -> bins [NT, B, 3], cls [NT, C, 3], sums [NT, 2]."""
    parts = [stats_one(p, labels, B) for p in prob_maps]
    return tuple(np.stack([part[k] for part in parts]) for k in range(3))


def ece_by_hand(bins_t):
    """sum_b n_b / n |hit_b / n_b - qsum_b / (2^24 n_b)| of one temperature's bins, bin by bin in Python floats."""
    n = float(sum(int(r[0]) for r in bins_t))
    ece, mce = 0.0, 0.0
    for cnt, hit, q in ((int(r[0]), int(r[1]), int(r[2])) for r in bins_t):
        if cnt:
            gap = abs(hit / cnt - q / (16777216.0 * cnt))
            ece += cnt / n * gap
            mce = max(mce, gap)
    return ece, mce
