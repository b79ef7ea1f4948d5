"""Segmented stable radix sort on the MI355X (sscg_sort_u32_desc, functional.sort_u32_desc) against numpy's stable argsort, bit for
bit in both outputs: lengths around the wave, the block and the scatter kernel's per-block chunk, one and five segments, key
patterns that exercise every digit, ties and the pass skipping; outputs and workspace between 0xFF guards; a short workspace; a
workspace filled with 0xFF."""
import numpy as np
import pytest
import torch

from lovasz_reference import sort_u32_desc_reference

pytestmark = pytest.mark.gpu


def lengths(F):
    chunk = F.lib.sscg_sort_chunk()
    return [1, 2, 63, 64, 65, 255, 256, 257, chunk - 1, chunk, chunk + 1, 3 * chunk + 77]


PATTERNS = ["equal", "top_digit", "bottom_digit", "sorted", "reverse", "four_values", "random"]


def make_keys(pattern, S, L, seed):
    """(keys uint32 [S, L], the `upper` bound to pass: None = none)"""
    rng = np.random.RandomState(seed)
    if pattern == "equal":
        return np.full((S, L), 0x12345678, np.uint32), None
    if pattern == "top_digit":
        return np.where(rng.rand(S, L) < 0.5, 0x01000000, 0xFF000000).astype(np.uint32), None
    if pattern == "bottom_digit":
        return np.where(rng.rand(S, L) < 0.5, 0x3F800001, 0x3F8000FE).astype(np.uint32), 0x3F800100
    if pattern == "sorted":
        return np.tile(np.arange(L, 0, -1, dtype=np.uint32) * 3, (S, 1)), 3 * L + 1
    if pattern == "reverse":
        return np.tile(np.arange(L, dtype=np.uint32) * 1021, (S, 1)), None
    if pattern == "four_values":
        return np.asarray([0, 5, 0x3F800001, 0x00010000], np.uint32)[rng.randint(0, 4, size=(S, L))], 0x3F800002
    return rng.randint(0, 2 ** 32, size=(S, L), dtype=np.uint64).astype(np.uint32), None


def dev_keys(keys, dev):
    return torch.from_numpy(keys.view(np.int32)).to(dev)


def as_u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("S", [1, 5])
def test_sort_equals_numpys_stable_argsort(S, F, dev):
    for L in lengths(F):
        for pi, pattern in enumerate(PATTERNS):
            keys, upper = make_keys(pattern, S, L, 1000 * S + 10 * pi + L % 7)
            want_k, want_i = sort_u32_desc_reference(keys)
            got_k, got_i = F.sort_u32_desc(dev_keys(keys, dev), upper=upper)
            assert got_i.dtype == torch.int32 and got_k.shape == (S, L)
            assert np.array_equal(as_u32(got_k), want_k), (S, L, pattern)
            assert np.array_equal(got_i.cpu().numpy(), want_i), (S, L, pattern)
            if pattern == "equal":
                assert (got_i.cpu() == torch.arange(L, dtype=torch.int32)).all()
            if upper is not None:                                                  # the bound only skips passes: the same bits without it
                full_k, full_i = F.sort_u32_desc(dev_keys(keys, dev))
                assert torch.equal(full_k, got_k) and torch.equal(full_i, got_i), (S, L, pattern)


def test_a_single_row_is_a_single_segment(F, dev):
    keys, _ = make_keys("random", 1, 300, 3)
    k, i = F.sort_u32_desc(dev_keys(keys[0], dev))
    want_k, want_i = sort_u32_desc_reference(keys)
    assert k.shape == (300,) and np.array_equal(as_u32(k), want_k[0]) and np.array_equal(i.cpu().numpy(), want_i[0])


def raw_sort(F, dev, keys, upper, fill, short=0):
    """sscg_sort_u32_desc itself: outputs and workspace inside 0xFF-filled allocations (256 guard bytes on either side), the
    workspace filled with `fill` first.  (rc, sorted, index)"""
    lib = F.lib
    S, L = keys.shape
    n = S * L * 4
    nws = lib.sscg_sort_ws_bytes(S, L)
    G = 256
    bufs = [torch.full((sz + 2 * G,), 0xFF, dtype=torch.uint8, device=dev) for sz in (n, n, nws)]
    bufs[2][G:G + nws] = fill
    kd = dev_keys(keys, dev)
    before = kd.clone()
    rc = lib.sscg_sort_u32_desc(kd.data_ptr(), S, L, 0 if upper is None else upper, bufs[0].data_ptr() + G, bufs[1].data_ptr() + G,
                                bufs[2].data_ptr() + G, nws - short, F._stream())
    torch.cuda.synchronize()
    for b, sz in zip(bufs, (n, n, nws)):
        assert (b[:G] == 0xFF).all() and (b[G + sz:] == 0xFF).all(), "guard bytes"
    assert torch.equal(kd, before), "the input is read only"
    out_k = bufs[0][G:G + n].clone().view(torch.int32).view(S, L)
    out_i = bufs[1][G:G + n].clone().view(torch.int32).view(S, L)
    return rc, out_k, out_i


def test_guards_short_workspace_and_dirty_workspace(F, dev):
    chunk = F.lib.sscg_sort_chunk()
    for S, L in ((5, 257), (1, 3 * chunk + 77), (5, chunk + 1)):
        # keys without the byte 0xFF in any position, indices below 2^24: an element the sort did not write would still read 0xFF..FF
        rng = np.random.RandomState(S + L)
        keys = rng.randint(0, 0xFE, size=(S, L, 4)).astype(np.uint8).view(np.uint32).reshape(S, L)
        want_k, want_i = sort_u32_desc_reference(keys)
        rc, k0, i0 = raw_sort(F, dev, keys, None, 0x00)
        assert rc == 0
        assert np.array_equal(as_u32(k0), want_k) and np.array_equal(i0.cpu().numpy(), want_i), (S, L)     # every element was written
        rc, k1, i1 = raw_sort(F, dev, keys, None, 0xFF)
        assert rc == 0 and torch.equal(k0, k1) and torch.equal(i0, i1), (S, L)                            # whatever the workspace held
        rc, k2, i2 = raw_sort(F, dev, keys, None, 0x00, short=1)
        assert rc == -3 and (k2 == -1).all() and (i2 == -1).all()                                         # refused: nothing was touched
