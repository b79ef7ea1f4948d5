"""Mixed-sample augmentation (CutMix, ClassMix) in the device batch finish, the parts that need no GPU: the `--augment cutmix=` /
`classmix=` items, the tables `Compose.mixes` draws, `mix_batch` against the restatement of tests/mix_reference.py, the loaders'
scope (the 'label' set, the device finish only), main.py's checks, the C entry's declaration and argument checks, the wrapper's -
and the conditions of the GPU tests' small case, which are properties of the reference alone."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_sub
from mix_reference import pasted_mask


def _aug():
    return load_sub("data_utils.augmentations")


# ------------------------------------------------------------------------------------------------ the spec
def test_from_spec_takes_the_two_items_and_refuses_bad_ones():
    A = _aug()
    comp = A.from_spec("hflip, cutmix=0.5 ,classmix=0.25,rotate=10", (32, 48), out_size=(32, 48))
    assert [type(o).__name__ for o in comp.ops] == ["RandomHorizontallyFlip", "RandomCutMix", "RandomClassMix", "RandomRotate"]
    cut, cls = comp.mix_ops
    assert (cut.p, cut.lo, cut.hi) == (0.5, 0.25, 0.5) and (cls.p, cls.skip) == (0.25, ()) and cls.keep == 2 ** 64 - 1
    assert [type(o).__name__ for o in comp.geometric_ops] == ["RandomHorizontallyFlip", "RandomRotate"] and comp.colour_ops == []
    (cut,) = A.from_spec("cutmix=1:0.1:0.1", (32, 48)).mix_ops
    assert (cut.p, cut.lo, cut.hi) == (1.0, 0.1, 0.1)
    (cls,) = A.from_spec("classmix=0:0:19:63", (32, 48)).mix_ops
    assert (cls.p, cls.skip) == (0.0, (0, 19, 63)) and cls.keep == 2 ** 64 - 1 - 1 - 2 ** 19 - 2 ** 63
    assert A.from_spec("hflip", (32, 48)).mix_ops == [] and A.from_spec("cutmix=1:0.5:1", (32, 48)).mix_ops[0].hi == 1.0
    for bad in ("cutmix", "cutmix=", "cutmix=0.5,cutmix=0.5", "classmix=0.5,hflip,classmix=0.5:1", "cutmix=1.5", "cutmix=-0.1", "cutmix=nan",
                "classmix=1.01", "classmix=-1", "classmix=nan", "cutmix=0.5:0.6:0.5", "cutmix=0.5:0:0.5", "cutmix=0.5:0.3", "cutmix=0.5:0.2:1.1",
                "cutmix=0.5:0.2:0.3:0.4", "cutmix=x", "classmix", "classmix=", "classmix=0.5:64", "classmix=0.5:-1", "classmix=0.5:1.5",
                "classmix=0.5:x", "classmix=0.5:", "classmix=x:1"):
        with pytest.raises(ValueError):
            A.from_spec(bad, (32, 48))
    with pytest.raises(ValueError):                                          # ... and the classes refuse what the spec refuses
        A.Compose([A.RandomCutMix(0.5), A.RandomCutMix(0.5)])
    with pytest.raises(ValueError):
        A.Compose([A.RandomClassMix(0.5), A.RandomClassMix(0.5, (1,))])
    for args in ((1.5,), (0.5, 0.0, 0.5), (0.5, 0.6, 0.5), (0.5, 0.5, 1.5), (float("nan"),)):
        with pytest.raises(ValueError):
            A.RandomCutMix(*args)
    for args in ((2.0,), (0.5, (64,)), (0.5, (-1,)), (0.5, (1.5,))):
        with pytest.raises(ValueError):
            A.RandomClassMix(*args)


# ------------------------------------------------------------------------------------------------ the tables
@pytest.mark.parametrize("n", [1, 2, 5])
def test_mixes_draws_boxes_partners_and_masks(n):
    """1000 tables of n rows at a 64 x 48 output (ow x oh), lo = 0.2, hi = 0.45.
    The area bound, from the formula: A = a.ow.oh with a in [lo, hi]; bw = clamp(round(sqrt(A.rho)), 1, ow), bh = clamp(round(A / bw),
    1, oh).  Where bh is not clamped |bh - A / bw| <= 1/2, so |bw.bh - A| <= bw / 2 <= ow / 2 and the share bw.bh / (ow.oh) lies in
    [lo - 1/(2 oh), hi + 1/(2 oh)].  Clamping bh to oh only lowers the area (upper bound kept); the box then has the full height and
    bw >= sqrt(A.rho) - 1/2 >= sqrt(lo.ow.oh / 2) - 1/2, which bounds the share from below by (sqrt(lo.ow.oh / 2) - 1/2) / ow.
    Clamping up to 1 does not happen here: A / bw >= lo.ow.oh / ow = lo.oh = 9.6."""
    A = _aug()
    ow, oh, lo, hi, skip, p = 64, 48, 0.2, 0.45, (0, 19, 40, 63), 0.3
    comp = A.Compose([A.RandomCutMix(p, lo, hi), A.RandomClassMix(p, skip)])
    sure = A.Compose([A.RandomCutMix(1.0, lo, hi), A.RandomClassMix(p, skip)])            # the other op at p = 1: the draw-count rule
    rng, rng_sure = np.random.RandomState(31 + n), np.random.RandomState(31 + n)
    fired_box = fired_cls = 0
    for _ in range(1000):
        table, classes = comp.mixes(rng, n, ow, oh)
        always, _ = sure.mixes(rng_sure, n, ow, oh)
        assert classes is True and table.dtype == np.int32 and table.shape == (n, 8) and not table[:, 7].any()
        for i in range(n):
            part, x0, y0, x1, y1 = (int(v) for v in table[i, :5])
            mask = (int(table[i, 6]) % 2 ** 32) << 32 | int(table[i, 5]) % 2 ** 32
            has_box, has_mask = (x0, y0, x1, y1) != (0, 0, 0, 0), mask != 0
            if n == 1:
                assert part == i and not has_box and not has_mask
                continue
            assert 0 <= part < n and (part != i) == (has_box or has_mask)             # (64 - 4 fair bits are never all zero here)
            fired_box, fired_cls = fired_box + has_box, fired_cls + has_mask
            assert not any(mask >> c & 1 for c in skip)
            # the class op's draws do not depend on whether the box op fired: the same mask in the p = 1 twin, where the box always is
            assert tuple(always[i, 1:5]) != (0, 0, 0, 0) and always[i, 0] != i
            if has_mask:
                assert tuple(always[i, 5:7]) == tuple(table[i, 5:7]) and always[i, 0] == part
            if has_box:
                assert tuple(always[i, 1:5]) == (x0, y0, x1, y1)
                bw, bh = x1 - x0, y1 - y0
                assert 0 <= x0 < x1 <= ow and 0 <= y0 < y1 <= oh
                share = bw * bh / float(ow * oh)
                assert share <= hi + 0.5 / oh
                assert share >= (lo - 0.5 / oh if bh < oh else (math.sqrt(lo * ow * oh / 2) - 0.5) / ow)
    if n == 5:
        # 5000 independent trials per op at p = 0.3: sigma = sqrt(5000 * 0.3 * 0.7) = 32.4.  A 4-sigma bound fails 6.3 times in 10^5 runs
        # of a fresh seed (two ops: 1.3 in 10^4, more than once), so the bound is 5 sigma (1.1 in 10^6) - and the seed is fixed anyway
        sigma = math.sqrt(5000 * p * (1 - p))
        assert abs(fired_box - 5000 * p) < 5 * sigma and abs(fired_cls - 5000 * p) < 5 * sigma
    # `classes` reflects the ops
    assert A.Compose([A.RandomCutMix(1.0)]).mixes(np.random.RandomState(1), 3, ow, oh)[1] is False
    assert A.Compose([A.RandomClassMix(1.0)]).mixes(np.random.RandomState(1), 3, ow, oh)[1] is True
    assert A.Compose([A.RandomHorizontallyFlip()]).mix_ops == []


def test_mix_draws_leave_the_other_three_streams_alone():
    A = _aug()
    assert len({0, A.COLOUR_SEED_OFFSET, A.ELASTIC_SEED_OFFSET, A.MIX_SEED_OFFSET}) == 4
    spec = "hflip,rotate=10,scale=0.5:2,brightness=0.4,contrast=0.3,elastic=6:16"
    plain = A.from_spec(spec, (24, 32), out_size=(24, 32))
    for with_mix in ("cutmix=1,classmix=1:0," + spec, spec + ",cutmix=1,classmix=1:0"):
        mixed = A.from_spec(with_mix, (24, 32), out_size=(24, 32))
        a, b = plain.matrices(np.random.RandomState(5), 6, 50, 40), mixed.matrices(np.random.RandomState(5), 6, 50, 40)
        assert np.array_equal(a, b)
        ta, tb = plain.colours(np.random.RandomState(505), 6, 3), mixed.colours(np.random.RandomState(505), 6, 3)
        assert np.array_equal(ta[0], tb[0]) and ta[1] == tb[1]
        fa, fb = plain.fields(np.random.RandomState(905), 6, 50, 40, a), mixed.fields(np.random.RandomState(905), 6, 50, 40, b)
        assert np.array_equal(fa[0], fb[0]) and fa[1] == fb[1]


# ------------------------------------------------------------------------------------------------ the host statement of the rule
def test_mix_batch_equals_the_reference_mask_rule():
    """A hand-made finished batch of 4 samples, 5 x 6, two channels: the chain 0 <- 1 <- 2, sample 3 with a partner outside the batch;
    classes up to 70 (>= 64: never pasted, although 64 and 70 alias the set bits 0 and 6 modulo 64) and a negative one."""
    A = _aug()
    rng = np.random.RandomState(3)
    img = rng.standard_normal((4, 2, 5, 6)).astype(np.float32)
    gt = rng.randint(0, 8, (4, 1, 5, 6)).astype(np.int64)
    gt[1, 0, 0, :3], gt[2, 0, 4, 3:] = (64, 70, -1), (63, 64, 6)
    mask = 1 | 1 << 6 | 1 << 63
    lo, hi = (int(np.array(w, dtype=np.uint32).view(np.int32)) for w in (mask & 0xFFFFFFFF, mask >> 32))
    table = np.array([[1, 1, 1, 4, 3, lo, hi, 0], [2, -2, 3, 2, 9, lo, hi, 0], [2, 0, 0, 6, 5, lo, hi, 0], [4, 0, 0, 6, 5, lo, hi, 0]], dtype=np.int32)
    for classes in (0, 1):
        pasted, partner = pasted_mask(table, classes, gt[:, 0], (5, 6))
        assert list(partner) == [1, 2, -1, -1] and pasted[:2].any() and not pasted[2:].any()
        want_img, want_gt = img.copy(), gt.copy()
        for n in (0, 1):
            want_img[n] = np.where(pasted[n][None], img[partner[n]], img[n])
            want_gt[n, 0] = np.where(pasted[n], gt[partner[n], 0], gt[n, 0])
        got_img, got_gt = A.mix_batch(img, gt, table, classes)
        assert np.array_equal(got_img, want_img) and np.array_equal(got_gt, want_gt) and got_gt.shape == gt.shape
        assert np.array_equal(A.mix_batch(torch.from_numpy(img), torch.from_numpy(gt[:, 0]), table, classes)[1], want_gt[:, 0])
    pasted, _ = pasted_mask(table, 1, gt[:, 0], (5, 6))
    assert not pasted[0, 0, :3].any()                    # sample 1's classes 64, 70, -1 at row 0, outside sample 0's box
    assert pasted[1, 4, 3] and not pasted[1, 4, 4] and pasted[1, 4, 5]               # sample 2's classes 63 (bit set), 64 (never), 6 (bit set)
    assert np.array_equal(want_gt[0, 0, 1:3, 1:4], gt[1, 0, 1:3, 1:4])                # the chain: sample 1's own pixels, not its mixed ones
    assert not np.array_equal(want_gt[1], gt[1])
    img_only, none = A.mix_batch(img, None, table, 0)
    assert none is None and np.array_equal(img_only, A.mix_batch(img, gt, table, 0)[0])
    with pytest.raises(ValueError):
        A.mix_batch(img, None, table, 1)


def test_gpu_case_conditions_hold_on_the_reference():
    """tests/test_augment_mix_gpu.py asserts on its expected outputs that both kinds of pixel exist on every mixed sample, that the
    class rule alone pastes somewhere, that fill pixels of a partner are pasted, that a class >= 64 never is and that chains do not
    propagate: all of that is the reference's, so it is checked here, where no GPU is needed."""
    from test_augment_mix_gpu import VARIANTS, case_one
    for c in (1, 3):
        for lut_name in ("cityscapes", "voc2012"):
            for variant in VARIANTS:
                assert len(case_one(c, lut_name, variant)[-1]) == 2


# ------------------------------------------------------------------------------------------------ scope
def test_the_per_sample_host_path_raises_with_a_mix_op():
    from PIL import Image
    A = _aug()
    img = Image.fromarray(np.zeros((8, 8, 3), dtype=np.uint8))
    for spec in ("hflip,cutmix=0.5", "classmix=0"):
        with pytest.raises(ValueError, match="device finish"):
            A.from_spec(spec, (8, 8), seed=1)(img, Image.fromarray(np.zeros((8, 8), dtype=np.uint8)))
    assert A.from_spec("hflip", (8, 8), seed=1)(img).size == (8, 8)


def test_build_loaders_give_the_mix_items_to_the_label_set_only(tmp_path):
    """DeviceLoader is built on a CPU device here: it draws and uploads on whatever device it is given and only its launches need the
    MI355X, so the Composes the three sets carry can be inspected without one."""
    from test_data_utils import _voc_tree
    from types import SimpleNamespace
    du, A = load_sub("data_utils"), _aug()
    root = str(tmp_path / "VOC2012")
    _voc_tree(root)
    spec = "hflip,cutmix=0.5,rotate=10,classmix=0.5:0,brightness=0.2"
    args = SimpleNamespace(dataset="voc2012", crop_height=32, crop_width=48, batch_size=2, augment=spec)
    with pytest.raises(ValueError, match="device finish"):                   # host mode: no path for a batch operation
        du.build_loaders(args, roots={"voc2012": root})
    lab, unl, val = du.build_loaders(args, roots={"voc2012": root}, device=torch.device("cpu"))
    assert [type(o).__name__ for o in lab.augmentation.mix_ops] == ["RandomCutMix", "RandomClassMix"] and lab.augmentation.mix_ops[1].skip == (0,)
    assert unl.augmentation.mix_ops == [] and val.augmentation is None
    assert [type(o).__name__ for o in unl.augmentation.ops] == ["RandomHorizontallyFlip", "RandomRotate", "RandomBrightness"]
    # everything else of the 'unlabel' set, and its draws, are those of the spec without the items
    args.augment = "hflip,rotate=10,brightness=0.2"
    lab2, unl2, _ = du.build_loaders(args, roots={"voc2012": root}, device=torch.device("cpu"))
    assert lab2.augmentation.mix_ops == [] and unl2.mix_rng.uniform() == unl.mix_rng.uniform()
    for a, b in ((unl, unl2), (lab, lab2)):
        assert np.array_equal(a.augmentation.matrices(a.rng, 4, 48, 32), b.augmentation.matrices(b.rng, 4, 48, 32))
        assert np.array_equal(a.augmentation.colours(a.colour_rng, 4, 3)[0], b.augmentation.colours(b.colour_rng, 4, 3)[0])
    assert lab.mix_rng.uniform() == np.random.RandomState(du.AUGMENT_SEED + A.MIX_SEED_OFFSET).uniform()
    args.augment = ""                                                        # and host mode without the items is what it was
    assert du.build_loaders(args, roots={"voc2012": root})[0].dataset.augmentation is None


def test_main_takes_the_items_and_checks_the_class_ids():
    import importlib
    import sys
    sys.path.insert(0, ROOT)
    main = importlib.import_module("main")
    assert main.get_args(["--augment", "hflip,classmix=0.5:0"]).augment == "hflip,classmix=0.5:0"
    assert main.get_args(["--augment", "cutmix=0.5,classmix=0.5:20", "--dataset", "voc2012"]).augment.endswith(":20")
    assert main.get_args(["--augment", "classmix=0.5:19", "--dataset", "cityscapes"]).dataset == "cityscapes"
    for argv in (["--augment", "classmix=0.5:21"], ["--augment", "hflip,classmix=0.5:0:21", "--dataset", "voc2012"],
                 ["--augment", "classmix=0.5:20", "--dataset", "cityscapes"], ["--augment", "classmix=0.5:4", "--dataset", "acdc"],
                 ["--augment", "classmix=0.5:x"]):
        with pytest.raises(SystemExit):
            main.get_args(argv)
    # without the items the parsed namespace is what it is without the flag's new items: nothing new is stored
    assert vars(main.get_args(["--augment", "hflip"])) == dict(vars(main.get_args([])), augment="hflip")
    assert "cutmix" not in " ".join(vars(main.get_args([])).keys()) and "classmix" not in " ".join(vars(main.get_args([])).keys())
    src = open(os.path.join(ROOT, "main.py")).read()
    assert "cutmix=<p>[:<lo>:<hi>]" in src and "classmix=<p>[:<id>[:<id>...]]" in src


# ------------------------------------------------------------------------------------------------ the C entry and the wrapper
def test_symbol_is_declared_exported_and_bound_and_the_abi_version_stays():
    L = load_sub("_lib")
    src = open(os.path.join(ROOT, "include", "sscg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint sscg_augment_mix_u8\s*\(", code)
    sig = L.SIGNATURES["sscg_augment_mix_u8"][1]
    elastic = L.SIGNATURES["sscg_augment_elastic_u8"][1]
    assert len(sig) == 26 and sig[:23] == elastic[:23] and sig[23:] == [C.c_void_p, C.c_int, C.c_void_p]
    assert L.lib.sscg_augment_mix_u8 is not None
    assert "#define SSCG_ABI_VERSION 18" in src and L.ABI_VERSION == 18 and L.lib.sscg_abi_version() == 18
    comment = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int sscg_augment_mix_u8", src, flags=re.S).group(1)
    assert "SSCG_ABI_VERSION stays 18" in comment and "mask_hi << 32" in comment and "where(pasted, plain[p], plain[n])" in comment
    kinds = dict(L.dev_tool("racecheck").parse_header(os.path.join(ROOT, "include", "sscg.h"))["sscg_augment_mix_u8"])
    assert kinds["mix"] == "r" and kinds["nodes"] == "r" and kinds["classes"] == "-" and kinds["out_img"] == "w" and kinds["stream"] == "stream"
    assert len(elastic) == 24 and len(L.SIGNATURES["sscg_augment_u8"][1]) == 17 and len(L.SIGNATURES["sscg_augment_colour_u8"][1]) == 20


def test_argument_errors_are_returned_before_any_hip_call():
    lib = load_sub("_lib").lib
    BAD_ARG, UNSUPPORTED = -1, -2
    one = C.c_void_p(16)                                                     # never dereferenced

    def call(img=one, gt=one, mats=one, out=one, out_gt=one, N=2, H=8, W=8, Cc=3, OH=8, OW=8, mean=one, std=one, lut=one, ifill=0, lfill=0,
             colour=one, need_mean=0, ws=one, nodes=one, grid=4, GH=5, GW=5, mix=one, classes=1):
        return lib.sscg_augment_mix_u8(img, gt, mats, out, out_gt, N, H, W, Cc, OH, OW, mean, std, lut, ifill, lfill, colour, need_mean, ws,
                                       nodes, grid, GH, GW, mix, classes, None)
    # its own
    assert call(mix=None) == BAD_ARG
    assert call(gt=None, lut=None, out_gt=None, classes=1) == BAD_ARG and call(gt=None, lut=None, out_gt=None, classes=-1) == BAD_ARG
    # with a lattice the lattice's rules; without one grid, GH and GW are ignored (the calls below then fail on something later: C)
    assert call(grid=3, GH=6, GW=6) == BAD_ARG and call(grid=0) == BAD_ARG and call(GH=4) == BAD_ARG and call(GW=6) == BAD_ARG
    assert call(nodes=None, grid=0, GH=-1, GW=99, Cc=2) == UNSUPPORTED
    # every SSCG_ERR_BAD_ARG case of sscg_augment_u8 and of the colour entry
    for null in ("img", "mats", "out", "mean", "std"):
        assert call(**{null: None}) == BAD_ARG, null
    assert call(Cc=0) == BAD_ARG and call(Cc=5) == BAD_ARG
    for size in ("N", "H", "W", "OH", "OW"):
        assert call(**{size: 0}) == BAD_ARG and call(**{size: -3}) == BAD_ARG, size
    assert call(ifill=256) == BAD_ARG and call(ifill=-1) == BAD_ARG and call(lfill=256) == BAD_ARG and call(lfill=-1) == BAD_ARG
    assert call(lut=None) == BAD_ARG and call(out_gt=None) == BAD_ARG and call(gt=None, lut=None, classes=0) == BAD_ARG
    assert call(need_mean=1, ws=None) == BAD_ARG and call(need_mean=1, ws=C.c_void_p(20)) == BAD_ARG
    # unsupported: C of 2 or 4 with or without a colour table, the size limits
    for colour in (one, None):
        assert call(Cc=2, colour=colour) == UNSUPPORTED and call(Cc=4, colour=colour) == UNSUPPORTED
    assert call(Cc=2, mix=None) == BAD_ARG                                   # a bad argument is reported first
    assert call(N=2, OH=32768, OW=32768, GH=8195, GW=8195) == UNSUPPORTED    # N * OH * OW = 2^31
    assert call(H=32768) == UNSUPPORTED and call(W=32768) == UNSUPPORTED
    assert call(N=65536, OH=1, OW=1, GH=4, GW=4, need_mean=1) == UNSUPPORTED
    assert call(grid=2 ** 22 + 1, GH=4, GW=4) == UNSUPPORTED


def test_wrapper_refuses_cpu_tensors_and_wrong_tables():
    F, L = load_sub("functional"), load_sub("_lib")
    img, mats = torch.zeros(2, 4, 4, 3, dtype=torch.uint8), torch.zeros(2, 6, dtype=torch.int32)
    with pytest.raises(L.SscgError):
        F.augment_batch(img, None, mats, (4, 4), torch.zeros(3), torch.ones(3), None, mix=(torch.zeros(2, 8, dtype=torch.int32), 0))

    class OnDevice:                                                          # stand-ins that claim to be on the device
        def __init__(self, t):
            self.t = t
            self.is_cuda, self.dtype, self.shape = True, t.dtype, t.shape

        def dim(self):
            return self.t.dim()
    for bad in (torch.zeros(2, 8, dtype=torch.int32), np.zeros((2, 8), dtype=np.int32)):
        with pytest.raises(L.SscgError, match="mix table"):
            F.augment_batch(OnDevice(img), None, OnDevice(mats), (4, 4), torch.zeros(3), torch.ones(3), None, mix=(bad, 0))
