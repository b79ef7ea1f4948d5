"""Sliding-window inference (sscg_window_gather / sscg_predict_head_sw, `--sliding`) on a GPU-less host: the window geometry and the
weight / normalisation tables against their definition (restated in tests/sliding_reference.py), the option parser and the driver's
refusals, the two entries' declarations and argument errors (returned before any HIP call), and the loaders' evaluation size."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sliding_reference as R
from conftest import ROOT, load_sub

BAD_ARG, UNSUPPORTED = -1, -2
ONE = C.c_void_p(16)          # never dereferenced
EPS = float(np.finfo(np.float32).eps)

TABLE = [((23, 12, 0.5), [0, 6, 11]), ((29, 16, 0.5), [0, 8, 13]), ((29, 16, 0.75), [0, 4, 8, 12, 13]), ((23, 12, 0.0), [0, 11]),
         ((97, 65, 0.5), [0, 32]), ((113, 65, 0.5), [0, 33, 48]), ((12, 12, 0.0), [0]), ((12, 12, 0.5), [0]), ((12, 12, 0.75), [0])]


def test_window_positions_are_the_documented_ones():
    F = load_sub("functional")
    for (L, w, ov), want in TABLE:
        assert F.sliding_positions(L, w, ov) == want, (L, w, ov)
        assert R.positions(L, w, ov)[0] == want, (L, w, ov)
    for L in range(12, 80):
        for w in (12, 7, 1):
            for ov in (0.0, 0.25, 0.5, 0.6, 0.75):
                pos = F.sliding_positions(L, w, ov)
                assert pos == R.positions(L, w, ov)[0]
                assert pos[0] == 0 and pos[-1] == L - w and pos == sorted(pos) and len(set(pos)) == len(pos)
    with pytest.raises(ValueError):
        F.sliding_positions(11, 12, 0.5)


def test_every_pixel_is_covered_and_at_most_five_times_per_axis():
    F = load_sub("functional")
    for L in list(range(12, 120)) + [256, 1024, 2048]:
        for w in (12, 16, 65):
            if w > L:
                continue
            for ov in (0.0, 0.5, 0.75):
                pos = F.sliding_positions(L, w, ov)
                _, cnt = R.coverage(L, w, pos, np.ones(w))
                assert cnt.min() >= 1, (L, w, ov)
                assert cnt.max() <= 5, (L, w, ov, int(cnt.max()))


def _plan(size, window, **kw):
    F = load_sub("functional")
    return F.sliding_plan(size[0], size[1], F.SlidingOptions(window, size, **kw))


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("case", [((23, 29), (12, 16), 0.5), ((23, 29), (12, 16), 0.75), ((97, 113), (65, 65), 0.5), ((512, 1024), (256, 512), 0.5),
                                  ((12, 16), (12, 16), 0.5)])
def test_tables_follow_their_definition(case, flip):
    size, window, ov = case
    for blend in ("gauss", "const"):
        p = _plan(size, window, overlap=ov, blend=blend, flip=flip)
        assert (p.OH, p.OW, p.wh, p.ww) == size + window and p.views == p.ky * p.kx * (2 if flip else 1)
        assert (p.sy, p.sx) == (R.positions(size[0], window[0], ov)[1], R.positions(size[1], window[1], ov)[1])
        for wt, r, L, w, pos, half in ((p.wy, p.ry, size[0], window[0], p.pos_y, flip), (p.wx, p.rx, size[1], window[1], p.pos_x, False)):
            assert wt.dtype == np.float32 and r.dtype == np.float32 and wt.shape == (w,) and r.shape == (L,)
            assert pos == R.positions(L, w, ov)[0]
            assert np.array_equal(wt, R.weights(w, blend, p.options.sigma).astype(np.float32))          # float64, rounded once
            assert np.array_equal(wt, wt[::-1])                                                          # symmetric bit for bit
            cov = np.zeros(L, dtype=np.float32)
            for q in pos:                                                                                # fp32, ascending window order
                cov[q:q + w] += wt
            target = np.float32(0.5 if half else 1.0)
            assert np.array_equal(r, (np.float32(1) / cov) * target)
            assert float(np.abs(r * cov - target).max()) <= 2 * EPS * float(target), (blend, float(np.abs(r * cov - target).max()))
            cov64, _ = R.coverage(L, w, pos, R.weights(w, blend, p.options.sigma))
            assert float(np.abs(r.astype(np.float64) * cov64 / float(target) - 1).max()) < 1e-6


def test_const_blend_without_overlap_on_whole_windows_needs_no_normalising():
    p = _plan((36, 64), (12, 16), overlap=0.0, blend="const")
    assert (p.ky, p.kx) == (3, 4) and bool((p.ry == 1).all()) and bool((p.rx == 1).all()) and bool((p.wy == 1).all())
    F = load_sub("functional")
    assert F.sliding_plan(36, 64, F.SlidingOptions((12, 16), (36, 64), overlap=0.0, blend="const")) is p          # cached


def test_parse_sliding():
    U, F = load_sub("utils"), load_sub("functional")
    assert U.parse_sliding("", (12, 16)) is None and U.parse_sliding(None, (12, 16)) is None
    on = U.parse_sliding("on", (256, 512))
    assert on == F.SlidingOptions((256, 512), (512, 1024), overlap=0.5, blend="gauss", sigma=0.125, flip=False)
    assert "untuned" in U.parse_sliding.__doc__
    assert U.parse_sliding("size=23x29", (12, 16)).size == (23, 29)
    assert U.parse_sliding("scale=1.5", (65, 65)).size == (98, 98)                     # 97.5 rounds half up
    assert U.parse_sliding("scale=1", (12, 16)).size == (12, 16)
    o = U.parse_sliding("size=23x29, overlap=0.75,blend=const,sigma=0.25,flip", (12, 16))
    assert (o.window, o.size, o.overlap, o.blend, o.sigma, o.flip) == ((12, 16), (23, 29), 0.75, "const", 0.25, True)
    bad = {"size=11x29": "size=11x29", "size=23x15": "below", "scale=0.5": "below", "scale=2,overlap=0.8": "0.8", "scale=2,overlap=-0.1": "-0.1",
           "scale=40,overlap=0.75": "at most 16", "scale=2,scale=3": "scale=3", "scale=2,overlap=0.5,overlap=0.5": "overlap=0.5",
           "size=30x30,scale=2": "once", "overlap=0.5": "once", "scale=2,foo=1": "foo=1", "scale=2,flip=1": "flip=1", "scale=2,overlap": "overlap",
           "size=23": "size=23", "scale=x": "scale=x", "scale=2,blend=linear": "linear", "scale=2,sigma=0": "sigma", "scale=2,sigma=1.5": "sigma",
           "scale=2,,flip": "''"}
    for spec, names in bad.items():
        with pytest.raises(ValueError) as e:
            U.parse_sliding(spec, (12, 16))
        assert str(e.value).startswith("--sliding") and names in str(e.value), (spec, str(e.value))
    with pytest.raises(ValueError):
        F.SlidingOptions((12, 16), (12 + 16 * 3, 16), overlap=0.75)                    # 17 windows along H
    assert len(F.sliding_positions(12 + 15 * 3, 12, 0.75)) == 16


def test_main_refuses_what_sliding_does_not_combine_with():
    sys.path.insert(0, ROOT)
    import main
    a = main.get_args([])
    assert a.sliding == "" and "sliding" not in vars(a)                                # no other default moved: nothing is stored
    assert main.get_args(["--sliding", "on"]).sliding == "on"
    assert "--sliding" in main.__doc__
    for argv, names in ((["--sliding", "on", "--tta", "0.5,1.0"], "--tta"), (["--sliding", "on", "--panels", "out"], "--panels"),
                        (["--sliding", "on", "--calibration", "fit"], "temperature"),
                        (["--sliding", "on", "--calibration", "temps=0.5/2"], "temperature"),
                        (["--sliding", "size=100x100"], "below"), (["--sliding", "scale=2,overlap=0.8"], "0.8")):
        with pytest.raises(ValueError) as e:
            main.main(argv)
        assert "--sliding" in str(e.value) and names in str(e.value), (argv, str(e.value))
    ok = main.get_args(["--sliding", "scale=1.5,flip", "--calibration", "on", "--crf", "on", "--components", "on", "--boundary", "on"])
    ok.crop_height, ok.crop_width = 320, 320
    assert main.check_sliding(ok).size == (480, 480) and main.check_sliding(ok).flip
    off = main.get_args(["--tta", "0.5,1.0"])
    off.crop_height, off.crop_width = 320, 320
    assert main.check_sliding(off) is None


def test_both_entries_are_declared_bound_and_the_abi_stays():
    L = load_sub("_lib")
    hdr = open(os.path.join(ROOT, "include", "sscg.h")).read()
    assert ("int sscg_window_gather(const float* x, float* y, int N, int H, int W, int C, int wh, int ww, int sy, int sx, int ky, int kx, "
            "int flip,") in hdr
    assert "int sscg_predict_head_sw(const float* x, int N, int h, int w, int C, int wh, int ww, int sy, int sx, int ky, int kx, int flip, int OH," in hdr
    block = hdr[hdr.index("sliding-window inference:"):hdr.index("int sscg_window_gather(")]
    assert "SSCG_ABI_VERSION stays 18" in " ".join(block.replace(" * ", " ").split())
    assert len(L.SIGNATURES["sscg_window_gather"][1]) == 14 and len(L.SIGNATURES["sscg_predict_head_sw"][1]) == 24
    assert callable(L.lib.sscg_window_gather) and callable(L.lib.sscg_predict_head_sw)
    assert L.ABI_VERSION == 18 and L.lib.sscg_abi_version() == 18 and "#define SSCG_ABI_VERSION 18" in hdr
    rc = L.dev_tool("racecheck")
    row = dict(rc.parse_header(os.path.join(ROOT, "include", "sscg.h"))["sscg_predict_head_sw"])
    assert all(row[k] == "r" for k in ("x", "wy", "wx", "ry", "rx", "label_true"))      # the tables are device reads
    assert all(row[k] == "w" for k in ("prob", "index", "label_u8", "hist")) and row["stream"] == "stream"


def test_head_argument_errors_are_returned_before_any_launch():
    lib = load_sub("_lib").lib

    def call(x=ONE, N=2, h=5, w=7, Cn=21, wh=12, ww=16, sy=6, sx=8, ky=3, kx=3, flip=0, OH=23, OW=29, wy=ONE, wx=ONE, ry=ONE, rx=ONE,
             prob=None, index=ONE, u8=None, lt=None, hist=None):
        return lib.sscg_predict_head_sw(x, N, h, w, Cn, wh, ww, sy, sx, ky, kx, flip, OH, OW, wy, wx, ry, rx, prob, index, u8, lt, hist, None)

    assert call(x=None) == BAD_ARG
    assert call(wy=None) == BAD_ARG and call(wx=None) == BAD_ARG and call(ry=None) == BAD_ARG and call(rx=None) == BAD_ARG
    assert call(N=0) == BAD_ARG and call(h=0) == BAD_ARG and call(w=-1) == BAD_ARG and call(Cn=0) == BAD_ARG and call(Cn=65) == BAD_ARG
    assert call(wh=0) == BAD_ARG and call(sy=0) == BAD_ARG and call(sx=-2) == BAD_ARG and call(ky=0) == BAD_ARG and call(OW=0) == BAD_ARG
    assert call(wh=24) == BAD_ARG and call(ww=30) == BAD_ARG                       # the window is larger than the output
    assert call(ky=2) == BAD_ARG and call(kx=2) == BAD_ARG                         # (k - 1) * s < L - w: the windows leave a gap
    assert call(sy=5) == BAD_ARG                                                   # 2 * 5 < 23 - 12
    assert call(hist=ONE) == BAD_ARG and call(lt=ONE) == BAD_ARG                   # hist without label_true and the reverse
    assert call(index=None) == BAD_ARG                                             # no output asked for
    # 2^31 output pixels; 2^31 elements of prob
    assert call(N=2, OH=32768, OW=32768, wh=16384, ww=16384, sy=16384, sx=16384, ky=2, kx=2) == UNSUPPORTED
    assert call(N=1, Cn=64, OH=8192, OW=4096, wh=4096, ww=4096, sy=4096, sx=4096, ky=2, kx=1, prob=ONE) == UNSUPPORTED


def test_gather_argument_errors_are_returned_before_any_launch():
    lib = load_sub("_lib").lib

    def call(x=ONE, y=ONE, N=2, H=23, W=29, Cn=3, wh=12, ww=16, sy=6, sx=8, ky=3, kx=3, flip=1):
        return lib.sscg_window_gather(x, y, N, H, W, Cn, wh, ww, sy, sx, ky, kx, flip, None)

    assert call(x=None) == BAD_ARG and call(y=None) == BAD_ARG
    assert call(N=0) == BAD_ARG and call(H=0) == BAD_ARG and call(Cn=0) == BAD_ARG and call(ww=0) == BAD_ARG and call(sx=0) == BAD_ARG
    assert call(wh=24) == BAD_ARG and call(ww=30) == BAD_ARG and call(ky=2) == BAD_ARG and call(kx=1) == BAD_ARG
    assert call(N=1 << 22, H=12 + 15 * 64, W=16 + 15 * 64, sy=64, sx=64, ky=16, kx=16) == UNSUPPORTED       # 2^31 windows


def test_wrappers_refuse_cpu_tensors_and_foreign_plans():
    F, L, U = load_sub("functional"), load_sub("_lib"), load_sub("utils")
    p = _plan((23, 29), (12, 16))
    with pytest.raises(L.SscgError):
        F.window_gather(torch.zeros(1, 3, 23, 29), p)
    with pytest.raises(L.SscgError):
        F.predict_labels_sw(torch.zeros(9, 4, 5, 7), p)
    with pytest.raises(TypeError):
        F.sliding_plan(23, 29, "on")
    with pytest.raises(ValueError):
        F.sliding_plan(11, 29, F.SlidingOptions((12, 16), (23, 29)))                 # images below the window
    assert isinstance(F.FUSE_SLIDING[0], bool)
    assert callable(getattr(U.runningScore, "update_logits_sw")) and callable(U.sliding_logits)
    import inspect
    md = load_sub("model")
    for cls in (md.semisuper_cycleGAN, md.supervised_model):          # the option is state of the model: evaluate() keeps its parameters
        assert list(inspect.signature(cls.evaluate).parameters) == ["self", "val_loader", "first_batch", "tta", "crf", "boundary"]
        assert list(inspect.signature(cls.set_sliding).parameters) == ["self", "opts"] and callable(cls.get_sliding)
    assert "sliding" in inspect.signature(U.crf_scores).parameters


def test_the_loaders_keep_the_validation_set_at_the_evaluation_size(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from data_trees import data_trees
    du = load_sub("data_utils")
    roots = data_trees(str(tmp_path))
    for dataset, ch in (("voc2012", 3), ("acdc", 1)):
        args = SimpleNamespace(dataset=dataset, crop_height=12, crop_width=16, batch_size=2, sliding="size=23x29,overlap=0.5")
        lab, unl, val = du.build_loaders(args, roots=roots)
        img, gt, _ = next(iter(val))
        assert tuple(img.shape) == (2, ch, 23, 29) and tuple(gt.shape) == (2, 1, 23, 29)
        img, gt, _ = next(iter(lab))
        assert tuple(img.shape) == (2, ch, 12, 16) and tuple(gt.shape) == (2, 1, 12, 16)
        assert tuple(next(iter(unl))[0].shape) == (2, ch, 12, 16)
        (test,) = du.build_loaders(args, roots=roots, sets=("test",))
        assert tuple(next(iter(test))[0].shape) == (2, ch, 23, 29)
        args.sliding = ""
        val = du.build_loaders(args, roots=roots)[2]
        assert tuple(next(iter(val))[0].shape) == (2, ch, 12, 16)                      # off: the crop, as before
