"""Contour scores of the evaluation (sscg_boundary_counts, `--boundary`) on a GPU-less host: the numpy restatement the GPU test is pinned
to (tests/boundary_reference.py) against the erosion form of the published Boundary IoU and against cases worked by hand; the spec
parser, the options object and the score arithmetic; the entry is exported, declared and bound and returns every argument error before
any HIP call; the drivers take the option and the command line moves no other default."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import boundary_reference as R
from conftest import ROOT, load_sub

BAD_ARG, UNSUPPORTED = -1, -2
ONE = C.c_void_p(16)          # never dereferenced


# ------------------------------------------------------------------------------------------ the restatement itself
def _erosion_counts(gt, pred, Cn, d):
    """bt, bp, bi by the published implementation's form: mask & ~erode(mask padded with zeros, 3x3, d times), per class and image."""
    nd = pytest.importorskip("scipy.ndimage")
    bt, bp, bi = (np.zeros(Cn, dtype=np.int64) for _ in range(3))

    def contour(mask):
        padded = np.pad(mask, d + 1)
        return mask & ~nd.binary_erosion(padded, structure=np.ones((3, 3), dtype=bool), iterations=d)[d + 1:-d - 1, d + 1:-d - 1]

    for n in range(gt.shape[0]):
        for c in range(Cn):
            g, p = contour(gt[n] == c), contour(pred[n] == c)
            bt[c] += g.sum()
            bp[c] += p.sum()
            bi[c] += (g & p).sum()
    return bt, bp, bi


@pytest.mark.parametrize("shape", [(37, 53), (70, 45), (33, 33), (5, 9)])
@pytest.mark.parametrize("Cn", [4, 21, 64])
def test_window_form_equals_the_erosion_form_on_void_free_maps(shape, Cn):
    gt, pred = R.make_case(shape[0] + Cn, 2, shape[0], shape[1], Cn, void=False)
    for d in (1, 2, 3, 7, 8):
        bt, bp, bi, _ = R.split(R.counts(gt, pred, Cn, d), Cn)
        want = _erosion_counts(gt, pred, Cn, d)
        assert np.array_equal(bt, want[0]) and np.array_equal(bp, want[1]) and np.array_equal(bi, want[2]), (shape, Cn, d)
        assert 0 < bi.sum() < min(bt.sum(), bp.sum())          # the prediction is neither the ground truth nor unrelated to it


def test_uniform_map_counts_the_border_ring_only():
    gt = np.full((1, 5, 5), 1)
    bt, bp, bi, tri = R.split(R.counts(gt, gt.astype(np.uint8), 3, 1), 3)
    assert bt.tolist() == [0, 16, 0] and bp.tolist() == [0, 16, 0] and bi.tolist() == [0, 16, 0] and not tri.any()
    # at d = 2 only the centre pixel's window stays inside; from d = 3 on every window leaves the image
    assert R.split(R.counts(gt, gt.astype(np.uint8), 3, 2), 3)[0].tolist() == [0, 24, 0]
    assert R.split(R.counts(gt, gt.astype(np.uint8), 3, 3), 3)[0].tolist() == [0, 25, 0]
    assert not R.split(R.counts(gt, gt.astype(np.uint8), 3, 32), 3)[3].any()


def test_one_vertical_label_change_at_width_one():
    gt = np.zeros((1, 5, 5), dtype=np.int64)
    gt[:, :, 2:] = 1                                            # columns 0-1 are class 0, columns 2-4 class 1
    bt, bp, bi, tri = R.split(R.counts(gt, gt.astype(np.uint8), 2, 1), 2)
    # E_t: the ring (16) and, inside it, columns 1 and 2 (rows 1-3): every pixel but (1..3, 3)
    assert bt.tolist() == [10, 12] and bp.tolist() == [10, 12] and bi.tolist() == [10, 12]
    # the band: columns 1 and 2 in all five rows - the border alone adds nothing
    assert tri.tolist() == [[5, 0], [0, 5]]
    # a prediction that puts the change one column further right: its contour is columns 2 and 3
    pred = np.zeros((1, 5, 5), dtype=np.uint8)
    pred[:, :, 3:] = 1
    bt, bp, bi, tri = R.split(R.counts(gt, pred, 2, 1), 2)
    assert bt.tolist() == [10, 12] and bp.tolist() == [12, 10]          # E_r: every pixel but (1..3, 1)
    assert bi.tolist() == [7, 7]                   # t = r = 0: column 0 and (0, 1), (4, 1); t = r = 1: column 4 and (0, 3), (4, 3)
    assert tri.tolist() == [[5, 0], [5, 0]]        # band columns 1 (t = 0, r = 0) and 2 (t = 1, r = 0)


def test_a_void_column_is_a_label_but_is_counted_nowhere():
    gt = np.zeros((1, 5, 5), dtype=np.int64)
    gt[:, :, 2] = 255
    pred = np.zeros((1, 5, 5), dtype=np.uint8)
    for void in (255, -1, 2, 1 << 40):
        gt[:, :, 2] = void
        bt, bp, bi, tri = R.split(R.counts(gt, pred, 2, 1), 2)
        assert bt.tolist() == [20, 0]                  # every valid pixel: columns 0 and 4 are ring, 1 and 3 touch the void column
        assert bp.tolist() == [14, 0]                  # the prediction is uniform: the ring, less the void column's two ring pixels
        assert bi.tolist() == [14, 0]
        assert tri.tolist() == [[10, 0], [0, 0]]       # the band: columns 1 and 3


def test_prediction_equal_to_ground_truth_scores_one():
    U = load_sub("utils")
    gt, _ = R.make_case(5, 2, 37, 53, 4, seeds=8, void=False)
    v = R.counts(gt, gt.astype(np.uint8), 4, 3)
    bt, bp, bi, tri = R.split(v, 4)
    assert np.array_equal(bt, bi) and np.array_equal(bp, bi) and (bt > 0).all()
    assert np.array_equal(tri, np.diag(np.diag(tri))) and (np.diag(tri) > 0).all()
    s = U.boundary_scores(v, 4, "voc2012")                     # VOC drops class 0
    assert s["boundary_iou"] == 1.0 and s["trimap_iou"] == 1.0 and list(s["class_boundary_iou"].values()) == [1.0, 1.0, 1.0]


def test_predicted_values_at_or_above_the_class_count_are_compared_but_not_counted():
    gt = np.zeros((1, 5, 5), dtype=np.int64)
    pred = np.zeros((1, 5, 5), dtype=np.uint8)
    pred[:, 2, 2] = 200
    bt, bp, bi, tri = R.split(R.counts(gt, pred, 2, 1), 2)
    # in_r holds in the whole 3x3 interior, so E_r is every pixel; the centre's own r = 200 is in no bin
    assert bt.tolist() == [16, 0] and bp.tolist() == [24, 0] and bi.tolist() == [16, 0] and not tri.any()


def test_reference_cases_keep_both_paths_alive():
    for (h, w, d) in ((37, 53, 1), (37, 53, 7), (70, 45, 3), (97, 131, 32)):
        gt, _ = R.make_case(1, 1, h, w, 4, seeds=3 if d < 32 else 0)
        assert 0.1 <= R.edge_share(gt, 4, d) <= 0.9, (h, w, d)
    assert R.width(256, 256, 0.02) == 7 and R.width(256, 512, 0.02) == 11 and R.width(512, 1024, 0.02) == 23


# ------------------------------------------------------------------------------------------ options, parser, scores
def test_boundary_options_and_the_width_rule():
    F = load_sub("functional")
    o = F.BoundaryOptions()
    assert o.d is None and o.ratio == 0.02
    assert (o.width(256, 256), o.width(256, 512), o.width(512, 1024)) == (7, 11, 23)
    assert o.width(5, 9) == 1 and F.BoundaryOptions(ratio=1.0).width(3, 4) == 5
    assert F.BoundaryOptions(d=3).width(512, 1024) == 3 and F.BoundaryOptions(d=32).width(2, 2) == 32 and F.BoundaryOptions(d=4.0).d == 4
    assert F.BoundaryOptions(d=3) == F.BoundaryOptions(d=3) and F.BoundaryOptions(d=3) != F.BoundaryOptions(d=4)
    assert F.BoundaryOptions() == F.BoundaryOptions(ratio=0.02)
    with pytest.raises(ValueError) as e:
        o.width(1024, 2048)                                    # 0.02 of that diagonal is 46
    assert "46" in str(e.value)
    for bad in (dict(d=3, ratio=0.02), dict(d=0), dict(d=-1), dict(d=33), dict(d=1.5), dict(d="3"), dict(d=True), dict(d=float("nan")),
                dict(ratio=0), dict(ratio=-0.1), dict(ratio=1.5), dict(ratio=float("nan")), dict(ratio="x"), dict(ratio=True)):
        with pytest.raises(ValueError):
            F.BoundaryOptions(**bad)


def test_parse_boundary_table():
    F, U = load_sub("functional"), load_sub("utils")
    assert U.parse_boundary("") is None and U.parse_boundary(None) is None and U.parse_boundary("  ") is None
    assert U.parse_boundary("on") == F.BoundaryOptions() and U.parse_boundary(" on ") == F.BoundaryOptions()
    assert U.parse_boundary("d=3") == F.BoundaryOptions(d=3) and U.parse_boundary("d=32").d == 32
    assert U.parse_boundary("ratio=0.05") == F.BoundaryOptions(ratio=0.05) and U.parse_boundary("ratio=1").ratio == 1.0
    for spec in ("off", "d", "d=", "d=x", "d=1.5", "d=0", "d=33", "d=-2", "ratio=0", "ratio=2", "ratio=nan", "ratio=x", "width=3",
                 "d=3,ratio=0.02", "D=3", "=3", "on,d=3"):
        with pytest.raises(ValueError) as e:
            U.parse_boundary(spec)
        assert repr(spec) in str(e.value) and "--boundary" in str(e.value), (spec, str(e.value))


def test_boundary_scores_arithmetic_nan_classes_and_class_dropping():
    U = load_sub("utils")
    Cn = 4
    bt, bp, bi = np.array([10, 8, 0, 6]), np.array([12, 8, 0, 2]), np.array([6, 8, 0, 0])
    tri = np.array([[5, 1, 0, 0], [2, 6, 0, 0], [0, 0, 0, 0], [1, 0, 0, 3]])
    v = np.concatenate([bt, bp, bi, tri.reshape(-1)])
    s = U.boundary_scores(v, Cn, "acdc")
    assert set(s) == {"boundary_iou", "class_boundary_iou", "trimap_iou", "class_trimap_iou"}
    b = s["class_boundary_iou"]
    assert b[0] == 6 / 16 and b[1] == 1.0 and np.isnan(b[2]) and b[3] == 0.0
    assert abs(s["boundary_iou"] - (6 / 16 + 1.0 + 0.0) / 3) < 1e-15          # the NaN class is left out of the mean
    t = s["class_trimap_iou"]
    assert t[0] == 5 / (6 + 8 - 5) and t[1] == 6 / (8 + 7 - 6) and np.isnan(t[2]) and t[3] == 3 / (4 + 3 - 3)
    assert abs(s["trimap_iou"] - (5 / 9 + 6 / 9 + 3 / 4) / 3) < 1e-15
    # the trimap arithmetic IS get_scores()'s, class dropping included: the same matrix through runningScore
    for dataset in ("voc2012", "cityscapes", "acdc"):
        rs = U.runningScore(Cn, dataset)
        rs.confusion_matrix = tri.astype(np.float64)
        score, cls = rs.get_scores()
        s = U.boundary_scores(v, Cn, dataset)
        assert s["trimap_iou"] == score["Mean IoU : \t"] and len(s["class_trimap_iou"]) == len(cls) == (4 if dataset == "acdc" else 3)
        assert all(s["class_trimap_iou"][k] == cls[k] or (np.isnan(cls[k]) and np.isnan(s["class_trimap_iou"][k])) for k in cls)
    voc, city = U.boundary_scores(v, Cn, "voc2012"), U.boundary_scores(v, Cn, "cityscapes")
    assert list(voc["class_boundary_iou"].values())[0] == 1.0 and abs(voc["boundary_iou"] - 0.5) < 1e-15          # classes 1..3
    assert list(city["class_boundary_iou"].values())[0] == 6 / 16 and abs(city["boundary_iou"] - (6 / 16 + 1) / 2) < 1e-15
    empty = U.boundary_scores(np.zeros(3 * Cn + Cn * Cn, dtype=np.int64), Cn, "acdc")
    assert np.isnan(empty["boundary_iou"]) and np.isnan(empty["trimap_iou"])
    with pytest.raises(ValueError):
        U.boundary_scores(v[:-1], Cn, "acdc")


def test_running_score_holds_the_option_as_state():
    F, U = load_sub("functional"), load_sub("utils")
    rs = U.runningScore(4, "acdc")
    assert rs.get_boundary() is None and rs.get_boundary_scores() is None
    rs.set_boundary(F.BoundaryOptions(d=3))
    assert rs.get_boundary() == F.BoundaryOptions(d=3)
    s = rs.get_boundary_scores()                               # nothing counted yet: every class is empty
    assert np.isnan(s["boundary_iou"]) and len(s["class_boundary_iou"]) == 4
    rs.set_boundary(5)
    assert rs.get_boundary() == F.BoundaryOptions(d=5)
    rs.reset()
    assert rs.get_boundary() == F.BoundaryOptions(d=5)         # reset() clears counts, not the option
    rs.set_boundary(None)
    assert rs.get_boundary() is None and rs.get_boundary_scores() is None
    # the host path (numpy label maps) is as it was: the option is not in its way
    rs.update([np.array([[0, 1], [2, 255]])], [np.array([[0, 1], [1, 3]])])
    assert rs.confusion_matrix.sum() == 3


# ------------------------------------------------------------------------------------------ the entry, the wrapper, the drivers
def test_entry_is_exported_declared_and_bound():
    L = load_sub("_lib")
    hdr = open(os.path.join(ROOT, "include", "sscg.h")).read()
    assert "int sscg_boundary_counts(const int64_t* label_true, const uint8_t* label_pred, int N, int H, int W, int C, int d, int64_t* counts," in hdr
    assert "utils.py:357-412" in hdr[hdr.index("contour scores of the evaluation"):hdr.index("int sscg_boundary_counts(")]
    assert len(L.SIGNATURES["sscg_boundary_counts"][1]) == 9 and callable(L.lib.sscg_boundary_counts)
    assert L.ABI_VERSION == 18 and L.lib.sscg_abi_version() == 18 and "#define SSCG_ABI_VERSION 18" in hdr          # an addition
    assert "boundary.hip" in open(os.path.join(ROOT, "semi-supervised-segmentation-cyclegan_amd", "csrc", "Makefile")).read()


def test_argument_errors_are_returned_before_any_launch():
    lib = load_sub("_lib").lib

    def call(lt=ONE, lp=ONE, N=1, H=5, W=5, Cn=4, d=1, counts=ONE):
        return lib.sscg_boundary_counts(lt, lp, N, H, W, Cn, d, counts, None)

    assert call(lt=None) == BAD_ARG and call(lp=None) == BAD_ARG and call(counts=None) == BAD_ARG
    assert call(d=0) == BAD_ARG and call(d=33) == BAD_ARG and call(d=-1) == BAD_ARG
    assert call(Cn=0) == BAD_ARG and call(Cn=65) == BAD_ARG and call(Cn=-4) == BAD_ARG
    for size in ("N", "H", "W"):
        assert call(**{size: 0}) == BAD_ARG and call(**{size: -3}) == BAD_ARG, size
    assert call(N=2, H=32768, W=32768) == UNSUPPORTED and call(N=1, H=1 << 16, W=1 << 15) == UNSUPPORTED          # N*H*W >= 2^31
    assert call(N=1 << 30, H=1 << 30, W=1 << 30) == UNSUPPORTED                                                    # and no overflow on the way
    assert call(N=2, H=32768, W=32768, d=0) == BAD_ARG                                                             # the argument errors come first


def test_wrapper_refuses_cpu_tensors_bad_widths_and_the_drivers_take_the_option():
    F, L, U, md = load_sub("functional"), load_sub("_lib"), load_sub("utils"), load_sub("model")
    lt, lp = torch.zeros(1, 5, 5, dtype=torch.int64), torch.zeros(1, 5, 5, dtype=torch.uint8)
    with pytest.raises(L.SscgError):
        F.boundary_counts(lt, lp, 4, 1)
    assert list(inspect.signature(F.boundary_counts).parameters) == ["label_true", "label_pred", "num_classes", "d", "counts"]
    assert inspect.signature(F.boundary_counts).parameters["counts"].default is None
    for cls in (md.semisuper_cycleGAN, md.supervised_model):
        p = inspect.signature(cls.evaluate).parameters
        assert p["boundary"].default is None and list(p) == ["self", "val_loader", "first_batch", "tta", "crf", "boundary"]
    assert callable(U.runningScore.set_boundary) and callable(U.runningScore.get_boundary)


def test_main_takes_boundary_and_moves_no_other_default():
    sys.path.insert(0, ROOT)
    import main
    a = main.get_args([])
    assert a.boundary == "" and "boundary" not in vars(a)               # an absent flag leaves the namespace as it always was
    b = main.get_args(["--boundary", "d=3"])
    assert b.boundary == "d=3" and set(vars(b)) - set(vars(a)) == {"boundary"}
    rest = dict(vars(b))
    del rest["boundary"]
    assert rest == vars(a)
    assert main.get_args(["--boundary", "on"]).boundary == "on" and main.get_args(["--boundary", "ratio=0.01"]).boundary == "ratio=0.01"
    old = ["--dataset", "acdc", "--tta", "0.5,1.0:flip", "--crf", "on", "--ema_decay", "0.99", "--batch_size", "4"]
    assert vars(main.get_args(old + ["--boundary", "on"])).items() >= vars(main.get_args(old)).items()
    for bad in ("zap", "d=0", "d=33", "d=x", "ratio=2"):
        with pytest.raises(SystemExit):
            main.get_args(["--boundary", bad])
