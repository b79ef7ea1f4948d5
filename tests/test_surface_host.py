"""Surface distances of the evaluation (sscg_surface_stats, `--surface`) on a GPU-less host: the numpy / scipy restatement the GPU test
is pinned to (tests/surface_reference.py) against the Euclidean distance transform, np.percentile and cases worked by hand; the spec
parser, the options object and the score arithmetic; the entries are exported, declared and bound and return every argument error
before any HIP call; the drivers take the option and the command line moves no other default."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

import surface_reference as R
from conftest import ROOT, load_sub

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
ONE = C.c_void_p(16)          # never dereferenced


# ------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("shape", [(33, 47), (5, 9), (40, 72)])
def test_brute_force_distances_equal_the_distance_transform(shape):
    gt, pred = R.make_case(shape[0], 2, shape[0], shape[1], 4)
    seen = 0
    for n in range(2):
        for c in range(4):
            t, p = R.class_masks(gt[n], pred[n], c)
            st, sp = R.surface(t), R.surface(p)
            for src, tgt in ((st, sp), (sp, st)):
                d2 = R.directed_d2(src, tgt)
                if d2 is None:
                    continue
                edt = ndimage.distance_transform_edt(~tgt)
                assert np.array_equal(d2, np.rint(edt[src] ** 2).astype(np.int64))
                seen += 1
    assert seen >= 8


def test_surface_is_the_mask_minus_its_erosion_by_the_cross():
    m = np.zeros((7, 7), dtype=bool)
    m[1:6, 1:6] = True
    s = R.surface(m)
    assert s.sum() == 16 and not s[2:5, 2:5].any()                     # the ring of the 5 x 5 square
    m[3, 3] = False                                                     # a hole: its four neighbours become surface, the diagonals do not
    s = R.surface(m)
    assert s[2, 3] and s[4, 3] and s[3, 2] and s[3, 4] and not s[2, 2] and s.sum() == 20


@pytest.mark.parametrize("pct", [1, 50, 95, 99, 100])
def test_integer_rank_percentile_is_numpys(pct):
    rs = np.random.RandomState(pct)
    worst = 0.0
    for cnt in (1, 2, 3, 7, 20, 21, 100, 101, 977):
        d2 = rs.randint(0, 5000, cnt).astype(np.int64)
        want = float(np.percentile(np.sqrt(d2.astype(np.float64)), pct))
        worst = max(worst, abs(R.percentile_by_ranks(d2, pct) - want))
    assert worst <= 1e-9, worst


# ------------------------------------------------------------------------------------------ cases worked by hand
def test_two_single_pixels_three_four_five():
    U = load_sub("utils")
    gt = np.full((1, 6, 7), 0, dtype=np.int64)
    pred = np.zeros((1, 6, 7), dtype=np.uint8)
    gt[0, 0, 0] = 1
    pred[0, 3, 4] = 1
    st, sm = R.stats(gt, pred, 2, tol2=4, pct=95)
    for d in (0, 1):
        assert st[d, 0, 1].tolist() == [1, 0, 25, 25, 25] and sm[d, 0, 1] == 5.0
    s = U.surface_scores(st, sm, 2, "voc2012", 95)                      # VOC keeps class 1 only
    assert s["hd"] == 5.0 and s["hd95"] == 5.0 and s["assd"] == 5.0 and s["nsd"] == 0.0
    assert s["cases"] == {0: 1} and s["missing"] == {0: 0}
    assert U.surface_scores(*R.stats(gt, pred, 2, tol2=25, pct=95), 2, "voc2012", 95)["nsd"] == 1.0      # d <= tol at tol = 5


def test_identical_maps_are_at_distance_zero():
    U = load_sub("utils")
    gt, _ = R.make_case(3, 2, 33, 47, 4)
    st, sm = R.stats(gt, gt.astype(np.uint8), 4, tol2=0, pct=95)
    defined = st[0, ..., R.CNT] > 0
    assert defined.any() and np.array_equal(st[0], st[1])
    assert (st[..., R.MAX2][:, defined] == 0).all() and (st[..., R.V_HI][:, defined] == 0).all() and not sm.any()
    assert np.array_equal(st[..., R.WITHIN], st[..., R.CNT])
    s = U.surface_scores(st, sm, 4, "acdc", 95)
    assert s["hd"] == 0.0 and s["hd95"] == 0.0 and s["assd"] == 0.0 and s["nsd"] == 1.0 and sum(s["missing"].values()) == 0


def test_a_class_filling_the_image_has_the_border_ring_as_surface():
    gt = np.full((1, 5, 6), 2, dtype=np.int64)
    st, sm = R.stats(gt, gt.astype(np.uint8), 3, tol2=4, pct=95)
    assert st[0, 0, 2].tolist() == [18, 18, 0, 0, 0] and st[0, 0, 0].tolist() == [0, 0, -1, -1, -1]
    assert R.surface(gt[0] == 2).sum() == 2 * 6 + 2 * 3
    assert R.surface(np.ones((1, 4), dtype=bool)).all() and R.surface(np.ones((1, 1), dtype=bool)).all()


def test_void_and_out_of_range_values_belong_to_no_class():
    gt = np.array([[[255, 0, 0], [-1, 0, 0], [3, 0, 0]]], dtype=np.int64)
    pred = np.array([[[0, 0, 200], [0, 0, 3], [0, 0, 0]]], dtype=np.uint8)
    st, _ = R.stats(gt, pred, 3, tol2=4, pct=95)
    assert st[0, 0, 0, R.CNT] == 6 and st[1, 0, 0, R.CNT] == 7 and st[:, 0, 1:, R.CNT].sum() == 0


def test_a_case_with_one_surface_absent_is_missing():
    U = load_sub("utils")
    gt = np.zeros((2, 5, 5), dtype=np.int64)
    pred = np.zeros((2, 5, 5), dtype=np.uint8)
    gt[0, 2, 2] = 1                      # sample 0: class 1 in the ground truth only -> missing; sample 1: in neither -> not counted
    st, sm = R.stats(gt, pred, 2, tol2=4, pct=95)
    assert st[0, 0, 1].tolist() == [1, 0, -1, -1, -1] and st[1, 0, 1].tolist() == [0, 0, -1, -1, -1] and sm[0, 0, 1] == 0.0
    assert R.case_census(st) == (2, 1, 1)
    s = U.surface_scores(st, sm, 2, "acdc", 95)
    assert s["cases"] == {0: 2, 1: 0} and s["missing"] == {0: 0, 1: 1} and np.isnan(s["class_hd"][1])
    assert s["hd"] == s["class_hd"][0] and np.isfinite(s["hd"])        # the NaN class is left out of the headline
    ref = R.scores(st, sm, 2, "acdc", 95)
    assert ref["cases"] == s["cases"] and ref["missing"] == s["missing"] and ref["hd"] == s["hd"]


def test_random_maps_define_most_cases():
    defined = total = 0
    for seed, (N, H, W, Cn) in enumerate(((3, 33, 47, 4), (2, 64, 64, 4), (1, 40, 72, 21))):
        gt, pred = R.make_case(seed, N, H, W, Cn)
        d, m, z = R.case_census(R.stats(gt, pred, Cn, 4, 95)[0])
        defined, total = defined + d, total + d + m + z
    assert defined >= 0.6 * total, (defined, total)


# ------------------------------------------------------------------------------------------ scores, options, parser, state
@pytest.mark.parametrize("dataset", ["acdc", "voc2012", "cityscapes"])
@pytest.mark.parametrize("pct", [95, 100, 37])
def test_surface_scores_equal_the_restated_arithmetic(dataset, pct):
    U = load_sub("utils")
    gt, pred = R.make_case(11, 3, 33, 47, 5)
    pred[1][pred[1] == 2] = 0                                           # class 2 of sample 1 has no predicted surface: a missing case
    st, sm = R.stats(gt, pred, 5, 4, pct)
    got, want = U.surface_scores(st, sm, 5, dataset, pct), R.scores(st, sm, 5, dataset, pct)
    assert set(got) == {"hd", "hd95", "assd", "nsd", "class_hd", "class_hd95", "class_assd", "class_nsd", "cases", "missing"}
    assert got["cases"] == want["cases"] and got["missing"] == want["missing"] and sum(got["missing"].values()) >= 1
    assert len(got["class_hd"]) == (5 if dataset == "acdc" else 4)
    for key in ("hd", "hd95", "assd", "nsd"):
        assert abs(got[key] - want[key]) <= 1e-12 * max(1.0, abs(want[key])), key
        for c in want["class_" + key]:
            a, b = got["class_" + key][c], want["class_" + key][c]
            assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-12 * max(1.0, abs(b)), (key, c)
    assert got["hd"] >= got["hd95"] > 0 and 0 < got["nsd"] < 1
    # hd95 per case is np.percentile's, per direction
    n, c = 0, 1
    t, p = R.class_masks(gt[n], pred[n], c)
    a, b = R.directed_d2(R.surface(t), R.surface(p)), R.directed_d2(R.surface(p), R.surface(t))
    one = U.surface_scores(st[:, n:n + 1], sm[:, n:n + 1], 5, "acdc", pct)
    want_c = max(np.percentile(np.sqrt(a.astype(np.float64)), pct), np.percentile(np.sqrt(b.astype(np.float64)), pct))
    assert abs(one["class_hd95"][c] - want_c) <= 1e-9
    empty = U.surface_scores(np.zeros((2, 0, 5, 5), dtype=np.int64), np.zeros((2, 0, 5)), 5, dataset, pct)
    assert np.isnan(empty["hd"]) and np.isnan(empty["nsd"])
    with pytest.raises(ValueError):
        U.surface_scores(st[:, :, :4], sm, 5, dataset, pct)


def test_surface_options():
    F = load_sub("functional")
    o = F.SurfaceOptions()
    assert o.tol == 2.0 and o.pct == 95 and o.tol2 == 4
    assert F.SurfaceOptions(tol=2.5).tol2 == 6 and F.SurfaceOptions(tol=0).tol2 == 0 and F.SurfaceOptions(tol=1e9).tol2 == 2 ** 30
    assert F.SurfaceOptions(tol=3, pct=100) == F.SurfaceOptions(tol=3.0, pct=100) and F.SurfaceOptions() != F.SurfaceOptions(pct=94)
    for bad in (dict(tol=-0.1), dict(tol=float("nan")), dict(tol=float("inf")), dict(tol="2"), dict(tol=True), dict(tol=None),
                dict(pct=0), dict(pct=101), dict(pct=95.0), dict(pct="95"), dict(pct=True), dict(pct=-5)):
        with pytest.raises(ValueError):
            F.SurfaceOptions(**bad)


def test_parse_surface_table():
    F, U = load_sub("functional"), load_sub("utils")
    assert U.parse_surface("") is None and U.parse_surface(None) is None and U.parse_surface("  ") is None
    assert U.parse_surface("on") == F.SurfaceOptions() and U.parse_surface(" on ") == F.SurfaceOptions()
    assert U.parse_surface("tol=3") == F.SurfaceOptions(tol=3.0) and U.parse_surface("pct=100") == F.SurfaceOptions(pct=100)
    assert U.parse_surface("tol=1.5,pct=90") == F.SurfaceOptions(1.5, 90) and U.parse_surface("pct=90, tol=0") == F.SurfaceOptions(0.0, 90)
    for spec, token in (("off", "off"), ("tol", "tol"), ("tol=", "tol="), ("tol=x", "tol=x"), ("tol=-1", "tol=-1"), ("tol=nan", "tol=nan"),
                        ("tol=inf", "tol=inf"), ("pct=0", "pct=0"), ("pct=101", "pct=101"), ("pct=95.5", "pct=95.5"), ("pct=x", "pct=x"),
                        ("tol=2,pct=0", "pct=0"), ("tol=2,tol=3", "tol=3"), ("d=3", "d=3"), ("on,tol=2", "on"), ("TOL=2", "TOL=2"),
                        ("tol=2,", "")):
        with pytest.raises(ValueError) as e:
            U.parse_surface(spec)
        assert repr(token) in str(e.value) and "--surface" in str(e.value), (spec, str(e.value))


def test_running_score_holds_the_option_as_state():
    F, U = load_sub("functional"), load_sub("utils")
    rs = U.runningScore(4, "acdc")
    assert rs.get_surface() is None and rs.get_surface_scores() is None
    rs.set_surface(F.SurfaceOptions(tol=1.0))
    assert rs.get_surface() == F.SurfaceOptions(tol=1.0)
    s = rs.get_surface_scores()                                 # nothing scored yet: no case
    assert np.isnan(s["hd"]) and s["cases"] == {0: 0, 1: 0, 2: 0, 3: 0}
    rs.reset()
    assert rs.get_surface() == F.SurfaceOptions(tol=1.0)        # reset() clears records, not the option
    with pytest.raises(TypeError):
        rs.set_surface(3)
    rs.set_surface(None)
    assert rs.get_surface() is None and rs.get_surface_scores() is None and rs.get_boundary() is None
    rs.update([np.array([[0, 1], [2, 255]])], [np.array([[0, 1], [1, 3]])])        # the host path is as it was
    assert rs.confusion_matrix.sum() == 3


# ------------------------------------------------------------------------------------------ the entries, the wrapper, the drivers
def test_entries_are_exported_declared_and_bound():
    L = load_sub("_lib")
    hdr = open(os.path.join(ROOT, "include", "sscg.h")).read()
    assert "size_t sscg_surface_workspace(int N, int H, int W, int C);" in hdr
    assert "int sscg_surface_stats(const int64_t* label_true, const uint8_t* label_pred, int N, int H, int W, int C, int tol2, int pct," in hdr
    assert "2^30" in hdr[hdr.index("surface distances of the evaluation"):hdr.index("size_t sscg_surface_workspace(")]
    assert len(L.SIGNATURES["sscg_surface_stats"][1]) == 13 and len(L.SIGNATURES["sscg_surface_workspace"][1]) == 4
    assert callable(L.lib.sscg_surface_stats) and callable(L.lib.sscg_surface_workspace)
    assert L.ABI_VERSION == 18 and L.lib.sscg_abi_version() == 18 and "#define SSCG_ABI_VERSION 18" in hdr          # an addition
    assert "surface.hip" in open(os.path.join(ROOT, "semi-supervised-segmentation-cyclegan_amd", "csrc", "Makefile")).read()


def test_workspace_size_follows_the_documented_layout():
    lib = load_sub("_lib").lib
    up = lambda b: -(-b // 256) * 256
    for (N, H, W, Cn) in ((1, 1, 1, 1), (2, 33, 47, 4), (8, 256, 256, 21), (16, 256, 512, 20), (1, 7, 5, 64)):
        pix, G, ch = N * H * W, 2 * N * Cn, min(Cn, 8)
        want = up(2 * pix) + up(8 * pix) + up(4 * ch * pix) + up(4096 * G) + up(16 * G) + up(8 * G * H)
        assert lib.sscg_surface_workspace(N, H, W, Cn) == want, (N, H, W, Cn)
    assert lib.sscg_surface_workspace(0, 5, 5, 4) == 0 and lib.sscg_surface_workspace(1, 5, 5, 65) == 0
    assert lib.sscg_surface_workspace(1, 32768, 32768, 4) == 0


def test_argument_errors_are_returned_before_any_launch():
    lib = load_sub("_lib").lib

    def call(lt=ONE, lp=ONE, N=1, H=5, W=5, Cn=4, tol2=4, pct=95, stats=ONE, sums=ONE, ws=ONE, ws_bytes=1 << 40):
        return lib.sscg_surface_stats(lt, lp, N, H, W, Cn, tol2, pct, stats, sums, ws, ws_bytes, None)

    for ptr in ("lt", "lp", "stats", "sums", "ws"):
        assert call(**{ptr: None}) == BAD_ARG, ptr
    assert call(Cn=0) == BAD_ARG and call(Cn=65) == BAD_ARG and call(Cn=-4) == BAD_ARG
    assert call(tol2=-1) == BAD_ARG and call(pct=0) == BAD_ARG and call(pct=101) == BAD_ARG and call(pct=-95) == BAD_ARG
    for size in ("N", "H", "W"):
        assert call(**{size: 0}) == BAD_ARG and call(**{size: -3}) == BAD_ARG, size
    assert call(N=2, H=32768, W=32768) == UNSUPPORTED and call(N=1, H=1 << 16, W=1 << 15) == UNSUPPORTED          # N*H*W >= 2^31
    assert call(N=1 << 30, H=1 << 30, W=1 << 30) == UNSUPPORTED                                                    # and no overflow on the way
    assert call(N=1, H=32769, W=1) == UNSUPPORTED and call(N=1, H=23172, W=23172) == UNSUPPORTED                   # (H-1)^2 + (W-1)^2 >= 2^30
    assert call(N=2, H=32768, W=32768, pct=0) == BAD_ARG                                                           # the argument errors come first
    need = lib.sscg_surface_workspace(1, 5, 5, 4)
    assert need > 0 and call(ws_bytes=need - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    # the limit itself is at least 2^24: a 4097 x 4097 map is accepted by the size query
    assert lib.sscg_surface_workspace(1, 4097, 4097, 4) > 0 and lib.sscg_surface_workspace(1, 23170, 23170, 1) > 0


def test_wrapper_refuses_cpu_tensors_and_the_drivers_take_the_option():
    F, L, U, md = load_sub("functional"), load_sub("_lib"), load_sub("utils"), load_sub("model")
    lt, lp = torch.zeros(1, 5, 5, dtype=torch.int64), torch.zeros(1, 5, 5, dtype=torch.uint8)
    with pytest.raises(L.SscgError):
        F.surface_stats(lt, lp, 4, F.SurfaceOptions())
    assert list(inspect.signature(F.surface_stats).parameters)[:4] == ["label_true", "label_pred", "num_classes", "options"]
    for cls in (md.semisuper_cycleGAN, md.supervised_model):
        assert list(inspect.signature(cls.evaluate).parameters) == ["self", "val_loader", "first_batch", "tta", "crf", "boundary"]
        assert callable(cls.set_surface) and list(inspect.signature(cls.set_surface).parameters) == ["self", "opts"]
    assert callable(U.runningScore.set_surface) and callable(U.runningScore.get_surface) and callable(U.runningScore.get_surface_scores)


def test_main_takes_surface_and_moves_no_other_default():
    sys.path.insert(0, ROOT)
    import main
    a = main.get_args([])
    assert a.surface == "" and "surface" not in vars(a)                 # an absent flag leaves the namespace as it always was
    b = main.get_args(["--surface", "tol=3"])
    assert b.surface == "tol=3" and set(vars(b)) - set(vars(a)) == {"surface"}
    rest = dict(vars(b))
    del rest["surface"]
    assert rest == vars(a)
    assert main.get_args(["--surface", "on"]).surface == "on" and main.get_args(["--surface", "tol=1,pct=100"]).surface == "tol=1,pct=100"
    old = ["--dataset", "acdc", "--tta", "0.5,1.0:flip", "--crf", "on", "--boundary", "on", "--batch_size", "4"]
    assert vars(main.get_args(old + ["--surface", "on"])).items() >= vars(main.get_args(old)).items()
    for bad in ("zap", "tol=-1", "pct=0", "pct=x", "tol=2,pct=101"):
        with pytest.raises(SystemExit):
            main.get_args(["--surface", bad])
