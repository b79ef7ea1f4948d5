"""Windowed dense-CRF refinement (sscg_crf_head / sscg_crf_workspace, `--crf`) on a GPU-less host: the entries are exported, declared
and bound (tests/test_abi.py holds the three-way match), sscg_crf_head returns every argument error before any HIP call, the spec
parser and the options object accept and refuse what they document, the driver flag moves no other default - and the fp64 numpy
restatement the GPU test is pinned to (tests/crf_reference.py) has the properties the definition implies."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import crf_reference as R
from conftest import ROOT, load_sub

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
ONE = C.c_void_p(16)          # never dereferenced


def test_entries_are_exported_declared_and_bound():
    L = load_sub("_lib")
    hdr = open(os.path.join(ROOT, "include", "sscg.h")).read()
    assert "size_t sscg_crf_workspace(int N, int C, int OH, int OW, int iterations);" in hdr
    assert "int sscg_crf_head(const float* x, int kind, int N, int H, int W, int C, int OH, int OW, const float* img, int IC," in hdr
    assert "The reference has no CRF, so there is no call site to name" in hdr
    assert len(L.SIGNATURES["sscg_crf_head"][1]) == 19 and len(L.SIGNATURES["sscg_crf_workspace"][1]) == 5
    assert callable(L.lib.sscg_crf_head) and callable(L.lib.sscg_crf_workspace)
    assert L.ABI_VERSION == 18 and L.lib.sscg_abi_version() == 18          # an addition: the version stays
    assert (L.CRF_LOGITS, L.CRF_PROBS) == (0, 1) and "#define SSCG_CRF_LOGITS 0" in hdr and "#define SSCG_CRF_PROBS 1" in hdr
    # the parameter block mirrors the header's struct: eight four-byte members in its order
    body = hdr[hdr.index("typedef struct sscg_crf_params {"):hdr.index("} sscg_crf_params;")]
    members = [m.strip() for decl in body.split("{")[1].split(";") if decl.strip() for m in decl.strip().split(None, 1)[1].split(",")]
    assert members == [f[0] for f in L.CrfParams._fields_] and C.sizeof(L.CrfParams) == 32


def test_workspace_is_three_class_maps_and_nothing_without_iterations():
    lib = load_sub("_lib").lib
    assert lib.sscg_crf_workspace(2, 21, 37, 45, 5) == 3 * 2 * 21 * 37 * 45 * 4
    assert lib.sscg_crf_workspace(2, 21, 37, 45, 1) == 3 * 2 * 21 * 37 * 45 * 4
    assert lib.sscg_crf_workspace(2, 21, 37, 45, 0) == 0
    assert lib.sscg_crf_workspace(16, 20, 256, 512, 5) == 3 * 16 * 20 * 256 * 512 * 4          # about 2 GB: past 32 bits
    assert lib.sscg_crf_workspace(0, 21, 37, 45, 5) == 0 and lib.sscg_crf_workspace(2, 21, 37, 45, -1) == 0


def test_argument_errors_are_returned_before_any_launch():
    L = load_sub("_lib")
    lib = L.lib
    need = lib.sscg_crf_workspace(1, 21, 32, 32, 5)
    good = dict(radius=3, dilation=2, iterations=5, w_bilateral=4.0, w_spatial=3.0, theta_alpha=8.0, theta_beta=0.5, theta_gamma=3.0)

    def call(x=ONE, kind=0, N=1, H=9, W=9, Cn=21, OH=32, OW=32, img=ONE, IC=3, p="good", q=None, index=ONE, u8=None, lt=None, hist=None,
             ws=ONE, ws_bytes=need, **over):
        pp = C.byref(L.CrfParams(**dict(good, **over))) if p == "good" else p
        return lib.sscg_crf_head(x, kind, N, H, W, Cn, OH, OW, img, IC, pp, q, index, u8, lt, hist, ws, ws_bytes, None)

    assert call(x=None) == BAD_ARG and call(img=None) == BAD_ARG and call(p=None) == BAD_ARG          # null tensors, null parameters
    assert call(kind=2) == BAD_ARG and call(kind=-1) == BAD_ARG                                       # an unknown kind
    for size in ("N", "H", "W", "OH", "OW"):
        assert call(**{size: 0}) == BAD_ARG and call(**{size: -3}) == BAD_ARG, size
    assert call(Cn=0) == BAD_ARG and call(Cn=65) == BAD_ARG
    assert call(IC=0) == BAD_ARG and call(IC=5) == BAD_ARG
    assert call(radius=0) == BAD_ARG and call(radius=6) == BAD_ARG and call(radius=-1) == BAD_ARG
    assert call(dilation=0) == BAD_ARG and call(dilation=-2) == BAD_ARG
    assert call(iterations=-1) == BAD_ARG
    for wname in ("w_bilateral", "w_spatial"):
        for v in (-1.0, float("nan"), float("inf"), -float("inf")):
            assert call(**{wname: v}) == BAD_ARG, (wname, v)
    for tname in ("theta_alpha", "theta_beta", "theta_gamma"):
        for v in (0.0, -0.5, float("nan"), 1e-30):                     # the last: 1 / (2 theta^2) is not a finite fp32 number
            assert call(**{tname: v}) == BAD_ARG, (tname, v)
    assert call(index=None) == BAD_ARG                                                                # no output at all
    assert call(lt=ONE) == BAD_ARG and call(hist=ONE) == BAD_ARG                                      # label_true without hist and the reverse
    assert call(kind=1) == BAD_ARG and call(kind=1, H=32, W=31) == BAD_ARG                            # scores at another size
    assert call(iterations=0, index=None, q=ONE) == BAD_ARG                                           # Q without a mean-field step
    assert call(radius=5, dilation=4) == UNSUPPORTED and call(radius=1, dilation=17) == UNSUPPORTED   # radius * dilation > 16
    assert call(N=2, Cn=64, OH=4096, OW=4096) == UNSUPPORTED                                          # 2^31 elements of a class map
    assert call(N=1, Cn=1, OH=32768, OW=65536) == UNSUPPORTED
    assert call(ws_bytes=need - 1) == WORKSPACE and call(ws=None) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    assert call(q=ONE, index=None, ws_bytes=need - 1) == WORKSPACE                                    # Q alone is an output
    assert call(kind=1, H=32, W=32, ws_bytes=need - 1) == WORKSPACE
    assert call(lt=ONE, hist=ONE, index=None, ws_bytes=need - 1) == WORKSPACE
    # the argument errors come first whatever the workspace
    assert call(radius=6, ws_bytes=0) == BAD_ARG and call(radius=5, dilation=4, ws_bytes=0) == UNSUPPORTED


def test_crf_options_validation():
    F = load_sub("functional")
    o = F.CrfOptions()
    assert (o.iterations, o.radius, o.dilation, o.w_bilateral, o.w_spatial, o.theta_alpha, o.theta_beta, o.theta_gamma) == \
        (5, 3, 2, 4.0, 3.0, 8.0, 0.5, 3.0)
    p = o.params()
    assert (p.radius, p.dilation, p.iterations, p.w_bilateral, p.theta_beta) == (3, 2, 5, 4.0, 0.5)
    assert F.CrfOptions(iterations=0).iterations == 0 and F.CrfOptions(radius=1, dilation=16).dilation == 16
    assert F.CrfOptions(iterations=2.0).iterations == 2 and F.CrfOptions(w_bilateral=0, w_spatial=0).w_spatial == 0.0
    assert F.CrfOptions() == F.CrfOptions(iterations=5) and F.CrfOptions() != F.CrfOptions(iterations=4)
    for bad in (dict(iterations=-1), dict(iterations=1.5), dict(iterations="3"), dict(iterations=True), dict(iterations=float("nan")),
                dict(radius=0), dict(radius=6), dict(dilation=0), dict(radius=5, dilation=4), dict(dilation=9),
                dict(w_bilateral=-1), dict(w_spatial=float("inf")), dict(w_bilateral=float("nan")),
                dict(theta_alpha=0), dict(theta_beta=-1), dict(theta_gamma=float("nan"))):
        with pytest.raises(ValueError):
            F.CrfOptions(**bad)


def test_parse_crf_table():
    F, U = load_sub("functional"), load_sub("utils")
    assert U.parse_crf("") is None and U.parse_crf(None) is None and U.parse_crf("   ") is None
    assert U.parse_crf("on") == F.CrfOptions()
    assert U.parse_crf("iters=5,radius=3,dilation=2,wb=4,ws=3,alpha=8,beta=0.5,gamma=3") == F.CrfOptions()
    got = U.parse_crf("iters=2, radius=5 ,dilation=1,wb=0.5,ws=0.3,alpha=4,beta=0.25,gamma=2")
    assert got == F.CrfOptions(iterations=2, radius=5, dilation=1, w_bilateral=0.5, w_spatial=0.3, theta_alpha=4.0, theta_beta=0.25,
                               theta_gamma=2.0)
    assert U.parse_crf("iters=0") == F.CrfOptions(iterations=0) and U.parse_crf("wb=1e-1").w_bilateral == 0.1
    assert U.parse_crf("radius=1,dilation=16").dilation == 16
    # every bad token is named in the error
    for spec, token in (("off", "off"), ("iters", "iters"), ("iters=", "iters="), ("iters=x", "iters=x"), ("iters=1.5", "iters=1.5"),
                        ("iters=-1", "iters=-1"), ("radius=6", "radius=6"), ("radius=0", "radius=0"), ("iters=2,radius=6", "radius=6"),
                        ("dilation=0", "dilation=0"), ("dilation=17", "dilation=17"), ("foo=1", "foo=1"), ("on,iters=2", "on"),
                        ("wb=-1", "wb=-1"), ("wb=nan", "wb=nan"), ("ws=inf", "ws=inf"), ("alpha=0", "alpha=0"), ("beta=-2", "beta=-2"),
                        ("gamma=nan", "gamma=nan"), ("gamma=3x", "gamma=3x"), ("iters=1,,wb=2", "''"), ("iters=1,iters=2", "iters=2"),
                        ("radius=5,dilation=4", "radius=5,dilation=4"), ("=3", "=3"), ("ITERS=3", "ITERS=3")):
        with pytest.raises(ValueError) as e:
            U.parse_crf(spec)
        assert token in str(e.value) and "--crf" in str(e.value), (spec, str(e.value))


def test_wrappers_refuse_cpu_tensors_and_the_drivers_take_the_option():
    import inspect
    F, L, U, md = load_sub("functional"), load_sub("_lib"), load_sub("utils"), load_sub("model")
    x, img = torch.zeros(1, 4, 9, 9), torch.zeros(1, 3, 17, 17)
    with pytest.raises(L.SscgError):
        F.crf_labels(x, img, (17, 17), F.CrfOptions())
    with pytest.raises(TypeError):
        F.crf_labels(x, img, (17, 17), dict(iterations=5))
    assert callable(getattr(U.runningScore, "update_logits_crf"))
    assert list(inspect.signature(U.runningScore.update_logits_crf).parameters) == ["self", "label_trues", "logits_or_probs", "image", "size",
                                                                                   "crf", "probs"]
    for cls in (md.semisuper_cycleGAN, md.supervised_model):
        assert inspect.signature(cls.evaluate).parameters["crf"].default is None
    sig = inspect.signature(F.crf_labels)
    assert [p for p in sig.parameters] == ["x", "image", "size", "crf", "probs", "want_q", "want_index", "want_u8", "label_true", "hist",
                                           "num_classes"]
    assert (sig.parameters["probs"].default, sig.parameters["want_q"].default, sig.parameters["want_u8"].default) == (False, False, True)


def test_main_takes_crf_and_moves_no_other_default():
    sys.path.insert(0, ROOT)
    import main
    a = main.get_args([])
    assert a.crf == "" and "crf" not in vars(a)               # an absent flag leaves the namespace as it always was
    spec = "iters=3,radius=2,dilation=1,wb=1,ws=1,alpha=4,beta=0.5,gamma=2"
    b = main.get_args(["--crf", spec])
    assert b.crf == spec and main.get_args(["--crf", "on"]).crf == "on"
    rest = dict(vars(b))
    del rest["crf"]
    assert rest == vars(a)
    old = ["--dataset", "acdc", "--tta", "0.5,1.0:flip", "--batch_size", "4"]
    assert vars(main.get_args(old + ["--crf", "on"])).items() >= vars(main.get_args(old)).items()
    for bad in ("zap", "iters=x", "radius=9"):
        with pytest.raises(SystemExit):
            main.get_args(["--crf", bad])


# ------------------------------------------------------------------------------------------ the restatement itself
def _case(seed=3, N=2, H=5, W=6, Cn=5, OH=11, OW=13, IC=3):
    return R.make_inputs(seed, N, H, W, Cn, OH, OW, IC)


def test_restatement_without_weights_stays_at_the_softmax_of_the_unary():
    x, img = _case()
    for dt, tol in ((np.float64, 1e-15), (np.float32, 1e-6)):
        u, qs = R.crf(x, R.LOGITS, img, (11, 13), 4, 3, 2, dt, w_bilateral=0.0, w_spatial=0.0, theta_alpha=8.0, theta_beta=0.5,
                      theta_gamma=3.0)
        assert len(qs) == 5 and u.dtype == dt
        for q in qs:
            assert np.abs(q - R.softmax(u)).max() <= tol and np.abs(q.sum(axis=3) - 1).max() < 1e-5
        # u is a log-probability: its softmax is exp(u)
        assert np.abs(np.exp(u) - qs[0]).max() < (1e-12 if dt == np.float64 else 1e-6)
    # scores: the unary is their log, so Q0 is the scores normalised, whatever their scale; zeros are clamped, not -inf
    p = np.abs(x[:, :, :, :]).astype(np.float32)
    p = R.resize(p, 11, 13, np.float64).astype(np.float32)
    p[0, 0, 0, 1] = 0.0
    s = (np.float32(3.0) * p).astype(np.float64)
    u, qs = R.crf(s.astype(np.float32), R.PROBS, img, (11, 13), 0, 3, 2, np.float64, **R.STRONG)
    assert np.isfinite(u).all() and np.abs(qs[0] - s / s.sum(axis=3, keepdims=True)).max() < 1e-12


def test_restatement_is_mirror_symmetric_on_constant_inputs():
    N, Cn, OH, OW = 1, 3, 9, 12
    x = np.tile(np.array([0.3, -0.2, 0.1], dtype=np.float32), (N, 4, 5, 1))
    img = np.full((N, OH, OW, 2), 0.7, dtype=np.float32)
    u, qs = R.crf(x, R.LOGITS, img, (OH, OW), 2, 2, 2, np.float64, **R.GENTLE)
    q = qs[-1]
    assert np.abs(q - q[:, ::-1]).max() < 1e-14 and np.abs(q - q[:, :, ::-1]).max() < 1e-14
    # the borders see fewer taps than the middle, and nothing is renormalised: the result is NOT constant over the map
    assert np.abs(q[0, 0, 0] - q[0, OH // 2, OW // 2]).max() > 1e-3
    # with the same number of taps everywhere it would be: a map no larger than the dilation has no tap inside it at all
    u1, q1 = R.crf(x, R.LOGITS, img[:, :2, :2], (2, 2), 2, 2, 2, np.float64, **R.GENTLE)
    assert np.abs(q1[-1] - R.softmax(u1)).max() < 1e-15


def test_restatement_skips_taps_outside_the_map():
    """Pixel (0, 0) with radius 1: only the taps (0, +d), (+d, 0) and (+d, +d) exist.  Their message, written out by hand, is the whole
    message - the five taps outside the map contribute nothing, and a change far outside every window changes nothing either."""
    x, img = _case(seed=5, N=1, H=7, W=7, Cn=4, OH=7, OW=7, IC=2)
    d = 2
    u, qs = R.crf(x, R.LOGITS, img, (7, 7), 1, 1, d, np.float64, **R.GENTLE)
    q0, im = qs[0][0], img[0].astype(np.float64)
    ia, ib, ig = (float(np.float32(1.0 / (2.0 * R.GENTLE[k] ** 2))) for k in ("theta_alpha", "theta_beta", "theta_gamma"))
    msg = np.zeros(4)
    for dy, dx in ((0, 1), (1, 0), (1, 1)):          # row-major order of the taps that exist
        d2 = (dy * d) ** 2 + (dx * d) ** 2
        c2 = ((im[0, 0] - im[dy * d, dx * d]) ** 2).sum()
        k = R.GENTLE["w_bilateral"] * np.exp(-(d2 * ia + c2 * ib)) + R.GENTLE["w_spatial"] * np.exp(-d2 * ig)
        msg += k * q0[dy * d, dx * d]
    want = np.exp(u[0, 0, 0] + msg)
    assert np.abs(qs[1][0, 0, 0] - want / want.sum()).max() < 1e-14
    assert R.taps(1) == [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)] and len(R.taps(5)) == 120
    x2, img2 = x.copy(), img.copy()
    x2[0, 6, 6] += 5.0
    img2[0, 6, 6] -= 3.0
    _, qs2 = R.crf(x2, R.LOGITS, img2, (7, 7), 1, 1, d, np.float64, **R.GENTLE)
    assert np.array_equal(qs2[1][0, :4, :4], qs[1][0, :4, :4]) and not np.array_equal(qs2[1][0, 4, 4], qs[1][0, 4, 4])


def test_restatement_resize_matches_torch_and_fp32_tracks_fp64():
    x, img = _case(seed=7)
    z = R.resize(x, 11, 13, np.float64)
    want = torch.nn.functional.interpolate(torch.from_numpy(x).double().permute(0, 3, 1, 2), size=(11, 13), mode="bilinear",
                                           align_corners=True).permute(0, 2, 3, 1).numpy()
    assert np.abs(z - want).max() < 1e-12
    assert R.resize(x, 5, 6, np.float64) is not None and np.array_equal(R.resize(x, 5, 6, np.float32), x)       # the identity resize
    _, q64 = R.crf(x, R.LOGITS, img, (11, 13), 3, 2, 1, np.float64, **R.STRONG)
    _, q32 = R.crf(x, R.LOGITS, img, (11, 13), 3, 2, 1, np.float32, **R.STRONG)
    assert q32[-1].dtype == np.float32 and 0 < np.abs(q32[-1] - q64[-1]).max() < 1e-3
    assert np.array_equal(R.first_max(np.array([[[[0.2, 0.5, 0.5, 0.1]]]])), [[[1]]])          # the first maximum wins
    assert abs(R.top_two_margin(np.array([[[[0.2, 0.5, 0.25, 0.05]]]]))[0, 0, 0] - 0.25) < 1e-15
