"""Multi-scale / mirrored inference (sscg_predict_head_ms / sscg_resize_flip) on a GPU-less host: the two entries are exported,
declared and bound (tests/test_abi.py holds the three-way match), the C entries return every argument error before any HIP call, the
view-list parser and the driver flag behave as documented, and no other default of main.py moved."""
import ctypes as C
import os
import sys

import pytest
import torch

from conftest import ROOT, load_sub

BAD_ARG, UNSUPPORTED = -1, -2
ONE = C.c_void_p(16)          # never dereferenced


def _views(ptrs, hs=None, ws=None):
    n = len(ptrs)
    return ((C.c_void_p * n)(*ptrs), (C.c_int * n)(*(hs or [9] * n)), (C.c_int * n)(*(ws or [9] * n)))


def test_both_entries_are_exported_declared_and_bound():
    L = load_sub("_lib")
    hdr = open(os.path.join(ROOT, "include", "sscg.h")).read()
    assert "int sscg_predict_head_ms(const float* const* xs, const int* Hs, const int* Ws, int S, uint32_t flip_mask," in hdr
    assert "int sscg_resize_flip(const float* x, float* y, int N, int H, int W, int C, int OH, int OW, int flip, void* stream);" in hdr
    assert len(L.SIGNATURES["sscg_predict_head_ms"][1]) == 15 and len(L.SIGNATURES["sscg_resize_flip"][1]) == 10
    assert callable(L.lib.sscg_predict_head_ms) and callable(L.lib.sscg_resize_flip)
    assert L.ABI_VERSION == 18 and L.lib.sscg_abi_version() == 18          # an addition: the version stays


def test_head_argument_errors_are_returned_before_any_launch():
    lib = load_sub("_lib").lib
    xs, hs, ws = _views([16, 32, 48])

    def call(xs=xs, hs=hs, ws=ws, S=3, flip=0, N=1, Cn=21, OH=32, OW=32, prob=None, index=ONE, u8=None, lt=None, hist=None):
        return lib.sscg_predict_head_ms(xs, hs, ws, S, flip, N, Cn, OH, OW, prob, index, u8, lt, hist, None)

    assert call(xs=None) == BAD_ARG and call(hs=None) == BAD_ARG and call(ws=None) == BAD_ARG
    assert call(xs=_views([16, None, 48])[0]) == BAD_ARG                  # a null member of xs
    assert call(S=0) == BAD_ARG and call(S=-1) == BAD_ARG
    nine = _views([16] * 9)
    assert call(xs=nine[0], hs=nine[1], ws=nine[2], S=9) == BAD_ARG
    assert call(flip=0b1000) == BAD_ARG and call(flip=1 << 31) == BAD_ARG   # a flip bit at or above S
    assert call(S=1, flip=0b10) == BAD_ARG
    assert call(N=0) == BAD_ARG and call(OH=0) == BAD_ARG and call(OW=-3) == BAD_ARG
    assert call(hs=_views([16] * 3, hs=[9, 0, 9])[1]) == BAD_ARG and call(ws=_views([16] * 3, ws=[9, 9, -1])[2]) == BAD_ARG
    assert call(Cn=0) == BAD_ARG and call(Cn=65) == BAD_ARG
    assert call(index=None) == BAD_ARG                                    # no output at all
    assert call(lt=ONE) == BAD_ARG and call(hist=ONE) == BAD_ARG          # label_true without hist and the reverse
    assert call(N=2, OH=32768, OW=32768) == UNSUPPORTED                   # 2^31 output pixels
    assert call(N=1, Cn=64, OH=8192, OW=4096, prob=ONE) == UNSUPPORTED    # 2^31 elements of prob_sum


def test_resize_flip_argument_errors():
    lib = load_sub("_lib").lib
    assert lib.sscg_resize_flip(None, ONE, 1, 9, 9, 3, 5, 5, 1, None) == BAD_ARG
    assert lib.sscg_resize_flip(ONE, None, 1, 9, 9, 3, 5, 5, 1, None) == BAD_ARG
    for bad in ((0, 9, 9, 3, 5, 5), (1, 0, 9, 3, 5, 5), (1, 9, -1, 3, 5, 5), (1, 9, 9, 0, 5, 5), (1, 9, 9, 3, 0, 5), (1, 9, 9, 3, 5, 0)):
        assert lib.sscg_resize_flip(ONE, ONE, *bad, 0, None) == BAD_ARG


def test_wrappers_refuse_cpu_tensors_and_bad_view_lists():
    F, L, U = load_sub("functional"), load_sub("_lib"), load_sub("utils")
    x = torch.zeros(1, 4, 9, 9)
    with pytest.raises(L.SscgError):
        F.resize_flip(torch.zeros(1, 3, 9, 9), (5, 5), True)
    with pytest.raises(L.SscgError):
        F.predict_labels_ms([x], [False], (17, 17))
    with pytest.raises(L.SscgError):
        F.predict_labels_ms([], [], (17, 17))
    with pytest.raises(L.SscgError):
        F.predict_labels_ms([x] * 9, [False] * 9, (17, 17))
    with pytest.raises(L.SscgError):
        F.predict_labels_ms([x, x], [False], (17, 17))
    assert isinstance(F.FUSE_TTA[0], bool)
    assert callable(getattr(U.runningScore, "update_logits_ms"))


def test_parse_tta_and_tta_size():
    U = load_sub("utils")
    assert U.parse_tta("0.5,0.75,1.0") == [(0.5, False), (0.75, False), (1.0, False)]
    assert U.parse_tta("0.5,0.75,1.0:flip") == [(0.5, False), (0.5, True), (0.75, False), (0.75, True), (1.0, False), (1.0, True)]
    assert U.parse_tta("") is None and U.parse_tta(None) is None
    assert len(U.parse_tta("0.5,0.75,1.0,1.25:flip")) == 8
    for bad in ("0.5,0.75,1.0,1.25,1.5:flip", "1,1,1,1,1,1,1,1,1", "0", "-0.5", "abc", "1.0:mirror", "1.0,,0.5", "nan", "inf"):
        with pytest.raises(ValueError):
            U.parse_tta(bad)
    assert U.tta_size(65, 65, 0.5) == (33, 33) and U.tta_size(1, 1, 0.1) == (1, 1)
    assert U.tta_size(256, 512, 0.75) == (192, 384) and U.tta_size(65, 33, 1.0) == (65, 33)


def test_main_takes_tta_and_moves_no_other_default():
    sys.path.insert(0, ROOT)
    import main
    a = main.get_args([])
    assert a.tta == ""
    assert main.get_args(["--tta", "0.5,1.0:flip"]).tta == "0.5,1.0:flip"
    got = dict(vars(a))
    del got["tta"]
    # the defaults tests/test_host_logic.py relies on (the reference's), and the build-only flags as they stood
    want = dict(epochs=400, decay_epoch=100, batch_size=2, lr=.0002, gpu_ids="0", crop_height=None, crop_width=None, lamda_img=0.5,
                lamda_gt=0.1, lamda_perceptual=0, lab_CE_weight=1, lab_MSE_weight=1, lab_perceptual_weight=0, adversarial_weight=1.0,
                discriminator_weight=1.0, training=False, testing=False, validation=False, model="supervised_model",
                results_dir="./results", validation_dir="./val_results", checkpoint_dir="./checkpoints/semisupervised_cycleGAN",
                dataset="voc2012", norm="instance", no_dropout=False, ngf=64, ndf=64, gen_net="deeplab", dis_net="fc_disc",
                synthetic_steps=8, as_written=1, data="auto", dtype="f32", honour_nets=0, variants="", vgg_weights=None, augment="",
                panels=None, testing_gen="resnet_9blocks_softmax")
    assert got == want


def test_the_switch_is_read_from_the_environment():
    """SSCG_FUSE_TTA=0 in a fresh process keeps predict_labels_ms on the chain of separate passes."""
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); from conftest import load_sub; "
            "print(load_sub('functional').FUSE_TTA[0])" % (ROOT, os.path.join(ROOT, "tests")))
    for val, want in ((None, "True"), ("0", "False"), ("1", "True")):
        env = dict(os.environ)
        env.pop("SSCG_FUSE_TTA", None)
        if val is not None:
            env["SSCG_FUSE_TTA"] = val
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.stdout.strip().splitlines()[-1] == want, (r.stdout, r.stderr[-2000:])
