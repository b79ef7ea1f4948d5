"""The inference heads (sscg_predict_head / sscg_image_head, ABI v18) on a GPU-less host: the three layers agree (tests/test_abi.py
holds declared == exported == bound), the version moved, the wrappers refuse CPU tensors and the C entries return argument errors
before any HIP call."""
import ctypes as C
import os
import sys

import pytest
import torch

from conftest import ROOT, load_sub


def test_abi_version_is_18_and_both_entries_are_bound():
    L = load_sub("_lib")
    assert L.ABI_VERSION == 18 and L.lib.sscg_abi_version() == 18
    assert "#define SSCG_ABI_VERSION 18" in open(os.path.join(ROOT, "include", "sscg.h")).read()
    assert len(L.SIGNATURES["sscg_predict_head"][1]) == 12 and len(L.SIGNATURES["sscg_image_head"][1]) == 10


def test_racecheck_reads_the_const_qualifiers_of_both_entries():
    """tools/racecheck.py derives read / write sets from the header: x and label_true are read, every output and hist written."""
    rc = load_sub("_lib").dev_tool("racecheck")
    tab = rc.parse_header(os.path.join(ROOT, "include", "sscg.h"))
    assert dict(tab["sscg_predict_head"]) == {"x": "r", "N": "-", "H": "-", "W": "-", "C": "-", "OH": "-", "OW": "-", "index": "w",
                                              "label_u8": "w", "label_true": "r", "hist": "w", "stream": "stream"}
    assert dict(tab["sscg_image_head"]) == {"x": "r", "N": "-", "H": "-", "W": "-", "C": "-", "OH": "-", "OW": "-", "y_nhwc": "w",
                                            "rgb_u8": "w", "stream": "stream"}


def test_wrappers_refuse_cpu_tensors():
    F, L = load_sub("functional"), load_sub("_lib")
    with pytest.raises(L.SscgError):
        F.predict_labels(torch.zeros(1, 21, 9, 9), (32, 32))
    with pytest.raises(L.SscgError):
        F.predict_image(torch.zeros(1, 3, 9, 9), (32, 32))
    assert callable(getattr(load_sub("utils").runningScore, "update_logits"))
    assert isinstance(F.FUSE_PREDICT[0], bool)


def test_argument_errors_are_returned_before_any_launch():
    lib = load_sub("_lib").lib
    one = C.c_void_p(16)          # never dereferenced
    BAD_ARG, UNSUPPORTED = -1, -2
    assert lib.sscg_predict_head(None, 1, 9, 9, 21, 32, 32, one, None, None, None, None) == BAD_ARG        # no logits
    assert lib.sscg_predict_head(one, 1, 9, 9, 21, 32, 32, None, None, None, None, None) == BAD_ARG        # no output at all
    assert lib.sscg_predict_head(one, 1, 9, 9, 65, 32, 32, one, None, None, None, None) == BAD_ARG         # C > 64
    assert lib.sscg_predict_head(one, 1, 9, 9, 21, 32, 32, one, None, one, None, None) == BAD_ARG          # labels without hist
    assert lib.sscg_predict_head(one, 1, 9, 9, 21, 32, 32, one, None, None, one, None) == BAD_ARG          # hist without labels
    assert lib.sscg_predict_head(one, 1, 9, 9, 21, 0, 32, one, None, None, None, None) == BAD_ARG
    assert lib.sscg_predict_head(one, 64, 9, 9, 21, 8192, 8192, one, None, None, None, None) == UNSUPPORTED  # >= 2^31 output pixels
    assert lib.sscg_image_head(None, 1, 9, 9, 3, 32, 32, one, one, None) == BAD_ARG
    assert lib.sscg_image_head(one, 1, 9, 9, 3, 32, 32, None, None, None) == BAD_ARG                        # no output at all
    assert lib.sscg_image_head(one, 1, 9, 9, 5, 32, 32, one, None, None) == BAD_ARG                         # C > 4
    assert lib.sscg_image_head(one, 1024, 9, 9, 3, 1024, 1024, one, None, None) == UNSUPPORTED              # >= 2^31 output elements


def test_the_switch_is_read_from_the_environment():
    """SSCG_FUSE_PREDICT=0 in a fresh process turns the call sites back to the chain of separate passes."""
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); from conftest import load_sub; "
            "print(load_sub('functional').FUSE_PREDICT[0])" % (ROOT, os.path.join(ROOT, "tests")))
    for val, want in ((None, "True"), ("0", "False"), ("1", "True")):
        env = dict(os.environ)
        env.pop("SSCG_FUSE_PREDICT", None)
        if val is not None:
            env["SSCG_FUSE_PREDICT"] = val
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.stdout.strip().splitlines()[-1] == want, (r.stdout, r.stderr[-2000:])
