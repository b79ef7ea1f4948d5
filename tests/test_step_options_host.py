"""Host side of the every-option schedule scenarios (tests/aids/step_options.py, tests/test_schedule_gpu.py): the bitwise record of
fuzz_step.py can tell one flipped bit, the non-vacuity conditions reject a run in which an option did nothing, and no combination
of loss flags and variants that main.py accepts is refused for the number of terms in the generator loss."""
import importlib.util
import itertools
import os
import sys

import pytest
import torch

from conftest import ROOT, load_sub

HERE = os.path.dirname(os.path.abspath(__file__))


def _so():
    spec = importlib.util.spec_from_file_location("step_options", os.path.join(HERE, "aids", "step_options.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _record():
    g = torch.Generator().manual_seed(5)
    rec = {"loss lab_loss_dice": torch.rand(3, generator=g), "loss unl_pseudo_kept": torch.rand(3, generator=g),
           "grad norms (G, D)": torch.rand(3, 2, generator=g) * 40, "EMA arena": torch.randn(1 << 16, generator=g)}
    return {k: v.view(torch.int32) for k, v in rec.items()}


def test_the_widened_record_flags_one_flipped_bit():
    """fuzz_step.py compares runs with step_options.record_diff: equal records give nothing; the lowest mantissa bit of one extra
    loss key of one step, of one gradient norm, or of one word in the middle of the EMA arena is named; so are a missing record and
    one of another shape."""
    SO = _so()
    ref = _record()
    assert SO.record_diff(ref, _record()) == []
    for key, index in (("loss lab_loss_dice", 1), ("loss unl_pseudo_kept", 2), ("grad norms (G, D)", 3), ("EMA arena", 40001)):
        got = _record()
        got[key].view(-1)[index] ^= 1
        diff = SO.record_diff(ref, got)
        assert len(diff) == 1 and diff[0].startswith(key + ": 1 of") and diff[0].endswith("first at %d" % index), diff
    got = _record()
    del got["EMA arena"]
    assert SO.record_diff(ref, got) == ["EMA arena: missing"]
    got = _record()
    got["loss lab_loss_dice"] = got["loss lab_loss_dice"][:2]
    assert len(SO.record_diff(ref, got)) == 1
    got = _record()
    got["loss new"] = got["loss lab_loss_dice"]
    assert SO.record_diff(ref, got) == ["loss new: unexpected"]


def test_a_scenario_whose_option_did_nothing_is_rejected():
    SO = _so()
    good = {k: 0.5 for k in SO.EXTRA_KEYS["all"]}
    counts = {e: 3 for e in SO.ENTRIES["all"]}
    clip = SO.OPTIONS["all"]["clip_grad_norm"]
    norms = [("G", clip * 3, clip), ("D", clip * 1.5, clip)]
    assert SO.check_not_vacuous("all", [good, good], counts, norms)
    cases = [([good, {k: v for k, v in good.items() if k != "gt_cycle_lovasz"}], counts, norms, "gt_cycle_lovasz is missing"),
             ([dict(good, unl_maxsq=float("nan"))], counts, norms, "not finite"),
             ([dict(good, unl_pseudo_kept=0.0)], counts, norms, "unl_pseudo_kept"),            # the default 0.9 at 21 classes
             ([dict(good, lab_ohem_kept=1.0)], counts, norms, "lab_ohem_kept"),
             ([dict(good, gt_cycle_ohem_kept=0.0)], counts, norms, "gt_cycle_ohem_kept"),
             ([good], dict(counts, sscg_sdm=0), norms, "sscg_sdm was never launched"),
             ([good], {k: v for k, v in counts.items() if k != "sscg_adam_step_ex"}, norms, "sscg_adam_step_ex"),
             ([good], counts, [("G", clip * 3, clip), ("D", clip, clip)], "D: last_grad_norm"),
             ([good], counts, [], "no gradient norm")]
    for steps, cnt, nrm, what in cases:
        with pytest.raises(AssertionError, match=what):
            SO.check_not_vacuous("all", steps, cnt, nrm)
    # the table itself: "all" is the union, a class weighs nothing, the thresholds are set
    assert SO.OPTIONS["all"] == dict(SO.OPTIONS["losses"], **SO.OPTIONS["optim"])
    w = [float(v) for v in SO.CE_WEIGHTS.split(",")]
    assert len(w) == 21 and w.count(0.0) == 1
    assert SO.parse_argv(["3", "64", "options=all"]) == (["3", "64"], "all") and SO.parse_argv(["3", "64"]) == (["3", "64"], None)
    with pytest.raises(SystemExit):
        SO.parse_argv(["options=nothing"])


LOSS_FLAGS = ("dice_weight", "boundary_loss", "lovasz_weight", "ssim_weight", "unl_entropy", "unl_maxsq", "unl_pseudo")
VARIANTS = ("l1_cycle", "lab_gt_dis", "gauss_noise", "perceptual")


def test_no_accepted_combination_of_loss_flags_is_refused_for_its_term_count():
    """Every subset of the seven loss flags that add terms to gen_loss, times every subset of --variants, through main.py's own
    parser: the count the step checks its assembled list against (model.gen_loss_terms_of) is what the flags imply, it passes 16 -
    the raw entry's cap - for 'every loss flag + l1_cycle' and tops out at 21, and functional.weighted_sum_launches serves each."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import main
    md, F = load_sub("model"), load_sub("functional")
    seen = set()
    for on in itertools.product((False, True), repeat=len(LOSS_FLAGS)):
        for vs in itertools.product((False, True), repeat=len(VARIANTS)):
            argv = [x for k, o in zip(LOSS_FLAGS, on) if o for x in ("--" + k, "0.5")]
            names = [v for v, o in zip(VARIANTS, vs) if o]
            if names:
                argv += ["--variants", ",".join(names)]
            args = main.get_args(argv)
            n = md.gen_loss_terms_of(args)
            flags = dict(zip(LOSS_FLAGS, on))
            want = 6 + 2 * (flags["dice_weight"] + flags["boundary_loss"] + flags["lovasz_weight"]) + flags["ssim_weight"] \
                + flags["unl_entropy"] + flags["unl_maxsq"] + flags["unl_pseudo"] \
                + ("l1_cycle" in names) * (1 + flags["ssim_weight"]) + 2 * ("perceptual" in names) + ("lab_gt_dis" in names)
            assert n == want, (argv, n, want)
            launches = F.weighted_sum_launches(n)
            assert launches == (1 if n <= 16 else 1 + -(-(n - 16) // 15)) and (launches == 1) == (n <= F.WSUM_MAX_TERMS)
            seen.add(n)
    assert min(seen) == 6 and max(seen) == 21
    every = [x for k in LOSS_FLAGS for x in ("--" + k, "0.5")]
    assert md.gen_loss_terms_of(main.get_args(every)) == 16
    assert md.gen_loss_terms_of(main.get_args(every + ["--variants", "l1_cycle"])) == 18           # refused at the first step before
    assert md.gen_loss_terms_of(_so_args(_so().OPTIONS["all"])) == 18
    assert [F.weighted_sum_launches(n) for n in (1, 16, 17, 31, 32, 40, 46, 47)] == [1, 1, 2, 2, 3, 3, 3, 4]
    with pytest.raises(ValueError):
        F.weighted_sum_launches(0)


def _so_args(opts):
    import types
    return types.SimpleNamespace(**opts)


def test_the_raw_entry_refuses_17_terms_on_the_host():
    """What the 17th term met before functional.weighted_sum folded: sscg_weighted_sum checks its count on the host, before any
    launch (no GPU is touched: the pointers are never followed), and returns SSCG_ERR_BAD_ARG, which the wrapper's `check` raised as
    SscgError at the first step of `every loss flag + --variants l1_cycle`.  16 terms is the last count the raw entry takes."""
    import ctypes as C
    L = load_sub("_lib")
    terms = torch.zeros(17)
    out = torch.zeros(())
    tab = (C.c_void_p * 17)(*[terms[i].data_ptr() for i in range(17)])
    ws = (C.c_float * 17)(*([1.0] * 17))
    rc = L.lib.sscg_weighted_sum(tab, ws, 17, out.data_ptr(), None)
    assert rc == -1 and L._ERRS[rc] == "SSCG_ERR_BAD_ARG"
    with pytest.raises(L.SscgError):
        L.check(rc, "sscg_weighted_sum")
    assert L.lib.sscg_weighted_sum(tab, ws, 0, out.data_ptr(), None) == -1
