"""Named sets of opt-in step options, shared by the schedule aids (racecheck_step.py, fuzz_step.py: `options=<name>`) and the tests
that drive them (tests/test_schedule_gpu.py): keyword arguments of oracle.fixtures.make_args, the loss keys a step must then return,
the library entries it must launch, the conditions under which a run with them is not vacuous, and the bitwise record the fuzzed
schedules are compared on.  A plain module: no fixture, no pytest hook.

The three thresholds below cannot be derived: OHEM keeps a pixel whose true-class probability is at most `ohem_thresh`, the pseudo
labels keep a pixel whose top probability is at least `unl_pseudo_thresh`, and clipping only scales when the gradient norm exceeds
`clip_grad_norm` - all three depend on what the networks emit at their first steps.  The CONDITIONS (`check_not_vacuous`) are the
contract; the numbers were read off the serial runs recorded in profiles/schedule_options.txt and are free to move with them."""
import math

CE_WEIGHTS = "1,0.5,2,1,0,1,1.5,1,1,0.75,1,1,1.25,1,1,2,1,1,0.5,1,1"     # 21 explicit weights (no loader pass resolves them); class 4 weighs 0

OPTIONS = {
    "losses": dict(
        ce_weights=CE_WEIGHTS, label_smoothing=0.1, dice_weight=0.5,
        ohem_thresh=0.03,               # threshold grid in profiles/schedule_options.txt: keeps 0.66 .. 0.87 of the pixels (0.12: up to 0.95)
        ohem_min_frac=0.0625,
        boundary_loss=0.1, lovasz_weight=0.5, lovasz_per_image=True, ssim_weight=0.5,
        unl_entropy=0.1, unl_maxsq=0.1, unl_pseudo=0.5,
        unl_pseudo_thresh=0.6,          # the same grid: keeps 0.13 .. 0.58 over the three steps (0.2: 0.95 .. 0.995; 0.8: from 0.03)
        variants="l1_cycle"),
    "optim": dict(
        clip_grad_norm=1.0,             # the same grid: the norms are ~1e6 (G), 3.1 .. 3.7 (D) and ~5e3 (supervised Gsi) at every step
        weight_decay=1e-4, adamw=True, ema_decay=0.999),
}
OPTIONS["all"] = dict(OPTIONS["losses"], **OPTIONS["optim"])

# loss keys the semi-supervised step returns beside model.LOSS_KEYS
EXTRA_KEYS = {
    "losses": ("lab_ohem_kept", "gt_cycle_ohem_kept", "lab_loss_dice", "gt_cycle_dice", "lab_loss_boundary", "gt_cycle_boundary",
               "lab_loss_lovasz", "gt_cycle_lovasz", "unl_entropy", "unl_maxsq", "unl_pseudo_ce", "unl_pseudo_kept", "lab_loss_ssim",
               "img_cycle_l1", "img_cycle_ssim"),
    "optim": (),
}
EXTRA_KEYS["all"] = EXTRA_KEYS["losses"] + EXTRA_KEYS["optim"]
KEPT_SHARES = ("lab_ohem_kept", "gt_cycle_ohem_kept", "unl_pseudo_kept")     # each strictly inside (0, 1), or the option did nothing

# library entries a semi-supervised step launches only because of the options
# (sscg_sort_u32_desc is not among them: sscg_lovasz_fwd calls the segmented sort inside the library, csrc/lovasz.hip, and the launch
# log holds what Python calls through the C ABI - the sort is covered by sscg_lovasz_fwd's own entry and workspace)
ENTRIES = {
    "losses": ("sscg_dice_fwd", "sscg_ohem_fwd", "sscg_sdm", "sscg_boundary_loss_fwd", "sscg_lovasz_fwd",
               "sscg_lovasz_scale_add", "sscg_upsample_head_bwd_b", "sscg_unl_fwd", "sscg_upsample_head_bwd_u", "sscg_l1_ssim_fwd",
               "sscg_l1_ssim_bwd"),
    "optim": ("sscg_grad_norm", "sscg_adam_step_ex"),
}
ENTRIES["all"] = ENTRIES["losses"] + ENTRIES["optim"]
UNLABELLED_ENTRIES = ("sscg_unl_fwd", "sscg_upsample_head_bwd_u", "sscg_l1_ssim_fwd", "sscg_l1_ssim_bwd")   # no supervised step has them
SUPERVISED_EXTRAS = ("ohem_kept", "dice_loss", "boundary_loss", "lovasz_loss")      # supervised_model.extras under "losses"

# the batch finish of racecheck_step.py's loaders: an affine op, a colour op that needs the mean (contrast), an elastic op, a mix op.
# data_utils.build_loaders gives the mix item to the labelled set only, so the two sets reach two different entries.
AUGMENT = "hflip,rotate=10,contrast=0.3,elastic=2:8,cutmix=0.5"
AUGMENT_ENTRIES = ("sscg_augment_mix_u8", "sscg_augment_elastic_u8")


def parse_argv(argv):
    """(positionals, option-set name or None): `options=<name>` is accepted as the last argument only."""
    if argv and argv[-1].startswith("options="):
        name = argv[-1][len("options="):]
        if name not in OPTIONS:
            raise SystemExit("unknown option set %r (known: %s)" % (name, ", ".join(sorted(OPTIONS))))
        return argv[:-1], name
    return argv, None


def supervised(opts):
    """The same flags for supervised_model: minus the unlabelled ones (it has no unlabelled batch)."""
    return {k: v for k, v in opts.items() if not k.startswith("unl_")}


def check_not_vacuous(name, steps, counts, norms, entries=None, keys=None, shares=KEPT_SHARES):
    """A scenario proves nothing if an option was silently a no-op.  `steps`: one {loss key: float} per step; `counts`: {entry
    point: launches} of the run; `norms`: one (name, last_grad_norm, max_grad_norm) per optimiser and recorded step.  Raises
    AssertionError naming every condition that does not hold."""
    bad = []
    keys = EXTRA_KEYS[name] if keys is None else keys
    for s, rec in enumerate(steps):
        for k in keys:
            if k not in rec:
                bad.append("step %d: loss key %s is missing" % (s, k))
            elif not math.isfinite(rec[k]):
                bad.append("step %d: %s = %r is not finite" % (s, k, rec[k]))
        for k in shares:
            if k in keys and k in rec and not 0.0 < rec[k] < 1.0:
                bad.append("step %d: kept share %s = %r is not strictly inside (0, 1)" % (s, k, rec[k]))
    for e in (ENTRIES[name] if entries is None else entries):
        if not counts.get(e, 0) > 0:
            bad.append("entry %s was never launched" % e)
    if OPTIONS[name].get("clip_grad_norm") is not None:
        if not norms:
            bad.append("no gradient norm was recorded")
        for who, norm, cap in norms:
            if not (math.isfinite(norm) and norm > cap):
                bad.append("%s: last_grad_norm %r does not exceed max_grad_norm %r: clipping scaled nothing" % (who, norm, cap))
    if bad:
        raise AssertionError("option set %r ran vacuously:\n  %s" % (name, "\n  ".join(bad)))
    return True


def record_diff(ref, got):
    """The bitwise comparison of two runs.  A record is an ordered {name: integer tensor holding raw bits}; returns one line per name
    whose bits differ (with the first differing flat index), or whose shape or presence differs.  Empty = the same bits."""
    out = []
    for k in ref:
        if k not in got:
            out.append("%s: missing" % k)
            continue
        a, b = ref[k], got[k]
        if tuple(a.shape) != tuple(b.shape) or a.dtype != b.dtype:
            out.append("%s: shape %s %s against %s %s" % (k, tuple(b.shape), b.dtype, tuple(a.shape), a.dtype))
            continue
        ne = (a != b).reshape(-1)
        if bool(ne.any()):
            out.append("%s: %d of %d words differ, first at %d" % (k, int(ne.sum()), ne.numel(), int(ne.nonzero()[0])))
    out += ["%s: unexpected" % k for k in got if k not in ref]
    return out
