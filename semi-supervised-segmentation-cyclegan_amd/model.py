"""Training drivers of the reference (model.py) on the MI355X kernels.

`semisuper_cycleGAN` mirrors /root/reference model.py:202-662 - same constructor argument (`args` from
main.py), same networks / losses / optimisers / checkpoint keys - but factors the 350-line `train` method
into `step(l_img, l_gt, unl_img)` (one iteration of model.py:370-552) plus a thin epoch loop.  Differences
that are deliberate and MI355X-first:
  * every tensor of the step stays in HBM: the image pools hold device tensors (the reference round-trips
    three activation batches through numpy per step, model.py:490-495) and the nine losses are device
    scalars that are only read back when they are logged;
  * forwards whose outputs the reference never uses (model.py:409) run without an autograd graph;
  * gradients accumulate into flat arenas (optim.FusedAdam) that RCCL all-reduces in one piece per
    optimiser under data parallelism (parallel.py).
`supervised_model` mirrors model.py:33-199 (BASELINE config 1)."""
import functools
import itertools
import os

import torch

from . import functional as F
from . import utils
from . import arch
from .arch import define_Dis, define_Gen, set_grad
from .optim import FusedAdam
from .utils import CLASSES, make_one_hot

_DBG_TOPWAIT = [x for x in os.environ.get("SSCG_DBG_TOPWAIT", "").split(",") if x]
# where the host ISSUES the frozen generators' pass (model.py:418-423: it feeds the D step only) and the unused Gis(lab_gt) pass (:409):
# "early" = the reference's program order, "mid" = behind the trainable generators' forwards, "late" = behind the backward's launches
_PHASES = os.environ.get("SSCG_PHASE_EVENTS") == "1"      # diagnostic: timed events around the passes of a step (tools/phases.py)
_FROZEN_AT = os.environ.get("SSCG_FROZEN_AT", "early")
_UNUSED_AT = os.environ.get("SSCG_UNUSED_AT", "early")
for _name, _v in (("SSCG_FROZEN_AT", _FROZEN_AT), ("SSCG_UNUSED_AT", _UNUSED_AT)):
    if _v not in ("early", "mid", "late"):      # (a typo would silently skip a pass: BN running statistics diverge from model.py:409)
        raise ValueError("%s=%r: expected early, mid or late" % (_name, _v))


def _check_bf16_widths(args):
    """--dtype bf16: the bf16 conv kernels move 64-channel k-tiles, so every activation between a network's first conv and its head
    must have a multiple of 64 channels - true for the reference's default widths (--ngf 64 --ndf 64), not for e.g. --ngf 32."""
    if F.get_conv_precision() == "bf16":
        for name in ("ngf", "ndf"):
            v = getattr(args, name, 64)
            if v % 64:
                raise ValueError("--dtype bf16 needs --%s to be a multiple of 64 (got %d): bf16 activations are tiled 64 channels at a "
                                 "time; use --dtype f32 for narrower networks" % (name, v))


def _select_device(args):
    """The reference puts everything on gpu_ids[0] (arch/ops.py:31-34, utils.py:221-227).  Kernels are launched on the
    CURRENT device's stream, so that device is made current once, here - `--gpu_ids 1` then works as in the reference."""
    if getattr(args, "gpu_ids", None):
        torch.cuda.set_device(int(args.gpu_ids[0]))


LOSS_KEYS = ("img_dis_loss", "gt_dis_loss", "cycle_img_dis_loss", "img_gen_loss", "gt_gen_loss", "img_cycle_loss",
             "gt_cycle_loss", "lab_loss_CE", "lab_loss_MSE")


# ---- per-epoch image panels (model.py:576-638, :164-186 of the reference)
PANEL_TAGS = ('Generated segmented image: ', 'Generated image back from segmentation: ', 'Ground truth for the image: ',
              'Image generated from val labels: ', 'Labels generated back from the cycle: ')      # model.py:634-638, as written
SUPERVISED_PANEL_TAGS = ('Generated segmented image', 'Ground truth for the image')               # model.py:185-186
PANEL_NROW = 2                      # make_grid(..., nrow=2, normalize=True) at every call site
PANEL_SCALE = PANEL_SHIFT = 0.5     # trans_std / trans_mean of model.py:603-615: 0.5 for all three datasets


def _panel_ids(logits, size, num_classes, want_onehot):
    """interp -> Softmax2d -> max(1)[1] [-> make_one_hot] of model.py:580-585.  Returns (ids [N,OH,OW], one-hot or None): one launch
    and uint8 ids by default; with SSCG_FUSE_PANELS=0 the inference head's int64 map, then label_onehot.
    (At batch size 1 the reference's `.squeeze_(1).squeeze_(0)` also drops the batch axis and make_one_hot then fails on a 3-D
    tensor: what was meant - the one-hot map of the single prediction - is served here.)"""
    if F.FUSE_PANELS[0]:
        return F.panel_labels(logits, size, want_onehot=want_onehot)
    index = F.predict_labels(logits, size, want_index=True, want_u8=False)[1]
    return index, (F.label_onehot(index.unsqueeze(1), num_classes) if want_onehot else None)


def _panel_arrays(dataset, entries):
    """entries: (tag, kind, source) with kind / source as F.panel_range takes them (COLOUR ids may also be the separate path's int64
    map).  Returns an ordered dict tag -> uint8 [3,GH,GW] numpy array: make_grid(nrow=2, normalize=True) and the image writer's byte
    conversion of every panel.  Default: range + grid per panel on the device, then five small copies; SSCG_FUSE_PANELS=0: the maps
    go to the host and through colorize_mask, PIL_to_tensor, make_grid and grid_to_u8, as in the reference."""
    from collections import OrderedDict
    out = OrderedDict()
    if F.FUSE_PANELS[0]:
        for tag, kind, src in entries:
            pal = utils.palette_tensor(dataset, src.device) if kind == F.PANEL_COLOUR else None
            sc, sh = (PANEL_SCALE, PANEL_SHIFT) if kind == F.PANEL_IMAGE else (1.0, 0.0)
            rng = F.panel_range(src, kind, sc, sh, pal)
            out[tag] = F.panel_grid(src, kind, rng, PANEL_NROW, 2, sc, sh, pal)
        for tag in out:
            out[tag] = out[tag].cpu().numpy()
        return out
    for tag, kind, src in entries:
        host = src.detach().cpu()
        if kind == F.PANEL_IMAGE:
            t = host.contiguous() * PANEL_SCALE + PANEL_SHIFT                                   # model.py:603-615
        elif kind == F.PANEL_COLOUR:
            maps = host.numpy()
            t = torch.stack([utils.PIL_to_tensor(utils.colorize_mask(maps[i], dataset), dataset) for i in range(maps.shape[0])])
        else:
            t = host.reshape(host.shape[0], 1, host.shape[-2], host.shape[-1]).float().expand(-1, 3, -1, -1)     # :627
        out[tag] = utils.grid_to_u8(utils.make_grid(t, nrow=PANEL_NROW, normalize=True))
    return out


def write_panels(panels, epoch, writer=None, panel_dir=None):
    """writer.add_image(tag, array, epoch) for every panel (model.py:634-638) and / or panel_dir/epoch%03d_<1..n>.png"""
    for i, (tag, arr) in enumerate(panels.items()):
        if writer is not None:
            writer.add_image(tag, arr, epoch)
        if panel_dir is not None:
            os.makedirs(panel_dir, exist_ok=True)
            utils.save_panel_png(arr, os.path.join(panel_dir, "epoch%03d_%d.png" % (epoch, i + 1)))


GEN_LOSS_BASE_TERMS = 6     # lab_loss_CE, lab_loss_MSE, img_gen_loss, gt_gen_loss, img_cycle_loss, gt_cycle_loss (model.py:464-468)


def gen_loss_terms(variants=(), dice=False, boundary=False, lovasz=False, ssim=False, unl=0):
    """How many terms semisuper_cycleGAN.step hands to F.weighted_sum as gen_loss: the reference's six, one per enabled region loss
    (Dice, boundary, Lovasz) on each of the two ground-truth heads, `unl` losses of the unlabelled prediction (0..4: the unlabelled
    head's three and the gated CRF loss), an SSIM term beside every image L1 (lab_loss_MSE; img_cycle_l1 under l1_cycle), and the
    variants' own terms.  Pure: the step checks its assembled list
    against it, tests/test_step_options_host.py walks every flag combination main.py accepts."""
    variants = set(variants)
    n = GEN_LOSS_BASE_TERMS + 2 * (bool(dice) + bool(boundary) + bool(lovasz)) + int(unl) + bool(ssim)
    if "l1_cycle" in variants:
        n += 1 + bool(ssim)
    if "perceptual" in variants:
        n += 2
    if "lab_gt_dis" in variants:
        n += 1
    return n


def gen_loss_terms_of(args):
    """gen_loss_terms for a parsed command line (main.get_args) or its twin: a loss flag counts when its weight is > 0."""
    on = lambda key: float(getattr(args, key, 0.0) or 0.0) > 0.0
    return gen_loss_terms((v for v in str(getattr(args, "variants", "") or "").split(",") if v), dice=on("dice_weight"),
                          boundary=on("boundary_loss"), lovasz=on("lovasz_weight"), ssim=on("ssim_weight"),
                          unl=sum(on(k) for k in ("unl_entropy", "unl_maxsq", "unl_pseudo", "unl_crf")) + _teacher_terms_of(args))


def _teacher_terms_of(args):
    """The generator-loss terms --unl_teacher adds: one per weight (mse, ce) that is > 0."""
    t = utils.parse_unl_teacher(getattr(args, "unl_teacher", "") or "")
    return 0 if t is None else int(t.mse > 0.0) + int(t.ce > 0.0)


def _optim_options(args, ema):
    """--clip_grad_norm / --weight_decay / --adamw / --ema_decay (opt-in; the reference has none of them) -> FusedAdam's keyword
    arguments.  `ema`: this optimiser keeps the EMA copy (the generators' and the supervised Gsi's do, the discriminators' does not)."""
    return dict(weight_decay=getattr(args, "weight_decay", 0.0) or 0.0, decoupled=bool(getattr(args, "adamw", False)),
                max_grad_norm=getattr(args, "clip_grad_norm", None), ema_decay=getattr(args, "ema_decay", None) if ema else None)


def _with_ema(opt_name):
    """Run a method inside `ema_weights()` of the optimiser the attribute names (a no-op without --ema_decay)."""
    def deco(fn):
        @functools.wraps(fn)
        def run(self, *a, **k):
            with getattr(self, opt_name).ema_weights():
                return fn(self, *a, **k)
        return run
    return deco


class _WeightedCE(object):
    """--ce_weights / --label_smoothing (opt-in; the reference has neither): the class weights and the smoothing of the ground-truth
    cross entropies of both drivers.  A list of weights is final at construction; a rule (median, invlog) needs the labelled set's
    class frequencies: resolve_ce_weights(labeled_loader), which train() calls before its first step."""
    ce_weight = None        # fp32 [C] on the device, or None = unweighted
    ce_smoothing = 0.0
    _ce_rule = None         # a rule of utils.parse_ce_weights still to be resolved

    def _init_ce(self, args, C):
        self.ce_smoothing = float(getattr(args, "label_smoothing", 0.0) or 0.0)
        if not 0.0 <= self.ce_smoothing < 1.0:
            raise ValueError("--label_smoothing %r is outside [0, 1)" % (args.label_smoothing,))
        spec = utils.parse_ce_weights(getattr(args, "ce_weights", ""), C)
        if isinstance(spec, list):
            self._set_ce_weight(spec, "--ce_weights")
        else:
            self._ce_rule = spec
        self._init_dice(args, C)
        self._init_ohem(args)
        self._init_boundary_loss(args, C)
        self._init_lovasz(args, C)

    # --dice_weight / --dice_smooth / --dice_skip / --dice_batch (opt-in; the reference has no Dice): every ground-truth cross entropy L
    # becomes L + dice_w * D inside its existing weight, D = the soft Dice loss of the same resized logits (functional.dice_loss)
    dice_w = 0.0            # 0 = off: no Dice launch, no extra loss key, the evaluation's result as it always was
    dice_options = None     # functional.DiceOptions when on

    def _init_dice(self, args, C):
        self.dice_w = float(getattr(args, "dice_weight", 0.0) or 0.0)
        if not self.dice_w >= 0.0:
            raise ValueError("--dice_weight %r must be >= 0" % (getattr(args, "dice_weight", None),))
        if self.dice_w == 0.0:
            return
        weight = None
        skip = utils.parse_dice_skip(getattr(args, "dice_skip", ""), C)
        if skip:
            weight = F.dice_weight([0.0 if c in skip else 1.0 for c in range(C)], C, self._ce_device())
        self.dice_options = F.DiceOptions(weight=weight, smooth=float(getattr(args, "dice_smooth", 1.0)),
                                          batch=bool(getattr(args, "dice_batch", False)))
        if not (self.dice_options.smooth > 0.0 and self.dice_options.smooth < float("inf")):
            raise ValueError("--dice_smooth %r must be a finite number > 0" % (getattr(args, "dice_smooth", None),))

    # --ohem_thresh / --ohem_min_kept / --ohem_min_frac (opt-in; the reference mines nothing): every ground-truth cross entropy runs over
    # its hardest pixels only (functional.OhemOptions; per call = per head and rank)
    ohem_options = None     # functional.OhemOptions when on: no new launch, loss key or checkpoint key otherwise

    def _init_ohem(self, args):
        thresh = getattr(args, "ohem_thresh", None)
        if thresh is None:
            return
        self.ohem_options = F.OhemOptions(thresh, min_kept=getattr(args, "ohem_min_kept", 0), min_frac=getattr(args, "ohem_min_frac", 0.0625))

    # --boundary_loss / --boundary_loss_skip / --boundary_loss_ramp (opt-in; the reference has no boundary loss): every ground-truth
    # cross entropy L becomes L + b * Boundary inside its existing weight, Boundary = Kervadec's loss of the same resized logits on the
    # labels' signed distance maps (functional.boundary_loss), b = boundary_w * min(1, epoch / ramp): a host scalar per epoch
    boundary_w = 0.0                # 0 = off: no launch, no loss key, no checkpoint key
    boundary_ramp = 0               # epochs over which b rises linearly from 0 to boundary_w; 0 = constant
    boundary_loss_options = None    # functional.BoundaryLossOptions when on
    _boundary_b = 0.0               # the weight of the current epoch (set_boundary_epoch)

    def _init_boundary_loss(self, args, C):
        self.boundary_w = float(getattr(args, "boundary_loss", 0.0) or 0.0)
        if not (self.boundary_w >= 0.0 and self.boundary_w < float("inf")):
            raise ValueError("--boundary_loss %r must be a finite number >= 0" % (getattr(args, "boundary_loss", None),))
        if self.boundary_w == 0.0:
            return
        ramp = getattr(args, "boundary_loss_ramp", 0) or 0
        if isinstance(ramp, bool) or ramp != int(ramp) or int(ramp) < 0:
            raise ValueError("--boundary_loss_ramp %r must be an integer >= 0" % (ramp,))
        self.boundary_ramp = int(ramp)
        weight = None
        skip = utils.parse_boundary_loss_skip(getattr(args, "boundary_loss_skip", ""), C)
        if skip:
            weight = F.boundary_weight([0.0 if c in skip else 1.0 for c in range(C)], C, self._ce_device())
        self.boundary_loss_options = F.BoundaryLossOptions(weight=weight)
        self.set_boundary_epoch(0)

    def set_boundary_epoch(self, epoch):
        """--boundary_loss_ramp: the boundary term's weight for `epoch` (utils.boundary_loss_schedule); train() calls it once per epoch.
        Off: nothing changes."""
        if self.boundary_loss_options is not None:
            self._boundary_b = utils.boundary_loss_schedule(self.boundary_w, self.boundary_ramp, epoch)
        return self._boundary_b

    # --lovasz_weight / --lovasz_per_image / --lovasz_classes / --lovasz_skip (opt-in; the reference has no IoU surrogate): every
    # ground-truth cross entropy L becomes L + lovasz_w * Lovasz inside its existing weight, Lovasz = the Lovasz-softmax loss of the same
    # resized logits (functional.lovasz_softmax; per call = per head and rank, as the Dice statistics are)
    lovasz_w = 0.0              # 0 = off: no launch, no loss key, no checkpoint key
    lovasz_options = None       # functional.LovaszOptions when on

    def _init_lovasz(self, args, C):
        self.lovasz_w = float(getattr(args, "lovasz_weight", 0.0) or 0.0)
        if not (self.lovasz_w >= 0.0 and self.lovasz_w < float("inf")):
            raise ValueError("--lovasz_weight %r must be a finite number >= 0" % (getattr(args, "lovasz_weight", None),))
        if self.lovasz_w == 0.0:
            return
        self.lovasz_options = F.LovaszOptions(classes=getattr(args, "lovasz_classes", "present") or "present",
                                              per_image=bool(getattr(args, "lovasz_per_image", False)),
                                              skip=utils.parse_lovasz_skip(getattr(args, "lovasz_skip", ""), C))
        self.lovasz_options.skip_mask(C)        # (refuses classes='all' with every class skipped here, not at the first step)

    def _head(self, logits, labels, want_soft, kept=None):
        """(softmax map or None, cross entropy, Dice loss or None) of the ground-truth head: the plain fused head by default.
        --ohem_thresh: the cross entropy is the mined one, and `kept` (a dict) receives the kept share of this head under "ohem_kept"
        - a device scalar from the counts the forward left, no sync.  --boundary_loss: `kept` also receives the boundary loss of this
        head under "boundary" (without a dict the term is not computed).  --lovasz_weight: likewise the Lovasz-softmax loss under
        "lovasz"."""
        kw = self._ce_kwargs()
        if self.ohem_options is not None:
            kw = dict(kw, ohem=self.ohem_options)
        if self.lovasz_options is not None and kept is not None:
            out = F.upsample_softmax_losses(logits, self.crop, labels, want_soft=want_soft, dice=self.dice_options,
                                            boundary=self.boundary_loss_options, lovasz=self.lovasz_options, **kw)
            if self.boundary_loss_options is not None:
                kept["boundary"] = out[3]
            kept["lovasz"] = out[4]
            out = out[:3]
        elif self.boundary_loss_options is not None and kept is not None:
            out = F.upsample_softmax_losses(logits, self.crop, labels, want_soft=want_soft, dice=self.dice_options,
                                            boundary=self.boundary_loss_options, **kw)
            kept["boundary"] = out[3]
            out = out[:3]
        elif self.dice_options is None:
            out = F.upsample_softmax_ce(logits, self.crop, labels, want_soft=want_soft, **kw) + (None,)
        else:
            out = F.upsample_softmax_ce_dice(logits, self.crop, labels, want_soft=want_soft, dice=self.dice_options, **kw)
        if self.ohem_options is not None and kept is not None:
            _, n_kept, n_counted = F.ohem_stats()
            kept["ohem_kept"] = n_kept.float() / n_counted.float()
        return out

    def _dice_scores(self, running):
        """--dice_weight: the per-class Dice of the confusion matrix the evaluation has just scored (utils.dice_scores), with the class
        dropping of runningScore - kept in `self.eval_dice` = {"mean_dice", "class_dice"}.  Off: nothing is computed or kept."""
        if self.dice_options is not None:
            self.eval_dice = running.get_dice()

    def _boundary_scores(self, running):
        """--boundary: the contour scores of the evaluation that has just run (runningScore.get_boundary_scores), kept in
        `self.eval_boundary` = {"boundary_iou", "class_boundary_iou", "trimap_iou", "class_trimap_iou"}.  Off: the attribute is absent."""
        scores = running.get_boundary_scores()
        if scores is not None:
            self.eval_boundary = scores
        elif hasattr(self, "eval_boundary"):
            del self.eval_boundary

    def set_surface(self, opts):
        """--surface: a F.SurfaceOptions (utils.parse_surface), or None = off, handed to the score keeper (runningScore.set_surface):
        evaluate()'s parameter list stays as it is, the option is state like the Dice and OHEM options."""
        self.running_metrics_val.set_surface(opts)

    def _surface_scores(self, running):
        """--surface: the surface distances of the evaluation that has just run (runningScore.get_surface_scores), kept in
        `self.eval_surface` = {"hd", "hd95", "assd", "nsd", "class_*", "cases", "missing"}.  Off: the attribute is absent."""
        scores = running.get_surface_scores()
        if scores is not None:
            self.eval_surface = scores
        elif hasattr(self, "eval_surface"):
            del self.eval_surface

    def set_components(self, opts):
        """--components: a F.ComponentOptions (utils.parse_components), or None = off, handed to the score keeper
        (runningScore.set_components): evaluate()'s parameter list stays as it is, the option is state like the surface option."""
        self.running_metrics_val.set_components(opts)

    def _component_scores(self, running):
        """--components: what the component filter did in the evaluation that has just run (runningScore.get_component_scores), kept
        in `self.eval_components` = {"components", "kept_components", "removed_pixels", "class_*"}.  Off: the attribute is absent."""
        scores = running.get_component_scores()
        if scores is not None:
            self.eval_components = scores
        elif hasattr(self, "eval_components"):
            del self.eval_components

    def set_sliding(self, opts):
        """--sliding: a F.SlidingOptions (utils.parse_sliding), or None = off, kept as state of the model: evaluate()'s parameter list
        stays as it is, like for the surface option.  While set, evaluate() takes the label maps from overlapping crop-sized windows
        of the loader's (larger) images; while off it launches exactly what it launches without the option."""
        if opts is not None and not isinstance(opts, F.SlidingOptions):
            raise TypeError("set_sliding: a functional.SlidingOptions or None expected, not %r" % (opts,))
        if opts is not None and opts.window != tuple(self.crop):
            raise ValueError("set_sliding: the window %r is not the crop %r the network was trained at" % (opts.window, tuple(self.crop)))
        self._sliding = opts

    def get_sliding(self):
        return getattr(self, "_sliding", None)

    def _evaluate_sliding(self, val_img, val_gt, sliding, crf):
        """One batch of evaluate() under set_sliding(): Gsi on the windows of the batch, `batch_size` windows per forward; the blended label map is
        scored at the batch's own size.  With `crf`: the CRF runs on the blended, normalised probabilities, guided by the batch."""
        size = tuple(val_img.shape[2:])
        chunk = max(1, int(getattr(self.args, "batch_size", 0) or val_img.shape[0]))
        if crf is not None:
            scores, probs = utils.crf_scores(self.Gsi, val_img, size, sliding=sliding, chunk=chunk)
            self.running_metrics_val.update_logits_crf(val_gt.squeeze(1), scores, val_img, size, crf, probs=probs)
            return
        plan = F.sliding_plan(size[0], size[1], sliding, val_img.device)
        self.running_metrics_val.update_logits_sw(val_gt.squeeze(1), utils.sliding_logits(self.Gsi, val_img, plan, chunk), plan)

    def set_calibration(self, opts, tta=None, crf=None, sliding=None):
        """--calibration: a F.CalibrationOptions (utils.parse_calibration), or None = off, handed to the score keeper
        (runningScore.set_calibration): evaluate()'s parameter list stays as it is, the option is state like the surface option.  A
        temperature grid together with `tta` / `crf` / `sliding` (what evaluate() will be called with) or SSCG_FUSE_PREDICT=0 is refused
        here."""
        self.running_metrics_val.set_calibration(opts, tta=tta, crf=crf, sliding=sliding)

    def _calibration_scores(self, running):
        """--calibration: the calibration scores of the evaluation that has just run (runningScore.get_calibration_scores), kept in
        `self.eval_calibration` = {"ece", "mce", "nll", "brier", "accuracy", "confidence", "counted", "class_gap", "bins", "above"} and,
        with a temperature grid, {"temperature", "temperature_at_edge", "temperature_grid"}.  They score the prediction as the network
        makes it: --components changes label maps, not probabilities.  Off: the attribute is absent."""
        scores = running.get_calibration_scores()
        if scores is not None:
            self.eval_calibration = scores
        elif hasattr(self, "eval_calibration"):
            del self.eval_calibration

    def _print_calibration(self):
        if hasattr(self, "eval_calibration"):
            s = self.eval_calibration
            print("The ECE / MCE / NLL / Brier score for the epoch are: ", s["ece"], s["mce"], s["nll"], s["brier"],
                  *(("| NLL-optimal temperature: ", s["temperature"], "(at the end of the grid)" if s["temperature_at_edge"] else "")
                    if "temperature" in s else ()))

    def _ce_device(self):
        ids = getattr(self.args, "gpu_ids", None)
        return torch.device("cuda", int(ids[0])) if ids else torch.device("cpu")

    def _set_ce_weight(self, values, origin):
        self.ce_weight = F.ce_weight(values, self.n_channels, self._ce_device())
        self._ce_rule = None
        if self.dp is None or self.dp.rank == 0:
            print("cross-entropy class weights (%s): %s" % (origin, ", ".join("%.6g" % v for v in values)))

    def resolve_ce_weights(self, labeled_loader):
        """One pass over the labelled loader's label maps (F.label_hist on the device; the counts are summed over the ranks of a
        process group, so every rank trains with the same weights) -> the weights of the rule --ce_weights names.  A no-op otherwise."""
        if self._ce_rule is None:
            return self.ce_weight
        rule, counts = self._ce_rule, None
        for _, l_gt, _ in labeled_loader:
            counts = F.label_hist(utils.cuda(l_gt, self.args.gpu_ids), self.n_channels, counts)
        if counts is None:
            raise ValueError("--ce_weights %s: the labelled loader is empty" % rule[0])
        if self.dp is not None:
            from .parallel import allreduce_flat
            allreduce_flat(counts)
        self._set_ce_weight(utils.ce_weights_from_counts(rule, counts.cpu().tolist()),
                            "%s of the labelled set's class frequencies" % ":".join(str(r) for r in rule))
        return self.ce_weight

    def _ce_kwargs(self):
        if self._ce_rule is not None:
            raise RuntimeError("--ce_weights %s needs the labelled set's class frequencies: call resolve_ce_weights(labeled_loader) "
                               "before the first step (train() does)" % self._ce_rule[0])
        if self.ce_weight is None and self.ce_smoothing == 0.0:
            return {}
        return {"weight": self.ce_weight, "label_smoothing": self.ce_smoothing}


class _UnlabelledLosses(object):
    # --unl_entropy / --unl_maxsq / --unl_pseudo / --unl_pseudo_thresh / --unl_ramp (opt-in; the reference's unlabelled batch reaches Gsi
    # through the cycle and adversarial terms only): the entropy, the max-squares loss and the thresholded pseudo-label cross entropy of
    # the unlabelled prediction join the generator loss as terms of their own, weight F * min(1, epoch / ramp) each
    # (functional.upsample_softmax_unl: the unlabelled head's forward plus one statistics pass, the same single backward launch)
    unl_options = None              # functional.UnlabelledOptions when a weight is > 0: no launch, loss key or checkpoint key otherwise
    unl_ramp = 0                    # epochs over which the three weights rise linearly from 0; 0 = constant
    _unl_scale = 1.0                # min(1, epoch / ramp) of the current epoch (set_unl_epoch)
    # --unl_crf / --unl_crf_kernel (opt-in): the gated CRF loss of the same prediction under the unlabelled image (functional.crf_loss:
    # one stencil launch on the softmax map the head returns, one scale launch backward), a term of its own under the same ramp
    unl_crf = 0.0                   # its weight; 0 = no launch, loss key or checkpoint key
    unl_crf_options = None          # functional.CrfOptions of the pairwise kernel when the weight is > 0

    # --unl_teacher (opt-in): mean-teacher consistency - the same Gsi under the EMA weights (--ema_decay), in evaluation mode, predicts
    # the unlabelled batch first (_teacher_logits); the head then scores the student against it (functional.upsample_softmax_teacher:
    # one statistics launch more, the same single stencil launch backward), two terms of their own under the same ramp
    unl_teacher = None              # functional.TeacherOptions when the flag is given: no launch, loss key or checkpoint key otherwise
    _teacher_rng = None             # the mirror draws' own CPU generator (`flip`): no other draw of a seed moves
    TEACHER_SEED = 0x7EAC

    def _init_unl_teacher(self, args):
        opts = utils.parse_unl_teacher(getattr(args, "unl_teacher", "") or "")
        if opts is None:
            return
        if getattr(args, "ema_decay", None) is None:
            raise ValueError("--unl_teacher needs --ema_decay: the teacher is the averaged weights")
        if opts.ce > 0.0 and float(getattr(args, "unl_pseudo", 0.0) or 0.0) > 0.0:
            raise ValueError("--unl_teacher ce= and --unl_pseudo are the same term from two label sources (the head's backward has one "
                             "pseudo-label slot): give one")
        self.unl_teacher = opts
        if opts.flip:
            self._teacher_rng = torch.Generator().manual_seed(self.TEACHER_SEED)

    # --unl_cutmix (opt-in, with --unl_teacher): CutMix consistency (French et al. 2020) - after the teacher predicted the UNMIXED batch,
    # every sample takes, with probability p, a box of a partner (functional.mix_boxes: one copy launch); the mixed batch is the step's
    # unlabelled batch from there on, and the head holds the student to the same mix of the teacher's predictions
    # (functional.upsample_softmax_teacher(mix=): sscg_teacher_fwd_mix in sscg_teacher_fwd's place, the same backward)
    unl_cutmix = None               # data_utils.augmentations.Compose of one RandomCutMix when the flag is given: nothing changes otherwise
    _cutmix_rng = None              # the boxes' own numpy generator: the flip draws and every other draw of a seed stay where they were
    CUTMIX_SEED = 0xC417
    _cutmix_said = False

    def _init_unl_cutmix(self, args):
        spec = utils.parse_unl_cutmix(getattr(args, "unl_cutmix", "") or "")
        if spec is None:
            return
        if self.unl_teacher is None:
            raise ValueError("--unl_cutmix needs --unl_teacher (and with it --ema_decay): it mixes what the teacher and the student see")
        import numpy as np
        from .data_utils import augmentations
        self.unl_cutmix = augmentations.Compose([augmentations.RandomCutMix(*spec)])
        self._cutmix_rng = np.random.RandomState(self.CUTMIX_SEED)

    def _cutmix_table(self, n):
        """One step's draw: the host int32 [n, 8] table (partner, x0, y0, x1, y1, 0, 0, 0) of Compose.mixes - its partner rule,
        RandomCutMix's boxes - at the head's output size."""
        return self.unl_cutmix.mixes(self._cutmix_rng, n, self.crop[1], self.crop[0])[0]

    def _cutmix_unl(self, unl_img, extras):
        """(the mixed unlabelled batch, the table on the device - None for a batch of one): the step's draw applied to the batch
        the teacher has already seen.  extras["unl_cutmix_share"] = the pasted share of the batch's pixels, from the host's table: a
        CPU scalar, no launch and no sync."""
        n, _, h, w = unl_img.shape
        if (h, w) != (int(self.crop[0]), int(self.crop[1])):
            raise ValueError("--unl_cutmix: the unlabelled images are %dx%d, the head's output %dx%d - the boxes are drawn at the "
                             "output size and must mean the same pixels of both" % (h, w, self.crop[0], self.crop[1]))
        if n == 1 and not self._cutmix_said:
            print("--unl_cutmix: a batch of one has no partner and is never mixed")
            self._cutmix_said = True
        rows = F.mix_table_rows(self._cutmix_table(n), n)
        live = F.mix_rows_live(rows)
        bw = (rows[:, 3].clamp(max=w) - rows[:, 1].clamp(min=0)).clamp(min=0)
        bh = (rows[:, 4].clamp(max=h) - rows[:, 2].clamp(min=0)).clamp(min=0)
        extras["unl_cutmix_share"] = ((bw * bh * live).sum().double() / float(n * h * w)).float()
        if n == 1:
            return unl_img, None
        # (a draw in which no sample fired still takes the table to the head: the mix entry then gives the plain entry's bits)
        table = F.upload_mix_table(rows, unl_img.device)
        return F.mix_boxes(unl_img, rows, table), table

    def _teacher_view(self, unl_img):
        """What the teacher sees: the unlabelled batch, each sample mirrored on W with probability 1/2 under `flip` - (view, the flip
        bytes uint8 [N] on the device or None).  The draws are the host's, so the view is built per run of equal draws
        (functional.mirror_samples: each sample read and written once) and nothing waits for the device."""
        if self._teacher_rng is None:
            return unl_img, None
        draws = torch.rand(unl_img.shape[0], generator=self._teacher_rng) < 0.5
        flip = draws.to(torch.uint8).to(unl_img.device)
        return F.mirror_samples(unl_img, draws.tolist()), flip

    def _teacher_logits(self, view):
        """The teacher's low-resolution logits of `view` (_teacher_view's batch), detached, fp32: Gsi under the EMA weights
        (g_optimizer.ema_weights: two arena swaps with their operand copies) in evaluation mode - the folded-BatchNorm inference path,
        no dropout, no running statistic moves - and back to the mode it had."""
        was = self.Gsi.training
        with self.g_optimizer.ema_weights(), torch.no_grad():
            self.Gsi.eval()
            try:
                logits = self.Gsi(view)
            finally:
                self.Gsi.train(was)
        return logits.detach().float()

    def _init_unl_crf(self, args):
        w = float(getattr(args, "unl_crf", 0.0) or 0.0)
        if not (w >= 0.0 and w < float("inf")):
            raise ValueError("--unl_crf %r must be a finite number >= 0" % (getattr(args, "unl_crf", None),))
        spec = str(getattr(args, "unl_crf_kernel", "") or "").strip()
        if spec and not w > 0.0:
            raise ValueError("--unl_crf_kernel needs --unl_crf F with F > 0")
        if w > 0.0:
            self.unl_crf, self.unl_crf_options = w, utils.parse_unl_crf_kernel(spec)

    def _init_unl(self, args):
        self._init_unl_crf(args)
        self._init_unl_teacher(args)
        self._init_unl_cutmix(args)
        w = {}
        for key in ("unl_entropy", "unl_maxsq", "unl_pseudo"):
            w[key] = float(getattr(args, key, 0.0) or 0.0)
            if not (w[key] >= 0.0 and w[key] < float("inf")):
                raise ValueError("--%s %r must be a finite number >= 0" % (key, getattr(args, key, None)))
        thresh = getattr(args, "unl_pseudo_thresh", None)
        if thresh is not None and not w["unl_pseudo"] > 0.0:
            raise ValueError("--unl_pseudo_thresh needs --unl_pseudo F with F > 0")
        thresh = 0.9 if thresh is None else float(thresh)
        if not 0.0 <= thresh <= 1.0:
            raise ValueError("--unl_pseudo_thresh %r is outside [0, 1]" % (thresh,))
        ramp = getattr(args, "unl_ramp", 0) or 0
        if isinstance(ramp, bool) or ramp != int(ramp) or int(ramp) < 0:
            raise ValueError("--unl_ramp %r must be an integer >= 0" % (ramp,))
        if not any(v > 0.0 for v in w.values()) and not self.unl_crf > 0.0 and self.unl_teacher is None:
            return
        self.unl_ramp = int(ramp)
        if any(v > 0.0 for v in w.values()):
            self.unl_options = F.UnlabelledOptions(entropy=w["unl_entropy"], maxsq=w["unl_maxsq"], pseudo=w["unl_pseudo"], thresh=thresh)
        self.set_unl_epoch(0)

    def set_unl_epoch(self, epoch):
        """--unl_ramp: the factor on the unlabelled weights for `epoch` (utils.boundary_loss_schedule's arithmetic); train() calls
        it once per epoch.  Off: nothing changes."""
        if self.unl_options is not None or self.unl_crf > 0.0 or self.unl_teacher is not None:
            self._unl_scale = utils.boundary_loss_schedule(1.0, self.unl_ramp, epoch)
        return self._unl_scale

    def _unl_head(self, fake_logits, extras, extra_terms, extra_weights, unl_img=None, teacher=None, mix=None):
        """The softmax map of the unlabelled prediction (:401-402): the plain fused head by default.  With an --unl_* weight the head
        also returns the enabled losses: each joins the extras under its own key with its own ramped weight, and --unl_pseudo reports
        the kept share K / V - a device scalar from the sums the forward left, no sync.  --unl_crf: the gated CRF loss of the map under
        `unl_img`, a node of its own beside the head - autograd adds its gradient to the map's.  --unl_teacher: `teacher` = (the
        teacher's logits, its flip bytes) of this batch, and the head is functional.upsample_softmax_teacher; --unl_cutmix: `mix` =
        the step's table on the device (_cutmix_unl), handed to that head."""
        if self.unl_teacher is not None:
            if teacher is None:
                raise ValueError("--unl_teacher: _unl_head needs the teacher's logits of this batch (_teacher_logits)")
            fake_gt = self._unl_teacher_losses(fake_logits, teacher, extras, extra_terms, extra_weights, mix)
        else:
            fake_gt = self._unl_head_losses(fake_logits, extras, extra_terms, extra_weights)
        if self.unl_crf > 0.0:
            if unl_img is None:
                raise ValueError("--unl_crf: _unl_head needs the unlabelled image batch, the guide of the CRF loss")
            extras["unl_crf"] = F.crf_loss(fake_gt, utils.crf_guide(unl_img, self.crop), self.unl_crf_options)
            extra_terms.append(extras["unl_crf"])
            extra_weights.append(self.unl_crf * self._unl_scale)
        return fake_gt

    def _unl_head_losses(self, fake_logits, extras, extra_terms, extra_weights):
        o = self.unl_options
        if o is None:
            return F.upsample_softmax_ce(fake_logits, self.crop)[0]
        fake_gt, l_ent, l_msq, l_pl, stats = F.upsample_softmax_unl(fake_logits, self.crop, o)
        for key, term, w in (("unl_entropy", l_ent, o.entropy), ("unl_maxsq", l_msq, o.maxsq), ("unl_pseudo_ce", l_pl, o.pseudo)):
            if w > 0.0:
                extras[key] = term
                extra_terms.append(term)
                extra_weights.append(w * self._unl_scale)
        if o.pseudo > 0.0:
            extras["unl_pseudo_kept"] = (stats["sums"][3] / float(fake_gt.shape[0] * self.crop[0] * self.crop[1])).float()
        return fake_gt


    def _unl_teacher_losses(self, fake_logits, teacher, extras, extra_terms, extra_weights, mix=None):
        """_unl_head_losses with the teacher: the --unl_* terms as they were, then unl_teacher_mse / unl_teacher_ce with their ramped
        weights, and the diagnostics unl_teacher_kept = K / V and unl_teacher_agree = A / max(K, 1) - device scalars from the sums."""
        o, t = self.unl_options, self.unl_teacher
        kw = {"mix": mix} if mix is not None else {}
        fake_gt, l_mse, l_ce, l_ent, l_msq, l_pl, stats = F.upsample_softmax_teacher(fake_logits, self.crop, teacher[0], t, o, flip=teacher[1], **kw)
        V = float(fake_gt.shape[0] * self.crop[0] * self.crop[1])
        for key, term, w in ((("unl_entropy", l_ent, o.entropy), ("unl_maxsq", l_msq, o.maxsq), ("unl_pseudo_ce", l_pl, o.pseudo))
                             if o is not None else ()) + (("unl_teacher_mse", l_mse, t.mse), ("unl_teacher_ce", l_ce, t.ce)):
            if w > 0.0:
                extras[key] = term
                extra_terms.append(term)
                extra_weights.append(w * self._unl_scale)
        if o is not None and o.pseudo > 0.0:
            extras["unl_pseudo_kept"] = (stats["unl_sums"][3] / V).float()
        sums = stats["sums"]
        extras["unl_teacher_kept"] = (sums[3] / V).float()
        extras["unl_teacher_agree"] = (sums[1] / sums[3].clamp(min=1.0)).float()
        return fake_gt


class semisuper_cycleGAN(_WeightedCE, _UnlabelledLosses):
    def __init__(self, args, data_parallel=None):
        self.args = args
        _select_device(args)
        _check_bf16_widths(args)
        self.n_channels = CLASSES[args.dataset]                     # model.py:205-210
        C, ids = self.n_channels, args.gpu_ids
        drop = not args.no_dropout
        # construction order = the reference's (model.py:215-230)
        # The reference hard-codes 'deeplab' / 'pixel' and never reads --gen_net / --dis_net (model.py:215-222).  Opt-in
        # (SURVEY 8(f) N4): --honour_nets 1 builds what the flags name; --variants enables loss terms that are commented
        # out in the reference (l1_cycle: model.py:453; lab_gt_dis: :439,:447).  Defaults reproduce the reference.
        honour = bool(getattr(args, "honour_nets", 0))
        gen = args.gen_net if honour else 'deeplab'
        dis = args.dis_net if honour else 'pixel'
        self.variants = set(v for v in str(getattr(args, "variants", "") or "").split(",") if v)
        unknown = self.variants - {"l1_cycle", "lab_gt_dis", "gauss_noise", "perceptual"}
        if unknown:
            raise ValueError("unknown --variants %s" % sorted(unknown))
        # model.py:281,486-488: `if torch.rand(1) < 0.0` never fires, but draws one number from torch's CPU generator per
        # step (the stream DataLoader shuffling also draws from).  The draw is kept; the variant raises the threshold to 1.
        self.gauss_noise = utils.GaussianNoise(sigma=0.2)
        self.noise_prob = 1.0 if "gauss_noise" in self.variants else 0.0
        self.Gis = define_Gen(input_nc=C, output_nc=3, ngf=args.ngf, netG=gen, norm=args.norm, use_dropout=drop, gpu_ids=ids)
        self.Gsi = define_Gen(input_nc=3, output_nc=C, ngf=args.ngf, netG=gen, norm=args.norm, use_dropout=drop, gpu_ids=ids)
        self.Di = define_Dis(input_nc=3, ndf=args.ndf, netD=dis, n_layers_D=3, norm=args.norm, gpu_ids=ids)
        self.Ds = define_Dis(input_nc=C, ndf=args.ndf, netD=dis, n_layers_D=3, norm=args.norm, gpu_ids=ids)
        self.old_Gis = define_Gen(input_nc=C, output_nc=3, ngf=args.ngf, netG='resnet_9blocks', norm=args.norm, use_dropout=drop, gpu_ids=ids)
        self.old_Gsi = define_Gen(input_nc=3, output_nc=C, ngf=args.ngf, netG='resnet_9blocks_softmax', norm=args.norm, use_dropout=drop, gpu_ids=ids)
        self.old_Di = define_Dis(input_nc=3, ndf=args.ndf, netD='pixel', n_layers_D=3, norm=args.norm, gpu_ids=ids)
        if args.dataset == 'voc2012':                               # model.py:251-257
            try:
                ck = utils.load_checkpoint('./ckpt_for_Arnab_loss.ckpt')
                self.old_Gis.load_state_dict(ck['Gis'])
                self.old_Gsi.load_state_dict(ck['Gsi'])
            except Exception:
                print('**There is an error in loading the ckpt_for_Arnab_loss**')
        utils.print_networks([self.Gis, self.Gsi, self.Di, self.Ds], ['Gis', 'Gsi', 'Di', 'Ds'])

        self.crop = (args.crop_height, args.crop_width)             # nn.Upsample(..., align_corners=True), model.py:268
        self.running_metrics_val = utils.runningScore(C, args.dataset)
        self.as_written = getattr(args, "as_written", True)         # keep the reference's unused forwards
        self.fork_forward = getattr(args, "fork_forward", True)     # two stream lanes for the trainable generator passes
        self.stack_gsi = getattr(args, "stack_gsi", True)           # the two independent Gsi passes as one grouped-BN pass
        # D step on its own stream: it then overlaps the NEXT step's generator forwards (which read no discriminator
        # weight until :431).  Opt-in, because the three discriminator losses a step returns are then produced on that
        # stream: callers read them after `sync_losses()` (train() and bench.py do).
        self.overlap_d = bool(getattr(args, "overlap_d", False))
        self.dp = data_parallel
        self._init_ce(args, C)
        self._init_ssim(args)
        self._init_unl(args)
        self.gen_terms = gen_loss_terms_of(args)
        F.weighted_sum_launches(self.gen_terms)      # (any count is served; a refusal would come here, not at the first step)

        self.g_optimizer = FusedAdam(itertools.chain(self.Gis.parameters(), self.Gsi.parameters()), lr=args.lr, betas=(0.5, 0.999),
                                     **_optim_options(args, ema=True))
        self.d_optimizer = FusedAdam(itertools.chain(self.Di.parameters(), self.Ds.parameters()), lr=args.lr, betas=(0.5, 0.999),
                                     **_optim_options(args, ema=False))
        if self.dp is not None:
            self.dp.attach(self.g_optimizer, self.d_optimizer, [self.Gis, self.Gsi, self.Di, self.Ds, self.old_Gis, self.old_Gsi, self.old_Di])
        lam = utils.LambdaLR(args.epochs, 0, args.decay_epoch).step
        self.g_lr_scheduler = torch.optim.lr_scheduler.LambdaLR(self.g_optimizer, lr_lambda=lam)
        self.d_lr_scheduler = torch.optim.lr_scheduler.LambdaLR(self.d_optimizer, lr_lambda=lam)

        self.pools = [utils.Sample_from_Pool() for _ in range(3)]   # new_img_fake / img_fake / gt_fake, model.py:350-352

        if not os.path.isdir(args.checkpoint_dir):
            os.makedirs(args.checkpoint_dir, exist_ok=True)
        # model.py:298-311.  Only a MISSING file starts from scratch: the reference's bare `except` also swallows a file that exists and
        # cannot be restored (unreadable, a key missing, a shape mismatch) and then trains over it - here that stops the run
        try:
            ck = utils.load_checkpoint('%s/latest_semisuper_cycleGAN.ckpt' % (args.checkpoint_dir))
        except FileNotFoundError:
            ck = None
            print(' [*] No checkpoint!')
            self.start_epoch = 0
            self.best_iou = -100
        if ck is not None:
            self.start_epoch = ck['epoch']
            for k in ('Di', 'Ds', 'Gis', 'Gsi'):
                getattr(self, k).load_state_dict(ck[k])
            self.d_optimizer.load_state_dict(ck['d_optimizer'])
            self.g_optimizer.load_state_dict(ck['g_optimizer'])
            if self.g_optimizer.ema_decay is not None and 'Gsi_ema' in ck and 'Gis_ema' in ck:    # (else: the EMA restarts from the weights)
                self.g_optimizer.load_ema_state_dict(self.Gsi, ck['Gsi_ema'])
                self.g_optimizer.load_ema_state_dict(self.Gis, ck['Gis_ema'])
            self.best_iou = float(ck['best_iou'])

    # --ssim_weight / --ssim_window / --ssim_sigma (opt-in; the reference's image terms are plain L1): every image L1 term gains
    # ssim_w * (1 - mean SSIM) inside its own weight, from the L1's own forward and backward launch (functional.l1_ssim_loss)
    ssim_w = 0.0                    # 0 = off: no launch, no loss key, no checkpoint key
    ssim_options = None             # functional.SsimOptions when on

    def _init_ssim(self, args):
        self.ssim_w = float(getattr(args, "ssim_weight", 0.0) or 0.0)
        if not (self.ssim_w >= 0.0 and self.ssim_w < float("inf")):
            raise ValueError("--ssim_weight %r must be a finite number >= 0" % (getattr(args, "ssim_weight", None),))
        if self.ssim_w == 0.0:
            return
        window, sigma = getattr(args, "ssim_window", 11), getattr(args, "ssim_sigma", 1.5)
        try:
            opts = F.SsimOptions(window=window, sigma=sigma, data_range=2.0)         # Normalize(.5, .5): images in [-1, 1]
        except ValueError as e:
            raise ValueError("--ssim_window / --ssim_sigma: %s" % e)
        if opts.window > min(self.crop):
            raise ValueError("--ssim_window %d is larger than the %dx%d crop" % (opts.window, self.crop[0], self.crop[1]))
        self.ssim_options = opts

    def _image_l1(self, pred, img, extras, key, weight, extra_terms, extra_weights):
        """An image L1 term; with --ssim_weight the SSIM term of the same pair joins the extras under `key` with `weight` * ssim_w."""
        if self.ssim_options is None:
            return F.l1_loss(pred, img)
        l1, extras[key] = F.l1_ssim_loss(pred, img, self.ssim_options)
        extra_terms.append(extras[key])
        extra_weights.append(weight * self.ssim_w)
        return l1

    # ------------------------------------------------------------------------------------------ one iteration
    def _mark(self, name, stream=None):
        """Diagnostic (SSCG_PHASE_EVENTS=1): a timed event on `stream` (default: the current one) + the host's clock, under `name`."""
        if not _PHASES:
            return
        import time
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(stream if stream is not None else torch.cuda.current_stream())
        self.phase_marks.append((name, ev, time.perf_counter()))

    def interp(self, x):
        return F.upsample_bilinear(x, self.crop)

    def step(self, l_img, l_gt, unl_img):
        """One G step + one D step (model.py:376-542).  Returns the nine losses as 0-dim device tensors."""
        a, C = self.args, self.n_channels
        self.phase_marks = []
        self._mark("step start")
        F.set_side_priority(F.side_priority_for(l_img.shape[0] * l_img.shape[2] * l_img.shape[3]))      # (the process's first step decides)
        if self.overlap_d and _DBG_TOPWAIT:     # bisection aid: these streams wait for the previous D step before anything of this step
            F.debug_wait_for_d(l_img.device, _DBG_TOPWAIT)
        # ---- generators (model.py:376-474)
        set_grad([self.Di, self.Ds, self.old_Di], False)
        set_grad([self.old_Gsi, self.old_Gis], False)
        self.g_optimizer.zero_grad()
        if self.dp is not None:
            self.dp.begin_backward(self.g_optimizer)     # SSCG_DP_BUCKETS: buckets of the gradient arena go out as the backward fills them
        # the generators' operand copies (bf16 shadow / split planes) exist and are current before any lane reads them: a no-op
        # after the first step (the Adam kernel rewrites them); the discriminators' follow at :431, behind their own update
        self.g_optimizer.ensure_operand_copies()
        teacher = unl_mix = None
        unl_extras = {}
        if self.unl_teacher is not None:        # --unl_teacher: the EMA weights predict the unlabelled batch before any lane starts
            view, flip = self._teacher_view(unl_img)
            teacher = (self._teacher_logits(view), flip)
            if self.unl_cutmix is not None:     # --unl_cutmix: the teacher saw the unmixed batch; every reader below sees the mixed one
                unl_img, unl_mix = self._cutmix_unl(unl_img, unl_extras)
        labels = l_gt.reshape(l_gt.shape[0], l_gt.shape[2], l_gt.shape[3])          # l_gt.squeeze(1)
        onehot_gt = make_one_hot(l_gt, a.dataset, a.gpu_ids)

        # The frozen generators depend only on the input images and feed only the D step: their forward runs
        # on the side stream, concurrently with the DeepLab forwards/backwards below.
        def frozen_branch():
            with torch.no_grad():
                if self.as_written:
                    # :418-423 runs old_Gsi/old_Gis on unl_img (used) and on l_img (results never used): both batches
                    # in one pass (per-sample InstanceNorm; batch_groups keeps a BatchNorm variant equivalent too)
                    self._mark("frozen: start")
                    with arch.batch_groups(2):
                        both = self.old_Gis(F.softmax2d(self.old_Gsi(torch.cat([unl_img, l_img], 0))))
                    self._mark("frozen: end")
                    return both[:unl_img.shape[0]]
                fake = F.softmax2d(self.old_Gsi(unl_img))                            # :418,421
                return self.old_Gis(fake)                                            # :422
        resnet_recon_img = F.run_on_side_stream(l_img.device, (unl_img, l_img), frozen_branch) if _FROZEN_AT == "early" else None
        dev = l_img.device
        fork = F.SideStream.enabled and self.fork_forward
        self._wait_operand_copies(torch.cuda.current_stream(dev))
        if fork:
            # Two lanes: Gis(onehot) -> Gsi(fake_img) on the fork stream, Gsi(unl) -> Gsi(l_img) -> Gis(fake_gt) here.
            # The reference's order of BN running-stat updates (Gis: :385 before :408; Gsi: :386, :387 before :410) is kept
            # with two events; autograd runs every backward op on its forward's stream, so the backward chains fork too.
            # (the generators' copies only: the discriminators' update of the previous step may still be in flight on
            # the D stream - rebuilding THEIR copies here would read half-updated weights and free copies still being read)
            F.refresh_transposed_weights((p for net in (self.Gis, self.Gsi) for p in net.parameters() if p.dim() == 4),
                                         all_users=False)
            main, lane = torch.cuda.current_stream(dev), F.ForkStream.get(dev)
            lane.wait_stream(main)
            with torch.cuda.stream(lane):
                self._mark("fork Gis(onehot): start")
                fake_img = self.interp(self.Gis(onehot_gt))                          # :385,390
                self._mark("fork Gis(onehot): end")
                gis_first = torch.cuda.Event()
                gis_first.record(lane)
            onehot_gt.record_stream(lane)
        else:
            fake_img = self.interp(self.Gis(onehot_gt))                              # :385,390
        fake_img_all = None
        if self.stack_gsi:
            # Gsi(unl_img) and Gsi(l_img) (:386-387) as ONE pass over both batches: every BatchNorm normalises the two
            # halves separately and advances its running statistics twice, in order (arch.batch_groups) - the same
            # arithmetic, on convolutions with twice the rows and half the launches.
            self._mark("main Gsi(unl, l): start")
            with arch.batch_groups(2):
                both = self.Gsi(torch.cat([unl_img, l_img], 0))
            self._mark("main Gsi(unl, l): end")
            fake_logits, lab_logits = F.split_batch(both, 2)
        else:
            fake_logits = self.Gsi(unl_img)                                          # :386
            lab_logits = self.Gsi(l_img)                                             # :387
        if fork:
            gsi_second = torch.cuda.Event()
            gsi_second.record(main)
        # :391-392 (interp), :398 (CE of the resized logits), :401-402 (their softmax) from the low-resolution logits in one pass each:
        # the resized [B, C, crop] logits are never written (functional.UpsampleHeadFn)
        ohem_kept = {}
        lab_gt, lab_loss_CE, lab_loss_dice = self._head(lab_logits, labels, True, ohem_kept)   # (plain nn.CrossEntropyLoss() by default)
        extra_terms, extra_weights, extras = [], [], unl_extras
        fake_gt = self._unl_head(fake_logits, extras, extra_terms, extra_weights, unl_img, teacher, unl_mix)    # (--unl_*: plus the enabled losses)
        if fork:
            main.wait_event(gis_first)
        # (Gis(onehot_gt) and Gis(fake_gt) as ONE grouped-BatchNorm pass on the main lane was built in round 4 and measured slower than
        # the two lanes; deleted in round 6)
        self._mark("main Gis(fake_gt): start")
        recon_img = self.interp(self.Gis(fake_gt))                               # :408,413
        self._mark("main Gis(fake_gt): end")
        # :409 - output unused by the reference, but it advances Gis' BN running stats (after those of the :408 pass
        # above, which the side stream waits for).  Nothing reads the result: it runs beside the critical path and is
        # joined before the optimiser touches Gis' weights.
        lab_det = lab_gt.detach()

        def unused_pass():
            with torch.no_grad():
                self._mark("side Gis(lab_gt) unused: start")
                self.Gis(lab_det)
                self._mark("side Gis(lab_gt) unused: end")
        if _UNUSED_AT == "early":
            F.run_on_side_stream(l_img.device, (lab_det,), unused_pass)
        if fork:
            with torch.cuda.stream(lane):
                lane.wait_event(gsi_second)
                fake_img_all = fake_img
                fake_img, fake_img_d, fake_img_l1 = F.split(fake_img, 3)             # consumers: Gsi, Di, L1
                self._mark("fork Gsi(fake_img): start")
                recon_logits = self.Gsi(fake_img)                                    # :410
                self._mark("fork Gsi(fake_img): end")
            main.wait_stream(lane)
            fake_img.record_stream(main)
            recon_logits.record_stream(main)
        else:
            fake_img_all = fake_img
            fake_img, fake_img_d, fake_img_l1 = F.split(fake_img, 3)                 # consumers: Gsi, Di, L1
            recon_logits = self.Gsi(fake_img)                                        # :410
        if "ohem_kept" in ohem_kept:                                                 # --ohem_thresh: the share of counted pixels lab_loss_CE kept
            extras["lab_ohem_kept"] = ohem_kept.pop("ohem_kept")
        if lab_loss_dice is not None:                                                # --dice_weight: inside lab_loss_CE's weight
            extras["lab_loss_dice"] = lab_loss_dice
            extra_terms.append(lab_loss_dice)
            extra_weights.append(a.lab_CE_weight * self.dice_w)
        if "boundary" in ohem_kept:                                                  # --boundary_loss: inside lab_loss_CE's weight
            extras["lab_loss_boundary"] = ohem_kept.pop("boundary")
            extra_terms.append(extras["lab_loss_boundary"])
            extra_weights.append(a.lab_CE_weight * self._boundary_b)
        if "lovasz" in ohem_kept:                                                    # --lovasz_weight: inside lab_loss_CE's weight
            extras["lab_loss_lovasz"] = ohem_kept.pop("lovasz")
            extra_terms.append(extras["lab_loss_lovasz"])
            extra_weights.append(a.lab_CE_weight * self.lovasz_w)
        if "l1_cycle" in self.variants:                                              # :453 (commented out in the reference)
            recon_img, recon_img_l1 = F.split(recon_img, 2)
            extras["img_cycle_l1"] = self._image_l1(recon_img_l1, unl_img, extras, "img_cycle_ssim", a.lamda_img, extra_terms, extra_weights)
            extra_terms.append(extras["img_cycle_l1"])
            extra_weights.append(a.lamda_img)
        if "perceptual" in self.variants:                                            # :454,:462 (commented out; weights main.py:23,28)
            if getattr(self, "vgg", None) is None:
                self.vgg = utils.Vgg16(requires_grad=False, weights=getattr(a, "vgg_weights", None)).to(dev)
            recon_img, recon_img_p = F.split(recon_img, 2)
            fake_img_l1, fake_img_p = F.split(fake_img_l1, 2)
            extras["img_cycle_loss_perceptual"] = utils.perceptual_loss(recon_img_p, unl_img, a.gpu_ids, self.vgg)
            extras["lab_loss_perceptual"] = utils.perceptual_loss(fake_img_p, l_img, a.gpu_ids, self.vgg)
            extra_terms += [extras["img_cycle_loss_perceptual"], extras["lab_loss_perceptual"]]
            extra_weights += [a.lamda_perceptual, a.lab_perceptual_weight]
        if "lab_gt_dis" in self.variants:                                            # :439,:447 (commented out)
            extras["gt_label_gen_loss"] = F.mse_const(self.Ds(lab_gt), 1.0)
            extra_terms.append(extras["gt_label_gen_loss"])
            extra_weights.append(a.adversarial_weight)
        if _UNUSED_AT == "mid":
            F.run_on_side_stream(l_img.device, (lab_det,), unused_pass)
        if _FROZEN_AT == "mid":
            resnet_recon_img = F.run_on_side_stream(l_img.device, (unl_img, l_img), frozen_branch)
        if self.overlap_d:      # the previous step's discriminator update (on the D stream) must have landed
            torch.cuda.current_stream(dev).wait_stream(F.d_stream(dev))
        self.d_optimizer.ensure_operand_copies()
        fake_img_dis = self.Di(fake_img_d)                                           # :431
        resnet_fake_img_dis = self.old_Di(recon_img)                                 # :432
        fake_gt_onehot, _ = F.argmax_onehot(fake_gt.detach())                        # :435-437 (no gradient path)
        fake_gt_dis = self.Ds(fake_gt_onehot)                                        # :438
        img_gen_loss = F.mse_const(fake_img_dis, 1.0)                                # :445
        gt_gen_loss = F.mse_const(fake_gt_dis, 1.0)                                  # :446
        img_cycle_loss = F.mse_const(resnet_fake_img_dis, 1.0)                       # :452
        _, gt_cycle_loss, gt_cycle_dice = self._head(recon_logits, labels, False, ohem_kept)    # :415 (interp), :455
        if "ohem_kept" in ohem_kept:                                                 # --ohem_thresh: gt_cycle_loss's kept share
            extras["gt_cycle_ohem_kept"] = ohem_kept.pop("ohem_kept")
        if gt_cycle_dice is not None:                                                # --dice_weight: inside gt_cycle_loss's weight
            extras["gt_cycle_dice"] = gt_cycle_dice
            extra_terms.append(gt_cycle_dice)
            extra_weights.append(a.lamda_gt * self.dice_w)
        if "boundary" in ohem_kept:                                                  # --boundary_loss: inside gt_cycle_loss's weight
            extras["gt_cycle_boundary"] = ohem_kept.pop("boundary")
            extra_terms.append(extras["gt_cycle_boundary"])
            extra_weights.append(a.lamda_gt * self._boundary_b)
        if "lovasz" in ohem_kept:                                                    # --lovasz_weight: inside gt_cycle_loss's weight
            extras["gt_cycle_lovasz"] = ohem_kept.pop("lovasz")
            extra_terms.append(extras["gt_cycle_lovasz"])
            extra_weights.append(a.lamda_gt * self.lovasz_w)
        lab_loss_MSE = self._image_l1(fake_img_l1, l_img, extras, "lab_loss_ssim", a.lab_MSE_weight, extra_terms, extra_weights)   # :461
        # :464-468  gen_loss = CE_w*CE + MSE_w*L1 + adv_w*(img_gen + gt_gen) + img_cycle + lamda_gt*gt_cycle
        if GEN_LOSS_BASE_TERMS + len(extra_terms) != self.gen_terms:      # a term added here must be added to gen_loss_terms too
            raise RuntimeError("gen_loss has %d terms, gen_loss_terms counted %d" % (GEN_LOSS_BASE_TERMS + len(extra_terms), self.gen_terms))
        gen_loss = F.weighted_sum(
            [lab_loss_CE, lab_loss_MSE, img_gen_loss, gt_gen_loss, img_cycle_loss, gt_cycle_loss] + extra_terms,
            [a.lab_CE_weight, a.lab_MSE_weight, a.adversarial_weight, a.adversarial_weight, 1.0, a.lamda_gt] + extra_weights)
        self._mark("main: backward start")
        if _PHASES:     # when each pass's backward STARTS (the gradient at its output arrives): host clock + an event on the stream the engine runs it on
            for name, t in (("bwd: d recon_logits (fork Gsi(fake_img) backward starts)", recon_logits), ("bwd: d recon_img (main Gis(fake_gt) backward starts)", recon_img),
                            ("bwd: d fake_img summed (fork Gis(onehot) backward starts)", fake_img_all), ("bwd: d fake_gt (main head + Gsi(unl, l) backward starts)", fake_gt),
                            ("bwd: d lab_logits / fake_logits reached", fake_logits)):
                if t is not None and t.requires_grad:
                    t.register_hook(lambda g, name=name: self._mark(name))
        F.backward(gen_loss)                                                         # :472
        self._mark("main: backward issued / main's part done")
        if _UNUSED_AT == "late":
            F.run_on_side_stream(l_img.device, (lab_det,), unused_pass)
        if _FROZEN_AT == "late":
            resnet_recon_img = F.run_on_side_stream(l_img.device, (unl_img, l_img), frozen_branch)
        F.ForkStream.join(l_img.device)
        F.SideStream.join(l_img.device)            # side stream: weight gradients + frozen generators are complete
        self._mark("main: all lanes joined")
        resnet_recon_img.record_stream(torch.cuda.current_stream(l_img.device))
        g_works = None
        if self.dp is not None:
            g_works = self.dp.sync_grads_async(self.g_optimizer)     # overlaps the D step; the update is applied below
        else:
            self.g_optimizer.step()                                                  # :474
            # the transposed weight copies the next step's data gradients read: rebuilt beside the discriminator step.  The
            # list holds the discriminators' copies too (stale since the previous D update): every stream that reads a copy
            # - the discriminator step below, the next step's lanes - first waits for this event.
            F.run_on_side_stream(l_img.device, (), F.refresh_transposed_weights)
            if F.SideStream.enabled:
                self._copies_ready = torch.cuda.Event()
                self._copies_ready.record(F.SideStream.get(dev, 0))

        # ---- discriminators (model.py:477-542)
        if self.overlap_d:
            main_s, d_s = torch.cuda.current_stream(dev), F.d_stream(dev)
            d_s.wait_stream(main_s)
            self._wait_operand_copies(d_s)
            for t in (recon_img, fake_img, fake_gt, unl_img, onehot_gt, resnet_recon_img):
                t.record_stream(d_s)
            with torch.cuda.stream(d_s):
                d_vals = self._d_step(a, recon_img, fake_img, fake_gt, unl_img, onehot_gt, resnet_recon_img)
            if self.dp is not None:
                self.dp.wait(g_works)
                self.g_optimizer.step()                                              # :474 (deferred past the all-reduce)
                self._refresh_generator_copies(dev)
        else:
            self._wait_operand_copies(torch.cuda.current_stream(dev))
            d_vals = self._d_step(a, recon_img, fake_img, fake_gt, unl_img, onehot_gt, resnet_recon_img)
            if self.dp is not None:
                self.dp.wait(g_works)
                self.g_optimizer.step()                                              # :474 (deferred: no D-step op reads G weights)
                self._refresh_generator_copies(dev)
        self._mark("main: step issued (G update queued)")
        if self.overlap_d:
            self._mark("D stream: D step done", F.d_stream(dev))
        vals = d_vals + (img_gen_loss, gt_gen_loss, img_cycle_loss, gt_cycle_loss, lab_loss_CE, lab_loss_MSE)
        out = {k: v.detach() for k, v in zip(LOSS_KEYS, vals)}
        out.update({k: v.detach() for k, v in extras.items()})
        return out

    def second_pass(self, fake_img, fake_gt, l_gt, unl_img):
        """Diagnostic twin of the part of `step` that sits two DeepLab passes deep, on GIVEN first-pass outputs (teacher forcing,
        SURVEY App. D.3): the same modules, fused head and loss kernels as step() uses for model.py:408,410,413,415,432,452,455 and for the
        discriminator step's :418-422,501-502,527-528,534 - but no optimiser, no pools.  Returns img_cycle_loss, gt_cycle_loss,
        cycle_img_dis_loss (device scalars), d(img_cycle_loss)/d(fake_gt), d(gt_cycle_loss)/d(fake_img) and recon_img.  The parity
        tests feed it the fp64 oracle's first-pass outputs, so that the three losses the step can only bound statistically (the
        first pass's fp32 noise is amplified by the second) are held to 1e-3 here."""
        set_grad([self.Di, self.Ds, self.old_Di, self.old_Gsi, self.old_Gis], False)
        self.g_optimizer.zero_grad()
        self.g_optimizer.ensure_operand_copies()
        self.d_optimizer.ensure_operand_copies()
        labels = l_gt.reshape(l_gt.shape[0], l_gt.shape[2], l_gt.shape[3])
        x_gt = fake_gt.detach().clone().requires_grad_(True)
        x_img = fake_img.detach().clone().requires_grad_(True)
        recon_img = self.interp(self.Gis(x_gt))                                          # :408,413
        img_cycle_loss = F.mse_const(self.old_Di(recon_img), 1.0)                        # :432,452
        _, gt_cycle_loss, gt_cycle_dice = self._head(self.Gsi(x_img), labels, False)     # :410,415,455
        if gt_cycle_dice is None:
            F.backward(F.weighted_sum([img_cycle_loss, gt_cycle_loss], [1.0, 1.0]))      # (each term reaches one of the two inputs only)
        else:                                                                            # --dice_weight: gt_cycle_loss + dice_w * Dice
            F.backward(F.weighted_sum([img_cycle_loss, gt_cycle_loss, gt_cycle_dice], [1.0, 1.0, self.dice_w]))
        F.SideStream.join(l_gt.device)
        with torch.no_grad():
            resnet_recon_img = self.old_Gis(F.softmax2d(self.old_Gsi(unl_img)))          # :418,421,422
            r_c = F.mse_const(self.old_Di(resnet_recon_img), 1.0)                        # :501,527
            f_c = F.mse_const(self.old_Di(recon_img.detach()), 0.0)                      # :502,528 (the pool returns the current item)
            cycle_img_dis_loss = F.weighted_sum([r_c, f_c], [1.0, 1.0])                  # :534
        self.g_optimizer.zero_grad()
        out = dict(img_cycle_loss=img_cycle_loss.detach(), gt_cycle_loss=gt_cycle_loss.detach(), cycle_img_dis_loss=cycle_img_dis_loss,
                   d_fake_gt=x_gt.grad, d_fake_img=x_img.grad, recon_img=recon_img.detach())
        if gt_cycle_dice is not None:
            out["gt_cycle_dice"] = gt_cycle_dice.detach()
        return out

    def _refresh_generator_copies(self, dev):
        """Data parallel: the generator update lands AFTER the discriminator step was queued, so the operand copies of the
        GENERATORS' weights are rebuilt here, on side lane 0, off the next step's critical path (the discriminators' copies are
        rebuilt lazily by their own step: its stream may still be reading the old ones)."""
        gen_w = [p for net in (self.Gis, self.Gsi) for p in net.parameters() if p.dim() == 4]
        F.run_on_side_stream(dev, (), lambda: F.refresh_transposed_weights(gen_w, all_users=False))
        if F.SideStream.enabled:
            self._copies_ready = torch.cuda.Event()
            self._copies_ready.record(F.SideStream.get(dev, 0))

    def _wait_operand_copies(self, stream):
        """Order `stream` behind the side lane that rebuilt the transposed / bf16 operand copies of the weights."""
        ev = getattr(self, "_copies_ready", None)
        if ev is not None:
            stream.wait_event(ev)

    def sync_losses(self):
        """Make the current stream wait for the discriminator stream (overlap_d): call before reading a step's losses."""
        if self.overlap_d:
            dev = torch.device("cuda", self.args.gpu_ids[0])
            torch.cuda.current_stream(dev).wait_stream(F.d_stream(dev))

    def _d_step(self, a, recon_img, fake_img, fake_gt, unl_img, onehot_gt, resnet_recon_img):
        l_img = unl_img
        set_grad([self.Di, self.Ds], True)
        set_grad([self.old_Di], self.as_written)   # old_Di is in no optimiser: its wgrad only exists in the as-written graph
        self.d_optimizer.zero_grad()
        if torch.rand(1) < self.noise_prob:                                          # :486 (threshold 0.0 in the reference)
            fake_img = self.gauss_noise(fake_img.detach())                           # :487
            fake_gt = self.gauss_noise(fake_gt.detach())                             # :488
        recon_img_p = self.pools[0]([recon_img.detach()])[0]                         # :490
        fake_img_p = self.pools[1]([fake_img.detach()])[0]                           # :491
        fake_gt_p = self.pools[2]([fake_gt.detach()])[0]                             # :493
        if self.overlap_d:      # a pool may hand back a tensor of an earlier step (allocated on the main stream)
            for t in (recon_img_p, fake_img_p, fake_gt_p):
                t.record_stream(torch.cuda.current_stream(t.device))
        unl_img_dis = self.Di(unl_img)                                               # :499
        fake_img_dis = self.Di(fake_img_p)                                           # :500
        resnet_recon_img_dis = self.old_Di(resnet_recon_img)                         # :501
        resnet_fake_img_dis = self.old_Di(recon_img_p)                               # :502
        real_gt_dis = self.Ds(onehot_gt)                                             # :506-507
        fake_gt_onehot, _ = F.argmax_onehot(fake_gt_p)                               # :509-511
        fake_gt_dis = self.Ds(fake_gt_onehot)                                        # :512
        r_i, f_i = F.mse_const(unl_img_dis, 1.0), F.mse_const(fake_img_dis, 0.0)     # :521-522
        r_g, f_g = F.mse_const(real_gt_dis, 1.0), F.mse_const(fake_gt_dis, 0.0)      # :523-524
        r_c, f_c = F.mse_const(resnet_recon_img_dis, 1.0), F.mse_const(resnet_fake_img_dis, 0.0)  # :527-528
        img_dis_loss = F.weighted_sum([r_i, f_i], [0.5, 0.5])                        # :531
        gt_dis_loss = F.weighted_sum([r_g, f_g], [0.5, 0.5])                         # :532
        cycle_img_dis_loss = F.weighted_sum([r_c, f_c], [1.0, 1.0])                  # :534
        dis_loss = F.weighted_sum([img_dis_loss, gt_dis_loss, cycle_img_dis_loss],
                                  [a.discriminator_weight, a.discriminator_weight, 1.0])  # :538
        F.backward(dis_loss)                                                         # :539
        F.SideStream.join(l_img.device)
        if self.dp is not None:
            self.dp.sync_grads(self.d_optimizer)
        self.d_optimizer.step()                                                      # :542
        return (img_dis_loss, gt_dis_loss, cycle_img_dis_loss)

    # ------------------------------------------------------------------------------------------ evaluation (model.py:555-574)
    @_with_ema("g_optimizer")
    @torch.no_grad()
    def evaluate(self, val_loader, first_batch=None, tta=None, crf=None, boundary=None):
        """`first_batch`: a list that receives the first batch's (val_img, val_gt) as they went through the network - the batch the
        panels are drawn from, without a second iterator on the loader.  `tta`: a view list of utils.parse_tta - Gsi runs once per
        view on the resized / mirrored batch and the views' probabilities are summed (multi-scale / mirrored inference; the
        reference evaluates one view only).  None = the single forward of the reference.  `crf`: a F.CrfOptions (utils.parse_crf) - the
        label is taken after its mean-field steps on the (summed) probabilities (the reference has no CRF); None = the plain first maximum.
        `boundary`: a F.BoundaryOptions (utils.parse_boundary) - the Boundary IoU and the trimap mIoU of the same label maps are kept in
        `self.eval_boundary` (utils.boundary_scores); None = neither is computed, nothing more is launched.  The return value is the same.
        With set_sliding() (a F.SlidingOptions, utils.parse_sliding; the option is state like the surface option) the loader's images
        keep their own (larger) size, Gsi runs on overlapping crop-sized windows and the windows' probabilities are blended
        (utils.sliding_logits, runningScore.update_logits_sw); the label maps have the batch's size, not the crop.  Off: the images
        are the crop, nothing more is launched."""
        sliding = self.get_sliding()
        if sliding is not None and tta:
            raise ValueError("evaluate: sliding-window inference does not combine with tta (its own key 'flip' mirrors the windows)")
        self.Gsi.eval()
        self.Gis.eval()
        self.running_metrics_val.reset()
        self.running_metrics_val.set_boundary(boundary)
        self.running_metrics_val.check_calibration(tta, crf, sliding=sliding)      # --calibration: a temperature grid needs the single fused head
        calibrated = self.running_metrics_val.get_calibration() is not None
        for val_img, val_gt, _ in val_loader:
            val_img, val_gt = utils.cuda([val_img, val_gt], self.args.gpu_ids)
            if first_batch is not None and not first_batch:
                first_batch.extend((val_img, val_gt))
            if sliding is not None:         # overlapping crop-sized windows over the batch's own size, blended into one label map
                self._evaluate_sliding(val_img, val_gt, sliding, crf)
                continue
            if crf is not None:             # the windowed dense CRF between the softmax and the first maximum, guided by the batch
                scores, probs = utils.crf_scores(self.Gsi, val_img, self.crop, tta)
                self.running_metrics_val.update_logits_crf(val_gt.squeeze(1), scores, utils.crf_guide(val_img, self.crop), self.crop, crf,
                                                           probs=probs)
                continue
            if tta:
                self.running_metrics_val.update_logits_ms(val_gt.squeeze(1), *utils.tta_logits(self.Gsi, val_img, tta), self.crop)
                continue
            logits = self.Gsi(val_img)
            if F.FUSE_PREDICT[0]:            # interp -> Softmax2d -> max(1)[1] -> _fast_hist in one launch (:565-569)
                self.running_metrics_val.update_logits(val_gt.squeeze(1), logits, self.crop)
                continue
            outputs = F.softmax2d(self.interp(logits))
            if calibrated:                   # --calibration on the chain of separate passes: the softmax map itself is scored
                self.running_metrics_val.update_probs(val_gt.squeeze(1), outputs)
            self.running_metrics_val.update_device(val_gt.squeeze(1), F.argmax_index(outputs))   # :566-569 without the host round trip
        score, class_iou = self.running_metrics_val.get_scores()
        self._dice_scores(self.running_metrics_val)
        self._boundary_scores(self.running_metrics_val)
        self._surface_scores(self.running_metrics_val)
        self._component_scores(self.running_metrics_val)
        self._calibration_scores(self.running_metrics_val)
        self.Gsi.train()
        self.Gis.train()
        return score["Mean IoU : \t"], class_iou

    # ------------------------------------------------------------------------------------------ image panels (model.py:576-638)
    @_with_ema("g_optimizer")
    @torch.no_grad()
    def panels(self, val_img, val_gt):
        """The five image grids the reference sends to TensorBoard after every epoch, from one validation batch on the device:
        an ordered dict tag -> uint8 [3,GH,GW] numpy array (the reference's tags, make_grid(nrow=2, normalize=True), the image
        writer's bytes).  Both generators run in eval mode (folded BatchNorm) and return to the mode they were in; no parameter,
        buffer or optimiser state changes.  SSCG_FUSE_PANELS=0 builds the same bytes by the separate passes and the host."""
        a, C = self.args, self.n_channels
        modes = (self.Gsi.training, self.Gis.training)
        self.Gsi.eval()
        self.Gis.eval()
        try:
            fake_ids, fake_onehot = _panel_ids(self.Gsi(val_img), self.crop, C, True)           # :580-585
            fake_img = self.interp(self.Gis(fake_onehot))                                       # :586-587 (no tanh: :588)
            from_labels = self.interp(self.Gis(make_one_hot(val_gt, a.dataset, a.gpu_ids)))     # :590-591
            regen_ids, _ = _panel_ids(self.Gsi(from_labels), self.crop, C, False)               # :593-597
            return _panel_arrays(a.dataset, list(zip(PANEL_TAGS, (F.PANEL_COLOUR, F.PANEL_IMAGE, F.PANEL_GREY, F.PANEL_IMAGE, F.PANEL_COLOUR),
                                                     (fake_ids, fake_img, val_gt.long(), from_labels, regen_ids))))
        finally:
            self.Gsi.train(modes[0])
            self.Gis.train(modes[1])

    # ------------------------------------------------------------------------------------------ epoch loop
    def train(self, args, loaders=None, max_steps=None, log_every=1, writer=None, panel_dir=None):
        """Epoch loop of model.py:359-660.  `loaders` = (labeled, unlabeled, val) iterables yielding the
        reference's dataset tuples (img f32[B,3,H,W], gt i64[B,1,H,W], name); None builds synthetic ones
        (the real datasets / transforms of data_utils are outside this build's scope).
        `writer` (add_scalars / add_image, e.g. tensorboardX.SummaryWriter) and `panel_dir` (PNG files) receive the epoch's image
        panels on rank 0; neither changes what is trained."""
        if loaders is None:
            from .data import synthetic_loaders
            loaders = synthetic_loaders(args, self.n_channels, rank=self.dp.rank if self.dp is not None else 0)
        labeled_loader, unlabeled_loader, val_loader = loaders
        self.resolve_ce_weights(labeled_loader)
        rank0 = self.dp is None or self.dp.rank == 0
        done = 0
        history = []
        self.set_surface(utils.parse_surface(getattr(args, 'surface', '')))
        self.set_components(utils.parse_components(getattr(args, 'components', '')))
        sliding = utils.parse_sliding(getattr(args, 'sliding', ''), self.crop)
        self.set_sliding(sliding)
        self.set_calibration(utils.parse_calibration(getattr(args, 'calibration', '')), tta=utils.parse_tta(getattr(args, 'tta', '')),
                             crf=utils.parse_crf(getattr(args, 'crf', '')), sliding=sliding)
        for epoch in range(self.start_epoch, args.epochs):
            self.set_boundary_epoch(epoch)
            self.set_unl_epoch(epoch)
            if rank0:
                print('learning rate = %.7f' % self.g_optimizer.param_groups[0]['lr'])
            self.Gsi.train()
            self.Gis.train()
            n_it = min(len(labeled_loader), len(unlabeled_loader))
            for i, ((l_img, l_gt, _), (unl_img, _, _)) in enumerate(zip(labeled_loader, unlabeled_loader)):
                l_img, unl_img, l_gt = utils.cuda([l_img, unl_img, l_gt], args.gpu_ids)
                losses = self.step(l_img, l_gt, unl_img)
                done += 1
                if (i % log_every == 0) and rank0:
                    self.sync_losses()
                    norms = [o.last_grad_norm for o in (self.g_optimizer, self.d_optimizer) if o.last_grad_norm is not None]
                    ssim_keys = [k for k in ("lab_loss_ssim", "img_cycle_ssim") if k in losses]          # --ssim_weight
                    vals = torch.stack([losses[k] for k in LOSS_KEYS + tuple(ssim_keys)] + norms).cpu().tolist()   # the only host sync of the step
                    rec = dict(zip(LOSS_KEYS, vals))
                    history.append(rec)
                    if ssim_keys:
                        print("SSIM Loss (weight %g): " % self.ssim_w + " ".join(
                            "%s:%.2e" % (k, v) for k, v in zip(ssim_keys, vals[len(LOSS_KEYS):])))
                    if norms:       # --clip_grad_norm: the norms the two updates of this step clipped
                        print("Grad norm G:%.3e D:%.3e (clip %.3e)" % (vals[-2], vals[-1], self.g_optimizer.max_grad_norm))
                    print("Epoch: (%3d) (%5d/%5d) | Dis Loss:%.2e | Unlab Gen Loss:%.2e | Lab Gen loss:%.2e" % (
                        epoch, i + 1, n_it, rec["img_dis_loss"] + rec["gt_dis_loss"],
                        args.adversarial_weight * (rec["img_gen_loss"] + rec["gt_gen_loss"]) + rec["img_cycle_loss"] + rec["gt_cycle_loss"] * args.lamda_gt,
                        args.lab_CE_weight * rec["lab_loss_CE"] + args.lab_MSE_weight * rec["lab_loss_MSE"]))
                    if writer is not None:
                        it = len(labeled_loader) * epoch + i
                        writer.add_scalars('Dis Loss', {k: rec[k] for k in LOSS_KEYS[0:3]}, it)
                        writer.add_scalars('Unlabelled Loss', {k: rec[k] for k in LOSS_KEYS[3:7]}, it)
                        writer.add_scalars('Labelled Loss', {k: rec[k] for k in LOSS_KEYS[7:9]}, it)
                if max_steps is not None and done >= max_steps:
                    return history
            self.sync_losses()                       # the last discriminator update is visible to what follows on this stream
            if val_loader is not None:
                want_panels = rank0 and (writer is not None or panel_dir is not None)
                first = [] if want_panels else None
                with self.g_optimizer.ema_weights():    # --ema_decay: the epoch's mIoU and panels are the averaged weights' (one swap)
                    miou, class_iou = self.evaluate(val_loader, first_batch=first, tta=utils.parse_tta(getattr(args, 'tta', '')),
                                                    crf=utils.parse_crf(getattr(args, 'crf', '')),
                                                    boundary=utils.parse_boundary(getattr(args, 'boundary', '')))
                    if rank0:
                        print("The mIoU for the epoch is: ", miou)
                        if self.dice_options is not None:
                            print("The mean Dice for the epoch is: ", self.eval_dice["mean_dice"])
                        if hasattr(self, "eval_boundary"):
                            print("The Boundary IoU / trimap mIoU for the epoch are: ", self.eval_boundary["boundary_iou"], self.eval_boundary["trimap_iou"])
                        if hasattr(self, "eval_surface"):
                            print("The HD / HD%d / ASSD / NSD for the epoch are: " % self.running_metrics_val.get_surface().pct,
                                  self.eval_surface["hd"], self.eval_surface["hd95"], self.eval_surface["assd"], self.eval_surface["nsd"])
                        self._print_calibration()
                        if hasattr(self, "eval_components"):
                            print("The components found / kept and the pixels relabelled for the epoch are: ", self.eval_components["components"],
                                  self.eval_components["kept_components"], self.eval_components["removed_pixels"])
                    if first:       # model.py:576-638, on the batch evaluate() has just consumed: no second iterator on the loader
                        write_panels(self.panels(*first), epoch, writer, panel_dir)
                if miou >= self.best_iou and rank0:                                 # model.py:641-655
                    self.best_iou, class_iou = utils.checkpoint_scores(miou, class_iou)     # plain numbers: the file loads weights-only
                    ck = {'epoch': epoch + 1, 'Di': self.Di.state_dict(), 'Ds': self.Ds.state_dict(),
                          'Gis': self.Gis.state_dict(), 'Gsi': self.Gsi.state_dict(),
                          'd_optimizer': self.d_optimizer.state_dict(), 'g_optimizer': self.g_optimizer.state_dict(),
                          'best_iou': self.best_iou, 'class_iou': class_iou}
                    if self.g_optimizer.ema_decay is not None:
                        ck['Gis_ema'] = self.g_optimizer.ema_state_dict(self.Gis)
                        ck['Gsi_ema'] = self.g_optimizer.ema_state_dict(self.Gsi)
                    utils.save_checkpoint(ck, '%s/latest_semisuper_cycleGAN.ckpt' % (args.checkpoint_dir))
            self.g_lr_scheduler.step()                                              # model.py:659-660
            self.d_lr_scheduler.step()
        return history


class supervised_model(_WeightedCE):
    """DeepLab Gsi + CrossEntropy + Adam(0.9, 0.999) (model.py:33-199; BASELINE config 1)."""

    def __init__(self, args, data_parallel=None):
        self.args = args
        _select_device(args)
        _check_bf16_widths(args)
        self.n_channels = CLASSES[args.dataset]
        self.Gsi = define_Gen(input_nc=3, output_nc=self.n_channels, ngf=args.ngf, netG='deeplab', norm=args.norm,
                              use_dropout=not args.no_dropout, gpu_ids=args.gpu_ids)
        utils.print_networks([self.Gsi], ['Gsi'])
        self.crop = (args.crop_height, args.crop_width)
        self.gsi_optimizer = FusedAdam(self.Gsi.parameters(), lr=args.lr, betas=(0.9, 0.999), **_optim_options(args, ema=True))   # model.py:69
        self.dp = data_parallel
        if self.dp is not None:
            self.dp.attach_one(self.gsi_optimizer, [self.Gsi])
        self._init_ce(args, self.n_channels)
        if float(getattr(args, "ssim_weight", 0.0) or 0.0) != 0.0:
            print("--ssim_weight is ignored: the supervised model has no image term")
        if any(float(getattr(args, k, 0.0) or 0.0) != 0.0 for k in ("unl_entropy", "unl_maxsq", "unl_pseudo")):
            print("--unl_entropy / --unl_maxsq / --unl_pseudo are ignored: the supervised model has no unlabelled batch")
        if float(getattr(args, "unl_crf", 0.0) or 0.0) != 0.0:
            print("--unl_crf is ignored: the supervised model has no unlabelled batch")
        if str(getattr(args, "unl_teacher", "") or "").strip():
            print("--unl_teacher is ignored: the supervised model has no unlabelled batch")
        if str(getattr(args, "unl_cutmix", "") or "").strip():
            print("--unl_cutmix is ignored: the supervised model has no unlabelled batch")
        self.running_metrics_val = utils.runningScore(self.n_channels, args.dataset)
        if not os.path.isdir(args.checkpoint_dir):
            os.makedirs(args.checkpoint_dir, exist_ok=True)
        try:                # (only a missing file starts from scratch, as in semisuper_cycleGAN)
            ck = utils.load_checkpoint('%s/latest_supervised_model.ckpt' % (args.checkpoint_dir))
        except FileNotFoundError:
            ck = None
            print(' [*] No checkpoint!')
            self.start_epoch = 0
            self.best_iou = -100
        if ck is not None:
            self.start_epoch = ck['epoch']
            self.Gsi.load_state_dict(ck['Gsi'])
            self.gsi_optimizer.load_state_dict(ck['gsi_optimizer'])
            if self.gsi_optimizer.ema_decay is not None and 'Gsi_ema' in ck:      # (else: the EMA restarts from the weights)
                self.gsi_optimizer.load_ema_state_dict(self.Gsi, ck['Gsi_ema'])
            self.best_iou = float(ck['best_iou'])

    def step(self, l_img, l_gt):
        """model.py:120-143."""
        self.gsi_optimizer.zero_grad()
        ohem_kept = {}
        _, loss, dice = self._head(self.Gsi(l_img), l_gt.reshape(l_gt.shape[0], l_gt.shape[2], l_gt.shape[3]), False, ohem_kept)
        bnd = ohem_kept.pop("boundary", None)
        lov = ohem_kept.pop("lovasz", None)
        if ohem_kept:   # --ohem_thresh: the step returns the mined cross entropy, the kept share of the counted pixels goes to self.extras
            self.extras = ohem_kept
        if dice is None and bnd is None and lov is None:
            F.backward(loss)
        elif bnd is None and lov is None:       # --dice_weight: CE + dice_w * Dice; the step still returns the cross entropy, the Dice term goes to self.extras
            self.extras = dict(ohem_kept, dice_loss=dice.detach())
            F.backward(F.weighted_sum([loss, dice], [1.0, self.dice_w]))
        else:       # --boundary_loss / --lovasz_weight: CE [+ dice_w * Dice] [+ b * Boundary] [+ lovasz_w * Lovasz], reported the same way
            terms, weights = [loss], [1.0]
            self.extras = dict(ohem_kept)
            if bnd is not None:
                terms.append(bnd)
                weights.append(self._boundary_b)
                self.extras["boundary_loss"] = bnd.detach()
            if lov is not None:
                terms.append(lov)
                weights.append(self.lovasz_w)
                self.extras["lovasz_loss"] = lov.detach()
            if dice is not None:
                terms.append(dice)
                weights.append(self.dice_w)
                self.extras["dice_loss"] = dice.detach()
            F.backward(F.weighted_sum(terms, weights))
        if self.dp is not None:
            F.SideStream.join(l_img.device)
            self.dp.sync_grads(self.gsi_optimizer)
        self.gsi_optimizer.step()
        return loss.detach()

    @_with_ema("gsi_optimizer")
    @torch.no_grad()
    def evaluate(self, val_loader, first_batch=None, tta=None, crf=None, boundary=None):
        """model.py:145-162.  The reference interpolates to a hard-coded 512x512 (`interp_val`, model.py:63,152), which only
        works for a 512x512 crop; the crop size is used here, as the semi-supervised driver does.
        `first_batch`: a list that receives the first batch's (val_img, val_gt) on the device (the batch of the panels).
        `tta`: a view list of utils.parse_tta, `crf`: a F.CrfOptions, both as in semisuper_cycleGAN.evaluate; None = the reference's
        single forward and plain first maximum.  `boundary`: a F.BoundaryOptions, as in semisuper_cycleGAN.evaluate (the scores are
        kept in `self.eval_boundary`); None = off.  set_sliding(): sliding-window inference, as in semisuper_cycleGAN.evaluate."""
        sliding = self.get_sliding()
        if sliding is not None and tta:
            raise ValueError("evaluate: sliding-window inference does not combine with tta (its own key 'flip' mirrors the windows)")
        self.Gsi.eval()
        self.running_metrics_val.reset()
        self.running_metrics_val.set_boundary(boundary)
        self.running_metrics_val.check_calibration(tta, crf, sliding=sliding)      # --calibration: a temperature grid needs the single fused head
        calibrated = self.running_metrics_val.get_calibration() is not None
        for val_img, val_gt, _ in val_loader:
            val_img, val_gt = utils.cuda([val_img, val_gt], self.args.gpu_ids)
            if first_batch is not None and not first_batch:
                first_batch.extend((val_img, val_gt))
            if sliding is not None:         # overlapping crop-sized windows over the batch's own size, blended into one label map
                self._evaluate_sliding(val_img, val_gt, sliding, crf)
                continue
            if crf is not None:             # the windowed dense CRF between the softmax and the first maximum, guided by the batch
                scores, probs = utils.crf_scores(self.Gsi, val_img, self.crop, tta)
                self.running_metrics_val.update_logits_crf(val_gt.squeeze(1), scores, utils.crf_guide(val_img, self.crop), self.crop, crf,
                                                           probs=probs)
                continue
            if tta:
                self.running_metrics_val.update_logits_ms(val_gt.squeeze(1), *utils.tta_logits(self.Gsi, val_img, tta), self.crop)
                continue
            logits = self.Gsi(val_img)
            if F.FUSE_PREDICT[0]:
                self.running_metrics_val.update_logits(val_gt.squeeze(1), logits, self.crop)
                continue
            outputs = F.softmax2d(F.upsample_bilinear(logits, self.crop))
            if calibrated:                   # --calibration on the chain of separate passes: the softmax map itself is scored
                self.running_metrics_val.update_probs(val_gt.squeeze(1), outputs)
            self.running_metrics_val.update_device(val_gt.squeeze(1), F.argmax_index(outputs))
        score, class_iou = self.running_metrics_val.get_scores()
        self._dice_scores(self.running_metrics_val)
        self._boundary_scores(self.running_metrics_val)
        self._surface_scores(self.running_metrics_val)
        self._component_scores(self.running_metrics_val)
        self._calibration_scores(self.running_metrics_val)
        self.running_metrics_val.reset()
        self.Gsi.train()
        return score["Mean IoU : \t"], class_iou

    @_with_ema("gsi_optimizer")
    @torch.no_grad()
    def panels(self, val_img, val_gt):
        """The two image grids of model.py:164-186 (prediction, ground truth) from one validation batch: tag -> uint8 [3,GH,GW]
        numpy array.  Gsi runs in eval mode and returns to the mode it was in; nothing else changes."""
        mode = self.Gsi.training
        self.Gsi.eval()
        try:
            ids, _ = _panel_ids(self.Gsi(val_img), self.crop, self.n_channels, False)           # :168-171
            return _panel_arrays(self.args.dataset, list(zip(SUPERVISED_PANEL_TAGS, (F.PANEL_COLOUR, F.PANEL_GREY), (ids, val_gt.long()))))
        finally:
            self.Gsi.train(mode)

    def train(self, args, loaders=None, max_steps=None, writer=None, panel_dir=None):
        rank = self.dp.rank if self.dp is not None else 0
        if loaders is None:
            from .data import synthetic_loaders
            loaders = synthetic_loaders(args, self.n_channels, rank=rank)
        labeled_loader = loaders[0]
        self.resolve_ce_weights(labeled_loader)
        val_loader = loaders[2] if len(loaders) > 2 else None
        history, done = [], 0
        self.set_surface(utils.parse_surface(getattr(args, 'surface', '')))
        self.set_components(utils.parse_components(getattr(args, 'components', '')))
        sliding = utils.parse_sliding(getattr(args, 'sliding', ''), self.crop)
        self.set_sliding(sliding)
        self.set_calibration(utils.parse_calibration(getattr(args, 'calibration', '')), tta=utils.parse_tta(getattr(args, 'tta', '')),
                             crf=utils.parse_crf(getattr(args, 'crf', '')), sliding=sliding)
        for epoch in range(self.start_epoch, args.epochs):
            self.set_boundary_epoch(epoch)
            self.Gsi.train()
            for i, (l_img, l_gt, _) in enumerate(labeled_loader):
                l_img, l_gt = utils.cuda([l_img, l_gt], args.gpu_ids)
                loss = float(self.step(l_img, l_gt))
                history.append(loss)
                if rank == 0:
                    print("Epoch: (%3d) (%5d/%5d) | Crossentropy Loss:%.2e" % (epoch, i + 1, len(labeled_loader), loss))
                    if self.dice_options is not None:
                        print("Dice Loss:%.2e (weight %g)" % (float(self.extras["dice_loss"]), self.dice_w))
                    if self.boundary_loss_options is not None:
                        print("Boundary Loss:%.2e (weight %g)" % (float(self.extras["boundary_loss"]), self._boundary_b))
                    if self.lovasz_options is not None:
                        print("Lovasz Loss:%.2e (weight %g)" % (float(self.extras["lovasz_loss"]), self.lovasz_w))
                    if self.ohem_options is not None:
                        print("OHEM kept:%.4f of the labelled pixels" % float(self.extras["ohem_kept"]))
                    if self.gsi_optimizer.last_grad_norm is not None:       # --clip_grad_norm: the norm this step's update clipped
                        print("Grad norm:%.3e (clip %.3e)" % (float(self.gsi_optimizer.last_grad_norm), self.gsi_optimizer.max_grad_norm))
                    if writer is not None:                                          # model.py:143
                        writer.add_scalars('Supervised Loss', {'CE Loss ': loss}, len(labeled_loader) * epoch + i)
                done += 1
                if max_steps is not None and done >= max_steps:
                    return history
            if val_loader is not None:                                              # model.py:145-197
                first = [] if rank == 0 and (writer is not None or panel_dir is not None) else None
                with self.gsi_optimizer.ema_weights():  # --ema_decay: the epoch's mIoU and panels are the averaged weights' (one swap)
                    miou, class_iou = self.evaluate(val_loader, first_batch=first, tta=utils.parse_tta(getattr(args, 'tta', '')),
                                                    crf=utils.parse_crf(getattr(args, 'crf', '')),
                                                    boundary=utils.parse_boundary(getattr(args, 'boundary', '')))
                    if rank == 0:
                        print("The mIoU for the epoch is: ", miou)
                        if self.dice_options is not None:
                            print("The mean Dice for the epoch is: ", self.eval_dice["mean_dice"])
                        if hasattr(self, "eval_boundary"):
                            print("The Boundary IoU / trimap mIoU for the epoch are: ", self.eval_boundary["boundary_iou"], self.eval_boundary["trimap_iou"])
                        if hasattr(self, "eval_surface"):
                            print("The HD / HD%d / ASSD / NSD for the epoch are: " % self.running_metrics_val.get_surface().pct,
                                  self.eval_surface["hd"], self.eval_surface["hd95"], self.eval_surface["assd"], self.eval_surface["nsd"])
                        self._print_calibration()
                        if hasattr(self, "eval_components"):
                            print("The components found / kept and the pixels relabelled for the epoch are: ", self.eval_components["components"],
                                  self.eval_components["kept_components"], self.eval_components["removed_pixels"])
                    if first:                                                       # model.py:164-186
                        write_panels(self.panels(*first), epoch, writer, panel_dir)
                if miou >= self.best_iou and rank == 0:
                    self.best_iou, class_iou = utils.checkpoint_scores(miou, class_iou)     # plain numbers: the file loads weights-only
                    ck = {'epoch': epoch + 1, 'Gsi': self.Gsi.state_dict(), 'gsi_optimizer': self.gsi_optimizer.state_dict(),
                          'best_iou': self.best_iou, 'class_iou': class_iou}
                    if self.gsi_optimizer.ema_decay is not None:
                        ck['Gsi_ema'] = self.gsi_optimizer.ema_state_dict(self.Gsi)
                    utils.save_checkpoint(ck, '%s/latest_supervised_model.ckpt' % (self.args.checkpoint_dir))
        return history
