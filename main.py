#!/usr/bin/env python
"""Command line of the reference (main.py:10-87) driving the MI355X build: same flags, same defaults, same
dispatch on --training / --model.  Extra flags (never change a reference default): --synthetic_steps,
--as_written, --augment, --panels, --tta, --ce_weights, --label_smoothing, --clip_grad_norm, --weight_decay, --adamw,
--ema_decay, --dice_weight, --dice_smooth, --dice_skip, --dice_batch, --ohem_thresh, --ohem_min_kept, --ohem_min_frac, --crf, --boundary, --surface, --components,
--calibration, --boundary_loss, --boundary_loss_skip, --boundary_loss_ramp, --ssim_weight, --ssim_window, --ssim_sigma, --unl_entropy, --unl_maxsq, --unl_pseudo, --unl_pseudo_thresh, --unl_ramp, --unl_crf, --unl_crf_kernel, --unl_teacher, --unl_cutmix,
--lovasz_weight, --lovasz_per_image, --lovasz_classes, --lovasz_skip, --sliding.  Multi-GPU: launch with `python -m torch.distributed.run --nproc-per-node N main.py ...`
(one process per MI355X; gradients all-reduced with RCCL).  --augment's items `cutmix=` / `classmix=` mix two samples of a
labelled batch, labels with pixels, inside the device-side batch finish; their class ids are checked against --dataset here."""
import importlib
import os
import sys
from argparse import SUPPRESS, ArgumentParser, Namespace

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
PKG = "semi-supervised-segmentation-cyclegan_amd"

# (flag, type, default) - verbatim from the reference, including its quirks: `type=bool` flags are true for
# ANY non-empty string and the loss weights are type=int with float defaults
FLAGS = [
    ("epochs", int, 400), ("decay_epoch", int, 100), ("batch_size", int, 2), ("lr", float, .0002), ("gpu_ids", str, "0"),
    ("crop_height", int, None), ("crop_width", int, None), ("lamda_img", int, 0.5), ("lamda_gt", int, 0.1),
    ("lamda_perceptual", int, 0), ("lab_CE_weight", int, 1), ("lab_MSE_weight", int, 1), ("lab_perceptual_weight", int, 0),
    ("adversarial_weight", int, 1.0), ("discriminator_weight", int, 1.0), ("training", bool, False), ("testing", bool, False),
    ("validation", bool, False), ("model", str, "supervised_model"), ("results_dir", str, "./results"),
    ("validation_dir", str, "./val_results"), ("checkpoint_dir", str, "./checkpoints/semisupervised_cycleGAN"),
    ("ngf", int, 64), ("ndf", int, 64), ("gen_net", str, "deeplab"), ("dis_net", str, "fc_disc"),
]
DEFAULT_CROP = {"voc2012": (320, 320), "acdc": (256, 256), "cityscapes": (512, 1024)}   # main.py:60-67


DATA_ROOTS = {'voc2012': './data/VOC2012', 'cityscapes': './data/Cityscape', 'acdc': './data/ACDC'}   # model.py:21-23


class _Args(Namespace):
    """Defaults of the opt-in loss and optimiser flags as CLASS attributes (their parser default is SUPPRESS: argparse stores nothing for a flag
    that is not given), so a run that names neither flag parses to the namespace it always did - `vars(args)` lists what the earlier
    flags put there and nothing else - while `args.ce_weights` / `args.label_smoothing` read "" / 0.0 and the optimiser options read
    FusedAdam's own defaults (off)."""
    ce_weights = ""
    label_smoothing = 0.0
    clip_grad_norm = None
    weight_decay = 0.0
    adamw = False
    ema_decay = None
    dice_weight = 0.0
    dice_smooth = 1.0
    dice_skip = ""
    dice_batch = False
    ohem_thresh = None
    ohem_min_kept = 0
    ohem_min_frac = 0.0625
    crf = ""
    boundary = ""
    surface = ""
    components = ""
    calibration = ""
    boundary_loss = 0.0
    boundary_loss_skip = ""
    boundary_loss_ramp = 0
    ssim_weight = 0.0
    ssim_window = 11
    ssim_sigma = 1.5
    unl_entropy = 0.0
    unl_maxsq = 0.0
    unl_pseudo = 0.0
    unl_pseudo_thresh = None        # 0.9 once --unl_pseudo is given
    unl_ramp = 0
    unl_crf = 0.0
    unl_crf_kernel = ""
    unl_teacher = ""
    unl_cutmix = ""
    lovasz_weight = 0.0
    lovasz_per_image = False
    lovasz_classes = "present"
    lovasz_skip = ""
    sliding = ""


def get_args(argv=None):
    parser = ArgumentParser(description="cycleGAN PyTorch (MI355X-native build)")
    for name, typ, default in FLAGS:
        parser.add_argument("--" + name, type=typ, default=default)
    parser.add_argument("--dataset", type=str, choices=["voc2012", "cityscapes", "acdc"], default="voc2012")
    parser.add_argument("--norm", type=str, default="instance", help="instance normalization or batch normalization")
    parser.add_argument("--no_dropout", action="store_true", help="no dropout for the generator")
    # build-only additions
    parser.add_argument("--synthetic_steps", type=int, default=8, help="iterations per epoch of the synthetic loaders")
    parser.add_argument("--as_written", type=int, default=1, help="1: also run the forwards whose outputs the reference never uses")
    parser.add_argument("--data", type=str, choices=["auto", "real", "synthetic"], default="auto",
                        help="real: the datasets under ./data (reference layout); synthetic: seeded random batches; auto: real if present")
    parser.add_argument("--dtype", type=str, choices=["f32", "f32x", "f32s", "bf16", "bf16c"], default="f32",
                        help="f32: the reference's dtype - fp32 tensors; heavy convolutions contract with the fp32-accurate 3-piece "
                             "split-bf16 scheme on the bf16 matrix cores (= f32s), everything else with the exact fp32 MFMA; f32x: exact "
                             "fp32 MFMA everywhere; bf16: bf16 activations / weight operands in HBM, fp32 master weights, statistics and "
                             "losses (BASELINE configs 3/5); bf16c: fp32 tensors, bf16 contractions")
    parser.add_argument("--honour_nets", type=int, default=0,
                        help="1: build the generators / discriminators --gen_net / --dis_net name (the reference ignores both flags)")
    parser.add_argument("--variants", type=str, default="",
                        help="comma list of what the reference has commented out / disabled: l1_cycle, lab_gt_dis, gauss_noise, "
                             "perceptual (weights --lamda_perceptual / --lab_perceptual_weight)")
    parser.add_argument("--vgg_weights", type=str, default=None,
                        help="torchvision VGG16 state dict for --variants perceptual (the reference downloads vgg16(pretrained=True))")
    parser.add_argument("--augment", type=str, default="",
                        help="comma list of geometric and colour augmentations of the labelled and unlabelled training batches, applied "
                             "in one launch inside the device-side batch finish: hflip, rotate=<deg>, scale=<lo>:<hi>, sizedcrop, "
                             "elastic=<alpha>[:<grid>] (a B-spline deformation of the output: control nodes every <grid> output pixels, "
                             "default 32, untuned, each moved by up to <alpha> pixels; alpha <= 0.4 * grid, at most one such item); "
                             "brightness=<x>, contrast=<x>, saturation=<x> (factor in max(0,1-x)..1+x), hue=<x> (0..0.5 of a turn), "
                             "gray=<p> - colour behind geometry, each in the order written, clamped to [0,1] once at the end; "
                             "contrast adds a sum pass for the image mean; cutmix=<p>[:<lo>:<hi>] (with probability p a box of lo..hi of "
                             "the area, default 0.25:0.5, untuned, is pasted from another sample of the batch) and "
                             "classmix=<p>[:<id>[:<id>...]] (with probability p every pixel of a random half of another sample's classes "
                             "is pasted; the listed class ids never are, e.g. classmix=0.5:0 for VOC's background) mix the LABELLED "
                             "batches only, labels with pixels, inside the same launch, at most one item of each (default: none)")
    parser.add_argument("--panels", type=str, default=None, metavar="DIR",
                        help="write the reference's per-epoch image panels (model.py:576-638) to DIR/epoch%%03d_<n>.png, and to a "
                             "tensorboardX.SummaryWriter(DIR) when that module is installed (default: off)")
    parser.add_argument("--tta", type=str, default="", metavar="SPEC",
                        help="multi-scale / mirrored inference in the per-epoch evaluation, --validation and --testing: a comma list "
                             "of input scales, ':flip' adds the mirrored twin of each (e.g. 0.5,0.75,1.0:flip; at most 8 views); the "
                             "views' probabilities are summed (default: one forward at the crop size, as the reference)")
    parser.add_argument("--testing_gen", type=str, default="resnet_9blocks_softmax",
                        help="generator testing.py builds (the reference hard-codes resnet_9blocks_softmax, testing.py:40)")
    parser.add_argument("--ce_weights", type=str, default=SUPPRESS, metavar="SPEC",
                        help="class weights of the ground-truth cross entropies (lab_loss_CE, gt_cycle_loss, the supervised loss): a "
                             "comma list of one weight per class, or a rule computed from the labelled set's class frequencies in one "
                             "pass at start - median (median-frequency balancing) or invlog[:k] (1 / ln(k + f), k = 1.02) "
                             "(default: none, the reference's nn.CrossEntropyLoss())")
    parser.add_argument("--label_smoothing", type=float, default=SUPPRESS, metavar="F",
                        help="label smoothing of the same cross entropies, in [0, 1) (default: 0.0)")
    parser.add_argument("--clip_grad_norm", type=float, default=SUPPRESS, metavar="F",
                        help="clip the global gradient norm to F before every update, as torch.nn.utils.clip_grad_norm_; every "
                             "optimiser clips its own parameters - generators, discriminators, the supervised Gsi (default: off)")
    parser.add_argument("--weight_decay", type=float, default=SUPPRESS, metavar="F",
                        help="weight decay of every optimiser, as torch.optim.Adam(weight_decay=F) (default: 0.0)")
    parser.add_argument("--adamw", action="store_true", default=SUPPRESS,
                        help="apply --weight_decay decoupled from the gradient, as torch.optim.AdamW")
    parser.add_argument("--ema_decay", type=float, default=SUPPRESS, metavar="F",
                        help="keep an exponential moving average of the generators' (the supervised Gsi's) weights with decay F in "
                             "[0, 1); the per-epoch evaluation, the panels, --validation and --testing use it and checkpoints gain "
                             "Gsi_ema / Gis_ema (default: off)")
    parser.add_argument("--dice_weight", type=float, default=SUPPRESS, metavar="F",
                        help="add F times the soft Dice loss to every ground-truth cross entropy (lab_loss_CE, gt_cycle_loss, the "
                             "supervised loss), inside that term's own weight: L + F * Dice of the same resized logits; reported as "
                             "lab_loss_dice / gt_cycle_dice / dice_loss, and the evaluation also scores the mean and per-class Dice; "
                             "F >= 0, 0 = off (default: off, the reference's losses)")
    parser.add_argument("--dice_smooth", type=float, default=SUPPRESS, metavar="F",
                        help="the smoothing constant s > 0 of the Dice ratio (2 I + s) / (P + T + s) (default: 1.0)")
    parser.add_argument("--dice_skip", type=str, default=SUPPRESS, metavar="LIST",
                        help="comma list of class ids the Dice loss leaves out (weight 0), e.g. 0 for VOC's background, 19 for the "
                             "Cityscapes void class - the classes the mIoU drops (default: none)")
    parser.add_argument("--dice_batch", action="store_true", default=SUPPRESS,
                        help="one Dice per class over the whole batch instead of one per sample and class (per rank under data "
                             "parallelism)")
    parser.add_argument("--ohem_thresh", type=float, default=SUPPRESS, metavar="F",
                        help="online hard example mining of the same cross entropies: a labelled pixel takes part when the probability "
                             "of its true class is at most F, in (0, 1], and the --ohem_min_kept / --ohem_min_frac hardest pixels of a "
                             "batch always do (per head and per rank); the kept share is reported as lab_ohem_kept / "
                             "gt_cycle_ohem_kept / ohem_kept (default: off, every labelled pixel takes part)")
    parser.add_argument("--ohem_min_kept", type=int, default=SUPPRESS, metavar="N",
                        help="with --ohem_thresh: at least N pixels of a batch are kept, N >= 0 (default: 0)")
    parser.add_argument("--ohem_min_frac", type=float, default=SUPPRESS, metavar="F",
                        help="with --ohem_thresh: at least the share F, in [0, 1], of a batch's labelled pixels is kept (default: 0.0625)")
    parser.add_argument("--crf", type=str, default=SUPPRESS, metavar="SPEC",
                        help="refine the predicted label maps of the per-epoch evaluation, --validation and --testing with a windowed "
                             "dense CRF guided by the input image: 'on' for the (untuned) defaults, or a comma list of key=value over "
                             "iters, radius, dilation, wb, ws, alpha, beta, gamma (e.g. iters=5,radius=3,dilation=2,wb=4,ws=3,alpha=8,"
                             "beta=0.5,gamma=3); with --tta it runs on the views' summed probabilities (default: off, the plain argmax)")
    parser.add_argument("--boundary", type=str, default=SUPPRESS, metavar="SPEC",
                        help="also score the per-epoch evaluation's label maps near object contours: the Boundary IoU (Cheng et al., "
                             "CVPR 2021) and the trimap mIoU of the DeepLab papers, printed beside the mIoU; 'on' for the published "
                             "width (0.02 of the image diagonal), d=N for N pixels (1..32), or ratio=F of the diagonal; combines with "
                             "--tta, --crf and --ema_decay (default: off, region scores only)")
    parser.add_argument("--surface", type=str, default=SUPPRESS, metavar="SPEC",
                        help="also score the per-epoch evaluation's label maps by their surface distances per sample and class: the "
                             "Hausdorff distance, its percentile (HD95), the average symmetric surface distance and the normalised "
                             "surface Dice, in pixels, printed beside the mIoU; 'on' for tol=2,pct=95, or a comma list over tol=F (the "
                             "NSD tolerance) and pct=N (1..100); combines with --tta, --crf, --boundary and --ema_decay (default: off)")
    parser.add_argument("--components", type=str, default=SUPPRESS, metavar="SPEC",
                        help="filter the predicted label maps of the evaluation, validation and testing by connected components "
                             "before they are scored or saved: per sample and class keep only the largest component ('largest') and / "
                             "or the components of at least N pixels ('min_area=N'), relabel the rest as class K ('fill=K', default 0); "
                             "'conn=4|8' (default 8), 'skip=a:b:c' for classes never filtered; 'on' for min_area=64 (an untuned "
                             "default); e.g. largest,min_area=16,skip=3; combines with --tta, --crf, --boundary, --surface and "
                             "--ema_decay (default: off, the maps are scored as predicted)")
    parser.add_argument("--calibration", type=str, default=SUPPRESS, metavar="SPEC",
                        help="also score the per-epoch evaluation's (and --validation's) probabilities by their calibration: the "
                             "expected and maximum calibration error over a reliability diagram, the negative log-likelihood, the "
                             "Brier score, the per-class confidence gap and the accuracy / coverage above every confidence threshold "
                             "(what --unl_pseudo_thresh would keep), printed beside the mIoU; 'on' for bins=15 at temperature 1, "
                             "'fit' for bins=15,temps=0.5:3.0:7, which also fits the NLL-optimal temperature (both untuned defaults), "
                             "or a comma list over bins=N (2..32) and temps=lo:hi:n (log-spaced) or temps=a/b/c; temperature 1 is "
                             "always scored, at most 8 with it; a temperature list does not combine with --tta or --crf; it scores "
                             "the prediction before --components; --testing has no ground truth and ignores it (default: off)")
    parser.add_argument("--boundary_loss", type=float, default=SUPPRESS, metavar="F",
                        help="add F times the boundary loss of Kervadec et al. (MIDL 2019) to every ground-truth cross entropy "
                             "(lab_loss_CE, gt_cycle_loss, the supervised loss), inside that term's own weight: the softmax "
                             "probabilities times the signed distance to the ground-truth contour of each class, computed on the "
                             "device; reported as lab_loss_boundary / gt_cycle_boundary / boundary_loss (it may be negative); "
                             "combines with --ce_weights, --label_smoothing, --dice_weight and --ohem_thresh; F >= 0, 0 = off "
                             "(default: off, the reference's losses)")
    parser.add_argument("--boundary_loss_skip", type=str, default=SUPPRESS, metavar="LIST",
                        help="comma list of class ids the boundary loss leaves out (weight 0), as --dice_skip (default: none)")
    parser.add_argument("--boundary_loss_ramp", type=int, default=SUPPRESS, metavar="N",
                        help="raise the boundary term's weight linearly over the first N epochs, F * min(1, epoch / N); N >= 0, "
                             "0 = constant (default: 0)")
    parser.add_argument("--ssim_weight", type=float, default=SUPPRESS, metavar="F",
                        help="add F times the structural-similarity loss 1 - mean SSIM (Wang et al. 2004) to every image L1 term "
                             "(lab_loss_MSE; img_cycle_l1 under --variants l1_cycle), inside that term's own weight, from the same "
                             "forward and backward launch as the L1; reported as lab_loss_ssim / img_cycle_ssim; the supervised "
                             "model has no image term and ignores it; F >= 0, 0 = off (default: off, the reference's losses)")
    parser.add_argument("--ssim_window", type=int, default=SUPPRESS, metavar="N",
                        help="side of the SSIM term's Gaussian window: odd, 3..11, at most the crop (default: 11)")
    parser.add_argument("--ssim_sigma", type=float, default=SUPPRESS, metavar="F",
                        help="standard deviation of the SSIM term's Gaussian window, > 0 (default: 1.5)")
    parser.add_argument("--unl_entropy", type=float, default=SUPPRESS, metavar="F",
                        help="add F times the entropy of the UNLABELLED batch's prediction to the generator loss (entropy "
                             "minimisation, Grandvalet & Bengio 2004; ADVENT's MinEnt): the mean over its pixels of the softmax "
                             "entropy divided by ln C, from the unlabelled head's own forward and backward; reported as unl_entropy; "
                             "the supervised model has no unlabelled batch and ignores it; F >= 0, 0 = off (default: off)")
    parser.add_argument("--unl_maxsq", type=float, default=SUPPRESS, metavar="F",
                        help="add F times the maximum-squares loss (Chen et al., ICCV 2019) of the same prediction, the mean of "
                             "-sum_c p_c^2 / 2; reported as unl_maxsq; F >= 0, 0 = off (default: off)")
    parser.add_argument("--unl_pseudo", type=float, default=SUPPRESS, metavar="F",
                        help="add F times the cross entropy of the same prediction against its own argmax, over the pixels whose "
                             "maximum probability is at least --unl_pseudo_thresh (self-training, Lee 2013; per rank); reported as "
                             "unl_pseudo_ce, the kept share as unl_pseudo_kept; F >= 0, 0 = off (default: off)")
    parser.add_argument("--unl_pseudo_thresh", type=float, default=SUPPRESS, metavar="T",
                        help="with --unl_pseudo: the confidence threshold, in [0, 1] (default: 0.9)")
    parser.add_argument("--unl_ramp", type=int, default=SUPPRESS, metavar="N",
                        help="raise the three --unl_* weights linearly over the first N epochs, F * min(1, epoch / N); N >= 0, "
                             "0 = constant (default: 0)")
    parser.add_argument("--unl_crf", type=float, default=SUPPRESS, metavar="F",
                        help="add F times the gated CRF loss (Tang et al., ECCV 2018; Obukhov et al., 2019) of the UNLABELLED batch's "
                             "prediction to the generator loss: nearby pixels of similar colour in the unlabelled image that are "
                             "predicted differently are penalised, the mean over the pixels of sum_j k(i, j) (1 - p(i) . p(j)) with "
                             "--crf's pairwise kernel; the training-side counterpart of --crf; reported as unl_crf; --unl_ramp "
                             "applies; the supervised model ignores it; F >= 0, 0 = off (default: off)")
    parser.add_argument("--unl_crf_kernel", type=str, default=SUPPRESS, metavar="SPEC",
                        help="with --unl_crf: the pairwise kernel in --crf's grammar, a comma list of key=value over radius, dilation, "
                             "wb, ws, alpha, beta, gamma ('iters' is accepted and ignored), or 'on' (default: --crf's defaults, "
                             "untuned for training)")
    parser.add_argument("--unl_teacher", type=str, default=SUPPRESS, metavar="SPEC",
                        help="mean-teacher consistency on the UNLABELLED batch (Tarvainen & Valpola 2017; French et al. 2020): a "
                             "teacher - the same Gsi under --ema_decay's averaged weights, in evaluation mode - predicts the same "
                             "images and the student is pulled towards it where the teacher's confidence is at least thresh; a comma "
                             "list over mse=F (weight of the squared distance of the two probability maps), ce=F (weight of the cross "
                             "entropy against the teacher's hard labels, FixMatch's form; not with --unl_pseudo), thresh=T in [0, 1] "
                             "(default 0), temp=T > 0 (the teacher's softmax temperature, default 1) and flip (the teacher sees each "
                             "sample mirrored with probability 1/2), or 'on' for mse=1 (an untuned default); needs --ema_decay; "
                             "reported as unl_teacher_mse / unl_teacher_ce with the kept share unl_teacher_kept and the agreement "
                             "unl_teacher_agree; --unl_ramp applies; the supervised model ignores it (default: off)")
    parser.add_argument("--unl_cutmix", type=str, default=SUPPRESS, metavar="SPEC",
                        help="with --unl_teacher: CutMix consistency (French et al. 2020) - the teacher predicts the unlabelled batch "
                             "as it is, then every sample of it takes, with probability p, a box of a partner sample, and the student, "
                             "which sees the mixed batch from there on, is held to the same mix of the teacher's two predictions; SPEC "
                             "= p[:lo:hi] in the grammar of --augment cutmix=: 0 < p <= 1, the box's share of the area in lo..hi "
                             "(default 0.25:0.5, untuned); the unlabelled images must have the crop's size; a batch of one is never "
                             "mixed; reported as unl_cutmix_share, the pasted share of the batch's pixels; the supervised model "
                             "ignores it (default: off)")
    parser.add_argument("--lovasz_weight", type=float, default=SUPPRESS, metavar="F",
                        help="add F times the Lovasz-softmax loss (Berman et al., CVPR 2018), the mIoU surrogate, to every "
                             "ground-truth cross entropy (lab_loss_CE, gt_cycle_loss, the supervised loss), inside that term's own "
                             "weight: per class the errors |[y == c] - p_c| sorted on the device and weighted by the gradient of the "
                             "Jaccard index; reported as lab_loss_lovasz / gt_cycle_lovasz / lovasz_loss; per rank under data "
                             "parallelism; combines with --ce_weights, --label_smoothing, --dice_weight, --ohem_thresh and "
                             "--boundary_loss; F >= 0, 0 = off (default: off, the reference's losses)")
    parser.add_argument("--lovasz_per_image", action="store_true", default=SUPPRESS,
                        help="one Lovasz loss per sample, averaged over the samples with a labelled pixel (default: the batch is "
                             "one segment)")
    parser.add_argument("--lovasz_classes", type=str, choices=["present", "all"], default=SUPPRESS,
                        help="average the Lovasz loss over the classes present in the segment, or over all (default: present)")
    parser.add_argument("--lovasz_skip", type=str, default=SUPPRESS, metavar="LIST",
                        help="comma list of class ids the Lovasz loss leaves out, as --dice_skip (default: none)")
    parser.add_argument("--sliding", type=str, default=SUPPRESS, metavar="SPEC",
                        help="sliding-window inference in the per-epoch evaluation, --validation and --testing: the val / test images "
                             "are kept at a larger evaluation size instead of being resized to the crop, the network runs on "
                             "overlapping crop-sized windows and the windows' probabilities are blended with a centre-weighted map; "
                             "'on' for scale=2,overlap=0.5,blend=gauss (an untuned default), or a comma list over size=HxW or scale=F "
                             "(exactly one: the evaluation size, at least the crop), overlap=F (0..0.75, default 0.5), "
                             "blend=gauss|const, sigma=F (of the window, default 0.125, untuned) and flip (every window also mirrored); "
                             "at most 16 windows per axis; combines with --crf, --components, --boundary, --surface, --calibration "
                             "(temperature 1) and --ema_decay, not with --tta or --panels (default: off, the images are the crop)")
    args = parser.parse_args(argv, namespace=_Args())
    if args.crf.strip():
        try:
            importlib.import_module(PKG + ".utils").parse_crf(args.crf)
        except ValueError as e:
            parser.error(str(e))
    if args.boundary.strip():
        try:
            importlib.import_module(PKG + ".utils").parse_boundary(args.boundary)
        except ValueError as e:
            parser.error(str(e))
    if args.surface.strip():
        try:
            importlib.import_module(PKG + ".utils").parse_surface(args.surface)
        except ValueError as e:
            parser.error(str(e))
    if args.components.strip():
        try:
            importlib.import_module(PKG + ".utils").parse_components(args.components).exempt_mask(
                {"voc2012": 21, "cityscapes": 20, "acdc": 4}[args.dataset])
        except ValueError as e:
            parser.error("--components: %s" % e if not str(e).startswith("--components") else str(e))
    if args.calibration.strip():
        try:
            cal = importlib.import_module(PKG + ".utils").parse_calibration(args.calibration)
        except ValueError as e:
            parser.error(str(e))
        if len(cal.temps) > 1 and (getattr(args, "tta", "").strip() or args.crf.strip()):
            parser.error("--calibration: a temperature list rescales the logits of the single fused head and does not combine with "
                         "--tta or --crf")
    for item in (s.strip() for s in args.augment.split(",")):
        if item.partition("=")[0] == "classmix":
            n_cls = {"voc2012": 21, "cityscapes": 20, "acdc": 4}[args.dataset]
            if not all(t.isdigit() and int(t) < n_cls for t in item.partition("=")[2].split(":")[1:]):
                parser.error("--augment classmix=<p>[:<id>...] skips class ids in [0, %d), given %r" % (n_cls, item))
    if args.ohem_thresh is not None and not 0.0 < args.ohem_thresh <= 1.0:
        parser.error("--ohem_thresh must lie in (0, 1]")
    if args.ohem_min_kept < 0:
        parser.error("--ohem_min_kept must be >= 0")
    if not 0.0 <= args.ohem_min_frac <= 1.0:
        parser.error("--ohem_min_frac must lie in [0, 1]")
    if args.ohem_thresh is None and ("ohem_min_kept" in vars(args) or "ohem_min_frac" in vars(args)):
        parser.error("--ohem_min_kept / --ohem_min_frac need --ohem_thresh F")
    if not args.dice_weight >= 0.0 or args.dice_weight == float("inf"):
        parser.error("--dice_weight must be a finite number >= 0")
    if not (args.dice_smooth > 0.0 and args.dice_smooth < float("inf")):
        parser.error("--dice_smooth must be a finite number > 0")
    if args.dice_skip.strip():
        toks = [t.strip() for t in args.dice_skip.split(",")]
        n_cls = {"voc2012": 21, "cityscapes": 20, "acdc": 4}[args.dataset]
        if not all(t.isdigit() and int(t) < n_cls for t in toks) or len(set(int(t) for t in toks)) >= n_cls:
            parser.error("--dice_skip must be a comma list of class ids in [0, %d) that leaves a class over" % n_cls)
    if not args.boundary_loss >= 0.0 or args.boundary_loss == float("inf"):
        parser.error("--boundary_loss must be a finite number >= 0")
    if args.boundary_loss_ramp < 0:
        parser.error("--boundary_loss_ramp must be an integer >= 0")
    if args.boundary_loss_skip.strip():
        toks = [t.strip() for t in args.boundary_loss_skip.split(",")]
        n_cls = {"voc2012": 21, "cityscapes": 20, "acdc": 4}[args.dataset]
        if not all(t.isdigit() and int(t) < n_cls for t in toks) or len(set(int(t) for t in toks)) >= n_cls:
            parser.error("--boundary_loss_skip must be a comma list of class ids in [0, %d) that leaves a class over" % n_cls)
    if not args.ssim_weight >= 0.0 or args.ssim_weight == float("inf"):
        parser.error("--ssim_weight must be a finite number >= 0")
    if not 3 <= args.ssim_window <= 11 or args.ssim_window % 2 == 0:
        parser.error("--ssim_window must be an odd integer in 3..11")
    if not (args.ssim_sigma > 0.0 and args.ssim_sigma < float("inf")):
        parser.error("--ssim_sigma must be a finite number > 0")
    for key in ("unl_entropy", "unl_maxsq", "unl_pseudo"):
        if not getattr(args, key) >= 0.0 or getattr(args, key) == float("inf"):
            parser.error("--%s must be a finite number >= 0" % key)
    if args.unl_pseudo_thresh is not None:
        if not args.unl_pseudo > 0.0:
            parser.error("--unl_pseudo_thresh needs --unl_pseudo F with F > 0")
        if not 0.0 <= args.unl_pseudo_thresh <= 1.0:
            parser.error("--unl_pseudo_thresh must lie in [0, 1]")
    if args.unl_ramp < 0:
        parser.error("--unl_ramp must be an integer >= 0")
    if not args.unl_crf >= 0.0 or args.unl_crf == float("inf"):
        parser.error("--unl_crf must be a finite number >= 0")
    if args.unl_crf_kernel.strip():
        if not args.unl_crf > 0.0:
            parser.error("--unl_crf_kernel needs --unl_crf F with F > 0")
        try:
            importlib.import_module(PKG + ".utils").parse_unl_crf_kernel(args.unl_crf_kernel)
        except ValueError as e:
            parser.error(str(e))
    if args.unl_teacher.strip():
        try:
            teacher = importlib.import_module(PKG + ".utils").parse_unl_teacher(args.unl_teacher)
        except ValueError as e:
            parser.error(str(e))
        if args.ema_decay is None:
            parser.error("--unl_teacher needs --ema_decay: the teacher is the averaged weights")
        if teacher.ce > 0.0 and args.unl_pseudo > 0.0:
            parser.error("--unl_teacher ce= and --unl_pseudo are the same term from two label sources: give one")
    if args.unl_cutmix.strip():
        try:
            importlib.import_module(PKG + ".utils").parse_unl_cutmix(args.unl_cutmix)
        except ValueError as e:
            parser.error(str(e))
        if not args.unl_teacher.strip() or args.ema_decay is None:
            parser.error("--unl_cutmix needs --unl_teacher (and with it --ema_decay): it mixes what the teacher and the student see")
    if not args.lovasz_weight >= 0.0 or args.lovasz_weight == float("inf"):
        parser.error("--lovasz_weight must be a finite number >= 0")
    if args.lovasz_skip.strip():
        toks = [t.strip() for t in args.lovasz_skip.split(",")]
        n_cls = {"voc2012": 21, "cityscapes": 20, "acdc": 4}[args.dataset]
        if not all(t.isdigit() and int(t) < n_cls for t in toks) or len(set(int(t) for t in toks)) >= n_cls:
            parser.error("--lovasz_skip must be a comma list of class ids in [0, %d) that leaves a class over" % n_cls)
    if args.adamw and not args.weight_decay > 0.0:
        parser.error("--adamw decouples the weight decay from the gradient: it needs --weight_decay F with F > 0")
    if args.weight_decay < 0.0 or args.weight_decay != args.weight_decay:
        parser.error("--weight_decay must be >= 0")
    if args.clip_grad_norm is not None and not args.clip_grad_norm > 0.0:
        parser.error("--clip_grad_norm must be > 0")
    if args.ema_decay is not None and not 0.0 <= args.ema_decay < 1.0:
        parser.error("--ema_decay must lie in [0, 1)")
    return args


def check_sliding(args):
    """--sliding against the crop (known once the dataset's default is in) and the options it does not combine with: ValueError."""
    if not args.sliding.strip():
        return None
    utils = importlib.import_module(PKG + ".utils")
    opts = utils.parse_sliding(args.sliding, (args.crop_height, args.crop_width))
    if getattr(args, "tta", "").strip():
        raise ValueError("--sliding does not combine with --tta: multi-scale windows are not built; 'flip' is --sliding's own key")
    if args.panels:
        raise ValueError("--sliding does not combine with --panels: the panels are drawn at the crop size")
    if args.calibration.strip() and len(utils.parse_calibration(args.calibration).temps) > 1:
        raise ValueError("--sliding does not combine with a --calibration temperature list: the blended probabilities are not one "
                         "softmax of logits that could be rescaled; ask for temperature 1 only")
    return opts


def main(argv=None):
    args = get_args(argv)
    args.gpu_ids = [int(s) for s in args.gpu_ids.split(",") if int(s) >= 0]
    args.as_written = bool(args.as_written)
    args.overlap_d = True                # train() reads the losses after sync_losses()
    if args.crop_height is None and args.crop_width is None:
        args.crop_height, args.crop_width = DEFAULT_CROP[args.dataset]
    check_sliding(args)
    if args.gpu_ids:
        import torch
        torch.cuda.set_device(args.gpu_ids[0])          # arch/ops.py:31-34: everything lives on gpu_ids[0]
    md = importlib.import_module(PKG + ".model")
    importlib.import_module(PKG + ".functional").set_conv_precision(args.dtype)
    dp = None
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        par = importlib.import_module(PKG + ".parallel")
        dp = par.DataParallel()
        args.gpu_ids = [dp.device_index]
    if args.training:
        loaders = None
        root = DATA_ROOTS[args.dataset]
        if args.data == "real" or (args.data == "auto" and os.path.isdir(root)):
            import torch
            du = importlib.import_module(PKG + ".data_utils")
            loaders = du.build_loaders(args, roots=DATA_ROOTS, device=torch.device("cuda", args.gpu_ids[0]),
                                       rank=dp.rank if dp is not None else 0)
        else:
            print("no dataset under %s: training on synthetic batches (--synthetic_steps per epoch)" % root)
        writer = None
        if args.panels:
            try:
                from tensorboardX import SummaryWriter
                writer = SummaryWriter(args.panels)
            except ImportError:
                print("tensorboardX is not installed: the panels go to %s as PNG files only" % args.panels)
        if args.model == "semisupervised_cycleGAN":
            print("Training semi-supervised cycleGAN")
            md.semisuper_cycleGAN(args, data_parallel=dp).train(args, loaders=loaders, writer=writer, panel_dir=args.panels)
        if args.model == "supervised_model":
            print("Training base model")
            md.supervised_model(args, data_parallel=dp).train(args, loaders=loaders, writer=writer, panel_dir=args.panels)
    if args.testing:                                        # main.py:69-71
        print("Testing")
        import testing
        testing.test(args)
    if args.validation:                                     # main.py:72-74
        print("Validating")
        import validation
        validation.validation(args)


if __name__ == "__main__":
    main()
