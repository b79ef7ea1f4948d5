"""Hot-path helpers of the reference's utils.py (make_one_hot :314, Sample_from_Pool :278, cuda :221,
LambdaLR :434, runningScore :357, checkpoint I/O :265-273), re-expressed for a device-resident step:
nothing here moves activations to the host."""
import numpy as np
import torch

from . import functional as F

CLASSES = {"voc2012": 21, "cityscapes": 20, "acdc": 4}   # model.py:205-210, utils.py:335-342


def cuda(xs, gpu_id):
    """utils.cuda (utils.py:221-227): move a tensor / list of tensors to gpu_id[0] when a GPU exists."""
    if torch.cuda.is_available() and len(gpu_id) > 0:
        dev = torch.device("cuda", int(gpu_id[0]))
        if not isinstance(xs, (list, tuple)):
            return xs.to(dev, non_blocking=True)
        return [x.to(dev, non_blocking=True) for x in xs]
    return xs


def make_one_hot(labels, dataname, gpu_id=None):
    """Integer labels [N,1,H,W] -> fp32 one-hot [N,C,H,W] (utils.py:314-350), one HIP pass."""
    assert dataname in CLASSES, "dataset name should be one of the following: 'voc2012',given {}".format(dataname)
    return F.label_onehot(labels.long(), CLASSES[dataname])


class Sample_from_Pool(object):
    """History pool of Shrivastava et al. (utils.py:278-299): `max_elements` slots; once full, with p=0.5 a
    random stored item is returned and replaced.  Items stay on the device (the reference round-trips three
    activation batches through numpy every step, model.py:490-495); the host RNG calls (np.random.ranf /
    randint) are the reference's, so a seeded run makes the same decisions."""

    def __init__(self, max_elements=50):
        self.max_elements = max_elements
        self.cur_elements = 0
        self.items = []

    def __call__(self, in_items):
        out = []
        for item in in_items:
            if self.cur_elements < self.max_elements:
                self.items.append(item)
                self.cur_elements += 1
                out.append(item)
            elif np.random.ranf() > 0.5:
                idx = np.random.randint(0, self.max_elements)
                out.append(self.items[idx])
                self.items[idx] = item
            else:
                out.append(item)
        return out


class GaussianNoise(object):
    """utils.GaussianNoise (utils.py:116-140): x + sigma * x.detach() * N(0,1) in training mode - the (dead) noise branch of
    the discriminator step, model.py:486-488.  Device-resident: the reference moves the batch to the CPU first."""

    def __init__(self, sigma=0.1, is_relative_detach=True):
        self.sigma, self.is_relative_detach, self.training = sigma, is_relative_detach, True
        self._calls = 0

    def __call__(self, x):
        if self.training and self.sigma != 0:
            self._calls += 1
            seed = (torch.initial_seed() * 0x9E3779B1 + self._calls) & 0x7FFFFFFFFFFFFFF
            return F.gauss_noise(x.detach(), self.sigma, seed)
        return x


class _MaxPool2(torch.nn.Module):
    """nn.MaxPool2d(kernel_size=2, stride=2) (torchvision VGG16 features[4, 9, 16, 23])."""

    def forward(self, x):
        return F.maxpool2x2(x)


class Vgg16(torch.nn.Module):
    """utils.py:145-177: the first 23 layers of torchvision's VGG16 `features`, cut into four slices (relu1_2, relu2_2, relu3_3,
    relu4_3); state-dict keys `slice{1..4}.{features index}.{weight,bias}`.  The reference loads `vgg16(pretrained=True)`; there is
    no network here, so the weights are He-initialised unless `weights` names a torchvision VGG16 state dict (`features.N.*`)."""

    _LAYOUT = (("slice1", ((0, 3, 64), (2, 64, 64))),
               ("slice2", ((4, None, None), (5, 64, 128), (7, 128, 128))),
               ("slice3", ((9, None, None), (10, 128, 256), (12, 256, 256), (14, 256, 256))),
               ("slice4", ((16, None, None), (17, 256, 512), (19, 512, 512), (21, 512, 512))))

    def __init__(self, requires_grad=False, weights=None):
        super().__init__()
        from .arch import ops
        for name, layers in self._LAYOUT:
            seq = ops.FusedSequential()
            for idx, cin, cout in layers:
                if cin is None:
                    seq.add_module(str(idx), _MaxPool2())
                else:
                    conv = ops.Conv2d(cin, cout, 3, 1, 1)
                    conv.head = True          # the features stay fp32 in bf16 mode (they feed a loss)
                    with torch.no_grad():
                        conv.weight.copy_(torch.empty(conv.weight.shape).normal_(0.0, (2.0 / (cin * 9)) ** 0.5))
                    seq.add_module(str(idx), conv)
                    seq.add_module(str(idx + 1), ops.ReLU(True))
            setattr(self, name, seq)
        if weights is None:
            # the reference always loads the ImageNet weights (utils.py:149): without them the loss is finite but not the
            # reference's perceptual loss - say so, once per construction
            print("**perceptual loss: no --vgg_weights given, VGG16 is He-initialised (NOT the reference's pretrained features)**")
        if weights is not None:
            sd = torch.load(weights, map_location="cpu") if isinstance(weights, str) else weights
            own = self.state_dict()
            for k in own:
                own[k] = sd["features." + k.split(".", 1)[1]]
            self.load_state_dict(own, strict=True)
        if not requires_grad:
            for p in self.parameters():
                p.requires_grad = False

    def forward(self, x):
        h1 = self.slice1(x)
        h2 = self.slice2(h1)
        h3 = self.slice3(h2)
        h4 = self.slice4(h3)
        return {"relu1_2": h1, "relu2_2": h2, "relu3_3": h3, "relu4_3": h4}

    def relu2_2(self, x):
        return self.slice2(self.slice1(x))


_TRANS_MEAN = (0.485, 0.456, 0.406)
_TRANS_STD = (0.229, 0.224, 0.225)


def perceptual_loss(x, y, gpu_ids=None, vgg=None):
    """utils.py:181-208 as written: u = x / 2 + 1 / 2, then per channel u * std + mean (sic: the reference multiplies by the
    ImageNet std and adds the mean), both images through VGG16 up to relu2_2, nn.MSELoss between the features.
    `vgg`: a Vgg16 to reuse (the reference builds - and downloads - a new one on every call)."""
    dev = x.device
    if vgg is None:
        vgg = Vgg16(requires_grad=False).to(dev)
    a = torch.tensor([0.5 * s for s in _TRANS_STD], device=dev)
    b = torch.tensor([0.5 * s + m for s, m in zip(_TRANS_STD, _TRANS_MEAN)], device=dev)
    zero, one = torch.zeros(3, device=dev), torch.full((3,), 1.0 - 1e-5, device=dev)

    def prep(t):        # per-channel affine = the eval-mode BatchNorm kernel with mean 0, var + eps = 1
        return F.batch_norm_act(t, a, b, zero, one, False, 0.0, 1e-5)

    return F.mse_loss(vgg.relu2_2(prep(y)), vgg.relu2_2(prep(x)))


class LambdaLR():
    """Linear decay to zero after `decay_epoch` (utils.py:434-441)."""

    def __init__(self, epochs, offset, decay_epoch):
        self.epochs, self.offset, self.decay_epoch = epochs, offset, decay_epoch

    def step(self, epoch):
        return 1.0 - max(0, epoch + self.offset - self.decay_epoch) / (self.epochs - self.decay_epoch)


class runningScore(object):
    """Confusion-matrix mIoU (utils.py:357-412).  VOC ignores class 0, Cityscapes the last class, ACDC none."""

    def __init__(self, n_classes, dataset):
        self.n_classes, self.dataset = n_classes, dataset
        self.confusion_matrix = np.zeros((n_classes, n_classes))
        self._device_hist = None     # int64 [C, C] accumulated by sscg_confusion_hist; folded in by get_scores()
        self._boundary = None        # set_boundary(): a F.BoundaryOptions, or None = no contour scores, no launch for them
        self._boundary_counts = None    # int64 [3 C + C C] accumulated by sscg_boundary_counts while the option is set
        self._surface = None         # set_surface(): a F.SurfaceOptions, or None = no surface distances, no launch for them
        self._surface_records = []   # per update_* call (stats int64 [2, N, C, 5], sums float64 [2, N, C]) on the device
        self._components = None      # set_components(): a F.ComponentOptions, or None = the label maps are scored as predicted
        self._component_stats = []   # per update_* call F.component_filter's stats int64 [N, C, 4] on the device
        self._calibration = None     # set_calibration(): a F.CalibrationOptions, or None = no calibration scores, no launch for them
        self._calibration_state = None  # (bins, cls, sums) accumulated by sscg_calib_stats while the option is set

    def set_boundary(self, boundary):
        """The contour scores (Boundary IoU, trimap mIoU) as STATE of the score keeper: a F.BoundaryOptions (utils.parse_boundary), or an
        integer width d, or None = off.  While set, every update_* on device tensors also asks its head for the uint8 label map and
        hands it to F.boundary_counts; while off, every method launches exactly what it launches without the option."""
        if boundary is not None and not isinstance(boundary, F.BoundaryOptions):
            boundary = F.BoundaryOptions(d=boundary)
        if boundary != self._boundary:
            self._boundary_counts = None
        self._boundary = boundary

    def get_boundary(self):
        return self._boundary

    def set_surface(self, surface):
        """The surface distances (HD, HD95, ASSD, NSD) as STATE of the score keeper: a F.SurfaceOptions (utils.parse_surface), or None =
        off.  While set, every update_* on device tensors also asks its head for the uint8 label map and keeps the call's two small
        record tensors of F.surface_stats; while off, every method launches exactly what it launches without the option."""
        if surface is not None and not isinstance(surface, F.SurfaceOptions):
            raise TypeError("set_surface: a functional.SurfaceOptions or None expected, not %r" % (surface,))
        if surface != self._surface:
            self._surface_records = []
        self._surface = surface

    def get_surface(self):
        return self._surface

    def set_calibration(self, calibration, tta=None, crf=None, sliding=None):
        """The calibration scores (ECE, MCE, NLL, Brier, the per-class gap, the fitted temperature) as STATE of the score keeper: a
        F.CalibrationOptions (utils.parse_calibration), or None = off.  While set, every update_* on logits also hands what its head
        takes the labels from to F.calibration_stats: the logits themselves (update_logits), the views' summed probabilities
        (update_logits_ms, scale 1 / views), the CRF's Q (update_logits_crf), a softmax map (update_probs).  The scores are those of
        the prediction AS THE NETWORK MAKES IT: the component filter changes label maps, not probabilities, and is not seen here.
        A temperature grid rescales logits, which only update_logits has: together with `tta` (a view list), `crf` (a F.CrfOptions) or
        SSCG_FUSE_PREDICT=0 it is refused here (check_calibration), not at the first batch.  While off, every method launches exactly
        what it launches without the option."""
        if calibration is not None and not isinstance(calibration, F.CalibrationOptions):
            raise TypeError("set_calibration: a functional.CalibrationOptions or None expected, not %r" % (calibration,))
        self.check_calibration(tta, crf, calibration, sliding=sliding)
        if calibration != self._calibration:
            self._calibration_state = None
        self._calibration = calibration

    def get_calibration(self):
        return self._calibration

    def check_calibration(self, tta=None, crf=None, calibration=False, sliding=None):
        """Refuse a temperature grid (more than one temperature) where there are no logits to rescale: under multi-scale / mirrored
        inference, behind the CRF and on the chain of separate passes (SSCG_FUSE_PREDICT=0); and, at any temperature, a CRF of 0
        iterations behind several views (it has no Q, and its scores' number of views is not known to update_logits_crf).  evaluate()
        calls it before the first batch.  `calibration`: the option to check instead of the one that is set.  `sliding` (a
        F.SlidingOptions, or True): sliding-window inference blends several softmaxes too, so it is refused like `tta`."""
        opts = self._calibration if calibration is False else calibration
        if opts is None:
            return
        if (tta or sliding) and crf is not None and crf.iterations == 0:
            raise ValueError("calibration: a CRF of 0 iterations behind several views has no Q to score and is those views alone: "
                             "drop the CRF")
        if len(opts.temps) == 1:
            return
        why = "--tta" if tta else "--sliding" if sliding else ("--crf" if crf is not None else ("SSCG_FUSE_PREDICT=0" if not F.FUSE_PREDICT[0] else None))
        if why is not None:
            raise ValueError("calibration: a temperature grid %r rescales the logits of the single fused head and does not combine with "
                             "%s (the probabilities there are not one softmax of logits): ask for temperature 1 only" % (opts.temps, why))

    def update_calibration(self, label_trues, x, size, probs=False, scale=1.0):
        """F.calibration_stats of one batch into the kept counts: `x` = logits to be resized to `size`, or (probs=True) scores at
        `size` whose probability is x * scale.  What the update_* methods call while the option is set."""
        if self._calibration is None:
            raise ValueError("update_calibration: no calibration option is set (set_calibration)")
        self._calibration_state = F.calibration_stats(x, size, label_trues, self._calibration, probs=probs, scale=scale,
                                                      state=self._calibration_state)

    def update_probs(self, label_trues, probs):
        """What the calibration option asks of a batch whose softmax map [N,C,OH,OW] already exists (the chain of separate passes,
        SSCG_FUSE_PREDICT=0): F.calibration_stats on the map.  The label map of the same batch goes to update_device().  Nothing is
        launched while the option is off."""
        if self._calibration is not None:
            self.update_calibration(label_trues, probs, probs.shape[2:], probs=True)

    def set_components(self, components):
        """The component filter (F.component_filter) as STATE of the score keeper: a F.ComponentOptions (utils.parse_components), or
        None = off.  While set, every update_* on device tensors asks its head for the uint8 label map ONLY (no label_true, no
        confusion matrix), filters it, and takes the confusion matrix (inside the filter's last launch), the contour counts and the
        surface records from the FILTERED map; the call's small stats tensor is kept.  While off, every method launches exactly what
        it launches without the option."""
        if components is not None and not isinstance(components, F.ComponentOptions):
            raise TypeError("set_components: a functional.ComponentOptions or None expected, not %r" % (components,))
        if components is not None:
            try:
                components.exempt_mask(self.n_classes)
            except ValueError as e:
                raise ValueError("set_components: %s" % e)
        if components != self._components:
            self._component_stats = []
        self._components = components

    def get_components(self):
        return self._components

    def _filter_components(self, label_trues, label_u8):
        """The component filter on one batch's uint8 label map: the confusion matrix, the contour options and the kept stats all see
        the filtered map, which is returned."""
        u8, self._device_hist, stats = F.component_filter(label_u8, self.n_classes, self._components, label_true=label_trues,
                                                          hist=self._device_hist, stats=True)
        self._component_stats.append(stats)
        if self._boundary is not None or self._surface is not None:
            self._count_boundary(label_trues, u8)
        return u8

    def _count_boundary(self, label_trues, label_u8):
        """What the contour options ask of one batch's uint8 label map: the boundary counts and / or the surface records."""
        if self._boundary is not None:
            self._boundary_counts = F.boundary_counts(label_trues.reshape(label_u8.shape), label_u8, self.n_classes,
                                                      self._boundary.width(*label_u8.shape[-2:]), self._boundary_counts)
        if self._surface is not None:
            self._surface_records.append(F.surface_stats(label_trues.reshape(label_u8.shape), label_u8, self.n_classes, self._surface))

    def update_device(self, label_trues, label_preds):
        """Same counts as update(), for label / prediction tensors that already live on the MI355X: no
        device->host copy of the maps per batch (model.py:568-569 moves both to numpy)."""
        if self._components is not None:
            self._filter_components(label_trues, label_preds.to(torch.uint8))
            return
        self._device_hist = F.confusion_hist(label_trues, label_preds, self.n_classes, self._device_hist)
        if self._boundary is not None or self._surface is not None:
            self._count_boundary(label_trues, label_preds.to(torch.uint8))

    def update_logits(self, label_trues, logits, size):
        """update_device() from the network's low-resolution logits: resize -> softmax -> argmax -> counts in one launch
        (F.predict_labels); neither the resized logits nor a predicted label map reach memory (with set_boundary(): the uint8 map
        does, for F.boundary_counts).  With set_calibration(): one more launch pair on the same logits (F.calibration_stats)."""
        if self._calibration is not None:
            self.update_calibration(label_trues, logits, size)
        if self._components is not None:
            self._filter_components(label_trues, F.predict_labels(logits, size, want_u8=True, num_classes=self.n_classes)[0])
            return
        want = self._boundary is not None or self._surface is not None
        u8, _, self._device_hist = F.predict_labels(logits, size, want_u8=want, label_true=label_trues, hist=self._device_hist,
                                                    num_classes=self.n_classes)
        if want:
            self._count_boundary(label_trues, u8)

    def update_logits_ms(self, label_trues, logits_list, flips, size):
        """update_logits() over several views of the batch (multi-scale / mirrored inference): the views' probabilities are summed
        and the counts taken in one launch (F.predict_labels_ms).  With set_calibration() the head also writes the summed
        probabilities, which F.calibration_stats scores with scale 1 / views."""
        cal = self._calibration is not None
        if cal:
            self.check_calibration(tta=True)
        if self._components is not None:
            out = F.predict_labels_ms(logits_list, flips, size, want_u8=True, num_classes=self.n_classes, **({"want_prob": True} if cal else {}))
            if cal:
                self.update_calibration(label_trues, out[3], size, probs=True, scale=inv_views(len(logits_list)))
            self._filter_components(label_trues, out[0])
            return
        want = self._boundary is not None or self._surface is not None
        out = F.predict_labels_ms(logits_list, flips, size, want_u8=want, label_true=label_trues, hist=self._device_hist,
                                  num_classes=self.n_classes, **({"want_prob": True} if cal else {}))
        u8, self._device_hist = out[0], out[2]
        if cal:
            self.update_calibration(label_trues, out[3], size, probs=True, scale=inv_views(len(logits_list)))
        if want:
            self._count_boundary(label_trues, u8)

    def update_logits_sw(self, label_trues, logits, plan):
        """update_logits() under sliding-window inference: `logits` are the maps of every window of the batch in F.window_gather's
        order (utils.sliding_logits), `plan` the F.sliding_plan of the batch's size; the windows' probabilities are blended and the
        counts taken in one launch (F.predict_labels_sw).  With set_calibration() the head also writes the blended, normalised
        probabilities, which F.calibration_stats scores with scale 1."""
        cal = self._calibration is not None
        size = (plan.OH, plan.OW)
        if cal:
            self.check_calibration(sliding=True)
        if self._components is not None:
            out = F.predict_labels_sw(logits, plan, want_u8=True, num_classes=self.n_classes, **({"want_prob": True} if cal else {}))
            if cal:
                self.update_calibration(label_trues, out[3], size, probs=True, scale=1.0)
            self._filter_components(label_trues, out[0])
            return
        want = self._boundary is not None or self._surface is not None
        out = F.predict_labels_sw(logits, plan, want_u8=want, label_true=label_trues, hist=self._device_hist,
                                  num_classes=self.n_classes, **({"want_prob": True} if cal else {}))
        u8, self._device_hist = out[0], out[2]
        if cal:
            self.update_calibration(label_trues, out[3], size, probs=True, scale=1.0)
        if want:
            self._count_boundary(label_trues, u8)

    def update_logits_crf(self, label_trues, logits_or_probs, image, size, crf, probs=False):
        """update_logits() with the windowed dense CRF (F.crf_labels) between the softmax and the first maximum: `image` guides it;
        probs=True: the scores are the summed probabilities of several views (F.predict_labels_ms(want_prob=True)) at `size`.
        With set_calibration() the head also writes Q after its last step, which F.calibration_stats scores with scale 1; a CRF of 0
        iterations has no Q: on logits it is update_logits() and is scored as such, on summed probabilities it is refused (the number
        of views is not known here: check_calibration)."""
        cal = self._calibration is not None
        want_q = cal and crf.iterations > 0
        if cal:
            self.check_calibration(tta=probs, crf=crf)
            if not want_q:
                self.update_calibration(label_trues, logits_or_probs, size)
        if self._components is not None:
            out = F.crf_labels(logits_or_probs, image, size, crf, probs=probs, want_u8=True, num_classes=self.n_classes,
                               **({"want_q": True} if want_q else {}))
            if want_q:
                self.update_calibration(label_trues, out[3], size, probs=True)
            self._filter_components(label_trues, out[0])
            return
        want = self._boundary is not None or self._surface is not None
        out = F.crf_labels(logits_or_probs, image, size, crf, probs=probs, want_u8=want, label_true=label_trues, hist=self._device_hist,
                           num_classes=self.n_classes, **({"want_q": True} if want_q else {}))
        u8, self._device_hist = out[0], out[2]
        if want_q:
            self.update_calibration(label_trues, out[3], size, probs=True)
        if want:
            self._count_boundary(label_trues, u8)

    def get_boundary_scores(self):
        """boundary_scores() of the counts accumulated since the last reset(); None while the option is off.  One device -> host copy
        of 3 C + C C integers."""
        if self._boundary is None:
            return None
        c = self.n_classes
        counts = np.zeros(3 * c + c * c, dtype=np.int64) if self._boundary_counts is None else self._boundary_counts.cpu().numpy()
        return boundary_scores(counts, c, self.dataset)

    def get_surface_scores(self):
        """surface_scores() of the records kept since the last reset(); None while the option is off.  The list is concatenated once
        and copied to the host once: 2 N C (5 integers + 1 double) per evaluated sample."""
        if self._surface is None:
            return None
        c = self.n_classes
        if self._surface_records:
            stats = torch.cat([r[0] for r in self._surface_records], dim=1)
            sums = torch.cat([r[1] for r in self._surface_records], dim=1)
            packed = torch.cat([stats.reshape(-1), sums.reshape(-1).view(torch.int64)]).cpu().numpy()
            stats = packed[:stats.numel()].reshape(tuple(stats.shape))
            sums = packed[stats.size:].view(np.float64).reshape(tuple(sums.shape))
        else:
            stats, sums = np.zeros((2, 0, c, 5), dtype=np.int64), np.zeros((2, 0, c), dtype=np.float64)
        return surface_scores(stats, sums, c, self.dataset, self._surface.pct)

    def get_calibration_scores(self):
        """calibration_scores() of the counts accumulated since the last reset(); None while the option is off.  One device -> host copy
        of NT (3 B + 3 C + 2) eight-byte values."""
        if self._calibration is None:
            return None
        c, opts = self.n_classes, self._calibration
        nt, b = len(opts.temps), opts.bins
        if self._calibration_state is None:
            bins, cls = np.zeros((nt, b, 3), dtype=np.int64), np.zeros((nt, c, 3), dtype=np.int64)
            sums = np.zeros((nt, 2), dtype=np.float64)
        else:
            sb, sc, ss = self._calibration_state
            packed = torch.cat([sb.reshape(-1), sc.reshape(-1), ss.reshape(-1).view(torch.int64)]).cpu().numpy()
            bins, cls = packed[:sb.numel()].reshape(nt, b, 3), packed[sb.numel():sb.numel() + sc.numel()].reshape(nt, c, 3)
            sums = packed[sb.numel() + sc.numel():].view(np.float64).reshape(nt, 2)
        return calibration_scores(bins, cls, sums, opts.temps, c, self.dataset)

    def get_component_scores(self):
        """What the component filter did since the last reset(), summed over the evaluated samples; None while the option is off.
        class_components / class_kept_components = the components found / kept per class, class_removed_pixels = the pixels a class
        lost (0 for the fill class, which only gains), components / kept_components / removed_pixels = their sums over the classes.
        One device -> host copy of 4 C integers."""
        if self._components is None:
            return None
        c = self.n_classes
        if self._component_stats:
            st = torch.cat(self._component_stats, dim=0).sum(dim=0).cpu().numpy()
        else:
            st = np.zeros((c, 4), dtype=np.int64)
        removed = np.where(np.arange(c) == self._components.fill, 0, st[:, 2] - st[:, 3])
        return {"components": int(st[:, 0].sum()), "kept_components": int(st[:, 1].sum()), "removed_pixels": int(removed.sum()),
                "class_components": dict(zip(range(c), (int(v) for v in st[:, 0]))),
                "class_kept_components": dict(zip(range(c), (int(v) for v in st[:, 1]))),
                "class_removed_pixels": dict(zip(range(c), (int(v) for v in removed)))}

    def _fold_device(self):
        if self._device_hist is not None:
            self.confusion_matrix += self._device_hist.cpu().numpy().astype(np.float64)
            self._device_hist = None

    def update(self, label_trues, label_preds):
        n = self.n_classes
        for lt, lp in zip(label_trues, label_preds):
            lt, lp = np.asarray(lt).ravel(), np.asarray(lp).ravel()
            keep = (lt >= 0) & (lt < n)
            self.confusion_matrix += np.bincount(n * lt[keep].astype(int) + lp[keep], minlength=n * n).reshape(n, n)

    def get_scores(self):
        self._fold_device()
        h, n = self.confusion_matrix, self.n_classes
        with np.errstate(divide="ignore", invalid="ignore"):
            acc = np.diag(h).sum() / h.sum()
            acc_cls = np.nanmean(np.diag(h) / h.sum(axis=1))
            iu = kept_iou(h, n, self.dataset)
        cls_iu = dict(zip(range(len(iu)), iu))
        return {"Overall Acc: \t": acc, "Mean Acc : \t": acc_cls, "Mean IoU : \t": np.nanmean(iu)}, cls_iu

    def get_dice(self):
        """{"mean_dice", "class_dice"} of the accumulated confusion matrix (dice_scores), over the classes get_scores() keeps."""
        self._fold_device()
        h, n = self.confusion_matrix, self.n_classes
        k = kept_classes(n, self.dataset)
        sub = h[k, k]
        d = dice_scores(sub)
        with np.errstate(invalid="ignore"):
            mean = float(np.nanmean(d)) if np.isfinite(d).any() else float("nan")
        return {"mean_dice": mean, "class_dice": dict(zip(range(len(d)), d))}

    def reset(self):
        self.confusion_matrix = np.zeros((self.n_classes, self.n_classes))
        self._device_hist = None
        self._boundary_counts = None
        self._surface_records = []
        self._component_stats = []
        self._calibration_state = None


def inv_views(views):
    """1 / views as the fp32 value the calibration kernel multiplies summed probabilities by."""
    return float(np.float32(1) / np.float32(int(views)))


def kept_classes(n_classes, dataset):
    """The classes the mean scores run over, as a slice: VOC ignores class 0, Cityscapes the last class, ACDC none (utils.py:398-405)."""
    return slice(1, n_classes) if dataset == "voc2012" else (slice(0, n_classes - 1) if dataset == "cityscapes" else slice(0, n_classes))


def kept_iou(hist, n_classes, dataset):
    """Per-class IoU TP / (TP + FP + FN) of the kept classes' block of a confusion matrix hist[true][predicted] (NaN on an empty
    denominator): runningScore.get_scores()'s arithmetic, which the trimap mIoU applies to its band-restricted matrix."""
    k = kept_classes(n_classes, dataset)
    sub = hist[k, k]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.diag(sub) / (sub.sum(axis=1) + sub.sum(axis=0) - np.diag(sub))


def _nanmean(v):
    with np.errstate(invalid="ignore"):
        return float(np.nanmean(v)) if np.isfinite(v).any() else float("nan")


def boundary_scores(counts, n_classes, dataset):
    """The contour scores of F.boundary_counts' vector bt | bp | bi | tri (include/sscg.h: sscg_boundary_counts):
    class_boundary_iou[c] = bi / (bt + bp - bi) (Cheng et al.; NaN on an empty denominator), class_trimap_iou = kept_iou(tri) (the
    DeepLab papers' trimap: the confusion matrix restricted to the band around the ground-truth label changes), boundary_iou /
    trimap_iou = their nanmean - all over the classes runningScore.get_scores() keeps for the dataset."""
    c = int(n_classes)
    v = np.asarray(counts).reshape(-1)
    if v.size != 3 * c + c * c:
        raise ValueError("boundary_scores: %d counts, 3 C + C C = %d expected" % (v.size, 3 * c + c * c))
    v = v.astype(np.float64)
    bt, bp, bi, tri = v[:c], v[c:2 * c], v[2 * c:3 * c], v[3 * c:].reshape(c, c)
    with np.errstate(divide="ignore", invalid="ignore"):
        biou = np.where(bt + bp - bi > 0, bi / (bt + bp - bi), np.nan)[kept_classes(c, dataset)]
    tiou = kept_iou(tri, c, dataset)
    return {"boundary_iou": _nanmean(biou), "class_boundary_iou": dict(zip(range(len(biou)), biou)),
            "trimap_iou": _nanmean(tiou), "class_trimap_iou": dict(zip(range(len(tiou)), tiou))}


def parse_boundary(spec):
    """`--boundary`: the contour scores of the evaluation.  "on" = F.BoundaryOptions() (the published width: 0.02 of the image
    diagonal); "d=N" = N pixels, 1..32; "ratio=F" = F of the diagonal, in (0, 1].  Returns a F.BoundaryOptions, None for "" / None.
    Raises ValueError naming the bad token."""
    spec = (spec or "").strip()
    if not spec:
        return None
    if spec == "on":
        return F.BoundaryOptions()
    key, sep, val = spec.partition("=")
    if not sep or key not in ("d", "ratio"):
        raise ValueError("--boundary: %r is not 'on', d=N or ratio=F" % spec)
    try:
        num = int(val) if key == "d" else float(val)
    except ValueError:
        raise ValueError("--boundary: %r is not a number%s" % (spec, " (an integer)" if key == "d" else ""))
    try:
        return F.BoundaryOptions(**{key: num})
    except ValueError as e:
        raise ValueError("--boundary: %r: %s" % (spec, e))


def surface_scores(stats, sums, n_classes, dataset, pct):
    """The surface distances of F.surface_stats' records (include/sscg.h: sscg_surface_stats): stats int64 [2, M, C, 5] = cnt, within,
    max2, v_lo, v_hi and sums float64 [2, M, C] per direction, case sample and class.  A case (sample, class) is DEFINED when both
    surfaces exist, MISSING when exactly one does, not counted when neither does.  Per defined case, in fp64:
    hd = sqrt(max of the two max2); hd95 = the larger of the two directions' a + (b - a) * (((cnt - 1) * pct) % 100) / 100 with
    a = sqrt(v_lo), b = sqrt(v_hi) - numpy's linear percentile written with integer ranks, so that the device selects two order
    statistics and no rank is ever formed in floating point; assd = (sum0 + sum1) / (cnt0 + cnt1); nsd = (within0 + within1) /
    (cnt0 + cnt1).  class_* = the mean over the class's defined cases (NaN without one), cases / missing = their numbers, hd / hd95 /
    assd / nsd = the nanmean over the classes runningScore.get_scores() keeps for the dataset."""
    c = int(n_classes)
    st = np.asarray(stats, dtype=np.int64)
    sm = np.asarray(sums, dtype=np.float64)
    if st.ndim != 4 or st.shape[0] != 2 or st.shape[2:] != (c, 5) or sm.shape != st.shape[:3]:
        raise ValueError("surface_scores: stats [2, M, %d, 5] and sums [2, M, %d] expected, got %s and %s" % (c, c, st.shape, sm.shape))
    cnt, within, max2, vlo, vhi = (st[..., k] for k in range(5))
    defined = (cnt[0] > 0) & (cnt[1] > 0)                                   # [M, C]
    missing = (cnt[0] > 0) ^ (cnt[1] > 0)
    frac = (((cnt - 1) * int(pct)) % 100).astype(np.float64) / 100.0
    with np.errstate(invalid="ignore", divide="ignore"):
        a, b = np.sqrt(vlo.astype(np.float64)), np.sqrt(vhi.astype(np.float64))
        per_dir = a + (b - a) * frac
        total = (cnt[0] + cnt[1]).astype(np.float64)
        case = {"hd": np.sqrt(np.maximum(max2[0], max2[1]).astype(np.float64)), "hd95": np.maximum(per_dir[0], per_dir[1]),
                "assd": (sm[0] + sm[1]) / total, "nsd": (within[0] + within[1]).astype(np.float64) / total}
    k = kept_classes(c, dataset)
    n_def = defined.sum(axis=0)
    out = {}
    for name, v in case.items():
        with np.errstate(invalid="ignore", divide="ignore"):
            cls = np.where(n_def > 0, np.where(defined, v, 0.0).sum(axis=0) / n_def, np.nan)[k]
        out[name] = _nanmean(cls)
        out["class_" + name] = dict(zip(range(len(cls)), cls))
    out["cases"] = dict(zip(range(len(n_def[k])), (int(v) for v in n_def[k])))
    out["missing"] = dict(zip(range(len(n_def[k])), (int(v) for v in missing.sum(axis=0)[k])))
    return out


def parse_surface(spec):
    """`--surface`: the surface distances of the evaluation.  "on" = F.SurfaceOptions() (tol 2 pixels, the 95th percentile); else a
    comma list over tol=F (the NSD tolerance in pixels, >= 0) and pct=N (the percentile, an integer in 1..100) - keys left out keep
    their defaults.  Returns a F.SurfaceOptions, None for "" / None.  Raises ValueError naming the bad token."""
    spec = (spec or "").strip()
    if not spec:
        return None
    if spec == "on":
        return F.SurfaceOptions()
    kw = {}
    for tok in spec.split(","):
        key, sep, val = tok.strip().partition("=")
        if not sep or key not in ("tol", "pct") or key in kw:
            raise ValueError("--surface: %r is not 'on' or one key=value over tol, pct" % tok)
        try:
            kw[key] = int(val) if key == "pct" else float(val)
        except ValueError:
            raise ValueError("--surface: %r is not a number%s" % (tok, " (an integer)" if key == "pct" else ""))
        try:
            F.SurfaceOptions(**{key: kw[key]})
        except ValueError as e:
            raise ValueError("--surface: %r: %s" % (tok, e))
    return F.SurfaceOptions(**kw)


def calibration_scores(bins, cls, sums, temps, n_classes, dataset):
    """The calibration scores of F.calibration_stats' counts (include/sscg.h: sscg_calib_stats): bins int64 [NT, B, 3] and cls int64
    [NT, C, 3] = (pixels, hits, the sum of the confidences in Q24) per confidence bin / per PREDICTED class, sums float64 [NT, 2] = (the
    sum of -log p[label], the sum of the squared distances to the one-hot label), temps the NT temperatures, temps[0] == 1.  In fp64,
    at T = 1, with n = the counted pixels:
    ece = sum_b n_b / n |hit_b / n_b - qsum_b / (2^24 n_b)|;  mce = the largest of those gaps over the non-empty bins;  nll, brier = the
    sums / n;  accuracy = hits / n;  confidence = the mean confidence;  counted = n;  class_gap[c] = conf_c - acc_c of the pixels PREDICTED
    as c, over the classes runningScore.get_scores() keeps for the dataset, NaN where a class is never predicted;  bins = the
    reliability diagram, a list of (lo, hi, n_b, accuracy, mean confidence);  above = for every bin edge e a tuple (e, coverage,
    accuracy) of the pixels in the bins at or above it - what a confidence threshold e (`--unl_pseudo_thresh e`) would keep, and how
    right it would be.  With NT > 1 also temperature_grid = [(T, nll, ece)] in ascending T and temperature = the grid's NLL argmin,
    refined by the vertex of the parabola through it and its two neighbours in log T; at an end of the grid it is the grid point and
    temperature_at_edge is True.  Without a counted pixel every score is NaN and counted is 0."""
    c = int(n_classes)
    bn, cl, sm = np.asarray(bins, dtype=np.int64), np.asarray(cls, dtype=np.int64), np.asarray(sums, dtype=np.float64)
    temps = [float(t) for t in temps]
    nt = len(temps)
    if bn.ndim != 3 or bn.shape[0] != nt or bn.shape[2] != 3 or cl.shape != (nt, c, 3) or sm.shape != (nt, 2):
        raise ValueError("calibration_scores: bins [%d, B, 3], cls [%d, %d, 3] and sums [%d, 2] expected, got %s, %s and %s" % (
            nt, nt, c, nt, bn.shape, cl.shape, sm.shape))
    nb = bn.shape[1]
    q24 = float(1 << 24)

    def at(t):
        n_b, h_b, q_b = (bn[t, :, k].astype(np.float64) for k in range(3))
        n = n_b.sum()
        with np.errstate(invalid="ignore", divide="ignore"):
            acc_b, conf_b = h_b / n_b, q_b / (q24 * n_b)
            gap = np.where(n_b > 0, np.abs(acc_b - conf_b), 0.0)
            if n > 0:
                ece, mce = float((n_b / n * gap).sum()), float(gap.max())
            else:
                ece = mce = float("nan")
            return {"n": n, "ece": ece, "mce": mce, "nll": float(sm[t, 0] / n) if n > 0 else float("nan"),
                    "brier": float(sm[t, 1] / n) if n > 0 else float("nan"), "acc_b": acc_b, "conf_b": conf_b, "n_b": n_b, "h_b": h_b,
                    "q_b": q_b}

    one = at(0)
    n, n_b, h_b = one["n"], one["n_b"], one["h_b"]
    out = {"ece": one["ece"], "mce": one["mce"], "nll": one["nll"], "brier": one["brier"], "counted": int(n)}
    with np.errstate(invalid="ignore", divide="ignore"):
        out["accuracy"] = float(h_b.sum() / n) if n > 0 else float("nan")
        out["confidence"] = float(one["q_b"].sum() / (q24 * n)) if n > 0 else float("nan")
        cn, ch, cq = (cl[0, :, k].astype(np.float64) for k in range(3))
        gap_c = np.where(cn > 0, cq / (q24 * cn) - ch / cn, np.nan)[kept_classes(c, dataset)]
        out["class_gap"] = dict(zip(range(len(gap_c)), gap_c))
        out["bins"] = [(b / nb, (b + 1) / nb, int(n_b[b]), float(one["acc_b"][b]), float(one["conf_b"][b])) for b in range(nb)]
        tail_n, tail_h = np.cumsum(n_b[::-1])[::-1], np.cumsum(h_b[::-1])[::-1]
        out["above"] = [(b / nb, float(tail_n[b] / n) if n > 0 else float("nan"),
                         float(tail_h[b] / tail_n[b]) if tail_n[b] > 0 else float("nan")) for b in range(nb)]
    if nt > 1:
        order = sorted(range(nt), key=lambda t: temps[t])
        rows = [at(t) for t in order]
        grid = [(temps[t], r["nll"], r["ece"]) for t, r in zip(order, rows)]
        out["temperature_grid"] = grid
        nll = np.array([g[1] for g in grid])
        if not np.isfinite(nll).all():
            out["temperature"], out["temperature_at_edge"] = float("nan"), False
        else:
            i = int(np.argmin(nll))
            out["temperature"], out["temperature_at_edge"] = grid[i][0], i in (0, nt - 1)
            if not out["temperature_at_edge"]:
                x0, x1, x2 = (float(np.log(grid[k][0])) for k in (i - 1, i, i + 1))
                y0, y1, y2 = (float(nll[k]) for k in (i - 1, i, i + 1))
                den = (x1 - x0) * (y1 - y2) - (x1 - x2) * (y1 - y0)
                if den != 0.0:
                    xv = x1 - 0.5 * ((x1 - x0) ** 2 * (y1 - y2) - (x1 - x2) ** 2 * (y1 - y0)) / den
                    out["temperature"] = float(np.exp(min(max(xv, x0), x2)))
    return out


def parse_calibration(spec):
    """`--calibration`: the calibration scores of the evaluation.  "on" = F.CalibrationOptions(): 15 confidence bins, temperature 1
    only; "fit" = bins=15,temps=0.5:3.0:7: also seven log-spaced temperatures from 0.5 to 3.0, from which the NLL-optimal one is fitted
    (both are untuned defaults, not published ones); else a comma list over bins=N (2..32) and temps=lo:hi:n (n log-spaced
    temperatures from lo to hi) or temps=a/b/c (the temperatures themselves) - temperature 1 is always put in front, at most 8 with it;
    keys left out keep their defaults.  Returns a F.CalibrationOptions, None for "" / None.  Raises ValueError naming the bad token."""
    import math
    spec = (spec or "").strip()
    if not spec:
        return None
    if spec == "on":
        return F.CalibrationOptions()
    if spec == "fit":
        spec = "bins=15,temps=0.5:3.0:7"
    kw = {}
    for tok in spec.split(","):
        key, sep, val = tok.strip().partition("=")
        if not sep or key not in ("bins", "temps") or key in kw:
            raise ValueError("--calibration: %r is not 'on', 'fit' or one key=value over bins, temps" % tok)
        try:
            if key == "bins":
                kw[key] = int(val)
            elif ":" in val:
                lo, hi, cnt = val.split(":")
                lo, hi, cnt = float(lo), float(hi), int(cnt)
                if not (0.0 < lo < hi < float("inf")) or not 2 <= cnt <= F.CALIBRATION_MAX_TEMPS:
                    raise ValueError("--calibration: %r: lo:hi:n needs 0 < lo < hi and n in 2..%d" % (tok, F.CALIBRATION_MAX_TEMPS))
                step = (math.log(hi) - math.log(lo)) / (cnt - 1)
                kw[key] = tuple([lo] + [math.exp(math.log(lo) + k * step) for k in range(1, cnt - 1)] + [hi])
            else:
                kw[key] = tuple(float(v) for v in val.split("/"))
        except ValueError as e:
            if str(e).startswith("--calibration"):
                raise
            raise ValueError("--calibration: %r is not %s" % (tok, "an integer" if key == "bins" else "lo:hi:n or a list a/b/c of numbers"))
        try:
            F.CalibrationOptions(**{key: kw[key]})
        except ValueError as e:
            raise ValueError("--calibration: %r: %s" % (tok, e))
    return F.CalibrationOptions(**kw)


def parse_components(spec):
    """`--components`: the connected-component filter of the evaluation's label maps.  "on" = min_area=64 with 8-connectivity and
    fill=0 (an untuned default, not a published one); else a comma list over `largest` (keep only the largest component of each sample
    and class), min_area=N (keep components of at least N pixels), conn=4|8, fill=K (the class removed pixels get) and skip=a:b:c
    (classes never filtered) - at least one of largest / min_area has to be named, keys left out keep their defaults.  Returns a
    F.ComponentOptions, None for "" / None.  Raises ValueError naming the bad token."""
    spec = (spec or "").strip()
    if not spec:
        return None
    if spec == "on":
        return F.ComponentOptions(min_area=64)
    kw = {}
    for tok in spec.split(","):
        key, sep, val = tok.strip().partition("=")
        if key in kw or not ((key == "largest" and not sep) or (key in ("min_area", "conn", "fill", "skip") and sep)):
            raise ValueError("--components: %r is not 'on', largest or one key=value over min_area, conn, fill, skip" % tok)
        if key == "largest":
            kw[key] = True
            continue
        try:
            kw[key] = tuple(int(v) for v in val.split(":")) if key == "skip" else int(val)
        except ValueError:
            raise ValueError("--components: %r is not an integer%s" % (tok, " list a:b:c" if key == "skip" else ""))
        try:
            F.ComponentOptions(**{key: kw[key]})
        except ValueError as e:
            raise ValueError("--components: %r: %s" % (tok, e))
    if "largest" not in kw and "min_area" not in kw:
        raise ValueError("--components: %r names neither largest nor min_area: nothing would be filtered" % spec)
    return F.ComponentOptions(**kw)


def dice_scores(hist):
    """Per-class Dice 2 TP / (2 TP + FP + FN) of a confusion matrix hist[true][predicted]; NaN for a class with an empty denominator
    (it occurs in neither the labels nor the predictions)."""
    h = np.asarray(hist, dtype=np.float64)
    tp = np.diag(h)
    den = h.sum(axis=1) + h.sum(axis=0)          # (TP + FN) + (TP + FP)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, 2.0 * tp / den, np.nan)


def parse_dice_skip(spec, n_classes):
    """--dice_skip: a comma list of class ids the Dice loss gives weight 0 (e.g. 0: VOC's background; 19: the Cityscapes void class) ->
    a sorted list of distinct ids in [0, n_classes); "" / None -> [].  Skipping every class is refused (the loss divides by the sum of
    the weights).  Raises ValueError naming the bad token."""
    if spec is None or not str(spec).strip():
        return []
    ids = set()
    for tok in str(spec).split(","):
        t = tok.strip()
        if not (t.isdigit() and int(t) < int(n_classes)):
            raise ValueError("--dice_skip: %r is not a class id in [0, %d)" % (t, n_classes))
        ids.add(int(t))
    if len(ids) >= int(n_classes):
        raise ValueError("--dice_skip: %r skips every class" % (spec,))
    return sorted(ids)


def parse_boundary_loss_skip(spec, n_classes):
    """--boundary_loss_skip: a comma list of class ids the boundary loss gives weight 0, in parse_dice_skip's grammar -> a sorted list
    of distinct ids in [0, n_classes); "" / None -> [].  Skipping every class is refused (the loss divides by the sum of the weights).
    Raises ValueError naming the bad token."""
    if spec is None or not str(spec).strip():
        return []
    ids = set()
    for tok in str(spec).split(","):
        t = tok.strip()
        if not (t.isdigit() and int(t) < int(n_classes)):
            raise ValueError("--boundary_loss_skip: %r is not a class id in [0, %d)" % (t, n_classes))
        ids.add(int(t))
    if len(ids) >= int(n_classes):
        raise ValueError("--boundary_loss_skip: %r skips every class" % (spec,))
    return sorted(ids)


def parse_lovasz_skip(spec, n_classes):
    """--lovasz_skip: a comma list of class ids the Lovasz-softmax loss leaves out, in parse_dice_skip's grammar -> a sorted tuple of
    distinct ids in [0, n_classes); "" / None -> ().  Skipping every class is refused.  Raises ValueError naming the bad token."""
    if spec is None or not str(spec).strip():
        return ()
    ids = set()
    for tok in str(spec).split(","):
        t = tok.strip()
        if not (t.isdigit() and int(t) < int(n_classes)):
            raise ValueError("--lovasz_skip: %r is not a class id in [0, %d)" % (t, n_classes))
        ids.add(int(t))
    if len(ids) >= int(n_classes):
        raise ValueError("--lovasz_skip: %r skips every class" % (spec,))
    return tuple(sorted(ids))


def boundary_loss_schedule(weight, ramp, epoch):
    """--boundary_loss F with --boundary_loss_ramp N: the weight of the boundary term in `epoch` (0-based), b = F * min(1, epoch / N);
    N == 0: F from the first epoch on.  A host scalar: no kernel sees it."""
    weight, ramp, epoch = float(weight), int(ramp), int(epoch)
    if ramp <= 0:
        return weight
    return weight * min(1.0, max(epoch, 0) / float(ramp))


MAX_TTA_VIEWS = 8


def parse_tta(spec):
    """`--tta`: the views of multi-scale / mirrored inference.  "0.5,0.75,1.0" = one view per scale; a trailing ":flip" adds the
    horizontally mirrored twin of every scale directly after it.  Returns a list of (scale, flip) in view order, None for ""."""
    spec = (spec or "").strip()
    if not spec:
        return None
    scales, sep, mode = spec.partition(":")
    if sep and mode != "flip":
        raise ValueError("--tta: %r after ':' (only 'flip' is known)" % mode)
    views = []
    for tok in scales.split(","):
        try:
            scale = float(tok)
        except ValueError:
            raise ValueError("--tta: %r is not a scale" % tok)
        if not (scale > 0 and scale != float("inf")):
            raise ValueError("--tta: scale %r is not positive" % tok)
        views.append((scale, False))
        if sep:
            views.append((scale, True))
    if len(views) > MAX_TTA_VIEWS:
        raise ValueError("--tta: %d views, at most %d" % (len(views), MAX_TTA_VIEWS))
    return views


def tta_size(h, w, scale):
    """The network input size of a view: the crop scaled and rounded half up, never below one pixel."""
    return max(1, int(h * scale + 0.5)), max(1, int(w * scale + 0.5))


def tta_logits(net, images, views):
    """One forward of `net` per view on F.resize_flip of the batch: (logit maps, flip flags) for F.predict_labels_ms."""
    h, w = images.shape[2:]
    return [net(F.resize_flip(images, tta_size(h, w, scale), flip)) for scale, flip in views], [flip for _, flip in views]


_SLIDING_KEYS = ("size", "scale", "overlap", "blend", "sigma", "flip")


def parse_sliding(spec, crop):
    """`--sliding`: sliding-window inference of the evaluation, --validation and --testing.  The window is the crop (`crop` = (height,
    width), the size the network was trained at).  "on" = scale=2,overlap=0.5,blend=gauss (an untuned default); else a comma list over
    size=HxW or scale=F (exactly one: the evaluation size the images are kept at - scale multiplies the crop, rounded half up; never
    below the crop), overlap=F (0..0.75, default 0.5), blend=gauss|const (default gauss), sigma=F (in (0, 1] of the window, default
    0.125: MONAI's / nnU-Net's value, untuned here) and flip (every window also runs mirrored along W).  At most 16 windows per axis.
    Returns a F.SlidingOptions, None for "" / None.  Raises ValueError naming the bad token."""
    spec = (spec or "").strip()
    if not spec:
        return None
    crop = (int(crop[0]), int(crop[1]))
    if spec == "on":
        spec = "scale=2,overlap=0.5,blend=gauss"
    kw, seen = {}, set()
    for tok in spec.split(","):
        key, sep, val = tok.strip().partition("=")
        if key not in _SLIDING_KEYS or key in seen or (key == "flip") == bool(sep):
            raise ValueError("--sliding: %r is not 'on', flip or one key=value over size, scale, overlap, blend, sigma (each once)" % tok)
        seen.add(key)
        try:
            if key == "flip":
                kw["flip"] = True
            elif key == "size":
                hh, x, ww = val.partition("x")
                if not x:
                    raise ValueError
                kw["size"] = (int(hh), int(ww))
            elif key == "scale":
                f = float(val)
                if not (f > 0 and f < float("inf")):
                    raise ValueError
                kw["size"] = (int(crop[0] * f + 0.5), int(crop[1] * f + 0.5))
            elif key == "blend":
                kw["blend"] = val
            else:
                kw[key] = float(val)
        except ValueError:
            raise ValueError("--sliding: %r is not %s" % (tok, {"size": "size=<height>x<width>", "scale": "a positive scale"}.get(key, "a number")))
    if ("size" in seen) == ("scale" in seen):
        raise ValueError("--sliding: %r must name the evaluation size once, as size=HxW or as scale=F" % spec)
    try:
        return F.SlidingOptions(crop, **kw)
    except ValueError as e:
        raise ValueError("--sliding: %r: %s" % (spec, e))


def sliding_logits(net, images, plan, chunk):
    """`net` on every window of the batch (F.window_gather), `chunk` consecutive windows per forward - the loader's batch size, so the
    network sees the batch size it was sized for; eval-mode BatchNorm and InstanceNorm do not depend on the chunking.  Returns the
    logits of all windows in one buffer [N * views, C, h, w], the input of F.predict_labels_sw."""
    wins = F.window_gather(images, plan)
    total, chunk = wins.shape[0], max(1, int(chunk))
    if total <= chunk:
        return net(wins)
    out = None
    for i in range(0, total, chunk):
        lg = net(wins[i:i + chunk])
        if out is None:
            out = F.empty_nhwc(total, lg.shape[1], lg.shape[2], lg.shape[3], lg.device)
        out[i:i + lg.shape[0]].copy_(lg)
    return out


_CRF_KEYS = {"iters": "iterations", "radius": "radius", "dilation": "dilation", "wb": "w_bilateral", "ws": "w_spatial",
             "alpha": "theta_alpha", "beta": "theta_beta", "gamma": "theta_gamma"}


def parse_crf(spec):
    """`--crf`: the windowed dense CRF behind the evaluation's softmax.  "on" = F.CrfOptions() (untuned defaults); else a comma list of
    key=value over iters, radius, dilation, wb, ws, alpha, beta, gamma, e.g. "iters=5,radius=3,dilation=2,wb=4,ws=3,alpha=8,beta=0.5,
    gamma=3" - keys left out keep their defaults.  Returns a F.CrfOptions, None for "" / None.  Raises ValueError naming the bad token."""
    spec = (spec or "").strip()
    if not spec:
        return None
    if spec == "on":
        return F.CrfOptions()
    kw = {}
    for tok in spec.split(","):
        key, sep, val = tok.strip().partition("=")
        if not sep or key not in _CRF_KEYS or _CRF_KEYS[key] in kw:
            raise ValueError("--crf: %r is not one key=value over %s" % (tok, ", ".join(_CRF_KEYS)))
        try:
            kw[_CRF_KEYS[key]] = int(val) if key in ("iters", "radius", "dilation") else float(val)
        except ValueError:
            raise ValueError("--crf: %r is not a number%s" % (tok, " (an integer)" if key in ("iters", "radius", "dilation") else ""))
        try:
            F.CrfOptions(**dict({"radius": 1, "dilation": 1}, **{_CRF_KEYS[key]: kw[_CRF_KEYS[key]]}))      # the value's own range: the error names the token
        except ValueError as e:
            raise ValueError("--crf: %r: %s" % (tok, e))
    try:
        return F.CrfOptions(**kw)
    except ValueError as e:         # what only the combination breaks: radius * dilation
        raise ValueError("--crf: %r: %s" % (spec, e))


def parse_unl_crf_kernel(spec):
    """`--unl_crf_kernel`: the pairwise kernel of the gated CRF loss, in parse_crf's grammar (`iters` is accepted and ignored: the loss
    has no mean-field step).  "" / None / "on" = F.CrfOptions(), the UNTUNED defaults.  Raises ValueError naming the flag."""
    try:
        return parse_crf(spec) or F.CrfOptions()
    except ValueError as e:
        raise ValueError(str(e).replace("--crf:", "--unl_crf_kernel:", 1))


_TEACHER_KEYS = ("mse", "ce", "thresh", "temp")


def parse_unl_teacher(spec):
    """`--unl_teacher`: mean-teacher consistency on the unlabelled batch, in parse_crf's comma grammar: key=value over mse, ce, thresh,
    temp, plus the bare word `flip`, e.g. "mse=1,ce=0.5,thresh=0.6,flip" - keys left out keep F.TeacherOptions' defaults.  "on" =
    mse=1, an UNTUNED default.  Returns a F.TeacherOptions, None for "" / None.  Raises ValueError naming the bad token; a spec that
    turns neither term on is refused."""
    spec = (spec or "").strip()
    if not spec:
        return None
    if spec == "on":
        return F.TeacherOptions(mse=1.0)
    kw = {}
    for tok in spec.split(","):
        key, sep, val = tok.strip().partition("=")
        if key == "flip" and not sep and "flip" not in kw:
            kw["flip"] = True
            continue
        if not sep or key not in _TEACHER_KEYS or key in kw:
            raise ValueError("--unl_teacher: %r is not `flip` or one key=value over %s" % (tok, ", ".join(_TEACHER_KEYS)))
        try:
            kw[key] = float(val)
        except ValueError:
            raise ValueError("--unl_teacher: %r is not a number" % (tok,))
        try:
            F.TeacherOptions(**{key: kw[key]})      # the value's own range: the error names the token
        except ValueError as e:
            raise ValueError("--unl_teacher: %r: %s" % (tok, e))
    opts = F.TeacherOptions(**kw)
    if not opts.any:
        raise ValueError("--unl_teacher: %r turns on neither mse= nor ce=" % (spec,))
    return opts


def parse_unl_cutmix(spec):
    """`--unl_cutmix`: CutMix consistency for the mean teacher, in the grammar of `--augment cutmix=`: `p[:lo:hi]` - with probability p
    (0 < p <= 1) a sample of the unlabelled batch takes a box of lo..hi of the area (0 < lo <= hi <= 1; default 0.25:0.5, UNTUNED)
    from a partner.  Returns (p, lo, hi), None for "" / None.  Raises ValueError naming the bad token."""
    import math
    spec = (spec or "").strip()
    if not spec:
        return None
    toks = spec.split(":")
    if len(toks) not in (1, 3):
        raise ValueError("--unl_cutmix: %r is not p or p:lo:hi" % (spec,))
    vals = []
    for tok in toks:
        try:
            v = float(tok)
        except ValueError:
            raise ValueError("--unl_cutmix: %r is not a number" % (tok,))
        if not (math.isfinite(v) and 0.0 < v <= 1.0):
            raise ValueError("--unl_cutmix: %r is not in (0, 1]" % (tok,))
        vals.append(v)
    p, lo, hi = vals if len(vals) == 3 else (vals[0], 0.25, 0.5)
    if lo > hi:
        raise ValueError("--unl_cutmix: %r: lo %r is above hi %r" % (spec, toks[1], toks[2]))
    return p, lo, hi


def crf_guide(images, size):
    """The CRF's guide image: the batch as the network sees it (normalised), resized to `size` when it has another."""
    return images if tuple(images.shape[2:]) == (int(size[0]), int(size[1])) else F.upsample_bilinear(images, size)


def crf_scores(net, images, size, tta=None, sliding=None, chunk=None):
    """What F.crf_labels starts from, as (scores, probs): the logits of `net`'s single forward (probs=False), or with `tta` (a view list
    of parse_tta) the summed probabilities of the views at `size` - F.predict_labels_ms asked for nothing else (probs=True) - or with
    `sliding` (a F.SlidingOptions) the blended, normalised probabilities of the windows at the images' own size (probs=True; the
    guide is then the batch itself), `net` run on `chunk` windows at a time (default: the batch size)."""
    if sliding is not None:
        if tta:
            raise ValueError("sliding-window inference does not combine with --tta (its own key 'flip' mirrors the windows)")
        plan = F.sliding_plan(images.shape[2], images.shape[3], sliding, images.device)
        if (plan.OH, plan.OW) != (int(size[0]), int(size[1])):
            raise ValueError("crf_scores: sliding-window scores have the images' size %dx%d, not %r" % (plan.OH, plan.OW, tuple(size)))
        logits = sliding_logits(net, images, plan, chunk or images.shape[0])
        return F.predict_labels_sw(logits, plan, want_prob=True, want_u8=False)[3], True
    if tta:
        return F.predict_labels_ms(*tta_logits(net, images, tta), size, want_prob=True, want_u8=False)[3], True
    return net(images), False


CE_INVLOG_K = 1.02      # ENet's constant in w = 1 / ln(k + f)


def parse_ce_weights(spec, n_classes):
    """`--ce_weights`: the class weights of the ground-truth cross entropies.  "" -> None (the reference's unweighted loss); a comma
    list of exactly n_classes numbers (finite, >= 0) -> that list of floats; a rule computed from the labelled set's class frequencies
    (ce_weights_from_counts): "median" -> ("median",), "invlog" / "invlog:<k>" -> ("invlog", k) with k > 1, default 1.02."""
    import math
    spec = (spec or "").strip()
    if not spec:
        return None
    if spec == "median":
        return ("median",)
    name, sep, arg = spec.partition(":")
    if name == "invlog":
        if not sep:
            return ("invlog", CE_INVLOG_K)
        try:
            k = float(arg)
        except ValueError:
            raise ValueError("--ce_weights: %r is not a number (invlog:<k>)" % arg)
        if not (math.isfinite(k) and k > 1.0):
            raise ValueError("--ce_weights: invlog needs k > 1 (1 / ln(k + f) with f in (0, 1]), got %r" % arg)
        return ("invlog", k)
    vals = []
    for tok in spec.split(","):
        try:
            v = float(tok)
        except ValueError:
            raise ValueError("--ce_weights: %r is neither a number nor a rule (median, invlog[:k])" % tok)
        if not math.isfinite(v) or v < 0:
            raise ValueError("--ce_weights: %r is not a finite weight >= 0" % tok)
        vals.append(v)
    if len(vals) != int(n_classes):
        raise ValueError("--ce_weights: %r has %d entries, the dataset has %d classes" % (spec, len(vals), n_classes))
    return vals


def ce_weights_from_counts(rule, counts):
    """Class weights from per-class pixel counts (a pure host function).  f[c] = counts[c] / sum(counts);
    ("median",): median-frequency balancing, w[c] = median(f over the classes present) / f[c];
    ("invlog", k): w[c] = 1 / ln(k + f[c]) (ENet's rule).  A class with no pixel gets weight 0."""
    import math
    counts = [int(c) for c in counts]
    total = sum(counts)
    if total <= 0 or min(counts) < 0:
        raise ValueError("class weights: the label maps hold no pixel of any class (counts %r)" % (counts,))
    f = [c / total for c in counts]
    if rule[0] == "median":
        med = float(np.median([x for x in f if x > 0]))
        return [med / x if x > 0 else 0.0 for x in f]
    if rule[0] == "invlog":
        k = float(rule[1])
        return [1.0 / math.log(k + x) if x > 0 else 0.0 for x in f]
    raise ValueError("unknown class-weight rule %r" % (rule,))


def checkpoint_scores(miou, class_iou):
    """The two score entries of a checkpoint as plain Python numbers: ('best_iou': float, 'class_iou': {int: float}) of what
    runningScore.get_scores() returns (numpy.float64 scalars; an empty class stays NaN).  A file that holds only tensors, containers
    and Python numbers is read back by torch's default (weights-only) loading; numpy scalars are not."""
    return float(miou), {int(k): float(v) for k, v in class_iou.items()}


def save_checkpoint(state, save_path):
    torch.save(state, save_path)


def _numpy_scalar_globals():
    """The globals a pickled numpy scalar names: the reconstructor (written as numpy._core.multiarray.scalar by numpy 2.x, as
    numpy.core.multiarray.scalar by numpy 1.x), numpy.dtype and the dtype classes of float64 / int64.  Nothing else."""
    import importlib
    out = [np.dtype, type(np.dtype(np.float64)), type(np.dtype(np.int64))]
    paths = ("numpy._core.multiarray", "numpy.core.multiarray")
    for mod in paths:               # (the first that exists: numpy 2.x only keeps the old path as a deprecated alias of the new one)
        try:
            fn = importlib.import_module(mod).scalar
        except (ImportError, AttributeError):
            continue
        # the unpickler matches the name the FILE uses, whichever numpy wrote it: both names stand for this numpy's function
        out.extend((fn, m + ".scalar") for m in paths)
        break
    return out


def load_checkpoint(ckpt_path, map_location="cpu"):
    """torch.load with torch's safe (weights-only) unpickler.  Files written before checkpoint_scores() existed, and the reference's,
    hold numpy.float64 scalars ('best_iou', 'class_iou'): for those the load is repeated with exactly the numpy scalar globals
    allow-listed.  A file that holds any other pickled class raises (pickle.UnpicklingError), a missing file FileNotFoundError."""
    import pickle
    try:
        ckpt = torch.load(ckpt_path, map_location=map_location, weights_only=True)
    except pickle.UnpicklingError:
        with torch.serialization.safe_globals(_numpy_scalar_globals()):
            ckpt = torch.load(ckpt_path, map_location=map_location, weights_only=True)
    print(" [*] Loading checkpoint from %s succeed!" % ckpt_path)
    return ckpt


def print_networks(nets, names):
    print("------------Number of Parameters---------------")
    for net, name in zip(nets, names):
        n = sum(p.numel() for p in net.parameters())
        print("[Network %s] Total number of parameters : %.3f M" % (name, n / 1e6))
    print("-----------------------------------------------")


# ---- inference-script helpers (utils.py:14-55 of the reference; the palette values are dataset constants)
def _pad_palette(p):
    return p + [0] * (256 * 3 - len(p))


palette = _pad_palette([0, 0, 0, 128, 0, 0, 0, 128, 0, 128, 128, 0, 0, 0, 128, 128, 0, 128, 0, 128, 128,
                        128, 128, 128, 64, 0, 0, 192, 0, 0, 64, 128, 0, 192, 128, 0, 64, 0, 128, 192, 0, 128,
                        64, 128, 128, 192, 128, 128, 0, 64, 0, 128, 64, 0, 0, 192, 0, 128, 192, 0, 0, 64, 128])
cityscape_palette = _pad_palette([128, 64, 128, 244, 35, 232, 70, 70, 70, 102, 102, 156, 190, 153, 153, 153, 153, 153,
                                  250, 170, 30, 220, 220, 0, 107, 142, 35, 152, 251, 152, 0, 130, 180, 220, 20, 60,
                                  255, 0, 0, 0, 0, 142, 0, 0, 70, 0, 60, 100, 0, 80, 100, 0, 0, 230, 119, 11, 32])
acdc_palette = _pad_palette([0, 0, 0, 128, 64, 128, 70, 70, 70, 250, 170, 30])


def colorize_mask(mask, dataset):
    """One-channel class map (numpy) -> paletted PIL image (utils.py:41-55)."""
    from PIL import Image
    assert dataset in ('voc2012', 'cityscapes', 'acdc')
    new_mask = Image.fromarray(np.asarray(mask).astype(np.uint8)).convert('P')
    new_mask.putpalette(PALETTES[dataset])
    return new_mask


PALETTES = {'voc2012': palette, 'cityscapes': cityscape_palette, 'acdc': acdc_palette}
_PALETTE_TENSORS = {}


def palette_tensor(dataset, device):
    """The dataset's palette as the uint8 [256,3] device table of F.panel_range / F.panel_grid (uploaded once per device)."""
    key = (dataset, str(device))
    t = _PALETTE_TENSORS.get(key)
    if t is None:
        t = _PALETTE_TENSORS[key] = torch.tensor(PALETTES[dataset], dtype=torch.uint8).reshape(256, 3).to(device)
    return t


# ---- the per-epoch image panels on the host (model.py:617-638 of the reference): the separate-passes path of model.panels()
def PIL_to_tensor(img, dataset):
    """Paletted PIL image -> fp32 [3,H,W] of its palette colours, 0..255 (utils.py:59-94): the reference's per-pixel double loop
    (`index = int(img_arr[i, j] * 3)`, three palette reads) as three gathers."""
    assert dataset in ('voc2012', 'cityscapes', 'acdc')
    img_arr = np.array(img, dtype='float32')
    index = (img_arr * 3).astype(np.int64)
    pal = np.asarray(PALETTES[dataset], dtype='float32')
    return torch.tensor(np.stack([pal[index], pal[index + 1], pal[index + 2]]))


def make_grid(tensor, nrow=8, padding=2, normalize=False):
    """torchvision.utils.make_grid for a [N,C,H,W] batch (C in {1, 3}; pad_value 0, no value range, scale_each off): one-channel
    images are replicated to three; normalize=True shifts the whole batch to [0, 1] by its own min / max - (x - lo) / max(hi - lo,
    1e-5), the difference taken in double as torchvision's Python floats do, the rest in fp32; a single image is returned as it is;
    otherwise min(nrow, N) tiles per row, `padding` pixels of 0 around every tile.  Returns an fp32 [3,GH,GW] tensor."""
    t = torch.as_tensor(tensor)
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() == 3:
        t = t.unsqueeze(0)
    a = np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
    if a.shape[1] == 1:
        a = np.concatenate((a, a, a), 1)
    if normalize:
        lo, hi = float(a.min()), float(a.max())
        a = (np.clip(a, np.float32(lo), np.float32(hi)) - np.float32(lo)) / np.float32(max(hi - lo, 1e-5))
    n, c, h, w = a.shape
    if n == 1:
        return torch.from_numpy(a[0].copy())
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    grid = np.zeros((c, ymaps * (h + padding) + padding, xmaps * (w + padding) + padding), dtype=np.float32)
    for k in range(n):
        y0, x0 = (k // xmaps) * (h + padding) + padding, (k % xmaps) * (w + padding) + padding
        grid[:, y0:y0 + h, x0:x0 + w] = a[k]
    return torch.from_numpy(grid)


def grid_to_u8(t):
    """The image writer's float -> byte conversion of a [0, 1] CHW grid (tensorboardX: `(t * 255.0).astype(np.uint8)`)."""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return (a * 255.0).astype(np.uint8)


def save_panel_png(grid_u8, path):
    """One panel (uint8 CHW, as model.panels() returns it) as a PNG."""
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(np.asarray(grid_u8).transpose(1, 2, 0))).save(path)


def save_image_u8(pixels, path):
    """save_image() for the uint8 HWC pixels F.predict_image already holds (its x * 255 + 0.5, clamp, truncate ran on the device)."""
    from PIL import Image
    arr = np.asarray(pixels)
    Image.fromarray(arr[:, :, 0] if arr.shape[2] == 1 else arr).save(path)


def save_image(tensor, path):
    """torchvision.utils.save_image for one CHW image in [0, 1]: x*255 + 0.5, clamp, uint8, HWC."""
    from PIL import Image
    arr = tensor.detach().float().cpu().mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()
    Image.fromarray(arr[:, :, 0] if arr.shape[2] == 1 else arr).save(path)
