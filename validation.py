"""`python main.py --validation ...`: the reference's validation.py (:20-157) on the MI355X backend.
Loads `latest_{supervised_model,semisuper_cycleGAN}.ckpt`, runs the DeepLab generators in eval mode over the val
split and writes the paletted predictions (and, for the semi-supervised model, the regenerated labels / images)
under `--validation_dir`, with the reference's directory names."""
import importlib
import os

import torch

PKG = "semi-supervised-segmentation-cyclegan_amd"


def _mk(*parts):
    d = os.path.join(*parts)
    os.makedirs(d, exist_ok=True)
    return d


def validation(args, val_loader=None):
    F = importlib.import_module(PKG + ".functional")
    arch = importlib.import_module(PKG + ".arch")
    utils = importlib.import_module(PKG + ".utils")
    n_channels = {'voc2012': 21, 'cityscapes': 20, 'acdc': 4}[args.dataset]
    dev = torch.device("cuda", args.gpu_ids[0])
    # --sliding: the images keep the evaluation size, Gsi runs on overlapping crop-sized windows, the label maps have that size
    sliding = utils.parse_sliding(getattr(args, 'sliding', ''), (args.crop_height, args.crop_width))
    size = sliding.size if sliding is not None else (args.crop_height, args.crop_width)
    if val_loader is None:
        du = importlib.import_module(PKG + ".data_utils")
        from torch.utils.data import DataLoader
        tr = du.get_transformation(size, resize=True, dataset=args.dataset, device_finish=True)
        cls = {'voc2012': du.VOCDataset, 'cityscapes': du.CityscapesDataset, 'acdc': du.ACDCDataset}[args.dataset]
        root = {'voc2012': './data/VOC2012', 'cityscapes': './data/Cityscape', 'acdc': './data/ACDC'}[args.dataset]
        val_set = cls(root_path=root, name='val', ratio=0.5, transformation=tr, augmentation=None)
        val_loader = du.DeviceLoader(DataLoader(val_set, batch_size=args.batch_size, shuffle=False), tr, dev)

    mk = lambda i, o: arch.define_Gen(input_nc=i, output_nc=o, ngf=args.ngf, netG='deeplab', norm=args.norm,
                                      use_dropout=not args.no_dropout, gpu_ids=args.gpu_ids)
    Gsi, Gis = mk(3, n_channels), mk(n_channels, 3)            # validation.py:42-46
    best_iou = 0
    semi = args.model == 'semisupervised_cycleGAN'
    # only a MISSING file leaves the initial weights (the reference's behaviour); a file that exists and cannot be restored stops the
    # run: its predictions would be those of random networks
    try:
        ckpt = utils.load_checkpoint('%s/latest_%s.ckpt' % (args.checkpoint_dir, 'semisuper_cycleGAN' if semi else 'supervised_model'))
    except FileNotFoundError:
        ckpt = None
        print(' [*] No checkpoint!')
    if ckpt is not None:
        Gsi.load_state_dict(ckpt['Gsi'])
        if semi:
            Gis.load_state_dict(ckpt['Gis'])
        if getattr(args, 'ema_decay', None) is not None:       # --ema_decay: the averaged parameters over the trained ones (buffers stay)
            for net, key in ((Gsi, 'Gsi_ema'), (Gis, 'Gis_ema')):
                if key in ckpt:
                    net.load_state_dict(ckpt[key], strict=False)
        best_iou = float(ckpt['best_iou'])

    comp = utils.parse_components(getattr(args, 'components', ''))
    # --components: every predicted label map goes through the connected-component filter on the device before it is copied and saved
    filt = lambda t: t if comp is None else F.component_filter(t, n_channels, comp)[0]
    fused = F.FUSE_PREDICT[0]                     # SSCG_FUSE_PREDICT=0: the chain of separate passes (same bits)
    soft = lambda lg: F.softmax2d(F.upsample_bilinear(lg, size))                    # interp -> Softmax2d
    # Gsi's logits -> interp -> Softmax2d -> argmax: uint8 label maps from one launch, or the int64 maps of the separate passes
    labels = (lambda lg: filt(F.predict_labels(lg, size)[0]).cpu().numpy()) if fused else (lambda lg: filt(F.argmax_index(soft(lg))).cpu().numpy())
    tta = utils.parse_tta(getattr(args, 'tta', ''))
    if sliding is not None and tta:
        raise ValueError("--sliding does not combine with --tta: 'flip' is --sliding's own key")
    # --tta: Gsi once per view of the images, the views fused into one uint8 map (F.FUSE_TTA: in one launch)
    labels_ms = lambda x: filt(F.predict_labels_ms(*utils.tta_logits(Gsi, x, tta), size)[0]).cpu().numpy()


    def heads_sw(x, **kw):
        """F.predict_labels_sw on Gsi's logits of every window of the batch, `batch_size` windows per forward."""
        plan = F.sliding_plan(x.shape[2], x.shape[3], sliding, x.device)
        return F.predict_labels_sw(utils.sliding_logits(Gsi, x, plan, args.batch_size), plan, **kw)
    labels_sw = lambda x: filt(heads_sw(x)[0]).cpu().numpy()
    crf = utils.parse_crf(getattr(args, 'crf', ''))
    # --crf: the windowed dense CRF, guided by the images, on Gsi's logits (with --tta: on the views' summed probabilities)
    # what the CRF starts from: Gsi's logits, the views' summed probabilities (--tta) or the windows' blended ones (--sliding)
    crf_start = lambda x, logits: (utils.crf_scores(Gsi, x, size, sliding=sliding, chunk=args.batch_size) if sliding is not None else
                                   utils.crf_scores(Gsi, x, size, tta) if tta else (logits, False))
    labels_crf = lambda x, scores, probs: filt(F.crf_labels(scores, utils.crf_guide(x, size), size, crf, probs=probs)[0]).cpu().numpy()
    cal = utils.parse_calibration(getattr(args, 'calibration', ''))
    keeper = None
    if cal is not None:
        # --calibration: the counts behind ECE / MCE / NLL / Brier of what the saved prediction is taken from (before --components), against
        # the split's ground truth; a temperature grid with --tta, --crf or SSCG_FUSE_PREDICT=0 is refused here
        keeper = utils.runningScore(n_channels, args.dataset)
        keeper.set_calibration(cal, tta=tta, crf=crf, sliding=sliding)

    def scored(x, logits, gt):
        """The prediction of one batch as below, its probabilities scored against `gt` on the way."""
        if crf is not None:
            scores, probs = crf_start(x, logits)
            if crf.iterations == 0:         # no mean-field step, no Q: the logits' own softmax (with --tta this was refused above)
                keeper.update_calibration(gt, scores, size)
                return labels_crf(x, scores, probs)
            out = F.crf_labels(scores, utils.crf_guide(x, size), size, crf, probs=probs, want_q=True)
            keeper.update_calibration(gt, out[3], size, probs=True)
        elif sliding is not None:
            out = heads_sw(x, want_prob=True)
            keeper.update_calibration(gt, out[3], size, probs=True, scale=1.0)
        elif tta:
            out = F.predict_labels_ms(*utils.tta_logits(Gsi, x, tta), size, want_prob=True)
            keeper.update_calibration(gt, out[3], size, probs=True, scale=utils.inv_views(len(tta)))
        else:
            if fused:
                keeper.update_calibration(gt, logits, size)
            else:
                keeper.update_probs(gt, soft(logits))
            return labels(logits)
        return filt(out[0]).cpu().numpy()
    img =lambda x: F.act_fwd(F.to_nhwc(F.upsample_bilinear(Gis(x), size)), F.ACT_TANH)   # Gis -> interp -> Tanh
    Gsi.eval()
    with torch.no_grad():
        for i, (image_test, real_segmentation, image_name) in enumerate(val_loader):
            image_test, real_segmentation = utils.cuda([image_test, real_segmentation], args.gpu_ids)
            if sliding is not None:
                size = tuple(image_test.shape[2:])                    # the batch's own size: what every head below predicts at
            logits = Gsi(image_test) if semi or not (tta or sliding is not None) else None     # the image-regeneration branches stay single-view
            if keeper is not None:
                prediction = scored(image_test, logits, real_segmentation.squeeze(1))
            elif crf is not None:
                prediction = labels_crf(image_test, *crf_start(image_test, logits))
            else:
                prediction = labels_sw(image_test) if sliding is not None else labels_ms(image_test) if tta else labels(logits)
            if not semi:
                out = _mk(args.validation_dir, 'supervised')
                for j in range(prediction.shape[0]):
                    utils.colorize_mask(prediction[j], args.dataset).save(os.path.join(out, image_name[j] + '.png'))
            else:
                onehot = utils.make_one_hot(real_segmentation, args.dataset, args.gpu_ids)
                base = os.path.join(args.validation_dir, 'unsupervised')
                if fused:
                    # Gis -> interp -> Tanh -> un-normalise -> save_image's uint8 pixels in one launch; the fp32 image only where it
                    # goes back into Gsi
                    fake_img = F.predict_image(Gis(soft(logits)), size, want_float=False)[1].cpu().numpy()             # :108-110
                    from_labels, fake_img_from_labels = F.predict_image(Gis(onehot), size)                                # :112-114
                    fake_img_from_labels = fake_img_from_labels.cpu().numpy()
                    regenerated = labels(Gsi(from_labels))                                                                # :115-120
                    save = utils.save_image_u8
                else:
                    fake_img = img(soft(logits))
                    fake_img_from_labels = img(onehot)
                    regenerated = labels(Gsi(fake_img_from_labels))
                    fake_img = F.to_nchw(fake_img).cpu() * 0.5 + 0.5                                      # undo Normalize(.5, .5)
                    fake_img_from_labels = F.to_nchw(fake_img_from_labels).cpu() * 0.5 + 0.5
                    save = utils.save_image
                for j in range(prediction.shape[0]):
                    utils.colorize_mask(prediction[j], args.dataset).save(os.path.join(_mk(base, 'generated_labels'), image_name[j] + '.png'))
                    utils.colorize_mask(regenerated[j], args.dataset).save(os.path.join(_mk(base, 'regenerated_labels'), image_name[j] + '.png'))
                    save(fake_img[j], os.path.join(_mk(base, 'regenerated_image'), image_name[j] + '.jpg'))
                    save(fake_img_from_labels[j], os.path.join(_mk(base, 'image_from_labels'), image_name[j] + '.jpg'))
            print('Epoch-', str(i + 1), ' Done!')
    if keeper is not None:
        s = keeper.get_calibration_scores()
        print('The calibration of the resulting segment maps: ECE %s MCE %s NLL %s Brier %s accuracy %s confidence %s over %d pixels%s' % (
            s["ece"], s["mce"], s["nll"], s["brier"], s["accuracy"], s["confidence"], s["counted"],
            ' | NLL-optimal temperature %s%s' % (s["temperature"], ' (at the end of the grid)' if s["temperature_at_edge"] else '')
            if "temperature" in s else ''))
    print('The iou of the resulting segment maps: ', str(best_iou))
    return best_iou
