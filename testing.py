"""`python main.py --testing ...`: the reference's testing.py (:17-100) on the MI355X backend: paletted
predictions of Gsi over the test split under `--results_dir/{supervised,unsupervised}`.
As written there, Gsi is built as `resnet_9blocks_softmax` (testing.py:40) although training saves a DeepLab
`Gsi`: loading then fails, and the reference prints ' [*] No checkpoint!' and goes on with the initial weights.
Here only a missing file does that; a file that exists and does not fit the network stops the run with torch's
error (its predictions would be those of a random network).  `--testing_gen deeplab` builds the network the
checkpoint actually holds."""
import importlib
import os

import torch

PKG = "semi-supervised-segmentation-cyclegan_amd"


def test(args, test_loader=None):
    F = importlib.import_module(PKG + ".functional")
    arch = importlib.import_module(PKG + ".arch")
    utils = importlib.import_module(PKG + ".utils")
    n_channels = {'voc2012': 21, 'cityscapes': 20, 'acdc': 4}[args.dataset]
    dev = torch.device("cuda", args.gpu_ids[0])
    # --sliding: the images keep the evaluation size, Gsi runs on overlapping crop-sized windows, the label maps have that size
    sliding = utils.parse_sliding(getattr(args, 'sliding', ''), (args.crop_height, args.crop_width))
    if test_loader is None:
        du = importlib.import_module(PKG + ".data_utils")
        from torch.utils.data import DataLoader
        tr = du.get_transformation(sliding.size if sliding is not None else (args.crop_height, args.crop_width), resize=True,
                                   dataset=args.dataset, device_finish=True)
        cls = {'voc2012': du.VOCDataset, 'cityscapes': du.CityscapesDataset, 'acdc': du.ACDCDataset}[args.dataset]
        root = {'voc2012': './data/VOC2012', 'cityscapes': './data/Cityscape', 'acdc': './data/ACDC'}[args.dataset]
        test_set = cls(root_path=root, name='test', ratio=0.5, transformation=tr, augmentation=None)
        test_loader = du.DeviceLoader(DataLoader(test_set, batch_size=args.batch_size, shuffle=False), tr, dev)
    net = getattr(args, 'testing_gen', None) or 'resnet_9blocks_softmax'
    Gsi = arch.define_Gen(input_nc=3, output_nc=n_channels, ngf=args.ngf, netG=net, norm=args.norm,
                          use_dropout=not args.no_dropout, gpu_ids=args.gpu_ids)
    semi = args.model == 'semisupervised_cycleGAN'
    try:
        ckpt = utils.load_checkpoint('%s/latest_%s.ckpt' % (args.checkpoint_dir, 'semisuper_cycleGAN' if semi else 'supervised_model'))
    except FileNotFoundError:
        ckpt = None
        print(' [*] No checkpoint!')
    if ckpt is not None:
        Gsi.load_state_dict(ckpt['Gsi'])
        if getattr(args, 'ema_decay', None) is not None and 'Gsi_ema' in ckpt:      # --ema_decay: the averaged parameters (buffers stay)
            Gsi.load_state_dict(ckpt['Gsi_ema'], strict=False)
    out = os.path.join(args.results_dir, 'unsupervised' if semi else 'supervised')
    os.makedirs(out, exist_ok=True)
    tta = utils.parse_tta(getattr(args, 'tta', ''))
    if sliding is not None and tta:
        raise ValueError("--sliding does not combine with --tta: 'flip' is --sliding's own key")
    crf = utils.parse_crf(getattr(args, 'crf', ''))
    comp = utils.parse_components(getattr(args, 'components', ''))
    # --components: the predicted label maps go through the connected-component filter on the device before they are copied and saved
    filt = lambda t: t if comp is None else F.component_filter(t, n_channels, comp)[0]
    Gsi.eval()
    with torch.no_grad():
        for i, (image_test, image_name) in enumerate(test_loader):
            image_test = utils.cuda(image_test, args.gpu_ids)
            if sliding is not None:     # --sliding: Gsi on the windows of the batch, blended into one uint8 map at the images' size
                size = image_test.shape[2:]
                if crf is not None:
                    scores, probs = utils.crf_scores(Gsi, image_test, size, sliding=sliding, chunk=args.batch_size)
                    prediction = filt(F.crf_labels(scores, image_test, size, crf, probs=probs)[0]).cpu().numpy()
                else:
                    plan = F.sliding_plan(size[0], size[1], sliding, image_test.device)
                    prediction = filt(F.predict_labels_sw(utils.sliding_logits(Gsi, image_test, plan, args.batch_size), plan)[0]).cpu().numpy()
                for j in range(prediction.shape[0]):
                    utils.colorize_mask(prediction[j], args.dataset).save(os.path.join(out, image_name[j] + '.png'))
                print('Epoch-', str(i + 1), ' Done!')
                continue
            logits = None if tta else Gsi(image_test)
            if crf is not None:     # --crf: the windowed dense CRF, guided by the images, at the size the plain path predicts at
                size = image_test.shape[2:] if tta else logits.shape[2:]
                scores, probs = utils.crf_scores(Gsi, image_test, size, tta) if tta else (logits, False)
                prediction = filt(F.crf_labels(scores, utils.crf_guide(image_test, size), size, crf, probs=probs)[0]).cpu().numpy()
            elif tta:           # --tta: Gsi once per view, the views fused into one uint8 map at the images' size
                prediction = filt(F.predict_labels_ms(*utils.tta_logits(Gsi, image_test, tta), image_test.shape[2:])[0]).cpu().numpy()
            elif F.FUSE_PREDICT[0]:          # softmax -> argmax on the net's own output: one launch, a uint8 map (identity resize)
                prediction = filt(F.predict_labels(logits, logits.shape[2:])[0]).cpu().numpy()
            else:
                prediction = filt(F.argmax_index(F.softmax2d(logits))).cpu().numpy()
            for j in range(prediction.shape[0]):
                utils.colorize_mask(prediction[j], args.dataset).save(os.path.join(out, image_name[j] + '.png'))
            print('Epoch-', str(i + 1), ' Done!')
