#!/usr/bin/env python
"""evaluate() of the g5_eval configuration (tests/golden/meta.json) in a process of its own, so that an environment switch read at
import time can be A/B-ed: prints one JSON line with the confusion matrix, the mIoU and the per-class IoU.
usage: [SSCG_FUSE_PREDICT=0] [SSCG_TRACE=1 | SSCG_RACECHECK=1] python tests/aids/predict_eval.py [semi|sup]
Under SSCG_RACECHECK=1 the stream-ordering checker's report follows and the exit status is 1 if it found anything."""
import contextlib
import importlib
import io
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import PKG_NAME  # noqa: E402
from oracle import fixtures as FX  # noqa: E402

md = importlib.import_module(PKG_NAME + ".model")
F = importlib.import_module(PKG_NAME + ".functional")
kind = sys.argv[1] if len(sys.argv) > 1 else "semi"
cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "meta.json")))["g5_eval"]["config"]
C, H, W, B = cfg["C"], cfg["H"], cfg["W"], cfg["B"]
dev = torch.device("cuda", 0)
args = FX.make_args(dataset=cfg["dataset"], crop_height=H, crop_width=W, batch_size=B, gpu_ids=[0], checkpoint_dir="/tmp/sscg_predict_eval",
                    as_written=True)
with contextlib.redirect_stdout(io.StringIO()):
    m = md.semisuper_cycleGAN(args) if kind == "semi" else md.supervised_model(args)
m.Gsi.load_state_dict(FX.semisup_state_dicts(C, torch.float32, cfg["tag"])["Gsi"], strict=True)
batches = []
for b in range(cfg["batches"]):
    smp = [FX.synth_sample(cfg["tag"] + "/val", b * B + i, C, H, W) for i in range(B)]
    batches.append((torch.stack([a for a, _ in smp]), torch.stack([g for _, g in smp]), ["v"] * B))
torch.cuda.synchronize()
score = m.running_metrics_val
conf = []
fold = score._fold_device


def keep():         # supervised_model.evaluate() resets the matrix after get_scores(): keep the one the scores came from
    fold()
    conf[:] = [score.confusion_matrix.copy()]


score._fold_device = keep
miou, class_iou = m.evaluate(batches)
torch.cuda.synchronize()
print(json.dumps({"fused": bool(F.FUSE_PREDICT[0]), "miou": float(miou), "confusion": conf[0].astype("int64").tolist(),
                  "class_iou": {str(k): (None if v != v else float(v)) for k, v in class_iou.items()}}), flush=True)
if os.environ.get("SSCG_RACECHECK") and not os.environ.get("SSCG_TRACE"):
    rc = importlib.import_module(PKG_NAME + "._lib").dev_tool("racecheck")
    rc.name_streams(F, dev)
    print("launches checked: %d" % rc.CORE.launches)
    core = rc.report(sys.stdout)
    sys.exit(1 if core.reports else 0)
