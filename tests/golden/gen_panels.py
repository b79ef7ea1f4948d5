#!/usr/bin/env python
"""Golden vectors of the per-epoch image panels.  RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference, read-only).

Imports the reference's utils.py behind gen_golden.py's `torchvision` / `tensorboardX` stubs and records, per dataset,
`PIL_to_tensor(colorize_mask(ids, dataset), dataset)` - the reference's per-pixel double loop - for one 16x16 id map that holds
every class id of the dataset.  No reference source is copied: the fixture is numbers (tests/golden/g9_panels.npz, a few KB).
Usage: python tests/golden/gen_panels.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

from gen_golden import REF, install_stubs  # noqa: E402  (puts the repository root and the reference on sys.path)

CLASSES = {"voc2012": 21, "cityscapes": 20, "acdc": 4}


def id_map(dataset):
    """uint8 [16,16]: every class id of the dataset, in a seeded order"""
    c = CLASSES[dataset]
    ids = np.arange(256) % c
    np.random.RandomState(9 + c).shuffle(ids)
    return ids.reshape(16, 16).astype(np.uint8)


def main():
    install_stubs()
    assert os.path.isdir(REF), "the reference is not on this machine"
    import utils as rutils
    assert os.path.dirname(os.path.abspath(rutils.__file__)) == REF
    out = {}
    for ds, c in CLASSES.items():
        ids = id_map(ds)
        assert sorted(set(ids.ravel().tolist())) == list(range(c))
        rgb = rutils.PIL_to_tensor(rutils.colorize_mask(ids, ds), ds).numpy()
        assert rgb.dtype == np.float32 and rgb.shape == (3, 16, 16)
        out["ids_" + ds] = ids
        out["rgb_" + ds] = rgb
    path = os.path.join(HERE, "g9_panels.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
