"""The per-epoch image panels (sscg_panel_labels / sscg_panel_range / sscg_panel_grid) on a GPU-less host: the vectorised
PIL_to_tensor against the reference's recorded output, the host make_grid + grid_to_u8 against a plain-numpy restatement of the
arithmetic include/sscg.h states (`ref_range`, `ref_grid`: tests/test_panels_gpu.py holds the kernels to the same two functions), and
the argument errors of the three entries, returned before any HIP call.  Every comparison is equality."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_sub

HERE = os.path.dirname(os.path.abspath(__file__))
IMAGE, COLOUR, GREY = 0, 1, 2
DATASETS = ("voc2012", "cityscapes", "acdc")
f32 = np.float32


# ------------------------------------------------------------------------------------------ the restatement
def panel_values(src, kind, scale=1.0, shift=0.0, palette=None):
    """fp32 [N,3,H,W]: the pre-normalisation value v of every pixel and channel.  src: IMAGE fp32 [N,C,H,W] (C in {1, 3}), COLOUR
    integer ids [N,H,W] with palette uint8 [256,3], GREY integer ids [N,H,W]."""
    src = np.asarray(src)
    if kind == IMAGE:
        v = (src.astype(f32) * f32(scale)).astype(f32) + f32(shift)         # a multiply, then an add, each rounded to fp32
        v = v.astype(f32)
        return np.concatenate((v, v, v), 1) if v.shape[1] == 1 else v
    if kind == COLOUR:
        pal = np.asarray(palette, dtype=np.uint8).reshape(256, 3)
        return np.ascontiguousarray(pal[src.astype(np.int64)].astype(f32).transpose(0, 3, 1, 2))
    v = src.astype(np.int64).astype(f32)[:, None]
    return np.concatenate((v, v, v), 1)


def ref_range(src, kind, scale=1.0, shift=0.0, palette=None):
    v = panel_values(src, kind, scale, shift, palette)
    return np.array([v.min(), v.max()], dtype=f32)


def ref_grid(src, kind, rng, nrow, padding, scale=1.0, shift=0.0, palette=None):
    """uint8 [3,GH,GW]: make_grid(nrow, padding, normalize=True) + the byte conversion, operation by operation as the header has it"""
    v = panel_values(src, kind, scale, shift, palette)
    lo, hi = f32(rng[0]), f32(rng[1])
    d = f32(max(float(hi) - float(lo), 1e-5))
    u = ((v - lo).astype(f32) / d).astype(f32)
    b = np.minimum(np.maximum((u * f32(255.0)).astype(f32), f32(0.0)), f32(255.0)).astype(np.uint8)
    n, _, h, w = b.shape
    if n == 1:
        return b[0].copy()
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    grid = np.zeros((3, ymaps * (h + padding) + padding, xmaps * (w + padding) + padding), dtype=np.uint8)
    for k in range(n):
        y0, x0 = (k // xmaps) * (h + padding) + padding, (k % xmaps) * (w + padding) + padding
        grid[:, y0:y0 + h, x0:x0 + w] = b[k]
    return grid


def panel_case(kind, n, h, w, seed, c=3, dataset="voc2012", variant="random"):
    """(src, scale, shift, palette) of one test panel.  variant: random | constant | negative (images below zero)"""
    utils = load_sub("utils")
    g = np.random.RandomState(seed)
    pal = np.asarray(utils.PALETTES[dataset], dtype=np.uint8).reshape(256, 3)
    if kind == IMAGE:
        x = g.standard_normal((n, c, h, w)).astype(f32)
        if variant == "constant":
            x[:] = f32(0.25)
        if variant == "negative":
            x = (-np.abs(x) - f32(3.0)).astype(f32)
        return x, 0.5, 0.5, None
    classes = utils.CLASSES[dataset]
    ids = g.randint(0, classes, (n, h, w))
    if kind == GREY:
        ids[g.rand(n, h, w) < 0.1] = 255                 # the "void" label of VOC
        if variant == "constant":
            ids[:] = 7
        return ids.astype(np.int64), 1.0, 0.0, None
    if variant == "constant":
        grey = [i for i in range(classes) if pal[i, 0] == pal[i, 1] == pal[i, 2]]
        ids[:] = grey[0]                                 # a class whose three channels are equal (VOC's black class 0): hi == lo
    return ids.astype(np.uint8), 1.0, 0.0, pal


# ------------------------------------------------------------------------------------------ PIL_to_tensor
@pytest.mark.parametrize("dataset", DATASETS)
def test_pil_to_tensor_equals_the_reference(dataset):
    utils = load_sub("utils")
    gold = np.load(os.path.join(HERE, "golden", "g9_panels.npz"))
    ids, want = gold["ids_" + dataset], gold["rgb_" + dataset]
    assert sorted(set(ids.ravel().tolist())) == list(range(utils.CLASSES[dataset]))
    got = utils.PIL_to_tensor(utils.colorize_mask(ids, dataset), dataset)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 16, 16)
    assert np.array_equal(got.numpy(), want)
    # and the restatement's COLOUR values are the same numbers
    pal = np.asarray(utils.PALETTES[dataset], dtype=np.uint8).reshape(256, 3)
    assert np.array_equal(panel_values(ids[None], COLOUR, palette=pal)[0], want)


# ------------------------------------------------------------------------------------------ make_grid + grid_to_u8
def host_tensor(utils, src, kind, scale, shift, dataset):
    """what the separate-passes path of model.panels() hands to make_grid"""
    if kind == IMAGE:
        return torch.from_numpy(src) * scale + shift
    if kind == COLOUR:
        return torch.stack([utils.PIL_to_tensor(utils.colorize_mask(m, dataset), dataset) for m in src])
    t = torch.from_numpy(src)
    return t.reshape(t.shape[0], 1, t.shape[1], t.shape[2]).float().expand(-1, 3, -1, -1)


@pytest.mark.parametrize("padding", [2, 0])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
@pytest.mark.parametrize("kind,c,variant", [(IMAGE, 3, "random"), (IMAGE, 1, "random"), (IMAGE, 3, "negative"), (IMAGE, 3, "constant"),
                                            (COLOUR, 1, "random"), (COLOUR, 1, "constant"), (GREY, 1, "random"), (GREY, 1, "constant")])
def test_host_make_grid_equals_the_restatement(kind, c, variant, n, padding):
    utils = load_sub("utils")
    h, w = 5, 7
    for dataset in (DATASETS if kind == COLOUR else DATASETS[:1]):
        src, scale, shift, pal = panel_case(kind, n, h, w, 100 * kind + 10 * n + padding, c, dataset, variant)
        rng = ref_range(src, kind, scale, shift, pal)
        want = ref_grid(src, kind, rng, 2, padding, scale, shift, pal)
        t = host_tensor(utils, src, kind, scale, shift, dataset)
        got = utils.grid_to_u8(utils.make_grid(t, nrow=2, padding=padding, normalize=True))
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert np.array_equal(got, want)
        xmaps = min(2, n)
        ymaps = -(-n // xmaps)
        assert want.shape == ((3, h, w) if n == 1 else (3, ymaps * (h + padding) + padding, xmaps * (w + padding) + padding))
        if variant == "constant":
            assert rng[0] == rng[1] and not want.any()                  # hi == lo: d = 1e-5, every byte 0
        else:
            assert want.max() == 255 and want.min() == 0                # the extremes map to the ends of the byte range
        if variant == "negative":
            assert rng[1] < 0
        if n in (3, 5) and padding == 2:                                # the unused cell and the borders are 0
            assert not want[:, -(h + padding):, -(w + padding):].any() and not want[:, :padding].any() and not want[:, :, :padding].any()


def test_make_grid_without_normalisation_places_the_tiles():
    utils = load_sub("utils")
    t = torch.arange(3 * 1 * 2 * 3, dtype=torch.float32).reshape(3, 1, 2, 3) + 1.0
    g = utils.make_grid(t, nrow=2, padding=1).numpy()
    assert g.shape == (3, 7, 9) and np.array_equal(g[0], g[2])
    assert np.array_equal(g[1, 1:3, 1:4], t[0, 0].numpy()) and np.array_equal(g[1, 1:3, 5:8], t[1, 0].numpy())
    assert np.array_equal(g[1, 4:6, 1:4], t[2, 0].numpy()) and not g[:, 4:6, 5:8].any() and not g[:, 0].any() and not g[:, 3].any()
    assert tuple(utils.make_grid(t[:1], nrow=2).shape) == (3, 2, 3)


# ------------------------------------------------------------------------------------------ the C entries and the wrappers
def test_the_three_entries_are_bound():
    L = load_sub("_lib")
    assert len(L.SIGNATURES["sscg_panel_labels"][1]) == 10 and len(L.SIGNATURES["sscg_panel_range"][1]) == 11
    assert len(L.SIGNATURES["sscg_panel_grid"][1]) == 14 and L.SIGNATURES["sscg_panel_range_workspace"][0] is C.c_size_t
    assert (L.PANEL_IMAGE, L.PANEL_COLOUR, L.PANEL_GREY) == (IMAGE, COLOUR, GREY)
    src = open(os.path.join(ROOT, "include", "sscg.h")).read()
    for name, val in (("IMAGE", 0), ("COLOUR", 1), ("GREY", 2)):
        assert "#define SSCG_PANEL_%s %d" % (name, val) in src


def test_argument_errors_are_returned_before_any_launch():
    lib = load_sub("_lib").lib
    one = C.c_void_p(16)          # never dereferenced
    BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
    # labels
    assert lib.sscg_panel_labels(None, 1, 9, 9, 21, 32, 32, one, one, None) == BAD_ARG                  # no logits
    assert lib.sscg_panel_labels(one, 1, 9, 9, 21, 32, 32, None, one, None) == BAD_ARG                  # label_u8 is required
    assert lib.sscg_panel_labels(one, 1, 9, 9, 0, 32, 32, one, None, None) == BAD_ARG
    assert lib.sscg_panel_labels(one, 1, 9, 9, 21, 0, 32, one, None, None) == BAD_ARG
    assert lib.sscg_panel_labels(one, 1, 9, 9, 65, 32, 32, one, None, None) == UNSUPPORTED              # C > 64
    assert lib.sscg_panel_labels(one, 64, 9, 9, 21, 8192, 8192, one, None, None) == UNSUPPORTED         # >= 2^31 ids
    assert lib.sscg_panel_labels(one, 8, 9, 9, 21, 4096, 4096, one, one, None) == UNSUPPORTED           # >= 2^31 one-hot floats
    # range
    assert lib.sscg_panel_range(None, IMAGE, 10, 3, 0.5, 0.5, None, one, None, 0, None) == BAD_ARG
    assert lib.sscg_panel_range(one, IMAGE, 10, 3, 0.5, 0.5, None, None, None, 0, None) == BAD_ARG      # no result
    assert lib.sscg_panel_range(one, 3, 10, 3, 0.5, 0.5, None, one, None, 0, None) == BAD_ARG           # unknown kind
    assert lib.sscg_panel_range(one, IMAGE, 10, 2, 0.5, 0.5, None, one, None, 0, None) == BAD_ARG       # C outside {1, 3}
    assert lib.sscg_panel_range(one, GREY, 10, 3, 1.0, 0.0, None, one, None, 0, None) == BAD_ARG        # ids have one channel
    assert lib.sscg_panel_range(one, COLOUR, 10, 1, 1.0, 0.0, None, one, None, 0, None) == BAD_ARG      # COLOUR without a palette
    assert lib.sscg_panel_range(one, IMAGE, 0, 3, 0.5, 0.5, None, one, None, 0, None) == BAD_ARG
    assert lib.sscg_panel_range_workspace(10, 3) == 0 and lib.sscg_panel_range_workspace(1 << 20, 3) > 0
    assert lib.sscg_panel_range(one, IMAGE, 1 << 20, 3, 0.5, 0.5, None, one, None, 0, None) == WORKSPACE
    # grid
    assert lib.sscg_panel_grid(None, IMAGE, 2, 5, 7, 3, 0.5, 0.5, None, one, 2, 2, one, None) == BAD_ARG
    assert lib.sscg_panel_grid(one, IMAGE, 2, 5, 7, 3, 0.5, 0.5, None, None, 2, 2, one, None) == BAD_ARG        # no range
    assert lib.sscg_panel_grid(one, IMAGE, 2, 5, 7, 3, 0.5, 0.5, None, one, 2, 2, None, None) == BAD_ARG        # no grid
    assert lib.sscg_panel_grid(one, 7, 2, 5, 7, 3, 0.5, 0.5, None, one, 2, 2, one, None) == BAD_ARG             # unknown kind
    assert lib.sscg_panel_grid(one, IMAGE, 2, 5, 7, 4, 0.5, 0.5, None, one, 2, 2, one, None) == BAD_ARG         # C outside {1, 3}
    assert lib.sscg_panel_grid(one, IMAGE, 0, 5, 7, 3, 0.5, 0.5, None, one, 2, 2, one, None) == BAD_ARG
    assert lib.sscg_panel_grid(one, IMAGE, 2, 5, 7, 3, 0.5, 0.5, None, one, 0, 2, one, None) == BAD_ARG         # nrow
    assert lib.sscg_panel_grid(one, IMAGE, 2, 5, 7, 3, 0.5, 0.5, None, one, 2, -1, one, None) == BAD_ARG        # padding
    assert lib.sscg_panel_grid(one, COLOUR, 2, 5, 7, 1, 1.0, 0.0, None, one, 2, 2, one, None) == BAD_ARG        # no palette
    assert lib.sscg_panel_grid(one, GREY, 64, 4096, 4096, 1, 1.0, 0.0, None, one, 2, 2, one, None) == UNSUPPORTED   # >= 2^31 bytes
    assert lib.sscg_panel_grid(one, GREY, 2, 1 << 30, 1 << 30, 1, 1.0, 0.0, None, one, 2, 2, one, None) == UNSUPPORTED


def test_wrappers_refuse_cpu_tensors():
    F, L = load_sub("functional"), load_sub("_lib")
    with pytest.raises(L.SscgError):
        F.panel_labels(torch.zeros(1, 21, 9, 9), (32, 32))
    with pytest.raises(L.SscgError):
        F.panel_range(torch.zeros(1, 3, 9, 9), F.PANEL_IMAGE, 0.5, 0.5)
    with pytest.raises(L.SscgError):
        F.panel_grid(torch.zeros(1, 9, 9, dtype=torch.int64), F.PANEL_GREY, torch.zeros(2))
    assert isinstance(F.FUSE_PANELS[0], bool)
    assert F.panel_grid_shape(1, 5, 7, 2, 2) == (3, 5, 7) and F.panel_grid_shape(5, 5, 7, 2, 2) == (3, 23, 20)


def test_the_switch_is_read_from_the_environment():
    """SSCG_FUSE_PANELS=0 in a fresh process turns model.panels() back to the separate passes."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); from conftest import load_sub; "
            "print(load_sub('functional').FUSE_PANELS[0])" % (ROOT, os.path.join(ROOT, "tests")))
    for val, want in ((None, "True"), ("0", "False")):
        env = dict(os.environ)
        env.pop("SSCG_FUSE_PANELS", None)
        if val is not None:
            env["SSCG_FUSE_PANELS"] = val
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.stdout.strip().splitlines()[-1] == want, (r.stdout, r.stderr[-2000:])


def test_the_panel_tags_are_the_references():
    md = load_sub("model")
    assert md.PANEL_TAGS == ('Generated segmented image: ', 'Generated image back from segmentation: ', 'Ground truth for the image: ',
                             'Image generated from val labels: ', 'Labels generated back from the cycle: ')
    assert md.SUPERVISED_PANEL_TAGS == ('Generated segmented image', 'Ground truth for the image')
    import main
    assert main.get_args([]).panels is None and main.get_args(["--panels", "out"]).panels == "out"
