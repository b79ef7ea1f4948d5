"""Checkpoint files on the host: what train() writes is read back by utils.load_checkpoint with torch's weights-only unpickler, files
in the older format (numpy scalars, the reference's) still load, and nothing else does.

No GPU.  The resume itself (the restored run continues the uninterrupted one bit for bit) is tests/test_resume_gpu.py."""
import contextlib
import io
import math
import pickle

import numpy as np
import pytest
import torch

from conftest import load_sub


def _quiet(fn, *a, **k):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        r = fn(*a, **k)
    return r, out.getvalue()


def _scores_with_an_empty_class(utils):
    """runningScore.get_scores() of a 4-class confusion matrix in which class 2 occurs in neither labels nor predictions: its IoU is
    0 / 0 = NaN.  Returns (miou, class_iou) exactly as the trainers receive them: numpy.float64 scalars."""
    rs = utils.runningScore(4, "acdc")
    lt = np.array([[0, 0, 1, 1, 3, 3, 3, 0]])
    lp = np.array([[0, 1, 1, 1, 3, 0, 3, 0]])
    rs.update(lt, lp)
    score, class_iou = rs.get_scores()
    return score["Mean IoU : \t"], class_iou


def _adam_state_dict():
    """An optimiser state_dict in stock torch.optim.Adam layout after two steps."""
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(3, 4)), torch.nn.Parameter(torch.randn(5))]
    opt = torch.optim.Adam(ps, lr=2e-4, betas=(0.5, 0.999))
    for _ in range(2):
        for p in ps:
            p.grad = torch.randn_like(p)
        opt.step()
    return opt.state_dict()


def test_new_format_round_trip(tmp_path):
    utils = load_sub("utils")
    miou, class_iou = _scores_with_an_empty_class(utils)
    assert type(miou) is np.float64 and all(type(v) is np.float64 for v in class_iou.values())      # what get_scores() hands out
    assert math.isnan(class_iou[2]) and sum(math.isnan(v) for v in class_iou.values()) == 1 and np.isfinite(miou)
    best, cls = utils.checkpoint_scores(miou, class_iou)
    osd = _adam_state_dict()
    torch.manual_seed(1)
    net = {"conv.weight": torch.randn(4, 3, 3, 3), "bn.num_batches_tracked": torch.tensor(7)}
    path = str(tmp_path / "new.ckpt")
    utils.save_checkpoint({"epoch": 3, "Gsi": net, "gsi_optimizer": osd, "best_iou": best, "class_iou": cls}, path)
    back, printed = _quiet(utils.load_checkpoint, path)
    assert "succeed" in printed
    assert type(back["best_iou"]) is float and back["best_iou"] == float(miou)
    assert list(back["class_iou"]) == [0, 1, 2, 3] and all(type(k) is int for k in back["class_iou"])
    assert all(type(v) is float for v in back["class_iou"].values())
    want = [float(class_iou[k]) for k in range(4)]
    got = [back["class_iou"][k] for k in range(4)]
    assert np.array_equal(np.array(got), np.array(want), equal_nan=True) and math.isnan(got[2])
    assert back["epoch"] == 3 and type(back["epoch"]) is int
    assert all(torch.equal(back["Gsi"][k], net[k]) and back["Gsi"][k].dtype == net[k].dtype for k in net)
    assert back["gsi_optimizer"]["param_groups"] == osd["param_groups"]
    n_t = 0
    for i, st in osd["state"].items():
        assert set(back["gsi_optimizer"]["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        for k, v in st.items():
            assert torch.equal(back["gsi_optimizer"]["state"][i][k], v)
            n_t += 1
    print("new format: best_iou %r, class_iou %r, %d net tensors and %d optimiser tensors read back by the weights-only unpickler"
          % (back["best_iou"], back["class_iou"], len(net), n_t))
    # the file itself needs no allow-list: torch's own default loading reads it
    plain = torch.load(path, map_location="cpu", weights_only=True)
    assert plain["best_iou"] == best


def test_old_format_still_loads(tmp_path):
    """The format train() wrote before checkpoint_scores() (and the reference writes): numpy.float64 for best_iou and in class_iou.
    torch's default loading refuses it; utils.load_checkpoint reads it, values unchanged."""
    utils = load_sub("utils")
    miou, class_iou = _scores_with_an_empty_class(utils)
    path = str(tmp_path / "old.ckpt")
    torch.save({"epoch": 1, "Gsi": {"w": torch.ones(2)}, "best_iou": miou, "class_iou": class_iou}, path)
    with pytest.raises(pickle.UnpicklingError):
        torch.load(path, map_location="cpu", weights_only=True)
    back, printed = _quiet(utils.load_checkpoint, path)
    assert "succeed" in printed and back["epoch"] == 1 and torch.equal(back["Gsi"]["w"], torch.ones(2))
    assert float(back["best_iou"]) == float(miou)
    assert np.array_equal(np.array([float(back["class_iou"][k]) for k in range(4)]), np.array([float(class_iou[k]) for k in range(4)]),
                          equal_nan=True)
    # the allow-list is not left behind: the default loading still refuses the file afterwards
    with pytest.raises(pickle.UnpicklingError):
        torch.load(path, map_location="cpu", weights_only=True)


def test_old_format_under_numpy_1_names_still_loads(tmp_path):
    """A file written under numpy 1.x names the scalar reconstructor `numpy.core.multiarray.scalar`.  Where this numpy still answers
    that path (2.x does, with the function of the new path), such a file is written here by pickling through a stand-in that carries
    the old name, and must load: the allow-list covers the name the FILE uses."""
    import importlib
    import warnings
    utils = load_sub("utils")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            old = importlib.import_module("numpy.core.multiarray")
            real = old.scalar
        except (ImportError, AttributeError):
            pytest.skip("this numpy has no numpy.core.multiarray.scalar")
    if real.__module__ == "numpy.core.multiarray":
        pytest.skip("numpy 1.x: test_old_format_still_loads writes this very format")

    def scalar(*a):
        return real(*a)
    scalar.__module__, scalar.__qualname__, scalar.__name__ = "numpy.core.multiarray", "scalar", "scalar"

    class Numpy1Scalar(object):
        def __init__(self, v):
            self.v = np.float64(v)

        def __reduce__(self):
            return (scalar, self.v.__reduce__()[1])
    path = str(tmp_path / "numpy1.ckpt")
    old.scalar = scalar             # (pickle checks that the name it writes resolves to the object it was given)
    try:
        torch.save({"epoch": 1, "best_iou": Numpy1Scalar(0.25), "class_iou": {0: Numpy1Scalar(float("nan"))}}, path)
    finally:
        del old.scalar
    with pytest.raises(pickle.UnpicklingError, match=r"numpy\.core\.multiarray\.scalar"):
        torch.load(path, map_location="cpu", weights_only=True)
    back, _ = _quiet(utils.load_checkpoint, path)
    assert type(back["best_iou"]) is np.float64 and back["best_iou"] == 0.25 and math.isnan(back["class_iou"][0])


class _NotANumber(object):
    def __init__(self):
        self.x = 1


def test_unknown_classes_are_refused(tmp_path):
    utils = load_sub("utils")
    path = str(tmp_path / "bad.ckpt")
    torch.save({"epoch": 1, "best_iou": 0.5, "extra": _NotANumber()}, path)
    with pytest.raises(pickle.UnpicklingError):
        _quiet(utils.load_checkpoint, path)
    # ... also beside numpy scalars (the retry's allow-list holds those and nothing else)
    torch.save({"epoch": 1, "best_iou": np.float64(0.5), "extra": _NotANumber()}, path)
    with pytest.raises(pickle.UnpicklingError):
        _quiet(utils.load_checkpoint, path)
    # a numpy ARRAY is not a scalar: its reconstructor is not on the list
    torch.save({"epoch": 1, "best_iou": np.arange(3.0)}, path)
    with pytest.raises(pickle.UnpicklingError):
        _quiet(utils.load_checkpoint, path)


def test_missing_file_raises_file_not_found(tmp_path):
    utils = load_sub("utils")
    with pytest.raises(FileNotFoundError):
        _quiet(utils.load_checkpoint, str(tmp_path / "nothing_here.ckpt"))
