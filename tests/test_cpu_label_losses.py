"""--label_loss without a GPU: the class names, the float64 restatement of the losses (tests/_label_losses_ref.py) against torch
autograd, the counts file of CrossEntropyLossClassImbalance, what train.build_graph refuses before it touches a device, and the
checkpoint key."""
import types

import numpy as np
import pytest
import torch

import _label_losses_ref as ref
from efficientvideoclassification_youtube8m_amd import frame_level_models, losses, ops, train
from efficientvideoclassification_youtube8m_amd.flags import FLAGS

TEN = ("CrossEntropyLoss", "CrossEntropyLossWithSparsity", "CrossEntropyLossTop50", "PWELoss", "CrossEntropyLossClassImbalance",
       "CrossEntropyLossPositives", "NewLoss", "HingeLoss", "SoftmaxLoss", "BaseLoss")


@pytest.fixture(autouse=True)
def _clean_flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


def test_the_ten_class_names_resolve():
    for name in TEN:
        cls = train.find_class_by_name(name, [losses])
        assert isinstance(cls, type) and issubclass(cls, losses.BaseLoss) and cls.__name__ == name
        cls()                                                   # constructing a loss reads no file and touches no device
    for kind, name in ref.CLASS_NAMES.items():
        assert getattr(losses, name).kind == ref.KIND_IDS[kind] == getattr(ops, "LOSS_" + kind)
    assert losses.CrossEntropyLoss.kind is None
    assert isinstance(losses.resolve(None), losses.CrossEntropyLoss) and isinstance(losses.resolve("HingeLoss"), losses.HingeLoss)
    with pytest.raises(ValueError, match="label_loss"):
        losses.resolve("NoSuchLoss")


def test_pwe_loss_refuses_itself():
    with pytest.raises(NotImplementedError, match=r"\[128, 4716\]"):
        losses.PWELoss().calculate_loss(torch.zeros(2, 3), torch.zeros(2, 3))
    with pytest.raises(NotImplementedError, match="PWELoss"):
        train.build_graph(frame_level_models.HierarchicalLstmModel(), losses.PWELoss(), 128, 4, 10, "cpu")


def _torch_loss(kind, p, y, w):
    """sum_b row loss in torch float64 with the graph the reference builds: detach() on the masks and the threshold, clamp for the hinge."""
    eps = 10e-6
    a, b = p + eps, 1 - p + eps
    ce = -(y * torch.log(a) + (1 - y) * torch.log(b))
    if kind == "WITH_SPARSITY":
        return (ce + 0.1 * p).sum()
    if kind == "TOP50":
        t = torch.topk(p.detach(), 50, dim=1).values[:, 49:50]
        return ((p.detach() >= t).double() * ce * (4716.0 / 50.0)).sum()
    if kind == "CLASS_IMBALANCE":
        return (-(w[None, :] * y * torch.log(a) + (1 - y) * torch.log(b))).sum()
    if kind == "POSITIVES":
        return (-(y * torch.log(a))).sum()
    if kind == "NEW":
        pd = p.detach()
        # the threshold in float32, as the f32 graph takes it
        mpp = torch.clamp((pd * y + (1 - y)).min().float() - torch.tensor(0.1, dtype=torch.float32), min=0.1)
        bp = (pd.float() < torch.tensor(0.9, dtype=torch.float32)).double()
        bn = ((pd * (1 - y)).float() > mpp).double()
        return (-(bp * y * torch.log(a) + bn * (1 - y) * torch.log(b))).sum()
    if kind == "HINGE":
        return torch.clamp(1 - (2 * y - 1) * p, min=0).sum()
    yhat = y / torch.clamp(y.sum(1, keepdim=True), min=10e-8)
    return -(yhat * torch.log_softmax(p, dim=1)).sum()


@pytest.mark.parametrize("kind,wide", [(k, False) for k in ref.KINDS] + [("HINGE", True), ("SOFTMAX", True)])
def test_reference_agrees_with_torch_float64_autograd(kind, wide):
    B, V = 5, 64
    p32, y8 = ref.make_inputs(kind, B, V, seed=3, wide=wide)
    w32 = ref.make_weights(V) if kind == "CLASS_IMBALANCE" else None
    want = ref.reference(kind, p32, y8, w32)
    p = torch.from_numpy(p32.astype(np.float64)).requires_grad_(True)
    y = torch.from_numpy(y8.astype(np.float64))
    w = None if w32 is None else torch.from_numpy(w32.astype(np.float64))
    total = _torch_loss(kind, p, y, w)
    total.backward()
    assert abs(float(total.detach()) / B - want["loss"]) <= 1e-10 * max(1.0, abs(want["loss"]))
    err = (p.grad.numpy() - want["grad"])
    assert np.all(np.abs(err) <= 1e-10 * np.maximum(1.0, want["mag"])), float(np.abs(err).max())
    assert np.all(want["mag"] >= np.abs(want["grad"]) - 1e-300)
    if kind == "NEW":                                           # the generator puts elements on both sides of both thresholds
        pos = y8 != 0
        assert want["bp"][pos].min() == 0 and want["bp"][pos].max() == 1 and want["bn"][~pos].min() == 0 and want["bn"][~pos].max() == 1
        assert want["mpp"] == pytest.approx(0.25, abs=1e-6)
    if kind == "TOP50":
        assert np.all(want["mask"].sum(1) == 50)


def test_counts_file(tmp_path):
    V = 7
    counts = [1, 10, 100, 4906660, 1401828, 6308488, 3]
    good = tmp_path / "counts_tv"
    good.write_text("".join("%d\n" % c for c in counts))
    w = losses.load_class_weights(str(good), V)
    want = np.array([np.float32(1.0 / np.sqrt(c / (4906660.0 + 1401828.0))) for c in counts], dtype=np.float32)
    assert w.dtype == np.float32 and np.array_equal(w, want) and np.array_equal(w, ref.class_weights_from_counts(counts))
    assert w[5] == 1.0
    FLAGS.parse(["--label_loss_counts_file", str(good)])
    fn = losses.CrossEntropyLossClassImbalance()
    fn.check(V)
    assert np.array_equal(fn.host_weights(V), want)
    with pytest.raises(ValueError, match="--label_loss_counts_file"):
        losses.CrossEntropyLossClassImbalance().check(V + 1)    # a wrong line count
    FLAGS.reset()
    assert FLAGS.label_loss_counts_file == "counts_tv"
    with pytest.raises(ValueError, match="--label_loss_counts_file .*missing"):
        losses.load_class_weights(str(tmp_path / "missing"), V)
    short = tmp_path / "short"
    short.write_text("".join("%d\n" % c for c in counts[:-1]))
    with pytest.raises(ValueError, match="--label_loss_counts_file .*6 lines for 7 classes"):
        losses.load_class_weights(str(short), V)
    zero = tmp_path / "zero"
    zero.write_text("".join("%d\n" % c for c in [5, 0] + counts[2:]))
    with pytest.raises(ValueError, match="--label_loss_counts_file .*class 1 is 0"):
        losses.load_class_weights(str(zero), V)
    FLAGS.parse(["--label_loss_counts_file", str(tmp_path / "missing")])
    with pytest.raises(ValueError, match="--label_loss_counts_file"):       # build time, before a device is asked for anything
        train.build_graph(frame_level_models.HierarchicalLstmModel(), losses.CrossEntropyLossClassImbalance(), 128, 4, 10, "cpu")


def test_build_graph_refuses_serial_modes_with_another_loss(tmp_path):
    model = frame_level_models.HierarchicalLstmModel()
    FLAGS.parse(["--teacher_dir", "/t/"])
    with pytest.raises(ValueError, match=r"--label_loss HingeLoss with --teacher_dir / --serial_student_dirs"):
        train.build_graph(model, losses.HingeLoss(), 128, 4, 10, "cpu")
    FLAGS.reset()
    FLAGS.parse(["--teacher_dir", "/t/", "--serial_student_dirs", "%s,%s" % (tmp_path / "a", tmp_path / "b")])
    with pytest.raises(ValueError, match=r"--label_loss SoftmaxLoss with --teacher_dir / --serial_student_dirs"):
        train.build_graph(model, losses.SoftmaxLoss(), 128, 4, 10, "cpu")


def test_main_refuses_before_it_touches_a_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("a device was selected"))
    with pytest.raises(ValueError, match="--label_loss HingeLoss with --teacher_dir"):
        train.main(["--teacher_dir", "/t/", "--label_loss", "HingeLoss"])
    FLAGS.reset()
    with pytest.raises(NotImplementedError, match="PWELoss"):
        train.main(["--label_loss", "PWELoss"])


def test_build_graph_refuses_top50_below_50_classes(monkeypatch):
    monkeypatch.setattr(train, "NUM_CLASSES", 49)
    with pytest.raises(ValueError, match="CrossEntropyLossTop50 needs at least 50 classes"):
        train.build_graph(frame_level_models.HierarchicalLstmModel(), losses.CrossEntropyLossTop50(), 128, 4, 10, "cpu")
    with pytest.raises(ValueError, match="at least 50 classes"):
        losses.CrossEntropyLossTop50().calculate_loss(torch.zeros(2, 49), torch.zeros(2, 49, dtype=torch.uint8))
    losses.CrossEntropyLossTop50().check(50)


def test_checkpoint_names_the_loss_only_when_it_is_not_the_default(tmp_path):
    for fn, want in ((None, None), (losses.CrossEntropyLoss(), None), (losses.HingeLoss(), "HingeLoss"), (losses.NewLoss(), "NewLoss")):
        g = types.SimpleNamespace(global_step=4)
        if fn is not None:
            g.label_loss = fn
        sd = torch.load(train.save_checkpoint(g, str(tmp_path), 0))
        if want is None:
            assert set(sd) == {"global_step"}                   # the default checkpoint keeps its exact key set
        else:
            assert sd["label_loss"] == want and set(sd) == {"global_step", "label_loss"}
        g2 = types.SimpleNamespace(global_step=0)
        train.restore_checkpoint(g2, train.latest_checkpoint(str(tmp_path)))     # the key is ignored on restore
        assert g2.global_step == 4 and not hasattr(g2, "label_loss")
