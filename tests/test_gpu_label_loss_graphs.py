"""--label_loss through the graphs: SingleTowerGraph, DistillGraph, train.main and validate.main with another loss than
CrossEntropyLoss, and the default path next to an explicit "CrossEntropyLoss".  pytest -m gpu.

The float64 side is tests/_label_losses_ref.py evaluated on the f32 predictions the loss kernel read (a mask such as TOP50's cannot be
compared across two forwards that differ by the bf16 rounding of the tower), oracle.model_math for the towers."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _label_losses_ref as ref
from oracle import model_math as mm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, F, H, V = 8, 64, 64, 64


def _np(t):
    return t.detach().cpu().double().numpy()


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _batch(seed):
    q, x, n, labels = mm.synthetic_batch(B, seed=seed, feature_size=F, vocab_size=V, dtype=np.float32)
    return x, n, labels, (torch.from_numpy(x).to(DEV), torch.from_numpy(labels.astype(np.uint8)).to(DEV), torch.from_numpy(n).to(DEV))


@pytest.mark.parametrize("name,kind", [("HingeLoss", "HINGE"), ("CrossEntropyLossTop50", "TOP50")])
def test_single_tower_graph_with_another_loss(name, kind):
    from efficientvideoclassification_youtube8m_amd import losses
    from efficientvideoclassification_youtube8m_amd.distill import SingleTowerGraph
    from efficientvideoclassification_youtube8m_amd.towers import LogisticTower
    x, n, labels, dev = _batch(2)
    tw = LogisticTower(B, 300, F, V, device=DEV, seed=1)
    tw.store.p(tw.Bn).normal_(0, 0.1)
    pre = tw.scope + "/"
    P = {k[len(pre):]: _np(v) for k, v in tw.state_dict().items()}
    g = SingleTowerGraph(tw, label_loss=name)
    assert type(g.label_loss).__name__ == name
    out = g.step(*dev, apply=False)
    torch.cuda.synchronize()
    p_ref, avg = mm.logistic_fwd(mm.l2_normalize(x.astype(np.float64), 2), n, P["fully_connected/weights"], P["fully_connected/biases"])
    assert np.abs(_np(out["predictions"]) - p_ref).max() < 1e-3
    want = ref.reference(kind, out["predictions"].cpu().numpy(), labels.astype(np.uint8))
    print(name, "loss", out["loss"].item(), "ref", want["loss"])
    assert abs(out["loss"].item() - want["loss"]) <= 1e-4 * abs(want["loss"])
    assert torch.equal(g.label_grads()["teacher"], g._dp)
    dW, db = mm.logistic_bwd(want["grad"] / B, p_ref, avg)
    assert _rel(_np(tw.store.g(tw.W).t()), dW) < 2e-2
    assert _rel(_np(tw.store.g(tw.Bn)), db) < 2e-2
    with pytest.raises(ValueError, match="label_loss"):
        SingleTowerGraph(tw, label_loss="NoSuchLoss")
    assert isinstance(SingleTowerGraph(tw, label_loss=losses.HingeLoss()).label_loss, losses.HingeLoss)


def _distill_graph(label_loss, seed=5):
    from efficientvideoclassification_youtube8m_amd.distill import DistillGraph
    return DistillGraph(B, feature_size=F, lstm_cells=H, vocab_size=V, mode="teacher_student", device=DEV, seed=seed, label_loss=label_loss)


def test_distill_graph_with_new_loss():
    from efficientvideoclassification_youtube8m_amd import ops
    x, n, labels, dev = _batch(21)
    g = _distill_graph("NewLoss")
    out = g.step(*dev, apply=False, num_frames_host=n)
    torch.cuda.synchronize()
    assert g.global_step == 0
    grads = g.label_grads()
    assert set(grads) == {"teacher", "student"}
    t_pred, s_pred = out["predictions"], out["student_predictions"]
    # teacher: a direct call on the graph's own predictions
    loss = torch.zeros(2, dtype=torch.float32, device=DEV)
    dp = torch.full_like(t_pred, float("nan"))
    ops.label_loss(ops.LOSS_NEW, t_pred, dev[1], loss[0:1], dp, grad_scale=1.0 / B)
    assert torch.equal(grads["teacher"], dp) and torch.equal(loss[0], out["loss"])
    # student: the label loss, then L_PRED accumulated on top of it
    dps = torch.full_like(s_pred, float("nan"))
    ops.label_loss(ops.LOSS_NEW, s_pred, dev[1], loss[1:2], dps, grad_scale=1.0 / B)
    kl = torch.zeros(1, dtype=torch.float32, device=DEV)
    ops.kl_pred_loss(t_pred, g.teacher.rowsum, s_pred, g.student.rowsum, kl, dps, grad_scale=1.0, accumulate_grad=True)
    torch.cuda.synchronize()
    assert torch.equal(grads["student"], dps) and torch.equal(loss[1], out["student_label_loss"])
    # (evc_kl_pred_loss joins its B = 8 non-negative row sums by float atomics: the same sum in another order, 7 f32 additions of at most
    # 6e-8 relative each - 1e-6 relative covers any order)
    assert abs(float(kl[0]) - float(out["pred_loss"])) <= 1e-6 * abs(float(out["pred_loss"]))
    rep = g.loss_report()
    y = labels.astype(np.uint8)
    want_t, want_s = ref.reference("NEW", t_pred.cpu().numpy(), y), ref.reference("NEW", s_pred.cpu().numpy(), y)
    print("NewLoss teacher", rep["label_loss"], want_t["loss"], "student", rep["student_label_loss"], want_s["loss"])
    assert want_t["loss"] > 0 and want_s["loss"] > 0
    assert abs(rep["label_loss"] - want_t["loss"]) <= 1e-4 * want_t["loss"]
    assert abs(rep["student_label_loss"] - want_s["loss"]) <= 1e-4 * want_s["loss"]
    g.apply_gradients(B)
    torch.cuda.synchronize()
    assert g.global_step == 2


def test_distill_graph_refuses_serial_mode_with_another_loss():
    from efficientvideoclassification_youtube8m_amd.distill import DistillGraph
    with pytest.raises(ValueError, match="CrossEntropyLoss built into"):
        DistillGraph(B, feature_size=F, lstm_cells=H, vocab_size=V, mode="serial", device=DEV, label_loss="HingeLoss")
    with pytest.raises(ValueError, match="at least 50 classes"):
        DistillGraph(B, feature_size=F, lstm_cells=H, vocab_size=40, device=DEV, label_loss="CrossEntropyLossTop50")


def _default_path_step(label_loss):
    """One step(apply=False) of a fresh graph: [(name, tensor)] of its outputs, loss values, dL/dpred and weight gradients."""
    x, n, labels, dev = _batch(21)
    g = _distill_graph(label_loss)
    out = g.step(*dev, apply=False, num_frames_host=n)
    torch.cuda.synchronize()
    got = [(k, out[k].clone()) for k in ("predictions", "student_predictions", "teacher_state", "student_state")]
    got.append(("losses", g.losses.clone()))
    got += [("dpred " + k, v.clone()) for k, v in sorted(g.label_grads().items())]
    got += [("grad " + tw.scope, tw.store.grad.clone()) for tw in (g.teacher, g.student)]
    return got


def test_default_path_is_the_cross_entropy_path():
    from efficientvideoclassification_youtube8m_amd import losses
    assert type(_distill_graph(None).label_loss) is losses.CrossEntropyLoss
    a, b = _default_path_step(None), _default_path_step("CrossEntropyLoss")
    for (name, u), (_, v) in zip(a, b):
        # (loss sums and weight gradients are joined by float atomics outside EVC_DETERMINISTIC: their bits are compared in the child)
        if name == "losses":
            assert torch.allclose(u, v, rtol=1e-5, atol=0), (u, v)
        elif not name.startswith("grad "):
            assert torch.equal(u, v), name
    y = _batch(21)[2]
    ce = mm.cross_entropy_loss(_np(a[0][1]), y)
    assert abs(float(a[4][1][0]) - ce) <= 1e-4 * ce                      # slot 0 is the teacher's cross entropy, as ever
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(root, "tests", "_label_loss_child.py"), "graph"],
                       env=dict(os.environ, EVC_DETERMINISTIC="1"), capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("ok")


TRAIN = ["--frame_features", "True", "--feature_names", "rgb, audio", "--feature_sizes", "64, 64", "--model", "HierarchicalLstmModel",
         "--gpu", "0", "--num_inputs_to_lstm", "20", "--lstm_layers", "2", "--lstm_cells", "64", "--every_n", "10"]


def test_train_and_validate_with_hinge_loss(tmp_path, monkeypatch):
    from efficientvideoclassification_youtube8m_amd import distill, train, validate
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    tdir = str(tmp_path / "hinge") + "/"
    FLAGS.reset()
    res = train.main(TRAIN + ["--train_data_pattern", "synthetic", "--synthetic_videos", "16", "--batch_size", "8", "--max_steps", "2",
                              "--train_dir", tdir, "--start_new_model", "True", "--label_loss", "HingeLoss", "--log_every", "1"])
    assert res["iterations"] == 2 and len(res["history"]) == 2
    for _, rep, _ in res["history"]:
        assert all(np.isfinite(v) for v in rep.values()) and rep["label_loss"] > 0 and rep["student_label_loss"] > 0
    sd = torch.load(train.latest_checkpoint(tdir))
    assert sd["label_loss"] == "HingeLoss" and sd["global_step"] == 4
    # validate: the logged loss is the hinge loss of the predictions it fetched
    seen = []
    step = distill.EvalGraph.step

    def spy(self, x_raw, labels_u8, num_frames, num_frames_host=None):
        out = step(self, x_raw, labels_u8, num_frames, num_frames_host=num_frames_host)
        seen.append((out["predictions"].clone(), labels_u8.clone(), type(self.label_loss).__name__))
        return out
    monkeypatch.setattr(distill.EvalGraph, "step", spy)
    FLAGS.reset()
    info = validate.main(TRAIN + ["--eval_data_pattern", "synthetic", "--synthetic_videos", "8", "--batch_size", "8", "--train_dir", tdir,
                                  "--run_once", "True", "--label_loss", "HingeLoss"])
    FLAGS.reset()
    assert len(seen) == 1 and seen[0][2] == "HingeLoss" and info["epoch_id"] == 4
    want = ref.reference("HINGE", seen[0][0].cpu().numpy(), seen[0][1].cpu().numpy())["loss"]
    print("validate avg_loss", info["avg_loss"], "float64 hinge", want)
    assert abs(info["avg_loss"] - want) <= 1e-4 * want


def test_train_refuses_serial_distillation_with_hinge_loss(tmp_path):
    from efficientvideoclassification_youtube8m_amd import train
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    FLAGS.reset()
    with pytest.raises(ValueError, match="--label_loss HingeLoss with --teacher_dir"):
        train.main(TRAIN + ["--train_data_pattern", "synthetic", "--train_dir", str(tmp_path / "s") + "/", "--teacher_dir",
                            str(tmp_path / "t") + "/", "--label_loss", "HingeLoss"])
    FLAGS.reset()
