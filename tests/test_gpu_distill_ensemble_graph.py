"""Ensemble distillation: EnsembleDistillGraph - one student against several frozen teachers - and the train --teacher_only (twice) ->
train --teacher_dirs -> validate -> train_convert_model -> resume recipe.  pytest -m gpu.

Bounds: the step's loss values and every teacher's own CE against the float64 reference (tests/_distill_ensemble_ref.py) evaluated on
the predictions and states the step itself returns: 1e-4 relative, for all of them (the serial tests compare with the oracle's own
forward under 2e-2 and have no separate bound for pred_loss, so none is taken over).  Everything else is bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _distill_ensemble_ref as eref
from oracle import model_math as mm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, F, H, V, EVERY_N = 5, 64, 64, 40, 30
KW = dict(feature_size=F, vocab_size=V, lstm_cells=H, device=DEV)
RTOL_LOSS = 1e-4
_SHARED = {}


def _shared():
    """The batch, two teachers that have made two training steps from two seeds, and an every_n = 10 student trained next to the first."""
    if not _SHARED:
        from efficientvideoclassification_youtube8m_amd.distill import DistillGraph
        q, x, n, labels = mm.synthetic_batch(B, seed=21, feature_size=F, vocab_size=V, dtype=np.float32)
        dev = (torch.from_numpy(x).to(DEV), torch.from_numpy(labels.astype(np.uint8)).to(DEV), torch.from_numpy(n).to(DEV))
        sds = []
        for seed in (5, 6):
            t = DistillGraph(B, mode="teacher", seed=seed, every_n=EVERY_N, **KW)
            for _ in range(2):
                t.step(*dev, num_frames_host=n)
            sds.append({k: v.clone() for k, v in t.teacher.state_dict().items()})
        ts = DistillGraph(B, mode="teacher_student", seed=5, every_n=10, student_sampling="last", **KW)
        for _ in range(2):
            ts.step(*dev, num_frames_host=n)
        ts.flush()
        assistant = {k: v.clone() for k, v in ts.student.state_dict().items()}
        torch.cuda.synchronize()
        _SHARED.update(x=x, n=n, labels=labels, dev=dev, teacher_sds=sds, assistant_sd=assistant)
    return _SHARED


def _graph(teachers, sds, **kw):
    from efficientvideoclassification_youtube8m_amd.distill import EnsembleDistillGraph
    g = EnsembleDistillGraph(B, teachers=teachers, every_n=EVERY_N, seed=5, **dict(KW, **kw))
    for tw, sd in zip(g.teachers, sds):
        tw.load_state_dict(sd)
    return g


def _check_losses(g, out, labels, mode, weights, rep_weights, what):
    """LOSS_SLOTS and the per-teacher CE of the step against float64 on the tensors the step returned."""
    torch.cuda.synchronize()
    inp = dict(labels=labels.astype(np.uint8), pred_s=out["student_predictions"].cpu().numpy(), state_s=out["student_state"].cpu().numpy())
    preds = [p.cpu().numpy() for p in out["teacher_predictions"]]
    states = [s.cpu().numpy() for s in out["teacher_states"]]
    want = eref.reference(inp, preds, states, mode, weights, rep_weights, g_ce=1.0 / B, g_kl=1.0, g_rep=2.0)
    rep = g.loss_report()
    assert set(rep) == set(g.LOSS_SLOTS) | {"teacher_%d_label_loss" % j for j in range(g.J)}
    missed = []
    for i, k in enumerate(g.LOSS_SLOTS):
        print("%s %s: %.9g, float64 %.9g" % (what, k, rep[k], want["losses"][i]))
        if not abs(rep[k] - want["losses"][i]) <= RTOL_LOSS * abs(want["losses"][i]):
            missed.append((k, rep[k], float(want["losses"][i])))
    for j in range(g.J):
        k = "teacher_%d_label_loss" % j
        print("%s %s: %.9g, float64 %.9g" % (what, k, rep[k], want["teacher_ce"][j]))
        if not abs(rep[k] - want["teacher_ce"][j]) <= RTOL_LOSS * abs(want["teacher_ce"][j]):
            missed.append((k, rep[k], float(want["teacher_ce"][j])))
    assert not missed, missed
    assert np.array_equal(out["predictions"].cpu().numpy().view(np.uint32), want["pred_comb"].view(np.uint32))     # the combined row
    return want


@pytest.mark.parametrize("mode", ["mean", "max"])
def test_two_teachers_are_wired_into_the_loss_section_and_entry_0_is_the_frozen_teacher(mode):
    from efficientvideoclassification_youtube8m_amd.distill import EvalGraph
    sh = _shared()
    w = [0.75, 0.25] if mode == "mean" else None
    r = [0.5, 0.5]
    g = _graph([("teacher",), ("teacher",)], sh["teacher_sds"], teacher_mode=mode, teacher_weights=w, rep_weights=r)
    assert all(t.training is False and t.store.m is None and t.store.grad is None for t in g.teachers) and g.student.training
    assert g.teacher is g.teachers[0] and g.mode == "ensemble"
    before = [{k: v.clone() for k, v in t.state_dict().items()} for t in g.teachers]
    out = g.step(*sh["dev"], num_frames_host=sh["n"])
    assert g.global_step == 1 and out["global_step"] == 1 and g.student.adam_t == 1
    assert set(out) >= {"predictions", "teacher_predictions", "teacher_states", "teacher_state", "loss", "student_predictions", "student_state",
                        "num_frames_student", "student_loss_state", "pred_loss", "student_label_loss", "teacher_label_losses", "global_step"}
    _check_losses(g, out, sh["labels"], mode, w, r, "two teachers, %s" % mode)
    assert not torch.equal(out["teacher_predictions"][0], out["teacher_predictions"][1])          # two different teachers
    # every frozen forward is the forward EvalGraph serves from that checkpoint, bit for bit
    for j in range(2):
        e = EvalGraph(B, teacher_only=True, every_n=EVERY_N, **KW)
        e.restore(sh["teacher_sds"][j])
        out_e = e.step(*sh["dev"], num_frames_host=sh["n"])
        assert torch.equal(out_e["predictions"], out["teacher_predictions"][j]) and torch.equal(out_e["teacher_state"], out["teacher_states"][j]), j
    g.flush()
    for t, sd in zip(g.teachers, before):                                                       # and nothing wrote to them
        for k, v in t.state_dict().items():
            assert torch.equal(v, sd[k]), k


def test_one_teacher_computes_what_the_serial_graph_reports():
    """J = 1 against DistillGraph(mode="serial") on the same weights: the same forwards bit for bit.  The serial graph's loss values come
    from evc_distill_losses, whose all-f32 L_PRED is 3e-4 off float64 on a student this close to its teacher (measured: 0.00052619469
    here, 0.00052602409 there, float64 0.00052619447), so they are compared under the bound test_gpu_serial_distill.py holds that graph's
    loss values to: 2e-2 relative + 1e-6."""
    from efficientvideoclassification_youtube8m_amd.distill import DistillGraph
    sh = _shared()
    g = _graph([("teacher",)], sh["teacher_sds"][:1])
    s = DistillGraph(B, mode="serial", seed=5, every_n=EVERY_N, **KW)
    s.teacher.load_state_dict(sh["teacher_sds"][0])
    out = g.step(*sh["dev"], apply=False, num_frames_host=sh["n"])
    out_s = s.step(*sh["dev"], apply=False, num_frames_host=sh["n"])
    assert g.global_step == 0
    assert torch.equal(out["teacher_predictions"][0], out_s["predictions"]) and torch.equal(out["predictions"], out_s["predictions"])
    assert torch.equal(out["student_predictions"], out_s["student_predictions"]) and torch.equal(out["student_state"], out_s["student_state"])
    _check_losses(g, out, sh["labels"], "mean", [1.0], [1.0], "one teacher")
    a, b = g.loss_report(), s.loss_report()
    for k in g.LOSS_SLOTS:
        assert abs(a[k] - b[k]) <= 2e-2 * abs(b[k]) + 1e-6, (k, a[k], b[k])


def test_a_teaching_assistant_runs_at_its_own_every_n_and_sampling():
    from efficientvideoclassification_youtube8m_amd.distill import EvalGraph
    sh = _shared()
    g = _graph([("teacher",), ("student", 10, "last")], [sh["teacher_sds"][0], sh["assistant_sd"]], distill_losses=("rep", "pred"))
    assert g.teachers[1].scope == "model_student" and g.teachers[1].store.m is None and g.teacher_every_n == (1, 10)
    assert g.teacher_meta() == dict(towers=["teacher", "student"], every_n=[1, 10], sampling=["uniform", "last"], mode="mean",
                                    weights=[0.5, 0.5], rep_weights=[1.0, 0.0])
    for it in range(2):
        out = g.step(*sh["dev"], num_frames_host=sh["n"])
    assert g.global_step == 2
    _check_losses(g, out, sh["labels"], "mean", None, None, "teacher + assistant")
    e = EvalGraph(B, student_only=True, every_n=10, student_sampling="last", **KW)
    e.restore(sh["assistant_sd"])
    out_e = e.step(*sh["dev"], num_frames_host=sh["n"])
    assert torch.equal(out_e["predictions"], out["teacher_predictions"][1]) and torch.equal(out_e["student_state"], out["teacher_states"][1])
    assert tuple(out["student_predictions"].shape) == (B, V) and all(np.isfinite(v) for v in g.loss_report().values())


def test_duplicated_teachers_train_the_student_as_one_does():
    """The same checkpoint twice under mean [.5, .5] and three times under max against J = 1, two iterations, bit for bit - in a fresh
    process under EVC_DETERMINISTIC=1."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(root, "tests", "_distill_ensemble_child.py")],
                       env=dict(os.environ, EVC_DETERMINISTIC="1"), capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("ok")


COMMON = ["--frame_features", "True", "--feature_names", "rgb, audio", "--feature_sizes", "64, 64", "--model", "HierarchicalLstmModel",
          "--gpu", "0", "--num_inputs_to_lstm", "20", "--lstm_layers", "2", "--lstm_cells", "64", "--every_n", "30", "--num_readers", "2"]


def _tensors(sd, scope):
    return {k: v for k, v in sd.items() if k.startswith(scope) and torch.is_tensor(v)}


def test_two_teacher_only_runs_then_teacher_dirs_then_validate_convert_resume(tmp_path):
    from efficientvideoclassification_youtube8m_amd import readers, train, train_convert_model, validate
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    data = tmp_path / "yt8m"
    readers.write_synthetic_frame_dataset(str(data), 2, 12, feature_sizes=(64, 64), min_frames=60, max_frames=310, seed=1, prefix="train")
    readers.write_synthetic_frame_dataset(str(data), 2, 7, feature_sizes=(64, 64), min_frames=60, max_frames=310, seed=2, prefix="validate")
    a, b, sdir = (str(tmp_path / n) + "/" for n in ("teacher_a", "teacher_b", "ensemble_train"))
    feed = ["--train_data_pattern", str(data / "train*.tfrecord"), "--batch_size", "8"]
    try:
        for d, lr in ((a, "0.001"), (b, "0.002")):                       # two teachers that differ
            FLAGS.reset()
            train.main(COMMON + feed + ["--train_dir", d, "--max_steps", "2", "--start_new_model", "True", "--teacher_only", "True",
                                        "--base_learning_rate", lr])
        src = torch.load(train.latest_checkpoint(a))
        other = torch.load(train.latest_checkpoint(b))
        assert any(not torch.equal(v, other[k]) for k, v in _tensors(src, "model/").items())

        FLAGS.reset()
        res = train.main(COMMON + feed + ["--train_dir", sdir, "--max_steps", "3", "--start_new_model", "True", "--teacher_dirs", a + "," + b])
        g = res["graph"]
        assert g.mode == "ensemble" and g.J == 2 and res["iterations"] == 3 and g.global_step == 3
        assert [h[0] for h in res["history"]] == [1, 2, 3]
        assert set(res["history"][0][1]) == set(g.LOSS_SLOTS) | {"teacher_0_label_loss", "teacher_1_label_loss"}
        assert all(np.isfinite(v) for h in res["history"] for v in h[1].values())
        assert train.latest_checkpoint(sdir).endswith("model.ckpt-3.pt")                  # one train op per iteration
        sd = torch.load(train.latest_checkpoint(sdir))
        want = _tensors(src, "model/")
        assert len(want) == 11 and set(_tensors(sd, "model/")) == set(want)
        for k, v in want.items():
            assert torch.equal(sd[k], v), k                                               # entry 0, bit for bit
        assert "model_student/adam" in sd and "model/adam" not in sd and len(_tensors(sd, "model_student/")) == 11
        assert sd["model_student/adam"]["t"] == 3
        assert sd["distill_mode"] == "ensemble" and sd["distill_losses"] == "rep,pred,ce" and sd["student_sampling"] == "uniform"
        assert sd["distill_teachers"] == {"dirs": [a, b], "checkpoints": ["model.ckpt-2.pt"] * 2, "towers": ["teacher", "teacher"],
                                          "every_n": [1, 1], "sampling": ["uniform", "uniform"], "mode": "mean", "weights": [0.5, 0.5],
                                          "rep_weights": [1.0, 0.0]}

        FLAGS.reset()
        info = validate.main(COMMON + ["--eval_data_pattern", str(data / "validate*.tfrecord"), "--train_dir", sdir, "--batch_size", "5",
                                       "--top_k", "20", "--run_once", "True"])
        assert info["epoch_id"] == 3
        for k in ("avg_hit_at_one", "avg_perr", "avg_loss", "gap"):
            assert np.isfinite(info[k]), (k, info[k])

        FLAGS.reset()
        conv = torch.load(train_convert_model.main(["--train_dir", sdir]))
        assert not _tensors(conv, "model/") and conv["global_step"] == 0
        for k, v in _tensors(sd, "model_student/").items():
            assert torch.equal(conv[k], v), k

        FLAGS.reset()       # resume: the student and entry 0 from --train_dir, teacher 1 from its directory again
        res = train.main(COMMON + feed + ["--train_dir", sdir, "--max_steps", "2", "--teacher_dirs", a + "," + b])
        assert res["graph"].mode == "ensemble" and res["graph"].global_step == 5 and [h[0] for h in res["history"]] == [4, 5]
        sd5 = torch.load(train.latest_checkpoint(sdir))
        assert train.latest_checkpoint(sdir).endswith("model.ckpt-5.pt") and sd5["model_student/adam"]["t"] == 5
        for k, v in want.items():
            assert torch.equal(sd5[k], v), k
        for k, v in _tensors(other, "model/").items():                                    # teacher 1 was reloaded from b
            assert torch.equal(res["graph"].teachers[1].state_dict()[k].cpu(), v), k
        assert any(not torch.equal(sd5[k], v) for k, v in _tensors(sd, "model_student/").items())
        assert sd5["distill_teachers"] == sd["distill_teachers"]

        FLAGS.reset()       # the teachers swapped: refused, both lists shown
        with pytest.raises(ValueError) as e:
            train.main(COMMON + feed + ["--train_dir", sdir, "--max_steps", "1", "--teacher_dirs", b + "," + a])
        assert str([a, b]) in str(e.value) and str([b, a]) in str(e.value)
    finally:
        FLAGS.reset()
