"""Serial distillation of several students against ONE teacher forward: distill.SerialStudentsGraph against the float64 oracle
(oracle.model_math.teacher_student_step treats the teacher as a constant of the student's loss: its student_grads ARE the serial
gradients) and against DistillGraph(mode="serial"), and the train --teacher_only -> train --teacher_dir --serial_student_dirs ->
validate -> train_convert_model -> resume recipe.  pytest -m gpu.

Bounds: those of test_gpu_serial_distill.py - student gradients max-relative < 3e-2 and relative L2 < 1.2e-2 per tensor, loss values
within 2e-2 relative + 1e-6."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _frame_select_ref as fref
from oracle import model_math as mm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, F, H, V = 5, 64, 64, 40                       # the shapes of test_gpu_serial_distill.py
MOE_W = ("classifier/gates/weights", "classifier/experts/weights")
KW = dict(feature_size=F, vocab_size=V, lstm_cells=H, device=DEV)
EVERY_N, SAMPLING = (30, 10, 30), ("uniform", "uniform", "last")
_SHARED = {}


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _rel2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / (np.linalg.norm(b) + 1e-30))


def _shared():
    """The batch and the weights of a teacher that has made two training steps (mode "teacher"), once per session."""
    if not _SHARED:
        from efficientvideoclassification_youtube8m_amd.distill import DistillGraph
        q, x, n, labels = mm.synthetic_batch(B, seed=21, feature_size=F, vocab_size=V, dtype=np.float32)
        dev = (torch.from_numpy(x).to(DEV), torch.from_numpy(labels.astype(np.uint8)).to(DEV), torch.from_numpy(n).to(DEV))
        t = DistillGraph(B, mode="teacher", seed=5, every_n=30, **KW)
        for _ in range(2):
            t.step(*dev, num_frames_host=n)
        sd = {k: v.clone() for k, v in t.teacher.state_dict().items()}
        torch.cuda.synchronize()
        _SHARED.update(x=x, n=n, labels=labels, dev=dev, teacher_sd=sd)
    return _SHARED


def _graph(every_n=EVERY_N, sampling=SAMPLING, losses=None):
    from efficientvideoclassification_youtube8m_amd.distill import SerialStudentsGraph
    g = SerialStudentsGraph(B, every_n=every_n, student_sampling=sampling, distill_losses=losses, seed=5, **KW)
    g.teacher.load_state_dict(_shared()["teacher_sd"])
    return g


def _check_grads(got, want, what):
    l2s = {}
    for k in mm.HLSTM_PARAM_ORDER:
        gref = want[k]
        if np.abs(gref).max() == 0.0:
            assert not got[k].any(), (what, k)
            continue
        assert _rel(got[k], gref) < 3e-2, (what, k, _rel(got[k], gref))
        l2s[k] = _rel2(got[k], gref)
        assert l2s[k] < 1.2e-2, (what, k, l2s[k])
    print("%s: gradient relative L2:" % what, {k: round(v, 4) for k, v in l2s.items()})


def test_one_teacher_forward_and_every_students_gradients():
    from efficientvideoclassification_youtube8m_amd import smoke
    from efficientvideoclassification_youtube8m_amd.distill import DistillGraph, EvalGraph
    sh = _shared()
    g = _graph()
    assert g.teacher.training is False and g.teacher.store.m is None and g.teacher.store.grad is None
    assert len(g.students) == 3 and all(s.training and s.scope == "model_student" for s in g.students)
    calls, inner = [], g.teacher.forward
    g.teacher.forward = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    out = g.step(*sh["dev"], apply=False, num_frames_host=sh["n"])
    assert len(calls) == 1                                             # ONE teacher forward for the three students
    assert g.global_step == 0 and out["global_step"] == 0 and len(out["students"]) == 3
    assert set(out) >= {"predictions", "teacher_state", "loss", "global_step", "students"}
    for o in out["students"]:
        assert set(o) >= {"student_predictions", "student_state", "num_frames_student", "student_loss_state", "pred_loss", "student_label_loss"}
    e = EvalGraph(B, teacher_only=True, every_n=30, **KW)
    e.restore(sh["teacher_sd"])
    out_e = e.step(*sh["dev"], num_frames_host=sh["n"])
    assert torch.equal(out_e["predictions"], out["predictions"]) and torch.equal(out_e["teacher_state"], out["teacher_state"])
    teacher = smoke.tower_params_numpy(g.teacher)
    rep = g.loss_report()
    assert len(rep) == 3 and all(set(r) == set(g.LOSS_SLOTS) for r in rep)
    assert rep[0]["label_loss"] == rep[1]["label_loss"] == rep[2]["label_loss"]
    for k in (0, 1):                                                   # the uniform students against the oracle
        student = smoke.tower_params_numpy(g.students[k])
        ref = mm.teacher_student_step(sh["x"].astype(np.float64), sh["n"], sh["labels"], teacher, student, EVERY_N[k])
        want = dict(ref["student_grads"])
        for w in MOE_W:
            want[w] = want[w] - 2.0 * 1e-8 * student[w]                # the l2 term is folded in at apply time
        _check_grads(smoke.tower_grads_numpy(g.students[k]), want, "student %d (every_n %d) vs float64" % (k, EVERY_N[k]))
        for name in g.LOSS_SLOTS:
            assert abs(rep[k][name] - ref[name]) <= 2e-2 * abs(ref[name]) + 1e-6, (k, name, rep[k][name], float(ref[name]))
    # the `last` student against the single-student serial graph on the same weights and batch: wrong frames move the gradients by O(1)
    assert g.last_frame_tables[0] is None and g.last_frame_tables[1] is None
    assert np.array_equal(g.last_frame_tables[2].cpu().numpy(), fref.table(sh["n"], 300, 30, "last", seed=0, draw=0, row0=0))
    s = DistillGraph(B, mode="serial", seed=5, every_n=30, student_sampling="last", **KW)
    s.teacher.load_state_dict(sh["teacher_sd"])
    s.student.load_state_dict(g.students[2].state_dict())
    s.step(*sh["dev"], apply=False, num_frames_host=sh["n"])
    assert np.array_equal(s.last_frame_table.cpu().numpy(), g.last_frame_tables[2].cpu().numpy())
    _check_grads(smoke.tower_grads_numpy(g.students[2]), smoke.tower_grads_numpy(s.student), "student 2 (last) vs DistillGraph serial")
    single = s.loss_report()
    for name in g.LOSS_SLOTS:
        assert abs(rep[2][name] - single[name]) <= 2e-2 * abs(single[name]) + 1e-6, (name, rep[2][name], single[name])
    uniform = smoke.tower_grads_numpy(g.students[0])                   # (and it is not the uniform student of the same every_n)
    assert _rel2(smoke.tower_grads_numpy(g.students[2])[MOE_W[0]], uniform[MOE_W[0]]) > 0.1


def test_three_iterations_track_the_oracle_and_leave_the_teacher_alone():
    from efficientvideoclassification_youtube8m_amd import smoke
    sh = _shared()
    g = _graph()
    before = {k: v.clone() for k, v in g.teacher.state_dict().items()}
    shadows = {k: v.clone() for k, v in g.teacher.shadow_fwd.items()}
    s0 = [{k: v.clone() for k, v in s.state_dict().items()} for s in g.students]
    teacher = smoke.tower_params_numpy(g.teacher)
    students = {k: smoke.tower_params_numpy(g.students[k]) for k in (0, 1)}
    slots = {0: {}, 1: {}}
    for it in range(3):
        out = g.step(*sh["dev"], num_frames_host=sh["n"])
        assert out["global_step"] == it + 1
        rep = g.loss_report()
        for k in (0, 1):
            ref = mm.teacher_student_step(sh["x"].astype(np.float64), sh["n"], sh["labels"], teacher, students[k], EVERY_N[k])
            for name in g.LOSS_SLOTS:
                assert abs(rep[k][name] - ref[name]) <= 2e-2 * abs(ref[name]) + 1e-6, (it, k, name, rep[k][name], float(ref[name]))
            students[k] = mm.apply_train_op(students[k], ref["student_grads"], slots[k], it + 1, 1e-3, 1.0)
    assert g.global_step == 3 and all(s.adam_t == 3 for s in g.students) and g.teacher.adam_t == 0
    g.flush()
    g.consolidate()
    after = g.teacher.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    for k, v in shadows.items():
        assert torch.equal(g.teacher.shadow_fwd[k], v), k
    for s, old in zip(g.students, s0):
        new = s.state_dict()
        assert all(not torch.equal(new[k], old[k]) for k in old)


def test_a_students_training_does_not_depend_on_its_company():
    """K = 3 against three K = 1 graphs, two iterations, bit for bit - in a fresh process under EVC_DETERMINISTIC=1."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(root, "tests", "_serial_students_child.py")],
                       env=dict(os.environ, EVC_DETERMINISTIC="1"), capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("ok")


def test_per_student_loss_selection():
    from efficientvideoclassification_youtube8m_amd import smoke
    sh = _shared()
    g = _graph(every_n=(30, 30), sampling=("uniform", "uniform"), losses=(("rep", "pred", "ce"), ("rep",)))
    assert g.distill_losses == (("rep", "pred", "ce"), ("rep",))
    g.step(*sh["dev"], apply=False, num_frames_host=sh["n"])
    g0, g1 = smoke.tower_grads_numpy(g.students[0]), smoke.tower_grads_numpy(g.students[1])
    for w in MOE_W:
        assert not g1[w].any() and g0[w].any(), w                      # L_REP alone never reaches the MoE head
    assert any(g1[k].any() for k in mm.HLSTM_PARAM_ORDER if k not in MOE_W)
    rep = g.loss_report()                                              # the same weights and frames: the same four values
    assert rep[0] == rep[1]


COMMON = ["--frame_features", "True", "--feature_names", "rgb, audio", "--feature_sizes", "64, 64", "--model",
          "HierarchicalLstmModel", "--gpu", "0", "--num_inputs_to_lstm", "20", "--lstm_layers", "2", "--lstm_cells", "64",
          "--every_n", "10", "--num_readers", "2"]


def _tensors(sd, scope):
    return {k: v for k, v in sd.items() if k.startswith(scope) and torch.is_tensor(v)}


def test_teacher_only_then_two_students_then_validate_convert_resume(tmp_path):
    from efficientvideoclassification_youtube8m_amd import readers, train, train_convert_model, validate
    from efficientvideoclassification_youtube8m_amd.distill import SerialStudentsGraph
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    data = tmp_path / "yt8m"
    readers.write_synthetic_frame_dataset(str(data), 2, 12, feature_sizes=(64, 64), min_frames=60, max_frames=310, seed=1, prefix="train")
    readers.write_synthetic_frame_dataset(str(data), 2, 7, feature_sizes=(64, 64), min_frames=60, max_frames=310, seed=2, prefix="validate")
    tdir, a, b = (str(tmp_path / d) + "/" for d in ("teacher_train", "a", "b"))
    feed = ["--train_data_pattern", str(data / "train*.tfrecord"), "--batch_size", "8"]
    multi = ["--teacher_dir", tdir, "--serial_student_dirs", "%s,%s" % (a, b), "--serial_every_n", "10,30", "--serial_sampling",
             "uniform,last", "--serial_losses", "rep+pred+ce,rep+pred"]
    meta = {a: ("rep,pred,ce", "uniform"), b: ("rep,pred", "last")}
    try:
        FLAGS.reset()
        train.main(COMMON + feed + ["--train_dir", tdir, "--max_steps", "2", "--start_new_model", "True", "--teacher_only", "True"])
        src = torch.load(train.latest_checkpoint(tdir))
        want = _tensors(src, "model/")
        assert len(want) == 11

        FLAGS.reset()
        res = train.main(COMMON + feed + multi + ["--max_steps", "2", "--start_new_model", "True", "--train_dir", str(tmp_path / "unused")])
        assert isinstance(res["graph"], SerialStudentsGraph) and res["iterations"] == 2 and res["graph"].global_step == 2
        assert [h[0] for h in res["history"]] == [1, 2]
        assert all(len(h[1]) == 2 and all(set(r) == set(res["graph"].LOSS_SLOTS) for r in h[1]) for h in res["history"])
        assert not os.path.exists(str(tmp_path / "unused"))                              # --train_dir is not consulted
        sds = {}
        for d in (a, b):
            assert train.latest_checkpoint(d).endswith("model.ckpt-2.pt"), d
            sd = sds[d] = torch.load(train.latest_checkpoint(d))
            assert set(_tensors(sd, "model/")) == set(want)
            for k, v in want.items():
                assert torch.equal(sd[k], v), (d, k)                                      # the frozen teacher, bit for bit
            assert "model_student/adam" in sd and "model/adam" not in sd and len(_tensors(sd, "model_student/")) == 11
            assert sd["model_student/adam"]["t"] == 2 and sd["global_step"] == 2
            assert sd["distill_mode"] == "serial" and (sd["distill_losses"], sd["student_sampling"]) == meta[d]

        for d, extra in ((a, []), (b, ["--every_n", "30", "--student_sampling", "last"])):
            FLAGS.reset()
            info = validate.main(COMMON + extra + ["--eval_data_pattern", str(data / "validate*.tfrecord"), "--train_dir", d, "--batch_size",
                                                   "5", "--top_k", "20", "--run_once", "True"])
            assert info["epoch_id"] == 2
            for k in ("avg_hit_at_one", "avg_perr", "avg_loss", "gap"):
                assert np.isfinite(info[k]), (d, k, info[k])

        FLAGS.reset()
        conv = torch.load(train_convert_model.main(["--train_dir", a]))
        assert not _tensors(conv, "model/")
        for k, v in _tensors(sds[a], "model_student/").items():
            assert torch.equal(conv[k], v), k

        FLAGS.reset()       # resume: every student from its directory, the teacher from the first; --teacher_dir only selects the mode
        res = train.main(COMMON + feed + multi[2:] + ["--teacher_dir", str(tmp_path / "nothing_here"), "--max_steps", "1"])
        assert res["graph"].global_step == 3
        for d in (a, b):
            assert train.latest_checkpoint(d).endswith("model.ckpt-3.pt"), d
            sd3 = torch.load(train.latest_checkpoint(d))
            assert sd3["model_student/adam"]["t"] == 3
            for k, v in want.items():
                assert torch.equal(sd3[k], v), (d, k)
            assert any(not torch.equal(sd3[k], v) for k, v in _tensors(sds[d], "model_student/").items())
            assert (sd3["distill_losses"], sd3["student_sampling"]) == meta[d]

        FLAGS.reset()       # a/ alone moves on with the single-student path ...
        train.main(COMMON + feed + ["--train_dir", a, "--max_steps", "1", "--teacher_dir", tdir])
        assert train.latest_checkpoint(a).endswith("model.ckpt-4.pt")
        FLAGS.reset()       # ... and the two no longer resume together
        with pytest.raises(ValueError, match="step 4.*step 3"):
            train.main(COMMON + feed + multi + ["--max_steps", "1"])
    finally:
        FLAGS.reset()
