"""Offline distillation end to end on tiny records: train --teacher_only -> inference --output_file teacher.csv over the training records
-> train --teacher_preds_pattern teacher.csv, with no teacher checkpoint in the student's run.  pytest -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

COMMON = ["--frame_features", "True", "--feature_names", "rgb, audio", "--feature_sizes", "64, 64", "--model", "HierarchicalLstmModel",
          "--gpu", "0", "--num_inputs_to_lstm", "20", "--lstm_layers", "2", "--lstm_cells", "64", "--every_n", "10", "--num_readers", "2"]


def test_a_student_is_trained_from_a_file_written_by_inference(tmp_path):
    from efficientvideoclassification_youtube8m_amd import eval_finetune, inference, readers, train
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    data = tmp_path / "yt8m"
    readers.write_synthetic_frame_dataset(str(data), 2, 8, feature_sizes=(64, 64), min_frames=60, max_frames=310, seed=1, prefix="train")
    pattern = str(data / "train*.tfrecord")
    tdir, sdir = str(tmp_path / "model_teacher") + "/", str(tmp_path / "model_student") + "/"

    # ---- 1. the teacher, two steps; 2. its top-20 predictions over the training records ----
    FLAGS.reset()
    train.main(COMMON + ["--train_data_pattern", pattern, "--train_dir", tdir, "--batch_size", "8", "--num_epochs", "1", "--max_steps", "2",
                         "--start_new_model", "True", "--teacher_only", "True"])
    preds = str(tmp_path / "teacher.csv")
    FLAGS.reset()
    st = inference.main(COMMON + ["--input_data_pattern", pattern, "--train_dir", tdir, "--output_file", preds, "--batch_size", "5",
                                  "--top_k", "20"])
    assert st["tower"] == "teacher" and st["videos"] == 16

    # ---- 3. the student against the file alone, three steps ----
    FLAGS.reset()
    res = train.main(COMMON + ["--train_data_pattern", pattern, "--train_dir", sdir, "--batch_size", "8", "--num_epochs", "2", "--max_steps", "3",
                               "--start_new_model", "True", "--teacher_preds_pattern", preds])
    assert res["iterations"] == 3 and len(res["history"]) == 3 and res["graph"].teacher is None
    for step, losses, _ in res["history"]:
        assert all(np.isfinite(v) for v in losses.values()), losses
        assert losses["pred_loss"] > 0 and losses["student_label_loss"] > 0 and losses["label_loss"] > 0 and losses["student_loss_state"] == 0
    assert [h[0] for h in res["history"]] == [1, 2, 3]                            # global_step += 1 per iteration
    ck = train.latest_checkpoint(sdir)
    assert ck.endswith("model.ckpt-3.pt")
    sd = torch.load(ck)
    assert not any(k.startswith("model/") for k in sd) and any(k.startswith("model_student/") for k in sd)      # the student alone
    assert sd["distill_mode"] == "offline" and sd["distill_losses"] == "pred,ce" and sd["student_sampling"] == "uniform"
    assert sd["distill_teacher_files"] == {"files": ["teacher.csv"], "mode": "mean", "weights": [1.0]}
    assert "model_student/adam" in sd and sd["model_student/adam"]["t"] == 3

    # ---- the checkpoint serves inference (auto = student) and eval_finetune ----
    out = str(tmp_path / "student.csv")
    FLAGS.reset()
    st = inference.main(COMMON + ["--input_data_pattern", pattern, "--train_dir", sdir, "--output_file", out, "--batch_size", "5", "--top_k", "5"])
    assert st["tower"] == "student" and st["videos"] == 16
    assert len(inference.read_prediction_file(out)) == 16
    FLAGS.reset()
    info = eval_finetune.main(COMMON + ["--eval_data_pattern", pattern, "--train_dir", sdir, "--batch_size", "8", "--run_once", "True"])
    assert info["epoch_id"] == 3 and np.isfinite(info["avg_loss"])

    # ---- resume: the same settings go on from step 3, another --teacher_mode is refused ----
    FLAGS.reset()
    with pytest.raises(ValueError, match="recorded"):
        train.main(COMMON + ["--train_data_pattern", pattern, "--train_dir", sdir, "--batch_size", "8", "--num_epochs", "1", "--max_steps", "1",
                             "--teacher_preds_pattern", preds, "--teacher_mode", "max"])
    FLAGS.reset()
    res = train.main(COMMON + ["--train_data_pattern", pattern, "--train_dir", sdir, "--batch_size", "8", "--num_epochs", "1", "--max_steps", "1",
                               "--teacher_preds_pattern", preds])
    assert res["graph"].global_step == 4 and train.latest_checkpoint(sdir).endswith("model.ckpt-4.pt")

    # ---- a record whose id the file does not hold ----
    lines = open(preds).read().splitlines(keepends=True)
    short = str(tmp_path / "short.csv")
    with open(short, "w") as f:
        f.writelines(lines[:-1])
    gone = lines[-1].split(",")[0]
    FLAGS.reset()
    with pytest.raises(KeyError) as e:
        train.main(COMMON + ["--train_data_pattern", pattern, "--train_dir", str(tmp_path / "model_short") + "/", "--batch_size", "8",
                             "--num_epochs", "1", "--start_new_model", "True", "--teacher_preds_pattern", short])
    assert gone in str(e.value) and short in str(e.value)
    FLAGS.reset()

    # ---- two identical runs under EVC_DETERMINISTIC=1 (read once per process: a fresh one) write bit-identical checkpoints ----
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(root, "tests", "_offline_distill_child.py"), pattern, preds,
                        str(tmp_path / "det_a") + "/", str(tmp_path / "det_b") + "/"],
                       env=dict(os.environ, EVC_DETERMINISTIC="1"), capture_output=True, text=True)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1].startswith("ok")
