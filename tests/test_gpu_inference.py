"""inference.py on TFRecord files at the small dims of test_gpu_workflow.py: a train.py checkpoint serves the teacher, a
train_convert_model checkpoint the student; the file is checked line by line against the host top-k of the same tower's
EvalGraph predictions on the same batches, and its confidences against the float64 oracle."""
import numpy as np
import pytest
import torch

from oracle import model_math as mm

pytestmark = pytest.mark.gpu

COMMON = ["--frame_features", "True", "--feature_names", "rgb, audio", "--feature_sizes", "64, 64", "--model",
          "HierarchicalLstmModel", "--gpu", "0", "--num_inputs_to_lstm", "20", "--lstm_layers", "2", "--lstm_cells", "64",
          "--every_n", "10", "--num_readers", "2"]


def _reference_format_lines(video_ids, predictions, top_k):
    """cs/inference_ensemble.py:63-74 with the class-ascending order of ties (the reference leaves it undefined)."""
    col = np.broadcast_to(np.arange(predictions.shape[1]), predictions.shape)
    order = np.lexsort((col, -predictions.astype(np.float64)), axis=-1)[:, :top_k]
    for r, vid in enumerate(video_ids):
        yield vid + "," + " ".join("%i %f" % (c, predictions[r, c]) for c in order[r]) + "\n"


def _oracle(files, sd, tower):
    """Dequantize / pad / l2-normalise (/ sub-sample) + H-LSTM forward in float64 for every record: {video id: predictions}."""
    from efficientvideoclassification_youtube8m_amd import readers
    rd = readers.YT8MFrameFeatureReader(feature_names=["rgb", "audio"], feature_sizes=[64, 64], max_frames=300)
    ids, q, n = [], [], []
    for i, mat, _, nf in rd.prepare_reader(files):
        ids.append(i[0]); q.append(mat[0]); n.append(nf[0])
    q, n = np.stack(q), np.asarray(n)
    xn = mm.l2_normalize(mm.dequantize(q.astype(np.float64)) * (np.arange(300)[None, :, None] < n[:, None, None]), 2)

    def params(scope):
        return {k[len(scope) + 1:]: v.double().numpy() for k, v in sd.items() if k.startswith(scope + "/") and torch.is_tensor(v)}
    if tower == "teacher":
        _, pred, _ = mm.hlstm_fwd(xn, n, params("model"), 20)
    else:
        _, pred, _ = mm.hlstm_fwd(xn[:, mm.every_n_indices(10)], mm.student_num_frames(n, 10), params("model_student"), 5)
    return dict(zip(ids, pred))


def _check_file(path, files, sd, tower, k, precision):
    from efficientvideoclassification_youtube8m_amd import readers
    from efficientvideoclassification_youtube8m_amd.distill import EvalGraph
    text = open(path).read()
    assert text.startswith("VideoId,LabelConfidencePairs\n") and text.endswith("\n")
    lines = text.split("\n")[1:-1]
    # the same tower's EvalGraph predictions on the same batches (batch size 5, 2 readers), top-k on the host
    g = EvalGraph(5, every_n=10, student_only=tower == "student", teacher_only=tower == "teacher", feature_size=128, lstm_cells=64,
                  device="cuda:0", precision=precision)
    g.restore(sd)
    rd = readers.YT8MFrameFeatureReader(feature_names=["rgb", "audio"], feature_sizes=[64, 64], max_frames=300)
    want, pred = [], {}
    for ids, qd, yd, nd, nh in readers.get_input_evaluation_tensors(rd, files, 5, 2, device="cuda:0", with_host_counts=True):
        p = g.step(qd, yd, nd, num_frames_host=nh)["predictions"].cpu().numpy()
        want += list(_reference_format_lines(ids, p, k))
        pred.update(zip(ids, p))
    assert len(lines) == len(want) == len(pred) == 16
    for got, exp in zip(lines, want):
        assert got + "\n" == exp
    oracle, checked, worst = _oracle(files, sd, tower), 0, 0.0
    for line in lines:
        vid, pairs = line.split(",")
        toks = pairs.split(" ")
        assert len(toks) == 2 * k
        cls, conf = np.array(toks[0::2], np.int64), np.array(toks[1::2], np.float64)
        worst = max(worst, float(np.abs(conf - oracle[vid][cls]).max()))     # every printed confidence, "%f" rounding included
        o = np.sort(oracle[vid])[::-1]
        if o[k - 1] - o[k] > 2e-3:                       # the oracle's top-k is unambiguous at this precision: same classes
            assert set(cls.tolist()) == set(np.argsort(-oracle[vid])[:k].tolist())
            checked += 1
    print("%s inference vs float64 oracle: %.2e; class sets compared on %d of %d videos" % (tower, worst, checked, len(lines)))
    assert worst < 1e-3 + 1e-6
    return lines


def test_inference_serves_teacher_then_student(tmp_path):
    from efficientvideoclassification_youtube8m_amd import inference, readers, train, train_convert_model
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    data = tmp_path / "yt8m"
    readers.write_synthetic_frame_dataset(str(data), 2, 8, feature_sizes=(64, 64), min_frames=60, max_frames=310, seed=1, prefix="train")
    files = readers.write_synthetic_frame_dataset(str(data), 2, 7, feature_sizes=(64, 64), min_frames=60, max_frames=310, seed=2,
                                                  prefix="test")
    rng = np.random.default_rng(3)                        # two test-set records without labels (one of 40 frames)
    extra = [readers.encode_frame_example("nolabel%d" % i, [], {"rgb": rng.integers(0, 256, (nf, 64), dtype=np.uint8),
                                                                  "audio": rng.integers(0, 256, (nf, 64), dtype=np.uint8)})
             for i, nf in enumerate((200, 40))]
    readers.write_tfrecord(str(data / "test0002.tfrecord"), extra)
    files = files + [str(data / "test0002.tfrecord")]     # 16 videos: batches of 5, 5, 5, 1
    pattern = str(data / "test*.tfrecord")
    tdir = str(tmp_path / "model_train") + "/"
    FLAGS.reset()
    train.main(COMMON + ["--train_data_pattern", str(data / "train*.tfrecord"), "--train_dir", tdir, "--batch_size", "8",
                         "--num_epochs", "1", "--start_new_model", "True"])
    sd = torch.load(train.latest_checkpoint(tdir))

    # ---- train.py checkpoint (model/* + model_student/*): the teacher ----
    out = str(tmp_path / "teacher.csv")
    FLAGS.reset()
    st = inference.main(COMMON + ["--input_data_pattern", pattern, "--train_dir", tdir, "--output_file", out, "--batch_size", "5",
                                  "--top_k", "20", "--precision", "high"])
    assert st["tower"] == "teacher" and st["videos"] == 16 and st["batches"] == 4
    lines = _check_file(out, files, sd, "teacher", 20, "high")
    assert any(l.startswith("nolabel0,") for l in lines) and any(l.startswith("nolabel1,") for l in lines)

    # ---- train_convert_model checkpoint (model_student/* only): the student ----
    FLAGS.reset()
    ck = train_convert_model.main(["--train_dir", tdir])
    fdir = train_convert_model.finetune_dir(tdir)
    sdf = torch.load(ck)
    for k in (20, 5):
        out = str(tmp_path / ("student%d.csv" % k))
        FLAGS.reset()
        st = inference.main(COMMON + ["--input_data_pattern", pattern, "--train_dir", fdir, "--output_file", out, "--batch_size", "5",
                                      "--top_k", str(k), "--precision", "high"])
        assert st["tower"] == "student" and st["videos"] == 16
        _check_file(out, files, sdf, "student", k, "high")
    FLAGS.reset()
