"""Child process of tests/test_gpu_ensemble_inference.py: one training run and its converted student, then every inference.py /
validate.py call the module checks, under EVC_DETERMINISTIC=1 (set by the parent; the library reads it once per process: the
cross-entropy loss is then summed in a fixed order, so two validate runs log the same scalar).

    python tests/_ensemble_child.py <work dir> <result.pkl>

Writes a dict: per inference case the file's lines, the lines expected from tests/_ensemble_ref.py applied to the members' own EvalGraph
predictions on the same batches (for the prediction-file case: to the values parsed from the file), and the largest distance of a
printed confidence from the float64 oracle combined the same way; for validate the two epoch dicts, the host-side expectation and the
rows with an exact tie at a selection boundary (the precondition of comparing host and device metrics with ==).
"""
import os
import pickle
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _ensemble_ref as ref  # noqa: E402
import _eval_select_ref as sel_ref  # noqa: E402
from oracle import model_math as mm  # noqa: E402

COMMON = ["--frame_features", "True", "--feature_names", "rgb, audio", "--feature_sizes", "64, 64", "--model",
          "HierarchicalLstmModel", "--gpu", "0", "--num_inputs_to_lstm", "20", "--lstm_layers", "2", "--lstm_cells", "64",
          "--every_n", "10", "--num_readers", "2"]
BATCH, TOP_K = 5, 20
WEIGHTS_B = [0.5, 0.25, 0.25]                               # case (b): sums to 1


def format_lines(ids, values, indices):
    """The file's line format (cs/inference_ensemble.py:63-74), restated."""
    return [vid + "," + " ".join("%i %f" % (c, v) for c, v in zip(i, vals)) + "\n"
            for vid, vals, i in zip(ids, values.tolist(), indices.tolist())]


def parse_file(path):
    """{id: (classes, float32 confidences)} of a prediction file, parsed here (not by the code under test)."""
    out = {}
    for line in open(path).read().split("\n")[1:-1]:
        vid, pairs = line.split(",")
        toks = pairs.split(" ")
        out[vid] = (np.array(toks[0::2], np.int32), np.array([float(t) for t in toks[1::2]], np.float32))
    return out


def member_predictions(files, towers):
    """towers: {name: (state dict, 'teacher' | 'student')} -> ([(ids, {name: predictions [b, 4716]}, labels)] per batch): each
    tower's own EvalGraph on the batches the binaries see (batch size 5, 2 readers, --precision high)."""
    from efficientvideoclassification_youtube8m_amd import readers
    from efficientvideoclassification_youtube8m_amd.distill import EvalGraph
    graphs = {}
    for name, (sd, tower) in towers.items():
        g = EvalGraph(BATCH, every_n=10, student_only=tower == "student", teacher_only=tower == "teacher", feature_size=128, lstm_cells=64,
                      device="cuda:0", precision="high")
        g.restore(sd)
        graphs[name] = g
    rd = readers.YT8MFrameFeatureReader(feature_names=["rgb", "audio"], feature_sizes=[64, 64], max_frames=300)
    batches = []
    for ids, qd, yd, nd, nh in readers.get_input_evaluation_tensors(rd, files, BATCH, 2, device="cuda:0", with_host_counts=True):
        preds = {name: g.step(qd, yd, nd, num_frames_host=nh)["predictions"].cpu().numpy().copy() for name, g in graphs.items()}
        batches.append(([i.decode("utf-8") if isinstance(i, bytes) else i for i in ids], preds, yd.cpu().numpy().copy()))
    return batches


def oracle_predictions(files, towers):
    """{name: {video id: float64 predictions}}: dequantize / pad / l2-normalise (/ sub-sample) + H-LSTM forward in float64."""
    from efficientvideoclassification_youtube8m_amd import readers
    rd = readers.YT8MFrameFeatureReader(feature_names=["rgb", "audio"], feature_sizes=[64, 64], max_frames=300)
    ids, q, n = [], [], []
    for i, mat, _, nf in rd.prepare_reader(files):
        ids.append(i[0]); q.append(mat[0]); n.append(nf[0])
    ids = [i.decode("utf-8") if isinstance(i, bytes) else i for i in ids]
    q, n = np.stack(q), np.asarray(n)
    xn = mm.l2_normalize(mm.dequantize(q.astype(np.float64)) * (np.arange(300)[None, :, None] < n[:, None, None]), 2)
    out = {}
    for name, (sd, tower) in towers.items():
        scope = "model" if tower == "teacher" else "model_student"
        params = {k[len(scope) + 1:]: v.double().numpy() for k, v in sd.items() if k.startswith(scope + "/") and torch.is_tensor(v)}
        if tower == "teacher":
            _, pred, _ = mm.hlstm_fwd(xn, n, params, 20)
        else:
            _, pred, _ = mm.hlstm_fwd(xn[:, mm.every_n_indices(10)], mm.student_num_frames(n, 10), params, 5)
        out[name] = dict(zip(ids, pred))
    return out


def worst_distance(lines, combined_oracle):
    """Largest |printed confidence - oracle| over every printed pair; combined_oracle(video id) -> float64 [4716]."""
    worst = 0.0
    for line in lines:
        vid, pairs = line.rstrip("\n").split(",")
        toks = pairs.split(" ")
        assert len(toks) == 2 * TOP_K
        cls, conf = np.array(toks[0::2], np.int64), np.array(toks[1::2], np.float64)
        worst = max(worst, float(np.abs(conf - combined_oracle(vid)[cls]).max()))
    return worst


def host_ce(pred, labels):
    """mean_b sum_c -(y log(p + 1e-5) + (1 - y) log(1 - p + 1e-5)) in float64 (cs/losses.py:90-97)."""
    p, y = pred.astype(np.float64), (labels != 0).astype(np.float64)
    return float((-(y * np.log(p + 1e-5) + (1 - y) * np.log(1 - p + 1e-5))).sum(1).mean())


def main():
    work, result = sys.argv[1:3]
    from efficientvideoclassification_youtube8m_amd import eval_util, inference, ops, readers, train, train_convert_model, validate
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    assert ops.DETERMINISTIC, "run with EVC_DETERMINISTIC=1"
    data = os.path.join(work, "yt8m")
    kw = dict(feature_sizes=(64, 64), num_classes=12, min_frames=60, max_frames=310)
    readers.write_synthetic_frame_dataset(data, 2, 8, seed=1, prefix="train", **kw)
    files = readers.write_synthetic_frame_dataset(data, 2, 7, seed=2, prefix="test", **kw)
    rng = np.random.default_rng(3)                            # two records without labels (one of 40 frames): 16 videos, batches of 5, 5, 5, 1
    extra = [readers.encode_frame_example("nolabel%d" % i, [], {"rgb": rng.integers(0, 256, (nf, 64), dtype=np.uint8),
                                                                  "audio": rng.integers(0, 256, (nf, 64), dtype=np.uint8)})
             for i, nf in enumerate((200, 40))]
    readers.write_tfrecord(os.path.join(data, "test0002.tfrecord"), extra)
    files = files + [os.path.join(data, "test0002.tfrecord")]
    pattern = os.path.join(data, "test*.tfrecord")
    tdir = os.path.join(work, "model_train") + "/"
    FLAGS.reset()
    train.main(COMMON + ["--train_data_pattern", os.path.join(data, "train*.tfrecord"), "--train_dir", tdir, "--batch_size", "8",
                         "--num_epochs", "1", "--start_new_model", "True"])
    sd = torch.load(train.latest_checkpoint(tdir))
    FLAGS.reset()
    sdf = torch.load(train_convert_model.main(["--train_dir", tdir]))
    fdir = train_convert_model.finetune_dir(tdir)

    def run_inference(name, args):
        out = os.path.join(work, name + ".csv")
        FLAGS.reset()
        st = inference.main(COMMON + ["--input_data_pattern", pattern, "--output_file", out, "--batch_size", str(BATCH), "--top_k", str(TOP_K),
                                      "--precision", "high"] + args)
        text = open(out).read()
        assert text.startswith("VideoId,LabelConfidencePairs\n") and text.endswith("\n")
        return out, text.split("\n")[1:-1], {k: st[k] for k in ("tower", "members", "videos", "batches")}

    towers = {"teacher": (sd, "teacher"), "student_parallel": (sd, "student"), "student": (sdf, "student")}
    batches = member_predictions(files, towers)
    oracle = oracle_predictions(files, towers)
    res = {"cases": {}}

    def case(name, args, expected, combined_oracle):
        path, lines, st = run_inference(name, args)
        res["cases"][name] = dict(lines=[l + "\n" for l in lines], expected=expected, stats=st,
                                  worst=worst_distance(lines, combined_oracle))
        return path

    def expected_lines(members, mode, weights=None, priors_of=None):
        want = []
        for ids, preds, _ in batches:
            comb = ref.combine([preds[m] for m in members], mode, weights, None if priors_of is None else priors_of(ids))
            want += format_lines(ids, *ref.topk(comb, TOP_K))
        return want

    # ---- no ensemble flag: the single-model files, the path tests/test_gpu_inference.py checks ----
    case("single_teacher", ["--train_dir", tdir], expected_lines(["teacher"], "max"), lambda v: oracle["teacher"][v])
    student_csv = case("single_student", ["--train_dir", fdir], expected_lines(["student"], "max"), lambda v: oracle["student"][v])

    # ---- (a) teacher + converted student, max ----
    case("a", ["--ensemble_dirs", tdir + "," + fdir, "--ensemble_mode", "max"], expected_lines(["teacher", "student"], "max"),
         lambda v: np.maximum(oracle["teacher"][v], oracle["student"][v]))

    # ---- (b) one directory twice (teacher + the student trained next to it) + the converted student, weighted mean ----
    wb = np.asarray(WEIGHTS_B, np.float32)
    case("b", ["--ensemble_dirs", ",".join([tdir, tdir, fdir]), "--ensemble_towers", "teacher,student,auto", "--ensemble_every_n", "1,10,10",
               "--ensemble_mode", "mean", "--ensemble_weights", ",".join(str(w) for w in WEIGHTS_B)],
         expected_lines(["teacher", "student_parallel", "student"], "mean", wb),
         lambda v: sum(float(w) * oracle[m][v] for w, m in zip(wb, ("teacher", "student_parallel", "student"))))

    # ---- (c) the teacher served + the student's own file through --preds_pattern, max ----
    parsed = parse_file(student_csv)

    def priors_of(ids):
        idx = np.full((1, len(ids), TOP_K), -1, np.int32)
        val = np.zeros((1, len(ids), TOP_K), np.float32)
        for b, vid in enumerate(ids):
            idx[0, b, :parsed[vid][0].size], val[0, b, :parsed[vid][1].size] = parsed[vid]
        return idx, val

    def oracle_c(vid):
        comb, listed = oracle["teacher"][vid].copy(), parsed[vid][0]
        comb[listed] = np.maximum(comb[listed], oracle["student"][vid][listed])
        return comb
    case("c", ["--ensemble_dirs", tdir, "--preds_pattern", student_csv, "--ensemble_mode", "max"],
         expected_lines(["teacher"], "max", None, priors_of), oracle_c)

    # ---- validate on the same two members as (a): host metrics, then --metrics_on_device ----
    vargs = COMMON + ["--eval_data_pattern", pattern, "--train_dir", os.path.join(work, "events") + "/", "--ensemble_dirs", tdir + "," + fdir,
                      "--ensemble_mode", "max", "--batch_size", str(BATCH), "--top_k", str(TOP_K), "--run_once", "True", "--precision", "high"]
    FLAGS.reset()
    res["validate_host"] = validate.main(vargs)
    FLAGS.reset()
    res["validate_device"] = validate.main(vargs + ["--metrics_on_device", "True"])
    FLAGS.reset()
    metrics = eval_util.EvaluationMetrics(4716, TOP_K)
    ties_k, ties_n = [], []
    for ids, preds, labels in batches:
        comb = ref.combine([preds["teacher"], preds["student"]], "max")
        metrics.accumulate(comb, labels.astype(np.float32), host_ce(comb, labels))
        at_k, at_n = sel_ref.boundary_ties(comb, labels, TOP_K)
        ties_k += [ids[r] for r in at_k]
        ties_n += [ids[r] for r in at_n]
    res["validate_expected"] = metrics.get()
    res["ties_at_k"], res["ties_at_n_pos"] = ties_k, ties_n
    with open(result, "wb") as f:
        pickle.dump(res, f)


if __name__ == "__main__":
    main()
