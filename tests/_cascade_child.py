"""Child process of tests/test_gpu_cascade_inference.py: one training run and its converted student, then every inference.py /
validate.py call with --cascade_dirs the module checks, under EVC_DETERMINISTIC=1 (set by the parent), at --precision bf16.

    python tests/_cascade_child.py <work dir> <result.pkl>

First each tower's own EvalGraph predictions on the batches the binaries see; the expectations are tests/_cascade_ref.py applied to
those.  Writes a dict: per case the file's lines, the expected lines, the run's stats; the stage file and its expectation; for validate
the two epoch dicts and the host-side expectation; for the one --precision high case the largest distance of a printed confidence from
the float64 oracle of the tower that decided the video.
"""
import os
import pickle
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _cascade_ref as ref  # noqa: E402
import _ensemble_ref as ens_ref  # noqa: E402
import _eval_select_ref as sel_ref  # noqa: E402
from oracle import model_math as mm  # noqa: E402

COMMON = ["--frame_features", "True", "--feature_names", "rgb, audio", "--feature_sizes", "64, 64", "--model",
          "HierarchicalLstmModel", "--gpu", "0", "--num_inputs_to_lstm", "20", "--lstm_layers", "2", "--lstm_cells", "64",
          "--every_n", "10", "--num_readers", "2"]
BATCH, TOP_K = 5, 20
# name -> (checkpoint, tower, every_n, student_sampling): the three stages the cases are built from
STAGES = {"student30": ("student", "student", 30, "uniform"), "student10last": ("student", "student", 10, "last"),
          "teacher": ("teacher", "teacher", 1, "uniform")}


def format_lines(ids, values, indices):
    """The prediction file's line format (cs/inference_ensemble.py:63-74), restated."""
    return [vid + "," + " ".join("%i %f" % (c, v) for c, v in zip(i, vals)) + "\n"
            for vid, vals, i in zip(ids, values.tolist(), indices.tolist())]


def stage_lines(ids, stage_of, confidence):
    return ["%s,%d,%f\n" % (vid, s, c) for vid, s, c in zip(ids, stage_of.tolist(), confidence.tolist())]


def tower_predictions(files, sds, precision):
    """[(ids, {stage name: predictions [b, 4716]}, labels)] per batch: each tower's own EvalGraph, every row live."""
    from efficientvideoclassification_youtube8m_amd import readers
    from efficientvideoclassification_youtube8m_amd.distill import EvalGraph
    graphs = {}
    for name, (ck, tower, every_n, sampling) in STAGES.items():
        g = EvalGraph(BATCH, every_n=every_n, student_only=tower == "student", teacher_only=tower == "teacher", feature_size=128,
                      lstm_cells=64, device="cuda:0", precision=precision, student_sampling=sampling)
        g.restore(sds[ck])
        graphs[name] = g
    rd = readers.YT8MFrameFeatureReader(feature_names=["rgb", "audio"], feature_sizes=[64, 64], max_frames=300)
    batches = []
    for ids, qd, yd, nd, nh in readers.get_input_evaluation_tensors(rd, files, BATCH, 2, device="cuda:0", with_host_counts=True):
        preds = {name: g.step(qd, yd, nd, num_frames_host=nh)["predictions"].cpu().numpy().copy() for name, g in graphs.items()}
        batches.append(([i.decode("utf-8") if isinstance(i, bytes) else i for i in ids], preds, yd.cpu().numpy().copy(),
                        np.asarray(nh).astype(np.int32).copy()))
    return batches


def oracle_predictions(files, sds):
    """{stage name: {video id: float64 predictions}} for the uniform stages (float64 H-LSTM forward of the oracle)."""
    from efficientvideoclassification_youtube8m_amd import readers
    rd = readers.YT8MFrameFeatureReader(feature_names=["rgb", "audio"], feature_sizes=[64, 64], max_frames=300)
    ids, q, n = [], [], []
    for i, mat, _, nf in rd.prepare_reader(files):
        ids.append(i[0]); q.append(mat[0]); n.append(nf[0])
    ids = [i.decode("utf-8") if isinstance(i, bytes) else i for i in ids]
    q, n = np.stack(q), np.asarray(n)
    xn = mm.l2_normalize(mm.dequantize(q.astype(np.float64)) * (np.arange(300)[None, :, None] < n[:, None, None]), 2)
    out = {}
    for name in ("student30", "teacher"):
        ck, tower, every_n, _ = STAGES[name]
        scope = "model" if tower == "teacher" else "model_student"
        params = {k[len(scope) + 1:]: v.double().numpy() for k, v in sds[ck].items() if k.startswith(scope + "/") and torch.is_tensor(v)}
        if tower == "teacher":
            _, pred, _ = mm.hlstm_fwd(xn, n, params, 20)
        else:
            _, pred, _ = mm.hlstm_fwd(xn[:, mm.every_n_indices(every_n)], mm.student_num_frames(n, every_n), params, 5)
        out[name] = dict(zip(ids, pred))
    return out


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
    sds = {"teacher": sd, "student": sdf}

    def run_inference(name, args, precision="bf16"):
        out = os.path.join(work, name + ".csv")
        FLAGS.reset()
        st = inference.main(COMMON + ["--input_data_pattern", pattern, "--output_file", out, "--batch_size", str(BATCH), "--top_k", str(TOP_K),
                                      "--precision", precision] + args)
        text = open(out).read()
        assert text.startswith("VideoId,LabelConfidencePairs\n") and text.endswith("\n")
        keep = ("tower", "members", "videos", "batches", "stage_videos", "stage_frames", "stage_steps", "gate_wait_s")
        return [l + "\n" for l in text.split("\n")[1:-1]], {k: st[k] for k in keep if k in st}

    batches = tower_predictions(files, sds, "bf16")
    res = {"cases": {}}

    def expect(names, kind, thresholds=None, fractions=None):
        """(prediction lines, stage lines, rows per stage, stage_of per video id, merged per batch) of the reference's cascade over `names`."""
        lines, slines, rows, decided, merged = [], [], [0] * len(names), {}, []
        for ids, preds, _, nf in batches:
            out = ref.cascade([preds[n] for n in names], nf, kind, thresholds, fractions)
            lines += format_lines(ids, *ens_ref.topk(out["merged"], TOP_K))
            slines += stage_lines(ids, out["stage_of"], out["confidence"])
            rows = [a + b for a, b in zip(rows, out["stage_rows"])]
            decided.update(zip(ids, out["stage_of"].tolist()))
            merged.append(out["merged"])
        return dict(lines=lines, stage_lines=slines, stage_rows=rows, decided=decided, merged=merged)

    def case(name, args, want, precision="bf16"):
        lines, st = run_inference(name, args, precision)
        res["cases"][name] = dict(lines=lines, stats=st, expected=want["lines"] if want else None,
                                  expected_rows=want["stage_rows"] if want else None)
        return lines

    two = ["--cascade_dirs", fdir + "," + tdir, "--cascade_every_n", "30,1"]
    # ---- the single-model files cases (a) and (b) must reproduce ----
    case("single_student30", ["--train_dir", fdir, "--every_n", "30"], None)
    case("single_teacher", ["--train_dir", tdir], None)
    # ---- (a) nobody escalates, (b) everybody does ----
    case("a", two + ["--cascade_thresholds=-inf"], expect(["student30", "teacher"], "top1", thresholds=[-np.inf]))
    case("b", two + ["--cascade_fractions", "1"], expect(["student30", "teacher"], "top1", fractions=[1.0]))
    # ---- (c) the threshold is the median of the student's own top1 confidences: half of the videos escalate ----
    own = np.concatenate([preds["student30"].max(axis=1) for _, preds, _, _ in batches])
    t_c = float(np.median(own.astype(np.float64)))
    want_c = expect(["student30", "teacher"], "top1", thresholds=[t_c])
    res["c_decided"], res["c_threshold"] = want_c["decided"], t_c
    res["c_single"] = {}
    for ids, preds, _, _ in batches:                          # every video's line as each tower alone prints it
        for n in ("student30", "teacher"):
            for vid, line in zip(ids, format_lines(ids, *ens_ref.topk(preds[n], TOP_K))):
                res["c_single"][(n, vid)] = line
    case("c", two + ["--cascade_thresholds", repr(t_c)], want_c)
    # ---- (d) margin, at most half of each batch ----
    case("d", two + ["--cascade_confidence", "margin", "--cascade_fractions", "0.5"], expect(["student30", "teacher"], "margin", fractions=[0.5]))
    # ---- (e) three stages from the two checkpoints, a threshold and a fraction on the first gate, the stage file ----
    own10 = np.concatenate([preds["student10last"].max(axis=1) for _, preds, _, _ in batches])
    t_e1 = float(np.median(own10.astype(np.float64)))
    want_e = expect(["student30", "student10last", "teacher"], "top1", thresholds=[t_c, t_e1], fractions=[0.6, 1.0])
    stage_csv = os.path.join(work, "e_stages.csv")
    case("e", ["--cascade_dirs", ",".join([fdir, fdir, tdir]), "--cascade_every_n", "30,10,1", "--cascade_sampling", "uniform,last,uniform",
               "--cascade_thresholds", "%r,%r" % (t_c, t_e1), "--cascade_fractions", "0.6,1", "--cascade_stage_file", stage_csv], want_e)
    res["e_stage_file"], res["e_stage_expected"] = open(stage_csv).read(), "VideoId,Stage,Confidence\n" + "".join(want_e["stage_lines"])

    # ---- (f) validate on the cascade of (c): host metrics, then --metrics_on_device ----
    vargs = COMMON + ["--eval_data_pattern", pattern, "--train_dir", os.path.join(work, "events") + "/", "--batch_size", str(BATCH),
                      "--top_k", str(TOP_K), "--run_once", "True", "--precision", "bf16"] + two + ["--cascade_thresholds", repr(t_c)]
    FLAGS.reset()
    res["validate_host"] = validate.main(vargs)
    FLAGS.reset()
    res["validate_device"] = validate.main(vargs + ["--metrics_on_device", "True"])
    FLAGS.reset()
    metrics = eval_util.EvaluationMetrics(4716, TOP_K)
    ties_k, ties_n = [], []
    for (ids, _, labels, _), comb in zip(batches, want_c["merged"]):
        metrics.accumulate(comb, labels.astype(np.float32), host_ce(comb, labels))
        at_k, at_n = sel_ref.boundary_ties(comb, labels, TOP_K)
        ties_k += [ids[r] for r in at_k]
        ties_n += [ids[r] for r in at_n]
    res["validate_expected"], res["validate_expected_rows"] = metrics.get(), want_c["stage_rows"]
    res["ties_at_k"], res["ties_at_n_pos"] = ties_k, ties_n

    # ---- one case at --precision high: against the float64 oracle of the deciding tower only ----
    high_csv = os.path.join(work, "high_stages.csv")
    lines, st = run_inference("high", two + ["--cascade_thresholds", repr(t_c), "--cascade_stage_file", high_csv], "high")
    oracle = oracle_predictions(files, sds)
    decided = {l.split(",")[0]: int(l.split(",")[1]) for l in open(high_csv).read().split("\n")[1:-1]}
    worst = 0.0
    for line in lines:
        vid, pairs = line.rstrip("\n").split(",")
        toks = pairs.split(" ")
        cls, conf = np.array(toks[0::2], np.int64), np.array(toks[1::2], np.float64)
        worst = max(worst, float(np.abs(conf - oracle[("student30", "teacher")[decided[vid]]][vid][cls]).max()))
    res["high"] = dict(worst=worst, stats=st, decided=decided, videos=len(lines))
    with open(result, "wb") as f:
        pickle.dump(res, f)


if __name__ == "__main__":
    main()
