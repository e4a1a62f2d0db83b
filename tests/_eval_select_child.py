"""Child process of tests/test_gpu_eval_select.py: one evaluation binary on one checkpoint, with and without --metrics_on_device,
under EVC_DETERMINISTIC=1 (set by the parent; the library reads it once per process).  The default cross-entropy loss is summed
with float atomics, so the loss of two separate runs - of the same path, too - differs in its last bits; with the fixed-order
sum both runs log the same device scalar and avg_loss can be compared with ==, like the metrics.

    python tests/_eval_select_child.py <validate|eval_finetune> <data dir> <train dir> <result.pkl>

Writes {"host": epoch dict, "device": epoch dict, "videos": n, "ties_at_k": [ids], "ties_at_n_pos": [ids]}: the ties are the
rows of the predictions the binaries see (same checkpoint, records, batches, precision) where np.argpartition and the device may
select differently - the precondition of ==.
"""
import os
import pickle
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _eval_select_ref as ref  # noqa: E402

COMMON = ["--frame_features", "True", "--feature_names", "rgb, audio", "--feature_sizes", "64, 64", "--model",
          "HierarchicalLstmModel", "--gpu", "0", "--num_inputs_to_lstm", "20", "--lstm_layers", "2", "--lstm_cells", "64",
          "--every_n", "10", "--num_readers", "2"]
BATCH, TOP_K = 5, 20


def boundary_ties(pattern, sd, student_only):
    from efficientvideoclassification_youtube8m_amd import readers
    from efficientvideoclassification_youtube8m_amd.distill import EvalGraph
    eg = EvalGraph(BATCH, every_n=10, student_only=student_only, feature_size=128, lstm_cells=64, device="cuda:0")
    eg.restore({k: v for k, v in sd.items() if torch.is_tensor(v)})
    rd = readers.YT8MFrameFeatureReader(feature_names=["rgb", "audio"], feature_sizes=[64, 64], max_frames=300)
    videos, ties_k, ties_n = 0, [], []
    for ids, qd, yd, nd, nh in readers.get_input_evaluation_tensors(rd, pattern, BATCH, 2, device="cuda:0", with_host_counts=True):
        p = eg.step(qd, yd, nd, num_frames_host=nh)["predictions"].cpu().numpy()
        at_k, at_n = ref.boundary_ties(p, yd.cpu().numpy(), TOP_K)
        ties_k += [ids[r] for r in at_k]
        ties_n += [ids[r] for r in at_n]
        videos += len(ids)
    return videos, ties_k, ties_n


def main():
    binary, data, tdir, result = sys.argv[1:5]
    from efficientvideoclassification_youtube8m_amd import eval_finetune, ops, train, validate
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    assert ops.DETERMINISTIC, "run with EVC_DETERMINISTIC=1"
    run = {"validate": validate.main, "eval_finetune": eval_finetune.main}[binary]
    pattern = os.path.join(data, "validate*.tfrecord")
    sd = torch.load(train.latest_checkpoint(tdir))
    videos, ties_k, ties_n = boundary_ties(pattern, sd, binary == "eval_finetune")
    args = COMMON + ["--eval_data_pattern", pattern, "--train_dir", tdir, "--batch_size", str(BATCH), "--top_k", str(TOP_K),
                     "--run_once", "True"]
    FLAGS.reset()
    host = run(args)
    FLAGS.reset()
    device = run(args + ["--metrics_on_device", "True"])
    with open(result, "wb") as f:
        pickle.dump({"host": host, "device": device, "videos": videos, "ties_at_k": ties_k, "ties_at_n_pos": ties_n}, f)


if __name__ == "__main__":
    main()
