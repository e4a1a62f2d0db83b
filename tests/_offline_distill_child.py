"""Helper process of tests/test_gpu_offline_distill_workflow.py (started with EVC_DETERMINISTIC=1, which is read once per process): the
same train --teacher_preds_pattern run twice, into two directories; the two checkpoints must hold the same keys, the same metadata and
torch.equal tensors (weights and Adam moments).  Exits non-zero on the first mismatch.

    python tests/_offline_distill_child.py <train records pattern> <teacher prediction file> <directory A> <directory B>
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from efficientvideoclassification_youtube8m_amd import ops, train  # noqa: E402
from efficientvideoclassification_youtube8m_amd.flags import FLAGS  # noqa: E402

COMMON = ["--frame_features", "True", "--feature_names", "rgb, audio", "--feature_sizes", "64, 64", "--model", "HierarchicalLstmModel",
          "--gpu", "0", "--num_inputs_to_lstm", "20", "--lstm_layers", "2", "--lstm_cells", "64", "--every_n", "10", "--num_readers", "2"]

if not ops.DETERMINISTIC:
    sys.exit("EVC_DETERMINISTIC is not set in this process")
pattern, preds, dirs = sys.argv[1], sys.argv[2], sys.argv[3:5]
sds = []
for d in dirs:
    FLAGS.reset()
    train.main(COMMON + ["--train_data_pattern", pattern, "--train_dir", d, "--batch_size", "8", "--num_epochs", "2", "--max_steps", "3",
                         "--start_new_model", "True", "--teacher_preds_pattern", preds, "--student_sampling", "random"])
    sds.append(torch.load(train.latest_checkpoint(d), map_location="cpu"))
FLAGS.reset()
a, b = sds
if a.keys() != b.keys():
    sys.exit("the two checkpoints hold different keys: %s" % sorted(set(a) ^ set(b)))


def same(x, y):
    if torch.is_tensor(x):
        return torch.is_tensor(y) and torch.equal(x, y)
    if isinstance(x, dict):
        return isinstance(y, dict) and x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)
    return x == y


for k in a:
    if not same(a[k], b[k]):
        sys.exit("%s differs between two identical runs" % k)
print("ok: %d entries bit-identical" % len(a))
