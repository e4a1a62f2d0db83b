"""Helper process of tests/test_gpu_serial_students.py (started with EVC_DETERMINISTIC=1, which is read once per process): a K = 3
SerialStudentsGraph and three K = 1 graphs start from the same weights and run two iterations on the same batch; student k's weights
and Adam moments must be torch.equal between the two.  Exits non-zero on the first mismatch.

    python tests/_serial_students_child.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import model_math as mm  # noqa: E402
from efficientvideoclassification_youtube8m_amd import ops  # noqa: E402
from efficientvideoclassification_youtube8m_amd.distill import DistillGraph, SerialStudentsGraph  # noqa: E402

DEV = "cuda:0"
B, F, H, V = 5, 64, 64, 40
KW = dict(feature_size=F, vocab_size=V, lstm_cells=H, device=DEV)
EVERY_N, SAMPLING, LOSSES = (30, 10, 30), ("uniform", "uniform", "last"), (("rep", "pred", "ce"), ("rep", "pred"), ("rep", "pred", "ce"))

if not ops.DETERMINISTIC:
    sys.exit("EVC_DETERMINISTIC is not set in this process")
q, x, n, labels = mm.synthetic_batch(B, seed=21, feature_size=F, vocab_size=V, dtype=np.float32)
dev = (torch.from_numpy(x).to(DEV), torch.from_numpy(labels.astype(np.uint8)).to(DEV), torch.from_numpy(n).to(DEV))
t = DistillGraph(B, mode="teacher", seed=5, every_n=30, **KW)
for _ in range(2):
    t.step(*dev, num_frames_host=n)
teacher_sd = {k: v.clone() for k, v in t.teacher.state_dict().items()}


def run(every_n, sampling, losses):
    g = SerialStudentsGraph(B, every_n=every_n, student_sampling=sampling, distill_losses=losses, seed=5, sampling_seed=3, **KW)
    g.teacher.load_state_dict(teacher_sd)
    for _ in range(2):
        g.step(*dev, num_frames_host=n)
    g.flush()
    torch.cuda.synchronize()
    assert g.global_step == 2
    return g


together = run(EVERY_N, SAMPLING, LOSSES)
for k in range(3):
    alone = run(EVERY_N[k:k + 1], SAMPLING[k:k + 1], LOSSES[k:k + 1])
    a, b = alone.students[0], together.students[k]
    if a.adam_t != 2 or b.adam_t != 2:
        sys.exit("student %d: adam_t %d alone, %d together" % (k, a.adam_t, b.adam_t))
    sa, sb = a.state_dict(), b.state_dict()
    for name in sa:
        if not torch.equal(sa[name], sb[name]):
            sys.exit("student %d: %s differs between the K = 1 and the K = 3 run (max |diff| %.3g)" % (
                k, name, float((sa[name] - sb[name]).abs().max())))
    for what, u, v in (("m", a.store.m, b.store.m), ("v", a.store.v, b.store.v)):
        if not torch.equal(u, v):
            sys.exit("student %d: Adam moment %s differs between the K = 1 and the K = 3 run" % (k, what))
    if not torch.equal(alone.losses[0], together.losses[k]):
        sys.exit("student %d: the loss values of the last step differ" % k)
    print("student %d (every_n %d, %s, %s): weights, moments and losses bit-identical alone and in company" % (
        k, EVERY_N[k], SAMPLING[k], "+".join(LOSSES[k])))
print("ok")
