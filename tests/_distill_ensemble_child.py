"""Helper process of tests/test_gpu_distill_ensemble_graph.py (started with EVC_DETERMINISTIC=1, which is read once per process): an
EnsembleDistillGraph with ONE teacher, one with the same teacher listed twice under mean [.5, .5] and one with it listed three times
under max start from the same weights and run two iterations on the same batch; the student's weights and Adam moments must be
torch.equal among them.  Exits non-zero on the first mismatch.

    python tests/_distill_ensemble_child.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import model_math as mm  # noqa: E402
from efficientvideoclassification_youtube8m_amd import ops  # noqa: E402
from efficientvideoclassification_youtube8m_amd.distill import DistillGraph, EnsembleDistillGraph  # noqa: E402

DEV = "cuda:0"
B, F, H, V = 5, 64, 64, 40
KW = dict(feature_size=F, vocab_size=V, lstm_cells=H, device=DEV)

if not ops.DETERMINISTIC:
    sys.exit("EVC_DETERMINISTIC is not set in this process")
q, x, n, labels = mm.synthetic_batch(B, seed=21, feature_size=F, vocab_size=V, dtype=np.float32)
dev = (torch.from_numpy(x).to(DEV), torch.from_numpy(labels.astype(np.uint8)).to(DEV), torch.from_numpy(n).to(DEV))
t = DistillGraph(B, mode="teacher", seed=5, every_n=30, **KW)
for _ in range(2):
    t.step(*dev, num_frames_host=n)
teacher_sd = {k: v.clone() for k, v in t.teacher.state_dict().items()}


def run(J, **kw):
    g = EnsembleDistillGraph(B, teachers=[("teacher",)] * J, every_n=30, seed=5, **dict(KW, **kw))
    for tw in g.teachers:
        tw.load_state_dict(teacher_sd)
    for _ in range(2):
        g.step(*dev, num_frames_host=n)
    g.flush()
    torch.cuda.synchronize()
    assert g.global_step == 2
    return g


one = run(1)
for what, g in (("twice under mean [.5, .5]", run(2, teacher_mode="mean", teacher_weights=[0.5, 0.5])),
                ("three times under max", run(3, teacher_mode="max", rep_weights=[0.0, 0.0, 1.0]))):
    a, b = one.student, g.student
    if a.adam_t != 2 or b.adam_t != 2:
        sys.exit("%s: adam_t %d with one teacher, %d here" % (what, a.adam_t, b.adam_t))
    sa, sb = a.state_dict(), b.state_dict()
    for name in sa:
        if not torch.equal(sa[name], sb[name]):
            sys.exit("%s: %s differs from the one-teacher run (max |diff| %.3g)" % (what, name, float((sa[name] - sb[name]).abs().max())))
    for mom, u, v in (("m", a.store.m, b.store.m), ("v", a.store.v, b.store.v)):
        if not torch.equal(u, v):
            sys.exit("%s: Adam moment %s differs from the one-teacher run" % (what, mom))
    if not torch.equal(one.losses[0:4], g.losses[0:4]):
        sys.exit("%s: the loss values of the last step differ" % what)
    print("the teacher listed %s: weights, moments and losses bit-identical to the one-teacher run" % what)
print("ok")
