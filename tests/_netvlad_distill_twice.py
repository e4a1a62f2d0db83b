"""Helper process of tests/test_gpu_netvlad_distill.py (the library reads EVC_DETERMINISTIC once per process): two
NetVladDistillGraph built from the same seeds and the same teacher weights make the same two steps on the same batch; the loss
values, the student's gradient store and its master weights must agree BIT FOR BIT after each.  Prints one line per compared tensor
and exits 1 if any differs.

    EVC_DETERMINISTIC=1 python tests/_netvlad_distill_twice.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import model_math as mm  # noqa: E402
from efficientvideoclassification_youtube8m_amd import ops  # noqa: E402
from efficientvideoclassification_youtube8m_amd.distill import NetVladDistillGraph  # noqa: E402
from efficientvideoclassification_youtube8m_amd.towers import NetVladTower  # noqa: E402

DEV = "cuda:0"
B, T, F, V = 16, 60, 128, 40
SIZES = dict(feature_size=F, vocab_size=V, max_frames=T, cluster_size=64, hidden_size=64)
bad = []


def same(name, a, b):
    ok = a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    print("%-28s %s" % (name, "equal" if ok else "DIFFERS"))
    if not ok:
        bad.append(name)


q, x, n, labels = mm.synthetic_batch(B, seed=7, max_frames=T, feature_size=F, vocab_size=V, dtype=np.float32)
n[2], n[9] = 0, 3
qd, nd, yd = torch.from_numpy(q).to(DEV), torch.from_numpy(n).to(DEV), torch.from_numpy(labels.astype(np.uint8)).to(DEV)
teacher = NetVladTower(B, T, F, V, cluster_size=64, hidden_size=64, device=DEV, seed=3, frames="grid", every_n=1)
teacher.forward(qd, nd, num_frames_host=n)             # (moving statistics away from their initial values)
sd = teacher.state_dict()
graphs = []
for _ in range(2):
    g = NetVladDistillGraph(B, every_n=10, teacher_every_n=1, device=DEV, seed=5, base_learning_rate=0.01, **SIZES)
    g.teacher.load_state_dict(sd)
    graphs.append(g)
print("deterministic %d" % int(ops.DETERMINISTIC))
for it in range(2):
    for g in graphs:
        g.step(qd, yd, nd, num_frames_host=n)
    torch.cuda.synchronize()
    a, b = graphs
    same("step %d: losses" % it, a.losses, b.losses)
    same("step %d: gradient store" % it, a.student.store.grad, b.student.store.grad)
    same("step %d: master weights" % it, a.student.store.master, b.student.store.master)
    same("step %d: teacher masters" % it, a.teacher.store.master, b.teacher.store.master)
assert all(np.isfinite(v) for v in graphs[0].loss_report().values())
sys.exit(1 if bad else 0)
