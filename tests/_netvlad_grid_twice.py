"""Helper process of tests/test_gpu_netvlad_packed.py (the library reads EVC_DETERMINISTIC once per process): two SingleTowerGraph
over NetVLAD grid towers built from the same seed make the same two steps on the same two batches (another row count in the
second); the loss, the gradient store and the master weights must agree BIT FOR BIT after each.  Prints one line per compared tensor
and exits 1 if any differs.

    EVC_DETERMINISTIC=1 python tests/_netvlad_grid_twice.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import model_math as mm  # noqa: E402
from efficientvideoclassification_youtube8m_amd import ops  # noqa: E402
from efficientvideoclassification_youtube8m_amd.distill import SingleTowerGraph  # noqa: E402
from efficientvideoclassification_youtube8m_amd.towers import NetVladTower  # noqa: E402

DEV = "cuda:0"
B, F, V = 16, 128, 40
bad = []


def same(name, a, b):
    ok = a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    print("%-28s %s" % (name, "equal" if ok else "DIFFERS"))
    if not ok:
        bad.append(name)


q, x, n, labels = mm.synthetic_batch(B, seed=7, feature_size=F, vocab_size=V, dtype=np.float32)
qd, yd = torch.from_numpy(q).to(DEV), torch.from_numpy(labels.astype(np.uint8)).to(DEV)
counts = [n, np.maximum(n // 2, 1).astype(np.int32)]
graphs = [SingleTowerGraph(NetVladTower(B, 300, F, V, cluster_size=64, hidden_size=64, device=DEV, seed=5, frames="grid", every_n=10),
                           base_learning_rate=0.01) for _ in range(2)]
print("deterministic %d" % int(ops.DETERMINISTIC))
for it in range(2):
    nh = counts[it]
    nd = torch.from_numpy(nh).to(DEV)
    outs = [g.step(qd, yd, nd, num_frames_host=nh) for g in graphs]
    torch.cuda.synchronize()
    a, b = graphs
    same("step %d: loss" % it, outs[0]["loss"], outs[1]["loss"])
    same("step %d: gradient store" % it, a.tower.store.grad, b.tower.store.grad)
    same("step %d: master weights" % it, a.tower.store.master, b.tower.store.master)
    assert np.isfinite(float(outs[0]["loss"]))
sys.exit(1 if bad else 0)
