"""Helper process of tests/test_gpu_step_entry.py (started with EVC_DETERMINISTIC=1, which is read once per process): the two paths of
the graphs' shared step() entry.  Two graphs from the same seed; one steps from the default stream (ordered onto the graph's main
stream and back), the other from inside torch.cuda.stream(graph._main) (the shortcut).  Every output tensor and every tower's
state_dict() must be torch.equal.  Exits non-zero on the first mismatch.

    python tests/_step_entry_child.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from efficientvideoclassification_youtube8m_amd import ops  # noqa: E402
from efficientvideoclassification_youtube8m_amd.distill import DistillGraph, EvalGraph, SerialStudentsGraph  # noqa: E402

DEV = "cuda:0"
B, F, V, H = 4, 128, 100, 128
KW = dict(feature_size=F, vocab_size=V, lstm_cells=H, device=DEV)

if not ops.DETERMINISTIC:
    sys.exit("EVC_DETERMINISTIC is not set in this process")
rng = np.random.default_rng(4)
n = np.asarray([300, 7, 295, 151], dtype=np.int32)           # full length, one short video, counts off every grid
batch = (torch.from_numpy(rng.standard_normal((B, 300, F)).astype(np.float32)).to(DEV),
         torch.from_numpy((rng.random((B, V)) < 0.05).astype(np.uint8)).to(DEV), torch.from_numpy(n).to(DEV))
torch.cuda.synchronize()


def tensors(v, path, into):
    if isinstance(v, torch.Tensor):
        into[path] = v
    elif isinstance(v, dict):
        for k in v:
            tensors(v[k], "%s/%s" % (path, k), into)
    elif isinstance(v, (list, tuple)):
        for i, e in enumerate(v):
            tensors(e, "%s/%d" % (path, i), into)
    return into


def run(make, towers, from_main):
    g = make()
    if from_main:
        with torch.cuda.stream(g._main):
            out = g.step(*batch, num_frames_host=n)
    else:
        out = g.step(*batch, num_frames_host=n)
    torch.cuda.synchronize()
    got = tensors(out, "out", {})
    for i, tw in enumerate(towers(g)):
        if tw is not None:
            tensors(tw.state_dict(), "tower%d" % i, got)
    return {k: v.clone() for k, v in got.items()}


GRAPHS = (
    ("DistillGraph teacher_student", lambda: DistillGraph(B, every_n=10, seed=5, **KW), lambda g: (g.teacher, g.student)),
    ("SerialStudentsGraph K = 2", lambda: SerialStudentsGraph(B, every_n=(10, 30), student_sampling=("uniform", "last"), seed=5, **KW),
     lambda g: [g.teacher] + g.students),
    ("EvalGraph", lambda: EvalGraph(B, every_n=10, **KW), lambda g: (g.teacher, g.student)),
)
for name, make, towers in GRAPHS:
    a, b = run(make, towers, False), run(make, towers, True)
    if sorted(a) != sorted(b) or not a:
        sys.exit("%s: the two entries return different tensors: %s" % (name, sorted(set(a) ^ set(b))))
    for k in sorted(a):
        if not torch.equal(a[k], b[k]):
            sys.exit("%s: %s differs between step() from the default stream and from the graph's main stream" % (name, k))
    print("%s: %d tensors bit-identical from either stream" % (name, len(a)))
print("ok")
