"""Helper process of tests/test_gpu_label_losses.py and tests/test_gpu_label_loss_graphs.py, started with EVC_DETERMINISTIC=1 (read once
per process).

    python tests/_label_loss_child.py digest    two digests over the loss and dpred bits of every evc_label_loss kind (two runs), then ok
    python tests/_label_loss_child.py graph     DistillGraph(label_loss=None) and (label_loss="CrossEntropyLoss") from the same seed run the
                                                same step: outputs, loss values, dL/dpred and every weight gradient must be torch.equal
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from efficientvideoclassification_youtube8m_amd import ops  # noqa: E402

if not ops.DETERMINISTIC:
    sys.exit("EVC_DETERMINISTIC is not set in this process")
mode = sys.argv[1] if len(sys.argv) > 1 else ""
if mode == "digest":
    import test_gpu_label_losses as t
    print(t._digest())
    print(t._digest())
elif mode == "graph":
    import test_gpu_label_loss_graphs as t
    a, b = t._default_path_step(None), t._default_path_step("CrossEntropyLoss")
    for (name, u), (_, v) in zip(a, b):
        if not torch.equal(u, v):
            sys.exit("%s differs between label_loss=None and label_loss='CrossEntropyLoss'" % name)
    print("%d tensors bit-identical" % len(a))
else:
    sys.exit("usage: _label_loss_child.py digest | graph")
print("ok")
