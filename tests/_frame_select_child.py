"""Helper process of tests/test_gpu_frame_select.py, started under EVC_DETERMINISTIC=1 (no floating-point atomics on the training path, so
two steps on the same numbers give the same bits): training steps of DistillGraph under --student_sampling words against the uniform
step, and the student's forward against EvalGraph.  Writes what it compared, as a dict of booleans and figures, to <out.pt>.

    python tests/_frame_select_child.py <out.pt>
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import _frame_select_ref as ref  # noqa: E402
from oracle import model_math as mm  # noqa: E402
from efficientvideoclassification_youtube8m_amd.distill import DistillGraph, EvalGraph  # noqa: E402

out_path = sys.argv[1]
DEV = "cuda:0"
B, EVERY_N = 6, 10
KW = dict(every_n=EVERY_N, feature_size=128, vocab_size=50, lstm_cells=64, device=DEV)          # the sizes of tests/test_gpu_workflow.py
q, x, n, labels = mm.synthetic_batch(B, seed=3, feature_size=128, vocab_size=50, dtype=np.float32)
n[0], n[1] = 300, 79
x[np.arange(300)[None, :] >= n[:, None]] = 0.0
xd, yd, nd = torch.from_numpy(x).to(DEV), torch.from_numpy(labels.astype(np.uint8)).to(DEV), torch.from_numpy(n).to(DEV)
res = {"deterministic": os.environ.get("EVC_DETERMINISTIC")}


def weights(tower):
    return {k: v.clone() for k, v in tower.state_dict().items()}


def same(a, b):
    return sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)


# ---- teacher + student: one step under "last" next to the step under "uniform" ----------------------------------------------------------
g_u, g_l = DistillGraph(B, seed=3, **KW), DistillGraph(B, seed=3, student_sampling="last", **KW)
res["same_start"] = same(weights(g_u.teacher), weights(g_l.teacher)) and same(weights(g_u.student), weights(g_l.student))
start = {**weights(g_l.teacher), **weights(g_l.student)}
o_u = g_u.step(xd, yd, nd, num_frames_host=n)
o_l = g_l.step(xd, yd, nd, num_frames_host=n)
torch.cuda.synchronize()
res["teacher_loss"] = (float(o_u["loss"]), float(o_l["loss"]))
res["teacher_loss_equal"] = torch.equal(o_u["loss"], o_l["loss"])
res["teacher_pred_equal"] = torch.equal(o_u["predictions"], o_l["predictions"]) and torch.equal(o_u["teacher_state"], o_l["teacher_state"])
res["teacher_weights_equal"] = same(weights(g_u.teacher), weights(g_l.teacher))
res["teacher_moved"] = not same(weights(g_l.teacher), {k: v for k, v in start.items() if k.startswith("model/")})
res["student_differs"] = not torch.equal(o_u["student_predictions"], o_l["student_predictions"])
res["table_last"] = bool((g_l.last_frame_table.cpu().numpy() == ref.table(n, 300, EVERY_N, "last")).all())
# the student's forward of that step against the forward-only graph on the weights the step started from
e = EvalGraph(B, student_sampling="last", **KW)
e.restore(start)
o_e = e.step(xd, yd, nd, num_frames_host=n)
torch.cuda.synchronize()
res["student_forward_equal"] = torch.equal(o_e["predictions"], o_l["student_predictions"]) and torch.equal(o_e["student_state"], o_l["student_state"])
res["eval_teacher_equal"] = torch.equal(o_e["teacher_predictions"], o_l["predictions"])
del g_u, g_l, e

# ---- student only: the step under "first" on x against the uniform step on the rearranged x' ---------------------------------------------
src = ref.table(n, 300, EVERY_N, "first")
xp = torch.from_numpy(ref.rearrange(x, src, EVERY_N)).to(DEV)
g_f, g_p = DistillGraph(B, mode="student", seed=3, student_sampling="first", **KW), DistillGraph(B, mode="student", seed=3, **KW)
w0 = weights(g_f.student)
o_f = g_f.step(xd, yd, nd, num_frames_host=n)
o_p = g_p.step(xp, yd, nd, num_frames_host=n)
o_x = DistillGraph(B, mode="student", seed=3, **KW).step(xd, yd, nd, num_frames_host=n)          # uniform on x itself: something else
torch.cuda.synchronize()
res["first_loss"] = (float(o_f["student_label_loss"]), float(o_p["student_label_loss"]))
res["first_loss_equal"] = torch.equal(o_f["student_label_loss"], o_p["student_label_loss"])
res["first_pred_equal"] = torch.equal(o_f["student_predictions"], o_p["student_predictions"])
res["first_weights_equal"] = same(weights(g_f.student), weights(g_p.student))
res["first_moved"] = not same(weights(g_f.student), w0)
res["first_is_not_uniform"] = not torch.equal(o_f["student_predictions"], o_x["student_predictions"])
res["table_first"] = bool((g_f.last_frame_table.cpu().numpy() == src).all())

# ---- "random": a new draw per iteration, reproducible from the seed -------------------------------------------------------------------
g_r = DistillGraph(B, mode="student", seed=3, student_sampling="random", sampling_seed=5, **KW)
tabs = []
for it in range(2):
    g_r.step(xd, yd, nd, num_frames_host=n)
    tabs.append(g_r.last_frame_table.cpu().numpy().copy())
res["random_tables"] = all((tabs[it] == ref.table(n, 300, EVERY_N, "random", seed=5, draw=it)).all() for it in range(2))
res["random_redrawn"] = bool((tabs[0] != tabs[1]).any())
torch.save(res, out_path)
print(res)
