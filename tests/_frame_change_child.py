"""Helper process of tests/test_gpu_frame_change.py, started under EVC_DETERMINISTIC=1 (no floating-point atomics on the training path, so
two steps on the same numbers give the same bits): training steps of DistillGraph under --student_sampling change / segment_change against
the uniform step on host-rearranged frames, the teacher next to the uniform graph's, and a SerialStudentsGraph step with both words, its
key launches counted.  Writes what it compared, as a dict of booleans and figures, to <out.pt>.

    python tests/_frame_change_child.py <out.pt>
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import _frame_change_ref as ref  # noqa: E402
import _frame_select_ref as sel_ref  # noqa: E402
from oracle import model_math as mm  # noqa: E402
from efficientvideoclassification_youtube8m_amd import ops  # noqa: E402
from efficientvideoclassification_youtube8m_amd.distill import DistillGraph, SerialStudentsGraph  # noqa: E402

out_path = sys.argv[1]
DEV = "cuda:0"
B, EVERY_N = 6, 10
SIZES = dict(feature_size=128, vocab_size=50, lstm_cells=64, device=DEV)          # the sizes of tests/_frame_select_child.py
KW = dict(every_n=EVERY_N, **SIZES)
q, x, n, labels = mm.synthetic_batch(B, seed=3, feature_size=128, vocab_size=50, dtype=np.float32)
n[0], n[1] = 300, 79
x[np.arange(300)[None, :] >= n[:, None]] = 0.0
xd, yd, nd = torch.from_numpy(x).to(DEV), torch.from_numpy(labels.astype(np.uint8)).to(DEV), torch.from_numpy(n).to(DEV)
res = {"deterministic": os.environ.get("EVC_DETERMINISTIC")}
# general f32 frames: the contract leaves near-ties among f32 scores to the device's summation order, so the expected tables are the
# reference's ranking of the keys the device computed (those keys are held to the reference in the key tests)
keys = ops.frame_change_keys(xd, nd).cpu().numpy().view(np.uint32)
res["keys_repeat"] = bool((ops.frame_change_keys(xd, nd).cpu().numpy().view(np.uint32) == keys).all())

calls = []
inner = ops.frame_change_keys


def counted(*a, **k):
    calls.append(1)
    return inner(*a, **k)


ops.frame_change_keys = counted


def weights(tower):
    return {k: v.clone() for k, v in tower.state_dict().items()}


def same(a, b):
    return sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)


# ---- student only: the step under each word on x against the uniform step on the rearranged x' ----------------------------------------
o_x = DistillGraph(B, mode="student", seed=3, **KW).step(xd, yd, nd, num_frames_host=n)          # uniform on x itself: something else
for word in ref.STRATEGIES:
    src = ref.table(keys, n, 300, EVERY_N, word)
    xp = torch.from_numpy(sel_ref.rearrange(x, src, EVERY_N)).to(DEV)
    g_w, g_p = DistillGraph(B, mode="student", seed=3, student_sampling=word, **KW), DistillGraph(B, mode="student", seed=3, **KW)
    w0 = weights(g_w.student)
    del calls[:]
    o_w = g_w.step(xd, yd, nd, num_frames_host=n)
    res[word + "_key_launches"] = len(calls)
    o_p = g_p.step(xp, yd, nd, num_frames_host=n)
    torch.cuda.synchronize()
    res[word + "_loss"] = (float(o_w["student_label_loss"]), float(o_p["student_label_loss"]))
    res[word + "_loss_equal"] = torch.equal(o_w["student_label_loss"], o_p["student_label_loss"])
    res[word + "_pred_equal"] = torch.equal(o_w["student_predictions"], o_p["student_predictions"])
    res[word + "_weights_equal"] = same(weights(g_w.student), weights(g_p.student))
    res[word + "_moved"] = not same(weights(g_w.student), w0)
    res[word + "_is_not_uniform"] = not torch.equal(o_w["student_predictions"], o_x["student_predictions"])
    res[word + "_table"] = bool((g_w.last_frame_table.cpu().numpy() == src).all())
    del g_w, g_p

# ---- teacher + student: the teacher under `change` is the teacher of the uniform graph -------------------------------------------------
g_u, g_c = DistillGraph(B, seed=3, **KW), DistillGraph(B, seed=3, student_sampling="change", **KW)
res["same_start"] = same(weights(g_u.teacher), weights(g_c.teacher)) and same(weights(g_u.student), weights(g_c.student))
o_u = g_u.step(xd, yd, nd, num_frames_host=n)
o_c = g_c.step(xd, yd, nd, num_frames_host=n)
torch.cuda.synchronize()
res["teacher_loss"] = (float(o_u["loss"]), float(o_c["loss"]))
res["teacher_loss_equal"] = torch.equal(o_u["loss"], o_c["loss"])
res["teacher_pred_equal"] = torch.equal(o_u["predictions"], o_c["predictions"]) and torch.equal(o_u["teacher_state"], o_c["teacher_state"])
res["teacher_weights_equal"] = same(weights(g_u.teacher), weights(g_c.teacher))
res["student_differs"] = not torch.equal(o_u["student_predictions"], o_c["student_predictions"])
res["teacher_student_table"] = bool((g_c.last_frame_table.cpu().numpy() == ref.table(keys, n, 300, EVERY_N, "change")).all())
del g_u, g_c

# ---- serial students: two students on the two words (and a third on `last`, which needs no keys): ONE key launch per batch -------------
g_s = SerialStudentsGraph(B, every_n=(10, 30, 30), student_sampling=("change", "segment_change", "last"), seed=5, **SIZES)
counts = []
for _ in range(2):
    del calls[:]
    g_s.step(xd, yd, nd, num_frames_host=n)
    counts.append(len(calls))
torch.cuda.synchronize()
res["serial_key_launches"] = counts
tabs = [t.cpu().numpy() for t in g_s.last_frame_tables]
res["serial_tables"] = bool((tabs[0] == ref.table(keys, n, 300, 10, "change")).all()
                            and (tabs[1] == ref.table(keys, n, 300, 30, "segment_change")).all()
                            and (tabs[2] == sel_ref.table(n, 300, 30, "last")).all())
del calls[:]
SerialStudentsGraph(B, every_n=(10, 30), student_sampling=("uniform", "last"), seed=5, **SIZES).step(xd, yd, nd, num_frames_host=n)
res["serial_unscored_key_launches"] = len(calls)
torch.cuda.synchronize()
torch.save(res, out_path)
print(res)
