"""Offline distillation as a graph: OfflineDistillGraph - the mode "student" step with ops.distill_losses_sparse as its loss section -
against DistillGraph(mode="serial") on the same student and the serial graph's own teacher rows handed over as full lists (k = V, the
f32 values themselves, so the scattered row holds the teacher's bits).  pytest -m gpu.

vocab_size = 200: a full row fits the 256 entries of a list.  Bounds: pred_loss and student_label_loss 1e-4 relative between the two
graphs; the student's dpred within twice the kernel bound of test_gpu_distill_sparse.py, 2 * 1e-5 (|ce term| + |kl term|), the terms in
float64 from tests/_distill_losses_ref.py on the rows the step returned.  Everything else is bit for bit."""
import numpy as np
import pytest
import torch

import _distill_losses_ref as lref
from oracle import model_math as mm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, F, H, V, EVERY_N = 5, 64, 64, 200, 30
KW = dict(feature_size=F, vocab_size=V, lstm_cells=H, device=DEV)
RTOL_LOSS, RTOL_GRAD = 1e-4, 1e-5
_SHARED = {}


def _shared():
    """The batch and a teacher that has made six training steps at a learning rate of 0.02, so that its rows stand well away from the
    untrained student's: evc_distill_losses, the serial graph's loss section, evaluates L_PRED in f32 throughout and is 3e-4 off float64
    where student and teacher nearly coincide and the sum cancels to 3e-4 (test_gpu_distill_ensemble_graph.py); the 1e-4 between the two
    graphs is asked of a teacher whose L_PRED does not cancel."""
    if not _SHARED:
        from efficientvideoclassification_youtube8m_amd.distill import DistillGraph
        q, x, n, labels = mm.synthetic_batch(B, seed=21, feature_size=F, vocab_size=V, dtype=np.float32)
        dev = (torch.from_numpy(x).to(DEV), torch.from_numpy(labels.astype(np.uint8)).to(DEV), torch.from_numpy(n).to(DEV))
        t = DistillGraph(B, mode="teacher", seed=5, every_n=EVERY_N, base_learning_rate=0.02, **KW)
        for _ in range(6):
            t.step(*dev, num_frames_host=n)
        sd = {k: v.clone() for k, v in t.teacher.state_dict().items()}
        torch.cuda.synchronize()
        _SHARED.update(n=n, labels=labels, dev=dev, teacher_sd=sd)
    return _SHARED


def _full_lists(t_pred):
    """A [B, V] prediction matrix as ONE file's lists with k = V: every class in order, the f32 values themselves."""
    idx = torch.arange(V, dtype=torch.int32, device=DEV).repeat(t_pred.shape[0], 1).unsqueeze(0).contiguous()
    return idx, t_pred.clone().unsqueeze(0).contiguous()


def test_the_step_against_the_serial_graph_on_the_same_teacher_rows():
    from efficientvideoclassification_youtube8m_amd.distill import DistillGraph, OfflineDistillGraph
    sh = _shared()
    a = DistillGraph(B, mode="serial", seed=5, every_n=EVERY_N, distill_losses=("pred", "ce"), **KW)
    a.teacher.load_state_dict(sh["teacher_sd"])
    out_a = a.step(*sh["dev"], apply=False, num_frames_host=sh["n"])
    dp_a = a.label_grads()["student"].clone()
    g = OfflineDistillGraph(B, every_n=EVERY_N, seed=5, teacher_mode="mean", teacher_weights=[1.0], **KW)
    assert g.teacher is None and g.mode == "student" and g.offline_losses == ("pred", "ce")
    assert not any(k.startswith("model/") for k in g.state_dict()) and all(k.startswith("model_student/") for k in g.state_dict())
    out_b = g.step(*sh["dev"], apply=False, num_frames_host=sh["n"], teacher_lists=_full_lists(out_a["predictions"]))
    dp_b = g.label_grads()["student"].clone()
    torch.cuda.synchronize()
    assert g.global_step == 0 and "predictions" not in out_b
    assert torch.equal(out_a["student_predictions"], out_b["student_predictions"])         # the same student, the same forward
    ra, rb = a.loss_report(), g.loss_report()
    missed = []
    for k in ("pred_loss", "student_label_loss"):
        print("%s: serial %.9g, offline %.9g" % (k, ra[k], rb[k]))
        if not abs(ra[k] - rb[k]) <= RTOL_LOSS * abs(ra[k]):
            missed.append((k, ra[k], rb[k]))
    assert rb["pred_loss"] > 0 and rb["student_loss_state"] == 0.0
    inp = dict(pred_t=out_a["predictions"].cpu().numpy(), pred_s=out_a["student_predictions"].cpu().numpy(),
               labels=sh["labels"].astype(np.uint8), state_t=np.zeros((B, 1), np.float32), state_s=np.zeros((B, 1), np.float32))
    want = lref.reference(inp, 1.0 / B, 1.0, 0.0)
    print("pred_loss in float64 on the same rows: %.9g" % want["losses"][2])
    bound = 2 * RTOL_GRAD * (np.abs(want["ce"]) + np.abs(want["kl"]))
    err = np.abs(dp_a.double().cpu().numpy() - dp_b.double().cpu().numpy())
    print("dpred serial - offline: worst %.3g of its bound, %d of %d elements over it" % (float((err / bound).max()), int((~(err <= bound)).sum()), err.size))
    assert not missed, missed
    assert (err <= bound).all()
    # and against float64 directly, under the kernel bound itself
    err64 = np.abs(dp_b.double().cpu().numpy() - (want["ce"] + want["kl"]))
    assert (err64 <= bound / 2).all(), float((err64 / bound).max())


@pytest.mark.parametrize("on", [("pred",), ("ce",)])
def test_a_loss_left_out_is_reported_and_not_trained_on(on):
    from efficientvideoclassification_youtube8m_amd.distill import OfflineDistillGraph
    sh = _shared()
    rng = np.random.default_rng(3)
    t_pred = torch.from_numpy(rng.uniform(0.01, 0.99, (B, V)).astype(np.float32)).to(DEV)
    both = OfflineDistillGraph(B, every_n=EVERY_N, seed=5, teacher_weights=[1.0], **KW)
    one = OfflineDistillGraph(B, every_n=EVERY_N, seed=5, teacher_weights=[1.0], distill_losses=on, **KW)
    both.step(*sh["dev"], apply=False, num_frames_host=sh["n"], teacher_lists=_full_lists(t_pred))
    one.step(*sh["dev"], apply=False, num_frames_host=sh["n"], teacher_lists=_full_lists(t_pred))
    torch.cuda.synchronize()
    assert both.loss_report() == one.loss_report()
    assert not torch.equal(both.label_grads()["student"], one.label_grads()["student"])
    with pytest.raises(ValueError, match="no state"):
        OfflineDistillGraph(B, every_n=EVERY_N, distill_losses=("rep", "pred"), **KW)
    with pytest.raises(ValueError, match="teacher_weights"):
        both.step(*sh["dev"], apply=False, num_frames_host=sh["n"], teacher_lists=tuple(t.repeat(2, 1, 1) for t in _full_lists(t_pred)))


def test_without_lists_the_step_is_the_student_only_step_bit_for_bit():
    """DistillGraph(mode="student") and OfflineDistillGraph stepping with teacher_lists=None, twice each with the update applied: the same
    predictions, losses, dpred and weights; then one step WITH lists moves the weights elsewhere and counts one global step."""
    from efficientvideoclassification_youtube8m_amd.distill import DistillGraph, OfflineDistillGraph
    sh = _shared()
    s = DistillGraph(B, mode="student", seed=5, every_n=EVERY_N, **KW)
    g = OfflineDistillGraph(B, every_n=EVERY_N, seed=5, **KW)
    for it in range(2):
        out_s = s.step(*sh["dev"], num_frames_host=sh["n"])
        out_g = g.step(*sh["dev"], num_frames_host=sh["n"])
        assert torch.equal(out_s["student_predictions"], out_g["student_predictions"]), it
        assert torch.equal(s.losses, g.losses) and torch.equal(s.label_grads()["student"], g.label_grads()["student"]), it
    s.flush()
    sd_s, sd_g = s.student.state_dict(), g.state_dict()
    assert s.global_step == g.global_step == 2 and sd_s.keys() == sd_g.keys()
    for k in sd_s:
        assert torch.equal(sd_s[k], sd_g[k]), k
    t_pred = torch.full((B, V), 0.25, dtype=torch.float32, device=DEV)
    out = g.step(*sh["dev"], num_frames_host=sh["n"], teacher_lists=_full_lists(t_pred))
    assert g.global_step == 3 and out["global_step"] == 3 and float(out["pred_loss"]) > 0
    assert any(not torch.equal(v, sd_g[k]) for k, v in g.state_dict().items())
