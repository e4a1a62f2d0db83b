"""Float64 numpy restatement of serial distillation over the NetVLAD towers, on top of tests/_netvlad_packed_ref.py:
the frozen teacher's EVALUATION forward (netvlad_packed_fwd(stats=...): the three batch norms on given moving statistics, epsilon
1e-3), the student's reverse mode with a gradient `dstate` on h6 = relu6(hidden1_bn(hid)) added to the MoE head's in front of the
relu6 mask, and the three distillation losses with evc_distill_losses' definitions (tests/_nextvlad_distill_ref.distill_losses: the
oracle's rep_loss / pred_kl_loss / cross_entropy_loss, shared by the families).  Parameters in TF layouts and names."""
import numpy as np

import _netvlad_packed_ref as px
from _nextvlad_distill_ref import distill_losses  # noqa: F401  (model-independent: predictions, states and labels only)
from oracle import model_math as mm

BN_SCOPES = ("input_bn", "cluster_bn", "hidden1_bn")


def moving_stats(M):
    """{"<scope>/moving_mean", "<scope>/moving_variance"} -> the stats= argument of px.netvlad_packed_fwd."""
    return {s: (M[s + "/moving_mean"], M[s + "/moving_variance"]) for s in BN_SCOPES}


def netvlad_packed_eval_fwd(xn, n, every_n, P, M, num_mixtures=2):
    """The evaluation forward on the moving statistics M.  Returns (pred, h6, cache)."""
    pred, cache = px.netvlad_packed_fwd(xn, n, every_n, P, num_mixtures=num_mixtures, stats=moving_stats(M))
    return pred, cache["h6"], cache


def netvlad_packed_bwd(dpred, cache, dstate=None):
    """The reverse mode of px.netvlad_packed_bwd with d(h6) = the MoE head's gradient + dstate (None: the head's alone, and then that
    function itself).  Written out once more, not patched in: the two must agree for dstate = 0 (test_cpu_netvlad_distill.py)."""
    if dstate is None:
        return px.netvlad_packed_bwd(dpred, cache)
    c, P = cache, cache["P"]
    B, R, F, K = c["dims"]
    g = {}
    dh6, g["classifier/gates/weights"], g["classifier/experts/weights"], g["classifier/experts/biases"] = mm.moe_bwd(dpred, c["c_moe"])
    dh6 = dh6 + dstate                                                # L_REP's gradient joins the head's here, in front of the mask
    dhid_bn = dh6 * ((c["hid_bn"] > 0) & (c["hid_bn"] < 6))
    dhid, g["hidden1_bn/gamma"], g["hidden1_bn/beta"] = mm.batch_norm_train_bwd(dhid_bn, c["c_h"])
    Y, n2, Uc, n1 = c["Y"], c["n2"], c["U"], c["n1"]
    g["hidden1_weights"] = Y.T @ dhid
    dY = dhid @ P["hidden1_weights"].T
    dUf = (dY - Y * (Y * dY).sum(axis=1, keepdims=True)) / n2[:, None]
    dU = dUf.reshape(B, F, K).transpose(0, 2, 1)
    dV = (dU - Uc * (Uc * dU).sum(axis=2, keepdims=True)) / n1[:, :, None]
    g["cluster_weights2"] = -np.einsum("bk,bkf->fk", c["asum"], dV)
    da, dX = px.aggregate_bwd(dV, c)
    a = c["a"]
    dz = a * (da - (a * da).sum(axis=1, keepdims=True))
    dact, g["cluster_bn/gamma"], g["cluster_bn/beta"] = mm.batch_norm_train_bwd(dz, c["c_cl"])
    g["cluster_weights"] = c["r_bn"].T @ dact
    dr_bn = dact @ P["cluster_weights"].T + dX
    _, g["input_bn/gamma"], g["input_bn/beta"] = mm.batch_norm_train_bwd(dr_bn, c["c_in"])
    return g


def distill_step(xn, n, y, teacher, teacher_moving, student, teacher_every_n, every_n, rep_w=2.0, on=("rep", "pred", "ce"), with_grads=True):
    """One step's math up to (not including) the update: the frozen teacher's evaluation forward on every teacher_every_n-th real
    frame, the student's training forward on every every_n-th, the losses, the student's gradients."""
    t_pred, t_state, t_cache = netvlad_packed_eval_fwd(xn, n, teacher_every_n, teacher, teacher_moving)
    s_pred, s_cache = px.netvlad_packed_fwd(xn, n, every_n, student)
    vals, total, dpred, dstate = distill_losses(t_pred, t_state, s_pred, s_cache["h6"], y, rep_w, on)
    out = dict(vals, total=total, teacher_predictions=t_pred, teacher_state=t_state, student_predictions=s_pred,
               student_state=s_cache["h6"], dpred=dpred, dstate=dstate, teacher_cache=t_cache, student_cache=s_cache)
    if with_grads:
        out["student_grads"] = netvlad_packed_bwd(dpred, s_cache, dstate)
    return out


def perturbed_moving(P, rng, sizes):
    """Moving statistics that are not the initial ones, and batch-norm scales / offsets to go with them, as DESIGN.md 7.14 perturbs them:
    0.2 N(0,1) on mean and beta, exp(0.2 N(0,1)) on variance and gamma.  sizes: {scope: C}.  Changes P's gamma / beta in place."""
    M = {}
    for s, C in sizes.items():
        M[s + "/moving_mean"] = 0.2 * rng.standard_normal(C)
        M[s + "/moving_variance"] = np.exp(0.2 * rng.standard_normal(C))
        P[s + "/beta"] = 0.2 * rng.standard_normal(C)
        P[s + "/gamma"] = np.exp(0.2 * rng.standard_normal(C))
    return M
