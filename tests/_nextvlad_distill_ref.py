"""Float64 numpy restatement of serial distillation over the NeXtVLAD towers, on top of tests/_nextvlad_packed_ref.py:
the frozen teacher's EVALUATION forward (the four batch norms on given moving statistics, epsilon 1e-3), the student's reverse mode with
a gradient `dstate` on the gated hidden vector `out` added to the MoE head's, and the three distillation losses with
evc_distill_losses' definitions - oracle.model_math's rep_loss / pred_kl_loss / cross_entropy_loss, the float64 definitions the
H-LSTM serial-distillation tests use.  Parameters as in _nextvlad_ref (TF layouts and names)."""
import numpy as np

import _nextvlad_packed_ref as px
from oracle import model_math as mm

BN_NAMES = px.BN_NAMES
EPS = mm.BN_EPSILON


def batch_moments(cache):
    """The moving statistics under which the evaluation forward IS the training forward of ``cache``: every batch norm's own batch
    mean and (biased) variance, as {"<scope>/moving_mean": ..., "<scope>/moving_variance": ...}."""
    out = {}
    for scope, key in (("cluster_bn", "c_cl"), ("vlad_bn", "c_v"), ("hidden1_bn", "c_h"), ("gating_bn", "c_g")):
        _, _, _, mu, var = cache[key]
        out[scope + "/moving_mean"], out[scope + "/moving_variance"] = mu.copy(), var.copy()
    return out


def _bn_eval(x, P, M, scope):
    return (x - M[scope + "/moving_mean"]) / np.sqrt(M[scope + "/moving_variance"] + EPS) * P[scope + "/gamma"] + P[scope + "/beta"]


def nextvlad_packed_eval_fwd(xn, n, every_n, P, M, num_mixtures=2):
    """The forward of px.nextvlad_packed_fwd with every batch norm on the moving statistics M.  Returns (pred, out, cache of the
    intermediate values a test compares: a, Y, row_off, k)."""
    B, T, F = xn.shape
    frames = px.grid_frames(n, every_n, T)
    k = np.array([len(f) for f in frames], np.int64)
    row_off = np.concatenate([[0], np.cumsum(k)])
    R = int(row_off[-1])
    r = np.concatenate([xn[b, frames[b], :] for b in range(B)], axis=0).reshape(R, F)
    G = P["attention_weights"].shape[1]
    D, K = P["cluster_weights2"].shape
    xe = r @ P["expansion_weights"] + P["expansion_biases"]
    att = mm.sigmoid(xe @ P["attention_weights"] + P["attention_biases"])
    z3 = _bn_eval(xe @ P["cluster_weights"], P, M, "cluster_bn").reshape(R, G, K)
    e = np.exp(z3 - z3.max(axis=2, keepdims=True))
    a = e / e.sum(axis=2, keepdims=True) * att[:, :, None]
    x3 = xe.reshape(R, G, D)
    V = np.zeros((B, K, D))
    for b in range(B):
        lo, hi = row_off[b], row_off[b + 1]
        V[b] = np.einsum("rgk,rgd->kd", a[lo:hi], x3[lo:hi]) - a[lo:hi].sum(axis=(0, 1))[:, None] * P["cluster_weights2"].T
    U = V / np.maximum(np.sqrt((V * V).sum(axis=2)), 1e-12)[:, :, None]
    Y = _bn_eval(U.transpose(0, 2, 1).reshape(B, D * K), P, M, "vlad_bn")                    # TF order d*K + k
    h = _bn_eval(Y @ P["hidden1_weights"], P, M, "hidden1_bn")
    g1 = mm.relu6(_bn_eval(h @ P["gating_weights_1"], P, M, "gating_bn"))
    out = h * mm.sigmoid(g1 @ P["gating_weights_2"])
    pred, _ = mm.moe_fwd(out, P["classifier/gates/weights"], P["classifier/experts/weights"], P["classifier/experts/biases"], num_mixtures)
    return pred, out, dict(a=a, Y=Y, V=V, row_off=row_off, k=k, r=r)


def nextvlad_packed_bwd(dpred, cache, dstate=None):
    """The reverse mode of px.nextvlad_packed_bwd with d(out) = the MoE head's gradient + dstate (None: the head's alone, and then that
    function itself).  Written out once more, not patched in: the two must agree for dstate = 0 (test_cpu_nextvlad_distill.py)."""
    if dstate is None:
        return px.nextvlad_packed_bwd(dpred, cache)
    c, P = cache, cache["P"]
    B, R, G, K, D = c["dims"]
    g = {}
    dout, g["classifier/gates/weights"], g["classifier/experts/weights"], g["classifier/experts/biases"] = mm.moe_bwd(dpred, c["c_moe"])
    dout = dout + dstate                                                                     # L_REP's gradient joins the head's here
    h, gate, g1, g1bn = c["h"], c["gate"], c["g1"], c["g1bn"]
    dh = dout * gate
    dgl = dout * h * gate * (1 - gate)
    g["gating_weights_2"] = g1.T @ dgl
    dg1bn = (dgl @ P["gating_weights_2"].T) * ((g1bn > 0) & (g1bn < 6))
    dg1pre, g["gating_bn/gamma"], g["gating_bn/beta"] = mm.batch_norm_train_bwd(dg1bn, c["c_g"])
    g["gating_weights_1"] = h.T @ dg1pre
    dh = dh + dg1pre @ P["gating_weights_1"].T
    dhid, g["hidden1_bn/gamma"], g["hidden1_bn/beta"] = mm.batch_norm_train_bwd(dh, c["c_h"])
    g["hidden1_weights"] = c["Y"].T @ dhid
    dUf, g["vlad_bn/gamma"], g["vlad_bn/beta"] = mm.batch_norm_train_bwd(dhid @ P["hidden1_weights"].T, c["c_v"])
    dU = dUf.reshape(B, D, K).transpose(0, 2, 1)                                             # [B, K, D]
    U, nrm = c["U"], c["nrm"]
    dV = (dU - U * (U * dU).sum(axis=2, keepdims=True)) / nrm[:, :, None]
    g["cluster_weights2"] = -np.einsum("bk,bkd->dk", c["asum"], dV)
    da, dx3 = px.aggregate_bwd(dV, c)
    p, att = c["p"], c["att"]
    t = (p * da).sum(axis=2)                                                                 # [R, G]
    dz = p * att[:, :, None] * (da - t[:, :, None])
    datt = t * att * (1 - att)
    dact, g["cluster_bn/gamma"], g["cluster_bn/beta"] = mm.batch_norm_train_bwd(dz.reshape(R, G * K), c["c_cl"])
    xe = c["xe"]
    g["cluster_weights"] = xe.T @ dact
    g["attention_weights"] = xe.T @ datt
    g["attention_biases"] = datt.sum(axis=0)
    dxe = dx3.reshape(R, G * D) + dact @ P["cluster_weights"].T + datt @ P["attention_weights"].T
    g["expansion_biases"] = dxe.sum(axis=0)
    g["expansion_weights"] = c["r"].T @ dxe
    return g


def distill_losses(t_pred, t_state, s_pred, s_state, y, rep_w=2.0, on=("rep", "pred", "ce")):
    """The four reported values (DistillGraph.LOSS_SLOTS order: teacher CE, L_REP, L_PRED, student CE), the total the student is
    trained on - rep_w L_REP + L_PRED + L_CE over the words of ``on`` - and its gradients (dpred_s, dstate_s)."""
    vals = dict(label_loss=mm.cross_entropy_loss(t_pred, y), student_loss_state=mm.rep_loss(t_state, s_state),
                pred_loss=mm.pred_kl_loss(t_pred, s_pred), student_label_loss=mm.cross_entropy_loss(s_pred, y))
    g_rep, g_kl, g_ce = (rep_w if "rep" in on else 0.0), (1.0 if "pred" in on else 0.0), (1.0 if "ce" in on else 0.0)
    total = g_rep * vals["student_loss_state"] + g_kl * vals["pred_loss"] + g_ce * vals["student_label_loss"]
    dpred = g_kl * mm.pred_kl_grad_student(t_pred, s_pred) + g_ce * mm.cross_entropy_grad(s_pred, y)
    dstate = g_rep * mm.rep_loss_grad_student(t_state, s_state)
    return vals, total, dpred, dstate


def distill_step(xn, n, y, teacher, teacher_moving, student, teacher_every_n, every_n, rep_w=2.0, on=("rep", "pred", "ce"), with_grads=True):
    """One step's math up to (not including) the update: the frozen teacher's evaluation forward on every teacher_every_n-th real
    frame, the student's training forward on every every_n-th, the losses, the student's gradients."""
    t_pred, t_state, t_cache = nextvlad_packed_eval_fwd(xn, n, teacher_every_n, teacher, teacher_moving)
    s_pred, s_cache = px.nextvlad_packed_fwd(xn, n, every_n, student)
    vals, total, dpred, dstate = distill_losses(t_pred, t_state, s_pred, s_cache["out"], y, rep_w, on)
    out = dict(vals, total=total, teacher_predictions=t_pred, teacher_state=t_state, student_predictions=s_pred,
               student_state=s_cache["out"], dpred=dpred, dstate=dstate, teacher_cache=t_cache, student_cache=s_cache)
    if with_grads:
        out["student_grads"] = nextvlad_packed_bwd(dpred, s_cache, dstate)
    return out
