"""Float64 numpy restatement of the NetVLAD tower with the context gate (--netvlad_gating), on top of
tests/_netvlad_packed_ref.py / _netvlad_distill_ref.py.  With h6 = relu6(hidden1_bn(hid)):

    gl = h6 . gating_weights     gn = gating_bn(gl)     g = sigmoid(gn)     state = h6 * g     (what the MoE head and L_REP read)

and in reverse mode, with e = the head's gradient on state (+ dstate): dh6 = e * g + dgl . gating_weights^T, dgn = e * h6 * g * (1 - g).
A parameter dict without "gating_weights" is the ungated tower and goes through the older functions themselves.  The device rounds h6
to bf16 in front of the product; float64 does not.  Parameters in TF layouts and names.

Also an f32 evaluation of the three device entries' expressions (gate_f32), and three planted faults for the reverse mode."""
import numpy as np

import _netvlad_distill_ref as dx
import _netvlad_packed_ref as px
from _nextvlad_distill_ref import distill_losses
from oracle import model_math as mm

GW, GBN = "gating_weights", "gating_bn"
GATE_NAMES = (GW, GBN + "/beta", GBN + "/gamma")
FAULTS = ("no_one_minus_g", "dstate_after_gate", "no_via")


def gated(P):
    return GW in P


def add_gate_params(P, rng, H):
    """The five new variables' trainable three, as the tower initialises them: randn / sqrt(H), gamma 1, beta 0."""
    P[GW] = rng.standard_normal((H, H)) / np.sqrt(H)
    P[GBN + "/beta"], P[GBN + "/gamma"] = np.zeros(H), np.ones(H)
    return P


def moving_stats(M):
    out = dx.moving_stats(M)
    if GBN + "/moving_mean" in M:
        out[GBN] = (M[GBN + "/moving_mean"], M[GBN + "/moving_variance"])
    return out


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def fwd(xn, n, every_n, P, num_mixtures=2, frames=None, stats=None):
    """(pred, cache); cache["state"] is the tower's representation (h6 without a gate)."""
    pred, c = px.netvlad_packed_fwd(xn, n, every_n, P, num_mixtures=num_mixtures, frames=frames, stats=stats)
    if not gated(P):
        c["state"] = c["h6"]
        return pred, c
    h6 = c["h6"]
    gl = h6 @ P[GW]
    gn, c_g = px._bn(gl, P[GBN + "/gamma"], P[GBN + "/beta"], None if stats is None else stats[GBN])
    g = sigmoid(gn)
    state = h6 * g
    pred, c_moe = mm.moe_fwd(state, P["classifier/gates/weights"], P["classifier/experts/weights"], P["classifier/experts/biases"], num_mixtures)
    c.update(gl=gl, gn=gn, g=g, c_g=c_g, state=state, c_moe=c_moe)
    return pred, c


def eval_fwd(xn, n, every_n, P, M, num_mixtures=2):
    pred, c = fwd(xn, n, every_n, P, num_mixtures=num_mixtures, stats=moving_stats(M))
    return pred, c["state"], c


def bwd(dpred, cache, dstate=None, fault=None):
    """Every trainable variable's gradient.  fault: one of FAULTS, a wrong reverse mode on purpose."""
    c, P = cache, cache["P"]
    if not gated(P):
        assert fault is None
        return dx.netvlad_packed_bwd(dpred, cache, dstate)
    B, R, F, K = c["dims"]
    out = {}
    e, out["classifier/gates/weights"], out["classifier/experts/weights"], out["classifier/experts/biases"] = mm.moe_bwd(dpred, c["c_moe"])
    if dstate is not None and fault != "dstate_after_gate":
        e = e + dstate
    h6, g = c["h6"], c["g"]
    dgn = e * h6 * g if fault == "no_one_minus_g" else e * h6 * g * (1.0 - g)
    dgl, out[GBN + "/gamma"], out[GBN + "/beta"] = mm.batch_norm_train_bwd(dgn, c["c_g"])
    out[GW] = h6.T @ dgl
    dh6 = e * g
    if fault != "no_via":
        dh6 = dh6 + dgl @ P[GW].T
    if dstate is not None and fault == "dstate_after_gate":
        dh6 = dh6 + dstate
    dhid_bn = dh6 * ((c["hid_bn"] > 0) & (c["hid_bn"] < 6))
    dhid, out["hidden1_bn/gamma"], out["hidden1_bn/beta"] = mm.batch_norm_train_bwd(dhid_bn, c["c_h"])
    Y, n2, Uc, n1 = c["Y"], c["n2"], c["U"], c["n1"]
    out["hidden1_weights"] = Y.T @ dhid
    dY = dhid @ P["hidden1_weights"].T
    dUf = (dY - Y * (Y * dY).sum(axis=1, keepdims=True)) / n2[:, None]
    dU = dUf.reshape(B, F, K).transpose(0, 2, 1)
    dV = (dU - Uc * (Uc * dU).sum(axis=2, keepdims=True)) / n1[:, :, None]
    out["cluster_weights2"] = -np.einsum("bk,bkf->fk", c["asum"], dV)
    da, dX = px.aggregate_bwd(dV, c)
    a = c["a"]
    dz = a * (da - (a * da).sum(axis=1, keepdims=True))
    dact, out["cluster_bn/gamma"], out["cluster_bn/beta"] = mm.batch_norm_train_bwd(dz, c["c_cl"])
    out["cluster_weights"] = c["r_bn"].T @ dact
    dr_bn = dact @ P["cluster_weights"].T + dX
    _, out["input_bn/gamma"], out["input_bn/beta"] = mm.batch_norm_train_bwd(dr_bn, c["c_in"])
    return out


def distill_step(xn, n, y, teacher, teacher_moving, student, teacher_every_n, every_n, rep_w=2.0, on=("rep", "pred", "ce"), with_grads=True,
                 fault=None):
    """dx.distill_step with either tower gated or not; the states are `state` as defined above."""
    t_pred, t_state, t_cache = eval_fwd(xn, n, teacher_every_n, teacher, teacher_moving)
    s_pred, s_cache = fwd(xn, n, every_n, student)
    vals, total, dpred, dstate = distill_losses(t_pred, t_state, s_pred, s_cache["state"], y, rep_w, on)
    out = dict(vals, total=total, teacher_predictions=t_pred, teacher_state=t_state, student_predictions=s_pred,
               student_state=s_cache["state"], dpred=dpred, dstate=dstate, teacher_cache=t_cache, student_cache=s_cache)
    if with_grads:
        out["student_grads"] = bwd(dpred, s_cache, dstate, fault=fault)
    return out


# ---------------------------------------------------------------------------- the device entries' expressions in f32
def gate_f32(gl, h, d, d2, mean, var, gamma, beta, R_total=None, fused=True):
    """out, dh, dgl, dgamma, dbeta as evc_bn_gate_fwd / _bwd_partial / _bwd_finalize form them, one f32 rounding per operation (exp and
    the reciprocals through float64, rounded once; the column sums in float64 as the kernels keep them).  fused=False rounds where the
    chain of older entries stores an f32 - the same places, which is the point: the two must agree bit for bit."""
    f = np.float32
    gl, h, d = gl.astype(f), h.astype(f), d.astype(f)
    R = gl.shape[0]
    R_total = R if R_total is None else R_total
    inv = (1.0 / np.sqrt((var.astype(f) + f(1e-3)).astype(np.float64))).astype(f)
    xh = ((gl - mean.astype(f)).astype(f) * inv).astype(f)
    gn = (xh.astype(np.float64) * gamma.astype(f) + beta.astype(f)).astype(f)          # one fma
    g = (1.0 / (f(1) + np.exp(-gn.astype(np.float64)).astype(f)).astype(f).astype(np.float64)).astype(f)
    out = (h * g).astype(f)
    e = d if d2 is None else (d + d2.astype(f)).astype(f)
    dh = (e * g).astype(f)
    dy = ((((e * h).astype(f) * g).astype(f)) * (f(1) - g).astype(f)).astype(f)
    s = dy.astype(np.float64).sum(axis=0)
    q = (dy.astype(np.float64) * xh.astype(np.float64)).sum(axis=0)
    sd, sdx = s.astype(f), q.astype(f)
    t = ((dy - (sd / f(R_total)).astype(f)).astype(f) - ((xh * sdx).astype(f) / f(R_total)).astype(f)).astype(f)
    dgl = ((gamma.astype(f) * inv).astype(f) * t).astype(f)
    return dict(out=out, dh=dh, dgl=dgl, dgamma=sdx, dbeta=sd, g=g, xh=xh)
