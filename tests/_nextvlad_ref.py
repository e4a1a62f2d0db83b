"""Float64 numpy restatement of the NeXtVLAD tower (an extension - the reference's NeXtVLADModel is an empty
stub, so there is no reference math) with a hand-written reverse mode.  The MoE head, the frame sampling and the batch-norm
primitives are oracle.model_math's.  Parameters are in TF layout under their checkpoint names (no scope prefix):
expansion_weights [F,E], expansion_biases [E], attention_weights [E,G], attention_biases [G], cluster_weights [E,G*K],
cluster_bn/*, cluster_weights2 [D,K], vlad_bn/* [D*K] (index d*K+k), hidden1_weights [D*K,H] (row d*K+k), hidden1_bn/*,
gating_weights_1 [H,Hg], gating_bn/*, gating_weights_2 [Hg,H] and the MoE names.  Training-mode batch-norm throughout."""
import math

import numpy as np

from oracle import model_math as mm

BN_NAMES = ("cluster_bn", "vlad_bn", "hidden1_bn", "gating_bn")


def init_params(rng, F, expansion, G, K, H, reduction, V, num_mixtures=2, dtype=np.float64):
    E = expansion * F
    D, Hg = E // G, H // reduction
    n = lambda shape, fan: (rng.standard_normal(shape) / math.sqrt(fan)).astype(dtype)
    P = {
        "expansion_weights": n((F, E), F), "expansion_biases": (0.1 * rng.standard_normal(E)).astype(dtype),
        "attention_weights": n((E, G), E), "attention_biases": (0.1 * rng.standard_normal(G)).astype(dtype),
        "cluster_weights": n((E, G * K), E),
        "cluster_weights2": n((D, K), D),
        "hidden1_weights": n((D * K, H), K),
        "gating_weights_1": n((H, Hg), H), "gating_weights_2": n((Hg, H), Hg),
        "classifier/gates/weights": mm.glorot_uniform(rng, (H, V * (num_mixtures + 1)), dtype),
        "classifier/experts/weights": mm.glorot_uniform(rng, (H, V * num_mixtures), dtype),
        "classifier/experts/biases": np.zeros(V * num_mixtures, dtype),
    }
    for s, c in zip(BN_NAMES, (G * K, D * K, H, Hg)):
        P[s + "/gamma"], P[s + "/beta"] = np.ones(c, dtype), np.zeros(c, dtype)
    return P


def nextvlad_fwd(xn, n, u, P, num_mixtures=2):
    """xn [B,T,F] (already l2-normalised where the caller normalises), n [B] frame counts, u [B,S] the sampling draw."""
    B = xn.shape[0]
    idx = mm.sample_random_frames_index(u, n)
    S = idx.shape[1]
    r = xn[np.arange(B)[:, None], idx, :].reshape(B * S, xn.shape[2])
    G = P["attention_weights"].shape[1]
    D, K = P["cluster_weights2"].shape
    xe = r @ P["expansion_weights"] + P["expansion_biases"]                                  # [R, E]
    att = mm.sigmoid(xe @ P["attention_weights"] + P["attention_biases"])                    # [R, G]
    act = xe @ P["cluster_weights"]                                                          # [R, G*K]
    z, c_cl = mm.batch_norm_train_fwd(act, P["cluster_bn/gamma"], P["cluster_bn/beta"])
    z3 = z.reshape(B * S, G, K)
    e = np.exp(z3 - z3.max(axis=2, keepdims=True))
    p = e / e.sum(axis=2, keepdims=True)
    a = p * att[:, :, None]                                                                  # [R, G, K]
    a4 = a.reshape(B, S, G, K)
    x4 = xe.reshape(B, S, G, D)
    asum = a4.sum(axis=(1, 2))                                                               # [B, K]
    C2 = P["cluster_weights2"]                                                               # [D, K]
    V = np.einsum("bsgk,bsgd->bkd", a4, x4) - asum[:, :, None] * C2.T[None]                  # [B, K, D]
    nrm = np.maximum(np.sqrt((V * V).sum(axis=2)), 1e-12)
    U = V / nrm[:, :, None]
    Uf = U.transpose(0, 2, 1).reshape(B, D * K)                                              # TF order d*K + k
    Y, c_v = mm.batch_norm_train_fwd(Uf, P["vlad_bn/gamma"], P["vlad_bn/beta"])
    hid = Y @ P["hidden1_weights"]
    h, c_h = mm.batch_norm_train_fwd(hid, P["hidden1_bn/gamma"], P["hidden1_bn/beta"])
    g1bn, c_g = mm.batch_norm_train_fwd(h @ P["gating_weights_1"], P["gating_bn/gamma"], P["gating_bn/beta"])
    g1 = mm.relu6(g1bn)
    gate = mm.sigmoid(g1 @ P["gating_weights_2"])
    out = h * gate
    pred, c_moe = mm.moe_fwd(out, P["classifier/gates/weights"], P["classifier/experts/weights"], P["classifier/experts/biases"],
                             num_mixtures)
    cache = dict(idx=idx, r=r, xe=xe, att=att, p=p, a=a, a4=a4, x4=x4, asum=asum, V=V, nrm=nrm, U=U, Y=Y, h=h, g1bn=g1bn, g1=g1,
                 gate=gate, out=out, c_cl=c_cl, c_v=c_v, c_h=c_h, c_g=c_g, c_moe=c_moe, dims=(B, S, G, K, D), P=P)
    return pred, cache


def nextvlad_bwd(dpred, cache):
    c, P = cache, cache["P"]
    B, S, G, K, D = c["dims"]
    g = {}
    dout, g["classifier/gates/weights"], g["classifier/experts/weights"], g["classifier/experts/biases"] = mm.moe_bwd(dpred, c["c_moe"])
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
    dY = dhid @ P["hidden1_weights"].T
    dUf, g["vlad_bn/gamma"], g["vlad_bn/beta"] = mm.batch_norm_train_bwd(dY, c["c_v"])
    dU = dUf.reshape(B, D, K).transpose(0, 2, 1)                                             # [B, K, D]
    U, nrm = c["U"], c["nrm"]
    dV = (dU - U * (U * dU).sum(axis=2, keepdims=True)) / nrm[:, :, None]
    C2 = P["cluster_weights2"]
    g["cluster_weights2"] = -np.einsum("bk,bkd->dk", c["asum"], dV)
    da4 = np.einsum("bkd,bsgd->bsgk", dV, c["x4"]) - np.einsum("bkd,dk->bk", dV, C2)[:, None, None, :]
    dx4 = np.einsum("bsgk,bkd->bsgd", c["a4"], dV)
    da = da4.reshape(B * S, G, K)
    p, att = c["p"], c["att"]
    t = (p * da).sum(axis=2)                                                                 # [R, G]
    dz = p * att[:, :, None] * (da - t[:, :, None])
    datt = t * att * (1 - att)
    dact, g["cluster_bn/gamma"], g["cluster_bn/beta"] = mm.batch_norm_train_bwd(dz.reshape(B * S, G * K), c["c_cl"])
    xe = c["xe"]
    g["cluster_weights"] = xe.T @ dact
    g["attention_weights"] = xe.T @ datt
    g["attention_biases"] = datt.sum(axis=0)
    dxe = dx4.reshape(B * S, G * D) + dact @ P["cluster_weights"].T + datt @ P["attention_weights"].T
    g["expansion_biases"] = dxe.sum(axis=0)
    g["expansion_weights"] = c["r"].T @ dxe
    return g
