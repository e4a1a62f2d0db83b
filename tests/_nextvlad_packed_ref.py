"""Float64 numpy restatement of the NeXtVLAD tower over a RAGGED, packed list of frames per video: the math of
DESIGN.md 7.12 / tests/_nextvlad_ref.py with video b contributing the frames j * every_n, j < k_b = ceil(min(n_b, T) / every_n), as
the rows row_off[b] .. row_off[b+1] of every per-frame matrix; cluster_bn runs over the R = sum_b k_b real rows, the per-video
sums over each video's own rows (none for k_b = 0).  Hand-written reverse mode.  Parameters as in _nextvlad_ref."""
import numpy as np

import _nextvlad_ref as nx          # noqa: F401  (init_params / BN_NAMES are shared with the fixed-length restatement)
from oracle import model_math as mm

init_params = nx.init_params
BN_NAMES = nx.BN_NAMES


def grid_frames(n, every_n, max_frames):
    """Per video the frame indices 0, every_n, 2 every_n, ... below min(n_b, max_frames), written out the slow way."""
    return [np.array([t for t in range(0, max(0, min(int(nb), max_frames)), every_n)], np.int64) for nb in np.asarray(n).reshape(-1)]


def nextvlad_packed_fwd(xn, n, every_n, P, num_mixtures=2, frames=None):
    """xn [B,T,F] (already l2-normalised where the caller normalises), n [B] frame counts.  frames: the per-video index lists
    (default grid_frames(n, every_n, T))."""
    B, T, F = xn.shape
    frames = grid_frames(n, every_n, T) if frames is None else frames
    k = np.array([len(f) for f in frames], np.int64)
    row_off = np.concatenate([[0], np.cumsum(k)])
    R = int(row_off[-1])
    vid = np.repeat(np.arange(B), k)                                                         # video of every row
    r = np.concatenate([xn[b, frames[b], :] for b in range(B)], axis=0).reshape(R, F)
    G = P["attention_weights"].shape[1]
    D, K = P["cluster_weights2"].shape
    xe = r @ P["expansion_weights"] + P["expansion_biases"]                                  # [R, E]
    att = mm.sigmoid(xe @ P["attention_weights"] + P["attention_biases"])                    # [R, G]
    act = xe @ P["cluster_weights"]                                                          # [R, G*K]
    z, c_cl = mm.batch_norm_train_fwd(act, P["cluster_bn/gamma"], P["cluster_bn/beta"])      # statistics over the R real rows
    z3 = z.reshape(R, G, K)
    e = np.exp(z3 - z3.max(axis=2, keepdims=True))
    p = e / e.sum(axis=2, keepdims=True)
    a = p * att[:, :, None]                                                                  # [R, G, K]
    x3 = xe.reshape(R, G, D)
    C2 = P["cluster_weights2"]                                                               # [D, K]
    asum = np.zeros((B, K))
    V = np.zeros((B, K, D))
    for b in range(B):
        lo, hi = row_off[b], row_off[b + 1]
        asum[b] = a[lo:hi].sum(axis=(0, 1))
        V[b] = np.einsum("rgk,rgd->kd", a[lo:hi], x3[lo:hi]) - asum[b][:, None] * C2.T
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
    cache = dict(frames=frames, k=k, row_off=row_off, vid=vid, r=r, xe=xe, att=att, p=p, a=a, x3=x3, asum=asum, V=V, nrm=nrm, U=U, Y=Y,
                 h=h, g1bn=g1bn, g1=g1, gate=gate, out=out, c_cl=c_cl, c_v=c_v, c_h=c_h, c_g=c_g, c_moe=c_moe, dims=(B, R, G, K, D), P=P)
    return pred, cache


def aggregate_bwd(dV, cache):
    """da [R,G,K] and the aggregation's share of dxe [R,G,D] from dV [B,K,D]: each row takes its own video's dV."""
    C2 = cache["P"]["cluster_weights2"]
    dVr = dV[cache["vid"]]                                                                   # [R, K, D]
    qv = np.einsum("bkd,dk->bk", dV, C2)[cache["vid"]]                                       # [R, K]
    da = np.einsum("rkd,rgd->rgk", dVr, cache["x3"]) - qv[:, None, :]
    dx3 = np.einsum("rgk,rkd->rgd", cache["a"], dVr)
    return da, dx3


def nextvlad_packed_bwd(dpred, cache):
    c, P = cache, cache["P"]
    B, R, G, K, D = c["dims"]
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
    g["cluster_weights2"] = -np.einsum("bk,bkd->dk", c["asum"], dV)
    da, dx3 = aggregate_bwd(dV, c)
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
    c["dV"], c["da"], c["dx3"], c["dxe"] = dV, da, dx3, dxe
    return g
