"""Reference for the NeXtVLAD dropout: a numpy Philox4x32-10, the mask the kernels must regenerate, and the float64
tower of tests/_nextvlad_ref.py restated with Yd = Y * m / keep in front of the hidden layer and dY masked on the way back.

The mask is defined over the INTERNAL cluster-major index j = k*D + d of row b: element e = b*(K*D) + j is lane e & 3 of quad e >> 2,
w = Philox4x32-10(counter (q_lo, q_hi, step_lo, step_hi), key (seed, rank))[e & 3], and the element is kept iff w < floor(keep * 2^32)
as unsigned 32-bit values.  The float64 tower works in TF order d*K + k, so nextvlad_fwd transposes the mask it is given."""
import numpy as np

import _nextvlad_ref as nx
from oracle import model_math as mm

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF

init_params = nx.init_params
BN_NAMES = nx.BN_NAMES


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two; returns the four output words as uint64 arrays < 2^32.
    Round: (c0, c1, c2, c3) <- (hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1, lo(M0*c0)); the key is bumped by the Weyl
    constants between rounds.  All arithmetic in uint64 (a 32 x 32 product fits)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK32) for c in counter)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & np.uint64(MASK32) for k in key)
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(W0)) & m32, (k1 + np.uint64(W1)) & m32
    return c0, c1, c2, c3


def dropout_words(B, C, seed, rank, step):
    """The [B, C] uint64 Philox words (< 2^32) of every element for (seed, rank, step); C % 4 == 0.  Independent of keep."""
    assert C % 4 == 0
    nq = B * C // 4
    q = np.arange(nq, dtype=np.uint64)
    step = int(step)
    w = philox4x32_10((q & np.uint64(MASK32), q >> np.uint64(32), np.full(nq, step & MASK32, np.uint64), np.full(nq, (step >> 32) & MASK32, np.uint64)),
                      (np.full(nq, int(seed) & MASK32, np.uint64), np.full(nq, int(rank) & MASK32, np.uint64)))
    return np.stack(w, axis=1).reshape(B, C)


def threshold(keep):
    """T = floor(keep * 2^32) from the Python float, as the host computes it."""
    return int(np.floor(float(keep) * 4294967296.0))


def dropout_mask(B, K, D, keep, seed, rank, step):
    """The [B, K*D] mask (bool) in internal order k*D + d."""
    return dropout_words(B, K * D, seed, rank, step) < np.uint64(threshold(keep))


def nextvlad_fwd(xn, n, u, P, mask=None, keep=1.0, num_mixtures=2):
    """_nextvlad_ref.nextvlad_fwd with Yd = Y * m / keep between vlad_bn and the hidden layer.  mask: [B, K*D] in INTERNAL order
    (dropout_mask), or None for no dropout.  cache["Y"] is the dropped operand Yd (TF order), cache["Ybn"] the batch-norm output."""
    B = xn.shape[0]
    idx = mm.sample_random_frames_index(u, n)
    S = idx.shape[1]
    r = xn[np.arange(B)[:, None], idx, :].reshape(B * S, xn.shape[2])
    G = P["attention_weights"].shape[1]
    D, K = P["cluster_weights2"].shape
    xe = r @ P["expansion_weights"] + P["expansion_biases"]
    att = mm.sigmoid(xe @ P["attention_weights"] + P["attention_biases"])
    act = xe @ P["cluster_weights"]
    z, c_cl = mm.batch_norm_train_fwd(act, P["cluster_bn/gamma"], P["cluster_bn/beta"])
    z3 = z.reshape(B * S, G, K)
    e = np.exp(z3 - z3.max(axis=2, keepdims=True))
    p = e / e.sum(axis=2, keepdims=True)
    a = p * att[:, :, None]
    a4 = a.reshape(B, S, G, K)
    x4 = xe.reshape(B, S, G, D)
    asum = a4.sum(axis=(1, 2))
    C2 = P["cluster_weights2"]
    V = np.einsum("bsgk,bsgd->bkd", a4, x4) - asum[:, :, None] * C2.T[None]
    nrm = np.maximum(np.sqrt((V * V).sum(axis=2)), 1e-12)
    U = V / nrm[:, :, None]
    Uf = U.transpose(0, 2, 1).reshape(B, D * K)                                              # TF order d*K + k
    Ybn, c_v = mm.batch_norm_train_fwd(Uf, P["vlad_bn/gamma"], P["vlad_bn/beta"])
    if mask is None:
        mt = np.ones((B, D * K))
        keep = 1.0
    else:
        mt = np.asarray(mask, dtype=np.float64).reshape(B, K, D).transpose(0, 2, 1).reshape(B, D * K)   # internal k*D+d -> TF d*K+k
    Y = Ybn * mt / keep
    hid = Y @ P["hidden1_weights"]
    h, c_h = mm.batch_norm_train_fwd(hid, P["hidden1_bn/gamma"], P["hidden1_bn/beta"])
    g1bn, c_g = mm.batch_norm_train_fwd(h @ P["gating_weights_1"], P["gating_bn/gamma"], P["gating_bn/beta"])
    g1 = mm.relu6(g1bn)
    gate = mm.sigmoid(g1 @ P["gating_weights_2"])
    out = h * gate
    pred, c_moe = mm.moe_fwd(out, P["classifier/gates/weights"], P["classifier/experts/weights"], P["classifier/experts/biases"],
                             num_mixtures)
    cache = dict(idx=idx, r=r, xe=xe, att=att, p=p, a=a, a4=a4, x4=x4, asum=asum, V=V, nrm=nrm, U=U, Y=Y, Ybn=Ybn, mt=mt, keep=keep, h=h,
                 g1bn=g1bn, g1=g1, gate=gate, out=out, c_cl=c_cl, c_v=c_v, c_h=c_h, c_g=c_g, c_moe=c_moe, dims=(B, S, G, K, D), P=P)
    return pred, cache


def nextvlad_bwd(dpred, cache):
    """_nextvlad_ref.nextvlad_bwd with dY = dYd * m / keep; dWh contracts the dropped operand (cache["Y"])."""
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
    dY = (dhid @ P["hidden1_weights"].T) * c["mt"] / c["keep"]
    dUf, g["vlad_bn/gamma"], g["vlad_bn/beta"] = mm.batch_norm_train_bwd(dY, c["c_v"])
    dU = dUf.reshape(B, D, K).transpose(0, 2, 1)
    U, nrm = c["U"], c["nrm"]
    dV = (dU - U * (U * dU).sum(axis=2, keepdims=True)) / nrm[:, :, None]
    C2 = P["cluster_weights2"]
    g["cluster_weights2"] = -np.einsum("bk,bkd->dk", c["asum"], dV)
    da4 = np.einsum("bkd,bsgd->bsgk", dV, c["x4"]) - np.einsum("bkd,dk->bk", dV, C2)[:, None, None, :]
    dx4 = np.einsum("bsgk,bkd->bsgd", c["a4"], dV)
    da = da4.reshape(B * S, G, K)
    p, att = c["p"], c["att"]
    t = (p * da).sum(axis=2)
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
