"""Float64 numpy references for NetVLAD over a RAGGED, packed list of frames per video (--netvlad_frames grid).

1.  The tower: the math of oracle.model_math.netvlad_fwd / _bwd with video b contributing the frames j * every_n, j < L_b =
    ceil(min(n_b, T) / every_n), as the rows row_off[b] .. row_off[b+1] of every per-frame matrix; input_bn and cluster_bn run over the
    R = sum_b L_b real rows, the per-video sums over each video's own rows (none for L_b = 0).  Hand-written reverse mode.  With
    stats=... the forward runs on given moving statistics (the evaluation forward of a training=False tower).

2.  The two packed entries (evc_netvlad_aggregate_packed_fwd / _bwd) per element, each with a bound on |got - ref| DERIVED with the
    pair arithmetic of tests/_vlad_ref.py (a quantity is (value, bound on the kernel's f32 value's distance from it); U = 2^-24):
        xb = add(mul(sub(r, mean), mul(rsq(add(var, C3)), gamma)), beta)               the expression of the kernels, per element
        V    acc = tsum(mul(a, xb), L_b): ONE chain over the video's L_b rows (the MFMA takes (l, l + 1) as k = 0, 1 on the same
             accumulator: still a chain of depth L_b); asum = tsum(a, L_b); V = sub(acc, mul(asum, c2))  -  aggregate_fwd of _vlad_ref
             with the chain length L_b.  An fma has one rounding fewer than mul + add: the bound covers both.  L_b = 0: exactly 0.
        dx   the chain over k = 0 .. K - 1 of exact inputs: (K + 1) U sum_k |a dV|
        da   acc = tsum(mul(dV, xb), F): the chain over f = 0 .. F - 1, xb's own error carried through the products;
             q = sum_f dV c2 by one wave: d_q = (ceil(F / 64) + 7) U sum |dV c2| (its depth and the products); da = sub(acc, q)
    No measured constant enters a bound.  emulate() runs each kernel's chain in numpy float32 (separate roundings), for the CPU test
    that the bounds hold for an honest f32 evaluation and reject planted faults."""
import numpy as np

from _vlad_ref import C3, F32, F64, U, Case, Out, add, ex, f64, mul, rsq, sub, tsum, wave_depth  # noqa: F401
from oracle import model_math as mm


# ---------------------------------------------------------------------------- the tower
def grid_frames(n, every_n, max_frames):
    """Per video the frame indices 0, every_n, 2 every_n, ... below min(n_b, max_frames), written out the slow way."""
    return [np.array([t for t in range(0, max(0, min(int(nb), max_frames)), every_n)], np.int64) for nb in np.asarray(n).reshape(-1)]


def _bn(x, gamma, beta, stats):
    """Training batch-norm over the rows of x, or (stats = (mean, var)) the evaluation form on given statistics: (y, cache or None)."""
    if stats is None:
        return mm.batch_norm_train_fwd(x, gamma, beta)
    mean, var = stats
    return (x - mean) / np.sqrt(var + mm.BN_EPSILON) * gamma + beta, None


def netvlad_packed_fwd(xn, n, every_n, P, num_mixtures=2, frames=None, stats=None):
    """xn [B,T,F] (already l2-normalised where the caller normalises), n [B] frame counts.  frames: the per-video index lists (default
    grid_frames(n, every_n, T)).  stats: None (training statistics over the live rows) or {bn scope: (moving mean, moving variance)}."""
    B, T, F = xn.shape
    frames = grid_frames(n, every_n, T) if frames is None else frames
    k = np.array([len(f) for f in frames], np.int64)
    row_off = np.concatenate([[0], np.cumsum(k)])
    R = int(row_off[-1])
    vid = np.repeat(np.arange(B), k)
    r = np.concatenate([xn[b, frames[b], :] for b in range(B)], axis=0).reshape(R, F)
    st = (lambda s: None) if stats is None else (lambda s: stats[s])
    r_bn, c_in = _bn(r, P["input_bn/gamma"], P["input_bn/beta"], st("input_bn"))
    Wc = P["cluster_weights"]                                        # [F, K]
    K = Wc.shape[1]
    act = r_bn @ Wc
    act_bn, c_cl = _bn(act, P["cluster_bn/gamma"], P["cluster_bn/beta"], st("cluster_bn"))
    e = np.exp(act_bn - act_bn.max(axis=1, keepdims=True))
    a = e / e.sum(axis=1, keepdims=True)                             # [R, K]
    C2 = P["cluster_weights2"]                                       # [F, K]
    asum = np.zeros((B, K))
    V = np.zeros((B, K, F))
    for b in range(B):
        lo, hi = row_off[b], row_off[b + 1]
        asum[b] = a[lo:hi].sum(axis=0)
        V[b] = a[lo:hi].T @ r_bn[lo:hi] - asum[b][:, None] * C2.T
    n1 = np.sqrt(np.maximum((V * V).sum(axis=2), 1e-12))
    Uc = V / n1[:, :, None]
    Uf = Uc.transpose(0, 2, 1).reshape(B, F * K)                     # index f*K + k
    n2 = np.sqrt(np.maximum((Uf * Uf).sum(axis=1), 1e-12))
    Y = Uf / n2[:, None]
    hid = Y @ P["hidden1_weights"]
    hid_bn, c_h = _bn(hid, P["hidden1_bn/gamma"], P["hidden1_bn/beta"], st("hidden1_bn"))
    h6 = mm.relu6(hid_bn)
    pred, c_moe = mm.moe_fwd(h6, P["classifier/gates/weights"], P["classifier/experts/weights"], P["classifier/experts/biases"], num_mixtures)
    cache = dict(frames=frames, k=k, row_off=row_off, vid=vid, r=r, r_bn=r_bn, a=a, asum=asum, V=V, n1=n1, U=Uc, n2=n2, Y=Y, hid_bn=hid_bn,
                 h6=h6, c_in=c_in, c_cl=c_cl, c_h=c_h, c_moe=c_moe, dims=(B, R, F, K), P=P)
    return pred, cache


def aggregate_bwd(dV, cache):
    """da [R,K] and the aggregation's share of dr_bn [R,F] from dV [B,K,F]: each row takes its own video's dV."""
    C2 = cache["P"]["cluster_weights2"]
    dVr = dV[cache["vid"]]                                           # [R, K, F]
    q = np.einsum("bkf,fk->bk", dV, C2)[cache["vid"]]                # [R, K]
    da = np.einsum("rkf,rf->rk", dVr, cache["r_bn"]) - q
    dX = np.einsum("rk,rkf->rf", cache["a"], dVr)
    return da, dX


def netvlad_packed_bwd(dpred, cache):
    """Gradients of every trainable variable (TF layouts, as oracle.model_math.netvlad_bwd) from a training-mode forward's cache."""
    c, P = cache, cache["P"]
    B, R, F, K = c["dims"]
    g = {}
    dh6, g["classifier/gates/weights"], g["classifier/experts/weights"], g["classifier/experts/biases"] = mm.moe_bwd(dpred, c["c_moe"])
    dhid_bn = dh6 * ((c["hid_bn"] > 0) & (c["hid_bn"] < 6))
    dhid, g["hidden1_bn/gamma"], g["hidden1_bn/beta"] = mm.batch_norm_train_bwd(dhid_bn, c["c_h"])
    Y, n2, Uc, n1 = c["Y"], c["n2"], c["U"], c["n1"]
    g["hidden1_weights"] = Y.T @ dhid
    dY = dhid @ P["hidden1_weights"].T
    dUf = (dY - Y * (Y * dY).sum(axis=1, keepdims=True)) / n2[:, None]
    dU = dUf.reshape(B, F, K).transpose(0, 2, 1)
    dV = (dU - Uc * (Uc * dU).sum(axis=2, keepdims=True)) / n1[:, :, None]
    g["cluster_weights2"] = -np.einsum("bk,bkf->fk", c["asum"], dV)
    da, dX = aggregate_bwd(dV, c)
    a = c["a"]
    dz = a * (da - (a * da).sum(axis=1, keepdims=True))
    dact, g["cluster_bn/gamma"], g["cluster_bn/beta"] = mm.batch_norm_train_bwd(dz, c["c_cl"])
    g["cluster_weights"] = c["r_bn"].T @ dact
    dr_bn = dact @ P["cluster_weights"].T + dX
    _, g["input_bn/gamma"], g["input_bn/beta"] = mm.batch_norm_train_bwd(dr_bn, c["c_in"])
    c["dV"], c["da"], c["dX"] = dV, da, dX
    return g


# ---------------------------------------------------------------------------- the two packed entries, per element
# (K, F, rows of every video) - chosen for the edges: empty videos first / last / in a row and K, F / 4 odd; K no multiple of 4 or 32,
# F no multiple of 32 or 96, lengths around the MFMA's pairs and the load batch of 8; lengths across the 64-row staging pass, odd
# lengths, F / 4 = 68 > 64 and two 192-column tiles; one video of 300 rows, far past the fixed-length entries' 64.
NV_PACKED = [(7, 12, (0, 5, 2, 0)), (18, 100, (0, 1, 16, 17, 33, 40)), (64, 272, (63, 64, 65, 129, 1)), (40, 64, (300,))]
NV_T = 300


def packed_case(K, F, ks):
    rng = np.random.default_rng(10300 + 7 * K + F + len(ks))
    c = Case()
    c.B, c.K, c.F, c.ks, c.T = len(ks), K, F, tuple(ks), NV_T
    c.name = "K=%d F=%d ks=%s" % (K, F, ",".join(str(k) for k in ks))
    c.row_off = np.concatenate([[0], np.cumsum(ks)]).astype(np.int32)
    c.R, c.max_k = int(c.row_off[-1]), int(max(ks))
    R = c.R
    c.r = rng.standard_normal((R, F)).astype(F32)
    c.mean = (rng.standard_normal(F) * 0.1).astype(F32)              # non-trivial statistics, scale and offset
    c.var = (0.5 + rng.random(F)).astype(F32)
    c.gamma = (1.0 + 0.2 * rng.standard_normal(F)).astype(F32)
    c.beta = (0.2 * rng.standard_normal(F)).astype(F32)
    raw = rng.random((R, K)) ** 3
    c.a = (raw / raw.sum(axis=1, keepdims=True)).astype(F32)
    c.c2 = (rng.standard_normal((K, F)) / np.sqrt(F)).astype(F32)
    c.dV = rng.standard_normal((c.B, K, F)).astype(F32)
    return c


def equal_case(B, S, K, F):
    """Every video S rows long: the shape the fixed-length entries take too."""
    return packed_case(K, F, (S,) * B)


def xbn(c):
    """xb as the kernels form it: (r - mean) * (rsqrtf(var + C3) * gamma) + beta -> (value, bound) [R][F]."""
    return add(mul(sub(ex(c.r), ex(c.mean)), mul(rsq(add(ex(c.var), ex(C3))), ex(c.gamma))), ex(c.beta))


def fwd_video(A, xb, c2):
    """A [L][K] f32, xb = (value, bound) [L][F], c2 [K][F] -> (V, d_V, asum, d_asum)."""
    A = f64(A)
    L, K = A.shape
    F = xb[0].shape[1]
    if L == 0:
        z = np.zeros((K, F))
        return z, z, np.zeros(K), np.zeros(K)
    acc = tsum(mul((A[:, :, None], 0.0), (xb[0][:, None, :], xb[1][:, None, :])), 0, L)
    asum = tsum(ex(A), 0, L)
    V = sub(acc, mul((asum[0][:, None], asum[1][:, None]), ex(c2)))
    return V[0], V[1], asum[0], asum[1]


def bwd_video(A, xb, c2, dV):
    """-> (dx [L][F], d, da [L][K], d) for one video with L > 0 rows."""
    A, dV = f64(A), f64(dV)
    K, F = dV.shape
    dx = A @ dV, (K + 1) * U * (np.abs(A) @ np.abs(dV))
    t = mul((dV[None, :, :], 0.0), (xb[0][:, None, :], xb[1][:, None, :]))                  # [L][K][F]
    acc = tsum(t, 2, F)
    qt = dV * f64(c2)
    q = qt.sum(axis=1), (wave_depth(F) + 1) * U * np.abs(qt).sum(axis=1)
    da = sub(acc, (q[0][None, :], q[1][None, :]))
    return dx[0], dx[1], da[0], da[1]


def agg_ref(c):
    """A packed case -> dict of Out: V [B][K][F], asum [B][K], dx [R][F], da [R][K]."""
    B, K, F, R = c.B, c.K, c.F, c.R
    xb = xbn(c)
    V, dVv, s, ds = np.zeros((B, K, F)), np.zeros((B, K, F)), np.zeros((B, K)), np.zeros((B, K))
    dx, ddx, da, dda = np.zeros((R, F)), np.zeros((R, F)), np.zeros((R, K)), np.zeros((R, K))
    for b in range(B):
        lo, hi = int(c.row_off[b]), int(c.row_off[b + 1])
        xv = xb[0][lo:hi], np.broadcast_to(xb[1], xb[0].shape)[lo:hi]
        V[b], dVv[b], s[b], ds[b] = fwd_video(c.a[lo:hi], xv, c.c2)
        if hi > lo:
            dx[lo:hi], ddx[lo:hi], da[lo:hi], dda[lo:hi] = bwd_video(c.a[lo:hi], xv, c.c2, c.dV[b])
    return dict(V=Out(V, dVv), asum=Out(s, ds), dx=Out(dx, ddx), da=Out(da, dda))


# ---------------------------------------------------------------------------- an f32 evaluation of each kernel's chain
def wave_sum32(x):
    """sum of a 1-D f32 vector as one wave adds it: lane j takes elements j, j + 64, .. in turn, then six xor-shuffle steps."""
    lanes = np.zeros(64, F32)
    for j0 in range(0, len(x), 64):
        seg = np.asarray(x[j0:j0 + 64], F32)
        lanes[:len(seg)] = lanes[:len(seg)] + seg
    o = 32
    while o:
        lanes = (lanes + lanes[np.arange(64) ^ o]).astype(F32)
        o >>= 1
    return lanes[0]


def xb32(c, with_beta=True):
    sc = ((1.0 / np.sqrt(f64(c.var) + C3)).astype(F32) * c.gamma).astype(F32)
    x = ((c.r - c.mean).astype(F32) * sc).astype(F32)
    return (x + c.beta).astype(F32) if with_beta else x


def emulate(c, drop_last=False, wrong_c2=False, no_q=False, no_beta=False):
    """The four outputs in f32 with each kernel's summation order (one rounding per operation).  The keywords plant a fault each: the
    last row of every video left out of V / asum; c2 of the next cluster in V; da without - q; xb without beta."""
    B, K, F, R = c.B, c.K, c.F, c.R
    xb = xb32(c, not no_beta)
    V, asum = np.zeros((B, K, F), F32), np.zeros((B, K), F32)
    dx, da = np.zeros((R, F), F32), np.zeros((R, K), F32)
    c2 = np.roll(c.c2, 1, axis=0) if wrong_c2 else c.c2
    for b in range(B):
        lo, hi = int(c.row_off[b]), int(c.row_off[b + 1])
        acc, s = np.zeros((K, F), F32), np.zeros(K, F32)
        for l in range(lo, hi - 1 if drop_last else hi):
            acc = (acc + (c.a[l][:, None] * xb[l][None, :]).astype(F32)).astype(F32)
            s = (s + c.a[l]).astype(F32)
        V[b], asum[b] = (acc - (s[:, None] * c2).astype(F32)).astype(F32), s
        if hi == lo:
            continue
        ax = np.zeros((hi - lo, F), F32)
        for k in range(K):
            ax = (ax + (c.a[lo:hi, k][:, None] * c.dV[b, k][None, :]).astype(F32)).astype(F32)
        dx[lo:hi] = ax
        aa = np.zeros((hi - lo, K), F32)
        for f in range(F):
            aa = (aa + (xb[lo:hi, f][:, None] * c.dV[b, :, f][None, :]).astype(F32)).astype(F32)
        q = np.array([wave_sum32((c.dV[b, k] * c.c2[k]).astype(F32)) for k in range(K)], F32)
        da[lo:hi] = aa if no_q else (aa - q[None, :]).astype(F32)
    return dict(V=V, asum=asum, dx=dx, da=da)
