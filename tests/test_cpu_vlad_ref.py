"""tests/_vlad_ref.py on the CPU: every reference against oracle.model_math.netvlad_fwd / _bwd and tests/_nextvlad_ref.py (1e-12,
composed piecewise), an f32 numpy emulation of every kernel of csrc/evc_nextvlad.hip and csrc/evc_netvlad.hip on every case of the GPU
suite - the kernel's own order: one sequential chain over l in the products, the colsum trees, a wave's sum as lane partials and the
xor butterfly, exp / rsqrt / sqrt evaluated in float64 and rounded to f32 - which must lie inside every bound (`ratio emu` lines: the
bounds hold on the reference side and none is vacuous), the coverage the case table must keep under the restated nx_pick, and planted
faults in the emulations, each of which must leave the bound at the element it predicts.  Buffers carry the guards of the GPU suite
(one NaN row behind every output, NaN columns where an entry takes a row stride), judged by the same _vlad_ref.judge."""
import math

import numpy as np
import pytest

import _nextvlad_ref as nxr
import _vlad_ref as vr
from _vlad_ref import F32, F64, bf16_bits
from oracle import model_math as mm

NANBF = np.uint16(0x7FC0)
_cache = {}


def once(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


# ---------------------------------------------------------------------------- f32 building blocks
def rsqrt32(v):
    return (1.0 / np.sqrt(np.asarray(v, F64))).astype(F32)


def sqrt32(v):
    return np.sqrt(np.asarray(v, F64)).astype(F32)


def exp32(z):
    with np.errstate(over="ignore"):
        return np.exp(np.asarray(z, F64)).astype(F32)


def sig32(x):
    return (F32(1.0) / (F32(1.0) + exp32(-x))).astype(F32)


def seq_sum(x, axis):
    """Sequential f32 sum from zero along an axis."""
    x = np.moveaxis(np.asarray(x, F32), axis, 0)
    acc = np.zeros(x.shape[1:], F32)
    for i in range(x.shape[0]):
        acc = acc + x[i]
    return acc


def butterfly(v):
    """wave_sum: [.., 64] -> [..] by the xor butterfly 32, 16, .., 1 (as lane 0 sees it; every lane holds the same bits)."""
    n = 64
    while n > 1:
        n //= 2
        v = v[..., :n] + v[..., n:2 * n]
    return v[..., 0]


def lane_sum(x, lanes=64):
    """[.., n] -> [.., lanes]: lane j adds elements j, j + lanes, .. in turn from zero."""
    n = x.shape[-1]
    trips = -(-n // lanes)
    pad = np.zeros(x.shape[:-1] + (trips * lanes,), F32)
    pad[..., :n] = x
    return seq_sum(pad.reshape(x.shape[:-1] + (trips, lanes)), -2)


def wave_sum(x):
    return butterfly(lane_sum(x))


def block_sum_256(x):
    """[.., n] over 256 threads: thread partials, the four waves' butterflies, sh[0] + sh[1] + sh[2] + sh[3]."""
    w = butterfly(lane_sum(x, 256).reshape(x.shape[:-1] + (4, 64)))
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def nanbuf(shape):
    return np.full(shape, np.nan, F32)


def e_bn(x, mean, var, gamma, beta):
    return (x - mean) * rsqrt32(var + F32(1e-3)) * gamma + beta


def e_softmax(y, fault=None):
    mx = (y[..., :64] if fault == "max_reg0" else y).max(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", over="ignore"):
        e = exp32(y - mx)
        inv = F32(1.0) / wave_sum(e)
        return e * inv[..., None]


# ---------------------------------------------------------------------------- the emulations
def chain32(T, Bm, L):
    acc = np.zeros((T.shape[1], Bm.shape[1]), F32)
    for l in range(L):
        acc = acc + T[l][:, None] * Bm[l][None, :]
    return acc


def emu_agg(c, fault=None):
    cov = vr.coverage(c.B, c.P, c.K, c.D)
    B, K, D = c.B, c.K, c.D
    Kp = (K + 3) // 4 * 4
    Pt = int(c.off[-1])
    V, asum, dxe = nanbuf((B + 1, K, D)), nanbuf((B + 1, K)), nanbuf((Pt + 1, D))
    da = nanbuf((Pt + 1) * K)

    def leff(mode, L):
        return (-(-L // 64) - 1) * 64 if fault == "drop%d" % mode and L > 0 else L
    for b in range(B):
        lo, hi = int(c.off[b]), int(c.off[b + 1])
        P = hi - lo
        src = int(c.off[b - 1]) if fault == "prev_off" and b > 0 else lo
        A, X = c.a[src:src + P], c.xe[src:src + P]
        acc = chain32(A, X, leff(0, P))
        s = seq_sum(A[:min(P, 64)] if fault == "asum_first" else A[:leff(0, P)], 0)
        sv = np.repeat(s[:, None], D, axis=1)
        if fault == "mtile_sa":
            mt = cov[0]["MT"]
            sv[mt:] = sv[:K - mt]
        cc = c.c2
        if fault == "ntile_c2":
            w = 4 * cov[0]["DW"]
            cc = c.c2.copy()
            cc[:, w:2 * w] = c.c2[:, :cc[:, w:2 * w].shape[1]]
        V[b], asum[b] = acc - sv * cc, s
        if P == 0:
            continue
        dxe[lo:hi] = chain32(A.T, c.dV[b], leff(1, K))
        q = wave_sum(c.dV[b] * c.c2)
        acc2 = chain32(X.T, c.dV[b].T, leff(2, D))
        res = acc2 if fault == "no_q" else acc2 - q[None, :]
        if fault == "pad_cols":
            for m in range(lo, hi):
                da[m * K + K:m * K + Kp] = 0.0
        da[lo * K:hi * K] = res.reshape(-1)
    return dict(V=V, asum=asum, dxe=dxe, da=da.reshape(Pt + 1, K))


def emu_assign(c, fault=None):
    R, G, K = c.R, c.G, c.K
    sh = (G, K)
    p = e_softmax(e_bn(c.act, c.mean.reshape(sh), c.var.reshape(sh), c.gamma.reshape(sh), c.beta.reshape(sh)), fault)
    z = c.attl[:, :G] + (c.att_bias if c.att_bias is not None else F32(0.0))
    att = sig32(z)
    a, dz, datt = nanbuf((R + 1, G, K)), nanbuf((R + 1, G, K)), nanbuf((R + 1, G))
    a[:R] = p * att[:, :, None]
    t = p * c.da
    dot = wave_sum(t[..., :64] if fault == "dot_reg0" else t)
    with np.errstate(invalid="ignore"):
        dz[:R] = p * att[:, :, None] * (c.da - dot[:, :, None])
        dl = dot * att * (F32(1.0) - att)
    datt[:R] = dl
    bf = np.full((R + 1) * c.ld_bf, NANBF, np.uint16)
    ld = G if fault == "bf_stride" else c.ld_bf
    for r in range(R):
        bf[r * ld:r * ld + G] = bf16_bits(dl[r])
    return dict(a=a, dz=dz, datt=datt, datt_bf=bf.reshape(R + 1, c.ld_bf))


def emu_nv_softmax(c, a_in, fault=None):
    R, K = c.R, c.K
    a, dz = nanbuf((R + 1, K)), nanbuf((R + 1, K))
    a[:R] = e_softmax(e_bn(c.act, c.mean, c.var, c.gamma, c.beta), fault)
    dot = wave_sum(a_in * c.da)
    dz[:R] = a_in * (c.da - dot[:, None])
    return dict(a=a, dz=dz)


def emu_nx_norm(c, fault=None):
    B, K, D = c.B, c.K, c.D
    n = sqrt32(wave_sum(c.V * c.V))
    if fault != "no_clamp":
        n = np.maximum(n, F32(1e-12))
    Uo, norms, dV = nanbuf((B + 1, K, D)), nanbuf((B + 1, K)), nanbuf((B + 1, K, D))
    with np.errstate(divide="ignore", invalid="ignore"):
        Uo[:B] = c.V * (F32(1.0) / n)[:, :, None]
    norms[:B] = n
    inv = (F32(1.0) / c.nrm)[:, :, None]
    s = np.where(c.nrm > F32(1e-12), wave_sum(c.V * inv * c.dU), F32(0.0))[:, :, None]
    dV[:B] = (c.dU - c.V * inv * s) * inv
    return dict(U=Uo, norms=norms, dV=dV)


def emu_gate(c, with_dout2, fault=None):
    n = c.n
    live = min(n, vr.CAP) if fault == "tail" else n
    g = sig32(c.gl)
    d = c.dout + c.dout2 if with_dout2 else c.dout
    dl = d * c.h * g * (F32(1.0) - g)
    out, dh, dgl = nanbuf(n + 16), nanbuf(n + 16), nanbuf(n + 16)
    out[:live], dh[:live], dgl[:live] = (c.h * g)[:live], (d * g)[:live], dl[:live]
    bf = np.full(n + 16, NANBF, np.uint16)
    bf[:live] = bf16_bits(dl)[:live]
    return dict(out=out, dh=dh, dgl=dgl, dgl_bf=bf, dgl_bf_alone=bf)


def emu_center(c):
    out = np.full((c.R + 1, c.E), NANBF, np.uint16)
    out[:c.R] = bf16_bits(c.xe - c.be)
    return dict(out=out)


def emu_bias(c):
    out = nanbuf(c.n_out + 16)
    out[:c.n_out] = 0.0
    s = wave_sum(c.be[None, :] * c.W)
    out[:c.N] = s + c.add if c.add is not None else s
    return dict(out=out)


def emu_uncenter(c):
    dW = nanbuf((c.N + 1, c.E))
    dW[:c.N] = c.dWc + c.du[:, None] * c.be[None, :]
    return dict(dW=dW)


def emu_colsum(c, fault=None):
    R, Cc = c.R, c.C
    x = np.vstack([c.x[:, :Cc], nanbuf((64, Cc))])                       # rows >= R: what a read past the input finds
    out = nanbuf(Cc + 16)
    if c.two_pass:
        rpp = -(-R // vr.CS_PARTS)
        parts = []
        for p in range(vr.CS_PARTS):
            r0 = p * rpp
            r1 = min(R, r0 + rpp) if not (fault == "empty_range" and r0 >= R) else min(R + 64, r0 + rpp)
            w = [seq_sum(x[r0 + k:max(r1, r0 + k):4], 0) if r0 + k < r1 else np.zeros(Cc, F32) for k in range(4)]
            parts.append((w[0] + w[1]) + (w[2] + w[3]))
        out[:Cc] = seq_sum(np.stack(parts), 0)
    else:
        out[:Cc] = seq_sum(np.stack([seq_sum(x[w:R:16], 0) if w < R else np.zeros(Cc, F32) for w in range(16)]), 0)
    return dict(out=out)


def emu_nv_agg(c, fault=None):
    B, S, K, F = c.B, c.S, c.K, c.F
    sc = rsqrt32(c.var + F32(1e-3)) * c.gamma
    xb = (c.r - c.mean) * sc + c.beta
    Kt = -(-K // 8) * 8 if fault == "dead_clusters" else K                # the ragged tile's dead clusters computed and stored
    aflat = np.concatenate([c.a.reshape(-1), np.ones(8 * S * K, F32)])     # what a read past a row of a finds: the next rows
    V, asum = nanbuf((B + 1) * K * F), nanbuf((B + 1) * K)
    for b in range(B):
        ab = np.stack([[aflat[(b * S + s) * K + k] for k in range(Kt)] for s in range(S)]).astype(F32)      # [S][Kt]
        acc = np.zeros((Kt, F), F32)
        for s in range(S):
            acc = acc + ab[s][:, None] * xb[b, s][None, :]
        sk = seq_sum(ab, 0)
        c2 = np.vstack([c.c2, np.ones((Kt - K, F), F32)])
        v = acc - sk[:, None] * c2
        if fault == "skip_f4_256":
            v[:, 1024:] = np.nan
        V[b * K * F:b * K * F + Kt * F] = v.reshape(-1)
        asum[b * K:b * K + Kt] = sk
    dx, da = nanbuf((B + 1, S, F)), nanbuf((B + 1, S, K))
    acc = np.zeros((B, S, F), F32)
    for k in range(K):
        acc = acc + c.a[:, :, k, None] * c.dV[:, k, None, :]
    dx[:B] = acc
    if fault == "skip_s0":
        dx[:B, 16:] = np.nan
    xb3 = (c.r - c.mean) * rsqrt32(c.var + F32(1e-3)) * c.gamma + c.beta
    t = c.dV[:, None, :, :] * (xb3[:, :, None, :] - c.c2[None, None])
    t = t.reshape(B, S, K, F // 4, 4)
    da[:B] = wave_sum(((t[..., 0] + t[..., 1]) + t[..., 2]) + t[..., 3])
    return dict(V=V.reshape(B + 1, K, F), asum=asum.reshape(B + 1, K), dx=dx, da=da)


def emu_nv_dc(c, fault=None):
    acc = np.zeros((c.K, c.F), F32)
    for b in range(c.B):
        acc = acc - c.asum[b][:, None] * c.dV[b]
    dc2 = nanbuf((c.K + 1) * c.F)
    n = c.K * c.F
    live = min(n, 4 * vr.CAP) if fault == "tail" else n
    dc2[:live] = acc.reshape(-1)[:live]
    return dict(dc2=dc2.reshape(c.K + 1, c.F))


def emu_nv_norm(c, fault=None):
    B, K, F = c.B, c.K, c.F
    s = wave_sum(c.V * c.V)
    sn1 = sqrt32(s if fault == "no_clamp" else np.maximum(s, F32(1e-12)))
    with np.errstate(divide="ignore", invalid="ignore"):
        u = c.V / sn1[:, :, None]
        nn2 = sqrt32(np.maximum(block_sum_256((u * u).reshape(B, K * F)), F32(1e-12)))
        y = c.V / (sn1[:, :, None] * nn2[:, None, None])
    n1, n2, Y, dV = nanbuf((B + 1, K)), nanbuf(B + 1), nanbuf((B + 1, K, F)), nanbuf((B + 1, K, F))
    n1[:B], n2[:B], Y[:B] = sn1, nn2, y
    Yb = np.full((B + 1, K, F), NANBF, np.uint16)
    Yb[:B] = bf16_bits(y)
    i1, i2 = c.n1[:, :, None], c.n2[:, None, None]
    ydy = block_sum_256((c.V / (i1 * i2) * c.dY).reshape(B, K * F))[:, None, None]
    in1 = F32(1.0) / i1
    uu = c.V * in1
    du = (c.dY - (uu / i2) * ydy) / i2
    tk = wave_sum(uu * du)[:, :, None]
    dV[:B] = (du - uu * tk) * in1
    return dict(n1=n1, n2=n2, Y=Y, Y_bf=Yb, dV=dV)


# ---------------------------------------------------------------------------- every case: the emulation inside every bound
def report(entry, name, q):
    bad = []
    for out, arr in q.items():
        r, at = vr.worst(arr)
        print("ratio emu %s %s %s %.4f at %s" % (entry, name, out, r, at))
        if not r <= 1.0:
            bad.append("%s %s %s %.4f at %s" % (entry, name, out, r, at))
    assert q and not bad, "\n".join(bad)


def agg_cases():
    return [vr.agg_case(*s) for s in vr.NX_FIXED] + [vr.agg_packed_case(*s) for s in vr.NX_PACKED]


def agg_ref(c):
    return once(("aggref", c.name), lambda: vr.agg_ref(c))


def test_products_emulation_inside_every_bound():
    for c in agg_cases():
        report("nextvlad_aggregate", c.name, vr.judge(agg_ref(c), emu_agg(c)))


def test_case_table_keeps_its_coverage():
    """Over the table, for each MODE: a second column tile, a second row tile, several passes with a ragged last one, a last column
    tile with idle lanes, a last row tile with idle rows; and every DW once."""
    fixed = [vr.coverage(B, S * G, K, D) for B, S, G, K, D in vr.NX_FIXED]
    packed = [vr.coverage(len(ks), max(ks) * G, K, D) for G, K, D, ks in vr.NX_PACKED]
    for mode in (0, 1, 2):
        m = [cv[mode] for cv in fixed]
        assert any(x["ntiles"] > 1 for x in m) and any(x["mtiles"] > 1 for x in m), mode
        assert any(x["passes"] > 1 and x["ragged"] for x in m), mode
        assert any(x["ntiles"] > 1 and x["col_edge"] for x in m) and any(x["mtiles"] > 1 and x["row_edge"] for x in m), mode
    for mode in (1, 2):                                                 # the packed backward: second passes, column tiles, row tiles
        m = [cv[mode] for cv in packed]
        assert any(x["ntiles"] > 1 and x["mtiles"] > 1 and x["passes"] > 1 and x["ragged"] for x in m), mode
    assert {cv[m]["DW"] for cv in fixed for m in (0, 1, 2)} == {16, 32, 64}
    cv = vr.coverage(1, 1024, 130, 260)[0]
    assert (cv["DW"], cv["ntiles"], cv["mtiles"]) == (32, 3, 3) and 130 - 2 * cv["MT"] == 2
    cv = vr.coverage(3, 240, 64, 288)
    assert cv[0]["ntiles"] == 5 and 72 - 4 * 16 == 8 and cv[1]["mtiles"] == 2 and 240 - 128 == 112
    assert (cv[0]["passes"], cv[1]["passes"], cv[2]["passes"]) == (4, 1, 5) and 288 % 64 == 32
    assert vr.colsum_case(513, 65, 65, True).two_pass and 31 * math.ceil(513 / 32) >= 513     # the last of the 32 row ranges is empty


def test_assignment_emulation_inside_every_bound():
    for K in vr.ASSIGN_KS:
        for G in vr.ASSIGN_GS:
            for wb in (True, False):
                c = vr.assign_case(K, G, wb)
                y = vr.bn(c.act, *(v.reshape(G, K) for v in (c.mean, c.var, c.gamma, c.beta)))[0]
                assert y[0].max() - y[0].min() > 79.0 and (vr.softmax((y, 0.0))[0][0] < vr.U).mean() > 0.5
                refs = vr.assign_ref(c)
                got = emu_assign(c)
                q = vr.judge({k: refs[k] for k in ("a", "dz", "datt")}, got)
                q["datt_bf"] = vr.bits_vs(got["datt_bf"], got["datt"][:c.R])
                report("nextvlad_assign", c.name, q)
    for K in vr.NV_SOFTMAX_KS:
        c = vr.nv_softmax_case(K)
        a_in = vr.softmax_f32(c.act, c.mean, c.var, c.gamma, c.beta)
        report("netvlad_softmax", c.name, vr.judge(vr.nv_softmax_ref(c, a_in), emu_nv_softmax(c, a_in)))


def test_nextvlad_elementwise_emulation_inside_every_bound():
    for s in vr.NX_NORM_SHAPES:
        c = vr.nx_norm_case(*s)
        got = emu_nx_norm(c)
        assert not got["U"][0, 0].any() and got["norms"][0, 0] == F32(1e-12)
        report("nextvlad_normalize", c.name, vr.judge(vr.nx_norm_ref(c), got))
    for n in vr.GATE_NS:
        c = vr.gate_case(n)
        for d2 in (False, True):
            refs, got = vr.gate_ref(c, d2), emu_gate(c, d2)
            q = vr.judge(refs, got)
            q["dgl_bf"] = vr.bits_vs(got["dgl_bf"], got["dgl"][:n])
            report("nextvlad_gate" + ("_add" if d2 else ""), c.name, q)
    for s in vr.CENTER_SHAPES:
        c = vr.center_case(*s)
        report("nextvlad_center_cast", c.name, vr.judge(vr.center_ref(c), emu_center(c)))
    for s in vr.BIAS_SHAPES:
        for wa in (True, False):
            c = vr.bias_case(*s, wa)
            report("nextvlad_bias_logits", c.name, vr.judge(vr.bias_ref(c), emu_bias(c)))
    for s in vr.UNCENTER_SHAPES:
        c = vr.uncenter_case(*s)
        report("nextvlad_wgrad_uncenter", c.name, vr.judge(vr.uncenter_ref(c), emu_uncenter(c)))
    for s in vr.COLSUM_CASES:
        c = vr.colsum_case(*s)
        report("nextvlad_colsum", c.name, vr.judge(vr.colsum_ref(c), emu_colsum(c)))


def test_netvlad_emulation_inside_every_bound():
    for s in vr.NV_SHAPES:
        c = vr.nv_case(*s)
        refs = vr.nv_agg_ref(c)
        report("netvlad_aggregate", c.name, vr.judge({k: refs[k] for k in ("V", "asum", "dx", "da")}, emu_nv_agg(c)))
        c = vr.nv_norm_case(*s)
        got = emu_nv_norm(c)
        assert not got["Y"][0, 1].any()
        q = vr.judge(vr.nv_norm_ref(c), got)
        q["Y_bf"] = vr.bits_vs(got["Y_bf"], got["Y"][:c.B])
        report("netvlad_normalize", c.name, q)
    for s in vr.NV_DC_SHAPES:
        c = vr.nv_dc_case(*s)
        report("netvlad_dcenters", c.name, vr.judge(vr.nv_dc_ref(c), emu_nv_dc(c)))


# ---------------------------------------------------------------------------- planted faults
def _fixed(i):
    return vr.agg_case(*vr.NX_FIXED[i])


def _fault_table():
    """(name, the case, the faulty emulation, the references, output, predicted element)."""
    small, tower, wide = _fixed(1), _fixed(2), _fixed(4)
    pk = vr.agg_packed_case(*vr.NX_PACKED[3])
    w0 = 4 * vr.coverage(small.B, small.P, small.K, small.D)[0]["DW"]
    mt0 = vr.coverage(wide.B, wide.P, wide.K, wide.D)[0]["MT"]
    agg = lambda c, f: (lambda: emu_agg(c, f), lambda: agg_ref(c))
    rows = [
        ("MODE 0 drops its last pass", *agg(tower, "drop0"), "V", (0, 0, 0)),
        ("MODE 1 drops its last pass", *agg(small, "drop1"), "dxe", (0, 0)),
        ("MODE 2 drops its last pass", *agg(small, "drop2"), "da", (0, 0)),
        ("column tile 1 reads tile 0's c2 columns", *agg(small, "ntile_c2"), "V", (0, 0, w0)),
        ("asum from the first pass only", *agg(tower, "asum_first"), "asum", (0, 0)),
        ("row tile 1 uses row tile 0's sa[]", *agg(wide, "mtile_sa"), "V", (0, mt0, 0)),
        ("MODE 2 without q", *agg(small, "no_q"), "da", (0, 0)),
        ("MODE 2 writes the padding columns K..Kp", *agg(small, "pad_cols"), "da guard", None),
        ("packed video b at video b-1's row offset", *agg(pk, "prev_off"), "V", (2, 0, 0)),
    ]
    big = vr.assign_case(128, 3, True)
    rows += [
        ("softmax maximum over register 0 only", lambda: emu_assign(big, "max_reg0"), lambda: vr.assign_ref(big), "a", (2, 0, 127)),
        ("assign backward's dot without k >= 64", lambda: emu_assign(big, "dot_reg0"), lambda: vr.assign_ref(big), "datt", (3, 0)),
        ("datt_bf16 at row stride G", lambda: emu_assign(big, "bf_stride"), None, "datt_bf", None),
    ]
    rag, chunk = vr.nv_case(*vr.NV_SHAPES[1]), vr.nv_case(*vr.NV_SHAPES[2])
    rows += [
        ("NetVLAD ragged cluster tile's dead clusters stored", lambda: emu_nv_agg(rag, "dead_clusters"), lambda: vr.nv_agg_ref(rag), "V guard", None),
        ("NetVLAD backward skips the second s0 chunk", lambda: emu_nv_agg(chunk, "skip_s0"), lambda: vr.nv_agg_ref(chunk), "dx", (0, 16, 0)),
        ("NetVLAD forward skips the columns F4 >= 256", lambda: emu_nv_agg(rag, "skip_f4_256"), lambda: vr.nv_agg_ref(rag), "V", (0, 0, 1024)),
    ]
    nn, nx = vr.nv_norm_case(*vr.NV_SHAPES[0]), vr.nx_norm_case(*vr.NX_NORM_SHAPES[0])
    cs = vr.colsum_case(513, 65, 65, True)
    gt, dc = vr.gate_case(vr.GATE_NS[-1]), vr.nv_dc_case(*vr.NV_DC_SHAPES[-1])
    rows += [
        ("NetVLAD normalize without the clamp", lambda: emu_nv_norm(nn, "no_clamp"), lambda: vr.nv_norm_ref(nn), "Y", (0, 1, 0)),
        ("NeXtVLAD normalize without the clamp", lambda: emu_nx_norm(nx, "no_clamp"), lambda: vr.nx_norm_ref(nx), "U", (0, 0, 0)),
        ("colsum's empty last range reads rows >= R", lambda: emu_colsum(cs, "empty_range"), lambda: vr.colsum_ref(cs), "out", (0,)),
        ("gate: the grid-stride tail left unwritten", lambda: emu_gate(gt, False, "tail"), lambda: vr.gate_ref(gt, False), "out", (vr.CAP,)),
        ("dcenters: the grid-stride tail left unwritten", lambda: emu_nv_dc(dc, "tail"), lambda: vr.nv_dc_ref(dc), "dc2", (4 * vr.CAP // dc.F, 4 * vr.CAP % dc.F)),
    ]
    return rows


@pytest.mark.parametrize("i", range(20))
def test_planted_fault_leaves_the_bound_where_predicted(i):
    name, emu, ref, out, at = once("faults", _fault_table)[i]
    got = emu()
    if out == "datt_bf":                                                 # rows land at stride G: row 1 starts inside row 0's guard columns
        c = vr.assign_case(128, 3, True)
        q = vr.bits_vs(got["datt_bf"], got["datt"][:c.R])
        assert np.isinf(q).any(), name
        return
    refs = ref()
    q = vr.judge({k: v for k, v in refs.items() if isinstance(v, vr.Out)}, got)
    arr = q[out]
    v = float(arr.max()) if at is None else float(arr[at])
    print("fault %-55s %s at %s: ratio %.3g" % (name, out, at, v))
    assert v > 1.0, name


def test_fault_table_has_twenty_rows():
    assert len(_fault_table()) == 20


# ---------------------------------------------------------------------------- the references against the oracles
def test_netvlad_references_are_the_oracle():
    rng = np.random.default_rng(5)
    B, S, F, K, H, Vc = 4, 6, 8, 5, 7, 9
    P = mm.init_netvlad_params(rng, F, K, H, Vc)
    for k in P:
        if k.endswith("/gamma") or k.endswith("/beta"):
            P[k] = P[k] + 0.2 * rng.standard_normal(P[k].shape)
    x = rng.standard_normal((B, 10, F))
    n = np.array([10, 3, 7, 1], np.int32)
    u = rng.random((B, S)).astype(np.float32)
    pred, cache = mm.netvlad_fwd(x, n, u, P)
    idx, r_bn, c_in, a3, X, a_sum, C2, V, n1, Uo, n2, Y, hid_bn, c_h, h6, c_moe, c_cl, _, _ = cache
    c = vr.Case()
    c.B, c.S, c.K, c.F = B, S, K, F
    c.r, c.mean, c.var, c.gamma, c.beta = X, np.zeros(F), np.full(F, 1.0 - vr.C3), np.ones(F), np.zeros(F)
    c.a, c.c2 = a3, C2.T
    close = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-12 * max(1.0, np.abs(b).max())
    # forward: softmax, aggregation, normalisation
    act = r_bn @ P["cluster_weights"]
    act_bn, _ = mm.batch_norm_train_fwd(act, P["cluster_bn/gamma"], P["cluster_bn/beta"])
    ident = (np.zeros(K), np.full(K, 1.0 - vr.C3), np.ones(K), np.zeros(K))
    assert close(vr.softmax(vr.bn(act_bn, *ident))[0], a3.reshape(B * S, K))
    dpred = rng.standard_normal(pred.shape)
    g = mm.netvlad_bwd(dpred, cache)
    dh6 = mm.moe_bwd(dpred, c_moe)[0]
    dhid = mm.batch_norm_train_bwd(dh6 * ((hid_bn > 0) & (hid_bn < 6)), c_h)[0]
    dY = (dhid @ P["hidden1_weights"].T).reshape(B, F, K).transpose(0, 2, 1)
    c.V, c.dY, c.n1, c.n2 = V, dY, n1, n2
    nr = vr.nv_norm_ref(c)
    assert close(nr["n1"].ref, n1) and close(nr["n2"].ref, n2) and close(nr["Y"].ref, Y.reshape(B, F, K).transpose(0, 2, 1))
    c.dV = nr["dV"].ref
    ar = vr.nv_agg_ref(c)
    assert close(ar["V"].ref, V) and close(ar["asum"].ref, a_sum)
    c.asum = a_sum
    assert close(vr.nv_dc_ref(c)["dc2"].ref.T, g["cluster_weights2"])
    s = vr.Case()
    s.K, s.act, s.da = K, act_bn, ar["da"].ref.reshape(B * S, K)
    s.mean, s.var, s.gamma, s.beta = ident
    dz = vr.nv_softmax_ref(s, a3.reshape(B * S, K))["dz"].ref
    dact, gg, gb = mm.batch_norm_train_bwd(dz, c_cl)
    assert close(gg, g["cluster_bn/gamma"]) and close(gb, g["cluster_bn/beta"]) and close(r_bn.T @ dact, g["cluster_weights"])
    dr_bn = dact @ P["cluster_weights"].T + ar["dx"].ref.reshape(B * S, F)
    _, gi, bi = mm.batch_norm_train_bwd(dr_bn, c_in)
    assert close(gi, g["input_bn/gamma"]) and close(bi, g["input_bn/beta"])


def test_nextvlad_references_are_the_restatement():
    rng = np.random.default_rng(6)
    B, S, F, G, K, H, Vc = 3, 5, 6, 2, 4, 8, 7
    P = nxr.init_params(rng, F, 2, G, K, H, 2, Vc)
    xn = rng.standard_normal((B, 9, F))
    n = np.array([9, 2, 5], np.int32)
    u = rng.random((B, S)).astype(np.float32)
    pred, ca = nxr.nextvlad_fwd(xn, n, u, P)
    D = ca["dims"][4]
    R = B * S
    close = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-12 * max(1.0, np.abs(b).max())
    z, _ = mm.batch_norm_train_fwd(ca["xe"] @ P["cluster_weights"], P["cluster_bn/gamma"], P["cluster_bn/beta"])
    dpred = rng.standard_normal(pred.shape)
    g = nxr.nextvlad_bwd(dpred, ca)
    # the tail of the restatement down to dU, with its own primitives
    dout = mm.moe_bwd(dpred, ca["c_moe"])[0]
    gc = vr.Case()
    gc.h, gc.gl, gc.dout, gc.dout2 = ca["h"], ca["g1"] @ P["gating_weights_2"], dout, np.zeros_like(dout)
    gr = vr.gate_ref(gc, False)
    assert close(gr["out"].ref, ca["out"]) and close(ca["g1"].T @ gr["dgl"].ref, g["gating_weights_2"])
    dg1bn = (gr["dgl"].ref @ P["gating_weights_2"].T) * ((ca["g1bn"] > 0) & (ca["g1bn"] < 6))
    dg1pre = mm.batch_norm_train_bwd(dg1bn, ca["c_g"])[0]
    dh = gr["dh"].ref + dg1pre @ P["gating_weights_1"].T
    dhid = mm.batch_norm_train_bwd(dh, ca["c_h"])[0]
    dUf = mm.batch_norm_train_bwd(dhid @ P["hidden1_weights"].T, ca["c_v"])[0]
    nc = vr.Case()
    nc.B, nc.K, nc.D, nc.V, nc.dU, nc.nrm = B, K, D, ca["V"], dUf.reshape(B, D, K).transpose(0, 2, 1), ca["nrm"]
    nr = vr.nx_norm_ref(nc)
    assert close(nr["U"].ref, ca["U"]) and close(nr["norms"].ref, ca["nrm"])
    c = vr.Case()
    c.B, c.K, c.D, c.P = B, K, D, S * G
    c.off = np.arange(B + 1) * c.P
    c.a, c.xe, c.c2, c.dV = ca["a"].reshape(R * G, K), ca["xe"].reshape(R * G, D), P["cluster_weights2"].T, nr["dV"].ref
    ar = vr.agg_ref(c)
    assert close(ar["V"].ref, ca["V"]) and close(ar["asum"].ref, ca["asum"])
    assert close(-np.einsum("bk,bkd->dk", ar["asum"].ref, c.dV), g["cluster_weights2"])
    s = vr.Case()
    s.R, s.G, s.K, s.act, s.da = R, G, K, z.reshape(R, G, K), ar["da"].ref.reshape(R, G, K)
    s.mean, s.var, s.gamma, s.beta = np.zeros(G * K), np.full(G * K, 1.0 - vr.C3), np.ones(G * K), np.zeros(G * K)
    s.attl, s.att_bias = ca["xe"] @ P["attention_weights"], P["attention_biases"]
    sr = vr.assign_ref(s)
    assert close(sr["a"].ref, ca["a"]) and close(sr["datt"].ref.sum(axis=0), g["attention_biases"])
    dact, gg, gb = mm.batch_norm_train_bwd(sr["dz"].ref.reshape(R, G * K), ca["c_cl"])
    assert close(gg, g["cluster_bn/gamma"]) and close(gb, g["cluster_bn/beta"])
    dxe = ar["dxe"].ref.reshape(R, G * D) + dact @ P["cluster_weights"].T + sr["datt"].ref @ P["attention_weights"].T
    cs = vr.Case()
    cs.R, cs.C, cs.two_pass, cs.x = R, G * D, False, dxe
    assert close(vr.colsum_ref(cs)["out"].ref, g["expansion_biases"])
    # the centred products: bf16-free identities of center_cast / bias_logits / wgrad_uncenter
    be, Wa = P["expansion_biases"], P["attention_weights"].T
    bc = vr.Case()
    bc.N, bc.E, bc.n_out, bc.be, bc.W, bc.add = G, be.size, G + 2, be, Wa, P["attention_biases"]
    cc = vr.Case()
    cc.xe, cc.be = ca["xe"], be
    logits = vr.center_ref(cc)["out"].ref @ Wa.T + vr.bias_ref(bc)["out"].ref[:G]
    assert close(logits, s.attl + s.att_bias)
    uc = vr.Case()
    uc.dWc, uc.du, uc.be = sr["datt"].ref.T @ vr.center_ref(cc)["out"].ref, sr["datt"].ref.sum(axis=0), be
    assert close(vr.uncenter_ref(uc)["dW"].ref.T, g["attention_weights"])
