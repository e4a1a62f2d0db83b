"""Float64 references of the two VLAD kernel families (csrc/evc_nextvlad.hip, csrc/evc_netvlad.hip), each with a derived per-element
bound on |got - ref| and a case generator.  numpy only.  Used by tests/test_cpu_vlad_ref.py (the references against
oracle.model_math.netvlad_fwd / _bwd and tests/_nextvlad_ref.py, an f32 emulation of every kernel, planted faults) and
tests/test_gpu_vlad_parity.py (the kernels).  The companion of tests/_head_ref.py, whose notation and error models it reuses:

    U = 2^-24, EPS = 2^-20, RB = 2^-8, prod(), TINY = 2^-100 are imported from _head_ref; sig() is its sigmoid_ref (the sigmoidf_ bound
    p (1 - p) d_z + d_z^2 + EPS, d_z = 2U(|z| + 2)) with the error of the argument itself added to d_z
    __expf(z): a shift of the argument by 2U(|z| + 2);   rsqrtf / sqrtf: 1 ulp = 2U relative;   IEEE division: U
    an f32 sum whose tree has depth D is off by at most D U sum|terms|

Every reference is fed the kernel's own f32 inputs as exact float64 numbers (the kernels' f32 constants 1e-3f, 1e-12f likewise: C3, C12
below).  No measured constant enters a bound.  A value stored as f32: limit = d.  A value stored as bf16: limit = RB (|ref| + d) + d.

Pair arithmetic.  A quantity is a pair (v, d): the float64 value and a bound on the distance of the kernel's f32 value from it.
    mul((a, da), (b, db)) = (ab, (|a| + da)(|b| + db) - |ab| + U (|a| + da)(|b| + db))      one rounding: prod() of two factors
    sub / add            = (a -+ b, da + db + U (|a -+ b| + da + db))
    div((a, da), (b, db)) = (a / b, hi - |a / b| + U hi),  hi = (|a| + da) / (|b| - db)       correctly rounded; needs db < |b|
    tsum(terms, D)       = (sum v, sum d + D U sum (|v| + d))                                the depth-D sum above
    rsq((v, d))          = v^-1/2 to (rel(v) / 2 (1 + rel(v)) + 2U) of itself;  sq((v, d)) = v^1/2 likewise
An fma (hipcc contracts a * b + c) has one rounding fewer than mul followed by add: the bound covers both.

Batch-norm of a logit or a feature (every kernel recomputes it):  y = (x - mean) * rsqrtf(var + C3) * gamma + beta, left to right:
    bn(x) = add(mul(mul(sub(x, mean), rsq(add(var, C3))), gamma), beta)

Softmax over K clusters held as k = lane + 64 i in 16 registers a lane (nx_group_softmax, netvlad_softmax_fwd_kernel):
    z_k = y_k - max y: the maximum of the computed y is within max_k d_y of the true one, so d_z = d_y + max d_y + U (|z| + ..)
    e_k = __expf(z_k): argument shift s_k = d_z + 2U(|z_k| + 2), relative error rho_k = expm1(s_k)
    sum = sum_k e_k: ceil(K / 64) sequential additions a lane + 6 shuffle steps: depth Ds; its relative error is at most
          r2 = sum_k p_k rho_k + Ds U (1 + sum_k p_k rho_k)   (each term weighs in by its share: an underflowed term adds nothing)
    p_k = e_k * (1 / sum): two roundings:   d_p = p (rho_k + 2U + r2 + 2U rho_k) / (1 - r2) + TINY   (TINY: an e_k flushed to zero)
NeXtVLAD assignment: att = sigmoidf_(attl + bias) (the sum rounds by U |z|: added to the shift of sigmoid_ref), a = mul(p, att).
Backward (softmax recomputed): dot = tsum(mul(p, da), Ds), dz = p * att * (da - dot) = prod(p, att, sub(da, dot)),
datt = dot * att * (1 - att) = prod(dot, att, (1 - att, d_att + U)); the bf16 copy at row stride ld_bf16 is bf16 of the f32 value bit for bit.

NeXtVLAD products (nx_product_kernel; nx_aggregate_mfma_kernel computes the same chain).  Every output element is ONE sequential chain
over l = 0 .. L - 1 from a zero accumulator (the passes of 64 only stage the operand): L additions and L products,
    d_acc = (L + 1) U sum_l |T[l][m] Bm[l][n]|        (depth L, not a tree, + the products' own rounding)
    MODE 0  V = acc - asum * c2:  asum = the chain of a over l: d_asum = L U sum |a|;  V = sub(acc, mul(asum, c2))
    MODE 1  dxe = acc (L = K)
    MODE 2  da = acc - q (L = D):  q[k] = sum_d dV[k][d] c2[k][d] by one wave (nextvlad_q_kernel): depth ceil(D / 64) + 6 and the
            products: d_q = (ceil(D / 64) + 7) U sum |dV c2|;  da = sub(acc, q)
A video without pairs gives V = asum = 0 exactly.  nx_pick() restates the tile choice of the launcher; coverage() lists, per case and
MODE, the tiles, passes and ragged edges the case reaches, and tests/test_cpu_vlad_ref.py asserts the table reaches all of them.

NeXtVLAD elementwise and reductions
    normalize_fwd   s = sum v^2: depth Dn = ceil(D / 64) + 6 and the squares: rel (Dn + 1) U; n = max(sqrtf(s), C12): rel_n = sq's;
                    U = V * (1 / n) = mul(V, div(1, n)).  A zero row: n = C12 exactly and U = 0 exactly.
    normalize_bwd   n is an input.  inv = div(1, n); s = tsum(prod(V, inv, dU), Dn) where n > C12, else exactly 0 (the
                    clamped derivative is dU / n); dV = mul(sub(dU, prod(V, inv, s)), inv)
    gate_fwd        out = mul(h, sigmoid_ref(gl));   gate_bwd: d = dout (+ dout2: one f32 add), dh = mul(d, g),
                    dgl = prod(d, h, g, (1 - g, d_g + U)); the bf16 dgl is bf16 of the f32 value (bit for bit when both are stored)
    center_cast     bf16 of one f32 subtraction: within RB (|ref| + d) + d, d = U |ref|; bit for bit bf16(f32(xe - be))
    bias_logits     out[n] = tsum(mul(be, W[n]), ceil(E / 64) + 6) (+ add[n]: add()); exactly 0 for N <= n < n_out
    wgrad_uncenter  dW = add(dWc, mul(du, be))
    colsum          single pass: wave w adds rows w, w + 16, ..: depth ceil(R / 16) + 16; two passes (ws given and R >= 512): 32 row
                    ranges of rpp = ceil(R / 32) rows, wave w of 4 adds rows w, w + 4, .. of its range: depth ceil(rpp / 4) + 4 + 32

NetVLAD (references = oracle.model_math.netvlad_fwd / _bwd piecewise, in the kernels' cluster-major layout)
    softmax_fwd     the softmax above with one group; softmax_bwd: a is an input: dot = tsum(mul(a, da), ceil(K / 64) + 6), dz = mul(a, sub(da, dot)) + TINY (a subnormal a, flushed or not)
    aggregate_fwd   xb = add(mul(sub(x, mean), mul(rsq(add(var, C3)), gamma)), beta); acc = tsum(mul(a, xb), S) (a chain over the S
                    frames), asum = tsum(a, S), V = sub(acc, mul(asum, c2))
    aggregate_bwd   dx = the chain over k: (K + 1) U sum |a dV|;  da = tsum(mul(dV, sub(bn(x), c2)), 4 ceil(F4 / 64) + 6): a lane adds the
                    four products of a float4 to each other and onto its sum (4 a trip), F4 = F / 4
    dcenters        dc2 = - the chain over b: (B + 1) U sum |asum dV|
    normalize_fwd   n1 = sq(max(tsum(v^2, ceil(F / 64) + 6), C12)); t = tsum(mul(u, u), ceil(K F / 256) + 6 + 3), u = div(V, n1) (a thread's
                    trips, 6 shuffle steps, the 4 wave sums in turn); n2 = sq(max(t, C12)); y = div(V, mul(n1, n2)); Y_bf16 = bf16 of the
                    f32 y bit for bit.  An all-zero cluster: n1 = 1e-6 (to rel), y = 0 exactly; an all-zero video: n2 = 1e-6 as well.
    normalize_bwd   n1, n2 are inputs.  ydy = tsum(mul(div(V, mul(n1, n2)), dY), ceil(K F / 256) + 9); in1 = div(1, n1), u = mul(V, in1),
                    du = div(sub(dY, mul(div(u, n2), ydy)), n2), tk = tsum(mul(u, du), ceil(F / 64) + 6), dV = mul(sub(du, mul(u, tk)), in1)
"""
import math

import numpy as np

from _head_ref import EPS, F32, F64, RB, TINY, U, Case, bf16_bits, bf16_to_f64, exact, f64, prod, ratio, sigmoid, worst  # noqa: F401

C3 = float(F32(1e-3))
C12 = float(F32(1e-12))
CAP = 8192 * 256                                                        # work items of one sweep of a grid-stride kernel (nx_grid / nv_grid)


# ---------------------------------------------------------------------------- pair arithmetic
def ex(v):
    return f64(v), 0.0


def mul(a, b):
    return prod(a, b)


def add(a, b, sign=1.0):
    v = f64(a[0]) + sign * f64(b[0])
    d = f64(a[1]) + f64(b[1])
    return v, d + U * (np.abs(v) + d)


def sub(a, b):
    return add(a, b, -1.0)


def div(a, b):
    av, bv = f64(a[0]), f64(b[0])
    assert np.all(f64(b[1]) < np.abs(bv))
    v = av / bv
    hi = (np.abs(av) + f64(a[1])) / (np.abs(bv) - f64(b[1]))
    return v, hi - np.abs(v) + U * hi


def tsum(t, axis, depth, keepdims=False):
    v, d = f64(t[0]), np.broadcast_to(f64(t[1]), np.shape(t[0]))
    return v.sum(axis=axis, keepdims=keepdims), d.sum(axis=axis, keepdims=keepdims) + depth * U * (np.abs(v) + d).sum(axis=axis, keepdims=keepdims)


def _root(a, power):
    v, d = f64(a[0]), f64(a[1])
    rel = d / v
    r = v ** power
    return r, r * (0.5 * rel * (1.0 + rel) + 2 * U)


def rsq(a):
    return _root(a, -0.5)


def sq(a):
    return _root(a, 0.5)


def sig(z, d_in=0.0):
    """sigmoidf_ of an f32 argument known to d_in (sigmoid_ref of _head_ref with the argument's own error added to the shift)."""
    p = sigmoid(z)
    dz = 2 * U * (np.abs(f64(z)) + 2.0) + d_in
    return p, p * (1.0 - p) * dz + dz * dz + EPS


def bn(x, mean, var, gamma, beta):
    return add(mul(mul(sub(ex(x), ex(mean)), rsq(add(ex(var), ex(C3)))), ex(gamma)), ex(beta))


def wave_depth(n):
    """Depth of a wave's sum over n elements: lane j adds elements j, j + 64, .. in turn, then 6 shuffle steps."""
    return math.ceil(n / 64) + 6


def softmax(y):
    """y = (value, bound) [.., K] -> p (value, bound) [.., K]."""
    yv, yd = f64(y[0]), np.broadcast_to(f64(y[1]), np.shape(y[0]))
    K = yv.shape[-1]
    z = yv - yv.max(axis=-1, keepdims=True)
    dz = yd + yd.max(axis=-1, keepdims=True)
    dz = dz + U * (np.abs(z) + dz)
    rho = np.expm1(dz + 2 * U * (np.abs(z) + 2.0))
    e = np.exp(z)
    p = e / e.sum(axis=-1, keepdims=True)
    w = (p * rho).sum(axis=-1, keepdims=True)
    r2 = w + wave_depth(K) * U * (1.0 + w)
    return p, p * (rho + 2 * U + r2 + 2 * U * rho) / (1.0 - r2) + TINY


def judge(refs, got):
    """refs: name -> Out; got: name -> the buffer the entry wrote into, prefilled with NaN and larger than the output along any axis
    (a guard row behind it, guard columns where the entry takes a row stride; bf16 as bit patterns).  -> name -> ratio per element of
    the output (inf where not finite: no element is exempt) and "name guard" -> inf where a guard lost its NaN."""
    q = {}
    for name, o in refs.items():
        if name not in got or not isinstance(o, Out):
            continue
        g = got[name]
        g = bf16_to_f64(g) if g.dtype == np.uint16 else f64(g)
        assert g.ndim == o.ref.ndim and all(a >= b for a, b in zip(g.shape, o.ref.shape)) and g.size > o.ref.size, name
        body = tuple(slice(0, n) for n in o.ref.shape)
        q[name] = np.where(np.isfinite(g[body]), o.ratio(g[body]), np.inf)
        mask = np.ones(g.shape, bool)
        mask[body] = False
        q[name + " guard"] = np.where(np.isnan(g[mask]), 0.0, np.inf)
    return q


def bits_vs(bf_buf, twin):
    """A bf16 copy (bit patterns, with guards) against bf16 of its f32 twin: inf where a pattern differs or a guard lost its NaN."""
    twin = np.asarray(twin, F32)
    body = tuple(slice(0, n) for n in twin.shape)
    mask = np.ones(bf_buf.shape, bool)
    mask[body] = False
    guard = bf_buf[mask]
    return np.concatenate([np.where(bf_buf[body] == bf16_bits(twin), 0.0, np.inf).reshape(-1), np.where((guard & 0x7FFF) > 0x7F80, 0.0, np.inf)])


class Out:
    """One output of an entry: the reference, its bound, r = RB for a value stored as bf16 alone, and whether zeros must be exact."""

    def __init__(self, ref, d, r=0.0):
        self.ref, self.d, self.r = f64(ref), np.broadcast_to(f64(d), np.shape(ref)), r

    def ratio(self, got):
        return ratio(got, self.ref, self.d, self.r)


# ---------------------------------------------------------------------------- NeXtVLAD products
NX_LC = 64


def ceil_div(a, b):
    return -(-a // b)


def nx_pick(N4, M, B):
    """The tile choice of nx_pick (csrc/evc_nextvlad.hip) -> (DW, MT, ntiles, mtiles)."""
    best, out = -1.0, None
    for dw in (16, 32, 64):
        mt = 8 * (256 // dw)
        nt, mtl = ceil_div(N4, dw), ceil_div(M, mt)
        blocks = float(B) * nt * mtl
        score = (N4 / (float(nt) * dw)) * (M / (float(mtl) * mt)) * (blocks / 512.0 if blocks < 512.0 else 1.0)
        if score > best:
            best, out = score, (dw, mt, nt, mtl)
    return out


def nx_modes(B, P, K, D):
    """(N4, M, L) of the three products at P pairs a video (packed: the longest video's)."""
    Kp = (K + 3) // 4 * 4
    return {0: (D // 4, K, P), 1: (D // 4, P, K), 2: (Kp // 4, P, D)}


def coverage(B, P, K, D):
    """Per MODE what the launch reaches: DW, ntiles, mtiles, passes, ragged (last pass shorter than 64), col_edge (the last column tile has
    fewer than DW lanes), row_edge (the last row tile has fewer than MT rows)."""
    out = {}
    for mode, (N4, M, L) in nx_modes(B, P, K, D).items():
        dw, mt, nt, mtl = nx_pick(N4, M, B)
        out[mode] = dict(DW=dw, MT=mt, ntiles=nt, mtiles=mtl, passes=ceil_div(L, NX_LC), ragged=L % NX_LC != 0,
                         col_edge=N4 - (nt - 1) * dw < dw, row_edge=M - (mtl - 1) * mt < mt)
    return out


def _chain(T, Bm, spec):
    """sum_l over the einsum `spec` as one sequential chain of length L = the contracted extent -> (value, bound)."""
    T, Bm = f64(T), f64(Bm)
    L = T.shape[spec.index("l")]
    return np.einsum(spec, T, Bm), (L + 1) * U * np.einsum(spec, np.abs(T), np.abs(Bm))


def agg_fwd_video(A, X, c2):
    """A [P][K], X [P][D], c2 [K][D] -> (V, d_V, asum, d_asum)."""
    A = f64(A)
    P = A.shape[0]
    acc = _chain(A, X, "lk,ld->kd")
    asum = A.sum(axis=0), P * U * np.abs(A).sum(axis=0)
    V = sub(acc, mul((asum[0][:, None], asum[1][:, None]), ex(c2)))
    if P == 0:
        V = (np.zeros_like(V[0]), np.zeros_like(V[0]))
    return V[0], V[1], asum[0], asum[1]


def agg_bwd_video(A, X, c2, dV):
    """-> (dxe [P][D], d, da [P][K], d)."""
    D = np.shape(X)[1]
    dxe = _chain(np.transpose(f64(A)), dV, "lp,ld->pd")
    qv = (f64(dV) * f64(c2)).sum(axis=1)
    q = qv, (wave_depth(D) + 1) * U * np.abs(f64(dV) * f64(c2)).sum(axis=1)
    da = sub(_chain(np.transpose(f64(X)), np.transpose(f64(dV)), "lp,lk->pk"), (q[0][None, :], q[1][None, :]))
    return dxe[0], dxe[1], da[0], da[1]


def agg_ref(c):
    """A product case (fixed-length or packed: c.off [B+1] in pairs) -> dict of Out: V [B][K][D], asum [B][K], dxe [Ptot][D], da [Ptot][K]."""
    B, K, D = c.B, c.K, c.D
    V, dVv, s, ds = np.zeros((B, K, D)), np.zeros((B, K, D)), np.zeros((B, K)), np.zeros((B, K))
    Pt = int(c.off[-1])
    dxe, ddxe, da, dda = np.zeros((Pt, D)), np.zeros((Pt, D)), np.zeros((Pt, K)), np.zeros((Pt, K))
    for b in range(B):
        lo, hi = int(c.off[b]), int(c.off[b + 1])
        V[b], dVv[b], s[b], ds[b] = agg_fwd_video(c.a[lo:hi], c.xe[lo:hi], c.c2)
        if hi > lo:
            dxe[lo:hi], ddxe[lo:hi], da[lo:hi], dda[lo:hi] = agg_bwd_video(c.a[lo:hi], c.xe[lo:hi], c.c2, c.dV[b])
    return dict(V=Out(V, dVv), asum=Out(s, ds), dxe=Out(dxe, ddxe), da=Out(da, dda))


NX_FIXED = [(2, 5, 2, 7, 12), (2, 7, 3, 65, 68), (3, 30, 8, 64, 288), (2, 30, 8, 128, 288), (1, 64, 16, 130, 260), (512, 1, 1, 32, 256)]
# packed: (G, K, D, frames of every video); the last row: every video as long as S = 7, compared bit for bit with the fixed-length entry
NX_PACKED = [(4, 18, 20, (0, 1, 16, 17, 33, 40)), (1, 40, 100, (0, 1, 16, 17, 33, 40)), (8, 128, 288, (30, 7)), (3, 65, 68, (0, 22, 1, 43, 0)),
             (3, 65, 68, (7, 7))]


def _agg_fill(c, rng, Pt):
    c.a = (rng.random((Pt, c.K)) * rng.random((Pt, 1))).astype(F32)
    c.xe = rng.standard_normal((Pt, c.D)).astype(F32)
    c.c2 = rng.standard_normal((c.K, c.D)).astype(F32)
    c.dV = rng.standard_normal((c.B, c.K, c.D)).astype(F32)
    return c


def agg_case(B, S, G, K, D):
    c = Case()
    c.B, c.S, c.G, c.K, c.D, c.P = B, S, G, K, D, S * G
    c.packed = False
    c.name = "B=%d S=%d G=%d K=%d D=%d" % (B, S, G, K, D)
    c.off = np.arange(B + 1, dtype=np.int64) * c.P
    return _agg_fill(c, np.random.default_rng(9100 + B + 3 * S + 5 * G + 7 * K + D), B * c.P)


def agg_packed_case(G, K, D, ks):
    c = Case()
    c.B, c.G, c.K, c.D, c.ks = len(ks), G, K, D, tuple(ks)
    c.packed = True
    c.T = 48
    c.name = "G=%d K=%d D=%d ks=%s" % (G, K, D, ",".join(str(k) for k in ks))
    c.row_off = np.concatenate([[0], np.cumsum(ks)]).astype(np.int32)
    c.off = c.row_off.astype(np.int64) * G
    c.R, c.max_k = int(c.row_off[-1]), int(max(ks))
    c.P = c.max_k * G
    return _agg_fill(c, np.random.default_rng(9200 + G + 7 * K + D + len(ks)), c.R * G)


# ---------------------------------------------------------------------------- assignment / softmax
ASSIGN_KS = (7, 64, 65, 128, 1024)
ASSIGN_GS = (1, 3)
ASSIGN_R = 5                                                            # R G = 5, 15: the last workgroup of 4 waves is partly idle


def assign_case(K, G, with_bias=True, R=ASSIGN_R):
    """Row 0: logits spread over +-40 inside every group (most of the softmax underflows), its attention logits +-40; row 1: the
    maximum in the LAST cluster (register (K - 1) // 64 of lane (K - 1) % 64); row 2 (K > 64): -50 everywhere but +50 in the last
    cluster, so that a maximum taken over k < 64 alone overflows __expf; the rest N(0, 2)."""
    rng = np.random.default_rng(9300 + 11 * K + G + (1 if with_bias else 0))
    c = Case()
    c.R, c.G, c.K, c.with_bias = R, G, K, with_bias
    c.ld_att, c.ld_bf = G + 2, G + 3
    c.name = "K=%d G=%d %s" % (K, G, "bias" if with_bias else "nobias")
    C = G * K
    c.mean = (rng.standard_normal(C) * 0.1).astype(F32)
    c.var = (0.5 + rng.random(C)).astype(F32)
    c.gamma = (1.0 + 0.2 * rng.standard_normal(C)).astype(F32)
    c.beta = (0.2 * rng.standard_normal(C)).astype(F32)
    y = rng.standard_normal((R, G, K)) * 2.0                            # the logits after batch-norm; act = its inverse, rounded to f32
    y[0] = np.linspace(-40.0, 40.0, G * K).reshape(K, G).T
    y[1, :, K - 1] = 9.0
    if K > 64:                                                          # row 2: a maximum outside register 0 that register 0's alone overflows
        y[2] = -50.0
        y[2, :, K - 1] = 50.0
    sh = (G, K)
    act = (y - c.beta.reshape(sh)) / c.gamma.reshape(sh) * np.sqrt(f64(c.var).reshape(sh) + C3) + c.mean.reshape(sh)
    c.act = act.astype(F32)
    c.attl = np.full((R, c.ld_att), np.nan, F32)
    c.attl[:, :G] = (rng.standard_normal((R, G)) * 2.0).astype(F32)
    c.attl[0, :G] = np.where(np.arange(G) % 2 == 0, 40.0, -40.0)
    c.att_bias = (rng.standard_normal(G) * 0.5).astype(F32) if with_bias else None
    c.da = rng.standard_normal((R, G, K)).astype(F32)
    return c


def assign_ref(c):
    R, G, K = c.R, c.G, c.K
    sh = (G, K)
    y = bn(c.act, c.mean.reshape(sh), c.var.reshape(sh), c.gamma.reshape(sh), c.beta.reshape(sh))
    p = softmax(y)
    zl = f64(c.attl[:, :G])
    if c.att_bias is not None:
        zl = zl + f64(c.att_bias)
        att = sig(zl, U * np.abs(zl))
    else:
        att = sig(zl)
    att3 = att[0][:, :, None], att[1][:, :, None]
    a = mul(p, att3)
    dot = tsum(mul(p, ex(c.da)), 2, wave_depth(K), keepdims=True)
    dz = prod(p, att3, sub(ex(c.da), dot))
    dot2 = dot[0][:, :, 0], dot[1][:, :, 0]
    datt = prod(dot2, att, (1.0 - att[0], att[1] + U))
    return dict(a=Out(*a), dz=Out(*dz), datt=Out(*datt), p=p)


NV_SOFTMAX_KS = (24, 64, 65, 1024)


def nv_softmax_case(K, R=5):
    a = assign_case(K, 1, False, R)
    c = Case()
    c.R, c.K, c.name = R, K, "K=%d" % K
    c.act, c.mean, c.var, c.gamma, c.beta, c.da = a.act.reshape(R, K), a.mean, a.var, a.gamma, a.beta, a.da.reshape(R, K)
    return c


def nv_softmax_ref(c, a_in):
    """a_in: the f32 assignment the backward is fed (an input of its own)."""
    p = softmax(bn(c.act, c.mean, c.var, c.gamma, c.beta))
    dot = tsum(mul(ex(a_in), ex(c.da)), 1, wave_depth(c.K), keepdims=True)
    dz = mul(ex(a_in), sub(ex(c.da), dot))
    return dict(a=Out(*p), dz=Out(dz[0], dz[1] + TINY))                 # (TINY: an assignment below 1e-38 is a subnormal input, flushed or not)


def softmax_f32(act, mean, var, gamma, beta):
    """The plain f32 evaluation (numpy, any order): an input generator for the backward kernels, not an emulation."""
    y = (f64(act) - mean) / np.sqrt(f64(var) + C3) * gamma + beta
    e = np.exp(y - y.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(F32)


# ---------------------------------------------------------------------------- NeXtVLAD elementwise and reductions
NX_NORM_SHAPES = [(2, 7, 12), (2, 5, 65), (1, 3, 288)]


def nx_norm_case(B, K, D):
    """Row (0, 0) all zero (the clamp), row (0, 1) around 1e-20 (its norm is below the clamp too), row (B-1, K-1) large."""
    rng = np.random.default_rng(9400 + B + K + D)
    c = Case()
    c.B, c.K, c.D, c.name = B, K, D, "B=%d K=%d D=%d" % (B, K, D)
    c.V = rng.standard_normal((B, K, D)).astype(F32)
    c.V[0, 0] = 0.0
    c.V[0, 1] *= F32(1e-20)
    c.V[B - 1, K - 1] *= F32(1e4)
    c.dU = rng.standard_normal((B, K, D)).astype(F32)
    v = c.V.astype(F64)
    c.nrm = np.maximum(np.sqrt((v * v).sum(axis=2)), C12).astype(F32)   # the backward's input: the f32 norm, clamped
    c.nrm[0, 0] = F32(1e-12)
    c.nrm[0, 1] = F32(1e-12)
    return c


def nx_norm_ref(c):
    V = f64(c.V)
    Dn = wave_depth(c.D)
    s = (V * V).sum(axis=2)
    rel = (Dn + 1) * U
    n = np.maximum(np.sqrt(s), C12)
    d_n = n * (0.5 * rel * (1 + rel) + 2 * U)
    nn = n[:, :, None], d_n[:, :, None]
    Uo = mul(ex(V), div(ex(1.0), nn))
    nin = f64(c.nrm)[:, :, None]
    inv = div(ex(1.0), ex(nin))
    live = nin > C12
    sdot = tsum(prod(ex(V), inv, ex(c.dU)), 2, Dn, keepdims=True)
    sdot = np.where(live, sdot[0], 0.0), np.where(live, sdot[1], 0.0)
    dV = mul(sub(ex(c.dU), prod(ex(V), inv, sdot)), inv)
    return dict(U=Out(*Uo), norms=Out(n, d_n), dV=Out(*dV))


GATE_NS = (1, 255, 1027, CAP + 259)


def gate_case(n):
    rng = np.random.default_rng(9500 + n % 1000)
    c = Case()
    c.n, c.name = n, "n=%d" % n
    c.h = rng.standard_normal(n).astype(F32)
    c.gl = (rng.standard_normal(n) * 4.0).astype(F32)
    plants = np.array([100.0, -100.0, 0.0, -0.0], F32)
    k = min(n, 4)
    c.gl[:k] = plants[:k]
    if n > 8:
        c.gl[-4:] = plants[::-1]
    c.dout = rng.standard_normal(n).astype(F32)
    c.dout2 = rng.standard_normal(n).astype(F32)
    return c


def gate_ref(c, with_dout2):
    g = sig(c.gl)
    out = mul(ex(c.h), g)
    d = add(ex(c.dout), ex(c.dout2)) if with_dout2 else ex(c.dout)
    dh = mul(d, g)
    dgl = prod(d, ex(c.h), g, (1.0 - g[0], g[1] + U))
    return dict(out=Out(*out), dh=Out(*dh), dgl=Out(*dgl), dgl_bf_alone=Out(dgl[0], dgl[1], RB))


CENTER_SHAPES = [(3, 12), (5, 260), (8161, 1028)]                       # R E / 4 = 9, 325, 2 097 377 = CAP + 225 float4s


def center_case(R, E):
    rng = np.random.default_rng(9600 + R + E)
    c = Case()
    c.R, c.E, c.name = R, E, "R=%d E=%d" % (R, E)
    c.be = rng.standard_normal(E).astype(F32)
    c.xe = (rng.standard_normal((R, E)) * 0.5 + c.be).astype(F32)
    c.xe[0, 0] = c.be[0]                                                # an exact zero
    return c


def center_ref(c):
    ref = f64(c.xe) - f64(c.be)
    return dict(out=Out(ref, U * np.abs(ref), RB))


BIAS_SHAPES = [(1, 1, 1), (3, 65, 8), (8, 130, 8), (5, 1152, 32)]       # (N, E, n_out)


def bias_case(N, E, n_out, with_add):
    rng = np.random.default_rng(9700 + N + E)
    c = Case()
    c.N, c.E, c.n_out, c.name = N, E, n_out, "N=%d E=%d n_out=%d %s" % (N, E, n_out, "add" if with_add else "noadd")
    c.be = rng.standard_normal(E).astype(F32)
    c.W = rng.standard_normal((N, E)).astype(F32)
    c.add = rng.standard_normal(N).astype(F32) if with_add else None
    return c


def bias_ref(c):
    s = tsum(mul(ex(c.be), ex(c.W)), 1, wave_depth(c.E))
    if c.add is not None:
        s = add(s, ex(c.add))
    ref, d = np.zeros(c.n_out), np.zeros(c.n_out)
    ref[:c.N], d[:c.N] = s
    return dict(out=Out(ref, d))


UNCENTER_SHAPES = [(1, 1), (3, 65), (2049, 1025)]                       # N E = 2 100 225 = CAP + 3073


def uncenter_case(N, E):
    rng = np.random.default_rng(9800 + N + E)
    c = Case()
    c.N, c.E, c.name = N, E, "N=%d E=%d" % (N, E)
    c.dWc = rng.standard_normal((N, E)).astype(F32)
    c.du = rng.standard_normal(N).astype(F32)
    c.be = rng.standard_normal(E).astype(F32)
    return c


def uncenter_ref(c):
    return dict(dW=Out(*add(ex(c.dWc), mul(ex(c.du[:, None]), ex(c.be[None, :])))))


COLSUM_CASES = [(1, 1, 1, False), (15, 65, 70, False), (17, 64, 64, False), (511, 130, 130, False), (512, 65, 65, True), (513, 65, 65, True),
                (1000, 65, 65, True), (600, 65, 65, False)]                  # (R, C, ld, ws given)
CS_PARTS = 32


def colsum_case(R, Cc, ld, ws):
    rng = np.random.default_rng(9900 + R + Cc)
    c = Case()
    c.R, c.C, c.ld, c.ws = R, Cc, ld, ws
    c.two_pass = ws and R >= 512
    c.name = "R=%d C=%d ld=%d %s" % (R, Cc, ld, "ws" if ws else "nows")
    c.x = np.full((R, ld), np.nan, F32)
    c.x[:, :Cc] = (rng.standard_normal((R, Cc)) + 0.5).astype(F32)
    return c


def colsum_depth(R, two_pass):
    if two_pass:
        return math.ceil(math.ceil(R / CS_PARTS) / 4) + 4 + CS_PARTS
    return math.ceil(R / 16) + 16


def colsum_ref(c):
    x = f64(c.x[:, :c.C])
    return dict(out=Out(x.sum(axis=0), colsum_depth(c.R, c.two_pass) * U * np.abs(x).sum(axis=0)))


# ---------------------------------------------------------------------------- NetVLAD
NV_SHAPES = [(2, 7, 24, 40), (2, 64, 13, 1028), (2, 17, 5, 260), (1, 33, 257, 8)]     # (B, S, K, F)


def nv_case(B, S, K, F):
    rng = np.random.default_rng(10000 + B + 3 * S + 5 * K + F)
    c = Case()
    c.B, c.S, c.K, c.F, c.name = B, S, K, F, "B=%d S=%d K=%d F=%d" % (B, S, K, F)
    c.r = rng.standard_normal((B, S, F)).astype(F32)
    c.mean = (rng.standard_normal(F) * 0.1).astype(F32)
    c.var = (0.5 + rng.random(F)).astype(F32)
    c.gamma = (1.0 + 0.2 * rng.standard_normal(F)).astype(F32)
    c.beta = (0.2 * rng.standard_normal(F)).astype(F32)
    raw = rng.random((B, S, K)) ** 3
    c.a = (raw / raw.sum(axis=2, keepdims=True)).astype(F32)
    c.c2 = (rng.standard_normal((K, F)) / math.sqrt(F)).astype(F32)
    c.dV = rng.standard_normal((B, K, F)).astype(F32)
    c.asum = c.a.astype(F64).sum(axis=1).astype(F32)                    # the input of dcenters
    return c


def nv_xbn(c):
    """x_bn as netvlad_aggregate_fwd forms it: (x - mean) * (rsqrtf(var + C3) * gamma) + beta."""
    return add(mul(sub(ex(c.r), ex(c.mean)), mul(rsq(add(ex(c.var), ex(C3))), ex(c.gamma))), ex(c.beta))


def nv_agg_ref(c):
    B, S, K, F = c.B, c.S, c.K, c.F
    xb = nv_xbn(c)
    t = mul((f64(c.a)[:, :, :, None], 0.0), (xb[0][:, :, None, :], xb[1][:, :, None, :]))      # [B][S][K][F]
    acc = tsum(t, 1, S)
    asum = tsum(ex(c.a), 1, S)
    V = sub(acc, mul((asum[0][:, :, None], asum[1][:, :, None]), ex(c.c2)))
    dx = np.einsum("bsk,bkf->bsf", f64(c.a), f64(c.dV)), (K + 1) * U * np.einsum("bsk,bkf->bsf", np.abs(f64(c.a)), np.abs(f64(c.dV)))
    xb3 = bn(c.r, c.mean, c.var, c.gamma, c.beta)
    diff = sub((xb3[0][:, :, None, :], xb3[1][:, :, None, :]), ex(c.c2))
    da = tsum(mul(ex(c.dV[:, None, :, :]), diff), 3, 4 * math.ceil((F // 4) / 64) + 6)
    return dict(V=Out(*V), asum=Out(*asum), dx=Out(*dx), da=Out(*da), xb=xb[0])


NV_DC_SHAPES = [(3, 7, 24), (1, 2049, 4100)]                            # (B, K, F): K F / 4 = 2 100 225 = CAP + 3073 float4s at B = 1


def nv_dc_case(B, K, F):
    rng = np.random.default_rng(10100 + B + K + F)
    c = Case()
    c.B, c.K, c.F, c.name = B, K, F, "B=%d K=%d F=%d" % (B, K, F)
    c.asum = (rng.random((B, K)) * 3.0).astype(F32)
    c.dV = rng.standard_normal((B, K, F)).astype(F32)
    return c


def nv_dc_ref(c):
    t = f64(c.asum)[:, :, None] * f64(c.dV)
    return dict(dc2=Out(-t.sum(axis=0), (c.B + 1) * U * np.abs(t).sum(axis=0)))


def nv_norm_case(B, S, K, F):
    """The V of an aggregation case with video 0's cluster 1 all zero and, where B > 1, the last video all zero."""
    c = nv_case(B, S, K, F)
    rng = np.random.default_rng(10200 + K + F)
    c.V = (rng.standard_normal((B, K, F)) * (0.1 + rng.random((B, K, 1)))).astype(F32)
    c.V[0, 1] = 0.0
    if B > 1:
        c.V[B - 1] = 0.0
    c.dY = rng.standard_normal((B, K, F)).astype(F32)
    v = c.V.astype(F64)
    n1 = np.sqrt(np.maximum((v * v).sum(axis=2), C12))
    u = v / n1[:, :, None]
    c.n1 = n1.astype(F32)                                               # the backward's inputs
    c.n2 = np.sqrt(np.maximum((u * u).sum(axis=(1, 2)), C12)).astype(F32)
    return c


def nv_norm_ref(c):
    B, K, F = c.B, c.K, c.F
    V = f64(c.V)
    s = tsum(mul(ex(V), ex(V)), 2, wave_depth(F))
    s = np.maximum(s[0], C12), s[1]
    n1 = sq(s)
    n13 = n1[0][:, :, None], n1[1][:, :, None]
    u = div(ex(V), n13)
    D2 = math.ceil(K * F / 256) + 9
    t = tsum(mul(u, u), (1, 2), D2)
    t = np.maximum(t[0], C12), t[1]
    n2 = sq(t)
    n23 = n2[0][:, None, None], n2[1][:, None, None]
    y = div(ex(V), mul(n13, n23))
    # backward, from the f32 n1 / n2 it is fed
    i1, i2 = ex(f64(c.n1)[:, :, None]), ex(f64(c.n2)[:, None, None])
    ydy = tsum(mul(div(ex(V), mul(i1, i2)), ex(c.dY)), (1, 2), D2, keepdims=True)
    in1 = div(ex(1.0), i1)
    uu = mul(ex(V), in1)
    du = div(sub(ex(c.dY), mul(div(uu, i2), ydy)), i2)
    tk = tsum(mul(uu, du), 2, wave_depth(F), keepdims=True)
    dV = mul(sub(du, mul(uu, tk)), in1)
    return dict(n1=Out(*n1), n2=Out(*n2), Y=Out(*y), dV=Out(*dV))
