"""Float64 references of the clip + Adam update kernels, each with a derived per-element bound on |got - ref|, an f32 emulation and a case
generator.  numpy only (the e4m3 image alone goes through torch's CPU float8_e4m3fn cast).  Used by tests/test_cpu_optim_ref.py (the references
against the oracle, the emulations inside every bound, planted faults outside it, sharpness) and tests/test_gpu_optim_parity.py (the kernels).
The companion of tests/_head_ref.py: that file covers what turns the last state into a loss and the first gradient, this one the last link of a
training step - what turns a gradient into new weights, new moments and every operand image the next forward and backward read:

    csrc/evc_elementwise.hip (a8 + a9)   evc_grad_sqnorm, evc_clip_adam_step, evc_clip_adam_small
    csrc/evc_optim.hip                   evc_sqnorm2_partials, evc_lstm_adam_fused, evc_adam2d_fused
    csrc/evc_gemm_tn.hip                 moe_update_kernel: evc_moe_grad_update, _phase, _apply, _wide
    csrc/evc_moe_norms.hip               evc_gram_slabs + evc_moe_grad_norms (the clip norm from Gram matrices of the factors; derivation at gram_norm_ref)

Every reference is fed the kernel's own f32 / bf16 inputs and its f32 scalars as exact float64 numbers (Hyper: b1 = f32(0.9), 1.f - b1 and 1.f - b2
as f32 evaluates them, f32(eps), f32(lr_t), f32(l2), f32(clip)), so a correct kernel differs from it only by its own roundings.  Where an entry
READS a squared norm (evc_clip_adam_step, evc_moe_grad_update_apply, phase 2) the reference uses that f32 value as given: an error of the norm
belongs to the norm entry's own check.  No measured constant enters a bound.

Notation (as tests/_head_ref.py)
--------------------------------
    U = 2^-24   f32 unit roundoff: one f32 operation or one f32 store moves a value by U of its magnitude
    an f32 sum of terms in ANY order whose tree has depth D is off by at most D U sum|terms|
    IEEE division and sqrtf (clip / max(sqrtf(ss), clip): the library is built without fast-math) are correctly rounded: U
    rcpf_ (v_rcp_f32) and sqrtf_ (v_sqrt_f32): 1 ulp = 2U relative, as evc_common.h states and the LSTM files model rcpf_
    prod((v_1, d_1), .., (v_k, d_k)): a product of k factors formed with k - 1 roundings (_head_ref.prod; every second-order term kept)
    FLOOR = 2^-126: the absolute error of an f32 product whose result is subnormal or flushed to zero.  It is added wherever a product can underflow
    (gc, both moment terms, the step): whether the hardware keeps or flushes a subnormal, the result is within FLOOR of the true product.

The chain (adam_ref), per element; p, m, v are exact f32 inputs, g is known to d_g (0 for a stored gradient)
---------------------------------------------------------------------------------------------------------
Clip scale (scale_ref).  scale = clip / max(sqrtf(ss), clip), exactly 1 when clip <= 0.  ss is known to rel relative: 0 when it is an input, (D + 1) U
when the kernel sums g^2 itself over a tree of depth D (one rounding a square, D additions of non-negative terms; exactly: (1 + U)^(D+1) - 1).  Then
    nrm = sqrt(ss)         d_nrm = nrm rel (1 + rel) / 2 + U (nrm + ..)                 (sqrt halves a relative error; sqrtf is correctly rounded)
    mx  = max(nrm, clip)   d_mx <= d_nrm: max is 1-Lipschitz, so the bound holds on both sides of the clip, and the kernel's mx is >= clip
    s   = clip / mx        d_s = clip d_nrm / (mx max(mx - d_nrm, clip)) + U (s + ..)   (the division is correctly rounded)
    nrm + d_nrm <= clip:   the kernel's fmaxf returns clip itself and clip / clip = 1 exactly: s = 1, d_s = 0.
Gradient term.  t = l2 p (U |t|), a = g + t (U (|a| + d_g + d_t); no rounding at all when l2 = 0: g + 0 = g), gc = a s:
    d_a = d_g + U |l2 p| + [l2 != 0] U (|a| + d_g + U |l2 p|);    (gc, d_gc) = prod((a, d_a), (s, d_s)) + FLOOR
Under an fma (l2 p + g in one rounding) the error is smaller; every bound below likewise counts BOTH roundings of a two-term sum, so it holds whether
or not hipcc contracts the sum into an fma.
Moments, two-term sums bounded on the sum of the magnitudes of their terms (b1 m and (1 - b1) gc cancel where the gradient turns against its average):
    m' = T1 + T2, T1 = b1 m (U |T1|), (T2, d_T2) = prod((1 - b1, 0), (gc, d_gc)):   d_m = U |T1| + d_T2 + U (|T1| + |T2| + U |T1| + d_T2) + FLOOR
    v' = V1 + V2, V1 = b2 v (U |V1|), (V2, d_V2) = prod((1 - b2, 0), (gc, d_gc), (gc, d_gc)) + FLOOR  (the kernel's (1 - b2) * gc * gc, left to right; gc * gc
         underflows in f32 below |gc| ~ 1e-19: V2 is then known to FLOOR absolutely and to nothing relatively):
                                                                                     d_v = U |V1| + d_V2 + U (|V1| + |V2| + U |V1| + d_V2) + FLOOR
Denominator.  den = sqrtf_(v') + eps.  |sqrt(a) - sqrt(b)| = |a - b| / (sqrt a + sqrt b) <= sqrt|a - b|, so the error of v' enters through
    d_sq = min(d_v / (sqrt v' + sqrt max(v' - d_v, 0)), sqrt d_v)    (for v' >> d_v this is d_v / (2 sqrt v'); v' near 0 does not blow the bound up)
         + 2U (sqrt v' + d_sq)                                       (v_sqrt_f32 at 1 ulp)
         + [v' - d_v < 2^-125] 2^-63                                 (a subnormal v': see below)
    d_den = d_sq + U (den + d_sq)
A subnormal argument of v_sqrt_f32.  Neither the project nor the guides state what v_sqrt_f32 returns for a subnormal input (the compiler's own sqrtf
scales such inputs first, which suggests it flushes them).  No measurement is needed: for v' < 2^-125 anything between 0 and sqrt(2^-126) = 2^-63 =
1.1e-19 is inside the bound, eleven orders below any eps in use.
Reciprocal and step.  r = rcpf_(den) at 1 ulp; lr_t * m' * r is evaluated left to right; the final subtraction rounds once:
    d_r = d_den / (den (den - d_den)) + 2U / (den - d_den)
    (step, d_step) = prod((lr_t, 0), (m', d_m), (r, d_r)) + FLOOR;     p' = p - step:   d_p = d_step + U (|p'| + d_step)
g = m = v = 0 (and l2 = 0): gc = 0, m' = v' = 0, den = eps, step = lr_t * 0 * r = 0 and p' = p bit for bit; the tests assert that separately.
A value stored as f32 IS the kernel's f32 result: limit = d.

Recomputed MoE gradient tile (moe_ref).  g = dlogits^T x over the batch rows is an MFMA accumulation of bf16 factors in f32.  The reference is the
float64 product of the bf16 factors; in any order of the `rows` terms the f32 result is within d_g = rows U sum_r |a_r| |x_r| of it (rows <= 96 here).
d_g is carried through the chain above.  Pad rows / columns of a ragged tile are masked by the kernel and never stored.

Shadows and images carry no tolerance.  They are exact functions of the f32 p the kernel itself stored, computed on the host from that p:
    bf16 shadow                 round to nearest even bit arithmetic (bf16_bits)
    f16 image                   numpy astype(float16); wide layout [f16(Wx) | f16(f16(Wx) / 64) | f16((Wx - f16(Wx)) * 64) (nseg blocks) | f16(Wh)], in f32 numpy
    e4m3 image                  clamp to +-448, torch's CPU float8_e4m3fn cast: [lo(first hi_cols) | hi(first hi_cols) | lo(rest) | hi(rest) if hi_tail] of the columns
                                from col0, lo = (p - f16(p)) 2^lo_exp, hi = p 2^hi_exp
    transposed shadow           index map only: LSTM kernel column u * 4 + g <- row g * H + u; plain weight: the transpose, rows R .. round_up(R, 64) zero
    [hi | lo] split-bf16 image  hi = bf16(p), lo = bf16(p - hi)

Norm sums: the depth D of each kernel's real tree
-------------------------------------------------
Each element's square is a product (sq_terms: with an l2 term a = g + l2 p carries U |l2 p| + U |a| into it), then
    |sum_got - sum_ref| <= sum d_sq + D U (sum (sq + d_sq) + |value the sum is added onto|)
D = trips per thread x 4 on the float4 paths (four squares a trip join the running sum) + 1 for a scalar tail + 6 shuffle steps + the waves of the
block + what joins the block results:
    evc_grad_sqnorm (sqnorm_depth)     grid = min(ceil(n / 4 / 256), 512) blocks of 4 waves, the grid's float atomics in any order onto sums:
                                       D = 4 ceil(n4 / (256 grid)) + [n % 4] + 6 + 4 + grid
        n = 1, 3        0 + 1 + 10 + 1   = 12           n = 1027      4 + 1 + 10 + 1   = 16
        n = 262147      4 + 1 + 10 + 256 = 271          n = 1100003   12 + 1 + 10 + 512 = 535    (a third strided trip)
    evc_sqnorm2_partials (partials_depth)   1024 blocks own float4 i with (i / 256) % 1024 = block, block 0 the tail; one more block sums the second tensor:
                                       D = 4 ceil(n4 / 262144) + 1 + 6 + 4          na = 4: 15;  1027: 15;  3153923: 4 x 4 + 11 = 27;   nb = 64: 15;  4096: 4 x 4 + 11 = 27
    sum_partials (evc_lstm_adam_fused, evc_adam2d_fused)   16 partials a lane in index order + 6 shuffle steps:  D_w = D_partials + 22;  the bias: D_b = D_partials
        every LSTM / 2-D case below has at most 262144 float4 (one trip): D_w = 4 + 11 + 22 = 37, except the 2-D weight (1024, 3080): 788480 float4, 4 trips:
        D_w = 16 + 11 + 22 = 49.  The bias block walks its tensor alone: R = 64, 192, 256: D_b = 15;  R = 1088 (272 float4, two trips): D_b = 8 + 11 = 19
    evc_clip_adam_small (small_depth)  one block of 16 waves a tensor:  D = ceil(n / 1024) + 6 + 16        (n <= 1024: 23;  1025, 2049: 24, 25;  4099: 27;  8193: 31;  12288: 34;  32768: 54)
    moe_update_kernel pass 1 / the |W|^2 of pass 2 (moe_depth)   a 128 x 128 tile on 512 threads: 32 elements a thread in turn + 6 + 8 waves, then
        moe_update_finalize_kernel: ceil(tiles / 1024) + 6 + 16, + 1 where it adds onto sums:   D = 32 + 14 + 1 + 22 + 1 = 70 for every case here
    evc_moe_grad_norms (gram_depths)   <GA, GX>: min(R^2 / 256, 256) blocks, ceil(R^2 / (256 blocks)) trips + 6 + 4:  R = 32: 4 blocks, 11;  R = 96: 36 blocks, 11
                                       <A, logits - bias>: one block per (row, quarter of the V columns): ceil(56 / 256) + 6 + 4 = 11 at V = 200
                                       the slabs of a Gram matrix are added in turn (depth S <= 4); the block partials meet in double precision
"""
import math

import numpy as np

from _bptt_ref import U, bf16_bits, bf16_to_f64  # noqa: F401
from _head_ref import F32, F64, Case, exact, f64, prod, ratio, worst  # noqa: F401

FLOOR = 2.0 ** -126
SQRT_FLOOR = 2.0 ** -63


class Hyper:
    """The f32 scalars of one launch as exact float64 numbers."""

    def __init__(self, lr_t=3e-4, b1=0.9, b2=0.999, eps=1e-8, l2=0.0, clip=1.0):
        self.lr, self.b1, self.b2, self.eps, self.l2, self.clip = (float(F32(x)) for x in (lr_t, b1, b2, eps, l2, clip))
        self.omb1 = float(F32(1.0) - F32(b1))
        self.omb2 = float(F32(1.0) - F32(b2))

    def but(self, **kw):
        h = Hyper(self.lr, self.b1, self.b2, self.eps, self.l2, self.clip)
        for k, x in kw.items():
            assert hasattr(h, k)
            setattr(h, k, float(F32(x)))
        h.omb1 = float(F32(1.0) - F32(h.b1))
        h.omb2 = float(F32(1.0) - F32(h.b2))
        return h

    def kw(self):
        return dict(beta1=self.b1, beta2=self.b2, eps=self.eps)


def ss_rel(D):
    """Relative error of an f32 sum of f32 squares over a tree of depth D."""
    return math.expm1((D + 1) * math.log1p(U))


def scale_ref(ss, clip, rel=0.0):
    if clip <= 0.0:
        return 1.0, 0.0
    nrm = math.sqrt(float(ss))
    d_n = nrm * 0.5 * rel * (1.0 + rel)
    d_n += U * (nrm + d_n)
    if nrm + d_n <= clip:
        return 1.0, 0.0
    mx = max(nrm, clip)
    s = clip / mx
    d_s = clip * d_n / (mx * max(mx - d_n, clip))
    return s, d_s + U * (s + d_s)


def adam_ref(p, g, m, v, hp, s=1.0, d_s=0.0, d_g=0.0, l2=None):
    """-> dict p, m, v, d_p, d_m, d_v (float64, the shape of p)."""
    p, g, m, v, d_g = f64(p), f64(g), f64(m), f64(v), f64(d_g)
    l2 = hp.l2 if l2 is None else l2
    t = l2 * p
    d_t = U * np.abs(t)
    a = g + t
    d_a = d_g + d_t + (U * (np.abs(a) + d_g + d_t) if l2 != 0.0 else 0.0)
    gc, d_gc = prod((a, d_a), (s, d_s))
    d_gc = d_gc + FLOOR
    T1 = hp.b1 * m
    T2, d_T2 = prod((hp.omb1, 0.0), (gc, d_gc))
    mn = T1 + T2
    d_m = U * np.abs(T1) + d_T2 + U * (np.abs(T1) + np.abs(T2) + U * np.abs(T1) + d_T2) + FLOOR
    V1 = hp.b2 * v
    V2, d_V2 = prod((hp.omb2, 0.0), (gc, d_gc), (gc, d_gc))
    d_V2 = d_V2 + FLOOR
    vn = V1 + V2
    d_v = U * np.abs(V1) + d_V2 + U * (np.abs(V1) + np.abs(V2) + U * np.abs(V1) + d_V2) + FLOOR
    sq = np.sqrt(vn)
    lo = np.sqrt(np.maximum(vn - d_v, 0.0))
    d_sq = np.minimum(d_v / (sq + lo + 1e-300), np.sqrt(d_v))
    d_sq = d_sq + 2 * U * (sq + d_sq) + np.where(vn - d_v < 2.0 ** -125, SQRT_FLOOR, 0.0)
    den = sq + hp.eps
    d_den = d_sq + U * (den + d_sq)
    r = 1.0 / den
    d_r = d_den / (den * (den - d_den)) + 2 * U / (den - d_den)
    step, d_step = prod((hp.lr, 0.0), (mn, d_m), (r, d_r))
    d_step = d_step + FLOOR
    pn = p - step
    return dict(p=pn, m=mn, v=vn, d_p=d_step + U * (np.abs(pn) + d_step), d_m=d_m, d_v=d_v, gc=gc, step=step)


# ---------------------------------------------------------------------------- norm sums
def sq_terms(g, p=None, l2=0.0):
    """(g + l2 p)^2 per element with its bound."""
    g = f64(g)
    if p is None or l2 == 0.0:
        a, d_a = g, np.zeros_like(g)
    else:
        t = l2 * f64(p)
        a = g + t
        d_a = U * np.abs(t) + U * (np.abs(a) + U * np.abs(t))
    sq, d = prod((a, d_a), (a, d_a))
    return sq, d + FLOOR


def sum_bound(sq, d_sq, D, onto=0.0):
    return float(np.sum(d_sq) + D * U * (np.sum(sq + d_sq) + abs(onto)))


def sqnorm_grid(n):
    nb = (n // 4 + 255) // 256
    return max(1, min(nb, 512))


def sqnorm_depth(n):
    grid = sqnorm_grid(n)
    return 4 * math.ceil((n // 4) / (256 * grid)) + (1 if n % 4 else 0) + 6 + 4 + grid


def sqnorm_ref(g, p, l2, before=(0.0, 0.0)):
    """evc_grad_sqnorm: -> (sums [2], bounds [2]); sums[1] (the weights squared) is touched only when p is given."""
    n = np.size(g)
    D = sqnorm_depth(n)
    sq, d = sq_terms(g, p, l2)
    out = [before[0] + sq.sum(), before[1]]
    bnd = [sum_bound(sq, d, D, before[0]), 0.0]
    if p is not None:
        pq, dq = sq_terms(p)
        out[1] = before[1] + pq.sum()
        bnd[1] = sum_bound(pq, dq, D, before[1])
    return np.array(out), np.array(bnd)


NBA = 1024                                                               # EVC_SQN_BLOCKS


def partials_depth(n, strided=True):
    return 4 * math.ceil((n // 4) / (256 * (NBA if strided else 1))) + 1 + 6 + 4


def partials_owner(n):
    """The block that owns element k of the first tensor."""
    k = np.arange(n)
    return np.where(k < (n // 4) * 4, (k // 4 // 256) % NBA, 0)


def partials_ref(a, b=None):
    """evc_sqnorm2_partials: -> (part [1024 or 1025], bound)."""
    a = f64(a).reshape(-1)
    sq, d = sq_terms(a)
    own = partials_owner(a.size)
    D = partials_depth(a.size)
    part = np.bincount(own, weights=sq, minlength=NBA)
    bnd = np.bincount(own, weights=d, minlength=NBA) + D * U * np.bincount(own, weights=sq + d, minlength=NBA)
    if b is not None:
        sqb, db = sq_terms(f64(b).reshape(-1))
        part = np.append(part, sqb.sum())
        bnd = np.append(bnd, sum_bound(sqb, db, partials_depth(np.size(b), False)))
    return part, bnd


def small_depth(n):
    return math.ceil(n / 1024) + 6 + 16


MOE_DEPTH = 32 + 6 + 8 + 1 + 6 + 16 + 1


# ---------------------------------------------------------------------------- f32 emulations
def _f32(a):
    return np.asarray(a, dtype=F32)


def _butterfly(x):
    """wave_sum over the last axis (64 lanes): v += shfl_xor(v, o) for o = 32 .. 1."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = (x + x[..., lane ^ o]).astype(F32)
    return x[..., 0]


def _block_sum(per_thread):
    """per_thread [.., T] (T a multiple of 64) -> [..]: butterflies inside a wave, the wave totals in order."""
    w = _butterfly(per_thread.reshape(per_thread.shape[:-1] + (-1, 64)))
    t = np.zeros(w.shape[:-1], F32)
    for i in range(w.shape[-1]):
        t = (t + w[..., i]).astype(F32)
    return t


def _quad_sq(x4):
    """[.., 4] f32 -> a a + b b + c c + d d, left to right."""
    q = (x4 * x4).astype(F32)
    return (((q[..., 0] + q[..., 1]).astype(F32) + q[..., 2]).astype(F32) + q[..., 3]).astype(F32)


def _strided_sum(val4, tail, blocks, threads=256):
    """val4 [n4] the float4 terms in index order, tail [< 4] scalar terms (block 0, threads 0 ..) -> per-thread sums [blocks][threads]: thread t of block b
    adds the terms b * threads + t + j * blocks * threads in turn, then its tail term."""
    n4 = val4.size
    per = blocks * threads
    J = max(1, math.ceil(n4 / per))
    pad = np.zeros(J * per, F32)
    pad[:n4] = val4
    pad = pad.reshape(J, blocks, threads)
    s = np.zeros((blocks, threads), F32)
    for j in range(J):
        s = (s + pad[j]).astype(F32)
    s[0, :tail.size] = (s[0, :tail.size] + tail).astype(F32)
    return s


def partials_emul(a, b=None):
    a = _f32(a).reshape(-1)
    n4 = a.size // 4
    tl = a[n4 * 4:]
    part = _block_sum(_strided_sum(_quad_sq(a[:n4 * 4].reshape(-1, 4)), (tl * tl).astype(F32), NBA))
    if b is not None:
        b = _f32(b).reshape(-1)
        m4 = b.size // 4
        tb = b[m4 * 4:]
        part = np.append(part, _block_sum(_strided_sum(_quad_sq(b[:m4 * 4].reshape(-1, 4)), (tb * tb).astype(F32), 1)))
    return part.astype(F32)


def sum_partials_emul(part):
    """sum_partials(part, 1024): 16 a lane in index order, one butterfly."""
    s = np.zeros(64, F32)
    for j in range(NBA // 64):
        s = (s + _f32(part[j * 64:(j + 1) * 64])).astype(F32)
    return F32(_butterfly(s[None, :])[0])


def sqnorm_emul(g, p, l2, before=(0.0, 0.0), order=None):
    """evc_grad_sqnorm; the atomics land in block order (or `order`, a permutation of the blocks)."""
    g = _f32(g).reshape(-1)
    n = g.size
    grid = sqnorm_grid(n)
    n4 = n // 4
    pv = np.zeros_like(g) if p is None else _f32(p).reshape(-1)
    a = (g + (F32(l2) * pv).astype(F32)).astype(F32)
    out = [F32(before[0]), F32(before[1])]
    for k, x in enumerate((a, pv)):
        if k == 1 and p is None:
            break
        tl = x[n4 * 4:]
        blk = _block_sum(_strided_sum(_quad_sq(x[:n4 * 4].reshape(-1, 4)), (tl * tl).astype(F32), grid))
        for i in (range(grid) if order is None else order):
            out[k] = F32(out[k] + blk[i])
    return np.array(out, F32)


def small_sum_emul(g):
    g = _f32(g).reshape(-1)
    return F32(_block_sum(_strided_sum((g * g).astype(F32), np.zeros(0, F32), 1, 1024))[0])


def scale_emul(ss32, clip):
    if clip <= 0.0:
        return F32(1.0)
    c = F32(clip)
    return F32(c / max(np.sqrt(F32(ss32)), c))


def _fma(a, b, c):
    return (f64(a) * f64(b) + f64(c)).astype(F32)


def _ulp(x, mode):
    """mode 0: as numpy rounds; 1: every even element one ulp up and every odd one down (a 1-ulp intrinsic at its worst)."""
    if not mode:
        return x
    x = np.atleast_1d(x).copy()
    flat = x.reshape(-1)
    flat[0::2] = np.nextafter(flat[0::2], F32(np.inf))
    flat[1::2] = np.nextafter(flat[1::2], F32(-np.inf))
    return x


def adam_emul(p, g, m, v, hp, scale32=1.0, fma=False, ulp=0, g_l2=True):
    """The kernels' operation order in f32 -> (p, m, v) f32."""
    p, g, m, v = _f32(p), _f32(g), _f32(m), _f32(v)
    l2, s = F32(hp.l2 if g_l2 else 0.0), F32(scale32)
    b1, b2, omb1, omb2, eps, lr = F32(hp.b1), F32(hp.b2), F32(hp.omb1), F32(hp.omb2), F32(hp.eps), F32(hp.lr)
    with np.errstate(under="ignore"):
        a = _fma(l2, p, g) if fma else (g + (l2 * p).astype(F32)).astype(F32)
        gc = (a * s).astype(F32)
        t2 = (omb1 * gc).astype(F32)
        w2 = ((omb2 * gc).astype(F32) * gc).astype(F32)
        if fma:
            mn, vn = _fma(b1, m, t2), _fma(b2, v, w2)
        else:
            mn, vn = ((b1 * m).astype(F32) + t2).astype(F32), ((b2 * v).astype(F32) + w2).astype(F32)
        den = (_ulp(np.sqrt(vn), ulp) + eps).astype(F32)
        r = _ulp((F32(1.0) / den).astype(F32), ulp)
        lm = (lr * mn).astype(F32)
        pn = _fma(-lm, r, p) if fma else (p - (lm * r).astype(F32)).astype(F32)
    return pn.reshape(p.shape), mn.reshape(p.shape), vn.reshape(p.shape)


# ---------------------------------------------------------------------------- shadows and images: exact functions of the stored p
def e4m3_bytes(x):
    """clamp to +-448, torch's CPU float8_e4m3fn cast -> uint8."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(np.clip(_f32(x), F32(-448.0), F32(448.0))))
    return t.to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def f16_of(p):
    with np.errstate(over="ignore"):
        return _f32(p).astype(np.float16)


def f16_wide(p, nin, nseg):
    """[f16(Wx) | f16(f16(Wx) / 64) | f16((Wx - f16(Wx)) * 64) (the first nseg blocks) | f16(Wh)]."""
    p = _f32(p)
    h = f16_of(p)
    hf = h.astype(F32)
    blocks = [h[:, :nin]]
    if nseg >= 2:
        blocks.append((hf[:, :nin] * F32(1.0 / 64.0)).astype(F32).astype(np.float16))
    if nseg >= 3:
        blocks.append(((p[:, :nin] - hf[:, :nin]).astype(F32) * F32(64.0)).astype(F32).astype(np.float16))
    return np.concatenate(blocks + [h[:, nin:]], axis=1)


def fp8_image(p, col0, hi_cols, lo_exp, hi_exp, hi_tail=False):
    """[lo(first hi_cols) | hi(first hi_cols) | lo(rest) | hi(rest) if hi_tail] of p[:, col0:]."""
    p = _f32(p)[:, col0:]
    hf = f16_of(p).astype(F32)
    lo = e4m3_bytes(((p - hf).astype(F32) * F32(2.0 ** lo_exp)).astype(F32))
    hi = e4m3_bytes((p * F32(2.0 ** hi_exp)).astype(F32))
    parts = [lo[:, :hi_cols], hi[:, :hi_cols], lo[:, hi_cols:]]
    if hi_tail:
        parts.append(hi[:, hi_cols:])
    return np.concatenate(parts, axis=1)


def lstm_transposed(bits, H):
    """bits [4H][C] -> [C][4H]: column u * 4 + g <- row g * H + u."""
    C = bits.shape[1]
    return np.ascontiguousarray(bits.reshape(4, H, C).transpose(2, 1, 0).reshape(C, 4 * H))


def split_hilo(p):
    """-> (hi, lo) bf16 bit patterns: hi = bf16(p), lo = bf16(p - hi) (p - hi is exact in f32)."""
    p = _f32(p)
    hi = bf16_bits(p)
    return hi, bf16_bits((p.astype(F64) - bf16_to_f64(hi)).astype(F32))


# ---------------------------------------------------------------------------- cases
REGIMES = ("first_step", "g0", "all0", "eps_dominates", "underflow", "v_large")


def _set(c, idx, kind, rng):
    k = len(idx)
    if kind == "first_step":
        c.m[idx] = 0.0
        c.v[idx] = 0.0
    elif kind == "g0":
        c.g[idx] = 0.0
    elif kind == "all0":
        c.g[idx] = 0.0
        c.m[idx] = 0.0
        c.v[idx] = 0.0
    elif kind == "eps_dominates":
        c.g[idx] = (rng.choice([-1.0, 1.0], k) * rng.uniform(0.5e-9, 2e-9, k)).astype(F32)
        c.m[idx] = 0.0
        c.v[idx] = 0.0
    elif kind == "underflow":
        c.g[idx] = (rng.choice([-1.0, 1.0], k) * rng.uniform(0.5e-20, 2e-20, k)).astype(F32)
        c.m[idx] = 0.0
        c.v[idx] = 0.0
    elif kind == "v_large":
        c.v[idx] = rng.uniform(0.5e4, 2e4, k).astype(F32)


def plant(c, rng, row=None):
    """The regimes of REGIMES at fixed index ranges of the flattened tensors: from 4096 elements on all six, each 6 elements wide, at the start (from
    element 1: across float4 lanes), in the middle and at the very end (the last tile, row and float4 lane, the scalar tail included).  Smaller
    tensors hold as many as fit: n >= 512 two elements of each at both ends, n >= 64 one of each at the end, n >= 5 the two whose update stays of the order of lr_t (first step, g = 0
    with moments), n = 2, 3 the first step alone.  c.where[kind] lists the elements."""
    n = c.p.size
    for a in ("p", "g", "m", "v"):
        setattr(c, a, getattr(c, a).reshape(-1))
    c.where = {k: [] for k in REGIMES}
    if n >= 4096:
        w, starts = 6, (1, n // 2 - 17, n - 6 * 6)
    elif n >= 512:
        w, starts = 2, (1, n - 2 * 6)
    elif n >= 64:
        w, starts = 1, (n - 6,)
    else:
        w, starts = 1, ()
        if n >= 2:
            c.where["first_step"] = [n - 1]
        if n >= 5:
            c.where["g0"] = [1]
    for s0 in starts:
        for r, kind in enumerate(REGIMES):
            c.where[kind] += list(range(s0 + r * w, s0 + (r + 1) * w))
    for kind in REGIMES:
        c.where[kind] = np.array(c.where[kind], np.int64)
        if c.where[kind].size:
            _set(c, c.where[kind], kind, rng)


def bulk(shape, seed, gs=0.02, ms=1e-3, vs=1e-5):
    """|p| <= 0.3, g ~ gs, m ~ ms = 1e-3, sqrt(v) ~ sqrt(vs) = 3e-3: updates of the order of lr_t."""
    rng = np.random.default_rng(seed)
    c = Case()
    n = int(np.prod(shape))
    c.p = np.clip(rng.standard_normal(n) * 0.05, -0.3, 0.3).astype(F32)
    c.g = (rng.standard_normal(n) * gs).astype(F32)
    c.m = (rng.standard_normal(n) * ms).astype(F32)
    c.v = ((rng.random(n) + 0.01) * vs).astype(F32)
    plant(c, rng)
    c.shape = tuple(shape) if not isinstance(shape, int) else (shape,)
    return c


def norm64(g, p=None, l2=0.0):
    a = f64(g) if p is None or l2 == 0.0 else f64(g) + l2 * f64(p)
    return float(np.sum(a * a))


def clip_for(ss, mode):
    """The clip setting of a case relative to its norm: "off" = 0, "inactive" = twice the norm (scale exactly 1), "active" = half of it."""
    nrm = math.sqrt(ss)
    return {"off": 0.0, "inactive": float(F32(2.0 * nrm + 1e-3)), "active": float(F32(0.5 * nrm + 1e-12))}[mode]


CLIPS = ("off", "inactive", "active")
L2S = (0.0, 2e-8, 0.5)
HP_ODD = dict(b1=0.5, b2=0.9, eps=1e-3)

SQNORM_NS = (1, 3, 1027, 262147, 1100003)
PARTIALS_NS = ((4, None), (1027, 64), (3153923, 4096))
STEP_NS = (1, 5, 4099, 4200003)
STEP_BIG = ((2e-8, "active"), (0.5, "off"), (0.0, "inactive"))              # (l2, clip) at the largest n; the smaller n take the full cross
SMALL_NS = (1, 2, 3, 5, 64, 77, 257, 1023, 1024, 1025, 4099, 8193, 32768, 31, 2049, 12288)
SMALL_ZERO_G = 5                                                         # the tensor (of 77) whose gradient is all zero
LSTM_SHAPES = ((16, 4), (48, 36), (64, 64), (272, 16))
LSTM_IMAGES = ("bf16", "f16_plain", "l1_fp8_layer0", "l1_fp8_upper", "l2_fp8_layer0", "lohi_l1", "lohi_l2_layer0", "lohi_l2_layer1", "nseg3")
ADAM2D_SHAPES = ((8, 4), (64, 64), (200, 68), (1024, 3080))
MOE_SHAPES = ((4, 8, 32), (128, 128, 32), (200, 192, 32), (388, 328, 96))


def step_case(n, l2, clip_mode, seed=0, odd=False):
    """One evc_clip_adam_step case: the norm is fed from the host (the f32 nearest to the float64 sum)."""
    c = bulk(n, 9100 + n % 1000 + seed)
    c.hp = Hyper(l2=l2, **(HP_ODD if odd else {}))
    c.ss32 = float(F32(norm64(c.g, c.p, c.hp.l2)))
    c.hp = c.hp.but(clip=clip_for(c.ss32, clip_mode))
    c.name = "n=%d l2=%g clip=%s%s" % (n, l2, clip_mode, " odd" if odd else "")
    return c


def step_ref(c, ss32=None, hp=None):
    hp = c.hp if hp is None else hp
    s, d_s = scale_ref(c.ss32 if ss32 is None else ss32, hp.clip)
    return adam_ref(c.p, c.g, c.m, c.v, hp, s, d_s)


def small_cases(seed=0):
    """The sixteen tensors of one evc_clip_adam_small launch: gradient scales alternate so that the norms fall below and above the clip of 0.25."""
    cs = []
    for i, n in enumerate(SMALL_NS):
        gs = (0.1 if i % 2 == 0 else 1.0) / math.sqrt(n)                # norm ~ 0.1 (scale exactly 1) or ~ 1 (clipped to 0.25)
        c = bulk(n, 9300 + i + seed, gs=gs)
        if i == SMALL_ZERO_G:
            c.g[:] = 0.0
        c.name = "tensor %d n=%d" % (i, n)
        cs.append(c)
    return cs, Hyper(clip=0.25)


def small_ref(c, hp):
    ss = norm64(c.g)
    s, d_s = scale_ref(ss, hp.clip, ss_rel(small_depth(c.p.size)))
    out = adam_ref(c.p, c.g, c.m, c.v, hp, s, d_s, l2=0.0)
    sq, d = sq_terms(c.g)
    out["ss"], out["d_ss"] = ss, sum_bound(sq, d, small_depth(c.p.size))
    return out


def lstm_case(H, nin, clip_w="active", clip_b="active", seed=0):
    """One evc_lstm_adam_fused case: kernel [4H][nin + H] and bias [4H].  One clip serves both tensors, so the gradients are scaled: "active" = a norm of
    twice the clip, "inactive" = half of it."""
    R, C = 4 * H, nin + H
    c = Case()
    c.H, c.nin, c.R, c.C = H, nin, R, C
    c.w = bulk((R, C), 9500 + H + nin + seed)
    c.b = bulk(R, 9600 + H + nin + seed)
    c.hp = Hyper(clip=0.5)
    for t, mode in ((c.w, clip_w), (c.b, clip_b)):
        want = {"active": 1.0, "inactive": 0.25}[mode]
        t.g = (t.g * F32(want / math.sqrt(norm64(t.g)))).astype(F32)
        if t.where["eps_dominates"].size:                               # keep the planted magnitudes where the regimes need them
            rng = np.random.default_rng(1)
            _set(t, t.where["eps_dominates"], "eps_dominates", rng)
            _set(t, t.where["underflow"], "underflow", rng)
    c.name = "H=%d nin=%d w %s b %s" % (H, nin, clip_w, clip_b)
    return c


def fused_ref(t, hp, D):
    """A tensor whose norm the fused kernel sums itself over a tree of depth D -> adam_ref + ss, d_ss."""
    ss = norm64(t.g)
    s, d_s = scale_ref(ss, hp.clip, ss_rel(D))
    out = adam_ref(t.p, t.g, t.m, t.v, hp, s, d_s, l2=0.0)
    sq, d = sq_terms(t.g)
    out["ss"], out["d_ss"] = ss, sum_bound(sq, d, D)
    return out


def lstm_images(images, H, nin):
    """-> (nseg, col0, hi_cols, hi_tail, has_f16, has_fp8) of the layouts of test_gpu_kernels' parametrisation, and nseg = 3."""
    if images == "bf16":
        return 1, 0, 0, False, False, False
    if images == "f16_plain":
        return 1, 0, 0, False, True, False
    if images == "nseg3":
        return 3, 0, 0, False, True, False
    nseg = 2 if images in ("l2_fp8_layer0", "lohi_l2_layer0") else 1
    col0 = nin if images in ("l2_fp8_layer0", "lohi_l2_layer0") else 0
    hi_cols = nin if images in ("l1_fp8_layer0", "lohi_l1", "lohi_l2_layer1") else 0
    return nseg, col0, hi_cols, images.startswith("lohi"), True, True


def adam2d_case(R, C, seed=0):
    c = Case()
    c.R, c.C = R, C
    c.w = bulk((R, C), 9700 + R + C + seed)
    c.w.g = (c.w.g * F32(1.0 / math.sqrt(norm64(c.w.g)))).astype(F32)
    if c.w.where["eps_dominates"].size:
        rng = np.random.default_rng(2)
        _set(c.w, c.w.where["eps_dominates"], "eps_dominates", rng)
        _set(c.w, c.w.where["underflow"], "underflow", rng)
    c.hp = Hyper(clip=0.5)
    c.name = "R=%d C=%d" % (R, C)
    return c


# ---------------------------------------------------------------------------- MoE
def moe_case(V, K, rows, l2, clip_mode, seed=0, ld=None, B=None):
    """dlogits [rows][ld] bf16 (bits), x [rows][K] bf16 (bits), W, m, v [V][K].  Columns of dlogits: every seventh is zero (a class absent from the
    batch), every seventh + 1 about 1e-9 (a rare class); the columns V .. ld hold finite garbage the kernel must mask.  m and v
    have the size of the gradient and of its square (m is its running average), so that the bound rows U sum |a| |x| of the recomputed tile, which the moments
    inherit, stays below 1e-5 of |m_new| + |m_old|."""
    rng = np.random.default_rng(9800 + V + K + rows + seed)
    c = Case()
    c.V, c.K, c.rows, c.ld = V, K, rows, (V + 7) // 8 * 8 + 8 if ld is None else ld
    a = rng.standard_normal((rows, c.ld)) * 0.05
    cols = np.arange(c.ld)
    if V >= 8:
        a[:, (cols % 7 == 0) & (cols < V)] = 0.0
        a[:, (cols % 7 == 1) & (cols < V)] *= 2e-8
    if ld is not None:                                                   # the engine's layout: pad columns and the rows from B on are zero
        a[:, V:] = 0.0
        a[B:] = 0.0
    c.a = bf16_bits(a.astype(F32))
    c.x = bf16_bits((rng.standard_normal((rows, K)) * 0.5).astype(F32))
    c.g64, c.d_g = moe_grad(c)
    gs = math.sqrt(float(np.mean(c.g64 ** 2)))                          # moments of the size a running average of such gradients has
    c.w = bulk((V, K), 9900 + V + K + seed, ms=2.0 * gs, vs=gs * gs)
    if V >= 8:                                                           # the first step of an absent class (g = m = v = 0: with l2 = 0 its weights must come
        c.w.m[:2 * K] = 0.0                                              # back bit for bit) and of a rare one (|g| ~ 1e-9, v = 0: eps dominates)
        c.w.v[:2 * K] = 0.0
    c.hp = Hyper(l2=l2)
    wp = c.w.p.reshape(V, K)
    c.ss = float(np.sum((c.g64 + c.hp.l2 * f64(wp)) ** 2))
    c.hp = c.hp.but(clip=clip_for(c.ss, clip_mode))
    c.name = "V=%d K=%d rows=%d l2=%g clip=%s" % (V, K, rows, l2, clip_mode)
    return c


def moe_grad(c, r0=0, r1=None):
    """The float64 product of the bf16 factors over rows r0 .. r1 and its bound in any order of the terms."""
    a = bf16_to_f64(c.a)[r0:r1, :c.V]
    x = bf16_to_f64(c.x)[r0:r1]
    return a.T @ x, a.shape[0] * U * (np.abs(a).T @ np.abs(x))


def moe_norm_ref(p, l2, g64, d_g, before=(0.0, 0.0)):
    """Pass 1 + finalize over the rows given: sums[0] += sum (g + l2 p)^2, sums[1] += sum p^2."""
    p = f64(p)
    t = l2 * p
    a = g64 + t
    d_a = d_g + U * np.abs(t) + (U * (np.abs(a) + d_g + U * np.abs(t)) if l2 != 0.0 else 0.0)
    sq, d = prod((a, d_a), (a, d_a))
    d = d + FLOOR
    pq, dq = sq_terms(p)
    return (np.array([before[0] + sq.sum(), before[1] + pq.sum()]),
            np.array([sum_bound(sq, d, MOE_DEPTH, before[0]), sum_bound(pq, dq, MOE_DEPTH, before[1])]))


def moe_ref(c, ss32, g64=None, d_g=None, hp=None):
    """Pass 2 from the f32 norm it reads."""
    hp = c.hp if hp is None else hp
    s, d_s = scale_ref(ss32, hp.clip)
    w = c.w
    sh = (c.V, c.K)
    return adam_ref(w.p.reshape(sh), c.g64 if g64 is None else g64, w.m.reshape(sh), w.v.reshape(sh), hp, s, d_s, d_g=c.d_g if d_g is None else d_g)


def wsq_ref(p_stored):
    """The |W|^2 of the new weights: the float64 sum of the squares of the stored p, and its bound."""
    sq, d = sq_terms(p_stored)
    return float(sq.sum()), sum_bound(sq, d, MOE_DEPTH)


# ---------------------------------------------------------------------------- the Gram-matrix clip norm (csrc/evc_moe_norms.hip)
GRAM_V, GRAM_K = 200, 192
GRAM_RS = (32, 96)
GRAM_SLABS = ((3, 3), (4, 2))                                            # (SA, SX): 8 k steps of dlogits in 3 + 3 + 2 / 4 x 2, 6 of x in 3 x 2 / 2 x 3
GRAM_BEFORE = (0.25, 0.5)


def gram_case(R, l2, with_bias, seed=0):
    """dlogits [R][256] (V = 200 live columns, zero pad as the engine keeps them; rows from B on zero), x [R][192], W [200][192], and the forward's f32
    logits [B][V] = f32(x W^T + bias).  B = R - 2 at R = 32 (a batch that does not fill its rows), R at 96."""
    B = R - 2 if R == 32 else R
    c = moe_case(GRAM_V, GRAM_K, R, l2, "active", seed=seed + 7, ld=256, B=B)
    c.B = B
    rng = np.random.default_rng(9950 + R)
    c.bias = (rng.standard_normal(GRAM_V) * 0.1).astype(F32) if with_bias else None
    c.name = "R=%d B=%d l2=%g bias=%s" % (R, B, l2, "given" if with_bias else "None")
    return gram_set_weights(c, c.w.p)


def gram_set_weights(c, p):
    """The weights the norm is taken of (the GPU test: the p a preceding evc_moe_grad_update_apply stored) and the forward logits that go with them."""
    c.w.p = np.asarray(p, F32).reshape(-1).copy()
    w = f64(c.w.p).reshape(c.V, c.K)
    c.logits64 = bf16_to_f64(c.x)[:c.B] @ w.T + (0.0 if c.bias is None else f64(c.bias))
    c.logits = c.logits64.astype(F32)
    return c


def gram_slab_ranges(cols, S):
    nk = cols // 32
    per = (nk + S - 1) // S
    return [(32 * s * per, 32 * min(nk, (s + 1) * per)) for s in range(S)]


def gram_slabs_ref(bits, cols, S):
    """evc_gram_slabs: -> (slabs [S][R][R], bound): slab s = A[:, slab] A[:, slab]^T, an f32 MFMA accumulation of n_s = its columns terms: n_s U sum |a_i| |a_j|."""
    a = bf16_to_f64(bits)[:, :cols]
    out, bnd = [], []
    for k0, k1 in gram_slab_ranges(cols, S):
        out.append(a[:, k0:k1] @ a[:, k0:k1].T)
        bnd.append((k1 - k0) * U * (np.abs(a[:, k0:k1]) @ np.abs(a[:, k0:k1]).T))
    return np.array(out), np.array(bnd)


def gram_depths(R, V):
    nbf = min(R * R // 256, 256)
    vq = ((V + 3) // 4 + 7) // 8 * 8
    return math.ceil(R * R / (nbf * 256)) + 6 + 4, math.ceil(vq / 256) + 6 + 4


def gram_norm_ref(c, SA, SX, wsq32, before=GRAM_BEFORE, drop_cross=False):
    """evc_moe_grad_norms: sums[0] += |g|^2 + 2 l2 <g, W> + l2^2 wsq, sums[1] += wsq, against the MATERIALISED float64 gradient g = A^T x and the f32 W.
    wsq (the |W|^2 carried from the previous evc_moe_grad_update_apply) is an input and used as given.  Three terms of mixed sign, so the bound is absolute:
      |g|^2 = sum_ij (sum_s GA_s)(sum_s GX_s): each slab element known to its slab bound, the S slabs added in turn (depth S), one product, then the block tree
              D_f = trips + 6 + 4 over products of BOTH signs: sum d_term + D_f U sum (|term| + d_term)
      <g, W> = sum_{r < B, v} a (logit - bias): the logits are the f32 rounding of x W^T + bias (U |logit|), the difference rounds (U |diff|), one product,
              the tree D_d = ceil(vq / 256) + 6 + 4 per (row, segment) block
      the partials are combined in double (nothing to add), the total is cast to f32 (U |total|) and added onto sums[0] (U |result|)."""
    ga, d_ga = gram_slabs_ref(c.a, c.ld, SA)
    gx, d_gx = gram_slabs_ref(c.x, c.K, SX)
    Df, Dd = gram_depths(c.rows, c.V)
    A = np.sum(ga, axis=0)
    d_A = np.sum(d_ga, axis=0) + SA * U * np.sum(np.abs(ga) + d_ga, axis=0)
    X = np.sum(gx, axis=0)
    d_X = np.sum(d_gx, axis=0) + SX * U * np.sum(np.abs(gx) + d_gx, axis=0)
    t, d_t = prod((A, d_A), (X, d_X))
    d_gg = float(np.sum(d_t) + Df * U * np.sum(np.abs(t) + d_t))
    a = bf16_to_f64(c.a)[:c.B, :c.V]
    bias = 0.0 if c.bias is None else f64(c.bias)
    diff = c.logits64 - bias
    d_diff = U * np.abs(c.logits64) + (U * (np.abs(diff) + U * np.abs(c.logits64)) if c.bias is not None else 0.0)
    u, d_u = prod((a, 0.0), (diff, d_diff))
    d_gw = float(np.sum(d_u) + Dd * U * np.sum(np.abs(u) + d_u))
    w = f64(c.w.p).reshape(c.V, c.K)
    gg, gw = float(np.sum(c.g64 * c.g64)), float(np.sum(c.g64 * w))
    l2 = c.hp.l2
    tot = gg + (0.0 if drop_cross else 2.0 * l2 * gw) + l2 * l2 * wsq32
    d_tot = d_gg + 2.0 * l2 * d_gw
    d_tot += U * (abs(tot) + d_tot)
    s0 = before[0] + max(tot, 0.0)
    s1 = before[1] + wsq32
    return (np.array([s0, s1]), np.array([d_tot + U * (abs(s0) + d_tot), U * abs(s1)]),
            dict(ga=ga, d_ga=d_ga, gx=gx, d_gx=d_gx, materialised=float(np.sum((c.g64 + l2 * w) ** 2)), cross=2.0 * l2 * gw))


def gram_emul(c, SA, SX, wsq32, before=GRAM_BEFORE):
    """The kernels in f32: slabs accumulated one 32-column MFMA step at a time, the S slabs added in turn, a product, the block trees, the double combine."""
    def slabs(bits, cols, S):
        a = bf16_to_f64(bits)[:, :cols]
        out = []
        for k0, k1 in gram_slab_ranges(cols, S):
            acc = np.zeros((a.shape[0], a.shape[0]), F32)
            for k in range(k0, k1, 32):
                acc = (acc + (a[:, k:k + 32] @ a[:, k:k + 32].T).astype(F32)).astype(F32)
            out.append(acc)
        return out
    ga, gx = slabs(c.a, c.ld, SA), slabs(c.x, c.K, SX)
    A, X = np.zeros_like(ga[0]), np.zeros_like(gx[0])
    for s in ga:
        A = (A + s).astype(F32)
    for s in gx:
        X = (X + s).astype(F32)
    R = c.rows
    nbf = min(R * R // 256, 256)
    pf = _block_sum(_strided_sum((A * X).astype(F32).reshape(-1), np.zeros(0, F32), nbf))
    a = bf16_to_f64(c.a)[:c.B, :c.V].astype(F32)
    diff = c.logits if c.bias is None else (c.logits - c.bias).astype(F32)
    u = (a * diff).astype(F32)
    vq = ((c.V + 3) // 4 + 7) // 8 * 8
    pd = []
    for r in range(c.B):
        for q in range(4):
            seg = u[r, q * vq:min(c.V, (q + 1) * vq)]
            pd.append(_block_sum(_strided_sum(seg, np.zeros(0, F32), 1))[0])
    tot = float(np.sum(f64(pf))) + 2.0 * c.hp.l2 * float(np.sum(f64(pd))) + c.hp.l2 * c.hp.l2 * float(wsq32)
    s0 = F32(F32(before[0]) + F32(max(tot, 0.0)))
    return np.array(ga), np.array(gx), np.array([s0, F32(F32(before[1]) + F32(wsq32))], F32)


# ---------------------------------------------------------------------------- sharpness
def sharpness(ref, p_old, m_old):
    """(share of the elements with a non-zero update whose limit on p is below 1e-3 of the update, share whose limit on m is below 1e-5 of |m_new| + |m_old|)."""
    upd = np.abs(ref["p"] - f64(p_old).reshape(ref["p"].shape))
    live = upd > 0
    sp = float(np.mean(ref["d_p"][live] < 1e-3 * upd[live])) if live.any() else 1.0
    mm = np.abs(ref["m"]) + np.abs(f64(m_old).reshape(ref["m"].shape))
    lm = mm > 0
    sm = float(np.mean(ref["d_m"][lm] < 1e-5 * mm[lm])) if lm.any() else 1.0
    return sp, sm
