"""Float64 references of the head, loss and pooling kernels (csrc/evc_elementwise.hip, moe_elem onwards), each with a derived
per-element bound on |got - ref| and a case generator.  numpy only.  Used by tests/test_cpu_head_ref.py (the references against
the oracle, an f32 emulation of every kernel, planted faults) and tests/test_gpu_head_parity.py (the kernels).  The companion
of tests/_lstm_fwd_ref.py and tests/_bptt_ref.py: those cover the LSTM steps, this file what turns the last state into
predictions, a loss and the first gradient, and what pools frames.

Every reference is fed the kernel's own f32 / uint8 inputs as exact float64 numbers, so a correct kernel differs from it only by
its f32 roundings, its fast intrinsics and the rounding of each store.  No measured constant enters a bound, with one exception:
LOG_ABS / LOG_REL, the distance of __logf from log (see "CE").

Notation and the error models reused from the LSTM files
--------------------------------------------------------
    U   = 2^-24  f32 unit roundoff: one f32 operation or one f32 store moves a value by U of its magnitude
    EPS = 2^-20  the handful of roundings of an elementwise tail (1 + e, rcpf_ at 1 ulp, its products), absolute on values <= 2
    RB  = 2^-8   a bf16 store
    an f32 sum of terms in ANY order whose tree has depth D is off by at most D U sum|terms|
    __expf(-z): a shift of the argument by 2U(|z| + 2)
    IEEE division (1.f / a, s / (float)S) is correctly rounded: U (the library is built without fast-math)
    a product of k factors v_i known to d_i, formed with k - 1 roundings:  prod(|v_i| + d_i) - prod|v_i| + (k - 1) U prod(|v_i| + d_i)
    (function prod below; it keeps every second-order term, so no "1 + small" factor appears anywhere)

A value stored as f32 IS the kernel's f32 result: limit = d.  A value stored as bf16: limit = RB (|ref| + d) + d.

Depth of the scalar reductions.  The any-order bound (n - 1) U would be 1.6e-2 at n = 264 096 and hide everything, so every
scalar sum uses the depth of the kernel's actual tree: trips per thread (x 4 on the float4 path: four sequential additions a
trip) + 6 shuffle steps + 4 waves + the block partials joined (float atomics in any order, or the ordered finish, <= 256), + 3
for the scaling by 1/B and the addition onto the old *loss.  Per case (loss_depth):
    CE (1,1), (2,3)   1 trip, 1 block        D = 1 + 6 + 4 + 1 + 3   = 15
    CE (3,4717)       scalar, 56 blocks      D = 1 + 10 + 56 + 3     = 70
    CE (5,4716)       float4, 93 blocks, 1 trip x 4   D = 4 + 10 + 93 + 3 = 110;  as a misaligned view: scalar, D = 1 + 10 + 93 + 3 = 107
    CE (17,4717)      scalar, 256 blocks, 2 trips     D = 2 + 10 + 256 + 3 = 271
    CE (56,4716)      float4, 256 blocks, 2 trips x 4 D = 8 + 10 + 256 + 3 = 277
    REP (1,1) 15; (3,1023) 12 blocks 26; (5,4096) 80 blocks 94; (20,4099) 256 blocks, 2 trips 271
    MoE rowsum        one block a row: D = ceil(V / 256) + 6 + 4                    (V = 700: 13)
    meanpool          a wave adds its frames in turn, the 4 waves and 1/n follow, ceil(T / 32) blocks join by atomics:
                      D = ceil(T / (4 ceil(T / 32))) + 3 + ceil(T / 32) + 2          (T = 300: 8 + 3 + 10 + 2 = 23)

MoE tail (moe_elem, moe_tail_fwd_kernel, moe_tail_bwd_kernel) = oracle.model_math.moe_fwd / moe_bwd restated on logits
-----------------------------------------------------------------------------------------------------------------------
Per class the kernel reads ga[0..M], ea[0..M-1].  t_m = ga_m - max ga (one rounding: a shift U|t_m|), x_m = __expf(t_m) (a shift
2U(|t_m| + 2)): x_m carries a relative error rho_m = expm1(3U(|t_m| + 2)).  den = sum of M + 1 terms (M additions), inv = 1 / den
(U), g_m = x_m inv (U):
    d_g_m = g_m (rho_m + max_k rho_k + (M + 2) U) (1 + max_k rho_k) + 2^-100   (the floor covers an x_m flushed to zero below 1e-38)
    e_m   = sigmoidf_(ea_m):  d_z = 2U(|ea_m| + 2),  d_e = e (1 - e) d_z + d_z^2 + EPS          (as every sigmoid of the LSTM files)
    pred  = sum_{m<M} g_m e_m:  d_pred = sum_m prod-bound(g_m, e_m) + M U sum_m (g_m + d_g_m)(e_m + d_e_m)
    rowsum[b] = sum_c pred:     d = sum_c d_pred + D U sum_c (pred + d_pred)
Backward, dp = dpred (an f32 input, exact):
    sdot  = sum_{m<M} dp e_m g_m      d_sdot = sum_m prod-bound(dp, e_m, g_m) + M U sum_m |dp| (e_m + d_e)(g_m + d_g)
    dgm   = dp e_m [m < M]            prod-bound(dp, e_m);  exactly 0 for m = M
    diff  = dgm - sdot                d_diff = d_dgm + d_sdot + U (|diff| + d_dgm + d_sdot)
    dga_m = g_m diff                  prod-bound(g_m, diff), stored bf16 at row stride ld_dgate
    dea_m = dp g_m e_m (1 - e_m)      prod-bound(dp, g_m, e_m, 1 - e_m) with d(1 - e) = d_e + U, stored bf16 at row stride ld_dexpert

CE (ce_loss_kernel): a = p + 1e-5, bq = 1 - p + 1e-5 in f32
-----------------------------------------------------------
The kernel's eps is f32(1e-5); against the float64 1e-5 of the oracle that is U 1e-5.  d_a = U (a + 2e-5), d_bq = U (|1 - p| + bq
+ 2e-5).  Term t = -log(y ? a : bq): the argument error gives d_arg / (arg - d_arg), __logf itself LOG_ABS + LOG_REL |t|:
    d_t    = d_arg / (arg - d_arg) + LOG_ABS + LOG_REL |t|
    loss   = loss_before + (1/B) sum t:   d = (1/B) sum d_t + D U ((1/B) sum (|t| + d_t) + |loss_before|)
    dpred (+)= gs (y ? -1/a : 1/bq):      1/arg is correctly rounded: d_inv = d_arg / (arg (arg - d_arg)) + U / (arg - d_arg);
                                          prod-bound(inv, gs), and + U |result| for the addition when accumulating.
LOG_ABS, LOG_REL.  The project has no model of __logf.  evc_ce_loss with B = V = 1, dpred = None and loss zeroed leaves
-__logf(f32 argument) with nothing in between; log_sweep() is the fixed sweep of ~2000 arguments.  Over it the worst |got -
log64(argument)| is recorded in two parts: absolute where |log| <= 1, relative to |log| where |log| > 1.  Each constant is the
next power of two at or above 4 x its measured worst (the 4 is room for another ROCm's math library).  Measured on an MI355X
(profiles/head_parity_ratios.txt): 8.253e-08 = 2^-23.53 absolute and 1.771e-07 = 2^-22.43 relative, so LOG_ABS = 2^-21 and LOG_REL =
2^-20; the largest error of the sweep is 1.995e-06 at log = -11.26, below the 2^-16 at which __logf would be a finding.  The GPU test
repeats the sweep and asserts both parts.  Nothing else in this file is measured.

REP (rep_loss_kernel): d = a - b (U), term d d, loss += (1/B) sum, dstate_s (+)= -2 d (1/B) gs
-------------------------------------------------------------------------------------------
    d_term = prod-bound(d, d) with d_d = U |d|;  loss as for CE with D of the scalar path
    grad   = prod-bound(d, 1/B, gs) with d(1/B) = U / B (the factor -2 is exact), + U |result| when accumulating

Elementwise
-----------
    sigmoid_fwd (in place)   d = p (1 - p) d_z + d_z^2 + EPS,  d_z = 2U(|z| + 2)
    sigmoid_bwd              bf16(dp p (1 - p)): prod-bound(dp, p, 1 - p) with d(1 - p) = U (1 - p)
    relu6_fwd / relu6_bwd    exact (min, max, select); the bf16 outputs are the correctly rounded f32 ones: bit for bit
    ema_update               moving - c (moving - batch), c = 1 - decay (exact in f32 for decay >= 0.5): the difference U, the product
                             U (or none under an fma), the subtraction U:  d = 3 U |c (moving - batch)| + U |result|
    fill_f32, cast_f32_to_bf16, cast_f32_to_bf16_split (hi = bf16(x), lo = bf16(x - hi), x - hi exact in f32)   exact

Pooling and sampling
--------------------
Dequantise (uint8 input): v = q sc + bi with the kernel's f32 constants sc = f32(4 / 255), bi = 4 / 512 - 2 (exact).  The reference
evaluates q sc + bi with those constants in float64 (TF's Dequantize multiplies an f32 tensor by the same f32 scalar; f32(4/255)
lies 0.498 ulp above 4/255, which moves q = 255 by 3.97 U against oracle.model_math.dequantize - a property of the format, not of the
kernel).  The product is below 4 (half an ulp <= 2U) and the sum rounds by U |v|; under an fma only the latter:  d_v = U (|v| + 2).
l2-normalise (one wave a frame): ss = sum v^2 over F terms, <= 4 ceil(F / 256) sequential additions a lane + 6 shuffle steps + the
squaring: relative (D_ss + 1) U with D_ss = 4 ceil(F / 256) + 6, plus 2 |v| . d_v terms -> the norm moves by at most |d_v|_2;
rsqrtf at 1 ulp (2U) and half the relative error of ss:
    rel_n = |d_v|_2 / norm + ((D_ss + 1) / 2 + 2) U;    out = v / norm: prod-bound((v, d_v), (1 / norm, rel_n (1 + 2 rel_n) / norm))
    norm = sqrt(max(ss, 1e-12)): an all-zero frame gives exact zeros.
meanpool_fwd: float input sums ALL T frames, uint8 input the frames < min(T, num_frames); both divide by num_frames
(oracle.model_math.logistic_fwd's average; uint8 frames >= num_frames are padding = zero after Dequantize):
    d = (1/n) sum_t d_frame + D U (1/n) sum_t (|frame| + d_frame);   the bf16 copy is bf16 of the f32 result, bit for bit
sample_frames_gather / sample_sequence_gather: idx_out is exactly oracle.model_math.sample_random_frames_index /
sample_random_sequence_index (one f32 product, truncated).  The row is frame clamp(idx, 0, T - 1); for uint8 input zeros when that
clamped index is >= num_frames.  Without normalize a float row is the source frame bit for bit, a uint8 row within d_v.
For u < 1 the index stays below n: (1 - U) n rounds to the f32 neighbour below n or lower, never to n (n U is at least half the
spacing below n), which the CPU test checks for every n <= 300.  idx == n needs u == 1.0, outside the contract of a uniform draw;
the cases carry it all the same so that the clamp, the zero frame and the unclamped idx_out are pinned.
framepool_mean_fwd: S sequential additions and a correctly rounded division: d = (S - 1) U sum|y| / S + U |mean|; bf16 copy = bf16 of the
f32 result.  framepool_mean_bwd: dpooled (1/S): prod-bound(dpooled, 1/S) with d(1/S) = U / S.
framepool_max_fwd / _bwd: exact; the first maximum wins; the bf16 pool is the correctly rounded maximum.
"""
import math

import numpy as np

from _bptt_ref import EPS, RB, U, bf16_bits, bf16_round, bf16_to_f64  # noqa: F401

# the only measured constants (see "CE" above): next power of two at or above 4 x the worst of the sweep on an MI355X
LOG_ABS = 2.0 ** -21      # measured 8.253e-08 = 2^-23.53 where |log| <= 1 (near 1: most negative-class terms of a batch)
LOG_REL = 2.0 ** -20      # measured 1.771e-07 = 2^-22.43 of |log| where |log| > 1 (1.995e-06 absolute at log = -11.26)

TINY = 2.0 ** -100
CE_EPS32 = float(np.float32(10e-6))
GS = float(np.float32(0.37))                                             # the grad_scale of every loss case, as the f32 the ABI passes
LOSS0 = 2.5                                                              # what *loss holds before a loss entry runs
SC32 = float(np.float32(4.0) / np.float32(255.0))
BI32 = float(np.float32(4.0) / np.float32(512.0) - np.float32(2.0))
F32 = np.float32
F64 = np.float64


class Case:
    pass


def f64(a):
    return np.asarray(a, dtype=F64)


# ---------------------------------------------------------------------------- the comparison
def ratio(got, ref, bound, r=0.0):
    """|got - ref| / (r (|ref| + bound) + bound) per element; 0 where both agree exactly (inf == inf included), inf where the
    kernel left something not finite against a finite reference or missed a zero limit."""
    got, ref, bound = f64(got), f64(ref), f64(bound)
    lim = r * (np.abs(ref) + bound) + bound
    with np.errstate(invalid="ignore", divide="ignore"):
        same = (got == ref) | (np.isnan(got) & np.isnan(ref))
        q = np.where(same, 0.0, np.abs(got - ref) / lim)
    return np.where(np.isfinite(q), q, np.inf)


def exact(got, ref):
    """0 where equal as values (-0.0 == 0.0, NaN == NaN), inf elsewhere."""
    got, ref = np.asarray(got), np.asarray(ref)
    same = got == ref
    if got.dtype.kind == "f":
        same = same | (np.isnan(got) & np.isnan(ref))
    return np.where(same, 0.0, np.inf)


def worst(q):
    q = np.atleast_1d(np.asarray(q, dtype=F64))
    if q.size == 0:
        return 0.0, ()
    at = np.unravel_index(int(np.argmax(q)), q.shape)
    return float(q[at]), tuple(int(v) for v in at)


def prod(*fs):
    """fs = (value, bound) pairs -> (product, bound) of a product formed in f32 with len(fs) - 1 roundings."""
    v = np.ones(())
    lo = np.ones(())
    hi = np.ones(())
    for a, d in fs:
        a = f64(a)
        v = v * a
        lo = lo * np.abs(a)
        hi = hi * (np.abs(a) + f64(d))
    return v, (hi - lo) + (len(fs) - 1) * U * hi


def sigmoid(z):
    z = f64(z)
    with np.errstate(over="ignore"):
        e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def sigmoid_ref(z):
    p = sigmoid(z)
    dz = 2 * U * (np.abs(f64(z)) + 2.0)
    return p, p * (1.0 - p) * dz + dz * dz + EPS


# ---------------------------------------------------------------------------- MoE tail
def moe_ref(ga, ea, dp=None):
    """ga [B][V][M+1], ea [B][V][M] (the f32 logits), dp [B][V] or None -> dict of float64 arrays: pred, rowsum (+ d_*), and with
    dp: dga [B][V][M+1], dea [B][V][M] (+ d_*)."""
    ga, ea = f64(ga), f64(ea)
    B, V, M1 = ga.shape
    M = M1 - 1
    t = ga - ga.max(axis=2, keepdims=True)
    x = np.exp(t)
    g = x / x.sum(axis=2, keepdims=True)
    rho = np.expm1(3 * U * (np.abs(t) + 2.0))
    rmax = rho.max(axis=2, keepdims=True)
    d_g = g * (rho + rmax + (M + 2) * U) * (1.0 + rmax) + TINY
    e, d_e = sigmoid_ref(ea)
    ge, d_ge = prod((g[..., :M], d_g[..., :M]), (e, d_e))
    pred = ge.sum(axis=2)
    d_pred = d_ge.sum(axis=2) + M * U * ((g[..., :M] + d_g[..., :M]) * (e + d_e)).sum(axis=2)
    D = math.ceil(V / 256) + 6 + 4
    out = dict(g=g, e=e, pred=pred, d_pred=d_pred, rowsum=pred.sum(axis=1),
               d_rowsum=d_pred.sum(axis=1) + D * U * (pred + d_pred).sum(axis=1), M=M)
    if dp is not None:
        dp = f64(dp)[..., None]
        z0 = np.zeros_like(dp)
        tm, d_tm = prod((dp, z0), (e, d_e), (g[..., :M], d_g[..., :M]))
        sdot = tm.sum(axis=2, keepdims=True)
        d_sdot = d_tm.sum(axis=2, keepdims=True) + M * U * (np.abs(dp) * (e + d_e) * (g[..., :M] + d_g[..., :M])).sum(axis=2, keepdims=True)
        dgm = np.zeros_like(g)
        d_dgm = np.zeros_like(g)
        dgm[..., :M], d_dgm[..., :M] = prod((dp, z0), (e, d_e))
        diff = dgm - sdot
        d_diff = d_dgm + d_sdot + U * (np.abs(diff) + d_dgm + d_sdot)
        out["dga"], out["d_dga"] = prod((g, d_g), (diff, d_diff))
        out["dea"], out["d_dea"] = prod((dp, z0), (g[..., :M], d_g[..., :M]), (e, d_e), (1.0 - e, d_e + U))
    return out


MOE_B = 3
MOE_MS = (1, 2, 3, 4)
MOE_VS = (1, 255, 257, 700)


def moe_case(M, V, seed=0):
    """N(0, 3) logits with planted classes: (0, 0) all gates equal; (1, 0) gate 0 = +30; (2, 0) every gate -1e4 and expert logits
    +-100; and for V >= 2 in the last class: (0, V-1) every gate -1e4, (1, V-1) expert logits -+100, (2, V-1) the LAST gate +30."""
    rng = np.random.default_rng(7100 + 10 * M + V + seed)
    c = Case()
    c.B, c.M, c.V = MOE_B, M, V
    c.name = "M=%d V=%d" % (M, V)
    c.ga = (rng.standard_normal((c.B, V, M + 1)) * 3.0).astype(F32)
    c.ea = (rng.standard_normal((c.B, V, M)) * 3.0).astype(F32)
    pm = np.where(np.arange(M) % 2 == 0, 100.0, -100.0).astype(F32)
    c.ga[0, 0] = 0.5
    c.ga[1, 0, 0] = 30.0
    c.ga[2, 0] = -1e4
    c.ea[2, 0] = pm
    c.sat = [(2, 0)]                                                    # classes whose dexpert must be exactly zero
    if V >= 2:
        c.ga[0, V - 1] = -1e4
        c.ea[1, V - 1] = -pm
        c.ga[2, V - 1, M] = 30.0
        c.sat.append((1, V - 1))
    c.labels = (rng.random((c.B, V)) < 0.01).astype(np.uint8)
    c.labels[0, 0] = 1
    return c


def ce_grad_f32(pred32, labels, gs=1.0):
    """The f32 evaluation of the CE gradient (what evc_ce_loss leaves in dpred), for building a dpred on the CPU."""
    p = np.asarray(pred32, F32)
    eps = F32(10e-6)
    a = p + eps
    bq = F32(1.0) - p + eps
    return (np.where(np.asarray(labels) != 0, F32(-1.0) / a, F32(1.0) / bq) * F32(gs)).astype(F32)


# ---------------------------------------------------------------------------- losses
def loss_depth(n, vec):
    grid = min((n + 255) // 256, 256)
    per = n // 4 if vec else n
    trips = math.ceil(per / (grid * 256)) * (4 if vec else 1)
    return trips + 6 + 4 + grid + 3


def ce_ref(p, y, B, gs=GS, dp0=None, loss0=LOSS0, vec=False, want_grad=True):
    """p [n] f32, y [n] uint8 -> dict loss, d_loss (and grad, d_grad [n]: onto dp0 when given)."""
    p = f64(p).reshape(-1)
    pos = np.asarray(y).reshape(-1) != 0
    n = p.size
    a = p + 10e-6
    bq = 1.0 - p + 10e-6
    arg = np.where(pos, a, bq)
    d_arg = np.where(pos, U * (np.abs(a) + 2e-5), U * (np.abs(1.0 - p) + np.abs(bq) + 2e-5))
    t = -np.log(arg)
    d_t = d_arg / (arg - d_arg) + LOG_ABS + LOG_REL * np.abs(t)
    D = loss_depth(n, vec)
    out = dict(loss=loss0 + t.sum() / B, d_loss=d_t.sum() / B + D * U * ((np.abs(t) + d_t).sum() / B + abs(loss0)), depth=D, terms=t)
    if want_grad:
        inv = np.where(pos, -1.0, 1.0) / arg
        d_inv = d_arg / (arg * (arg - d_arg)) + U / (arg - d_arg)
        g, d_g = prod((inv, d_inv), (gs, 0.0))
        if dp0 is not None:
            g = f64(dp0).reshape(-1) + g
            d_g = d_g + U * (np.abs(g) + d_g)
        out["grad"], out["d_grad"] = g, d_g
    return out


def rep_ref(a, b, B, gs=GS, dp0=None, loss0=LOSS0, want_grad=True):
    a, b = f64(a).reshape(-1), f64(b).reshape(-1)
    n = a.size
    d = a - b
    d_d = U * np.abs(d)
    t, d_t = prod((d, d_d), (d, d_d))
    D = loss_depth(n, False)
    out = dict(loss=loss0 + t.sum() / B, d_loss=d_t.sum() / B + D * U * ((t + d_t).sum() / B + abs(loss0)), depth=D)
    if want_grad:
        g, d_g = prod((-2.0 * d, 2.0 * d_d), (1.0 / B, U / B), (gs, 0.0))
        if dp0 is not None:
            g = f64(dp0).reshape(-1) + g
            d_g = d_g + U * (np.abs(g) + d_g)
        out["grad"], out["d_grad"] = g, d_g
    return out


CE_SHAPES = [(1, 1), (2, 3), (3, 4717), (5, 4716), (17, 4717), (56, 4716)]
CE_VIEW_SHAPE = (5, 4716)                                               # run once more as views one float / one byte into larger buffers
CE_SPARSE_SHAPES = [(17, 4717), (56, 4716)]
REP_SHAPES = [(1, 1), (3, 1023), (5, 4096), (20, 4099)]
SWEEP = 256 * 256                                                       # elements of one grid sweep of a loss kernel (x 4 on the float4 path)


def ce_case(B, V, sparse=False):
    """p = uniform(0, 1)^4, labels in {0, 1, 255} at 1 % positives; planted at the end p = 1e-30 / y 0, p = 1 / y 255, p = 1 / y 0,
    p = 0 / y 1 (the last element: a heavy term inside the n % 4 tail), at the start p = 0 / y 0, p = 0 / y 255, p = 1 / y 1.
    sparse: p = 0 and y = 0 everywhere (-log(1 + 1e-5) an element) except y = 1 (a term of 11.5) at the last element, at the last
    element of the first grid sweep and at the first of the second."""
    rng = np.random.default_rng(7200 + 31 * B + V + (5 if sparse else 0))
    n = B * V
    c = Case()
    c.B, c.V, c.n = B, V, n
    c.name = "B=%d V=%d%s" % (B, V, " sparse" if sparse else "")
    if sparse:
        c.p = np.zeros(n, F32)
        c.y = np.zeros(n, np.uint8)
        sweep = SWEEP * (4 if n % 4 == 0 else 1)
        assert n > sweep
        c.heavy = [n - 1, sweep - 1, sweep]
        c.y[c.heavy] = 1
    else:
        c.p = (rng.random(n) ** 4).astype(F32)
        pos = rng.random(n) < 0.01
        c.y = np.where(pos, np.where(rng.random(n) < 0.5, 1, 255), 0).astype(np.uint8)
        plants = [(n - 1, 0.0, 1), (n - 2, 1.0, 0), (n - 3, 1.0, 255), (n - 4, 1e-30, 0), (0, 0.0, 0), (1, 0.0, 255), (2, 1.0, 1)]
        done = set()
        for i, pv, yv in plants:
            if 0 <= i < n and i not in done:
                c.p[i], c.y[i] = pv, yv
                done.add(i)
    c.dp0 = rng.standard_normal(n).astype(F32)
    return c


def rep_case(B, D):
    rng = np.random.default_rng(7300 + 31 * B + D)
    c = Case()
    c.B, c.D, c.n = B, D, B * D
    c.name = "B=%d D=%d" % (B, D)
    c.a = rng.standard_normal(c.n).astype(F32)
    c.b = rng.standard_normal(c.n).astype(F32)
    c.b[-1] = c.a[-1] - F32(3.0)                                        # a heavy last element
    if c.n > 2:
        c.b[1] = c.a[1]                                                 # an exact zero difference
    c.dp0 = rng.standard_normal(c.n).astype(F32)
    return c


def log_sweep():
    """The fixed sweep of the __logf constant: (p [k] f32, label [k] uint8).  a = p + 1e-5 spaced logarithmically over [1e-5, 0.5]
    (label 1), bq = 1 - p + 1e-5 for p spaced logarithmically over [1e-7, 0.5] (label 0), and p = 0, p = 1 under each label."""
    a = np.geomspace(1e-5, 0.5, 1000)
    p1 = np.maximum(a - 1e-5, 0.0)
    p0 = np.geomspace(1e-7, 0.5, 1000)
    p = np.concatenate([p1, p0, [0.0, 0.0, 1.0, 1.0]]).astype(F32)
    y = np.concatenate([np.ones(1000), np.zeros(1000), [0, 1, 0, 255]]).astype(np.uint8)
    return p, y


def log_sweep_ref(p, y):
    """float64 -log of the f32 argument the kernel forms (f32 additions are IEEE: numpy's are the kernel's)."""
    p = np.asarray(p, F32)
    eps = F32(10e-6)
    arg = np.where(np.asarray(y) != 0, p + eps, F32(1.0) - p + eps).astype(F32)
    return -np.log(arg.astype(F64)), arg


def log_sweep_parts(got, p, y):
    """(worst absolute error where |log| <= 1, worst error relative to |log| where |log| > 1)."""
    ref, _ = log_sweep_ref(p, y)
    err = np.abs(f64(got) - ref)
    near = np.abs(ref) <= 1.0
    return float(err[near].max()), float((err[~near] / np.abs(ref[~near])).max())


def pow2_at_or_above(v):
    return 2.0 ** math.ceil(math.log2(v))


# ---------------------------------------------------------------------------- elementwise
ELEM_NS = (1, 255, 257, 4096 * 256 + 3)


def sigmoid_case(n):
    rng = np.random.default_rng(7400 + n % 1000)
    c = Case()
    c.n, c.name = n, "n=%d" % n
    c.z = (rng.standard_normal(n) * 4.0).astype(F32)
    plants = np.array([100.0, -100.0, 0.0, -0.0], F32)
    k = min(n, 4)
    c.z[:k] = plants[:k]
    if n > 8:
        c.z[-4:] = plants[::-1]
    c.dp = rng.standard_normal(n).astype(F32)
    return c


def sigmoid_bwd_ref(p, dp):
    p = f64(p)
    return prod((dp, 0.0), (p, 0.0), (1.0 - p, U * np.abs(1.0 - p)))


def relu6_case(n):
    rng = np.random.default_rng(7500 + n % 1000)
    c = Case()
    c.n, c.name = n, "n=%d" % n
    c.x = (rng.standard_normal(n) * 4.0 + 2.0).astype(F32)
    six = F32(6.0)
    plants = np.array([0.0, -0.0, 6.0, np.nextafter(six, F32(7)), np.nextafter(six, F32(0))], F32)
    k = min(n, 5)
    c.x[:k] = plants[:k]
    if n > 10:
        c.x[-5:] = plants[::-1]
    c.edge = np.nonzero((c.x == 0) | (c.x == six))[0]                   # where a gradient of 1 AT 0 and 6 would show
    c.dy = (rng.standard_normal(n) + 3.0).astype(F32)
    return c


def relu6_ref(x, dy):
    x = f64(x)
    return np.minimum(np.maximum(x, 0.0), 6.0), np.where((x > 0) & (x < 6), f64(dy), 0.0)


EMA_NS = (1, 257, 8192)
EMA_DECAYS = (0.999, 0.5)


def ema_case(n, decay):
    rng = np.random.default_rng(7600 + n)
    c = Case()
    c.n, c.decay, c.name = n, float(F32(decay)), "n=%d decay=%g" % (n, decay)
    c.moving = rng.standard_normal(n).astype(F32)
    c.batch = (rng.standard_normal(n) * 2.0).astype(F32)
    return c


def ema_ref(moving, batch, decay32):
    m, b = f64(moving), f64(batch)
    step = (1.0 - decay32) * (m - b)
    res = m - step
    return res, 3 * U * np.abs(step) + U * np.abs(res)


CAST_SHAPES = [(1, 1), (3, 257), (8, 1024)]


def cast_case(R, Cc):
    rng = np.random.default_rng(7700 + R + Cc)
    c = Case()
    c.R, c.C, c.name = R, Cc, "R=%d C=%d" % (R, Cc)
    x = (rng.standard_normal((R, Cc)) * np.exp(rng.standard_normal((R, Cc)) * 4.0)).astype(F32)
    bits = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x00012345, 0x80000400, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF,
                     0x007FFFFF, 0x00000000, 0x80000000], np.uint32).view(F32)   # ties (to even: down, up), around a tie, subnormals, +-inf, +-max
    flat = x.reshape(-1)
    k = min(flat.size, bits.size)
    flat[:k] = bits[:k]
    if flat.size > 2 * bits.size:
        flat[-bits.size:] = bits
    c.x = x
    return c


def cast_ref(x):
    """-> (bf16(x), bf16(x - bf16(x))) as bit patterns; x - hi is exact in f32 (inf - inf = NaN: lo is then NaN)."""
    x = np.asarray(x, F32)
    hi = bf16_bits(x)
    with np.errstate(invalid="ignore", over="ignore"):
        rest = (x.astype(F64) - bf16_to_f64(hi)).astype(F32)
    return hi, bf16_bits(rest)


def bits_equal_bf16(got_bits, ref_bits):
    """inf where the patterns differ (any two NaN patterns agree)."""
    g, r = np.asarray(got_bits).view(np.uint16), np.asarray(ref_bits).view(np.uint16)
    nan = lambda b: (b & 0x7FFF) > 0x7F80
    return np.where((g == r) | (nan(g) & nan(r)), 0.0, np.inf)


# ---------------------------------------------------------------------------- pooling and sampling
def dequant_ref(q):
    v = f64(q) * SC32 + BI32
    return v, U * (np.abs(v) + 2.0)


def l2n_ref(v, d_v):
    """Rows of v [.., F] known to d_v -> (v / sqrt(max(sum v^2, 1e-12)), bound)."""
    v, d_v = f64(v), np.broadcast_to(f64(d_v), np.shape(v))
    F = v.shape[-1]
    nrm = np.sqrt(np.maximum((v * v).sum(axis=-1, keepdims=True), 1e-12))
    Dss = 4 * math.ceil(F / 256) + 6
    rel = np.sqrt((d_v * d_v).sum(axis=-1, keepdims=True)) / nrm + ((Dss + 1) / 2 + 2) * U
    return prod((v, d_v), (1.0 / nrm, rel * (1.0 + 2.0 * rel) / nrm))


def meanpool_depth(T):
    ts = math.ceil(T / 32)
    return math.ceil(T / (4 * ts)) + 3 + ts + 2


def meanpool_ref(x, nfr, normalize):
    """x [B][T][F] f32 or uint8, nfr [B] -> (avg [B][F], bound)."""
    x = np.asarray(x)
    B, T, F = x.shape
    u8 = x.dtype == np.uint8
    nfr = np.asarray(nfr).astype(np.int64)
    if u8:
        v, d_v = dequant_ref(x)
    else:
        v, d_v = f64(x), np.zeros(x.shape)
    if normalize:
        v, d_v = l2n_ref(v, d_v)
    if u8:
        live = (np.arange(T)[None, :] < np.minimum(T, nfr)[:, None])[:, :, None]
        v, d_v = np.where(live, v, 0.0), np.where(live, d_v, 0.0)
    n = nfr.astype(F64)[:, None]
    avg = v.sum(axis=1) / n
    return avg, d_v.sum(axis=1) / n + meanpool_depth(T) * U * (np.abs(v) + d_v).sum(axis=1) / n


MP_B = 3
MP_TS = (1, 5, 33, 300)
MP_FS = (4, 252, 260, 1152, 1280)


def meanpool_case(T, F, u8):
    """num_frames = (1, T // 2 + 1, T).  Float frames beyond num_frames hold data (they count), uint8 frames beyond it hold 255 (they
    must not).  Float input: frame 0 of video 1 is all zero (the 1e-12 clamp under normalize)."""
    rng = np.random.default_rng(7800 + 7 * T + F + (1 if u8 else 0))
    c = Case()
    c.B, c.T, c.F, c.u8 = MP_B, T, F, u8
    c.name = "T=%d F=%d %s" % (T, F, "uint8" if u8 else "float")
    c.nfr = np.array([1, T // 2 + 1, T], np.int32)
    if u8:
        c.x = rng.integers(0, 256, size=(c.B, T, F)).astype(np.uint8)
        for b in range(c.B):
            c.x[b, c.nfr[b]:] = 255
    else:
        c.x = rng.standard_normal((c.B, T, F)).astype(F32)
        c.x[1, 0] = 0.0
    return c


def frames_index(u, nfr):
    """= oracle.model_math.sample_random_frames_index."""
    return (np.asarray(u, F32) * np.asarray(nfr).astype(F32)[:, None]).astype(np.int32)


def sequence_index(u, nfr, S):
    """= oracle.model_math.sample_random_sequence_index."""
    n = np.asarray(nfr).astype(np.int64)
    mx = np.maximum(n - S, 0)
    start = (np.asarray(u, F32).reshape(-1) * (mx + 1).astype(F32)).astype(np.int32).astype(np.int64)
    return np.minimum(start[:, None] + np.arange(S)[None, :], (n - 1)[:, None]).astype(np.int32)


def gather_ref(x, idx, nfr, normalize):
    """x [B][T][F] f32 or uint8, idx [B][S] -> (rows [B][S][F], bound).  Frame clamp(idx, 0, T-1); uint8: zeros when that is >= nfr."""
    x = np.asarray(x)
    B, T, F = x.shape
    ic = np.clip(np.asarray(idx).astype(np.int64), 0, T - 1)
    rows = x[np.arange(B)[:, None], ic]
    if x.dtype == np.uint8:
        v, d_v = dequant_ref(rows)
        pad = (ic >= np.asarray(nfr).astype(np.int64)[:, None])[:, :, None]
        v, d_v = np.where(pad, 0.0, v), np.where(pad, 0.0, d_v)
    else:
        v, d_v = f64(rows), np.zeros(rows.shape)
    return l2n_ref(v, d_v) if normalize else (v, d_v)


SG_B, SG_T = 3, 12
SG_SS = (1, 5, 30)
SG_FS = (4, 252, 1152)
SG_NFR = (1, 7, 12)


def _near(k, n, up):
    v = F32(k) / F32(n)
    return np.nextafter(v, F32(2.0) if up else F32(-1.0))


def sample_case(S, F, u8):
    """u [B][S] for the frame sampler: 0, nextafter(1, 0), values an ulp either side of k / n, and 1.0 (outside a uniform draw: it alone
    reaches idx == n).  useq [B]: one draw a video for the sequence sampler, the same kinds spread over the three S."""
    rng = np.random.default_rng(7900 + 7 * S + F + (1 if u8 else 0))
    c = Case()
    c.B, c.T, c.S, c.F, c.u8 = SG_B, SG_T, S, F, u8
    c.name = "S=%d F=%d %s" % (S, F, "uint8" if u8 else "float")
    c.nfr = np.array(SG_NFR, np.int32)
    if u8:
        c.x = rng.integers(0, 256, size=(c.B, c.T, F)).astype(np.uint8)
        for b in range(c.B):
            c.x[b, c.nfr[b]:] = 255
    else:
        c.x = rng.standard_normal((c.B, c.T, F)).astype(F32)
    one_m = np.nextafter(F32(1.0), F32(0.0))
    u = rng.random((c.B, S)).astype(F32)
    if S == 1:
        u[:, 0] = [0.0, one_m, 1.0]
    else:
        u[:, 0] = 0.0
        u[:, 1] = one_m
        u[:, 2] = 1.0
        for b in range(c.B):
            n = int(c.nfr[b])
            u[b, 3] = _near(max(n - 1, 1), n, False)
            u[b, 4] = _near(max(n // 2, 1), n, True) if n > 1 else F32(0.5)
        if S > 5:
            for b in range(c.B):
                n = int(c.nfr[b])
                for j, k in enumerate(range(1, min(n, 12))):
                    u[b, 5 + 2 * j] = _near(k, n, False)
                    u[b, 6 + 2 * j] = _near(k, n, True)
    c.u = u
    kinds = {1: [one_m, F32(1.0), F32(0.0)], 5: [F32(1.0), _near(1, 3, False), one_m], 30: [F32(0.0), one_m, F32(0.5)]}[S]
    c.useq = np.array(kinds, F32)
    return c


FP_SHAPES = [(3, 1, 5), (2, 30, 257), (3, 7, 64)]
FP_BWD_BIG = (9, 30, 8192)                                              # backward kernels alone: past the 8192- and 4096-block caps


def framepool_case(B, S, Cc):
    """y [B][S][C] N(0, 1); for the max: column 0 has its maximum at frames 0 and S - 1 (two equal), column 1 is equal over all S frames,
    column 2 is -inf throughout (video 0 only: the mean of the other videos stays finite)."""
    rng = np.random.default_rng(8000 + B + 3 * S + Cc)
    c = Case()
    c.B, c.S, c.C, c.name = B, S, Cc, "B=%d S=%d C=%d" % (B, S, Cc)
    c.y = rng.standard_normal((B, S, Cc)).astype(F32)
    c.y[:, 0, 0] = 9.0
    c.y[:, S - 1, 0] = 9.0
    c.y[:, :, 1] = 0.25
    c.ymax = c.y.copy()
    c.ymax[0, :, 2] = -np.inf
    c.dpooled = rng.standard_normal((B, Cc)).astype(F32)
    return c


def framepool_mean_ref(y):
    y = f64(y)
    S = y.shape[1]
    m = y.sum(axis=1) / S
    return m, (S - 1) * U * np.abs(y).sum(axis=1) / S + U * np.abs(m)


def framepool_mean_bwd_ref(dpooled, S):
    v, d = prod((f64(dpooled), 0.0), (1.0 / S, U / S))
    return np.repeat(v[:, None, :], S, axis=1), np.repeat(d[:, None, :], S, axis=1)


def framepool_max_ref(y):
    """-> (max [B][C], argmax [B][C] int32: the first maximum)."""
    y = f64(y)
    return y.max(axis=1), np.argmax(y, axis=1).astype(np.int32)


def framepool_max_bwd_ref(dpooled, argmax, S):
    sel = np.arange(S)[None, :, None] == np.asarray(argmax)[:, None, :]
    return np.where(sel, f64(dpooled)[:, None, :], 0.0)


FILL_NS = (1, 3, 4, 1027)
FILL_VALUES = (-0.0, 1.5)
