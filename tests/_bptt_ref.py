"""Float64 replay of the BPTT step kernels' own tape (csrc/evc_lstm_bwd.hip), one step at a time, with a derived
per-element error bound.  numpy only.  Used by tests/test_cpu_bptt_ref.py (the replay against the oracle, an f32 emulation
of the step, planted faults) and tests/test_gpu_bptt_parity.py (the kernels).

What a step reads
-----------------
Step t of a layer reads the saved tape (`gates` slab t: 8-byte records of bf16 i, j, f, o; `c_all` slabs t and t+1, bf16),
the bf16 weights in the backward layout, `len`, the final-state gradient `dS`, the gradient from the layer above (as bf16
`dh_above`, or as `dz_above` + `w_above` contracted in the same launch), and `dz_{t+1}`, which the previous launch wrote
as bf16.  Only the carried cell-state gradient `dc` is hidden.  The replay is fed exactly those values - for the recurrent
product of step t it takes the KERNEL's dz_{t+1} - and carries dc itself in float64, so every step is checked on its own
and differs from a correct kernel only by f32 accumulation, the fast tanhf_, and the final bf16 rounding of dz.

The step (active row: t < len; `last`: t == len - 1)
---------------------------------------------------
    acc  = dz_{t+1} . Wh^T  (+ dz_above_t . Wx_above^T in the fused and pair forms)
    dh   = acc                     not last
           dS_h                    last, plain form   (the product is REPLACED)
           acc + dS_h              last, fused form   (the product still holds the gradient from above: ADDED)
    dh  += dh_above_t              (plain form with an upper layer)
    dc   = dc_in + dh o (1 - tc^2)           tc = tanh(c_t), dc_in = dS_c at the last step, else the carry
    dz_i = dc j i (1 - i)   dz_j = dc i (1 - j^2)   dz_f = dc c_{t-1} f (1 - f)   dz_o = dh tc o (1 - o)     (c_{-1} = 0)
    carry: dc f
Inactive (row, step) pairs get dz = 0 exactly.

The bound (no measured constant enters it)
------------------------------------------
    u   = 2^-24   f32 unit roundoff
    rb  = 2^-8    bf16 unit roundoff: round-to-nearest-even to 8 significant bits is off by up to half an ulp = 2^-8 of the
                  binade's lower end, so up to 2^-8 relative (not 2^-9)
    eps = 2^-20   16 f32 ulps: the ~10 roundings of the elementwise tail plus __expf / rcpf_ inside tanhf_

An f32 sum of K exact products (bf16 x bf16 is exact in f32) in ANY order, plus a few more additions, is off by at most
(K + 4) u times the sum of the magnitudes, so with S = sum_k |a_k| |b_k| over the operands of the float64 product (0 where
the product is not used: t == T-1 for the recurrent part, the row's last step in the plain form)

    d_dh  = (K + 4) u (S + |dS_h used| + |dh_above|)              K = 4H, or 8H in the fused and pair forms
    q     = dh o (1 - tc^2)
    d_q   = d_dh |o (1 - tc^2)| + eps |dh o|                      second term ABSOLUTE in the tanh factor: 1 - tc^2 cancels
                                                                  for large |c|, its error does not shrink with it
    d_dc  = d_dcin + d_q + eps (|dc_in| + |q|)                    d_dcin = u |dS_c| at the last step, else the carried bound
    d_dzg = d_dc |G_g| + eps |dz_ref|                             g = i, j, f;  G = dz_g / dc
    d_dzo = d_dh |tc o (1 - o)| + eps |dh o| + eps |dz_ref|
    carry: d_dc f + eps |dc f|       (+ rb |dc f| when the kernel rounds the carry to bf16, EVC_BWD_DC_BF16=1)

and the kernel's bf16 result must satisfy, for each of the four gate values of every active (row, unit, step),

    |dz_got - dz_ref| <= rb (|dz_ref| + d_dz) + d_dz

(the f32 value is within d_dz of the reference, and rounding it moves it by at most rb of its own magnitude).

EVC_BWD_DC_BF16=1: the carry crosses the launch boundary as bf16(dc f), in the kernel and in the replay alike, and the carry
bound takes the rb |dc f| of that rounding.  (To first order: the two round nearly equal numbers and so, all but always, the
same way.  Should a value sit within the carried bound of a rounding boundary, the two can land a whole bf16 ulp apart, which
one rb term does not cover - the check would then report that element, and the report would name this cause.)

db (summed in f32 from the unrounded dz, float atomics): against the float64 sum of the unrounded reference dz, per gate
column, within  sum d_dz + n_active u sum |dz_ref|.
"""
import numpy as np

U = 2.0 ** -24
RB = 2.0 ** -8
EPS = 2.0 ** -20
GATES = "ijfo"


# ---------------------------------------------------------------------------- bf16 <-> numpy
def bf16_bits(a):
    """float -> bf16 bit patterns (uint16), round to nearest even (NaN stays NaN)."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    r = ((b.astype(np.uint64) + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, np.uint16(0x7FC0), r)


def bf16_to_f64(bits):
    """bf16 bit patterns ((u)int16) -> float64."""
    b = np.ascontiguousarray(bits).view(np.uint16).astype(np.uint32) << 16
    with np.errstate(invalid="ignore"):                                # (a signalling NaN in a record nobody reads)
        return b.view(np.float32).astype(np.float64)


def bf16_round(a):
    return bf16_to_f64(bf16_bits(a))


def pack_gates(i, j, f, o):
    """bf16-exact i, j, f, o [..] -> int32 records [.., 2]: .x = i | j << 16, .y = f | o << 16."""
    x = bf16_bits(i).astype(np.uint32) | (bf16_bits(j).astype(np.uint32) << 16)
    y = bf16_bits(f).astype(np.uint32) | (bf16_bits(o).astype(np.uint32) << 16)
    return np.stack([x, y], axis=-1).view(np.int32)


def decode_tape(gates_int32, c_all_bf16):
    """gates [T][M][H][2] int32 records, c_all [(T+1)][M][H] bf16 bit patterns ((u)int16) -> i, j, f, o [T][M][H] and
    c [(T+1)][M][H] as float64.  A record's .x holds i in the low and j in the high 16 bits, .y holds f low and o high."""
    g = np.ascontiguousarray(gates_int32).view(np.uint32)
    x, y = g[..., 0], g[..., 1]
    lo = lambda w: bf16_to_f64((w & 0xFFFF).astype(np.uint16))
    hi = lambda w: bf16_to_f64((w >> 16).astype(np.uint16))
    return lo(x), hi(x), lo(y), hi(y), bf16_to_f64(c_all_bf16)


def interleave_w(kernel, H):
    """TF-layout kernel [in+H][4H] (column g*H+u) -> the backward layout (column u*4+g)."""
    n = kernel.shape[0]
    return np.ascontiguousarray(kernel.reshape(n, 4, H).transpose(0, 2, 1).reshape(n, 4 * H))


# ---------------------------------------------------------------------------- the replay
def replay_layer(tape, lens, W_il, dS_c, dS_h, dh_above=None, dz_above=None, w_above=None, dz_kernel=None,
                 row_map=None, rows_per_step=None, dc_bf16=False):
    """One layer, steps T-1 .. 0.

    tape           (i, j, f, o, c) from decode_tape, float64
    lens           [M] length of each row (slot, under a row plan)
    W_il           [Kin+H][4H] the bf16 weights as float64, backward layout (column u*4+g); rows Kin.. are Wh
    dS_c, dS_h     [rows][H] final-state gradient, indexed by row_map[slot] under a row plan
    dh_above       [T][M][H] bf16-exact gradient on the outputs (plain form), or None
    dz_above, w_above   fused form: the upper layer's dz [T][M][4H] and its backward-layout kernel (first H rows = Wx_above)
    dz_kernel      [T][M][4H] the kernel's dz as float64: step t's recurrent product reads slab t+1 of it.  None: the
                   replay chains its own unrounded dz (the exact BPTT of the tape)
    rows_per_step  [T] active prefix per step (row plan); must agree with lens
    dc_bf16        EVC_BWD_DC_BF16=1: the carry is rounded to bf16 and its bound widened by rb |dc f| (see the module docstring)

    Returns a dict: dz [T][M][H][4], bound (same shape), active [T][M] bool, db [4H] (index g*H+u) and db_bound [4H].
    """
    gi, gj, gf, go, c = tape
    T, M, H = gi.shape
    lens = np.asarray(lens).astype(np.int64)
    assert lens.shape == (M,) and c.shape == (T + 1, M, H)
    Kin = W_il.shape[0] - H
    assert W_il.shape == (Kin + H, 4 * H)
    Wh = W_il[Kin:]
    fused = dz_above is not None
    assert fused == (w_above is not None) and not (fused and dh_above is not None)
    Wxa = np.asarray(w_above)[:H] if fused else None
    K = 8 * H if fused else 4 * H
    rows = np.arange(M) if row_map is None else np.asarray(row_map)[:M].astype(np.int64)
    dSc, dSh = np.asarray(dS_c, np.float64)[rows], np.asarray(dS_h, np.float64)[rows]
    if rows_per_step is not None:
        for t in range(T):
            assert np.all(np.nonzero(lens > t)[0] < rows_per_step[t]), "rows_per_step does not cover the rows active at step %d" % t
    dz = np.zeros((T, M, H, 4))
    bound = np.zeros((T, M, H, 4))
    active = np.zeros((T, M), bool)
    dc = np.zeros((M, H))
    d_dc = np.zeros((M, H))
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T - 1, -1, -1):
            act = (t < lens)[:, None]
            last = (t == lens - 1)[:, None]
            active[t] = act[:, 0]
            acc = np.zeros((M, H))
            S = np.zeros((M, H))
            if t + 1 < T:
                nxt = dz_kernel[t + 1] if dz_kernel is not None else dz[t + 1].reshape(M, 4 * H)
                nxt = np.asarray(nxt, np.float64).reshape(M, 4 * H)
                acc += nxt @ Wh.T
                S += np.abs(nxt) @ np.abs(Wh).T
            if fused:
                za = np.asarray(dz_above[t], np.float64).reshape(M, 4 * H)
                acc += za @ Wxa.T
                S += np.abs(za) @ np.abs(Wxa).T
            if fused:
                dh = acc + np.where(last, dSh, 0.0)
                mag = S + np.where(last, np.abs(dSh), 0.0)
            else:
                dh = np.where(last, dSh, acc)
                mag = np.where(last, np.abs(dSh), S)
            if dh_above is not None:
                da = np.asarray(dh_above[t], np.float64)
                dh = dh + da
                mag = mag + np.abs(da)
            d_dh = (K + 4) * U * mag
            i, j, f, o = gi[t], gj[t], gf[t], go[t]
            tc = np.tanh(c[t + 1])
            omt = 1.0 - tc * tc
            cp = c[t] if t > 0 else np.zeros((M, H))
            q = dh * o * omt
            d_q = d_dh * np.abs(o * omt) + EPS * np.abs(dh * o)
            dc_in = np.where(last, dSc, dc)
            d_in = np.where(last, U * np.abs(dSc), d_dc)
            dcn = dc_in + q
            d_dcn = d_in + d_q + EPS * (np.abs(dc_in) + np.abs(q))
            G = np.stack([j * i * (1 - i), i * (1 - j * j), cp * f * (1 - f)], axis=-1)
            z = np.concatenate([dcn[..., None] * G, (dh * tc * o * (1 - o))[..., None]], axis=-1)
            b = np.concatenate([d_dcn[..., None] * np.abs(G), (d_dh * np.abs(tc * o * (1 - o)) + EPS * np.abs(dh * o))[..., None]], axis=-1)
            b = b + EPS * np.abs(z)
            a4 = act[..., None]
            dz[t] = np.where(a4, z, 0.0)
            bound[t] = np.where(a4, b, 0.0)
            car = dcn * f
            d_car = d_dcn * np.abs(f) + EPS * np.abs(car)
            if dc_bf16:
                d_car = d_car + RB * np.abs(car)
            if dc_bf16:
                car = bf16_round(car)
            dc = np.where(act, car, dc)
            d_dc = np.where(act, d_car, d_dc)
    n_act = int(active.sum())
    db = dz.sum(axis=(0, 1)).T.reshape(4 * H)                           # [4][H] -> index g*H+u
    db_bound = (bound.sum(axis=(0, 1)) + n_act * U * np.abs(dz).sum(axis=(0, 1))).T.reshape(4 * H)
    return {"dz": dz, "bound": bound, "active": active, "db": db, "db_bound": db_bound}


def replay_stack2(tape0, tape1, lens, W_il0, W_il1, dS, dz0_kernel, dz1_kernel, row_map=None, rows_per_step=None, dc_bf16=False):
    """Two-layer stack (evc_lstm_stack2_bwd, or the layer-after-layer fused calls): layer 1 in the plain form, layer 0 in the
    fused form with dz_above = the kernel's dz1.  dS [rows][4H] = d(final state) as [c0 | h0 | c1 | h1].  Returns (r0, r1)."""
    H = tape0[0].shape[2]
    dS = np.asarray(dS, np.float64)
    r1 = replay_layer(tape1, lens, W_il1, dS[:, 2 * H:3 * H], dS[:, 3 * H:], dz_kernel=dz1_kernel, row_map=row_map,
                      rows_per_step=rows_per_step, dc_bf16=dc_bf16)
    T, M = tape0[0].shape[:2]
    above = dz1_kernel if dz1_kernel is not None else r1["dz"].reshape(T, M, 4 * H)      # (no kernel output: the exact chain)
    r0 = replay_layer(tape0, lens, W_il0, dS[:, :H], dS[:, H:2 * H], dz_above=above, w_above=W_il1, dz_kernel=dz0_kernel,
                      row_map=row_map, rows_per_step=rows_per_step, dc_bf16=dc_bf16)
    return r0, r1


def worst_ratio(dz_got, dz_ref, bound, mask):
    """max over the active (step, row, unit, gate) of |got - ref| / (rb (|ref| + bound) + bound), and where it is, as
    (t, row, unit, gate).  Inactive elements must be exactly zero: any that is not (NaN included) gives inf at its place.  A
    non-finite value at an active element gives inf too."""
    T, M, H, _ = dz_ref.shape
    got = np.asarray(dz_got, np.float64).reshape(T, M, H, 4)
    m4 = np.broadcast_to(np.asarray(mask, bool)[:, :, None, None], got.shape)
    lim = RB * (np.abs(dz_ref) + bound) + bound
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - dz_ref)
        ratio = np.where(err == 0, 0.0, err / lim)                     # 0 / 0 (an exact zero against an exact zero) passes
    ratio = np.where(np.isfinite(ratio), ratio, np.inf)
    ratio = np.where(m4, ratio, np.where(got == 0, 0.0, np.inf))
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), tuple(int(v) for v in at)


def db_ratio(db_got, rep):
    """max |db_got - db_ref| / db_bound and the [4H] index (g*H+u) where it is."""
    err = np.abs(np.asarray(db_got, np.float64) - rep["db"])
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, err / rep["db_bound"])
    r = np.where(np.isfinite(r), r, np.inf)
    k = int(np.argmax(r))
    return float(r[k]), k


def describe(ratio, at):
    t, m, u, g = at
    return "%.4f at t=%d row=%d unit=%d gate=%s (row tile %d of 128, %d of 32; unit tile %d of 128)" % (
        ratio, t, m, u, GATES[g], m // 128, m // 32, u // 128)


# ---------------------------------------------------------------------------- the cases (shared by the CPU and the GPU tests)
T_STEPS = 4
# evc_lstm_layer_bwd, plain form: (M, Kin, H, planned, dh_above given, db requested)
LAYER_CASES = [(200, 192, 256, False, True, True), (200, 64, 256, True, False, False), (70, 64, 64, False, True, True)]
# fused form (dz_above / w_above), Kin = 64: (M, H, planned)
FUSED_CASES = [(200, 128, False), (200, 128, True), (200, 256, False), (200, 256, True)]
# evc_lstm_stack2_bwd, Kin0 = 192: (M, H, planned); M <= 512: skinny pair launches, M > 512: the 128 x 128 pair kernel
STACK2_CASES = [(70, 128, False), (70, 128, True), (200, 256, False), (200, 256, True),
                (520, 128, False), (520, 128, True), (520, 256, False), (520, 256, True)]
FUSED_KIN, STACK2_KIN = 64, 192
SAT_M, SAT_H = 70, 128                                                  # the saturated synthetic tape


def make_lens(seed, M, T, zero_frac=0.0):
    """Ragged lengths (longer ones more likely) holding 0, 1 and T, every value 1..T (so at every t some row has its last
    step), and a full-length row in every block of 32 rows (so every row tile of the unplanned layout has an active row at
    every step).  zero_frac: extra share of empty rows (what a row plan drops)."""
    rng = np.random.default_rng(seed)
    w = np.arange(T + 1) + 2.0
    lens = rng.choice(T + 1, size=M, p=w / w.sum()).astype(np.int32)
    if zero_frac > 0:
        lens[rng.random(M) < zero_frac] = 0
    for r0 in range(0, M, 32):
        lens[min(r0 + 5, M - 1)] = T
    lens[:3] = [0, T, 1]
    lens[6:6 + T] = np.arange(1, T + 1)
    return lens


def case_lens(kind, M, H, planned, T=None):
    """The lengths of a shared case (the CPU emulation and the GPU test use the same ones)."""
    T = T_STEPS if T is None else T
    lens = make_lens({"layer": 10, "fused": 20, "stack2": 30, "sat": 40}[kind] + M + H, M, T, 0.15 if planned else 0.0)
    if planned and M > 512:      # keep the planned row count above 512 (the 128 x 128 pair kernel, not the skinny launches): few empty rows
        lens[np.nonzero(lens == 0)[0][3:]] = 2
    return lens


def check_lens(lens, T, tile=32):
    lens = np.asarray(lens)
    M = lens.shape[0]
    assert {0, 1, T} <= set(lens.tolist())
    act = np.arange(T)[:, None] < lens[None, :]
    assert act.mean() >= 0.4, act.mean()
    for t in range(T):
        assert np.any(lens - 1 == t)                                   # some row has its last step here
        for r0 in range(0, M, tile):
            assert act[t, r0:r0 + tile].any(), (t, r0)
    return act


def host_plan(lens, T):
    """What ops.RowPlan computes, on the host: (inv = row of each slot, longest first; P; rows per step)."""
    lens = np.asarray(lens)
    M = lens.shape[0]
    inv = np.argsort(-lens.astype(np.int64), kind="stable").astype(np.int32)
    rows = [int((lens > t).sum()) for t in range(T)]
    P = min(M, max(32, -(-rows[0] // 32) * 32))
    return inv, P, rows


def check_plan(P, rows, tile=128):
    """Some step cuts the active prefix inside a row tile, and some row tile lies entirely beyond it."""
    assert any(r % tile for r in rows) and any(r % 32 for r in rows), rows
    assert any(-(-max(r, 1) // tile) * tile < P for r in rows), (rows, P)


def synthetic_saturated_tape(seed, M, T, H, lens):
    """A tape no forward would write but every BPTT step must survive: gate values of exactly 0 and 1, |j| = 1, |c| up to
    20 (1 - tc^2 cancels), c slab 0 = NaN (never read: c_old at t == 0 is 0), and NaN records wherever the row is inactive
    (nothing of an inactive row is read).  Returns (gates int32 [T][M][H][2], c_all bf16 bits uint16 [(T+1)][M][H])."""
    rng = np.random.default_rng(seed)

    def gate(lo, hi):
        v = rng.uniform(lo, hi, size=(T, M, H))
        k = rng.integers(0, 6, size=(T, M, H))
        return bf16_round(np.where(k == 0, lo, np.where(k == 1, hi, v)))
    i, f, o = gate(0.0, 1.0), gate(0.0, 1.0), gate(0.0, 1.0)
    j = gate(-1.0, 1.0)
    c = bf16_round(rng.standard_normal((T + 1, M, H)) * np.where(rng.random((T + 1, M, H)) < 0.3, 10.0, 1.0))
    c = np.clip(c, -20.0, 20.0)
    c[1:, :, :4] = np.array([20.0, -20.0, 9.0, 0.0])
    c[0] = np.nan
    act = (np.arange(T)[:, None] < np.asarray(lens)[None, :])[:, :, None]
    nan = np.full((T, M, H), np.nan)
    i, j, f, o = (np.where(act, a, nan) for a in (i, j, f, o))
    c[1:] = np.where(act, c[1:], np.nan)
    return pack_gates(i, j, f, o), bf16_bits(c)
