"""Float64 replay of the forward LSTM step kernels (csrc/evc_lstm_fwd.hip, lstm_fwd_epilogue), one step at a time, with a
derived per-element error bound on everything a step stores.  numpy only.  Used by tests/test_cpu_lstm_fwd_ref.py (the replay
against the oracle, an f32 emulation of the step, planted faults) and tests/test_gpu_lstm_fwd_parity.py (the kernels).  The
mirror image of tests/_bptt_ref.py: that file proves the backward steps right GIVEN the tape, this one checks the tape's writer.

What a step reads
-----------------
Step t of a layer reads x_t (the caller's bf16 or f16 values), h_{t-1} = slab t of the kernel's own hbuf (slab 0 is zeroed by
the entry), the weights [Kin+H][4H] in TF gate order i, j, f, o (stored transposed, wT [4H][Kin+H]), bias [4H] (forget_bias
1.0 is added to f), len, and the running f32 cell state, which lives in c_state and is updated in place: only its last value
is visible.  The replay is fed exactly those values - for the recurrent product of step t it takes the KERNEL's slab t - and
carries c itself in float64 together with a carried bound, so every step is checked on its own and differs from a correct
kernel only by f32 accumulation, the fast sigmoidf_ / tanhf_, and the final rounding of each store.

The step (active row: t < len)
------------------------------
    z    = [x_t | h_{t-1}] . W + bias (+ 1 on f)            (x-part possibly hoisted into an f32 workspace: same sum)
    i, f, o = sigmoid(z_i, z_f, z_o)    j = tanh(z_j)
    c_t  = c_{t-1} f + i j                                   c_{-1} = 0 whatever c_state held before the call
    h_t  = tanh(c_t) o
    stores: record t of `gates` = bf16 i, j, f, o (.x = i | j << 16, .y = f | o << 16); slab t+1 of c_all = bf16(c_t); slab t+1
            of hbuf = bf16(h_t) (f16 form: f16(h_t) in hbuf and bf16(h_t) in hbuf_bf16, both from the same f32 h_t);
            c_state = c_t (f32) at every active step; h_state = h_t (f32) at t == len - 1; state row = row_map[slot] under a
            row plan.
Inactive row (t >= len) inside the launch: slab t+1 of hbuf (and of the bf16 copy) is exactly zero, the state keeps the
values of step len - 1, a len == 0 row inside rows_per_step[0] gets an all-zero state at t == 0.  Nothing else of an
inactive row is written, and under a row plan nothing at all of the slots >= rows_per_step[t].

The bound (no measured constant enters it)
------------------------------------------
    u   = 2^-24   f32 unit roundoff
    eps = 2^-20   16 f32 ulps: the handful of roundings of an elementwise tail (1 + e, rcpf_ at 1 ulp, the products)
    r   = 2^-8 for a bf16 store, 2^-11 for an f16 store, u for the f32 states (round to nearest: half an ulp of the binade's
          lower end)

Pre-activation.  bf16 x bf16 and f16 x f16 products are exact in f32 (16 resp. 22 significant bits).  An f32 sum of K exact
products in ANY order, plus a few more additions (bias + forget_bias, the hoisted part added behind the loop), is off by at
most (K + 4) u times the sum of the magnitudes.  K is the full contraction length Kin + H whether or not the x-part was
hoisted.  With S = |a| . |W| + |bias| + 1 over the float64 operands:

    d_acc = (K + 4) u S

sigmoidf_(z) = rcpf_(1 + __expf(-z)) and tanhf_(z) = (1 - e) rcpf_(1 + e), e = __expf(-2|z|).  __expf scales its argument by
log2(e) in f32 (relative u: a shift of the argument by u |z|, doubled in tanhf_ whose argument is 2|z| - as a shift of z again
u |z|) and takes v_exp_f32 at 1 ulp = 2u relative (a shift of the argument by 2u, of z by at most 2u).  A relative error rho
of e IS a shift of z by rho, so both are charged to the pre-activation, with a factor 2 for the roundings in between:

    d_z   = d_acc + 2 u (|z| + 2)

Gates.  |g(z + d) - g(z)| <= |g'(z)| d + d^2 / 2 max|g''| and max|g''| < 1 for sigmoid and tanh alike; the rest of the fast
formula (1 + e, rcpf_, and in tanhf_ 1 - e, which cancels near z = 0 so that the error is ABSOLUTE there) is a few ulps of
values <= 2, far inside eps:

    d_g   = |g'(z)| d_z + d_z^2 + eps                        g' = g (1 - g) for sigmoid, 1 - g^2 for tanh; absolute

Cell state, carried.  The kernel's c_{t-1} is within d_c_prev of the replay's; the product rule with its second-order terms,
and eps for the two roundings of c f + i j relative to the magnitudes:

    d_c   = d_c_prev f + |c_prev| d_f + d_c_prev d_f + |j| d_i + |i| d_j + d_i d_j + eps (|c_prev f| + |i j|)

Hidden state.  tanhf_(c) sees c with the argument error of __expf as above, d_c' = d_c + 2 u (|c| + 2):

    d_t   = (1 - tanh^2 c) d_c' + d_c'^2 + eps
    d_h   = |o| d_t + |tanh c| d_o + d_t d_o + eps |tanh c  o|

Every stored value must satisfy

    |got - ref| <= r (|ref| + d) + d

(the f32 value is within d of the reference and rounding moves it by at most r of its own magnitude).  f16 subnormals
(|h| < 2^-14: absolute rounding step 2^-25) sit inside eps.  c_state is compared at the row's last step (d = d_c there, r = u),
h_state likewise (d = d_h).  Saturation: for z < -88 __expf(-z) overflows to +inf and rcpf_ gives 0 against a reference below
1e-38; for large |z| tanhf_ gives exactly 1: both inside eps.

Out of scope: the "high"-precision forms (evc_lstm_layer_fwd_f16_fp8lo, _f16_dith, _hp, evc_lstm_level2_fwd_high,
evc_lstm_stack2_fwd_f16*).  Their operands are composite images; they have oracle and bit-equality tests of their own.
replay_layer takes plain float64 operand matrices so that a later change can feed it decoded images.
"""
import numpy as np

from _bptt_ref import (EPS, RB, U, bf16_bits, bf16_round, bf16_to_f64, check_lens, check_plan, decode_tape, host_plan,  # noqa: F401
                       make_lens)

RH = 2.0 ** -11                                                         # f16 unit roundoff
GATES = "ijfo"
NAN16 = 0x7FC0                                                          # a NaN as bf16 and as f16
NAN_REC = np.uint32(0x7FC07FC0).view(np.int32)                          # a record half of two bf16 NaNs
NAN32 = np.uint32(0x7FC00000)


def _sigmoid(z):
    with np.errstate(over="ignore"):
        return np.where(z >= 0, 1.0 / (1.0 + np.exp(-np.abs(z))), np.exp(-np.abs(z)) / (1.0 + np.exp(-np.abs(z))))


def f16_bits(a):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(a, dtype=np.float32).astype(np.float16).view(np.uint16)


def f16_to_f64(bits):
    return np.ascontiguousarray(bits).view(np.uint16).view(np.float16).astype(np.float64)


def f16_round(a):
    return f16_to_f64(f16_bits(a))


# ---------------------------------------------------------------------------- the replay
def replay_layer(x, hbuf_kernel, W, bias, lens, row_map=None, rows_per_step=None, n_state_rows=None, requantise=bf16_round,
                 forget_bias=1.0):
    """One layer, steps 0 .. T-1.

    x              [T][M][Kin] float64, the caller's (bf16- or f16-exact) inputs, in slot order under a row plan
    hbuf_kernel    [T+1][M][H] float64, the kernel's own hbuf: step t reads slab t (only rows active at t are looked at).  None:
                   the replay chains its own h, re-quantised by `requantise` (None: not at all - the exact forward)
    W              [Kin+H][4H] float64, TF layout (column g*H+u), rows Kin.. are Wh
    bias           [4H] float64
    lens           [M] length of each row (slot, under a row plan)
    row_map        slot -> state row (row plan), rows_per_step [T] active prefix per step; must agree with lens
    n_state_rows   rows of c_state / h_state (default M)

    Returns a dict of float64 arrays:
      gates, gates_bound [T][M][H][4]   i, j, f, o of step t and d_g          z [T][M][H][4] the pre-activations
      c, c_bound [T][M][H]              c_t (what slab t+1 of c_all holds) and d_c
      h, h_bound [T][M][H]              h_t (slab t+1 of hbuf) and d_h
      c_state, c_state_bound, h_state, h_state_bound [rows][H]   the final state and its bound, by state row
      active [T][M] bool; launched [T][M] bool (slot < rows_per_step[t]); state_written [rows] bool
    """
    x = np.asarray(x, np.float64)
    T, M, Kin = x.shape
    W = np.asarray(W, np.float64)
    H = W.shape[1] // 4
    assert W.shape == (Kin + H, 4 * H)
    K = Kin + H
    bias = np.asarray(bias, np.float64).copy()
    fb = np.zeros(4 * H)
    fb[2 * H:3 * H] = forget_bias
    lens = np.asarray(lens).astype(np.int64)
    assert lens.shape == (M,)
    rows = np.arange(M) if row_map is None else np.asarray(row_map)[:M].astype(np.int64)
    R = (M if row_map is None else int(np.max(rows)) + 1) if n_state_rows is None else n_state_rows
    launched = np.ones((T, M), bool)
    if rows_per_step is not None:
        for t in range(T):
            assert np.all(np.nonzero(lens > t)[0] < rows_per_step[t]), "rows_per_step does not cover the rows active at step %d" % t
            launched[t, rows_per_step[t]:] = False
    out = {k: np.zeros((T, M, H, 4)) for k in ("gates", "gates_bound", "z")}
    out.update({k: np.zeros((T, M, H)) for k in ("c", "c_bound", "h", "h_bound")})
    active = np.zeros((T, M), bool)
    c = np.zeros((M, H))
    d_c = np.zeros((M, H))
    hl = np.zeros((M, H))                                               # h at the row's last step, and its bound
    d_hl = np.zeros((M, H))
    h_own = np.zeros((M, H))
    Wa = np.abs(W)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            act = (t < lens)[:, None]
            active[t] = act[:, 0]
            if t == 0:
                hp = np.zeros((M, H))
            elif hbuf_kernel is not None:
                hp = np.where(act, np.asarray(hbuf_kernel[t], np.float64), 0.0)      # (rows not active now: never read)
            else:
                hp = h_own
            a = np.concatenate([x[t], hp], axis=1)
            a = np.where(act, a, 0.0)
            z = a @ W + bias + fb
            S = np.abs(a) @ Wa + np.abs(bias) + 1.0
            d_z = (K + 4) * U * S + 2 * U * (np.abs(z) + 2.0)
            z4 = z.reshape(M, 4, H)
            dz4 = d_z.reshape(M, 4, H)
            gi, gf, go = _sigmoid(z4[:, 0]), _sigmoid(z4[:, 2]), _sigmoid(z4[:, 3])
            gj = np.tanh(z4[:, 1])
            sl = lambda g: g * (1.0 - g)
            d_i = sl(gi) * dz4[:, 0] + dz4[:, 0] ** 2 + EPS
            d_j = (1.0 - gj * gj) * dz4[:, 1] + dz4[:, 1] ** 2 + EPS
            d_f = sl(gf) * dz4[:, 2] + dz4[:, 2] ** 2 + EPS
            d_o = sl(go) * dz4[:, 3] + dz4[:, 3] ** 2 + EPS
            cn = c * gf + gi * gj
            d_cn = (d_c * gf + np.abs(c) * d_f + d_c * d_f + np.abs(gj) * d_i + np.abs(gi) * d_j + d_i * d_j
                    + EPS * (np.abs(c * gf) + np.abs(gi * gj)))
            tc = np.tanh(cn)
            d_ca = d_cn + 2 * U * (np.abs(cn) + 2.0)
            d_t = (1.0 - tc * tc) * d_ca + d_ca ** 2 + EPS
            hn = tc * go
            d_h = np.abs(go) * d_t + np.abs(tc) * d_o + d_t * d_o + EPS * np.abs(hn)
            a4 = act[..., None]
            out["gates"][t] = np.where(a4, np.stack([gi, gj, gf, go], axis=-1), 0.0)
            out["gates_bound"][t] = np.where(a4, np.stack([d_i, d_j, d_f, d_o], axis=-1), 0.0)
            out["z"][t] = np.where(a4, z4.transpose(0, 2, 1), 0.0)
            out["c"][t] = np.where(act, cn, 0.0)
            out["c_bound"][t] = np.where(act, d_cn, 0.0)
            out["h"][t] = np.where(act, hn, 0.0)
            out["h_bound"][t] = np.where(act, d_h, 0.0)
            c = np.where(act, cn, c)
            d_c = np.where(act, d_cn, d_c)
            hl = np.where(act, hn, hl)
            d_hl = np.where(act, d_h, d_hl)
            h_own = np.where(act, hn if requantise is None else requantise(hn), 0.0)
    wr = launched[0]                                                    # step 0 writes the zero state of the empty rows it covers
    for k, v in (("c_state", c), ("c_state_bound", d_c), ("h_state", hl), ("h_state_bound", d_hl)):
        full = np.zeros((R, H))
        full[rows[wr]] = v[wr]
        out[k] = full
    sw = np.zeros(R, bool)
    sw[rows[wr]] = True
    out.update(active=active, launched=launched, state_written=sw, rows=rows, lens=lens)
    return out


def replay_level2(x, hbuf0_kernel, hbuf1_kernel, W0, bias0, W1, bias1, lens, **kw):
    """Two layers: layer 1's x_t is the KERNEL's layer-0 slab t+1 (only its rows active at t are looked at).  Returns (r0, r1)."""
    r0 = replay_layer(x, hbuf0_kernel, W0, bias0, lens, **kw)
    if hbuf0_kernel is not None:
        x1 = np.where(r0["active"][:, :, None], np.asarray(hbuf0_kernel, np.float64)[1:], 0.0)
    else:
        rq = kw.get("requantise", bf16_round)
        x1 = r0["h"] if rq is None else rq(r0["h"])
    r1 = replay_layer(x1, hbuf1_kernel, W1, bias1, lens, **kw)
    return r0, r1


# ---------------------------------------------------------------------------- the check of one layer's outputs
def _ratio(got, ref, bound, r):
    lim = r * (np.abs(ref) + bound) + bound
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - ref)
        q = np.where(err == 0, 0.0, err / lim)                          # 0 / 0 (an exact zero against an exact zero) passes
    return np.where(np.isfinite(q), q, np.inf)


def _worst(q):
    at = np.unravel_index(int(np.argmax(q)), q.shape)
    return float(q[at]), tuple(int(v) for v in at)


def check_layer(rep, hbuf, gates, c_all, c_state, h_state, hbuf_bf16=None, h_f16=False):
    """Every element of everything the layer stored, as BIT PATTERNS the way the kernel left them in buffers prefilled with NaN
    (NAN16 in the 16-bit arrays, NAN_REC in the records, NAN32 in the states):

      hbuf [T+1][M][H] uint16 (bf16, or f16 with h_f16), hbuf_bf16 the same or None, gates [T][M][H][2] int32, c_all [T+1][M][H]
      uint16, c_state / h_state [rows][H] float32.

    Returns {output: ratio array}.  Outputs: "gates" [T][M][H][4], "c_all" [T+1][M][H], "hbuf" [T+1][M][H] (and "hbuf_bf16"),
    "c_state", "h_state" [rows][H].  Active elements: |got - ref| / (r (|ref| + d) + d), inf where not finite.  Where the kernel
    must leave a definite pattern, anything else is inf: slab 0 of hbuf all zero bits; slab t+1 of hbuf exactly zero for a
    launched inactive row; the prefill untouched in slab 0 of c_all, in every slot >= rows_per_step[t] of slab t+1 / record
    slab t, and in the state rows no launch covers.  (Records and c_all of a launched inactive row are read by nobody: ratio 0.)"""
    act, lau = rep["active"], rep["launched"]
    T, M = act.shape
    H = rep["c"].shape[2]
    res = {}
    gi, gj, gf, go, cs = decode_tape(gates, c_all)
    got = np.stack([gi, gj, gf, go], axis=-1)
    q = _ratio(got, rep["gates"], rep["gates_bound"], RB)
    raw = np.ascontiguousarray(gates).view(np.int32).reshape(T, M, H, 2)
    untouched = np.repeat(raw == NAN_REC, 2, axis=-1)                   # i, j live in .x, f, o in .y
    q = np.where(act[:, :, None, None], q, np.where(lau[:, :, None, None], 0.0, np.where(untouched, 0.0, np.inf)))
    res["gates"] = q

    def slabs(bits, ref, bound, r, dec, zero_inactive):
        bits = np.ascontiguousarray(bits).view(np.uint16).reshape(T + 1, M, H)
        qq = np.zeros((T + 1, M, H))
        qq[0] = np.where(bits[0] == (0 if zero_inactive else NAN16), 0.0, np.inf)
        body = _ratio(dec(bits[1:]), ref, bound, r)
        idle = np.where(bits[1:] == 0, 0.0, np.inf) if zero_inactive else np.zeros((T, M, H))
        qq[1:] = np.where(act[:, :, None], body, np.where(lau[:, :, None], idle, np.where(bits[1:] == NAN16, 0.0, np.inf)))
        return qq
    res["c_all"] = slabs(c_all, rep["c"], rep["c_bound"], RB, bf16_to_f64, False)
    res["hbuf"] = slabs(hbuf, rep["h"], rep["h_bound"], RH if h_f16 else RB, f16_to_f64 if h_f16 else bf16_to_f64, True)
    if hbuf_bf16 is not None:
        res["hbuf_bf16"] = slabs(hbuf_bf16, rep["h"], rep["h_bound"], RB, bf16_to_f64, True)
    sw = rep["state_written"][:, None]
    for name, arr in (("c_state", c_state), ("h_state", h_state)):
        arr = np.ascontiguousarray(arr, dtype=np.float32)
        body = _ratio(arr.astype(np.float64), rep[name], rep[name + "_bound"], U)
        res[name] = np.where(sw, body, np.where(arr.view(np.uint32) == NAN32, 0.0, np.inf))
    return res


OUTPUTS = ("gates", "c_all", "hbuf", "hbuf_bf16", "c_state", "h_state")


def worst_ratio(res):
    """{output: (worst ratio, index)} of check_layer's result.  Index: gates (t, slot, unit, gate); c_all / hbuf (slab, slot, unit)
    with slab = t + 1; states (state row, unit)."""
    return {k: _worst(res[k]) for k in OUTPUTS if k in res}


# EVC_FORCE_TILE -> (rows, units) of the forward tile (pick_fwd_tile in csrc/evc_lstm_fwd.hip)
TILES = {1: (256, 64), 2: (128, 32), 3: (64, 16), 4: (320, 64), 5: (288, 64), 6: (224, 64), 7: (192, 64), 8: (160, 64), 9: (128, 64),
         10: (64, 64), 11: (240, 64)}


def describe(output, ratio, at, tile=None, rep=None):
    """One output's worst place in words: step, row (slot), unit, which value, the row tile and unit tile it lies in (tile =
    (rows, units) of the launch's tile when known, else on the 256 / 128 / 64-row and 64 / 32 / 16-unit grids)."""
    if output in ("c_state", "h_state"):
        row, u = at
        slot = int(np.nonzero(rep["rows"] == row)[0][0]) if rep is not None and np.any(rep["rows"] == row) else row
        t = int(rep["lens"][slot]) - 1 if rep is not None else -1
        what = "%s state row=%d slot=%d" % (output, row, slot)
    elif output == "gates":
        t, slot, u, g = at
        what = "gate %s slot=%d" % (GATES[g], slot)
    else:
        t, slot, u = at[0] - 1, at[1], at[2]
        what = "%s slab=%d slot=%d" % (output, at[0], slot)
    if tile is not None:
        where = "row tile %d of %d, unit tile %d of %d" % (slot // tile[0], tile[0], u // tile[1], tile[1])
    else:
        where = "row tile %d of 256, %d of 128, %d of 64; unit tile %d of 64, %d of 32, %d of 16" % (
            slot // 256, slot // 128, slot // 64, u // 64, u // 32, u // 16)
    return "%.4f at t=%d %s unit=%d (%s)" % (ratio, t, what, u, where)


# ---------------------------------------------------------------------------- the cases (shared by the CPU and the GPU tests)
T_STEPS = 4
T_SAT = 6
# (M, Kin, H): two row tiles with a ragged second one on every tile height and 2 / 4 / 8 unit tiles; Kin != H, two K segments
# of different length; a single unit tile with the H - 4 bias clamp at its end
SHAPES = [(330, 64, 128), (200, 192, 256), (70, 64, 64)]
HOIST_SHAPE = (200, 192, 256)
STACK2_SHAPES = [(70, 64, 128), (200, 192, 256)]
SAT_SHAPE = (70, 64, 128)
SAT_SCALE = 24.0                                                        # weights x 24: |z| reaches 40 - 90 (asserted by the CPU test)


class Case:
    pass


def make_case(M, Kin, H, planned, nlayers=1, fmt="bf16", saturated=False):
    """Operands of a case as float64 (exact in `fmt`), in slot order under a row plan.  x ~ 0.5 N(0, 1), Glorot x 2 weights,
    bias ~ 0.1 N(0, 1) (f32), as in test_lstm_layer_fwd_and_bwd.  saturated: T = 6, weights and bias scaled so that |z| reaches
    40 - 90 (gates exactly 0 and 1 in bf16), the first 8 units biased to i = j = f = 1 so that |c| grows by 1 a step."""
    rd = bf16_round if fmt == "bf16" else f16_round
    T = T_SAT if saturated else T_STEPS
    seed = 5000 + M + 3 * Kin + 7 * H + 11 * planned + 13 * nlayers + (17 if fmt == "f16" else 0) + (19 if saturated else 0)
    rng = np.random.default_rng(seed)
    c = Case()
    c.M, c.Kin, c.H, c.T, c.planned, c.nlayers, c.fmt = M, Kin, H, T, planned, nlayers, fmt
    c.name = "M=%d Kin=%d H=%d plan=%d%s" % (M, Kin, H, planned, " saturated" if saturated else "")
    c.lens_rows = make_lens(seed, M, T, 0.15 if planned else 0.0)
    check_lens(c.lens_rows, T)
    if planned:
        c.inv, c.P, c.rows = host_plan(c.lens_rows, T)
        check_plan(c.P, c.rows, tile=128 if M >= 200 else 32)
        assert all(a > b for a, b in zip(c.rows, c.rows[1:]))          # the two roles of a level2 launch (steps s and s - 1) differ in rows
        c.lens = c.lens_rows[c.inv[:c.P]]
    else:
        c.inv, c.P, c.rows, c.lens = None, M, None, c.lens_rows
    c.x = rd(rng.standard_normal((T, c.P, Kin)) * 0.5)
    c.W, c.bias = [], []
    for l in range(nlayers):
        nin = Kin if l == 0 else H
        w = glorot_uniform(rng, (nin + H, 4 * H)) * 2.0
        b = rng.standard_normal(4 * H) * 0.1
        if saturated:
            w, b = w * SAT_SCALE, b * SAT_SCALE
            for g in (0, 1, 2):
                b[g * H:g * H + 8] = 30.0
                w[:, g * H:g * H + 8] *= 0.01
        c.W.append(rd(w))
        c.bias.append(b.astype(np.float32).astype(np.float64))
    return c


def glorot_uniform(rng, shape):
    lim = np.sqrt(6.0 / (shape[0] + shape[1]))
    return rng.uniform(-lim, lim, size=shape)
