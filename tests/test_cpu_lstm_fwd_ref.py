"""tests/_lstm_fwd_ref.py without a GPU: the float64 replay of the forward step is the oracle's forward, an honest f32 emulation
of the step kernels stays inside the derived bound on every case the GPU test uses (the saturated one included), and planted
faults leave it - at the place each fault predicts.

Ratios of the emulation (worst |got - ref| / limit of a case): 0.93 - 0.99 on the bf16 stores, which are rounding dominated, 0.71 -
0.88 on the f16 store of h (8x finer: the accumulation term weighs as much as the rounding), below 0.01 on the f32 states."""
import numpy as np
import pytest

import _lstm_fwd_ref as fr
from oracle import model_math as mm

F32 = np.float32


# ---------------------------------------------------------------------------- f32 emulation of a layer's forward steps
def expf_(x):
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(x.astype(F32)).astype(F32)


def sigmoidf_(x):
    return (F32(1.0) / (F32(1.0) + expf_(-x))).astype(F32)


def tanhf_(x):
    e = expf_(F32(-2.0) * np.abs(x).astype(F32))
    t = ((F32(1.0) - e) / (F32(1.0) + e)).astype(F32)
    return np.copysign(t, x).astype(F32)


def trunc_bf16_bits(a):
    return (np.ascontiguousarray(a, dtype=F32).view(np.uint32) >> 16).astype(np.uint16)


def emulate_layer(x, W, bias, lens, T, fmt="bf16", row_map=None, rows_per_step=None, n_state_rows=None, seed=0, fault=None, arg=None):
    """What a correct kernel leaves in its buffers, in numpy f32 - or, with `fault`, a kernel that is wrong in one named way.
    Buffers are prefilled the way the GPU test prefills them.  Returns a dict of bit patterns for fr.check_layer."""
    rng = np.random.default_rng(seed)
    _, M, Kin = x.shape
    H = W.shape[1] // 4
    lens = np.asarray(lens)
    R = M if n_state_rows is None else n_state_rows
    rows = np.arange(M) if (row_map is None or fault == "ignore_row_map") else np.asarray(row_map)[:M]
    hbits = fr.bf16_bits if fmt == "bf16" else fr.f16_bits
    hdec = fr.bf16_to_f64 if fmt == "bf16" else fr.f16_to_f64
    hbuf = np.full((T + 1, M, H), fr.NAN16, np.uint16)
    hbuf[0] = 0
    hbf = np.full((T + 1, M, H), fr.NAN16, np.uint16)
    hbf[0] = 0
    gates = np.full((T, M, H, 2), fr.NAN_REC, np.int32)
    c_all = np.full((T + 1, M, H), fr.NAN16, np.uint16)
    c_state = np.full((R, H), fr.NAN32, np.uint32).view(F32)
    h_state = np.full((R, H), fr.NAN32, np.uint32).view(F32)
    b = np.asarray(bias, F32).copy()
    if fault == "bias_clamp":                                           # the last 4 units read the previous 4 units' bias
        b4 = b.reshape(4, H)
        b4[:, H - 4:] = b4[:, H - 8:H - 4]
    if fault != "no_forget_bias":
        b[2 * H:3 * H] += F32(1.0)
    Wf = np.asarray(W, F32)
    eff = lens.copy()
    if fault == "advance_row":
        eff[arg] += 1
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            Mt = M if rows_per_step is None else rows_per_step[t]
            a = np.concatenate([x[t].astype(F32), hdec(hbuf[t]).astype(F32)], axis=1)
            acc = np.broadcast_to(b, (M, 4 * H)).astype(F32)
            for k in rng.permutation((Kin + (H if t > 0 else 0)) // 32):                   # K in shuffled 32-wide chunks
                part = (a[:, k * 32:(k + 1) * 32] @ Wf[k * 32:(k + 1) * 32]).astype(F32)
                if fault == "drop_chunk" and k == arg[0]:
                    part.reshape(M, 4, H)[:, :, arg[1]] = 0
                acc = (acc + part).astype(F32)
            z = acc.reshape(M, 4, H)
            zi, zj, zf, zo = z[:, 0], z[:, 1], z[:, 2], z[:, 3]
            if fault == "swap_jf":
                zj, zf = zf, zj
            gi, gf, go = sigmoidf_(zi), sigmoidf_(zf), sigmoidf_(zo)
            gj = sigmoidf_(zj) if fault == "sigmoid_j" else tanhf_(zj)
            if t == 0:
                co = np.full((M, H), F32(3.0)) if fault == "c_state_at_0" else np.zeros((M, H), F32)
            else:
                co = np.zeros((M, H), F32)
                co[:Mt] = c_state[rows[:Mt]]
            cn = (co * gf + (gi * gj).astype(F32)).astype(F32)
            hn = (tanhf_(cn) * go).astype(F32)
            rec = fr.bf16_bits
            ri, rj = (gj, gi) if fault == "swap_ij_record" else (gi, gj)
            gx = rec(ri).astype(np.uint32) | (rec(rj).astype(np.uint32) << 16)
            gy = rec(gf).astype(np.uint32) | (rec(go).astype(np.uint32) << 16)
            for m in range(Mt):
                if t >= eff[m]:
                    hbuf[t + 1, m] = 0
                    hbf[t + 1, m] = 0
                    if t == 0:
                        c_state[rows[m]] = 0
                        h_state[rows[m]] = 0
                    if fault == "h_state_late" and t == eff[m] and eff[m] > 0:             # the condition t == len, evaluated as if live
                        h_state[rows[m]] = hn[m]
                    continue
                c_state[rows[m]] = cn[m]
                c_all[t if fault == "c_all_slab" else t + 1, m] = fr.bf16_bits(cn[m])
                if fault == "h_state_late" or t == eff[m] - 1:
                    h_state[rows[m]] = hn[m]
                hbuf[t + 1, m] = trunc_bf16_bits(hn[m]) if fault == "truncate_h" else hbits(hn[m])
                hbf[t + 1, m] = fr.bf16_bits(hn[m])
                gates[t, m, :, 0] = gx[m].view(np.int32)
                gates[t, m, :, 1] = gy[m].view(np.int32)
    return dict(hbuf=hbuf, gates=gates, c_all=c_all, c_state=c_state, h_state=h_state, hbuf_bf16=hbf if fmt == "f16" else None)


def run(c, fmt=None, layer=0, x=None, **kw):
    fmt = c.fmt if fmt is None else fmt
    x = c.x if x is None else x
    o = emulate_layer(x, c.W[layer], c.bias[layer], c.lens, c.T, fmt=fmt, row_map=c.inv, rows_per_step=c.rows, n_state_rows=c.M, **kw)
    dec = fr.bf16_to_f64 if fmt == "bf16" else fr.f16_to_f64
    rep = fr.replay_layer(x, dec(o["hbuf"]), c.W[layer], c.bias[layer], c.lens, row_map=c.inv, rows_per_step=c.rows, n_state_rows=c.M)
    res = fr.check_layer(rep, o["hbuf"], o["gates"], o["c_all"], o["c_state"], o["h_state"], hbuf_bf16=o["hbuf_bf16"], h_f16=fmt == "f16")
    return o, rep, res


# ---------------------------------------------------------------------------- the replay is the oracle's forward
@pytest.mark.parametrize("nlayers", [1, 2])
@pytest.mark.parametrize("planned", [False, True])
def test_replay_chained_on_its_own_h_is_the_oracle(nlayers, planned):
    """hbuf_kernel=None and no re-quantisation of h: states and every per-step value equal oracle.model_math.multi_rnn_seq_fwd on
    the same operands to 1e-10, for one and two layers, plain and by slot under a row plan."""
    c = fr.make_case(200, 192, 256, planned, nlayers=nlayers)
    sl = np.arange(c.M) if c.inv is None else c.inv[:c.P]
    x_rows = np.zeros((c.M, c.T, c.Kin))
    x_rows[sl] = c.x.transpose(1, 0, 2)
    state, (cache, _, _, _) = mm.multi_rnn_seq_fwd(x_rows, c.lens_rows, list(zip(c.W, c.bias)))
    kw = dict(row_map=c.inv, rows_per_step=c.rows, n_state_rows=c.M, requantise=None)
    if nlayers == 1:
        reps = [fr.replay_layer(c.x, None, c.W[0], c.bias[0], c.lens, **kw)]
    else:
        reps = fr.replay_level2(c.x, None, None, c.W[0], c.bias[0], c.W[1], c.bias[1], c.lens, **kw)
    H = c.H
    for l, rep in enumerate(reps):
        w = rep["state_written"]
        assert w.sum() == (c.rows[0] if planned else c.M)
        assert np.max(np.abs(rep["c_state"][w] - state[w, 2 * l * H:(2 * l + 1) * H])) < 1e-10
        assert np.max(np.abs(rep["h_state"][w] - state[w, (2 * l + 1) * H:(2 * l + 2) * H])) < 1e-10
        assert np.all(state[~w] == 0)                                   # (rows no launch covers are empty rows)
        for t in range(c.T):
            a = rep["active"][t]
            assert np.array_equal(a, c.lens > t)
            inp, hprev, cprev, (i, j, f, o, tc) = cache[t][l]
            got = rep["gates"][t][a]
            ref = np.stack([i, j, f, o], axis=-1)[sl][a]
            assert np.max(np.abs(got - ref)) < 1e-10
            cn = cprev * f + i * j
            assert np.max(np.abs(rep["c"][t][a] - cn[sl][a])) < 1e-10
            assert np.max(np.abs(rep["h"][t][a] - (tc * o)[sl][a])) < 1e-10
            assert np.all(rep["h"][t][~a] == 0) and np.all(rep["gates_bound"][t][~a] == 0)


# ---------------------------------------------------------------------------- the emulation is inside the bound
CASES = [(M, Kin, H, planned, "bf16") for (M, Kin, H) in fr.SHAPES for planned in (False, True)] + \
        [(M, Kin, H, planned, "f16") for (M, Kin, H) in fr.SHAPES for planned in (False, True)]


@pytest.mark.parametrize("M,Kin,H,planned,fmt", CASES)
def test_f32_emulation_is_inside_the_bound(M, Kin, H, planned, fmt):
    c = fr.make_case(M, Kin, H, planned, fmt=fmt)
    _, rep, res = run(c)
    w = fr.worst_ratio(res)
    for k, (r, at) in w.items():
        print("ratio emulation %s %-9s %s" % (c.name, k, fr.describe(k, r, at, rep=rep)))
    assert all(r <= 1.0 for r, _ in w.values()), w
    # sharp: the bf16 stores are rounding dominated (an f16 store of h is 8x finer: there the accumulation term, which an honest f32
    # sum stays far below, is as large as the rounding)
    assert w["gates"][0] > 0.8 and w["c_all"][0] > 0.8 and w["hbuf"][0] > (0.8 if fmt == "bf16" else 0.5)
    assert w["c_state"][0] < 0.1 and w["h_state"][0] < 0.1


def test_two_layers_of_the_emulation_are_inside_the_bound():
    """replay_level2: layer 1's x_t is the lower layer's own slab t+1."""
    c = fr.make_case(200, 192, 256, True, nlayers=2)
    o0 = emulate_layer(c.x, c.W[0], c.bias[0], c.lens, c.T, row_map=c.inv, rows_per_step=c.rows, n_state_rows=c.M)
    h0 = fr.bf16_to_f64(o0["hbuf"])
    x1 = np.where((np.arange(c.T)[:, None] < c.lens[None, :])[:, :, None], h0[1:], 0.0)
    o1 = emulate_layer(x1, c.W[1], c.bias[1], c.lens, c.T, row_map=c.inv, rows_per_step=c.rows, n_state_rows=c.M, seed=1)
    r0, r1 = fr.replay_level2(c.x, h0, fr.bf16_to_f64(o1["hbuf"]), c.W[0], c.bias[0], c.W[1], c.bias[1], c.lens, row_map=c.inv,
                              rows_per_step=c.rows, n_state_rows=c.M)
    for o, rep in ((o0, r0), (o1, r1)):
        w = fr.worst_ratio(fr.check_layer(rep, o["hbuf"], o["gates"], o["c_all"], o["c_state"], o["h_state"]))
        assert all(r <= 1.0 for r, _ in w.values()), w


def test_saturated_case():
    """|z| reaches 40 - 90: gates of exactly 0 and 1 in bf16, |c| growing by 1 a step in the biased units; everything finite and inside."""
    c = fr.make_case(*fr.SAT_SHAPE, False, saturated=True)
    assert c.T == fr.T_SAT
    o, rep, res = run(c)
    zmax = np.abs(rep["z"][rep["active"]]).max()
    assert 40.0 <= zmax <= 90.0, zmax
    g = rep["gates"][rep["active"]]
    assert np.mean((fr.bf16_round(g) == 0) | (np.abs(fr.bf16_round(g)) == 1)) > 0.3
    full = np.nonzero(c.lens == c.T)[0]
    assert np.allclose(rep["c"][:, full, :8], np.arange(1, c.T + 1)[:, None, None], atol=1e-3)
    for k in ("gates", "gates_bound", "c", "c_bound", "h", "h_bound"):
        assert np.isfinite(rep[k]).all(), k
    w = fr.worst_ratio(res)
    for k, (r, at) in w.items():
        print("ratio emulation %s %-9s %s" % (c.name, k, fr.describe(k, r, at, rep=rep)))
    assert all(r <= 1.0 for r, _ in w.values()), w


# ---------------------------------------------------------------------------- planted faults
@pytest.fixture(scope="module")
def plain():
    c = fr.make_case(330, 64, 128, False)
    return c, run(c)


@pytest.fixture(scope="module")
def planned():
    return fr.make_case(330, 64, 128, True)


def bad(res, k):
    return res[k] > 1.0


def only(res, *outputs):
    """The outputs that leave the bound are exactly these."""
    w = fr.worst_ratio(res)
    assert {k for k, (r, _) in w.items() if r > 1.0} == set(outputs), w


def test_fault_forget_bias_omitted(plain):
    """f is wrong wherever a row is live; c only from t = 1 on (c_{-1} = 0: f multiplies nothing at t = 0); h follows c."""
    c, _ = plain
    _, rep, res = run(c, fault="no_forget_bias")
    g = res["gates"]
    assert not bad(res, "gates")[..., [0, 1, 3]].any()
    assert np.mean(g[..., 2][rep["active"]] > 1.0) > 0.95
    assert not bad(res, "c_all")[:2].any() and bad(res, "c_all")[2:].any()
    assert not bad(res, "hbuf")[:2].any() and bad(res, "hbuf")[2:].any()
    assert bad(res, "c_state")[c.lens >= 2].any() and not bad(res, "c_state")[c.lens <= 1].any()


def test_fault_gate_order_j_f(plain):
    c, _ = plain
    _, rep, res = run(c, fault="swap_jf")
    g = res["gates"]
    assert not bad(res, "gates")[..., [0, 3]].any()
    assert np.mean(g[..., 1][rep["active"]] > 1.0) > 0.95 and np.mean(g[..., 2][rep["active"]] > 1.0) > 0.95
    assert bad(res, "c_all")[1].any()                                   # j is wrong: c is, from the first step on


def test_fault_sigmoid_on_j(plain):
    c, _ = plain
    _, rep, res = run(c, fault="sigmoid_j")
    assert not bad(res, "gates")[..., [0, 2, 3]].any()
    assert np.mean(res["gates"][..., 1][rep["active"]] > 1.0) > 0.95
    assert np.mean(res["c_all"][1][rep["active"][0]] > 1.0) > 0.95


def test_fault_c_state_read_at_step_0(plain):
    """Garbage (3.0) in c_state taken as c_{-1}: every gate is still right (each step is replayed from the kernel's own h), c is
    wrong from slab 1 on, on every live row."""
    c, _ = plain
    _, rep, res = run(c, fault="c_state_at_0")
    only(res, "c_all", "hbuf", "c_state", "h_state")
    assert np.mean(res["c_all"][1][rep["active"][0]] > 1.0) > 0.95
    assert np.all(bad(res, "c_state").any(axis=1) == (c.lens >= 1))


def test_fault_dropped_k_chunk_of_wh(plain):
    """K chunk 2 + 1 of the h-part (h units 32..63) dropped for output units 32..63: nothing at t = 0, where the recurrent product does
    not exist; afterwards the gates of exactly those units, on live rows."""
    c, _ = plain
    _, rep, res = run(c, fault="drop_chunk", arg=(c.Kin // 32 + 1, slice(32, 64)))
    b = bad(res, "gates")
    assert not b[0].any() and not b[:, :, :32].any() and not b[:, :, 64:].any()
    for t in range(1, c.T):
        assert b[t][rep["active"][t]][:, 32:64].any() and not b[t][~rep["active"][t]].any()
    assert not bad(res, "c_all")[:2].any() and bad(res, "c_all")[2:, :, 32:64].any() and not bad(res, "c_all")[:, :, 64:].any()


def test_fault_h_state_one_step_late(plain):
    """h_state taken at t == len: wrong exactly on the rows with 1 <= len < T (a full-length row has no step T; an empty row is
    written by the zero branch)."""
    c, _ = plain
    _, rep, res = run(c, fault="h_state_late")
    only(res, "h_state")
    rows_bad = bad(res, "h_state").any(axis=1)
    assert np.array_equal(rows_bad, (c.lens >= 1) & (c.lens < c.T))


def test_fault_row_advanced_past_its_length(plain):
    c, _ = plain
    m = int(np.nonzero(c.lens == 2)[0][0])
    _, rep, res = run(c, fault="advance_row", arg=m)
    only(res, "hbuf", "c_state", "h_state")
    b = bad(res, "hbuf")
    assert b[3, m].all() and b.sum() == c.H and np.isinf(res["hbuf"][3, m]).all()       # slab len + 1 of that row is not zero
    assert np.array_equal(np.nonzero(bad(res, "c_state").any(axis=1))[0], [m])
    assert np.array_equal(np.nonzero(bad(res, "h_state").any(axis=1))[0], [m])


def test_fault_c_all_one_slab_early(plain):
    c, _ = plain
    _, rep, res = run(c, fault="c_all_slab")
    only(res, "c_all")
    assert np.isinf(res["c_all"][0][rep["active"][0]]).all()            # slab 0 was written
    assert np.isinf(res["c_all"][c.T][rep["active"][c.T - 1]]).all()    # slab T was not


def test_fault_i_j_swapped_in_the_record(plain):
    c, _ = plain
    _, rep, res = run(c, fault="swap_ij_record")
    only(res, "gates")
    assert not bad(res, "gates")[..., [2, 3]].any()
    assert np.mean(res["gates"][..., 0][rep["active"]] > 1.0) > 0.9 and np.mean(res["gates"][..., 1][rep["active"]] > 1.0) > 0.9


def test_fault_h_truncated_to_bf16(plain):
    """Truncation is off by up to a whole bf16 ulp where round-to-nearest is allowed 2^-8 |h|, between half an ulp and a whole one
    depending on where h sits in its binade: less than half of the elements leave the bound, none by more than a factor 2."""
    c, _ = plain
    _, rep, res = run(c, fault="truncate_h")
    only(res, "hbuf")
    live = res["hbuf"][1:][rep["active"]]
    assert 0.1 < np.mean(live > 1.0) < 0.5 and live.max() < 2.1


def test_fault_row_map_ignored_for_the_state(planned):
    c = planned
    _, rep, res = run(c)
    assert all(r <= 1.0 for r, _ in fr.worst_ratio(res).values())
    _, rep, res = run(c, fault="ignore_row_map")
    only(res, "c_state", "h_state")
    n0 = c.rows[0]
    moved = np.zeros(c.M, bool)
    moved[c.inv[:n0][c.inv[:n0] != np.arange(n0)]] = True               # rows whose slot is not their own number
    moved[np.arange(n0)[c.inv[:n0] != np.arange(n0)]] = True            # and the rows written in their place
    assert moved.sum() > c.M // 2
    rows_bad = bad(res, "c_state").any(axis=1)
    assert not rows_bad[~moved].any() and np.mean(rows_bad[moved]) > 0.95


def test_fault_bias_clamp_off_by_a_lane(plain):
    """The last 4 units take the bias of the 4 before them: their gates only, on every live row at every step."""
    c, _ = plain
    H = c.H
    d = np.abs(c.bias[0].reshape(4, H)[:, H - 4:] - c.bias[0].reshape(4, H)[:, H - 8:H - 4])
    assert d.min() > 1e-3                                               # the two bias groups differ in every gate and unit
    _, rep, res = run(c, fault="bias_clamp")
    b = bad(res, "gates")
    assert not b[:, :, :H - 4].any()
    for t in range(c.T):
        assert np.mean(b[t][rep["active"][t]][:, H - 4:].any(axis=(1, 2))) > 0.95
    assert not bad(res, "c_all")[:, :, :H - 4].any() and bad(res, "c_all")[1:, :, H - 4:].any()
