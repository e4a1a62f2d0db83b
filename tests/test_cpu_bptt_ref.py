"""tests/_bptt_ref.py without a GPU: the float64 tape replay is the oracle's BPTT, an honest f32 emulation of the step kernels
stays inside the derived bound on every shape the GPU test uses, and planted faults leave it - at the right place."""
import numpy as np
import pytest

import _bptt_ref as br
from oracle import model_math as mm

T = br.T_STEPS
F32 = np.float32


# ---------------------------------------------------------------------------- problems
class Problem:
    pass


def build(kind, M, Kin, H, nlayers=1, planned=False, rounded=True, lens=None):
    """Oracle forward of `nlayers` stacked layers -> per-layer tapes (bf16-rounded like the kernels' tape, or exact float64), in slot
    order under a row plan."""
    rng = np.random.default_rng(1000 + len(kind) + M + H if isinstance(kind, str) else kind)
    p = Problem()
    p.M, p.Kin, p.H, p.planned = M, Kin, H, planned
    if lens is None:
        lens = br.case_lens(kind, M, H, planned) if isinstance(kind, str) else br.make_lens(kind, M, T, 0.15 if planned else 0.0)
    p.lens_rows = np.asarray(lens, np.int32)
    rd = br.bf16_round if rounded else (lambda a: np.asarray(a, np.float64))
    p.x = rd(rng.standard_normal((M, T, Kin)) * 0.5)
    p.layers = []
    for l in range(nlayers):
        nin = Kin if l == 0 else H
        p.layers.append((rd(mm.glorot_uniform(rng, (nin + H, 4 * H)) * 2.0), (rng.standard_normal(4 * H) * 0.1).astype(F32).astype(np.float64)))
    _, p.cache = mm.multi_rnn_seq_fwd(p.x, p.lens_rows, p.layers)
    steps = p.cache[0]
    if planned:
        p.inv, p.P, p.rows = br.host_plan(p.lens_rows, T)
        sl = p.inv[:p.P]
    else:
        p.inv, p.P, p.rows, sl = None, M, None, np.arange(M)
    p.slots = sl
    p.lens = p.lens_rows[sl]
    act = (np.arange(T)[:, None] < p.lens[None, :])[:, :, None]
    p.tapes, p.inputs = [], []
    for l in range(nlayers):
        i, j, f, o = (np.stack([steps[t][l][3][k][sl] for t in range(T)]) for k in range(4))
        c = np.stack([steps[t][l][2][sl] for t in range(T)] + [np.zeros((p.P, H))])
        cn = steps[T - 1][l][2][sl] * f[T - 1] + i[T - 1] * j[T - 1]
        c[T] = cn
        for t in range(T - 1):          # slab t+1 = the state after step t (for an active row that is c_prev of step t+1)
            c[t + 1] = np.where(act[t], c[t + 1], np.nan)
        c[T] = np.where(act[T - 1], c[T], np.nan)
        c[0] = np.nan                    # never read
        if rounded:
            i, j, f, o = (np.where(act, a, np.nan) for a in (i, j, f, o))
            tape = br.decode_tape(br.pack_gates(i, j, f, o), br.bf16_bits(c))
        else:
            tape = (i, j, f, o, c)
        p.tapes.append(tape)
        p.inputs.append(np.stack([np.concatenate([steps[t][l][0], steps[t][l][1]], axis=1)[sl] for t in range(T)]))
    p.W_il = [br.bf16_round(br.interleave_w(k, H)) if rounded else br.interleave_w(k, H) for k, _ in p.layers]
    p.dS = rng.standard_normal((M, 2 * H * nlayers)).astype(F32).astype(np.float64)
    p.dh_above = rd(rng.standard_normal((T, p.P, H)) * 0.3)
    return p


# ---------------------------------------------------------------------------- f32 emulation of a layer's BPTT steps
def tanhf_(x):
    ax = np.abs(x).astype(F32)
    e = np.exp(F32(-2.0) * ax).astype(F32)
    t = ((F32(1.0) - e) / (F32(1.0) + e)).astype(F32)
    return np.copysign(t, x).astype(F32)


def matmul_chunks(rng, A, B, drop=None):
    """A [M][K] . B [N][K]^T in f32, K summed in shuffled 32-wide chunks.  drop = (chunk, slice of N): that chunk is left out there."""
    acc = np.zeros((A.shape[0], B.shape[0]), F32)
    for k in rng.permutation(A.shape[1] // 32):
        part = (A[:, k * 32:(k + 1) * 32].astype(F32) @ B[:, k * 32:(k + 1) * 32].astype(F32).T).astype(F32)
        if drop is not None and k == drop[0]:
            part[:, drop[1]] = 0
        acc = (acc + part).astype(F32)
    return acc


def emulate_layer(tape, lens, W_il, dS_c, dS_h, dh_above=None, dz_above=None, w_above=None, row_map=None, dc_bf16=False, seed=0,
                  fault=None, fault_arg=None):
    """What a correct kernel computes, in numpy f32 - or, with `fault`, a kernel that is wrong in one named way.  Returns dz
    [T][M][4H] (bf16 values as float64, NaN-prefilled like the GPU test's buffer) and db [4H] f32."""
    rng = np.random.default_rng(seed)
    i_, j_, f_, o_, c_ = (a.astype(F32) for a in tape)
    if fault == "swap_fo":
        f_, o_ = o_, f_
    Tn, M, H = i_.shape
    Kin = W_il.shape[0] - H
    Wh = W_il[Kin:]
    fused = dz_above is not None
    rows = np.arange(M) if (row_map is None or fault == "ignore_row_map") else np.asarray(row_map)[:M]
    dSc, dSh = np.asarray(dS_c)[rows].astype(F32), np.asarray(dS_h)[rows].astype(F32)
    lens = np.asarray(lens)
    dz = np.full((Tn, M, 4 * H), np.nan)
    dc = np.zeros((M, H), F32)
    db = np.zeros((H, 4), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(Tn - 1, -1, -1):
            act = (t < lens)[:, None]
            last = (t == lens - 1)[:, None]
            acc = np.zeros((M, H), F32)
            if t + 1 < Tn:
                drop = fault_arg if (fault == "drop_chunk" and t == fault_arg[2]) else None
                acc = matmul_chunks(rng, dz[t + 1], Wh, drop)
            if fused:
                acc = (acc + matmul_chunks(rng, np.asarray(dz_above[t]).reshape(M, 4 * H), np.asarray(w_above)[:H])).astype(F32)
            add = fused != (fault in ("fused_replace", "plain_add"))
            dh = np.where(last, (acc + dSh) if add else dSh, acc).astype(F32)
            if dh_above is not None:
                dh = (dh + dh_above[t].astype(F32)).astype(F32)
            tc = tanhf_(c_[t + 1])
            omt = (F32(1.0) - tc * tc).astype(F32) if fault != "no_omt" else F32(1.0)
            cp = c_[t] if (t > 0 or fault == "c_old_at_0") else np.zeros((M, H), F32)
            i, j, f, o = i_[t], j_[t], f_[t], o_[t]
            dcn = (np.where(last, dSc, dc) + dh * o * omt).astype(F32)
            z = np.stack([dcn * j * i * (F32(1.0) - i), dcn * i * (F32(1.0) - j * j), dcn * cp * f * (F32(1.0) - f),
                          dh * tc * o * (F32(1.0) - o)], axis=-1).astype(F32)
            if fault == "scale_gate" and t == fault_arg[0]:
                u0, g = fault_arg[1], fault_arg[2]
                z[:, u0:u0 + 4, g] *= F32(1.01)
            z = np.where(act[..., None], z, F32(0.0))
            db = (db + z.sum(axis=0, dtype=F32)).astype(F32)
            car = (dcn * f).astype(F32)
            if dc_bf16:
                car = br.bf16_round(car).astype(F32)
            dc = np.where(act, car, dc)
            out = br.bf16_round(z).reshape(M, 4 * H)
            if fault == "zero_row" and t == fault_arg[0]:
                out[fault_arg[1]] = 0.0
            if fault == "inactive_nonzero" and t == fault_arg[0]:
                out[fault_arg[1], fault_arg[2] * 4 + fault_arg[3]] = 2.0 ** -20
            dz[t] = out
    return dz, db.T.reshape(4 * H).astype(np.float64)


def run_plain(p, dh_above=True, **kw):
    H = p.H
    da = p.dh_above if dh_above else None
    dz, db = emulate_layer(p.tapes[0], p.lens, p.W_il[0], p.dS[:, :H], p.dS[:, H:2 * H], dh_above=da, row_map=p.inv, **kw)
    rep = br.replay_layer(p.tapes[0], p.lens, p.W_il[0], p.dS[:, :H], p.dS[:, H:2 * H], dh_above=da, dz_kernel=dz, row_map=p.inv,
                          rows_per_step=p.rows, dc_bf16=kw.get("dc_bf16", False))
    return dz, db, rep


def run_stack(p, fault0=None, fault_arg0=None, dc_bf16=False):
    """Layer 1 plain, then layer 0 fused with the emulated dz1 - what both the layer-after-layer calls and the pair launches compute."""
    H = p.H
    dz1, db1 = emulate_layer(p.tapes[1], p.lens, p.W_il[1], p.dS[:, 2 * H:3 * H], p.dS[:, 3 * H:], row_map=p.inv, dc_bf16=dc_bf16, seed=1)
    dz0, db0 = emulate_layer(p.tapes[0], p.lens, p.W_il[0], p.dS[:, :H], p.dS[:, H:2 * H], dz_above=dz1, w_above=p.W_il[1], row_map=p.inv,
                             dc_bf16=dc_bf16, seed=2, fault=fault0, fault_arg=fault_arg0)
    r0, r1 = br.replay_stack2(p.tapes[0], p.tapes[1], p.lens, p.W_il[0], p.W_il[1], p.dS, dz0, dz1, row_map=p.inv, rows_per_step=p.rows,
                              dc_bf16=dc_bf16)
    return (dz0, db0, r0), (dz1, db1, r1)


def ratio_of(dz, rep):
    return br.worst_ratio(dz, rep["dz"], rep["bound"], rep["active"])


def check_honest(name, dz, db, rep):
    r, at = ratio_of(dz, rep)
    rd, k = br.db_ratio(db, rep)
    print("emulation %-44s dz %s; db %.4f at %d" % (name, br.describe(r, at), rd, k))
    assert r <= 1.0, (name, br.describe(r, at))
    assert rd <= 1.0, (name, rd, k)
    return r


# ---------------------------------------------------------------------------- helpers of the module itself
def test_bf16_helpers_round_to_nearest_even_and_decode_the_record_layout():
    import torch
    rng = np.random.default_rng(0)
    a = np.concatenate([rng.standard_normal(4096) * 10.0 ** rng.integers(-6, 6, 4096), [0.0, -0.0, 1.0, 1.00390625, 1.01171875, np.inf, -np.inf]]).astype(F32)
    want = torch.from_numpy(a).bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(br.bf16_bits(a), want)                       # ties to even: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    assert np.isnan(br.bf16_to_f64(br.bf16_bits(np.array([np.nan], F32))))[0]
    rec = np.array([[0x3F004000, 0x3E803F80]], np.uint32).view(np.int32)   # i = 2.0 (0x4000) | j = 0.5 (0x3F00); f = 1.0 | o = 0.25
    i, j, f, o, c = br.decode_tape(rec.reshape(1, 1, 1, 2), np.array([0x4120, 0xC120], np.uint16).reshape(2, 1, 1))
    assert (i.item(), j.item(), f.item(), o.item()) == (2.0, 0.5, 1.0, 0.25) and c.ravel().tolist() == [10.0, -10.0]
    g = br.pack_gates(i, j, f, o)
    assert np.array_equal(g.view(np.uint32).ravel(), rec.view(np.uint32).ravel())


def test_case_lengths_and_plans_have_the_required_structure():
    for (M, Kin, H, planned, _, _) in br.LAYER_CASES:
        p = build("layer", M, Kin, H, planned=planned)
        act = br.check_lens(p.lens_rows, T)
        assert act.mean() >= 0.4
        if planned:
            br.check_plan(p.P, p.rows)
            assert np.all(np.diff(p.lens.astype(int)) <= 0) and p.rows == [int((p.lens > t).sum()) for t in range(T)]


# ---------------------------------------------------------------------------- 1. the replay is the right mathematics
def _tf(dz):     # replay dz [M][H][4] -> TF gate order [M][4H] (column g*H+u)
    return dz.transpose(0, 2, 1).reshape(dz.shape[0], -1)


def _rel(a, b):
    return np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-300)


@pytest.mark.parametrize("planned", [False, True])
def test_replay_of_an_exact_tape_is_the_oracle_bptt_one_layer(planned):
    from test_gpu_kernels import _bwd_ref
    M, Kin, H = 37, 24, 16
    p = build(3, M, Kin, H, planned=planned, rounded=False)
    assert {0, 1, T} <= set(p.lens_rows.tolist())
    dh_rows = np.zeros((T, M, H))
    dh_rows[:, p.slots] = p.dh_above
    dx_ref, [(dK_ref, db_ref)] = _bwd_ref(p.x, p.lens_rows, p.layers[0][0], p.layers[0][1], p.dS, dh_rows)
    rep = br.replay_layer(p.tapes[0], p.lens, p.W_il[0], p.dS[:, :H], p.dS[:, H:], dh_above=p.dh_above, row_map=p.inv, rows_per_step=p.rows)
    kernel = p.layers[0][0]
    dK, dx = np.zeros_like(kernel), np.zeros((M, T, Kin))
    for t in range(T):
        dz = _tf(rep["dz"][t])
        dK += p.inputs[0][t].T @ dz
        dx[p.slots, t] = (dz @ kernel.T)[:, :Kin]
    assert _rel(dK, dK_ref) < 1e-10 and _rel(dx, dx_ref) < 1e-10 and _rel(rep["db"], db_ref) < 1e-10
    assert not rep["dz"][~rep["active"]].any()


@pytest.mark.parametrize("planned", [False, True])
def test_replay_of_an_exact_tape_is_the_oracle_bptt_two_layers_through_wx1(planned):
    M, Kin, H = 37, 24, 16
    p = build(4, M, Kin, H, nlayers=2, planned=planned, rounded=False)
    dx_ref, grads_ref = mm.multi_rnn_seq_bwd(p.dS, p.cache, p.layers)
    r0, r1 = br.replay_stack2(p.tapes[0], p.tapes[1], p.lens, p.W_il[0], p.W_il[1], p.dS, None, None, row_map=p.inv, rows_per_step=p.rows)
    dx = np.zeros((M, T, Kin))
    for l, rep in enumerate((r0, r1)):
        kernel = p.layers[l][0]
        dK = np.zeros_like(kernel)
        for t in range(T):
            dz = _tf(rep["dz"][t])
            dK += p.inputs[l][t].T @ dz
            if l == 0:
                dx[p.slots, t] = (dz @ kernel.T)[:, :Kin]
        assert _rel(dK, grads_ref[l][0]) < 1e-10 and _rel(rep["db"], grads_ref[l][1]) < 1e-10, l
    assert _rel(dx, dx_ref) < 1e-10


# ---------------------------------------------------------------------------- 2. an honest f32 emulation passes, on every GPU shape
@pytest.mark.parametrize("M,Kin,H,planned,above,want_db", br.LAYER_CASES)
def test_f32_emulation_of_the_plain_layer_stays_inside_the_bound(M, Kin, H, planned, above, want_db):
    p = build("layer", M, Kin, H, planned=planned)
    check_honest("layer M=%d Kin=%d H=%d plan=%d" % (M, Kin, H, planned), *run_plain(p, dh_above=above))


@pytest.mark.parametrize("M,H,planned", br.FUSED_CASES)
def test_f32_emulation_of_the_fused_layer_stays_inside_the_bound(M, H, planned):
    p = build("fused", M, br.FUSED_KIN, H, nlayers=2, planned=planned)
    l0, l1 = run_stack(p)
    check_honest("fused M=%d H=%d plan=%d upper" % (M, H, planned), *l1)
    check_honest("fused M=%d H=%d plan=%d lower" % (M, H, planned), *l0)


@pytest.mark.parametrize("M,H,planned", br.STACK2_CASES)
def test_f32_emulation_of_the_two_layer_stack_stays_inside_the_bound(M, H, planned):
    p = build("stack2", M, br.STACK2_KIN, H, nlayers=2, planned=planned)
    br.check_lens(p.lens_rows, T)
    l0, l1 = run_stack(p)
    check_honest("stack2 M=%d H=%d plan=%d layer 1" % (M, H, planned), *l1)
    check_honest("stack2 M=%d H=%d plan=%d layer 0" % (M, H, planned), *l0)


def _saturated(nlayers):
    rng = np.random.default_rng(77)
    M, H = br.SAT_M, br.SAT_H
    p = Problem()
    p.M = p.P = M
    p.H, p.inv, p.rows = H, None, None
    p.lens = br.case_lens("sat", M, H, False)
    p.tapes = [br.decode_tape(*br.synthetic_saturated_tape(70 + l, M, T, H, p.lens)) for l in range(nlayers)]
    p.W_il = [br.bf16_round(br.interleave_w(mm.glorot_uniform(rng, (H + H, 4 * H)) * 2.0, H)) for _ in range(nlayers)]
    p.dS = rng.standard_normal((M, 2 * H * nlayers)).astype(F32).astype(np.float64)
    p.dh_above = br.bf16_round(rng.standard_normal((T, M, H)) * 0.3)
    return p


def test_f32_emulation_on_the_saturated_tape_stays_inside_the_bound():
    p = _saturated(2)
    i, j, f, o, c = p.tapes[0]
    act = p.lens > 0
    assert np.isnan(c[0]).all() and np.nanmax(np.abs(c)) == 20.0
    assert (i[0][act] == 0).any() and (i[0][act] == 1).any() and (np.abs(j[0][act]) == 1).any() and (f[0][act] == 1).any() and (o[0][act] == 0).any()
    dz, db, rep = run_plain(p)
    assert np.isfinite(rep["dz"]).all() and np.isfinite(rep["bound"]).all()
    check_honest("saturated plain", dz, db, rep)
    l0, l1 = run_stack(p)
    check_honest("saturated pair layer 1", *l1)
    check_honest("saturated pair layer 0", *l0)


def test_f32_emulation_with_a_bf16_carry_stays_inside_the_widened_bound():
    M, Kin, H = br.LAYER_CASES[0][:3]
    p = build("layer", M, Kin, H)
    check_honest("dc_bf16 layer M=%d H=%d" % (M, H), *run_plain(p, dc_bf16=True))
    p = build("stack2", 520, br.STACK2_KIN, 128, nlayers=2)
    l0, l1 = run_stack(p, dc_bf16=True)
    check_honest("dc_bf16 stack2 M=520 H=128 layer 1", *l1)
    check_honest("dc_bf16 stack2 M=520 H=128 layer 0", *l0)
    # the widening is needed: the same bf16-carry output against the plain-carry bound does leave it
    dz, db, _ = run_plain(build("layer", M, Kin, H), dc_bf16=True)
    q = build("layer", M, Kin, H)
    rep = br.replay_layer(q.tapes[0], q.lens, q.W_il[0], q.dS[:, :H], q.dS[:, H:2 * H], dh_above=q.dh_above, dz_kernel=dz)
    assert ratio_of(dz, rep)[0] > 1.0


def test_bf16_unit_roundoff_is_two_to_the_minus_eight():
    """The mirror case: with rb = 2^-9 the honest emulation fails, so the bound is essentially the final bf16 rounding."""
    M, Kin, H = 70, 64, 128
    p = build(5, M, Kin, H)
    dz, db, rep = run_plain(p)
    r, _ = ratio_of(dz, rep)
    assert 0.5 < r <= 1.0, r
    old = br.RB
    try:
        br.RB = 2.0 ** -9
        assert ratio_of(dz, rep)[0] > 1.0
    finally:
        br.RB = old


# ---------------------------------------------------------------------------- 3. planted faults are caught, at their place
def _lens_of(p, at):
    return int(p.lens[at[1]])


def test_fault_dropped_k_chunk():
    p = build(41, 200, 64, 256)
    dz, _, rep = run_plain(p, fault="drop_chunk", fault_arg=(7, slice(128, 256), 1))     # chunk 7 of 32, units 128.., at step 1
    r, at = ratio_of(dz, rep)
    print("fault dropped K chunk:", br.describe(r, at))
    assert r > 1.0 and at[0] == 1 and at[2] >= 128 and _lens_of(p, at) > 2       # a row whose product is used (not its last step)
    # the steps before it in time order of the walk (t = 3, 2) are clean: the failure names its step.  (Step 0 is not: it
    # inherits the wrong dc, the one thing a step takes over that the replay cannot read back from the kernel's output.)
    assert br.worst_ratio(dz[2:], rep["dz"][2:], rep["bound"][2:], rep["active"][2:])[0] <= 1.0


def test_fault_missing_tanh_derivative():
    p = build(42, 70, 64, 128)
    dz, _, rep = run_plain(p, fault="no_omt")
    r, at = ratio_of(dz, rep)
    print("fault missing (1 - tc^2):", br.describe(r, at))
    assert r > 1.0 and at[3] != 3                                        # dz_o does not hold the factor


def test_fault_f_and_o_swapped_in_the_record_decode():
    p = build(43, 70, 64, 128)
    dz, _, rep = run_plain(p, fault="swap_fo")
    r, at = ratio_of(dz, rep)
    print("fault f/o swapped:", br.describe(r, at))
    assert r > 1.0 and rep["active"][at[0], at[1]]
    # and the replay's own decode is what a forward writes: i low / j high in .x, f low / o high in .y
    i, j, f, o, _ = p.tapes[0]
    g = br.pack_gates(*(np.nan_to_num(a) for a in (i, j, f, o))).view(np.uint32)
    assert np.array_equal(br.bf16_to_f64((g[..., 1] >> 16).astype(np.uint16)), np.nan_to_num(o))


def test_fault_one_percent_on_one_gate_of_one_unit_group():
    p = build(44, 200, 64, 256)
    dz, _, rep = run_plain(p, fault="scale_gate", fault_arg=(2, 132, 1))  # step 2, units 132..135, gate j
    r, at = ratio_of(dz, rep)
    print("fault 1 % on one gate of 4 units:", br.describe(r, at))
    assert r > 1.0 and at[0] == 2 and 132 <= at[2] < 136 and at[3] == 1


@pytest.mark.parametrize("planned", [False, True])
def test_fault_final_state_gradient_replaces_where_the_fused_form_adds(planned):
    p = build(45, 200, 64, 128, nlayers=2, planned=planned)
    (dz0, _, r0), _ = run_stack(p, fault0="fused_replace")
    r, at = ratio_of(dz0, r0)
    print("fault replace-for-add (fused):", br.describe(r, at))
    assert r > 1.0 and _lens_of(p, at) - 1 == at[0]                      # at a row's last step


def test_adding_in_the_plain_form_is_the_same_computation():
    """The reverse mix-up - ADD the final-state gradient in the plain form - is not a fault the output can show: at a row's
    last step dz_{t+1} of that row is zero (and at t == T-1 the product is empty), so the product it would add is exactly 0.
    The emulation with the mix-up is bit-identical; what the check does catch is the consequence once that premise breaks, a
    nonzero dz left in an inactive row (test_fault_nonzero_left_in_an_inactive_row)."""
    p = build(46, 70, 64, 128)
    a, _, _ = run_plain(p)
    b, _, rep = run_plain(p, fault="plain_add")
    assert np.array_equal(a, b) and ratio_of(b, rep)[0] <= 1.0


def test_fault_row_map_ignored():
    p = build(47, 200, 64, 128, planned=True)
    dz, _, rep = run_plain(p, fault="ignore_row_map")
    r, at = ratio_of(dz, rep)
    print("fault row_map ignored:", br.describe(r, at))
    assert r > 1.0 and p.inv[at[1]] != at[1]
    dz, _, rep = run_plain(p)
    assert ratio_of(dz, rep)[0] <= 1.0


def test_fault_last_ragged_row_of_a_row_tile_zeroed():
    lens = br.make_lens(48, 200, T)
    lens[199] = T
    p = build(48, 200, 64, 128, lens=lens)
    dz, _, rep = run_plain(p, fault="zero_row", fault_arg=(1, 199))
    r, at = ratio_of(dz, rep)
    print("fault last row zeroed:", br.describe(r, at))
    assert r > 1.0 and at[:2] == (1, 199)


def test_fault_nonzero_left_in_an_inactive_row():
    p = build(49, 70, 64, 128)
    row = int(np.nonzero(p.lens == 2)[0][0])
    dz, _, rep = run_plain(p, fault="inactive_nonzero", fault_arg=(2, row, 33, 2))
    r, at = ratio_of(dz, rep)
    print("fault nonzero in an inactive row:", br.describe(r, at))
    assert r == np.inf and at == (2, row, 33, 2)
    dz, _, rep = run_plain(p)
    dz[3, int(np.nonzero(p.lens == 0)[0][0]), 5] = np.nan               # an unwritten (NaN-prefilled) element is caught the same way
    assert ratio_of(dz, rep)[0] == np.inf


def test_fault_c_old_read_at_the_first_step():
    p = _saturated(1)                                                    # slab 0 of c_all is NaN there
    dz, _, rep = run_plain(p, fault="c_old_at_0")
    r, at = ratio_of(dz, rep)
    assert r == np.inf and at[0] == 0 and at[3] == 2                     # dz_f of step 0
    p = build(50, 70, 64, 128)
    p.tapes[0][4][0] = 0.75                                              # a finite stale value in slab 0
    dz, _, rep = run_plain(p, fault="c_old_at_0")
    r, at = ratio_of(dz, rep)
    print("fault c_old read at t == 0:", br.describe(r, at))
    assert r > 1.0 and at[0] == 0 and at[3] == 2
