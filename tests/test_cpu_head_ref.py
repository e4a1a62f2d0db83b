"""tests/_head_ref.py checked on the CPU, no GPU needed: every reference against the oracle's function to 1e-12; an f32 numpy emulation
of every kernel (f32 arithmetic, exp / log evaluated in float64 and rounded to f32, numpy's summation order) inside every bound on every
case the GPU test runs, worst ratio printed - so the reference alone fits and no bound is vacuous; and 20 planted faults, each of which
must leave the bound at the element it predicts.  pytest -s shows the ratio lines."""
import numpy as np
import pytest
import torch

import _head_ref as hr
from _head_ref import F32, F64, U, bf16_bits, bf16_round, bf16_to_f64
from oracle import model_math as mm

TOL = dict(rtol=1e-12, atol=1e-12)
NAN = np.nan


def _line(entry, case, output, q):
    r, at = hr.worst(q)
    print("ratio emu %s %s %s %.4f at %s" % (entry, case, output, r, at))
    return r


def _inside(entry, case, **qs):
    bad = {k: hr.worst(q) for k, q in qs.items() if _line(entry, case, k, q) > 1.0}
    assert not bad, (entry, case, bad)


def _exp32(x):
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(np.asarray(x, F32).astype(F64)).astype(F32)


def _sig32(z):
    with np.errstate(over="ignore"):
        return (F32(1.0) / (F32(1.0) + _exp32(-np.asarray(z, F32)))).astype(F32)


# ---------------------------------------------------------------------------- MoE tail
def emu_moe(c, dp=None, fault=None, pad=8):
    """-> pred [B][V], rowsum [B], dgate [B][ld] and dexpert [B][ld] as float64 of the bf16 stored, NaN where nothing was written."""
    B, V, M = c.B, c.V, c.M
    ga, ea = c.ga, c.ea
    t = ga - ga.max(axis=2, keepdims=True)
    x = _exp32(t)
    den = (x[..., :M] if fault == "den without last gate" else x).sum(axis=2, keepdims=True, dtype=F32)
    g = x * (F32(1.0) / den)
    e = _sig32(ea)
    pred = (g[..., :M] * e).sum(axis=2, dtype=F32)
    if fault == "pred over m <= M":
        pred = pred + g[..., M] * e[..., M - 1]
    rowsum = (pred[:, :V - 1] if fault == "rowsum drops last class" else pred).sum(axis=1, dtype=F32)
    if dp is None:
        return pred, rowsum, None, None
    dp = np.asarray(dp, F32)[..., None]
    sdot = ((dp * e) if fault == "sdot without g" else (dp * e * g[..., :M])).sum(axis=2, keepdims=True, dtype=F32)
    dgm = np.zeros_like(g)
    dgm[..., :M] = dp * e
    dga = g * (dgm - sdot)
    if fault == "dgate component M zero":
        dga[..., M] = 0
    dea = dp * g[..., :M] * e if fault == "dexpert without (1 - e)" else dp * g[..., :M] * e * (F32(1.0) - e)
    ldg, lde = V * (M + 1) + pad, V * M + pad
    dg = np.full((B, ldg), NAN)
    de = np.full((B, lde), NAN)
    if fault == "dgate at dense stride":
        dg.reshape(-1)[:B * V * (M + 1)] = bf16_round(dga.reshape(-1))
    else:
        dg[:, :V * (M + 1)] = bf16_round(dga.reshape(B, -1))
    de[:, :V * M] = bf16_round(dea.reshape(B, -1))
    return pred, rowsum, dg, de


def check_moe(c, ref, pred, rowsum, dg, de):
    B, V, M = c.B, c.V, c.M
    qs = dict(pred=hr.ratio(pred, ref["pred"], ref["d_pred"]), rowsum=hr.ratio(rowsum, ref["rowsum"], ref["d_rowsum"]))
    if dg is not None:
        n = V * (M + 1)
        qs["dgate"] = hr.ratio(dg[:, :n].reshape(B, V, M + 1), ref["dga"], ref["d_dga"], hr.RB)
        qs["dgate_pad"] = np.where(np.isnan(dg[:, n:]), 0.0, np.inf)
        qs["dexpert"] = hr.ratio(de[:, :V * M].reshape(B, V, M), ref["dea"], ref["d_dea"], hr.RB)
        qs["dexpert_pad"] = np.where(np.isnan(de[:, V * M:]), 0.0, np.inf)
    return qs


def _moe_dp(c, ref):
    return hr.ce_grad_f32(ref["pred"].astype(F32), c.labels)


@pytest.mark.parametrize("M", hr.MOE_MS)
def test_moe_reference_is_the_oracle_and_the_emulation_is_inside(M):
    for V in hr.MOE_VS:
        c = hr.moe_case(M, V)
        dp = _moe_dp(c, hr.moe_ref(c.ga, c.ea))
        ref = hr.moe_ref(c.ga, c.ea, dp)
        x = np.eye(c.B)
        p, cache = mm.moe_fwd(x, hr.f64(c.ga).reshape(c.B, -1), hr.f64(c.ea).reshape(c.B, -1), np.zeros(V * M), num_mixtures=M)
        _, dWg, dWe, _ = mm.moe_bwd(hr.f64(dp), cache)
        assert np.allclose(ref["pred"], p, **TOL) and np.allclose(ref["rowsum"], p.sum(axis=1), **TOL)
        assert np.allclose(ref["dga"].reshape(c.B, -1), dWg, rtol=1e-12, atol=1e-12 * max(1.0, np.abs(dWg).max()))
        assert np.allclose(ref["dea"].reshape(c.B, -1), dWe, rtol=1e-12, atol=1e-12 * max(1.0, np.abs(dWe).max()))
        _inside("moe_tail", c.name, **check_moe(c, ref, *emu_moe(c, dp)))
        for b, k in c.sat:                                              # e exactly 0 or 1 in f32: dexpert exactly zero
            assert (emu_moe(c, dp)[3][b, k * M:(k + 1) * M] == 0).all()


MOE_FAULTS = ["den without last gate", "pred over m <= M", "dgate component M zero", "sdot without g", "dexpert without (1 - e)",
              "dgate at dense stride", "rowsum drops last class"]


@pytest.mark.parametrize("fault", MOE_FAULTS)
def test_moe_planted_fault_leaves_the_bound_where_predicted(fault):
    c = hr.moe_case(2, 257)
    dp = _moe_dp(c, hr.moe_ref(c.ga, c.ea))
    ref = hr.moe_ref(c.ga, c.ea, dp)
    qs = check_moe(c, ref, *emu_moe(c, dp, fault=fault))
    out = {k: q > 1.0 for k, q in qs.items()}
    plain = (1, 100)                                                    # an unplanted class
    if fault == "den without last gate":
        assert out["pred"][plain] and out["dgate"][plain].all() and out["dexpert"][plain].all()
    elif fault == "pred over m <= M":
        assert out["pred"][plain] and out["rowsum"].all() and not out["dgate"].any() and not out["dexpert"].any()
    elif fault == "dgate component M zero":
        assert out["dgate"][plain][c.M] and not out["dgate"][..., :c.M].any() and not out["dexpert"].any() and not out["pred"].any()
    elif fault == "sdot without g":
        assert out["dgate"][plain].all() and not out["dexpert"].any() and not out["pred"].any()
    elif fault == "dexpert without (1 - e)":
        assert out["dexpert"][plain].all() and not out["dgate"].any() and not out["pred"].any()
    elif fault == "dgate at dense stride":
        assert not out["dgate"][0].any() and out["dgate"][1][100].any() and out["dgate"][2][100].any() and not out["dgate_pad"][c.B - 1].any()
        assert out["dgate_pad"][0].all() and not out["dexpert"].any()     # row 1 starts inside row 0's padding
    else:
        dropped = ref["pred"][:, c.V - 1] / ref["d_rowsum"]             # row 0 only: the last class of rows 1 and 2 is planted to pred ~ 0
        assert dropped[0] > 100 and out["rowsum"][0] and (out["rowsum"] == (dropped > 2.0)).all() and not out["pred"].any()
    print("fault moe_tail '%s': %s" % (fault, {k: "%.3g" % hr.worst(q)[0] for k, q in qs.items()}))


# ---------------------------------------------------------------------------- losses
def emu_ce(c, acc=False, want_grad=True, fault=None, gs=hr.GS, loss0=hr.LOSS0):
    p, n = c.p, c.n
    eps = F32(1e-6) if fault == "eps 1e-6" else F32(10e-6)
    pos = (c.y == 1) if fault == "label 255 negative" else (c.y != 0)
    a = p + eps
    bq = F32(1.0) - p + eps
    arg = np.where(pos, a, bq).astype(F32)
    t = (-np.log(arg.astype(F64))).astype(F32)
    live = np.ones(n, bool)
    if fault == "tail skipped":
        live[n - n % 4:] = False
    loss = F32(loss0) + t[live].sum(dtype=F32) * (F32(1.0) / F32(c.B))
    if not want_grad:
        return loss, None
    g = np.where(pos, F32(-1.0) / a, F32(1.0) / bq).astype(F32)
    if fault != "grad_scale missing":
        g = g * F32(gs)
    out = c.dp0 + g if (acc and fault != "accumulate overwrites") else g
    out = np.where(live, out, c.dp0 if acc else F32(NAN))
    return loss, out.astype(F32)


def _ce_cases():
    for B, V in hr.CE_SHAPES:
        yield hr.ce_case(B, V)
    for B, V in hr.CE_SPARSE_SHAPES:
        yield hr.ce_case(B, V, sparse=True)


def test_ce_reference_is_the_oracle_and_the_emulation_is_inside():
    for c in _ce_cases():
        r1 = hr.ce_ref(c.p, c.y, c.B, gs=1.0, loss0=0.0)
        p64, y = hr.f64(c.p).reshape(c.B, c.V), (c.y != 0).reshape(c.B, c.V)
        assert np.isclose(r1["loss"], mm.cross_entropy_loss(p64, y), **TOL)
        assert np.allclose(r1["grad"].reshape(c.B, c.V) / c.B, mm.cross_entropy_grad(p64, y), rtol=1e-12, atol=1e-9)
        for vec in sorted({False, c.n % 4 == 0}):
            for acc in (False, True):
                ref = hr.ce_ref(c.p, c.y, c.B, dp0=c.dp0 if acc else None, vec=vec)
                loss, g = emu_ce(c, acc=acc)
                _inside("ce_loss", "%s vec=%d acc=%d" % (c.name, vec, acc), loss=hr.ratio(loss, ref["loss"], ref["d_loss"]),
                        dpred=hr.ratio(g, ref["grad"], ref["d_grad"]))


def test_ce_depths_are_the_documented_ones():
    d = {(B, V): hr.loss_depth(B * V, (B * V) % 4 == 0) for B, V in hr.CE_SHAPES}
    assert d == {(1, 1): 15, (2, 3): 15, (3, 4717): 70, (5, 4716): 110, (17, 4717): 271, (56, 4716): 277}
    assert hr.loss_depth(5 * 4716, False) == 107
    assert [hr.loss_depth(B * D, False) for B, D in hr.REP_SHAPES] == [15, 26, 94, 271]
    assert hr.meanpool_depth(300) == 23


def test_ce_sparse_case_a_dropped_heavy_term_is_far_outside():
    """Each heavy term is 11.5 against a background of 1e-5 an element: leaving one out moves the loss by many bounds."""
    for B, V in hr.CE_SPARSE_SHAPES:
        c = hr.ce_case(B, V, sparse=True)
        ref = hr.ce_ref(c.p, c.y, B, vec=c.n % 4 == 0, want_grad=False)
        for i in c.heavy:
            r = (ref["terms"][i] / B) / ref["d_loss"]
            print("sparse %s: dropping element %d moves the loss by %.1f bounds" % (c.name, i, r))
            assert ref["terms"][i] > 11.5 and r > 10.0


CE_FAULTS = ["tail skipped", "label 255 negative", "accumulate overwrites", "grad_scale missing", "eps 1e-6"]


@pytest.mark.parametrize("fault", CE_FAULTS)
def test_ce_planted_fault_leaves_the_bound_where_predicted(fault):
    c = hr.ce_case(3, 4717)
    n = c.n
    acc = fault == "accumulate overwrites"
    ref = hr.ce_ref(c.p, c.y, c.B, dp0=c.dp0 if acc else None)
    loss, g = emu_ce(c, acc=acc, fault=fault)
    ql, qg = hr.ratio(loss, ref["loss"], ref["d_loss"]), hr.ratio(g, ref["grad"], ref["d_grad"])
    out = qg > 1.0
    if fault == "tail skipped":
        assert n % 4 == 3 and out[n - 3:].all() and not out[:n - 3].any() and ql > 1.0       # the last element holds a term of 11.5
    elif fault == "label 255 negative":
        assert (out == (c.y == 255)).all() and ql > 1.0                                    # p = 1 under label 255 is planted
    elif fault == "accumulate overwrites":
        assert out.mean() > 0.99 and ql <= 1.0
    elif fault == "grad_scale missing":
        assert out.all() and ql <= 1.0
    else:
        assert out[n - 1] and out[1] and ql > 1.0                                          # p = 0 under labels 1 and 255
    print("fault ce_loss '%s': loss %.3g dpred %.3g at %s" % ((fault, float(ql)) + hr.worst(qg)))


def emu_rep(c, acc=False, fault=None, gs=hr.GS, loss0=hr.LOSS0):
    d = c.a - c.b
    invb = F32(1.0) if fault == "1/B missing" else F32(1.0) / F32(c.B)
    loss = F32(loss0) + (d * d).sum(dtype=F32) * invb
    g = F32(2.0 if fault == "gradient sign" else -2.0) * d * invb * F32(gs)
    return loss, (c.dp0 + g if acc else g).astype(F32)


def test_rep_reference_is_the_oracle_and_the_emulation_is_inside():
    for B, D in hr.REP_SHAPES:
        c = hr.rep_case(B, D)
        a, b = hr.f64(c.a).reshape(B, D), hr.f64(c.b).reshape(B, D)
        r1 = hr.rep_ref(c.a, c.b, B, gs=1.0, loss0=0.0)
        assert np.isclose(r1["loss"], mm.rep_loss(a, b), **TOL)
        assert np.allclose(r1["grad"].reshape(B, D), mm.rep_loss_grad_student(a, b), **TOL)
        for acc in (False, True):
            ref = hr.rep_ref(c.a, c.b, B, dp0=c.dp0 if acc else None)
            loss, g = emu_rep(c, acc=acc)
            _inside("rep_loss", "%s acc=%d" % (c.name, acc), loss=hr.ratio(loss, ref["loss"], ref["d_loss"]),
                    dstate=hr.ratio(g, ref["grad"], ref["d_grad"]))


@pytest.mark.parametrize("fault", ["gradient sign", "1/B missing"])
def test_rep_planted_fault_leaves_the_bound_where_predicted(fault):
    c = hr.rep_case(3, 1023)
    ref = hr.rep_ref(c.a, c.b, c.B)
    loss, g = emu_rep(c, fault=fault)
    ql, out = hr.ratio(loss, ref["loss"], ref["d_loss"]), hr.ratio(g, ref["grad"], ref["d_grad"]) > 1.0
    nz = c.a != c.b
    assert (out == nz).all() and not out[1]                             # everywhere but the planted zero difference
    assert (ql > 1.0) == (fault == "1/B missing")
    print("fault rep_loss '%s': loss %.3g" % (fault, float(ql)))


# ---------------------------------------------------------------------------- elementwise
def test_sigmoid_emulation_is_inside():
    for n in hr.ELEM_NS:
        c = hr.sigmoid_case(n)
        p = _sig32(c.z)
        ref, d = hr.sigmoid_ref(c.z)
        assert np.allclose(ref, mm.sigmoid(hr.f64(c.z)), **TOL)
        v, dv = hr.sigmoid_bwd_ref(p, c.dp)
        dz = bf16_round(c.dp * p * (F32(1.0) - p))
        _inside("sigmoid", c.name, fwd=hr.ratio(p, ref, d), bwd=hr.ratio(dz, v, dv, hr.RB))
        assert p[0] == 1.0 and (n < 2 or p[1] == 0.0)                   # +-100 saturate exactly


def emu_relu6_bwd(c, fault=None):
    x = c.x
    inside = ((x >= 0) & (x <= 6)) if fault else ((x > 0) & (x < 6))
    return np.where(inside, c.dy, F32(0.0)).astype(F32)


def test_relu6_reference_is_the_oracle_and_the_edge_fault_shows_at_0_and_6():
    for n in hr.ELEM_NS:
        c = hr.relu6_case(n)
        y, dx = hr.relu6_ref(c.x, c.dy)
        assert np.array_equal(y, mm.relu6(hr.f64(c.x)))
        y32 = np.minimum(np.maximum(c.x, F32(0.0)), F32(6.0))
        _inside("relu6", c.name, fwd=hr.exact(y32, y), fwd_bf16=hr.exact(bf16_round(y32), bf16_round(y)), bwd=hr.exact(emu_relu6_bwd(c), dx))
        out = hr.exact(emu_relu6_bwd(c, fault="gradient 1 at 0 and 6"), dx) > 1.0
        assert c.edge.size >= min(n, 3) and np.array_equal(np.nonzero(out)[0], c.edge)


def test_ema_reference_is_the_oracle_and_the_emulation_is_inside():
    for n in hr.EMA_NS:
        for decay in hr.EMA_DECAYS:
            c = hr.ema_case(n, decay)
            ref, d = hr.ema_ref(c.moving, c.batch, c.decay)
            assert np.allclose(ref, mm.bn_moving_update(hr.f64(c.moving), hr.f64(c.batch), c.decay), **TOL)
            got = c.moving - (F32(1.0) - F32(c.decay)) * (c.moving - c.batch)
            _inside("ema_update", c.name, moving=hr.ratio(got, ref, d))


def test_cast_reference_is_torch_round_to_nearest_even():
    for R, Cc in hr.CAST_SHAPES:
        c = hr.cast_case(R, Cc)
        hi, lo = hr.cast_ref(c.x)
        x = torch.from_numpy(c.x)
        thi = x.bfloat16()
        tlo = (x - thi.float()).bfloat16()
        _inside("cast_bf16", c.name, hi=hr.bits_equal_bf16(hi, thi.view(torch.int16).numpy()), lo=hr.bits_equal_bf16(lo, tlo.view(torch.int16).numpy()))
    assert bf16_bits(np.array([0x3F808000, 0x3F818000], np.uint32).view(F32)).tolist() == [0x3F80, 0x3F82]   # ties go to even


# ---------------------------------------------------------------------------- pooling and sampling
def _deq32(q):
    return (q.astype(F32) * F32(hr.SC32) + F32(hr.BI32)).astype(F32)


def _l2n32(v):
    ss = (v * v).sum(axis=-1, keepdims=True, dtype=F32)
    return (v * (F32(1.0) / np.sqrt(np.maximum(ss, F32(1e-12))))).astype(F32)


def emu_meanpool(c, normalize, fault=None):
    v = _deq32(c.x) if c.u8 else c.x
    if normalize:
        v = _l2n32(v)
    stop = c.u8 != (fault is not None)                                  # fault: the float path stops at num_frames / the uint8 path does not
    if stop:
        v = np.where((np.arange(c.T)[None, :] < c.nfr[:, None])[:, :, None], v, F32(0.0))
    return v.sum(axis=1, dtype=F32) * (F32(1.0) / c.nfr.astype(F32))[:, None]


def _oracle_avg(c, normalize):
    if c.u8:
        v = hr.f64(c.x) * hr.SC32 + hr.BI32
    else:
        v = hr.f64(c.x)
    if normalize:
        v = mm.l2_normalize(v)
    if c.u8:
        v = np.where((np.arange(c.T)[None, :] < c.nfr[:, None])[:, :, None], v, 0.0)   # padding is zero after Dequantize
    return mm.logistic_fwd(v, c.nfr, np.zeros((c.F, 1)), np.zeros(1))[1]


def test_dequantise_constant_sits_within_4U_of_the_oracle():
    q = np.arange(256)
    v, d = hr.dequant_ref(q)
    assert np.abs(v - mm.dequantize(q.astype(F64))).max() <= 4 * U
    assert hr.ratio(_deq32(q), v, d).max() <= 1.0
    fma = (q.astype(F64) * hr.SC32 + hr.BI32).astype(F32)               # the contracted form: one rounding
    assert hr.ratio(fma, v, d).max() <= 1.0


@pytest.mark.parametrize("u8", [False, True])
def test_meanpool_reference_is_the_oracle_and_the_emulation_is_inside(u8):
    for T in hr.MP_TS:
        for F in hr.MP_FS:
            c = hr.meanpool_case(T, F, u8)
            for normalize in (False, True):
                ref, d = hr.meanpool_ref(c.x, c.nfr, normalize)
                assert np.allclose(ref, _oracle_avg(c, normalize), **TOL)
                _inside("meanpool", "%s norm=%d" % (c.name, normalize), avg=hr.ratio(emu_meanpool(c, normalize), ref, d))


@pytest.mark.parametrize("u8", [False, True])
def test_meanpool_planted_fault_shows_on_the_videos_shorter_than_T(u8):
    c = hr.meanpool_case(33, 252, u8)
    ref, d = hr.meanpool_ref(c.x, c.nfr, False)
    out = hr.ratio(emu_meanpool(c, False, fault="num_frames handling swapped"), ref, d) > 1.0
    assert out[0].all() and out[1].mean() > 0.9 and not out[2].any()    # num_frames = 1, 17, 33 = T


def test_index_references_are_the_oracle_and_u_below_one_never_reaches_n():
    one_m = np.nextafter(F32(1.0), F32(0.0))
    n = np.arange(1, 301)
    assert (hr.frames_index(np.full((300, 1), one_m, F32), n)[:, 0] == n - 1).all()
    assert (hr.frames_index(np.ones((300, 1), F32), n)[:, 0] == n).all()
    for S in hr.SG_SS:
        c = hr.sample_case(S, 4, False)
        idx = hr.frames_index(c.u, c.nfr)
        assert np.array_equal(idx, mm.sample_random_frames_index(c.u, c.nfr))
        assert np.array_equal(hr.sequence_index(c.useq, c.nfr, S), mm.sample_random_sequence_index(c.useq, c.nfr, S))
        assert ((idx == c.nfr[:, None]) == (c.u == 1.0)).all() and (idx == c.nfr[:, None]).any()
        # fault: rounded instead of truncated - differs exactly where the fraction of u n is >= 1/2
        prod = c.u * c.nfr.astype(F32)[:, None]
        rounded = np.floor(prod.astype(F64) + 0.5).astype(np.int32)
        assert np.array_equal(rounded != idx, (prod - np.floor(prod)) >= 0.5) and (rounded != idx).any()
        # fault: the sequence index without min(., n - 1) - differs exactly where start + s passes n - 1
        seq = hr.sequence_index(c.useq, c.nfr, S)
        mx = np.maximum(c.nfr.astype(np.int64) - S, 0)
        start = (c.useq * (mx + 1).astype(F32)).astype(np.int32)
        raw = start[:, None] + np.arange(S)[None, :]
        assert np.array_equal(raw != seq, raw > (c.nfr - 1)[:, None]) and (raw != seq).any()


@pytest.mark.parametrize("u8", [False, True])
def test_gather_emulation_is_inside(u8):
    for S in hr.SG_SS:
        for F in hr.SG_FS:
            c = hr.sample_case(S, F, u8)
            for idx, name in ((hr.frames_index(c.u, c.nfr), "frames"), (hr.sequence_index(c.useq, c.nfr, S), "sequence")):
                ic = np.clip(idx, 0, c.T - 1)
                rows = c.x[np.arange(c.B)[:, None], ic]
                v = np.where((ic >= c.nfr[:, None])[:, :, None], F32(0.0), _deq32(rows)) if u8 else rows
                for normalize in (False, True):
                    ref, d = hr.gather_ref(c.x, idx, c.nfr, normalize)
                    _inside("sample_%s_gather" % name, "%s norm=%d" % (c.name, normalize), rows=hr.ratio(_l2n32(v) if normalize else v, ref, d))
                    if u8 and name == "frames" and S > 1:
                        assert (ref[1, 2] == 0).all() and not (ref[2, 2] == 0).any()   # u = 1: a zero frame at n = 7 < T, frame T - 1 at n = T


def test_framepool_references_and_the_last_maximum_fault():
    for B, S, Cc in hr.FP_SHAPES + [hr.FP_BWD_BIG]:
        c = hr.framepool_case(B, S, Cc)
        big = (B, S, Cc) == hr.FP_BWD_BIG
        if not big:
            ref, d = hr.framepool_mean_ref(c.y)
            assert np.allclose(ref, hr.f64(c.y).mean(axis=1), **TOL)
            s = np.zeros((B, Cc), F32)
            for f in range(S):
                s = s + c.y[:, f]
            _inside("framepool_mean_fwd", c.name, pooled=hr.ratio(s / F32(S), ref, d))
        bw, dbw = hr.framepool_mean_bwd_ref(c.dpooled, S)
        got = np.repeat((c.dpooled * (F32(1.0) / F32(S)))[:, None, :], S, axis=1)
        _inside("framepool_mean_bwd", c.name, dy=hr.ratio(got, bw, dbw))
        mx, am = hr.framepool_max_ref(c.ymax)
        assert (am[:, 0] == 0).all() and (am[:, 1] == 0).all() and am[0, 2] == 0 and mx[0, 2] == -np.inf
        last = (S - 1 - np.argmax(c.ymax[:, ::-1], axis=1)).astype(np.int32)             # fault: the last maximum wins
        diff = last != am
        if S > 1:
            assert diff[:, 0].all() and diff[:, 1].all() and diff[0, 2] and not diff[:, 3:].any()
            dy = hr.framepool_max_bwd_ref(c.dpooled, am, S)
            bad = hr.exact(hr.framepool_max_bwd_ref(c.dpooled, last, S), dy) > 1.0
            assert bad[:, 0, 0].all() and bad[:, S - 1, 0].all() and not bad[:, :, 3:].any()
        else:
            assert not diff.any()
