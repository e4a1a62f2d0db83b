"""The head, loss and pooling kernels (csrc/evc_elementwise.hip, moe_elem onwards) through their ops wrappers: every element of everything
an entry stores against the float64 reference of tests/_head_ref.py, within the bound derived there.  Covered: moe_tail_fwd / _bwd, ce_loss
and rep_loss (the plain entries and evc_ce_loss_ordered / evc_rep_loss_ordered called directly with a 256-float scratch), sigmoid_ /
sigmoid_bwd, relu6_fwd / _bwd, ema_update, fill_f32, cast_bf16 / cast_bf16_split, meanpool, sample_frames_gather / sample_sequence_gather,
framepool_mean_fwd / _bwd, framepool_max_fwd / _bwd, the __logf sweep behind LOG_ABS / LOG_REL, and three negative controls.  Output buffers
are prefilled with NaN (integers: -7) and carry a sentinel tail; every case runs twice and must repeat bit for bit, except the sums joined
by float atomics (the loss of evc_ce_loss / evc_rep_loss, evc_meanpool_fwd at T > 32).  Everything runs in this process; EVC_DETERMINISTIC
stays unset.  pytest -m gpu; every check prints `ratio <entry> <case> <output> <worst err/limit> at <index>` (pytest -s shows the lines).

Measured on an MI355X: profiles/head_parity_ratios.txt.
"""
import numpy as np
import pytest
import torch

import _head_ref as hr
from _head_ref import F32, bf16_bits, bf16_to_f64
from efficientvideoclassification_youtube8m_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 16
BF16 = torch.bfloat16


@pytest.fixture(autouse=True)
def _stop_on_a_gpu_error():
    """A GPU fault ends the session: nothing more is started on a device that a kernel of this file has just faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:   # a sticky HIP error
        pytest.exit("GPU error after a head parity test, stopping: %s" % e, returncode=3)


# ---------------------------------------------------------------------------- buffers, read-back, reporting
class Outs:
    """The output buffers of one run: each prefilled with NaN (-7 for integers) with PAD untouched elements behind it (and `lead` before)."""

    def __init__(self):
        self.bufs = []

    def new(self, shape, dtype=torch.float32, lead=0):
        n = int(np.prod(shape))
        full = torch.full((lead + n + PAD,), -7 if dtype == torch.int32 else float("nan"), dtype=dtype, device=DEV)
        self.bufs.append((full, lead, n))
        return full[lead:lead + n].view(shape)

    def holding(self, values, lead=0):
        """An in / out buffer: `values` (numpy) in the body, sentinels around it."""
        t = self.new(values.shape, torch.from_numpy(np.ascontiguousarray(values)).dtype, lead)
        t.copy_(torch.from_numpy(np.ascontiguousarray(values)))
        return t

    def finish(self):
        torch.cuda.synchronize()
        for full, lead, n in self.bufs:
            edge = torch.cat([full[:lead], full[lead + n:]])
            ok = (edge == -7).all() if full.dtype == torch.int32 else edge.isnan().all()
            assert bool(ok), "sentinel overwritten around a %s buffer of %d" % (full.dtype, n)


def dev(a, lead=0):
    """A device copy of an input; lead > 0: a view `lead` elements into a larger buffer (a misaligned pointer)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not lead:
        return t.to(DEV)
    full = torch.zeros(lead + t.numel() + PAD, dtype=t.dtype, device=DEV)
    v = full[lead:lead + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def host(t):
    """numpy of a device tensor; bf16 as bit patterns (uint16)."""
    if t.dtype == BF16:
        return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def twice(run, loose=()):
    """Run a case twice: every output not named in `loose` must repeat bit for bit.  Returns the first run's outputs."""
    a, b = run(), run()
    for k in a:
        if k not in loose and a[k] is not None:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), "%s did not repeat bit for bit" % k
    return a


class Report:
    def __init__(self, entry):
        self.entry, self.bad, self.n = entry, [], 0

    def add(self, case, output, q, limit=1.0):
        r, at = hr.worst(q)
        line = "ratio %s %s %s %.4f at %s" % (self.entry, case, output, r, at)
        print(line)
        self.n += 1
        if not r <= limit:
            self.bad.append(line)
        return r

    def done(self):
        assert self.n > 0 and not self.bad, "\n".join(self.bad)


def bf(a):
    return bf16_to_f64(a)


# ---------------------------------------------------------------------------- MoE tail
def _moe_run(c, with_rowsum=True):
    B, V, M = c.B, c.V, c.M
    ga, ea, lab = dev(c.ga), dev(c.ea), dev(c.labels)
    ldg, lde = V * (M + 1) + 8, V * M + 8

    def run():
        o = Outs()
        pred, rowsum = o.new((B, V)), o.new((B,)) if with_rowsum else None
        ops.moe_tail_fwd(ga, ea, B, V, M, pred, rowsum)
        loss = o.holding(np.zeros(1, F32))
        dpred = o.new((B, V))
        ops.ce_loss(pred, lab, loss, dpred, grad_scale=1.0)             # the step's first gradient, of the forward's own pred
        dg, de = o.new((B, ldg), BF16), o.new((B, lde), BF16)
        ops.moe_tail_bwd(ga, ea, dpred, B, V, M, dg, de)
        o.finish()
        return dict(pred=host(pred), rowsum=host(rowsum) if with_rowsum else None, dpred=host(dpred), dgate=host(dg), dexpert=host(de))
    return twice(run)


def _moe_check(rep, c, got, ref, tag=""):
    B, V, M = c.B, c.V, c.M
    n = V * (M + 1)
    name = c.name + tag
    rep.add(name, "pred", hr.ratio(got["pred"], ref["pred"], ref["d_pred"]))
    if got["rowsum"] is not None:
        rep.add(name, "rowsum", hr.ratio(got["rowsum"], ref["rowsum"], ref["d_rowsum"]))
    dg, de = bf(got["dgate"]), bf(got["dexpert"])
    rep.add(name, "dgate", hr.ratio(dg[:, :n].reshape(B, V, M + 1), ref["dga"], ref["d_dga"], hr.RB))
    rep.add(name, "dgate_pad", np.where(np.isnan(dg[:, n:]), 0.0, np.inf))
    rep.add(name, "dexpert", hr.ratio(de[:, :V * M].reshape(B, V, M), ref["dea"], ref["d_dea"], hr.RB))
    rep.add(name, "dexpert_pad", np.where(np.isnan(de[:, V * M:]), 0.0, np.inf))
    return de


@pytest.mark.parametrize("M", hr.MOE_MS)
def test_moe_tail_fwd_and_bwd(M):
    rep = Report("moe_tail")
    for V in hr.MOE_VS:
        c = hr.moe_case(M, V)
        got = _moe_run(c)
        assert np.isfinite(got["dpred"]).all()
        ref = hr.moe_ref(c.ga, c.ea, got["dpred"])
        de = _moe_check(rep, c, got, ref)
        for b, k in c.sat:                                              # expert logits +-100: e exactly 0 or 1 in f32, dexpert exactly zero
            assert (de[b, k * M:(k + 1) * M] == 0).all(), (c.name, b, k)
        if V == 255:
            plain = _moe_run(c, with_rowsum=False)
            assert np.array_equal(_bits(plain["pred"]), _bits(got["pred"])) and np.array_equal(plain["dgate"], got["dgate"])
            _moe_check(rep, c, plain, ref, " rowsum=None")
    rep.done()


def test_moe_tail_refuses_five_mixtures():
    c = hr.moe_case(4, 255)
    z = torch.zeros(3 * 255 * 6, device=DEV)
    with pytest.raises(_lib.EvcError):
        ops.moe_tail_fwd(z, z, 3, 255, 5, z, None)
    with pytest.raises(_lib.EvcError):
        ops.moe_tail_bwd(z, z, z, 3, 255, 5, z.view(3, -1), z.view(3, -1))
    assert c.M == 4


# ---------------------------------------------------------------------------- losses
def _loss_call(kind, ordered, x0, x1, B, W, loss, grad, acc, ws):
    name = "evc_%s_loss%s" % (kind, "_ordered" if ordered else "")
    args = [x0.data_ptr(), x1.data_ptr(), B, W, hr.GS, loss.data_ptr(), None if grad is None else grad.data_ptr(), 1 if acc else 0]
    if ordered:
        args.append(ws.data_ptr())
    _lib.call(name, *args, ops._stream())


def _loss_case(rep, kind, c, x0, x1, B, W, ref_fn, lead=0, tag=""):
    """One loss case on the plain and the ordered entry: accumulate_grad off, on (onto a random gradient) and no gradient at all.  loss holds 2.5
    before the call: the entries add onto it."""
    name = c.name + tag
    for variant in ("acc=0", "acc=1", "nograd"):
        acc, want = variant == "acc=1", variant != "nograd"
        ref = ref_fn(c.dp0 if acc else None, want)
        grads = {}
        for ordered in (False, True):
            def run():
                o = Outs()
                loss = o.holding(np.full(1, hr.LOSS0, F32))
                grad = (o.holding(c.dp0, lead) if acc else o.new((c.n,), lead=lead)) if want else None
                ws = o.new((256,)) if ordered else None
                _loss_call(kind, ordered, x0, x1, B, W, loss, grad, acc, ws)
                o.finish()
                return dict(loss=host(loss), grad=host(grad) if want else None)
            got = twice(run, loose=() if ordered else ("loss",))
            ent = "%s_loss%s" % (kind, "_ordered" if ordered else "")
            rep.entry = ent
            rep.add("%s %s" % (name, variant), "loss", hr.ratio(got["loss"][0], ref["loss"], ref["d_loss"]))
            if want:
                rep.add("%s %s" % (name, variant), "grad", hr.ratio(got["grad"], ref["grad"], ref["d_grad"]))
                grads[ordered] = got["grad"]
        if want:
            assert np.array_equal(_bits(grads[False]), _bits(grads[True])), "plain and ordered gradients differ: %s %s" % (name, variant)


CE_CASES = [(B, V, False, 0) for B, V in hr.CE_SHAPES] + [hr.CE_VIEW_SHAPE + (False, 1)] + [(B, V, True, 0) for B, V in hr.CE_SPARSE_SHAPES]


@pytest.mark.parametrize("B,V,sparse,lead", CE_CASES)
def test_ce_loss_plain_and_ordered(B, V, sparse, lead):
    c = hr.ce_case(B, V, sparse)
    p, y = dev(c.p, lead), dev(c.y, lead)
    vec = c.n % 4 == 0 and lead == 0
    assert (p.data_ptr() % 16 == 0) == (lead == 0)
    rep = Report("ce_loss")
    _loss_case(rep, "ce", c, p, y, B, V, lambda dp0, want: hr.ce_ref(c.p, c.y, B, dp0=dp0, vec=vec, want_grad=want), lead,
               " view+1" if lead else "")
    rep.done()


@pytest.mark.parametrize("B,D", hr.REP_SHAPES)
def test_rep_loss_plain_and_ordered(B, D):
    c = hr.rep_case(B, D)
    rep = Report("rep_loss")
    _loss_case(rep, "rep", c, dev(c.a), dev(c.b), B, D, lambda dp0, want: hr.rep_ref(c.a, c.b, B, dp0=dp0, want_grad=want))
    rep.done()


def test_logf_sweep_stays_under_the_recorded_constants():
    """evc_ce_loss with B = V = 1, no gradient and loss zeroed leaves -__logf(f32 argument): the fixed sweep of _head_ref.log_sweep."""
    p, y = hr.log_sweep()
    pd, yd = dev(p), dev(y)
    loss = torch.zeros(p.size, device=DEV)
    for i in range(p.size):
        _lib.call("evc_ce_loss", pd[i:].data_ptr(), yd[i:].data_ptr(), 1, 1, 1.0, loss[i:].data_ptr(), None, 0, ops._stream())
    torch.cuda.synchronize()
    got = host(loss)
    wa, wr = hr.log_sweep_parts(got, p, y)
    ref, arg = hr.log_sweep_ref(p, y)
    err = np.abs(got.astype(np.float64) - ref)
    i = int(np.argmax(err))
    print("logf sweep: %d arguments; worst absolute error where |log| <= 1: %.4g (2^%.2f); worst relative error where |log| > 1: %.4g (2^%.2f)"
          % (p.size, wa, np.log2(wa), wr, np.log2(wr)))
    print("logf sweep: worst error overall %.4g at argument %.9g (log %.9g)" % (err[i], arg[i], ref[i]))
    print("logf sweep: LOG_ABS = 2^%d (4 x worst -> 2^%d), LOG_REL = 2^%d (4 x worst -> 2^%d)"
          % (np.log2(hr.LOG_ABS), np.log2(hr.pow2_at_or_above(4 * wa)), np.log2(hr.LOG_REL), np.log2(hr.pow2_at_or_above(4 * wr))))
    assert wa <= hr.LOG_ABS and wr <= hr.LOG_REL
    assert err.max() <= 2.0 ** -16, "__logf further than 2^-16 from log: a finding, see DESIGN.md 4.5"


# ---------------------------------------------------------------------------- elementwise
@pytest.mark.parametrize("n", hr.ELEM_NS)
def test_sigmoid_fwd_and_bwd(n):
    c = hr.sigmoid_case(n)
    dp = dev(c.dp)

    def run():
        o = Outs()
        z = o.holding(c.z)
        ops.sigmoid_(z)
        dz = o.new((n,), BF16)
        ops.sigmoid_bwd(z, dp, dz)
        o.finish()
        return dict(p=host(z), dz=host(dz))
    got = twice(run)
    rep = Report("sigmoid")
    ref, d = hr.sigmoid_ref(c.z)
    rep.add(c.name, "fwd", hr.ratio(got["p"], ref, d))
    v, dv = hr.sigmoid_bwd_ref(got["p"], c.dp)
    rep.add(c.name, "bwd", hr.ratio(bf(got["dz"]), v, dv, hr.RB))
    assert got["p"][0] == 1.0 and (n < 2 or got["p"][1] == 0.0)
    rep.done()


@pytest.mark.parametrize("n", hr.ELEM_NS)
def test_relu6_fwd_and_bwd(n):
    c = hr.relu6_case(n)
    x, dy = dev(c.x), dev(c.dy)
    y_ref, dx_ref = hr.relu6_ref(c.x, c.dy)
    rep = Report("relu6")
    for f32o, bfo in ((True, False), (False, True), (True, True)):
        def run():
            o = Outs()
            y, yb = o.new((n,)) if f32o else None, o.new((n,), BF16) if bfo else None
            dx, dxb = o.new((n,)) if f32o else None, o.new((n,), BF16) if bfo else None
            ops.relu6_fwd(x, y, yb)
            ops.relu6_bwd(x, dy, dx, dxb)
            o.finish()
            return {k: None if t is None else host(t) for k, t in (("y", y), ("y_bf16", yb), ("dx", dx), ("dx_bf16", dxb))}
        got = twice(run)
        name = "%s f32=%d bf16=%d" % (c.name, f32o, bfo)
        if f32o:
            rep.add(name, "y", hr.exact(got["y"], y_ref))
            rep.add(name, "dx", hr.exact(got["dx"], dx_ref))
        if bfo:
            rep.add(name, "y_bf16", hr.exact(bf(got["y_bf16"]), bf(bf16_bits(y_ref))))
            rep.add(name, "dx_bf16", hr.exact(bf(got["dx_bf16"]), bf(bf16_bits(dx_ref))))
    rep.done()


@pytest.mark.parametrize("n", hr.EMA_NS)
def test_ema_update(n):
    rep = Report("ema_update")
    for decay in hr.EMA_DECAYS:
        c = hr.ema_case(n, decay)
        batch = dev(c.batch)

        def run():
            o = Outs()
            m = o.holding(c.moving)
            ops.ema_update(m, batch, decay)
            o.finish()
            return dict(moving=host(m))
        ref, d = hr.ema_ref(c.moving, c.batch, c.decay)
        rep.add(c.name, "moving", hr.ratio(twice(run)["moving"], ref, d))
    rep.done()


def test_fill_f32():
    rep = Report("fill_f32")
    for n in hr.FILL_NS:
        for lead in (0, 1):
            for value in hr.FILL_VALUES:
                def run():
                    o = Outs()
                    t = o.new((n,), lead=lead)
                    assert (t.data_ptr() % 16 == 0) == (lead == 0)
                    ops.fill_f32(t, value)
                    o.finish()
                    return dict(t=host(t))
                got = twice(run)["t"]
                same = _bits(got) == _bits(np.full(n, value, F32))      # bit for bit: -0.0 keeps its sign
                rep.add("n=%d lead=%d value=%r" % (n, lead, value), "t", np.where(same, 0.0, np.inf))
    rep.done()


@pytest.mark.parametrize("R,C", hr.CAST_SHAPES)
def test_cast_bf16_and_split(R, C):
    c = hr.cast_case(R, C)
    hi_ref, lo_ref = hr.cast_ref(c.x)
    xt = torch.from_numpy(c.x)
    t_hi = xt.bfloat16()
    t_lo = (xt - t_hi.float()).bfloat16()
    assert np.isfinite(hr.bits_equal_bf16(hi_ref, host(t_hi))).all() and np.isfinite(hr.bits_equal_bf16(lo_ref, host(t_lo))).all()
    rep = Report("cast_bf16")
    for ld_pad in (0, 8):
        xin = torch.zeros((R, C + ld_pad), device=DEV)
        xin[:, :C] = xt.to(DEV)
        xv = xin[:, :C]

        def run():
            o = Outs()
            out = o.new((R, C + ld_pad), BF16)[:, :C]
            hi, lo = o.new((R, C + ld_pad), BF16)[:, :C], o.new((R, C + ld_pad), BF16)[:, :C]
            assert xv.stride(0) == C + ld_pad and out.stride(0) == C + ld_pad
            ops.cast_bf16(xv, out) if ld_pad == 0 else _lib.call("evc_cast_f32_to_bf16", xv.data_ptr(), xv.stride(0), R, C, out.data_ptr(), out.stride(0),
                                                                  ops._stream())
            ops.cast_bf16_split(xv, hi, lo)
            o.finish()
            full = lambda v: host(v._base.view(-1)[:R * (C + ld_pad)].view(R, C + ld_pad))
            return dict(out=full(out), hi=full(hi), lo=full(lo))
        got = twice(run)
        name = "%s ld=C+%d" % (c.name, ld_pad)
        for k, r in (("out", hi_ref), ("hi", hi_ref), ("lo", lo_ref)):
            rep.add(name, k, hr.bits_equal_bf16(got[k][:, :C], r))
            if ld_pad:
                rep.add(name, k + "_pad", np.where((got[k][:, C:] & 0x7FFF) > 0x7F80, 0.0, np.inf))
    rep.done()


# ---------------------------------------------------------------------------- pooling and sampling
@pytest.mark.parametrize("u8", [False, True])
def test_meanpool(u8):
    rep = Report("meanpool")
    for T in hr.MP_TS:
        for F in hr.MP_FS:
            c = hr.meanpool_case(T, F, u8)
            x, nfr = dev(c.x), dev(c.nfr)
            for normalize in (False, True):
                ref, d = hr.meanpool_ref(c.x, c.nfr, normalize)
                for with_bf16 in (False, True):
                    def run():
                        o = Outs()
                        avg, avb = o.new((c.B, F)), o.new((c.B, F), BF16) if with_bf16 else None
                        ops.meanpool(x, nfr, avg, avb, normalize=normalize)
                        o.finish()
                        return dict(avg=host(avg), avg_bf16=host(avb) if with_bf16 else None)
                    got = twice(run, loose=("avg", "avg_bf16") if T > 32 else ())
                    name = "%s norm=%d bf16=%d" % (c.name, normalize, with_bf16)
                    rep.add(name, "avg", hr.ratio(got["avg"], ref, d))
                    if with_bf16:
                        rep.add(name, "avg_bf16", np.where(got["avg_bf16"] == bf16_bits(got["avg"]), 0.0, np.inf))
    rep.done()


def test_meanpool_refuses_bad_feature_sizes():
    for F in (6, 1284):
        x = torch.zeros((3, 5, F), device=DEV)
        with pytest.raises(_lib.EvcError):
            ops.meanpool(x, torch.ones(3, dtype=torch.int32, device=DEV), torch.zeros((3, F), device=DEV))


def _dequantise_form(c, out, idx):
    """Which f32 evaluation of q sc + bi the compiler chose (both are inside U (|v| + 2)): one rounding (an fma) or two.  Printed, not asserted."""
    ic = np.clip(idx, 0, c.T - 1)
    live = np.broadcast_to((ic < c.nfr[:, None])[:, :, None], out.shape)
    q = c.x[np.arange(c.B)[:, None], ic][live]
    fma = (q.astype(np.float64) * hr.SC32 + hr.BI32).astype(F32)        # q sc is exact in float64: one rounding
    two = (q.astype(F32) * F32(hr.SC32) + F32(hr.BI32)).astype(F32)
    print("dequantise %s: %d values, %d differ between the two forms; the kernel equals the fma form on %d of them and the two-rounding form on %d"
          % (c.name, q.size, int((fma != two).sum()), int(((out[live] == fma) & (fma != two)).sum()), int(((out[live] == two) & (fma != two)).sum())))


@pytest.mark.parametrize("u8", [False, True])
def test_sample_frames_and_sequence_gather(u8):
    rep = Report("sample_gather")
    for S in hr.SG_SS:
        for F in hr.SG_FS:
            c = hr.sample_case(S, F, u8)
            x, nfr, u, useq = dev(c.x), dev(c.nfr), dev(c.u), dev(c.useq)
            for kind, idx_ref in (("frames", hr.frames_index(c.u, c.nfr)), ("sequence", hr.sequence_index(c.useq, c.nfr, S))):
                rep.entry = "sample_%s_gather" % kind
                for normalize in (False, True):
                    ref, d = hr.gather_ref(c.x, idx_ref, c.nfr, normalize)
                    for with_idx in (True, False):
                        def run():
                            o = Outs()
                            out, idx = o.new((c.B, S, F)), o.new((c.B, S), torch.int32) if with_idx else None
                            if kind == "frames":
                                ops.sample_frames_gather(x, u, nfr, out, idx, normalize=normalize)
                            else:
                                ops.sample_sequence_gather(x, useq, nfr, S, out, idx, normalize=normalize)
                            o.finish()
                            return dict(out=host(out), idx=host(idx) if with_idx else None)
                        got = twice(run)
                        name = "%s norm=%d idx=%d" % (c.name, normalize, with_idx)
                        if with_idx:
                            rep.add(name, "idx", hr.exact(got["idx"], idx_ref))
                        if not u8 and not normalize:                    # the source frame, bit for bit
                            rep.add(name, "rows", np.where(_bits(got["out"]) == _bits(ref.astype(F32)), 0.0, np.inf))
                        else:
                            rep.add(name, "rows", hr.ratio(got["out"], ref, d))
                        if u8 and not normalize and with_idx and kind == "frames" and S == 30:
                            _dequantise_form(c, got["out"], idx_ref)
    rep.done()


@pytest.mark.parametrize("B,S,C", hr.FP_SHAPES + [hr.FP_BWD_BIG])
def test_framepool_mean_and_max(B, S, C):
    c = hr.framepool_case(B, S, C)
    big = (B, S, C) == hr.FP_BWD_BIG
    dpo = dev(c.dpooled)
    rep = Report("framepool")
    mx_ref, am_ref = hr.framepool_max_ref(c.ymax)
    if not big:
        y, ymax = dev(c.y), dev(c.ymax)
        mean_ref, d_mean = hr.framepool_mean_ref(c.y)
        for f32o, bfo in ((True, False), (False, True), (True, True)):
            def run():
                o = Outs()
                pf, pb = o.new((B, C)) if f32o else None, o.new((B, C), BF16) if bfo else None
                mf, mb, am = o.new((B, C)) if f32o else None, o.new((B, C), BF16) if bfo else None, o.new((B, C), torch.int32)
                ops.framepool_mean_fwd(y, B, S, C, pf, pb)
                ops.framepool_max_fwd(ymax, B, S, C, mf, mb, am)
                o.finish()
                return {k: None if t is None else host(t) for k, t in (("mean", pf), ("mean_bf16", pb), ("max", mf), ("max_bf16", mb), ("argmax", am))}
            got = twice(run)
            name = "%s f32=%d bf16=%d" % (c.name, f32o, bfo)
            rep.entry = "framepool_mean_fwd"
            if f32o:
                rep.add(name, "pooled", hr.ratio(got["mean"], mean_ref, d_mean))
            if bfo:
                rep.add(name, "pooled_bf16", hr.ratio(bf(got["mean_bf16"]), mean_ref, d_mean, hr.RB))
            if f32o and bfo:
                rep.add(name, "pooled_bf16_of_f32", np.where(got["mean_bf16"] == bf16_bits(got["mean"]), 0.0, np.inf))
            rep.entry = "framepool_max_fwd"
            rep.add(name, "argmax", hr.exact(got["argmax"], am_ref))
            if f32o:
                rep.add(name, "pooled", hr.exact(got["max"], mx_ref))
            if bfo:
                rep.add(name, "pooled_bf16", hr.ratio(bf(got["max_bf16"]), mx_ref, 0.0, hr.RB))
                rep.add(name, "pooled_bf16_exact", hr.bits_equal_bf16(got["max_bf16"], bf16_bits(mx_ref)))
    am = dev(am_ref)

    def run_bwd():
        o = Outs()
        dmean, dmax = o.new((B, S, C)), o.new((B, S, C))
        ops.framepool_mean_bwd(dpo, B, S, C, dmean)
        ops.framepool_max_bwd(dpo, am, B, S, C, dmax)
        o.finish()
        return dict(dmean=host(dmean), dmax=host(dmax))
    got = twice(run_bwd)
    ref, d = hr.framepool_mean_bwd_ref(c.dpooled, S)
    rep.entry = "framepool_mean_bwd"
    rep.add(c.name, "dy", hr.ratio(got["dmean"], ref, d))
    rep.entry = "framepool_max_bwd"
    want = hr.framepool_max_bwd_ref(c.dpooled, am_ref, S).astype(F32)
    rep.add(c.name, "dy", np.where(_bits(got["dmax"]) == _bits(want), 0.0, np.inf))      # routed values and exact +0.0 elsewhere
    rep.done()


# ---------------------------------------------------------------------------- negative controls: a correct kernel against a reference fed a changed input
def test_negative_control_moe_last_gate_logit_shifted():
    c = hr.moe_case(2, 257)
    got = _moe_run(c)
    ga = c.ga.copy()
    ga[..., c.M] += F32(1e-2)
    ref = hr.moe_ref(ga, c.ea, got["dpred"])
    r = hr.worst(hr.ratio(got["pred"], ref["pred"], ref["d_pred"]))
    rg = hr.worst(hr.ratio(bf(got["dgate"])[:, :c.V * 3].reshape(c.B, c.V, 3), ref["dga"], ref["d_dga"], hr.RB))
    print("negative control moe_tail (last gate logit + 1e-2 in the reference): pred %.1f at %s, dgate %.1f at %s" % (r + rg))
    assert r[0] > 10 and rg[0] > 10


def test_negative_control_ce_one_label_flipped():
    c = hr.ce_case(5, 4716)
    p, y = dev(c.p), dev(c.y)
    o = Outs()
    loss, grad = o.holding(np.full(1, hr.LOSS0, F32)), o.new((c.n,))
    ops.ce_loss(p.view(c.B, c.V), y.view(c.B, c.V), loss, grad, grad_scale=hr.GS)
    o.finish()
    y2 = c.y.copy()
    k = c.n // 2
    y2[k] = 0 if y2[k] else 1
    ref = hr.ce_ref(c.p, y2, c.B, vec=True)
    rl = float(hr.ratio(host(loss)[0], ref["loss"], ref["d_loss"]))
    rg, at = hr.worst(hr.ratio(host(grad), ref["grad"], ref["d_grad"]))
    print("negative control ce_loss (label %d flipped in the reference, p = %.4g): loss %.1f, dpred %.1f at %s" % (k, c.p[k], rl, rg, at))
    assert rg > 10 and at == (k,) and rl > 10


def test_negative_control_meanpool_one_more_frame():
    c = hr.meanpool_case(33, 252, True)
    avg = Outs()
    out = avg.new((c.B, c.F))
    ops.meanpool(dev(c.x), dev(c.nfr), out)
    avg.finish()
    ref, d = hr.meanpool_ref(c.x, c.nfr + 1, False)
    r, at = hr.worst(hr.ratio(host(out), ref, d))
    print("negative control meanpool (num_frames + 1 in the reference): avg %.1f at %s" % (r, at))
    assert r > 10
