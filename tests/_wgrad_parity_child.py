"""The GPU side of tests/test_gpu_wgrad_parity.py: the TN products of csrc/evc_gemm_tn.hip, the slab entries, the bias-gradient column sums and
engine.LstmStack._wgrad_tn against the references of tests/_wgrad_ref.py.

Imported by the test for what runs in its own process, and run as a fresh process where a switch is read once per process:

    EVC_FORCE_TILE=11   python tests/_wgrad_parity_child.py tile11   the forced 128 x 128 branch (cases of group "tile11", its negative controls)
    EVC_DETERMINISTIC=1 python tests/_wgrad_parity_child.py det      splits 1 and no segment walk (group "det"), ops.gemm_tn_det with the
                                                                     segment gap, ops.colsum_bf16, _wgrad_tn's deterministic routes

Every check prints a line `ratio <case> | <path by plan_tn> | <kind> acc=<0|1> | exact` or `| <worst err/d> at <where>` before anything is
asserted; `ok` ends a clean run.
"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import _wgrad_ref as wr  # noqa: E402

DEV = "cuda:0"
RESULTS = []                    # (line, failure message or "")


def failures():
    return [m for _, m in RESULTS if m]


def _lib():
    from efficientvideoclassification_youtube8m_amd import _lib, ops
    ops.check_device(0)
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def dev_bf16(x):
    """float32 array of bf16 values -> device bf16 tensor, bit for bit."""
    return torch.from_numpy(wr.bf16_bits(x)).to(DEV).view(torch.bfloat16)


def record(name, path, kind, acc, ratio, where, msg):
    line = "ratio %s | %s | %s acc=%d | %s" % (name, path, kind, acc, "exact" if kind == "exact" and not msg else
                                              ("DIFFERS" if kind == "exact" else "%.4f at %s" % (ratio, where)))
    print(line, flush=True)
    RESULTS.append((line, msg))


def launch(case, d, A, B1, B2, buf, acc):
    """One call of the entry the case names, C inside buf at float offset d.c0."""
    lib = _lib()
    C = buf.data_ptr() + 4 * d.c0
    if case.rows is not None:
        arr = (ctypes.c_int32 * len(case.rows))(*[int(r) for r in case.rows])
        lib.call("evc_gemm_tn2_rows", A.data_ptr(), case.lda, B1.data_ptr(), case.ldb1, case.N1, B2.data_ptr() if case.N2 else None, case.ldb2 if case.N2 else 0,
                 case.N2, case.c_col2, C, case.ldc, case.M, case.slab_rows, len(case.rows), arr, case.H, acc, _stream())
    elif case.N2:
        lib.call("evc_gemm_tn2", A.data_ptr(), case.lda, B1.data_ptr(), case.ldb1, case.N1, B2.data_ptr(), case.ldb2, case.N2, case.c_col2, C, case.ldc,
                 case.M, case.K, case.H, acc, _stream())
    else:
        lib.call("evc_gemm_tn", A.data_ptr(), case.lda, B1.data_ptr(), case.ldb1, C, case.ldc, case.M, case.N1, case.K, case.H, acc, _stream())


def run_gpu(case, d):
    """The call twice from the same prefill; returns the two buffers as numpy."""
    A, B1 = dev_bf16(d.A), dev_bf16(d.B1)
    B2 = dev_bf16(d.B2) if case.N2 else None
    b0 = torch.from_numpy(d.buf0).to(DEV)
    outs = []
    for _ in range(2):
        buf = b0.clone()
        launch(case, d, A, B1, B2, buf, d.acc)
        torch.cuda.synchronize()
        outs.append(buf.cpu().numpy())
    return outs


def run_case(case, kinds=None, accs=None):
    """Plain and accumulate, both data kinds: every element against the reference, the sentinels, and - on a path without atomics, and for
    the exact kind on every path - the second run bit for bit."""
    for kind in (case.kinds if kinds is None else kinds):
        for acc in (case.accs if accs is None else accs):
            d = wr.make_data(case, kind, acc)
            plan = case.plan(acc)
            exp, lim = wr.reference(case, d)
            g1, g2 = run_gpu(case, d)
            bad, ratio, at, msg = wr.check(case, d, g1, exp, lim, plan)
            if not msg and not wr.sentinels_intact(case, d, g1):
                msg = "%s: a sentinel changed" % case.name
            if not msg and (kind == "exact" or "atomic" not in plan["store_set"]) and not np.array_equal(wr.bits(g1), wr.bits(g2)):
                i = int(np.flatnonzero(wr.bits(g1) != wr.bits(g2))[0])
                msg = "%s [%s, %s]: the second run differs at %s" % (case.name, wr.path_name(plan), kind, wr.where_is(case, plan, d, i))
            if not msg and kind == "wide":
                msg = wr.check(case, d, g2, exp, lim, plan)[3]
            record(case.name, wr.path_name(plan), kind, acc, ratio, wr.where_is(case, plan, d, at) if at is not None else "", msg)


# ---------------------------------------------------------------------------------------------------------------------------------------
# negative controls: the kernel untouched, the reference fed a changed input
# ---------------------------------------------------------------------------------------------------------------------------------------
def negative_control(case, what, kind, acc):
    d = wr.make_data(case, kind, acc)
    plan = case.plan(acc)
    got = run_gpu(case, d)[0]
    exp, lim = wr.reference(case, d)
    msg = wr.check(case, d, got, exp, lim, plan)[3]
    if what == "row of A negated":
        k = int(np.flatnonzero(case.live_mask()[0])[3])
        d2 = wr.make_data(case, kind, acc)
        d2.A[k] = -d2.A[k]
        wrong, wlim = wr.reference(case, d2)
    elif what == "rows[t] lowered by 32":
        t = int(np.argmax(np.asarray(case.rows) > 64))
        rows = list(case.rows)
        rows[t] -= 32
        c2 = wr.Case(case.name, case.M, case.N1, case.K, N2=case.N2, rows=rows, slab_rows=case.slab_rows, forced=case.forced)
        wrong, wlim = wr.reference(c2, d)
    else:                                                  # "c_col2 off by 8": the second segment 8 columns further right, same ldc
        c2 = wr.Case(case.name, case.M, case.N1, case.K, N2=case.N2, c_col2=case.c_col2 + 8, ldc_extra=0, forced=case.forced)
        assert c2.ldc == case.ldc
        wrong, wlim = wr.reference(c2, d)
    pred = wr.bits(wrong.astype(np.float32)) != wr.bits(exp.astype(np.float32))
    bad, ratio, at, _ = wr.check(case, d, got, wrong, wlim, plan)
    if not msg and not pred.any():
        msg = "negative control %s on %s: the changed input changes nothing" % (what, case.name)
    if not msg and kind == "exact" and not np.array_equal(bad, pred):
        msg = "negative control %s on %s: %d elements flagged, %d predicted" % (what, case.name, int(bad.sum()), int(pred.sum()))
    if not msg and kind == "wide" and not (ratio > 1.0 and pred[at]):
        msg = "negative control %s on %s: worst err/d %.3g at a %s element" % (what, case.name, ratio, "predicted" if pred[at] else "not predicted")
    line = "ratio negative control (%s) %s | %s | %s acc=%d | %s" % (what, case.name, wr.path_name(plan), kind, acc,
                                                                   "%d elements flagged = predicted" % int(bad.sum()) if kind == "exact" else "factor %.3g at %s" % (ratio, wr.where_is(case, plan, d, at)))
    print(line, flush=True)
    RESULTS.append((line, msg))


NEGATIVE = {"tn128": ("tn128f 136x136 nk=6", "tn128f rows 136x136: first slab empty", "tn128f 136x(256+8) nk=6"),
            "strip": ("strip 264x72x2080", "strip rows 264x72: 16 slabs split", None),
            "tile256": ("tile256 264x264x2080", "tile256 rows 264x264: 16 slabs split", "tile256 264x(256+8)x192 gap")}


def negative_controls(branch):
    a, r, c = NEGATIVE[branch]
    for kind in ("exact", "wide"):
        negative_control(wr.case_by_name(a), "row of A negated", kind, 0)
        negative_control(wr.case_by_name(r), "rows[t] lowered by 32", kind, 1)
        if c:                                              # (the strip branch takes one column segment only)
            negative_control(wr.case_by_name(c), "c_col2 off by 8", kind, 1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# slab entries
# ---------------------------------------------------------------------------------------------------------------------------------------
SLAB_K = 3104


def slab_case(two):
    if two:
        return wr.Case("slabs2 264x(256+8)x3104 H=66 gap", 264, 256, SLAB_K, N2=8, c_col2=256 + 64, H=66, accs=(0,), det=True, branch="tile256")
    return wr.Case("slabs 264x264x3104", 264, 264, SLAB_K, ldc_extra=0, accs=(0,), det=True, branch="tile256")     # (det: plan_tn then names the plain stores of a slab)


def run_slabs(two, nslab, kind):
    """evc_gemm_tn_slabs / evc_gemm_tn2_slabs: EVERY slab against the partial product over its own K rows.  Each slab is one image of the
    case's buffer (for evc_gemm_tn_slabs, whose slabs are dense, the images overlap: FRONT sentinels, then nslab dense slabs, then sentinels)."""
    lib = _lib()
    case = slab_case(two)
    d = wr.make_data(case, kind, 0)
    M, N, ldc = case.M, case.N, case.ldc
    stride = (M + wr.BACK_ROWS) * ldc if two else M * N
    nk = SLAB_K // 32
    per = wr.ceil_div(nk, nslab)
    img = d.buf0[d.c0:]
    host = np.full(d.c0 + nslab * stride + wr.BACK_ROWS * ldc, wr.SENT, np.float32)
    for s in range(nslab):
        host[d.c0 + s * stride:d.c0 + s * stride + M * ldc] = img[:M * ldc]
    A, B1 = dev_bf16(d.A), dev_bf16(d.B1)
    outs = []
    for _ in range(2):
        buf = torch.from_numpy(host).to(DEV)
        if two:
            B2 = dev_bf16(d.B2)
            lib.call("evc_gemm_tn2_slabs", A.data_ptr(), case.lda, B1.data_ptr(), case.ldb1, case.N1, B2.data_ptr(), case.ldb2, case.N2, case.c_col2,
                     buf.data_ptr() + 4 * d.c0, ldc, stride, M, SLAB_K, case.H, nslab, _stream())
        else:
            lib.call("evc_gemm_tn_slabs", A.data_ptr(), case.lda, B1.data_ptr(), case.ldb1, buf.data_ptr() + 4 * d.c0, M, N, SLAB_K, nslab, _stream())
        torch.cuda.synchronize()
        outs.append(buf.cpu().numpy())
    got = outs[0]
    msg, worst, where = "", 0.0, ""
    if not np.array_equal(wr.bits(outs[0]), wr.bits(outs[1])):
        msg = "%s nslab=%d: the second run differs" % (case.name, nslab)
    plan = case.plan(0)
    keep = np.ones(host.shape, bool)
    for s in range(nslab):
        r0, r1 = s * per * 32, min((s + 1) * per * 32, SLAB_K)
        exp, lim = wr.reference(case, d, wr.products(case, d, rows=np.arange(r0, r1)), depth=(r1 - r0) + 2)
        n = M * ldc
        g = np.concatenate([got[:d.c0], got[d.c0 + s * stride:d.c0 + s * stride + n], exp[d.c0 + n:].astype(np.float32)])
        bad, ratio, at, m = wr.check(case, d, g, exp, lim, plan)
        keep[d.c0 + s * stride:d.c0 + s * stride + n] = False
        if m and not msg:
            msg = "slab %d of %d (K rows %d..%d): %s" % (s, nslab, r0, r1, m)
        if ratio > worst:
            worst, where = ratio, "slab %d %s" % (s, wr.where_is(case, plan, d, at))
    if not msg and not (wr.bits(got)[keep] == wr.bits(host)[keep]).all():
        msg = "%s nslab=%d: a sentinel between or behind the slabs changed" % (case.name, nslab)
    record("%s nslab=%d" % (case.name, nslab), "tile256 %d slabs x %d steps, plain stores" % (nslab, per), kind, 0, worst, where, msg)


def slab_refusal():
    """nslab = 50 at 97 K steps: 2 steps per slab, the last slab would start at step 98."""
    lib = _lib()
    from efficientvideoclassification_youtube8m_amd._lib import EvcError
    case = slab_case(False)
    d = wr.make_data(case, "exact", 0)
    A, B1 = dev_bf16(d.A), dev_bf16(d.B1)
    buf = torch.full((50 * case.M * case.N,), float(wr.SENT), device=DEV)
    for name, args in (("evc_gemm_tn_slabs", (A.data_ptr(), case.lda, B1.data_ptr(), case.ldb1, buf.data_ptr(), case.M, case.N, SLAB_K, 50, _stream())),
                       ("evc_gemm_tn2_slabs", (A.data_ptr(), case.lda, B1.data_ptr(), case.ldb1, case.N, None, 0, 0, case.N, buf.data_ptr(), case.N, case.M * case.N,
                                               case.M, SLAB_K, 0, 50, _stream()))):
        try:
            lib.call(name, *args)
            msg = "%s took nslab=50 at 97 K steps" % name
        except EvcError as e:
            msg = "" if "empty slab" in str(e) else "%s: %s" % (name, e)
        torch.cuda.synchronize()
        if not msg and not bool((buf == float(wr.SENT)).all()):
            msg = "%s refused the call and wrote" % name
        record("%s nslab=50 refused" % name, "refusal", "exact", 0, 0.0, "", msg)


def rows_refusal():
    """slab_rows = 40, 3 slabs: K = 120 is no multiple of 32."""
    lib = _lib()
    from efficientvideoclassification_youtube8m_amd._lib import EvcError
    A = torch.zeros((128, 16), dtype=torch.bfloat16, device=DEV)
    buf = torch.full((8 * 8,), float(wr.SENT), device=DEV)
    arr = (ctypes.c_int32 * 3)(40, 20, 8)
    try:
        lib.call("evc_gemm_tn2_rows", A.data_ptr(), 16, A.data_ptr(), 16, 8, None, 0, 0, 0, buf.data_ptr(), 8, 8, 40, 3, arr, 0, 0, _stream())
        msg = "evc_gemm_tn2_rows took slab_rows = 40 x 3"
    except EvcError as e:
        msg = "" if "K %" in str(e) else str(e)
    torch.cuda.synchronize()
    if not msg and not bool((buf == float(wr.SENT)).all()):
        msg = "evc_gemm_tn2_rows refused the call and wrote"
    record("evc_gemm_tn2_rows slab_rows=40 x 3 refused", "refusal", "exact", 0, 0.0, "", msg)


def run_sum_slabs(kind, acc):
    """evc_sum_slabs with ld != ldc: the in-order f32 sum, reproduced on the host bit for bit (for the exact kind that is the integer sum)."""
    lib = _lib()
    rng = np.random.default_rng(31 + acc)
    nslab, M, N, ld, ldc, stride = 5, 37, 44, 52, 48, 37 * 52 + 8
    if kind == "exact":
        slabs = rng.integers(-2 ** 20, 2 ** 20, (nslab, stride)).astype(np.float32) * np.float32(wr.SA * wr.SB)
        C0 = rng.integers(-2 ** 20, 2 ** 20, (M + 2, ldc)).astype(np.float32) * np.float32(wr.SA * wr.SB)
    else:
        slabs = (rng.standard_normal((nslab, stride)) * 10.0 ** rng.uniform(-6, 0, (nslab, stride))).astype(np.float32)
        C0 = rng.standard_normal((M + 2, ldc)).astype(np.float32)
    if not acc:
        C0[:M, :N] = np.nan
    C0[M:] = wr.SENT
    C0[:, N:] = wr.SENT
    want = C0.copy()
    a = C0[:M, :N].copy() if acc else np.zeros((M, N), np.float32)
    for s in range(nslab):
        a = a + slabs[s, :M * ld].reshape(M, ld)[:, :N]
    want[:M, :N] = a
    sl, C = torch.from_numpy(slabs).to(DEV), torch.from_numpy(C0).to(DEV)
    lib.call("evc_sum_slabs", sl.data_ptr(), stride, nslab, M, N, ld, C.data_ptr(), ldc, acc, _stream())
    torch.cuda.synchronize()
    got = C.cpu().numpy()
    bad = wr.bits(got) != wr.bits(want)
    msg = ""
    if bad.any():
        r, c = np.argwhere(bad)[0]
        msg = "evc_sum_slabs %s acc=%d: %d elements differ, first at row %d col %d: got %r want %r" % (kind, acc, int(bad.sum()), r, c, float(got[r, c]), float(want[r, c]))
    line = "ratio evc_sum_slabs 5 x 37x44 ld=52 ldc=48 | in-order f32 sum | %s acc=%d | %s" % (kind, acc, "bit-equal" if not msg else "DIFFERS")
    print(line, flush=True)
    RESULTS.append((line, msg))


# ---------------------------------------------------------------------------------------------------------------------------------------
# bias gradient: column sums of a bf16 matrix
# ---------------------------------------------------------------------------------------------------------------------------------------
COLSUM_R = (1, 63, 64, 200, 64 * 513)
COLSUM_C = (8, 264, 2056)
TAIL = 64


_COLSUM_CACHE = {}


def colsum_data(R, C, kind, ld):
    """[R][ld] float32 of bf16 values: a block of at most 1026 random rows, repeated (the wide kind scales each repeat by 2^(i % 3 - 1))."""
    rng = np.random.default_rng(R * 4099 + C + (kind == "wide"))
    blk = min(R, 1026)
    if kind == "exact":
        b = rng.integers(-255, 256, (blk, C)).astype(np.float32) * np.float32(wr.SA)
    else:
        b = rng.standard_normal((blk, C)) * 10.0 ** rng.uniform(-6, -1, (blk, C))
        b = wr.to_bf16(np.where(np.abs(b) < 1e-15, 1e-15, b))
    x = np.full((R, ld), 3.0, np.float32)
    for i, r0 in enumerate(range(0, R, blk)):
        n = min(blk, R - r0)
        x[r0:r0 + n, :C] = b[:n] * np.float32(2.0 ** (i % 3 - 1) if kind == "wide" else 1.0)
    return x


def run_colsum(R, C, kind, H=0, entry="atomic", ws_rows=0):
    """entry: atomic (evc_colsum_bf16), det (evc_colsum_bf16_det with ws_rows partial rows), ops (ops.colsum_bf16)."""
    lib = _lib()
    ld = C + 8
    if _COLSUM_CACHE.get("key") != (R, C, kind):                      # (one matrix per (R, C, kind), shared by the entries and both layouts)
        x = colsum_data(R, C, kind, ld)
        x64 = x[:, :C].astype(np.float64)
        _COLSUM_CACHE.update(key=(R, C, kind), xd=dev_bf16(x), want=x64.sum(0), lim=R * wr.U * np.abs(x64).sum(0), top=np.abs(x64).sum(0).max())
    xd, want, lim = _COLSUM_CACHE["xd"], _COLSUM_CACHE["want"], _COLSUM_CACHE["lim"]
    if kind == "exact":
        assert _COLSUM_CACHE["top"] / wr.SA < 2.0 ** 24
    if H:
        c = np.arange(C)
        perm = (c % 4) * H + c // 4
        w2, l2 = np.empty_like(want), np.empty_like(lim)
        w2[perm], l2[perm] = want, lim
        want, lim = w2, l2
    outs = []
    for _ in range(2):
        out = torch.full((C + TAIL,), float(wr.SENT), device=DEV)
        out[:C] = float("nan")
        if entry == "atomic":
            lib.call("evc_colsum_bf16", xd.data_ptr(), ld, R, C, H, out.data_ptr(), _stream())
        elif entry == "det":
            ws = torch.full((ws_rows * C + TAIL,), float(wr.SENT), device=DEV)
            lib.call("evc_colsum_bf16_det", xd.data_ptr(), ld, R, C, H, out.data_ptr(), ws.data_ptr(), ws_rows, _stream())
            torch.cuda.synchronize()
            assert bool((ws[ws_rows * C:] == float(wr.SENT)).all()), "evc_colsum_bf16_det wrote behind its workspace"
        else:
            from efficientvideoclassification_youtube8m_amd import ops
            ops.colsum_bf16(xd, R, C, out, deinterleave_H=H)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    got = outs[0]
    msg, ratio, at = "", 0.0, 0
    if not (got[C:] == wr.SENT).all():
        msg = "colsum R=%d C=%d: the floats behind out[C] changed" % (R, C)
    elif kind == "exact":
        bad = wr.bits(got[:C]) != wr.bits(want.astype(np.float32))
        if bad.any():
            at = int(np.flatnonzero(bad)[0])
            msg = "colsum %s R=%d C=%d H=%d exact: %d columns differ, first out[%d]: got %r want %r" % (entry, R, C, H, int(bad.sum()), at, float(got[at]), want[at])
    else:
        r = np.abs(got[:C].astype(np.float64) - want) / lim
        r = np.where(np.isnan(r), np.inf, r)
        at = int(np.argmax(r))
        ratio = float(r[at])
        if ratio > 1.0:
            msg = "colsum %s R=%d C=%d H=%d wide: err/d %.3g at out[%d]: got %r want %r" % (entry, R, C, H, ratio, at, float(got[at]), want[at])
    if not msg and (kind == "exact" or entry != "atomic") and not np.array_equal(wr.bits(outs[0]), wr.bits(outs[1])):
        msg = "colsum %s R=%d C=%d: the second run differs" % (entry, R, C)
    record("colsum R=%d C=%d H=%d" % (R, C, H), entry + (" ws_rows=%d" % ws_rows if entry == "det" else ""), kind, 0, ratio, "out[%d]" % at, msg)


def run_colsums(entry):
    for R in COLSUM_R:
        for C in COLSUM_C:
            for kind in ("exact", "wide"):
                for H in (0, C // 4):
                    if entry == "det":
                        for ws in sorted({max(1, R // 64 - 1), R // 64 + 7} if R >= 128 else {1, 3}):      # below and above R / 64
                            run_colsum(R, C, kind, H, "det", ws)
                    else:
                        run_colsum(R, C, kind, H, entry)


# ---------------------------------------------------------------------------------------------------------------------------------------
# engine.LstmStack._wgrad_tn
# ---------------------------------------------------------------------------------------------------------------------------------------
class _Stack:
    def __init__(self, H):
        self.H = H


def run_engine(H, kin, rows, live=None, qmax=None):
    """_wgrad_tn unbound on a stand-in that carries H: gW [4H][kin + H] (prefilled with integers, accumulate is its contract) against
    gW0 + de-interleaved dz^T [layer_in | h_prev], exact kind, the whole image bit for bit.  live = (rows per slab, slab rows)."""
    from efficientvideoclassification_youtube8m_amd import engine, ops
    ops.check_device(0)
    rng = np.random.default_rng(H + kin + rows)
    M = 4 * H
    if live is None:
        idx = np.arange(rows)
        cover = idx
    else:
        lr, slab = live
        idx = np.concatenate([t * slab + np.arange(min(max(r, 0), slab)) for t, r in enumerate(lr)])
        cover = np.concatenate([t * slab + np.arange((min(max(r, 0), slab) + 31) // 32 * 32) for t, r in enumerate(lr)])
    q = wr.q_of(max(len(cover), 32)) if qmax is None else qmax
    ia = rng.integers(-q, q + 1, (len(idx), M)).astype(np.float32)
    ib = rng.integers(-q, q + 1, (len(cover), kin + H)).astype(np.float32)
    assert q * q * len(idx) + 2 ** 22 < 2 ** 24
    dz = torch.zeros((rows, M), dtype=torch.bfloat16, device=DEV)
    dz[torch.from_numpy(idx).to(DEV)] = dev_bf16(ia * np.float32(wr.SA))
    xin = torch.full((rows, kin), wr.GARBAGE, dtype=torch.bfloat16, device=DEV)
    hp = torch.full((rows, H), -wr.GARBAGE, dtype=torch.bfloat16, device=DEV)
    cv = torch.from_numpy(cover).to(DEV)
    xin[cv] = dev_bf16(np.ascontiguousarray(ib[:, :kin]) * np.float32(wr.SB))
    hp[cv] = dev_bf16(np.ascontiguousarray(ib[:, kin:]) * np.float32(wr.SB))
    g0 = rng.integers(-2 ** 22, 2 ** 22 + 1, (M + 1, kin + H)).astype(np.float32) * np.float32(wr.SA * wr.SB)
    g0[M:] = wr.SENT
    pos = {int(r): i for i, r in enumerate(cover)}
    ibl = ib[[pos[int(r)] for r in idx]]
    if len(idx) * M * (kin + H) > 2e9:                    # exact in f32 as well (every partial sum an integer below 2^24): an f32 BLAS product
        P = (torch.from_numpy(ia).T @ torch.from_numpy(ibl)).numpy().astype(np.float64)
    else:
        P = wr.int_product(ia, ibl).astype(np.float64)
    want = g0.astype(np.float64)
    want[wr.out_rows(M, H)] += P * (wr.SA * wr.SB)
    outs = []
    for _ in range(2):
        gW = torch.from_numpy(g0).to(DEV)
        engine.LstmStack._wgrad_tn(_Stack(H), dz, xin, hp, kin, rows, gW[:M], live=live)
        torch.cuda.synchronize()
        outs.append(gW.cpu().numpy())
    bad = wr.bits(outs[0]) != wr.bits(want.astype(np.float32))
    msg = ""
    if bad.any():
        r, c = np.argwhere(bad)[0]
        msg = "_wgrad_tn H=%d kin=%d rows=%d: %d elements differ, first at gW[%d][%d] (gate %d unit %d, %s column %d): got %r want %r" % (
            H, kin, rows, int(bad.sum()), r, c, r // H, r % H, "input" if c < kin else "recurrent", c if c < kin else c - kin, float(outs[0][r, c]), want[r, c])
    elif not np.array_equal(wr.bits(outs[0]), wr.bits(outs[1])):
        msg = "_wgrad_tn H=%d kin=%d rows=%d: the second run differs" % (H, kin, rows)
    line = "ratio _wgrad_tn H=%d kin=%d rows=%d live=%s | %s | exact acc=1 | %s" % (H, kin, rows, "no" if live is None else "%d of %d rows" % (len(idx), rows),
                                                                                 "deterministic" if ops.DETERMINISTIC else "default", "exact" if not msg else "DIFFERS")
    print(line, flush=True)
    RESULTS.append((line, msg))


# ---------------------------------------------------------------------------------------------------------------------------------------
def det_gap():
    """ops.gemm_tn_det as the engine calls it: two segments with a gap, rows de-interleaved, accumulate - slabs, then the slab sum."""
    from efficientvideoclassification_youtube8m_amd import ops
    case = wr.Case("ops.gemm_tn_det 264x(256+8)x3104 H=66 gap", 264, 256, 3104, N2=8, c_col2=256 + 64, H=66, ldc_extra=0, det=True, accs=(1,), branch="tile256")
    for kind in ("exact", "wide"):
        d = wr.make_data(case, kind, 1)
        exp, lim = wr.reference(case, d, depth=case.K + 3 + 1)
        A, B1, B2 = dev_bf16(d.A), dev_bf16(d.B1), dev_bf16(d.B2)
        outs = []
        for _ in range(2):
            buf = torch.from_numpy(d.buf0).to(DEV)
            out = buf[d.c0:d.c0 + case.M * case.ldc].view(case.M, case.ldc)
            ops.gemm_tn_det(A[:, :case.M], B1[:, :case.N1], case.M, case.N1, case.K, out, row_interleave_H=case.H, accumulate=True, ldc=case.ldc,
                            B2=B2[:, :case.N2], N2=case.N2, c_col2=case.c_col2)
            torch.cuda.synchronize()
            outs.append(buf.cpu().numpy())
        bad, ratio, at, msg = wr.check(case, d, outs[0], exp, lim)
        if not msg and not np.array_equal(wr.bits(outs[0]), wr.bits(outs[1])):
            msg = case.name + ": the second run differs"
        record(case.name, "3 slabs + slab sum", kind, 1, ratio, wr.where_is(case, case.plan(1), d, at) if at is not None else "", msg)


def main(mode):
    if mode == "tile11":
        assert os.environ.get("EVC_FORCE_TILE") == "11"
        for c in wr.CASES:
            if c.group == "tile11":
                run_case(c)
        negative_controls("tn128")
    elif mode == "det":
        assert os.environ.get("EVC_DETERMINISTIC") == "1"
        for c in wr.DET_CASES:
            run_case(c)
        det_gap()
        for R, C in ((200, 264), (64 * 513, 2056), (63, 8)):
            for kind in ("exact", "wide"):
                run_colsum(R, C, kind, C // 4, "ops")
        run_engine(64, 264, 2080)
        run_engine(64, 72, 2080)
    else:
        raise SystemExit("unknown mode %r" % mode)
    torch.cuda.synchronize()
    if failures():
        print("\n".join(failures()))
        raise SystemExit(1)
    print("ok")


if __name__ == "__main__":
    main(sys.argv[1])
