"""The clip + Adam update kernels (csrc/evc_optim.hip, the a8 + a9 block of csrc/evc_elementwise.hip, moe_update_kernel of csrc/evc_gemm_tn.hip)
and the Gram-matrix clip norm (csrc/evc_moe_norms.hip) through their ops wrappers, or _lib.call where a wrapper cannot reach a path (strided
images, ldT beyond the live columns): every element of everything an entry stores against the float64 reference of tests/_optim_ref.py, within
the bound derived there; every shadow and image bit for bit against the host's own cast of the f32 p the kernel stored.  Output and in / out
buffers sit inside NaN (bytes: 0xA5) sentinels, the columns between C and ld of every strided image and the region behind ldT included; every
case runs twice and must repeat bit for bit, except the sums of evc_grad_sqnorm (float atomics).  Everything runs in this process with no
environment variable set.  pytest -m gpu; every check prints `ratio <entry> <case> <output> <worst err/limit> at <index>` (pytest -s shows the
lines).

Measured on an MI355X: profiles/optim_parity_ratios.txt.
"""
import numpy as np
import pytest
import torch

import _optim_ref as orf
from _optim_ref import F32, bf16_bits, exact, f64, ratio
from efficientvideoclassification_youtube8m_amd import _lib, ops
from test_gpu_head_parity import Report, _bits, dev, host, twice

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 16
BF16, F16, U8 = torch.bfloat16, torch.float16, torch.uint8
BYTE = 0xA5


@pytest.fixture(autouse=True)
def _stop_on_a_gpu_error():
    """A GPU fault ends the session: nothing more is started on a device that a kernel of this file has just faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:   # a sticky HIP error
        pytest.exit("GPU error after an optimizer parity test, stopping: %s" % e, returncode=3)


class Bufs:
    """The output and in / out buffers of one run: NaN (uint8: 0xA5) everywhere the kernel is not meant to write - `lead` elements in front, PAD
    behind, and the columns C .. ld of a strided image."""

    def __init__(self):
        self.bufs = []

    def _full(self, n, dtype):
        return torch.full((n,), BYTE if dtype == U8 else float("nan"), dtype=dtype, device=DEV)

    def new(self, shape, dtype=torch.float32, lead=0, ld=None):
        """A [..] buffer; with ld a [R][C] view of rows ld apart."""
        if ld is None:
            n = int(np.prod(shape))
            full = self._full(lead + n + PAD, dtype)
            self.bufs.append((full, lead, n, None))
            return full[lead:lead + n].view(shape)
        R, C = shape
        full = self._full(lead + R * ld + PAD, dtype)
        self.bufs.append((full, lead, R * ld, (R, C, ld)))
        return full[lead:lead + R * ld].view(R, ld)[:, :C]

    def holding(self, values, lead=0):
        values = np.ascontiguousarray(values)
        t = self.new(values.shape, torch.from_numpy(values).dtype, lead)
        t.copy_(torch.from_numpy(values))
        return t

    def finish(self):
        torch.cuda.synchronize()
        for full, lead, n, strided in self.bufs:
            edge = [full[:lead], full[lead + n:]]
            if strided:
                R, C, ld = strided
                edge.append(full[lead:lead + n].view(R, ld)[:, C:].reshape(-1))
            edge = torch.cat(edge)
            ok = (edge == BYTE).all() if full.dtype == U8 else edge.isnan().all()
            assert bool(ok), "sentinel overwritten around a %s buffer of %d" % (full.dtype, n)


def dev_bf16(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(DEV).view(BF16)


def pmv_check(rep, name, got, ref, tag=""):
    for k in "pmv":
        rep.add(name, tag + k, ratio(got[tag + k].reshape(np.shape(ref[k])), ref[k], ref["d_" + k]))


def unchanged(rep, name, what, got, want):
    rep.add(name, what, exact(_bits(np.asarray(got)), _bits(np.asarray(want))))


def all0_check(rep, name, what, p_got, t):
    """g = m = v = 0 (no l2 term in these entries): p comes back bit for bit."""
    i = t.where["all0"]
    if i.size:
        unchanged(rep, name, what + " where g=m=v=0", p_got.reshape(-1)[i], t.p[i])


# ---------------------------------------------------------------------------- evc_grad_sqnorm
@pytest.mark.parametrize("n", orf.SQNORM_NS)
def test_grad_sqnorm(n):
    rep = Report("grad_sqnorm")
    c = orf.bulk(n, 9000 + n % 1000)
    g, p = dev(c.g), dev(c.p)
    before = np.array([0.37, 1.5], F32)
    for with_p, l2 in ((False, 0.0), (True, 2e-8), (True, 0.5)):
        l2 = float(F32(l2))

        def run():
            o = Bufs()
            sums = o.holding(before)
            ops.grad_sqnorm(g, p if with_p else None, l2, sums)
            o.finish()
            return dict(sums=host(sums))
        got = twice(run, loose=("sums",))["sums"]                       # float atomics: the only sums of this file that may differ between runs
        ref, bnd = orf.sqnorm_ref(c.g, c.p if with_p else None, l2, f64(before))
        name = "n=%d %s" % (n, "l2=%g" % l2 if with_p else "p=None")
        rep.add(name, "sums[0]", ratio(got[0], ref[0], bnd[0]))
        if with_p:
            rep.add(name, "sums[1]", ratio(got[1], ref[1], bnd[1]))
        else:
            unchanged(rep, name, "sums[1] untouched", got[1], before[1])
    rep.done()


# ---------------------------------------------------------------------------- evc_sqnorm2_partials
@pytest.mark.parametrize("na,nb", orf.PARTIALS_NS)
def test_sqnorm2_partials(na, nb):
    rep = Report("sqnorm2_partials")
    a = orf.bulk(na, 9050).g
    b = None if nb is None else orf.bulk(nb, 9051).g
    ga, gb = dev(a), None if b is None else dev(b)
    k = 1024 if b is None else 1025

    def run():
        o = Bufs()
        part = o.new((k,))
        _lib.call("evc_sqnorm2_partials", ga.data_ptr(), na, None if gb is None else gb.data_ptr(), 0 if gb is None else nb, part.data_ptr(), ops._stream())
        o.finish()
        return dict(part=host(part))
    got = twice(run)["part"]
    ref, bnd = orf.partials_ref(a, b)
    own = np.bincount(orf.partials_owner(na), minlength=1024) > 0
    name = "na=%d nb=%s" % (na, nb)
    rep.add(name, "partials", ratio(got, ref, bnd))
    rep.add(name, "blocks that own nothing", exact(got[:1024][~own], np.zeros((~own).sum(), F32)))
    rep.done()


# ---------------------------------------------------------------------------- evc_clip_adam_step
def _step_run(c, lead, with_bf16, ss32=None):
    n = c.p.size
    g = dev(c.g, lead)
    sums = dev(np.array([c.ss32 if ss32 is None else ss32, 0.0], F32))   # the norm is fed from the host: nothing here depends on an atomic

    def run():
        o = Bufs()
        p, m, v = o.holding(c.p, lead), o.holding(c.m, lead), o.holding(c.v, lead)
        pb = o.new((n,), BF16, lead) if with_bf16 else None
        assert (p.data_ptr() % 16 == 0) == (lead == 0)
        ops.clip_adam_step(p, g, m, v, c.hp.l2, sums, c.hp.clip, c.hp.lr, p_bf16=pb, **c.hp.kw())
        o.finish()
        return dict(p=host(p), m=host(m), v=host(v), pb=host(pb) if with_bf16 else None)
    return twice(run)


def _step_check(rep, c, got, ref, tag):
    name = c.name + tag
    pmv_check(rep, name, got, ref)
    if got["pb"] is not None:
        rep.add(name, "p_bf16", exact(got["pb"], bf16_bits(got["p"])))
    if c.hp.l2 == 0.0 and c.where["all0"].size:
        i = c.where["all0"]
        unchanged(rep, name, "p where g=m=v=0", got["p"][i], c.p[i])
    assert np.isfinite(got["p"]).all() and np.isfinite(got["m"]).all() and (got["v"] >= 0).all()


@pytest.mark.parametrize("n", orf.STEP_NS[:3])
def test_clip_adam_step(n):
    rep = Report("clip_adam_step")
    cases = [orf.step_case(n, l2, mode) for l2 in orf.L2S for mode in orf.CLIPS] + [orf.step_case(n, 2e-8, "active", odd=True)]
    for c in cases:
        ref = orf.step_ref(c)
        for lead in (0, 1):
            for with_bf16 in (True, False):
                got = _step_run(c, lead, with_bf16)
                _step_check(rep, c, got, ref, " %s%s" % ("aligned" if lead == 0 else "offset", " bf16" if with_bf16 else ""))
    rep.done()


@pytest.mark.parametrize("k", range(len(orf.STEP_BIG)))
def test_clip_adam_step_past_the_grid(k):
    """n = 4200003: past 4096 blocks x 256 x 4, a second strided trip; aligned with the bf16 shadow, offset (scalar path) without, aligned without."""
    rep = Report("clip_adam_step")
    l2, mode = orf.STEP_BIG[k]
    c = orf.step_case(orf.STEP_NS[3], l2, mode)
    lead, with_bf16 = ((0, True), (1, False), (0, False))[k]
    got = _step_run(c, lead, with_bf16)
    _step_check(rep, c, got, orf.step_ref(c), " %s%s" % ("aligned" if lead == 0 else "offset", " bf16" if with_bf16 else ""))
    rep.done()


# ---------------------------------------------------------------------------- evc_clip_adam_small
def test_clip_adam_small():
    rep = Report("clip_adam_small")
    cs, hp = orf.small_cases()
    gs = [dev(c.g) for c in cs]
    for count in (16, 1):
        def run():
            o = Bufs()
            ps, ms, vs = ([o.holding(getattr(c, a)) for c in cs[:count]] for a in "pmv")
            sums = o.new((count, 2))
            ops.clip_adam_small(ps, gs[:count], ms, vs, [sums[i] for i in range(count)], hp.clip, hp.lr, **hp.kw())
            o.finish()
            out = dict(sums=host(sums))
            for i in range(count):
                out.update({"p%d" % i: host(ps[i]), "m%d" % i: host(ms[i]), "v%d" % i: host(vs[i])})
            return out
        got = twice(run)
        for i, c in enumerate(cs[:count]):
            ref = orf.small_ref(c, hp)
            name = "%s count=%d" % (c.name, count)
            rep.add(name, "sums[0]", ratio(got["sums"][i, 0], ref["ss"], ref["d_ss"]))
            rep.add(name, "sums[1]", exact(got["sums"][i, 1], F32(0.0)))
            pmv_check(rep, name, {k: got["%s%d" % (k, i)] for k in "pmv"}, ref)
            all0_check(rep, name, "p", got["p%d" % i], c)
            assert np.isfinite(got["p%d" % i]).all()
        if count == 16:
            z = orf.SMALL_ZERO_G
            assert got["sums"][z, 0] == 0.0 and not (cs[z].g != 0).any()
    rep.done()


# ---------------------------------------------------------------------------- evc_lstm_adam_fused, evc_adam2d_fused
def _images_check(rep, name, got, p, H, lay):
    """Every shadow and image against the host's cast of the stored f32 p [R][C]."""
    R, C = p.shape
    pb = bf16_bits(p)
    rep.add(name, "p_bf16", exact(got["p_bf16"], pb))
    if H:
        rep.add(name, "pT", exact(got["pT"][:, :R], orf.lstm_transposed(pb, H)))
        live = R
    else:
        live = (R + 63) // 64 * 64
        rep.add(name, "pT", exact(got["pT"][:, :R], np.ascontiguousarray(pb.T)))
        rep.add(name, "pT pad zero", exact(got["pT"][:, R:live], np.zeros((C, live - R), np.uint16)))
    rep.add(name, "pT behind the live columns", np.where(np.isnan(orf.bf16_to_f64(got["pT"][:, live:])), 0.0, np.inf))
    if lay["f16"]:
        rep.add(name, "p_f16", exact(_bits(got["p_f16"]), _bits(orf.f16_wide(p, lay["nin"], lay["nseg"]))))
    if lay["fp8"]:
        rep.add(name, "p_fp8", exact(got["p_fp8"], orf.fp8_image(p, lay["col0"], lay["hi_cols"], lay["lo_exp"], lay["hi_exp"], lay["hi_tail"])))


def _lstm_run(c, images, ldT_extra=0):
    H, nin, R, C = c.H, c.nin, c.R, c.C
    nseg, col0, hi_cols, hi_tail, has16, has8 = orf.lstm_images(images, H, nin)
    lay = dict(f16=has16, fp8=has8, nin=nin, nseg=nseg, col0=col0, hi_cols=hi_cols, hi_tail=hi_tail, lo_exp=ops.FP8_W_SCALE_EXP, hi_exp=ops.FP8_WX_HI_EXP)
    w16 = nseg * nin + (C - nin)
    w8 = 2 * (C - col0) if hi_tail else C - col0 + hi_cols
    ldT = 4 * H + ldT_extra
    g, gb = dev(c.w.g), dev(c.b.g)
    hp = c.hp

    def run():
        o = Bufs()
        p, m, v = (o.holding(getattr(c.w, a).reshape(R, C)) for a in "pmv")
        pb, mb, vb = (o.holding(getattr(c.b, a)) for a in "pmv")
        part = o.new((1025,))
        sw, sb = o.holding(np.array([7.0, 9.0], F32)), o.holding(np.array([5.0, 3.0], F32))
        shf, shb = o.new((R, C), BF16), o.new((C, ldT), BF16)
        p16 = o.new((R, w16), F16, ld=w16 + 4) if has16 else None
        p8 = o.new((R, w8), U8, ld=w8 + 4) if has8 else None
        _lib.call("evc_sqnorm2_partials", g.data_ptr(), R * C, gb.data_ptr(), R, part.data_ptr(), ops._stream())
        _lib.call("evc_lstm_adam_fused", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), pb.data_ptr(), gb.data_ptr(), mb.data_ptr(), vb.data_ptr(),
                  H, C, part.data_ptr(), sw.data_ptr(), sb.data_ptr(), hp.clip, hp.lr, hp.b1, hp.b2, hp.eps, shf.data_ptr(), shb.data_ptr(), ldT,
                  None if p16 is None else p16.data_ptr(), w16 + 4 if has16 else 0, nin, nseg, None if p8 is None else p8.data_ptr(), w8 + 4 if has8 else 0,
                  col0, hi_cols, lay["lo_exp"], lay["hi_exp"], 1 if hi_tail else 0, ops._stream())
        o.finish()
        out = dict(p=host(p), m=host(m), v=host(v), bp=host(pb), bm=host(mb), bv=host(vb), part=host(part), sw=host(sw), sb=host(sb),
                   p_bf16=host(shf), pT=host(shb))
        if has16:
            out["p_f16"] = host(p16)
        if has8:
            out["p_fp8"] = host(p8)
        return out
    return twice(run), lay


def _lstm_check(rep, c, got, lay, name):
    Dp, Db = orf.partials_depth(c.R * c.C), orf.partials_depth(c.R, False)
    rw, rb = orf.fused_ref(c.w, c.hp, Dp + 22), orf.fused_ref(c.b, c.hp, Db)
    pr, pbnd = orf.partials_ref(c.w.g, c.b.g)
    rep.add(name, "partials", ratio(got["part"], pr, pbnd))
    rep.add(name, "sums_w[0]", ratio(got["sw"][0], rw["ss"], rw["d_ss"]))
    rep.add(name, "sums_b[0]", ratio(got["sb"][0], rb["ss"], rb["d_ss"]))
    unchanged(rep, name, "sums[1] untouched", np.array([got["sw"][1], got["sb"][1]]), np.array([9.0, 3.0], F32))
    pmv_check(rep, name, got, {k: (x.reshape(c.R, c.C) if np.ndim(x) else x) for k, x in rw.items()})
    pmv_check(rep, name, got, rb, tag="b")
    all0_check(rep, name, "p", got["p"], c.w)
    all0_check(rep, name, "bp", got["bp"], c.b)
    _images_check(rep, name, got, got["p"], c.H, lay)
    return rw, rb


@pytest.mark.parametrize("H,nin", orf.LSTM_SHAPES)
def test_lstm_adam_fused(H, nin):
    rep = Report("lstm_adam_fused")
    c = orf.lstm_case(H, nin)
    for images in (orf.LSTM_IMAGES if H == 64 else ("bf16", "lohi_l1")):
        got, lay = _lstm_run(c, images, ldT_extra=8 if images in ("bf16", "nseg3") else 0)
        _lstm_check(rep, c, got, lay, "%s %s" % (c.name, images))
    rep.done()


def test_lstm_adam_fused_clips_each_tensor_by_its_own_norm():
    rep = Report("lstm_adam_fused")
    for cw, cb in (("inactive", "active"), ("active", "inactive")):
        c = orf.lstm_case(48, 36, cw, cb)
        got, lay = _lstm_run(c, "bf16")
        rw, rb = _lstm_check(rep, c, got, lay, c.name)
        below, above = (rw, rb) if cw == "inactive" else (rb, rw)
        assert np.sqrt(below["ss"]) < c.hp.clip < np.sqrt(above["ss"])
    rep.done()


@pytest.mark.parametrize("R,C", orf.ADAM2D_SHAPES)
def test_adam2d_fused(R, C):
    rep = Report("adam2d_fused")
    c = orf.adam2d_case(R, C)
    hp = c.hp
    Rp = (R + 63) // 64 * 64
    g = dev(c.w.g)
    ref = orf.fused_ref(c.w, hp, orf.partials_depth(R * C) + 22)
    ref2 = {k: (x.reshape(R, C) if np.ndim(x) else x) for k, x in ref.items()}
    pr, pbnd = orf.partials_ref(c.w.g)
    for images in (False, True):
        ldT = Rp + (8 if images else 0)
        lay = dict(f16=images, fp8=images, nin=C, nseg=1, col0=0, hi_cols=C, hi_tail=False, lo_exp=19, hi_exp=8)

        def run():
            o = Bufs()
            p, m, v = (o.holding(getattr(c.w, a).reshape(R, C)) for a in "pmv")
            part, sw = o.new((1024,)), o.holding(np.array([7.0, 9.0], F32))
            shf, shb = o.new((R, C), BF16), o.new((C, ldT), BF16)
            p16 = o.new((R, C), F16, ld=C + 4) if images else None
            p8 = o.new((R, 2 * C), U8, ld=2 * C + 4) if images else None
            _lib.call("evc_sqnorm2_partials", g.data_ptr(), R * C, None, 0, part.data_ptr(), ops._stream())
            _lib.call("evc_adam2d_fused", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), R, C, part.data_ptr(), sw.data_ptr(), hp.clip, hp.lr, hp.b1, hp.b2,
                      hp.eps, shf.data_ptr(), shb.data_ptr(), ldT, None if p16 is None else p16.data_ptr(), C + 4 if images else 0,
                      None if p8 is None else p8.data_ptr(), 2 * C + 4 if images else 0, C, 19, 8, ops._stream())
            o.finish()
            out = dict(p=host(p), m=host(m), v=host(v), part=host(part), sw=host(sw), p_bf16=host(shf), pT=host(shb))
            if images:
                out.update(p_f16=host(p16), p_fp8=host(p8))
            return out
        got = twice(run)
        name = "%s%s" % (c.name, " images" if images else "")
        rep.add(name, "partials", ratio(got["part"], pr, pbnd))
        rep.add(name, "sums_w[0]", ratio(got["sw"][0], ref["ss"], ref["d_ss"]))
        unchanged(rep, name, "sums_w[1] untouched", got["sw"][1], F32(9.0))
        pmv_check(rep, name, got, ref2)
        all0_check(rep, name, "p", got["p"], c.w)
        _images_check(rep, name, got, got["p"], 0, lay)
    rep.done()


# ---------------------------------------------------------------------------- evc_moe_grad_update, _phase, _apply, _wide
MOE_BEFORE = np.array([0.25, 0.5], F32)


def _moe_bufs(o, c, images, v0=0, v1=None):
    """The weights, moments, shadows and images of rows v0 .. v1 of the matrix."""
    v1 = c.V if v1 is None else v1
    V, K = v1 - v0, c.K
    sl = lambda a: a.reshape(c.V, K)[v0:v1]                              # noqa: E731
    b = dict(p=o.holding(sl(c.w.p)), m=o.holding(sl(c.w.m)), v=o.holding(sl(c.w.v)), pb=o.new((V, K), BF16), pT=o.new((K, V), BF16, ld=V + 8))
    b["wide"] = o.new((V, 2 * K), BF16) if images == "split" else None
    b["f16"] = o.new((V, K), F16) if images == "high" else None
    b["fp8"] = o.new((V, 2 * K), U8) if images == "high" else None
    return b


def _moe_host(b):
    return {k: host(t) for k, t in b.items() if t is not None}


def _moe_images_check(rep, name, got):
    p = got["p"]
    pb = bf16_bits(p)
    rep.add(name, "p_bf16", exact(got["pb"], pb))
    rep.add(name, "pT", exact(got["pT"], np.ascontiguousarray(pb.T)))
    if "wide" in got:
        hi, lo = orf.split_hilo(p)
        rep.add(name, "p_wide [hi | lo]", exact(got["wide"], np.concatenate([hi, lo], axis=1)))
    if "f16" in got:
        K = p.shape[1]
        rep.add(name, "p_f16", exact(_bits(got["f16"]), _bits(orf.f16_of(p))))
        rep.add(name, "p_fp8 [lo | hi]", exact(got["fp8"], orf.fp8_image(p, 0, K, ops.FP8_MOE["w_lo_exp"], ops.FP8_MOE["w_hi_exp"])))


def _moe_selection(i):
    full = [(l2, mode) for l2 in orf.L2S for mode in orf.CLIPS]
    return full if i in (0, 2) else [(2e-8, "active"), (0.5, "inactive"), (0.0, "off")]


@pytest.mark.parametrize("i", range(len(orf.MOE_SHAPES)))
def test_moe_grad_update_both_passes(i):
    """Phase 0: pass 1 + finalize add the norm onto sums, pass 2 reads it; then the same update from evc_moe_grad_update_wide with either image set."""
    rep = Report("moe_grad_update")
    V, K, rows = orf.MOE_SHAPES[i]
    tiles = ((V + 127) // 128) * ((K + 127) // 128)
    for l2, mode in _moe_selection(i):
        c = orf.moe_case(V, K, rows, l2, mode)
        a, x = dev_bf16(c.a), dev_bf16(c.x)
        plain = None
        for images in ((None, "split", "high") if mode == "active" else (None,)):
            def run():
                o = Bufs()
                b = _moe_bufs(o, c, images)
                sums, ws = o.holding(MOE_BEFORE), o.new((2 * tiles,))
                ops.moe_grad_update(a, x, rows, V, K, b["p"], b["m"], b["v"], b["pb"], b["pT"], c.hp.l2, sums, ws, c.hp.clip, c.hp.lr,
                                    p_wide=b["wide"], p_f16=b["f16"], p_fp8=b["fp8"], **c.hp.kw())
                o.finish()
                return dict(_moe_host(b), sums=host(sums), ws=host(ws))
            got = twice(run)
            name = "%s %s" % (c.name, images or "plain")
            nref, nbnd = orf.moe_norm_ref(c.w.p.reshape(V, K), c.hp.l2, c.g64, c.d_g, f64(MOE_BEFORE))
            rep.add(name, "sums", ratio(got["sums"], nref, nbnd))
            part = f64(got["ws"]).reshape(tiles, 2).sum(axis=0) + f64(MOE_BEFORE)
            rep.add(name, "pass 1 partials, summed", ratio(part, nref, nbnd))
            pmv_check(rep, name, got, orf.moe_ref(c, float(got["sums"][0])))
            _moe_images_check(rep, name, got)
            if l2 == 0.0 and V >= 8:
                unchanged(rep, name, "p of an absent class at its first step", got["p"][0], c.w.p.reshape(V, K)[0])
            if images is None:
                plain = got
            else:
                for k in ("p", "m", "v", "pb", "pT", "sums"):
                    assert np.array_equal(_bits(got[k]), _bits(plain[k])), "%s changes with the images written" % k
    rep.done()


@pytest.mark.parametrize("i", (2, 3))
def test_moe_grad_update_phases_over_two_row_slabs(i):
    """A matrix sharded by rows: phase 1 of each slab adds onto the same sums, phase 2 of each slab clips by the norm of the whole matrix."""
    rep = Report("moe_grad_update_phase")
    V, K, rows = orf.MOE_SHAPES[i]
    c = orf.moe_case(V, K, rows, 2e-8, "active")
    cut = 104 if V == 200 else 192
    a, x = dev_bf16(c.a), dev_bf16(c.x)
    slabs = ((0, cut), (cut, V))

    def run():
        o = Bufs()
        sums = o.holding(np.zeros(2, F32))
        bs, wss, mid = [], [], []
        for v0, v1 in slabs:
            bs.append(_moe_bufs(o, c, None, v0, v1))
            wss.append(o.new((2 * ((v1 - v0 + 127) // 128) * ((K + 127) // 128),)))
        for ph in (1, 2):
            for (v0, v1), b, ws in zip(slabs, bs, wss):
                ops.moe_grad_update(a[:, v0:], x, rows, v1 - v0, K, b["p"], b["m"], b["v"], b["pb"], b["pT"], c.hp.l2, sums, ws, c.hp.clip, c.hp.lr,
                                    phase=ph, **c.hp.kw())
                if ph == 1:
                    mid.append(host(sums))
        o.finish()
        out = dict(sums=host(sums), mid0=mid[0], mid1=mid[1])
        for s, b in enumerate(bs):
            out.update({"%s%d" % (k, s): t for k, t in _moe_host(b).items()})
        return out
    got = twice(run)
    before = np.zeros(2)
    p2 = c.w.p.reshape(V, K)
    for s, (v0, v1) in enumerate(slabs):
        nref, nbnd = orf.moe_norm_ref(p2[v0:v1], c.hp.l2, c.g64[v0:v1], c.d_g[v0:v1], before)
        rep.add(c.name, "sums after phase 1 of slab %d" % s, ratio(got["mid%d" % s], nref, nbnd))
        before = f64(got["mid%d" % s])
    assert np.array_equal(got["sums"], got["mid1"])                      # phase 2 reads the norm, it does not touch it
    ref = orf.moe_ref(c, float(got["sums"][0]))
    for s, (v0, v1) in enumerate(slabs):
        g = {k: got["%s%d" % (k, s)] for k in ("p", "m", "v", "pb", "pT")}
        pmv_check(rep, "%s slab %d" % (c.name, s), g, {k: x[v0:v1] if np.ndim(x) else x for k, x in ref.items()})
        _moe_images_check(rep, "%s slab %d" % (c.name, s), g)
    rep.done()


@pytest.mark.parametrize("i", range(len(orf.MOE_SHAPES)))
def test_moe_grad_update_apply(i):
    """The update pass alone from a norm that is given, with each image set, and wsq_out = the sum of the squares of the p it stored."""
    rep = Report("moe_grad_update_apply")
    V, K, rows = orf.MOE_SHAPES[i]
    tiles = ((V + 127) // 128) * ((K + 127) // 128)
    for (l2, mode), images in zip(((2e-8, "active"), (0.5, "inactive"), (0.0, "off")), (None, "split", "high")):
        c = orf.moe_case(V, K, rows, l2, mode)
        a, x = dev_bf16(c.a), dev_bf16(c.x)
        ss32 = float(F32(c.ss))
        sums = dev(np.array([ss32, 0.0], F32))

        def run():
            o = Bufs()
            b = _moe_bufs(o, c, images)
            ws, wsq = o.new((2 * tiles,)), o.new((2,))
            ops.moe_grad_update_apply(a, x, rows, V, K, b["p"], b["m"], b["v"], b["pb"], b["pT"], c.hp.l2, sums, ws, c.hp.clip, c.hp.lr, wsq,
                                      p_wide=b["wide"], p_f16=b["f16"], p_fp8=b["fp8"], **c.hp.kw())
            o.finish()
            return dict(_moe_host(b), ws=host(ws), wsq=host(wsq))
        got = twice(run)
        name = "%s %s" % (c.name, images or "plain")
        pmv_check(rep, name, got, orf.moe_ref(c, ss32))
        _moe_images_check(rep, name, got)
        want, bnd = orf.wsq_ref(got["p"])
        rep.add(name, "wsq_out[0]", ratio(got["wsq"][0], want, bnd))
        rep.add(name, "wsq_out[1]", exact(got["wsq"][1], F32(0.0)))
        rep.add(name, "|W|^2 partials, summed", ratio(f64(got["ws"]).reshape(tiles, 2)[:, 0].sum(), want, bnd))
        assert float(host(sums)[0]) == ss32
    rep.done()


# ---------------------------------------------------------------------------- evc_gram_slabs + evc_moe_grad_norms
@pytest.mark.parametrize("R", orf.GRAM_RS)
def test_gram_route_clip_norm(R):
    """The default route at batch <= 512: evc_moe_grad_update_apply leaves new weights and their |W|^2; the next step's norm comes from the Gram
    matrices of the factors, the forward logits of those weights and that |W|^2 - checked against the materialised float64 gradient."""
    rep = Report("gram_norms")
    V, K = orf.GRAM_V, orf.GRAM_K
    tiles = ((V + 127) // 128) * ((K + 127) // 128)
    for l2 in orf.L2S:
        for with_bias in (False, True):
            c = orf.gram_case(R, l2, with_bias)
            a, x = dev_bf16(c.a), dev_bf16(c.x)
            o = Bufs()
            b = _moe_bufs(o, c, None)
            ws, wsq = o.new((2 * tiles,)), o.new((2,))
            ops.moe_grad_update_apply(a, x, R, V, K, b["p"], b["m"], b["v"], b["pb"], b["pT"], c.hp.l2, dev(np.array([F32(c.ss), 0.0], F32)), ws, c.hp.clip,
                                      c.hp.lr, wsq, **c.hp.kw())
            o.finish()
            wsq32 = float(host(wsq)[0])
            orf.gram_set_weights(c, host(b["p"]))
            c.g64, c.d_g = orf.moe_grad(c)
            logits = dev(np.concatenate([c.logits, np.full((2, V), np.nan, F32)]))[:c.B]         # rows from B on must not be read
            bias = None if c.bias is None else dev(c.bias)
            for SA, SX in orf.GRAM_SLABS:
                def run():
                    o = Bufs()
                    ga, gx = o.new((SA * R * R,)), o.new((SX * R * R,))
                    part, sums = o.new((256 + 4 * c.B,)), o.holding(np.array(orf.GRAM_BEFORE, F32))
                    ops.gram_slabs(a, R, c.ld, SA, ga)
                    ops.gram_slabs(x, R, K, SX, gx)
                    ops.moe_grad_norms(ga, SA, gx, SX, R, a, logits, bias, c.B, V, c.hp.l2, wsq, part, sums)
                    o.finish()
                    return dict(ga=host(ga).reshape(SA, R, R), gx=host(gx).reshape(SX, R, R), sums=host(sums), part=host(part))
                got = twice(run)
                ref, bnd, parts = orf.gram_norm_ref(c, SA, SX, wsq32)
                name = "%s SA=%d SX=%d" % (c.name, SA, SX)
                rep.add(name, "gram_a slabs", ratio(got["ga"], parts["ga"], parts["d_ga"]))
                rep.add(name, "gram_x slabs", ratio(got["gx"], parts["gx"], parts["d_gx"]))
                rep.add(name, "sums", ratio(got["sums"], ref, bnd))
                want = parts["materialised"]
                assert abs(float(got["sums"][0]) - orf.GRAM_BEFORE[0] - want) <= bnd[0] + l2 * l2 * orf.wsq_ref(host(b["p"]))[1], name
    rep.done()


# ---------------------------------------------------------------------------- negative controls: a correct kernel against a reference fed a changed input
def test_negative_control_clip_adam_step_wrong_eps_beta2_and_norm():
    c = orf.step_case(4099, 2e-8, "active")
    got = _step_run(c, 0, False)
    bulk = np.ones(c.p.size, bool)
    for w in c.where.values():
        bulk[w] = False
    for what, ref, k, idx in (("eps = 1e-7", orf.step_ref(c, hp=c.hp.but(eps=1e-7)), "p", c.where["eps_dominates"]),
                              ("beta2 = 0.99", orf.step_ref(c, hp=c.hp.but(b2=0.99)), "v", bulk),
                              ("a norm 1 % larger", orf.step_ref(c, ss32=c.ss32 * 1.01), "m", bulk)):
        q = ratio(got[k], ref[k], ref["d_" + k])
        print("negative control clip_adam_step (%s in the reference): %s worst %.1f, outside on %.3f of the elements named" % (what, k, q.max(), np.mean(q[idx] > 1)))
        assert np.mean(q[idx] > 1.0) > 0.99 and q.max() > 10


def test_negative_control_lstm_adam_fused_the_other_tensors_norm():
    c = orf.lstm_case(48, 36, "inactive", "active")
    got, _ = _lstm_run(c, "bf16")
    Dp, Db = orf.partials_depth(c.R * c.C), orf.partials_depth(c.R, False)
    swap_w = orf.adam_ref(c.w.p, c.w.g, c.w.m, c.w.v, c.hp, *orf.scale_ref(orf.norm64(c.b.g), c.hp.clip, orf.ss_rel(Dp + 22)))
    swap_b = orf.adam_ref(c.b.p, c.b.g, c.b.m, c.b.v, c.hp, *orf.scale_ref(orf.norm64(c.w.g), c.hp.clip, orf.ss_rel(Db)))
    rw = orf.worst(ratio(got["m"].reshape(-1), swap_w["m"], swap_w["d_m"]))
    rb = orf.worst(ratio(got["bm"], swap_b["m"], swap_b["d_m"]))
    print("negative control lstm_adam_fused (each tensor clipped by the other's norm in the reference): m %.1f at %s, bias m %.1f at %s" % (rw + rb))
    assert rw[0] > 10 and rb[0] > 10
    for wrong in (c.hp.but(eps=1e-7), c.hp.but(b2=0.99)):
        ref = orf.fused_ref(c.b, wrong, Db)
        assert max(orf.worst(ratio(got["bp"], ref["p"], ref["d_p"]))[0], orf.worst(ratio(got["bv"], ref["v"], ref["d_v"]))[0]) > 10


def test_negative_control_moe_grad_update_wrong_eps_beta2_and_norm():
    V, K, rows = orf.MOE_SHAPES[2]
    c = orf.moe_case(V, K, rows, 2e-8, "active")
    a, x = dev_bf16(c.a), dev_bf16(c.x)
    ss32 = float(F32(c.ss))
    o = Bufs()
    b = _moe_bufs(o, c, None)
    ws, wsq = o.new((2 * 4,)), o.new((2,))
    ops.moe_grad_update_apply(a, x, rows, V, K, b["p"], b["m"], b["v"], b["pb"], b["pT"], c.hp.l2, dev(np.array([ss32, 0.0], F32)), ws, c.hp.clip, c.hp.lr, wsq,
                              **c.hp.kw())
    o.finish()
    got = _moe_host(b)
    ok = orf.moe_ref(c, ss32)
    assert ratio(got["p"], ok["p"], ok["d_p"]).max() <= 1.0
    for what, ref, k, rowsel in (("eps = 1e-7", orf.moe_ref(c, ss32, hp=c.hp.but(eps=1e-7)), "p", [1]),
                                 ("beta2 = 0.99", orf.moe_ref(c, ss32, hp=c.hp.but(b2=0.99)), "v", np.arange(2, V)),
                                 ("the norm of the weights instead of the gradient's", orf.moe_ref(c, orf.norm64(c.w.p)), "m", np.arange(V) % 7 >= 2)):
        q = ratio(got[k], ref[k], ref["d_" + k])
        print("negative control moe_grad_update_apply (%s in the reference): %s worst %.1f, outside on %.3f of the rows named" % (what, k, q.max(), np.mean(q[rowsel] > 1)))
        assert np.mean(q[rowsel] > 1.0) > 0.9 and q.max() > 10
