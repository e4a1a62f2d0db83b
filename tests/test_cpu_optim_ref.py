"""tests/_optim_ref.py without a GPU: every float64 reference against oracle.model_math (clip_by_norm + adam_step with lr_t passed through,
apply_train_op for the per-tensor clip) to 1e-12, an f32 emulation of every kernel (its operation order, float4 grouping and reduction tree; with and
without the fma contraction of the two-term sums, with correctly rounded and with 1-ulp-off sqrt / rcp) inside every bound on every case, planted
faults outside the bound at the element or regime where each must show, and the sharpness condition per case: the limit on the new p below 1e-3 of
the update and the limit on the new m below 1e-5 of |m_new| + |m_old| on at least 90 % of the elements."""
import functools
import math

import numpy as np

import _optim_ref as orf
from _optim_ref import F32, U, Hyper, bf16_bits, exact, f64, ratio, worst
from oracle import model_math as mm

def hyper64(clip):
    """apply_train_op's own float64 scalars (0.9, 0.999, 1e-8: it takes no others), to hold the reference FUNCTIONS and the per-tensor clip to 1e-12."""
    hp = Hyper(clip=clip)
    hp.b1, hp.b2, hp.eps, hp.omb1, hp.omb2 = 0.9, 0.999, 1e-8, 1.0 - 0.9, 1.0 - 0.999
    return hp


BIG_T = 10 ** 6                                                          # Adam step count at which the oracle's bias correction is exactly 1: lr_t = lr


def oracle_step(p, g, m, v, hp, clip_ss=None):
    """oracle clip_by_norm (from the norm clip_ss when the kernel reads it as an input) + adam_step on float64 copies."""
    p, g, m, v = (f64(a).copy() for a in (p, g, m, v))
    if hp.clip > 0:
        g = mm.clip_by_norm(g, hp.clip) if clip_ss is None else g * (hp.clip / max(math.sqrt(clip_ss), hp.clip))
    assert float(F32(1.0) - F32(hp.b1)) == 1.0 - hp.b1 and float(F32(1.0) - F32(hp.b2)) == 1.0 - hp.b2      # exact f32 differences
    return mm.adam_step(p, g, m, v, BIG_T, hp.lr, beta1=hp.b1, beta2=hp.b2, eps=hp.eps)


def close(a, b, scale=0.0):
    """|a - b| <= 1e-12 max(|b|, scale); scale: the magnitude of the terms where b is a sum that cancels."""
    a, b = f64(a), f64(b)
    return bool(np.all(np.abs(a - b) <= 1e-12 * np.maximum(np.abs(b), scale) + 1e-290))


def close3(ref, want, p_old, m_old, g):
    """p, m, v of a reference against the oracle's; m = b1 m + (1 - b1) gc and p - step cancel, so they are held to 1e-12 of |m_old| + |g| (|gc| <= |g|)
    and of |p_old|."""
    sh = np.shape(ref["p"])
    return (close(ref["p"], want[0], np.abs(f64(p_old)).reshape(sh)) and close(ref["m"], want[1], np.abs(f64(m_old)).reshape(sh) + np.abs(f64(g)).reshape(sh))
            and close(ref["v"], want[2]))


def inside(name, got, ref, keys="pmv"):
    for i, k in enumerate(keys):
        r, at = worst(ratio(got[i], ref[k], ref["d_" + k]))
        assert r <= 1.0, "%s %s: %.4f at %s" % (name, k, r, at)


def sharp(name, ref, p_old, m_old):
    sp, sm = orf.sharpness(ref, p_old, m_old)
    assert sp >= 0.9 and sm >= 0.9, "%s: sharpness p %.3f m %.3f" % (name, sp, sm)


VARIANTS = [(fma, ulp) for fma in (False, True) for ulp in (0, 1)]


def step_cases():
    for n in orf.STEP_NS[:3]:
        for l2 in orf.L2S:
            for mode in orf.CLIPS:
                yield orf.step_case(n, l2, mode)
        yield orf.step_case(n, 2e-8, "active", odd=True)
    for l2, mode in orf.STEP_BIG:
        yield orf.step_case(orf.STEP_NS[3], l2, mode)


# ---------------------------------------------------------------------------- references against the oracle
def test_references_equal_the_oracle():
    for c in list(step_cases())[:31]:
        ref = orf.step_ref(c)
        g = f64(c.g) + c.hp.l2 * f64(c.p)
        assert close(c.ss32, np.sum(g * g)) or abs(c.ss32 - np.sum(g * g)) <= U * c.ss32
        want = oracle_step(c.p, g, c.m, c.v, c.hp, clip_ss=c.ss32)
        assert close3(ref, want, c.p, c.m, g), c.name
        own = orf.adam_ref(c.p, c.g, c.m, c.v, c.hp, *orf.scale_ref(orf.norm64(c.g, c.p, c.hp.l2), c.hp.clip))
        want = oracle_step(c.p, g, c.m, c.v, c.hp)                       # and with the oracle's own norm
        assert close3(own, want, c.p, c.m, g), c.name


def test_per_tensor_references_equal_apply_train_op():
    cs, hp = orf.small_cases()
    hp = hyper64(hp.clip)
    params = {c.name: f64(c.p) for c in cs}
    slots = {c.name: (f64(c.m).copy(), f64(c.v).copy()) for c in cs}
    new = mm.apply_train_op(params, {c.name: f64(c.g) for c in cs}, slots, BIG_T, hp.lr, clip_norm=hp.clip)
    below = above = 0
    for c in cs:
        ref = orf.small_ref(c, hp)
        assert close3(ref, (new[c.name],) + slots[c.name], c.p, c.m, c.g), c.name
        below += math.sqrt(ref["ss"]) < hp.clip
        above += math.sqrt(ref["ss"]) > hp.clip
    assert below >= 7 and above >= 7
    c = orf.lstm_case(48, 36, "inactive", "active")
    params = {"w": f64(c.w.p), "b": f64(c.b.p)}
    slots = {"w": (f64(c.w.m).copy(), f64(c.w.v).copy()), "b": (f64(c.b.m).copy(), f64(c.b.v).copy())}
    new = mm.apply_train_op(params, {"w": f64(c.w.g), "b": f64(c.b.g)}, slots, BIG_T, c.hp.lr, clip_norm=c.hp.clip)
    for k, t in (("w", c.w), ("b", c.b)):
        ref = orf.fused_ref(t, hyper64(c.hp.clip), 40)
        assert close3(ref, (new[k],) + slots[k], t.p, t.m, t.g), k
    assert math.sqrt(orf.norm64(c.w.g)) < c.hp.clip < math.sqrt(orf.norm64(c.b.g))


def test_moe_reference_equals_the_oracle_on_the_materialised_gradient():
    for shape in orf.MOE_SHAPES[:3]:
        c = orf.moe_case(*shape, 0.5, "active")
        a, x = orf.bf16_to_f64(c.a)[:, :c.V], orf.bf16_to_f64(c.x)
        g = sum(np.outer(a[r], x[r]) for r in range(c.rows)) + c.hp.l2 * f64(c.w.p).reshape(c.V, c.K)
        assert close(c.ss, np.sum(g * g))
        sums, _ = orf.moe_norm_ref(c.w.p.reshape(c.V, c.K), c.hp.l2, c.g64, c.d_g, (3.0, 5.0))
        assert close(sums[0] - 3.0, np.sum(g * g)) and close(sums[1] - 5.0, np.sum(f64(c.w.p) ** 2))
        ss32 = float(F32(c.ss))
        ref = orf.moe_ref(c, ss32)
        want = oracle_step(c.w.p.reshape(c.V, c.K), g, c.w.m.reshape(c.V, c.K), c.w.v.reshape(c.V, c.K), c.hp, clip_ss=ss32)
        assert close3(ref, want, c.w.p, c.w.m, g), c.name


def test_norm_references_equal_plain_sums():
    rng = np.random.default_rng(1)
    g, p = rng.standard_normal(1027).astype(F32), rng.standard_normal(1027).astype(F32)
    l2 = float(F32(0.5))
    s, _ = orf.sqnorm_ref(g, p, l2, (2.0, 3.0))
    assert close(s[0], 2.0 + np.sum((f64(g) + l2 * f64(p)) ** 2)) and close(s[1], 3.0 + np.sum(f64(p) ** 2))
    s, b = orf.sqnorm_ref(g, None, 0.0, (2.0, 3.0))
    assert close(s[0], 2.0 + np.sum(f64(g) ** 2)) and s[1] == 3.0 and b[1] == 0.0
    part, _ = orf.partials_ref(g, p[:64])
    assert close(part[:1024].sum(), np.sum(f64(g) ** 2)) and close(part[1024], np.sum(f64(p[:64]) ** 2)) and (part[5:1024] == 0).all()


def test_depths_are_the_ones_the_docstring_lists():
    assert [orf.sqnorm_depth(n) for n in orf.SQNORM_NS] == [12, 12, 16, 271, 535]
    assert [orf.partials_depth(n) for n in (4, 1027, 3153923)] == [15, 15, 27] and [orf.partials_depth(n, False) for n in (64, 4096)] == [15, 27]
    assert orf.small_depth(32768) == 54 and orf.MOE_DEPTH == 70
    assert orf.partials_depth(1024 * 3080) + 22 == 49


# ---------------------------------------------------------------------------- emulations inside every bound, sharpness
def test_clip_adam_step_emulation_stays_inside_and_the_bound_is_sharp():
    for c in step_cases():
        ref = orf.step_ref(c)
        s32 = orf.scale_emul(c.ss32, c.hp.clip)
        if "inactive" in c.name or "off" in c.name:
            assert s32 == 1.0
        for fma, ulp in (VARIANTS if c.p.size < 10 ** 6 else VARIANTS[::3]):
            inside(c.name + " fma=%d ulp=%d" % (fma, ulp), orf.adam_emul(c.p, c.g, c.m, c.v, c.hp, s32, fma, ulp), ref)
        sharp(c.name, ref, c.p, c.m)
        if c.hp.l2 == 0.0 and c.where["all0"].size:                     # g = m = v = 0: p comes back bit for bit
            i = c.where["all0"]
            pn = orf.adam_emul(c.p, c.g, c.m, c.v, c.hp, s32)[0]
            assert np.array_equal(pn[i].view(np.uint32), c.p[i].view(np.uint32)) and np.array_equal(ref["p"][i], f64(c.p[i]))


def test_every_large_case_holds_every_regime_in_the_first_a_middle_and_the_last_tile():
    c = orf.step_case(4099, 0.0, "active")
    for kind in orf.REGIMES:
        w = c.where[kind]
        assert w.size == 18 and w.min() < 64 and w.max() >= 4099 - 36 and ((w > 1024) & (w < 3072)).any(), kind
    assert c.where["v_large"].max() == 4098 and len({int(i) % 4 for i in c.where["all0"]}) == 4
    assert (c.m[c.where["first_step"]] == 0).all() and (c.g[c.where["g0"]] == 0).all() and (c.m[c.where["g0"]] != 0).all()
    assert (np.abs(c.g[c.where["underflow"]]) < 3e-20).all() and (c.v[c.where["v_large"]] > 1e3).all() and np.abs(c.p).max() <= 0.3


def test_grad_sqnorm_emulation_stays_inside():
    for n in orf.SQNORM_NS:
        c = orf.bulk(n, 9000 + n % 1000)
        for p, l2 in ((None, 0.0), (c.p, 2e-8), (c.p, 0.5)):
            l2 = float(F32(l2))
            before = (float(F32(0.37)), float(F32(1.5)))
            ref, bnd = orf.sqnorm_ref(c.g, p, l2, before)
            grid = orf.sqnorm_grid(n)
            for order in (None, list(range(grid))[::-1]):
                got = orf.sqnorm_emul(c.g, p, l2, before, order)
                q = ratio(got, ref, bnd)
                assert q.max() <= 1.0, (n, l2, q)
                if p is None:
                    assert got[1] == F32(before[1])
            assert bnd[0] < 1e-4 * ref[0]                               # the depth-based bound: far below the 1e-3 the older tests allow


def test_sqnorm2_partials_emulation_stays_inside_per_partial():
    for na, nb in orf.PARTIALS_NS:
        a = orf.bulk(na, 9050).g
        b = None if nb is None else orf.bulk(nb, 9051).g
        ref, bnd = orf.partials_ref(a, b)
        got = orf.partials_emul(a, b)
        assert got.size == ref.size == (1024 if b is None else 1025)
        assert ratio(got, ref, bnd).max() <= 1.0, (na, nb)
        own = np.bincount(orf.partials_owner(na), minlength=1024)
        assert (got[:1024][own == 0] == 0).all() and (ref[:1024][own == 0] == 0).all()
        if na == 4:
            assert (own > 0).sum() == 1
        if na == 3153923:
            assert own[0] == 4 * 1024 + 3 and own[7] == 4 * 1024 and own[8] == 3 * 1024 == own.min()       # 788480 float4 = 3 x 262144 + 8 x 256: both loops, a 3-element tail


def test_clip_adam_small_emulation_stays_inside_and_the_bound_is_sharp():
    cs, hp = orf.small_cases()
    for c in cs:
        ref = orf.small_ref(c, hp)
        ss32 = orf.small_sum_emul(c.g)
        assert ratio(ss32, ref["ss"], ref["d_ss"]).max() <= 1.0, c.name
        s32 = orf.scale_emul(ss32, hp.clip)
        for fma, ulp in VARIANTS:
            got = orf.adam_emul(c.p, c.g, c.m, c.v, hp, s32, fma, ulp, g_l2=False)
            assert np.isfinite(got[0]).all()
            inside(c.name, got, ref)
        sharp(c.name, ref, c.p, c.m)
    z = cs[orf.SMALL_ZERO_G]
    assert orf.small_ref(z, hp)["ss"] == 0.0 and orf.scale_ref(0.0, hp.clip) == (1.0, 0.0)


def _fused_emul(c, t, bias, fma, ulp, part):
    ss32 = part[1024] if bias else orf.sum_partials_emul(part[:1024])
    return ss32, orf.adam_emul(t.p, t.g, t.m, t.v, c.hp, orf.scale_emul(ss32, c.hp.clip), fma, ulp, g_l2=False)


def lstm_cases():
    for H, nin in orf.LSTM_SHAPES:
        yield orf.lstm_case(H, nin)
    yield orf.lstm_case(48, 36, "inactive", "active")
    yield orf.lstm_case(48, 36, "active", "inactive")


def test_lstm_adam_fused_emulation_stays_inside_and_the_bound_is_sharp():
    for c in lstm_cases():
        part = orf.partials_emul(c.w.g, c.b.g)
        Dp, Db = orf.partials_depth(c.w.p.size), orf.partials_depth(c.b.p.size, False)
        for t, bias, D in ((c.w, False, Dp + 22), (c.b, True, Db)):
            ref = orf.fused_ref(t, c.hp, D)
            for fma, ulp in VARIANTS:
                ss32, got = _fused_emul(c, t, bias, fma, ulp, part)
                assert ratio(ss32, ref["ss"], ref["d_ss"]).max() <= 1.0
                inside(c.name + (" bias" if bias else " kernel"), got, ref)
            sharp(c.name, ref, t.p, t.m)


def test_adam2d_fused_emulation_stays_inside_and_the_bound_is_sharp():
    for R, C in orf.ADAM2D_SHAPES:
        c = orf.adam2d_case(R, C)
        ref = orf.fused_ref(c.w, c.hp, orf.partials_depth(R * C) + 22)
        part = orf.partials_emul(c.w.g)
        for fma, ulp in (VARIANTS if R * C < 10 ** 6 else VARIANTS[::3]):
            ss32, got = _fused_emul(c, c.w, False, fma, ulp, part)
            assert ratio(ss32, ref["ss"], ref["d_ss"]).max() <= 1.0
            inside(c.name, got, ref)
        sharp(c.name, ref, c.w.p, c.w.m)


def _moe_g32(c, r0=0, r1=None, reverse=False):
    """The tile as an f32 accumulation over the rows in turn (every product of two bf16 numbers is exact in f32)."""
    a, x = orf.bf16_to_f64(c.a)[r0:r1, :c.V].astype(F32), orf.bf16_to_f64(c.x)[r0:r1].astype(F32)
    g = np.zeros((c.V, c.K), F32)
    for r in (range(a.shape[0])[::-1] if reverse else range(a.shape[0])):
        g = (g + np.outer(a[r], x[r]).astype(F32)).astype(F32)
    return g


def _moe_sum_emul(sq32, V, K, before):
    """Per 128 x 128 tile: 32 terms a thread in turn, 512 threads = 8 waves; the tile partials through the 1024-thread finish, added onto `before`
    (the assignment of elements to threads is not the MFMA layout; the depth of the tree is the kernel's)."""
    parts = []
    for v0 in range(0, V, 128):
        for k0 in range(0, K, 128):
            t = np.zeros((128, 128), F32)
            blk = sq32[v0:v0 + 128, k0:k0 + 128]
            t[:blk.shape[0], :blk.shape[1]] = blk
            parts.append(orf._block_sum(orf._strided_sum(t.reshape(-1), np.zeros(0, F32), 1, 512)[0][None, :])[0])
    fin = np.zeros(1024, F32)
    fin[:len(parts)] = parts
    return F32(F32(before) + orf._block_sum(fin[None, :])[0])


def moe_cases():
    for i, shape in enumerate(orf.MOE_SHAPES):
        for l2 in orf.L2S:
            for mode in orf.CLIPS:
                if i in (0, 2) or (l2, mode) in ((2e-8, "active"), (0.5, "inactive"), (0.0, "off")):
                    yield orf.moe_case(*shape, l2, mode)


def test_moe_update_emulation_stays_inside_and_the_bound_is_sharp():
    for c in moe_cases():
        p = c.w.p.reshape(c.V, c.K)
        for reverse in (False, True):
            g32 = _moe_g32(c, reverse=reverse)
            assert ratio(g32, c.g64, c.d_g).max() <= 1.0
            w32 = (g32 + (F32(c.hp.l2) * p).astype(F32)).astype(F32)
            sums, bnd = orf.moe_norm_ref(p, c.hp.l2, c.g64, c.d_g, (0.25, 0.5))
            got = [_moe_sum_emul((w32 * w32).astype(F32), c.V, c.K, 0.25), _moe_sum_emul((p * p).astype(F32), c.V, c.K, 0.5)]
            assert ratio(np.array(got), sums, bnd).max() <= 1.0, c.name
            ss32 = float(F32(c.ss))
            ref = orf.moe_ref(c, ss32)
            s32 = orf.scale_emul(ss32, c.hp.clip)
            for fma, ulp in VARIANTS[::3]:
                got = orf.adam_emul(p, g32, c.w.m.reshape(c.V, c.K), c.w.v.reshape(c.V, c.K), c.hp, s32, fma, ulp)
                inside(c.name, got, ref)
                wsq, d_wsq = orf.wsq_ref(got[0])
                assert abs(float(_moe_sum_emul((got[0] * got[0]).astype(F32), c.V, c.K, 0.0)) - wsq) <= d_wsq
        sharp(c.name, ref, c.w.p, c.w.m)
        if c.V >= 8:
            assert (c.g64[::7] == 0).all() and (c.d_g[::7] == 0).all() and 0 < np.abs(c.g64[1::7]).max() < 1e-7


def gram_cases():
    for R in orf.GRAM_RS:
        for l2 in orf.L2S:
            for with_bias in (False, True):
                yield orf.gram_case(R, l2, with_bias)


def test_gram_route_norm_equals_the_materialised_gradient_and_its_emulation_stays_inside():
    for c in gram_cases():
        w = f64(c.w.p).reshape(c.V, c.K)
        wsq32 = float(F32(np.sum(w * w)))
        assert (orf.bf16_to_f64(c.a)[c.B:] == 0).all() and (orf.bf16_to_f64(c.a)[:, c.V:] == 0).all() and c.logits.shape == (c.B, c.V)
        for SA, SX in orf.GRAM_SLABS:
            ref, bnd, parts = orf.gram_norm_ref(c, SA, SX, wsq32, (0.0, 0.0))
            mat = parts["materialised"] - c.hp.l2 ** 2 * (float(np.sum(w * w)) - wsq32)        # the materialised norm with the |W|^2 that is given
            assert abs(ref[0] - mat) <= 1e-12 * mat, c.name
            g = orf.bf16_to_f64(c.a)[:, :c.V].T @ orf.bf16_to_f64(c.x)                           # and the Gram identities themselves, in float64
            assert abs(np.sum(parts["ga"].sum(axis=0) * parts["gx"].sum(axis=0)) - np.sum(g * g)) <= 1e-12 * np.sum(g * g)
            bias = 0.0 if c.bias is None else f64(c.bias)
            assert abs(np.sum(orf.bf16_to_f64(c.a)[:c.B, :c.V] * (c.logits64 - bias)) - np.sum(g * w)) <= 1e-12 * np.sum(np.abs(g * w))
            ref, bnd, parts = orf.gram_norm_ref(c, SA, SX, wsq32)
            ga, gx, sums = orf.gram_emul(c, SA, SX, wsq32)
            assert ratio(ga, parts["ga"], parts["d_ga"]).max() <= 1.0 and ratio(gx, parts["gx"], parts["d_gx"]).max() <= 1.0, c.name
            assert ratio(sums, ref, bnd).max() <= 1.0, (c.name, ratio(sums, ref, bnd))
            assert bnd[0] < 1e-4 * ref[0]                               # absolute, and still four digits of the norm
    assert [len(set(k1 - k0 for k0, k1 in orf.gram_slab_ranges(256, S))) for S in (3, 4)] == [2, 1]      # 3 + 3 + 2 k steps / 4 x 2


def test_fault_cross_term_dropped_from_the_gram_norm():
    c = orf.gram_case(96, 0.5, True)
    wsq32 = float(F32(orf.norm64(c.w.p)))
    ref, bnd, parts = orf.gram_norm_ref(c, 3, 3, wsq32)
    bad, _, _ = orf.gram_norm_ref(c, 3, 3, wsq32, drop_cross=True)
    assert abs(bad[0] - ref[0]) > 10 * bnd[0] and abs(parts["cross"]) > 10 * bnd[0]        # at l2 = 0.5; at 2e-8 the term is below the f32 cast of the total
    c = orf.gram_case(96, 2e-8, True)
    ref, bnd, parts = orf.gram_norm_ref(c, 3, 3, wsq32)
    assert abs(parts["cross"]) < bnd[0]


# ---------------------------------------------------------------------------- images
def test_e4m3_cast_and_the_image_layouts():
    assert orf.e4m3_bytes(np.array([0.3, 500.0, -1e-3, 17.3], F32)).tolist() == [42, 126, 129, 89]
    p = (np.arange(4 * 12, dtype=F32).reshape(4, 12) - 20.0) * F32(0.0123)
    w = orf.f16_wide(p, 8, 3)
    assert w.shape == (4, 28) and np.array_equal(w[:, :8], p[:, :8].astype(np.float16)) and np.array_equal(w[:, 24:], p[:, 8:].astype(np.float16))
    assert np.array_equal(w[:, 8:16].astype(F32) * 64, w[:, :8].astype(F32))
    rest = f64(p[:, :8]) - f64(w[:, :8])
    assert np.abs(f64(w[:, 16:24]) / 64 - rest).max() <= 2.0 ** -11 * np.abs(rest).max() and np.abs(rest).max() > 0
    img = orf.fp8_image(p, 4, 4, 17, 6, hi_tail=True)
    assert img.shape == (4, 16) and np.array_equal(img[:, 4:8], orf.e4m3_bytes(p[:, 4:8] * 64)) and np.array_equal(img[:, 12:], orf.e4m3_bytes(p[:, 8:] * 64))
    assert orf.fp8_image(p, 4, 4, 17, 6).shape == (4, 12)
    bits = np.arange(8 * 3, dtype=np.uint16).reshape(8, 3)               # H = 2: row g * 2 + u
    t = orf.lstm_transposed(bits, 2)
    assert t.shape == (3, 8) and all(t[k, u * 4 + g] == bits[g * 2 + u, k] for k in range(3) for u in range(2) for g in range(4))
    hi, lo = orf.split_hilo(p)
    assert np.abs(orf.bf16_to_f64(hi) + orf.bf16_to_f64(lo) - f64(p)).max() <= 2.0 ** -16 * np.abs(p).max()


# ---------------------------------------------------------------------------- planted faults
@functools.lru_cache(maxsize=None)
def _fc(l2=2e-8, mode="active"):
    c = orf.step_case(4099, l2, mode)
    return c, orf.step_ref(c), orf.scale_emul(c.ss32, c.hp.clip)


def _chain(c, s32, eps_inside=False, eps_dropped=False, v_unclipped=False, old_m=False):
    """adam_emul's chain with a fault planted."""
    hp = c.hp
    l2, s, b1, b2, omb1, omb2, eps, lr = (F32(x) for x in (hp.l2, s32, hp.b1, hp.b2, hp.omb1, hp.omb2, hp.eps, hp.lr))
    a = (c.g + (l2 * c.p).astype(F32)).astype(F32)
    gc = (a * s).astype(F32)
    gv = a if v_unclipped else gc
    with np.errstate(under="ignore", invalid="ignore", divide="ignore"):
        mn = ((b1 * c.m).astype(F32) + (omb1 * gc).astype(F32)).astype(F32)
        vn = ((b2 * c.v).astype(F32) + ((omb2 * gv).astype(F32) * gv).astype(F32)).astype(F32)
        den = np.sqrt((vn + eps).astype(F32)) if eps_inside else np.sqrt(vn) if eps_dropped else (np.sqrt(vn) + eps).astype(F32)
        pn = (c.p - ((lr * (c.m if old_m else mn)).astype(F32) * (F32(1.0) / den).astype(F32)).astype(F32)).astype(F32)
    return pn, mn, vn


def _out(got, ref, k, idx=None):
    """The share of the elements idx (all) of output k outside the bound."""
    q = ratio(got, ref[k], ref["d_" + k]).reshape(-1)
    return float(np.mean((q if idx is None else q[idx]) > 1.0))


def _bulk_idx(c):
    m = np.ones(c.p.size, bool)
    for w in c.where.values():
        m[w] = False
    return np.nonzero(m)[0]


def test_fault_eps_inside_the_square_root():
    c, ref, s32 = _fc()
    got = _chain(c, s32, eps_inside=True)
    assert _out(got[0], ref, "p", c.where["eps_dominates"]) == 1.0      # den = 1e-4 instead of 1e-8
    assert _out(got[0], ref, "p", c.where["first_step"]) == 1.0 and _out(got[0], ref, "p", _bulk_idx(c)) > 0.9
    assert _out(got[1], ref, "m") == 0.0 and _out(got[2], ref, "v") == 0.0


def test_fault_eps_dropped():
    c, ref, s32 = _fc()
    got = _chain(c, s32, eps_dropped=True)
    assert _out(got[0], ref, "p", c.where["eps_dominates"]) == 1.0 and _out(got[0], ref, "p", c.where["all0"]) == 1.0      # 0 / 0 = NaN
    assert _out(got[0], ref, "p", _bulk_idx(c)) > 0.1                   # 1e-8 against sqrt(v) ~ 3e-3 is 3e-6 of the update: visible where |p| is small


def test_fault_beta2_of_099():
    c, ref, s32 = _fc()
    got = orf.adam_emul(c.p, c.g, c.m, c.v, c.hp.but(b2=0.99), s32)
    assert _out(got[2], ref, "v", _bulk_idx(c)) == 1.0 and _out(got[0], ref, "p", _bulk_idx(c)) > 0.99 and _out(got[1], ref, "m") == 0.0


def test_fault_bias_correction_applied_twice():
    c, ref, s32 = _fc()
    t = 10
    got = orf.adam_emul(c.p, c.g, c.m, c.v, c.hp.but(lr=c.hp.lr * math.sqrt(1 - c.hp.b2 ** t) / (1 - c.hp.b1 ** t)), s32)
    assert _out(got[0], ref, "p", _bulk_idx(c)) > 0.99 and _out(got[1], ref, "m") == 0.0 and _out(got[2], ref, "v") == 0.0


def test_fault_clip_applied_although_the_norm_is_below_it():
    c, ref, s32 = _fc(mode="inactive")
    assert s32 == 1.0
    got = orf.adam_emul(c.p, c.g, c.m, c.v, c.hp, F32(c.hp.clip) / np.sqrt(F32(c.ss32)))     # g * clip / norm: a scale of 2
    assert _out(got[1], ref, "m", _bulk_idx(c)) > 0.99 and _out(got[2], ref, "v", _bulk_idx(c)) > 0.99


def test_fault_the_other_tensors_norm():
    c = orf.lstm_case(48, 36, "inactive", "active")
    part = orf.partials_emul(c.w.g, c.b.g)
    ss_w, ss_b = orf.sum_partials_emul(part[:1024]), part[1024]
    ref_w = orf.fused_ref(c.w, c.hp, orf.partials_depth(c.w.p.size) + 22)
    ref_b = orf.fused_ref(c.b, c.hp, orf.partials_depth(c.b.p.size, False))
    got = orf.adam_emul(c.w.p, c.w.g, c.w.m, c.w.v, c.hp, orf.scale_emul(ss_b, c.hp.clip))        # the bias's norm for the kernel matrix
    assert _out(got[1], ref_w, "m", _bulk_idx(c.w)) > 0.99 and _out(got[0], ref_w, "p", _bulk_idx(c.w)) > 0.9
    got = orf.adam_emul(c.b.p, c.b.g, c.b.m, c.b.v, c.hp, orf.scale_emul(ss_w, c.hp.clip))        # and the reverse
    assert _out(got[1], ref_b, "m", _bulk_idx(c.b)) > 0.99 and _out(got[0], ref_b, "p", _bulk_idx(c.b)) > 0.9


def test_fault_l2_left_out_of_the_gradient_term():
    c, ref, s32 = _fc(l2=0.5)
    got = orf.adam_emul(c.p, c.g, c.m, c.v, c.hp, s32, g_l2=False)
    assert _out(got[1], ref, "m", _bulk_idx(c)) > 0.99 and _out(got[1], ref, "m", c.where["g0"]) == 1.0      # there l2 p is the whole gradient


def test_fault_l2_left_out_of_the_norm_only():
    c, ref, _ = _fc(l2=0.5)
    s32 = orf.scale_emul(F32(orf.norm64(c.g)), c.hp.clip)
    got = orf.adam_emul(c.p, c.g, c.m, c.v, c.hp, s32)
    assert _out(got[1], ref, "m", _bulk_idx(c)) > 0.99 and _out(got[2], ref, "v", _bulk_idx(c)) > 0.99
    n, b = orf.sqnorm_ref(c.g, c.p, c.hp.l2)
    assert abs(orf.sqnorm_emul(c.g, None, 0.0)[0] - n[0]) > b[0]         # and the norm entry's own check sees it


def test_fault_v_from_the_unclipped_gradient():
    c, ref, s32 = _fc()
    got = _chain(c, s32, v_unclipped=True)
    assert _out(got[2], ref, "v", _bulk_idx(c)) > 0.99 and _out(got[1], ref, "m") == 0.0
    assert _out(got[2], ref, "v", c.where["g0"]) == 0.0                 # (l2 p)^2 ~ 1e-18 against v ~ 1e-5


def test_fault_p_stepped_with_the_old_m():
    c, ref, s32 = _fc(l2=0.0)
    got = _chain(c, s32, old_m=True)
    assert _out(got[0], ref, "p", _bulk_idx(c)) > 0.99 and _out(got[0], ref, "p", c.where["first_step"]) == 1.0
    assert _out(got[0], ref, "p", c.where["all0"]) == 0.0 and _out(got[1], ref, "m") == 0.0


def _lstm_got(c, t, bias):
    part = orf.partials_emul(c.w.g, c.b.g)
    return _fused_emul(c, t, bias, False, 0, part)[1]


def test_fault_one_float4_of_the_ragged_last_column_tile_not_updated():
    c = orf.lstm_case(16, 4)                                             # C = 20: columns 16 .. 19 are the only live float4 of the last lanes
    ref = orf.fused_ref(c.w, c.hp, orf.partials_depth(c.w.p.size) + 22)
    got = [a.reshape(c.R, c.C).copy() for a in _lstm_got(c, c.w, False)]
    r = 37
    for a, old in zip(got, (c.w.p, c.w.m, c.w.v)):
        a[r, 16:20] = old.reshape(c.R, c.C)[r, 16:20]
    for i, k in enumerate("pmv"):
        q = ratio(got[i], ref[k].reshape(c.R, c.C), ref["d_" + k].reshape(c.R, c.C))
        assert (q[r, 16:20] > 1.0).all() and (np.delete(q, r, axis=0) <= 1.0).all() and (q[r, :16] <= 1.0).all(), k


def test_fault_the_last_bias_block_skipped():
    c = orf.lstm_case(272, 16)                                           # R = 1088: elements 1024 .. 1087 are the second bias block
    ref = orf.fused_ref(c.b, c.hp, orf.partials_depth(c.b.p.size, False))
    got = [a.copy() for a in _lstm_got(c, c.b, True)]
    for a, old in zip(got, (c.b.p, c.b.m, c.b.v)):
        a[1024:] = old[1024:]
    for i, k in enumerate("pmv"):
        q = ratio(got[i], ref[k], ref["d_" + k])
        assert (q[:1024] <= 1.0).all() and np.mean(q[1024:] > 1.0) > 0.8, k
    assert c.b.where["v_large"].max() == 1087


def test_fault_a_shadow_taken_from_the_old_weights():
    c, ref, s32 = _fc()
    pn = orf.adam_emul(c.p, c.g, c.m, c.v, c.hp, s32)[0]
    assert np.isinf(exact(bf16_bits(c.p), bf16_bits(pn))).mean() > 0.2  # an update of 1e-4 against a bf16 spacing of 2.4e-4 at 0.05
    assert np.isinf(exact(orf.f16_of(c.p), orf.f16_of(pn))).mean() > 0.9


def test_fault_gate_interleave_swapped_for_one_tile():
    c = orf.lstm_case(48, 36)
    bits = bf16_bits(_lstm_got(c, c.w, False)[0]).reshape(c.R, c.C)
    want = orf.lstm_transposed(bits, c.H)
    bad = want.copy()
    tile = bits.reshape(4, c.H, c.C)[:, 16:32, :]                        # the units 16 .. 31: written as g * 16 + u instead of u * 4 + g
    bad[:, 64:128] = tile.transpose(2, 0, 1).reshape(c.C, 64)
    q = exact(bad, want)
    assert np.isinf(q[:, 64:128]).mean() > 0.8 and (q[:, :64] == 0).all() and (q[:, 128:] == 0).all()
    assert (q[:, 64] == 0).all() and (q[:, 127] == 0).all()             # (u, g) = (0, 0) and (15, 3) map to themselves under the swap


def test_fault_the_lo_image_scaled_by_the_wrong_power_of_two():
    c = orf.lstm_case(64, 64)
    p = _lstm_got(c, c.w, False)[0].reshape(c.R, c.C)
    good, bad = orf.fp8_image(p, 0, 64, 17, 6), orf.fp8_image(p, 0, 64, 16, 6)
    q = exact(bad, good)
    assert np.isinf(q[:, :64]).mean() > 0.9 and np.isinf(q[:, 128:]).mean() > 0.9 and (q[:, 64:128] == 0).all()     # the hi block is untouched
    w3, b3 = orf.f16_wide(p, 64, 3), orf.f16_wide(p, 64, 3)
    b3[:, 128:192] = (b3[:, 128:192].astype(F32) * 2).astype(np.float16)                  # (p - f16(p)) * 128
    assert np.isinf(exact(b3, w3)[:, 128:192]).mean() > 0.9
    hi, lo = orf.split_hilo(p)
    assert np.isinf(exact(bf16_bits(orf.bf16_to_f64(lo) * 2), lo)).mean() > 0.9


def test_fault_the_scalar_tail_skipped_and_a_partial_owned_by_the_wrong_block():
    c, ref, s32 = _fc()
    got = [a.copy() for a in orf.adam_emul(c.p, c.g, c.m, c.v, c.hp, s32)]
    got[2][4096:] = c.v[4096:]                                           # n = 4099: the three elements behind the float4 body
    assert (ratio(got[2], ref["v"], ref["d_v"])[4096:] > 1.0).all()
    a = orf.bulk(3153923, 9050).g
    pr, bnd = orf.partials_ref(a)
    n4 = a.size // 4
    wrong = np.bincount(np.arange(n4) % 1024, weights=(f64(a[:n4 * 4]) ** 2).reshape(-1, 4).sum(axis=1), minlength=1024)     # i % 1024 instead of (i / 256) % 1024
    assert np.mean(np.abs(wrong - pr) > bnd) > 0.99


def test_fault_moe_tile_from_half_the_rows_and_a_rare_class_column_dropped():
    c = orf.moe_case(200, 192, 32, 2e-8, "active")
    ss32 = float(F32(c.ss))
    ref = orf.moe_ref(c, ss32)
    p, m, v = (a.reshape(c.V, c.K) for a in (c.w.p, c.w.m, c.w.v))
    s32 = orf.scale_emul(ss32, c.hp.clip)
    got = orf.adam_emul(p, _moe_g32(c, 0, 16), m, v, c.hp, s32)         # one K step of the TN loop lost
    q = ratio(got[1], ref["m"], ref["d_m"])
    generic = np.arange(c.V) % 7 >= 2
    assert (q[::7] <= 1.0).all() and np.mean(q[generic] > 1.0) > 0.99   # absent classes: nothing to lose
    g = _moe_g32(c)
    g[1::7] = 0.0                                                        # a rare class (|dlogits| ~ 1e-9) treated as absent
    got = orf.adam_emul(p, g, m, v, c.hp, s32)
    q = ratio(got[1], ref["m"], ref["d_m"])
    assert np.mean(q[1] > 1.0) > 0.99 and (q[np.arange(c.V) % 7 != 1] <= 1.0).all()      # row 1: the class's first step, nothing else in m
