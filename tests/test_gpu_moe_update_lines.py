"""The row-major epilogue of the fused MoE update (moe_update_kernel, pass 2): the gradient tile changes layout through LDS, p, m, v and every
image of the new weights move as whole rows of the tile.  Small shapes where that path can go wrong: one exact tile, 2 x 2 tiles and 4 x 3
tiles with ragged last tiles in both directions.  pytest -m gpu."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(128, 128, 32), (200, 192, 32), (388, 328, 64)]      # (V, K, rows): V % 4 == 0, K % 8 == 0
PAD = 3                                                         # canary rows in front of and behind every live region
L2, CLIP, LR = 1e-3, 0.05, 1e-3


class _Guarded:
    """A [R][C] tensor inside a larger allocation: PAD rows of a recognisable pattern on both sides (and, with ld > C, to the right)."""

    def __init__(self, R, C, dtype, ld=None, seed=0):
        ld = C if ld is None else ld
        self.full = torch.empty(R + 2 * PAD, ld, dtype=dtype, device=DEV)
        pat = (torch.arange(self.full.numel(), device=DEV, dtype=torch.int64) * 37 + seed) % 251 + 1
        raw = self.full.view(-1).view(torch.uint8)
        raw.copy_(pat.repeat_interleave(self.full.element_size())[:raw.numel()].to(torch.uint8))
        self.live = self.full[PAD:PAD + R]
        self.R, self.C, self.ld = R, C, ld
        self.before = None

    def arm(self):
        self.before = self.full.clone()

    def margins_intact(self):
        a, b = self.full, self.before
        same = lambda x, y: torch.equal(x.contiguous().view(-1).view(torch.uint8), y.contiguous().view(-1).view(torch.uint8))  # noqa: E731
        return same(a[:PAD], b[:PAD]) and same(a[PAD + self.R:], b[PAD + self.R:]) and same(a[:, self.C:], b[:, self.C:])


def _inputs(V, K, rows):
    g = torch.Generator(device=DEV).manual_seed(1000 + V)
    Vp = (V + 63) // 64 * 64
    dlog = torch.zeros(rows, Vp, dtype=torch.bfloat16, device=DEV)
    dlog[:, :V] = (torch.randn(rows, V, device=DEV, generator=g) * 0.05).to(torch.bfloat16)
    x = (torch.randn(rows, K, device=DEV, generator=g) * 0.5).to(torch.bfloat16)
    p = torch.randn(V, K, device=DEV, generator=g) * 0.05
    m = torch.randn(V, K, device=DEV, generator=g) * 0.01
    v = (torch.randn(V, K, device=DEV, generator=g) * 0.01).square() + 1e-6
    return Vp, dlog, x, p, m, v


def _launch(V, K, rows, images=None, apply_sums=None):
    """One fused update from the seeded inputs, every output inside canary margins.  images: None, "split" (p_wide) or "high" (p_f16 + p_fp8);
    apply_sums: run evc_moe_grad_update_apply with these norm sums instead of evc_moe_grad_update."""
    from efficientvideoclassification_youtube8m_amd import ops
    Vp, dlog, x, p0, m0, v0 = _inputs(V, K, rows)
    out = {"p": _Guarded(V, K, torch.float32, seed=1), "m": _Guarded(V, K, torch.float32, seed=2), "v": _Guarded(V, K, torch.float32, seed=3),
           "pb": _Guarded(V, K, torch.bfloat16, seed=4), "pT": _Guarded(K, V, torch.bfloat16, ld=Vp + 64, seed=5)}
    if images == "split":
        out["wide"] = _Guarded(V, 2 * K, torch.bfloat16, seed=6)
    if images == "high":
        out["f16"] = _Guarded(V, K, torch.float16, seed=7)
        out["fp8"] = _Guarded(V, 2 * K, torch.uint8, seed=8)
    out["p"].live.copy_(p0)
    out["m"].live.copy_(m0)
    out["v"].live.copy_(v0)
    for t in out.values():
        t.arm()
    tiles = ((V + 127) // 128) * ((K + 127) // 128)
    ws = torch.zeros(2 * tiles, device=DEV)
    kw = dict(p_wide=out["wide"].live if images == "split" else None, p_f16=out["f16"].live if images == "high" else None,
              p_fp8=out["fp8"].live if images == "high" else None)
    if apply_sums is None:
        sums = torch.zeros(2, device=DEV)
        ops.moe_grad_update(dlog, x, rows, V, K, out["p"].live, out["m"].live, out["v"].live, out["pb"].live, out["pT"].live, L2, sums, ws, CLIP, LR, **kw)
        wsq = None
    else:
        sums, wsq = apply_sums.clone(), torch.zeros(2, device=DEV)
        ops.moe_grad_update_apply(dlog, x, rows, V, K, out["p"].live, out["m"].live, out["v"].live, out["pb"].live, out["pT"].live, L2, sums, ws, CLIP, LR,
                                  wsq, **kw)
    torch.cuda.synchronize()
    return out, sums, ws, wsq


@functools.lru_cache(maxsize=None)
def _fused(shape, images=None):
    return _launch(*shape, images=images)


@functools.lru_cache(maxsize=None)
def _materialised(shape):
    """The plain path: weight-gradient product, grad_sqnorm, clip_adam."""
    from efficientvideoclassification_youtube8m_amd import ops
    V, K, rows = shape
    Vp, dlog, x, p, m, v = _inputs(V, K, rows)
    V8 = (V + 7) // 8 * 8
    g = torch.zeros(V8, K, device=DEV)
    ops.gemm_tn(dlog, x, V8, K, rows, g)
    g = g[:V].contiguous()
    sums = torch.zeros(2, device=DEV)
    ops.grad_sqnorm(g, p, L2, sums)
    ops.clip_adam_step(p, g, m, v, L2, sums, CLIP, LR)
    torch.cuda.synchronize()
    return p, m, v, sums


def _bits(t):
    return t.contiguous().view(-1).view(torch.uint8)


@pytest.mark.parametrize("shape", SHAPES)
def test_update_matches_the_materialised_path(shape):
    """p, m, v after evc_moe_grad_update against gemm_tn + grad_sqnorm + clip_adam, within the bounds of
    test_gpu_step.py::test_fused_moe_update_matches_materialised_gradient_path (p: 2e-6 absolute, moments: 1e-4 of the largest); the clip bites."""
    out, sums, _, _ = _fused(shape)
    p, m, v, sums_ref = _materialised(shape)
    assert float(sums_ref[0]) ** 0.5 > 2 * CLIP                              # the clip scales the gradient down
    assert torch.allclose(sums, sums_ref, rtol=1e-4, atol=1e-12)
    dp = (out["p"].live - p).abs().max().item()
    dm = (out["m"].live - m).abs().max().item()
    dv = (out["v"].live - v).abs().max().item()
    print("shape", shape, "max |dp|", dp, "max |dm|", dm, "of", m.abs().max().item(), "max |dv|", dv, "of", v.abs().max().item())
    assert dp < 2e-6
    assert dm <= 1e-4 * m.abs().max().item() + 1e-12
    assert dv <= 1e-4 * v.abs().max().item() + 1e-12
    assert (out["p"].live - _inputs(*shape)[3]).abs().max().item() > 1e-4    # and the weights did move


@pytest.mark.parametrize("shape", SHAPES)
def test_shadows_are_exact_images_of_the_new_weights(shape):
    V, K, _ = shape
    out, _, _, _ = _fused(shape)
    p = out["p"].live
    assert torch.equal(_bits(out["pb"].live), _bits(p.bfloat16()))
    assert torch.equal(_bits(out["pT"].live[:, :V]), _bits(out["pb"].live.t()))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("images", ["split", "high"])
def test_high_and_split_images_equal_the_cast_entries(shape, images):
    """p_wide = [hi | lo] of evc_cast_f32_to_bf16_wide, p_f16 = evc_cast_f32_to_f16, p_fp8 = evc_cast_f32_to_fp8_lo of the new weights, bit for bit;
    the update itself does not depend on which images it writes."""
    from efficientvideoclassification_youtube8m_amd import ops
    V, K, _ = shape
    out, _, _, _ = _fused(shape, images)
    plain, _, _, _ = _fused(shape)
    p = out["p"].live
    for k in ("p", "m", "v", "pb", "pT"):
        assert torch.equal(_bits(out[k].full), _bits(plain[k].full)), k
    if images == "split":
        want = torch.empty(V, 2 * K, dtype=torch.bfloat16, device=DEV)
        ops.cast_bf16_wide(p, want, lo_first=False)
        assert torch.equal(_bits(out["wide"].live), _bits(want))
    else:
        want16 = torch.empty(V, K, dtype=torch.float16, device=DEV)
        ops.cast_f16(p.contiguous(), want16)
        assert torch.equal(_bits(out["f16"].live), _bits(want16))
        want8 = torch.empty(V, 2 * K, dtype=torch.uint8, device=DEV)
        ops.cast_fp8_lo(p.contiguous(), want8, hi_cols=K, scale_exp=ops.FP8_MOE["w_lo_exp"], hi_exp=ops.FP8_MOE["w_hi_exp"])
        assert torch.equal(out["fp8"].live, want8)
    for k, t in out.items():
        assert t.margins_intact(), k


@pytest.mark.parametrize("shape", SHAPES)
def test_nothing_outside_the_live_regions_is_written(shape):
    """Canary rows around p, m, v and both shadows, and the pad columns of the transposed shadow beyond V, keep their pattern."""
    out, _, _, _ = _fused(shape)
    for k, t in out.items():
        assert t.margins_intact(), k
        assert not torch.equal(_bits(t.live), _bits(t.before[PAD:PAD + t.R])), k      # while the live region was written


@pytest.mark.parametrize("shape", SHAPES)
def test_two_launches_give_the_same_bits(shape):
    """p, m, v, shadows and pass 1's partials (evc_moe_grad_update), and the |W|^2 partials of evc_moe_grad_update_apply, whose sum is the
    squared norm of the new weights."""
    a, sums_a, ws_a, _ = _fused(shape)
    b, sums_b, ws_b, _ = _launch(*shape)
    for k in a:
        assert torch.equal(_bits(a[k].full), _bits(b[k].full)), k
    assert torch.equal(_bits(ws_a), _bits(ws_b)) and torch.equal(_bits(sums_a), _bits(sums_b))
    c, _, ws_c, wsq_c = _launch(*shape, apply_sums=sums_a)
    d, _, ws_d, wsq_d = _launch(*shape, apply_sums=sums_a)
    for k in a:                                           # the update pass alone, from the same norm: the same update
        assert torch.equal(_bits(c[k].full), _bits(a[k].full)), k
        assert torch.equal(_bits(c[k].full), _bits(d[k].full)), k
        assert c[k].margins_intact(), k
    assert torch.equal(_bits(ws_c), _bits(ws_d)) and torch.equal(_bits(wsq_c), _bits(wsq_d))
    want = c["p"].live.double().square().sum().item()
    assert abs(wsq_c[0].item() - want) <= 1e-5 * want and wsq_c[1].item() == 0.0
    assert abs(ws_c.view(-1, 2)[:, 0].double().sum().item() - want) <= 1e-5 * want
