"""The MoE head's backward from the forward weight image: MoeHead with dx_fwd_image on (ops.gemm_kn on shadow_fwd, no transposed image kept or
written) against the transposed-image path (ops.gemm_nt on shadow_bwd), and the fused update kernel with and without its transposed pointer.
pytest -m gpu."""
import pytest
import torch

from efficientvideoclassification_youtube8m_amd import ops
from efficientvideoclassification_youtube8m_amd.engine import MoeHead
from efficientvideoclassification_youtube8m_amd.video_level_models import MoeTower

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
B, K, V, MX = 64, 256, 100, 2          # gates 300 -> 320 factor columns, experts 200 -> 256: both products meet the row clamp


def _bits(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _tower(monkeypatch, fwd_image, one_launch=True):
    monkeypatch.setattr(MoeHead, "dx_fwd_image", fwd_image)
    monkeypatch.setattr(MoeHead, "dx_one_launch", one_launch)
    tw = MoeTower(B, K, V, MX, device=DEV, training=True, seed=3)
    kept = MoeHead.GATES in tw.shadow_bwd and MoeHead.EXPERTS in tw.shadow_bwd
    assert kept == (not fwd_image) and (kept or (MoeHead.GATES not in tw.shadow_bwd and MoeHead.EXPERTS not in tw.shadow_bwd))
    return tw


def _step(tw, x, dpred, dx_init=None):
    """forward, backward for dx, then one fused update; returns dx (a copy)."""
    tw.forward(x)
    dx = tw.moe.backward(dpred, dx_init=dx_init, weight_grads=False).clone()
    tw.begin_update()
    tw.moe.fused_update(tw.adam_lr_t(1e-3), 1.0, 1e-8)
    torch.cuda.synchronize()
    return dx


@pytest.mark.parametrize("with_init", [False, True])
def test_head_dx_and_one_update(monkeypatch, with_init):
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn(B, K, generator=g).to(DEV)
    dpred = (torch.randn(B, V, generator=g) * 1e-2).to(DEV)
    dx_init = torch.randn(B, K, generator=g).to(DEV) if with_init else None
    old = _tower(monkeypatch, False)
    dx_old = _step(old, x, dpred, dx_init)
    # the float64 product of the factors the old tower left, for the bound: |dx - ref| <= (depth + splits + 1) U (sum |a b| + |dx_init|)
    m = old.moe
    a = torch.cat([m.dgl.double(), m.del_.double()], 1).cpu()
    results = {}
    for one_launch in (False, True):
        new = _tower(monkeypatch, True, one_launch)
        # (the weights before the update, as both towers' backward read them: same seed, same bf16 image)
        w = torch.cat([torch.nn.functional.pad(new.shadow_fwd[n].double(), (0, 0, 0, ops.round_up(new.shadow_fwd[n].shape[0], 64) - new.shadow_fwd[n].shape[0]))
                       for n in (MoeHead.GATES, MoeHead.EXPERTS)], 0).cpu()
        dx_new = _step(new, x, dpred, dx_init)
        results[one_launch] = dx_new
        base = dx_init.double().cpu() if with_init else torch.zeros(B, K, dtype=torch.float64)
        ref, absref = a @ w + base, a.abs() @ w.abs() + base.abs()
        depth = a.shape[1]
        splits = 1 if ops.DETERMINISTIC else max(ops.gemm_kn_splits(K, m.dgl.shape[1]), ops.gemm_kn_splits(K, m.dgl.shape[1], m.del_.shape[1]))
        bound = (depth + 2 * splits + 2) * U * absref
        for name, dx in (("new", dx_new), ("old", dx_old)):
            ratio = float(((dx.double().cpu() - ref).abs() / bound).max())
            print("dx %s one_launch=%s: max err / bound = %.3f" % (name, one_launch, ratio))
            assert ratio <= 1.0, (name, ratio)
        if not one_launch and ops.gemm_kn_splits(K, m.dgl.shape[1]) == 1 and ops.gemm_kn_splits(K, m.del_.shape[1]) == 1:
            assert torch.equal(_bits(dx_new), _bits(dx_old))          # unsplit, one launch per matrix: the transposed-image path's bits
        # masters, moments and the forward image after the update: the same bits on both paths
        for n in (MoeHead.GATES, MoeHead.EXPERTS, MoeHead.EBIAS):
            for what, t_new, t_old in (("p", new.store.p(n), old.store.p(n)), ("m", new.store.view(new.store.m, n), old.store.view(old.store.m, n)),
                                       ("v", new.store.view(new.store.v, n), old.store.view(old.store.v, n))):
                assert torch.equal(_bits(t_new), _bits(t_old)), (n, what)
        for n in (MoeHead.GATES, MoeHead.EXPERTS):
            assert torch.equal(_bits(new.shadow_fwd[n]), _bits(old.shadow_fwd[n])), n
            # ... and the old path's transposed image is the transpose of that forward image: what the new backward reads is what it read
            assert torch.equal(old.shadow_bwd[n][:, :old.shadow_fwd[n].shape[0]], old.shadow_fwd[n].t())


def test_switch_after_construction_and_precision(monkeypatch):
    """sync_bwd_images() brings the images back (filled from the masters) when the switch goes off or the precision leaves bf16."""
    tw = _tower(monkeypatch, True)
    tw.moe.dx_fwd_image = False
    tw.moe.sync_bwd_images()
    for n in (MoeHead.GATES, MoeHead.EXPERTS):
        assert torch.equal(tw.shadow_bwd[n][:, :tw.shadow_fwd[n].shape[0]], tw.shadow_fwd[n].t())
    tw2 = _tower(monkeypatch, True)
    tw2.set_precision("split")
    assert MoeHead.GATES in tw2.shadow_bwd and MoeHead.EXPERTS in tw2.shadow_bwd
    tw2.set_precision("bf16")
    assert MoeHead.GATES not in tw2.shadow_bwd


@pytest.mark.parametrize("apply", [False, True])
def test_update_kernel_without_transposed_pointer(apply):
    """rows 32, V 200, K 256 (2 x 2 tiles, ragged in V): p, m, v, the forward image and the returned sums are the same bits with pT and with NULL."""
    rows, Vn, Kn = 32, 200, 256
    g = torch.Generator(device=DEV).manual_seed(5)
    Vp = ops.round_up(Vn, 64)
    dlog = torch.zeros(rows, Vp, dtype=torch.bfloat16, device=DEV)
    dlog[:, :Vn] = (torch.randn(rows, Vn, device=DEV, generator=g) * 0.05).to(torch.bfloat16)
    x = (torch.randn(rows, Kn, device=DEV, generator=g) * 0.5).to(torch.bfloat16)
    p0 = torch.randn(Vn, Kn, device=DEV, generator=g) * 0.05
    m0 = torch.randn(Vn, Kn, device=DEV, generator=g) * 0.01
    v0 = (torch.randn(Vn, Kn, device=DEV, generator=g) * 0.01).square() + 1e-6
    out = {}
    for with_pt in (True, False):
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        pb = torch.full((Vn, Kn), 7.0, dtype=torch.bfloat16, device=DEV)
        pT = torch.full((Kn, Vp), 7.0, dtype=torch.bfloat16, device=DEV) if with_pt else None
        ws = torch.zeros(2 * ((Vn + 127) // 128) * ((Kn + 127) // 128), device=DEV)
        if apply:
            sums, wsq = torch.tensor([4.0, 0.0], device=DEV), torch.zeros(2, device=DEV)
            ops.moe_grad_update_apply(dlog, x, rows, Vn, Kn, p, m, v, pb, pT, 1e-3, sums, ws, 0.05, 1e-3, wsq)
            ret = wsq
        else:
            sums = torch.zeros(2, device=DEV)
            ops.moe_grad_update(dlog, x, rows, Vn, Kn, p, m, v, pb, pT, 1e-3, sums, ws, 0.05, 1e-3)
            ret = sums
        torch.cuda.synchronize()
        out[with_pt] = (p, m, v, pb, ret, pT)
    for i, name in enumerate(("p", "m", "v", "forward image", "sums")):
        assert torch.equal(_bits(out[True][i]), _bits(out[False][i])), name
    assert float(out[True][4][0]) > 0
    assert torch.equal(out[True][5][:, :Vn], out[True][3].t())          # (the transposed image, where asked for, is still written)


def test_null_transposed_pointer_needs_the_plain_bf16_form():
    """EVC_ERR_BAD_ARG (-5) before any launch: no transposed image and no bf16 forward image / with the split image."""
    from efficientvideoclassification_youtube8m_amd import _lib
    rows, Vn, Kn = 32, 128, 128
    dlog = torch.zeros(rows, Vn, dtype=torch.bfloat16, device=DEV)
    x = torch.zeros(rows, Kn, dtype=torch.bfloat16, device=DEV)
    p, m, v = (torch.full((Vn, Kn), 0.5, device=DEV) for _ in range(3))
    ws, sums = torch.zeros(8, device=DEV), torch.zeros(2, device=DEV)
    wide = torch.zeros(Vn, 2 * Kn, dtype=torch.bfloat16, device=DEV)
    pb = torch.zeros(Vn, Kn, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(_lib.EvcError, match=r"\(-5\).*pT_bf16 == NULL"):
        ops.moe_grad_update(dlog, x, rows, Vn, Kn, p, m, v, None, None, 0.0, sums, ws, 1.0, 1e-3)
    with pytest.raises(_lib.EvcError, match=r"\(-5\).*pT_bf16 == NULL"):
        ops.moe_grad_update(dlog, x, rows, Vn, Kn, p, m, v, pb, None, 0.0, sums, ws, 1.0, 1e-3, p_wide=wide)
    torch.cuda.synchronize()
    assert bool((p == 0.5).all()) and bool((m == 0.5).all())
