"""evc_distill_losses (ops.distill_losses): the loss section of the serial distillation step - teacher CE, L_REP, L_PRED, student CE
and the student's two gradients in one launch + a fixed-order finish - against float64 (tests/_distill_losses_ref.py).  pytest -m gpu.

Bounds.  Gradients, elementwise, no element exempt: |got - ref| <= 1e-5 (|ce term| + |kl term|) for dpred, 1e-5 |rep term| for dstate
(IEEE f32 on these formulas stays below 1.9e-7 of that scale on these shapes; 1e-5 leaves ~50x for approximate division and FMA
contraction).  Where a scale is 0 the remaining term stands alone; the KL gradient is a DIFFERENCE, -P/p_s + 1/sum(p_s), that cancels
where teacher and student agree, so alone it is held to 1e-5 of the magnitudes of its two addends (f32 rounds each addend to 6e-8 of
itself: nothing can be asked relative to a difference that may be 0).  Loss values: 1e-4 relative."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _distill_losses_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL_GRAD, RTOL_LOSS = 1e-5, 1e-4
_CACHE = {}


def _scales(B):
    return dict(g_ce=1.0 / B, g_kl=1.0, g_rep=2.0)          # the serial step's: CE batch mean, L_PRED batch sum, L_REP counted twice


def _case(shape):
    """Inputs (host + device) and the float64 reference of one shape, computed once per session and never modified."""
    if shape not in _CACHE:
        B, V, D = shape
        inp = ref.make_inputs(B, V, D)
        _CACHE[shape] = (inp, {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}, ref.reference(inp, **_scales(B)))
    return _CACHE[shape]


def _run(dv, scales, want_dp=True, want_ds=True, rowsum_t=None, pred_t=None):
    from efficientvideoclassification_youtube8m_amd import ops
    losses = torch.zeros(4, dtype=torch.float32, device=DEV)
    dp = torch.full_like(dv["pred_s"], float("nan")) if want_dp else None
    ds = torch.full_like(dv["state_s"], float("nan")) if want_ds else None
    ops.distill_losses(dv["pred_t"] if pred_t is None else pred_t, dv["rowsum_t"] if rowsum_t is None else rowsum_t, dv["pred_s"],
                       dv["rowsum_s"], dv["labels"], dv["state_t"], dv["state_s"], losses, dp, ds, **scales)
    torch.cuda.synchronize()
    return losses, dp, ds


def _check(got, want, bound, what):
    err = np.abs(got.double().cpu().numpy() - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: worst error %.3g of its bound" % (what, worst))
    assert np.all(err <= bound), (what, worst)


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_losses_and_gradients_against_float64(shape):
    inp, dv, want = _case(shape)
    losses, dp, ds = _run(dv, _scales(shape[0]))
    got_l = losses.double().cpu().numpy()
    print("losses", got_l, "ref", want["losses"])
    assert np.all(np.abs(got_l - want["losses"]) <= RTOL_LOSS * np.abs(want["losses"])), (got_l, want["losses"])
    _check(dp, want["ce"] + want["kl"], RTOL_GRAD * (np.abs(want["ce"]) + np.abs(want["kl"])), "dpred %s" % (shape,))
    _check(ds, want["rep"], RTOL_GRAD * np.abs(want["rep"]), "dstate %s" % (shape,))


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_each_scale_at_zero_leaves_the_other_terms_and_the_same_losses(shape):
    inp, dv, want = _case(shape)
    full = _scales(shape[0])
    base, _, _ = _run(dv, full)
    for off in ("g_ce", "g_kl", "g_rep"):
        losses, dp, ds = _run(dv, dict(full, **{off: 0.0}))
        assert torch.equal(losses, base), off                       # the values do not depend on the scales
        ce = 0.0 * want["ce"] if off == "g_ce" else want["ce"]
        kl, kl_parts = (0.0 * want["kl"], 0.0 * want["kl_parts"]) if off == "g_kl" else (want["kl"], want["kl_parts"])
        rep = 0.0 * want["rep"] if off == "g_rep" else want["rep"]
        _check(dp, ce + kl, RTOL_GRAD * (np.abs(ce) + (np.abs(kl) if off != "g_ce" else kl_parts)), "dpred %s %s=0" % (shape, off))
        _check(ds, rep, RTOL_GRAD * np.abs(rep), "dstate %s %s=0" % (shape, off))
        if off == "g_rep":
            assert not ds.any()
    losses, dp, ds = _run(dv, dict(g_ce=0.0, g_kl=0.0, g_rep=0.0))
    assert torch.equal(losses, base)
    assert not dp.any() and not ds.any()                            # exactly 0 (the buffers were NaN-filled: every element was written)


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_teacher_row_with_sum_zero(shape):
    """A collapsed teacher row (sum 0 < FLT_MIN): everything finite, that row's KL gradient exactly 0 (at any scale, 0 included), its
    CE gradient intact."""
    inp, dv, want = _case(shape)
    B = shape[0]
    r = B - 1
    pt = dv["pred_t"].clone()
    pt[r] = 0.0
    rs = dv["rowsum_t"].clone()
    rs[r] = 0.0
    full = _scales(B)
    for scales in (full, dict(full, g_kl=0.0), dict(full, g_ce=0.0)):
        losses, dp, ds = _run(dv, scales, rowsum_t=rs, pred_t=pt)
        assert torch.isfinite(losses).all() and torch.isfinite(dp).all() and torch.isfinite(ds).all()
        ce = want["ce"][r] * (scales["g_ce"] / full["g_ce"])
        _check(dp[r], ce, RTOL_GRAD * np.abs(ce), "dpred of the degenerate row %s %s" % (shape, scales))     # = the CE term alone: KL adds exactly 0
        if scales["g_ce"] == 0.0:
            assert not dp[r].any()
    both = _run(dv, full, want_ds=False, rowsum_t=rs, pred_t=pt)[1]
    alone = _run(dv, dict(full, g_kl=0.0), want_ds=False, rowsum_t=rs, pred_t=pt)[1]
    assert torch.equal(both[r], alone[r])                           # bit for bit: the row's KL gradient is 0, not small


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_two_calls_give_identical_bits_and_null_gradients_give_losses_only(shape):
    inp, dv, want = _case(shape)
    sc = _scales(shape[0])
    a, b = _run(dv, sc), _run(dv, sc)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    l0, dp0, ds0 = _run(dv, sc, want_dp=False, want_ds=False)
    assert dp0 is None and ds0 is None and torch.equal(l0, a[0])
    l1, dp1, ds1 = _run(dv, sc, want_dp=True, want_ds=False)
    assert torch.equal(l1, a[0]) and torch.equal(dp1, a[1])
    l2, dp2, ds2 = _run(dv, sc, want_dp=False, want_ds=True)
    assert torch.equal(l2, a[0]) and torch.equal(ds2, a[2])


def test_losses_accumulate_into_the_four_slots():
    """losses[i] += value: a second call on the same buffer doubles every slot (the graph zeroes it once per step)."""
    from efficientvideoclassification_youtube8m_amd import ops
    inp, dv, want = _case(ref.SHAPES[2])
    losses = torch.zeros(6, dtype=torch.float32, device=DEV)
    for _ in range(2):
        ops.distill_losses(dv["pred_t"], dv["rowsum_t"], dv["pred_s"], dv["rowsum_s"], dv["labels"], dv["state_t"], dv["state_s"], losses)
    got = losses.double().cpu().numpy()
    assert np.all(np.abs(got[:4] - 2 * want["losses"]) <= RTOL_LOSS * 2 * np.abs(want["losses"])) and not got[4:].any()


def test_kl_pred_loss_repeats_bit_for_bit_under_evc_deterministic():
    """EVC_DETERMINISTIC=1 (read once per process: a child): ops.kl_pred_loss joins its row sums in row order (evc_kl_pred_loss_ordered),
    not by float atomics - 20 calls on 64 rows give the same bits, and value and gradient are float64's within the bounds above."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(root, "tests", "_label_loss_child.py"), "kl"],
                       env=dict(os.environ, EVC_DETERMINISTIC="1"), capture_output=True, text=True)
    print(r.stdout[-2000:])
    if r.returncode in (-6, -11, -9, 134, 139, 137, 124):
        pytest.exit("the kl child died with %d, stopping:\n%s" % (r.returncode, r.stdout[-2000:] + r.stderr[-3000:]), returncode=3)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]
