"""evc_label_loss (ops.label_loss): the seven label losses of --label_loss besides CrossEntropyLoss - value and dL/dpred in one pass -
against float64 (tests/_label_losses_ref.py).  pytest -m gpu.

Bounds - the project's existing ones for the same formulas (tests/test_gpu_distill_losses.py).  Gradients, elementwise, no element
exempt: |got - ref| <= 1e-5 grad_scale sum|addends of the kind's expression| (SOFTMAX: the two addends softmax_c sum(yhat) and yhat_c
of a difference that can cancel); an element whose reference gradient is exactly 0 - masked, the hinge's flat side, a label-free softmax
row - must be exactly 0.  Loss values: 1e-4 relative."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _label_losses_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL_GRAD, RTOL_LOSS = 1e-5, 1e-4
_CACHE = {}
WORST = {}


def _weights(kind, V):
    return ref.make_weights(V) if kind == "CLASS_IMBALANCE" else None


def _case(kind, shape, wide=False):
    """Inputs and the float64 reference of one (kind, shape), computed once per session and never modified."""
    key = (kind, shape, wide)
    if key not in _CACHE:
        p, y = ref.make_inputs(kind, shape[0], shape[1], wide=wide)
        w = _weights(kind, shape[1])
        _CACHE[key] = (p, y, w, ref.reference(kind, p, y, w))
    return _CACHE[key]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(kind, p, y, w=None, grad_scale=1.0, want_grad=True, dpred=None, accumulate=False, loss=None):
    from efficientvideoclassification_youtube8m_amd import ops
    p, y, w = (_dev(t) if isinstance(t, np.ndarray) else t for t in (p, y, w))
    if loss is None:
        loss = torch.zeros(1, dtype=torch.float32, device=DEV)
    if dpred is None and want_grad:
        dpred = torch.full_like(p, float("nan"))                   # every element must be written
    ops.label_loss(ref.KIND_IDS[kind], p, y, loss, dpred, grad_scale=grad_scale, accumulate_grad=accumulate, class_weights=w)
    torch.cuda.synchronize()
    return loss, dpred


def _check(kind, loss, dpred, want, grad_scale, what, extra=None):
    got_l = float(loss.double().cpu()[0])
    print("%s: loss %.9g ref %.9g" % (what, got_l, want["loss"]))
    assert abs(got_l - want["loss"]) <= RTOL_LOSS * abs(want["loss"]), (what, got_l, want["loss"])
    got = dpred.double().cpu().numpy()
    refg = want["grad"] * grad_scale
    bound = RTOL_GRAD * abs(grad_scale) * want["mag"] + (0.0 if extra is None else extra)
    err = np.abs(got - refg)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    WORST[kind] = max(WORST.get(kind, 0.0), worst if np.isfinite(worst) and worst < 1e200 else 0.0)
    print("%s: worst gradient error %.3g of its bound (worst of %s so far: %.3g)" % (what, worst, kind, WORST[kind]))
    assert np.all(err <= bound), (what, worst)
    if extra is None:
        zero = refg == 0
        assert not got[zero].any(), (what, "an element whose reference gradient is exactly 0 is not exactly 0")


ALL_CASES = [(k, s) for k in ref.KINDS for s in ref.SHAPES] + [(k, s) for k in ref.KINDS if k != "TOP50" for s in ref.SMALL_SHAPES]


@pytest.mark.parametrize("kind,shape", ALL_CASES)
def test_loss_and_gradient_against_float64(kind, shape):
    p, y, w, want = _case(kind, shape)
    gs = 1.0 / shape[0]
    loss, dp = _run(kind, p, y, w, grad_scale=gs)
    _check(kind, loss, dp, want, gs, "%s %s" % (kind, shape))


@pytest.mark.parametrize("kind", ["HINGE", "SOFTMAX"])
@pytest.mark.parametrize("shape", ref.SHAPES + ref.SMALL_SHAPES)
def test_logit_ranged_inputs(kind, shape):
    p, y, w, want = _case(kind, shape, wide=True)
    loss, dp = _run(kind, p, y, w, grad_scale=0.37)
    _check(kind, loss, dp, want, 0.37, "%s %s wide" % (kind, shape))


@pytest.mark.parametrize("shape", ref.SMALL_SHAPES + [(3, 49)])
def test_top50_refuses_fewer_than_50_classes(shape):
    from efficientvideoclassification_youtube8m_amd import _lib
    p, y = ref.make_inputs("POSITIVES", *shape)
    loss, dp = torch.full((1,), 3.0, device=DEV), torch.full(shape, 5.0, device=DEV)
    with pytest.raises(_lib.EvcError, match="V >= 50"):
        _run("TOP50", p, y, loss=loss, dpred=dp)
    torch.cuda.synchronize()
    assert float(loss[0]) == 3.0 and bool((dp == 5.0).all())


# ---- planted cases ----------------------------------------------------------------------------------------------------------------

def _planted(kind, p, y, w=None, gs=0.25, what=""):
    want = ref.reference(kind, p, y, w)
    loss, dp = _run(kind, p, y, w, grad_scale=gs)
    _check(kind, loss, dp, want, gs, "%s planted %s" % (kind, what))
    return want, dp


def test_top50_ties_at_the_threshold_are_all_kept():
    p, y = ref.make_inputs("TOP50", 3, 257, seed=5)
    order = np.argsort(-p[1])
    p[1, order[47:55]] = p[1, order[50]]                           # the 48th .. 55th largest are equal
    want, dp = _planted("TOP50", p, y, what="ties 48..55")
    assert want["mask"][1].sum() == 55 and want["mask"][0].sum() == 50
    assert int((dp[1] != 0).sum()) == 55


def test_top50_row_of_identical_values_keeps_every_class():
    p, y = ref.make_inputs("TOP50", 2, 130, seed=6)
    p[0, :] = np.float32(0.3)
    want, dp = _planted("TOP50", p, y, what="identical row")
    assert want["mask"][0].sum() == 130 and int((dp[0] != 0).sum()) == 130


def test_top50_49_ones_and_zeros_otherwise():
    p, y = ref.make_inputs("TOP50", 2, 257, seed=7)
    p[1, :] = 0
    p[1, np.random.RandomState(1).choice(257, 49, replace=False)] = 1
    want, dp = _planted("TOP50", p, y, what="49 ones")             # t = 0: the mask keeps all
    assert want["mask"][1].sum() == 257 and int((dp[1] != 0).sum()) == 257


def test_top50_with_exactly_50_classes():
    p, y = ref.make_inputs("TOP50", 4, 50, seed=8)
    want, dp = _planted("TOP50", p, y, what="V = 50")
    assert np.all(want["mask"] == 1)


def test_new_batch_without_a_positive():
    p, y = ref.make_inputs("NEW", 3, 257, seed=9)
    y[:] = 0
    p[0, :5] = [0.95, 0.9, 0.91, 0.89, 0.9000001]
    want, dp = _planted("NEW", p, y, what="no positive")
    assert want["mpp"] == float(np.float32(np.float32(1.0) - np.float32(0.1)))
    assert 0 < want["bn"].sum() < want["bn"].size


def test_new_clamp_at_one_tenth():
    p, y = ref.make_inputs("NEW", 3, 257, seed=10)
    b, c = np.argwhere(y != 0)[0]
    p[b, c] = np.float32(0.05)                                     # the smallest positive: 0.05 - 0.1 < 0.1
    neg = np.argwhere(y == 0)
    p[neg[0][0], neg[0][1]], p[neg[1][0], neg[1][1]] = np.float32(0.1), np.nextafter(np.float32(0.1), np.float32(1))
    want, dp = _planted("NEW", p, y, what="clamp")
    assert want["mpp"] == float(np.float32(0.1))
    assert want["bn"][neg[0][0], neg[0][1]] == 0 and want["bn"][neg[1][0], neg[1][1]] == 1


def test_new_positive_at_exactly_nine_tenths_is_not_bad():
    p, y = ref.make_inputs("NEW", 2, 64, seed=11)
    idx = np.argwhere(y != 0)
    p[idx[0][0], idx[0][1]] = np.float32(0.9)
    p[idx[1][0], idx[1][1]] = np.nextafter(np.float32(0.9), np.float32(0))
    want, dp = _planted("NEW", p, y, what="0.9f")
    assert want["bp"][idx[0][0], idx[0][1]] == 0 and want["bp"][idx[1][0], idx[1][1]] == 1
    assert float(dp[idx[0][0], idx[0][1]]) == 0.0 and float(dp[idx[1][0], idx[1][1]]) != 0.0


def test_hinge_ties_have_gradient_zero():
    p, y = ref.make_inputs("HINGE", 2, 64, seed=12, wide=True)
    pos, neg = np.argwhere(y != 0)[0], np.argwhere(y == 0)[0]
    p[pos[0], pos[1]], p[neg[0], neg[1]] = np.float32(1.0), np.float32(-1.0)
    want, dp = _planted("HINGE", p, y, what="ties")
    assert want["grad"][pos[0], pos[1]] == 0 and want["grad"][neg[0], neg[1]] == 0
    assert float(dp[pos[0], pos[1]]) == 0.0 and float(dp[neg[0], neg[1]]) == 0.0


def test_softmax_rows_without_and_with_one_label():
    p, y = ref.make_inputs("SOFTMAX", 3, 257, seed=13, wide=True)
    y[0, :] = 0
    y[1, :] = 0
    y[1, 200] = 1
    want, dp = _planted("SOFTMAX", p, y, what="0 and 1 labels")
    assert not want["grad"][0].any() and not dp[0].any()


def test_class_imbalance_weights_from_1_to_1000():
    V = 257
    p, y = ref.make_inputs("CLASS_IMBALANCE", 5, V, seed=14)
    w = ref.make_weights(V)
    assert w.min() == 1.0 and w.max() == pytest.approx(1000.0)
    y[0, int(np.argmax(w))] = 1
    y[1, int(np.argmin(w))] = 1
    _planted("CLASS_IMBALANCE", p, y, w, what="weights 1..1e3")


# ---- API behaviour ----------------------------------------------------------------------------------------------------------------

API_SHAPE = (4, 257)


@pytest.mark.parametrize("kind", ref.KINDS)
def test_accumulate_no_gradient_zero_scale_and_two_calls(kind):
    p, y, w, want = _case(kind, API_SHAPE)
    gs = 0.5
    base_loss, base_dp = _run(kind, p, y, w, grad_scale=gs)
    # accumulate_grad on a prefilled dpred
    pre = torch.from_numpy(np.random.RandomState(3).uniform(-2, 2, size=API_SHAPE).astype(np.float32)).to(DEV)
    loss, dp = _run(kind, p, y, w, grad_scale=gs, dpred=pre.clone(), accumulate=True)
    assert torch.equal(loss, base_loss)
    got = dp.double() - pre.double()
    extra = 6e-8 * (np.abs(pre.double().cpu().numpy()) + np.abs(want["grad"] * gs))
    _check(kind, loss, got, want, gs, "%s accumulate" % kind, extra=extra)
    # dpred = None leaves the same loss bits
    loss, none = _run(kind, p, y, w, grad_scale=gs, want_grad=False)
    assert none is None and torch.equal(loss, base_loss)
    # grad_scale = 0: exact zeros, the same loss
    loss, dp = _run(kind, p, y, w, grad_scale=0.0)
    assert torch.equal(loss, base_loss) and not dp.any()
    # two calls add the loss twice
    loss, _ = _run(kind, p, y, w, grad_scale=gs)
    loss, dp = _run(kind, p, y, w, grad_scale=gs, loss=loss)
    assert float(loss[0]) == float(base_loss[0] + base_loss[0]) and torch.equal(dp, base_dp)


def _digest(shape=(7, 1023)):
    """sha256 over the loss and dpred bits of every kind on one shape."""
    h = hashlib.sha256()
    for kind in ref.KINDS:
        p, y = ref.make_inputs(kind, *shape)
        loss, dp = _run(kind, p, y, _weights(kind, shape[1]), grad_scale=1.0 / shape[0])
        h.update(loss.cpu().numpy().tobytes())
        h.update(dp.cpu().numpy().tobytes())
    return h.hexdigest()


def test_two_runs_give_the_same_bits_with_and_without_deterministic_mode():
    a, b = _digest(), _digest()
    assert a == b
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(root, "tests", "_label_loss_child.py"), "digest"],
                       env=dict(os.environ, EVC_DETERMINISTIC="1"), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok" and lines[-3] == lines[-2] == a, (lines[-3:], a)


@pytest.mark.parametrize("kind", ref.KINDS)
def test_unaligned_views_give_the_values_of_aligned_copies(kind):
    B, V = API_SHAPE
    p, y, w, want = _case(kind, API_SHAPE)
    base_loss, base_dp = _run(kind, p, y, w, grad_scale=0.5)
    pbuf = torch.zeros(B * V + 8, dtype=torch.float32, device=DEV)
    dbuf = torch.full((B * V + 8,), float("nan"), dtype=torch.float32, device=DEV)
    ybuf = torch.zeros(B * V + 8, dtype=torch.uint8, device=DEV)
    pv, dv, yv = pbuf[1:1 + B * V].view(B, V), dbuf[1:1 + B * V].view(B, V), ybuf[1:1 + B * V].view(B, V)
    pv.copy_(_dev(p))
    yv.copy_(_dev(y))
    assert pv.data_ptr() % 16 == 4 and dv.data_ptr() % 16 == 4 and yv.data_ptr() % 4 == 1
    loss, dp = _run(kind, pv, yv, w, grad_scale=0.5, dpred=dv)
    assert torch.equal(dp, base_dp)
    assert abs(float(loss[0]) - float(base_loss[0])) <= 1e-6 * abs(float(base_loss[0]))     # (the lanes take other elements: another sum order)
    assert bool(torch.isnan(dbuf[:1]).all()) and bool(torch.isnan(dbuf[1 + B * V:]).all())   # nothing written outside the view
    _check(kind, loss, dp, want, 0.5, "%s unaligned" % kind)


def test_refusals_raise_and_launch_nothing():
    from efficientvideoclassification_youtube8m_amd import _lib, ops
    B, V = 3, 64
    p, y = (_dev(t) for t in ref.make_inputs("HINGE", B, V))
    w = _dev(ref.make_weights(V))
    loss = torch.full((1,), 3.0, device=DEV)
    dp = torch.full((B, V), 5.0, device=DEV)
    ws = torch.empty(B + 320, dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def raw(kind, B_, V_, weights, workspace):
        _lib.call("evc_label_loss", kind, p.data_ptr(), y.data_ptr(), B_, V_, 1.0, None if weights is None else weights.data_ptr(),
                  loss.data_ptr(), dp.data_ptr(), 0, None if workspace is None else workspace.data_ptr(), st)

    for args in ((ops.LOSS_HINGE, 0, V, None, ws), (ops.LOSS_HINGE, B, 0, None, ws), (ops.LOSS_HINGE, -1, V, None, ws),
                 (ops.LOSS_HINGE, 1, 32769, None, ws),                             # V > 32768
                 (0, B, V, None, ws), (8, B, V, None, ws), (-3, B, V, None, ws),   # unknown kinds
                 (ops.LOSS_TOP50, B, 49, None, ws),                                # TOP50 with V < 50
                 (ops.LOSS_CLASS_IMBALANCE, B, V, None, ws),                       # CLASS_IMBALANCE without weights
                 (ops.LOSS_HINGE, B, V, w, ws), (ops.LOSS_TOP50, B, V, w, ws),     # weights with another kind
                 (ops.LOSS_HINGE, B, V, None, None)):                              # NULL workspace
        with pytest.raises(_lib.EvcError, match="evc_label_loss"):
            raw(*args)
    with pytest.raises(_lib.EvcError):
        ops.label_loss(ops.LOSS_CLASS_IMBALANCE, p, y, loss, dp)
    with pytest.raises(_lib.EvcError):
        ops.label_loss(ops.LOSS_NEW, p, y, loss, dp, class_weights=w)
    torch.cuda.synchronize()
    assert float(loss[0]) == 3.0 and bool((dp == 5.0).all())       # nothing was launched
    raw(ops.LOSS_HINGE, B, V, None, ws)                            # the same call, accepted
    torch.cuda.synchronize()
    assert float(loss[0]) != 3.0 and not bool((dp == 5.0).any())


def test_losses_classes_go_through_the_same_kernels():
    """losses.<Class>().calculate_loss: the mean-of-rows value and, in grad_out, dLoss/dpredictions (grad_scale = 1/B)."""
    from efficientvideoclassification_youtube8m_amd import losses
    for kind in ref.KINDS:
        p, y, w, want = _case(kind, (5, 64))
        fn = getattr(losses, ref.CLASS_NAMES[kind])(**({"weights": w} if w is not None else {}))
        grad = torch.full((5, 64), float("nan"), device=DEV)
        val = fn.calculate_loss(_dev(p), _dev(y), grad_out=grad)
        base_loss, base_dp = _run(kind, p, y, w, grad_scale=1.0 / 5)
        assert val.dim() == 0 and torch.equal(val, base_loss[0]) and torch.equal(grad, base_dp)
        assert torch.equal(fn.calculate_loss(_dev(p), _dev(y).float()), val)       # float labels are cast, no gradient asked for


def test_worst_ratios_report():
    """Not a check of its own: prints the worst gradient error of every kind relative to its bound over the tests above."""
    for kind in ref.KINDS:
        print("worst ratio %-16s %.3g" % (kind, WORST.get(kind, float("nan"))))
