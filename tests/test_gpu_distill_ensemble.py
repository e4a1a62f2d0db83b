"""evc_distill_losses_ensemble (ops.distill_losses_ensemble): the loss section of the serial distillation step for one student against J
frozen teachers, against float64 on the combined arrays (tests/_distill_ensemble_ref.py).  pytest -m gpu.

Inputs: labels and the student are make_inputs(B, V, D); teacher j takes pred_t / state_t of make_inputs(B, V, D, seed=j).
Bounds: those of test_gpu_distill_losses_multi.py, unchanged - gradients elementwise, no element exempt: |got - ref| <= 1e-5 (|ce term| +
|kl term|) for dpred, 1e-5 |rep term| for dstate; loss values and every teacher's own CE 1e-4 relative.  Output buffers are NaN-filled
first: an unwritten element fails.  The combined row is compared bit for bit with ops.ensemble_topk_rows' dense output."""
import numpy as np
import pytest
import torch

import _distill_ensemble_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL_GRAD, RTOL_LOSS = 1e-5, 1e-4
# (B, V, D), J
CASES = [((1, 5, 3), 1), ((1, 5, 3), 3),          # the smallest case
         ((2, 1023, 100), 2),                     # V and B * D not multiples of 4: the scalar paths
         ((7, 257, 4), 8),                        # the maximum J
         ((3, 4716, 4096), 3),                    # the real V and D
         ((1030, 8, 4), 2),                       # the finish launch with more than one piece of 1024; the cancellation case
         ((70, 12, 4096), 2)]                     # NS = 256 and a partial second grid-stride trip of the state part
MODES = ("mean", "max")
_CACHE = {}


def _weights(J, mode):
    """Non-uniform weights that sum to 1 in mode mean (None in mode max, where none are read); rep weights over every teacher."""
    if mode == "max":
        w = None
    else:
        w = np.arange(1, J + 1, dtype=np.float32)
        w = (w / w.sum()).astype(np.float32)
    r = np.linspace(1.0, 0.25, J).astype(np.float32)
    return w, (r / r.sum()).astype(np.float32)


def _scales(B):
    return dict(g_ce=1.0 / B, g_kl=1.0, g_rep=2.0)


def _case(shape, J, mode):
    """Host inputs, device tensors and the float64 reference of one case; computed once, never modified."""
    key = (shape, J, mode)
    if key not in _CACHE:
        B, V, D = shape
        inp = ref.make_inputs(B, V, D)
        preds, states = ref.teachers(B, V, D, J)
        w, r = _weights(J, mode)
        want = ref.reference(inp, preds, states, mode, w, r, **_scales(B))
        dv = {n: torch.from_numpy(inp[n]).to(DEV) for n in ("labels", "pred_s", "state_s")}
        dv["preds_t"] = [torch.from_numpy(p).to(DEV) for p in preds]
        dv["states_t"] = [torch.from_numpy(s).to(DEV) for s in states]
        _CACHE[key] = (inp, dv, want, w, r)
    return _CACHE[key]


def _run(dv, mode, w, r, scales, preds_t=None, states_t=None, pred_s=None, dp=None, want_dp=True, want_ds=True, losses=None, comb=False):
    from efficientvideoclassification_youtube8m_amd import ops
    preds_t = dv["preds_t"] if preds_t is None else preds_t
    states_t = dv["states_t"] if states_t is None else states_t
    pred_s = dv["pred_s"] if pred_s is None else pred_s
    J = len(preds_t)
    if losses is None:
        losses = torch.zeros(4, dtype=torch.float32, device=DEV)
    if dp is None and want_dp:
        dp = torch.full_like(dv["pred_s"], float("nan"))
    ds = torch.full_like(dv["state_s"], float("nan")) if want_ds else None
    tce = torch.zeros(J, dtype=torch.float32, device=DEV)
    pc = torch.full_like(dv["pred_s"], float("nan")) if comb else None
    ops.distill_losses_ensemble(preds_t, states_t, dv["labels"], pred_s, dv["state_s"], losses, dp, ds, mode=mode, weights=w,
                                rep_weights=r, teacher_ce=tce, pred_comb=pc, **scales)
    torch.cuda.synchronize()
    return dict(losses=losses, dp=dp, ds=ds, tce=tce, comb=pc)


def _check(got, want, bound, what):
    """Prints the figure, then returns the list of misses (empty: within the bound everywhere) for the caller to assert on."""
    err = np.abs(got.double().cpu().numpy() - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    over = int((err > bound).sum())
    print("%s: worst error %.3g of its bound, %d of %d elements over it" % (what, worst, over, err.size))
    return [] if over == 0 else [(what, worst, over)]


def _check_all(out, want, what):
    got_l = out["losses"].double().cpu().numpy()
    got_t = out["tce"].double().cpu().numpy()
    print(what, "losses", got_l, "ref", want["losses"], "teacher CE", got_t, "ref", want["teacher_ce"])
    missed = []
    if not np.all(np.abs(got_l - want["losses"]) <= RTOL_LOSS * np.abs(want["losses"])):
        missed.append(("losses " + what, got_l, want["losses"]))
    if not np.all(np.abs(got_t - want["teacher_ce"]) <= RTOL_LOSS * np.abs(want["teacher_ce"])):
        missed.append(("teacher_ce " + what, got_t, want["teacher_ce"]))
    ce, kl = want["ce"], want["kl"]
    missed += _check(out["dp"], ce + kl, RTOL_GRAD * (np.abs(ce) + np.abs(kl)), "dpred " + what)
    missed += _check(out["ds"], want["rep"], RTOL_GRAD * np.abs(want["rep"]), "dstate " + what)
    return missed


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,J", CASES)
def test_combined_row_losses_and_gradients(shape, J, mode):
    """The combined row against ops.ensemble_topk_rows' dense output (and the numpy restatement) bit for bit; losses, per-teacher CE and
    gradients against float64; two identical calls give the same bits."""
    from efficientvideoclassification_youtube8m_amd import ops
    inp, dv, want, w, r = _case(shape, J, mode)
    out = _run(dv, mode, w, r, _scales(shape[0]), comb=True)
    dense = ops.ensemble_topk_rows(dv["preds_t"], 0, mode=mode, weights=w, dense=True)[2]
    assert torch.equal(out["comb"], dense)
    assert np.array_equal(out["comb"].cpu().numpy().view(np.uint32), want["pred_comb"].view(np.uint32))
    missed = _check_all(out, want, "%s J=%d %s" % (shape, J, mode))
    assert not missed, missed
    again = _run(dv, mode, w, r, _scales(shape[0]), comb=True)
    for k in ("losses", "dp", "ds", "tce", "comb"):
        assert torch.equal(out[k], again[k]), k


@pytest.mark.parametrize("shape", [(1, 5, 3), (2, 1023, 100), (3, 4716, 4096), (1030, 8, 4)])
def test_duplicates_give_the_bits_of_one_teacher(shape):
    """[p, p] under mean [.5, .5] and max over three copies against J = 1 on [p] with w = [1]: losses, dpred and dstate bit for bit."""
    inp, dv, want, _, _ = _case(shape, 1, "mean")
    sc = _scales(shape[0])
    p, s = dv["preds_t"][0], dv["states_t"][0]
    one = _run(dv, "mean", [1.0], [1.0], sc, preds_t=[p], states_t=[s])
    two = _run(dv, "mean", [0.5, 0.5], [1.0, 0.0], sc, preds_t=[p, p.clone()], states_t=[s, None])
    three = _run(dv, "max", None, [0.0, 0.0, 1.0], sc, preds_t=[p, p.clone(), p], states_t=[None, None, s])
    one_max = _run(dv, "max", None, [1.0], sc, preds_t=[p], states_t=[s])
    for other in (two, three, one_max):
        for k in ("losses", "dp", "ds"):
            assert torch.equal(one[k], other[k]), k


@pytest.mark.parametrize("shape", [(2, 1023, 100), (3, 4716, 4096), (70, 12, 4096)])
def test_rep_weights_select_the_state(shape):
    """r = [1, 0]: dstate and losses[1] of J = 1 on teacher 0's state, bit for bit; r = [0, 1] with no tensor for entry 0's state: teacher 1's."""
    inp, dv, want, w, _ = _case(shape, 2, "mean")
    sc = _scales(shape[0])
    for pick in (0, 1):
        r = [1.0, 0.0] if pick == 0 else [0.0, 1.0]
        states = [dv["states_t"][0], None] if pick == 0 else [None, dv["states_t"][1]]       # None -> a NULL pointer in the argument block
        got = _run(dv, "mean", w, r, sc, states_t=states)
        alone = _run(dv, "mean", [1.0], [1.0], sc, preds_t=[dv["preds_t"][pick]], states_t=[dv["states_t"][pick]])
        assert torch.equal(got["ds"], alone["ds"]) and torch.equal(got["losses"][1], alone["losses"][1]), pick
        d = dv["states_t"][pick].double() - dv["state_s"].double()
        rep = -2.0 * d.cpu().numpy() / shape[0] * sc["g_rep"]
        assert not _check(got["ds"], rep, RTOL_GRAD * np.abs(rep), "dstate r picks %d %s" % (pick, shape))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,J", CASES)
def test_all_zero_scales_give_exact_zeros_and_the_same_losses(shape, J, mode):
    inp, dv, want, w, r = _case(shape, J, mode)
    base = _run(dv, mode, w, r, _scales(shape[0]))
    zero = _run(dv, mode, w, r, dict(g_ce=0.0, g_kl=0.0, g_rep=0.0))
    assert torch.equal(zero["losses"], base["losses"]) and torch.equal(zero["tce"], base["tce"])      # the values do not depend on the scales
    assert not zero["dp"].any() and not zero["ds"].any()              # exactly 0, every element written (the buffers were NaN-filled)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,J", [((1, 5, 3), 3), ((2, 1023, 100), 2), ((3, 4716, 4096), 3)])
def test_collapsed_combined_row(shape, J, mode):
    """Every teacher zero on the last row (combined sum 0 < FLT_MIN): everything finite, the row's KL gradient exactly 0."""
    inp, dv, want, w, r = _case(shape, J, mode)
    B = shape[0]
    row = B - 1
    preds = [p.clone() for p in dv["preds_t"]]
    for p in preds:
        p[row] = 0.0
    full = dict(g_ce=1.0 / B, g_kl=1.5, g_rep=2.0)
    both = _run(dv, mode, w, r, full, preds_t=preds)
    for k in ("losses", "dp", "ds", "tce"):
        assert torch.isfinite(both[k]).all(), k
    ce = want["ce"][row]                                              # = the CE term alone: KL adds exactly 0
    assert not _check(both["dp"][row], ce, RTOL_GRAD * np.abs(ce), "dpred of the collapsed row %s %s" % (shape, mode))
    alone = _run(dv, mode, w, r, dict(full, g_kl=0.0), preds_t=preds, want_ds=False)
    assert torch.equal(both["dp"][row], alone["dp"][row])             # bit for bit: the row's KL gradient is 0, not small


@pytest.mark.parametrize("mode", MODES)
def test_a_misaligned_student(mode):
    """(3, 4716, 4096): pred_s and dpred_s start 4 bytes into their allocations; the same bounds, nothing written in front of the view."""
    shape, J = (3, 4716, 4096), 3
    inp, dv, want, w, r = _case(shape, J, mode)
    B, V, D = shape
    buf = torch.empty(B * V + 1, dtype=torch.float32, device=DEV)
    shifted = buf[1:].view(B, V)
    shifted.copy_(dv["pred_s"])
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    dbuf = torch.full((B * V + 1,), float("nan"), dtype=torch.float32, device=DEV)
    dp = dbuf[1:].view(B, V)
    assert dp.data_ptr() % 16 == 4
    out = _run(dv, mode, w, r, _scales(B), pred_s=shifted, dp=dp)
    missed = _check_all(out, want, "%s misaligned student %s" % (shape, mode))
    assert not missed, missed
    assert torch.isnan(dbuf[0])                                      # nothing written in front of the view
    aligned = _run(dv, mode, w, r, _scales(B))
    for k in ("losses", "dp", "ds"):                                 # the same elements in the same order: the same bits
        assert torch.equal(out[k], aligned[k]), k


def test_losses_accumulate():
    """losses[i] += value, teacher_ce[j] += value: a second call on the same buffers doubles every slot."""
    from efficientvideoclassification_youtube8m_amd import ops
    shape, J = (7, 257, 4), 8
    inp, dv, want, w, r = _case(shape, J, "mean")
    once = _run(dv, "mean", w, r, _scales(shape[0]), want_dp=False, want_ds=False)
    losses = torch.zeros(4, dtype=torch.float32, device=DEV)
    tce = torch.zeros(J, dtype=torch.float32, device=DEV)
    for _ in range(2):
        ops.distill_losses_ensemble(dv["preds_t"], dv["states_t"], dv["labels"], dv["pred_s"], dv["state_s"], losses, mode="mean", weights=w,
                                    rep_weights=r, teacher_ce=tce, **_scales(shape[0]))
    torch.cuda.synchronize()
    assert torch.equal(losses, 2 * once["losses"]) and torch.equal(tce, 2 * once["tce"])       # x + x is exact


def test_refusals():
    """J of 0 or 9, a bad mode, weights in mode max, every rep weight 0 with a state gradient asked for: refused before any launch, by the
    wrapper and by the entry itself."""
    import ctypes as C
    from efficientvideoclassification_youtube8m_amd import _lib, ops
    inp, dv, want, w, r = _case((1, 5, 3), 1, "mean")
    p, s = dv["preds_t"][0], dv["states_t"][0]
    losses = torch.zeros(4, dtype=torch.float32, device=DEV)
    args = (dv["labels"], dv["pred_s"], dv["state_s"], losses)
    for J in (0, 9):
        with pytest.raises(ValueError, match="teachers"):
            ops.distill_losses_ensemble([p] * J, [s] * J, *args)
    with pytest.raises(ValueError, match="mode"):
        ops.distill_losses_ensemble([p], [s], *args, mode="median")
    with pytest.raises(ValueError, match="mean"):
        ops.distill_losses_ensemble([p], [s], *args, mode="max", weights=[1.0])
    with pytest.raises(ValueError, match="rep_weight"):
        ops.distill_losses_ensemble([p], [s], *args, rep_weights=[0.0], dstate_s=torch.empty_like(dv["state_s"]))
    ws = torch.empty(64 * 12 + 256, dtype=torch.float32, device=DEV)
    ptrs = (C.c_void_p * 9)(*[p.data_ptr()] * 9)
    sts = (C.c_void_p * 9)(*[s.data_ptr()] * 9)
    ones = (C.c_float * 9)(*[1.0] * 9)
    zeros = (C.c_float * 9)(*[0.0] * 9)

    def entry(J, mode, rw=ones, g_rep=1.0, ds=None):
        _lib.call("evc_distill_losses_ensemble", J, ptrs, sts, ones, rw, mode, dv["labels"].data_ptr(), dv["pred_s"].data_ptr(),
                  dv["state_s"].data_ptr(), 1, 5, 3, 1.0, 1.0, g_rep, losses.data_ptr(), None, None, None, ds, ws.data_ptr(), None)

    for J, mode, kw in ((0, 1, {}), (9, 1, {}), (1, 2, {}), (1, -1, {}), (2, 1, dict(rw=zeros)),
                        (2, 1, dict(rw=zeros, g_rep=0.0, ds=ws.data_ptr()))):
        with pytest.raises(_lib.EvcError):
            entry(J, mode, **kw)
    torch.cuda.synchronize()
    assert not losses.any()                                          # nothing was launched


@pytest.mark.parametrize("shape", [(3, 4716, 4096), (2, 1023, 100)])
def test_difference_to_the_composition_is_printed(shape):
    """ensemble_topk_rows(dense) then distill_losses_multi with K = 1 is compiled separately: its bits may differ.  Printed, not asserted."""
    from efficientvideoclassification_youtube8m_amd import ops
    inp, dv, want, w, _ = _case(shape, 2, "mean")
    sc = _scales(shape[0])
    out = _run(dv, "mean", w, [1.0, 0.0], sc)
    comb = ops.ensemble_topk_rows(dv["preds_t"], 0, mode="mean", weights=w, dense=True)[2]
    l1 = torch.zeros(1, 4, dtype=torch.float32, device=DEV)
    dp1, ds1 = torch.empty_like(dv["pred_s"]), torch.empty_like(dv["state_s"])
    ops.distill_losses_multi(comb, comb.sum(1), dv["labels"], dv["states_t"][0], [dv["pred_s"]], [dv["pred_s"].sum(1)], [dv["state_s"]], l1,
                             [dp1], [ds1], **sc)
    torch.cuda.synchronize()
    print("%s: ensemble - composition: losses %s, dpred max |diff| %.3g (max |dpred| %.3g), dstate max |diff| %.3g" % (
        shape, (out["losses"] - l1[0]).tolist(), float((out["dp"] - dp1).abs().max()), float(dp1.abs().max()),
        float((out["ds"] - ds1).abs().max())))
