"""evc_distill_losses_multi (ops.distill_losses_multi): the loss section of the serial distillation step for K students against one
teacher in one launch + its finish, against float64 (tests/_distill_losses_ref.py).  pytest -m gpu.

Inputs: teacher, labels and student 0 are make_inputs(B, V, D); student k > 0 takes pred_s, rowsum_s and state_s of
make_inputs(B, V, D, seed=k); the float64 reference of student k is reference() on the teacher's arrays with student k's.

Bounds: those of test_gpu_distill_losses.py, unchanged and for every student alike - gradients elementwise, no element exempt:
|got - ref| <= 1e-5 (|ce term| + |kl term|) for dpred, 1e-5 |rep term| for dstate (a KL gradient standing alone: 1e-5 of the magnitudes
of its two addends); loss values 1e-4 relative.  Output buffers are NaN-filled first: an unwritten element fails.
Bit-independence (torch.equal): a student's outputs in a K = 3 launch are those of a K = 1 launch on it alone, at any position.

(1030, 8, 4) is the hard case for dpred: few classes under a large batch.  The KL gradient's two addends, -P/p_s and 1/sum(p_s), are
~0.25 each and cancel, next to a CE term of ~1e-3 (its 1/B): the bound is ~1e-8 there, below one f32 rounding of an addend or of a
row sum handed in as f32 (correctly rounded f32 arithmetic gives 2.376 of the bound, exact arithmetic on f32 row sums 1.287).  The
kernel therefore takes the row sums and this one difference in double, which is worth 0.013 of the bound in IEEE arithmetic."""
import numpy as np
import pytest
import torch

import _distill_losses_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL_GRAD, RTOL_LOSS = 1e-5, 1e-4
# (B, V, D), K
CASES = [((1, 5, 3), 1), ((1, 5, 3), 3),          # the smallest case
         ((2, 1023, 100), 2),                     # V and B * D not multiples of 4: the scalar paths
         ((7, 257, 4), 8),                        # the maximum K
         ((3, 4716, 4096), 3),                    # the real V and D
         ((1030, 8, 4), 2),                       # the finish launch with more than one piece of 1024
         ((70, 12, 4096), 2)]                     # NS = 256 and a partial second grid-stride trip of the state part
_CACHE = {}


def _scales(B, k):
    """Per-student scales that differ within a launch: student 0 the serial step's (all terms), student 1 without its CE, student 2
    its CE alone, the others varied weights."""
    full = dict(g_ce=1.0 / B, g_kl=1.0, g_rep=2.0)
    if k == 1:
        return dict(full, g_ce=0.0)
    if k == 2:
        return dict(full, g_kl=0.0, g_rep=0.0)
    if k >= 3:
        return dict(g_ce=(1.0 + k) / B, g_kl=0.5 * k, g_rep=1.0 / k)
    return full


def _case(shape, K):
    """Host inputs, device tensors and the float64 references of the first K students of one shape; computed once, never modified."""
    B, V, D = shape
    for k in range(K):
        if (shape, k) in _CACHE:
            continue
        inp = ref.make_inputs(B, V, D, seed=k)
        if k > 0:
            base = _CACHE[(shape, 0)][0]
            inp = dict(base, pred_s=inp["pred_s"], rowsum_s=inp["rowsum_s"], state_s=inp["state_s"])
        dv = {n: torch.from_numpy(v).to(DEV) for n, v in inp.items()}
        _CACHE[(shape, k)] = (inp, dv, ref.reference(inp, **_scales(B, k)))
    return [_CACHE[(shape, k)] for k in range(K)]


def _run(students, scales, want_dp=True, want_ds=True, rowsum_t=None, pred_t=None, dps=None, losses=None):
    """students: list of device dicts (the teacher's arrays are taken from the first), scales: list of dicts.  want_dp / want_ds: a bool
    for all or a list per student."""
    from efficientvideoclassification_youtube8m_amd import ops
    K = len(students)
    t = students[0]
    want_dp = [want_dp] * K if isinstance(want_dp, bool) else want_dp
    want_ds = [want_ds] * K if isinstance(want_ds, bool) else want_ds
    if losses is None:
        losses = torch.zeros(K, 4, dtype=torch.float32, device=DEV)
    if dps is None:
        dps = [torch.full_like(s["pred_s"], float("nan")) if w else None for s, w in zip(students, want_dp)]
    dss = [torch.full_like(s["state_s"], float("nan")) if w else None for s, w in zip(students, want_ds)]
    ops.distill_losses_multi(t["pred_t"] if pred_t is None else pred_t, t["rowsum_t"] if rowsum_t is None else rowsum_t, t["labels"],
                             t["state_t"], [s["pred_s"] for s in students], [s["rowsum_s"] for s in students],
                             [s["state_s"] for s in students], losses, dps, dss, g_ce=[s["g_ce"] for s in scales],
                             g_kl=[s["g_kl"] for s in scales], g_rep=[s["g_rep"] for s in scales])
    torch.cuda.synchronize()
    return losses, dps, dss


def _check(got, want, bound, what):
    """Prints the figure, then returns the list of misses (empty: within the bound everywhere) for the caller to assert on."""
    err = np.abs(got.double().cpu().numpy() - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    over = int((err > bound).sum())
    print("%s: worst error %.3g of its bound, %d of %d elements over it" % (what, worst, over, err.size))
    return [] if over == 0 else [(what, worst, over)]


def _check_student(losses_k, dp, ds, want, sc, what):
    """One student against its float64 reference under its scales; a term whose scale is 0 is absent and the other stands alone."""
    got_l = losses_k.double().cpu().numpy()
    print(what, "losses", got_l, "ref", want["losses"])
    missed = []
    if not np.all(np.abs(got_l - want["losses"]) <= RTOL_LOSS * np.abs(want["losses"])):
        missed.append(("losses " + what, got_l, want["losses"]))
    ce, kl = want["ce"], want["kl"]                                   # already scaled: 0 where the scale is 0
    kl_bound = np.abs(kl) if sc["g_ce"] != 0.0 else want["kl_parts"]
    missed += _check(dp, ce + kl, RTOL_GRAD * (np.abs(ce) + kl_bound), "dpred " + what)
    missed += _check(ds, want["rep"], RTOL_GRAD * np.abs(want["rep"]), "dstate " + what)
    if sc["g_rep"] == 0.0 and ds.any():
        missed.append(("dstate not exactly 0 " + what,))
    if sc["g_ce"] == 0.0 and sc["g_kl"] == 0.0 and dp.any():
        missed.append(("dpred not exactly 0 " + what,))
    return missed


@pytest.mark.parametrize("shape,K", CASES)
def test_losses_and_gradients_against_float64_per_student(shape, K):
    cases = _case(shape, K)
    scales = [_scales(shape[0], k) for k in range(K)]
    losses, dps, dss = _run([c[1] for c in cases], scales)
    missed = []
    for k in range(K):
        missed += _check_student(losses[k], dps[k], dss[k], cases[k][2], scales[k], "%s K=%d student %d" % (shape, K, k))
    for k in range(1, K):
        assert torch.equal(losses[k, 0], losses[0, 0])               # the teacher's CE: the same bits in every row
    assert not missed, missed


@pytest.mark.parametrize("shape,K", CASES)
def test_all_zero_scales_give_exact_zeros_and_the_same_losses(shape, K):
    cases = _case(shape, K)
    students = [c[1] for c in cases]
    base = _run(students, [_scales(shape[0], k) for k in range(K)])[0]
    zero = dict(g_ce=0.0, g_kl=0.0, g_rep=0.0)
    scales = [zero if k % 2 == 0 else _scales(shape[0], 0) for k in range(K)]       # the zeros next to a student with every term
    losses, dps, dss = _run(students, scales)
    assert torch.equal(losses, base)                                 # the values do not depend on the scales
    for k in range(0, K, 2):
        assert not dps[k].any() and not dss[k].any()                 # exactly 0, every element written (the buffers were NaN-filled)


@pytest.mark.parametrize("shape,K", [c for c in CASES if c[1] >= 2])
def test_a_students_bits_do_not_depend_on_its_company(shape, K):
    """K = 1 launches against the entries of the K-student launch, the list permuted, two identical calls."""
    cases = _case(shape, K)
    students = [c[1] for c in cases]
    scales = [_scales(shape[0], k) for k in range(K)]
    together = _run(students, scales)
    again = _run(students, scales)
    for x, y in zip(together[1] + together[2] + [together[0]], again[1] + again[2] + [again[0]]):
        assert torch.equal(x, y)
    for k in range(K):
        # student k alone: it needs the teacher's arrays, which every device dict carries
        l1, dp1, ds1 = _run([students[k]], [scales[k]])
        assert torch.equal(l1[0], together[0][k]), ("losses", k)
        assert torch.equal(dp1[0], together[1][k]), ("dpred", k)
        assert torch.equal(ds1[0], together[2][k]), ("dstate", k)
    perm = list(range(K))[::-1] if K == 2 else [(k + 1) % K for k in range(K)]
    lp, dpp, dsp = _run([students[k] for k in perm], [scales[k] for k in perm])
    for pos, k in enumerate(perm):
        assert torch.equal(lp[pos], together[0][k]) and torch.equal(dpp[pos], together[1][k]) and torch.equal(dsp[pos], together[2][k]), (pos, k)


@pytest.mark.parametrize("shape,K", [((1, 5, 3), 3), ((2, 1023, 100), 2), ((3, 4716, 4096), 3)])
def test_teacher_row_with_sum_zero(shape, K):
    """A collapsed teacher row (sum 0 < FLT_MIN): everything finite, every student's KL gradient on that row exactly 0."""
    cases = _case(shape, K)
    students = [c[1] for c in cases]
    B = shape[0]
    r = B - 1
    pt = students[0]["pred_t"].clone()
    pt[r] = 0.0
    rs = students[0]["rowsum_t"].clone()
    rs[r] = 0.0
    full = [dict(g_ce=1.0 / B, g_kl=1.0 + k, g_rep=2.0) for k in range(K)]
    losses, both, dss = _run(students, full, rowsum_t=rs, pred_t=pt)
    assert torch.isfinite(losses).all()
    for k in range(K):
        assert torch.isfinite(both[k]).all() and torch.isfinite(dss[k]).all()
        ce = cases[k][2]["ce"][r] * (full[k]["g_ce"] / _scales(B, k)["g_ce"]) if _scales(B, k)["g_ce"] else None
        if ce is not None:                                            # = the CE term alone: KL adds exactly 0
            assert not _check(both[k][r], ce, RTOL_GRAD * np.abs(ce), "dpred of the degenerate row %s student %d" % (shape, k))
    alone = _run(students, [dict(s, g_kl=0.0) for s in full], want_ds=False, rowsum_t=rs, pred_t=pt)[1]
    for k in range(K):
        assert torch.equal(both[k][r], alone[k][r]), k               # bit for bit: the row's KL gradient is 0, not small


def test_a_misaligned_student_next_to_aligned_ones():
    """(3, 4716, 4096): student 1's pred_s and dpred_s start 4 bytes into their allocations; the same bounds for every student."""
    shape, K = (3, 4716, 4096), 3
    cases = _case(shape, K)
    B, V, D = shape
    students = [dict(c[1]) for c in cases]
    buf = torch.empty(B * V + 1, dtype=torch.float32, device=DEV)
    shifted = buf[1:].view(B, V)
    shifted.copy_(students[1]["pred_s"])
    students[1]["pred_s"] = shifted
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    dbuf = torch.full((B * V + 1,), float("nan"), dtype=torch.float32, device=DEV)
    dps = [torch.full((B, V), float("nan"), dtype=torch.float32, device=DEV), dbuf[1:].view(B, V),
           torch.full((B, V), float("nan"), dtype=torch.float32, device=DEV)]
    assert dps[1].data_ptr() % 16 == 4
    scales = [_scales(B, k) for k in range(K)]
    losses, dps, dss = _run(students, scales, dps=dps)
    missed = []
    for k in range(K):
        missed += _check_student(losses[k], dps[k], dss[k], cases[k][2], scales[k], "%s misaligned student 1, student %d" % (shape, k))
    assert not missed, missed
    assert torch.isnan(dbuf[0])                                      # nothing written in front of the view
    # the aligned students' bits are those of the all-aligned launch
    ref_run = _run([c[1] for c in cases], scales)
    for k in (0, 2):
        assert torch.equal(dps[k], ref_run[1][k]) and torch.equal(dss[k], ref_run[2][k]) and torch.equal(losses[k], ref_run[0][k])


@pytest.mark.parametrize("shape,K", [((1, 5, 3), 3), ((3, 4716, 4096), 3), ((2, 1023, 100), 2)])
def test_null_gradients_for_one_student_leave_the_rest_bit_identical(shape, K):
    cases = _case(shape, K)
    students = [c[1] for c in cases]
    scales = [_scales(shape[0], k) for k in range(K)]
    base = _run(students, scales)
    for which in ("dp", "ds", "both"):
        want_dp = [not (k == 1 and which in ("dp", "both")) for k in range(K)]
        want_ds = [not (k == 1 and which in ("ds", "both")) for k in range(K)]
        losses, dps, dss = _run(students, scales, want_dp=want_dp, want_ds=want_ds)
        assert torch.equal(losses, base[0]), which
        for k in range(K):
            assert (dps[k] is None and not want_dp[k]) or torch.equal(dps[k], base[1][k]), (which, k)
            assert (dss[k] is None and not want_ds[k]) or torch.equal(dss[k], base[2][k]), (which, k)
    losses = _run(students, scales, want_dp=False, want_ds=False)[0]
    assert torch.equal(losses, base[0])


def test_losses_accumulate():
    """losses[k][i] += value: a second call on the same buffer doubles every slot."""
    shape, K = (7, 257, 4), 8
    cases = _case(shape, K)
    students = [c[1] for c in cases]
    scales = [_scales(shape[0], k) for k in range(K)]
    once = _run(students, scales, want_dp=False, want_ds=False)[0]
    losses = torch.zeros(K, 4, dtype=torch.float32, device=DEV)
    for _ in range(2):
        _run(students, scales, want_dp=False, want_ds=False, losses=losses)
    assert torch.equal(losses, 2 * once)                             # x + x is exact


def test_k_outside_1_to_8_is_refused():
    from efficientvideoclassification_youtube8m_amd import ops
    cases = _case((1, 5, 3), 1)
    s = cases[0][1]
    for K in (0, 9):
        with pytest.raises(ValueError, match="students"):
            ops.distill_losses_multi(s["pred_t"], s["rowsum_t"], s["labels"], s["state_t"], [s["pred_s"]] * K, [s["rowsum_s"]] * K,
                                     [s["state_s"]] * K, torch.zeros(max(K, 1), 4, dtype=torch.float32, device=DEV))


@pytest.mark.parametrize("shape", [(3, 4716, 4096), (2, 1023, 100)])
def test_difference_to_the_single_student_entry_is_printed(shape):
    """evc_distill_losses is compiled separately: its bits may differ.  Printed, not asserted."""
    from efficientvideoclassification_youtube8m_amd import ops
    inp, dv, want = _case(shape, 1)[0]
    sc = _scales(shape[0], 0)
    losses, dps, dss = _run([dv], [sc])
    l1 = torch.zeros(4, dtype=torch.float32, device=DEV)
    dp1, ds1 = torch.empty_like(dv["pred_s"]), torch.empty_like(dv["state_s"])
    ops.distill_losses(dv["pred_t"], dv["rowsum_t"], dv["pred_s"], dv["rowsum_s"], dv["labels"], dv["state_t"], dv["state_s"], l1, dp1, ds1, **sc)
    torch.cuda.synchronize()
    print("%s: multi - single: losses %s, dpred max |diff| %.3g (max |dpred| %.3g), dstate max |diff| %.3g" % (
        shape, (losses[0] - l1).tolist(), float((dps[0] - dp1).abs().max()), float(dp1.abs().max()), float((dss[0] - ds1).abs().max())))
