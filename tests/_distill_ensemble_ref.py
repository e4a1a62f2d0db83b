"""Reference of evc_distill_losses_ensemble's contract (include/evc.h): the J teachers are combined in numpy float32 exactly as the
kernel combines them (tests/_ensemble_ref.py restates the two modes; the state is the same left-to-right f32 sum), and the float64
reference of the single-teacher loss section (tests/_distill_losses_ref.reference) runs on the combined arrays.  No GPU, no package
import."""
import numpy as np

import _distill_losses_ref as base
import _ensemble_ref as ens

make_inputs = base.make_inputs


def default_weights(J):
    return ens.default_weights(J)


def default_rep_weights(J):
    return np.asarray([1.0] + [0.0] * (J - 1), np.float32)


def teachers(B, V, D, J):
    """Teacher j takes pred_t / state_t of make_inputs(B, V, D, seed=j)."""
    ins = [make_inputs(B, V, D, seed=j) for j in range(J)]
    return [i["pred_t"] for i in ins], [i["state_t"] for i in ins]


def combine_pred(preds, mode, weights=None):
    """The combined row: the bits of ensemble_topk_rows' dense output for these members without prior files."""
    return ens.combine(preds, mode, weights)


def combine_state(states, rep_weights):
    """r_j state_j summed left to right in float32 over the entries with r_j != 0 (an entry with r_j == 0 is not read: it may be None)."""
    r = np.asarray(rep_weights, np.float32)
    acc = None
    for rj, s in zip(r, states):
        if rj == 0:
            continue
        prod = rj * np.ascontiguousarray(s, np.float32)
        acc = prod if acc is None else acc + prod
    assert acc is None or acc.dtype == np.float32
    return acc


def combined_inputs(inp, preds, states, mode, weights=None, rep_weights=None):
    """``inp`` (labels, pred_s, state_s of make_inputs) with pred_t / state_t replaced by the combination of the J teachers."""
    J = len(preds)
    r = default_rep_weights(J) if rep_weights is None else rep_weights
    st = combine_state(states, r)
    if st is None:
        st = np.zeros_like(inp["state_s"])
    return dict(inp, pred_t=combine_pred(preds, mode, weights), state_t=st)


def reference(inp, preds, states, mode, weights, rep_weights, g_ce, g_kl, g_rep):
    """_distill_losses_ref.reference on the combined arrays, plus "teacher_ce": each teacher's own CE in float64."""
    from oracle import model_math as mm
    comb = combined_inputs(inp, preds, states, mode, weights, rep_weights)
    out = base.reference(comb, g_ce, g_kl, g_rep)
    y = inp["labels"].astype(np.float64)
    out["teacher_ce"] = np.array([mm.cross_entropy_loss(p.astype(np.float64), y) for p in preds])
    out["pred_comb"], out["state_comb"] = comb["pred_t"], comb["state_t"]
    return out
