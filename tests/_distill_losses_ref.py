"""float64 restatement of evc_distill_losses' contract (include/evc.h) from the oracle's loss functions, and the inputs the
kernel test runs on.  No GPU, no package import: numpy and oracle.model_math only."""
import numpy as np

from oracle import model_math as mm

SHAPES = [(1, 5, 3), (3, 4716, 4096), (5, 40, 128), (2, 1023, 100), (7, 257, 4)]      # (B, V, D)
PLANTED = (1e-7, 1 - 1e-7, 0.5)


def make_inputs(B, V, D, seed=0):
    """f32 probabilities uniform in [1e-6, 1 - 1e-6] with PLANTED in the first three entries of row 0 (teacher and student), ~10 %
    positive labels, row sums computed in f32, states ~ N(0, 1)."""
    rng = np.random.default_rng(1000 * seed + B * 131 + V * 7 + D)
    out = {}
    for k in ("pred_t", "pred_s"):
        p = rng.uniform(1e-6, 1 - 1e-6, (B, V)).astype(np.float32)
        p[0, :3] = np.asarray(PLANTED, np.float32)
        out[k] = p
    out["labels"] = (rng.random((B, V)) < 0.1).astype(np.uint8)
    out["rowsum_t"] = out["pred_t"].sum(axis=1, dtype=np.float32)
    out["rowsum_s"] = out["pred_s"].sum(axis=1, dtype=np.float32)
    out["state_t"] = rng.standard_normal((B, D)).astype(np.float32)
    out["state_s"] = rng.standard_normal((B, D)).astype(np.float32)
    return out


def reference(inp, g_ce, g_kl, g_rep):
    """The four loss values (LOSS_SLOTS order) and the gradient TERMS in float64 on the f32 inputs.

    evc.h: dpred_s = g_ce d(sum_b CE_s) + g_kl dL_PRED, g_ce carrying the caller's 1/B - mm.cross_entropy_grad is the gradient of the
    batch MEAN, hence the factor B -; dstate_s = g_rep dL_REP (the mean's 1/B inside, as in mm.rep_loss_grad_student).
    kl_parts: the magnitudes of the two addends of the KL gradient, P/p_s and 1/sum(p_s), whose difference cancels."""
    pt, ps = inp["pred_t"].astype(np.float64), inp["pred_s"].astype(np.float64)
    y = inp["labels"].astype(np.float64)
    st, ss = inp["state_t"].astype(np.float64), inp["state_s"].astype(np.float64)
    B = pt.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        losses = np.array([mm.cross_entropy_loss(pt, y), mm.rep_loss(st, ss), mm.pred_kl_loss(pt, ps), mm.cross_entropy_loss(ps, y)])
        kl = g_kl * mm.pred_kl_grad_student(pt, ps)
        P = pt / pt.sum(axis=1, keepdims=True)
        kl_parts = abs(g_kl) * (P / ps + 1.0 / ps.sum(axis=1, keepdims=True))
    return {"losses": losses, "ce": g_ce * B * mm.cross_entropy_grad(ps, y), "kl": kl, "kl_parts": kl_parts,
            "rep": g_rep * mm.rep_loss_grad_student(st, ss)}
