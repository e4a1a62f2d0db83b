"""Reference of evc_distill_losses_sparse's contract (include/evc.h): the F sparse lists are scattered into a dense row in numpy float32
exactly as evc_ensemble_topk_rows scatters prior files over ONE all-zero member (tests/_ensemble_ref.combine, weights [0] + w), and the
float64 reference of the single-teacher loss section (tests/_distill_losses_ref.reference, g_rep = 0) runs on that row.

A scattered row holds exact zeros, which the dense reference was never written for: its L_PRED is sum P (log P - log Q), NaN at P = 0,
and a row no list names is 0 / 0.  Both are defined by the contract - 0 log 0 = 0, and a row whose sum is below FLT_MIN contributes
L_PRED 0 and a KL gradient of exactly 0 - so L_PRED's value and the KL terms of such rows are restated here in float64 with those two
rules; everything else is the dense reference's.  No GPU, no package import."""
import numpy as np

import _distill_losses_ref as base
import _ensemble_ref as ens

# (B, V, kp, F)
CASES = [(1, 5, 1, 1), (1, 5, 3, 3),              # the smallest
         (2, 1023, 20, 2),                        # V not a multiple of 4: the scalar paths
         (3, 4716, 20, 1), (3, 4716, 256, 8),     # the real V; the maximum kp and F
         (1030, 8, 4, 2),                         # the finish launch with more than one piece of 1024
         (2, 32768, 7, 2)]                        # the LDS limit
MODES = ("mean", "max")
FLT_MIN = float(np.finfo(np.float32).tiny)


def weights(F, mode):
    """Non-uniform weights that sum to 1 in mode mean (the combined row stays a probability); None in mode max, where none are read."""
    if mode == "max":
        return None
    w = np.arange(1, F + 1, dtype=np.float32)
    return (w / w.sum()).astype(np.float32)


def make_case(B, V, kp, F):
    """labels and pred_s of _distill_losses_ref.make_inputs; lists of _ensemble_ref.random_priors (0 .. kp entries per file and row,
    confidences in (0, 1), the files overlapping), with the conditions the tests name planted:
      row 0: a non-empty list in file 0, and with F >= 2 its first class also FIRST in file 1 (a class listed by several files);
      a padding entry in the middle of a list (index -1 with a non-zero confidence behind it, which nothing may read) where kp >= 3;
      with B >= 2: the last row all padding in every file."""
    inp = base.make_inputs(B, V, 1)
    rng = np.random.default_rng(77 + B * 131 + V * 7 + kp * 3 + F)
    idx, val = ens.random_priors(rng, F, B, kp, V, low=1e-6, high=1 - 1e-6)
    if idx[0, 0, 0] < 0:
        idx[0, 0, 0], val[0, 0, 0] = V // 2, np.float32(0.5)
    if F >= 2:
        c = idx[0, 0, 0]
        dup = np.flatnonzero(idx[1, 0] == c)
        if dup.size:                                   # already in file 1: swap it to the front
            j = int(dup[0])
            idx[1, 0, [0, j]], val[1, 0, [0, j]] = idx[1, 0, [j, 0]], val[1, 0, [j, 0]]
        else:
            idx[1, 0, 0], val[1, 0, 0] = c, np.float32(0.25)
    if kp >= 3:
        for p in range(F):                             # the first row of every file with three entries or more
            rows = np.flatnonzero((idx[p] >= 0).sum(axis=1) >= 3)
            if rows.size:
                idx[p, rows[0], 1], val[p, rows[0], 1] = -1, np.float32(0.7)
    if B >= 2:
        idx[:, B - 1, :] = -1
    for p in range(F):
        for b in range(B):
            c = idx[p, b][idx[p, b] >= 0]
            assert np.unique(c).size == c.size and (c < V).all()
    return dict(labels=inp["labels"], pred_s=inp["pred_s"], idx=idx, val=val)


def scatter(idx, val, V, mode, w=None):
    """The combined row [B, V] float32: the bits of ensemble_topk_rows' dense output for one all-zero member plus these files."""
    zeros = np.zeros((idx.shape[1], V), np.float32)
    full = None if mode == "max" else np.concatenate([np.zeros(1, np.float32), np.asarray(w, np.float32)])
    return ens.combine([zeros], mode, weights=full, priors=(idx, val))


def reference(case, mode, w, g_ce, g_kl):
    """{"losses" [4] (slot 1 = 0), "ce", "kl" (the gradient terms), "pred_comb"} in float64 on the f32 inputs."""
    B, V = case["pred_s"].shape
    P = scatter(case["idx"], case["val"], V, mode, w)
    one = np.zeros((B, 1), np.float32)
    inp = dict(pred_t=P, pred_s=case["pred_s"], labels=case["labels"], state_t=one, state_s=one)
    out = base.reference(inp, g_ce, g_kl, 0.0)
    pt, ps = P.astype(np.float64), case["pred_s"].astype(np.float64)
    sums = pt.sum(axis=1, keepdims=True)
    ok = sums[:, 0] >= FLT_MIN
    Pn = np.where(ok[:, None], pt / np.where(ok[:, None], sums, 1.0), 0.0)
    sq = ps.sum(axis=1, keepdims=True)
    Q = ps / sq
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = np.where(Pn > 0, Pn * (np.log(np.where(Pn > 0, Pn, 1.0)) - np.log(Q)), 0.0)
    out["losses"] = np.array([out["losses"][0], 0.0, terms.sum(), out["losses"][3]])
    out["kl"] = np.where(ok[:, None], g_kl * (-Pn / ps + 1.0 / sq), 0.0)
    out["pred_comb"] = P
    out.pop("kl_parts", None)
    out.pop("rep", None)
    return out
