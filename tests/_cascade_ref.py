"""numpy float32 restatement of the confidence cascade (include/evc.h: evc_cascade_confidence_rows, evc_cascade_pick_rows) and of the
stage loop of cascade.CascadeGraph.step, written from the documented semantics, not from the HIP.

confidence(row, kind)
    top1: the largest value of the row; margin: largest - second largest counting duplicates (one float32 subtraction), the second
    largest of a one-column row being 0.0f.  A row that holds a NaN gives NaN, and so does inf - inf.  Zeros: +0 ranks above -0 for the
    maximum (numpy leaves the sign of max(-0, +0) to the instruction it happens to use; the device follows IEEE 754-2019 `maximum`).
pick(conf, active, num_frames, threshold, max_rows)
    candidates = active rows for which conf >= threshold is false; with max_rows >= 0 and more candidates than that, the max_rows least
    confident: NaN first, then conf ascending with -0 = +0, then the lower row.
cascade(stage_preds, num_frames, kind, thresholds, fractions)
    the loop: stage k runs the active rows, their confidence / merged row / stage_of are written, the gate picks who goes on.
"""
import math

import numpy as np

NAN = np.float32(np.nan)


def confidence(row, kind):
    """One row's confidence as a float32 scalar."""
    row = np.asarray(row, np.float32)
    if np.isnan(row).any():
        return NAN
    s = np.sort(row)                                        # ascending; numpy sorts -0 and +0 as equals
    m1 = s[-1]
    if m1 == 0:                                             # the zero that is the maximum: +0 if the row holds one
        m1 = np.float32(0.0) if ((row == 0) & ~np.signbit(row)).any() else np.float32(-0.0)
    if kind == "top1":
        return np.float32(m1)
    assert kind == "margin", kind
    m2 = s[-2] if row.size > 1 else np.float32(0.0)
    with np.errstate(invalid="ignore"):
        return np.float32(np.float32(m1) - np.float32(m2))  # (the sign of a zero m1 / m2 never reaches a nonzero difference)


def confidence_rows(pred, kind, stage, conf, merged, stage_of, active=None):
    """In place, as the entry point: only the active rows of conf / merged / stage_of are written."""
    pred = np.asarray(pred, np.float32)
    for r in range(pred.shape[0]):
        if active is not None and not active[r]:
            continue
        conf[r] = confidence(pred[r], kind)
        merged[r, :pred.shape[1]] = pred[r]
        stage_of[r] = stage
    return conf


def order_key(c, r):
    """Least confident first: NaN, then the value with -0 = +0, then the row."""
    c = float(c)
    return (0, 0.0, r) if math.isnan(c) else (1, c + 0.0, r)      # -0.0 + 0.0 = +0.0; Python compares -0.0 == 0.0 anyway


def pick(conf, active, num_frames, threshold, max_rows=-1):
    """(active_next uint8 [rows], num_frames_next int32 [rows], count)."""
    conf = np.asarray(conf, np.float32)
    rows = conf.shape[0]
    thr = np.float32(threshold)
    with np.errstate(invalid="ignore"):
        cand = [r for r in range(rows) if (active is None or active[r]) and not (conf[r] >= thr)]
    if max_rows >= 0 and len(cand) > max_rows:
        cand = sorted(cand, key=lambda r: order_key(conf[r], r))[:max_rows]
    nxt = np.zeros(rows, np.uint8)
    nxt[cand] = 1
    nf = np.where(nxt != 0, np.asarray(num_frames, np.int32), 0).astype(np.int32)
    return nxt, nf, len(cand)


def quota(n_active, fraction, batch_rows):
    return -1 if fraction is None else min(n_active, int(math.ceil(float(fraction) * batch_rows)))


def cascade(stage_preds, num_frames, kind, thresholds=None, fractions=None):
    """stage_preds: K dense [b, V] float32 matrices, each what stage k's tower predicts for EVERY row of the batch (a row's prediction does
    not depend on which other rows are live).  Returns dict(merged [b, V], stage_of uint8 [b], confidence float32 [b], stage_rows [K])."""
    K = len(stage_preds)
    b, V = stage_preds[0].shape
    merged = np.zeros((b, V), np.float32)
    conf = np.zeros(b, np.float32)
    stage_of = np.zeros(b, np.uint8)
    active = None
    rows = [0] * K
    for k in range(K):
        n_active = b if active is None else int(active.sum())
        if n_active == 0:
            break
        rows[k] = n_active
        confidence_rows(stage_preds[k], kind, k, conf, merged, stage_of, active)
        if k == K - 1:
            break
        thr = float("inf") if thresholds is None else thresholds[k]
        active, _, _ = pick(conf, active, num_frames, thr, quota(n_active, None if fractions is None else fractions[k], b))
    return dict(merged=merged, stage_of=stage_of, confidence=conf, stage_rows=rows)
