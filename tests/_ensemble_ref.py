"""numpy restatement of evc_ensemble_topk_rows (ops.ensemble_topk_rows) for the tests: both combinations in np.float32 arithmetic with
one rounding per operation, the selection in the total order of tests/test_gpu_topk.py's reference, and the sparse merge of
cs/max_ensemble.py:21-36 (union of the files' lists, per-class maximum, sort, first k) written from its description."""
import numpy as np


def canonical_keys(x):
    """The order as unsigned keys (larger ranks first): -0 == +0, every NaN above +inf, otherwise IEEE order."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).copy()
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    u[u == 0x80000000] = 0
    key = np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)
    key[nan] = 0xFFFFFFFF
    return key


def combine_max(members, priors=None):
    """Per element the member value with the largest key, the lowest member on equal keys (the bits travel as uint32, so a NaN keeps
    its payload); then the prior files in order: row[c] = val where key(val) > key(row[c]).  priors: (idx [P, B, kp], val [P, B, kp]),
    idx < 0 = padding."""
    best = np.ascontiguousarray(members[0], np.float32).view(np.uint32).copy()
    bk = canonical_keys(members[0])
    for x in members[1:]:
        km = canonical_keys(x)
        take = km > bk
        best[take] = np.ascontiguousarray(x, np.float32).view(np.uint32)[take]
        bk[take] = km[take]
    if priors is not None:
        idx, val = priors
        for p in range(idx.shape[0]):
            for b in range(idx.shape[1]):
                on = idx[p, b] >= 0
                c, v = idx[p, b][on], np.ascontiguousarray(val[p, b][on], np.float32)
                take = canonical_keys(v) > bk[b, c]
                best[b, c[take]] = v.view(np.uint32)[take]
                bk[b, c[take]] = canonical_keys(v)[take]
    return best.view(np.float32)


def combine_mean(members, weights, priors=None):
    """acc = w[0] x_0; acc = acc + w[m] x_m, m ascending; acc = acc + w[M + p] val for the classes file p lists, p ascending.  numpy
    rounds every float32 product and every float32 sum on its own."""
    w = np.asarray(weights, np.float32)
    M = len(members)
    assert w.size == M + (0 if priors is None else priors[0].shape[0])
    acc = w[0] * np.ascontiguousarray(members[0], np.float32)
    assert acc.dtype == np.float32
    for m in range(1, M):
        prod = w[m] * np.ascontiguousarray(members[m], np.float32)
        acc = acc + prod
    if priors is not None:
        idx, val = priors
        for p in range(idx.shape[0]):
            for b in range(idx.shape[1]):
                on = idx[p, b] >= 0
                c = idx[p, b][on]
                prod = w[M + p] * np.ascontiguousarray(val[p, b][on], np.float32)
                acc[b, c] = acc[b, c] + prod                         # classes distinct within a list: a plain gather / scatter
    assert acc.dtype == np.float32
    return acc


def default_weights(M, P=0):
    return np.full(M + P, np.float32(1) / np.float32(M + P), np.float32)


def combine(members, mode, weights=None, priors=None):
    if mode == "max":
        return combine_max(members, priors)
    P = 0 if priors is None else priors[0].shape[0]
    return combine_mean(members, default_weights(len(members), P) if weights is None else weights, priors)


def topk(x, k):
    """(values [B, k], indices [B, k] int32): value descending in the total order, column ascending on ties; the values are x's bits."""
    col = np.broadcast_to(np.arange(x.shape[1]), x.shape)
    order = np.lexsort((col, -canonical_keys(x).astype(np.int64)), axis=-1)[:, :k].astype(np.int32)
    return np.take_along_axis(x, order, 1), order


def sparse_merge(lists, k):
    """cs/max_ensemble.py for one video: lists = the (classes, confidences) of every file; the union of the classes, each with the
    largest confidence any file gives it, sorted by confidence descending, the first k.  Returns (classes, confidences)."""
    merged = {}
    for classes, confs in lists:
        for c, v in zip(np.asarray(classes).tolist(), np.asarray(confs, np.float32)):
            if c not in merged or v > merged[c]:
                merged[c] = v
    ranked = sorted(merged.items(), key=lambda cv: cv[1], reverse=True)[:k]
    return np.asarray([c for c, _ in ranked], np.int32), np.asarray([v for _, v in ranked], np.float32)


def random_priors(rng, P, B, kp, cols, pool=None, low=0.0, high=1.0):
    """Lists for the tests: per (file, row) between 0 and kp entries, classes distinct within a list and drawn from a small pool so
    that the files overlap; shorter lists padded with idx = -1."""
    pool = min(cols, max(kp + 3, 2 * kp)) if pool is None else pool
    classes = rng.choice(cols, size=pool, replace=False)
    idx = np.full((P, B, kp), -1, np.int32)
    val = np.zeros((P, B, kp), np.float32)
    for p in range(P):
        for b in range(B):
            n = int(rng.integers(0, min(kp, pool) + 1))
            idx[p, b, :n] = rng.choice(classes, size=n, replace=False)
            val[p, b, :n] = rng.uniform(low, high, n).astype(np.float32)
    return idx, val
