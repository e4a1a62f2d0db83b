"""numpy restatement of evc_eval_select_rows (ops.eval_select_rows), shared by test_cpu_eval_select.py (as the stand-in for the
kernel in front of EvaluationMetrics.accumulate_selected) and test_gpu_eval_select.py (as the kernel's reference)."""
import numpy as np


def canonical_keys(x):
    """The order as unsigned keys (larger ranks first): -0 == +0, every NaN above +inf, otherwise IEEE order."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).copy()
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    u[u == 0x80000000] = 0
    key = np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)
    key[nan] = 0xFFFFFFFF
    return key


def reference_order(x):
    """np.lexsort on the column index, then on the canonicalised value descending: the full order of every row."""
    col = np.broadcast_to(np.arange(x.shape[1]), x.shape)
    return np.lexsort((col, -canonical_keys(x).astype(np.int64)), axis=-1)


def eval_select_rows(x, labels, k, order=None):
    """x [B, C] f32, labels [B, C] (nonzero = positive) -> the dict ops.eval_select_rows returns, as numpy arrays.
    order: reference_order(x), when the caller has it already."""
    x = np.ascontiguousarray(x, np.float32)
    on = np.asarray(labels) != 0
    cols = x.shape[1]
    if order is None:
        order = reference_order(x)
    top_idx = order[:, :k].astype(np.int32)
    n_pos = on.sum(axis=1).astype(np.int32)
    with np.errstate(invalid="ignore"):
        hit = np.take_along_axis(on, order, 1) & (np.take_along_axis(x, order, 1) > 0)       # NaN > 0 is False
    hit &= np.arange(cols)[None, :] < n_pos[:, None]                                          # the first n_pos columns of the order
    return {"top_val": np.take_along_axis(x, top_idx, 1), "top_idx": top_idx,
            "top_lab": np.take_along_axis(on, top_idx, 1).astype(np.uint8), "n_pos": n_pos,
            "perr_hits": hit.sum(axis=1).astype(np.int32), "class_pos": on.sum(axis=0).astype(np.int32)}


def boundary_ties(x, labels, k):
    """Rows where np.argpartition and the device may select differently: (rows with an exact tie across the k-th / (k+1)-th
    place, rows with a tie at a value > 0 across the n_pos-th / (n_pos+1)-th place)."""
    x = np.ascontiguousarray(x, np.float32)
    cols = x.shape[1]
    order = reference_order(x)
    key, val = np.take_along_axis(canonical_keys(x), order, 1), np.take_along_axis(x, order, 1)
    n_pos = (np.asarray(labels) != 0).sum(axis=1)
    at_k = np.nonzero(key[:, k - 1] == key[:, k])[0] if k < cols else np.zeros(0, np.int64)
    at_n = [r for r, n in enumerate(n_pos) if 0 < n < cols and key[r, n - 1] == key[r, n] and val[r, n - 1] > 0]
    return at_k, np.asarray(at_n, np.int64)
