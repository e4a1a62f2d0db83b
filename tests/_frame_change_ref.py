"""numpy restatement of the content-aware frame selection (include/evc.h: evc_frame_change_keys, evc_student_frame_select_scored), written
from the header's text and not imported from the product: the keys by int64 / float64 sums, the tables by np.lexsort and per-segment argmax."""
import numpy as np

STRATEGIES = ("change", "segment_change")
FIRST = np.uint32(0xFFFFFFFF)


def student_count(n, T, S):
    """int64(float64(n) / T * S): the student's frame count for a video of n <= T frames."""
    return int(np.trunc(np.float64(n) / np.float64(T) * np.float64(S)))


def keys_row(x, num_frames):
    """keys [T] uint32 of one video x [T][F] (uint8 or float32)."""
    T = x.shape[0]
    n = min(max(int(num_frames), 0), T)
    out = np.zeros(T, np.uint32)
    if n == 0:
        return out
    out[0] = FIRST
    if n > 1:
        if x.dtype == np.uint8:
            d = x[1:n].astype(np.int64) - x[:n - 1].astype(np.int64)
            out[1:n] = (d * d).sum(1).astype(np.uint32)                       # exact; fits while F <= 66051
        else:
            assert x.dtype == np.float32
            d = x[1:n].astype(np.float64) - x[:n - 1].astype(np.float64)
            with np.errstate(invalid="ignore", over="ignore"):
                s = (d * d).sum(1).astype(np.float32)
            out[1:n] = np.where(np.isnan(s), FIRST, s.view(np.uint32))
    return out


def keys(x, num_frames):
    return np.stack([keys_row(x[b], n) for b, n in enumerate(num_frames)])


def segments(n, k):
    """[(lo, hi)] of the k segments of [0, n)."""
    return [(j * n // k, (j + 1) * n // k) for j in range(k)]


def table_row(key, num_frames, T, every_n, strategy):
    """src [S] int32 of one video from its keys [T] uint32."""
    S = T // every_n
    n = min(max(int(num_frames), 0), T)
    k = student_count(n, T, S)
    out = np.full(S, -1, np.int32)
    key = np.asarray(key, np.uint32)[:n].astype(np.int64)
    if strategy == "change":
        order = np.lexsort((np.arange(n), -key))               # by descending key, then by ascending t
        out[:k] = np.sort(order[:k])
    elif strategy == "segment_change":
        for j, (lo, hi) in enumerate(segments(n, k)):
            out[j] = lo + int(np.argmax(key[lo:hi]))            # argmax: the first of the largest
    else:
        raise ValueError(strategy)
    return out


def table(keys_, num_frames, T, every_n, strategy):
    return np.stack([table_row(keys_[b], n, T, every_n, strategy) for b, n in enumerate(num_frames)])
