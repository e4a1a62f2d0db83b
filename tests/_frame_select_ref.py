"""numpy restatement of the student's frame-selection table (include/evc.h: evc_student_frame_select), written from the header's text and
not imported from the product: the hash in np.uint32 arithmetic, the selection by sorting (key, t) pairs."""
import numpy as np

STRATEGIES = ("uniform", "first", "middle", "last", "first_middle_last", "random")


def _fmix(h):
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def frame_keys(seed, draw, row, n):
    """key(t) for t in [0, n): uint32 [n]."""
    with np.errstate(over="ignore"):
        h = _fmix(np.uint32(seed & 0xFFFFFFFF) * np.uint32(0x9E3779B1) + np.uint32(draw & 0xFFFFFFFF))
        h = _fmix(h ^ (np.uint32(row & 0xFFFFFFFF) * np.uint32(0x85EBCA77)))
        t = np.arange(n, dtype=np.uint32)
        return _fmix(h ^ (t * np.uint32(0xC2B2AE3D)))


def student_count(n, T, S):
    """int64(float64(n) / T * S): the student's frame count for a video of n <= T frames (cs/train.py:263-264)."""
    return int(np.trunc(np.float64(n) / np.float64(T) * np.float64(S)))


def fml_runs(n, k):
    """(start, length) of the three runs of first_middle_last."""
    kf, km, kl = (k + 2) // 3, (k + 1) // 3, k // 3
    ms = min(max((n - km) // 2, kf), n - kl - km)
    return (0, kf), (ms, km), (n - kl, kl)


def table_row(num_frames, T, every_n, strategy, seed=0, draw=0, row=0):
    """src [S] int32 of one video (row: its index in the global batch, row0 + b)."""
    S = T // every_n
    n = min(max(int(num_frames), 0), T)
    k = student_count(n, T, S)
    out = np.full(S, -1, np.int32)
    j = np.arange(k)
    if strategy == "uniform":
        return (np.arange(S) * every_n).astype(np.int32)
    if strategy == "first":
        out[:k] = j
    elif strategy == "last":
        out[:k] = n - k + j
    elif strategy == "middle":
        out[:k] = (n - k) // 2 + j
    elif strategy == "first_middle_last":
        out[:k] = np.concatenate([np.arange(s, s + l) for s, l in fml_runs(n, k)]) if k else j
    elif strategy == "random":
        keys = frame_keys(seed, draw, row, n)
        order = np.lexsort((np.arange(n), keys))          # by key, then by t
        out[:k] = np.sort(order[:k])
    else:
        raise ValueError(strategy)
    return out


def table(num_frames, T, every_n, strategy, seed=0, draw=0, row0=0):
    return np.stack([table_row(n, T, every_n, strategy, seed, draw, row0 + b) for b, n in enumerate(num_frames)])


def rearrange(x, src, every_n):
    """x' with x'[b, j * every_n] = x[b, src[b, j]] and zeros elsewhere (also where src is -1): the uniform student of x' sees what the
    selected student of x sees."""
    xp = np.zeros_like(x)
    B, S = src.shape
    for b in range(B):
        for j in range(S):
            if src[b, j] >= 0:
                xp[b, j * every_n] = x[b, src[b, j]]
    return xp
