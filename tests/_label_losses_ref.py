"""float64 restatement of the label losses of evc_label_loss (include/evc.h; cs/losses.py), shared by tests/test_cpu_label_losses.py,
tests/test_gpu_label_losses.py and tests/test_gpu_label_loss_graphs.py.  numpy only.

Per kind a function (p float32 [B, V], y uint8 [B, V][, w float32 [V]]) -> dict with
  loss   float: mean_b of the row losses
  grad   [B, V] float64: d(sum_b row loss_b)/dp   (the caller scales by grad_scale)
  mag    [B, V] float64: the sum of the magnitudes of the addends of that gradient's expression (the scale of the 1e-5 bound)
Masks and thresholds - p >= t, p < 0.9f, mpp, p (1 - y) > mpp, 1 - s p > 0 - are evaluated on the float32 inputs in np.float32, exactly
as the reference's f32 graph would (no rounding can flip them: s p is exact, 1 - x > 0 iff x < 1, p (1 - y) is p or 0); everything else
is float64.  eps = 10e-6 (SOFTMAX: 10e-8)."""
import numpy as np

EPS = 10e-6
KINDS = ("WITH_SPARSITY", "TOP50", "CLASS_IMBALANCE", "POSITIVES", "NEW", "HINGE", "SOFTMAX")
KIND_IDS = {k: i + 1 for i, k in enumerate(KINDS)}            # EVC_LOSS_* of include/evc.h
CLASS_NAMES = {"WITH_SPARSITY": "CrossEntropyLossWithSparsity", "TOP50": "CrossEntropyLossTop50",
               "CLASS_IMBALANCE": "CrossEntropyLossClassImbalance", "POSITIVES": "CrossEntropyLossPositives", "NEW": "NewLoss",
               "HINGE": "HingeLoss", "SOFTMAX": "SoftmaxLoss"}
SHAPES = [(1, 50), (3, 51), (5, 64), (4, 257), (7, 1023), (300, 64), (2, 4716)]
SMALL_SHAPES = [(1, 1), (2, 3)]                                # every kind but TOP50, which must refuse them
K50 = 4716.0 / 50.0
TOTAL_LABEL_COUNT = 4906660.0 + 1401828.0


def _ce_parts(p, y):
    p, y = p.astype(np.float64), (y != 0).astype(np.float64)
    a, b = p + EPS, 1.0 - p + EPS
    return y, a, b


def with_sparsity(p, y, w=None):
    y64, a, b = _ce_parts(p, y)
    rows = (-(y64 * np.log(a) + (1 - y64) * np.log(b)) + 0.1 * p.astype(np.float64)).sum(1)
    dce = -y64 / a + (1 - y64) / b
    return dict(loss=float(rows.mean()), grad=dce + 0.1, mag=np.abs(dce) + 0.1)


def top50_mask(p):
    assert p.dtype == np.float32 and p.shape[1] >= 50
    t = np.sort(p, axis=1)[:, ::-1][:, 49:50]                 # the 50th largest counting duplicates, in float32
    return (p >= t)


def top50(p, y, w=None):
    y64, a, b = _ce_parts(p, y)
    m = top50_mask(p).astype(np.float64)
    rows = (m * K50 * -(y64 * np.log(a) + (1 - y64) * np.log(b))).sum(1)
    g = m * K50 * (-y64 / a + (1 - y64) / b)
    return dict(loss=float(rows.mean()), grad=g, mag=np.abs(g), mask=m)


def class_imbalance(p, y, w):
    y64, a, b = _ce_parts(p, y)
    w64 = w.astype(np.float64)[None, :]
    rows = (-(w64 * y64 * np.log(a) + (1 - y64) * np.log(b))).sum(1)
    g = -w64 * y64 / a + (1 - y64) / b
    return dict(loss=float(rows.mean()), grad=g, mag=np.abs(g))


def positives(p, y, w=None):
    y64, a, b = _ce_parts(p, y)
    rows = (-(y64 * np.log(a))).sum(1)
    g = -y64 / a
    return dict(loss=float(rows.mean()), grad=g, mag=np.abs(g))


def new_mpp(p, y):
    """max(min_{b,c}(y ? p : 1) - 0.1f, 0.1f) over the whole batch, in float32 in exactly that order."""
    assert p.dtype == np.float32
    mn = np.min(np.where(y != 0, p, np.float32(1.0))).astype(np.float32)
    return np.maximum(np.float32(mn - np.float32(0.1)), np.float32(0.1))


def new(p, y, w=None):
    y64, a, b = _ce_parts(p, y)
    y32 = (y != 0).astype(np.float32)
    mpp = new_mpp(p, y)
    bp = (p < np.float32(0.9)).astype(np.float64)
    bn = ((p * (np.float32(1.0) - y32)) > mpp).astype(np.float64)
    rows = (-(bp * y64 * np.log(a) + bn * (1 - y64) * np.log(b))).sum(1)
    g = -bp * y64 / a + bn * (1 - y64) / b
    return dict(loss=float(rows.mean()), grad=g, mag=np.abs(g), mpp=float(mpp), bp=bp, bn=bn)


def hinge(p, y, w=None):
    assert p.dtype == np.float32
    s32 = np.float32(2.0) * (y != 0).astype(np.float32) - np.float32(1.0)
    on = ((np.float32(1.0) - s32 * p) > 0).astype(np.float64)  # a tie goes to the zeros
    s64 = s32.astype(np.float64)
    rows = (on * (1.0 - s64 * p.astype(np.float64))).sum(1)
    g = -s64 * on
    return dict(loss=float(rows.mean()), grad=g, mag=np.abs(g))


def softmax(p, y, w=None):
    p64, y64 = p.astype(np.float64), (y != 0).astype(np.float64)
    yhat = y64 / np.maximum(y64.sum(1, keepdims=True), 10e-8)
    z = p64 - p64.max(1, keepdims=True)
    lse = np.log(np.exp(z).sum(1, keepdims=True))
    sm = np.exp(z - lse)
    rows = -(yhat * (z - lse)).sum(1)
    sy = yhat.sum(1, keepdims=True)
    return dict(loss=float(rows.mean()), grad=sm * sy - yhat, mag=sm * sy + yhat)


FUNCS = {"WITH_SPARSITY": with_sparsity, "TOP50": top50, "CLASS_IMBALANCE": class_imbalance, "POSITIVES": positives, "NEW": new,
         "HINGE": hinge, "SOFTMAX": softmax}


def reference(kind, p, y, w=None):
    return FUNCS[kind](p, y, w)


def class_weights_from_counts(counts):
    """cs/losses.py:107-114 in float64, then float32."""
    return (1.0 / np.sqrt(np.asarray(counts, dtype=np.float64) / TOTAL_LABEL_COUNT)).astype(np.float32)


def make_weights(V):
    """Class weights spanning 1 to 1e3 (the counts file's weights run from ~1.6 to ~250)."""
    return np.logspace(0.0, 3.0, V).astype(np.float32)[np.random.RandomState(V).permutation(V)]


def make_inputs(kind, B, V, seed=0, wide=False):
    """p float32 [B, V] in [0.02, 0.98] (wide: [-1.5, 1.5], for HINGE and SOFTMAX), y uint8 with about 3 positives per row.  For NEW the
    positives take values on both sides of 0.9 and the smallest is 0.35, so that mpp = 0.25 has negatives on both sides."""
    rng = np.random.RandomState(1000 * seed + 7 * B + V)
    lo, hi = (-1.5, 1.5) if wide else (0.02, 0.98)
    p = rng.uniform(lo, hi, size=(B, V)).astype(np.float32)
    y = np.zeros((B, V), dtype=np.uint8)
    k = max(1, min(3, V // 2))
    for b in range(B):
        y[b, rng.choice(V, size=k, replace=False)] = 1
    if kind == "NEW":
        vals = np.array([0.95, 0.6, 0.35, 0.92, 0.5, 0.9375], dtype=np.float32)
        idx = np.argwhere(y != 0)
        for j, (b, c) in enumerate(idx):
            p[b, c] = vals[j % len(vals)]
    return p, y
