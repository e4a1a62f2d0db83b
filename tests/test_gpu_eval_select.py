"""evc_eval_select_rows (ops.eval_select_rows) against its numpy restatement (tests/_eval_select_ref.py), exact on every
output; top_val / top_idx bitwise equal to ops.topk_rows; two launches with identical bits; class_pos adds up; bad arguments
refused before a launch; and validate.py / eval_finetune.py with --metrics_on_device against the same call without it."""
import numpy as np
import pytest
import torch

import _eval_select_ref as ref

pytestmark = pytest.mark.gpu

KEYS = ("top_val", "top_idx", "top_lab", "n_pos", "perr_hits", "class_pos")


def _device(a, ld, pad):
    """The array on the device; with ld, rows at stride ld and the columns beyond cols holding values that would count."""
    rows, cols = a.shape
    if ld is None:
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    buf = np.full((rows, ld), pad, a.dtype)
    buf[:, :cols] = a
    t = torch.from_numpy(buf).cuda()[:, :cols]
    assert t.stride(0) == ld
    return t


def _label_rows(rng, rows, cols, first=0):
    """Row patterns in turn: empty, full (n_pos = cols), min(cols, 300) positives (n_pos > k for every admissible k < cols),
    sparse (1 - 8 positives).  Nonzero bytes take any value."""
    lab = np.zeros((rows, cols), np.uint8)
    for r in range(rows):
        kind = (r + first) % 4
        if kind == 1:
            lab[r] = rng.integers(1, 256, cols)
        elif kind == 2:
            lab[r, rng.choice(cols, min(cols, 300), replace=False)] = rng.integers(1, 256, min(cols, 300))
        elif kind == 3:
            n = min(cols, int(rng.integers(1, 9)))
            lab[r, rng.choice(cols, n, replace=False)] = 1
    return lab


def _ks(cols):
    return sorted({k for k in (1, 20, 256, cols) if k <= min(cols, 256)})


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _check(x, lab, ks, ld=None, ld_lab=None):
    from efficientvideoclassification_youtube8m_amd import _lib, ops
    rows, cols = x.shape
    xd, yd = _device(x, ld, np.nan), _device(lab, ld_lab, 1)
    order = ref.reference_order(x)
    for k in ks:
        a = ops.eval_select_rows(xd, yd, k)
        b = ops.eval_select_rows(xd, yd, k)
        v, i = ops.topk_rows(xd, k)
        torch.cuda.synchronize()
        want = ref.eval_select_rows(x, lab, k, order)
        tag = (rows, cols, k, ld, ld_lab)
        assert set(a) == set(KEYS)
        for key in KEYS:
            got = a[key].cpu().numpy()
            assert got.shape == want[key].shape and got.dtype == want[key].dtype, (key, tag)
            if key == "top_val":
                got, w = got.view(np.uint32), want[key].view(np.uint32)
            else:
                w = want[key]
            bad = np.argwhere(got != w)
            assert len(bad) == 0, (key, tag, bad[:5].tolist())
            assert torch.equal(_bits(a[key]), _bits(b[key])), (key, tag)       # two launches: identical bits
        assert torch.equal(a["top_idx"], i) and torch.equal(_bits(a["top_val"]), _bits(v)), tag
    # class_pos is added to: two launches into one zeroed buffer give twice the column sum; NULL is allowed
    k = ks[0]
    out = ops.eval_select_rows(xd, yd, k)
    cp = torch.zeros(cols, dtype=torch.int32, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    args = (xd.data_ptr(), xd.stride(0) if rows > 1 else cols, yd.data_ptr(), yd.stride(0) if rows > 1 else cols, rows, cols, k,
            out["top_val"].data_ptr(), out["top_idx"].data_ptr(), out["top_lab"].data_ptr(), out["n_pos"].data_ptr(),
            out["perr_hits"].data_ptr())
    _lib.call("evc_eval_select_rows", *args, cp.data_ptr(), s)
    _lib.call("evc_eval_select_rows", *args, cp.data_ptr(), s)
    _lib.call("evc_eval_select_rows", *args, None, s)
    torch.cuda.synchronize()
    assert np.array_equal(cp.cpu().numpy(), 2 * (lab != 0).sum(axis=0).astype(np.int32)), (rows, cols)
    assert np.array_equal(out["perr_hits"].cpu().numpy(), ref.eval_select_rows(x, lab, k, order)["perr_hits"])


@pytest.mark.parametrize("rows", [1, 7, 1024])
@pytest.mark.parametrize("cols", [1, 63, 64, 65, 4716, 32768])
def test_random_rows(rows, cols):
    if rows == 1024 and cols == 32768:
        rows = 64                                       # (the numpy reference sort dominates the test time at 1024 rows)
    rng = np.random.default_rng(rows * 100003 + cols)
    x = rng.standard_normal((rows, cols), dtype=np.float32)
    _check(x, _label_rows(rng, rows, cols, first=cols), _ks(cols))


@pytest.mark.parametrize("rows,cols", [(7, 65), (1024, 4716), (7, 32768)])
def test_heavy_ties(rows, cols):
    """Values quantised to 1/64 (and shifted, so that ties occur at values <= 0 too): every boundary falls inside a tie."""
    rng = np.random.default_rng(cols)
    x = (np.floor(rng.random((rows, cols), dtype=np.float32) * 64) / 64).astype(np.float32) - np.float32(0.25)
    _check(x, _label_rows(rng, rows, cols), _ks(cols))


@pytest.mark.parametrize("cols", [1, 64, 4716, 32768])
def test_all_equal_row(cols):
    x = np.full((8, cols), 0.25, np.float32)
    x[1] = -0.0
    x[2, ::2] = 0.0                                     # +0 / -0 interleaved: all tied, none > 0
    x[3] = -1.5
    x[5] = 0.0
    x[6, ::2] = -0.0
    rng = np.random.default_rng(cols)
    _check(x, _label_rows(rng, 8, cols, first=1), _ks(cols))
    _check(x, _label_rows(rng, 8, cols, first=2), _ks(cols)[:1])


def test_signed_zero_inf_nan():
    rng = np.random.default_rng(11)
    specials = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF,
                         0x00000001, 0x80000001, 0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF], np.uint32)
    for cols in (63, 65, 4716):
        x = rng.choice(specials, size=(9, cols)).view(np.float32)
        x[0] = rng.standard_normal(cols, dtype=np.float32)
        x[0, rng.integers(0, cols, 5)] = np.nan
        _check(x, _label_rows(rng, 9, cols, first=1), _ks(cols))


@pytest.mark.parametrize("cols,extra,extra_lab", [(4716, 1, 3), (4716, 3, 0), (4716, 4, 1), (64, 1, 1), (65, 2, 7), (32768, 5, 3), (4716, 0, 5)])
def test_row_strides(cols, extra, extra_lab):
    rng = np.random.default_rng(cols + extra)
    x = rng.standard_normal((7, cols), dtype=np.float32)
    _check(x, _label_rows(rng, 7, cols), _ks(cols), ld=cols + extra if extra else None, ld_lab=cols + extra_lab if extra_lab else None)


def test_moe_head_outputs():
    """Real predictions: the MoE head of an H-LSTM student at 1024 x 4716 (sigmoid x softmax mixtures: many near-ties), random
    sparse labels, some of them on the best-ranked classes."""
    from efficientvideoclassification_youtube8m_amd.distill import EvalGraph
    g = EvalGraph(1024, every_n=10, student_only=True, feature_size=128, lstm_cells=64, device="cuda:0")
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(5)
    q = torch.randint(0, 256, (1024, 300, 128), dtype=torch.uint8, device="cuda:0", generator=gen)
    n = torch.randint(120, 301, (1024,), dtype=torch.int32, device="cuda:0", generator=gen)
    pred = g.step(q, torch.zeros((1024, 4716), dtype=torch.uint8, device="cuda:0"), n)["predictions"]
    assert pred.shape == (1024, 4716) and pred.dtype == torch.float32
    x = pred.cpu().numpy()
    rng = np.random.default_rng(5)
    lab = np.zeros((1024, 4716), np.uint8)
    best = ref.reference_order(x)[:, :10]
    for r in range(1024):
        lab[r, rng.choice(4716, int(rng.integers(0, 6)), replace=False)] = 1
        lab[r, rng.choice(best[r], int(rng.integers(0, 4)), replace=False)] = 1
    _check(x, lab, [1, 20, 256])


def test_bad_arguments():
    from efficientvideoclassification_youtube8m_amd import _lib, ops
    x = torch.randn((4, 64), device="cuda:0")
    y = torch.zeros((4, 64), dtype=torch.uint8, device="cuda:0")
    for k in (0, -1, 65):
        with pytest.raises(_lib.EvcError):
            ops.eval_select_rows(x, y, k)
    with pytest.raises(_lib.EvcError):
        ops.eval_select_rows(torch.randn((2, 300), device="cuda:0"), torch.zeros((2, 300), dtype=torch.uint8, device="cuda:0"), 257)
    with pytest.raises(_lib.EvcError):
        ops.eval_select_rows(torch.randn((1, 32769), device="cuda:0"), torch.zeros((1, 32769), dtype=torch.uint8, device="cuda:0"), 5)
    with pytest.raises(_lib.EvcError):
        ops.eval_select_rows(x.as_strided((2, 64), (32, 1)), y[:2], 5)                 # ld < cols
    with pytest.raises(_lib.EvcError):
        ops.eval_select_rows(x[:2], y.as_strided((2, 64), (32, 1)), 5)                 # ld_lab < cols
    for bad_x, bad_y in ((x.double(), y), (x.cpu(), y), (x, y.cpu()), (x, y.float()), (x, y.bool()), (x, y[:, :63]), (x, y[:3]),
                         (x[0], y[0]), (x, y.t().contiguous().t())):
        with pytest.raises(_lib.EvcError):
            ops.eval_select_rows(bad_x, bad_y, 5)
    o = ops.eval_select_rows(x, y, 5)
    s = torch.cuda.current_stream().cuda_stream
    outs = [o[key].data_ptr() for key in KEYS]
    good = [x.data_ptr(), 64, y.data_ptr(), 64, 4, 64, 5] + outs
    _lib.call("evc_eval_select_rows", *good, s)
    for pos, value in ((1, 63), (3, 63), (4, -1), (5, 0), (5, 32769), (6, 0), (6, 65), (0, None), (2, None), (7, None), (8, None),
                       (9, None), (10, None), (11, None)):
        args = list(good)
        args[pos] = value
        with pytest.raises(_lib.EvcError):
            _lib.call("evc_eval_select_rows", *args, s)
    e = ops.eval_select_rows(torch.empty((0, 64), device="cuda:0"), torch.empty((0, 64), dtype=torch.uint8, device="cuda:0"), 5)
    assert e["top_val"].shape == (0, 5) and e["top_idx"].shape == (0, 5) and e["top_lab"].shape == (0, 5)      # rows == 0: nothing launched
    assert e["n_pos"].shape == (0,) and e["perr_hits"].shape == (0,) and int(e["class_pos"].sum()) == 0
    torch.cuda.synchronize()


COMMON = ["--frame_features", "True", "--feature_names", "rgb, audio", "--feature_sizes", "64, 64", "--model",
          "HierarchicalLstmModel", "--gpu", "0", "--num_inputs_to_lstm", "20", "--lstm_layers", "2", "--lstm_cells", "64",
          "--every_n", "10", "--num_readers", "2"]


def _child(binary, data, tdir, result):
    """tests/_eval_select_child.py in a fresh process with EVC_DETERMINISTIC=1 (the library reads it once per process)."""
    import os
    import pickle
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "_eval_select_child.py"), binary, str(data), tdir, str(result)],
                       env=dict(os.environ, EVC_DETERMINISTIC="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(result, "rb") as f:
        return pickle.load(f)


@pytest.mark.parametrize("binary", ["validate", "eval_finetune"])
def test_binaries_with_metrics_on_device(tmp_path, binary):
    """validate.main / eval_finetune.main on a synthetic TFRecord set with a trained checkpoint: --metrics_on_device True against
    the same call without it, every number ==.  Both calls run in one child process under EVC_DETERMINISTIC=1: the default
    cross-entropy loss is summed with float atomics, so avg_loss of two separate runs differs in its last bits whichever path
    computes the metrics (seen here: 1905.8571254 against 1905.8571341); with the fixed-order sum it is the same device scalar.
    The child recomputes the predictions with an EvalGraph and lists the rows with an exact tie across the top_k boundary or a
    tie at a positive value across the n_pos boundary; one such row fails the test by name (the data seed is then changed)."""
    from efficientvideoclassification_youtube8m_amd import readers, train
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    data = tmp_path / "yt8m"
    # (labels from 12 of the 4716 classes and a learning rate that lets 36 iterations find them: metrics that are not all zero)
    kw = dict(feature_sizes=(64, 64), num_classes=12, min_frames=60, max_frames=310)
    readers.write_synthetic_frame_dataset(str(data), 2, 12, seed=1, prefix="train", **kw)
    readers.write_synthetic_frame_dataset(str(data), 2, 7, seed=2, prefix="validate", **kw)
    tdir = str(tmp_path / "model_train") + "/"
    FLAGS.reset()
    try:
        train.main(COMMON + ["--train_data_pattern", str(data / "train*.tfrecord"), "--train_dir", tdir, "--batch_size", "8",
                             "--num_epochs", "6", "--base_learning_rate", "0.02", "--start_new_model", "True"])
    finally:
        FLAGS.reset()
    got = _child(binary, data, tdir, tmp_path / "result.pkl")
    host, dev = got["host"], got["device"]
    print({k: v for k, v in host.items() if k != "aps"}, {k: v for k, v in dev.items() if k != "aps"})
    assert got["videos"] == 14
    assert got["ties_at_k"] == [] and got["ties_at_n_pos"] == [], "boundary ties in these rows - change the data seed"
    assert set(dev) == set(host)
    for key in ("epoch_id", "avg_hit_at_one", "avg_perr", "gap", "avg_loss"):
        assert dev[key] == host[key], key
    assert len(dev["aps"]) == len(host["aps"]) == 4716 and all(a == b for a, b in zip(host["aps"], dev["aps"]))
    assert host["epoch_id"] == 36 and host["avg_loss"] > 0
    assert host["avg_hit_at_one"] > 0 and host["avg_perr"] > 0 and host["gap"] > 0.05 and sum(1 for v in host["aps"] if v > 0) >= 6
    events = open(tdir + "events.jsonl").read()
    assert "Epoch/Eval_GAP" in events and "GlobalStep/Eval_Loss" in events
