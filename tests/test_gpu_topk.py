"""evc_topk_rows (ops.topk_rows) against a numpy restatement of its total order: exact indices, bitwise values, two launches
with identical bits, and every bad argument refused before a launch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


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


def _check(x, ks, ld=None, pad_value=np.nan):
    from efficientvideoclassification_youtube8m_amd import ops
    rows, cols = x.shape
    if ld is None:
        xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    else:                                               # rows at stride ld; the columns beyond cols hold values that would win
        buf = np.full((rows, ld), pad_value, np.float32)
        buf[:, :cols] = x
        xd = torch.from_numpy(buf).cuda()[:, :cols]
        assert xd.stride(0) == ld
    order = reference_order(x)
    for k in ks:
        v1, i1 = ops.topk_rows(xd, k)
        v2, i2 = ops.topk_rows(xd, k)
        torch.cuda.synchronize()
        want_i = order[:, :k].astype(np.int32)
        want_v = np.take_along_axis(x, want_i, 1)
        got_i, got_v = i1.cpu().numpy(), v1.cpu().numpy()
        assert got_i.shape == (rows, k) and got_v.shape == (rows, k)
        assert np.array_equal(got_i, want_i), (rows, cols, k, ld)
        assert np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32)), (rows, cols, k, ld)
        assert torch.equal(i1, i2) and torch.equal(v1.view(torch.int32), v2.view(torch.int32))


def _ks(cols):
    return sorted({k for k in (1, 20, 256, cols) if k <= min(cols, 256)})


@pytest.mark.parametrize("rows", [1, 7, 1024])
@pytest.mark.parametrize("cols", [1, 63, 64, 65, 4716, 32768])
def test_random_rows(rows, cols):
    if rows == 1024 and cols == 32768:
        rows = 64                                       # (the numpy reference sort dominates the test time at 1024 rows)
    rng = np.random.default_rng(rows * 100003 + cols)
    _check(rng.standard_normal((rows, cols), dtype=np.float32), _ks(cols))


@pytest.mark.parametrize("rows,cols", [(7, 65), (1024, 4716), (7, 32768)])
def test_heavy_ties(rows, cols):
    rng = np.random.default_rng(cols)
    x = (np.floor(rng.random((rows, cols), dtype=np.float32) * 64) / 64).astype(np.float32)
    _check(x, _ks(cols))


@pytest.mark.parametrize("cols", [1, 64, 4716, 32768])
def test_all_equal_row(cols):
    x = np.full((3, cols), 0.25, np.float32)
    x[1] = -0.0
    x[2, ::2] = 0.0                                     # +0 / -0 interleaved: all tied
    _check(x, _ks(cols))


def test_signed_zero_inf_nan():
    rng = np.random.default_rng(11)
    specials = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF,
                         0x00000001, 0x80000001, 0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF], np.uint32)
    for cols in (63, 65, 4716):
        x = rng.choice(specials, size=(7, cols)).view(np.float32)
        x[0] = rng.standard_normal(cols, dtype=np.float32)
        x[0, rng.integers(0, cols, 5)] = np.nan
        _check(x, _ks(cols))


@pytest.mark.parametrize("cols,extra", [(4716, 1), (4716, 3), (4716, 4), (64, 1), (65, 2), (32768, 5)])
def test_row_stride(cols, extra):
    rng = np.random.default_rng(cols + extra)
    x = rng.standard_normal((7, cols), dtype=np.float32)
    _check(x, _ks(cols), ld=cols + extra)                # odd ld: rows that are not 16-byte aligned


def test_moe_head_outputs():
    """Real predictions: the MoE head of an H-LSTM student at 1024 x 4716 (sigmoid x softmax mixtures: many near-ties)."""
    from efficientvideoclassification_youtube8m_amd.distill import EvalGraph
    g = EvalGraph(1024, every_n=10, student_only=True, feature_size=128, lstm_cells=64, device="cuda:0")
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(5)
    q = torch.randint(0, 256, (1024, 300, 128), dtype=torch.uint8, device="cuda:0", generator=gen)
    n = torch.randint(120, 301, (1024,), dtype=torch.int32, device="cuda:0", generator=gen)
    labels = torch.zeros((1024, 4716), dtype=torch.uint8, device="cuda:0")
    pred = g.step(q, labels, n)["predictions"]
    assert pred.shape == (1024, 4716) and pred.dtype == torch.float32
    _check(pred.cpu().numpy(), [1, 20, 256])


def test_bad_arguments():
    from efficientvideoclassification_youtube8m_amd import _lib, ops
    x = torch.randn((4, 64), device="cuda:0")
    for k in (0, -1, 65):
        with pytest.raises(_lib.EvcError):
            ops.topk_rows(x, k)
    with pytest.raises(_lib.EvcError):
        ops.topk_rows(torch.randn((2, 300), device="cuda:0"), 257)
    with pytest.raises(_lib.EvcError):
        ops.topk_rows(torch.randn((1, 32769), device="cuda:0"), 5)
    with pytest.raises(_lib.EvcError):
        ops.topk_rows(x.as_strided((2, 64), (32, 1)), 5)                      # ld < cols
    with pytest.raises(_lib.EvcError):
        ops.topk_rows(x.double(), 5)
    with pytest.raises(_lib.EvcError):
        ops.topk_rows(x.cpu(), 5)
    out = torch.empty(64, device="cuda:0")
    idx = torch.empty(64, dtype=torch.int32, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    for args in ((x.data_ptr(), 63, 4, 64, 5), (x.data_ptr(), 64, -1, 64, 5), (x.data_ptr(), 64, 4, 0, 1), (None, 64, 4, 64, 5)):
        with pytest.raises(_lib.EvcError):
            _lib.call("evc_topk_rows", *args, out.data_ptr(), idx.data_ptr(), s)
    v, i = ops.topk_rows(torch.empty((0, 64), device="cuda:0"), 5)             # rows == 0: nothing launched
    assert v.shape == (0, 5) and i.shape == (0, 5)
    torch.cuda.synchronize()
