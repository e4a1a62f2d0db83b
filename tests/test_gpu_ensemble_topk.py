"""evc_ensemble_topk_rows (ops.ensemble_topk_rows) against its numpy restatement (tests/_ensemble_ref.py): exact indices and
bit-equal values for both modes, with and without prior lists, the dense output, two launches with identical bits, M = 1 against
ops.topk_rows, and every bad argument refused before a launch.  No exclusions anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

import _ensemble_ref as ref

pytestmark = pytest.mark.gpu

MODES = ("max", "mean")


def _device(a, ld=None, pad=np.nan):
    """a on the device, rows at stride ld (the columns beyond hold values that would win a maximum / poison a sum)."""
    if ld is None:
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    buf = np.full((a.shape[0], ld), pad, a.dtype)
    buf[:, :a.shape[1]] = a
    t = torch.from_numpy(buf).cuda()[:, :a.shape[1]]
    assert t.stride(0) == ld or a.shape[0] == 1
    return t


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _check(members, k, mode, weights=None, priors=None, lds=None):
    """One case: top-k + dense against the reference, the dense-only and top-k-only calls, and a second launch."""
    from efficientvideoclassification_youtube8m_amd import ops
    rows, cols = members[0].shape
    xs = [_device(x, None if lds is None else lds[m]) for m, x in enumerate(members)]
    pd = None if priors is None else (torch.from_numpy(priors[0]).cuda(), torch.from_numpy(priors[1]).cuda())
    want = ref.combine(members, mode, weights, priors)
    want_v, want_i = ref.topk(want, k)
    v1, i1, d1 = ops.ensemble_topk_rows(xs, k, mode=mode, weights=weights, priors=pd, dense=True)
    v2, i2, d2 = ops.ensemble_topk_rows(xs, k, mode=mode, weights=weights, priors=pd, dense=True)
    v3, i3 = ops.ensemble_topk_rows(xs, k, mode=mode, weights=weights, priors=pd)                       # top-k only
    v0, i0, d0 = ops.ensemble_topk_rows(xs, 0, mode=mode, weights=weights, priors=pd, dense=True)       # dense only
    torch.cuda.synchronize()
    tag = (len(members), mode, rows, cols, k, lds)
    assert d1.shape == (rows, cols) and v1.shape == (rows, k) and i1.shape == (rows, k) and i1.dtype == torch.int32
    assert np.array_equal(_bits(d1), want.view(np.uint32)), tag
    assert np.array_equal(i1.cpu().numpy(), want_i), tag
    assert np.array_equal(_bits(v1), want_v.view(np.uint32)), tag
    assert np.array_equal(_bits(v1), np.take_along_axis(_bits(d1), i1.cpu().numpy().astype(np.int64), 1)), tag   # selected from the dense row
    for v, i in ((v2, i2), (v3, i3)):
        assert torch.equal(i, i1) and np.array_equal(_bits(v), _bits(v1)), tag
    assert np.array_equal(_bits(d2), _bits(d1)) and np.array_equal(_bits(d0), _bits(d1)), tag
    assert v0.shape == (rows, 0) and i0.shape == (rows, 0)


def _members(rng, M, rows, cols):
    return [rng.random((rows, cols), dtype=np.float32) for _ in range(M)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M", [1, 2, 3, 8])
@pytest.mark.parametrize("rows,cols", [(7, 64), (5, 4717), (1024, 4716), (3, 1), (2, 32768)])
def test_random_rows(M, mode, rows, cols):
    rng = np.random.default_rng(M * 7919 + rows * 31 + cols)
    for k in sorted({1, min(20, cols), min(256, cols)}):
        _check(_members(rng, M, rows, cols), k, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M", [2, 3, 8])
def test_members_with_different_row_strides(M, mode):
    """Each member at its own stride: cols + 1 and cols + 3 are not multiples of 4 (rows that are not 16-byte aligned), cols + 4 is."""
    rng = np.random.default_rng(M)
    for cols in (4716, 65):
        lds = [cols + (1, 4, 0, 3, 8, 5, 2, 12)[m] for m in range(M)]
        _check(_members(rng, M, 9, cols), min(20, cols), mode, lds=lds)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P,kp", [(1, 20), (3, 20), (3, 1), (8, 256)])
@pytest.mark.parametrize("M", [1, 3])
def test_prior_lists(M, mode, P, kp):
    """Lists shorter than kp (padding -1), classes that several files and the top of the members share, values that win and lose."""
    rng = np.random.default_rng(M * 100 + P * 10 + kp)
    for rows, cols in ((6, 4716), (1024, 4716), (5, 301)):
        if rows == 1024 and (P, kp) != (3, 20):
            continue
        members = _members(rng, M, rows, cols)
        priors = ref.random_priors(rng, P, rows, kp, cols, low=0.0, high=1.5)
        assert (priors[0] < 0).any() and (priors[0] >= 0).any()
        if P > 1 and kp > 1:                                          # (the inputs' own precondition: two files share classes)
            assert np.intersect1d(priors[0][0][priors[0][0] >= 0], priors[0][1][priors[0][1] >= 0]).size > 0
        w = None if mode == "max" else rng.uniform(0.05, 1.0, M + P).astype(np.float32)
        _check(members, 20, mode, weights=w, priors=priors)
        _check(members, 20, mode, priors=priors, lds=[cols + 1 + m for m in range(M)])      # default weights 1 / (M + P)


@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_non_default_weights(M):
    rng = np.random.default_rng(40 + M)
    members = _members(rng, M, 33, 4716)
    for w in (rng.uniform(-1, 1, M), rng.dirichlet(np.ones(M)), np.arange(1, M + 1) * 0.1, np.zeros(M)):
        _check(members, 20, "mean", weights=np.asarray(w, np.float32))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_heavy_ties_and_all_equal_rows(M, mode):
    rng = np.random.default_rng(M)
    for rows, cols in ((7, 65), (64, 4716)):
        members = [(np.floor(rng.random((rows, cols), dtype=np.float32) * 16) / 16).astype(np.float32) for _ in range(M)]
        for k in sorted({1, 20, min(256, cols)}):
            _check(members, k, mode)
        priors = ref.random_priors(rng, 3, rows, 8, cols)
        priors[1][...] = np.floor(priors[1] * 16) / 16
        _check(members, 20, mode, priors=priors)
    for cols in (1, 64, 4716):
        members = [np.full((3, cols), 0.25, np.float32) for _ in range(M)]
        _check(members, min(20, cols), mode)
        members[-1][1] = 0.5
        members[0][2, ::2] = 0.125
        _check(members, min(20, cols), mode)


@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_signed_zero_inf_nan_in_max_mode(M):
    rng = np.random.default_rng(11 + M)
    specials = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF,
                         0x00000001, 0x80000001, 0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF], np.uint32)
    for cols in (63, 65, 4716):
        members = [rng.choice(specials, size=(7, cols)).view(np.float32) for _ in range(M)]
        for x in members:
            x[0] = rng.standard_normal(cols, dtype=np.float32)
            x[0, rng.integers(0, cols, 5)] = np.nan
        members[0][1] = -0.0                                          # -0 against +0 in the other members: a tie, member 0 keeps its bits
        for x in members[1:]:
            x[1] = 0.0
        _check(members, min(20, cols), "max")
        idx, val = ref.random_priors(rng, 2, 7, 16, cols)
        val[...] = rng.choice(specials, size=val.shape).view(np.float32)
        _check(members, min(20, cols), "max", priors=(idx, val))


def test_one_member_in_max_mode_is_topk_rows():
    from efficientvideoclassification_youtube8m_amd import ops
    rng = np.random.default_rng(5)
    for rows, cols, ld in ((1024, 4716, None), (7, 65, 67), (3, 32768, None)):
        x = _device(rng.standard_normal((rows, cols), dtype=np.float32), ld)
        for k in (1, 20, min(256, cols)):
            v, i, d = ops.ensemble_topk_rows([x], k, dense=True)
            tv, ti = ops.topk_rows(x, k)
            assert torch.equal(i, ti) and np.array_equal(_bits(v), _bits(tv))
            assert np.array_equal(_bits(d), _bits(x))


def test_bad_arguments():
    from efficientvideoclassification_youtube8m_amd import _lib, ops
    x = torch.rand((4, 64), device="cuda:0")
    y = torch.rand((4, 64), device="cuda:0")
    bad = _lib.EvcError
    # ---- the wrapper's own checks ----
    for call in (lambda: ops.ensemble_topk_rows([], 5), lambda: ops.ensemble_topk_rows([x] * 9, 5),
                 lambda: ops.ensemble_topk_rows([x, y], 5, mode="median"),
                 lambda: ops.ensemble_topk_rows([x, y.cpu()], 5), lambda: ops.ensemble_topk_rows([x.cpu(), y.cpu()], 5),
                 lambda: ops.ensemble_topk_rows([x, y.double()], 5), lambda: ops.ensemble_topk_rows([x, y[:, :32]], 5),
                 lambda: ops.ensemble_topk_rows([x, y[:3]], 5), lambda: ops.ensemble_topk_rows([x, y.t().contiguous().t()], 5),
                 lambda: ops.ensemble_topk_rows([x, y], 5, mode="mean", weights=[0.5]),
                 lambda: ops.ensemble_topk_rows([x, y], 5, mode="mean", weights=[0.5, 0.25, 0.25]),
                 lambda: ops.ensemble_topk_rows([x, y], 5, mode="max", weights=[0.5, 0.5]),
                 lambda: ops.ensemble_topk_rows([x, y], 0), lambda: ops.ensemble_topk_rows([x, y], -1),
                 lambda: ops.ensemble_topk_rows([x, y], 65), lambda: ops.ensemble_topk_rows([x, y], -1, dense=True),
                 lambda: ops.ensemble_topk_rows([torch.rand((2, 300), device="cuda:0")] * 2, 257),
                 lambda: ops.ensemble_topk_rows([torch.rand((1, 32769), device="cuda:0")], 5),
                 lambda: ops.ensemble_topk_rows([x, x.as_strided((4, 64), (32, 1))], 5)):                    # ld < cols
        with pytest.raises(bad):
            call()
    pi = torch.zeros((1, 4, 3), dtype=torch.int32, device="cuda:0")
    pv = torch.zeros((1, 4, 3), dtype=torch.float32, device="cuda:0")
    for priors in ((pi.long(), pv), (pi, pv.double()), (pi[:, :3], pv[:, :3]), (pi, pv[:, :, :2]), (pi.cpu(), pv.cpu()),
                   (pi.expand(9, 4, 3).contiguous(), pv.expand(9, 4, 3).contiguous()),
                   (torch.zeros((1, 4, 257), dtype=torch.int32, device="cuda:0"), torch.zeros((1, 4, 257), device="cuda:0"))):
        with pytest.raises(bad):
            ops.ensemble_topk_rows([x, y], 5, priors=priors)
    with pytest.raises(bad):
        ops.ensemble_topk_rows([x, y], 5, mode="mean", weights=[0.5, 0.5], priors=(pi, pv))               # 2 members + 1 list: 3 weights
    # ---- every EVC_ERR_BAD_ARG of the entry itself ----
    ov = torch.empty(64, device="cuda:0")
    oi = torch.empty(64, dtype=torch.int32, device="cuda:0")
    od = torch.empty((4, 64), device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    ptr2 = (C.c_void_p * 2)(x.data_ptr(), y.data_ptr())
    ptr9 = (C.c_void_p * 9)(*[x.data_ptr()] * 9)
    ptr_null = (C.c_void_p * 2)(x.data_ptr(), None)
    ld2, ld9, ld_short = (C.c_int64 * 2)(64, 64), (C.c_int64 * 9)(*[64] * 9), (C.c_int64 * 2)(64, 63)
    w = (C.c_float * 16)(*[0.5] * 16)
    good = dict(preds=ptr2, ld=ld2, weights=w, M=2, prior_idx=None, prior_val=None, P=0, kp=0, rows=4, cols=64, mode=0, k=5,
                out_val=ov.data_ptr(), out_idx=oi.data_ptr(), out_dense=od.data_ptr(), ld_dense=64)

    def call(**kw):
        a = dict(good, **kw)
        _lib.call("evc_ensemble_topk_rows", a["preds"], a["ld"], a["weights"], a["M"], a["prior_idx"], a["prior_val"], a["P"], a["kp"],
                  a["rows"], a["cols"], a["mode"], a["k"], a["out_val"], a["out_idx"], a["out_dense"], a["ld_dense"], s)
    call()                                                                    # the base of the variations is accepted
    call(k=0, out_val=None, out_idx=None)
    call(out_dense=None)
    call(weights=None)                                                        # mode 0 does not read the weights
    call(rows=0, preds=ptr_null)                                              # rows == 0: nothing launched, nothing dereferenced
    prior = dict(prior_idx=pi.data_ptr(), prior_val=pv.data_ptr(), P=1, kp=3)
    call(**prior)
    for kw in (dict(M=0), dict(M=9, preds=ptr9, ld=ld9), dict(M=-1), dict(P=-1), dict(prior, P=9), dict(prior, kp=0), dict(prior, kp=257),
               dict(prior, prior_idx=None), dict(prior, prior_val=None), dict(mode=2), dict(mode=-1), dict(cols=0), dict(cols=32769),
               dict(k=-1), dict(k=65), dict(k=257, cols=300), dict(rows=-1), dict(preds=None), dict(ld=None), dict(mode=1, weights=None),
               dict(ld=ld_short), dict(ld_dense=63), dict(k=0), dict(k=0, out_val=None), dict(k=0, out_val=None, out_idx=None, out_dense=None),
               dict(out_val=None), dict(out_idx=None), dict(out_val=None, out_idx=None), dict(preds=ptr_null)):
        with pytest.raises(bad, match="-5"):
            call(**kw)
    torch.cuda.synchronize()
    v, i = ops.ensemble_topk_rows([torch.empty((0, 64), device="cuda:0")] * 2, 5)                          # rows == 0
    assert v.shape == (0, 5) and i.shape == (0, 5)
