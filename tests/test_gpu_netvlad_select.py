"""NetVLAD grid towers on the frames a --student_sampling word selects: evc_frames_gather_packed_tab bit for bit against
the grid gather on a table that names the grid's frames and against the existing gather on the rearranged batch for arbitrary tables, its
optional outputs and refusals; the selected tower against its float64 restatement (tests/_netvlad_packed_ref.py fed the table's rows),
"random" across steps and a restore, the distillation step against float64, and - in a child process under EVC_DETERMINISTIC=1 - the
bit-for-bit comparisons of two towers and train.main / validate.main end to end.  pytest -m gpu.  Every test prints the figures it judges
before it asserts; what an MI355X gave is recorded in DESIGN.md 7.20."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _frame_select_ref as fs
import _netvlad_distill_ref as dx
import _netvlad_packed_ref as nv
from oracle import model_math as mm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
GUARD = 3


def _np(t):
    return t.detach().cpu().double().numpy()


def _outs(Rp, F):
    """Both outputs prefilled with NaN, GUARD rows behind Rp."""
    return torch.full((Rp + GUARD, F), NAN, device=DEV), torch.full((Rp + GUARD, F), NAN, dtype=torch.bfloat16, device=DEV)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _twice(fn, *outs):
    """fn() fills `outs`; a second call on the same inputs must give the same bits.  NaN guards compare as bit patterns."""
    fn()
    first = [o.clone() for o in outs]
    fn()
    torch.cuda.synchronize()
    for o, f in zip(outs, first):
        assert torch.equal(_bits(o), _bits(f))


def _input(rng, B, T, F, u8):
    q = rng.integers(0, 256, (B, T, F), dtype=np.uint8)
    return torch.from_numpy(q).to(DEV) if u8 else torch.from_numpy(rng.standard_normal((B, T, F)).astype(np.float32)).to(DEV)


def _check_tail(out, out_bf, R, Rp):
    assert not out[R:Rp].any() and not out_bf[R:Rp].any()            # rows R .. Rp: zeros
    assert torch.isnan(out[Rp:]).all() and torch.isnan(out_bf[Rp:].float()).all()      # nothing at or beyond Rp is written
    assert torch.isfinite(out[:Rp]).all() and torch.isfinite(out_bf[:Rp].float()).all()


# ---------------------------------------------------------------------------- 1. a table that names the grid's frames
# (4, 12, 8, 1): F / 4 = 2 lanes; (3, 40, 260, 3): F / 4 = 65, a second trip of the row loop, T no multiple of every_n (the table stride
# is ceil(T / every_n) here); (2, 300, 1152, 10): the shipped row length.  An empty first and an empty last video in every case.
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("B,T,F,every_n,n", [(4, 12, 8, 1, [0, 5, 12, 0]), (3, 40, 260, 3, [0, 40, 0]), (2, 300, 1152, 10, [0, 151]),
                                             (4, 300, 1152, 10, [0, 300, 151, 0])])
def test_gather_equals_the_grid_gather(B, T, F, every_n, n, u8, normalize):
    from efficientvideoclassification_youtube8m_amd import ops
    rng = np.random.default_rng(B * 1000 + F)
    n = np.asarray(n, np.int32)
    plan = ops.GridPlan(n, every_n, T)
    R, Rp = plan.R, plan.Rp
    assert 0 < R < Rp and plan.k[0] == 0
    S = -(-T // every_n)
    src = np.full((B, S), -1, np.int32)
    for b in range(B):
        src[b, :plan.k[b]] = np.arange(plan.k[b]) * every_n
    x = _input(rng, B, T, F, u8)
    nd, off, srcd = torch.from_numpy(n).to(DEV), torch.from_numpy(plan.row_off).to(DEV), torch.from_numpy(src).to(DEV)
    want, want_bf = _outs(Rp, F)
    ops.frames_gather_packed(x, nd, off, every_n, R, Rp, want, want_bf, normalize=normalize)
    got, got_bf = _outs(Rp, F)
    _twice(lambda: ops.frames_gather_packed_tab(x, nd, off, srcd, R, Rp, got, got_bf, normalize=normalize), got, got_bf)
    assert torch.equal(_bits(got[:Rp]), _bits(want[:Rp])) and torch.equal(_bits(got_bf[:Rp]), _bits(want_bf[:Rp]))
    assert got[:R].any() and got_bf[:R].any()
    _check_tail(got, got_bf, R, Rp)


# ---------------------------------------------------------------------------- 2. arbitrary tables
B2, T2, F2, E2 = 5, 60, 68, 10
N2 = np.array([0, 60, 9, 33, 47], np.int32)


def _rearranged(x, src, k):
    """The batch with video b's frames src[b, :k_b] moved to its front (index_select per video), on the device."""
    xs = torch.zeros_like(x)
    for b in range(x.shape[0]):
        if k[b]:
            xs[b, :k[b]] = x[b].index_select(0, torch.from_numpy(src[b, :k[b]].astype(np.int64)).to(DEV))
    return xs


@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("word", ["first", "last", "first_middle_last", "random", "segment_change"])
def test_gather_on_device_tables(word, u8):
    """The device tables of the words at (B, T, F, every_n) = (5, 60, 68, 10): the gather through the table equals the existing gather at
    every_n = 1 on the batch rearranged on the host with num_frames' = k_b, bit for bit."""
    from efficientvideoclassification_youtube8m_amd import ops
    rng = np.random.default_rng(17)
    x = _input(rng, B2, T2, F2, u8)
    nd = torch.from_numpy(N2).to(DEV)
    if word in ops.STUDENT_SAMPLING_SCORED:
        srcd = ops.student_frame_select_scored(nd, ops.frame_change_keys(x, nd), T2, E2, word)
    else:
        srcd = ops.student_frame_select(nd, T2, E2, word, seed=5, draw=3, row0=2)
        assert np.array_equal(srcd.cpu().numpy(), fs.table(N2, T2, E2, word, seed=5, draw=3, row0=2))
    src = srcd.cpu().numpy()
    plan = ops.SelectPlan(N2, E2, T2)
    R, Rp = plan.R, plan.Rp
    assert list(plan.k) == [0, 6, 0, 3, 4] and np.array_equal((src >= 0).sum(axis=1), plan.k) and 0 < R < Rp
    off = torch.from_numpy(plan.row_off).to(DEV)
    got, got_bf = _outs(Rp, F2)
    _twice(lambda: ops.frames_gather_packed_tab(x, nd, off, srcd, R, Rp, got, got_bf, normalize=True), got, got_bf)
    want, want_bf = _outs(Rp, F2)
    kd = torch.from_numpy(plan.k).to(DEV)
    ops.frames_gather_packed(_rearranged(x, src, plan.k), kd, off, 1, R, Rp, want, want_bf, normalize=True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got[:Rp]), _bits(want[:Rp])) and torch.equal(_bits(got_bf[:Rp]), _bits(want_bf[:Rp]))
    assert bool(((got[:R].double().norm(dim=1) - 1.0).abs() < 1e-5).all())
    _check_tail(got, got_bf, R, Rp)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("u8", [True, False])
def test_gather_gives_zero_rows_for_entries_without_a_frame(u8, normalize):
    """A hand-made table with -1, T, a huge entry and, inside the first k_b slots, an entry >= n_b: exact zero rows for the first three
    with either input, for the last with uint8 input (an f32 batch holds whatever the reader left there: it is read).  A row count per
    video beyond S is the host's mistake, yet the table is not read there: zero rows."""
    from efficientvideoclassification_youtube8m_amd import ops
    B, T, F, S = 3, 20, 68, 4
    rng = np.random.default_rng(23)
    x = _input(rng, B, T, F, u8)
    n = np.array([12, 20, 7], np.int32)
    src = np.array([[3, -1, 11, 12], [T, 19, 2 ** 31 - 1, 0], [6, 7, -5, 1]], np.int32)
    row_off = np.array([0, 4, 8, 12], np.int32)
    R, Rp = 12, 32
    nd, off, srcd = torch.from_numpy(n).to(DEV), torch.from_numpy(row_off).to(DEV), torch.from_numpy(src).to(DEV)
    got, got_bf = _outs(Rp, F)
    _twice(lambda: ops.frames_gather_packed_tab(x, nd, off, srcd, R, Rp, got, got_bf, normalize=normalize), got, got_bf)
    zero = {1, 4, 6, 10} | ({3, 9} if u8 else set())
    for row in range(R):
        b, j = divmod(row, S)
        if row in zero:
            assert not got[row].any() and not got_bf[row].any(), row
        else:
            one, one_bf = _outs(32, F)
            ops.frames_gather_packed(x[b:b + 1, src[b, j]:src[b, j] + 1].contiguous(), torch.ones(1, dtype=torch.int32, device=DEV),
                                     torch.tensor([0, 1], dtype=torch.int32, device=DEV), 1, 1, 32, one, one_bf, normalize=normalize)
            assert torch.equal(got[row], one[0]) and torch.equal(_bits(got_bf[row]), _bits(one_bf[0])) and got[row].any(), row
    _check_tail(got, got_bf, R, Rp)
    # rows of a video beyond its S table slots: S = 2 of the same buffer read as [6][2] would name other videos' entries - never read
    off2 = torch.tensor([0, 3, 3, 3, 3, 3, 3], dtype=torch.int32, device=DEV)
    x6 = _input(rng, 6, T, F, u8)
    n6 = torch.full((6,), T, dtype=torch.int32, device=DEV)
    got, got_bf = _outs(32, F)
    ops.frames_gather_packed_tab(x6, n6, off2, srcd.view(6, 2), 3, 32, got, got_bf, normalize=normalize)
    torch.cuda.synchronize()
    assert got[0].any() and not got[1].any() and not got[2].any() and not got_bf[2].any()      # slots 0: frame 3, 1: -1, 2: beyond S


# ---------------------------------------------------------------------------- 3. one output alone
@pytest.mark.parametrize("u8", [True, False])
def test_gather_single_outputs(u8):
    from efficientvideoclassification_youtube8m_amd import ops
    rng = np.random.default_rng(29)
    x = _input(rng, B2, T2, F2, u8)
    nd = torch.from_numpy(N2).to(DEV)
    srcd = ops.student_frame_select(nd, T2, E2, "last")
    plan = ops.SelectPlan(N2, E2, T2)
    R, Rp = plan.R, plan.Rp
    off = torch.from_numpy(plan.row_off).to(DEV)
    both, both_bf = _outs(Rp, F2)
    ops.frames_gather_packed_tab(x, nd, off, srcd, R, Rp, both, both_bf, normalize=True)
    f32, untouched_bf = _outs(Rp, F2)
    _twice(lambda: ops.frames_gather_packed_tab(x, nd, off, srcd, R, Rp, f32, None, normalize=True), f32)
    untouched, bf = _outs(Rp, F2)
    _twice(lambda: ops.frames_gather_packed_tab(x, nd, off, srcd, R, Rp, None, bf, normalize=True), bf)
    assert torch.equal(_bits(f32), _bits(both)) and torch.equal(_bits(bf), _bits(both_bf)) and both[:R].any()
    assert torch.isnan(untouched).all() and torch.isnan(untouched_bf.float()).all()


# ---------------------------------------------------------------------------- 4. refusals
def test_gather_refuses_before_any_launch():
    """EVC_ERR_BAD_SHAPE (-1): F % 4 != 0, S < 1, R > B S, Rp < R, Rp - R >= 32.  EVC_ERR_BAD_ARG (-5): NULL num_frames / row_off / src,
    both outputs NULL, both or neither of x / x_u8.  EVC_ERR_BAD_ALIGN (-2): a misaligned x, x_u8, out, out_bf16 or src.  Nothing is
    written by any of them."""
    from efficientvideoclassification_youtube8m_amd import _lib
    lib = _lib.load()
    B, T, F, S, R, Rp = 2, 8, 8, 4, 6, 32
    xf = torch.zeros(B * T * F + 4, device=DEV)
    xq = torch.zeros(B * T * F + 4, dtype=torch.uint8, device=DEV)
    n = torch.tensor([8, 5, 0], dtype=torch.int32, device=DEV)
    off = torch.tensor([0, 4, 6, 0], dtype=torch.int32, device=DEV)
    src = torch.tensor([0, 1, 2, 3, 0, 1, -1, -1, 0], dtype=torch.int32, device=DEV)
    out = torch.full((64 * F + 4,), 3.0, device=DEV)
    bf = torch.full((64 * F + 4,), 3.0, dtype=torch.bfloat16, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def call(shape=(B, T, F, S, R, Rp), **kw):
        t = dict(x=xf, xq=None, n=n, off=off, src=src, out=out, bf=bf)
        t.update(kw)
        b_, t_, f_, s_, r_, rp_ = shape
        return lib.evc_frames_gather_packed_tab(p(t["x"]), p(t["xq"]), p(t["n"]), p(t["off"]), p(t["src"]), b_, t_, f_, s_, r_, rp_, 1,
                                                p(t["out"]), p(t["bf"]), stream)

    for shape in ((B, T, 6, S, R, Rp), (B, T, F, 0, R, Rp), (B, T, F, 2, R, Rp), (B, T, F, S, R, R - 1), (B, T, F, S, R, R + 32),
                  (0, T, F, S, R, Rp), (B, 0, F, S, R, Rp), (B, T, F, S, -1, 31)):
        assert call(shape) == -1, shape
    assert b"evc_frames_gather_packed_tab" in lib.evc_last_error()
    for name in ("n", "off", "src"):
        assert call(**{name: None}) == -5, name
    assert call(out=None, bf=None) == -5
    assert call(x=None) == -5 and call(xq=xq) == -5                  # neither, both
    assert call(x=xf[1:]) == -2 and call(x=None, xq=xq[1:]) == -2 and call(out=out[1:]) == -2 and call(bf=bf[1:]) == -2
    misaligned_src = src.view(torch.uint8)[1:33].view(torch.int8)     # one byte past a 4-byte boundary
    assert call(src=misaligned_src) == -2
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((bf == 3.0).all())
    assert call() == 0 and call(x=None, xq=xq) == 0 and call(out=None) == 0 and call(bf=None) == 0      # the accepted calls, for contrast
    torch.cuda.synchronize()
    assert not bool((out[:Rp * F] == 3.0).any()) and bool((out[Rp * F:] == 3.0).all()) and bool((bf[Rp * F:] == 3.0).all())


# ---------------------------------------------------------------------------- 6. the selected tower against float64
def _params(tw):
    pre = tw.scope + "/"
    return {k[len(pre):]: _np(v) for k, v in tw.state_dict().items()}


def _frames_of(table):
    return [row[row >= 0].astype(np.int64) for row in table]


def _tf_grad(tw, k):
    got = tw.store.g(k)
    got = _np(got.t() if got.dim() == 2 else got)
    if k == tw.HW:
        got = got.reshape(tw.Kc, tw.F, tw.Hd).transpose(1, 0, 2).reshape(tw.F * tw.Kc, tw.Hd)
    return got


B6, F6, K6, H6, V6, T6, E6 = 32, 128, 64, 128, 33, 60, 10
_BATCH = {}


def _batch6():
    """The batch of tests 6 and 8, made once: one empty video, one of 3 frames (k = 0 as well), one of 60."""
    if not _BATCH:
        q, x, n, labels = mm.synthetic_batch(B6, seed=B6, max_frames=T6, feature_size=F6, vocab_size=V6, dtype=np.float32)
        n[4], n[11], n[20] = 0, 3, 60
        x[np.arange(T6)[None, :] >= n[:, None]] = 0.0
        _BATCH.update(q=q, x=x, n=n, labels=labels, xn=mm.l2_normalize(x.astype(np.float64), 2))
    return _BATCH


@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("word", ["last", "segment_change"])
def test_selected_tower_against_float64(word, u8):
    """B = 32, F = 128, K = 64, H = 128, V = 33, T = 60, every_n = 10 against tests/_netvlad_packed_ref.py fed the table's rows, under
    the bounds of DESIGN.md 7.18 and none new: a 2e-2, Y_bf 2e-2, predictions 5e-3, every gradient tensor relative L2 0.12 or max abs
    1e-3; then a forward-only tower on perturbed moving statistics under the 5e-3 bound."""
    from efficientvideoclassification_youtube8m_amd import ops
    from efficientvideoclassification_youtube8m_amd.towers import NetVladTower
    bt = _batch6()
    n, labels, xn = bt["n"], bt["labels"], bt["xn"]
    rng = np.random.default_rng(B6 + K6)
    kw = dict(cluster_size=K6, hidden_size=H6, device=DEV, frames="grid", every_n=E6, sampling=word)
    tw = NetVladTower(B6, T6, F6, V6, seed=3, **kw)
    for k in tw.names:
        if k.endswith("/gamma") or k.endswith("/beta"):
            tw.store.p(k).add_(torch.from_numpy(rng.standard_normal(tw.store.p(k).shape).astype(np.float32) * 0.2).to(DEV))
    P = _params(tw)
    xin, nd = torch.from_numpy(bt["q"] if u8 else bt["x"]).to(DEV), torch.from_numpy(n).to(DEV)
    pred = tw.forward(xin, nd, num_frames_host=n)
    table = tw.last_frame_table.cpu().numpy()
    k_want = np.array([fs.student_count(int(v), T6, T6 // E6) for v in n], np.int32)
    assert table.shape == (B6, T6 // E6) and np.array_equal((table >= 0).sum(axis=1), k_want) and np.array_equal(tw.plan.k, k_want)
    assert k_want[4] == 0 and k_want[11] == 0 and k_want[20] == 6
    if word == "last":
        assert np.array_equal(table, fs.table(n, T6, E6, "last"))
    else:
        live = [row[row >= 0] for row in table]
        assert all((np.diff(r) > 0).all() and (r < nb).all() for r, nb in zip(live, n))
        assert not np.array_equal(table, fs.table(n, T6, E6, "last"))
    ref_pred, cache = nv.netvlad_packed_fwd(xn, n, E6, P, frames=_frames_of(table))
    R = cache["r"].shape[0]
    assert (tw.R, tw.Rp) == (R, ops.round_up(R, 32)) and np.array_equal(tw.row_off.cpu().numpy(), cache["row_off"])
    assert not tw.r_bn[R:tw.Rp].any() and not tw.Vv[4].any() and not tw.Vv[11].any()
    Yk = lambda Y: Y.reshape(B6, F6, K6).transpose(0, 2, 1).reshape(B6, K6 * F6)
    err_r = np.abs(_np(tw.r[:R]) - cache["r"]).max()
    err_a = np.abs(_np(tw.a[:R]) - cache["a"]).max()
    err_y = np.abs(tw.Y_bf[:B6].float().cpu().numpy() - Yk(cache["Y"])).max()
    err = np.abs(_np(pred) - ref_pred).max()
    print("netvlad %s u8=%d R=%d: r err %.2e  a err %.2e  Y_bf err %.2e  pred err %.2e" % (word, u8, R, err_r, err_a, err_y, err))
    missed = [(w, e, b) for w, e, b in (("r", err_r, 1e-6), ("a", err_a, 2e-2), ("Y_bf", err_y, 2e-2), ("pred", err, 5e-3)) if not e < b]
    dp = mm.cross_entropy_grad(ref_pred, labels)
    tw.backward(torch.from_numpy(dp.astype(np.float32)).to(DEV))
    assert not tw.dact_bf[R:tw.Rp].any()
    gref = nv.netvlad_packed_bwd(dp, cache)
    assert set(gref) == set(tw.names)
    for k, g in gref.items():
        got = _tf_grad(tw, k)
        l2 = float(np.linalg.norm(got - g) / (np.linalg.norm(g) + 1e-30))
        mx = float(np.abs(got - g).max())
        print("  grad %-28s rel l2 %.3e  max abs %.3e" % (k, l2, mx))
        if not (l2 < 0.12 or mx < 1e-3):
            missed.append(("grad " + k, (l2, mx), (0.12, 1e-3)))
    sd = tw.state_dict()
    stats = {}
    for s in ("input_bn", "cluster_bn", "hidden1_bn"):
        m, v = sd["model/%s/moving_mean" % s], sd["model/%s/moving_variance" % s]
        m.add_(torch.from_numpy(rng.standard_normal(m.shape).astype(np.float32) * 0.05).to(DEV))
        v.mul_(torch.from_numpy((1.0 + 0.2 * rng.random(v.shape)).astype(np.float32)).to(DEV))
        stats[s] = (_np(m), _np(v))
    ev = NetVladTower(B6, T6, F6, V6, seed=9, training=False, **kw)
    assert ev.store.grad is None and ev.store.m is None
    ev.load_state_dict(sd)
    pred_e = ev.forward(xin, nd, num_frames_host=n, is_training=False)
    assert torch.equal(ev.last_frame_table, tw.last_frame_table) and ev.R == R and not ev.r_bn[R:ev.Rp].any()
    ref_e, cache_e = nv.netvlad_packed_fwd(xn, n, E6, P, frames=_frames_of(table), stats=stats)
    ee_a = np.abs(_np(ev.a[:R]) - cache_e["a"]).max()
    ee_y = np.abs(ev.Y_bf[:B6].float().cpu().numpy() - Yk(cache_e["Y"])).max()
    ee = np.abs(_np(pred_e) - ref_e).max()
    print("  forward only: a err %.2e  Y_bf err %.2e  pred err %.2e" % (ee_a, ee_y, ee))
    missed += [("eval " + w, e, b) for w, e, b in (("a", ee_a, 2e-2), ("Y_bf", ee_y, 2e-2), ("pred", ee, 5e-3)) if not e < b]
    assert not missed, missed


def test_selected_tower_refuses_a_batch_without_frames():
    """Every video shorter than every_n: k_b = 0 for all, the grid towers' ValueError."""
    from efficientvideoclassification_youtube8m_amd.towers import NetVladTower
    tw = NetVladTower(4, 20, 64, 10, cluster_size=64, hidden_size=64, device=DEV, frames="grid", every_n=5, training=False, sampling="last")
    x = torch.zeros((4, 20, 64), device=DEV)
    n = np.array([4, 0, 3, 1], np.int32)
    with pytest.raises(ValueError, match="--netvlad_frames grid: no video of the batch has a frame"):
        tw.forward(x, torch.from_numpy(n).to(DEV), num_frames_host=n)


# ---------------------------------------------------------------------------- 7. random
def test_random_tables_follow_the_step_and_survive_a_restore(tmp_path):
    """SingleTowerGraph over a sampling="random" tower: the table of step s is _frame_select_ref.table(seed, draw = s, row0 = 0); the two
    steps' tables differ; a graph restored from the checkpoint written after step 1 draws step 2's table."""
    from efficientvideoclassification_youtube8m_amd import train
    from efficientvideoclassification_youtube8m_amd.distill import SingleTowerGraph
    from efficientvideoclassification_youtube8m_amd.towers import NetVladTower
    B, T, F, V, E = 8, 60, 64, 20, 10
    q, x, n, labels = mm.synthetic_batch(B, seed=5, max_frames=T, feature_size=F, vocab_size=V, dtype=np.float32)
    n = np.array([60, 45, 0, 33, 10, 59, 21, 7], np.int32)
    qd, yd, nd =torch.from_numpy(q).to(DEV), torch.from_numpy(labels.astype(np.uint8)).to(DEV), torch.from_numpy(n).to(DEV)
    make = lambda: SingleTowerGraph(NetVladTower(B, T, F, V, cluster_size=64, hidden_size=64, device=DEV, seed=5, frames="grid", every_n=E,
                                                 sampling="random", sampling_seed=77), base_learning_rate=0.01)
    g = make()
    tables = []
    for step in range(2):
        assert g.global_step == step
        out = g.step(qd, yd, nd, num_frames_host=n)
        assert np.isfinite(float(out["loss"]))
        tables.append(g.tower.last_frame_table.cpu().numpy().copy())
        assert np.array_equal(tables[-1], fs.table(n, T, E, "random", seed=77, draw=step, row0=0))
        if step == 0:
            train.save_checkpoint(g, str(tmp_path), 0)
    assert not np.array_equal(tables[0], tables[1])
    sd = torch.load(train.latest_checkpoint(str(tmp_path)))
    assert (sd["global_step"], sd["student_sampling"], sd["student_sampling_seed"], sd["netvlad_frames"], sd["every_n"]) == (1, "random", 77, "grid", E)
    g2 = make()
    train.restore_checkpoint(g2, train.latest_checkpoint(str(tmp_path)))
    assert g2.global_step == 1
    g2.step(qd, yd, nd, num_frames_host=n)
    assert np.array_equal(g2.tower.last_frame_table.cpu().numpy(), tables[1])


# ---------------------------------------------------------------------------- 8. distillation against float64
def _perturb(tw, rng, moving):
    for k in tw.names:
        if k.endswith("/gamma") or k.endswith("/beta"):
            z = torch.from_numpy(rng.standard_normal(tw.store.p(k).shape).astype(np.float32) * 0.2).to(DEV)
            tw.store.p(k).copy_(tw.store.p(k) * torch.exp(z) if k.endswith("/gamma") else tw.store.p(k) + z)
    tw.refresh_shadows()
    if moving:
        for k, v in tw.buffers.items():
            z = torch.from_numpy(rng.standard_normal(v.shape).astype(np.float32) * 0.2).to(DEV)
            v.copy_(v * torch.exp(z) if k.endswith("variance") else v + z)


@pytest.mark.parametrize("on", [("rep", "pred", "ce"), ("pred",)])
def test_distillation_step_against_float64(on):
    """Teacher on every real frame, student on "last" at every_n = 10, the shape of DESIGN.md 7.19's step test (B = 32, F = 128, K = 64,
    H = 128, V = 33, T = 60; uint8 input): against the float64 step built from tests/_netvlad_packed_ref.py with explicit frames, under
    7.19's bounds - the losses 2e-2 relative + 1e-6, predictions 5e-3, a and Y_bf 2e-2, gradients relative L2 0.12 or 1e-3 absolute.
    With distill_losses = pred, dstate is exactly zero."""
    from efficientvideoclassification_youtube8m_amd.distill import NetVladDistillGraph
    bt = _batch6()
    n, labels, xn = bt["n"], bt["labels"], bt["xn"]
    rng = np.random.default_rng(B6 + K6 + 1)
    g = NetVladDistillGraph(B6, every_n=E6, teacher_every_n=1, feature_size=F6, vocab_size=V6, max_frames=T6, cluster_size=K6,
                            hidden_size=H6, device=DEV, seed=3, distill_losses=on, student_sampling="last")
    assert (g.student.sampling, g.teacher.sampling, g.student_sampling) == ("last", "uniform", "last")
    _perturb(g.teacher, rng, True)
    _perturb(g.student, rng, False)
    teacher, student = _params(g.teacher), _params(g.student)
    moving = {k: teacher.pop(k) for k in list(teacher) if "/moving_" in k}
    for k in list(student):
        if "/moving_" in k:
            student.pop(k)
    frames = _frames_of(fs.table(n, T6, E6, "last"))
    t_pred, t_state, t_cache = dx.netvlad_packed_eval_fwd(xn, n, 1, teacher, moving)
    s_pred, s_cache = nv.netvlad_packed_fwd(xn, n, E6, student, frames=frames)
    vals, total, dpred, dstate = dx.distill_losses(t_pred, t_state, s_pred, s_cache["h6"], labels, 2.0, on)
    ref = dict(vals, total=total)
    grads = dx.netvlad_packed_bwd(dpred, s_cache, dstate)
    y = torch.from_numpy(labels.astype(np.uint8)).to(DEV)
    t_before = g.teacher.store.master.clone()
    out = g.step(torch.from_numpy(bt["q"]).to(DEV), y, torch.from_numpy(n).to(DEV), apply=False, num_frames_host=n)
    torch.cuda.synchronize()
    assert g.global_step == 0 and torch.equal(g.teacher.store.master, t_before)
    ts, tt = g.student, g.teacher
    R, Rt = s_cache["r"].shape[0], t_cache["r"].shape[0]
    assert ts.R == R and tt.R == Rt and np.array_equal(ts.plan.k, s_cache["k"]) and np.array_equal(out["num_frames_student"].numpy(), s_cache["k"])
    assert np.array_equal(ts.last_frame_table.cpu().numpy(), fs.table(n, T6, E6, "last")) and tt.last_frame_table is None
    rep = g.loss_report()
    missed = []
    for k in g.LOSS_SLOTS:
        print("on=%s loss %-20s got %.6f  float64 %.6f" % (",".join(on), k, rep[k], float(ref[k])))
        if not abs(rep[k] - ref[k]) <= 2e-2 * abs(ref[k]) + 1e-6:
            missed.append((k, rep[k], float(ref[k])))
    Yk = lambda Y: Y.reshape(B6, F6, K6).transpose(0, 2, 1).reshape(B6, K6 * F6)
    figures = (("teacher pred", np.abs(_np(out["predictions"]) - t_pred).max(), 5e-3),
               ("student a", np.abs(_np(ts.a[:R]) - s_cache["a"]).max(), 2e-2),
               ("student Y_bf", np.abs(ts.Y_bf[:B6].float().cpu().numpy() - Yk(s_cache["Y"])).max(), 2e-2),
               ("student pred", np.abs(_np(out["student_predictions"]) - s_pred).max(), 5e-3),
               ("dstate", np.abs(_np(g.state_grad()) - dstate).max(), None))
    for what, e, bound in figures:
        print("on=%s %-14s err %.2e%s" % (",".join(on), what, e, "" if bound is None else "  (bound %.0e)" % bound))
        if bound is not None and not e < bound:
            missed.append((what, e, bound))
    if on == ("pred",):
        assert not g.state_grad().any() and not dstate.any()
    else:
        assert g.state_grad().any()
    assert set(grads) == set(ts.names)
    for k, want in grads.items():
        got = _tf_grad(ts, k)
        l2 = float(np.linalg.norm(got - want) / (np.linalg.norm(want) + 1e-30))
        mx = float(np.abs(got - want).max())
        print("on=%s   grad %-28s rel l2 %.3e  max abs %.3e" % (",".join(on), k, l2, mx))
        if not (l2 < 0.12 or mx < 1e-3):
            missed.append(("grad " + k, (l2, mx), (0.12, 1e-3)))
    assert not missed, missed


# ---------------------------------------------------------------------------- 5. / 9. / 10. two towers compared bit for bit: a process of its own
@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """tests/_netvlad_select_child.py, once, in a fresh process under EVC_DETERMINISTIC=1 (the library reads it once per process)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    work = str(tmp_path_factory.mktemp("netvlad_select"))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "_netvlad_select_child.py"), work],
                       env=dict(os.environ, EVC_DETERMINISTIC="1"), capture_output=True, text=True, timeout=600)
    lines = [line for line in r.stdout.splitlines() if not line.startswith("Key: ")]
    print("\n".join(lines)[-8000:])
    return r, "\n".join(lines)


def test_first_is_a_truncated_video(child):
    """A training tower with sampling="first" at every_n = 10 against a grid tower at every_n = 1 fed num_frames = k_b (B = 8, T = 40,
    F = 128, K = 64, H = 64; uint8 and f32 input): r, a, V, the predictions and every gradient after one backward, bit for bit."""
    r, out = child
    assert "deterministic 1" in out and "first: ok" in out and "DIFFERS" not in out, out[-3000:] + r.stderr[-3000:]
    for u8 in (0, 1):
        for name in ("r", "a", "V", "predictions"):
            assert any(line.split() == ["first", "u8=%d" % u8, name, "equal"] for line in out.splitlines()), (u8, name)
        assert sum(line.startswith("first u8=%d grad " % u8) and line.endswith("equal") for line in out.splitlines()) == 12


def test_two_random_graphs_take_the_same_steps_bit_for_bit(child):
    r, out = child
    assert "twice: ok" in out, out[-3000:] + r.stderr[-3000:]
    for step in (0, 1):
        for name in ("table", "loss", "gradient store", "master weights"):
            assert any(line.startswith("twice step %d: %s" % (step, name)) and line.endswith("equal") for line in out.splitlines()), (step, name)


def test_train_and_validate_end_to_end(child):
    """train.main --student_sampling segment_change, then --teacher_dir ... --student_sampling last: finite losses, the metadata, model/*
    the teacher's bits; validate.main --student_sampling last equals eval_util on a fresh forward-only tower on that word; without the
    flag the warning appears and the grid's predictions are served."""
    r, out = child
    assert "workflow: ok" in out and r.returncode == 0, out[-3000:] + r.stderr[-3000:]
    assert "workflow: validate --student_sampling last" in out and "workflow: validate --student_sampling uniform" in out
