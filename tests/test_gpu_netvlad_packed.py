"""NetVLAD over a ragged, packed list of frames per video (--netvlad_frames grid): the two packed entries of
csrc/evc_netvlad.hip per element against numpy float64 under the DERIVED bounds of tests/_netvlad_packed_ref.py, against the
fixed-length entries on equal lengths, their refusals; the ragged tower against its float64 restatement; train.main and validate.main
end to end; run-to-run determinism in a child process.  pytest -m gpu.  Every test prints the figures it judges before it asserts;
what an MI355X gave is recorded in DESIGN.md 7.18."""
import ctypes
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _netvlad_packed_ref as nv
import _vlad_ref as vr
from oracle import model_math as mm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _np(t):
    return t.detach().cpu().double().numpy()


def _d(a, pad_rows=0):
    """The array on the device, followed by pad_rows rows of NaN (rows >= R of an operand: never read)."""
    a = np.ascontiguousarray(a, np.float32)
    if pad_rows:
        a = np.concatenate([a, np.full((pad_rows,) + a.shape[1:], np.nan, np.float32)], axis=0)
    return torch.from_numpy(a).to(DEV)


def _twice(fn, *outs):
    """fn() fills `outs`; a second call on the same inputs must give the same bits (fixed-order sums, no atomics).  NaN guards compare
    as bit patterns."""
    fn()
    first = [o.clone() for o in outs]
    fn()
    torch.cuda.synchronize()
    for o, f in zip(outs, first):
        assert torch.equal(o.view(torch.int32), f.view(torch.int32))


def _run_packed(c, ops):
    """Both packed entries on a case: outputs prefilled with NaN and longer than the output (guards), rows >= R of a / r NaN, each
    entry twice for equal bits.  -> dict name -> numpy buffer."""
    B, K, F, R = c.B, c.K, c.F, c.R
    a, r = _d(c.a, 3), _d(c.r, 3)
    off = torch.from_numpy(c.row_off).to(DEV)
    st = [_d(v) for v in (c.mean, c.var, c.gamma, c.beta)]
    c2, dV = _d(c.c2), _d(c.dV)
    V = torch.full((B + 1, K, F), NAN, device=DEV)
    asum = torch.full((B + 1, K), NAN, device=DEV)
    _twice(lambda: ops.netvlad_aggregate_packed_fwd(a, r, off, B, c.T, K, F, R, c.max_k, *st, c2, V, asum), V, asum)
    da = torch.full((R + 5, K), NAN, device=DEV)
    dx = torch.full((R + 5, F), NAN, device=DEV)
    _twice(lambda: ops.netvlad_aggregate_packed_bwd(a, r, off, B, c.T, K, F, R, c.max_k, *st, c2, dV, da, dx), da, dx)
    return dict(V=V.cpu().numpy(), asum=asum.cpu().numpy(), da=da.cpu().numpy(), dx=dx.cpu().numpy())


@pytest.mark.parametrize("K,F,ks", nv.NV_PACKED)
def test_packed_entries_per_element_against_float64(K, F, ks):
    """evc_netvlad_aggregate_packed_fwd / _bwd: every element of V, asum, dx, da within its derived bound of the float64 reference (no
    element exempt, not finite = inf); the guards behind every output keep their NaN (nothing beyond R or beyond B K F is written);
    empty videos give exact zeros."""
    from efficientvideoclassification_youtube8m_amd import ops
    c = nv.packed_case(K, F, ks)
    ref = nv.agg_ref(c)
    got = _run_packed(c, ops)
    q = vr.judge(ref, got)
    assert set(q) == {n + s for n in ("V", "asum", "dx", "da") for s in ("", " guard")}
    line = "  ".join("%s %.3f" % (n, q[n].max() if q[n].size else 0.0) for n in ("V", "asum", "dx", "da"))
    print("packed %s: worst |got - ref| / bound  %s" % (c.name, line))
    missed = {n: vr.worst(v) for n, v in q.items() if v.size and v.max() > 1.0}
    assert not missed, (c.name, missed)
    for b, L in enumerate(ks):
        if L == 0:
            assert not got["V"][b].any() and not got["asum"][b].any()          # zeros, not merely small


@pytest.mark.parametrize("B,S,K,F", [(3, 17, 24, 40), (2, 64, 64, 272)])
def test_packed_entries_against_the_fixed_length_entries(B, S, K, F):
    """On equal lengths S <= 64 the packed entries and evc_netvlad_aggregate_fwd / _bwd compute the same quantities in other
    orders: each of V, asum, dx, da differs by at most the sum of the two derived bounds (tests/_vlad_ref.nv_agg_ref's for the
    fixed-length kernels)."""
    from efficientvideoclassification_youtube8m_amd import ops
    c = nv.equal_case(B, S, K, F)
    ref = nv.agg_ref(c)
    got = _run_packed(c, ops)
    fc = vr.Case()
    fc.B, fc.S, fc.K, fc.F = B, S, K, F
    fc.r, fc.a = c.r.reshape(B, S, F), c.a.reshape(B, S, K)
    fc.mean, fc.var, fc.gamma, fc.beta, fc.c2, fc.dV = c.mean, c.var, c.gamma, c.beta, c.c2, c.dV
    fref = vr.nv_agg_ref(fc)
    a, r = _d(c.a), _d(c.r)
    st = [_d(v) for v in (c.mean, c.var, c.gamma, c.beta)]
    c2, dV = _d(c.c2), _d(c.dV)
    V = torch.empty((B, K, F), device=DEV); asum = torch.empty((B, K), device=DEV)
    da = torch.empty((B * S, K), device=DEV); dx = torch.empty((B * S, F), device=DEV)
    ops.netvlad_aggregate_fwd(a, r, B, S, K, F, *st, c2, V, asum)
    ops.netvlad_aggregate_bwd(a, r, B, S, K, F, *st, c2, dV, da, dx)
    fixed = dict(V=_np(V), asum=_np(asum), da=_np(da), dx=_np(dx))
    R = B * S
    body = dict(V=got["V"][:B], asum=got["asum"][:B], da=got["da"][:R], dx=got["dx"][:R])
    worst = {}
    for name in ("V", "asum", "dx", "da"):
        lim = ref[name].d + np.reshape(fref[name].d, ref[name].d.shape)
        diff = np.abs(body[name].astype(np.float64) - fixed[name].reshape(body[name].shape))
        assert np.isfinite(diff).all()
        worst[name] = float(np.where(diff == 0.0, 0.0, diff / lim).max())
    print("packed against fixed B=%d S=%d K=%d F=%d: |packed - fixed| / (sum of the two bounds)  %s"
          % (B, S, K, F, "  ".join("%s %.3f" % kv for kv in worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_packed_entries_refuse_before_any_launch():
    """For both entries: a bad shape is EVC_ERR_BAD_SHAPE (-1), a NULL operand EVC_ERR_BAD_ARG (-5), a misaligned pointer
    EVC_ERR_BAD_ALIGN (-2), a short ws EVC_ERR_BAD_ARG (-5); the outputs keep what they held."""
    from efficientvideoclassification_youtube8m_amd import _lib, ops
    lib = _lib.load()
    B, T, K, F, R, max_k = 2, 8, 8, 8, 6, 4
    off = torch.tensor([0, 2, 6], dtype=torch.int32, device=DEV)
    a = torch.zeros((R + 1, K), device=DEV); r = torch.zeros((R + 1, F), device=DEV)
    st = [torch.ones(F, device=DEV) for _ in range(4)]
    c2 = torch.zeros((K + 1, F), device=DEV); dV = torch.zeros((B, K, F), device=DEV)
    V = torch.full((B, K, F), 3.0, device=DEV); asum = torch.full((B, K), 3.0, device=DEV)
    da = torch.full((R + 1, K), 3.0, device=DEV); dx = torch.full((R + 1, F), 3.0, device=DEV)
    n_ws = ops.netvlad_aggregate_packed_bwd_ws(B, K, F)
    ws = torch.zeros(n_ws + 4, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def fwd(shape=(B, T, K, F, R, max_k), **kw):
        t = dict(a=a, r=r, off=off, mean=st[0], var=st[1], gamma=st[2], beta=st[3], c2=c2, V=V, asum=asum)
        t.update(kw)
        b_, t_, k_, f_, r_, m_ = shape
        return lib.evc_netvlad_aggregate_packed_fwd(p(t["a"]), p(t["r"]), p(t["off"]), b_, t_, k_, f_, r_, m_, p(t["mean"]), p(t["var"]),
                                                    p(t["gamma"]), p(t["beta"]), p(t["c2"]), p(t["V"]), p(t["asum"]), stream)

    def bwd(shape=(B, T, K, F, R, max_k), ws_floats=n_ws, **kw):
        t = dict(a=a, r=r, off=off, mean=st[0], var=st[1], gamma=st[2], beta=st[3], c2=c2, dV=dV, da=da, dx=dx, ws=ws)
        t.update(kw)
        b_, t_, k_, f_, r_, m_ = shape
        return lib.evc_netvlad_aggregate_packed_bwd(p(t["a"]), p(t["r"]), p(t["off"]), b_, t_, k_, f_, r_, m_, p(t["mean"]), p(t["var"]),
                                                    p(t["gamma"]), p(t["beta"]), p(t["c2"]), p(t["dV"]), p(t["da"]), p(t["dx"]), p(t["ws"]),
                                                    ws_floats, stream)

    bad_shapes = [(B, T, K, 6, R, max_k), (B, T, K, F, R, 9), (B, T, K, F, R, 2), (0, T, K, F, R, max_k), (65536, T, K, F, R, max_k),
                  (B, T, 0, F, R, max_k), (B, T, 1025, F, R, max_k), (B, T, K, F, 3, max_k), (B, T, K, F, R, -1)]
    for shape in bad_shapes:                     # F % 4; max_k > T; R > B max_k; B; K; R < max_k; max_k < 0
        assert fwd(shape) == -1 and bwd(shape) == -1, shape
    assert b"evc_netvlad_aggregate_packed_bwd" in lib.evc_last_error()
    for name in ("a", "r", "off", "mean", "var", "gamma", "beta", "c2"):
        assert fwd(**{name: None}) == -5 and bwd(**{name: None}) == -5, name
    for name in ("V", "asum"):
        assert fwd(**{name: None}) == -5, name
    for name in ("dV", "da", "dx", "ws"):
        assert bwd(**{name: None}) == -5, name
    off1 = lambda t: t.view(-1)[1:]              # 4 bytes past a 16-byte boundary
    for name in ("a", "r", "c2"):
        assert fwd(**{name: off1({"a": a, "r": r, "c2": c2}[name])}) == -2 and bwd(**{name: off1({"a": a, "r": r, "c2": c2}[name])}) == -2, name
    assert fwd(V=off1(torch.full((B * K * F + 1,), 3.0, device=DEV))) == -2
    for name, t in (("dV", torch.zeros(B * K * F + 1, device=DEV)), ("da", da), ("dx", dx)):
        assert bwd(**{name: off1(t)}) == -2, name
    assert bwd(ws_floats=n_ws - 1) == -5 and bwd(ws=off1(ws)) == -5
    assert b"ws holds" in lib.evc_last_error()
    torch.cuda.synchronize()
    for t in (V, asum, da, dx):
        assert bool((t == 3.0).all())
    assert fwd() == 0 and bwd() == 0             # the accepted call, for contrast
    torch.cuda.synchronize()
    assert not bool((V == 3.0).any()) and bool((da[R:] == 3.0).all()) and bool((dx[R:] == 3.0).all())


def _params(tw):
    pre = tw.scope + "/"
    return {k[len(pre):]: _np(v) for k, v in tw.state_dict().items()}


@pytest.mark.parametrize("every_n,T,u8", [(10, 300, True), (10, 300, False), (1, 40, True), (1, 40, False)])
def test_grid_tower_forward_backward_against_reference(every_n, T, u8):
    """The ragged tower against tests/_netvlad_packed_ref.py at B = 32, F = 128, K = 64, H = 128, V = 33 on the synthetic batch's own
    lengths.  Bounds of test_netvlad_forward_backward_against_oracle - the arithmetic in front of each quantity is the same: a 2e-2,
    Y_bf 2e-2, predictions 5e-3, every gradient tensor relative L2 0.12 or max abs 1e-3.  Then a second batch with another R in the
    same buffers, and a training=False tower on perturbed moving statistics against the reference's evaluation forward."""
    from efficientvideoclassification_youtube8m_amd import ops
    from efficientvideoclassification_youtube8m_amd.towers import NetVladTower
    B, F, K, H, V = 32, 128, 64, 128, 33
    rng = np.random.default_rng(B + K)
    q, x, n, labels = mm.synthetic_batch(B, seed=B, feature_size=F, vocab_size=V, dtype=np.float32)
    q, x = np.ascontiguousarray(q[:, :T]), np.ascontiguousarray(x[:, :T])
    tw = NetVladTower(B, T, F, V, cluster_size=K, hidden_size=H, device=DEV, seed=3, frames="grid", every_n=every_n)
    for k in tw.names:                                   # non-trivial batch-norm scale / offset
        if k.endswith("/gamma") or k.endswith("/beta"):
            tw.store.p(k).add_(torch.from_numpy(rng.standard_normal(tw.store.p(k).shape).astype(np.float32) * 0.2).to(DEV))
    P = _params(tw)
    xin, nd = torch.from_numpy(q if u8 else x).to(DEV), torch.from_numpy(n).to(DEV)
    pred = tw.forward(xin, nd, num_frames_host=n)
    xn = mm.l2_normalize(x.astype(np.float64), 2)
    ref_pred, cache = nv.netvlad_packed_fwd(xn, n, every_n, P)
    R = cache["r"].shape[0]
    assert (tw.R, tw.Rp) == (R, ops.round_up(R, 32)) and np.array_equal(tw.plan.k, cache["k"])
    assert np.array_equal(tw.row_off.cpu().numpy(), cache["row_off"])
    assert not tw.r_bn[R:tw.Rp].any()                    # the padding rows of the forward TN operand
    Yk = lambda Y: Y.reshape(B, F, K).transpose(0, 2, 1).reshape(B, K * F)             # reference order f*K+k -> cluster-major
    err_r = np.abs(_np(tw.r[:R]) - cache["r"]).max()
    err_a = np.abs(_np(tw.a[:R]) - cache["a"]).max()
    err_y = np.abs(tw.Y_bf[:B].float().cpu().numpy() - Yk(cache["Y"])).max()
    err = np.abs(_np(pred) - ref_pred).max()
    print("netvlad grid every_n=%d T=%d u8=%d R=%d: r err %.2e  a err %.2e  Y_bf err %.2e  pred err %.2e" % (every_n, T, u8, R, err_r, err_a, err_y, err))
    # every bound is evaluated (and every figure printed) before the first one fails the test
    missed = [(w, e, b) for w, e, b in (("r", err_r, 1e-6), ("a", err_a, 2e-2), ("Y_bf", err_y, 2e-2), ("pred", err, 5e-3)) if not e < b]
    dp = mm.cross_entropy_grad(ref_pred, labels)
    tw.backward(torch.from_numpy(dp.astype(np.float32)).to(DEV))
    assert not tw.dact_bf[R:tw.Rp].any()                 # the padding rows of the backward TN operand
    gref = nv.netvlad_packed_bwd(dp, cache)
    assert set(gref) == set(tw.names)
    for k, g in gref.items():
        got = tw.store.g(k)
        got = _np(got.t() if got.dim() == 2 else got)
        if k == tw.HW:
            got = got.reshape(K, F, H).transpose(1, 0, 2).reshape(F * K, H)
        l2 = float(np.linalg.norm(got - g) / (np.linalg.norm(g) + 1e-30))
        mx = float(np.abs(got - g).max())
        print("  grad %-28s rel l2 %.3e  max abs %.3e" % (k, l2, mx))
        if not (l2 < 0.12 or mx < 1e-3):
            missed.append(("grad " + k, (l2, mx), (0.12, 1e-3)))
    # a forward-only tower on perturbed moving statistics against the reference's evaluation forward
    sd = tw.state_dict()
    stats = {}
    for s in ("input_bn", "cluster_bn", "hidden1_bn"):
        m, v = sd["model/%s/moving_mean" % s], sd["model/%s/moving_variance" % s]
        m.add_(torch.from_numpy(rng.standard_normal(m.shape).astype(np.float32) * 0.05).to(DEV))
        v.mul_(torch.from_numpy((1.0 + 0.2 * rng.random(v.shape)).astype(np.float32)).to(DEV))
        stats[s] = (_np(m), _np(v))
    ev = NetVladTower(B, T, F, V, cluster_size=K, hidden_size=H, device=DEV, seed=9, frames="grid", every_n=every_n, training=False)
    assert ev.store.grad is None and ev.store.m is None
    ev.load_state_dict(sd)
    pred_e = ev.forward(xin, nd, num_frames_host=n, is_training=False)
    ref_e, cache_e = nv.netvlad_packed_fwd(xn, n, every_n, P, stats=stats)
    ee_a = np.abs(_np(ev.a[:R]) - cache_e["a"]).max()
    ee_y = np.abs(ev.Y_bf[:B].float().cpu().numpy() - Yk(cache_e["Y"])).max()
    ee = np.abs(_np(pred_e) - ref_e).max()
    print("  forward only: a err %.2e  Y_bf err %.2e  pred err %.2e" % (ee_a, ee_y, ee))
    missed += [("eval " + w, e, b) for w, e, b in (("a", ee_a, 2e-2), ("Y_bf", ee_y, 2e-2), ("pred", ee, 5e-3)) if not e < b]
    assert np.array_equal(_np(ev.buffers["input_bn/moving_mean"]), stats["input_bn"][0])      # an evaluation forward leaves them alone
    # a second batch with another R: forward and backward in the same buffers
    names = ("r", "r_bn", "act", "a", "da", "dz", "dx", "dact_bf", "agg_ws", "row_off")
    ptrs = {name: getattr(tw, name).data_ptr() for name in names}
    n2 = np.maximum(n // 2, 1).astype(np.int32)
    pred2 = tw.forward(xin, torch.from_numpy(n2).to(DEV), num_frames_host=n2)
    ref2, cache2 = nv.netvlad_packed_fwd(xn, n2, every_n, P)
    tw.backward(torch.from_numpy(mm.cross_entropy_grad(ref2, labels).astype(np.float32)).to(DEV))
    torch.cuda.synchronize()
    err2 = np.abs(_np(pred2) - ref2).max()
    print("  second batch R=%d: pred err %.2e" % (tw.R, err2))
    assert tw.R == cache2["r"].shape[0] and (tw.R != R or T == 40) and torch.isfinite(tw.store.grad).all()
    assert not tw.r_bn[tw.R:tw.Rp].any() and not tw.dact_bf[tw.R:tw.Rp].any()
    assert ptrs == {name: getattr(tw, name).data_ptr() for name in names}
    if not err2 < 5e-3:
        missed.append(("pred of the second batch", err2, 5e-3))
    assert not missed, missed


def test_grid_tower_refuses_a_batch_without_frames():
    from efficientvideoclassification_youtube8m_amd.towers import NetVladTower
    tw = NetVladTower(4, 20, 64, 10, cluster_size=64, hidden_size=64, device=DEV, frames="grid", every_n=2, training=False)
    x = torch.zeros((4, 20, 64), device=DEV)
    n = np.zeros(4, np.int32)
    with pytest.raises(ValueError, match="--netvlad_frames grid: no video of the batch has a frame"):
        tw.forward(x, torch.from_numpy(n).to(DEV), num_frames_host=n)


SIZES = ["--frame_features", "True", "--feature_names", "rgb, audio", "--feature_sizes", "64, 64", "--model", "NetVLADModel",
         "--netvlad_cluster_size", "64", "--netvlad_hidden_size", "64", "--batch_size", "16"]


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """train.main --netvlad_frames grid --every_n 10 on synthetic data: 64 videos in 4 steps, once for the tests below."""
    from efficientvideoclassification_youtube8m_amd import train
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    d = str(tmp_path_factory.mktemp("netvlad_grid")) + "/"
    FLAGS.reset()
    res = train.main(SIZES + ["--train_data_pattern", "synthetic", "--netvlad_frames", "grid", "--every_n", "10", "--synthetic_videos", "64",
                              "--num_epochs", "1", "--start_new_model", "True", "--base_learning_rate", "0.01", "--train_dir", d])
    FLAGS.reset()
    return dict(dir=d, res=res)


def test_grid_through_train_main(trained):
    """Finite losses; the checkpoint records the mode and the grid under the same variable names and shapes; a fresh forward-only grid
    tower restored from it reproduces the trained tower's evaluation predictions bit for bit; a sampled tower loads the same file;
    frame_level_models.NetVLADModel.create_model passes the mode through."""
    from efficientvideoclassification_youtube8m_amd import frame_level_models, train
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    from efficientvideoclassification_youtube8m_amd.towers import NetVladTower
    res = trained["res"]
    g = res["graph"]
    tw = g.tower
    assert res["iterations"] == 4 and g.global_step == 4 and tw.frames == "grid" and tw.every_n == 10
    losses = [h[1]["loss"] for h in res["history"]]
    print("netvlad grid train losses", losses, "rows of the last batch", tw.R)
    assert len(losses) == 4 and all(np.isfinite(l) for l in losses)
    sd = torch.load(train.latest_checkpoint(trained["dir"]))
    assert sd["netvlad_frames"] == "grid" and sd["every_n"] == 10 and "nextvlad_frames" not in sd
    assert sd["model/hidden1_weights"].shape == (128 * 64, 64) and sd["model/cluster_weights2"].shape == (128, 64)      # same names and shapes
    q, x, n, labels = mm.synthetic_batch(16, seed=4, feature_size=128, vocab_size=train.NUM_CLASSES, dtype=np.float32)
    qd, nd = torch.from_numpy(q).to(DEV), torch.from_numpy(n).to(DEV)
    kw = dict(max_frames=300, feature_size=128, vocab_size=train.NUM_CLASSES, cluster_size=64, hidden_size=64, device=DEV)
    last = tw.forward(qd, nd, num_frames_host=n, is_training=False).clone()
    fresh = NetVladTower(16, frames="grid", every_n=10, seed=9, training=False, **kw)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.forward(qd, nd, num_frames_host=n, is_training=False), last)
    sampled = NetVladTower(16, iterations=10, seed=9, **kw)
    sampled.load_state_dict(sd)
    assert torch.equal(sampled.store.master, fresh.store.master)
    FLAGS.reset()
    FLAGS.parse(["--netvlad_cluster_size", "64", "--netvlad_hidden_size", "64", "--netvlad_frames", "grid", "--every_n", "10"])
    try:
        m = frame_level_models.NetVLADModel()
        out = m.create_model(torch.from_numpy(x).to(DEV), 20, nd, normalize_input=True, num_frames_host=n)
        assert m.towers["model"].frames == "grid" and m.towers["model"].every_n == 10 and m.towers["model"].R == int(np.ceil(n / 10).sum())
        assert tuple(out["predictions"].shape) == (16, 20) and torch.isfinite(out["predictions"]).all()
    finally:
        FLAGS.reset()


def test_validate_end_to_end(trained, caplog):
    """validate.main --run_once True on that checkpoint (24 synthetic videos in batches of 16: a short last batch): Hit@1 / PERR / GAP /
    the per-class APs are exactly what eval_util computes on the host from the predictions of a fresh NetVladEvalGraph, the loss within
    float32 summation; the same numbers with --metrics_on_device True; --netvlad_serve_every_n 30 runs and logs the override;
    ensembles of this family stay unbuilt."""
    from efficientvideoclassification_youtube8m_amd import eval_util, train, validate
    from efficientvideoclassification_youtube8m_amd.distill import NetVladEvalGraph
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    d = trained["dir"]
    args = SIZES + ["--train_dir", d, "--eval_data_pattern", "synthetic", "--synthetic_videos", "24", "--run_once", "True", "--top_k", "20"]
    try:
        FLAGS.reset()
        info = validate.main(args)
        FLAGS.reset()
        on_device = validate.main(args + ["--metrics_on_device", "True"])
        FLAGS.reset()
        g = NetVladEvalGraph(16, every_n=10, feature_size=128, vocab_size=train.NUM_CLASSES, cluster_size=64, hidden_size=64, device=DEV)
        g.restore(torch.load(train.latest_checkpoint(d)))
        evl = eval_util.EvaluationMetrics(train.NUM_CLASSES, 20)
        ptr = g.teacher.r.data_ptr()
        for q, y, n, nh in train.synthetic_batches(16, 128, DEV, 24, 1, 4321):
            out = g.step(q, y, n, num_frames_host=nh)
            assert tuple(out["predictions"].shape) == (q.shape[0], train.NUM_CLASSES)
            assert np.array_equal(out["num_frames"].numpy(), np.ceil(nh / 10).astype(np.int32))
            evl.accumulate(out["predictions"].cpu().numpy(), y.cpu().numpy().astype(np.float32), out["loss"].cpu().numpy())
        assert g.teacher.r.data_ptr() == ptr and g.teacher.B == 8           # the short last batch allocated nothing
        want = evl.get()
        assert info["epoch_id"] == 4
        for got in (info, on_device):
            for k in ("avg_hit_at_one", "avg_perr", "gap"):
                assert got[k] == want[k], (k, got[k], want[k])
            assert np.array_equal(np.asarray(got["aps"]), np.asarray(want["aps"]))
            assert abs(got["avg_loss"] - want["avg_loss"]) <= 1e-5 * abs(want["avg_loss"])
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            other = validate.main(args + ["--netvlad_serve_every_n", "30"])
        FLAGS.reset()
        assert any("--netvlad_serve_every_n 30" in r.getMessage() and "every_n = 10" in r.getMessage() for r in caplog.records)
        assert other["epoch_id"] == 4 and np.isfinite(other["avg_loss"])
        with pytest.raises(NotImplementedError, match="NetVLADModel has no path here"):
            validate.main(args + ["--ensemble_dirs", d + "," + d])
    finally:
        FLAGS.reset()


def test_two_graphs_take_the_same_steps_bit_for_bit():
    """tests/_netvlad_grid_twice.py in a fresh process under EVC_DETERMINISTIC=1: loss, gradient store and master weights of two graphs
    agree after each of two steps (the second on another row count)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "_netvlad_grid_twice.py")], env=dict(os.environ, EVC_DETERMINISTIC="1"),
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "step 1: master weights" in r.stdout and "DIFFERS" not in r.stdout and "deterministic 1" in r.stdout
