"""NeXtVLAD over a ragged, packed list of frames per video (--nextvlad_frames grid): the packed entries of
csrc/evc_nextvlad.hip alone in f32 against numpy float64, their bit equivalence with the fixed-length path on equal lengths (in a
child process under EVC_DETERMINISTIC=1), the ragged tower against its float64 restatement tests/_nextvlad_packed_ref.py, and
train.main end to end.  pytest -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _nextvlad_packed_ref as px
from oracle import model_math as mm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _np(t):
    return t.detach().cpu().double().numpy()


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _twice(fn, *outs):
    """fn() fills `outs`; a second call on the same inputs must give the same bits (fixed-order sums, no atomics)."""
    fn()
    first = [o.clone() for o in outs]
    fn()
    torch.cuda.synchronize()
    for o, f in zip(outs, first):
        assert torch.equal(o, f)


# P_b = k_b * G = 0, 4, 64, 68, 132, 160: no row; fewer rows than the smallest row tile; exactly one pass of 64 contraction rows; one
# row into the second pass; several row tiles, with workgroups that leave early for the short videos.  K = 18 is no multiple of 4
# (padded transposed dV, da stored element by element), D / 4 = 5 is odd.  Second shape: G = 3, the empty video first and last.
@pytest.mark.parametrize("G,K,D,ks", [(4, 18, 20, (0, 1, 16, 17, 33, 40)), (3, 7, 12, (0, 5, 2, 0))])
def test_packed_aggregation_in_f32_against_numpy(G, K, D, ks):
    """evc_nextvlad_aggregate_packed_fwd / _bwd against numpy float64 to the bounds of test_nextvlad_kernels_in_f32_against_numpy
    for the same quantities: 1e-4 x max(1, |ref|max) for V, asum and dxe, 1e-3 for da.  Outputs are prefilled with NaN: every element
    of a live row (of V and asum: of every video, the empty ones as zeros) is written, no row beyond R is touched."""
    from efficientvideoclassification_youtube8m_amd import ops
    rng = np.random.default_rng(3 + G)
    B, T = len(ks), 48
    k = np.array(ks)
    off = np.concatenate([[0], np.cumsum(k)]).astype(np.int32)
    R, max_k = int(off[-1]), int(k.max())
    big = lambda ref: max(1.0, float(np.abs(ref).max()))
    a = rng.random((R, G, K)) * rng.random((R, G, 1))
    xe = rng.standard_normal((R, G, D)); c2 = rng.standard_normal((K, D))
    asum_ref = np.zeros((B, K)); V_ref = np.zeros((B, K, D))
    for b in range(B):
        asum_ref[b] = a[off[b]:off[b + 1]].sum((0, 1))
        V_ref[b] = np.einsum("rgk,rgd->kd", a[off[b]:off[b + 1]], xe[off[b]:off[b + 1]]) - asum_ref[b][:, None] * c2
    d_a, d_xe, d_c2, d_off = _d(a.reshape(R, G * K)), _d(xe.reshape(R, G * D)), _d(c2), torch.from_numpy(off).to(DEV)
    V = torch.full((B + 1, K, D), float("nan"), device=DEV); asum = torch.full((B + 1, K), float("nan"), device=DEV)
    _twice(lambda: ops.nextvlad_aggregate_packed_fwd(d_a, d_xe, d_off, B, T, G, K, D, R, max_k, d_c2, V, asum), V[:B], asum[:B])
    assert torch.isnan(V[B]).all() and torch.isnan(asum[B]).all()
    err_v, err_s = np.abs(_np(V[:B]) - V_ref).max(), np.abs(_np(asum[:B]) - asum_ref).max()
    print("packed aggregate fwd: V err %.2e (|ref| %.1f)  asum err %.2e" % (err_v, big(V_ref), err_s))
    assert err_v < 1e-4 * big(V_ref) and err_s < 1e-4 * big(asum_ref)
    for b in np.flatnonzero(k == 0):
        assert not V[b].any() and not asum[b].any()                  # zeros, not merely small
    dV = rng.standard_normal((B, K, D)); d_dV = _d(dV)
    vid = np.repeat(np.arange(B), k)
    da_ref = np.einsum("rkd,rgd->rgk", dV[vid], xe) - np.einsum("bkd,kd->bk", dV, c2)[vid][:, None, :]
    dxe_ref = np.einsum("rgk,rkd->rgd", a, dV[vid])
    da = torch.full((R + 5, G * K), float("nan"), device=DEV); dxe = torch.full((R + 5, G * D), float("nan"), device=DEV)
    _twice(lambda: ops.nextvlad_aggregate_packed_bwd(d_a, d_xe, d_off, B, T, G, K, D, R, max_k, d_c2, d_dV, da, dxe), da[:R], dxe[:R])
    assert torch.isnan(da[R:]).all() and torch.isnan(dxe[R:]).all()
    assert torch.isfinite(da[:R]).all() and torch.isfinite(dxe[:R]).all()
    err_da, err_dx = np.abs(_np(da[:R]).reshape(R, G, K) - da_ref).max(), np.abs(_np(dxe[:R]).reshape(R, G, D) - dxe_ref).max()
    print("packed aggregate bwd: da err %.2e (|ref| %.1f)  dxe err %.2e (|ref| %.1f)" % (err_da, big(da_ref), err_dx, big(dxe_ref)))
    assert err_da < 1e-3 * big(da_ref) and err_dx < 1e-4 * big(dxe_ref)


def test_packed_entries_refuse_bad_shapes():
    from efficientvideoclassification_youtube8m_amd import _lib, ops
    B, T, G, K, R = 2, 8, 2, 8, 6
    off = torch.tensor([0, 2, 6], dtype=torch.int32, device=DEV)
    for D, max_k in ((6, 4), (8, 9), (8, 2)):                        # D % 4 != 0; max_k > T; R > B * max_k
        a = torch.zeros((R, G * K), device=DEV); xe = torch.zeros((R, G * D), device=DEV); c2 = torch.zeros((K, D), device=DEV)
        V = torch.full((B, K, D), 3.0, device=DEV); asum = torch.full((B, K), 3.0, device=DEV)
        da = torch.full((R, G * K), 3.0, device=DEV); dxe = torch.full((R, G * D), 3.0, device=DEV)
        with pytest.raises(_lib.EvcError, match=r"evc_nextvlad_aggregate_packed_fwd failed \(-1\)"):
            ops.nextvlad_aggregate_packed_fwd(a, xe, off, B, T, G, K, D, R, max_k, c2, V, asum)
        with pytest.raises(_lib.EvcError, match=r"evc_nextvlad_aggregate_packed_bwd failed \(-1\)"):
            ops.nextvlad_aggregate_packed_bwd(a, xe, off, B, T, G, K, D, R, max_k, c2, V.clone(), da, dxe)
        torch.cuda.synchronize()
        for t in (V, asum, da, dxe):
            assert bool((t == 3.0).all())
    x = torch.zeros((B, T, 8), device=DEV); n = torch.tensor([2, 4], dtype=torch.int32, device=DEV)
    out = torch.full((64, 8), 3.0, device=DEV)
    for every_n, R_, Rp in ((0, 6, 32), (1, 17, 32), (1, 6, 64)):    # every_n < 1; R > B * ceil(T / every_n); Rp - R >= 32
        with pytest.raises(_lib.EvcError, match=r"evc_frames_gather_packed failed \(-1\)"):
            ops.frames_gather_packed(x, n, off, every_n, R_, Rp, out)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("normalize", [False, True])
def test_frames_gather_packed(u8, normalize):
    """evc_frames_gather_packed: the live rows against numpy float64 (1e-6 absolute: |v| <= 2 through two f32 roundings of the
    dequantisation, |v| <= 1 through a sum of squares, one rsqrt and one product after the normalisation) and BIT FOR BIT against
    evc_sample_frames_gather fed the draw that picks the same frames; f32 input without normalisation is the source frame's bits.
    Rows R .. Rp are exactly zero, the row after Rp keeps its NaN; the bf16 copy is the rounding of the f32 rows.  F / 4 = 68 > 64:
    lanes 0 - 3 take a second float4."""
    from efficientvideoclassification_youtube8m_amd import ops
    B, T, F, every_n = 6, 123, 272, 3
    n = np.array([0, 1, 46, 51, 97, 120], np.int32)
    plan = ops.GridPlan(n, every_n, T)
    assert list(plan.k) == [0, 1, 16, 17, 33, 40] and (plan.R, plan.Rp) == (107, 128)
    q, x, _, _ = mm.synthetic_batch(B, seed=2, max_frames=T, feature_size=F, vocab_size=4, dtype=np.float32)
    x[np.arange(T)[None, :] >= n[:, None]] = 0.0
    xin = torch.from_numpy(q if u8 else x).to(DEV)
    nd, off = torch.from_numpy(n).to(DEV), torch.from_numpy(plan.row_off).to(DEV)
    R, Rp = plan.R, plan.Rp
    out = torch.full((Rp + 1, F), float("nan"), device=DEV)
    out_bf = torch.full((Rp + 1, F), float("nan"), dtype=torch.bfloat16, device=DEV)
    _twice(lambda: ops.frames_gather_packed(xin, nd, off, every_n, R, Rp, out, out_bf, normalize=normalize), out[:Rp], out_bf[:Rp])
    assert torch.isnan(out[Rp]).all() and torch.isnan(out_bf[Rp]).all()
    assert not out[R:Rp].any() and not out_bf[R:Rp].any()
    assert torch.equal(out_bf[:Rp], out[:Rp].bfloat16())
    lists = px.grid_frames(n, every_n, T)
    xr = mm.dequantize(q.astype(np.float64)) if u8 else x.astype(np.float64)
    ref = np.concatenate([xr[b, lists[b]] for b in range(B)], 0)
    if normalize:
        ref = mm.l2_normalize(ref, 1)
    err = np.abs(_np(out[:R]) - ref).max()
    print("frames_gather_packed u8=%d normalize=%d: err %.2e" % (u8, normalize, err))
    assert err < 1e-6
    if not u8 and not normalize:
        assert np.array_equal(out[:R].cpu().numpy(), ref.astype(np.float32))
    # the existing gather on the same frames: S = max_k draws per video, u = (j * every_n + 0.5) / n_b for the k_b frames of the grid
    S = plan.max_k
    u = np.zeros((B, S), np.float32)
    for b in range(B):
        u[b, :plan.k[b]] = (np.arange(plan.k[b]) * every_n + 0.5) / max(int(n[b]), 1)
    samp = torch.empty((B * S, F), device=DEV); idx = torch.empty((B, S), dtype=torch.int32, device=DEV)
    ops.sample_frames_gather(xin, torch.from_numpy(u).to(DEV), nd, samp, idx, normalize=normalize)
    idx, samp = idx.cpu().numpy(), samp.view(B, S, F)
    for b in range(B):
        assert np.array_equal(idx[b, :plan.k[b]], lists[b])
        assert torch.equal(out[plan.row_off[b]:plan.row_off[b + 1]], samp[b, :plan.k[b]])


@pytest.mark.parametrize("S,every_n,u8", [(10, 3, True), (64, 1, False)])
def test_grid_tower_is_the_sampled_tower_bit_for_bit_on_equal_lengths(S, every_n, u8):
    """tests/_nextvlad_grid_equiv.py in a fresh process under EVC_DETERMINISTIC=1: every video has n_b = S * every_n frames and the
    sampled tower is fed the draw that picks j * every_n.  r, xe, a, V, asum, Y_bf, the predictions, dxe / da of the aggregation
    backward, the gradient store and the master weights after one SingleTowerGraph.step are equal, no tolerance: the packed kernels
    keep every element's summation order."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "_nextvlad_grid_equiv.py"), str(S), str(every_n), "1" if u8 else "0"],
                       env=dict(os.environ, EVC_DETERMINISTIC="1"), capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "step: master weights" in r.stdout and "DIFFERS" not in r.stdout and "deterministic 1" in r.stdout


def _params(tw):
    pre = tw.scope + "/"
    return {k[len(pre):]: _np(v) for k, v in tw.state_dict().items()}


@pytest.mark.parametrize("every_n,T", [(10, 300), (1, 40)])
def test_grid_tower_forward_backward_against_reference(every_n, T):
    """The ragged tower against tests/_nextvlad_packed_ref.py at B = 32, F = 192, lambda = 2, G = 8, K = 24, H = 128, rho = 2, V = 33 on the
    synthetic batch's own lengths (every_n = 10: k_b = 12 .. 30; every_n = 1 with the frames cut to T = 40: k_b = 40).  Bounds of
    test_nextvlad_forward_backward_against_reference - the arithmetic in front of each quantity is the same: a 2e-2, Y (the bf16
    operand Y_bf) 2e-2, predictions 5e-3, every gradient tensor relative L2 0.12 or max abs 1e-3.

    Measured on an MI355X (every_n = 10, R = 665 / every_n = 1 with T = 40, R = 1280): r 2.9e-8 / 3.2e-8, a 1.44e-3 / 1.59e-3, Y (Y_bf)
    1.17e-2 / 8.0e-3 (9.9e-3 / 7.2e-3 before the rounding to bf16; |Y| up to 2.85 / 2.14), predictions 2.7e-3 / 2.3e-3, largest
    relative L2 of a gradient 0.060 (gating_bn/beta) / 0.009 (expansion_biases), except vlad_bn/beta, whose true gradient is zero up
    to rounding and which is within 6.9e-5 / 8.0e-5 absolute.  Y is the tight one, as on the sampled tower (1.07e-2 at this B,
    DESIGN.md 7.12): vlad_bn over 32 videos whose descriptors differ little."""
    from efficientvideoclassification_youtube8m_amd import ops
    from efficientvideoclassification_youtube8m_amd.towers import NeXtVladTower
    B, F, lam, G, K, H, rho, V = 32, 192, 2, 8, 24, 128, 2, 33
    rng = np.random.default_rng(B + K)
    q, x, n, labels = mm.synthetic_batch(B, seed=B, feature_size=F, vocab_size=V, dtype=np.float32)
    q, x = np.ascontiguousarray(q[:, :T]), np.ascontiguousarray(x[:, :T])
    tw = NeXtVladTower(B, T, F, V, cluster_size=K, hidden_size=H, groups=G, expansion=lam, gating_reduction=rho, device=DEV, seed=3,
                       frames="grid", every_n=every_n)
    E, D = lam * F, lam * F // G
    for k in tw.names:                                   # non-trivial batch-norm scale / offset and biases
        if k.endswith("/gamma") or k.endswith("/beta") or k in (tw.EB, tw.AB):
            tw.store.p(k).add_(torch.from_numpy(rng.standard_normal(tw.store.p(k).shape).astype(np.float32) * 0.2).to(DEV))
    tw.refresh_shadows()
    P = _params(tw)
    pred = tw.forward(torch.from_numpy(q).to(DEV), torch.from_numpy(n).to(DEV), num_frames_host=n)
    xn = mm.l2_normalize(x.astype(np.float64), 2)
    ref_pred, cache = px.nextvlad_packed_fwd(xn, n, every_n, P)
    R = cache["r"].shape[0]
    assert (tw.R, tw.Rp) == (R, ops.round_up(R, 32)) and np.array_equal(tw.plan.k, cache["k"])
    assert np.array_equal(tw.row_off.cpu().numpy(), cache["row_off"])
    for name in ("r_bf", "xe_bf"):                       # the padding rows of the forward TN operands
        assert not getattr(tw, name)[R:tw.Rp].any()
    err_r = np.abs(_np(tw.r[:R]) - cache["r"]).max()
    err_a = np.abs(_np(tw.a[:R]).reshape(R, G, K) - cache["a"]).max()
    Yk = cache["Y"].reshape(B, D, K).transpose(0, 2, 1).reshape(B, K * D)          # reference order d*K+k -> cluster-major
    bv = tw.bn_v
    Yf = torch.empty((B, K * D), device=DEV)
    ops.bn_apply(tw.U, B, K * D, bv.mean, bv.var, bv.gamma(), bv.beta(), False, y_f32=Yf)
    assert torch.equal(tw.Y_bf[:B], Yf.bfloat16()) and not tw.Y_bf[B:].any()
    err_y_f32 = np.abs(_np(Yf) - Yk).max()
    err_y = np.abs(tw.Y_bf[:B].float().cpu().numpy() - Yk).max()
    err = np.abs(_np(pred) - ref_pred).max()
    print("grid every_n=%d T=%d R=%d: r err %.2e  a err %.2e  Y err %.2e (before the rounding to bf16 %.2e, |Y|max %.2f)  pred err %.2e"
          % (every_n, T, R, err_r, err_a, err_y, err_y_f32, np.abs(Yk).max(), err))
    # every bound is evaluated (and every figure printed) before the first one fails the test
    missed = [(w, e, b) for w, e, b in (("r", err_r, 1e-6), ("a", err_a, 2e-2), ("Y", err_y, 2e-2), ("pred", err, 5e-3)) if not e < b]
    dp = mm.cross_entropy_grad(ref_pred, labels)
    tw.backward(torch.from_numpy(dp.astype(np.float32)).to(DEV))
    for name in ("dact_bf", "datt_bf", "dxe_bf"):        # the padding rows of the backward TN operands
        assert not getattr(tw, name)[R:tw.Rp].any()
    gref = px.nextvlad_packed_bwd(dp, cache)
    assert set(gref) == set(tw.names)
    for k, g in gref.items():
        got = tw.store.g(k)
        got = _np(got.t() if got.dim() == 2 else got)
        if k == tw.HW:
            got = got.reshape(K, D, H).transpose(1, 0, 2).reshape(D * K, H)
        elif k.startswith("vlad_bn/"):
            got = got.reshape(K, D).T.reshape(-1)
        l2 = float(np.linalg.norm(got - g) / (np.linalg.norm(g) + 1e-30))
        mx = float(np.abs(got - g).max())
        print("  grad %-28s rel l2 %.3e  max abs %.3e" % (k, l2, mx))
        if not (l2 < 0.12 or mx < 1e-3):
            missed.append(("grad " + k, (l2, mx), (0.12, 1e-3)))
    assert not missed, missed


def test_grid_through_train_main(tmp_path):
    """train.main on synthetic data with --nextvlad_frames grid --every_n 10 at the sizes of
    test_nextvlad_through_create_model_and_train_main: finite, falling loss; the checkpoint records the mode; a fresh grid tower
    restored from it reproduces the last predictions bit for bit, a sampled tower loads the same file; a batch with another R runs
    in the same buffers."""
    from efficientvideoclassification_youtube8m_amd import train
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    from efficientvideoclassification_youtube8m_amd.towers import NeXtVladTower
    FLAGS.reset()
    common = ["--train_data_pattern", "synthetic", "--frame_features", "True", "--feature_names", "rgb, audio", "--model", "NeXtVLADModel",
              "--batch_size", "16", "--nextvlad_frames", "grid", "--every_n", "10", "--nextvlad_cluster_size", "16", "--nextvlad_groups", "4",
              "--nextvlad_hidden_size", "128", "--nextvlad_gating_reduction", "2", "--feature_sizes", "64, 64", "--synthetic_videos", "64",
              "--num_epochs", "1", "--start_new_model", "True", "--base_learning_rate", "0.01"]
    res = train.main(common + ["--train_dir", str(tmp_path) + "/"])
    FLAGS.reset()
    g = res["graph"]
    tw = g.tower
    assert res["iterations"] == 4 and g.global_step == 4 and tw.frames == "grid" and tw.every_n == 10
    losses = [h[1]["loss"] for h in res["history"]]
    print("nextvlad grid train losses", losses, "rows of the last batch", tw.R)
    assert all(np.isfinite(l) for l in losses) and losses[-1] < losses[0]            # it trains
    sd = torch.load(train.latest_checkpoint(str(tmp_path) + "/"))
    assert sd["nextvlad_frames"] == "grid" and sd["every_n"] == 10
    assert sd["model/hidden1_weights"].shape == (64 * 16, 128) and sd["model/cluster_weights2"].shape == (64, 16)     # same names and shapes
    # a fresh grid tower from the checkpoint against the trained one, in evaluation mode on one batch
    q, x, n, labels = mm.synthetic_batch(16, seed=4, feature_size=128, vocab_size=train.NUM_CLASSES, dtype=np.float32)
    qd, nd = torch.from_numpy(q).to(DEV), torch.from_numpy(n).to(DEV)
    kw = dict(max_frames=300, feature_size=128, vocab_size=train.NUM_CLASSES, cluster_size=16, hidden_size=128, groups=4, expansion=2,
              gating_reduction=2, device=DEV)
    last = tw.forward(qd, nd, num_frames_host=n, is_training=False).clone()
    ptrs = {name: getattr(tw, name).data_ptr() for name in ("r", "r_bf", "xe", "xe_bf", "attl", "act", "a", "da", "dz", "dact_bf", "datt",
                                                            "datt_bf", "dxe", "dxe_bf")}
    R1 = tw.R
    fresh = NeXtVladTower(16, frames="grid", every_n=10, seed=9, **kw)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.forward(qd, nd, num_frames_host=n, is_training=False), last)
    sampled = NeXtVladTower(16, iterations=10, seed=9, **kw)
    sampled.load_state_dict(sd)
    assert torch.equal(sampled.store.master, fresh.store.master)
    # a second batch with a different R: a whole step in the same buffers
    n2 = np.maximum(n // 2, 1).astype(np.int32)
    out = g.step(qd, torch.from_numpy(labels.astype(np.uint8)).to(DEV), torch.from_numpy(n2).to(DEV), num_frames_host=n2)
    torch.cuda.synchronize()
    assert tw.R != R1 and tw.R == int(np.ceil(n2 / 10).sum()) and np.isfinite(float(out["loss"]))
    assert ptrs == {name: getattr(tw, name).data_ptr() for name in ptrs}
    with pytest.raises(ValueError, match="--nextvlad_frames grid.*--precision high"):
        train.main(common + ["--train_dir", str(tmp_path) + "/p/", "--precision", "high"])
    FLAGS.reset()
