"""NeXtVLAD dropout before the hidden layer on the device: the two entries evc_nextvlad_dropout_fwd / _bwd against
the numpy Philox mask of tests/_nextvlad_dropout_ref.py at EVERY element, the values they write, their refusals, the tower's forward
and gradients against the float64 restatement under the reference mask, and the graphs / train.main / validate around it.
Figures measured on an MI355X: profiles/nextvlad_dropout_parity.txt (written by the tower test when EVC_NEXTVLAD_DROPOUT_PARITY names a
file).  pytest -m gpu."""
import functools
import os

import numpy as np
import pytest
import torch

import _nextvlad_dropout_ref as dr
from oracle import model_math as mm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, K, D).  63 quads (less than one workgroup), 600 (a ragged last workgroup), 4 752 (several workgroups, an odd row count), and the
# grid-cap shape: both launches cap their grid at 2048 workgroups of 256 threads (nx_drop_grid), 524 288 quads per sweep, so the
# grid-stride loop iterates a second time only beyond that.  At K*D = 128 * 256 a row holds 8192 quads: 64 rows fill the sweep
# exactly, and B = 65 is the smallest row count at that width whose quad count (532 480) exceeds it - the last 8192 quads are the
# second iteration of the first 32 workgroups.
SMALL_SHAPES = [(3, 7, 12), (5, 24, 20), (33, 16, 36)]
GRID_CAP_SHAPE = (65, 128, 256)
KEEPS = (0.5, 0.8, 1.0 - 2.0 ** -20)
# (seed, rank, step): two steps, two seeds, rank 1, and a step above 2^32 (the high counter word)
KEYS = [(0, 0, 0), (0, 0, 5), (9, 0, 0), (0, 1, 0), (0, 0, (1 << 32) + 5)]


def _np(t):
    return t.detach().cpu().double().numpy()


@functools.lru_cache(maxsize=None)
def _words(B, C, seed, rank, step):
    return dr.dropout_words(B, C, seed, rank, step)


@functools.lru_cache(maxsize=None)
def _bn_case(B, K, D):
    """U and the four per-column vectors (f32, on the device) with every batch-norm output in [1, 2] - no kept value is zero - and the
    float64 value of that output from the f32 inputs.  Made once per shape and left unchanged."""
    rng = np.random.default_rng(B * 1000 + K * D)
    C = K * D
    mean, var = rng.uniform(-1, 1, C), rng.uniform(0.5, 2.0, C)
    gamma, beta = rng.uniform(0.5, 1.5, C), rng.uniform(-0.5, 0.5, C)
    Y = rng.uniform(1.05, 1.95, (B, C))
    U = mean + (Y - beta) * np.sqrt(var + 1e-3) / gamma
    f32 = [np.ascontiguousarray(a, np.float32) for a in (U, mean, var, gamma, beta)]
    U6, m6, v6, g6, b6 = (a.astype(np.float64) for a in f32)
    Yref = (U6 - m6) / np.sqrt(v6 + 1e-3) * g6 + b6
    assert Yref.min() > 1.0 and Yref.max() < 2.0
    return tuple(torch.from_numpy(a).to(DEV) for a in f32), Yref


def _fwd(B, K, D, keep, seed, rank, step):
    from efficientvideoclassification_youtube8m_amd import ops
    (U, mean, var, gamma, beta), Yref = _bn_case(B, K, D)
    T, scale = ops.dropout_threshold(keep)
    Y = torch.full((B, K * D), 7.0, dtype=torch.bfloat16, device=DEV)
    ops.nextvlad_dropout_fwd(U, B, K * D, mean, var, gamma, beta, T, scale, seed, rank, step, Y)
    return Y, Yref, T, scale


def _check_fwd(B, K, D, keep, seed, rank, step):
    Y, Yref, T, _ = _fwd(B, K, D, keep, seed, rank, step)
    mask = _words(B, K * D, seed, rank, step) < np.uint64(T)
    assert T == dr.threshold(keep)
    bits = Y.view(torch.int16).cpu().numpy().view(np.uint16)
    got = Y.float().cpu().numpy().astype(np.float64)
    assert np.array_equal(bits != 0, mask), ("mask", (B, K, D), keep, seed, rank, step, int(((bits != 0) != mask).sum()))
    assert not bits[~mask].any()                                          # dropped: exactly +0
    ref = Yref / keep
    err = np.abs(got - ref)[mask] / np.abs(ref)[mask]
    worst = float(err.max()) if err.size else 0.0
    assert worst <= 2.0 ** -8, ("value", (B, K, D), keep, worst)
    return mask, worst


@pytest.mark.parametrize("B,K,D", SMALL_SHAPES)
def test_forward_mask_and_values_at_every_element(B, K, D):
    """(Y_bf != 0) is the reference mask at every element, for keep in {0.5, 0.8, 1 - 2^-20} x two steps, two seeds, rank 1 and a step
    above 2^32; kept elements within 2^-8 relative of the float64 bn(U) / keep, dropped elements exactly +0.  The bound is the issue's;
    what it leaves: bf16 keeps 8 significant bits, so its round-to-nearest is off by at most 2^-8 / (1 + 2^-8) = 3.891e-3 relative (a
    value just below the first midpoint of a binade), 1.5e-5 below 2^-8 = 3.906e-3 - room for the f32 batch-norm expression and the
    scale in front of the rounding, five operations of 2^-24 each (3e-7).  Measured on an MI355X: 3.59e-3, 3.89e-3, 3.88e-3."""
    worst, masks = 0.0, {}
    for keep in KEEPS:
        for key in KEYS:
            m, w = _check_fwd(B, K, D, keep, *key)
            worst = max(worst, w)
            masks[(keep,) + key] = m
    print("dropout fwd (%d, %d, %d): worst relative error of a kept element %.3e (bound %.3e)" % (B, K, D, worst, 2.0 ** -8))
    ref = masks[(0.5, 0, 0, 0)]
    assert 0 < ref.sum() < ref.size
    for key in KEYS[1:]:                                                  # another step / seed / rank / high step word: another mask
        assert not np.array_equal(ref, masks[(0.5,) + key]), key


def test_forward_and_backward_at_the_grid_cap_shape():
    """GRID_CAP_SHAPE: the grid-stride loop of both launches runs a second iteration.  Mask at every element (keep 0.5 and 1 - 2^-20,
    which drops a handful of the 2.1 M elements), values, and the backward on the same key."""
    from efficientvideoclassification_youtube8m_amd import ops
    B, K, D = GRID_CAP_SHAPE
    assert B * K * D // 4 > 2048 * 256 >= (B - 1) * K * D // 4
    m, w = _check_fwd(B, K, D, 0.5, 3, 0, 11)
    m2, w2 = _check_fwd(B, K, D, 1.0 - 2.0 ** -20, 3, 0, 11)
    print("dropout fwd grid-cap: worst relative error %.3e / %.3e, dropped at keep 1 - 2^-20: %d" % (w, w2, int((~m2).sum())))
    assert (~m2).sum() > 0 and not (m & ~m2).any()                        # (what keep 0.5 keeps, a larger keep keeps)
    assert abs(m.mean() - 0.5) <= 3.0 * np.sqrt(0.25 / m.size)
    rng = np.random.default_rng(1)
    dY = rng.standard_normal((B, K * D)).astype(np.float32)
    T, scale = ops.dropout_threshold(0.5)
    d = torch.from_numpy(dY).to(DEV)
    ops.nextvlad_dropout_bwd(d, B, K * D, T, scale, 3, 0, 11)
    got = d.cpu().numpy()
    want = np.where(m, dY * np.float32(scale), np.float32(0.0)).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("B,K,D", SMALL_SHAPES)
def test_backward_scales_in_place_under_the_forward_mask(B, K, D):
    """For random f32 dY the in-place result is float32(dY * scale) bit for bit where m = 1 (one f32 multiply has one correctly rounded
    answer) and 0 where m = 0; with the forward's (seed, rank, step) it masks exactly the elements the forward dropped."""
    from efficientvideoclassification_youtube8m_amd import ops
    rng = np.random.default_rng(B + K + D)
    dY = rng.standard_normal((B, K * D)).astype(np.float32)
    for keep in KEEPS:
        for seed, rank, step in KEYS:
            T, scale = ops.dropout_threshold(keep)
            mask = _words(B, K * D, seed, rank, step) < np.uint64(T)
            d = torch.from_numpy(dY).to(DEV)
            ops.nextvlad_dropout_bwd(d, B, K * D, T, scale, seed, rank, step)
            got = d.cpu().numpy()
            want = (dY * np.float32(scale)).astype(np.float32)
            assert np.array_equal(got.view(np.uint32)[mask], want.view(np.uint32)[mask]), (keep, seed, rank, step)
            assert not got.view(np.uint32)[~mask].any()
            Y, _, _, _ = _fwd(B, K, D, keep, seed, rank, step)
            fwd_dropped = (Y.view(torch.int16) == 0).cpu().numpy()
            assert np.array_equal(fwd_dropped, ~mask)


def test_two_calls_give_the_same_bits():
    from efficientvideoclassification_youtube8m_amd import ops
    B, K, D = SMALL_SHAPES[2]
    y1, _, T, scale = _fwd(B, K, D, 0.5, 4, 0, 9)
    y2, _, _, _ = _fwd(B, K, D, 0.5, 4, 0, 9)
    assert torch.equal(y1.view(torch.int16), y2.view(torch.int16))
    dY = torch.randn((B, K * D), device=DEV)
    a, b = dY.clone(), dY.clone()
    ops.nextvlad_dropout_bwd(a, B, K * D, T, scale, 4, 0, 9)
    ops.nextvlad_dropout_bwd(b, B, K * D, T, scale, 4, 0, 9)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_entries_refuse_bad_shapes_and_a_zero_threshold_without_a_launch():
    """C % 4 != 0 and B <= 0 are EVC_ERR_BAD_SHAPE (-1), T == 0 EVC_ERR_BAD_ARG (-5); the outputs keep their fill."""
    from efficientvideoclassification_youtube8m_amd import _lib, ops
    B, C = 3, 24
    U = torch.zeros((B, C), device=DEV)
    v = torch.ones(C, device=DEV)
    Y = torch.full((B, C), 3.0, dtype=torch.bfloat16, device=DEV)
    dY = torch.full((B, C), 3.0, device=DEV)
    T, scale = ops.dropout_threshold(0.5)
    for b, c, t, code in ((B, 22, T, -1), (0, C, T, -1), (B, C, 0, -5)):
        with pytest.raises(_lib.EvcError, match=r"evc_nextvlad_dropout_fwd failed \(%d\)" % code):
            ops.nextvlad_dropout_fwd(U, b, c, v, v, v, v, t, scale, 0, 0, 0, Y)
        with pytest.raises(_lib.EvcError, match=r"evc_nextvlad_dropout_bwd failed \(%d\)" % code):
            ops.nextvlad_dropout_bwd(dY, b, c, t, scale, 0, 0, 0)
    torch.cuda.synchronize()
    assert bool((Y == 3.0).all()) and bool((dY == 3.0).all())


# ---- the tower ----------------------------------------------------------------------------------------------------------------------
def _params(tw):
    pre = tw.scope + "/"
    return {k[len(pre):]: _np(v) for k, v in tw.state_dict().items()}


def _tf_grad(tw, k):
    got = tw.store.g(k)
    got = _np(got.t() if got.dim() == 2 else got)
    K, D, H = tw.Kc, tw.D, tw.Hd
    if k == tw.HW:
        got = got.reshape(K, D, H).transpose(1, 0, 2).reshape(D * K, H)
    elif k.startswith("vlad_bn/"):
        got = got.reshape(K, D).T.reshape(-1)
    return got


def _distances(tw, pred, ref_pred, cache, gref, B, S, G, K):
    """{tensor: distance} of a tower from its float64 restatement: max abs for a and the predictions, (relative L2, max abs) per gradient."""
    out = {"a": float(np.abs(_np(tw.a).reshape(B * S, G, K) - cache["a"]).max()), "pred": float(np.abs(_np(pred) - ref_pred).max())}
    for k, g in gref.items():
        got = _tf_grad(tw, k)
        out["grad " + k] = (float(np.linalg.norm(got - g) / (np.linalg.norm(g) + 1e-30)), float(np.abs(got - g).max()))
    return out


_PARITY = {}


def _write_parity():
    path = os.environ.get("EVC_NEXTVLAD_DROPOUT_PARITY")
    if not path:
        return
    with open(path, "w") as f:
        f.write("NeXtVLAD tower at dropout 0.5 (seed 3, step 5) and the same tower at rate 0, each against its float64 restatement\n"
                "(tests/_nextvlad_dropout_ref.py under the reference mask).  a / pred: max abs; gradients: relative L2, max abs.\n"
                "bound = the bound of test_nextvlad_forward_backward_against_reference, widened to twice the rate-0 distance where that is larger.\n"
                "(vlad_bn/beta at rate 0: the true gradient is exactly zero - the column sums of a training-mode batch-norm's input gradient\n"
                "vanish - so its relative L2 is a ratio to a float64 residue; the max abs column is the one that says something there.)\n")
        for shape, rows in _PARITY.items():
            f.write("\nshape (B, F, lambda, G, K, H, rho, V, S) = %s\n" % (shape,))
            for r in rows:
                f.write(r + "\n")


@pytest.mark.parametrize("B,F,lam,G,K,H,rho,V,S,u8", [(16, 64, 2, 4, 16, 128, 2, 40, 10, False), (32, 192, 2, 8, 24, 128, 2, 33, 30, True)])
def test_tower_forward_backward_against_reference_under_the_mask(B, F, lam, G, K, H, rho, V, S, u8):
    """NeXtVladTower(dropout=0.5) at the two shapes of test_nextvlad_forward_backward_against_reference, against the float64 helper
    under the reference mask of (seed 3, rank 0, step 5).  Bounds: that test's (a 2e-2, predictions 5e-3, every gradient relative L2
    0.12 or max abs 1e-3), each widened to twice the distance the RATE-0 tower - the unchanged path, same shape and weights - shows
    from its own float64 restatement in this run, where that is larger: at keep 0.5 the hidden product's bf16 operand has twice the
    magnitude and half as many terms average its rounding.  tower.Y_bf != 0 is the reference mask.  Every figure is printed (and
    written to the parity file) before the first assertion."""
    from efficientvideoclassification_youtube8m_amd.towers import NeXtVladTower
    q, x, n, labels = mm.synthetic_batch(B, seed=B, feature_size=F, vocab_size=V, dtype=np.float32)
    D = lam * F // G
    seed, step, keep = 3, 5, 0.5

    def mk(rate):
        tw = NeXtVladTower(B, 300, F, V, iterations=S, cluster_size=K, hidden_size=H, groups=G, expansion=lam, gating_reduction=rho,
                           device=DEV, seed=3, dropout=rate, dropout_seed=seed)
        rng = np.random.default_rng(B + K)               # the same perturbation in both towers
        for k in tw.names:
            if k.endswith("/gamma") or k.endswith("/beta") or k in (tw.EB, tw.AB):
                tw.store.p(k).add_(torch.from_numpy(rng.standard_normal(tw.store.p(k).shape).astype(np.float32) * 0.2).to(DEV))
        tw.refresh_shadows()
        return tw, rng

    tw0, _ = mk(0.0)
    tw, rng = mk(0.5)
    assert torch.equal(tw0.store.master, tw.store.master)
    P = _params(tw)
    u = rng.random((B, S)).astype(np.float32)
    xin = torch.from_numpy(q).to(DEV) if u8 else torch.from_numpy(x).to(DEV)
    nd, ud = torch.from_numpy(n).to(DEV), torch.from_numpy(u).to(DEV)
    xn = mm.l2_normalize(x.astype(np.float64), 2)
    mask = dr.dropout_mask(B, K, D, keep, seed, 0, step)
    dist = {}
    for name, t, m in (("rate 0", tw0, None), ("rate 0.5", tw, mask)):
        pred = t.forward(xin, nd, ud, dropout_step=step)
        ref_pred, cache = dr.nextvlad_fwd(xn, n, u, P, m, keep)
        dp = mm.cross_entropy_grad(ref_pred, labels)
        t.backward(torch.from_numpy(dp.astype(np.float32)).to(DEV))
        gref = dr.nextvlad_bwd(dp, cache)
        assert set(gref) == set(t.names)
        dist[name] = _distances(t, pred, ref_pred, cache, gref, B, S, G, K)
    got_mask = (tw.Y_bf[:B].view(torch.int16) != 0).cpu().numpy()
    base = {"a": 2e-2, "pred": 5e-3}
    rows, missed = [], []
    for k, d1 in dist["rate 0.5"].items():
        d0 = dist["rate 0"][k]
        if k.startswith("grad "):
            bound = (max(0.12, 2 * d0[0]), max(1e-3, 2 * d0[1]))
            ok = d1[0] < bound[0] or d1[1] < bound[1]
            rows.append("  %-34s rate 0: %.3e %.3e   rate 0.5: %.3e %.3e   bound: %.3e or %.3e" % (k, d0[0], d0[1], d1[0], d1[1], bound[0], bound[1]))
        else:
            bound = max(base[k], 2 * d0)
            ok = d1 < bound
            rows.append("  %-34s rate 0: %.3e             rate 0.5: %.3e             bound: %.3e" % (k, d0, d1, bound))
        if not ok:
            missed.append((k, d1, bound))
    rows.append("  mask: tower.Y_bf != 0 differs from the reference mask at %d of %d elements" % (int((got_mask != mask).sum()), mask.size))
    print("\n".join(rows))
    _PARITY[(B, F, lam, G, K, H, rho, V, S)] = rows
    _write_parity()
    assert np.array_equal(got_mask, mask) and not tw.Y_bf[B:].any()
    assert tw0.Y_bf[:B].view(torch.int16).ne(0).all()                    # (the rate-0 tower drops nothing)
    assert not missed, missed


SMALL = dict(max_frames=300, feature_size=128, vocab_size=40, cluster_size=16, hidden_size=128, groups=4, expansion=2, gating_reduction=2,
             device=DEV)
SK, SD = 16, 64                                                          # clusters, group width (2 * 128 / 4) of SMALL


def _raise(*a, **k):
    raise AssertionError("a dropout entry was called")


def test_eval_forward_is_the_rate_0_tower_and_rate_0_never_calls_the_entries(monkeypatch):
    """is_training=False on a dropout tower: Y_bf (and the predictions) bit-identical to a rate-0 tower with the same weights.  A tower
    built with dropout=0.0 never calls the new entries, forward or backward (both wrappers patched to raise); nor does the evaluation
    forward of the dropout tower."""
    from efficientvideoclassification_youtube8m_amd import ops
    from efficientvideoclassification_youtube8m_amd.towers import NeXtVladTower
    B, S = 8, 8
    q, x, n, labels = mm.synthetic_batch(B, seed=5, feature_size=128, vocab_size=40, dtype=np.float32)
    qd, nd = torch.from_numpy(q).to(DEV), torch.from_numpy(n).to(DEV)
    u = torch.rand((B, S), device=DEV)
    tw0 = NeXtVladTower(B, iterations=S, seed=3, **SMALL)
    twd = NeXtVladTower(B, iterations=S, seed=3, dropout=0.5, dropout_seed=2, **SMALL)
    assert tw0.dropout == 0.0 and twd.dropout == 0.5 and torch.equal(tw0.store.master, twd.store.master)
    monkeypatch.setattr(ops, "nextvlad_dropout_fwd", _raise)
    monkeypatch.setattr(ops, "nextvlad_dropout_bwd", _raise)
    p0 = tw0.forward(qd, nd, u, is_training=False).clone()
    pd = twd.forward(qd, nd, u, is_training=False, dropout_step=1)
    assert torch.equal(tw0.Y_bf.view(torch.int16), twd.Y_bf.view(torch.int16)) and torch.equal(p0, pd)
    p0 = tw0.forward(qd, nd, u, dropout_step=4)                          # training mode at rate 0: forward and backward
    tw0.backward(torch.randn_like(p0) * 1e-3)
    torch.cuda.synchronize()
    assert tw0.Y_bf[:B].view(torch.int16).ne(0).all()
    with pytest.raises(AssertionError, match="a dropout entry was called"):
        twd.forward(qd, nd, u, dropout_step=1)                           # (the patch is live: the dropout tower does call it)


def _perturbed(tw, seed):
    rng = np.random.default_rng(seed)
    for k in tw.names:
        if k.endswith("/beta"):                                          # (no batch-norm output is exactly zero)
            tw.store.p(k).add_(torch.from_numpy(rng.standard_normal(tw.store.p(k).shape).astype(np.float32) * 0.2).to(DEV))


def test_single_tower_graph_steps_through_the_masks_and_reproduces_them():
    """SingleTowerGraph at rate 0.5: the two steps carry the masks of global_step 0 and 1 (two different masks), and a second graph
    from the same seed and weights reproduces the first graph's Y_bf bits at each step."""
    from efficientvideoclassification_youtube8m_amd.distill import SingleTowerGraph
    from efficientvideoclassification_youtube8m_amd.towers import NeXtVladTower
    B, S, seed = 8, 8, 6
    q, x, n, labels = mm.synthetic_batch(B, seed=7, feature_size=128, vocab_size=40, dtype=np.float32)
    qd, yd, nd = torch.from_numpy(q).to(DEV), torch.from_numpy(labels.astype(np.uint8)).to(DEV), torch.from_numpy(n).to(DEV)
    us = [torch.rand((B, S), device=DEV) for _ in range(2)]
    runs = []
    for _ in range(2):
        tw = NeXtVladTower(B, iterations=S, seed=3, dropout=0.5, dropout_seed=seed, **SMALL)
        _perturbed(tw, 1)
        g = SingleTowerGraph(tw, base_learning_rate=0.01)
        ys = []
        for s in range(2):
            assert g.global_step == s
            g.step(qd, yd, nd, uniform=us[s])
            ys.append(tw.Y_bf[:B].view(torch.int16).clone())
        runs.append(ys)
    masks = [dr.dropout_mask(B, SK, SD, 0.5, seed, 0, s) for s in range(2)]
    assert not np.array_equal(masks[0], masks[1])
    for s in range(2):
        assert np.array_equal((runs[0][s] != 0).cpu().numpy(), masks[s]), s
        assert torch.equal(runs[0][s], runs[1][s]), s


def test_rank_of_the_default_group_reaches_the_key(monkeypatch):
    """train.main under a launcher initialises the DEFAULT group and builds the tower with process_group=None (the step's reductions
    fall back to the default group).  A tower built that way on rank 1 - torch.distributed patched around the constructor alone, so
    that no collective runs - carries rank 1 in its key: its Y_bf is dropout_mask(..., rank=1, ...), not rank 0's."""
    from efficientvideoclassification_youtube8m_amd.towers import NeXtVladTower
    B, S, seed, step = 8, 8, 6, 3
    with monkeypatch.context() as m:
        m.setattr(torch.distributed, "is_initialized", lambda: True)
        m.setattr(torch.distributed, "get_rank", lambda group=None: 1)
        tw = NeXtVladTower(B, iterations=S, seed=3, dropout=0.5, dropout_seed=seed, process_group=None, **SMALL)
    assert not torch.distributed.is_initialized() and tw.rank == 1 and tw.pg is None
    assert NeXtVladTower(B, iterations=S, seed=3, dropout=0.5, dropout_seed=seed, **SMALL).rank == 0     # no group: rank 0
    _perturbed(tw, 1)
    q, x, n, labels = mm.synthetic_batch(B, seed=7, feature_size=128, vocab_size=40, dtype=np.float32)
    tw.forward(torch.from_numpy(q).to(DEV), torch.from_numpy(n).to(DEV), torch.rand((B, S), device=DEV), dropout_step=step)
    got = (tw.Y_bf[:B].view(torch.int16) != 0).cpu().numpy()
    assert np.array_equal(got, dr.dropout_mask(B, SK, SD, 0.5, seed, 1, step))
    assert not np.array_equal(got, dr.dropout_mask(B, SK, SD, 0.5, seed, 0, step))


def test_train_main_two_ranks_drop_different_elements(tmp_path):
    """train.main with two ranks (sharing the GPU over gloo, EVC_TRAIN_SHARED_GPU=1, as tests/test_gpu_dp.py runs it), sampled mode,
    --nextvlad_dropout 0.5, one step: the tower each rank built carries its own rank in the key, and the mask of its forward at
    global_step 0 is dropout_mask(..., rank=r, step=0) - the ranks of a data-parallel run drop different elements."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT="29641", EVC_TRAIN_SHARED_GPU="1",
               PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    B, seed = 8, 21
    args = ["--train_data_pattern", "synthetic", "--train_dir", str(tmp_path) + "/", "--frame_features", "True", "--feature_names", "rgb, audio",
            "--feature_sizes", "64, 64", "--model", "NeXtVLADModel", "--batch_size", str(B), "--iterations", "8", "--nextvlad_cluster_size", "16",
            "--nextvlad_groups", "4", "--nextvlad_hidden_size", "128", "--nextvlad_gating_reduction", "2", "--num_epochs", "1",
            "--synthetic_videos", "32", "--start_new_model", "True", "--max_steps", "1", "--nextvlad_dropout", "0.5",
            "--nextvlad_dropout_seed", str(seed)]
    child = os.path.join(root, "tests", "_nextvlad_dropout_rank_child.py")
    outs = [str(tmp_path / ("rank%d.npz" % r)) for r in range(2)]
    procs = [subprocess.Popen([sys.executable, child, outs[r]] + args, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, cwd=root) for r in range(2)]
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for pp in procs:
                pp.kill()
            raise
        logs.append(o.decode()[-3000:])
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    masks = []
    for r in range(2):
        d = np.load(outs[r])
        assert int(d["rank"]) == r and int(d["seed"]) == seed and int(d["global_step"]) == 1 and (int(d["K"]), int(d["D"])) == (SK, SD)
        assert d["mask"].shape == (B, SK * SD)                           # (--batch_size is per rank)
        assert np.array_equal(d["mask"], dr.dropout_mask(B, SK, SD, 0.5, seed, r, 0)), r
        masks.append(d["mask"])
    assert not np.array_equal(masks[0], masks[1])


def test_distill_graph_drops_in_the_student_only():
    """NeXtVladDistillGraph(dropout=0.5): the student's Y_bf carries the mask of the step; the frozen teacher's Y_bf is the one of the
    rate-0 graph bit for bit (no zeros beyond those of its rate-0 run), and model/* stays bit-identical over the step (7.14)."""
    from efficientvideoclassification_youtube8m_amd.distill import NeXtVladDistillGraph
    B, seed = 8, 4
    q, x, n, labels = mm.synthetic_batch(B, seed=11, feature_size=128, vocab_size=40, dtype=np.float32)
    qd, yd, nd = torch.from_numpy(q).to(DEV), torch.from_numpy(labels.astype(np.uint8)).to(DEV), torch.from_numpy(n).to(DEV)
    kw = dict(every_n=10, teacher_every_n=1, feature_size=128, vocab_size=40, max_frames=300, cluster_size=16, hidden_size=128, groups=4,
              expansion=2, gating_reduction=2, device=DEV, seed=3)
    g0 = NeXtVladDistillGraph(B, **kw)
    g = NeXtVladDistillGraph(B, dropout=0.5, dropout_seed=seed, **kw)
    assert g.teacher.dropout == 0.0 and g.student.dropout == 0.5 and g.student.dropout_seed == seed
    for gr in (g0, g):
        _perturbed(gr.student, 1)
        _perturbed(gr.teacher, 2)
    before = {k: v.clone() for k, v in g.teacher.state_dict().items()}
    for s in range(2):
        g0.step(qd, yd, nd, num_frames_host=n, apply=False)
        g.step(qd, yd, nd, num_frames_host=n)
        assert g.global_step == s + 1
        mask = dr.dropout_mask(B, SK, SD, 0.5, seed, 0, s)
        assert np.array_equal((g.student.Y_bf[:B].view(torch.int16) != 0).cpu().numpy(), mask), s
        assert torch.equal(g.teacher.Y_bf.view(torch.int16), g0.teacher.Y_bf.view(torch.int16))
        assert g0.student.Y_bf[:B].view(torch.int16).ne(0).all()
    after = g.teacher.state_dict()
    assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)


def test_train_main_records_the_rate_and_validate_drops_nothing(tmp_path, monkeypatch):
    """train.main --model NeXtVLADModel --nextvlad_dropout 0.5 --max_steps 2 on synthetic data writes a checkpoint that records the
    rate and the seed; validate --run_once True on that directory runs with both dropout wrappers patched to raise."""
    from efficientvideoclassification_youtube8m_amd import ops, train, validate
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    model = ["--frame_features", "True", "--feature_names", "rgb, audio", "--feature_sizes", "64, 64", "--model", "NeXtVLADModel",
             "--nextvlad_cluster_size", "16", "--nextvlad_groups", "4", "--nextvlad_hidden_size", "128", "--nextvlad_gating_reduction", "2"]
    tdir = str(tmp_path) + "/"
    try:
        FLAGS.reset()
        res = train.main(model + ["--train_data_pattern", "synthetic", "--batch_size", "16", "--nextvlad_frames", "grid", "--every_n", "1",
                                  "--synthetic_videos", "64", "--num_epochs", "1", "--start_new_model", "True", "--max_steps", "2",
                                  "--nextvlad_dropout", "0.5", "--nextvlad_dropout_seed", "13", "--train_dir", tdir])
        FLAGS.reset()
        assert res["iterations"] == 2 and res["graph"].global_step == 2 and res["graph"].tower.dropout == 0.5
        assert all(np.isfinite(h[1]["loss"]) for h in res["history"])
        tw = res["graph"].tower
        assert (tw.Y_bf[:tw.B].view(torch.int16) == 0).any()             # the last step dropped
        sd = torch.load(train.latest_checkpoint(tdir), map_location="cpu")
        assert sd["nextvlad_dropout"] == 0.5 and sd["nextvlad_dropout_seed"] == 13 and sd["global_step"] == 2
        monkeypatch.setattr(ops, "nextvlad_dropout_fwd", _raise)
        monkeypatch.setattr(ops, "nextvlad_dropout_bwd", _raise)
        info = validate.main(model + ["--train_dir", tdir, "--eval_data_pattern", "synthetic", "--synthetic_videos", "24", "--batch_size", "16",
                                      "--run_once", "True", "--top_k", "20"])
        assert info["epoch_id"] == 2 and np.isfinite(info["avg_loss"])
        monkeypatch.undo()
        # a restored run continues with the masks of an uninterrupted one: a fresh graph restored from the checkpoint takes its next
        # step under the mask of global_step 2
        from efficientvideoclassification_youtube8m_amd.distill import SingleTowerGraph
        from efficientvideoclassification_youtube8m_amd.towers import NeXtVladTower
        B = 16
        tw2 = NeXtVladTower(B, 300, 128, train.NUM_CLASSES, cluster_size=16, hidden_size=128, groups=4, expansion=2, gating_reduction=2,
                            device=DEV, frames="grid", every_n=1, dropout=sd["nextvlad_dropout"], dropout_seed=sd["nextvlad_dropout_seed"])
        g2 = SingleTowerGraph(tw2)
        train.restore_checkpoint(g2, train.latest_checkpoint(tdir))
        assert g2.global_step == 2
        q, x, n, labels = mm.synthetic_batch(B, seed=3, feature_size=128, vocab_size=train.NUM_CLASSES, dtype=np.float32)
        g2.step(torch.from_numpy(q).to(DEV), torch.from_numpy(labels.astype(np.uint8)).to(DEV), torch.from_numpy(n).to(DEV), num_frames_host=n)
        assert g2.global_step == 3
        assert np.array_equal((tw2.Y_bf[:B].view(torch.int16) != 0).cpu().numpy(), dr.dropout_mask(B, SK, SD, 0.5, 13, 0, 2))
    finally:
        FLAGS.reset()
