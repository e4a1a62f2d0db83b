"""NeXtVLAD over a ragged, packed list of frames per video (--nextvlad_frames grid) on the CPU: the float64
restatement tests/_nextvlad_packed_ref.py against finite differences and against the fixed-length restatement, the host function
that lays the packed rows out, and the refused flag combinations - all without a device."""
import numpy as np
import pytest
import torch

import _nextvlad_packed_ref as px
import _nextvlad_ref as nx
from oracle import model_math as mm


def _setup(seed, n, T=12, F=8, lam=2, G=4, K=3, H=8, rho=2, V=6):
    rng = np.random.default_rng(seed)
    P = nx.init_params(rng, F, lam, G, K, H, rho, V)
    for k in P:
        if k.endswith("gamma") or k.endswith("beta"):
            P[k] = P[k] + 0.2 * rng.standard_normal(P[k].shape)
    B = len(n)
    x = rng.standard_normal((B, T, F))
    y = rng.random((B, V)) > 0.6
    return rng, P, x, np.asarray(n), y


def test_packed_ref_backward_matches_finite_differences():
    """Every parameter tensor, several random entries each, on ragged lengths (k_b = 4, 1, 2, 3, 4 at every_n = 3, T = 12, one
    video longer than T); bound and relu6-margin check as in test_cpu_nextvlad_ref.py."""
    rng, P, x, n, y = _setup(5, [12, 1, 5, 7, 17])
    every_n = 3

    def loss(Q):
        p, _ = px.nextvlad_packed_fwd(x, n, every_n, Q)
        return mm.cross_entropy_loss(p, y)

    pred, cache = px.nextvlad_packed_fwd(x, n, every_n, P)
    assert list(cache["k"]) == [4, 1, 2, 3, 4] and cache["r"].shape[0] == 14
    g1 = cache["g1bn"]
    margin = min(np.abs(g1).min(), np.abs(g1 - 6).min())
    assert margin > 1e-3, margin                   # far more than any relu6 input moves under a 1e-6 parameter step
    grads = px.nextvlad_packed_bwd(mm.cross_entropy_grad(pred, y), cache)
    assert set(grads) == set(P)
    eps = 1e-6
    for k in P:
        flat = P[k].reshape(-1)
        for j in rng.choice(flat.size, size=min(6, flat.size), replace=False):
            old = flat[j]
            flat[j] = old + eps
            lp = loss(P)
            flat[j] = old - eps
            lm = loss(P)
            flat[j] = old
            fd = (lp - lm) / (2 * eps)
            got = grads[k].reshape(-1)[j]
            assert abs(fd - got) <= 1e-5 * max(1.0, abs(fd)) + 1e-7, (k, j, fd, got)


@pytest.mark.parametrize("S,every_n", [(4, 3), (12, 1)])
def test_packed_ref_on_equal_lengths_is_the_fixed_length_ref(S, every_n):
    """n_b = S * every_n for every video and the draw u[b, j] = (j * every_n + 0.5) / n_b, which picks frame j * every_n: the two
    restatements see the same rows in the same order and agree to 1e-12 relative (float64 sums in another association)."""
    B = 4
    rng, P, x, n, y = _setup(11 + S, [S * every_n] * B)
    u = ((np.arange(S)[None, :] * every_n + 0.5) / n[:, None]).astype(np.float32)
    assert np.array_equal(mm.sample_random_frames_index(u, n), np.tile(np.arange(S) * every_n, (B, 1)))
    pred_f, cf = nx.nextvlad_fwd(x, n, u, P)
    pred_p, cp = px.nextvlad_packed_fwd(x, n, every_n, P)
    rel = lambda a, b: np.abs(a - b).max() / max(1.0, np.abs(b).max())
    assert np.array_equal(cp["r"], cf["r"])
    for key in ("xe", "V", "asum", "Y"):
        assert rel(cp[key], cf[key]) < 1e-12, key
    assert rel(cp["a"], cf["a"]) < 1e-12 and rel(pred_p, pred_f) < 1e-12
    dp = mm.cross_entropy_grad(pred_f, y)
    gf, gp = nx.nextvlad_bwd(dp, cf), px.nextvlad_packed_bwd(dp, cp)
    assert set(gf) == set(gp)
    for key in gf:
        assert rel(gp[key], gf[key]) < 1e-12, key


def test_packed_ref_video_without_frames():
    """k_b = 0: a zero descriptor (V, asum, U), no row, and nothing of its dV reaches da or dxe."""
    rng, P, x, n, y = _setup(3, [7, 0, 12, 0])
    pred, c = px.nextvlad_packed_fwd(x, n, 3, P)
    assert list(c["k"]) == [3, 0, 4, 0] and list(c["row_off"]) == [0, 3, 3, 7, 7] and list(c["vid"]) == [0] * 3 + [2] * 4
    for b in (1, 3):
        assert not c["V"][b].any() and not c["asum"][b].any() and not c["U"][b].any()
    assert np.isfinite(pred).all()
    px.nextvlad_packed_bwd(mm.cross_entropy_grad(pred, y), c)
    dV2 = c["dV"].copy()
    dV2[[1, 3]] += rng.standard_normal(dV2[[1, 3]].shape)
    da2, dx2 = px.aggregate_bwd(dV2, c)
    assert np.array_equal(da2, c["da"]) and np.array_equal(dx2, c["dx3"]) and c["da"].shape[0] == 7


@pytest.mark.parametrize("every_n", [1, 7, 12])
def test_grid_plan_offsets(every_n):
    """ops.GridPlan against the index lists written out the slow way, on n in {0, 1, every_n - 1, every_n, every_n + 1, T, T + 5}."""
    from efficientvideoclassification_youtube8m_amd import ops
    T = 12
    n = np.array([0, 1, every_n - 1, every_n, every_n + 1, T, T + 5], np.int32)
    plan = ops.GridPlan(n, every_n, T)
    lists = px.grid_frames(n, every_n, T)
    k = np.array([len(f) for f in lists])
    assert plan.k.dtype == np.int32 and plan.row_off.dtype == np.int32 and plan.row_off.shape == (len(n) + 1,)
    assert np.array_equal(plan.k, k) and np.array_equal(plan.row_off, np.concatenate([[0], np.cumsum(k)]))
    assert plan.R == k.sum() and plan.Rp % 32 == 0 and 0 <= plan.Rp - plan.R < 32 and plan.max_k == k.max()
    assert plan.k[0] == 0 and plan.k[-1] == plan.k[-2] == -(-T // every_n)       # no frame; clipped to T
    for f in lists:
        assert all(t < T for t in f)
    assert ops.grid_capacity(len(n), T, every_n) == ops.round_up(len(n) * -(-T // every_n), 32) >= plan.Rp
    empty = ops.GridPlan(np.zeros(3, np.int32), every_n, T)
    assert (empty.R, empty.Rp, empty.max_k) == (0, 0, 0)
    for bad in (0, -1, T + 1):
        with pytest.raises(ValueError, match="every_n"):
            ops.GridPlan(n, bad, T)


@pytest.fixture
def no_device(monkeypatch):
    from efficientvideoclassification_youtube8m_amd import ops

    def touched(*a, **k):
        raise AssertionError("the device was touched before the flags were checked")
    monkeypatch.setattr(torch.cuda, "set_device", touched)
    monkeypatch.setattr(torch.cuda, "_lazy_init", touched)
    monkeypatch.setattr(ops, "check_device", touched)


def test_grid_flag_defaults():
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    FLAGS.reset()
    assert FLAGS.nextvlad_frames == "sampled" and FLAGS.every_n == 1
    FLAGS.parse(["--nextvlad_frames", "grid", "--every_n", "10"])
    assert FLAGS.nextvlad_frames == "grid" and FLAGS.every_n == 10
    FLAGS.reset()


def test_grid_refusals_touch_no_device(no_device, monkeypatch, tmp_path):
    """Every refused combination is a ValueError naming the flags, from train.main and from the tower's constructor, before
    any device call."""
    from efficientvideoclassification_youtube8m_amd import train
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    from efficientvideoclassification_youtube8m_amd.towers import NeXtVladTower, check_nextvlad_frames
    common = ["--train_data_pattern", "synthetic", "--frame_features", "True", "--feature_names", "rgb, audio", "--feature_sizes", "64, 64",
              "--batch_size", "16", "--start_new_model", "True", "--train_dir", str(tmp_path) + "/", "--nextvlad_frames", "grid"]

    def main(extra, match, env=None):
        FLAGS.reset()
        if env:
            monkeypatch.setenv(*env)
        try:
            with pytest.raises(ValueError, match=match):
                train.main(common + extra)
        finally:
            FLAGS.reset()
            if env:
                monkeypatch.delenv(env[0])

    main(["--model", "DbofModel"], r"--nextvlad_frames grid.*NeXtVLADModel.*DbofModel")
    main(["--model", "NetVLADModel"], r"--nextvlad_frames grid.*NeXtVLADModel")
    main(["--model", "NeXtVLADModel", "--every_n", "0"], r"--every_n 0")
    main(["--model", "NeXtVLADModel", "--every_n", "301"], r"--every_n 301.*--max_num_frames 300")
    main(["--model", "NeXtVLADModel", "--every_n", "10", "--precision", "high"], r"--nextvlad_frames grid.*--precision high")
    main(["--model", "NeXtVLADModel", "--every_n", "10"], r"--nextvlad_frames grid.*2 ranks", env=("WORLD_SIZE", "2"))
    FLAGS.reset()
    with pytest.raises(ValueError, match=r"--nextvlad_frames 'every'"):
        train.main(common[:-1] + ["every", "--model", "NeXtVLADModel"])
    FLAGS.reset()
    kw = dict(max_frames=300, feature_size=64, vocab_size=10, cluster_size=16, hidden_size=128, groups=4, expansion=2, gating_reduction=2,
              device="cuda:0")
    for every_n in (0, 301):
        with pytest.raises(ValueError, match="--every_n %d" % every_n):
            NeXtVladTower(8, frames="grid", every_n=every_n, **kw)
    with pytest.raises(ValueError, match="--nextvlad_frames 'all'"):
        NeXtVladTower(8, frames="all", **kw)
    with pytest.raises(ValueError, match="2 ranks"):
        check_nextvlad_frames("grid", 10, 300, model="NeXtVLADModel", world=2)
    check_nextvlad_frames("grid", 300, 300, model="NeXtVLADModel")             # the edges that are allowed
    check_nextvlad_frames("grid", 1, 300)
    check_nextvlad_frames("sampled", 0, 300, model="DbofModel", world=8, precision="high")      # nothing of this concerns the sampled mode
