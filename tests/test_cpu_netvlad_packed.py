"""NetVLAD over a ragged, packed list of frames per video (--netvlad_frames grid) on the CPU: the float64 restatement
tests/_netvlad_packed_ref.py against oracle.model_math.netvlad_fwd / _bwd on equal lengths and against finite differences on ragged
ones, the derived per-element bounds of the two packed entries against an f32 evaluation of each kernel's chain and against planted
faults, and the refused flag combinations of train / validate - all without a device."""
import numpy as np
import pytest
import torch

import _netvlad_packed_ref as nv
from oracle import model_math as mm


def _setup(seed, n, T=12, F=8, K=3, H=8, V=6):
    rng = np.random.default_rng(seed)
    P = mm.init_netvlad_params(rng, F, K, H, V)
    for k in P:
        if k.endswith("gamma") or k.endswith("beta"):
            P[k] = P[k] + 0.2 * rng.standard_normal(P[k].shape)
    B = len(n)
    x = rng.standard_normal((B, T, F))
    y = rng.random((B, V)) > 0.6
    return rng, P, x, np.asarray(n), y


@pytest.mark.parametrize("S,every_n", [(4, 3), (12, 1)])
def test_packed_ref_on_equal_lengths_is_the_oracle(S, every_n):
    """n_b = S * every_n for every video and the draw u[b, j] = (j * every_n + 0.5) / n_b, which picks frame j * every_n: the ragged
    restatement and oracle.model_math.netvlad_fwd / _bwd see the same rows in the same order and agree to 1e-12 relative."""
    B = 4
    rng, P, x, n, y = _setup(11 + S, [S * every_n] * B)
    u = ((np.arange(S)[None, :] * every_n + 0.5) / n[:, None]).astype(np.float32)
    assert np.array_equal(mm.sample_random_frames_index(u, n), np.tile(np.arange(S) * every_n, (B, 1)))
    pred_f, cf = mm.netvlad_fwd(x, n, u, P)
    pred_p, cp = nv.netvlad_packed_fwd(x, n, every_n, P)
    rel = lambda a, b: np.abs(a - b).max() / max(1.0, np.abs(b).max())
    K = P["cluster_weights"].shape[1]
    assert np.array_equal(cp["r_bn"], cf[1])
    assert rel(cp["a"], cf[3].reshape(B * S, K)) < 1e-12 and rel(cp["asum"], cf[5]) < 1e-12
    assert rel(cp["V"], cf[7]) < 1e-12 and rel(cp["Y"], cf[11]) < 1e-12 and rel(pred_p, pred_f) < 1e-12
    dp = mm.cross_entropy_grad(pred_f, y)
    gf, gp = mm.netvlad_bwd(dp, cf), nv.netvlad_packed_bwd(dp, cp)
    assert set(gf) == set(gp) == set(P)
    for key in gf:
        assert rel(gp[key], gf[key]) < 1e-12, key


def test_packed_ref_backward_matches_finite_differences():
    """Every parameter tensor, several random entries each, on ragged lengths including 0 (L_b = 4, 0, 1, 2, 3, 4 at every_n = 3,
    T = 12, one video longer than T); the relu6 inputs stay clear of 0 and 6 by far more than a 1e-6 parameter step moves them."""
    rng, P, x, n, y = _setup(5, [12, 0, 1, 5, 7, 17])
    every_n = 3

    def loss(Q):
        p, _ = nv.netvlad_packed_fwd(x, n, every_n, Q)
        return mm.cross_entropy_loss(p, y)

    pred, cache = nv.netvlad_packed_fwd(x, n, every_n, P)
    assert list(cache["k"]) == [4, 0, 1, 2, 3, 4] and cache["r"].shape[0] == 14
    assert not cache["V"][1].any() and not cache["asum"][1].any()
    hb = cache["hid_bn"]
    margin = min(np.abs(hb).min(), np.abs(hb - 6).min())
    assert margin > 1e-4, margin
    grads = nv.netvlad_packed_bwd(mm.cross_entropy_grad(pred, y), cache)
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


def test_eval_forward_on_moving_statistics():
    """stats=...: with the training batch's own moments handed in as the statistics, the evaluation form reproduces the training forward."""
    rng, P, x, n, y = _setup(7, [12, 0, 5, 9])
    pred, c = nv.netvlad_packed_fwd(x, n, 2, P)
    stats = {s: (c[key][3], c[key][4]) for s, key in (("input_bn", "c_in"), ("cluster_bn", "c_cl"), ("hidden1_bn", "c_h"))}
    pred_e, _ = nv.netvlad_packed_fwd(x, n, 2, P, stats=stats)
    assert np.abs(pred_e - pred).max() < 1e-12


_CASES = {}


def _case(i):
    """The case, its references and the f32 evaluation of the kernels' chains: computed once, shared, never written to."""
    if i not in _CASES:
        c = nv.packed_case(*nv.NV_PACKED[i])
        _CASES[i] = (c, nv.agg_ref(c), nv.emulate(c))
    return _CASES[i]


@pytest.mark.parametrize("i", range(len(nv.NV_PACKED)))
def test_f32_chain_lies_inside_the_derived_bounds(i):
    """An honest f32 evaluation of each kernel's chain (numpy float32, one rounding per operation, the kernels' summation order) at
    every case of the GPU table: every element of V, asum, dx and da within its derived bound; empty videos exactly zero."""
    c, ref, emu = _case(i)
    for name in ("V", "asum", "dx", "da"):
        q = ref[name].ratio(emu[name])
        print("%s %-4s worst ratio %.3f" % (c.name, name, q.max() if q.size else 0.0))
        assert q.size == 0 or q.max() <= 1.0, (c.name, name, float(q.max()))
    for b, L in enumerate(c.ks):
        if L == 0:
            assert not ref["V"].ref[b].any() and not ref["V"].d[b].any() and not ref["asum"].d[b].any()
            assert not emu["V"][b].any() and not emu["asum"][b].any()


@pytest.mark.parametrize("i", [1, 2])
def test_planted_faults_lie_outside_the_bounds(i):
    """Each fault moves the output it belongs to beyond its bound (ratio > 1 somewhere, by a wide margin): the last frame of every video
    dropped from the forward sums, c2 of the wrong cluster in the epilogue, da without - q, xb without beta (forward and da)."""
    c, ref, _ = _case(i)
    worst = lambda name, got: float(ref[name].ratio(got[name]).max())
    dropped = nv.emulate(c, drop_last=True)
    assert worst("V", dropped) > 100 and worst("asum", dropped) > 100
    assert worst("V", nv.emulate(c, wrong_c2=True)) > 100
    assert worst("da", nv.emulate(c, no_q=True)) > 100
    nobeta = nv.emulate(c, no_beta=True)
    assert worst("V", nobeta) > 100 and worst("da", nobeta) > 100


def test_case_table_reaches_the_kernels_edges():
    """What the GPU table is chosen for, asserted on the table itself: an empty video first and last; a 64-row staging pass crossed by
    one row (65) and by a whole pass (129); odd lengths on the MFMA's (l, l + 1) pairs; F / 4 > 64 and more than one 192-column
    tile; K no multiple of 4 (the element-wise da store); one video far past the fixed-length entries' 64 frames."""
    ks_all = [ks for _, _, ks in nv.NV_PACKED]
    assert any(ks[0] == 0 and ks[-1] == 0 for ks in ks_all)
    assert any(65 in ks and 129 in ks and 64 in ks and 63 in ks and 1 in ks for ks in ks_all)
    assert any(F // 4 > 64 and F > 192 for _, F, _ in nv.NV_PACKED)
    assert any(K % 4 for K, _, _ in nv.NV_PACKED) and any(K % 4 == 0 and K % 32 for K, _, _ in nv.NV_PACKED)
    assert any(max(ks) >= 300 for ks in ks_all)


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
    assert FLAGS.netvlad_frames == "sampled" and FLAGS.netvlad_serve_every_n == 0 and FLAGS.every_n == 1
    FLAGS.parse(["--netvlad_frames", "grid", "--every_n", "10", "--netvlad_serve_every_n", "30"])
    assert FLAGS.netvlad_frames == "grid" and FLAGS.every_n == 10 and FLAGS.netvlad_serve_every_n == 30
    FLAGS.reset()


def test_ws_size_function():
    from efficientvideoclassification_youtube8m_amd import ops
    assert ops.netvlad_aggregate_packed_bwd_ws(3, 18, 100) == 3 * 100 * 20 + 3 * 18
    assert ops.netvlad_aggregate_packed_bwd_ws(256, 64, 1152) == 256 * 1152 * 64 + 256 * 64


def test_check_netvlad_frames():
    from efficientvideoclassification_youtube8m_amd.towers import check_netvlad_frames
    with pytest.raises(ValueError, match=r"--netvlad_frames 'every'.*sampled\|grid"):
        check_netvlad_frames("every", 1, 300)
    with pytest.raises(ValueError, match=r"--netvlad_frames grid.*NetVLADModel.*DbofModel"):
        check_netvlad_frames("grid", 1, 300, model="DbofModel")
    for every_n in (0, 301):
        with pytest.raises(ValueError, match=r"--netvlad_frames grid.*--every_n %d.*--max_num_frames 300" % every_n):
            check_netvlad_frames("grid", every_n, 300, model="NetVLADModel")
    with pytest.raises(ValueError, match=r"--netvlad_frames grid.*2 ranks"):
        check_netvlad_frames("grid", 10, 300, model="NetVLADModel", world=2)
    with pytest.raises(ValueError, match=r"--netvlad_frames grid.*--precision high"):
        check_netvlad_frames("grid", 10, 300, model="NetVLADModel", precision="high")
    check_netvlad_frames("grid", 300, 300, model="NetVLADModel")               # the edges that are allowed
    check_netvlad_frames("grid", 1, 300)
    check_netvlad_frames("sampled", 0, 300, model="DbofModel", world=8, precision="high")       # nothing of this concerns the sampled mode


def test_train_refusals_touch_no_device(no_device, monkeypatch, tmp_path):
    """Every refused combination is a ValueError naming the flags, from train.main and from the tower's constructor, before any
    device call; --nextvlad_frames grid with this model keeps its old message."""
    from efficientvideoclassification_youtube8m_amd import train
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    from efficientvideoclassification_youtube8m_amd.towers import NetVladTower
    common = ["--train_data_pattern", "synthetic", "--frame_features", "True", "--feature_names", "rgb, audio", "--feature_sizes", "64, 64",
              "--batch_size", "16", "--start_new_model", "True", "--train_dir", str(tmp_path) + "/", "--netvlad_frames", "grid"]

    def main(argv, match, env=None):
        FLAGS.reset()
        if env:
            monkeypatch.setenv(*env)
        try:
            with pytest.raises(ValueError, match=match):
                train.main(argv)
        finally:
            FLAGS.reset()
            if env:
                monkeypatch.delenv(env[0])

    main(common + ["--model", "DbofModel"], r"--netvlad_frames grid.*NetVLADModel.*DbofModel")
    main(common + ["--model", "NeXtVLADModel"], r"--netvlad_frames grid.*NetVLADModel.*NeXtVLADModel")
    main(common + ["--model", "NetVLADModel", "--every_n", "0"], r"--every_n 0")
    main(common + ["--model", "NetVLADModel", "--every_n", "301"], r"--every_n 301.*--max_num_frames 300")
    main(common + ["--model", "NetVLADModel", "--every_n", "10", "--precision", "high"], r"--netvlad_frames grid.*--precision high")
    main(common + ["--model", "NetVLADModel", "--every_n", "10"], r"--netvlad_frames grid.*2 ranks", env=("WORLD_SIZE", "2"))
    main(common[:-1] + ["every", "--model", "NetVLADModel"], r"--netvlad_frames 'every'")
    main(common[:-2] + ["--nextvlad_frames", "grid", "--model", "NetVLADModel"], r"--nextvlad_frames grid is built for --model NeXtVLADModel, not NetVLADModel")
    kw = dict(max_frames=300, feature_size=64, vocab_size=10, cluster_size=64, hidden_size=64, device="cuda:0")
    for every_n in (0, 301):
        with pytest.raises(ValueError, match="--every_n %d" % every_n):
            NetVladTower(8, frames="grid", every_n=every_n, **kw)
    with pytest.raises(ValueError, match="--netvlad_frames 'all'"):
        NetVladTower(8, frames="all", **kw)
    with pytest.raises(ValueError, match="iterations=65"):                      # the cap of the sampled mode stays
        NetVladTower(8, iterations=65, **kw)


def _host_checkpoint(path, F=128, V=None, K=64, H=64, Mx=2, meta=()):
    """A NetVLAD checkpoint written on the host with the names and TF layouts of NetVladTower.state_dict()."""
    from efficientvideoclassification_youtube8m_amd import train
    from efficientvideoclassification_youtube8m_amd.towers import NetVladTower
    V = train.NUM_CLASSES if V is None else V
    sd = {"global_step": 3}
    sd.update(meta)
    for k, shp in NetVladTower.checkpoint_shapes(F, V, K, H, Mx).items():
        sd["model/" + k] = torch.zeros(shp)
    torch.save(sd, str(path / "model.ckpt-3.pt"))
    return sd


def test_validate_refusals_touch_no_device(no_device, tmp_path):
    """validate.main --model NetVLADModel: no checkpoint, a checkpoint of other sizes (the first mismatching variable and both shapes
    are named), one of another family, a bad --netvlad_serve_every_n, another precision - all on the host.  The recorded grid is what
    a served tower runs on, every real frame for a sampled checkpoint, unless the flag names another."""
    from efficientvideoclassification_youtube8m_amd import validate
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    common = ["--eval_data_pattern", "synthetic", "--frame_features", "True", "--feature_names", "rgb, audio", "--feature_sizes", "64, 64",
              "--batch_size", "16", "--run_once", "True", "--model", "NetVLADModel", "--netvlad_cluster_size", "64", "--netvlad_hidden_size", "64"]

    def main(extra, exc, match):
        FLAGS.reset()
        try:
            with pytest.raises(exc, match=match):
                validate.main(common + extra)
        finally:
            FLAGS.reset()

    empty = tmp_path / "empty"
    empty.mkdir()
    main(["--train_dir", str(empty) + "/"], IOError, "unable to find a checkpoint")
    good = tmp_path / "good"
    good.mkdir()
    _host_checkpoint(good, meta={"netvlad_frames": "grid", "every_n": 10}.items())
    main(["--train_dir", str(good) + "/", "--netvlad_cluster_size", "128"], ValueError,
         r"model/cluster_weights of .* has shape \(128, 64\), the size flags \(--netvlad_\*.*\) give \(128, 128\)")
    main(["--train_dir", str(good) + "/", "--netvlad_hidden_size", "128"], ValueError, r"model/hidden1_weights of .*\(8192, 64\).*\(8192, 128\)")
    main(["--train_dir", str(good) + "/", "--feature_sizes", "64, 128"], ValueError, r"model/input_bn/beta of .*\(128,\).*\(192,\)")
    main(["--train_dir", str(good) + "/", "--netvlad_serve_every_n", "301"], ValueError, r"--netvlad_serve_every_n 301.*--max_num_frames 300")
    main(["--train_dir", str(good) + "/", "--netvlad_serve_every_n", "-1"], ValueError, r"--netvlad_serve_every_n -1")
    main(["--train_dir", str(good) + "/", "--precision", "high"], ValueError, r"--precision high with --model NetVLADModel")
    other = tmp_path / "other"
    other.mkdir()
    torch.save({"global_step": 1, "model/expansion_weights": torch.zeros(4, 4)}, str(other / "model.ckpt-1.pt"))
    main(["--train_dir", str(other) + "/"], ValueError, r"holds no variable model/input_bn/beta \(not a NetVLADModel checkpoint\)")
    sd = torch.load(str(good / "model.ckpt-3.pt"))
    assert validate.netvlad_every_n(sd) == 10 and validate.netvlad_every_n(sd, 30) == 30 and validate.netvlad_every_n(sd, 10) == 10
    assert validate.netvlad_every_n({"every_n": 10}) == 1 and validate.netvlad_every_n({}, 5) == 5      # a sampled checkpoint: every real frame


def test_other_entry_points_keep_their_refusals(no_device, tmp_path):
    """inference --model NetVLADModel stays unbuilt (NotImplementedError), as DESIGN.md 8 lists it."""
    from efficientvideoclassification_youtube8m_amd import inference
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    FLAGS.reset()
    try:
        FLAGS.parse(["--model", "NetVLADModel", "--output_file", str(tmp_path / "o.csv"), "--input_data_pattern", "synthetic", "--frame_features", "True"])
        with pytest.raises(NotImplementedError, match="NetVLADModel has no inference path"):
            inference.check_flags()
    finally:
        FLAGS.reset()
