"""Serial distillation over the NeXtVLAD towers on the CPU: the float64 restatement tests/_nextvlad_distill_ref.py
against finite differences of the student's total loss, its evaluation-mode forward against the training-mode one, the rule that
reads the teacher's grid from a checkpoint, and every refused combination - all without a device."""
import numpy as np
import pytest
import torch

import _nextvlad_distill_ref as dx
import _nextvlad_packed_ref as px
import _nextvlad_ref as nx
from oracle import model_math as mm


def _setup(seed, n, T=12, F=8, lam=2, G=4, K=3, H=8, rho=2, V=6):
    """The sizes of test_cpu_nextvlad_packed.py: a teacher and a student with perturbed batch-norm scales / offsets."""
    rng = np.random.default_rng(seed)
    towers = []
    for _ in range(2):
        P = nx.init_params(rng, F, lam, G, K, H, rho, V)
        for k in P:
            if k.endswith("gamma") or k.endswith("beta"):
                P[k] = P[k] + 0.2 * rng.standard_normal(P[k].shape)
        towers.append(P)
    x = rng.standard_normal((len(n), T, F))
    y = rng.random((len(n), V)) > 0.6
    return rng, towers[0], towers[1], x, np.asarray(n), y


def _teacher_moving(rng, teacher, x, n, every_n):
    """Moving statistics of a teacher that has been trained: its batch moments on this batch, perturbed."""
    _, cache = px.nextvlad_packed_fwd(x, n, every_n, teacher)
    M = dx.batch_moments(cache)
    for k in M:
        M[k] = M[k] * (1.0 + 0.1 * rng.random(M[k].shape)) if k.endswith("variance") else M[k] + 0.05 * rng.standard_normal(M[k].shape)
    return M


@pytest.mark.parametrize("on", [("rep", "pred", "ce"), ("rep",), ("pred", "ce")])
def test_student_gradients_match_finite_differences(on):
    """Central differences of g_rep L_REP + L_PRED + L_CE (the words of `on`) on every student parameter tensor, several random entries
    each; ragged lengths, teacher on every frame, student on every third; step and bound of test_cpu_nextvlad_packed.py."""
    rng, teacher, student, x, n, y = _setup(7, [12, 1, 5, 7, 17])
    M = _teacher_moving(rng, teacher, x, n, 1)

    def loss(Q):
        return dx.distill_step(x, n, y, teacher, M, Q, 1, 3, on=on, with_grads=False)["total"]

    ref = dx.distill_step(x, n, y, teacher, M, student, 1, 3, on=on)
    assert list(ref["teacher_cache"]["k"]) == [12, 1, 5, 7, 12] and list(ref["student_cache"]["k"]) == [4, 1, 2, 3, 4]
    g1 = ref["student_cache"]["g1bn"]
    assert min(np.abs(g1).min(), np.abs(g1 - 6).min()) > 1e-3          # no relu6 kink within a 1e-6 parameter step
    if "rep" not in on:
        assert not ref["dstate"].any()
    grads = ref["student_grads"]
    assert set(grads) == set(student)
    eps = 1e-6
    for k in student:
        flat = student[k].reshape(-1)
        for j in rng.choice(flat.size, size=min(6, flat.size), replace=False):
            old = flat[j]
            flat[j] = old + eps
            lp = loss(student)
            flat[j] = old - eps
            lm = loss(student)
            flat[j] = old
            fd = (lp - lm) / (2 * eps)
            got = grads[k].reshape(-1)[j]
            assert abs(fd - got) <= 1e-5 * max(1.0, abs(fd)) + 1e-7, (on, k, j, fd, got)


def test_dstate_none_is_the_packed_reverse_mode():
    rng, teacher, student, x, n, y = _setup(3, [9, 4, 12])
    pred, cache = px.nextvlad_packed_fwd(x, n, 3, student)
    dp = mm.cross_entropy_grad(pred, y)
    a, b = dx.nextvlad_packed_bwd(dp, cache), px.nextvlad_packed_bwd(dp, cache)
    assert all(np.array_equal(a[k], b[k]) for k in b)
    z = dx.nextvlad_packed_bwd(dp, cache, np.zeros_like(cache["out"]))
    assert set(z) == set(b) and all(np.array_equal(z[k], b[k]) for k in b)


@pytest.mark.parametrize("every_n", [1, 3])
def test_eval_forward_on_batch_moments_is_the_training_forward(every_n):
    rng, teacher, _, x, n, y = _setup(11, [12, 0, 5, 7, 17])
    pred, cache = px.nextvlad_packed_fwd(x, n, every_n, teacher)
    pe, oe, ce = dx.nextvlad_packed_eval_fwd(x, n, every_n, teacher, dx.batch_moments(cache))
    rel = lambda a, b: np.abs(a - b).max() / max(1.0, np.abs(b).max())
    assert np.array_equal(ce["r"], cache["r"]) and np.array_equal(ce["row_off"], cache["row_off"])
    for got, want in ((ce["a"], cache["a"]), (ce["V"], cache["V"]), (ce["Y"], cache["Y"]), (oe, cache["out"]), (pe, pred)):
        assert rel(got, want) < 1e-12
    M = _teacher_moving(rng, teacher, x, n, every_n)                   # other statistics: another function
    assert rel(dx.nextvlad_packed_eval_fwd(x, n, every_n, teacher, M)[0], pred) > 1e-6


def test_teacher_every_n_from_checkpoint_metadata():
    from efficientvideoclassification_youtube8m_amd.train import nextvlad_teacher_every_n as f
    assert f({"global_step": 4}) == 1                                                  # a sampled tower's checkpoint: every real frame
    assert f({"nextvlad_frames": "sampled", "every_n": 10}) == 1
    assert f({"nextvlad_frames": "grid", "every_n": 1}) == 1
    assert f({"nextvlad_frames": "grid", "every_n": 5}) == 5
    # a distillation checkpoint: every_n is its student's, model/* is the frozen teacher and runs on teacher_every_n (resume)
    assert f({"nextvlad_frames": "grid", "every_n": 10, "teacher_every_n": 2, "distill_losses": "rep,pred,ce"}) == 2


SIZES = dict(feature_size=128, vocab_size=10, cluster_size=16, hidden_size=128, groups=4, expansion=2, gating_reduction=2)


def test_checkpoint_shapes_and_size_mismatch(monkeypatch):
    from efficientvideoclassification_youtube8m_amd import train
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    from efficientvideoclassification_youtube8m_amd.towers import NeXtVladTower
    FLAGS.reset()
    FLAGS.parse(["--teacher_dir", "/t/", "--nextvlad_cluster_size", "16", "--nextvlad_groups", "4", "--nextvlad_hidden_size", "128",
                 "--nextvlad_gating_reduction", "2"])
    monkeypatch.setattr(train, "NUM_CLASSES", 10)
    want = NeXtVladTower.checkpoint_shapes(128, 10, 16, 128, 4, 2, 2, 2)
    assert want["hidden1_weights"] == (64 * 16, 128) and want["cluster_weights2"] == (64, 16) and want["expansion_weights"] == (128, 256)
    assert want["vlad_bn/moving_mean"] == (1024,) and want["classifier/gates/weights"] == (128, 30)
    assert len(want) == 28                       # 9 weights and biases, 4 x (beta, gamma, two moving statistics), 3 of the head
    sd = {"model/" + k: torch.zeros(shp) for k, shp in want.items()}
    train.check_nextvlad_teacher_shapes(sd, 128, "model.ckpt-4.pt")
    bad = dict(sd)
    bad["model/cluster_weights"] = torch.zeros((256, 4 * 32))
    with pytest.raises(ValueError, match=r"model/cluster_weights of model.ckpt-4.pt has shape \(256, 128\), the size flags.*\(256, 64\)"):
        train.check_nextvlad_teacher_shapes(bad, 128, "model.ckpt-4.pt")
    with pytest.raises(ValueError, match=r"no variable model/expansion_weights"):
        train.check_nextvlad_teacher_shapes({"model/RNN_L1/x": torch.zeros(1)}, 128, "model.ckpt-4.pt")
    with pytest.raises(ValueError, match=r"holds no model/\* variables"):
        train.check_nextvlad_teacher_shapes({"global_step": 3}, 128, "model.ckpt-4.pt")
    FLAGS.reset()


@pytest.fixture
def no_device(monkeypatch):
    from efficientvideoclassification_youtube8m_amd import ops

    def touched(*a, **k):
        raise AssertionError("the device was touched before the flags were checked")
    monkeypatch.setattr(torch.cuda, "set_device", touched)
    monkeypatch.setattr(torch.cuda, "_lazy_init", touched)
    monkeypatch.setattr(ops, "check_device", touched)


class _TwoRanks:
    def size(self):
        return 2


def test_graph_refusals_touch_no_device(no_device):
    from efficientvideoclassification_youtube8m_amd.distill import NeXtVladDistillGraph
    kw = dict(SIZES, max_frames=300, device="cuda:0")
    with pytest.raises(ValueError, match="not data parallel.*2 ranks"):
        NeXtVladDistillGraph(8, process_group=_TwoRanks(), **kw)
    with pytest.raises(ValueError, match="CrossEntropyLoss built into its loss section.*HingeLoss"):
        NeXtVladDistillGraph(8, label_loss="HingeLoss", **kw)
    with pytest.raises(ValueError, match="precision 'high' is refused"):
        NeXtVladDistillGraph(8, precision="high", **kw)
    for bad in (0, 301):
        with pytest.raises(ValueError, match="--every_n %d" % bad):
            NeXtVladDistillGraph(8, every_n=bad, **kw)
        with pytest.raises(ValueError, match="--every_n %d" % bad):
            NeXtVladDistillGraph(8, every_n=10, teacher_every_n=bad, **kw)
    with pytest.raises(ValueError, match="distill_losses"):
        NeXtVladDistillGraph(8, distill_losses="rep,kl", **kw)


def test_flag_refusals_touch_no_device(no_device, monkeypatch, tmp_path):
    """train.main: every refused combination of --teacher_dir with --model NeXtVLADModel is a ValueError naming the flags."""
    from efficientvideoclassification_youtube8m_amd import train
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    tdir = str(tmp_path / "teacher") + "/"
    common = ["--train_data_pattern", "synthetic", "--frame_features", "True", "--feature_names", "rgb, audio", "--feature_sizes", "64, 64",
              "--batch_size", "16", "--start_new_model", "True", "--train_dir", str(tmp_path) + "/", "--model", "NeXtVLADModel",
              "--nextvlad_frames", "grid", "--every_n", "10"]

    def main(extra, match, env=None, argv=common, finetune=False):
        FLAGS.reset()
        if env:
            monkeypatch.setenv(*env)
        try:
            with pytest.raises(ValueError, match=match):
                train.main(argv + extra + (["--finetune"] if finetune else []))
        finally:
            FLAGS.reset()
            if env:
                monkeypatch.delenv(env[0])

    sampled = [a if a != "grid" else "sampled" for a in common]
    main(["--teacher_dir", tdir], r"--teacher_dir .* with --model NeXtVLADModel and --nextvlad_frames sampled", argv=sampled)
    main(["--teacher_dir", tdir, "--serial_student_dirs", "%s,%s" % (tmp_path / "a", tmp_path / "b")],
         r"--serial_student_dirs.*HierarchicalLstmModel, not NeXtVLADModel")
    main(["--teacher_dirs", "%s,%s" % (tmp_path / "a", tmp_path / "b")], r"--teacher_dirs.*HierarchicalLstmModel, not --model NeXtVLADModel")
    main(["--teacher_preds_pattern", str(tmp_path / "*.csv"), "--train_data_pattern", str(tmp_path / "*.tfrecord")],
         r"--teacher_preds_pattern.*HierarchicalLstmModel, not --model NeXtVLADModel")
    main(["--teacher_dir", tdir, "--teacher_only", "True"], r"--teacher_dir .* with --teacher_only")
    main(["--teacher_dir", tdir], r"--teacher_dir .* with --finetune", finetune=True)
    main(["--teacher_dir", tdir], r"2 ranks", env=("WORLD_SIZE", "2"))
    main(["--teacher_dir", tdir, "--label_loss", "HingeLoss"], r"--label_loss HingeLoss with --teacher_dir")
    main(["--teacher_dir", tdir, "--precision", "high"], r"--nextvlad_frames grid.*--precision high")
    main(["--teacher_dir", tdir, "--every_n", "301"], r"--every_n 301.*--max_num_frames 300")
    main(["--teacher_dir", tdir], r"--teacher_dir .*: no model.ckpt-\*.pt checkpoint there")          # an empty teacher directory
    FLAGS.reset()
    FLAGS.parse(["--teacher_dir", tdir, "--model", "DbofModel"])
    try:
        from efficientvideoclassification_youtube8m_amd import frame_level_models, losses
        with pytest.raises(ValueError, match="built for HierarchicalLstmModel and NeXtVLADModel, not DbofModel"):
            train.build_graph(frame_level_models.DbofModel(), losses.CrossEntropyLoss(), 128, 16, 10, "cuda:0")
    finally:
        FLAGS.reset()


def test_student_init_flag_default():
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    FLAGS.reset()
    assert FLAGS.student_init_from_teacher is False
    FLAGS.parse(["--student_init_from_teacher", "True"])
    assert FLAGS.student_init_from_teacher is True
    FLAGS.reset()
