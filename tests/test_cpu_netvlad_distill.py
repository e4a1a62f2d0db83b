"""Serial distillation over the NetVLAD towers on the CPU: the float64 restatement tests/_netvlad_distill_ref.py
against finite differences of the student's total loss, the rule that reads the teacher's grid from a checkpoint, what validate makes
of a distillation checkpoint, and every refused combination - all without a device."""
import types

import numpy as np
import pytest
import torch

import _netvlad_distill_ref as dx
import _netvlad_packed_ref as px
from oracle import model_math as mm

EPS = 1e-6                                       # the parameter step of the central differences


def _setup(seed, n, T=12, F=8, K=3, H=8, V=6):
    """The sizes of test_cpu_netvlad_packed.py: a teacher and a student with perturbed batch-norm scales / offsets, and moving
    statistics of the teacher that are not its initial ones."""
    rng = np.random.default_rng(seed)
    towers = []
    for _ in range(2):
        P = mm.init_netvlad_params(rng, F, K, H, V)
        for k in P:
            if k.endswith("gamma") or k.endswith("beta"):
                P[k] = P[k] + 0.2 * rng.standard_normal(P[k].shape)
        towers.append(P)
    M = {}
    for s, C in (("input_bn", F), ("cluster_bn", K), ("hidden1_bn", H)):
        M[s + "/moving_mean"] = 0.2 * rng.standard_normal(C)
        M[s + "/moving_variance"] = np.exp(0.2 * rng.standard_normal(C))
    x = rng.standard_normal((len(n), T, F))
    y = rng.random((len(n), V)) > 0.6
    return rng, towers[0], M, towers[1], x, np.asarray(n), y


@pytest.mark.parametrize("on", [("rep", "pred", "ce"), ("rep",), ("pred", "ce")])
def test_student_gradients_match_finite_differences(on):
    """Central differences of g_rep L_REP + L_PRED + L_CE (the words of `on`) on every student parameter tensor, several random entries
    each; one empty video, one shorter than every_n, one longer than T; teacher on every frame, student on every third; step and
    bound of test_cpu_netvlad_packed.py.  The seed is one at which no pre-activation of hidden1_bn's relu6 comes near 0 or 6."""
    rng, teacher, M, student, x, n, y = _setup(4, [12, 0, 2, 5, 7, 17])

    def loss(Q):
        return dx.distill_step(x, n, y, teacher, M, Q, 1, 3, on=on, with_grads=False)["total"]

    ref = dx.distill_step(x, n, y, teacher, M, student, 1, 3, on=on)
    assert list(ref["teacher_cache"]["k"]) == [12, 0, 2, 5, 7, 12] and list(ref["student_cache"]["k"]) == [4, 0, 1, 2, 3, 4]
    hb = ref["student_cache"]["hid_bn"]
    margin = min(np.abs(hb).min(), np.abs(hb - 6).min())
    assert margin > 10 * EPS, margin                                   # the kink is not sampled
    assert ((hb > 0) & (hb < 6)).any() and not ((hb > 0) & (hb < 6)).all()      # both sides of the mask are exercised
    if "rep" not in on:
        assert not ref["dstate"].any()
    else:
        assert ref["dstate"].any()
    grads = ref["student_grads"]
    assert set(grads) == set(student)
    for k in student:
        flat = student[k].reshape(-1)
        for j in rng.choice(flat.size, size=min(6, flat.size), replace=False):
            old = flat[j]
            flat[j] = old + EPS
            lp = loss(student)
            flat[j] = old - EPS
            lm = loss(student)
            flat[j] = old
            fd = (lp - lm) / (2 * EPS)
            got = grads[k].reshape(-1)[j]
            assert abs(fd - got) <= 1e-5 * max(1.0, abs(fd)) + 1e-7, (on, k, j, fd, got)


def test_dstate_none_is_the_packed_reverse_mode():
    rng, teacher, M, student, x, n, y = _setup(3, [9, 0, 4, 12])
    pred, cache = px.netvlad_packed_fwd(x, n, 3, student)
    dp = mm.cross_entropy_grad(pred, y)
    b = px.netvlad_packed_bwd(dp, cache)
    a = dx.netvlad_packed_bwd(dp, cache)
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in b)
    z = dx.netvlad_packed_bwd(dp, cache, np.zeros_like(cache["h6"]))
    assert set(z) == set(b) and all(np.array_equal(z[k], b[k]) for k in b)
    d = dx.netvlad_packed_bwd(dp, cache, rng.standard_normal(cache["h6"].shape))        # a gradient on h6 reaches everything below it
    assert all(np.array_equal(d[k], b[k]) for k in b if k.startswith("classifier/"))
    assert not any(np.array_equal(d[k], b[k]) for k in b if not k.startswith("classifier/"))


def test_eval_forward_is_the_packed_forward_on_given_statistics():
    rng, teacher, M, _, x, n, y = _setup(11, [12, 0, 5, 7, 17])
    pred, cache = px.netvlad_packed_fwd(x, n, 2, teacher)
    own = {}
    for s, key in (("input_bn", "c_in"), ("cluster_bn", "c_cl"), ("hidden1_bn", "c_h")):
        own[s + "/moving_mean"], own[s + "/moving_variance"] = cache[key][3], cache[key][4]
    pe, he, _ = dx.netvlad_packed_eval_fwd(x, n, 2, teacher, own)
    assert np.abs(pe - pred).max() < 1e-12 and np.abs(he - cache["h6"]).max() < 1e-12
    assert np.abs(dx.netvlad_packed_eval_fwd(x, n, 2, teacher, M)[0] - pred).max() > 1e-6        # other statistics: another function


def test_teacher_every_n_from_checkpoint_metadata():
    from efficientvideoclassification_youtube8m_amd.train import netvlad_teacher_every_n as f
    assert f({"global_step": 4}) == 1                                                  # a sampled tower's checkpoint: every real frame
    assert f({"netvlad_frames": "sampled", "every_n": 10}) == 1
    assert f({"nextvlad_frames": "grid", "every_n": 10}) == 1                          # (the other family's key is not read)
    assert f({"netvlad_frames": "grid", "every_n": 1}) == 1
    assert f({"netvlad_frames": "grid", "every_n": 5}) == 5
    # a distillation checkpoint: every_n is its student's, model/* is the frozen teacher and runs on teacher_every_n (resume)
    assert f({"netvlad_frames": "grid", "every_n": 10, "teacher_every_n": 2, "distill_losses": "rep,pred,ce"}) == 2


def _host_checkpoint(path, scopes=("model",), F=128, V=None, K=64, H=64, Mx=2, meta=(), step=3):
    """A NetVLAD checkpoint written on the host with the names and TF layouts of NetVladTower.state_dict()."""
    from efficientvideoclassification_youtube8m_amd import train
    from efficientvideoclassification_youtube8m_amd.towers import NetVladTower
    V = train.NUM_CLASSES if V is None else V
    sd = {"global_step": step}
    sd.update(meta)
    for scope in scopes:
        for k, shp in NetVladTower.checkpoint_shapes(F, V, K, H, Mx).items():
            sd["%s/%s" % (scope, k)] = torch.zeros(shp)
    path.mkdir(exist_ok=True)
    torch.save(sd, str(path / ("model.ckpt-%d.pt" % step)))
    return sd


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


SIZES = dict(feature_size=128, vocab_size=10, cluster_size=64, hidden_size=64)


def test_graph_refusals_touch_no_device(no_device):
    from efficientvideoclassification_youtube8m_amd.distill import NetVladDistillGraph
    kw = dict(SIZES, max_frames=300, device="cuda:0")
    with pytest.raises(ValueError, match="not data parallel.*2 ranks"):
        NetVladDistillGraph(8, process_group=_TwoRanks(), **kw)
    with pytest.raises(ValueError, match="CrossEntropyLoss built into its loss section.*HingeLoss"):
        NetVladDistillGraph(8, label_loss="HingeLoss", **kw)
    with pytest.raises(ValueError, match="precision 'high' is refused"):
        NetVladDistillGraph(8, precision="high", **kw)
    for bad in (0, 301):
        with pytest.raises(ValueError, match="--every_n %d" % bad):
            NetVladDistillGraph(8, every_n=bad, **kw)
        with pytest.raises(ValueError, match="--every_n %d" % bad):
            NetVladDistillGraph(8, every_n=10, teacher_every_n=bad, **kw)
    with pytest.raises(ValueError, match="distill_losses"):
        NetVladDistillGraph(8, distill_losses="rep,kl", **kw)


def test_eval_graph_refusals_touch_no_device(no_device):
    from efficientvideoclassification_youtube8m_amd.distill import NetVladEvalGraph
    kw = dict(SIZES, max_frames=300, device="cuda:0")
    with pytest.raises(ValueError, match="tower 'pupil'"):
        NetVladEvalGraph(8, tower="pupil", **kw)
    with pytest.raises(ValueError, match="--every_n 301"):
        NetVladEvalGraph(8, tower="both", every_n=10, teacher_every_n=301, **kw)
    with pytest.raises(ValueError, match="--every_n 0"):
        NetVladEvalGraph(8, tower="student", every_n=0, **kw)


def test_flag_refusals_touch_no_device(no_device, monkeypatch, tmp_path):
    """train.main: every refused combination of --teacher_dir with --model NetVLADModel is a ValueError naming the flags, and the
    teacher's checkpoint is read and checked against the size flags on the host."""
    from efficientvideoclassification_youtube8m_amd import train
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    tdir = str(tmp_path / "teacher") + "/"
    common = ["--train_data_pattern", "synthetic", "--frame_features", "True", "--feature_names", "rgb, audio", "--feature_sizes", "64, 64",
              "--batch_size", "16", "--start_new_model", "True", "--train_dir", str(tmp_path) + "/", "--model", "NetVLADModel",
              "--netvlad_frames", "grid", "--every_n", "10", "--netvlad_cluster_size", "64", "--netvlad_hidden_size", "64"]

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
    main(["--teacher_dir", tdir], r"--teacher_dir .* with --model NetVLADModel and --netvlad_frames sampled", argv=sampled)
    main(["--teacher_dir", tdir, "--serial_student_dirs", "%s,%s" % (tmp_path / "a", tmp_path / "b")],
         r"--serial_student_dirs.*HierarchicalLstmModel, not NetVLADModel")
    main(["--teacher_dirs", "%s,%s" % (tmp_path / "a", tmp_path / "b")], r"--teacher_dirs.*HierarchicalLstmModel, not --model NetVLADModel")
    main(["--teacher_preds_pattern", str(tmp_path / "*.csv"), "--train_data_pattern", str(tmp_path / "*.tfrecord")],
         r"--teacher_preds_pattern.*HierarchicalLstmModel, not --model NetVLADModel")
    main(["--teacher_dir", tdir, "--teacher_only", "True"], r"--teacher_dir .* with --teacher_only")
    main(["--teacher_dir", tdir], r"--teacher_dir .* with --finetune", finetune=True)
    main(["--teacher_dir", tdir], r"2 ranks", env=("WORLD_SIZE", "2"))
    main(["--teacher_dir", tdir, "--label_loss", "HingeLoss"], r"--label_loss HingeLoss with --teacher_dir")
    main(["--teacher_dir", tdir, "--precision", "high"], r"--netvlad_frames grid.*--precision high")
    main(["--teacher_dir", tdir, "--every_n", "301"], r"--every_n 301.*--max_num_frames 300")
    main(["--teacher_dir", tdir], r"--teacher_dir .*: no model.ckpt-\*.pt checkpoint there")          # an empty teacher directory
    # a teacher of other sizes: the variable and both shapes are named; a checkpoint without model/*; one of another family
    _host_checkpoint(tmp_path / "teacher", meta={"netvlad_frames": "grid", "every_n": 1}.items())
    main(["--teacher_dir", tdir, "--netvlad_hidden_size", "128"],
         r"model/hidden1_weights of --teacher_dir .*model.ckpt-3.pt has shape \(8192, 64\), the size flags.*\(8192, 128\)")
    main(["--teacher_dir", tdir, "--netvlad_cluster_size", "128"], r"model/cluster_weights of .* has shape \(128, 64\).*\(128, 128\)")
    nomodel = tmp_path / "nomodel"
    nomodel.mkdir()
    torch.save({"global_step": 1}, str(nomodel / "model.ckpt-1.pt"))
    main(["--teacher_dir", str(nomodel) + "/"], r"holds no model/\* variables")
    torch.save({"global_step": 1, "model/expansion_weights": torch.zeros(4, 4)}, str(nomodel / "model.ckpt-1.pt"))
    main(["--teacher_dir", str(nomodel) + "/"], r"holds no variable model/input_bn/beta \(not a NetVLADModel checkpoint\)")
    # the remaining models keep their refusal, in its old words
    FLAGS.reset()
    FLAGS.parse(["--teacher_dir", tdir, "--model", "DbofModel"])
    try:
        from efficientvideoclassification_youtube8m_amd import frame_level_models, losses
        with pytest.raises(ValueError, match="built for HierarchicalLstmModel and NeXtVLADModel, not DbofModel"):
            train.build_graph(frame_level_models.DbofModel(), losses.CrossEntropyLoss(), 128, 16, 10, "cuda:0")
    finally:
        FLAGS.reset()


def test_distill_source_reads_the_teachers_grid_on_the_host(no_device, tmp_path):
    from efficientvideoclassification_youtube8m_amd import train
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    for name, meta, want in (("sampled", {}, 1), ("grid", {"netvlad_frames": "grid", "every_n": 5}, 5),
                             ("distill", {"netvlad_frames": "grid", "every_n": 10, "teacher_every_n": 2}, 2)):
        _host_checkpoint(tmp_path / name, V=train.NUM_CLASSES, meta=meta.items())
        FLAGS.reset()
        try:
            FLAGS.parse(["--teacher_dir", str(tmp_path / name) + "/", "--train_dir", str(tmp_path / "new") + "/", "--model", "NetVLADModel",
                         "--netvlad_frames", "grid", "--netvlad_cluster_size", "64", "--netvlad_hidden_size", "64"])
            assert train.check_netvlad_distill_flags() is True
            src = train.netvlad_distill_source(128)
            assert src["teacher_every_n"] == want and src["resume"] is False and src["ck"].endswith("model.ckpt-3.pt")
            FLAGS.parse(["--model", "NeXtVLADModel"])
            assert train.check_netvlad_distill_flags() is False
        finally:
            FLAGS.reset()


def test_validate_source_picks_the_towers_from_the_checkpoint(no_device, tmp_path):
    """validate.netvlad_source: 'both' for a checkpoint with model_student/* (the student at the recorded every_n, the teacher at the
    recorded teacher_every_n; --netvlad_serve_every_n moves the served grid only), 'teacher' for a single-tower one; model_student/* of
    other sizes is refused on the host with the variable and both shapes."""
    from efficientvideoclassification_youtube8m_amd import train, validate
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    reader = types.SimpleNamespace(feature_sizes=[64, 64], num_classes=train.NUM_CLASSES)
    meta = {"netvlad_frames": "grid", "every_n": 10, "teacher_every_n": 2, "distill_mode": "serial", "distill_losses": "rep,pred,ce"}
    _host_checkpoint(tmp_path / "distill", scopes=("model", "model_student"), meta=meta.items())
    _host_checkpoint(tmp_path / "single", meta={"netvlad_frames": "grid", "every_n": 5}.items())
    flags = ["--model", "NetVLADModel", "--netvlad_cluster_size", "64", "--netvlad_hidden_size", "64"]
    try:
        FLAGS.reset()
        FLAGS.parse(flags + ["--train_dir", str(tmp_path / "distill") + "/"])
        src = validate.netvlad_source(reader)
        assert (src["tower"], src["every_n"], src["teacher_every_n"]) == ("both", 10, 2)
        FLAGS.parse(["--netvlad_serve_every_n", "30"])
        src = validate.netvlad_source(reader)
        assert (src["tower"], src["every_n"], src["teacher_every_n"]) == ("both", 30, 2)
        FLAGS.reset()
        FLAGS.parse(flags + ["--train_dir", str(tmp_path / "single") + "/"])
        src = validate.netvlad_source(reader)
        assert (src["tower"], src["every_n"], src["teacher_every_n"]) == ("teacher", 5, 1)
        bad = torch.load(str(tmp_path / "distill" / "model.ckpt-3.pt"))
        bad["model_student/hidden1_bn/gamma"] = torch.zeros(128)
        (tmp_path / "bad").mkdir()
        torch.save(bad, str(tmp_path / "bad" / "model.ckpt-3.pt"))
        FLAGS.reset()
        FLAGS.parse(flags + ["--train_dir", str(tmp_path / "bad") + "/"])
        with pytest.raises(ValueError, match=r"model_student/hidden1_bn/gamma of .* has shape \(128,\), the size flags.*\(64,\)"):
            validate.netvlad_source(reader)
    finally:
        FLAGS.reset()


def test_tower_dstate_shape_is_checked_before_any_launch(no_device):
    """NetVladTower.backward(dstate=...) of a wrong shape: a ValueError naming both shapes (checked on a bare object: no device)."""
    from efficientvideoclassification_youtube8m_amd.towers import NetVladTower
    tw = object.__new__(NetVladTower)
    tw.training, tw._taped, tw.frames = True, True, "grid"
    tw.B, tw.F, tw.S, tw.Kc, tw.Hd, tw.R, tw.Rp = 4, 8, 30, 64, 64, 10, 32
    tw.store, tw.bn_in = None, None
    with pytest.raises(ValueError, match=r"dstate \(4, 32\): the state of this tower is \(4, 64\)"):
        tw.backward(None, dstate=torch.zeros(4, 32))
