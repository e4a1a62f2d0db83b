"""The NetVLAD context gate (--netvlad_gating) on the CPU: the float64 restatement tests/_netvlad_gating_ref.py against
central differences, the ungated case against the older references, an f32 evaluation of the device entries' expressions, three planted
faults against the bounds the GPU tests apply, the shape sets and metadata keys, what validate reads from gated / ungated / mixed
checkpoints, and every refusal - all without a device."""
import logging
import types

import numpy as np
import pytest
import torch

import _netvlad_distill_ref as dx
import _netvlad_gating_ref as gx
import _netvlad_packed_ref as px
from oracle import model_math as mm

EPS = 1e-6                                       # the parameter step of the central differences
NEW = ("gating_weights", "gating_bn/beta", "gating_bn/gamma", "gating_bn/moving_mean", "gating_bn/moving_variance")


def _setup(seed, n, gate=(False, True), T=12, F=8, K=3, H=8, V=6):
    """test_cpu_netvlad_distill.py's sizes: a teacher and a student (gate: which of the two has the context gate) with perturbed
    batch-norm scales / offsets, and moving statistics of the teacher that are not its initial ones."""
    rng = np.random.default_rng(seed)
    towers = []
    for gated in gate:
        P = mm.init_netvlad_params(rng, F, K, H, V)
        if gated:
            gx.add_gate_params(P, rng, H)
        for k in P:
            if k.endswith("gamma") or k.endswith("beta"):
                P[k] = P[k] + 0.2 * rng.standard_normal(P[k].shape)
        towers.append(P)
    M = {}
    for s, C in (("input_bn", F), ("cluster_bn", K), ("hidden1_bn", H), ("gating_bn", H)):
        M[s + "/moving_mean"] = 0.2 * rng.standard_normal(C)
        M[s + "/moving_variance"] = np.exp(0.2 * rng.standard_normal(C))
    x = rng.standard_normal((len(n), T, F))
    y = rng.random((len(n), V)) > 0.6
    return rng, towers[0], M, towers[1], x, np.asarray(n), y


GRID = [12, 0, 2, 5, 7, 17]                      # every_n = 3, T = 12: a video of T frames, an empty one, one shorter than every_n, one past T


@pytest.mark.parametrize("case,gate,on", [("ce alone, gated", (False, True), ("ce",)),
                                          ("gated student, ungated teacher", (False, True), ("rep", "pred", "ce")),
                                          ("ungated student, gated teacher", (True, False), ("rep", "pred", "ce"))])
def test_gradients_match_central_differences(case, gate, on):
    """Central differences of L_CE, and of g_rep L_REP + L_PRED + L_CE, on every student parameter tensor (the gate's three trainable
    ones included where the student has them), several random entries each.  No hidden1_bn pre-activation lies within ten steps of 0
    or 6, and both sides of the relu6 mask occur."""
    rng, teacher, M, student, x, n, y = _setup(4, GRID, gate)

    def loss(Q):
        return gx.distill_step(x, n, y, teacher, M, Q, 1, 3, on=on, with_grads=False)["total"]

    ref = gx.distill_step(x, n, y, teacher, M, student, 1, 3, on=on)
    assert list(ref["teacher_cache"]["k"]) == [12, 0, 2, 5, 7, 12] and list(ref["student_cache"]["k"]) == [4, 0, 1, 2, 3, 4]
    hb = ref["student_cache"]["hid_bn"]
    assert min(np.abs(hb).min(), np.abs(hb - 6).min()) > 10 * EPS
    assert ((hb > 0) & (hb < 6)).any() and not ((hb > 0) & (hb < 6)).all()
    assert bool(ref["dstate"].any()) == ("rep" in on)
    assert ("g" in ref["student_cache"]) == gate[1] and ("g" in ref["teacher_cache"]) == gate[0]
    grads = ref["student_grads"]
    assert set(grads) == set(student) and all(k in grads for k in gx.GATE_NAMES) == gate[1]
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
            assert abs(fd - got) <= 1e-5 * max(1.0, abs(fd)) + 1e-7, (case, k, j, fd, got)


def test_without_the_gate_it_is_the_existing_reference():
    rng, teacher, M, student, x, n, y = _setup(3, [9, 0, 4, 12], gate=(False, False))
    pred, cache = px.netvlad_packed_fwd(x, n, 3, student)
    gp, gc = gx.fwd(x, n, 3, student)
    assert np.array_equal(gp, pred) and np.array_equal(gc["state"], cache["h6"])
    dp, ds = mm.cross_entropy_grad(pred, y), rng.standard_normal(cache["h6"].shape)
    for dstate in (None, ds):
        a, b = gx.bwd(dp, gc, dstate), dx.netvlad_packed_bwd(dp, cache, dstate)
        assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in b)
    a = gx.distill_step(x, n, y, teacher, M, student, 1, 3)
    b = dx.distill_step(x, n, y, teacher, M, student, 1, 3)
    assert a["total"] == b["total"] and all(np.array_equal(a["student_grads"][k], b["student_grads"][k]) for k in b["student_grads"])


def test_the_gate_is_behind_the_aggregation_and_moves_the_state():
    """A gated tower's h6 is the ungated tower's; its state and predictions are not; a gradient on the state reaches the gate."""
    rng, _, M, student, x, n, y = _setup(5, [9, 0, 4, 12])
    plain = {k: v for k, v in student.items() if k not in gx.GATE_NAMES}
    p0, c0 = gx.fwd(x, n, 3, plain)
    p1, c1 = gx.fwd(x, n, 3, student)
    assert np.array_equal(c0["h6"], c1["h6"]) and np.array_equal(c1["state"], c1["h6"] * c1["g"])
    assert np.abs(p0 - p1).max() > 1e-6 and (c1["g"] > 0).all() and (c1["g"] < 1).all()
    dp = mm.cross_entropy_grad(p1, y)
    a, b = gx.bwd(dp, c1), gx.bwd(dp, c1, rng.standard_normal(c1["h6"].shape))
    assert all(np.array_equal(a[k], b[k]) for k in a if k.startswith("classifier/"))
    assert not any(np.array_equal(a[k], b[k]) for k in a if not k.startswith("classifier/"))
    pe, se, ce = gx.eval_fwd(x, n, 3, student, M)                      # the evaluation forward reads gating_bn's moving statistics
    M2 = dict(M)
    M2["gating_bn/moving_mean"] = M["gating_bn/moving_mean"] + 1.0
    assert np.abs(gx.eval_fwd(x, n, 3, student, M2)[0] - pe).max() > 1e-6


def test_planted_faults_miss_the_tower_bounds():
    """The bound the GPU tests hold every gradient tensor to (relative L2 0.12, or max abs 1e-3) rejects each of three wrong reverse
    modes: 1 - g dropped, dstate added behind the gate instead of in front of it, the path through gating_weights left out."""
    rng, teacher, M, student, x, n, y = _setup(4, GRID)
    good = gx.distill_step(x, n, y, teacher, M, student, 1, 3)["student_grads"]
    for fault in gx.FAULTS:
        bad = gx.distill_step(x, n, y, teacher, M, student, 1, 3, fault=fault)["student_grads"]
        missed = []
        for k in good:
            l2 = np.linalg.norm(bad[k] - good[k]) / (np.linalg.norm(good[k]) + 1e-30)
            mx = np.abs(bad[k] - good[k]).max()
            if not (l2 < 0.12 or mx < 1e-3):
                missed.append(k)
        print(fault, missed)
        assert missed, fault
        assert all(np.array_equal(bad[k], good[k]) for k in good if k.startswith("classifier/"))


def test_f32_evaluation_of_the_entries_expressions():
    """The expressions of evc_bn_gate_fwd / _bwd_partial / _bwd_finalize evaluated in f32 (one rounding per operation) against the float64
    definition, with and without d2, statistics away from (0, 1): out and dh to 1e-6 relative, the batch norm's backward to 1e-4 of the
    largest element (its column sums cancel)."""
    rng = np.random.default_rng(21)
    for (R, C), with_d2 in (((7, 65), True), ((33, 128), False)):
        gl, h = rng.standard_normal((R, C)) * 2.0 + 0.5, rng.random((R, C)) * 6.0
        d, d2 = rng.standard_normal((R, C)) * 0.1, (rng.standard_normal((R, C)) * 0.1 if with_d2 else None)
        gamma, beta = np.exp(0.2 * rng.standard_normal(C)), 0.2 * rng.standard_normal(C)
        f32 = lambda a: None if a is None else a.astype(np.float32).astype(np.float64)
        gl, h, d, d2, gamma, beta = (f32(a) for a in (gl, h, d, d2, gamma, beta))
        gn, cg = mm.batch_norm_train_fwd(gl, gamma, beta)
        mean, var = f32(cg[3]), f32(cg[4])
        gn = (gl - mean) / np.sqrt(var + 1e-3) * gamma + beta
        g = gx.sigmoid(gn)
        e = d if d2 is None else d + d2
        dgn = e * h * g * (1 - g)
        xh = (gl - mean) / np.sqrt(var + 1e-3)
        want = dict(out=h * g, dh=e * g, dbeta=dgn.sum(0), dgamma=(dgn * xh).sum(0))
        want["dgl"] = gamma / np.sqrt(var + 1e-3) * (dgn - want["dbeta"] / R - xh * want["dgamma"] / R)
        got = gx.gate_f32(gl, h, d, d2, mean, var, gamma, beta)
        for k, tol in (("out", 1e-6), ("dh", 1e-6), ("dgl", 1e-4), ("dgamma", 1e-4), ("dbeta", 1e-4)):
            err = np.abs(got[k].astype(np.float64) - want[k]).max() / np.abs(want[k]).max()
            assert got[k].dtype == np.float32 and err < tol, (k, err)


# ---------------------------------------------------------------------------- shapes, metadata, refusals
def test_checkpoint_shapes_with_and_without_the_keyword():
    from efficientvideoclassification_youtube8m_amd.towers import NetVladTower
    sizes = (128, 10, 64, 192, 2)
    plain, gated = NetVladTower.checkpoint_shapes(*sizes), NetVladTower.checkpoint_shapes(*sizes, gating=True)
    assert plain == NetVladTower.checkpoint_shapes(*sizes, gating=False) and not any(k in plain for k in NEW)
    assert [k for k in gated if k not in plain] == ["gating_weights", "gating_bn/beta", "gating_bn/gamma", "gating_bn/moving_mean",
                                                    "gating_bn/moving_variance"]
    assert gated["gating_weights"] == (192, 192) and all(gated[k] == (192,) for k in NEW[1:])
    assert all(gated[k] == plain[k] for k in plain)
    names = list(NetVladTower.variable_shapes(*sizes, gating=True))
    assert names.index("gating_weights") == names.index("hidden1_bn/gamma") + 1        # after hidden1_bn/*, in front of the head
    assert names.index("gating_bn/gamma") + 1 == names.index("classifier/gates/weights")
    assert list(NetVladTower.variable_shapes(*sizes)) == [k for k in names if not k.startswith("gating")]


def test_metadata_keys_only_when_true():
    from efficientvideoclassification_youtube8m_amd import train
    from efficientvideoclassification_youtube8m_amd.distill import NetVladDistillGraph
    from efficientvideoclassification_youtube8m_amd.towers import NetVladTower
    tw = object.__new__(NetVladTower)
    for gating, want in ((False, {}), (True, {"netvlad_gating": True})):
        tw.gating = gating
        assert train.netvlad_gating_metadata(types.SimpleNamespace(tower=tw)) == want
    g = object.__new__(NetVladDistillGraph)
    for s, t, want in ((False, False, {}), (True, False, {"netvlad_gating": True}), (False, True, {"teacher_netvlad_gating": True}),
                       (True, True, {"netvlad_gating": True, "teacher_netvlad_gating": True})):
        g.gating, g.teacher_gating = s, t
        assert train.netvlad_gating_metadata(g) == want
    assert train.netvlad_gating_metadata(types.SimpleNamespace(tower=object())) == {}


def _host_checkpoint(path, scopes=(("model", False),), F=128, V=None, K=64, H=64, Mx=2, meta=(), step=3):
    """A NetVLAD checkpoint written on the host with the names and TF layouts of NetVladTower.state_dict(); scopes: (name, gated)."""
    from efficientvideoclassification_youtube8m_amd import train
    from efficientvideoclassification_youtube8m_amd.towers import NetVladTower
    V = train.NUM_CLASSES if V is None else V
    sd = {"global_step": step}
    sd.update(meta)
    for scope, gated in scopes:
        for k, shp in NetVladTower.checkpoint_shapes(F, V, K, H, Mx, gating=gated).items():
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


def test_check_checkpoint_names_the_flag(no_device, tmp_path):
    from efficientvideoclassification_youtube8m_amd.distill import check_netvlad_checkpoint, netvlad_checkpoint_gating
    plain = _host_checkpoint(tmp_path / "p", V=10)
    gated = _host_checkpoint(tmp_path / "g", scopes=(("model", True),), V=10)
    sizes = (64, 64, 2)
    check_netvlad_checkpoint(plain, "model", 128, 10, sizes)
    check_netvlad_checkpoint(gated, "model", 128, 10, sizes, gating=True)
    assert netvlad_checkpoint_gating(gated, "model") and not netvlad_checkpoint_gating(plain, "model")
    assert not netvlad_checkpoint_gating(gated, "model_student")
    with pytest.raises(ValueError, match=r"--netvlad_gating False, but the checkpoint holds the variable model/gating_weights"):
        check_netvlad_checkpoint(gated, "model", 128, 10, sizes)
    with pytest.raises(ValueError, match=r"--netvlad_gating True, but the checkpoint holds no variable model/gating_weights"):
        check_netvlad_checkpoint(plain, "model", 128, 10, sizes, gating=True)
    bad = dict(gated)
    bad["model/gating_bn/moving_mean"] = torch.zeros(32)
    with pytest.raises(ValueError, match=r"model/gating_bn/moving_mean of the checkpoint has shape \(32,\), the size flags.*\(64,\)"):
        check_netvlad_checkpoint(bad, "model", 128, 10, sizes, gating=True)
    del bad["model/gating_bn/moving_mean"]
    with pytest.raises(ValueError, match=r"holds no variable model/gating_bn/moving_mean"):
        check_netvlad_checkpoint(bad, "model", 128, 10, sizes, gating=True)


def test_more_than_one_rank_is_refused_before_the_device(no_device, monkeypatch):
    from efficientvideoclassification_youtube8m_amd import towers
    towers.check_netvlad_gating(True, 1)
    towers.check_netvlad_gating(False, 8)
    with pytest.raises(ValueError, match=r"--netvlad_gating True refuses a process group of 2 ranks"):
        towers.check_netvlad_gating(True, 2)
    monkeypatch.setattr(torch.distributed, "is_available", lambda: True)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    with pytest.raises(ValueError, match=r"--netvlad_gating True refuses a process group of 2 ranks"):
        towers.NetVladTower(8, 300, 128, 10, 30, 64, 64, 2, device="cuda:0", process_group=object(), gating=True)


def test_flag_refusals_touch_no_device(no_device, monkeypatch, tmp_path):
    """train.main: several ranks; a resume whose checkpoint disagrees with --netvlad_gating (a tower alone and a distillation's student,
    both ways); --student_init_from_teacher with differing gates."""
    from efficientvideoclassification_youtube8m_amd import train
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    common = ["--train_data_pattern", "synthetic", "--frame_features", "True", "--feature_names", "rgb, audio", "--feature_sizes", "64, 64",
              "--batch_size", "16", "--model", "NetVLADModel", "--netvlad_frames", "grid", "--every_n", "10", "--netvlad_cluster_size", "64",
              "--netvlad_hidden_size", "64"]

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

    meta = {"netvlad_frames": "grid", "every_n": 10}
    _host_checkpoint(tmp_path / "plain", meta=meta.items())
    _host_checkpoint(tmp_path / "gated", scopes=(("model", True),), meta=dict(meta, netvlad_gating=True).items())
    dmeta = dict(meta, teacher_every_n=1, distill_mode="serial", distill_losses="rep,pred,ce")
    _host_checkpoint(tmp_path / "d_plain", scopes=(("model", True), ("model_student", False)), meta=dmeta.items())
    _host_checkpoint(tmp_path / "d_gated", scopes=(("model", False), ("model_student", True)), meta=dmeta.items())
    d = lambda name: str(tmp_path / name) + "/"
    sampled = ["--netvlad_frames", "sampled", "--start_new_model", "True", "--train_dir", d("new")]
    main(sampled + ["--netvlad_gating", "True"], r"--netvlad_gating True refuses a process group of 2 ranks", env=("WORLD_SIZE", "2"))
    main(["--train_dir", d("plain"), "--netvlad_gating", "True"], r"--netvlad_gating True, but --train_dir .*model.ckpt-3.pt holds no variable model/gating_weights")
    main(["--train_dir", d("gated")], r"--netvlad_gating False, but --train_dir .*model.ckpt-3.pt holds the variable model/gating_weights")
    main(["--train_dir", d("d_plain"), "--teacher_dir", d("plain"), "--netvlad_gating", "True"],
         r"--netvlad_gating True, but --train_dir .* holds no variable model_student/gating_weights")
    main(["--train_dir", d("d_gated"), "--teacher_dir", d("plain")],
         r"--netvlad_gating False, but --train_dir .* holds the variable model_student/gating_weights")
    new = ["--train_dir", d("new"), "--start_new_model", "True", "--student_init_from_teacher", "True"]
    main(new + ["--teacher_dir", d("plain"), "--netvlad_gating", "True"],
         r"--student_init_from_teacher True with --netvlad_gating True: the teacher of .* was trained without the context gate")
    main(new + ["--teacher_dir", d("gated")],
         r"--student_init_from_teacher True with --netvlad_gating False: the teacher of .* was trained with the context gate")


def test_distill_source_reports_the_teachers_gate(no_device, tmp_path):
    from efficientvideoclassification_youtube8m_amd import train
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    for name, gated in (("plain", False), ("gated", True)):
        _host_checkpoint(tmp_path / name, scopes=(("model", gated),), meta={"netvlad_frames": "grid", "every_n": 1}.items())
        for flag in ("False", "True"):                                 # the student's flag does not enter: the two may differ
            FLAGS.reset()
            try:
                FLAGS.parse(["--teacher_dir", str(tmp_path / name) + "/", "--train_dir", str(tmp_path / "new") + "/", "--model", "NetVLADModel",
                             "--netvlad_frames", "grid", "--netvlad_cluster_size", "64", "--netvlad_hidden_size", "64", "--netvlad_gating", flag])
                src = train.netvlad_distill_source(128)
                assert src["teacher_gating"] is gated and src["resume"] is False and src["teacher_every_n"] == 1
            finally:
                FLAGS.reset()


def test_validate_source_reads_each_scopes_gate_from_the_checkpoint(no_device, tmp_path, caplog):
    """validate.netvlad_source on host-written gated, ungated and mixed distillation checkpoints: every scope's gate from its own
    variables, whatever --netvlad_gating says; a flag that disagrees with the served tower is a warning."""
    from efficientvideoclassification_youtube8m_amd import train, validate
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    reader = types.SimpleNamespace(feature_sizes=[64, 64], num_classes=train.NUM_CLASSES)
    meta = {"netvlad_frames": "grid", "every_n": 10, "teacher_every_n": 2, "distill_mode": "serial", "distill_losses": "rep,pred,ce"}
    cases = {"single_plain": ((("model", False),), "teacher", False, False), "single_gated": ((("model", True),), "teacher", True, True),
             "both_gated": ((("model", True), ("model_student", True)), "both", True, True),
             "student_gated": ((("model", False), ("model_student", True)), "both", True, False),
             "teacher_gated": ((("model", True), ("model_student", False)), "both", False, True),
             "both_plain": ((("model", False), ("model_student", False)), "both", False, False)}
    flags = ["--model", "NetVLADModel", "--netvlad_cluster_size", "64", "--netvlad_hidden_size", "64"]
    try:
        for name, (scopes, tower, gating, teacher_gating) in cases.items():
            _host_checkpoint(tmp_path / name, scopes=scopes, meta=meta.items())
            for flag in (False, True):
                FLAGS.reset()
                FLAGS.parse(flags + ["--train_dir", str(tmp_path / name) + "/", "--netvlad_gating", str(flag)])
                caplog.clear()
                with caplog.at_level(logging.WARNING):
                    src = validate.netvlad_source(reader)
                assert (src["tower"], src["gating"], src["teacher_gating"]) == (tower, gating, teacher_gating), name
                warned = any("--netvlad_gating" in r.getMessage() for r in caplog.records)
                assert warned == (flag != gating), (name, flag)
        bad = torch.load(str(tmp_path / "both_gated" / "model.ckpt-3.pt"))
        bad["model_student/gating_bn/gamma"] = torch.zeros(128)
        (tmp_path / "bad").mkdir()
        torch.save(bad, str(tmp_path / "bad" / "model.ckpt-3.pt"))
        FLAGS.reset()
        FLAGS.parse(flags + ["--train_dir", str(tmp_path / "bad") + "/"])
        with pytest.raises(ValueError, match=r"model_student/gating_bn/gamma of .* has shape \(128,\), the size flags.*\(64,\)"):
            validate.netvlad_source(reader)
    finally:
        FLAGS.reset()


def test_graphs_take_the_gates_and_still_refuse_on_the_host(no_device):
    """The keyword does not move a refusal behind the device: the graphs' older refusals with gating given."""
    from efficientvideoclassification_youtube8m_amd.distill import NetVladDistillGraph, NetVladEvalGraph
    kw = dict(feature_size=128, vocab_size=10, cluster_size=64, hidden_size=64, max_frames=300, device="cuda:0")
    with pytest.raises(ValueError, match="--every_n 301"):
        NetVladDistillGraph(8, every_n=301, gating=True, teacher_gating=False, **kw)
    with pytest.raises(ValueError, match="--every_n 0"):
        NetVladEvalGraph(8, tower="student", every_n=0, gating=True, **kw)
