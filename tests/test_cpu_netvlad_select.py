"""NetVLAD grid towers on the frames a --student_sampling word selects, on the CPU: ops.SelectPlan's counts and packed
layout against tests/_frame_select_ref.py for every frame count, the flag surface of train / validate without a device (checkpoint
metadata, the warning of a sampled tower, the tables' limit on T, NeXtVLAD's unchanged refusals), and the float64 restatement -
tests/_netvlad_packed_ref.netvlad_packed_fwd fed the table's rows - against central differences."""
import logging
import types

import numpy as np
import pytest
import torch

import _frame_select_ref as fs
import _netvlad_packed_ref as nv
from oracle import model_math as mm

SHAPES = [(300, 1), (300, 7), (300, 10), (300, 30), (60, 10)]
WORDS = ("first", "middle", "last", "first_middle_last", "random")


def table_frames(n, T, every_n, word, seed=0, draw=0, row0=0):
    """The per-video frame lists of a word, from the reference table: the entries >= 0 of each row, in the row's order."""
    src = fs.table(n, T, every_n, word, seed, draw, row0)
    return [row[row >= 0].astype(np.int64) for row in src]


@pytest.mark.parametrize("T,every_n", SHAPES)
def test_plan_counts_are_the_tables_counts(T, every_n):
    """For every n in 0 .. T (and one below 0, one beyond T: clipped): k_b = student_count(n, T, T // every_n), and every row of the
    reference table holds exactly k_b entries >= 0, ascending, in its first k_b slots.  One fewer than the grid's ceil(n / every_n) for
    some n, never more; 0 for every video shorter than every_n."""
    from efficientvideoclassification_youtube8m_amd import ops
    n = np.concatenate([np.arange(T + 1), [-3, T + 5]]).astype(np.int32)
    S = T // every_n
    plan = ops.SelectPlan(n, every_n, T)
    want = np.array([fs.student_count(min(max(int(v), 0), T), T, S) for v in n], np.int32)
    assert plan.k.dtype == np.int32 and np.array_equal(plan.k, want) and plan.S == S and plan.B == n.size and plan.every_n == every_n
    grid = ops.GridPlan(n, every_n, T)
    # ceil(n / e) - trunc(n S / T) < 1 + 1 + n (T - e S) / (e T): at most one fewer where every_n divides T, two where it does not
    assert (plan.k <= grid.k).all() and (grid.k - plan.k <= (1 if T % every_n == 0 else 2)).all() and plan.k.max() <= S
    assert (grid.k - plan.k == 1).any()                                # (documented: the truncation loses a frame for some n)
    assert not plan.k[:every_n].any()                                  # n < every_n: no frame
    assert plan.B * S <= ops.grid_capacity(plan.B, T, every_n)
    for word in WORDS:
        src = fs.table(n, T, every_n, word, seed=3, draw=2, row0=0)
        assert src.shape == (n.size, S)
        for b in range(n.size):
            k = int(plan.k[b])
            row = src[b]
            assert (row[:k] >= 0).all() and (row[k:] == -1).all(), (word, b)
            assert (np.diff(row[:k]) > 0).all() and (k == 0 or row[k - 1] < min(max(int(n[b]), 0), T)), (word, b)


@pytest.mark.parametrize("T,every_n", SHAPES)
def test_plan_layout_follows_the_counts(T, every_n):
    from efficientvideoclassification_youtube8m_amd import ops
    rng = np.random.default_rng(T + every_n)
    n = rng.integers(0, T + 1, size=37).astype(np.int32)
    n[0], n[-1], n[5] = 0, 0, T
    plan = ops.SelectPlan(n, every_n, T)
    k = np.array([fs.student_count(int(v), T, T // every_n) for v in n], np.int64)
    assert plan.row_off.dtype == np.int32 and plan.row_off.shape == (38,)
    assert np.array_equal(plan.row_off, np.concatenate([[0], np.cumsum(k)]))
    assert plan.R == int(k.sum()) and plan.Rp == (plan.R + 31) // 32 * 32 and 0 <= plan.Rp - plan.R < 32 and plan.max_k == int(k.max())
    empty = ops.SelectPlan(np.zeros(4, np.int32), every_n, T)
    assert (empty.R, empty.Rp, empty.max_k) == (0, 0, 0) and not empty.row_off.any()
    with pytest.raises(ValueError, match="every_n=0"):
        ops.SelectPlan(n, 0, T)
    with pytest.raises(ValueError, match="max_num_frames=1025.*at most 1024"):
        ops.SelectPlan(n, 10, 1025)


@pytest.fixture
def no_device(monkeypatch):
    from efficientvideoclassification_youtube8m_amd import ops

    def touched(*a, **k):
        raise AssertionError("the device was touched before the flags were checked")
    monkeypatch.setattr(torch.cuda, "set_device", touched)
    monkeypatch.setattr(torch.cuda, "_lazy_init", touched)
    monkeypatch.setattr(ops, "check_device", touched)


def _bare_tower(sampling, seed=0, frames="grid"):
    from efficientvideoclassification_youtube8m_amd.towers import NetVladTower
    tw = object.__new__(NetVladTower)
    tw.frames, tw.every_n, tw.sampling, tw.sampling_seed = frames, 10, sampling, seed
    return tw


def test_checkpoint_metadata(no_device):
    """train.netvlad_sampling_metadata: the word of a tower trained alone, the seed under random alone, nothing for uniform; for a
    distillation graph the seed and the teacher's word (the student's word is recorded with every graph's student_sampling); and
    train.netvlad_teacher_sampling reads both kinds of checkpoint back."""
    from efficientvideoclassification_youtube8m_amd import train
    from efficientvideoclassification_youtube8m_amd.distill import NetVladDistillGraph
    meta = lambda w, s=0: train.netvlad_sampling_metadata(types.SimpleNamespace(tower=_bare_tower(w, s)))
    assert meta("last") == {"student_sampling": "last"}
    assert meta("segment_change", 5) == {"student_sampling": "segment_change"}
    assert meta("random", 5) == {"student_sampling": "random", "student_sampling_seed": 5}
    assert meta("uniform", 5) == {}
    assert train.netvlad_sampling_metadata(types.SimpleNamespace(tower=object())) == {}

    def distill(word, seed, t_word, t_seed):
        g = object.__new__(NetVladDistillGraph)
        g.student_sampling, g.sampling_seed, g.teacher_sampling, g.teacher_sampling_seed = word, seed, t_word, t_seed
        return train.netvlad_sampling_metadata(g)
    assert distill("uniform", 4, "uniform", 0) == {}
    assert distill("last", 4, "uniform", 0) == {}
    assert distill("random", 4, "uniform", 0) == {"student_sampling_seed": 4}
    assert distill("last", 0, "first", 9) == {"teacher_sampling": "first"}
    assert distill("uniform", 0, "random", 9) == {"teacher_sampling": "random", "teacher_sampling_seed": 9}
    f = train.netvlad_teacher_sampling
    assert f({"global_step": 3}) == ("uniform", 0)
    assert f({"netvlad_frames": "grid", "every_n": 10}) == ("uniform", 0)
    assert f({"netvlad_frames": "grid", "every_n": 10, "student_sampling": "last"}) == ("last", 0)
    assert f({"netvlad_frames": "grid", "every_n": 10, "student_sampling": "random", "student_sampling_seed": 6}) == ("random", 6)
    # a distillation checkpoint: student_sampling is its student's, model/* runs on the recorded teacher_sampling
    assert f({"netvlad_frames": "grid", "every_n": 10, "teacher_every_n": 1, "student_sampling": "last"}) == ("uniform", 0)
    assert f({"netvlad_frames": "grid", "every_n": 10, "teacher_every_n": 2, "student_sampling": "last", "teacher_sampling": "first"}) == ("first", 0)


def test_sampled_tower_with_a_word_warns_and_keeps_running(no_device, caplog):
    """--netvlad_frames sampled --student_sampling last: no error; the tower is built with "uniform" and one warning names both flags."""
    from efficientvideoclassification_youtube8m_amd import train
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    from efficientvideoclassification_youtube8m_amd.towers import check_netvlad_frames
    try:
        FLAGS.reset()
        FLAGS.parse(["--model", "NetVLADModel", "--netvlad_frames", "sampled", "--student_sampling", "last"])
        with caplog.at_level(logging.WARNING):
            assert train.netvlad_sampling_word() == "uniform"
            assert not caplog.records                                  # (the quiet form, for the host checks)
            assert train.netvlad_sampling_word(warn=True) == "uniform"
        msgs = [r.getMessage() for r in caplog.records]
        assert len(msgs) == 1 and "--student_sampling last" in msgs[0] and "--netvlad_frames sampled" in msgs[0]
        check_netvlad_frames("sampled", 10, 300, model="NetVLADModel", sampling=train.netvlad_sampling_word())
        FLAGS.parse(["--netvlad_frames", "grid"])
        assert train.netvlad_sampling_word(warn=True) == "last" and len(caplog.records) == 1
        FLAGS.parse(["--model", "NeXtVLADModel"])
        assert train.netvlad_sampling_word(warn=True) == "uniform" and len(caplog.records) == 1
    finally:
        FLAGS.reset()
    # the tower itself refuses what the command line never hands it
    with pytest.raises(ValueError, match="--student_sampling last selects among the rows of --netvlad_frames grid"):
        check_netvlad_frames("sampled", 10, 300, sampling="last")
    with pytest.raises(ValueError, match="--student_sampling: 'latest'"):
        check_netvlad_frames("grid", 10, 300, sampling="latest")


def test_refusals_touch_no_device(no_device, tmp_path):
    """T > 1024 under a word is refused on the host by train.main, the graphs and the tower; at "uniform" it is not the word's business.
    NeXtVLAD keeps its refusals in their words."""
    from efficientvideoclassification_youtube8m_amd import inference, train
    from efficientvideoclassification_youtube8m_amd.distill import NetVladDistillGraph, NetVladEvalGraph, NeXtVladEvalGraph
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    from efficientvideoclassification_youtube8m_amd.towers import NetVladTower, check_netvlad_frames
    common = ["--train_data_pattern", "synthetic", "--frame_features", "True", "--feature_names", "rgb, audio", "--feature_sizes", "64, 64",
              "--batch_size", "16", "--start_new_model", "True", "--train_dir", str(tmp_path) + "/", "--model", "NetVLADModel",
              "--netvlad_frames", "grid", "--every_n", "10", "--netvlad_cluster_size", "64", "--netvlad_hidden_size", "64"]
    try:
        FLAGS.reset()
        with pytest.raises(ValueError, match=r"--student_sampling last: --max_num_frames 1030 is refused.*at most 1024"):
            train.main(common + ["--student_sampling", "last", "--max_num_frames", "1030"])
        FLAGS.reset()
        with pytest.raises(ValueError, match=r"--student_sampling: 'latest'"):
            train.main(common + ["--student_sampling", "latest"])
    finally:
        FLAGS.reset()
    check_netvlad_frames("grid", 10, 1030)                             # uniform: as before
    check_netvlad_frames("grid", 10, 1024, sampling="random")
    kw = dict(feature_size=128, vocab_size=10, cluster_size=64, hidden_size=64, device="cuda:0")
    with pytest.raises(ValueError, match="--max_num_frames 1030 is refused"):
        NetVladTower(8, max_frames=1030, frames="grid", every_n=10, sampling="last", **kw)
    with pytest.raises(ValueError, match="--max_num_frames 1030 is refused"):
        NetVladDistillGraph(8, max_frames=1030, student_sampling="segment_change", **kw)
    with pytest.raises(ValueError, match="--max_num_frames 1030 is refused"):
        NetVladDistillGraph(8, max_frames=1030, teacher_sampling="first", **kw)
    with pytest.raises(ValueError, match="--max_num_frames 1030 is refused"):
        NetVladEvalGraph(8, max_frames=1030, student_sampling="last", **kw)
    with pytest.raises(ValueError, match="--student_sampling: 'latest'"):
        NetVladEvalGraph(8, student_sampling="latest", **kw)
    # NeXtVLAD: the words stay unbuilt
    with pytest.raises(ValueError, match="--student_sampling last with --model NeXtVLADModel.*not built for this family"):
        NeXtVladEvalGraph(8, student_sampling="last", device="cuda:0")
    try:
        FLAGS.reset()
        FLAGS.parse(["--model", "NeXtVLADModel", "--student_sampling", "last"])
        with pytest.raises(ValueError, match="--student_sampling last with --model NeXtVLADModel"):
            inference.check_nextvlad_serving_flags()
    finally:
        FLAGS.reset()


def test_selected_ref_backward_matches_finite_differences():
    """The float64 restatement of a selected tower - netvlad_packed_fwd(frames = the table's rows) - in reverse mode against central
    differences under "last" at every_n = 3, T = 12: one video without a frame, one shorter than every_n (k = 0 too), one of T frames,
    ragged ones between.  The rows are the LAST k_b frames of each video, not the grid's."""
    T, every_n = 12, 3
    n = np.array([12, 0, 2, 5, 7, 11])
    rng = np.random.default_rng(5)
    P = mm.init_netvlad_params(rng, 8, 3, 8, 6)
    for k in P:
        if k.endswith("gamma") or k.endswith("beta"):
            P[k] = P[k] + 0.2 * rng.standard_normal(P[k].shape)
    x = rng.standard_normal((len(n), T, 8))
    y = rng.random((len(n), 6)) > 0.6
    frames = table_frames(n, T, every_n, "last")
    assert [list(f) for f in frames] == [[8, 9, 10, 11], [], [], [4], [5, 6], [8, 9, 10]]

    def loss(Q):
        p, _ = nv.netvlad_packed_fwd(x, n, every_n, Q, frames=frames)
        return mm.cross_entropy_loss(p, y)

    pred, cache = nv.netvlad_packed_fwd(x, n, every_n, P, frames=frames)
    assert list(cache["k"]) == [4, 0, 0, 1, 2, 3] and cache["r"].shape[0] == 10
    assert np.array_equal(cache["r"][:4], x[0, 8:12]) and np.array_equal(cache["r"][4], x[3, 4])
    assert not cache["V"][1].any() and not cache["V"][2].any()
    assert not np.array_equal(pred, nv.netvlad_packed_fwd(x, n, every_n, P)[0])       # (the grid's rows are other rows)
    hb = cache["hid_bn"]
    assert min(np.abs(hb).min(), np.abs(hb - 6).min()) > 1e-4
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
