"""Student frame selection without a GPU: the properties of the table (on its numpy restatement, tests/_frame_select_ref.py, which the GPU
tests hold the kernel to bit for bit) for T = 300, every admissible every_n and every n, and the flags: parsing, the unknown word refused
before the device is touched, --ensemble_sampling checked like its siblings."""
import numpy as np
import pytest

import _frame_select_ref as ref

T = 300


def _admissible():
    from efficientvideoclassification_youtube8m_amd import distill
    out = []
    for e in range(1, T + 1):
        try:
            distill.validate_every_n(e, 5, T)
        except ValueError:
            continue
        out.append(e)
    return out


def test_admissible_every_n():
    assert _admissible() == [1, 2, 3, 4, 5, 6, 10, 12, 15, 20, 30, 60]


@pytest.mark.parametrize("every_n", [1, 2, 3, 4, 5, 6, 10, 12, 15, 20, 30, 60])
def test_table_properties(every_n):
    from efficientvideoclassification_youtube8m_amd import distill, ops
    S = T // every_n
    ns = np.arange(T + 1)
    ks, _, _ = ops.host_frame_counts(ns, every_n, 5, S // 5, T, subsampled=True)
    for n in ns:
        k = ref.student_count(n, T, S)
        assert k == ks[n] and k <= n and k <= S
        for strategy in ref.STRATEGIES:
            row = ref.table_row(n, T, every_n, strategy, seed=3, draw=n, row=7)
            assert row.shape == (S,) and row.dtype == np.int32
            if strategy == "uniform":
                assert row.tolist() == distill.every_n_indices(every_n, T)
                continue
            assert (row >= 0).sum() == k and (row[:k] >= 0).all() and (row[k:] == -1).all(), (strategy, n)
            assert (np.diff(row[:k]) > 0).all(), (strategy, n)                      # strictly increasing, so distinct
            assert k == 0 or (row[0] >= 0 and row[k - 1] < n), (strategy, n)
        (f0, fl), (m0, ml), (l0, ll) = ref.fml_runs(n, k)
        assert fl + ml + ll == k and f0 == 0 and l0 + ll == n
        assert f0 + fl <= m0 and m0 + ml <= l0, (n, k)                             # disjoint, in order (every_n = 1: the clamp acts)
        if k:
            assert ref.table_row(n, T, every_n, "first", row=1)[k - 1] == k - 1
            assert ref.table_row(n, T, every_n, "last", row=1)[k - 1] == n - 1
            mid = ref.table_row(n, T, every_n, "middle")
            assert mid[0] == (n - k) // 2 and mid[k - 1] == (n - k) // 2 + k - 1


def test_float64_quirk_is_kept():
    """At every_n = 1 the student count is n - 1 for n = 55, 79, ...: the table then leaves one frame out and ends in one -1."""
    S = T
    assert ref.student_count(55, T, S) == 54 and ref.student_count(79, T, S) == 78 and ref.student_count(56, T, S) == 56
    row = ref.table_row(55, T, 1, "last")
    assert row[:54].tolist() == list(range(1, 55)) and (row[54:] == -1).all()
    assert ref.fml_runs(55, 54) == ((0, 18), (18, 18), (37, 18))
    # the clamp: with k = n = 56 the middle run would start at (56 - 19) / 2 = 18, inside the first run of 19
    assert ref.fml_runs(56, 56) == ((0, 19), (19, 19), (38, 18))
    assert ref.table_row(56, T, 1, "first_middle_last")[:56].tolist() == list(range(56))


def test_random_depends_on_seed_draw_row_and_repeats():
    a = ref.table([300, 200, 120], T, 10, "random", seed=1, draw=0, row0=0)
    assert (a == ref.table([300, 200, 120], T, 10, "random", seed=1, draw=0, row0=0)).all()
    assert (a != ref.table([300, 200, 120], T, 10, "random", seed=2, draw=0, row0=0)).any()
    assert (a != ref.table([300, 200, 120], T, 10, "random", seed=1, draw=1, row0=0)).any()
    assert (a != ref.table([300, 200, 120], T, 10, "random", seed=1, draw=0, row0=3)).any()
    assert (ref.table([300, 300], T, 10, "random")[0] != ref.table([300, 300], T, 10, "random")[1]).any()      # other videos, other frames
    # no frame is favoured: over many draws every frame of a 300-frame video is taken about k / n = 1 / 10 of the time
    hits = np.zeros(T)
    for d in range(400):
        hits[ref.table_row(300, T, 10, "random", seed=5, draw=d)] += 1
    assert hits.sum() == 400 * 30 and hits.min() > 10 and hits.max() < 80      # mean 40, sd 6: more than 4.5 sd either way


# ---- flags ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def flags():
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    FLAGS.reset()
    yield FLAGS
    FLAGS.reset()


@pytest.fixture
def no_device(monkeypatch):
    import torch
    from efficientvideoclassification_youtube8m_amd import inference, ops, validate

    def touched(*a, **k):
        raise AssertionError("the device or the data was touched before the flags were checked")
    monkeypatch.setattr(torch.cuda, "set_device", touched)
    monkeypatch.setattr(ops, "check_device", touched)
    monkeypatch.setattr(inference, "latest_checkpoint", touched)
    monkeypatch.setattr(validate, "latest_checkpoint", touched)


def test_flag_defaults_and_parsing(flags):
    from efficientvideoclassification_youtube8m_amd import ops
    assert flags.student_sampling == "uniform" and flags.student_sampling_seed == 0 and flags.ensemble_sampling == ""
    assert ops.STUDENT_SAMPLING == ref.STRATEGIES
    for word in ref.STRATEGIES:
        flags.parse(["--student_sampling", word, "--student_sampling_seed=11"])
        assert flags.student_sampling == word and flags.student_sampling_seed == 11
    flags.parse(["--student_sampling=first_middle_last"])
    assert flags.student_sampling == "first_middle_last"


@pytest.mark.parametrize("binary", ["train", "train_finetune", "train_convert_model", "validate", "eval_finetune", "inference"])
def test_unknown_word_is_refused_before_the_device(flags, no_device, binary):
    import importlib
    mod = importlib.import_module("efficientvideoclassification_youtube8m_amd." + binary)
    with pytest.raises(ValueError, match="student_sampling"):
        mod.main(["--student_sampling", "evenly", "--train_dir", "/nonexistent/x_train/"])


def test_graphs_refuse_an_unknown_word():
    from efficientvideoclassification_youtube8m_amd import distill
    for make in (lambda: distill.EvalGraph(2, student_sampling="evenly", device="cpu"),
                 lambda: distill.DistillGraph(2, student_sampling="evenly", device="cpu"),
                 lambda: distill.EnsembleGraph(2, [("student", 10, "evenly")], device="cpu")):
        with pytest.raises(ValueError, match="evenly"):
            make()


def test_ensemble_sampling(flags):
    from efficientvideoclassification_youtube8m_amd import inference
    flags.parse(["--ensemble_dirs", "a/,b/,c/", "--student_sampling", "middle"])
    assert inference.ensemble_spec()["sampling"] == ["middle"] * 3                   # default: --student_sampling for all
    flags.parse(["--ensemble_sampling", "first, last,random"])
    assert inference.ensemble_spec()["sampling"] == ["first", "last", "random"]
    flags.parse(["--ensemble_sampling", "first,last"])
    with pytest.raises(ValueError, match="ensemble_sampling: 2 entries for 3"):
        inference.ensemble_spec()
    flags.parse(["--ensemble_sampling", "first,last,latest"])
    with pytest.raises(ValueError, match="ensemble_sampling"):
        inference.ensemble_spec()
    flags.reset()
    flags.parse(["--ensemble_sampling", "first"])
    with pytest.raises(ValueError, match="ensemble_sampling: 1 entries for 0"):
        inference.ensemble_spec()


def test_checkpoints_carry_the_word(flags, tmp_path, caplog):
    """train_convert_model keeps what the student was trained with; validate / inference warn when the flag disagrees."""
    import logging
    import torch
    from efficientvideoclassification_youtube8m_amd import inference, train_convert_model
    sd = {"global_step": 8, "model_student/w": torch.zeros(2), "model/w": torch.zeros(2), "student_sampling": "last"}
    assert train_convert_model.extract_student(sd)["student_sampling"] == "last"
    assert "student_sampling" not in train_convert_model.extract_student({"global_step": 8, "model_student/w": torch.zeros(2)})
    d = tmp_path / "m_train"
    d.mkdir()
    torch.save(sd, str(d / "model.ckpt-8.pt"))
    path = train_convert_model.main(["--train_dir", str(d) + "/", "--student_sampling", "last"])
    assert torch.load(path)["student_sampling"] == "last"
    with caplog.at_level(logging.WARNING):
        inference.warn_sampling(sd, "last", "x")
        assert not caplog.records
        inference.warn_sampling({"global_step": 1}, "first", "x")                     # an older checkpoint says nothing
        assert not caplog.records
        inference.warn_sampling(sd, "first", "x")
        assert len(caplog.records) == 1 and "trained with last" in caplog.records[0].getMessage()
