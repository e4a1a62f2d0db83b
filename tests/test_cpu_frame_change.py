"""Content-aware student frames (--student_sampling change | segment_change) without a GPU: self-checks of the numpy restatement
(tests/_frame_change_ref.py, which the GPU tests hold the kernels to bit for bit) on hand-worked cases and over every n, and the host side:
the words in the flags of the six binaries, in --ensemble_sampling / --serial_sampling, in the graphs, and refused where the frames are missing."""
import numpy as np
import pytest

import _frame_change_ref as ref
import _frame_select_ref as sel_ref

T = 300
FIRST = 0xFFFFFFFF


# ---- the reference itself ---------------------------------------------------------------------------------------------------------
def test_keys_by_hand():
    q = np.array([[1, 2, 3], [1, 2, 3], [4, 2, 1], [0, 255, 0], [9, 9, 9]], np.uint8)
    assert ref.keys_row(q, 5).tolist() == [FIRST, 0, 9 + 0 + 4, 16 + 253 * 253 + 1, 81 + 246 * 246 + 81]
    assert ref.keys_row(q, 3).tolist() == [FIRST, 0, 13, 0, 0]
    assert ref.keys_row(q, 1).tolist() == [FIRST, 0, 0, 0, 0]
    assert ref.keys_row(q, 0).tolist() == [0, 0, 0, 0, 0] and ref.keys_row(q, -3).tolist() == [0] * 5
    assert ref.keys_row(q, 9).tolist() == ref.keys_row(q, 5).tolist()                       # n = min(num_frames, T)
    x = np.array([[0.5, -1.0], [1.5, 1.0], [np.nan, 0.0], [0.0, 0.0], [0.0, 0.0]], np.float32)
    want = [FIRST, int(np.float32(5.0).view(np.uint32)), FIRST, FIRST, 0]
    assert ref.keys_row(x, 5).tolist() == want
    # the widest sums: all-0 against all-255 rows at F = 1152 and at the largest F that fits 32 bits
    for F in (1152, 66051):
        z = np.zeros((2, F), np.uint8)
        z[1] = 255
        assert ref.keys_row(z, 2)[1] == F * 65025 and F * 65025 <= FIRST
    assert 66052 * 65025 > FIRST


def test_tables_by_hand():
    # T = 12, every_n = 3: S = 4; n = 9: k = int(9 / 12 * 4) = 3, segments [0, 3) [3, 6) [6, 9)
    key = np.array([FIRST, 5, 7, 7, 2, 7, 1, 1, 0, 99, 99, 99], np.uint32)
    assert ref.segments(9, 3) == [(0, 3), (3, 6), (6, 9)]
    assert ref.table_row(key, 9, 12, 3, "change").tolist() == [0, 2, 3, -1]                 # 7 three times: the two smallest t
    assert ref.table_row(key, 9, 12, 3, "segment_change").tolist() == [0, 3, 6, -1]         # [7, 2, 7] -> 3; [1, 1, 0] -> 6
    assert ref.table_row(key, 12, 12, 3, "change").tolist() == [0, 9, 10, 11]
    assert ref.table_row(key, 12, 12, 3, "segment_change").tolist() == [0, 3, 6, 9]
    # all keys equal: the tie rule decides everything - the first k frames, and the first frame of every segment
    same = np.full(12, 4, np.uint32)
    assert ref.table_row(same, 9, 12, 3, "change").tolist() == [0, 1, 2, -1]
    assert ref.table_row(same, 9, 12, 3, "segment_change").tolist() == [0, 3, 6, -1]
    # the big jumps sit together: change follows them, segment_change keeps one frame per third
    jump = np.array([FIRST, 0, 0, 0, 0, 0, 50, 60, 70, 0, 0, 0], np.uint32)
    assert ref.table_row(jump, 12, 12, 2, "change").tolist() == [0, 1, 2, 6, 7, 8]
    assert ref.table_row(jump, 12, 12, 2, "segment_change").tolist() == [0, 2, 4, 7, 8, 10]


def test_edge_counts():
    key = np.arange(T, dtype=np.uint32)[::-1].copy()
    for strategy in ref.STRATEGIES:
        assert (ref.table_row(key, 0, T, 10, strategy) == -1).all()                         # n = 0
        assert (ref.table_row(key, 1, T, 10, strategy) == -1).all()                         # n = 1: k = int(1 / 300 * 30) = 0
        assert ref.table_row(key, 1, T, 1, strategy).tolist() == [0] + [-1] * (T - 1)       # n = 1, k = 1
        assert ref.table_row(key, 56, T, 1, strategy)[:56].tolist() == list(range(56))      # k = n: every frame
        assert ref.table_row(key, T + 9, T, 1, strategy).tolist() == list(range(T))
    # the float64 quirk at every_n = 1: k = 54 of n = 55 frames - one frame is left out, the one of smallest key / a segment of two
    assert ref.student_count(55, T, T) == 54 == sel_ref.student_count(55, T, T)
    row = ref.table_row(key, 55, T, 1, "change")                                           # keys fall with t: frame 54 is left out
    assert row[:54].tolist() == list(range(54)) and (row[54:] == -1).all()
    row = ref.table_row(key, 55, T, 1, "segment_change")
    assert (row[:54] >= 0).all() and (row[54:] == -1).all() and sorted(len(range(*s)) for s in ref.segments(55, 54))[-2:] == [1, 2]


@pytest.mark.parametrize("every_n", [1, 2, 10, 30])
def test_table_properties(every_n):
    S = T // every_n
    rng = np.random.default_rng(every_n)
    for n in range(T + 1):
        k = ref.student_count(n, T, S)
        assert k == sel_ref.student_count(n, T, S) and k <= n
        segs = ref.segments(n, k)
        assert all(lo < hi for lo, hi in segs)                                              # non-empty
        assert not segs or (segs[0][0] == 0 and segs[-1][1] == n and all(a[1] == b[0] for a, b in zip(segs, segs[1:])))
        key = rng.integers(0, 4, T).astype(np.uint32)                                       # many ties
        key[0] = FIRST
        for strategy in ref.STRATEGIES:
            row = ref.table_row(key, n, T, every_n, strategy)
            assert row.shape == (S,) and row.dtype == np.int32
            assert (row[:k] >= 0).all() and (row[k:] == -1).all() and (np.diff(row[:k]) > 0).all(), (strategy, n)
            assert k == 0 or row[k - 1] < n
        if k:
            ch = ref.table_row(key, n, T, every_n, "change")[:k]
            assert ch[0] == 0                                                               # the first frame is always taken
            left = np.setdiff1d(np.arange(n), ch)
            assert left.size == 0 or key[left].max() <= key[ch].min()
            sg = ref.table_row(key, n, T, every_n, "segment_change")[:k]
            assert all(lo <= t < hi and key[t] == key[lo:hi].max() for t, (lo, hi) in zip(sg, segs))


# ---- the host side ------------------------------------------------------------------------------------------------------------------
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


class _Parsed(Exception):
    pass


def test_the_words():
    from efficientvideoclassification_youtube8m_amd import ops
    assert ops.STUDENT_SAMPLING == sel_ref.STRATEGIES                                       # the stateless strategies: as they were
    assert ops.STUDENT_SAMPLING_SCORED == ref.STRATEGIES
    for word in ref.STRATEGIES:
        assert ops.check_student_sampling(word) == word
    with pytest.raises(ValueError) as e:
        ops.check_student_sampling("evenly", "--student_sampling")
    for word in sel_ref.STRATEGIES + ref.STRATEGIES:
        assert word in str(e.value)
    assert "--student_sampling" in str(e.value)


@pytest.mark.parametrize("binary", ["train", "train_finetune", "train_convert_model", "validate", "eval_finetune", "inference"])
def test_binaries_accept_the_words(flags, no_device, monkeypatch, binary):
    """Each binary parses its flags first: the new words pass the parse (the run is stopped right behind it), `evenly` does not."""
    import importlib
    mod = importlib.import_module("efficientvideoclassification_youtube8m_amd." + binary)
    parse = type(flags).parse

    def parse_and_stop(self, argv):
        parse(self, argv)
        raise _Parsed()
    monkeypatch.setattr(type(flags), "parse", parse_and_stop)
    for word in ref.STRATEGIES:
        with pytest.raises(_Parsed):
            mod.main(["--student_sampling", word, "--train_dir", "/nonexistent/x_train/"])
        assert flags.student_sampling == word
    with pytest.raises(ValueError, match="student_sampling"):
        mod.main(["--student_sampling", "evenly", "--train_dir", "/nonexistent/x_train/"])


def test_help_names_the_words(flags):
    from efficientvideoclassification_youtube8m_amd import flags as flags_mod
    text = open(flags_mod.__file__).read()
    assert "random|change|segment_change" in text


def test_ensemble_and_serial_sampling(flags):
    from efficientvideoclassification_youtube8m_amd import inference
    flags.parse(["--ensemble_dirs", "a/,b/,c/", "--ensemble_sampling", "change, segment_change,first"])
    assert inference.ensemble_spec()["sampling"] == ["change", "segment_change", "first"]
    flags.parse(["--ensemble_sampling", "change,segment_change,changes"])
    with pytest.raises(ValueError, match="ensemble_sampling"):
        inference.ensemble_spec()
    flags.reset()
    flags.parse(["--serial_sampling", "change,uniform,segment_change"])
    assert flags.serial_sampling == "change,uniform,segment_change"
    with pytest.raises(ValueError, match="student_sampling"):
        flags.parse(["--serial_sampling", "change,segments"])


def test_graphs_know_the_scored_words():
    """(The graphs themselves need a device: tests/test_gpu_frame_change.py.)  What they read: the word check and scored_sampling."""
    from efficientvideoclassification_youtube8m_amd import distill

    class G:
        student = object()
    for word, scored in (("uniform", False), ("random", False), ("change", True), ("segment_change", True)):
        G.student_sampling = word
        assert distill.scored_sampling(G) is scored
    G.student = None                                                                        # a teacher-only member never needs the keys
    assert not distill.scored_sampling(G)
    with pytest.raises(ValueError, match="evenly.*segment_change"):
        distill.EnsembleGraph(2, [("student", 10, "evenly")], device="cpu")


def test_the_stateless_entry_refuses_the_scored_words():
    import torch
    from efficientvideoclassification_youtube8m_amd import ops
    n = torch.tensor([300, 120], dtype=torch.int32)
    for word in ref.STRATEGIES:
        with pytest.raises(ValueError, match="frames are needed"):
            ops.student_frame_select(n, T, 10, word)
    with pytest.raises(ValueError, match="student_frame_select_scored"):
        ops.student_frame_select_scored(n, torch.zeros((2, T), dtype=torch.int32), T, 10, "random")


def test_checkpoints_carry_the_word(flags, tmp_path, caplog):
    import logging
    import torch
    from efficientvideoclassification_youtube8m_amd import inference, train_convert_model
    sd = {"global_step": 8, "model_student/w": torch.zeros(2), "model/w": torch.zeros(2), "student_sampling": "segment_change"}
    assert train_convert_model.extract_student(sd)["student_sampling"] == "segment_change"
    with caplog.at_level(logging.WARNING):
        inference.warn_sampling(sd, "segment_change", "x")
        assert not caplog.records
        inference.warn_sampling(sd, "change", "x")
        assert len(caplog.records) == 1 and "trained with segment_change" in caplog.records[0].getMessage()


def test_limits_are_refused_before_any_launch():
    """The argument checks of both entries run on the host and return before a launch: they can be held without a device."""
    import ctypes
    from efficientvideoclassification_youtube8m_amd import _lib
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    bad_shape, bad_arg = r"\(-1\)", r"\(-5\)"
    for args, code in (((p, None, p, 2, 1025, 8), bad_shape), ((None, None, p, 2, 4, 8), bad_arg), ((p, p, p, 2, 4, 8), bad_arg),
                       ((None, p, p, 2, 4, 66052), bad_shape), ((p, None, p, 0, 4, 8), bad_shape), ((p, None, p, 2, 4, 0), bad_shape),
                       ((p, None, None, 2, 4, 8), bad_arg)):
        with pytest.raises(_lib.EvcError, match=code):
            _lib.call("evc_frame_change_keys", *args, p, None)
    for args, code in (((p, p, 2, 300, 10, 5), bad_arg), ((p, p, 2, 300, 10, 8), bad_arg), ((p, p, 2, 1025, 10, 6), bad_shape),
                       ((p, p, 2, 300, 0, 7), bad_shape), ((p, p, 2, 300, 301, 7), bad_shape), ((p, None, 2, 300, 10, 6), bad_arg)):
        with pytest.raises(_lib.EvcError, match=code):
            _lib.call("evc_student_frame_select_scored", *args, p, None)
