"""Offline distillation without a GPU: the reference of the sparse loss section (tests/_distill_sparse_ref.py), the host tables behind
train --teacher_preds_pattern (inference.PriorTables against gather_priors, bit for bit), the flag with every refused combination
(before a device call), the --distill_losses default, and the recorded settings through the checkpoint dictionary and the resume check."""
import os

import numpy as np
import pytest
import torch

import _distill_losses_ref as base
import _distill_sparse_ref as sref
import _ensemble_ref as ens
from efficientvideoclassification_youtube8m_amd import _lib, distill, inference, ops, train
from efficientvideoclassification_youtube8m_amd.flags import FLAGS


@pytest.fixture(autouse=True)
def _fresh_flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("a device was selected"))


# ---- the reference --------------------------------------------------------------------------------------------------------------------
def test_reference_on_full_lists_is_the_dense_reference():
    """Lists that name every class scatter to the dense row's bits, and the reference on them is _distill_losses_ref.reference."""
    B, V = 3, 40
    inp = base.make_inputs(B, V, 1)
    idx = np.broadcast_to(np.arange(V, dtype=np.int32), (1, B, V)).copy()
    case = dict(labels=inp["labels"], pred_s=inp["pred_s"], idx=idx, val=inp["pred_t"][None].copy())
    for mode, w in (("mean", np.ones(1, np.float32)), ("max", None)):
        got = sref.reference(case, mode, w, 1.0 / B, 1.0)
        assert np.array_equal(got["pred_comb"].view(np.uint32), inp["pred_t"].view(np.uint32))
        want = base.reference(dict(inp, state_t=inp["state_s"]), 1.0 / B, 1.0, 0.0)
        assert np.allclose(got["losses"], want["losses"], rtol=1e-12, atol=0) and np.array_equal(got["ce"], want["ce"])
        assert np.allclose(got["kl"], want["kl"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("shape", [(1, 5, 3, 3), (2, 1023, 20, 2), (3, 4716, 256, 8)])
def test_reference_cases_hold_the_planted_conditions(shape):
    B, V, kp, F = shape
    case = sref.make_case(*shape)
    idx = case["idx"]
    assert idx[0, 0, 0] >= 0
    if F >= 2:
        assert idx[1, 0, 0] == idx[0, 0, 0]                                        # a class listed by several files
    if kp >= 20:                      # (at kp = 3 a row with three entries is a matter of the draw: these two shapes are known to hold one)
        assert any((idx[p, b, 1] < 0) and (idx[p, b, 2:] >= 0).any() for p in range(F) for b in range(B))      # padding in the middle
    for mode in sref.MODES:
        out = sref.reference(case, mode, sref.weights(F, mode), 1.0 / B, 1.0)
        assert np.isfinite(out["losses"]).all() and np.isfinite(out["kl"]).all() and out["losses"][1] == 0
        if B >= 2:
            assert (idx[:, B - 1] < 0).all() and not out["pred_comb"][B - 1].any() and not out["kl"][B - 1].any()
        c = idx[0, 0, 0]
        if mode == "mean" and F >= 2:                                              # left to right in float32, from +0.0
            w = sref.weights(F, mode)
            acc = np.float32(0)
            for p in range(F):
                hit = np.flatnonzero(idx[p, 0] == c)
                if hit.size:
                    acc = acc + w[p] * case["val"][p, 0, hit[0]]
            assert acc.dtype == np.float32 and out["pred_comb"][0, c] == acc


# ---- the host tables ------------------------------------------------------------------------------------------------------------------
def _write(path, lines):
    with open(path, "w") as f:
        f.write(inference.HEADER)
        for vid, pairs in lines:
            f.write("%s,%s\n" % (vid, " ".join("%d %f" % (c, v) for c, v in pairs)))


def _files(tmp_path):
    rng = np.random.default_rng(0)
    ids = ["vid%03d" % i for i in range(40)]
    paths = []
    for p, longest in enumerate((20, 7, 1)):
        lines = []
        for i, vid in enumerate(ids):
            n = 0 if (p == 1 and i == 3) else int(rng.integers(1, longest + 1))       # short lists, and one empty one
            lines.append((vid, list(zip(rng.choice(train.NUM_CLASSES, n, replace=False).tolist(), rng.random(n).tolist()))))
        rng.shuffle(lines)                                                             # every file in an order of its own
        paths.append(str(tmp_path / ("preds_%d.csv" % p)))
        _write(paths[-1], lines)
    return ids, paths


def test_the_batch_gather_returns_the_arrays_of_gather_priors(tmp_path):
    ids, paths = _files(tmp_path)
    tables = [inference.read_prediction_file(p) for p in paths]
    kp = inference.prior_list_length(tables)
    fast = inference.PriorTables(paths)
    assert fast.kp == kp == 20 and len(fast) == 3 and fast.idx[0].flags.c_contiguous and fast.idx[0].shape == (40, kp)
    rng = np.random.default_rng(1)
    for trial, files in enumerate(([0, 1, 2], [0], [2, 1])):
        sub = inference.PriorTables([paths[f] for f in files])
        sub_tables = [tables[f] for f in files]
        sub_kp = inference.prior_list_length(sub_tables)
        batch = rng.choice(ids, 17, replace=True).tolist()                             # a video may repeat within a batch
        if trial == 1:
            batch = [v.encode("utf-8") for v in batch]                                 # ids as bytes, as the reader hands them out
        elif trial == 2:
            batch = [v.encode("utf-8") if i % 2 else v for i, v in enumerate(batch)]
        want_i, want_v = inference.gather_priors(sub_tables, [paths[f] for f in files], batch, sub_kp)
        got_i, got_v = sub.gather(batch)
        assert got_i.dtype == np.int32 and got_v.dtype == np.float32 and got_i.shape == (len(files), 17, sub_kp)
        assert np.array_equal(got_i, want_i) and np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32))
        out = (np.full_like(want_i, 99), np.full_like(want_v, 99.0))                   # into the caller's buffers, every element written
        assert sub.gather(batch, out=out)[0] is out[0]
        assert np.array_equal(out[0], want_i) and np.array_equal(out[1].view(np.uint32), want_v.view(np.uint32))
    empty = fast.gather([])
    assert empty[0].shape == (3, 0, kp)


def test_a_missing_video_id_is_the_key_error_of_gather_priors(tmp_path):
    ids, paths = _files(tmp_path)
    _write(paths[1], [(v, [(1, 0.5)]) for v in ids if v != "vid007"])
    fast = inference.PriorTables(paths)
    tables = [inference.read_prediction_file(p) for p in paths]
    for batch in (["vid001", "vid007"], [b"vid001", b"vid007"]):
        with pytest.raises(KeyError) as slow:
            inference.gather_priors(tables, paths, batch, fast.kp)
        with pytest.raises(KeyError) as quick:
            fast.gather(batch)
        assert quick.value.args == slow.value.args and "vid007" in str(quick.value) and paths[1] in str(quick.value)


def test_the_loader_keeps_the_errors_of_read_prediction_file(tmp_path):
    bad = str(tmp_path / "bad.csv")
    with open(bad, "w") as f:
        f.write(inference.HEADER + "a,1 0.5 1 0.25\n")
    with pytest.raises(ValueError, match="listed twice"):
        inference.PriorTables([bad])
    with open(bad, "w") as f:
        f.write("a,1 0.5\n")
    with pytest.raises(ValueError, match="first line"):
        inference.PriorTables([bad])


# ---- the flag -------------------------------------------------------------------------------------------------------------------------
BASE = ["--train_data_pattern", "records/train*.tfrecord", "--model", "HierarchicalLstmModel", "--every_n", "10"]


def _pattern(tmp_path, count=1):
    for i in range(count):
        _write(str(tmp_path / ("t%02d.csv" % i)), [("a", [(1, 0.5)])])
    return str(tmp_path / "t*.csv")


def test_the_flag_resolves_to_the_documented_defaults(tmp_path):
    assert FLAGS.teacher_preds_pattern == "" and train.offline_teachers() is None
    FLAGS.parse(BASE + ["--teacher_preds_pattern", _pattern(tmp_path, 3)])
    spec = train.offline_teachers()
    assert spec["names"] == ["t00.csv", "t01.csv", "t02.csv"] and [os.path.basename(f) for f in spec["files"]] == spec["names"]
    assert spec["mode"] == "mean" and spec["losses"] == ("pred", "ce")                  # --distill_losses defaults to pred,ce here
    assert spec["weights"].dtype == np.float32 and np.array_equal(spec["weights"], np.full(3, np.float32(1) / np.float32(3), np.float32))
    assert FLAGS.distill_losses == "rep,pred,ce" and train.ensemble_teachers() is None and train.check_serial_flags() is False
    FLAGS.parse(["--teacher_mode", "max"])
    assert train.offline_teachers()["weights"] is None
    FLAGS.parse(["--teacher_mode", "mean", "--teacher_weights", "0.5,0.25,0.25", "--distill_losses", "pred"])
    spec = train.offline_teachers()
    assert spec["weights"].tolist() == [0.5, 0.25, 0.25] and spec["losses"] == ("pred",)
    assert train.ensemble_teachers() is None and train.check_serial_flags() is False    # the two reused flags need no --teacher_dirs here


def test_the_reused_flags_still_need_teacher_dirs_without_the_new_flag():
    FLAGS.parse(["--teacher_weights", "1.0"])
    with pytest.raises(ValueError, match="needs --teacher_dirs"):
        train.ensemble_teachers()
    FLAGS.reset()
    FLAGS.parse(["--distill_losses", "pred,ce"])
    with pytest.raises(ValueError, match="needs --teacher_dir"):
        train.check_serial_flags()


@pytest.mark.parametrize("extra,words", [
    (["--teacher_dir", "t/"], ["--teacher_preds_pattern", "--teacher_dir "]),
    (["--teacher_dirs", "a/,b/"], ["--teacher_preds_pattern", "--teacher_dirs"]),
    (["--teacher_dir", "t/", "--serial_student_dirs", "a/,b/"], ["--teacher_preds_pattern", "--teacher_dir"]),
    (["--serial_student_dirs", "a/,b/"], ["--teacher_preds_pattern", "--serial_student_dirs"]),
    (["--teacher_only", "True"], ["--teacher_preds_pattern", "--teacher_only"]),
    (["--label_loss", "CrossEntropyLossPositives"], ["--teacher_preds_pattern", "--label_loss"]),
    (["--finetune"], ["--teacher_preds_pattern", "train_finetune"]),
    (["--train_data_pattern", "synthetic"], ["--teacher_preds_pattern", "--train_data_pattern", "synthetic"]),
    (["--train_data_pattern", ""], ["--teacher_preds_pattern", "--train_data_pattern"]),
    (["--distill_losses", "rep,pred"], ["--teacher_preds_pattern", "--distill_losses", "no state"]),
    (["--distill_losses", "rep,pred,ce"], ["--teacher_preds_pattern", "--distill_losses", "no state"]),
    (["--model", "DbofModel"], ["--teacher_preds_pattern", "--model"]),
    (["--teacher_mode", "median"], ["--teacher_mode"]),
    (["--teacher_mode", "max", "--teacher_weights", "1.0"], ["--teacher_weights", "--teacher_mode"]),
    (["--teacher_weights", "0.5,0.5"], ["--teacher_weights", "--teacher_preds_pattern"]),
])
def test_refused_combinations_name_both_flags_before_the_device_is_touched(tmp_path, no_device, extra, words):
    argv = BASE + ["--teacher_preds_pattern", _pattern(tmp_path), "--train_dir", str(tmp_path / "out")] + extra
    with pytest.raises(ValueError) as e:
        train.main(argv)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_the_file_count_and_several_ranks_are_refused(tmp_path, no_device, monkeypatch):
    with pytest.raises(ValueError, match="matches no file"):
        train.main(BASE + ["--teacher_preds_pattern", str(tmp_path / "none*.csv")])
    FLAGS.reset()
    with pytest.raises(ValueError, match="9 files"):
        train.main(BASE + ["--teacher_preds_pattern", _pattern(tmp_path, 9)])
    FLAGS.reset()
    (tmp_path / "eight").mkdir()
    FLAGS.parse(BASE + ["--teacher_preds_pattern", _pattern(tmp_path / "eight", 8)])
    assert len(train.offline_teachers()["files"]) == 8
    with pytest.raises(ValueError, match="ranks"):
        train.offline_teachers(world=2)
    with pytest.raises(ValueError, match="train_finetune"):
        train.offline_teachers(finetune=True)


def test_train_finetune_refuses_the_flag(tmp_path, no_device):
    from efficientvideoclassification_youtube8m_amd import train_finetune
    with pytest.raises(ValueError, match="train_finetune"):
        train_finetune.main(BASE + ["--teacher_preds_pattern", _pattern(tmp_path)])


# ---- the recorded settings ------------------------------------------------------------------------------------------------------------
def test_the_recorded_settings_round_trip_and_the_resume_check(tmp_path, caplog):
    FLAGS.parse(BASE + ["--teacher_preds_pattern", _pattern(tmp_path, 2), "--teacher_weights", "0.75,0.25"])
    spec = train.offline_teachers()
    record = train.offline_record(spec)
    assert record == {"files": ["t00.csv", "t01.csv"], "mode": "mean", "weights": [0.75, 0.25]}
    ck = str(tmp_path / "model.ckpt-3.pt")
    torch.save({"global_step": 3, "distill_mode": "offline", "distill_losses": ",".join(spec["losses"]), "distill_teacher_files": record}, ck)
    sd = torch.load(ck, map_location="cpu")
    assert sd["distill_teacher_files"] == record and sd["distill_losses"] == "pred,ce"
    train.check_recorded_files(sd, spec, ck)                                            # the same settings: accepted
    train.check_recorded_files({"global_step": 0}, spec, ck)                            # a checkpoint that records none (train_convert_model's)
    renamed = dict(spec, names=["x.csv", "y.csv"])
    with caplog.at_level("INFO"):
        train.check_recorded_files(sd, renamed, ck)                                     # other names: logged, not refused
    assert "x.csv" in caplog.text
    for other in (dict(spec, mode="max", weights=None), dict(spec, weights=np.asarray([0.5, 0.5], np.float32)), dict(spec, losses=("pred",)),
                  dict(spec, names=["t00.csv"], files=spec["files"][:1], weights=np.asarray([0.75], np.float32))):
        with pytest.raises(ValueError, match="recorded"):
            train.check_recorded_files(sd, other, ck)


def test_resuming_with_another_mode_is_refused_before_the_device_is_touched(tmp_path, no_device):
    out = tmp_path / "out"
    out.mkdir()
    torch.save({"global_step": 3, "distill_mode": "offline", "distill_losses": "pred,ce",
                "distill_teacher_files": {"files": ["t00.csv"], "mode": "mean", "weights": [1.0]}}, str(out / "model.ckpt-3.pt"))
    with pytest.raises(ValueError, match="recorded"):
        train.main(BASE + ["--teacher_preds_pattern", _pattern(tmp_path), "--train_dir", str(out), "--teacher_mode", "max"])


# ---- the entry, the binding and the wrapper -------------------------------------------------------------------------------------------
def test_the_entry_is_declared_bound_and_wrapped():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "evc.h")).read()
    assert "int evc_distill_losses_sparse(" in header and "workspace: 3 * B floats" in header
    assert len(_lib.SIGNATURES["evc_distill_losses_sparse"]) == 17 and "evc_distill_losses_sparse" in _lib.EXPORTS
    build = open(os.path.join(root, "efficientvideoclassification_youtube8m_amd", "csrc", "build.sh")).read()
    assert " evc_distill_sparse " in build
    z = torch.zeros((1, 2, 3), dtype=torch.int32)
    with pytest.raises(_lib.EvcError, match="device tensors"):
        ops.distill_losses_sparse(z, z.float(), torch.zeros((2, 5), dtype=torch.uint8), torch.zeros((2, 5)), torch.zeros(4))
    with pytest.raises(ValueError, match="mode"):
        ops.distill_losses_sparse(z, z.float(), None, None, None, mode="median")
    assert issubclass(distill.OfflineDistillGraph, distill.DistillGraph) and distill.OfflineDistillGraph.MAX_FILES == 8
