"""Ensemble distillation without a GPU: the numpy / float64 reference of the J-teacher loss section (tests/_distill_ensemble_ref.py), the
--teacher_* flags with every refused combination (before a device call), the recorded teacher list through save_checkpoint and the
resume check, and the new header entry."""
import os

import numpy as np
import pytest
import torch

import _distill_ensemble_ref as eref
import _distill_losses_ref as base
from efficientvideoclassification_youtube8m_amd import _lib, distill, ops, train
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
def _same(a, b):
    for k in ("losses", "ce", "kl", "kl_parts", "rep"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("shape", [(1, 5, 3), (5, 40, 128), (7, 257, 4)])
def test_reference_with_one_teacher_is_the_single_teacher_reference(shape):
    inp = eref.make_inputs(*shape)
    sc = dict(g_ce=1.0 / shape[0], g_kl=1.0, g_rep=2.0)
    for mode, w in (("mean", [1.0]), ("max", None)):
        got = eref.reference(inp, [inp["pred_t"]], [inp["state_t"]], mode, w, [1.0], **sc)
        _same(got, base.reference(inp, **sc))
        assert np.array_equal(got["pred_comb"].view(np.uint32), inp["pred_t"].view(np.uint32))


@pytest.mark.parametrize("shape", [(1, 5, 3), (5, 40, 128), (7, 257, 4)])
def test_reference_on_duplicates_gives_the_one_teacher_arrays_bit_for_bit(shape):
    inp = eref.make_inputs(*shape)
    sc = dict(g_ce=1.0 / shape[0], g_kl=1.0, g_rep=2.0)
    p, s = inp["pred_t"], inp["state_t"]
    one = eref.reference(inp, [p], [s], "mean", [1.0], [1.0], **sc)
    two = eref.reference(inp, [p, p.copy()], [s, None], "mean", [0.5, 0.5], [1.0, 0.0], **sc)
    three = eref.reference(inp, [p, p.copy(), p], [None, s, None], "max", None, [0.0, 1.0, 0.0], **sc)
    for other in (two, three):
        _same(one, other)
        assert np.array_equal(other["pred_comb"].view(np.uint32), p.view(np.uint32))
        assert np.array_equal(other["state_comb"].view(np.uint32), s.view(np.uint32))


def test_reference_combines_in_float32_left_to_right():
    preds, states = eref.teachers(3, 40, 8, 3)
    w = np.asarray([0.2, 0.3, 0.5], np.float32)
    acc = w[0] * preds[0]
    acc = acc + w[1] * preds[1]
    acc = acc + w[2] * preds[2]
    assert acc.dtype == np.float32 and np.array_equal(eref.combine_pred(preds, "mean", w), acc)
    r = np.asarray([0.5, 0.0, 0.5], np.float32)
    assert np.array_equal(eref.combine_state([states[0], None, states[2]], r), r[0] * states[0] + r[2] * states[2])
    assert np.array_equal(eref.default_weights(3), np.full(3, np.float32(1) / np.float32(3), np.float32))


# ---- the flags ------------------------------------------------------------------------------------------------------------------------
def test_flags_default_to_empty_and_resolve_to_the_documented_defaults():
    for k in ("teacher_dirs",) + train.TEACHER_LIST_FLAGS:
        assert getattr(FLAGS, k) == ""
    assert FLAGS.teacher_mode == "mean" and train.ensemble_teachers() is None
    FLAGS.parse(["--teacher_dirs", "a/, b/,a/", "--every_n", "30", "--student_sampling", "last"])
    spec = train.ensemble_teachers()
    assert spec["dirs"] == ["a/", "b/", "a/"] and spec["towers"] == ["auto"] * 3 and spec["every_n"] == [30] * 3
    assert spec["sampling"] == ["last"] * 3 and spec["mode"] == "mean"
    assert spec["weights"].dtype == np.float32 and np.array_equal(spec["weights"], np.full(3, np.float32(1) / np.float32(3), np.float32))
    assert spec["rep_weights"].dtype == np.float32 and spec["rep_weights"].tolist() == [1.0, 0.0, 0.0]
    assert train.check_serial_flags() is False                       # not --teacher_dir's serial mode


def test_lists_are_read_per_entry():
    FLAGS.parse(["--teacher_dirs", "a/,a/", "--teacher_towers", "teacher, student", "--teacher_every_n", "1,10", "--teacher_sampling",
                 "uniform,last", "--teacher_weights", "0.75,0.25", "--teacher_rep_weights", "0.5,0.5", "--every_n", "30",
                 "--distill_losses", "rep,pred"])
    spec = train.ensemble_teachers()
    assert spec["towers"] == ["teacher", "student"] and spec["every_n"] == [1, 10] and spec["sampling"] == ["uniform", "last"]
    assert spec["weights"].tolist() == [0.75, 0.25] and spec["rep_weights"].tolist() == [0.5, 0.5]
    assert train.check_serial_flags() is False                       # --distill_losses is accepted next to --teacher_dirs
    FLAGS.parse(["--teacher_mode", "max", "--teacher_weights", ""])
    assert train.ensemble_teachers()["weights"] is None


REFUSED = [
    (["--teacher_dirs", "a/,b/", "--teacher_dir", "/t/"], {}, "--teacher_dirs.*--teacher_dir "),
    (["--teacher_dirs", "a/,b/", "--serial_student_dirs", "s/"], {}, "--teacher_dirs.*--serial_student_dirs"),
    (["--teacher_dirs", "a/,b/", "--teacher_only", "True"], {}, "--teacher_dirs.*--teacher_only"),
    (["--teacher_dirs", "a/,b/"], {"finetune": True}, "--teacher_dirs.*--finetune"),
    (["--teacher_dirs", "a/,b/"], {"world": 2}, "--teacher_dirs.*2 ranks"),
    (["--teacher_dirs", "a/,b/", "--model", "DbofModel"], {}, "--teacher_dirs.*HierarchicalLstmModel.*--model DbofModel"),
    (["--teacher_dirs", "a/,b/", "--label_loss", "HingeLoss"], {}, "--teacher_dirs.*--label_loss HingeLoss"),
    (["--teacher_dirs", "a/,b/", "--precision", "high"], {}, "--teacher_dirs.*--precision high"),
    (["--teacher_dirs", "a/,b/", "--teacher_towers", "teacher"], {}, "--teacher_towers.*1 entries for the 2 directories"),
    (["--teacher_dirs", "a/,b/", "--teacher_every_n", "10,10,10"], {}, "--teacher_every_n.*3 entries for the 2 directories"),
    (["--teacher_dirs", "a/,b/", "--teacher_sampling", "last"], {}, "--teacher_sampling.*1 entries for the 2 directories"),
    (["--teacher_dirs", "a/,b/", "--teacher_weights", "1"], {}, "--teacher_weights.*1 entries for the 2 directories"),
    (["--teacher_dirs", "a/,b/", "--teacher_rep_weights", "1,0,0"], {}, "--teacher_rep_weights.*3 entries for the 2 directories"),
    (["--teacher_dirs", "a/,b/", "--teacher_mode", "max", "--teacher_weights", ".5,.5"], {}, "--teacher_weights needs --teacher_mode mean"),
    (["--teacher_dirs", "a/,b/", "--teacher_mode", "median"], {}, "--teacher_mode"),
    (["--teacher_dirs", "a/,b/", "--teacher_towers", "student,teacher"], {}, "--teacher_towers.*entry 0"),
    (["--teacher_dirs", "a/,b/", "--teacher_towers", "teacher,pupil"], {}, "--teacher_towers"),
    (["--teacher_dirs", "a/,b/", "--teacher_towers", "teacher,student", "--teacher_every_n", "1,7"], {}, "every_n=7"),
    (["--teacher_dirs", "a/,b/", "--teacher_rep_weights", "0,0"], {}, "--teacher_rep_weights"),
    (["--teacher_dirs", ",".join("d%d/" % i for i in range(9))], {}, "--teacher_dirs.*9 entries"),
    (["--teacher_towers", "teacher"], {}, "--teacher_towers needs --teacher_dirs"),
    (["--teacher_every_n", "10"], {}, "--teacher_every_n needs --teacher_dirs"),
    (["--teacher_sampling", "last"], {}, "--teacher_sampling needs --teacher_dirs"),
    (["--teacher_weights", "1"], {}, "--teacher_weights needs --teacher_dirs"),
    (["--teacher_rep_weights", "1"], {}, "--teacher_rep_weights needs --teacher_dirs"),
]


@pytest.mark.parametrize("argv,kw,match", REFUSED)
def test_refused_combinations(argv, kw, match):
    FLAGS.parse(argv + ["--every_n", "30"])
    with pytest.raises(ValueError, match=match):
        train.ensemble_teachers(**kw)


@pytest.mark.parametrize("argv,kw,match", REFUSED)
def test_main_refuses_before_it_touches_a_device(argv, kw, match, no_device, monkeypatch):
    from efficientvideoclassification_youtube8m_amd import train_finetune
    if kw.get("world"):
        monkeypatch.setenv("WORLD_SIZE", str(kw["world"]))
    with pytest.raises(ValueError, match=match):
        (train_finetune.main if kw.get("finetune") else train.main)(list(argv) + ["--every_n", "30"])


def test_the_refusals_of_teacher_dir_keep_their_text():
    FLAGS.parse(["--distill_losses", "rep"])
    with pytest.raises(ValueError, match="needs --teacher_dir: it selects the student's losses of serial distillation"):
        train.check_serial_flags()


def _teacher_ckpt(d, step=2, student=False, fill=1.0):
    os.makedirs(d, exist_ok=True)
    sd = {"global_step": step, "model/w": torch.full((2, 3), float(fill))}
    if student:
        sd = {"global_step": step, "model_student/w": torch.full((2, 3), float(fill))}
    torch.save(sd, os.path.join(d, "model.ckpt-%d.pt" % step))


def test_entry_0_must_resolve_to_a_teacher_tower_and_every_directory_hold_a_checkpoint(tmp_path, no_device):
    a, b, c = (str(tmp_path / n) + "/" for n in "abc")
    _teacher_ckpt(a)
    _teacher_ckpt(b, student=True)
    os.makedirs(c)
    with pytest.raises(ValueError, match="entry 0.*student tower"):            # auto resolves b to its model_student/*
        train.main(["--teacher_dirs", b + "," + a, "--every_n", "30", "--train_dir", str(tmp_path / "out")])
    with pytest.raises(ValueError, match="no model.ckpt"):
        train.main(["--teacher_dirs", a + "," + c, "--every_n", "30", "--train_dir", str(tmp_path / "out")])
    with pytest.raises(ValueError, match="model_student"):                      # a holds no student to serve as an assistant
        train.main(["--teacher_dirs", a + "," + a, "--teacher_towers", "teacher,student", "--every_n", "30", "--train_dir", str(tmp_path / "out")])
    FLAGS.parse(["--teacher_dirs", a + "," + b, "--every_n", "30"])
    spec = train.ensemble_teachers()
    sds, towers, cks = train.load_teachers(spec)
    assert towers == ["teacher", "student"] and [os.path.basename(x) for x in cks] == ["model.ckpt-2.pt"] * 2
    rec = train.teacher_record(spec, towers, cks)
    assert rec == {"dirs": [a, b], "checkpoints": ["model.ckpt-2.pt"] * 2, "towers": ["teacher", "student"], "every_n": [1, 30],
                   "sampling": ["uniform", "uniform"], "mode": "mean", "weights": [0.5, 0.5], "rep_weights": [1.0, 0.0]}


# ---- the checkpoint -------------------------------------------------------------------------------------------------------------------
class _Store:
    def __init__(self, n, adam):
        self.m = torch.zeros(n) if adam else None
        self.v = torch.zeros(n) if adam else None


class _Tower:
    def __init__(self, scope, adam, fill):
        self.scope, self.adam_t, self.store = scope, 0, _Store(6, adam)
        self.w = torch.full((2, 3), float(fill))

    def state_dict(self):
        return {"%s/w" % self.scope: self.w.clone()}

    def load_state_dict(self, sd):
        self.w.copy_(sd["%s/w" % self.scope])

    def precision_layout(self):
        return {"precision": "bf16"}


class _Graph:
    """The fields save_checkpoint / restore_checkpoint read of an EnsembleDistillGraph, on CPU stand-in towers."""
    mode, distill_losses, student_sampling = "ensemble", ("rep", "pred"), "last"

    def __init__(self, t_fill, s_fill):
        self.global_step = 0
        self.teachers = [_Tower("model", False, t_fill), _Tower("model", False, 9.0)]
        self.teacher, self.student = self.teachers[0], _Tower("model_student", True, s_fill)


def test_metadata_round_trips_and_another_list_is_refused_with_both_shown(tmp_path, no_device):
    a, b, out = (str(tmp_path / n) + "/" for n in ("a", "b", "out"))
    _teacher_ckpt(a, fill=1.5)
    _teacher_ckpt(b, fill=9.0)
    FLAGS.parse(["--teacher_dirs", a + "," + b, "--every_n", "30", "--teacher_weights", "0.75,0.25"])
    spec = train.ensemble_teachers()
    _, towers, cks = train.load_teachers(spec)
    g = _Graph(1.5, 2.5)
    g.teacher_record = train.teacher_record(spec, towers, cks)
    g.global_step, g.student.adam_t = 3, 3
    path = train.save_checkpoint(g, out, 0)
    sd = torch.load(path)
    assert sd["distill_mode"] == "ensemble" and sd["distill_losses"] == "rep,pred" and sd["student_sampling"] == "last"
    assert "model/adam" not in sd and "model_student/adam" in sd and torch.equal(sd["model/w"], g.teacher.w)
    rec = sd["distill_teachers"]
    assert rec == g.teacher_record and rec["dirs"] == [a, b] and rec["weights"] == [0.75, 0.25] and rec["mode"] == "mean"
    train.check_recorded_teachers(rec, train.teacher_record(spec, towers, cks), path)          # the same flags: accepted
    h = _Graph(0.0, 0.0)
    train.restore_checkpoint(h, path)                                                       # the student and entry 0 come from the checkpoint
    assert h.global_step == 3 and torch.equal(h.teacher.w, g.teacher.w) and torch.equal(h.student.w, g.student.w)
    assert float(h.teachers[1].w[0, 0]) == 9.0 and h.teacher.store.m is None
    # the directories swapped: train.main refuses before a device is selected, and shows both lists
    with pytest.raises(ValueError) as e:
        train.main(["--teacher_dirs", b + "," + a, "--every_n", "30", "--teacher_weights", "0.75,0.25", "--train_dir", out])
    msg = str(e.value)
    assert "recorded" in msg and "flags" in msg and str([a, b]) in msg and str([b, a]) in msg
    FLAGS.reset()
    with pytest.raises(ValueError, match="0.5, 0.5"):                                        # other weights are another list too
        train.main(["--teacher_dirs", a + "," + b, "--every_n", "30", "--train_dir", out])
    FLAGS.reset()
    with pytest.raises(ValueError, match="records no teacher list"):                         # a checkpoint of another kind of run
        train.main(["--teacher_dirs", a + "," + b, "--every_n", "30", "--train_dir", a])


def test_graph_refuses_before_it_allocates(monkeypatch):
    monkeypatch.setattr(distill, "HLstmTower", lambda *a, **k: pytest.fail("a tower was allocated"))
    G = distill.EnsembleDistillGraph
    with pytest.raises(ValueError, match="0 teachers"):
        G(4, teachers=(), device="cpu")
    with pytest.raises(ValueError, match="9 teachers"):
        G(4, teachers=[("teacher",)] * 9, device="cpu")
    with pytest.raises(ValueError, match="entry 0"):
        G(4, teachers=[("student", 10, "last"), ("teacher",)], device="cpu")
    with pytest.raises(ValueError, match="precision"):
        G(4, teachers=[("teacher",)], device="cpu", precision="high")
    with pytest.raises(ValueError, match="precision"):
        G(4, teachers=[("teacher",)], device="cpu", precision="split")
    with pytest.raises(ValueError, match="teacher_mode"):
        G(4, teachers=[("teacher",)], device="cpu", teacher_mode="median")
    with pytest.raises(ValueError, match="mean"):
        G(4, teachers=[("teacher",)] * 2, device="cpu", teacher_mode="max", teacher_weights=[0.5, 0.5])
    with pytest.raises(ValueError, match="2 teachers"):
        G(4, teachers=[("teacher",)] * 2, device="cpu", teacher_weights=[1.0])
    with pytest.raises(ValueError, match="rep_weight"):
        G(4, teachers=[("teacher",)] * 2, device="cpu", rep_weights=[0.0, 0.0])
    with pytest.raises(ValueError, match="every_n=7"):
        G(4, teachers=[("teacher",), ("student", 7, "last")], device="cpu")
    with pytest.raises(ValueError, match="distill_losses"):
        G(4, teachers=[("teacher",)], device="cpu", distill_losses=("mse",))
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    with pytest.raises(ValueError, match="not data parallel"):
        G(4, teachers=[("teacher",)], device="cpu")


# ---- the header -----------------------------------------------------------------------------------------------------------------------
def test_the_new_entry_is_declared_bound_and_has_a_host_wrapper():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "evc.h")).read()
    assert "int evc_distill_losses_ensemble(" in src and "evc_distill_losses_ensemble" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["evc_distill_losses_ensemble"]) == 22 and "evc_distill_losses_ensemble" in _lib.EXPORTS
    assert callable(ops.distill_losses_ensemble) and ops.DISTILL_MAX_TEACHERS == 8 == distill.EnsembleDistillGraph.MAX_TEACHERS
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), "evc_distill_losses_ensemble")
