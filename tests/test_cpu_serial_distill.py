"""Serial distillation without a GPU: the --teacher_dir / --distill_losses flags, every refused combination, and the checkpoint
round trip of a graph whose teacher has no Adam state."""
import os

import pytest
import torch

from efficientvideoclassification_youtube8m_amd import distill, train
from efficientvideoclassification_youtube8m_amd.flags import FLAGS


@pytest.fixture(autouse=True)
def _clean_flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


def test_flags_parse_and_default():
    assert FLAGS.teacher_dir == "" and FLAGS.distill_losses == "rep,pred,ce" == train.DEFAULT_DISTILL_LOSSES
    FLAGS.parse(["--teacher_dir", "/some/teacher/", "--distill_losses", "ce, rep"])
    assert FLAGS.teacher_dir == "/some/teacher/" and FLAGS.distill_losses == "rep,ce"             # canonical order
    FLAGS.parse(["--distill_losses=pred"])
    assert FLAGS.distill_losses == "pred"
    assert train.check_serial_flags() is True
    FLAGS.reset()
    assert train.check_serial_flags() is False


@pytest.mark.parametrize("words", ["", "rep,", "kl", "rep,pred,ce,rep", "rep pred", "REP"])
def test_distill_losses_rejects_unknown_empty_and_repeated_words(words):
    with pytest.raises(ValueError, match="distill_losses"):
        FLAGS.parse(["--distill_losses", words])
    with pytest.raises(ValueError, match="distill_losses"):
        distill.check_distill_losses(words)


def test_check_distill_losses_takes_sequences():
    assert distill.check_distill_losses(("ce", "rep")) == ("rep", "ce")
    assert distill.check_distill_losses(["pred"]) == ("pred",)
    assert distill.check_distill_losses("rep, pred ,ce") == distill.DistillGraph.DISTILL_LOSSES
    with pytest.raises(ValueError):
        distill.check_distill_losses(())


def test_refused_flag_combinations():
    FLAGS.parse(["--teacher_dir", "/t/", "--teacher_only", "True"])
    with pytest.raises(ValueError, match="--teacher_only"):
        train.check_serial_flags()
    FLAGS.reset()
    FLAGS.parse(["--teacher_dir", "/t/"])
    with pytest.raises(ValueError, match="--finetune"):
        train.check_serial_flags(finetune=True)
    with pytest.raises(ValueError, match="2 ranks"):
        train.check_serial_flags(world=2)
    FLAGS.reset()
    FLAGS.parse(["--distill_losses", "rep"])
    with pytest.raises(ValueError, match="needs --teacher_dir"):
        train.check_serial_flags()


def test_main_refuses_before_it_touches_a_device(monkeypatch):
    """train.main / train_finetune.main stop on these flags before torch.cuda is asked for anything."""
    from efficientvideoclassification_youtube8m_amd import train_finetune
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("a device was selected"))
    with pytest.raises(ValueError, match="--teacher_only"):
        train.main(["--teacher_dir", "/t/", "--teacher_only", "True"])
    FLAGS.reset()
    with pytest.raises(ValueError, match="--finetune"):
        train_finetune.main(["--teacher_dir", "/t/"])
    FLAGS.reset()
    with pytest.raises(ValueError, match="needs --teacher_dir"):
        train.main(["--distill_losses", "ce"])
    FLAGS.reset()
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="2 ranks"):
        train.main(["--teacher_dir", "/t/"])


def test_other_models_refuse_teacher_dir():
    from efficientvideoclassification_youtube8m_amd import frame_level_models, losses
    FLAGS.parse(["--teacher_dir", "/t/", "--model", "DbofModel"])
    with pytest.raises(ValueError, match="HierarchicalLstmModel"):
        train.build_graph(frame_level_models.DbofModel(), losses.CrossEntropyLoss(), 128, 4, 10, "cpu")


def test_graph_refuses_data_parallel_serial_mode_and_stray_loss_lists(monkeypatch):
    class TwoRanks:
        world, active, rank = 2, True, 0

        def __init__(self, *a, **k):
            pass
    monkeypatch.setattr(distill, "GradReducer", TwoRanks)
    with pytest.raises(ValueError, match="not data parallel"):
        distill.DistillGraph(4, every_n=10, mode="serial", device="cpu")
    with pytest.raises(ValueError, match="mode 'serial' only"):
        distill.DistillGraph(4, every_n=10, mode="teacher_student", device="cpu", distill_losses=("ce",))
    with pytest.raises(ValueError, match="distill_losses"):
        distill.DistillGraph(4, every_n=10, mode="serial", device="cpu", distill_losses=("ce", "mse"))


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
    mode, distill_losses, student_sampling = "serial", ("rep", "ce"), "uniform"

    def __init__(self, t_fill, s_fill):
        self.global_step = 0
        self.teacher, self.student = _Tower("model", False, t_fill), _Tower("model_student", True, s_fill)


def test_checkpoint_round_trip_with_a_teacher_without_adam_state(tmp_path):
    g = _Graph(1.5, 2.5)
    g.global_step, g.student.adam_t = 7, 7
    g.student.store.m.fill_(0.25)
    g.student.store.v.fill_(0.5)
    path = train.save_checkpoint(g, str(tmp_path), 0)
    assert os.path.basename(path) == "model.ckpt-7.pt"
    sd = torch.load(path)
    assert "model/adam" not in sd and "model_student/adam" in sd
    assert sd["distill_mode"] == "serial" and sd["distill_losses"] == "rep,ce" and sd["student_sampling"] == "uniform"
    h = _Graph(0.0, 0.0)
    train.restore_checkpoint(h, path)
    assert h.global_step == 7 and h.student.adam_t == 7 and h.teacher.adam_t == 0
    assert torch.equal(h.teacher.w, g.teacher.w) and torch.equal(h.student.w, g.student.w)
    assert torch.equal(h.student.store.m, g.student.store.m) and torch.equal(h.student.store.v, g.student.store.v)
    assert h.teacher.store.m is None
    # a checkpoint that DOES hold model/adam (a teacher+student run) restores into the frozen teacher without its moments
    sd["model/adam"] = {"t": 3, "m": torch.ones(6), "v": torch.ones(6)}
    torch.save(sd, path)
    train.restore_checkpoint(h, path)
    assert h.teacher.store.m is None and h.teacher.adam_t == 0


def test_load_frozen_teacher_names_the_directory(tmp_path):
    g = _Graph(0.0, 0.0)
    with pytest.raises(ValueError, match="no model.ckpt"):
        train.load_frozen_teacher(g, str(tmp_path))
    torch.save({"global_step": 0, "model_student/w": torch.ones(2, 3)}, str(tmp_path / "model.ckpt.pt"))
    with pytest.raises(ValueError) as e:
        train.load_frozen_teacher(g, str(tmp_path))
    assert str(tmp_path) in str(e.value) and "model/*" in str(e.value)
    torch.save({"global_step": 4, "model/w": torch.full((2, 3), 9.0), "model/adam": {"t": 4}}, str(tmp_path / "model.ckpt-4.pt"))
    assert train.load_frozen_teacher(g, str(tmp_path)).endswith("model.ckpt-4.pt")
    assert float(g.teacher.w[0, 0]) == 9.0 and g.global_step == 0
