"""The graphs of the two VLAD families (NeXtVLAD, NetVLAD) over their grid towers: serial distillation of a grid student against a
frozen grid teacher (GridDistillGraph) and the forward-only graph validate, inference, ensembles and cascades hold
where they hold a distill.EvalGraph (GridEvalGraph), and the host check of a checkpoint against the size flags.

The two base classes hold everything that does not depend on the family.  A family is a small mix-in that names its
tower class and says how its towers are checked, built and called per step; the four public graphs are one family next to one base.
distill re-exports every public name of this module.
"""
from __future__ import annotations

import numpy as np
import torch

from . import losses as losses_mod
from . import ops
from .distill import F32, DistillGraph, FramePlan, _resolve_label_loss, _StepGraph, check_distill_losses
from .towers import NetVladTower, NeXtVladTower, check_netvlad_frames, check_nextvlad_frames


def _world_of(process_group):
    """Ranks of a process group without touching a device (None: the default group when one is initialised, else 1)."""
    if process_group is not None and hasattr(process_group, "size"):
        return int(process_group.size())
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        return int(torch.distributed.get_world_size(process_group))
    return 1


def check_vlad_checkpoint(tower_cls, sd, scope, feature_size, vocab_size, sizes, what="the checkpoint", prefix="", clause=None, **shape_kw):
    """The ``scope``/* variables of the checkpoint dict ``sd`` against the size flags of a VLAD tower class (sizes: variable_shapes'
    arguments behind the feature size and the classes; shape_kw: its keywords), on the host: ValueError naming the first missing or
    mismatching variable and both shapes.  prefix goes in front of either message (train's "--teacher_dir DIR: "); clause replaces the
    family's "not a ... checkpoint" words."""
    for k, shp in tower_cls.checkpoint_shapes(feature_size, vocab_size, *sizes, **shape_kw).items():
        have = sd.get("%s/%s" % (scope, k))
        if not torch.is_tensor(have):
            raise ValueError("%s%s holds no variable %s/%s (%s)" % (prefix, what, scope, k, clause or tower_cls.NOT_A_CHECKPOINT))
        if tuple(have.shape) != shp:
            raise ValueError("%s%s/%s of %s has shape %s, the size flags (%s_* / --feature_sizes / --moe_num_mixtures) give %s"
                             % (prefix, scope, k, what, tuple(have.shape), tower_cls.FLAG, shp))


def check_nextvlad_checkpoint(sd, scope, feature_size, vocab_size, sizes, what="the checkpoint"):
    """check_vlad_checkpoint for a NeXtVLAD tower (sizes: cluster_size, hidden_size, groups, expansion, gating_reduction, num_mixtures)."""
    check_vlad_checkpoint(NeXtVladTower, sd, scope, feature_size, vocab_size, sizes, what)


def netvlad_checkpoint_gating(sd, scope):
    """Whether the ``scope``/* tower of the checkpoint dict ``sd`` has the context gate: it holds <scope>/gating_weights."""
    return torch.is_tensor(sd.get("%s/gating_weights" % scope))


def check_netvlad_checkpoint(sd, scope, feature_size, vocab_size, sizes, what="the checkpoint", gating=False):
    """check_vlad_checkpoint for a NetVLAD tower (sizes: cluster_size, hidden_size, num_mixtures).  gating: whether the caller's tower has
    the context gate (--netvlad_gating); a checkpoint that disagrees is a ValueError naming the flag and the variable found or missing."""
    gw = "%s/%s" % (scope, NetVladTower.GW)
    if netvlad_checkpoint_gating(sd, scope) != bool(gating):
        if gating:
            raise ValueError("--netvlad_gating True, but %s holds no variable %s (a tower trained without the context gate)" % (what, gw))
        raise ValueError("--netvlad_gating False, but %s holds the variable %s (a tower trained with the context gate)" % (what, gw))
    check_vlad_checkpoint(NetVladTower, sd, scope, feature_size, vocab_size, sizes, what, gating=bool(gating))


class _NeXtVladFamily:
    """NeXtVLAD towers in a grid graph: the grid is the uniform sub-sampling of the real frames; only a training
    student drops (dropout / dropout_seed), its mask a function of the step."""

    tower_cls = NeXtVladTower
    family = "nextvlad"
    dropout, dropout_seed = 0.0, 0

    def _check_grid(self, which, every_n, max_frames, precision):
        check_nextvlad_frames("grid", every_n, max_frames, world=self.world, precision=precision)

    def _tower_kw(self, which):
        return dict(dropout=self.dropout, dropout_seed=self.dropout_seed) if which == "student" else {}

    def _step_kw(self, x_raw, num_frames, keys, step):
        """(teacher's, student's) forward keywords of one step."""
        return {}, {"dropout_step": step}

    def _check_checkpoint(self, sd, tw):
        check_nextvlad_checkpoint(sd, tw.scope, self.F, self.V, self.sizes)


class _NetVladFamily:
    """NetVLAD towers in a grid graph: each tower on its --student_sampling word and seed (7.20) and with or without the
    context gate (7.21); student_sampling / sampling_seed / gating are the student's, teacher_* the teacher's."""

    tower_cls = NetVladTower
    family = "netvlad"

    def _set_words(self, student_sampling, sampling_seed, teacher_sampling, teacher_sampling_seed, gating, teacher_gating):
        self.student_sampling, self.sampling_seed = ops.check_student_sampling(student_sampling, "--student_sampling"), int(sampling_seed)
        self.teacher_sampling, self.teacher_sampling_seed = ops.check_student_sampling(teacher_sampling, "teacher_sampling"), int(teacher_sampling_seed)
        self.gating, self.teacher_gating = bool(gating), bool(teacher_gating)

    def _check_grid(self, which, every_n, max_frames, precision):
        check_netvlad_frames("grid", every_n, max_frames, world=self.world, precision=precision,
                             sampling=self.student_sampling if which == "student" else self.teacher_sampling)

    def _tower_kw(self, which):
        if which == "student":
            return dict(sampling=self.student_sampling, sampling_seed=self.sampling_seed, gating=self.gating)
        return dict(sampling=self.teacher_sampling, sampling_seed=self.teacher_sampling_seed, gating=self.teacher_gating)

    def _step_kw(self, x_raw, num_frames, keys, step):
        """(teacher's, student's) forward keywords of one step: none when every tower runs on the uniform grid; else the batch's
        ops.frame_change_keys - computed here, once, under a scored word when the caller has none - and the draw of "random", 0 for a
        tower that is not trained (the same frames for the same batching) and the step for the student."""
        words = [tw.sampling for tw in self._towers()]
        if all(w == "uniform" for w in words):
            return {}, {}
        if keys is None and any(w in ops.STUDENT_SAMPLING_SCORED for w in words):
            keys = ops.frame_change_keys(x_raw, num_frames)
        return dict(keys=keys, draw=0, row0=0), dict(keys=keys, draw=step, row0=0)

    def _check_checkpoint(self, sd, tw):
        check_netvlad_checkpoint(sd, tw.scope, self.F, self.V, self.sizes, gating=tw.gating)


class GridDistillGraph(_StepGraph):
    """Serial distillation over the grid towers of one VLAD family: a grid student (frames j * every_n of every video, scope
    'model_student') against a FROZEN grid teacher (every teacher_every_n-th real frame, scope 'model': forward only, batch norms on the
    checkpoint's moving statistics, no gradient store / moments / tape, never written).  One step on one stream: teacher forward, student
    forward, the loss section of DistillGraph's mode 'serial' (ops.distill_losses on the towers' `state` and predictions, the same
    scales), the student's backward with dL_REP/dstate joining the MoE head's gradient on `state`, and the update SingleTowerGraph.step
    performs (_StepGraph._update_tower on one rank); global_step += 1.  Reporting follows DistillGraph's serial mode (`out` keys,
    LOSS_SLOTS, loss_report), so train's loop needs no special case.  Every refusal is a ValueError before the device is touched."""

    LOSS_SLOTS = DistillGraph.LOSS_SLOTS
    DISTILL_LOSSES = DistillGraph.DISTILL_LOSSES
    mode = "serial"
    student_sampling = "uniform"                 # (the grid is the uniform sub-sampling of the real frames; checkpoint metadata)
    dp = False

    def _build(self, batch_size, sizes, every_n, teacher_every_n, feature_size, vocab_size, max_frames, base_learning_rate,
               learning_rate_decay, learning_rate_decay_examples, regularization_penalty, clip_gradient_norm, count_rep_twice, device, seed,
               process_group, precision, distill_losses, label_loss):
        """Everything behind the family's own checks: the shared refusals in their order, then the two towers.  sizes: the tower's size
        arguments behind (batch_size, max_frames, feature_size, vocab_size, iterations)."""
        name, family = type(self).__name__, self.tower_cls.FAMILY
        self.world = _world_of(process_group)
        if self.world > 1:
            raise ValueError("%s is not data parallel (process group of %d ranks): train the student against the "
                             "frozen teacher on one device" % (name, self.world))
        self.label_loss = _resolve_label_loss(label_loss, vocab_size)
        if not losses_mod.is_default(self.label_loss):
            raise ValueError("%s has CrossEntropyLoss built into its loss section (evc_distill_losses), not %s"
                             % (name, type(self.label_loss).__name__))
        if precision != "bf16":
            raise ValueError("%s: precision %r is refused, the %s tower has no such forward mode (bf16 only)" % (name, precision, family))
        self.distill_losses = check_distill_losses(distill_losses)
        for which, n in (("student", every_n), ("teacher", teacher_every_n)):     # (ValueError naming --every_n and its range)
            self._check_grid(which, n, max_frames, precision)
        self.B, self.every_n, self.teacher_every_n, self.precision = batch_size, int(every_n), int(teacher_every_n), precision
        self.lr0, self.lr_decay, self.lr_decay_examples = base_learning_rate, learning_rate_decay, learning_rate_decay_examples
        self.reg_pen, self.clip, self.pg = regularization_penalty, clip_gradient_norm, process_group
        self.rep_w = 2.0 if count_rep_twice else 1.0
        self.device = torch.device(device)
        self.global_step = 0
        args = (batch_size, max_frames, feature_size, vocab_size, 30) + tuple(sizes)
        self.teacher = self.tower_cls(*args, device=device, training=False, scope="model", seed=seed, frames="grid",
                                      every_n=self.teacher_every_n, **self._tower_kw("teacher"))
        self.student = self.tower_cls(*args, device=device, training=True, scope="model_student", seed=seed + 1, frames="grid",
                                      every_n=self.every_n, **self._tower_kw("student"))
        self.moe = self.student.moe
        self.fused_moe_update = True
        self.losses = torch.zeros(8, dtype=F32, device=self.device)
        self._dp_s = self._ds_s = None

    def _towers(self):
        return [self.teacher, self.student]

    def consolidate(self):
        """Nothing is sharded on one rank (kept for train's checkpoint path)."""

    def state_dict(self):
        """Both scopes: model/* (the frozen teacher, the bits it was loaded with) and model_student/*."""
        out = self.teacher.state_dict()
        out.update(self.student.state_dict())
        return out

    def label_grads(self):
        """The student's dL/dpred buffer of the last step (its L_CE and L_PRED gradient), as DistillGraph names it."""
        return {} if self._dp_s is None else {"student": self._dp_s}

    def state_grad(self):
        """The dL_REP/dstate buffer of the last step (None before the first).  For tests and debugging."""
        return self._ds_s

    @property
    def losses_for_report(self):
        return self.losses

    def loss_report(self, losses=None):
        v = (self.losses if losses is None else losses).tolist()
        return {k: v[i] for i, k in enumerate(self.LOSS_SLOTS)}

    def step(self, x_raw, labels_u8, num_frames, apply=True, num_frames_host=None):
        """x_raw [B,T,F] uint8 or float32, labels_u8 [B,V], num_frames [B] int32 (num_frames_host: the same counts on the host - both
        towers lay their packed rows out from them; read back from the device when not given).  All launches on the caller's stream."""
        B, V = labels_u8.shape
        tt, ts = self.teacher, self.student
        if num_frames_host is None:
            num_frames_host = num_frames.cpu().numpy()
        if self._dp_s is None or self._dp_s.shape[0] != B:
            self._dp_s = torch.empty((B, V), dtype=F32, device=self.device)
            self._ds_s = torch.empty((B, ts.Hd), dtype=F32, device=self.device)
        tkw, skw = self._step_kw(x_raw, num_frames, None, self.global_step)
        t_pred = tt.forward(x_raw, num_frames, num_frames_host=num_frames_host, is_training=False, **tkw)
        s_pred = ts.forward(x_raw, num_frames, num_frames_host=num_frames_host, **skw)
        on = self.distill_losses
        self.losses.zero_()
        ops.distill_losses(t_pred, tt.rowsum, s_pred, ts.rowsum, labels_u8, tt.state, ts.state, self.losses, self._dp_s, self._ds_s,
                           g_ce=(1.0 / B) if "ce" in on else 0.0, g_kl=1.0 if "pred" in on else 0.0,
                           g_rep=self.rep_w if "rep" in on else 0.0)
        fuse, fused_names = self._fuse_moe_update(apply, self.moe, ts.precision)
        ts.backward(self._dp_s, moe_weight_grads=not fuse, dstate=self._ds_s)
        if apply:
            self._update_tower(ts, self.moe, B, fuse, fused_names)
        return dict(predictions=t_pred, teacher_state=tt.state, loss=self.losses[0], student_predictions=s_pred, student_state=ts.state,
                    num_frames_student=torch.from_numpy(ts.plan.k), student_loss_state=self.losses[1], pred_loss=self.losses[2],
                    student_label_loss=self.losses[3], global_step=self.global_step)


class NeXtVladDistillGraph(_NeXtVladFamily, GridDistillGraph):
    """GridDistillGraph for the NeXtVLAD family: `state` is the gated hidden vector `out`, and dL_REP/dstate joins the
    MoE head's gradient there.  dropout / dropout_seed: the STUDENT's drop rate before its hidden layer, its mask a
    function of global_step; the frozen teacher never drops."""

    def __init__(self, batch_size, every_n=10, teacher_every_n=1, feature_size=1152, vocab_size=4716, max_frames=300, cluster_size=64,
                 hidden_size=1024, groups=8, expansion=2, gating_reduction=8, num_mixtures=2, base_learning_rate=0.001,
                 learning_rate_decay=1.0, learning_rate_decay_examples=4000000, regularization_penalty=2.0, clip_gradient_norm=1.0,
                 count_rep_twice=True, device="cuda:0", seed=7, process_group=None, precision="bf16",
                 distill_losses=GridDistillGraph.DISTILL_LOSSES, label_loss=None, dropout=0.0, dropout_seed=0):
        self.dropout, self.dropout_seed = ops.check_dropout_rate(dropout), dropout_seed      # (before the device is touched)
        self._build(batch_size, (cluster_size, hidden_size, groups, expansion, gating_reduction, num_mixtures), every_n, teacher_every_n,
                    feature_size, vocab_size, max_frames, base_learning_rate, learning_rate_decay, learning_rate_decay_examples,
                    regularization_penalty, clip_gradient_norm, count_rep_twice, device, seed, process_group, precision, distill_losses,
                    label_loss)


class NetVladDistillGraph(_NetVladFamily, GridDistillGraph):
    """GridDistillGraph for the NetVLAD family: `state` is h6 = relu6(hidden1_bn(hid)), and dL_REP/dstate joins the MoE
    head's gradient in front of hidden1_bn's relu6 mask.

    student_sampling / sampling_seed: the --student_sampling word of the STUDENT, "random" drawn with draw =
    global_step and row0 = 0.  teacher_sampling / teacher_sampling_seed: what the frozen teacher's checkpoint records when that tower was
    itself trained on selected frames; it runs on them with draw 0, as evaluation does.  Under a scored word the batch's
    ops.frame_change_keys are computed once and handed to both towers.

    gating / teacher_gating: the context gate of the student (--netvlad_gating) and of the frozen teacher (what its
    checkpoint holds).  They may differ: both states are [B, H], and L_REP and dstate are on `state`, the gated vector where there is a gate."""

    def __init__(self, batch_size, every_n=10, teacher_every_n=1, feature_size=1152, vocab_size=4716, max_frames=300, cluster_size=64,
                 hidden_size=1024, num_mixtures=2, base_learning_rate=0.001, learning_rate_decay=1.0,
                 learning_rate_decay_examples=4000000, regularization_penalty=2.0, clip_gradient_norm=1.0, count_rep_twice=True,
                 device="cuda:0", seed=7, process_group=None, precision="bf16", distill_losses=GridDistillGraph.DISTILL_LOSSES,
                 label_loss=None, student_sampling="uniform", sampling_seed=0, teacher_sampling="uniform", teacher_sampling_seed=0,
                 gating=False, teacher_gating=False):
        self._set_words(student_sampling, sampling_seed, teacher_sampling, teacher_sampling_seed, gating, teacher_gating)
        self._build(batch_size, (cluster_size, hidden_size, num_mixtures), every_n, teacher_every_n, feature_size, vocab_size, max_frames,
                    base_learning_rate, learning_rate_decay, learning_rate_decay_examples, regularization_penalty, clip_gradient_norm,
                    count_rep_twice, device, seed, process_group, precision, distill_losses, label_loss)


class GridEvalGraph(_StepGraph):
    """Forward-only graph over the grid towers of one VLAD family with EvalGraph's interface: restore(state_dict) and
    step(x_raw, labels_u8, num_frames, num_frames_host=None, keys=None) -> dict with predictions, loss, num_frames, so that validate (and,
    for NeXtVLAD, inference, EnsembleGraph and CascadeGraph) hold it where they hold an EvalGraph.  tower: 'teacher' (scope model, on
    every `every_n`-th real frame), 'student' (scope model_student, the same) or 'both' (the student served at every_n, the teacher run
    too at teacher_every_n: validate's student_state_loss).  The towers are forward-only grid towers (training=False: the moving
    statistics), bf16 only, on the caller's stream.  The buffers are allocated once at batch_size: a shorter batch allocates nothing.

    A family sets loss_slots (the size of `losses` for one tower, for 'both') and full_report (whether a lone teacher's outputs and
    student_label_loss are in the returned dict, or only under 'both')."""

    loss_slots = (1, 2)
    full_report = False
    student_sampling = "uniform"

    def _check_tower_word(self, tower):
        if tower not in ("teacher", "student", "both"):
            raise ValueError("%s: tower %r (teacher | student | both)" % (type(self).__name__, tower))

    def _check_grids(self, tower, every_n, teacher_every_n, max_frames, precision):
        for which, n in [("student", every_n)] + ([("teacher", teacher_every_n)] if tower == "both" else []):
            self._check_grid(which, n, max_frames, precision)                     # (before the device is touched)

    def _build(self, batch_size, sizes, tower, every_n, teacher_every_n, feature_size, vocab_size, max_frames, device, precision, seed):
        """The towers the word names, behind the family's checks.  sizes: as GridDistillGraph._build's."""
        self.tower, self.every_n, self.teacher_every_n = tower, int(every_n), int(teacher_every_n if tower == "both" else every_n)
        self.batch_size, self.max_frames, self.precision = batch_size, max_frames, precision
        self.sizes = tuple(sizes)
        self.F, self.V = feature_size, vocab_size
        self.device = torch.device(device)
        args = (batch_size, max_frames, feature_size, vocab_size, 30) + self.sizes
        self.teacher = self.student = None
        if tower != "student":
            self.teacher = self.tower_cls(*args, device=device, training=False, scope="model", seed=seed, frames="grid",
                                          every_n=self.teacher_every_n, **self._tower_kw("teacher"))
        if tower != "teacher":
            self.student = self.tower_cls(*args, device=device, training=False, scope="model_student", seed=seed + 1, frames="grid",
                                          every_n=self.every_n, **self._tower_kw("student"))
        self.losses = torch.zeros(self.loss_slots[tower == "both"], dtype=F32, device=self.device)

    def _towers(self):
        return [tw for tw in (self.teacher, self.student) if tw is not None]

    def restore(self, state_dict):
        """Each tower's variables and moving statistics by name, after the host check of every tower's shapes against the graph's sizes
        (nothing is loaded when a check fails)."""
        for tw in self._towers():
            self._check_checkpoint(state_dict, tw)
        for tw in self._towers():
            tw.load_state_dict(state_dict)

    def _select(self, nh, b):
        """The videos the towers serve, as forward's sel (None: all of the batch)."""
        return None

    def _run(self, name, tw, x_raw, num_frames, nh, sel, kw):
        """(predictions [b, V], state [b, H]) of one tower for this batch."""
        return tw.forward(x_raw, num_frames, is_training=False, num_frames_host=nh, **kw), tw.state

    def step(self, x_raw, labels_u8, num_frames, num_frames_host=None, keys=None):
        """x_raw [b, T, F] uint8 or float32, b <= batch_size; labels_u8 [b, V]; num_frames [b] int32 (num_frames_host: the same counts
        on the host; read back from the device when not given).  keys is EvalGraph's argument: the batch's ops.frame_change_keys, read
        by a family with scored sampling words alone."""
        b = int(x_raw.shape[0])
        if b > self.batch_size:
            raise ValueError("%s: a batch of %d videos, the graph was built for %d" % (type(self).__name__, b, self.batch_size))
        if num_frames_host is None:
            num_frames_host = num_frames.cpu()
        nh = np.asarray(num_frames_host, dtype=np.int64).reshape(-1)
        sel = self._select(nh, b)
        tkw, skw = self._step_kw(x_raw, num_frames, keys, 0)
        out = {}
        if self.teacher is not None:
            pred, t_state = self._run("teacher", self.teacher, x_raw, num_frames, nh, sel, tkw)
            if self.full_report or self.tower == "both":
                out.update(teacher_predictions=pred, teacher_state=t_state)
        if self.student is not None:
            pred, s_state = self._run("student", self.student, x_raw, num_frames, nh, sel, skw)
            out["student_state"] = s_state
        served = self.student if self.student is not None else self.teacher
        self.losses.zero_()
        self.label_loss.fused(pred, labels_u8, self.losses[0:1])
        if self.tower == "both":
            ops.rep_loss(t_state, s_state, self.losses[1:2])
            out["student_state_loss"] = self.losses[1]
        if self.full_report or self.tower == "both":
            out["student_label_loss"] = self.losses[0]
        k = np.zeros(b, np.int32)
        k[sel if sel is not None else slice(None)] = served.plan.k
        out.update(predictions=pred, loss=self.losses[0], num_frames=torch.from_numpy(k))
        return out


class NeXtVladEvalGraph(_NeXtVladFamily, GridEvalGraph):
    """GridEvalGraph for the NeXtVLAD family (MFMA aggregation in the forward-only towers).

    compact: the towers run on the videos that have a frame.  sel = the ascending list of videos with num_frames_host > 0; when it is
    shorter than the batch the towers serve those b' videos of the unchanged batch (NeXtVladTower.forward(sel=...)) and
    ops.scatter_rows puts their rows back: predictions / states are [b, .] with zeros in the rows of videos without a frame.  With
    compact=False such a video runs through the tower after the aggregation like any other (its V is zero) and its row holds what the
    head makes of that.  A served subset allocates nothing either.  keys is not read."""

    loss_slots = (4, 4)
    full_report = True

    def __init__(self, batch_size, tower="teacher", every_n=1, teacher_every_n=1, feature_size=1152, vocab_size=4716, max_frames=300,
                 cluster_size=64, hidden_size=1024, groups=8, expansion=2, gating_reduction=8, num_mixtures=2, device="cuda:0",
                 precision="bf16", student_sampling="uniform", label_loss=None, compact=True, seed=7):
        self._check_tower_word(tower)
        if student_sampling != "uniform":
            raise ValueError("--student_sampling %s with --model NeXtVLADModel: a grid tower reads every every_n-th real frame (uniform); "
                             "the other selections are not built for this family" % (student_sampling,))
        if precision != "bf16":
            raise ValueError("--precision %s with --model NeXtVLADModel: the NeXtVLAD tower has no such forward mode (bf16 only)" % (precision,))
        self.label_loss = _resolve_label_loss(label_loss, vocab_size)
        self._check_grids(tower, every_n, teacher_every_n, max_frames, precision)
        self.compact = bool(compact)
        self._build(batch_size, (cluster_size, hidden_size, groups, expansion, gating_reduction, num_mixtures), tower, every_n,
                    teacher_every_n, feature_size, vocab_size, max_frames, device, precision, seed)
        self.frames = FramePlan()                  # (no H-LSTM student: scored_sampling() is False for this member)
        # what a compacted step hands out: [batch_size, .] once, rows of videos without a frame zero
        self._wide = {}
        if self.compact:
            for name, tw in (("teacher", self.teacher), ("student", self.student)):
                if tw is not None:
                    self._wide[name] = (torch.zeros((batch_size, vocab_size), dtype=F32, device=self.device),
                                        torch.zeros((batch_size, hidden_size), dtype=F32, device=self.device))

    def _select(self, nh, b):
        if self.compact:
            have = np.flatnonzero(nh > 0)
            if 0 < have.size < b:
                return have.astype(np.int32)
        return None

    def _run(self, name, tw, x_raw, num_frames, nh, sel, kw):
        """With sel, the rows of the other videos are zeros."""
        pred = tw.forward(x_raw, num_frames, is_training=False, num_frames_host=nh, sel=sel)
        if sel is None:
            return pred, tw.state
        b, n = x_raw.shape[0], int(sel.shape[0])
        wide_pred, wide_state = (t[:b] for t in self._wide[name])
        wide_pred.zero_()
        wide_state.zero_()
        ops.scatter_rows(pred, tw.sel[:n], wide_pred)
        ops.scatter_rows(tw.state, tw.sel[:n], wide_state)
        return wide_pred, wide_state


class NetVladEvalGraph(_NetVladFamily, GridEvalGraph):
    """GridEvalGraph for the NetVLAD family.  No row compaction: a video without a frame runs through the head with
    V = 0 like any other and its row holds what the head makes of that.

    student_sampling / sampling_seed: the --student_sampling word the SERVED tower runs on (the student, or the teacher
    when it is the only tower), as EvalGraph serves its student on the flag; "random" is drawn with draw 0 and row0 0, the same frames
    for the same batching.  With tower='both' the teacher runs on teacher_sampling / teacher_sampling_seed, what its checkpoint records.

    gating / teacher_gating: the context gate of the served tower and, with tower='both', of the teacher - what the
    checkpoint's own variables say (validate.netvlad_source), never the flag."""

    def __init__(self, batch_size, every_n=1, feature_size=1152, vocab_size=4716, max_frames=300, cluster_size=64, hidden_size=1024,
                 num_mixtures=2, device="cuda:0", precision="bf16", label_loss=None, seed=7, tower="teacher", teacher_every_n=1,
                 student_sampling="uniform", sampling_seed=0, teacher_sampling="uniform", teacher_sampling_seed=0, gating=False,
                 teacher_gating=False):
        self._check_tower_word(tower)
        if tower != "both":                                           # (the one tower is the served one)
            teacher_sampling, teacher_sampling_seed, teacher_gating = student_sampling, sampling_seed, gating
        self._set_words(student_sampling, sampling_seed, teacher_sampling, teacher_sampling_seed, gating, teacher_gating)
        self._check_grids(tower, every_n, teacher_every_n, max_frames, precision)
        self.label_loss = _resolve_label_loss(label_loss, vocab_size)
        self._build(batch_size, (cluster_size, hidden_size, num_mixtures), tower, every_n, teacher_every_n, feature_size, vocab_size,
                    max_frames, device, precision, seed)
