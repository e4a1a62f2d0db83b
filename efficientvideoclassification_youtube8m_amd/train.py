"""Training binary with the reference's flag surface (cs/train.py, and
cs/train_finetune.py via ``--finetune``):

    python -m efficientvideoclassification_youtube8m_amd.train \
        --train_data_pattern synthetic --train_dir ./model_HLSTM_TeaStud_every10_train/ \
        --frame_features True --feature_names "rgb, audio" --feature_sizes "1024, 128" \
        --model "HierarchicalLstmModel" --gpu 0 --batch_size 256 --num_inputs_to_lstm 20 \
        --lstm_layers 2 --start_new_model True --num_epochs 1 --every_n 10      # = run_train.sh:6

What is kept: flag names/defaults/syntax (flags.py), class lookup by name
(``find_class_by_name``, cs/train.py:179-182), the teacher+student graph
(``build_graph`` -> distill.DistillGraph), the per-step log line
(cs/train.py:528-533), global_step += 2, resume-unless-``--start_new_model``.
What is replaced: TF Supervisor/queue runners -> a plain loop; TF checkpoints ->
``torch.save`` of a TF-named state dict (model.ckpt-<step>.pt, max_to_keep=1);
TFRecord input -> readers.py (native parser, uint8 feed, pinned staging); the pattern
"synthetic" generates random uint8 videos on the device instead.
Serial distillation (not a reference mode; the paper's second way to train a student): ``--teacher_dir DIR`` trains the
student against the frozen teacher of DIR's latest checkpoint (distill.DistillGraph mode "serial").
``--serial_student_dirs A/,B/,...`` next to it trains up to 8 students in ONE run against one forward of that teacher per batch
(distill.SerialStudentsGraph): one checkpoint directory per student, each what a run of its own would have written.
``--teacher_dirs A/,B/,...`` trains ONE student against the combination of up to 8 frozen teachers - an ensemble folded back into one
small model, or a teacher next to the teaching assistants distilled from it (distill.EnsembleDistillGraph).
``--teacher_preds_pattern GLOB`` trains the student ALONE against 1 .. 8 teacher prediction files (what inference --output_file writes):
the train_finetune step with the loss section evc_distill_losses_sparse, no teacher tower in memory (distill.OfflineDistillGraph,
DESIGN.md 7.11).
``--model NeXtVLADModel --nextvlad_frames grid --every_n N --teacher_dir DIR`` trains a grid student against the frozen grid teacher of
DIR's latest checkpoint, which runs on the frames its checkpoint records (vlad_graphs.NeXtVladDistillGraph);
``--model NetVLADModel --netvlad_frames grid --every_n N --teacher_dir DIR`` does the same for the NetVLAD family
(vlad_graphs.NetVladDistillGraph).  With ``--student_sampling WORD`` a NetVLAD grid tower - alone or as that student - runs on
the frames the word selects instead of the grid.
Multi-GPU: launch with ``python -m torch.distributed.run --nproc-per-node N``;
``--gpu`` is then ignored in favour of LOCAL_RANK.
"""
from __future__ import annotations

import glob
import logging
import os
import sys
import time

import numpy as np
import torch

from . import eval_util, frame_level_models, losses, ops, readers, video_level_models
from .distill import DistillGraph, EnsembleDistillGraph, OfflineDistillGraph, SerialStudentsGraph, SingleTowerGraph
from .flags import FLAGS, GetListOfFeatureNamesAndSizes
from .towers import DbofTower, LogisticTower, NetVladTower, NeXtVladTower, check_netvlad_frames, check_netvlad_gating, check_nextvlad_frames
from .vlad_graphs import (GridDistillGraph, NetVladDistillGraph, NeXtVladDistillGraph, check_netvlad_checkpoint, check_vlad_checkpoint,
                          netvlad_checkpoint_gating)

NUM_CLASSES = 4716       # readers.YT8MFrameFeatureReader default num_classes (cs/readers.py:121)


def find_class_by_name(name, modules):
    """Searches the provided modules for the named class and returns it (cs/train.py:179-182)."""
    found = [getattr(module, name, None) for module in modules]
    return next(a for a in found if a)


def _apply_precision(tw):
    """--precision for the single-tower models: towers with a split-bf16 forward take it (DbofTower, LogisticTower); a tower
    without one (NetVladTower, NeXtVladTower) refuses anything but 'bf16' instead of silently ignoring the flag."""
    if FLAGS.precision != "bf16":
        if "high" not in getattr(tw, "PRECISIONS", ()):
            raise ValueError("--precision %s: %s has no such forward mode" % (FLAGS.precision, type(tw).__name__))
        tw.set_precision(FLAGS.precision)


DEFAULT_DISTILL_LOSSES = "rep,pred,ce"


_UNSET = object()


def check_serial_flags(finetune=False, world=1, students=_UNSET):
    """--teacher_dir / --distill_losses against the flags and the launch they exclude (all ValueError, before anything touches the device).
    Returns True when the flags ask for serial distillation."""
    serial = bool(FLAGS.teacher_dir)
    if students is _UNSET:
        serial_students(finetune, world)    # --serial_student_dirs and its lists: every refusal of theirs, before the rest
    if not serial:
        if FLAGS.distill_losses != DEFAULT_DISTILL_LOSSES and not FLAGS.teacher_dirs.strip() and not FLAGS.teacher_preds_pattern:
            raise ValueError("--distill_losses %s needs --teacher_dir: it selects the student's losses of serial distillation "
                             "(the teacher+student graph trains on all of them)" % FLAGS.distill_losses)
        return False
    if getattr(FLAGS, "teacher_only", False):
        raise ValueError("--teacher_dir %s with --teacher_only: a frozen teacher cannot be the tower that is trained" % FLAGS.teacher_dir)
    if finetune:
        raise ValueError("--teacher_dir %s with --finetune: train_finetune trains the student on L_CE alone, without a teacher "
                         "(serial distillation is train --teacher_dir)" % FLAGS.teacher_dir)
    if world > 1:
        raise ValueError("--teacher_dir %s on %d ranks: serial distillation is not data parallel yet, run it on one device" %
                         (FLAGS.teacher_dir, world))
    return True


def serial_students(finetune=False, world=1):
    """--serial_student_dirs / --serial_every_n / --serial_sampling / --serial_losses: None when no directories are given, else
    {"dirs", "every_n", "sampling", "losses"} with one entry per student ('' lists filled from --every_n / --student_sampling /
    --distill_losses).  Every refused combination is a ValueError here, before anything touches the device."""
    from .distill import check_distill_losses, validate_every_n
    dirs = [d.strip() for d in FLAGS.serial_student_dirs.split(",") if d.strip()]
    lists = {"serial_every_n": FLAGS.serial_every_n, "serial_sampling": FLAGS.serial_sampling, "serial_losses": FLAGS.serial_losses}
    if not dirs:
        stray = [k for k, v in lists.items() if v]
        if stray or FLAGS.serial_student_dirs.strip():
            raise ValueError("--%s needs --serial_student_dirs (one train directory per student)" % (stray[0] if stray else "serial_student_dirs"))
        return None
    K = len(dirs)
    what = "--serial_student_dirs %s" % FLAGS.serial_student_dirs
    if K > SerialStudentsGraph.MAX_STUDENTS:
        raise ValueError("%s: %d directories, at most %d students share a teacher's forward" % (what, K, SerialStudentsGraph.MAX_STUDENTS))
    norm = [os.path.normpath(os.path.abspath(d)) for d in dirs]
    twice = sorted({d for d, n in zip(dirs, norm) if norm.count(n) > 1})
    if twice:
        raise ValueError("%s: a directory is named more than once (%s): every student writes its own" % (what, ", ".join(twice)))
    if not FLAGS.teacher_dir:
        raise ValueError("%s needs --teacher_dir: the students are trained against its frozen teacher" % what)
    if getattr(FLAGS, "teacher_only", False):
        raise ValueError("%s with --teacher_only: a frozen teacher cannot be the tower that is trained" % what)
    if finetune:
        raise ValueError("%s with --finetune: train_finetune trains one student on L_CE alone, without a teacher" % what)
    if world > 1:
        raise ValueError("%s on %d ranks: serial distillation is not data parallel yet, run it on one device" % (what, world))
    if FLAGS.model != "HierarchicalLstmModel":
        raise ValueError("%s: serial distillation is built for HierarchicalLstmModel, not %s" % (what, FLAGS.model))
    if FLAGS.precision != "bf16":
        raise ValueError("%s with --precision %s: several students share a teacher's forward in bf16 only" % (what, FLAGS.precision))
    out = {"dirs": dirs}
    for key, flag, default in (("every_n", "serial_every_n", str(FLAGS.every_n)), ("sampling", "serial_sampling", FLAGS.student_sampling),
                               ("losses", "serial_losses", FLAGS.distill_losses.replace(",", "+"))):
        vals = [v.strip() for v in lists[flag].split(",")] if lists[flag] else [default] * K
        if len(vals) != K:
            raise ValueError("--%s %s: %d entries for the %d directories of %s" % (flag, lists[flag], len(vals), K, what))
        out[key] = vals
    out["every_n"] = [int(e) for e in out["every_n"]]
    for e in out["every_n"]:
        validate_every_n(e, 5, FLAGS.max_num_frames)
    out["losses"] = [check_distill_losses(e.split("+")) for e in out["losses"]]
    return out


TEACHER_LIST_FLAGS = ("teacher_towers", "teacher_every_n", "teacher_sampling", "teacher_weights", "teacher_rep_weights")


def ensemble_teachers(finetune=False, world=1):
    """--teacher_dirs and its lists: None when no directories are given, else {"dirs", "towers" (auto | teacher | student words),
    "every_n", "sampling", "mode", "weights" (float32 [J], None in mode max), "rep_weights" (float32 [J])}, one entry per teacher ('' lists
    filled from --every_n / --student_sampling, the weights with float32(1) / float32(J), the rep weights with 1, 0, ..., 0).  Every
    refused combination is a ValueError here, before anything touches the device."""
    from .distill import validate_every_n
    words = lambda text: [w.strip() for w in text.split(",")] if text.strip() else []
    dirs = words(FLAGS.teacher_dirs)
    lists = {k: words(getattr(FLAGS, k)) for k in TEACHER_LIST_FLAGS}
    if not dirs:
        # (--teacher_weights - like --teacher_mode - also combines the files of --teacher_preds_pattern: offline_teachers)
        stray = [k for k, v in lists.items() if v and not (k == "teacher_weights" and FLAGS.teacher_preds_pattern)]
        if stray:
            raise ValueError("--%s needs --teacher_dirs (the frozen teachers the student is trained against)" % stray[0])
        return None
    J = len(dirs)
    what = "--teacher_dirs %s" % FLAGS.teacher_dirs
    if J > EnsembleDistillGraph.MAX_TEACHERS or "" in dirs:
        raise ValueError("%s: %d entries (1 .. %d, none empty)" % (what, J, EnsembleDistillGraph.MAX_TEACHERS))
    if FLAGS.teacher_dir:
        raise ValueError("%s with --teacher_dir %s: one frozen teacher (--teacher_dir) or several (--teacher_dirs), not both" % (what, FLAGS.teacher_dir))
    if FLAGS.serial_student_dirs.strip():
        raise ValueError("%s with --serial_student_dirs: several students against several teachers in one run is not built" % what)
    if getattr(FLAGS, "teacher_only", False):
        raise ValueError("%s with --teacher_only: frozen teachers cannot be the tower that is trained" % what)
    if finetune:
        raise ValueError("%s with --finetune: train_finetune trains the student on L_CE alone, without a teacher" % what)
    if world > 1:
        raise ValueError("%s on %d ranks: ensemble distillation is not data parallel yet, run it on one device" % (what, world))
    if FLAGS.model != "HierarchicalLstmModel":
        raise ValueError("%s: ensemble distillation is built for HierarchicalLstmModel, not --model %s" % (what, FLAGS.model))
    if FLAGS.label_loss != "CrossEntropyLoss":
        raise ValueError("%s with --label_loss %s: ensemble distillation has CrossEntropyLoss built into its loss kernel "
                         "(evc_distill_losses_ensemble)" % (what, FLAGS.label_loss))
    if FLAGS.precision != "bf16":
        raise ValueError("%s with --precision %s: the teachers share their input image in bf16 only" % (what, FLAGS.precision))
    if FLAGS.teacher_mode not in ops.ENSEMBLE_MODES:
        raise ValueError("--teacher_mode %r (max | mean)" % FLAGS.teacher_mode)
    for key in TEACHER_LIST_FLAGS:
        if lists[key] and len(lists[key]) != J:
            raise ValueError("--%s %s: %d entries for the %d directories of %s" % (key, getattr(FLAGS, key), len(lists[key]), J, what))
    towers = lists["teacher_towers"] or ["auto"] * J
    for t in towers:
        if t not in ("auto", "teacher", "student"):
            raise ValueError("--teacher_towers: %r (auto | teacher | student)" % t)
    if towers[0] == "student":
        raise ValueError("--teacher_towers %s: entry 0 of --teacher_dirs is the model/* of the checkpoint, a teacher tower" % FLAGS.teacher_towers)
    try:
        every_n = [int(e) for e in lists["teacher_every_n"]] if lists["teacher_every_n"] else [FLAGS.every_n] * J
    except ValueError:
        raise ValueError("--teacher_every_n %r: a comma list of integers, one per --teacher_dirs entry" % FLAGS.teacher_every_n)
    sampling = [ops.check_student_sampling(w, "--teacher_sampling") for w in lists["teacher_sampling"]] or [FLAGS.student_sampling] * J
    for t, e in zip(towers, every_n):
        if t == "student":
            validate_every_n(e, 5, FLAGS.max_num_frames)
    validate_every_n(FLAGS.every_n, 5, FLAGS.max_num_frames)
    weights = None
    if lists["teacher_weights"] and FLAGS.teacher_mode != "mean":
        raise ValueError("--teacher_weights needs --teacher_mode mean (max has no weights)")
    try:
        if FLAGS.teacher_mode == "mean":
            weights = (np.asarray([float(x) for x in lists["teacher_weights"]], np.float32) if lists["teacher_weights"]
                       else np.full(J, np.float32(1) / np.float32(J), np.float32))
        rep = np.asarray([float(x) for x in lists["teacher_rep_weights"]] if lists["teacher_rep_weights"] else [1.0] + [0.0] * (J - 1), np.float32)
    except ValueError:
        raise ValueError("--teacher_weights %r / --teacher_rep_weights %r: comma lists of numbers" % (FLAGS.teacher_weights, FLAGS.teacher_rep_weights))
    if not rep.any():
        raise ValueError("--teacher_rep_weights %s: every weight is 0 (leave L_REP out with --distill_losses instead)" % FLAGS.teacher_rep_weights)
    return dict(dirs=dirs, towers=towers, every_n=every_n, sampling=sampling, mode=FLAGS.teacher_mode, weights=weights, rep_weights=rep)


OFFLINE_DISTILL_LOSSES = "pred,ce"


def offline_teachers(finetune=False, world=1, argv=None):
    """--teacher_preds_pattern: None when it is not set, else {"files" (sorted paths), "names" (their base names), "mode", "weights"
    (float32 [F], None in mode max), "losses" (the --distill_losses tuple; its default under this flag is pred,ce)}.  argv: the command
    line, to tell a --distill_losses that was given from the flag's default.  Every refused combination is a ValueError that names both
    flags, here, before a file is parsed or the device is touched."""
    from .distill import check_distill_losses, validate_every_n
    pattern = FLAGS.teacher_preds_pattern
    if not pattern:
        return None
    what = "--teacher_preds_pattern %s" % pattern
    if FLAGS.teacher_dir:
        raise ValueError("%s with --teacher_dir %s: the teacher is a set of prediction files or a frozen tower, not both (mixing them in "
                         "one step is not built)" % (what, FLAGS.teacher_dir))
    if FLAGS.teacher_dirs.strip():
        raise ValueError("%s with --teacher_dirs %s: the teachers are prediction files or frozen towers, not both (mixing them in one "
                         "step is not built)" % (what, FLAGS.teacher_dirs))
    if FLAGS.serial_student_dirs.strip():
        raise ValueError("%s with --serial_student_dirs: several students against prediction files in one run is not built" % what)
    if getattr(FLAGS, "teacher_only", False):
        raise ValueError("%s with --teacher_only: offline distillation trains the student alone, there is no teacher tower" % what)
    if FLAGS.label_loss != "CrossEntropyLoss":
        raise ValueError("%s with --label_loss %s: offline distillation has CrossEntropyLoss built into its loss kernel "
                         "(evc_distill_losses_sparse)" % (what, FLAGS.label_loss))
    if finetune:
        raise ValueError("%s with train_finetune (--finetune): train_finetune trains the student on L_CE alone, without a teacher "
                         "(offline distillation is train --teacher_preds_pattern)" % what)
    if FLAGS.train_data_pattern in ("", "synthetic"):
        raise ValueError("%s with --train_data_pattern %r: synthetic training data has no video ids to look up in the files" %
                         (what, FLAGS.train_data_pattern))
    if world > 1:
        raise ValueError("%s on %d ranks: offline distillation is not data parallel yet, run it on one device" % (what, world))
    if FLAGS.model != "HierarchicalLstmModel":
        raise ValueError("%s: offline distillation is built for HierarchicalLstmModel, not --model %s" % (what, FLAGS.model))
    if FLAGS.teacher_mode not in ops.ENSEMBLE_MODES:
        raise ValueError("--teacher_mode %r (max | mean)" % FLAGS.teacher_mode)
    given = argv is not None and any(a == "--distill_losses" or a.startswith("--distill_losses=") for a in argv)
    words = FLAGS.distill_losses if (given or FLAGS.distill_losses != DEFAULT_DISTILL_LOSSES) else OFFLINE_DISTILL_LOSSES
    on = check_distill_losses(words)
    if "rep" in on:
        raise ValueError("%s with --distill_losses %s: a prediction file carries no state, so there is no L_REP to train on (pred, ce)"
                         % (what, ",".join(on)))
    validate_every_n(FLAGS.every_n, 5, FLAGS.max_num_frames)
    files = sorted(glob.glob(pattern))
    if not files:
        raise ValueError("%s matches no file" % what)
    if len(files) > OfflineDistillGraph.MAX_FILES:
        raise ValueError("%s: %d files (1 .. %d)" % (what, len(files), OfflineDistillGraph.MAX_FILES))
    given_w = [w.strip() for w in FLAGS.teacher_weights.split(",")] if FLAGS.teacher_weights.strip() else []
    if given_w and FLAGS.teacher_mode != "mean":
        raise ValueError("--teacher_weights needs --teacher_mode mean (max has no weights)")
    if given_w and len(given_w) != len(files):
        raise ValueError("--teacher_weights %s: %d entries for the %d files of %s" % (FLAGS.teacher_weights, len(given_w), len(files), what))
    weights = None
    if FLAGS.teacher_mode == "mean":
        try:
            weights = (np.asarray([float(x) for x in given_w], np.float32) if given_w
                       else np.full(len(files), np.float32(1) / np.float32(len(files)), np.float32))
        except ValueError:
            raise ValueError("--teacher_weights %r: a comma list of numbers" % FLAGS.teacher_weights)
    return dict(files=files, names=[os.path.basename(f) for f in files], mode=FLAGS.teacher_mode, weights=weights, losses=on)


def offline_record(spec):
    """What a --teacher_preds_pattern checkpoint records of its teachers (metadata key "distill_teacher_files"): plain lists, strings and
    floats.  The loss list is recorded next to it, under "distill_losses"."""
    return {"files": list(spec["names"]), "mode": spec["mode"], "weights": None if spec["weights"] is None else [float(x) for x in spec["weights"]]}


def check_recorded_files(sd, spec, ck=""):
    """Resume of a --teacher_preds_pattern run from the checkpoint dict ``sd``: the number of files, the mode, the weights and the loss
    list must be the recorded ones (ValueError showing both); other file names are only logged.  A checkpoint that records no files
    (train_convert_model's, train_finetune's, a plain student) is a start from its weights."""
    recorded = sd.get("distill_teacher_files")
    if recorded is None:
        return
    current = offline_record(spec)
    was = (len(recorded["files"]), recorded["mode"], recorded["weights"], sd.get("distill_losses"))
    now = (len(current["files"]), current["mode"], current["weights"], ",".join(spec["losses"]))
    if was != now:
        raise ValueError("--teacher_preds_pattern: the checkpoint %s was trained against other teacher files than the flags name.\n"
                         "  recorded (files, --teacher_mode, --teacher_weights, --distill_losses): %s\n  flags: %s\n"
                         "(resume with the recorded settings, or start a new model)" % (ck, was, now))
    if recorded["files"] != current["files"]:
        logging.info("--teacher_preds_pattern: the checkpoint %s records the files %s, the flags name %s", ck, recorded["files"], current["files"])


def load_teachers(spec):
    """The checkpoints of an ensemble_teachers() spec, read on the host: ([state dict per teacher], [tower per teacher], [checkpoint
    path]).  'auto' resolves as for an ensemble member (inference.member_tower); a directory listed twice is read once.  ValueError
    when a directory holds no checkpoint, not the tower asked for, or entry 0 does not resolve to a teacher tower."""
    from .inference import member_tower
    loaded, sds, towers, cks = {}, [], [], []
    for d, word in zip(spec["dirs"], spec["towers"]):
        if d not in loaded:
            ck = latest_checkpoint(d)
            if ck is None:
                raise ValueError("--teacher_dirs: no model.ckpt-*.pt checkpoint in %s" % d)
            loaded[d] = (ck, torch.load(ck, map_location="cpu"))
        ck, sd = loaded[d]
        sds.append(sd)
        cks.append(ck)
        towers.append(member_tower(sd, word, ck))
    if towers[0] != "teacher":
        raise ValueError("--teacher_dirs / --teacher_towers: entry 0 (%s) resolves to a %s tower; entry 0 is the model/* of the checkpoint, a "
                         "teacher tower" % (cks[0], towers[0]))
    return sds, towers, cks


def teacher_record(spec, towers, cks):
    """What a --teacher_dirs checkpoint records of its teachers (metadata key "distill_teachers"): plain lists, strings and floats."""
    return {"dirs": list(spec["dirs"]), "checkpoints": [os.path.basename(c) for c in cks], "towers": list(towers),
            "every_n": [1 if t == "teacher" else int(e) for t, e in zip(towers, spec["every_n"])],
            "sampling": ["uniform" if t == "teacher" else w for t, w in zip(towers, spec["sampling"])], "mode": spec["mode"],
            "weights": None if spec["weights"] is None else [float(x) for x in spec["weights"]],
            "rep_weights": [float(x) for x in spec["rep_weights"]]}


def check_recorded_teachers(recorded, current, ck=""):
    """Resume of a --teacher_dirs run: the teachers the flags name must be the ones the checkpoint ``ck`` records (teacher_record of
    both); anything else is a ValueError that shows both."""
    if recorded is None:
        raise ValueError("--teacher_dirs: the checkpoint %s to resume from records no teacher list (it was not written by a --teacher_dirs "
                         "run); the flags name %s" % (ck, current))
    if recorded != current:
        raise ValueError("--teacher_dirs: the checkpoint %s was trained against other teachers than the flags name.\n  recorded: %s\n  "
                         "flags:    %s\n(resume with the recorded list, or start a new model)" % (ck, recorded, current))


def serial_students_checkpoints(dirs, start_new_model=False):
    """The checkpoints a --serial_student_dirs run resumes from: one path per directory when every directory holds one and all are
    at the same global_step, None for a fresh start (--start_new_model, or no directory holds one).  Anything else is a ValueError
    that names the directories and their steps.  Reads file names only."""
    if start_new_model:
        return None
    cks = [latest_checkpoint(d) for d in dirs]
    if all(c is None for c in cks):
        return None
    steps = [None if c is None else _ckpt_step(c) for c in cks]
    if any(c is None for c in cks) or len(set(steps)) != 1:
        raise ValueError("--serial_student_dirs: the students resume together or not at all, but the directories stand at %s (every "
                         "directory needs a checkpoint of the same global_step, or none of them any)" %
                         ", ".join("%s: %s" % (d, "no checkpoint" if st is None else "step %d" % st) for d, st in zip(dirs, steps)))
    return cks


def restore_serial_students(graph, cks):
    """Resume of a --serial_student_dirs run: student k from cks[k], the frozen teacher from cks[0].  The other checkpoints must carry
    the same model/* tensors - they were written next to each other by one run - or the directories do not belong together."""
    restore_checkpoint(graph.student_view(0), cks[0])
    teacher = {k: v.cpu() for k, v in graph.teacher.state_dict().items()}
    for k in range(1, len(cks)):
        sd = torch.load(cks[k], map_location="cpu")
        other = [n for n, v in teacher.items() if n not in sd or not torch.equal(sd[n], v)]
        if other:
            raise ValueError("--serial_student_dirs: %s holds another teacher than %s (%s differs): the students of one run share "
                             "their frozen teacher" % (cks[k], cks[0], other[0]))
        restore_checkpoint(graph.student_view(k, with_teacher=False), cks[k])


def nextvlad_size_flags():
    """The size flags of a NeXtVLAD tower, in the order of NeXtVladTower.variable_shapes (after the feature size and the classes)."""
    return (FLAGS.nextvlad_cluster_size, FLAGS.nextvlad_hidden_size, FLAGS.nextvlad_groups, FLAGS.nextvlad_expansion,
            FLAGS.nextvlad_gating_reduction, FLAGS.moe_num_mixtures)


def netvlad_size_flags():
    """The size flags of a NetVLAD tower, in the order of NetVladTower.variable_shapes (after the feature size and the classes)."""
    return (FLAGS.netvlad_cluster_size, FLAGS.netvlad_hidden_size, FLAGS.moe_num_mixtures)


def frames_key(fam):
    """'nextvlad_frames' | 'netvlad_frames': the family's frames flag without its dashes, which is also its checkpoint key."""
    return fam["tower"].FLAG[2:] + "_frames"


def check_vlad_distill_flags(model=None):
    """--teacher_dir with a VLAD --model (``model``: that one alone): the combinations it refuses, as ValueErrors that name the flags (no
    device).  Returns the family (VLAD_FAMILIES) when the flags ask for it, else None.  (--serial_student_dirs, --teacher_dirs and
    --teacher_preds_pattern refuse every model but HierarchicalLstmModel themselves: they are not built for these families.
    --teacher_only, --finetune, several ranks: check_serial_flags; another --label_loss: check_label_loss; another --precision,
    --every_n out of range: the family's check_frames.)"""
    fam = VLAD_FAMILIES.get(FLAGS.model)
    if not FLAGS.teacher_dir or fam is None or model not in (None, FLAGS.model):
        return None
    key = frames_key(fam)
    if getattr(FLAGS, key) != "grid":
        raise ValueError("--teacher_dir %s with --model %s and --%s %s: the student of this family is a grid tower "
                         "(--%s grid --every_n N); distillation of sampled towers is not built"
                         % (FLAGS.teacher_dir, FLAGS.model, key, getattr(FLAGS, key), key))
    return fam


def check_netvlad_distill_flags():
    return check_vlad_distill_flags("NetVLADModel") is not None


def check_nextvlad_dropout_flags():
    """--nextvlad_dropout: a drop rate outside [0, 1) and a non-zero rate with another --model are ValueErrors that name
    the flags (no device).  Returns the rate.  (--dropout is the reference's unused keep-probability: not read.)"""
    rate = ops.check_dropout_rate(FLAGS.nextvlad_dropout, "--nextvlad_dropout")
    if rate > 0.0 and FLAGS.model != "NeXtVLADModel":
        raise ValueError("--nextvlad_dropout %g with --model %s: the flag is the NeXtVLAD tower's drop rate before its hidden layer "
                         "(--model NeXtVLADModel); no other model has dropout" % (rate, FLAGS.model))
    return rate


def nextvlad_dropout_metadata(graph):
    """What a checkpoint records of --nextvlad_dropout: the rate and the seed of the tower that drops (the single tower, or the
    distillation student), and nothing at rate 0.  validate / inference ignore both entries; the weights are the same either way."""
    tw = getattr(graph, "student", None) if isinstance(graph, NeXtVladDistillGraph) else getattr(graph, "tower", None)
    rate = float(getattr(tw, "dropout", 0.0) or 0.0)
    return {"nextvlad_dropout": rate, "nextvlad_dropout_seed": int(tw.dropout_seed)} if rate > 0.0 else {}


def vlad_teacher_every_n(sd, key):
    """The grid the model/* tower of the checkpoint dict ``sd`` runs on as a frozen teacher (key: the family's frames_key): the
    teacher_every_n a distillation checkpoint records (its model/* IS such a teacher), else its every_n when it records <key> == "grid",
    else 1 - a sampled checkpoint, whose weights load into a grid tower, sees every real frame."""
    if sd.get(key) == "grid":
        return int(sd["teacher_every_n"]) if "teacher_every_n" in sd else int(sd["every_n"])
    return 1


nextvlad_teacher_every_n = lambda sd: vlad_teacher_every_n(sd, "nextvlad_frames")
netvlad_teacher_every_n = lambda sd: vlad_teacher_every_n(sd, "netvlad_frames")


def check_nextvlad_teacher_shapes(sd, feature_size, what=""):
    """model/* of the checkpoint dict ``sd`` against the size flags: ValueError naming the first missing or mismatching variable."""
    prefix = "--teacher_dir %s: " % FLAGS.teacher_dir
    if not any(k.startswith("model/") and torch.is_tensor(v) for k, v in sd.items()):
        raise ValueError("%s%s holds no model/* variables (not a teacher checkpoint)" % (prefix, what))
    check_vlad_checkpoint(NeXtVladTower, sd, "model", feature_size, NUM_CLASSES, nextvlad_size_flags(), what, prefix=prefix,
                          clause="not a NeXtVLADModel checkpoint")


def vlad_distill_source(fam, feature_size):
    """The checkpoint the frozen teacher of a VLAD family comes from, read on the host before the device is touched: --train_dir's latest
    on resume, else --teacher_dir's; its model/* variables against the size flags.  Returns {"ck", "sd", "teacher_every_n", "resume"};
    NetVLAD adds "teacher_sampling" and "teacher_gating".  teacher_gating: whether model/* holds the context gate's variables (DESIGN.md
    7.21) - the frozen teacher is built as its checkpoint says, the student as --netvlad_gating says; on resume the flag must agree with
    model_student/*, and --student_init_from_teacher needs the two gates to agree."""
    resume = None if FLAGS.start_new_model else latest_checkpoint(FLAGS.train_dir)
    ck = resume or latest_checkpoint(FLAGS.teacher_dir)
    if ck is None:
        raise ValueError("--teacher_dir %s: no model.ckpt-*.pt checkpoint there" % FLAGS.teacher_dir)
    sd = torch.load(ck, map_location="cpu")
    src = lambda: dict(ck=ck, sd=sd, teacher_every_n=vlad_teacher_every_n(sd, frames_key(fam)), resume=resume is not None)
    if fam["tower"] is NeXtVladTower:
        check_nextvlad_teacher_shapes(sd, feature_size, os.path.basename(ck))
        return src()
    what = "--teacher_dir %s: %s" % (FLAGS.teacher_dir, os.path.basename(ck))
    if not any(k.startswith("model/") and torch.is_tensor(v) for k, v in sd.items()):
        raise ValueError("%s holds no model/* variables (not a teacher checkpoint)" % what)
    teacher_gating = netvlad_checkpoint_gating(sd, "model")
    check_netvlad_checkpoint(sd, "model", feature_size, NUM_CLASSES, netvlad_size_flags(), what, gating=teacher_gating)
    if resume is not None:
        check_netvlad_gating_checkpoint(sd, "model_student", "--train_dir %s: %s" % (FLAGS.train_dir, os.path.basename(ck)))
    elif FLAGS.student_init_from_teacher and teacher_gating != bool(FLAGS.netvlad_gating):
        raise ValueError("--student_init_from_teacher True with --netvlad_gating %s: the teacher of %s was trained %s the context gate, "
                         "its variables do not fill this student" % (FLAGS.netvlad_gating, what, "with" if teacher_gating else "without"))
    return dict(src(), teacher_sampling=netvlad_teacher_sampling(sd), teacher_gating=teacher_gating)


netvlad_distill_source = lambda feature_size: vlad_distill_source(VLAD_FAMILIES["NetVLADModel"], feature_size)


def netvlad_sampling_word(warn=False):
    """The --student_sampling word a NetVLAD tower is built with: the flag under --netvlad_frames grid, and "uniform"
    for every other model.  A sampled tower draws its frames and has no rows to select among: it keeps running on drawn frames, and
    ``warn`` logs that once, naming both flags."""
    word = FLAGS.student_sampling
    if FLAGS.model != "NetVLADModel" or word == "uniform":
        return "uniform"
    if FLAGS.netvlad_frames != "grid":
        if warn:
            logging.warning("--student_sampling %s is not used with --netvlad_frames %s: the tower draws --iterations %d frames per video; "
                            "the word selects among the rows of --netvlad_frames grid", word, FLAGS.netvlad_frames, FLAGS.iterations)
        return "uniform"
    return word


def netvlad_sampling_metadata(graph):
    """The checkpoint keys of a NetVLAD tower trained on selected frames: student_sampling for the one tower of a
    SingleTowerGraph (a distillation graph's student word is recorded with every student's), student_sampling_seed under "random", and
    teacher_sampling[_seed] when the frozen teacher of a distillation runs on a word itself.  "uniform" adds no key."""
    out = {}
    tw = getattr(graph, "tower", None)
    if isinstance(tw, NetVladTower) and tw.sampling != "uniform":
        out["student_sampling"] = tw.sampling
        if tw.sampling == "random":
            out["student_sampling_seed"] = tw.sampling_seed
    if isinstance(graph, NetVladDistillGraph):
        if graph.student_sampling == "random":
            out["student_sampling_seed"] = graph.sampling_seed
        if graph.teacher_sampling != "uniform":
            out["teacher_sampling"] = graph.teacher_sampling
            if graph.teacher_sampling == "random":
                out["teacher_sampling_seed"] = graph.teacher_sampling_seed
    return out


def netvlad_gating_metadata(graph):
    """The checkpoint keys of the NetVLAD context gate, only when true: netvlad_gating for the one tower of a
    SingleTowerGraph or the student of a distillation, teacher_netvlad_gating for its frozen teacher."""
    out = {}
    tw = getattr(graph, "tower", None)
    if isinstance(tw, NetVladTower) and tw.gating:
        out["netvlad_gating"] = True
    if isinstance(graph, NetVladDistillGraph):
        if graph.gating:
            out["netvlad_gating"] = True
        if graph.teacher_gating:
            out["teacher_netvlad_gating"] = True
    return out


def check_netvlad_gating_checkpoint(sd, scope, what):
    """--netvlad_gating against the ``scope``/* tower of a checkpoint that training resumes from: a ValueError naming the flag and the
    variable found or missing when they disagree (no device)."""
    have, key = netvlad_checkpoint_gating(sd, scope), "%s/%s" % (scope, NetVladTower.GW)
    if have and not FLAGS.netvlad_gating:
        raise ValueError("--netvlad_gating False, but %s holds the variable %s: resume it with --netvlad_gating True" % (what, key))
    if FLAGS.netvlad_gating and not have:
        raise ValueError("--netvlad_gating True, but %s holds no variable %s: it was trained without the context gate" % (what, key))


def check_netvlad_gating_flags(world=1, serial=False):
    """--netvlad_gating before the device is touched: refused on several ranks; on resume of a NetVLAD tower trained alone, the flag
    against --train_dir's latest checkpoint (a distillation's resume is checked by vlad_distill_source)."""
    if FLAGS.model != "NetVLADModel":
        return
    check_netvlad_gating(FLAGS.netvlad_gating, world)
    ck = None if (FLAGS.start_new_model or serial) else latest_checkpoint(FLAGS.train_dir)
    if ck is not None:
        check_netvlad_gating_checkpoint(torch.load(ck, map_location="cpu"), "model", "--train_dir %s: %s" % (FLAGS.train_dir, os.path.basename(ck)))


def netvlad_teacher_sampling(sd):
    """(word, seed) the model/* tower of the checkpoint dict ``sd`` runs on as a frozen teacher: the teacher_sampling a distillation
    checkpoint records (its model/* IS such a teacher), else the student_sampling a grid tower trained alone records; "uniform" without
    either."""
    if sd.get("netvlad_frames") != "grid":
        return "uniform", 0
    if "teacher_every_n" in sd:
        return sd.get("teacher_sampling", "uniform"), int(sd.get("teacher_sampling_seed", 0))
    return sd.get("student_sampling", "uniform"), int(sd.get("student_sampling_seed", 0))


def nextvlad_distill_kw(teacher_sampling, teacher_gating):
    """NeXtVladDistillGraph's own keywords from the flags: the student's dropout."""
    return dict(dropout=check_nextvlad_dropout_flags(), dropout_seed=FLAGS.nextvlad_dropout_seed)


def netvlad_distill_kw(teacher_sampling, teacher_gating):
    """NetVladDistillGraph's own keywords from the flags and the teacher's checkpoint (vlad_distill_source): the sampling words (DESIGN.md
    7.20) and the context gates (7.21), each pair only off its default - the call of 7.19 otherwise."""
    kw = {}
    if netvlad_sampling_word() != "uniform" or teacher_sampling[0] != "uniform":
        kw.update(student_sampling=netvlad_sampling_word(), sampling_seed=FLAGS.student_sampling_seed,
                  teacher_sampling=teacher_sampling[0], teacher_sampling_seed=teacher_sampling[1])
    if FLAGS.netvlad_gating or teacher_gating:
        kw.update(gating=FLAGS.netvlad_gating, teacher_gating=teacher_gating)
    return kw


# The VLAD families by --model name: what train reads of a family beyond its tower class (the tower names its model, its
# flag prefix - the --<prefix>_frames flag, the <prefix>_frames checkpoint key - and its messages itself).  check_frames_kw / distill_kw:
# the family's own step behind the shared part.  A third family is one more entry.
VLAD_FAMILIES = {
    "NeXtVLADModel": dict(tower=NeXtVladTower, distill_graph=NeXtVladDistillGraph, size_flags=nextvlad_size_flags,
                          size_names=("cluster_size", "hidden_size", "groups", "expansion", "gating_reduction", "num_mixtures"),
                          check_frames=check_nextvlad_frames, check_frames_kw=lambda: {}, distill_kw=nextvlad_distill_kw),
    "NetVLADModel": dict(tower=NetVladTower, distill_graph=NetVladDistillGraph, size_flags=netvlad_size_flags,
                         size_names=("cluster_size", "hidden_size", "num_mixtures"), check_frames=check_netvlad_frames,
                         check_frames_kw=lambda: dict(sampling=netvlad_sampling_word()), distill_kw=netvlad_distill_kw),
}


def load_frozen_teacher(graph, teacher_dir):
    """The model/* variables of latest_checkpoint(teacher_dir) into the serial graph's frozen teacher.  Returns the checkpoint's path."""
    ck = latest_checkpoint(teacher_dir)
    if ck is None:
        raise ValueError("--teacher_dir %s: no model.ckpt-*.pt checkpoint there" % teacher_dir)
    sd = torch.load(ck, map_location="cpu")
    if not any(k.startswith("model/") and torch.is_tensor(v) for k, v in sd.items()):
        raise ValueError("--teacher_dir %s: %s holds no model/* variables (not a teacher checkpoint)" % (teacher_dir, os.path.basename(ck)))
    graph.teacher.load_state_dict(sd)
    return ck


def check_label_loss(label_loss_fn, finetune=False):
    """--label_loss against the number of classes and the flags it excludes (ValueError / NotImplementedError, before anything touches the
    device): PWELoss refuses itself, CrossEntropyLossTop50 needs 50 classes, CrossEntropyLossClassImbalance its counts file, and the
    serial modes have CrossEntropyLoss built into their loss kernels."""
    if not isinstance(label_loss_fn, losses.BaseLoss):
        raise ValueError("--label_loss: %r is not a losses.BaseLoss" % (label_loss_fn,))
    label_loss_fn.check(NUM_CLASSES)
    if not losses.is_default(label_loss_fn) and (FLAGS.teacher_dir or FLAGS.serial_student_dirs.strip()):
        raise ValueError("--label_loss %s with --teacher_dir / --serial_student_dirs: serial distillation has CrossEntropyLoss built into "
                         "its loss kernels (evc_distill_losses, evc_distill_losses_multi); train it with --label_loss CrossEntropyLoss"
                         % type(label_loss_fn).__name__)


def build_graph(model, label_loss_fn, feature_size, batch_size, every_n, device, finetune=False, process_group=None, students=_UNSET,
                teachers=None, offline=None, teacher_every_n=1, teacher_sampling=("uniform", 0), teacher_gating=False):
    """Equivalent of cs/train.py:185-427 (and cs/train_finetune.py:185-331 when
    finetune): returns the graph object whose ``step`` runs one iteration."""
    check_label_loss(label_loss_fn, finetune)
    common = dict(base_learning_rate=FLAGS.base_learning_rate, learning_rate_decay=FLAGS.learning_rate_decay,
                  learning_rate_decay_examples=FLAGS.learning_rate_decay_examples,
                  regularization_penalty=FLAGS.regularization_penalty, clip_gradient_norm=FLAGS.clip_gradient_norm,
                  process_group=process_group)
    if not losses.is_default(label_loss_fn):           # (the default keeps the graphs' own default: the same constructor calls as ever)
        common["label_loss"] = label_loss_fn
    if isinstance(model, frame_level_models.HierarchicalLstmModel):
        # every_n == 1 (the reference's default, cs/train.py:100-101) still builds and trains model_student, on all 300
        # frames in 5 chunks of 60 (cs/train.py:262-272,349-356): global_step += 2 and the checkpoint holds both scopes.
        # Teacher-only training (BASELINE cfg 2) is not a reference mode: it is asked for with --teacher_only.
        if teachers is not None:
            # one student against several frozen teachers (--teacher_dirs): teachers = an ensemble_teachers() spec with resolved "towers"
            common.pop("label_loss", None)        # (refused for anything but CrossEntropyLoss, which EnsembleDistillGraph has built in)
            return EnsembleDistillGraph(batch_size, teachers=list(zip(teachers["towers"], teachers["every_n"], teachers["sampling"])),
                                        every_n=every_n, teacher_mode=teachers["mode"], teacher_weights=teachers["weights"],
                                        rep_weights=teachers["rep_weights"], student_sampling=FLAGS.student_sampling,
                                        distill_losses=FLAGS.distill_losses, feature_size=feature_size, vocab_size=NUM_CLASSES,
                                        max_frames=FLAGS.max_num_frames, num_inputs_to_lstm=FLAGS.num_inputs_to_lstm,
                                        lstm_cells=FLAGS.lstm_cells, lstm_layers=FLAGS.lstm_layers, num_mixtures=FLAGS.moe_num_mixtures,
                                        device=device, precision=FLAGS.precision, sampling_seed=FLAGS.student_sampling_seed, **common)
        if offline is not None:
            # the student alone against prediction files (--teacher_preds_pattern): offline = an offline_teachers() spec
            common.pop("label_loss", None)        # (refused for anything but CrossEntropyLoss, which the loss kernel has built in)
            return OfflineDistillGraph(batch_size, every_n=every_n, teacher_mode=offline["mode"], teacher_weights=offline["weights"],
                                       distill_losses=offline["losses"], feature_size=feature_size, vocab_size=NUM_CLASSES,
                                       max_frames=FLAGS.max_num_frames, num_inputs_to_lstm=FLAGS.num_inputs_to_lstm,
                                       lstm_cells=FLAGS.lstm_cells, lstm_layers=FLAGS.lstm_layers, num_mixtures=FLAGS.moe_num_mixtures,
                                       device=device, precision=FLAGS.precision, student_sampling=FLAGS.student_sampling,
                                       sampling_seed=FLAGS.student_sampling_seed, **common)
        spec = serial_students(finetune) if students is _UNSET else students
        if spec is not None:
            # K students against one forward of the frozen teacher (--serial_student_dirs): hyper-parameters as below, one of each list per student
            common.pop("label_loss", None)        # (refused above for anything but CrossEntropyLoss, which SerialStudentsGraph has built in)
            return SerialStudentsGraph(batch_size, every_n=spec["every_n"], student_sampling=spec["sampling"], distill_losses=spec["losses"],
                                       feature_size=feature_size, vocab_size=NUM_CLASSES, max_frames=FLAGS.max_num_frames,
                                       num_inputs_to_lstm=FLAGS.num_inputs_to_lstm, lstm_cells=FLAGS.lstm_cells, lstm_layers=FLAGS.lstm_layers,
                                       num_mixtures=FLAGS.moe_num_mixtures, device=device, precision=FLAGS.precision,
                                       sampling_seed=FLAGS.student_sampling_seed, **common)
        mode = "student" if finetune else ("teacher" if getattr(FLAGS, "teacher_only", False) else "teacher_student")
        if FLAGS.teacher_dir and check_serial_flags(finetune):
            # Serial distillation (--teacher_dir): the student against a frozen teacher - not a reference mode either
            mode = "serial"
            common["distill_losses"] = FLAGS.distill_losses
        return DistillGraph(batch_size, every_n=every_n, mode=mode, feature_size=feature_size, vocab_size=NUM_CLASSES,
                            max_frames=FLAGS.max_num_frames, num_inputs_to_lstm=FLAGS.num_inputs_to_lstm,
                            lstm_cells=FLAGS.lstm_cells, lstm_layers=FLAGS.lstm_layers,
                            num_mixtures=FLAGS.moe_num_mixtures, device=device, precision=FLAGS.precision,
                            student_sampling=FLAGS.student_sampling, sampling_seed=FLAGS.student_sampling_seed, **common)
    fam = next((f for name, f in VLAD_FAMILIES.items() if isinstance(model, getattr(frame_level_models, name))), None)
    if FLAGS.teacher_dir and fam is not None:
        # the grid student against the frozen grid teacher; teacher_every_n / teacher_sampling / teacher_gating:
        # what vlad_distill_source reads of the teacher's checkpoint
        check_serial_flags(finetune)
        check_vlad_distill_flags()
        fam["check_frames"](getattr(FLAGS, frames_key(fam)), every_n, FLAGS.max_num_frames, model=FLAGS.model, precision=FLAGS.precision,
                            **fam["check_frames_kw"]())
        common.pop("label_loss", None)            # (refused above for anything but CrossEntropyLoss, which the loss kernel has built in)
        common.update(zip(fam["size_names"], fam["size_flags"]()))
        common.update(fam["distill_kw"](teacher_sampling, teacher_gating))
        return fam["distill_graph"](batch_size, every_n=every_n, teacher_every_n=teacher_every_n, feature_size=feature_size,
                                    vocab_size=NUM_CLASSES, max_frames=FLAGS.max_num_frames, device=device, precision=FLAGS.precision,
                                    distill_losses=FLAGS.distill_losses, **common)
    if FLAGS.teacher_dir:
        raise ValueError("--teacher_dir %s: serial distillation is built for HierarchicalLstmModel and NeXtVLADModel, not %s "
                         "(and for NetVLADModel with --netvlad_frames grid)" % (FLAGS.teacher_dir, type(model).__name__))
    if isinstance(model, frame_level_models.DbofModel):
        tw = DbofTower(batch_size, FLAGS.max_num_frames, feature_size, NUM_CLASSES, FLAGS.iterations,
                       FLAGS.dbof_cluster_size, FLAGS.dbof_hidden_size, FLAGS.moe_num_mixtures, device=device,
                       process_group=process_group)
        _apply_precision(tw)
        return SingleTowerGraph(tw, **common)
    if isinstance(model, frame_level_models.NetVLADModel):          # extension (the reference's class is an empty stub)
        tw = NetVladTower(batch_size, FLAGS.max_num_frames, feature_size, NUM_CLASSES, FLAGS.iterations, FLAGS.netvlad_cluster_size,
                          FLAGS.netvlad_hidden_size, FLAGS.moe_num_mixtures, device=device, process_group=process_group,
                          frames=FLAGS.netvlad_frames, every_n=every_n, sampling=netvlad_sampling_word(warn=True),
                          sampling_seed=FLAGS.student_sampling_seed, gating=FLAGS.netvlad_gating)
        _apply_precision(tw)
        return SingleTowerGraph(tw, **common)
    if isinstance(model, frame_level_models.NeXtVLADModel):         # extension (the reference's class is an empty stub)
        tw = NeXtVladTower(batch_size, FLAGS.max_num_frames, feature_size, NUM_CLASSES, FLAGS.iterations, FLAGS.nextvlad_cluster_size,
                           FLAGS.nextvlad_hidden_size, FLAGS.nextvlad_groups, FLAGS.nextvlad_expansion, FLAGS.nextvlad_gating_reduction,
                           FLAGS.moe_num_mixtures, device=device, process_group=process_group, frames=FLAGS.nextvlad_frames,
                           every_n=every_n, dropout=check_nextvlad_dropout_flags(), dropout_seed=FLAGS.nextvlad_dropout_seed)
        _apply_precision(tw)
        return SingleTowerGraph(tw, **common)
    if isinstance(model, frame_level_models.FrameLevelLogisticModel):
        tw = LogisticTower(batch_size, FLAGS.max_num_frames, feature_size, NUM_CLASSES, device=device)
        _apply_precision(tw)
        return SingleTowerGraph(tw, **common)
    raise NotImplementedError("model %s has no training graph" % type(model).__name__)


def synthetic_batches(batch_size, feature_size, device, videos_per_epoch, num_epochs, seed, drop_remainder=False):
    """Synthetic stand-in for get_input_data_tensors (cs/train.py:129-176): uint8
    features dequantised by the input kernel, n ~ U{120..300}, ~3 labels/video.
    Yields (features, labels, num_frames, num_frames on the host).  drop_remainder (data parallel): no smaller
    final batch."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    T = FLAGS.max_num_frames
    for _ in range(num_epochs):
        left = videos_per_epoch
        while left > 0:
            b = min(batch_size, left)                  # allow_smaller_final_batch=True (cs/train.py:175)
            left -= b
            if b < batch_size and drop_remainder:
                break
            q = torch.randint(0, 256, (b, T, feature_size), generator=g, device=device, dtype=torch.uint8)
            n = torch.randint(min(120, T), T + 1, (b,), generator=g, device=device, dtype=torch.int32)
            labels = torch.zeros((b, NUM_CLASSES), dtype=torch.uint8, device=device)
            labels.scatter_(1, torch.randint(0, NUM_CLASSES, (b, 3), generator=g, device=device), 1)
            yield q, labels, n, n.cpu().numpy()


def get_reader():
    """cs/train.py:618-630: the reader the flags select."""
    feature_names, feature_sizes = GetListOfFeatureNamesAndSizes(FLAGS.feature_names, FLAGS.feature_sizes)
    if FLAGS.frame_features:
        return readers.YT8MFrameFeatureReader(num_classes=NUM_CLASSES, feature_names=feature_names, feature_sizes=feature_sizes,
                                              max_frames=FLAGS.max_num_frames)
    return readers.YT8MAggregatedFeatureReader(num_classes=NUM_CLASSES, feature_names=feature_names, feature_sizes=feature_sizes)


LAST_BATCH = {"ids": None}


def get_input_data(data_pattern, batch_size, feature_size, device, num_epochs, seed, rank=0, world=1):
    """get_input_data_tensors (cs/train.py:129-176) -> iterator of (features uint8, labels uint8, num_frames int32)
    device tensors; ``batch_size`` is per GPU (cs/train.py:205 batch_size * num_towers)."""
    if data_pattern in ("", "synthetic"):
        return synthetic_batches(batch_size, feature_size, device, FLAGS.synthetic_videos, num_epochs, seed,
                                 drop_remainder=world > 1), None
    logging.info("Using batch size of %d for training.", batch_size)
    pipe = readers.get_input_data_tensors(get_reader(), data_pattern, batch_size=batch_size, num_epochs=num_epochs,
                                          num_readers=FLAGS.num_readers, seed=seed, device=device, rank=rank, world_size=world,
                                          with_host_counts=True)
    logging.info("Number of training files / records on this rank: %d / %d.", len(pipe.index), pipe.num_records)
    def batches():
        for b in pipe:
            LAST_BATCH["ids"] = b[0]                     # video ids of the batch being handed out (tests, debugging)
            yield b[1:]
    return batches(), pipe.num_batches


def _ckpt_step(path):
    name = os.path.basename(path)
    return int(name[len("model.ckpt-"):-3]) if name.startswith("model.ckpt-") else 0


def latest_checkpoint(train_dir):
    """tf.train.latest_checkpoint: the highest-numbered model.ckpt-<step>.pt; the un-numbered model.ckpt.pt that
    train_convert_model writes counts as step 0."""
    cks = glob.glob(os.path.join(train_dir, "model.ckpt-*.pt")) + glob.glob(os.path.join(train_dir, "model.ckpt.pt"))
    return max(cks, key=_ckpt_step) if cks else None


def save_checkpoint(graph, train_dir, rank):
    if hasattr(graph, "consolidate"):
        graph.consolidate()                 # collective: sharded optimizer state -> complete on every rank
    if rank != 0:
        return
    os.makedirs(train_dir, exist_ok=True)
    sd = {"global_step": graph.global_step}
    if getattr(graph, "student", None) is not None:
        sd["student_sampling"] = graph.student_sampling          # metadata: the frames this student was trained on (--student_sampling)
    if getattr(graph, "mode", None) == "serial":                 # metadata: trained against the frozen teacher in model/*, on these losses
        sd["distill_mode"], sd["distill_losses"] = "serial", ",".join(graph.distill_losses)
    if getattr(graph, "mode", None) == "ensemble":               # metadata: trained against several frozen teachers, model/* being entry 0
        sd["distill_mode"], sd["distill_losses"] = "ensemble", ",".join(graph.distill_losses)
        sd["distill_teachers"] = getattr(graph, "teacher_record", None) or graph.teacher_meta()
    if isinstance(graph, OfflineDistillGraph) and getattr(graph, "teacher_record", None):    # metadata: trained against these prediction files
        sd["distill_mode"], sd["distill_losses"] = "offline", ",".join(graph.offline_losses)
        sd["distill_teacher_files"] = graph.teacher_record
    if getattr(getattr(graph, "tower", None), "frames", None) == "grid":      # metadata: the frames this tower was trained on (--nextvlad_frames / --netvlad_frames grid)
        sd[type(graph.tower).FLAG[2:] + "_frames"], sd["every_n"] = "grid", graph.tower.every_n
    if isinstance(graph, GridDistillGraph):       # metadata: the student's grid and the one the frozen teacher in model/* runs on
        sd[graph.tower_cls.FLAG[2:] + "_frames"], sd["every_n"], sd["teacher_every_n"] = "grid", graph.every_n, graph.teacher_every_n
    sd.update(netvlad_sampling_metadata(graph))   # metadata: the --student_sampling word of a NetVLAD tower off the uniform grid
    sd.update(netvlad_gating_metadata(graph))     # metadata: --netvlad_gating of the tower / student and the frozen teacher's gate, when true
    sd.update(nextvlad_dropout_metadata(graph))   # metadata: --nextvlad_dropout and its seed, when the tower was trained with a non-zero rate
    fn = getattr(graph, "label_loss", None)
    if fn is not None and not losses.is_default(fn):            # metadata: the --label_loss these weights were trained on (the default: no key)
        sd["label_loss"] = type(fn).__name__
    for tw in (getattr(graph, "teacher", None), getattr(graph, "student", None), getattr(graph, "tower", None)):
        if tw is not None:
            sd.update({k: v.cpu() for k, v in tw.state_dict().items()})
            if tw.store.m is not None:                           # (a frozen tower has no optimizer state: serial distillation's teacher)
                sd["%s/adam" % tw.scope] = {"t": tw.adam_t, "m": tw.store.m.cpu(), "v": tw.store.v.cpu()}
            sd["%s/precision_layout" % tw.scope] = tw.precision_layout()      # metadata: the forward-operand layout these weights were trained under
    path = os.path.join(train_dir, "model.ckpt-%d.pt" % graph.global_step)
    # like tf.train.Saver: write to a temporary name, flush to disk, rename (a validate.py polling the directory never
    # sees a half-written file); the temporary name does not match the model.ckpt*.pt glob
    tmp = os.path.join(train_dir, ".tmp-%d-model.ckpt-%d" % (os.getpid(), graph.global_step))
    with open(tmp, "wb") as f:
        torch.save(sd, f)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)
    for old in glob.glob(os.path.join(train_dir, "model.ckpt*.pt")):       # max_to_keep=1 (cs/train.py:651)
        if old != path:
            try:
                os.remove(old)
            except FileNotFoundError:
                pass
    return path


def restore_checkpoint(graph, path):
    sd = torch.load(path, map_location="cpu")
    graph.global_step = int(sd["global_step"])
    for tw in (getattr(graph, "teacher", None), getattr(graph, "student", None), getattr(graph, "tower", None)):
        if tw is not None and any(k.startswith(tw.scope + "/") for k in sd):
            tw.load_state_dict(sd)
            ad = sd.get("%s/adam" % tw.scope)
            if ad and tw.store.m is not None:                    # (a frozen tower keeps no moments, whatever the checkpoint holds)
                tw.adam_t = ad["t"]
                tw.store.m.copy_(ad["m"])
                tw.store.v.copy_(ad["v"])


def agree_step_limit(max_steps, num_batches, world, device=None):
    """Number of iterations every rank will run: None = until the data ends, an int (0 INCLUDED) = exactly that many.

    Ranks own different files, so under data parallelism they agree on MIN(whole batches) up front - no rank may wait in
    a gradient all-reduce for a peer whose input has run dry.  A rank with fewer records than one batch reports 0 whole
    batches (drop_remainder): the agreed limit is then 0 and NO rank enters the loop (a rank that did would sit in a
    gradient all-reduce while the empty one is already in save_checkpoint's consolidate(): mismatched collectives)."""
    limit = int(max_steps) if max_steps else None
    if world > 1 and num_batches is not None:
        nb = torch.tensor([int(num_batches)], device=device)
        torch.distributed.all_reduce(nb, op=torch.distributed.ReduceOp.MIN)
        limit = int(nb) if limit is None else min(limit, int(nb))
    return limit


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    finetune = "--finetune" in argv
    argv = [a for a in argv if a != "--finetune"]
    FLAGS.parse(argv)
    for k, v in FLAGS.flag_values_dict().items():
        print("Key: %s Value: %s" % (k, v))
    logging.basicConfig(level=logging.INFO, format="INFO:evc:%(message)s")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    offline = offline_teachers(finetune, world, argv)
    ens = ensemble_teachers(finetune, world)
    multi = serial_students(finetune, world)
    serial = check_serial_flags(finetune, world, students=multi)
    check_label_loss(find_class_by_name(FLAGS.label_loss, [losses])(), finetune)
    vlad_fam = check_vlad_distill_flags("NeXtVLADModel") if serial else None
    check_nextvlad_dropout_flags()
    check_nextvlad_frames(FLAGS.nextvlad_frames, FLAGS.every_n, FLAGS.max_num_frames, model=FLAGS.model, world=world, precision=FLAGS.precision)
    check_netvlad_frames(FLAGS.netvlad_frames, FLAGS.every_n, FLAGS.max_num_frames, model=FLAGS.model, world=world, precision=FLAGS.precision,
                         sampling=netvlad_sampling_word())
    check_netvlad_gating_flags(world, serial=bool(serial))
    nx_src = None
    if serial and vlad_fam is None:
        vlad_fam = check_vlad_distill_flags("NetVLADModel")      # (this family's refusal has always come behind the flag checks above)
    if vlad_fam is not None:
        # the teacher's checkpoint on the host - its grid and its shapes against the size flags -, before the device is touched
        nx_src = vlad_distill_source(vlad_fam, sum(GetListOfFeatureNamesAndSizes(FLAGS.feature_names, FLAGS.feature_sizes)[1]))
    ens_sds = None
    if ens:
        # the teachers' checkpoints on the host, and - on resume - the recorded list against the flags: all before the device is touched
        ens_sds, ens_towers, ens_cks = load_teachers(ens)
        ens = dict(ens, towers=ens_towers)
        ens_record = teacher_record(ens, ens_towers, ens_cks)
        ens_resume = None if FLAGS.start_new_model else latest_checkpoint(FLAGS.train_dir)
        if ens_resume is not None:
            check_recorded_teachers(torch.load(ens_resume, map_location="cpu").get("distill_teachers"), ens_record, ens_resume)
    multi_cks = serial_students_checkpoints(multi["dirs"], FLAGS.start_new_model) if multi else None
    tables = None
    if offline:
        # the files parsed on the host, and - on resume - the recorded settings against the flags: all before the device is touched
        from .inference import PriorTables
        off_resume = None if FLAGS.start_new_model else latest_checkpoint(FLAGS.train_dir)
        if off_resume is not None:
            check_recorded_files(torch.load(off_resume, map_location="cpu"), offline, off_resume)
        tables = PriorTables(offline["files"], NUM_CLASSES)
        logging.info("offline distillation against %d prediction files (%s), lists of up to %d classes, --teacher_mode %s, losses %s",
                     len(tables), ", ".join(offline["names"]), tables.kp, offline["mode"], ",".join(offline["losses"]))
    local = int(os.environ.get("LOCAL_RANK", str(FLAGS.gpu)))
    # test hook (tests/test_gpu_dp.py): several ranks on ONE GPU over gloo, to run this file's multi-rank path on a
    # single-GPU box (RCCL refuses two ranks per device).  Never set in a real run.
    shared_gpu = os.environ.get("EVC_TRAIN_SHARED_GPU") == "1"
    if shared_gpu:
        local = 0
    torch.cuda.set_device(local)
    device = "cuda:%d" % local
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        from .distill import dp_timeout
        if shared_gpu:
            torch.distributed.init_process_group("gloo", timeout=dp_timeout())
        else:
            torch.distributed.init_process_group("nccl", device_id=torch.device(device), timeout=dp_timeout())
    ops.check_device(local)
    task = "/job:master/task:%d" % rank
    _, feature_sizes = GetListOfFeatureNamesAndSizes(FLAGS.feature_names, FLAGS.feature_sizes)
    feature_size = sum(feature_sizes)
    model = find_class_by_name(FLAGS.model, [frame_level_models, video_level_models])()
    label_loss_fn = find_class_by_name(FLAGS.label_loss, [losses])()
    if FLAGS.optimizer != "AdamOptimizer":
        raise NotImplementedError("only AdamOptimizer (the reference default, cs/train.py:91) is built")
    graph = build_graph(model, label_loss_fn, feature_size, FLAGS.batch_size, FLAGS.every_n, device, finetune, students=multi, teachers=ens,
                        offline=offline, teacher_every_n=nx_src["teacher_every_n"] if nx_src else 1,
                        teacher_sampling=(nx_src or {}).get("teacher_sampling", ("uniform", 0)),
                        teacher_gating=(nx_src or {}).get("teacher_gating", False))
    if offline:
        graph.teacher_record = offline_record(offline)
    logging.info("%s: Built graph.", task)
    ck = None if (FLAGS.start_new_model or multi) else latest_checkpoint(FLAGS.train_dir)
    if multi and multi_cks:
        for k, c in enumerate(multi_cks):
            logging.info("%s: Restoring student %d from %s", task, k, c)
        restore_serial_students(graph, multi_cks)
        logging.info("%s: --teacher_dir %s only selects serial distillation on resume: the frozen teacher comes from %s", task,
                     FLAGS.teacher_dir, multi_cks[0])
    elif multi:
        logging.info("%s: Building %d new students. Frozen teacher from %s", task, len(multi["dirs"]), load_frozen_teacher(graph, FLAGS.teacher_dir))
    elif FLAGS.start_new_model:
        logging.info("%s: Flag 'start_new_model' is set. Building a new model.", task)
    elif ck is None:
        logging.info("%s: No checkpoint file found. Building a new model.", task)
    else:
        logging.info("%s: Restoring from %s", task, ck)
        restore_checkpoint(graph, ck)
        if serial:
            logging.info("%s: --teacher_dir %s only selects serial distillation on resume: the frozen teacher and the student both "
                         "come from %s", task, FLAGS.teacher_dir, ck)
    if serial and ck is None and getattr(graph, "mode", None) == "serial":
        logging.info("%s: Frozen teacher from %s", task, load_frozen_teacher(graph, FLAGS.teacher_dir))
    if nx_src is not None:
        logging.info("%s: the frozen teacher runs on every %d-th real frame, the student on every %d-th", task, graph.teacher_every_n, graph.every_n)
        if FLAGS.student_init_from_teacher and ck is not None:
            logging.info("%s: --student_init_from_teacher is ignored on resume: the student comes from %s", task, ck)
        elif FLAGS.student_init_from_teacher:
            graph.student.load_state_dict(nx_src["sd"], prefix="model")
            logging.info("%s: the new student starts from the teacher's weights and moving statistics (%s)", task, nx_src["ck"])
        nx_src = None
    if ens:
        # entry 0 came with the student from --train_dir on resume (restore_checkpoint above); every other teacher from its directory
        graph.teacher_record = ens_record
        for j, (tw, sd_j, ck_j) in enumerate(zip(graph.teachers, ens_sds, ens_cks)):
            if j > 0 or ck is None:
                tw.load_state_dict(sd_j)
                logging.info("%s: Frozen teacher %d (%s tower) from %s", task, j, ens["towers"][j], ck_j)
        ens_sds = None
    data, num_batches = get_input_data(FLAGS.train_data_pattern, FLAGS.batch_size, feature_size, device, FLAGS.num_epochs,
                                       1234 + rank, rank, world)
    step_limit = agree_step_limit(FLAGS.max_steps, num_batches, world, device)
    if step_limit == 0:
        logging.warning("%s: a rank has fewer than one whole batch of %d records: no training step on any rank "
                        "(give every rank at least batch_size records)", task, FLAGS.batch_size)
    logging.info("%s: Entering training loop.", task)
    start, last_save, it = time.time(), time.time(), 0
    is_multi = isinstance(graph, SerialStudentsGraph)
    is_ens = isinstance(graph, EnsembleDistillGraph)
    is_distill = isinstance(graph, (DistillGraph, GridDistillGraph)) or is_multi or is_ens
    # --nextvlad_frames / --netvlad_frames grid (one tower, or the student and its frozen teacher): the packed rows are laid out from n_host
    is_grid = getattr(getattr(graph, "tower", None), "frames", None) == "grid" or isinstance(graph, GridDistillGraph)
    steps_per_it = 2 if is_distill and not is_multi and graph.mode == "teacher_student" else 1
    copy_stream = torch.cuda.Stream(device=device)
    host_bufs = {}                       # pinned staging, two alternating sets (one may still be read while the next fills)

    def snapshot(out, labels, it):
        """What the reference's sess.run fetch returns at a logging step (cs/train.py:515-526), taken WITHOUT stopping
        the GPU: device clones in stream order (the step's output buffers are overwritten by the next step), then D2H
        on a copy stream into pinned memory.  finish_log() reads it after the NEXT step has been enqueued, so the host
        metrics of step k are computed while the GPU runs step k+1; the log lines are the same, one step late."""
        pred = out.get("predictions", out.get("student_predictions")).clone()
        lab = labels.clone()
        loss_dev = graph.losses_for_report.clone() if is_distill else out["loss"].detach().clone().reshape(1)
        cur = torch.cuda.current_stream(device)
        copy_stream.wait_stream(cur)
        slot = host_bufs.setdefault(it % 2, {})
        with torch.cuda.stream(copy_stream):
            # the loss values travel to the host on EVERY rank (8 floats, already summed over the ranks inside the
            # step): the non-finite check below must stop all ranks together, not leave the others in a collective
            for key, t in ((("pred", pred), ("lab", lab), ("loss", loss_dev)) if rank == 0 else (("loss", loss_dev),)):
                if key not in slot or slot[key].shape != t.shape or slot[key].dtype != t.dtype:
                    slot[key] = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
                slot[key].copy_(t, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(copy_stream)
        for t in (pred, lab, loss_dev):
            t.record_stream(copy_stream)
        return {"slot": slot, "event": ev, "global_step": out["global_step"], "batch": labels.shape[0]}

    last_log_time = [time.time(), 0]     # (wall time, iteration) of the previous log line: rates over the interval in between

    def finish_log(snap, it_now):
        if rank != 0 and not is_distill:
            return
        snap["event"].synchronize()              # nothing here touches a stream that step it_now+1 has been queued on
        r = graph.loss_report(losses=snap["slot"]["loss"]) if is_distill else None
        if is_distill and not all(np.isfinite(v) for rk in (r if is_multi else [r]) for v in rk.values()):   # slim.learning.create_train_op's check_numerics;
            raise FloatingPointError("LossTensor is inf or nan : %s" % r)      # same (reduced) values on every rank: all stop
        if rank != 0:
            return
        p, y = snap["slot"]["pred"].numpy(), snap["slot"]["lab"].numpy().astype(np.float32)
        hit, perr, gap = (eval_util.calculate_hit_at_one(p, y), eval_util.calculate_precision_at_equal_recall_rate(p, y),
                          eval_util.calculate_gap(p, y))
        if is_multi:
            # one line per student in the reference's format, prefixed with its directory (Hit@1 / PERR / GAP: the shared teacher's predictions)
            history.append((snap["global_step"], [dict(rk) for rk in r]))
            for d, rk in zip(multi["dirs"], r):
                logging.info("%s %s: training step %d| Hit@1: %.2f| PERR: %.2f| GAP: %.2f| Teacher_Loss: %s| L_REP: %s| L_PRED: %s"
                             "| L_CE: %s", d, task, snap["global_step"], hit, perr, gap, round(rk["label_loss"], 2),
                             round(rk["student_loss_state"], 2), round(rk["pred_loss"], 2), round(rk["student_label_loss"], 2))
        elif is_distill:
            history.append((snap["global_step"], dict(r), {"hit_at_one": float(hit), "perr": float(perr), "gap": float(gap)}))
            logging.info("%s: training step %d| Hit@1: %.2f| PERR: %.2f| GAP: %.2f| Teacher_Loss: %s| L_REP: %s| L_PRED: %s"
                         "| L_CE: %s", task, snap["global_step"], hit, perr, gap, round(r["label_loss"], 2),
                         round(r["student_loss_state"], 2), round(r["pred_loss"], 2), round(r["student_label_loss"], 2))
            if is_ens:                   # Teacher_Loss above is the combined prediction's; each teacher's own next to it
                logging.info("%s: training step %d| Teacher_Losses: %s", task, snap["global_step"],
                             " ".join("%s" % round(r["teacher_%d_label_loss" % j], 2) for j in range(graph.J)))
        else:
            history.append((snap["global_step"], {"loss": float(snap["slot"]["loss"][0])},
                            {"hit_at_one": float(hit), "perr": float(perr), "gap": float(gap)}))
            logging.info("%s: training step %d| Hit@1: %.2f| PERR: %.2f| GAP: %.2f| Loss: %s", task, snap["global_step"],
                         hit, perr, gap, round(float(snap["slot"]["loss"][0]), 2))
        now = time.time()
        dt = max(now - last_log_time[0], 1e-9) / max(1, it_now - last_log_time[1])
        last_log_time[0], last_log_time[1] = now, it_now
        logging.info("global_step/sec: %g  Examples/Second: %g", steps_per_it / dt, snap["batch"] * world / dt)

    def save_checkpoints():
        """Wherever a single run saves: --train_dir, or one checkpoint per student into its own directory (--serial_student_dirs)."""
        if not is_multi:
            return save_checkpoint(graph, FLAGS.train_dir, rank)
        for k, d in enumerate(multi["dirs"]):
            save_checkpoint(graph.student_view(k), d, rank)

    history = []                         # (global_step, loss dict) of every logged step, returned to the caller
    pending = None
    for q, labels, n, n_host in (data if step_limit != 0 else ()):
        if tables is not None:      # the teacher files' lists of exactly these videos: pinned staging, non_blocking copies on this stream
            out = graph.step(q, labels, n, num_frames_host=n_host, teacher_lists=tables.gather_device(LAST_BATCH["ids"], device))
        else:
            out = graph.step(q, labels, n, num_frames_host=n_host) if is_distill or is_grid else graph.step(q, labels, n)    # uint8 features: Dequantize is fused into every input kernel
        it += 1
        graph.last_batch_ids = LAST_BATCH["ids"]
        logging_step = it % max(1, FLAGS.log_every) == 0
        snap = snapshot(out, labels, it) if logging_step else None
        if pending is not None:
            finish_log(pending, it - 1)                                        # step it-1's metrics, under step it
        pending = snap
        # the checkpoint decision is collective under data parallelism: rank 0's clock decides, every 64 iterations
        save_due = time.time() - last_save > 30 * 60                           # save_model_secs (cs/train.py:500)
        if world > 1:
            save_due = False
            if it % 64 == 0:                                                   # (a host sync: not at every step)
                flag = torch.tensor([1 if time.time() - last_save > 30 * 60 else 0], device=device)
                torch.distributed.broadcast(flag, src=0)
                save_due = bool(flag.item())
        if save_due:
            save_checkpoints()
            last_save = time.time()
        if step_limit is not None and it >= step_limit:
            break
    if pending is not None:
        finish_log(pending, it)
    logging.info("%s: Done training -- epoch limit reached.", task)
    save_checkpoints()
    logging.info("%s: Exited training loop.", task)
    print("Total time taken is " + str(time.time() - start))
    if world > 1:
        torch.distributed.destroy_process_group()
    return {"graph": graph, "history": history, "iterations": it}


if __name__ == "__main__":
    main()
