"""Inference binary with the reference's flag surface: cs/inference_ensemble.py / cs/inference_bias.py (the YouTube-8M
starter code's inference.py) - predictions for a set of (unlabelled) videos as a ``VideoId,LabelConfidencePairs`` file
with each video's top_k classes.

    python -m efficientvideoclassification_youtube8m_amd.inference \
        --input_data_pattern "./yt8m/test*.tfrecord" --train_dir ./model_HLSTM_TeaStud_every10/ --output_file ./predictions.csv \
        --frame_features True --feature_names "rgb, audio" --feature_sizes "1024, 128" --model "HierarchicalLstmModel" \
        --gpu 0 --batch_size 1024 --num_inputs_to_lstm 20 --lstm_layers 2 --every_n 10 --top_k 20

Kept: flags, error texts (cs/inference_ensemble.py:121,228-233), the file format of format_lines (:63-74: header line, then
``id,class conf class conf ...`` with ``"%i %f"``).  Which tower is served follows the variables the checkpoint holds: a
train.py checkpoint (``model/*``) serves the teacher, the tower cs/train.py:338 puts in "predictions"; a train_convert_model /
train_finetune checkpoint (``model_student/*`` only) serves the student at --every_n (cs/train_finetune.py:327).
Replaced: TF session / queue runners -> readers.get_input_evaluation_tensors + distill.EvalGraph; argpartition + sort of the
[B, 4716] predictions on the host -> ops.topk_rows (evc_topk_rows) on the device behind the MoE head: only the [B, top_k]
values and indices are copied back, and batch k is formatted while the GPU runs batch k+1.

Ensembles (cs/inference_ensemble.py:155-193 --preds_pattern, cs/max_ensemble.py): with ``--ensemble_dirs dirA,dirB,...`` every member
(``--ensemble_towers`` auto|teacher|student, ``--ensemble_every_n``) runs its forward on the same batch, the lists of the earlier prediction
files matched by ``--preds_pattern`` join as sparse members, and one launch of ops.ensemble_topk_rows (evc_ensemble_topk_rows) combines them
(``--ensemble_mode`` max | mean, ``--ensemble_weights``) and selects: the frames are read once and still only [B, top_k] leaves the device.

    python -m efficientvideoclassification_youtube8m_amd.inference \
        --input_data_pattern "./yt8m/test*.tfrecord" --output_file ./predictions_ensemble.csv --top_k 20 --batch_size 1024 \
        --ensemble_dirs "./model_train/,./model_train/,./model_every30_finetune/" --ensemble_towers "teacher,student,auto" \
        --ensemble_every_n "1,10,30" --ensemble_mode max --preds_pattern "./earlier_predictions/*.csv"  (+ the model / input flags above)

Cascades (an addition): with ``--cascade_dirs dirA,dirB[,...]`` (cheapest first; ``--cascade_towers`` / ``--cascade_every_n`` /
``--cascade_sampling`` per stage) stage 0 runs on the whole batch, a gate on the device measures each video's confidence
(``--cascade_confidence`` top1 | margin) and only the videos below ``--cascade_thresholds`` - at most ``--cascade_fractions`` of the batch,
the least confident first - run the next stage (cascade.CascadeGraph); ops.topk_rows then selects from the merged predictions, each video's
row being that of the last stage that ran it.  ``--cascade_stage_file`` records which stage decided each video.

    python -m efficientvideoclassification_youtube8m_amd.inference \
        --input_data_pattern "./yt8m/test*.tfrecord" --output_file ./predictions_cascade.csv --top_k 20 --batch_size 1024 \
        --cascade_dirs "./model_every30_finetune/,./model_train/" --cascade_every_n "30,1" --cascade_thresholds 0.9 --cascade_fractions 0.3

NeXtVLAD checkpoints (an addition): ``--model NeXtVLADModel`` serves a grid tower of --train_dir's checkpoint through
vlad_graphs.NeXtVladEvalGraph - ``--serve_tower`` auto (model_student/* when the checkpoint holds it, else model/*) | teacher | student, on
the grid the checkpoint records unless ``--nextvlad_serve_every_n`` names another.  The family of every ensemble member and cascade
stage is read from its own checkpoint (checkpoint_family), so H-LSTM and NeXtVLAD members mix; NeXtVLAD members take their sizes from
the --nextvlad_* flags and an every_n entry of 0 or '' means "as recorded".
"""
from __future__ import annotations

import glob
import logging
import sys
import time

import numpy as np
import torch

from . import frame_level_models, ops, readers, utils, video_level_models
from .distill import EnsembleGraph, EvalGraph
from .flags import FLAGS
from .train import NUM_CLASSES, find_class_by_name, get_reader, latest_checkpoint, nextvlad_size_flags, nextvlad_teacher_every_n
from .vlad_graphs import NeXtVladEvalGraph, check_nextvlad_checkpoint

HEADER = "VideoId,LabelConfidencePairs\n"


def format_lines(video_ids, values, indices):
    """cs/inference_ensemble.py:63-74 on the device's selection: one line per video, ``id,class conf class conf ...\\n``, the pairs
    in the order of the arrays (ops.topk_rows: confidence descending, class ascending on ties).  values [B, k] f32, indices [B, k].
    Byte-identical to the reference's text for rows without ties (where the reference's order is undefined, this one is
    class-ascending)."""
    for vid, v, i in zip(video_ids, np.asarray(values).tolist(), np.asarray(indices).tolist()):
        if isinstance(vid, bytes):
            vid = vid.decode("utf-8")
        yield vid + "," + " ".join("%i %f" % pair for pair in zip(i, v)) + "\n"


def _words(text):
    return [w.strip() for w in text.split(",")] if text.strip() else []


def ensemble_spec(allow_preds_files=True):
    """The ensemble the flags describe, checked: None without --ensemble_dirs, else dict(dirs, towers, every_n, sampling [M]; mode; weights
    float32 [M + P] or None; files [P], sorted by name as cs/inference_ensemble.py:169-170).  Raises ValueError for everything that can be
    refused before the device is touched."""
    dirs = _words(FLAGS.ensemble_dirs)
    towers, every_n, weights = _words(FLAGS.ensemble_towers), _words(FLAGS.ensemble_every_n), _words(FLAGS.ensemble_weights)
    sampling = _words(FLAGS.ensemble_sampling)
    if FLAGS.preds_pattern != "" and not allow_preds_files:
        raise ValueError("--preds_pattern: earlier prediction files join an ensemble in inference only")
    if not dirs:
        if FLAGS.preds_pattern != "":
            raise ValueError("--preds_pattern without --ensemble_dirs: no model is served that the files could join")
        for name, given in (("towers", towers), ("every_n", every_n), ("weights", weights), ("sampling", sampling)):
            if given:
                raise ValueError("--ensemble_%s: %d entries for 0 --ensemble_dirs" % (name, len(given)))
        return None
    M = len(dirs)
    if M > ops.ENSEMBLE_MAX_MEMBERS or "" in dirs:
        raise ValueError("--ensemble_dirs: %d members (1 .. %d, none empty)" % (M, ops.ENSEMBLE_MAX_MEMBERS))
    towers = towers or ["auto"] * M
    every_n = every_n or [str(FLAGS.every_n)] * M
    sampling = sampling or [FLAGS.student_sampling] * M
    for name, given in (("towers", towers), ("every_n", every_n), ("sampling", sampling)):
        if len(given) != M:
            raise ValueError("--ensemble_%s: %d entries for %d --ensemble_dirs" % (name, len(given), M))
    for t in towers:
        if t not in ("auto", "teacher", "student"):
            raise ValueError("--ensemble_towers: %r (auto | teacher | student)" % t)
    every_n = [int(e) if e else 0 for e in every_n]                  # (0 / '': a NeXtVLAD member's recorded grid, nextvlad_every_n)
    for s in sampling:
        ops.check_student_sampling(s, "--ensemble_sampling")
    if FLAGS.ensemble_mode not in ops.ENSEMBLE_MODES:
        raise ValueError("--ensemble_mode %r (max | mean)" % FLAGS.ensemble_mode)
    files = []
    if FLAGS.preds_pattern != "":
        files = sorted(glob.glob(FLAGS.preds_pattern))
        if not files:
            raise ValueError("--preds_pattern '%s' matches no file" % FLAGS.preds_pattern)
        if len(files) > ops.ENSEMBLE_MAX_PRIORS:
            raise ValueError("--preds_pattern: %d files (at most %d)" % (len(files), ops.ENSEMBLE_MAX_PRIORS))
    w = None
    if weights:
        if FLAGS.ensemble_mode != "mean":
            raise ValueError("--ensemble_weights needs --ensemble_mode mean (max has no weights)")
        if len(weights) != M + len(files):
            raise ValueError("--ensemble_weights: %d entries for %d members + %d prediction files" % (len(weights), M, len(files)))
        w = np.asarray([float(x) for x in weights], np.float32)
    return dict(dirs=dirs, towers=towers, every_n=every_n, sampling=sampling, mode=FLAGS.ensemble_mode, weights=w, files=files,
                every_n_given=bool(_words(FLAGS.ensemble_every_n)))


def cascade_spec():
    """The cascade the flags describe, checked: None without --cascade_dirs, else dict(dirs, towers, every_n, sampling [K]; confidence;
    thresholds / fractions: [K - 1] floats or None; stage_file).  Raises ValueError for everything that can be refused before the device is
    touched."""
    dirs = _words(FLAGS.cascade_dirs)
    lists = {name: _words(getattr(FLAGS, "cascade_" + name)) for name in ("towers", "every_n", "sampling", "thresholds", "fractions")}
    if not dirs:
        for name, given in lists.items():
            if given:
                raise ValueError("--cascade_%s: %d entries for 0 --cascade_dirs" % (name, len(given)))
        for name in ("confidence", "stage_file"):
            if getattr(FLAGS, "cascade_" + name) != "":
                raise ValueError("--cascade_%s without --cascade_dirs: there is no cascade it could apply to" % name)
        return None
    if FLAGS.ensemble_dirs != "" or FLAGS.preds_pattern != "":
        raise ValueError("--cascade_dirs together with --ensemble_dirs / --preds_pattern: a cascade serves each video from ONE of its stages, "
                         "an ensemble combines all members; choose one")
    K = len(dirs)
    if not 2 <= K <= ops.CASCADE_MAX_STAGES or "" in dirs:
        raise ValueError("--cascade_dirs: %d stages (2 .. %d, none empty)" % (K, ops.CASCADE_MAX_STAGES))
    towers = lists["towers"] or ["auto"] * K
    every_n = lists["every_n"] or [str(FLAGS.every_n)] * K
    sampling = lists["sampling"] or [FLAGS.student_sampling] * K
    for name, given in (("towers", towers), ("every_n", every_n), ("sampling", sampling)):
        if len(given) != K:
            raise ValueError("--cascade_%s: %d entries for %d --cascade_dirs" % (name, len(given), K))
    for t in towers:
        if t not in ("auto", "teacher", "student"):
            raise ValueError("--cascade_towers: %r (auto | teacher | student)" % t)
    every_n = [int(e) if e else 0 for e in every_n]                  # (0 / '': a NeXtVLAD stage's recorded grid, nextvlad_every_n)
    for s in sampling:
        ops.check_student_sampling(s, "--cascade_sampling")
    confidence = FLAGS.cascade_confidence or "top1"
    if confidence not in ops.CASCADE_CONFIDENCE:
        raise ValueError("--cascade_confidence %r (%s)" % (confidence, " | ".join(ops.CASCADE_CONFIDENCE)))
    gates = {}
    for name in ("thresholds", "fractions"):
        given = lists[name]
        if given and len(given) != K - 1:
            raise ValueError("--cascade_%s: %d entries for the %d gates of %d --cascade_dirs" % (name, len(given), K - 1, K))
        try:
            gates[name] = [float(x) for x in given] if given else None
        except ValueError:
            raise ValueError("--cascade_%s: %r is not a list of numbers" % (name, getattr(FLAGS, "cascade_" + name)))
    if gates["thresholds"] is None and gates["fractions"] is None:
        raise ValueError("--cascade_dirs needs --cascade_thresholds or --cascade_fractions (or both): without a gate no video would "
                         "leave the first stage")
    for f in gates["fractions"] or []:
        if not 0.0 <= f <= 1.0:
            raise ValueError("--cascade_fractions: %r is outside [0, 1]" % f)
    return dict(dirs=dirs, towers=towers, every_n=every_n, sampling=sampling, confidence=confidence, thresholds=gates["thresholds"],
                fractions=gates["fractions"], stage_file=FLAGS.cascade_stage_file, every_n_given=bool(lists["every_n"]))


def read_prediction_file(path, num_classes=NUM_CLASSES):
    """A ``VideoId,LabelConfidencePairs`` file (format_lines; read_pred_file of cs/inference_ensemble.py:155-167) as
    {video id: (classes int32 [n], confidences float32 [n])}, pairs in the order of the line.  ValueError for a missing header, a
    malformed line, a class repeated within a line or outside [0, num_classes), or more than 256 pairs (evc_ensemble_topk_rows' kp)."""
    table = {}
    with open(path) as f:
        if f.readline() != HEADER:
            raise ValueError("%s: the first line is not %r" % (path, HEADER.strip()))
        for lineno, line in enumerate(f, 2):
            line = line.rstrip("\n")
            if line == "":
                continue
            vid, sep, pairs = line.partition(",")
            toks = pairs.split()
            if sep == "" or len(toks) % 2:
                raise ValueError("%s:%d: not 'id,class conf class conf ...'" % (path, lineno))
            if len(toks) // 2 > ops.ENSEMBLE_MAX_KP:
                raise ValueError("%s:%d: %d pairs (at most %d)" % (path, lineno, len(toks) // 2, ops.ENSEMBLE_MAX_KP))
            cls = np.asarray([int(t) for t in toks[0::2]], np.int64)
            conf = np.asarray([float(t) for t in toks[1::2]], np.float32)
            if cls.size and (cls.min() < 0 or cls.max() >= num_classes):
                raise ValueError("%s:%d: class outside [0, %d)" % (path, lineno, num_classes))
            if np.unique(cls).size != cls.size:
                raise ValueError("%s:%d: a class is listed twice" % (path, lineno))
            table[vid] = (cls.astype(np.int32), conf)
    return table


def prior_list_length(tables):
    """kp of a set of parsed prediction files: their longest list (at least 1)."""
    return max([1] + [c.size for t in tables for c, _ in t.values()])


def gather_priors(tables, files, video_ids, kp, out=None):
    """The lists of one batch as the arrays evc_ensemble_topk_rows reads: (idx int32, val float32) [P, B, kp] in the order of tables
    and of video_ids, shorter lists padded with idx = -1 (val 0).  out: arrays to fill (the loop passes pinned ones).  A video id that
    a file does not hold is a KeyError naming both (the reference fails there too, cs/inference_ensemble.py:190)."""
    P, B = len(tables), len(video_ids)
    idx, val = out if out is not None else (np.empty((P, B, kp), np.int32), np.empty((P, B, kp), np.float32))
    idx[...] = -1
    val[...] = 0
    for p, (table, path) in enumerate(zip(tables, files)):
        for b, vid in enumerate(video_ids):
            if isinstance(vid, bytes):
                vid = vid.decode("utf-8")
            if vid not in table:
                raise KeyError("video id %r is not in the prediction file %s" % (vid, path))
            cls, conf = table[vid]
            idx[p, b, :cls.size] = cls
            val[p, b, :cls.size] = conf
    return idx, val


class PriorTables:
    """Prediction files as arrays, for a loop that gathers the lists of every training batch (train --teacher_preds_pattern): each file is
    parsed once by read_prediction_file (same format, same errors) and kept as contiguous idx int32 [N, kp] / val float32 [N, kp] (shorter
    lists padded with idx = -1, val 0: the padding of gather_priors) plus a {video id: row} dictionary; kp is the longest list of all the
    files (prior_list_length).  gather() then costs one dictionary lookup per id and one np.take per file."""

    def __init__(self, files, num_classes=NUM_CLASSES, tables=None):
        self.files = list(files)
        tables = [read_prediction_file(path, num_classes) for path in self.files] if tables is None else list(tables)
        self.kp = prior_list_length(tables)
        self.rows, self.idx, self.val = [], [], []
        for table in tables:
            n = len(table)
            idx, val = np.full((n, self.kp), -1, np.int32), np.zeros((n, self.kp), np.float32)
            rows = {}
            for r, (vid, (cls, conf)) in enumerate(table.items()):
                rows[vid] = r
                idx[r, :cls.size] = cls
                val[r, :cls.size] = conf
            self.rows.append(rows)
            self.idx.append(idx)
            self.val.append(val)
        self._pinned, self._turn = {}, 0

    def __len__(self):
        return len(self.files)

    def gather(self, video_ids, out=None):
        """gather_priors(tables, files, video_ids, kp, out): exactly its arrays (idx int32, val float32) [P, B, kp], and its KeyError naming
        the id and the file for an id a file does not hold."""
        P, B = len(self.files), len(video_ids)
        idx, val = out if out is not None else (np.empty((P, B, self.kp), np.int32), np.empty((P, B, self.kp), np.float32))
        ids = [v.decode("utf-8") if isinstance(v, bytes) else v for v in video_ids]
        for p, (rows, path) in enumerate(zip(self.rows, self.files)):
            try:
                sel = np.fromiter((rows[v] for v in ids), np.intp, B)
            except KeyError:
                vid = next(v for v in ids if v not in rows)
                raise KeyError("video id %r is not in the prediction file %s" % (vid, path)) from None
            np.take(self.idx[p], sel, axis=0, out=idx[p])
            np.take(self.val[p], sel, axis=0, out=val[p])
        return idx, val

    def gather_device(self, video_ids, device):
        """gather() into pinned buffers - two sets used alternately, so that the set of the step in flight is not overwritten - and their
        non_blocking copies to `device` on the current stream.  Returns (idx [P, B, kp] int32, val [P, B, kp] f32) device tensors."""
        P, B = len(self.files), len(video_ids)
        key = (self._turn, B)
        self._turn ^= 1
        if key not in self._pinned:          # (a smaller final batch gets sets of its own)
            self._pinned[key] = (torch.empty((P, B, self.kp), dtype=torch.int32, pin_memory=True),
                                 torch.empty((P, B, self.kp), dtype=torch.float32, pin_memory=True), [None])
        idx_h, val_h, ev = self._pinned[key]
        if ev[0] is not None:
            ev[0].synchronize()              # the copies of two steps ago have left these buffers
        self.gather(video_ids, out=(idx_h.numpy(), val_h.numpy()))
        idx_d, val_d = idx_h.to(device, non_blocking=True), val_h.to(device, non_blocking=True)
        ev[0] = torch.cuda.Event()
        ev[0].record(torch.cuda.current_stream(device))
        return idx_d, val_d


def check_flags():
    """Everything that is refused before a record is read or the device is touched.  Returns ensemble_spec() (cascade_spec() is checked
    here too; main() asks for it again)."""
    cascade_spec()
    if FLAGS.output_file == "":
        raise ValueError("'output_file' was not specified. Unable to continue with inference.")
    if FLAGS.input_data_pattern == "":
        raise ValueError("'input_data_pattern' was not specified. Unable to continue with inference.")
    if not FLAGS.frame_features:
        raise ValueError("--frame_features False: inference serves the frame-level HierarchicalLstmModel only")
    model = find_class_by_name(FLAGS.model, [frame_level_models, video_level_models])
    if isinstance(model, type) and issubclass(model, frame_level_models.NeXtVLADModel):
        check_nextvlad_serving_flags()
    elif not (isinstance(model, type) and issubclass(model, frame_level_models.HierarchicalLstmModel)):
        raise NotImplementedError("inference serves the H-LSTM teacher / student towers (cs/train.py:338, cs/train_finetune.py:327) and the "
                                  "NeXtVLAD grid towers; model %s has no inference path here" % FLAGS.model)
    if FLAGS.serve_tower not in ("auto", "teacher", "student"):
        raise ValueError("--serve_tower %r (auto | teacher | student)" % FLAGS.serve_tower)
    top_max = min(ops.TOPK_MAX_K, NUM_CLASSES)
    if not 1 <= FLAGS.top_k <= top_max:
        raise ValueError("--top_k %d: must be in [1, %d]" % (FLAGS.top_k, top_max))
    return ensemble_spec()


FAMILY_MODELS = {"hlstm": "HierarchicalLstmModel", "nextvlad": "NeXtVLADModel"}


def checkpoint_family(state_dict):
    """'nextvlad' or 'hlstm', from the names of the checkpoint's variables: */expansion_weights is a NeXtVLAD tower's, */RNN_L1/* and
    */RNN_L2/* are an H-LSTM tower's; anything else is a ValueError."""
    names = [k for k, v in state_dict.items() if torch.is_tensor(v)]
    if any(k.endswith("/expansion_weights") for k in names):
        return "nextvlad"
    if any("/RNN_L1/" in k or "/RNN_L2/" in k for k in names):
        return "hlstm"
    raise ValueError("the checkpoint holds neither NeXtVLAD (*/expansion_weights) nor H-LSTM (*/RNN_L1/*) variables; it holds e.g. %s"
                     % sorted(names)[:3])


def check_model_family(state_dict, where):
    """--model against the family of the checkpoint ``where``: a ValueError naming the flag when they disagree.  Returns the family."""
    family = checkpoint_family(state_dict)
    if FLAGS.model != FAMILY_MODELS[family]:
        raise ValueError("--model %s, but %s is a %s checkpoint (pass --model %s)" % (FLAGS.model, where, FAMILY_MODELS[family],
                                                                                      FAMILY_MODELS[family]))
    return family


def check_nextvlad_serving_flags(sampling=None, flag="--student_sampling"):
    """What serving a NeXtVLAD tower refuses, as ValueErrors that name the flags, before the device is touched."""
    if FLAGS.precision != "bf16":
        raise ValueError("--precision %s with --model NeXtVLADModel: the NeXtVLAD tower has no such forward mode (bf16 only)" % FLAGS.precision)
    sampling = FLAGS.student_sampling if sampling is None else sampling
    if sampling != "uniform":
        raise ValueError("%s %s with --model NeXtVLADModel: a grid tower reads every every_n-th real frame (uniform); the other "
                         "selections are not built for this family" % (flag, sampling))
    if FLAGS.nextvlad_serve_every_n < 0 or FLAGS.nextvlad_serve_every_n > FLAGS.max_num_frames:
        raise ValueError("--nextvlad_serve_every_n %d must lie in 0 .. --max_num_frames %d (0 = as the checkpoint records)"
                         % (FLAGS.nextvlad_serve_every_n, FLAGS.max_num_frames))


def nextvlad_tower(state_dict, word, where=""):
    """The tower of a NeXtVLAD checkpoint a word of auto|teacher|student serves: auto = model_student/* when the checkpoint holds it (the
    student is what a --teacher_dir run produces), else model/*; the others as member_tower."""
    if word == "auto":
        has_student = any(k.startswith("model_student/") and torch.is_tensor(v) for k, v in state_dict.items())
        return "student" if has_student else member_tower(state_dict, "teacher", where)
    return member_tower(state_dict, word, where)


def nextvlad_every_n(state_dict, tower, override=0, where="the checkpoint", flag="--nextvlad_serve_every_n"):
    """The grid a served NeXtVLAD tower runs on: what its checkpoint records - model_student/*: every_n; model/*:
    train.nextvlad_teacher_every_n, 1 for a sampled checkpoint - unless ``override`` > 0 names another, which wins with a warning."""
    if tower == "student":
        recorded = int(state_dict["every_n"]) if state_dict.get("nextvlad_frames") == "grid" and "every_n" in state_dict else 1
    else:
        recorded = nextvlad_teacher_every_n(state_dict)
    if override and int(override) != recorded:
        logging.warning("%s %d, but the %s of %s runs on every_n = %d there (the flag is used)", flag, override, tower, where, recorded)
        return int(override)
    return recorded


def check_nextvlad_shapes(reader, state_dict, tower, where="the checkpoint"):
    """The variables of the served tower ('both': validate's pair) against the --nextvlad_* / --feature_sizes / --moe_num_mixtures flags, on
    the host: a ValueError naming the first missing or mismatching variable and both shapes."""
    for scope in {"teacher": ("model",), "student": ("model_student",), "both": ("model", "model_student")}[tower]:
        check_nextvlad_checkpoint(state_dict, scope, sum(reader.feature_sizes), reader.num_classes, nextvlad_size_flags(), where)


def nextvlad_graph(reader, state_dict, tower, every_n, batch_size, device, where="the checkpoint", teacher_every_n=1, label_loss=None,
                   compact=True):
    """NeXtVladEvalGraph for one served tower ('both': validate's pair) at the sizes of the --nextvlad_* flags, after
    check_nextvlad_shapes."""
    check_nextvlad_shapes(reader, state_dict, tower, where)
    F, V = sum(reader.feature_sizes), reader.num_classes
    cs, hs, g, ex, gr, mx = nextvlad_size_flags()
    return NeXtVladEvalGraph(batch_size, tower=tower, every_n=every_n, teacher_every_n=teacher_every_n, feature_size=F, vocab_size=V,
                             max_frames=FLAGS.max_num_frames, cluster_size=cs, hidden_size=hs, groups=g, expansion=ex, gating_reduction=gr,
                             num_mixtures=mx, device=device, precision=FLAGS.precision, label_loss=label_loss, compact=compact)


def serving_tower(state_dict):
    """'teacher' for a checkpoint holding model/* (train.py), 'student' for one holding only model_student/* (train_convert_model,
    train_finetune)."""
    names = [k for k, v in state_dict.items() if torch.is_tensor(v)]
    if any(k.startswith("model/") for k in names):
        return "teacher"
    if any(k.startswith("model_student/") for k in names):
        return "student"
    raise ValueError("the checkpoint holds neither model/* nor model_student/* variables")


def member_tower(state_dict, word, where=""):
    """The tower a member serves: 'auto' = serving_tower(); 'teacher' / 'student' = that tower, which the checkpoint must hold
    ('student' on a train.py checkpoint serves the student trained next to the teacher)."""
    if word == "auto":
        return serving_tower(state_dict)
    scope = "model/" if word == "teacher" else "model_student/"
    if not any(k.startswith(scope) and torch.is_tensor(v) for k, v in state_dict.items()):
        raise ValueError("the checkpoint %sholds no %s* variables: it cannot serve the %s" % (where + " " if where else "", scope, word))
    return word


def warn_sampling(state_dict, word, where):
    """A student evaluated on other frames than it was trained on is a legitimate experiment, so the flag wins - but say so."""
    trained = state_dict.get("student_sampling")
    if trained is not None and trained != word:
        logging.warning("--student_sampling %s, but the student of %s was trained with %s (the flag is used)", word, where, trained)


def load_members(spec):
    """Checkpoints and towers of an ensemble_spec(): ([state dict per member], [(dir, tower, every_n)], [checkpoint path]).  A
    directory listed twice is read once."""
    loaded, sds, members, cks = {}, [], [], []
    for d, word, every_n in zip(spec["dirs"], spec["towers"], spec["every_n"]):
        if d not in loaded:
            ck = latest_checkpoint(d)
            if ck is None:
                raise IOError("unable to find a checkpoint at location: %s" % d)
            logging.info("restoring variables from " + ck)
            loaded[d] = (ck, torch.load(ck, map_location="cpu"))
        ck, sd = loaded[d]
        sds.append(sd)
        cks.append(ck)
        sampling = spec.get("sampling", [FLAGS.student_sampling] * len(spec["dirs"]))[len(members)]
        if checkpoint_family(sd) == "nextvlad":                          # its own family: sizes from the --nextvlad_* flags, host checks here
            check_nextvlad_serving_flags(sampling, "--ensemble_sampling / --cascade_sampling / --student_sampling")
            tower = nextvlad_tower(sd, word, ck)
            every_n = nextvlad_every_n(sd, tower, every_n if spec.get("every_n_given") else 0, ck, "--ensemble_every_n / --cascade_every_n")
            check_nextvlad_shapes(get_reader(), sd, tower, ck)
            members.append((d, tower, every_n))
            continue
        members.append((d, member_tower(sd, word, ck), every_n))
        if members[-1][1] == "student":
            warn_sampling(sd, sampling, ck)
    return sds, members, cks


def member_specs(reader, members, sampling, sds=None):
    """The entries EnsembleGraph / CascadeGraph build their members from: (tower, every_n, sampling) for an H-LSTM member, and with a
    fourth element - the NeXtVladEvalGraph keywords of the --nextvlad_* flags - for a member whose checkpoint (sds) is a NeXtVLAD one."""
    out = []
    for i, ((_, tower, every_n), s) in enumerate(zip(members, sampling)):
        if sds is not None and checkpoint_family(sds[i]) == "nextvlad":
            cs, hs, g, ex, gr, mx = nextvlad_size_flags()
            out.append((tower, every_n, "uniform", dict(cluster_size=cs, hidden_size=hs, groups=g, expansion=ex, gating_reduction=gr)))
        else:
            out.append((tower, every_n, s))
    return out


def build_ensemble_graph(reader, members, batch_size, device, sampling=None, sds=None):
    """Forward-only graphs of an ensemble's members (members: (dir, tower, every_n); sampling: the members' --ensemble_sampling words, None =
    --student_sampling for all); sizes, --precision and --student_sampling_seed shared.  sds: the members' checkpoints - a NeXtVLAD one
    makes its member a NeXtVladEvalGraph (member_specs)."""
    sampling = sampling or [FLAGS.student_sampling] * len(members)
    return EnsembleGraph(batch_size, member_specs(reader, members, sampling, sds),
                         feature_size=sum(reader.feature_sizes),
                         vocab_size=reader.num_classes, max_frames=FLAGS.max_num_frames, num_inputs_to_lstm=FLAGS.num_inputs_to_lstm,
                         lstm_cells=FLAGS.lstm_cells, lstm_layers=FLAGS.lstm_layers, num_mixtures=FLAGS.moe_num_mixtures, device=device,
                         precision=FLAGS.precision, sampling_seed=FLAGS.student_sampling_seed)


def build_cascade_graph(reader, members, batch_size, device, spec, sds=None):
    """Forward-only graphs of a cascade's stages (members: (dir, tower, every_n), cheapest first; spec: cascade_spec()); sizes, --precision
    and --student_sampling_seed shared.  sds: as build_ensemble_graph."""
    from .cascade import CascadeGraph
    return CascadeGraph(batch_size, member_specs(reader, members, spec["sampling"], sds),
                        confidence=spec["confidence"], thresholds=spec["thresholds"], fractions=spec["fractions"],
                        feature_size=sum(reader.feature_sizes), vocab_size=reader.num_classes, max_frames=FLAGS.max_num_frames,
                        num_inputs_to_lstm=FLAGS.num_inputs_to_lstm, lstm_cells=FLAGS.lstm_cells, lstm_layers=FLAGS.lstm_layers,
                        num_mixtures=FLAGS.moe_num_mixtures, device=device, precision=FLAGS.precision,
                        sampling_seed=FLAGS.student_sampling_seed)


def build_graph(reader, tower, batch_size, device):
    """Forward-only graph of the one tower served (EvalGraph: the validate / eval_finetune forward, row plans and --precision)."""
    return EvalGraph(batch_size, every_n=FLAGS.every_n, student_only=tower == "student", teacher_only=tower == "teacher",
                     feature_size=sum(reader.feature_sizes), vocab_size=reader.num_classes, max_frames=FLAGS.max_num_frames,
                     num_inputs_to_lstm=FLAGS.num_inputs_to_lstm, lstm_cells=FLAGS.lstm_cells, lstm_layers=FLAGS.lstm_layers,
                     num_mixtures=FLAGS.moe_num_mixtures, device=device, precision=FLAGS.precision,
                     student_sampling=FLAGS.student_sampling, sampling_seed=FLAGS.student_sampling_seed)


def _open_device():
    torch.cuda.set_device(FLAGS.gpu)
    ops.check_device(FLAGS.gpu)
    return "cuda:%d" % FLAGS.gpu


def _single_selector(reader, train_dir, batch_size, top_k, stats):
    """The one tower of --train_dir: (select, device) with select(ids, q, labels, n, n_host) -> (values, indices) on the device.  A
    missing checkpoint is reported before the device is touched."""
    ck = latest_checkpoint(train_dir)
    if ck is None:
        raise IOError("unable to find a checkpoint at location: %s" % train_dir)
    logging.info("restoring variables from " + ck)
    sd = torch.load(ck, map_location="cpu")
    family = check_model_family(sd, ck)                                  # (everything refused here is refused before the device is touched)
    if family == "nextvlad":
        tower = nextvlad_tower(sd, FLAGS.serve_tower, ck)
        every_n = nextvlad_every_n(sd, tower, FLAGS.nextvlad_serve_every_n, ck)
        check_nextvlad_shapes(reader, sd, tower, ck)
        device = _open_device()
        graph = nextvlad_graph(reader, sd, tower, every_n, batch_size, device, where=ck)
    else:
        tower, every_n = member_tower(sd, FLAGS.serve_tower, ck), FLAGS.every_n
        device = _open_device()
        graph = build_graph(reader, tower, batch_size, device)
    graph.restore(sd)
    if tower == "student":
        warn_sampling(sd, FLAGS.student_sampling, ck)
    logging.info("serving the %s tower (%s/*)%s", tower, "model" if tower == "teacher" else "model_student",
                 " at every_n = %d" % every_n if tower == "student" or family == "nextvlad" else "")
    stats.update(tower=tower, checkpoint=ck, members=[(train_dir, tower, every_n)])

    def select(ids, q, labels, n, n_host):
        predictions = graph.step(q, labels, n, num_frames_host=n_host)["predictions"]
        return ops.topk_rows(predictions, top_k)                           # same stream, right behind the MoE head
    return select, device


def _ensemble_selector(reader, spec, batch_size, top_k, stats):
    """The members of --ensemble_dirs and the files of --preds_pattern: (select, device), select(...) -> (values, indices) of their
    combination.  Unreadable prediction files and missing checkpoints are reported before the device is touched."""
    tables = []
    for path in spec["files"]:
        logging.info("reading: " + path)
        tables.append(read_prediction_file(path, reader.num_classes))
    kp = prior_list_length(tables)
    sds, members, cks = load_members(spec)
    device = _open_device()
    graph = build_ensemble_graph(reader, members, batch_size, device, spec["sampling"], sds)
    graph.restore(sds)
    for (d, tower, every_n), s in zip(members, spec["sampling"]):
        logging.info("ensemble member: the %s tower of %s%s", tower, d, " at every_n = %d, %s frames" % (every_n, s) if tower == "student" else "")
    logging.info("ensemble: %d members + %d prediction files, mode %s", len(members), len(tables), spec["mode"])
    stats.update(tower="ensemble", checkpoint=cks, members=members)

    def select(ids, q, labels, n, n_host):
        priors = None
        if tables:                                                         # this batch's lists: pinned arrays, copied on the stream
            shape = (len(tables), len(ids), kp)
            idx_h, val_h = torch.empty(shape, dtype=torch.int32, pin_memory=True), torch.empty(shape, dtype=torch.float32, pin_memory=True)
            gather_priors(tables, spec["files"], ids, kp, out=(idx_h.numpy(), val_h.numpy()))
            priors = (idx_h.to(device, non_blocking=True), val_h.to(device, non_blocking=True))
        preds = graph.step(q, labels, n, num_frames_host=n_host)
        return ops.ensemble_topk_rows(preds, top_k, mode=spec["mode"], weights=spec["weights"], priors=priors)
    return select, device


def log_cascade_stages(spec, members):
    for k, ((d, tower, every_n), s) in enumerate(zip(members, spec["sampling"])):
        logging.info("cascade stage %d: the %s tower of %s%s", k, tower, d, " at every_n = %d, %s frames" % (every_n, s) if tower == "student" else "")
    logging.info("cascade: %d stages, confidence %s, thresholds %s, fractions %s", len(members), spec["confidence"], spec["thresholds"],
                 spec["fractions"])


def cascade_shares(stage_videos, stage_frames):
    """The closing line of a cascade run: the share of the videos each stage ran, and the mean frames read per video over all stages."""
    total = max(int(stage_videos[0]), 1) if stage_videos else 1
    return "stage videos %s (%s), stage frames %s, mean frames read per video %.1f" % (
        list(stage_videos), " ".join("%.1f%%" % (100.0 * v / total) for v in stage_videos), list(stage_frames), sum(stage_frames) / total)


def _cascade_selector(reader, spec, batch_size, top_k, stats):
    """The stages of --cascade_dirs: (select, device), select(...) -> (values, indices, {stage_of, confidence}) of the merged predictions.
    Missing checkpoints are reported before the device is touched."""
    sds, members, cks = load_members(spec)
    device = _open_device()
    graph = build_cascade_graph(reader, members, batch_size, device, spec, sds)
    graph.restore(sds)
    log_cascade_stages(spec, members)
    K = len(members)
    stats.update(tower="cascade", checkpoint=cks, members=members, stage_videos=[0] * K, stage_frames=[0] * K, gate_wait_s=0.0,
                 stage_steps=graph.stage_steps)

    def select(ids, q, labels, n, n_host):
        out = graph.step(q, labels, n, num_frames_host=n_host)
        for k in range(K):
            stats["stage_videos"][k] += out["stage_rows"][k]
            stats["stage_frames"][k] += out["stage_frames"][k]
        stats["gate_wait_s"] += out["gate_wait_s"]
        values, indices = ops.topk_rows(out["predictions"], top_k)         # same stream, right behind the last gate
        return values, indices, {"stage_of": out["stage_of"], "confidence": out["confidence"]}
    return select, device


def inference(reader, train_dir, data_pattern, out_file_location, batch_size, top_k, ensemble=None, cascade=None):
    """cs/inference_ensemble.py:113-210.  ensemble: None = the one tower of train_dir, else an ensemble_spec() (train_dir is then not
    consulted); cascade: a cascade_spec() instead (stats then carry stage_videos / stage_frames [K] and gate_wait_s).  Returns the counts, the members served as (dir, tower, every_n) and the host-side time split: reader_wait_s (blocked
    on the reader threads / staging), fetch_wait_s (blocked on a batch's values + indices), format_s (text formatting and writing)."""
    files = sorted(glob.glob(data_pattern))
    if not files:
        raise IOError("Unable to find input files. data_pattern='" + data_pattern + "'")
    logging.info("number of input files: " + str(len(files)))
    stats = dict(tower=None, checkpoint=None, members=None, videos=0, batches=0, reader_wait_s=0.0, fetch_wait_s=0.0, format_s=0.0)
    stage_file = None
    if cascade is not None:
        select, device = _cascade_selector(reader, cascade, batch_size, top_k, stats)
        if cascade["stage_file"]:
            from .cascade import STAGE_FILE_HEADER, format_stage_lines
            stage_file = open(cascade["stage_file"], "w")
            stage_file.write(STAGE_FILE_HEADER)
    elif ensemble is None:
        select, device = _single_selector(reader, train_dir, batch_size, top_k, stats)
    else:
        select, device = _ensemble_selector(reader, ensemble, batch_size, top_k, stats)
    pipe = readers.get_input_evaluation_tensors(reader, files, batch_size=batch_size, num_readers=FLAGS.num_readers, device=device,
                                                with_host_counts=True)
    fetcher = utils.AsyncFetcher(device)
    start = time.time()
    with open(out_file_location, "w") as out_file:
        out_file.write(HEADER)

        def write(pending):
            """The host side of one batch, run while the GPU already works on the next one."""
            ids, handle = pending
            t0 = time.perf_counter()
            got = fetcher.result(handle)
            t1 = time.perf_counter()
            out_file.writelines(format_lines(ids, got["values"], got["indices"]))
            if stage_file is not None:
                stage_file.writelines(format_stage_lines(ids, got["stage_of"], got["confidence"]))
            stats["fetch_wait_s"] += t1 - t0
            stats["format_s"] += time.perf_counter() - t1
            stats["videos"] += len(ids)
            logging.info("num examples processed: %d elapsed seconds: %.2f", stats["videos"], time.time() - start)

        pending = None
        batches = iter(pipe)
        while True:
            t0 = time.perf_counter()
            try:
                ids, q, labels, n, n_host = next(batches)
            except StopIteration:
                break
            stats["reader_wait_s"] += time.perf_counter() - t0
            selected = select(ids, q, labels, n, n_host)
            handle = fetcher.fetch(dict({"values": selected[0], "indices": selected[1]}, **(selected[2] if len(selected) > 2 else {})))
            stats["batches"] += 1
            if pending is not None:
                write(pending)
            pending = (ids, handle)
        if pending is not None:
            write(pending)
    if stage_file is not None:
        stage_file.close()
    stats["seconds"] = time.time() - start
    logging.info("Done with inference. The output file was written to " + out_file_location)
    logging.info("%d videos in %.2f s: reader wait %.2f s, fetch wait %.2f s, formatting %.2f s", stats["videos"], stats["seconds"],
                 stats["reader_wait_s"], stats["fetch_wait_s"], stats["format_s"])
    if cascade is not None:
        logging.info("cascade: %s, gate wait %.2f s", cascade_shares(stats["stage_videos"], stats["stage_frames"]), stats["gate_wait_s"])
    return stats


def main(argv=None):
    FLAGS.parse(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(level=logging.INFO, format="INFO:evc:%(message)s")
    ensemble = check_flags()
    cascade = cascade_spec()
    reader = get_reader()
    return inference(reader, FLAGS.train_dir, FLAGS.input_data_pattern, FLAGS.output_file, FLAGS.batch_size, FLAGS.top_k, ensemble, cascade)


if __name__ == "__main__":
    main()
