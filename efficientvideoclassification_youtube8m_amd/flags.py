"""The reference's command-line flag surface.

Same names, defaults and syntax as the tf.flags definitions scattered over
cs/train.py:27-99, cs/frame_level_models.py:16-47, cs/video_level_models.py:14-19
and cs/validate.py:22-61: ``--flag value``, ``--flag=value``, booleans as a
separate token (``--frame_features True``, run_train.sh:6) or bare, list
strings with spaces (``--feature_names "rgb, audio"``); unknown flags are
tolerated (run_validate.sh:4 passes flags validate.py never defines).
"""
from __future__ import annotations

_DEFS = {}


def _define(name, default, typ, help_=""):
    _DEFS[name] = (default, typ, help_)


def _sampling(v):
    """A --student_sampling word, checked while the flags are parsed: an unknown one is a ValueError before anything touches the device."""
    from .ops import check_student_sampling
    return check_student_sampling(str(v).strip(), "--student_sampling")


def _distill_losses(v):
    """A --distill_losses list, checked while the flags are parsed (distill.check_distill_losses); kept as the canonical comma list."""
    from .distill import check_distill_losses
    return ",".join(check_distill_losses(str(v)))


def _serial_sampling(v):
    """A --serial_sampling list: one --student_sampling word per student, each checked while the flags are parsed; '' stays ''."""
    v = str(v).strip()
    return ",".join(_sampling(w) for w in v.split(",")) if v else ""


def _serial_losses(v):
    """A --serial_losses list: one '+'-joined --distill_losses subset per student, each canonicalised (distill.check_distill_losses)
    while the flags are parsed; '' stays ''."""
    from .distill import check_distill_losses
    v = str(v).strip()
    return ",".join("+".join(check_distill_losses([w.strip() for w in e.split("+")])) for e in v.split(",")) if v else ""


def _serial_every_n(v):
    """A --serial_every_n list: one positive integer per student; '' stays ''."""
    v = str(v).strip()
    if not v:
        return ""
    try:
        vals = [int(e) for e in v.split(",")]
    except ValueError:
        vals = [0]
    if min(vals) <= 0:
        raise ValueError("--serial_every_n %r: a comma list of positive integers, one per student" % v)
    return ",".join(str(e) for e in vals)


def _bool(v):
    if isinstance(v, bool):
        return v
    s = str(v).strip().lower()
    if s in ("true", "t", "1", "yes"):
        return True
    if s in ("false", "f", "0", "no"):
        return False
    raise ValueError("not a boolean: %r" % (v,))


# ---- cs/train.py:27-99 ------------------------------------------------------
_define("train_dir", "/tmp/yt8m_model/", str, "directory for checkpoints and logs")
_define("train_data_pattern", "", str, "glob of tf.SequenceExample records; '' or 'synthetic' = synthetic batches")
_define("feature_names", "rgb", str, "comma separated feature names")
_define("feature_sizes", "1024", str, "comma separated feature widths")
_define("frame_features", True, _bool)
_define("bagging", False, _bool)
_define("model", "HierarchicalLstmModel", str)
_define("start_new_model", False, _bool)
_define("batch_size", 1024, int)
_define("every_n", 1, int)
_define("label_loss", "CrossEntropyLoss", str)
_define("label_loss_counts_file", "counts_tv", str, "CrossEntropyLossClassImbalance: the file of class counts, one integer per line, one line per "
        "class (the reference opens 'counts_tv' in the working directory, cs/losses.py:107)")
_define("dropout", 0.5, float, "the reference's flag: a KEEP probability that cs/train.py hands to create_model, where its video-level "
        "MLP models apply it and the frame-level models this project ports ignore it; nothing here reads it.  It is not "
        "--nextvlad_dropout, the drop rate of the NeXtVLAD tower")
_define("regularization_penalty", 2.0, float)
_define("base_learning_rate", 0.001, float)
_define("learning_rate_decay", 1.0, float)
_define("learning_rate_decay_examples", 4000000.0, float)
_define("num_epochs", 10, int)
_define("num_readers", 4, int)
_define("optimizer", "AdamOptimizer", str)
_define("gpu", 0, int)
_define("clip_gradient_norm", 1.0, float)
_define("log_device_placement", False, _bool)
# ---- cs/frame_level_models.py:16-47 ---------------------------------------------
_define("iterations", 30, int)
_define("dbof_add_batch_norm", True, _bool)
_define("ppfs_normalize", False, _bool)
_define("sample_random_frames", True, _bool)
_define("dbof_cluster_size", 8192, int)
_define("dbof_hidden_size", 1024, int)
_define("dbof_pooling_method", "max", str)
_define("video_level_classifier_model", "MoeModel", str)
_define("lstm_cells", 1024, int)
_define("input_features", 1024, int)
_define("lstm_layers", 1, int)
_define("a_rate", "2", str)          # a *string* flag with an int default in the reference (:40)
_define("num_conv2d_layers", 4, int)
_define("filter_size", 10, int)
_define("max_num_frames", 300, int)
_define("num_inputs_to_lstm", 20, int)
_define("att_hid_size", 100, int)
# ---- cs/video_level_models.py:14-19 -----------------------------------------------
_define("moe_num_mixtures", 2, int)
_define("num_hidden_units", 1024, int)
# ---- cs/validate.py:22-61 (eval binaries) --------------------------------------------
_define("eval_data_pattern", "", str)
_define("run_once", False, _bool)
_define("top_k", 20, int)
# ---- cs/inference_ensemble.py:28-61 (inference binary; train_dir, top_k and the model / input flags as above) -------------
_define("output_file", "", str, "the file to save the predictions to")
_define("input_data_pattern", "", str, "glob of the tf.SequenceExample records to predict (labels not needed)")
# ---- additions of this build (not in the reference) --------------------------------
_define("max_steps", 0, int, "stop after this many iterations (0 = until the data ends)")
_define("synthetic_videos", 2048, int, "videos per epoch when train_data_pattern is synthetic")
_define("teacher_only", False, _bool, "HierarchicalLstmModel: train the teacher tower alone (BASELINE cfg 2; the reference "
        "always builds the student too, also at every_n=1)")
_define("precision", "bf16", str, "'bf16' (one bf16 MFMA product per forward contraction), 'high' (holds 1e-3 on logits at trained "
        "magnitudes: every forward product on IEEE f16 operands with the low-order halves of its weights - for the L1 level also of the input "
        "frames, for the MoE head of both operands - as OCP e4m3 operands on the MX-scaled MFMA behind the f16 stages of the same launch; the top layer of the L1 level "
        "contracts time-dithered f16 weight images instead (EVC_HIGH_DITHER_LAYERS, DESIGN.md 7); "
        "fixed power-of-two e4m3 scales: |x|, |h| <= 1, |W| < 4, head input |state| < 7, head weights |W| < 3.5 never clamp, larger values "
        "saturate at 448 and only lose their correction - engine.HLstmTower.fp8_saturation() counts them; the resolved layout depends on "
        "the EVC_HIGH_* environment and on the student's length and is logged / checkpointed as `precision_layout`) or "
        "'split' (split-bf16 operands, f32-operand accuracy, in every forward GEMM)")
_define("netvlad_cluster_size", 64, int, "NetVLADModel (extension): number of clusters")
_define("netvlad_hidden_size", 1024, int, "NetVLADModel (extension): width of the hidden layer after the aggregation")
_define("netvlad_frames", "sampled", str, "NetVLADModel (extension, DESIGN.md 7.18): sampled (--iterations <= 64 frames drawn per video and "
        "step) | grid (the frames 0, every_n, 2 every_n, ... of each video's real frames, a different number per video, packed without "
        "padding: --every_n 1 is every real frame, the teacher's input; --every_n 10 or 30 the fewer-frames student's; --iterations is not read)")
_define("netvlad_gating", False, _bool, "NetVLADModel (extension, DESIGN.md 7.21): the context gate of 'Learnable pooling with Context Gating' "
        "between the hidden layer and the MoE head, state = h6 * sigmoid(gating_bn(h6 . gating_weights)), in both --netvlad_frames modes; "
        "with --teacher_dir it is the student's gate (the frozen teacher's is read from its checkpoint).  One rank only")
_define("netvlad_serve_every_n", 0, int, "validate with --model NetVLADModel (DESIGN.md 7.18): the grid the served tower runs on, every N-th "
        "real frame; 0 = as the checkpoint records (its every_n for a --netvlad_frames grid checkpoint, 1 - every real frame - for a sampled "
        "one).  Another N than the recorded one is a legitimate experiment: the flag wins, with a warning")
_define("nextvlad_cluster_size", 64, int, "NeXtVLADModel (extension): number of clusters")
_define("nextvlad_hidden_size", 1024, int, "NeXtVLADModel (extension): width of the hidden layer after the aggregation")
_define("nextvlad_groups", 8, int, "NeXtVLADModel (extension): number of groups the expanded frame is split into")
_define("nextvlad_expansion", 2, int, "NeXtVLADModel (extension): expanded width = nextvlad_expansion x feature size")
_define("nextvlad_gating_reduction", 8, int, "NeXtVLADModel (extension): context gating bottleneck = nextvlad_hidden_size / nextvlad_gating_reduction")
_define("nextvlad_frames", "sampled", str, "NeXtVLADModel (extension): sampled (--iterations frames drawn per video and step) | grid (the frames "
        "0, every_n, 2 every_n, ... of each video's real frames, a different number per video, packed without padding: --every_n 1 is every real "
        "frame, the teacher's input; --every_n 10 or 30 the fewer-frames student's; --iterations is not read)")
_define("nextvlad_dropout", 0.0, float, "NeXtVLADModel (extension, DESIGN.md 7.17): the DROP rate in [0, 1) applied to the hidden layer's "
        "input in training (the paper trains with 0.5; 0 = off, the default).  The mask is a stateless function of "
        "(--nextvlad_dropout_seed, data-parallel rank, global_step, element), generated on the device where it is consumed and never stored: "
        "a run restored from a checkpoint continues with the masks an uninterrupted run would have drawn.  validate / inference never drop")
_define("nextvlad_dropout_seed", 0, int, "NeXtVLADModel: the seed of the --nextvlad_dropout masks (a 32-bit key word)")
_define("nextvlad_serve_every_n", 0, int, "validate / inference with --model NeXtVLADModel (DESIGN.md 7.15): the grid the served tower runs "
        "on, every N-th real frame; 0 = the grid its checkpoint records (model_student/*: every_n; model/*: the teacher's grid, 1 for a "
        "--nextvlad_frames sampled checkpoint).  Another N than the recorded one is a legitimate experiment: the flag wins, with a warning")
_define("serve_tower", "auto", str, "inference: auto|teacher|student - the tower of --train_dir's checkpoint that is served.  auto: for "
        "HierarchicalLstmModel the tower its variables name (inference.serving_tower: model/* before model_student/*); for NeXtVLADModel "
        "model_student/* when the checkpoint holds it (the student is what a --teacher_dir run produces), else model/*")
_define("log_every", 1, int, "host metrics / logging period in iterations (the reference logs every step)")
_define("metrics_on_device", False, _bool, "validate / eval_finetune: select what Hit@1 / PERR / GAP / mAP need from each batch on the device "
        "(ops.eval_select_rows) and fetch [B, top_k] + a few [B] vectors instead of the [B, 4716] predictions and labels; same metrics bit "
        "for bit except for rows with an exact tie at the top_k-th / label-count-th place, where the device admits the lowest class "
        "(eval_util.EvaluationMetrics.accumulate_selected); needs 1 <= top_k <= min(256, classes)")
# ---- which frames the student sees (train, train_finetune, train_convert_model, validate, eval_finetune, inference) ----------------------
_define("student_sampling", "uniform", _sampling, "uniform|first|middle|last|first_middle_last|random|change|segment_change: the student's int(n/300*S) frames are the "
        "grid s * every_n of the padded tensor (uniform: the reference), the first, the middle or the last ones of the video's n frames, three "
        "runs at its start, middle and end, or drawn at random without replacement (kept in time order).  The table is built on the device "
        "(ops.student_frame_select) and the input pass gathers the frames.  random: training draws anew at every iteration (hash of seed, "
        "iteration, position in the global batch, frame); evaluation and inference always use draw 0, so they are deterministic for a given "
        "batching (batch size and order of the records) - another batch size gives a video another position and other frames.  change / "
        "segment_change choose by content: every raw frame is scored on the device by its squared change from the frame before it "
        "(ops.frame_change_keys; the first frame counts as the largest change), and the student sees the k frames of largest change, or of "
        "each of k equal segments of the video the one of largest change; both read every live frame of the batch once more.  Checkpoints "
        "record the word; validate / inference warn when the flag disagrees with it, and the flag wins.  --model NetVLADModel "
        "--netvlad_frames grid: the tower - alone, as --teacher_dir's student, or served by validate - runs on the selected frames "
        "(DESIGN.md 7.20); a sampled NetVLAD tower draws its frames, ignores the word and warns; NeXtVLADModel refuses the words")
_define("student_sampling_seed", 0, int, "seed of --student_sampling random")
_define("ensemble_sampling", "", str, "one --student_sampling word per member (ignored for teachers); '' = --student_sampling for all")
# ---- serial distillation (train): the student against a finished, frozen teacher -----------------------------------------------------------
_define("teacher_dir", "", str, "HierarchicalLstmModel (and NeXtVLADModel with --nextvlad_frames grid, DESIGN.md 7.14, NetVLADModel with --netvlad_frames grid, DESIGN.md 7.19): directory of a finished teacher (train --teacher_only True, or any checkpoint with "
        "model/* variables).  Set: the student is trained against that FROZEN teacher (the paper's Serial training; DistillGraph mode "
        "'serial'): the teacher runs forward only and is never written, one train op per iteration (global_step += 1); the checkpoint keeps "
        "model/* bit-identical to the source next to model_student/*.  On resume both towers come from --train_dir.  Not with "
        "--teacher_only, train_finetune or several ranks")
_define("distill_losses", "rep,pred,ce", _distill_losses, "with --teacher_dir: which of L_REP, L_PRED, L_CE the student is trained on (comma "
        "list out of rep, pred, ce; the default is the reference's total, L_REP counted twice).  A loss left out is still computed and logged")
_define("student_init_from_teacher", False, _bool, "--model NeXtVLADModel or NetVLADModel with --teacher_dir (the grid student against the frozen grid "
        "teacher, distill.NeXtVladDistillGraph / NetVladDistillGraph): True starts a NEW student from the teacher's weights and moving statistics instead of its own "
        "seed; ignored (with a log line) on resume")
# ---- serial distillation of several students against ONE forward of the frozen teacher per batch (train) ---------------------------------
_define("serial_student_dirs", "", str, "with --teacher_dir: comma separated train directories, one per student (1 .. 8).  Set: all of them are "
        "trained in one run against one forward of the frozen teacher per batch (distill.SerialStudentsGraph); every batch is read once and "
        "each directory receives the checkpoints a --teacher_dir run of its own would write.  --train_dir is then not consulted.  On resume "
        "every directory must hold a checkpoint of the same global_step (or none of them any).  HierarchicalLstmModel, --precision bf16, one "
        "rank; not with --teacher_only or train_finetune")
_define("serial_every_n", "", _serial_every_n, "one every_n per --serial_student_dirs entry; '' = --every_n for all")
_define("serial_sampling", "", _serial_sampling, "one --student_sampling word per --serial_student_dirs entry; '' = --student_sampling for all "
        "(--student_sampling_seed is shared)")
_define("serial_losses", "", _serial_losses, "one --distill_losses subset per --serial_student_dirs entry, its words joined with '+' "
        "(rep+pred+ce,rep,rep+pred); '' = --distill_losses for all")
# ---- ensemble distillation (train): one student against SEVERAL frozen teachers, combined as an ensemble combines them -----------------
_define("teacher_dirs", "", str, "comma separated checkpoint directories of 1 .. 8 frozen teachers (a directory may repeat with another "
        "tower).  Set: the student is trained against their combination (distill.EnsembleDistillGraph): every teacher runs forward only, "
        "the predictions are combined as --teacher_mode says, the states by --teacher_rep_weights, one train op per iteration "
        "(global_step += 1).  Entry 0 is a teacher tower; the checkpoint keeps its model/* bit-identical next to model_student/*.  On resume "
        "the student and entry 0 come from --train_dir, the other teachers from --teacher_dirs again (the list must be the recorded one).  "
        "HierarchicalLstmModel, --precision bf16, --label_loss CrossEntropyLoss, one rank; not with --teacher_dir, --serial_student_dirs, "
        "--teacher_only or train_finetune")
_define("teacher_towers", "", str, "one word per --teacher_dirs entry from auto|teacher|student, as --ensemble_towers (student = the "
        "checkpoint's model_student/*, a teaching assistant); '' = auto for all")
_define("teacher_every_n", "", str, "one every_n per --teacher_dirs entry (ignored for teacher towers); '' = --every_n for all")
_define("teacher_sampling", "", str, "one --student_sampling word per --teacher_dirs entry (ignored for teacher towers); '' = "
        "--student_sampling for all")
_define("teacher_mode", "mean", str, "max (per-class maximum) | mean (weighted mean): how the teachers' predictions are combined")
_define("teacher_weights", "", str, "comma separated prediction weights, one per --teacher_dirs entry; --teacher_mode mean only; '' = 1 / J each")
_define("teacher_rep_weights", "", str, "comma separated weights of the teachers' states in L_REP's target; '' = 1,0,...,0: the state of "
        "entry 0 alone (a mean over independently trained teachers has no common basis; over a teacher and the students distilled from it, "
        "it has)")
# ---- offline distillation (train): the student against teacher PREDICTION FILES, no teacher tower in memory ----------------------------
_define("teacher_preds_pattern", "", str, "glob of 1 .. 8 VideoId,LabelConfidencePairs files (what inference --output_file writes for one "
        "tower or a whole ensemble, or any program writing that format), sorted by name.  Set: the student alone is trained against the "
        "lists of every batch's videos (distill.OfflineDistillGraph: the train_finetune step with the loss section "
        "evc_distill_losses_sparse), no teacher runs and none is loaded; the files are combined as --teacher_mode / --teacher_weights say "
        "(one weight per file), --distill_losses defaults to pred,ce and refuses rep (a prediction file carries no state); the checkpoint "
        "is train_finetune's, the student tower alone.  Every training video must be in every file.  HierarchicalLstmModel, --label_loss "
        "CrossEntropyLoss, one rank, real records (synthetic data has no video ids); not with --teacher_dir, --teacher_dirs, "
        "--serial_student_dirs, --teacher_only or train_finetune")
# ---- ensembles (inference / validate; cs/inference_ensemble.py:28-61 has preds_pattern, the others are additions) -----------------------
_define("ensemble_dirs", "", str, "comma separated checkpoint directories of the ensemble's members (1 .. 8); '' = the single model of "
        "--train_dir, which is not consulted otherwise.  Every member runs its forward on the same batch and ops.ensemble_topk_rows "
        "combines and selects in one launch")
_define("ensemble_towers", "", str, "one word per member from auto|teacher|student: auto = the tower the checkpoint's variables name "
        "(inference.serving_tower), student on a train.py checkpoint = its model_student/*; '' = auto for all")
_define("ensemble_every_n", "", str, "one every_n per member (ignored for H-LSTM teachers); '' = --every_n for all.  A NeXtVLAD member (the "
        "family is read from each member's own checkpoint; its sizes are the --nextvlad_* flags) runs on the grid its checkpoint records "
        "when the list is not given or its entry is 0 or empty, as 10,,30")
_define("ensemble_mode", "max", str, "max (per-class maximum, cs/max_ensemble.py) | mean (weighted mean)")
_define("ensemble_weights", "", str, "comma separated weights, one per member and then one per --preds_pattern file; mean mode only; "
        "'' = 1 / (members + files) each")
_define("preds_pattern", "", str, "inference: glob of earlier VideoId,LabelConfidencePairs files, sorted by name, that join the ensemble as "
        "sparse members (a class a file does not list counts 0; cs/inference_ensemble.py:155-193)")
# ---- confidence cascades (inference / validate; an addition): escalate only the videos the cheaper tower is unsure of -------------------
_define("cascade_dirs", "", str, "comma separated checkpoint directories of the cascade's stages, cheapest first (2 .. 8; a directory listed "
        "twice is read once); '' = no cascade.  Stage 0 runs on the whole batch, a gate on the device (ops.cascade_confidence_rows + "
        "ops.cascade_pick_rows) measures how sure each video's prediction is, and only the unsure videos run the next stage: their "
        "settled neighbours get num_frames = 0 and drop out of the row plans.  Under --precision split the row plans are off: the cascade "
        "is correct there but saves nothing.  Not with --ensemble_dirs or --preds_pattern; validate needs --run_once True")
_define("cascade_towers", "", str, "one word per stage from auto|teacher|student, as --ensemble_towers; '' = auto for all")
_define("cascade_every_n", "", str, "one every_n per stage (ignored for H-LSTM teachers); '' = --every_n for all; a NeXtVLAD stage: as "
        "--ensemble_every_n (0 or an empty entry = the grid its checkpoint records)")
_define("cascade_sampling", "", str, "one --student_sampling word per stage (ignored for teachers); '' = --student_sampling for all")
_define("cascade_confidence", "", str, "top1 (the video's largest prediction) | margin (largest - second largest); '' = top1")
_define("cascade_thresholds", "", str, "one value per gate (stages - 1): a video whose confidence is >= t_k is settled at stage k "
        "(-inf: every video settles, inf: every video goes on).  At least one of --cascade_thresholds / --cascade_fractions is needed; "
        "with both the threshold names the candidates and the fraction caps them")
_define("cascade_fractions", "", str, "one value in [0, 1] per gate: at most ceil(f_k * batch rows) videos leave stage k, the least "
        "confident first")
_define("cascade_stage_file", "", str, "inference: also write VideoId,Stage,Confidence per video to this file (the stage that decided "
        "the video and its confidence there, '%f')")


class FlagValues(object):
    def __init__(self):
        self.reset()

    def reset(self):
        self.__dict__["_v"] = {k: d[0] for k, d in _DEFS.items()}
        self.__dict__["_unknown"] = []

    def __getattr__(self, k):
        try:
            return self.__dict__["_v"][k]
        except KeyError:
            raise AttributeError("unknown flag %s" % k)

    def __setattr__(self, k, v):
        if k not in _DEFS:
            raise AttributeError("unknown flag %s" % k)
        self.__dict__["_v"][k] = _DEFS[k][1](v)

    def flag_values_dict(self):
        return dict(self.__dict__["_v"])

    def parse(self, argv):
        """Parses reference-style argv (without the program name); returns the
        list of unknown tokens (ignored, like the reference's launchers rely on)."""
        i, unknown = 0, []
        while i < len(argv):
            tok = argv[i]
            i += 1
            if not tok.startswith("--"):
                unknown.append(tok)
                continue
            body = tok[2:]
            if "=" in body:
                name, val = body.split("=", 1)
            else:
                name, val = body, None
            if name.startswith("no") and name[2:] in _DEFS and _DEFS[name[2:]][1] is _bool and val is None:
                self.__dict__["_v"][name[2:]] = False
                continue
            if name not in _DEFS:
                unknown.append(tok)
                if val is None and i < len(argv) and not argv[i].startswith("--"):
                    unknown.append(argv[i])
                    i += 1
                continue
            typ = _DEFS[name][1]
            if val is None:
                if typ is _bool:
                    if i < len(argv) and not argv[i].startswith("--"):
                        try:
                            self.__dict__["_v"][name] = _bool(argv[i])
                            i += 1
                            continue
                        except ValueError:
                            pass
                    self.__dict__["_v"][name] = True
                    continue
                if i >= len(argv):
                    raise ValueError("flag --%s needs a value" % name)
                val = argv[i]
                i += 1
            self.__dict__["_v"][name] = typ(val)
        self.__dict__["_unknown"] = unknown
        return unknown


FLAGS = FlagValues()


def GetListOfFeatureNamesAndSizes(feature_names, feature_sizes):
    """cs/utils.py:127-148: split on ',' and strip; sizes to int."""
    names = [n.strip() for n in feature_names.split(",")]
    sizes = [int(s) for s in feature_sizes.split(",")]
    if len(names) != len(sizes):
        raise ValueError("length of the feature names (=%d) != length of feature sizes (=%d)" % (len(names), len(sizes)))
    return names, sizes
