"""Evaluation binary with the reference's flag surface: cs/validate.py (teacher +
student restored from a teacher-student checkpoint, student metrics + the
representation loss logged) and, with ``student_only``, cs/eval_finetune.py
(student restored from a finetune checkpoint).

    python -m efficientvideoclassification_youtube8m_amd.validate \
        --eval_data_pattern "./yt8m/validate*.tfrecord" --train_dir ./model_HLSTM_TeaStud_every10_train/ \
        --frame_features True --feature_names "rgb, audio" --feature_sizes "1024, 128" \
        --model "HierarchicalLstmModel" --gpu 0 --batch_size 512 --num_inputs_to_lstm 20 --lstm_layers 2 \
        --every_n 10 --top_k 20 --run_once True                                     # = run_validate.sh

Kept: flags, IOError texts, the per-batch and per-epoch log lines (cs/utils.py:35-126), the
EvaluationMetrics accumulation (Hit@1 / PERR / mAP / GAP@top_k, host float64), "skip this checkpoint"
when the global step has not moved, looping until --run_once.  Replaced: TF session / queue runners
-> readers.get_input_evaluation_tensors + distill.EvalGraph; events file -> events.jsonl.
``--eval_data_pattern synthetic`` evaluates ``--synthetic_videos`` random videos (no data set on the box).
``--metrics_on_device True`` (off by default) keeps the [B, 4716] predictions and labels on the device: ops.eval_select_rows
(evc_eval_select_rows) runs behind the MoE head and the fetch carries [B, top_k] values / classes / labels, two [B] vectors and
the per-class positive counts, which EvaluationMetrics.accumulate_selected turns into the same numbers (ties: see there).
``--ensemble_dirs`` (+ --ensemble_towers / --ensemble_every_n / --ensemble_mode / --ensemble_weights, see inference.py; needs
``--run_once True``) evaluates the combination of several checkpoints: every member runs on the batch, ops.ensemble_topk_rows writes the
combined [B, 4716] predictions, and the loss (--label_loss; by default ops.ce_loss) and the metrics - host or --metrics_on_device - are those of the combination;
no student_state_loss is reported and --train_dir only receives events.jsonl.
``--cascade_dirs`` (+ --cascade_towers / --cascade_every_n / --cascade_sampling / --cascade_confidence / --cascade_thresholds /
--cascade_fractions, see inference.py; needs ``--run_once True``) evaluates a confidence cascade the same way: cascade.CascadeGraph merges
each video's predictions from the last stage that ran it, loss and metrics are those of the merged predictions, and the share of the
videos and the frames each stage read are logged and returned as ``cascade_stage_videos`` / ``cascade_stage_frames``.
``--model NeXtVLADModel`` evaluates a NeXtVLAD checkpoint through vlad_graphs.NeXtVladEvalGraph: a --teacher_dir checkpoint as
teacher + student (the student's metrics, student_loss logged), a single-tower one as model/*, each tower on the grid its checkpoint
records (--nextvlad_serve_every_n overrides); the graph is built for --train_dir's latest checkpoint, which must exist at the start.
Ensemble members and cascade stages take their family from their own checkpoints, so H-LSTM and NeXtVLAD members mix.
``--model NetVLADModel`` evaluates a NetVLAD checkpoint through vlad_graphs.NetVladEvalGraph: model/* as a forward-only grid
tower on the grid the checkpoint records, every real frame for a --netvlad_frames sampled one (--netvlad_serve_every_n overrides); its
variables are checked against the size flags on the host first.  A --teacher_dir checkpoint of this family is evaluated
as teacher + student: the student's metrics on the recorded every_n, student_loss logged against the teacher on the recorded
teacher_every_n.  --student_sampling WORD serves the served tower on the frames that word selects (a warning when the
checkpoint records another word), the teacher next to a served student stays on its recorded frames.  No ensemble or cascade serves this
family.
"""
from __future__ import annotations

import logging
import sys
import time

import numpy as np
import torch

from . import eval_util, frame_level_models, losses, ops, readers, utils, video_level_models
from .distill import EvalGraph
from .flags import FLAGS
from .train import NUM_CLASSES, find_class_by_name, get_reader, latest_checkpoint, synthetic_batches


def get_input_evaluation_tensors(reader, data_pattern, batch_size=1024, num_readers=1, device=None):
    """cs/validate.py:70-104."""
    logging.info("Using batch size of " + str(batch_size) + " for evaluation.")
    try:
        pipe = readers.get_input_evaluation_tensors(reader, data_pattern, batch_size=batch_size, num_readers=num_readers, device=device,
                                                    with_host_counts=True)
    except IOError as e:
        if "Unable to find" in str(e):
            raise IOError("Unable to find the evaluation files.")
        raise
    logging.info("number of evaluation files: " + str(len(pipe.index)))
    return pipe


def nextvlad_source(reader, student_only=False):
    """--model NeXtVLADModel: what is decided on the host, before the device is touched, from --train_dir's latest checkpoint - the graph
    is built for the towers that checkpoint holds and the grids it records.  Returns {"ck", "sd", "tower", "every_n", "teacher_every_n"}:
    tower 'both' for a distillation checkpoint (model/* and model_student/*: the student's metrics, student_state_loss logged),
    'teacher' for a single-tower one; --nextvlad_serve_every_n overrides the served tower's grid."""
    from . import inference
    if student_only:
        raise ValueError("eval_finetune with --model NeXtVLADModel: there is no convert / finetune step for this family, so no "
                         "student-only checkpoint to evaluate; validate evaluates the student of a --teacher_dir run")
    inference.check_nextvlad_serving_flags()
    ck = latest_checkpoint(FLAGS.train_dir)
    if ck is None:
        raise IOError("unable to find a checkpoint at location: %s" % FLAGS.train_dir)
    sd = torch.load(ck, map_location="cpu")
    inference.check_model_family(sd, ck)
    both = any(k.startswith("model_student/") and torch.is_tensor(v) for k, v in sd.items())
    tower = "both" if both else inference.member_tower(sd, "teacher", ck)
    every_n = inference.nextvlad_every_n(sd, "student" if both else "teacher", FLAGS.nextvlad_serve_every_n, ck)
    inference.check_nextvlad_shapes(reader, sd, tower, ck)
    return dict(ck=ck, sd=sd, tower=tower, every_n=every_n, teacher_every_n=inference.nextvlad_every_n(sd, "teacher"))


def netvlad_every_n(state_dict, override=0, where="the checkpoint"):
    """The grid a served NetVLAD tower runs on: the every_n of a --netvlad_frames grid checkpoint, every real frame (1) for a sampled one,
    unless ``override`` (--netvlad_serve_every_n) > 0 names another, which wins with a warning."""
    recorded = int(state_dict["every_n"]) if state_dict.get("netvlad_frames") == "grid" and "every_n" in state_dict else 1
    if override and int(override) != recorded:
        logging.warning("--netvlad_serve_every_n %d, but the tower of %s runs on every_n = %d there (the flag is used)", override, where, recorded)
        return int(override)
    return recorded


def netvlad_source(reader, student_only=False):
    """--model NetVLADModel: what is decided on the host, before the device is touched, from --train_dir's latest
    checkpoint - its variables against the size flags, and the grid it records.  Returns {"ck", "sd", "tower", "every_n",
    "teacher_every_n"}: tower 'both' for a distillation checkpoint (model/* and model_student/* - the student's metrics
    at the recorded every_n, student_state_loss logged against the teacher at the recorded teacher_every_n), 'teacher' for a single-tower
    one; --netvlad_serve_every_n overrides the served tower's grid only.  "gating" / "teacher_gating" (DESIGN.md 7.21): the context gate of
    the served tower and of the teacher next to a served student, each read from its scope's own variables; --netvlad_gating is not
    consulted, a flag that disagrees with the served tower is logged as a warning."""
    from .vlad_graphs import check_netvlad_checkpoint, netvlad_checkpoint_gating
    if student_only:
        raise ValueError("eval_finetune with --model NetVLADModel: there is no convert / finetune step for this family, so no "
                         "student-only checkpoint to evaluate")
    if FLAGS.precision != "bf16":
        raise ValueError("--precision %s with --model NetVLADModel: the NetVLAD tower has no such forward mode (bf16 only)" % FLAGS.precision)
    if FLAGS.netvlad_serve_every_n < 0 or FLAGS.netvlad_serve_every_n > FLAGS.max_num_frames:
        raise ValueError("--netvlad_serve_every_n %d must lie in 0 .. --max_num_frames %d (0 = as the checkpoint records)"
                         % (FLAGS.netvlad_serve_every_n, FLAGS.max_num_frames))
    ck = latest_checkpoint(FLAGS.train_dir)
    if ck is None:
        raise IOError("unable to find a checkpoint at location: %s" % FLAGS.train_dir)
    sd = torch.load(ck, map_location="cpu")
    both = any(k.startswith("model_student/") and torch.is_tensor(v) for k, v in sd.items())
    gates = {}
    for scope in ("model", "model_student") if both else ("model",):
        gates[scope] = netvlad_checkpoint_gating(sd, scope)
        check_netvlad_checkpoint(sd, scope, sum(reader.feature_sizes), reader.num_classes,
                                 (FLAGS.netvlad_cluster_size, FLAGS.netvlad_hidden_size, FLAGS.moe_num_mixtures), ck, gating=gates[scope])
    gating = gates["model_student" if both else "model"]
    if bool(FLAGS.netvlad_gating) != gating:
        logging.warning("--netvlad_gating %s, but the served tower of %s was trained %s the context gate (the checkpoint's variables are used)",
                        FLAGS.netvlad_gating, ck, "with" if gating else "without")
    teacher_every_n = int(sd.get("teacher_every_n", 1)) if both else 1
    #  the served tower runs on --student_sampling; the teacher next to a served student stays on what the checkpoint records
    teacher_sampling = (sd.get("teacher_sampling", "uniform"), int(sd.get("teacher_sampling_seed", 0))) if both else ("uniform", 0)
    return dict(ck=ck, sd=sd, tower="both" if both else "teacher", every_n=netvlad_every_n(sd, FLAGS.netvlad_serve_every_n, ck),
                teacher_every_n=teacher_every_n, teacher_sampling=teacher_sampling, gating=gating, teacher_gating=gates["model"])


def build_graph(reader, model, batch_size, device, student_only=False, label_loss=None, nextvlad=None, netvlad=None):
    """cs/validate.py:107-189 / cs/eval_finetune.py:108-175.  nextvlad: nextvlad_source() for --model NeXtVLADModel;
    netvlad: netvlad_source() for --model NetVLADModel."""
    if isinstance(model, frame_level_models.NetVLADModel):
        from .vlad_graphs import NetVladEvalGraph
        src = netvlad if netvlad is not None else netvlad_source(reader, student_only)
        return NetVladEvalGraph(batch_size, every_n=src["every_n"], feature_size=sum(reader.feature_sizes), vocab_size=reader.num_classes,
                                max_frames=FLAGS.max_num_frames, cluster_size=FLAGS.netvlad_cluster_size,
                                hidden_size=FLAGS.netvlad_hidden_size, num_mixtures=FLAGS.moe_num_mixtures, device=device,
                                precision=FLAGS.precision, label_loss=label_loss, tower=src.get("tower", "teacher"),
                                teacher_every_n=src.get("teacher_every_n", 1), student_sampling=FLAGS.student_sampling,
                                sampling_seed=FLAGS.student_sampling_seed, teacher_sampling=src.get("teacher_sampling", ("uniform", 0))[0],
                                teacher_sampling_seed=src.get("teacher_sampling", ("uniform", 0))[1], gating=src.get("gating", False),
                                teacher_gating=src.get("teacher_gating", False))
    if isinstance(model, frame_level_models.NeXtVLADModel):
        from . import inference
        src = nextvlad if nextvlad is not None else nextvlad_source(reader, student_only)
        return inference.nextvlad_graph(reader, src["sd"], src["tower"], src["every_n"], batch_size, device, where=src["ck"],
                                        teacher_every_n=src["teacher_every_n"], label_loss=label_loss)
    if not isinstance(model, frame_level_models.HierarchicalLstmModel):
        raise NotImplementedError("validate.py unpacks the H-LSTM (state, result) pair (cs/validate.py:150,157); "
                                  "model %s cannot be evaluated by the reference either" % type(model).__name__)
    return EvalGraph(batch_size, every_n=FLAGS.every_n, student_only=student_only, feature_size=sum(reader.feature_sizes),
                     vocab_size=reader.num_classes, max_frames=FLAGS.max_num_frames, num_inputs_to_lstm=FLAGS.num_inputs_to_lstm,
                     lstm_cells=FLAGS.lstm_cells, lstm_layers=FLAGS.lstm_layers, num_mixtures=FLAGS.moe_num_mixtures, device=device,
                     precision=FLAGS.precision, student_sampling=FLAGS.student_sampling, sampling_seed=FLAGS.student_sampling_seed,
                     label_loss=label_loss)


def build_ensemble(reader, model, spec, batch_size, device, label_loss=None, loaded=None):
    """The members of an inference.ensemble_spec(), restored, behind one step() that returns their combination.  loaded: the result of
    inference.load_members(spec) when the caller has read the checkpoints already (evaluate: before the device is touched)."""
    from . import inference
    if not isinstance(model, (frame_level_models.HierarchicalLstmModel, frame_level_models.NeXtVLADModel)):
        raise NotImplementedError("an ensemble serves H-LSTM and NeXtVLAD teacher / student towers; model %s has no path here" % type(model).__name__)
    sds, members, _ = loaded if loaded is not None else inference.load_members(spec)
    graph = inference.build_ensemble_graph(reader, members, batch_size, device, spec["sampling"], sds)
    graph.restore(sds)
    for d, tower, every_n in members:
        logging.info("ensemble member: the %s tower of %s%s", tower, d, " at every_n = %d" % every_n if tower == "student" else "")
    return _CombinedMembers(graph, spec, max(int(sd.get("global_step", 0)) for sd in sds), label_loss)


def build_cascade(reader, model, spec, batch_size, device, label_loss=None, loaded=None):
    """The stages of an inference.cascade_spec(), restored, behind one step() that returns the merged predictions.  loaded: as
    build_ensemble."""
    from . import inference
    if not isinstance(model, (frame_level_models.HierarchicalLstmModel, frame_level_models.NeXtVLADModel)):
        raise NotImplementedError("a cascade serves H-LSTM and NeXtVLAD teacher / student towers; model %s has no path here" % type(model).__name__)
    sds, members, _ = loaded if loaded is not None else inference.load_members(spec)
    graph = inference.build_cascade_graph(reader, members, batch_size, device, spec, sds)
    graph.restore(sds)
    inference.log_cascade_stages(spec, members)
    return _CascadeStages(graph, spec, max(int(sd.get("global_step", 0)) for sd in sds), label_loss)


def _batches(reader, device):
    if FLAGS.eval_data_pattern == "synthetic":
        for i, (q, y, n, nh) in enumerate(synthetic_batches(FLAGS.batch_size, sum(reader.feature_sizes), device, FLAGS.synthetic_videos, 1, 4321)):
            yield ["syn%06d" % (i * FLAGS.batch_size + j) for j in range(q.shape[0])], q, y, n, nh
    else:
        for b in get_input_evaluation_tensors(reader, FLAGS.eval_data_pattern, FLAGS.batch_size, FLAGS.num_readers, device):
            yield b


def check_flags():
    """What is refused before a record is read or the device is touched.  Returns the ensemble to evaluate (inference.ensemble_spec) or None."""
    if FLAGS.metrics_on_device:
        top_max = min(ops.TOPK_MAX_K, NUM_CLASSES)
        if not 1 <= FLAGS.top_k <= top_max:
            raise ValueError("--top_k %d: must be in [1, %d] with --metrics_on_device" % (FLAGS.top_k, top_max))
    from .inference import cascade_spec, ensemble_spec
    if cascade_spec() is not None and not FLAGS.run_once:
        raise ValueError("--cascade_dirs needs --run_once True: there is no one directory to poll for the checkpoints of several stages")
    spec = ensemble_spec(allow_preds_files=False)
    if spec is not None and not FLAGS.run_once:
        raise ValueError("--ensemble_dirs needs --run_once True: there is no one directory to poll for the checkpoints of several members")
    return spec


class _CombinedMembers:
    """An ensemble behind the step() of an EvalGraph: the members' predictions combined by ops.ensemble_topk_rows (its dense output)
    as "predictions", and the label loss of the combination (--label_loss; CrossEntropyLoss: ops.ce_loss) as "loss"."""

    def __init__(self, graph, spec, global_step, label_loss=None):
        self.graph, self.spec, self.global_step = graph, spec, global_step
        self.label_loss = losses.resolve(label_loss)
        self.teacher = self.student = None
        self._loss = None

    def step(self, x_raw, labels_u8, num_frames, num_frames_host=None):
        preds = self.graph.step(x_raw, labels_u8, num_frames, num_frames_host=num_frames_host)
        _, _, combined = ops.ensemble_topk_rows(preds, 0, mode=self.spec["mode"], weights=self.spec["weights"], dense=True)
        if self._loss is None:
            self._loss = torch.zeros(1, dtype=torch.float32, device=combined.device)
        self._loss.zero_()
        self.label_loss.fused(combined, labels_u8, self._loss[0:1])
        return {"predictions": combined, "loss": self._loss[0]}


class _CascadeStages(_CombinedMembers):
    """A cascade behind the step() of an EvalGraph: cascade.CascadeGraph's merged matrix as "predictions", its label loss (--label_loss) as
    "loss"; the rows and frames of every stage are summed over the batches (``stage_videos`` / ``stage_frames`` / ``gate_wait_s``)."""

    def __init__(self, graph, spec, global_step, label_loss=None):
        super().__init__(graph, spec, global_step, label_loss)
        self.reset()

    def reset(self):
        K = len(self.graph.graphs)
        self.stage_videos, self.stage_frames, self.gate_wait_s = [0] * K, [0] * K, 0.0

    def step(self, x_raw, labels_u8, num_frames, num_frames_host=None):
        out = self.graph.step(x_raw, labels_u8, num_frames, num_frames_host=num_frames_host)
        for k, (r, f) in enumerate(zip(out["stage_rows"], out["stage_frames"])):
            self.stage_videos[k] += r
            self.stage_frames[k] += f
        self.gate_wait_s += out["gate_wait_s"]
        merged = out["predictions"]
        if self._loss is None:
            self._loss = torch.zeros(1, dtype=torch.float32, device=merged.device)
        self._loss.zero_()
        self.label_loss.fused(merged, labels_u8, self._loss[0:1])
        return {"predictions": merged, "loss": self._loss[0]}


def evaluation_loop(graph, reader, label_loss_fn, summary_writer, evl_metrics, last_global_step_val, device):
    """Run the evaluation loop once (cs/validate.py:192-303).  Returns (global_step_val, epoch_info_dict or None)."""
    if isinstance(graph, _CascadeStages):
        graph.reset()
        step, info = _evaluate_restored(graph, reader, label_loss_fn, summary_writer, evl_metrics, graph.global_step, device)
        if info is not None:
            from .inference import cascade_shares
            info["cascade_stage_videos"], info["cascade_stage_frames"] = list(graph.stage_videos), list(graph.stage_frames)
            logging.info("cascade: %s, gate wait %.2f s", cascade_shares(graph.stage_videos, graph.stage_frames), graph.gate_wait_s)
        return step, info
    if isinstance(graph, _CombinedMembers):                              # restored in evaluate(); --run_once: nothing to poll
        return _evaluate_restored(graph, reader, label_loss_fn, summary_writer, evl_metrics, graph.global_step, device)
    ck = latest_checkpoint(FLAGS.train_dir)
    if not ck:
        logging.info("No checkpoint file found.")
        return -1, None
    logging.info("Loading checkpoint for eval: " + ck)
    try:
        sd = torch.load(ck, map_location="cpu")
    except FileNotFoundError as e:
        # the trainer replaced the file between the directory listing and the load (max_to_keep=1) - the only race an
        # atomic writer (train.save_checkpoint: temp file, fsync, os.replace) leaves; look again at the next poll.
        # Anything else (a corrupt or incompatible file) is an error of THIS checkpoint and propagates: polling it
        # forever - or ending a --run_once evaluation with no result and no failure - would hide it.
        logging.info("checkpoint %s disappeared before it could be loaded (%s); will look again.", ck, e)
        return last_global_step_val, None
    from .inference import check_model_family, warn_sampling
    if getattr(graph, "family", None) != "netvlad":                      # (a NetVLAD graph's restore checks every variable's name and shape)
        check_model_family(sd, ck)
    graph.restore(sd)
    if graph.student is not None or getattr(graph, "family", None) == "netvlad":      # (a NetVLAD tower trained alone records its word too)
        warn_sampling(sd, FLAGS.student_sampling, ck)
    global_step_val = int(sd.get("global_step", 0))
    if global_step_val == last_global_step_val:
        logging.info("skip this checkpoint global_step_val=%s (same as the previous one).", global_step_val)
        return global_step_val, None
    return _evaluate_restored(graph, reader, label_loss_fn, summary_writer, evl_metrics, global_step_val, device)


def _evaluate_restored(graph, reader, label_loss_fn, summary_writer, evl_metrics, global_step_val, device):
    """One pass over the evaluation set with the restored graph (cs/validate.py:225-303)."""
    logging.info("enter eval_once loop global_step_val = %s. ", global_step_val)
    evl_metrics.clear()
    examples_processed, total_example_per_sec = 0, []
    on_device = FLAGS.metrics_on_device
    fetcher = utils.AsyncFetcher(device)
    last_time = [time.time()]

    def account(handle):
        """The host side of one batch (cs/validate.py:240-282), run while the GPU already works on the next batch."""
        nonlocal examples_processed
        got = fetcher.result(handle)
        if on_device:
            batch = got["top_val"].shape[0]
        else:
            predictions_val, labels_val = got["predictions"], got["labels"].astype(np.float32)
            batch = labels_val.shape[0]
        loss_val = float(got["loss"].reshape(-1)[0])
        now = time.time()
        seconds_per_batch, last_time[0] = max(now - last_time[0], 1e-9), now
        example_per_second = batch / seconds_per_batch
        total_example_per_sec.append(example_per_second)
        examples_processed += batch
        if on_device:
            iteration_info_dict = evl_metrics.accumulate_selected(got["top_val"], got["top_idx"], got["top_lab"], got["n_pos"],
                                                                  got["perr_hits"], got["class_pos"], loss_val)
        else:
            iteration_info_dict = evl_metrics.accumulate(predictions_val, labels_val, loss_val)
        iteration_info_dict["examples_per_second"] = example_per_second
        iterinfo_pre = ""
        if "student_state_loss" in got:                                 # cs/validate.py:268-275
            student_loss_val = float(got["student_state_loss"].reshape(-1)[0])
            iteration_info_dict["student_loss"] = student_loss_val
            iterinfo_pre = "student_loss: %f | " % student_loss_val
        iterinfo = utils.AddGlobalStepSummary(summary_writer, global_step_val, iteration_info_dict, summary_scope="Eval")
        logging.info("examples_processed: %d | %s%s", examples_processed, iterinfo_pre, iterinfo)

    pending = None
    for ids, q, labels, n, n_host in _batches(reader, device):
        out = graph.step(q, labels, n, num_frames_host=n_host)
        loss_t = out["loss"]                                             # --label_loss, computed by the graph behind the MoE head
        if on_device:                                                    # same stream, right behind the MoE head
            fetch = ops.eval_select_rows(out["predictions"], labels, FLAGS.top_k)
            fetch["loss"] = loss_t.reshape(1)
        else:
            fetch = {"predictions": out["predictions"], "labels": labels, "loss": loss_t.reshape(1)}
        if "student_state_loss" in out:
            fetch["student_state_loss"] = out["student_state_loss"].reshape(1)
        handle = fetcher.fetch(fetch)                                    # the fetch: clones + D2H on a copy stream
        if pending is not None:
            account(pending)                                             # batch k's metrics, under batch k+1
        pending = handle
    if pending is not None:
        account(pending)
    if FLAGS.precision == "high":      # the fixed e4m3 scales of the "high" mode assume bounded operands: say so when the last batch broke them
        for tw, key in ((getattr(graph, "teacher", None), "teacher_state"), (getattr(graph, "student", None), "student_state")):
            if tw is not None and hasattr(tw, "fp8_saturation"):
                sat = {k: v for k, v in tw.fp8_saturation(out.get(key) if pending is not None else None).items() if v}
                if sat:
                    logging.warning("%s: operands beyond the e4m3 scales of --precision high (low-order corrections clamp, the 1e-3 contract "
                                    "degrades): %s - see flags.py / EVC_HIGH_MOE_FP8=0", tw.scope, sat)
    logging.info("Done with batched inference. Now calculating global performance metrics.")
    epoch_info_dict = evl_metrics.get()
    epoch_info_dict["epoch_id"] = global_step_val
    logging.info(utils.AddEpochSummary(summary_writer, global_step_val, epoch_info_dict, summary_scope="Eval"))
    if total_example_per_sec:
        logging.info("Average examples processed in one second %0.20f" % (np.sum(np.asarray(total_example_per_sec)) / len(total_example_per_sec)))
    evl_metrics.clear()
    return global_step_val, epoch_info_dict


def evaluate(student_only=False, max_evals=None):
    """cs/validate.py:306-397.  Returns the last epoch_info_dict (None if nothing was evaluated)."""
    start_time = time.time()
    spec = check_flags()
    if spec is not None and student_only:
        raise ValueError("--ensemble_dirs: evaluate an ensemble with validate.py (each member names its own tower)")
    from .inference import cascade_spec
    cascade = cascade_spec()
    if cascade is not None and student_only:
        raise ValueError("--cascade_dirs: evaluate a cascade with validate.py (each stage names its own tower)")
    if cascade is not None and cascade["stage_file"]:
        raise ValueError("--cascade_stage_file is written by inference.py only")
    reader = get_reader()
    model = find_class_by_name(FLAGS.model, [frame_level_models, video_level_models])()
    nextvlad = netvlad = loaded = None           # the NeXtVLAD / NetVLAD family's host checks, and every member's: before the device is touched
    if isinstance(model, frame_level_models.NeXtVLADModel) and spec is None and cascade is None:
        nextvlad = nextvlad_source(reader, student_only)
    elif isinstance(model, frame_level_models.NetVLADModel) and spec is None and cascade is None:
        netvlad = netvlad_source(reader, student_only)
    elif spec is not None or cascade is not None:
        if isinstance(model, (frame_level_models.HierarchicalLstmModel, frame_level_models.NeXtVLADModel)):
            from .inference import load_members
            loaded = load_members(cascade if cascade is not None else spec)
    elif isinstance(model, frame_level_models.HierarchicalLstmModel):
        ck = latest_checkpoint(FLAGS.train_dir)                          # (a --model that is not this checkpoint's family: refused here)
        if ck:
            from .inference import check_model_family
            try:
                check_model_family(torch.load(ck, map_location="cpu"), ck)
            except FileNotFoundError:
                pass                                                     # replaced by the trainer meanwhile: evaluation_loop looks again
    device = "cuda:%d" % FLAGS.gpu
    torch.cuda.set_device(FLAGS.gpu)
    ops.check_device(FLAGS.gpu)
    label_loss_fn = find_class_by_name(FLAGS.label_loss, [losses])()
    label_loss_fn.check(reader.num_classes)
    if FLAGS.eval_data_pattern == "":
        raise IOError("'eval_data_pattern' was not specified. Nothing to evaluate.")
    if cascade is not None:
        graph = build_cascade(reader, model, cascade, FLAGS.batch_size, device, label_loss=label_loss_fn, loaded=loaded)
    elif spec is None:
        graph = build_graph(reader, model, FLAGS.batch_size, device, student_only, label_loss=label_loss_fn, nextvlad=nextvlad, netvlad=netvlad)
    else:
        graph = build_ensemble(reader, model, spec, FLAGS.batch_size, device, label_loss=label_loss_fn, loaded=loaded)
    logging.info("built evaluation graph")
    for tw in (graph.teacher, graph.student):
        if tw is not None:
            logging.info("Names of %s Parameters ::", "Teacher" if tw is graph.teacher else "Student")
            logging.info(list(tw.state_dict().keys()))
    summary_writer = utils.JsonlSummaryWriter(FLAGS.train_dir)
    evl_metrics = eval_util.EvaluationMetrics(reader.num_classes, FLAGS.top_k)
    last_global_step_val, last, evals = -1, None, 0
    while True:
        last_global_step_val, info = evaluation_loop(graph, reader, label_loss_fn, summary_writer, evl_metrics,
                                                     last_global_step_val, device)
        last = info or last
        evals += 1
        if FLAGS.run_once or (max_evals and evals >= max_evals):
            break
        if info is None:
            time.sleep(10)                                              # wait for the trainer to write a new checkpoint
    summary_writer.close()
    print("Total time taken is " + str(time.time() - start_time))
    return last


def main(argv=None, student_only=False):
    FLAGS.parse(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(level=logging.INFO, format="INFO:evc:%(message)s")
    return evaluate(student_only)


if __name__ == "__main__":
    main()
