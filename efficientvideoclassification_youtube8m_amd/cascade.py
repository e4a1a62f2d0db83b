"""Confidence cascade inference: the cheapest tower runs on the whole batch, a gate on the device measures how sure each row's prediction
is, and only the unsure rows go on to the next, more expensive tower (usually the teacher last).

"Run the next stage on the escalated rows only" needs no packed sub-batch and no forward kernel of its own: the next stage is the same
EvalGraph step with num_frames = 0 for the settled rows, on the device and in the host copy ops.RowPlan takes its launch geometry from.
Rows of length 0 drop out of the input pass and of every L1 kernel (RowPlan.P = round_up(rows[0], 32)), and LstmStack.forward zeroes
the final state of rows no step touches.  What such a row's tower then predicts is never looked at: ops.cascade_confidence_rows copies
into the merged matrix only the rows the stage ran.

A NeXtVLAD stage (vlad_graphs.NeXtVladEvalGraph) takes the same step: its settled rows leave the packed frame rows and - the
graph serving only the videos that have a frame - everything behind the aggregation too.

The gate is ops.cascade_confidence_rows + ops.cascade_pick_rows (csrc/evc_cascade.hip).  Its result has to reach the host, because the
launch geometry of the next stage is host-side: one pinned copy and one wait per gate, timed as ``gate_wait_s``.

The stage bookkeeping (quota, masking of the host counts, the empty-stage skip, the frame accounting) is the pure function
``stage_bookkeeping`` below; tests reach it without a device.
"""
from __future__ import annotations

import math
import time

import numpy as np
import torch

from . import ops
from .distill import member_graph, scored_sampling

F32 = torch.float32


def parse_stage(stage):
    """(tower, every_n, student_sampling | None) of a ``stages`` entry (tower, every_n[, student_sampling[, nextvlad]]); the fourth
    element, the size keywords of a NeXtVLAD stage (distill.member_graph), is read by stage_family."""
    tower, every_n = stage[0], int(stage[1])
    if tower not in ("teacher", "student"):
        raise ValueError("CascadeGraph: tower %r (teacher | student)" % (tower,))
    return tower, every_n, (stage[2] if len(stage) > 2 else None)


def stage_family(stage):
    return "nextvlad" if len(stage) > 3 and stage[3] is not None else "hlstm"


def check_gates(num_stages, confidence, thresholds, fractions, what="CascadeGraph"):
    """The gates of a cascade of num_stages stages, checked: (thresholds [K - 1] floats with +inf where only a fraction is given,
    fractions [K - 1] floats or None).  thresholds / fractions: None or K - 1 values; at least one of them."""
    K = int(num_stages)
    if not 2 <= K <= ops.CASCADE_MAX_STAGES:
        raise ValueError("%s: %d stages (2 .. %d)" % (what, K, ops.CASCADE_MAX_STAGES))
    if confidence not in ops.CASCADE_CONFIDENCE:
        raise ValueError("%s: confidence %r (%s)" % (what, confidence, " | ".join(ops.CASCADE_CONFIDENCE)))
    if thresholds is None and fractions is None:
        raise ValueError("%s: neither thresholds nor fractions - no row would ever leave the first stage" % what)
    for name, given in (("thresholds", thresholds), ("fractions", fractions)):
        if given is not None and len(given) != K - 1:
            raise ValueError("%s: %d %s for %d stages (one per gate: %d)" % (what, len(given), name, K, K - 1))
    th = [float("inf")] * (K - 1) if thresholds is None else [float(t) for t in thresholds]
    fr = None
    if fractions is not None:
        fr = [float(f) for f in fractions]
        for f in fr:
            if not 0.0 <= f <= 1.0:                                     # NaN fails both comparisons
                raise ValueError("%s: fraction %r outside [0, 1]" % (what, f))
    return th, fr


def stage_quota(n_active, fraction, batch_rows):
    """m_k: at most this many rows leave the stage.  -1 (no cap) without a fraction, else min(n_active, ceil(f * b)) in Python float64."""
    if fraction is None:
        return -1
    return min(int(n_active), int(math.ceil(float(fraction) * int(batch_rows))))


def stage_bookkeeping(k, num_stages, active, num_frames_host, tower, every_n, threshold=None, fraction=None, max_frames=300,
                      num_inputs_to_lstm=20, num_inputs_l1_student=5, family="hlstm"):
    """Everything about stage k of a batch that is decided on the host.  active: None (stage 0: every row) or the bool / 0-1 vector [b] the
    gate before this stage returned; num_frames_host: the batch's ORIGINAL counts [b].  Returns a dict:
      run         False when no row is active: the stage's graph is not stepped and nothing is launched;
      rows        active rows;
      nh          int64 [b]: the host counts the stage's graph gets, where(active, num_frames_host, 0);
      frames      frames the stage's tower consumes over its rows (ops.host_frame_counts: the teacher reads n, a student int(n / 300 * S);
                  family "nextvlad", either tower: the grid's ceil(min(n, max_frames) / every_n));
      gate        whether a gate follows (run, and k is not the last stage);
      threshold   the gate's threshold (+inf where only a fraction is given);
      max_rows    the gate's quota stage_quota(rows, fraction, b)."""
    nh0 = np.asarray(num_frames_host, dtype=np.int64).reshape(-1)
    b = nh0.shape[0]
    act = np.ones(b, dtype=bool) if active is None else np.asarray(active).reshape(-1) != 0
    if act.shape[0] != b:
        raise ValueError("stage_bookkeeping: %d active flags for %d rows" % (act.shape[0], b))
    rows = int(act.sum())
    nh = np.where(act, nh0, 0).astype(np.int64)
    if family == "nextvlad":
        used = (np.clip(nh, 0, max_frames) + every_n - 1) // every_n             # (ops.GridPlan's k)
    elif tower == "teacher":
        C = num_inputs_to_lstm
        used = ops.host_frame_counts(nh, 1, C, max_frames // C, max_frames)[0]
    else:
        C, S = num_inputs_l1_student, max_frames // every_n
        used = ops.host_frame_counts(nh, every_n, C, S // C, max_frames, subsampled=True)[0]
    gate = rows > 0 and k < num_stages - 1
    return dict(run=rows > 0, rows=rows, nh=nh, frames=int(used[act].sum()), gate=gate,
                threshold=float("inf") if threshold is None else float(threshold), max_rows=stage_quota(rows, fraction, b))


def format_stage_lines(video_ids, stage_of, confidence):
    """The lines of --cascade_stage_file: ``VideoId,Stage,Confidence`` with "%f" as the prediction file prints its confidences."""
    for vid, s, c in zip(video_ids, np.asarray(stage_of).tolist(), np.asarray(confidence).tolist()):
        if isinstance(vid, bytes):
            vid = vid.decode("utf-8")
        yield "%s,%d,%f\n" % (vid, s, c)


STAGE_FILE_HEADER = "VideoId,Stage,Confidence\n"


class CascadeGraph:
    """K forward-only stages for one input, cheapest first: each a ``teacher_only`` or ``student_only`` EvalGraph at its own every_n
    (``stages``: list of (tower, every_n[, student_sampling]) as EnsembleGraph's members), one device, one --precision, one set of model
    sizes (the other keyword arguments are EvalGraph's).  confidence: "top1" | "margin"; thresholds / fractions: None or K - 1 values, at
    least one of the two - a row whose confidence is >= thresholds[k] is settled at stage k, at most ceil(fractions[k] * batch rows) rows
    leave stage k (the least confident first); with both the threshold names the candidates and the fraction caps them.

    Under precision "split" the row plans are off: the cascade is correct there but every stage computes every row."""

    def __init__(self, batch_size, stages, confidence="top1", thresholds=None, fractions=None, **kw):
        self.stages = [parse_stage(s) for s in stages]
        self.families = [stage_family(s) for s in stages]
        self.thresholds, self.fractions = check_gates(len(self.stages), confidence, thresholds, fractions)
        self.confidence = confidence
        if batch_size > ops.CASCADE_MAX_ROWS:
            raise ValueError("CascadeGraph: batch_size %d (at most %d rows per gate)" % (batch_size, ops.CASCADE_MAX_ROWS))
        self.graphs = []
        for stage in stages:
            self.graphs.append(member_graph(batch_size, stage, kw))
        g0 = self.graphs[0]
        self.device, self.max_frames = g0.device, g0.max_frames
        self.C1, self.C2 = kw.get("num_inputs_to_lstm", 20), kw.get("num_inputs_l1_student", 5)     # (EvalGraph's defaults)
        self.stage_steps = [0] * len(self.stages)                        # how often each stage's graph was stepped
        self._pin_active = torch.empty(batch_size, dtype=torch.uint8, pin_memory=True)
        self._pin_count = torch.empty(1, dtype=torch.int32, pin_memory=True)
        self._gate_done = torch.cuda.Event()
        self.marks = None              # set to a list: (name, timing event) around every stage and gate of a step (scripts/cascade_bench.py)

    def restore(self, state_dicts):
        """Each stage restores its own checkpoint (the 11 variables of its tower by name)."""
        if len(state_dicts) != len(self.graphs):
            raise ValueError("CascadeGraph.restore: %d state dicts for %d stages" % (len(state_dicts), len(self.graphs)))
        for g, sd in zip(self.graphs, state_dicts):
            g.restore(sd)

    def _mark(self, name):
        if self.marks is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.marks.append((name, ev))

    def step(self, x_raw, labels_u8, num_frames, num_frames_host=None):
        """One batch through the cascade.  Returns predictions [B, V] f32 (every row the bits of the last stage that ran it), stage_of [B]
        uint8, confidence [B] f32 (at the stage that decided the row), and the host numbers stage_rows / stage_frames [K] and gate_wait_s."""
        if num_frames_host is None:
            num_frames_host = num_frames.cpu()
        nh0 = np.asarray(num_frames_host, dtype=np.int64).reshape(-1)
        b, V, K = int(x_raw.shape[0]), int(labels_u8.shape[1]), len(self.graphs)
        merged = torch.empty((b, V), dtype=F32, device=self.device)
        conf = torch.empty(b, dtype=F32, device=self.device)
        stage_of = torch.empty(b, dtype=torch.uint8, device=self.device)
        out = dict(predictions=merged, stage_of=stage_of, confidence=conf, stage_rows=[0] * K, stage_frames=[0] * K, gate_wait_s=0.0)
        # the keys of the content-aware strategies depend on the batch alone: once, from the original counts, for every stage that ranks by them
        keys = ops.frame_change_keys(x_raw, num_frames) if any(scored_sampling(g.frames) for g in self.graphs) else None
        active_dev, active_host, nf_k = None, None, num_frames
        for k, (g, (tower, every_n, _)) in enumerate(zip(self.graphs, self.stages)):
            book = stage_bookkeeping(k, K, active_host, nh0, tower, every_n, self.thresholds[k] if k < K - 1 else None,
                                     self.fractions[k] if (self.fractions is not None and k < K - 1) else None, self.max_frames, self.C1,
                                     self.C2, family=self.families[k])
            if not book["run"]:
                break                                                  # no row is active: nor will one be at any later stage
            out["stage_rows"][k], out["stage_frames"][k] = book["rows"], book["frames"]
            self._mark("stage%d" % k)
            pred = g.step(x_raw, labels_u8, nf_k, num_frames_host=book["nh"], keys=keys if scored_sampling(g.frames) else None)["predictions"]
            self.stage_steps[k] += 1
            self._mark("gate%d" % k)
            ops.cascade_confidence_rows(pred, self.confidence, k, conf, merged, stage_of, active=active_dev)
            if not book["gate"]:
                self._mark("end")
                break
            active_dev, nf_k, count = ops.cascade_pick_rows(conf, num_frames, book["threshold"], book["max_rows"], active=active_dev)
            self._pin_active[:b].copy_(active_dev, non_blocking=True)
            self._pin_count.copy_(count, non_blocking=True)
            self._gate_done.record()
            self._mark("wait%d" % k)
            t0 = time.perf_counter()
            self._gate_done.synchronize()                              # the one host stall of the stage: the next launch geometry is host-side
            out["gate_wait_s"] += time.perf_counter() - t0
            active_host = self._pin_active[:b].numpy().astype(bool)
            assert int(self._pin_count[0]) == int(active_host.sum())
        return out
