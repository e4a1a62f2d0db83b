"""The training-iteration graph of the reference's train.py / train_finetune.py
as an explicit schedule over the HIP kernels.

Reference: ``build_graph`` cs/train.py:185-427 (teacher + student in one
``sess.run``, cs/train.py:516-517) and cs/train_finetune.py:185-331
(student only).  Quirks kept on purpose: L_REP counted
twice in the student objective (cs/train.py:406), global_step += 2 per
iteration (one increment per train op, :332,:416), per-tensor gradient
clipping, teacher tensors constant in the student loss, both updates computed
from the pre-update weights of the same step.

Serial distillation (new; the paper's Serial training, which the reference's train.py does not ship): mode "serial" trains
the student against a frozen, forward-only teacher - one train op, the loss section as one launch (ops.distill_losses).

Data parallel (new; the reference is single-device): one process per GPU,
replicated parameters, per-rank batch, gradients summed with RCCL all-reduce
(``torch.distributed`` backend "nccl") on the flat gradient buffer - the MoE
segment is reduced as soon as it is final so it overlaps the LSTM BPTT, the
teacher's reduce overlaps the student's forward/backward.  Batch-mean losses
(CE, L_REP) are scaled by 1/world so the summed gradient equals the
single-device gradient at the global batch; L_PRED is a batch *sum*
(cs/train.py:402) and is not scaled.
"""
from __future__ import annotations

import dataclasses
import math
import os

import numpy as np
import torch

from . import losses as losses_mod
from . import ops
from .streams import concurrent_streams
from .engine import HLstmTower, drain

F32 = torch.float32


def exponential_decay(lr0, global_step, batch_size, decay_examples, rate):
    """tf.train.exponential_decay(lr0, global_step*batch, decay_examples, rate,
    staircase=True) - cs/train.py:223-236."""
    return lr0 * rate ** math.floor(global_step * batch_size / decay_examples)


def every_n_indices(every_n, max_frames=300):
    """cs/train.py:265-269 (host-side restatement of the static index list)."""
    idx, k = [], 0
    while every_n * k <= max_frames - 1:
        idx.append(every_n * k)
        k += 1
    return idx


def validate_every_n(every_n, num_inputs_l1=5, max_frames=300):
    """The reference's graph only builds when len(index list) == int(300/every_n)
    and that count splits into 5 chunks (cs/train.py:262-272,
    cs/frame_level_models.py:286,307).  Same failure, as a ValueError."""
    if every_n <= 0:
        raise ValueError("every_n must be a positive integer")
    s = max_frames // every_n
    if len(every_n_indices(every_n, max_frames)) != s or s == 0 or s % num_inputs_l1 != 0:
        raise ValueError("every_n=%d: %d gathered frames cannot be split into %d equal chunks of the %d-frame "
                         "student input" % (every_n, len(every_n_indices(every_n, max_frames)), num_inputs_l1, s))


def dp_loss_scales(world):
    """Per-rank gradient scale factors such that an all-reduce SUM over `world`
    ranks (each holding B_local videos, losses normalised by B_local) equals the
    single-device gradient at the global batch: CE (cs/losses.py:97) and L_REP
    (cs/train.py:362) are batch means -> 1/world; L_PRED is a batch sum
    (cs/train.py:402) -> 1.  The l2 regulariser is added once, after the reduce."""
    return {"ce": 1.0 / world, "rep": 1.0 / world, "kl": 1.0}


class GradReducer:
    """Gradient all-reduce (SUM) on slices of a flat buffer and the collectives of the row-sharded MoE update.
    backend "nccl" (= RCCL over xGMI) on GPUs, "gloo" in the CPU tests.

    Two ways to place the collectives (both give the same numbers; chosen per process by EVC_DP_SERIAL_COMM):

    * default - every collective is a synchronous c10d op issued from inside the compute stream it belongs to, so the
      RCCL kernel sits in stream order between the kernels that produce and consume its data; the student tower uses a
      communicator of its own (DistillGraph), two communicators may be in flight on two streams at once.
    * EVC_DP_SERIAL_COMM=1 - the conservative form for a first run on real xGMI: ONE communicator for everything and ONE
      collective in flight at a time: every collective still runs on the stream it belongs to, but first waits for the end
      of the previous one (event chain in host issue order, identical on all ranks), and DistillGraph issues the two
      towers' backward phases in readiness order so that the chain follows the order in which the data becomes ready.
      RCCL kernels of this process then execute strictly one after the other; compute on the other streams overlaps them."""

    _last_ev = None                 # serial placement: the event behind the last collective this process issued (any stream)
    # Accounting for bench.py's N > 1 line (class-wide: every reducer of the process adds to it):
    #   stats[kind] = [collectives issued, payload bytes handed to them]     (always on: two integer adds per call)
    #   timing = None | list of (kind, bytes, start event, end event) recorded on the stream the collective runs on
    stats = {}
    timing = None

    @staticmethod
    def _sim():
        """EVC_DP_SIM=<busbw GB/s>:<blocks>:<LDS KB per block>[:<world>] -> (busbw, blocks, lds_kb, world) or None."""
        v = os.environ.get("EVC_DP_SIM")
        if not v:
            return None
        f = v.split(":")
        return float(f[0]), int(f[1]), int(f[2]), int(f[3]) if len(f) > 3 else 8

    @staticmethod
    def wire_bytes(kind, payload, world):
        """Bytes one rank sends (= receives) for a ring collective over `world` ranks: all-reduce 2 (w-1)/w of the payload,
        all-gather (w-1) times its own part (payload = the part this rank contributes)."""
        if world <= 1:
            return 0.0
        if kind.startswith("all_reduce"):
            return 2.0 * (world - 1) / world * payload
        if kind.startswith("reduce_scatter"):          # payload = the whole buffer every rank contributes (world slabs)
            return (world - 1.0) / world * payload
        return float(world - 1) * payload

    def __init__(self, process_group=None, grad_dtype=None):
        self.pg = process_group
        # gradient all-reduce payload type for the LSTM segments: "f32" (default) or "bf16" (EVC_DP_GRAD_DTYPE=bf16): half the
        # bytes on xGMI - for configurations whose step is shorter than their f32 all-reduce (cfg 5: 4.4 ms step, 187 MB per
        # tower) - at one bf16 rounding of each rank's gradient (2^-9 relative; the sum itself runs in RCCL's bf16 arithmetic)
        self.grad_dtype = grad_dtype or os.environ.get("EVC_DP_GRAD_DTYPE", "f32")
        if self.grad_dtype not in ("f32", "bf16"):
            raise ValueError("EVC_DP_GRAD_DTYPE / grad_dtype must be f32 or bf16, not %r" % self.grad_dtype)
        self._bf16_ws = None
        self.world = 1
        init = torch.distributed.is_available() and torch.distributed.is_initialized()
        self.rank = 0
        if init:
            self.world = torch.distributed.get_world_size(process_group)
            self.rank = torch.distributed.get_rank(process_group)
        # collectives are issued when there is more than one rank; EVC_DP_FORCE=1 (debug) also issues them on a
        # one-rank group, which runs the whole RCCL path of a step on a single-GPU box (scripts/rccl_one_rank.sh)
        self.active = self.world > 1 or (init and os.environ.get("EVC_DP_FORCE") == "1")
        # TIMING AID (scripts/dp_occupancy_sim.sh, round 6): EVC_DP_SIM_WORLD=W on a ONE-rank forced group - this process does the per-rank WORK
        # of rank 0 of W: MoE row slabs of 1/W of the rows (MoeHead.shard), factor all-gathers replicated to W x batch rows, slab gathers /
        # reduce-scatters on the own slab only.  The other W - 1 slabs are never updated: the step's numbers are meaningless, its kernel
        # times are those of one rank of a W-GPU node with zero time on the wire (EVC_DP_SIM adds the wire time).  Never set in a real run.
        self.shard_world = self.world
        if self.world == 1 and self.active and os.environ.get("EVC_DP_SIM_WORLD"):
            self.shard_world = max(1, int(os.environ["EVC_DP_SIM_WORLD"]))
        self.serial = self.active and serial_comm() and torch.cuda.is_available()
        self._pending = []

    def _run(self, fn, *tensors, kind="collective", nbytes=0):
        """Issue one collective: in stream order on the current stream, or through the process-wide serial stream."""
        st = GradReducer.stats.setdefault(kind, [0, 0])
        st[0] += 1
        st[1] += int(nbytes)
        sim = GradReducer._sim()
        if sim is not None and self.world == 1 and torch.cuda.is_available():
            # one-GPU stand-in for the fabric (EVC_DP_SIM, scripts/dp_occupancy_sim.sh): after the (empty) one-rank collective a kernel
            # with an RCCL-like footprint holds `blocks` CUs for the time the bytes would spend on the wire at `busbw`
            busbw, blocks, lds_kb, w = sim
            if kind == "all_gather_slabs" and self.shard_world == 1:
                wire = (w - 1.0) / w * nbytes          # (at one rank the "slab" is the whole matrix)
            else:
                wire = GradReducer.wire_bytes(kind, nbytes, w)
            us = wire / (busbw * 1e9) * 1e6 + 20.0       # + a launch / rendezvous latency
            real = fn

            def fn():
                out = real()
                from . import _lib
                _lib.call("evc_debug_occupy", blocks, 256, lds_kb * 1024, us, torch.cuda.current_stream().cuda_stream)
                return out
        if GradReducer.timing is not None and torch.cuda.is_available():
            inner = fn

            def fn():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = inner()
                e1.record()
                GradReducer.timing.append((kind, int(nbytes), e0, e1))
                return out
        if not self.serial:
            return fn()
        # ONE collective of this process at a time, in host issue order, each on the stream it belongs to: the collective waits for
        # the end of the previous one (an event recorded behind it on ITS stream) and leaves an event for the next.  (Round 3
        # funnelled them through a fifth stream instead - which shares one of the four hardware queues with a compute stream
        # (streams.py) and serialised with that stream's kernels: 16.5 ms per step in the stand-in runs of DESIGN.md 6.1.)
        cur = torch.cuda.current_stream()
        if GradReducer._last_ev is not None:
            cur.wait_event(GradReducer._last_ev)
        out = fn()
        ev = torch.cuda.Event()
        ev.record(cur)
        GradReducer._last_ev = ev
        return out

    def reduce(self, flat, lo, hi, f32=True):
        """All-reduce of flat[lo:hi] as an async c10d op, joined by wait() (the schedule without early apply).  The payload type
        follows grad_dtype only where the caller allows it (f32=False: LSTM segments); with a bf16 payload, and under the serial
        placement, the call goes through reduce_async (stream order) - one implementation of the dtype switch."""
        if not self.active or hi <= lo:
            return
        if self.serial or (self.grad_dtype == "bf16" and not f32):
            self.reduce_async(flat, lo, hi, f32=f32)
            return
        self._pending.append(torch.distributed.all_reduce(flat[lo:hi], op=torch.distributed.ReduceOp.SUM,
                                                          group=self.pg, async_op=True))

    def reduce_async(self, flat, lo, hi, f32=False):
        """f32=True: this segment crosses the fabric as f32 whatever grad_dtype says (the MoE segment when its update is not the
        fused one: EVC_DP_GRAD_DTYPE=bf16 is an option for the LSTM segments only).
        All-reduce of flat[lo:hi] in stream order: issued as a *synchronous* c10d op, which ProcessGroupNCCL
        enqueues on the CURRENT stream (the RCCL kernel sits between the kernels that produce the gradients and the
        ones that consume them; the host does not wait).  An async_op=True collective runs on the process group's
        own stream instead, which shares one of the 4 hardware queues with a compute stream: its event then waits
        for every packet already queued there - measured on a one-rank communicator, where no byte moves: 14.4
        instead of 13.5 ms per step (scripts/dp_host_probe.py).  Returns None (nothing left to wait for)."""
        if not self.active or hi <= lo:
            return None
        seg = flat[lo:hi]
        if self.grad_dtype == "bf16" and not f32:
            return self._reduce_bf16(seg)
        self._run(lambda: torch.distributed.all_reduce(seg, op=torch.distributed.ReduceOp.SUM, group=self.pg, async_op=False), seg,
                  kind="all_reduce_grad_f32", nbytes=seg.numel() * 4)
        return None

    def _reduce_bf16(self, seg):
        """seg (f32) <- SUM over the ranks of bf16(seg): the payload crosses the fabric as bf16.  (gloo has no bfloat16: the CPU
        tests reduce the bf16-rounded values in f32 - the same per-rank rounding, an exact sum.)"""
        n = seg.numel()
        if self._bf16_ws is None or self._bf16_ws.numel() < n or self._bf16_ws.device != seg.device:
            self._bf16_ws = torch.empty(n, dtype=torch.bfloat16, device=seg.device)
        ws = self._bf16_ws[:n]
        ws.copy_(seg)
        if torch.distributed.get_backend(self.pg) == "gloo":
            seg.copy_(ws)
            self._run(lambda: torch.distributed.all_reduce(seg, op=torch.distributed.ReduceOp.SUM, group=self.pg, async_op=False), seg,
                      kind="all_reduce_grad_bf16", nbytes=n * 2)
            return None
        self._run(lambda: torch.distributed.all_reduce(ws, op=torch.distributed.ReduceOp.SUM, group=self.pg, async_op=False), ws,
                  kind="all_reduce_grad_bf16", nbytes=n * 2)
        seg.copy_(ws)
        return None

    def all_gather_rows(self, t):
        """[rows, cols] bf16 (contiguous) of every rank stacked along the rows, in rank order (the collective
        moves raw bytes: gloo has neither bfloat16 nor int16).  Stream-ordered like reduce_async."""
        if not self.active:
            return t
        t = t.contiguous()

        def go():
            out = torch.empty((self.world * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
            torch.distributed.all_gather_into_tensor(out.view(torch.uint8), t.view(torch.uint8), group=self.pg)
            if self.shard_world != self.world:           # EVC_DP_SIM_WORLD: the contraction length of a W-rank gather
                out = out.repeat(self.shard_world, *([1] * (out.dim() - 1)))
            return out
        return self._run(go, t, kind="all_gather_factors", nbytes=t.numel() * t.element_size())

    def all_reduce_small(self, t):
        """In-place SUM of a few floats (the partial norm sums of a sharded tensor), stream-ordered."""
        if self.active:
            self._run(lambda: torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.SUM, group=self.pg, async_op=False), t,
                      kind="all_reduce_small", nbytes=t.numel() * t.element_size())

    def all_gather_slabs(self, full, slab_rows):
        """full [world * slab_rows, cols] (contiguous): rank r owns rows [r*slab_rows, (r+1)*slab_rows); every
        rank's slab is written into every rank's `full`, stream-ordered."""
        if not self.active:
            return
        assert full.is_contiguous() and full.shape[0] == self.shard_world * slab_rows

        def go():
            own = full[self.rank * slab_rows:(self.rank + 1) * slab_rows].clone()     # (24 MB at world 8: no aliasing of in / out)
            dst = full if self.shard_world == self.world else full[:self.world * slab_rows]      # (EVC_DP_SIM_WORLD: the own slab only)
            torch.distributed.all_gather_into_tensor(dst.view(torch.uint8), own.view(torch.uint8), group=self.pg)
            return own
        self._run(go, full, kind="all_gather_slabs", nbytes=slab_rows * full.shape[1] * full.element_size())

    def reduce_scatter_rows(self, full, slab_rows):
        """full [world * slab_rows, cols] bf16 (contiguous): this rank's contribution to every rank's slab.  Returns [slab_rows, cols] bf16 = the
        SUM over the ranks of slab `rank` (stream-ordered).  RCCL sums in bf16 along the ring; gloo has neither bfloat16 nor reduce_scatter:
        the CPU / shared-GPU tests all-reduce the bf16-rounded values in f32 (the same per-rank rounding, an exact sum) and round the own slab once."""
        assert full.is_contiguous() and full.dtype == torch.bfloat16 and full.shape[0] == self.shard_world * slab_rows
        if not self.active:
            return full[:slab_rows]

        def go():
            if torch.distributed.get_backend(self.pg) == "gloo":
                f = full.float()
                torch.distributed.all_reduce(f, op=torch.distributed.ReduceOp.SUM, group=self.pg)
                return f[self.rank * slab_rows:(self.rank + 1) * slab_rows].to(torch.bfloat16)
            own = torch.empty((slab_rows, full.shape[1]), dtype=full.dtype, device=full.device)
            src = full if self.shard_world == self.world else full[:self.world * slab_rows]      # (EVC_DP_SIM_WORLD: the own slab only)
            torch.distributed.reduce_scatter_tensor(own, src, op=torch.distributed.ReduceOp.SUM, group=self.pg)
            return own
        return self._run(go, full, kind="reduce_scatter_grad_bf16", nbytes=full.numel() * 2)

    def wait(self):
        for w in self._pending:
            w.wait()
        self._pending = []


def _resolve_label_loss(label_loss, vocab_size):
    """label_loss of a graph (None | class name | losses.BaseLoss) -> the instance, after its host-side refusals for vocab_size classes."""
    fn = losses_mod.resolve(label_loss)
    if vocab_size is not None:
        fn.check(vocab_size)
    return fn


def check_distill_losses(words):
    """--distill_losses / DistillGraph(distill_losses=...): a non-empty subset of ("rep", "pred", "ce"), as a comma list or a
    sequence; returned as a tuple in that canonical order.  Unknown, empty and repeated words are refused."""
    if isinstance(words, str):
        words = [w.strip() for w in words.split(",")]
    words = list(words)
    known = ("rep", "pred", "ce")
    bad = [w for w in words if w not in known]
    if bad or not words or len(set(words)) != len(words):
        raise ValueError("distill_losses %r: a comma list of distinct words out of rep, pred, ce (at least one)" % (",".join(map(str, words)),))
    return tuple(w for w in known if w in words)


def serial_comm():
    """EVC_DP_SERIAL_COMM=1: one communicator, one collective at a time (see GradReducer)."""
    return os.environ.get("EVC_DP_SERIAL_COMM") == "1"


def dp_timeout():
    """Process-group timeout for init_process_group (bench.py, train.py): a collective that has not completed after this long
    makes the watchdog abort the process - a wedged first contact with the fabric ends non-zero in minutes instead of sitting in
    the launcher's window (c10d's default is 10 minutes).  EVC_DP_TIMEOUT_S, default 120 s; the longest legitimate wait is a
    peer's checkpoint write or its first-step allocations."""
    import datetime
    return datetime.timedelta(seconds=float(os.environ.get("EVC_DP_TIMEOUT_S", "120")))


def student_light(student, precision):
    """The "high" precision layout of the STUDENT tower: plain f16 on its L1 level (no K-extensions).  It runs 6 steps per chunk
    over 5 chunks where the teacher runs 15 over 20, so the rounding terms the teacher's layout extends have no time
    to build up: all-f16 leaves 1e-4 on its logits (the teacher: up to 1e-3) - and the extensions would cost its six L1 layer-0
    launches 2.5x their depth.  Only for students of at most 30 frames (every_n >= 10).  It reads the first segment of the shared K-extended input image.
    OFF BY DEFAULT since round 6 (EVC_HIGH_STUDENT_LIGHT=1 switches it on): true 16 steps from initialisation (9e-5 on the student's logits), not on
    towers trained for 512 steps - 7.8e-4 .. 1.64e-3 over 12 weight draws against 3.7 .. 9.1e-4 with the teacher's layout
    (profiles/r06_precision_robustness_long.txt), for 0.14 ms of the 11.7 ms "high" step."""
    if (student is not None and precision == "high" and student.T <= 30       # (every_n >= 10; a longer student takes the teacher's layout)
            and os.environ.get("EVC_HIGH_STUDENT_LIGHT", "0") == "1"):
        student.f16_x_segments = 1
        student.f16_wh_ext_layers = ()
        student.f16_wx_ext_layers = ()
        student.f16_fp8_lo = False


def input_image_args(*towers):
    """f16_segments / fp8_tail of ops.l2norm_chunk for the towers that share one input image: the widest K-extension any of them
    contracts (a tower may read fewer segments than the rows hold); with a tower on the fp8 L1 level the rows are its 5F-byte ones."""
    tw = [t for t in towers if t is not None]
    fp8 = any(t.fp8_lo() for t in tw)
    if fp8:
        assert all(t.fp8_lo() or t.f16_x_segments == 1 for t in tw), "towers sharing an fp8 input image read its plain f16 part"
        return dict(f16_segments=1, fp8_tail=True)
    return dict(f16_segments=max(t.f16_x_segments for t in tw))


@dataclasses.dataclass(slots=True)
class FramePlan:
    """What frame_counts_and_plans / input_views / scored_sampling read, for the tower or towers that take their input in one pass: every field
    is declared here with its default, and a misspelt one raises (slots).  `sampling_draw` / `sampling_row0` are set per step by the owner."""
    teacher: object = None
    student: object = None
    every_n: int = 1
    C1: int = 20
    C2: int = 5
    max_frames: int = 300
    row_plans: bool = True
    student_sampling: str = "uniform"          # ops.STUDENT_SAMPLING
    sampling_seed: int = 0
    sampling_draw: int = 0
    sampling_row0: int = 0
    last_frame_table: object = None            # the source-frame table of the last batch (a student off the uniform grid), for tests and diagnostics

    @property
    def S(self):
        return self.max_frames // self.every_n


def scored_sampling(p):
    """Whether the student of FramePlan ``p`` takes its frames by their content (ops.STUDENT_SAMPLING_SCORED): its table needs ops.frame_change_keys."""
    return p.student is not None and p.student_sampling in ops.STUDENT_SAMPLING_SCORED


def input_views(p, x_raw, num_frames, tp, sp, need_student, keys=None):
    """The L1 input images of FramePlan ``p``'s towers for one batch (ops.l2norm_chunk): (teacher view, student view), each the plain bf16 image or - in
    the non-bf16 modes - a tuple (bf16 image, second image[, row scales]).  uint8 frames into "high" towers whose layer 0 is on the f16 + e4m3 form
    take the INTEGER-frame images (ops.l2norm_chunk_int, HLstmTower.x_int: the input exact, round 6).  ``keys``: the batch's
    ops.frame_change_keys where the owner of several graphs on one batch has computed them already (only read under a scored word)."""
    towers = [t for t in (p.teacher, p.student if need_student else None) if t is not None]
    p1, p2 = (tp[2] if tp else None), (sp[3] if sp else None)
    as_int = x_raw.dtype == torch.uint8 and towers and all(t.precision == "high" and t.x_int() for t in towers)
    nf = num_frames if x_raw.dtype == torch.uint8 else None
    if need_student and p.student_sampling != "uniform":
        # A student on other frames than the grid s * every_n (--student_sampling): the teacher view as ever, without a student view, then the
        # student view from the table of its source frames + the gathering pass, on the same stream.  The image forms are the ones the shared
        # call would have produced (decided over both towers), the frame counts and row plans do not depend on which frames are taken.
        img = input_image_args(p.teacher, p.student)
        xt = None
        if p.teacher is not None:
            if as_int:
                xt = ops.l2norm_chunk_int(x_raw, num_frames, p.C1, None, p.C2, plan1=p1)[0]
            else:
                xt = ops.l2norm_chunk(x_raw, p.C1, None, p.C2, num_frames=nf, split=towers[0].input_split(), plan1=p1, **img)[0]
        if p.student_sampling in ops.STUDENT_SAMPLING_SCORED:      # by content: one key per raw frame on this stream, then the ranking table
            if keys is None:
                keys = ops.frame_change_keys(x_raw, num_frames)
            src = ops.student_frame_select_scored(num_frames, keys, p.max_frames, p.every_n, p.student_sampling)
        else:
            src = ops.student_frame_select(num_frames, p.max_frames, p.every_n, p.student_sampling, seed=p.sampling_seed,
                                           draw=p.sampling_draw, row0=p.sampling_row0)
        p.last_frame_table = src
        if as_int:
            return xt, ops.l2norm_chunk_int_sel(x_raw, num_frames, src, p.every_n, p.C2, plan2=p2)
        return xt, ops.l2norm_chunk_sel(x_raw, src, p.every_n, p.C2, num_frames=nf, split=towers[0].input_split(), plan2=p2, **img)
    if as_int:
        return ops.l2norm_chunk_int(x_raw, num_frames, p.C1, p.every_n if need_student else None, p.C2, plan1=p1, plan2=p2, teacher_view=p.teacher is not None)
    return ops.l2norm_chunk(x_raw, p.C1, p.every_n if need_student else None, p.C2, num_frames=nf,
                            split=towers[0].input_split(), plan1=p1, plan2=p2, teacher_view=p.teacher is not None,
                            **input_image_args(p.teacher, p.student if need_student else None))


def frame_counts_and_plans(p, num_frames, nh, need_teacher, need_student):
    """Frame counts (device) and the L1 row plans of FramePlan ``p``'s towers: rows
    sorted by length so the padding rows drop out of every L1 kernel (ops.RowPlan).  Host twins of the counts
    give the launch geometry.  Returns ((len_l1, len_l2, plan) | None, (n_student, len_l1, len_l2, plan) | None)."""
    t = s = None
    if need_teacher:
        _, l1, l2 = ops.frame_counts(num_frames, 1, p.C1, p.max_frames // p.C1, p.max_frames)
        plan = None
        if p.row_plans:
            _, l1h, _ = ops.host_frame_counts(nh, 1, p.C1, p.max_frames // p.C1, p.max_frames)
            plan = ops.RowPlan(l1, l1h, p.max_frames // p.C1)
        t = (l1, l2, plan)
    if need_student:
        n_s, l1s, l2s = ops.frame_counts(num_frames, p.every_n, p.C2, p.S // p.C2, p.max_frames, subsampled=True)
        plan = None
        if p.row_plans:
            _, l1h, _ = ops.host_frame_counts(nh, p.every_n, p.C2, p.S // p.C2, p.max_frames, subsampled=True)
            plan = ops.RowPlan(l1s, l1h, p.S // p.C2)
        s = (n_s, l1s, l2s, plan)
    return t, s


class _StepGraph:
    """What every graph's step is built from: the learning rate, the entry onto the graph's own main stream, the keep-alive of tensors
    that cross streams (SingleTowerGraph takes the learning rate alone)."""

    world = 1
    debug_marks = None      # set to a list to collect (name, timing event) pairs of one step (scripts/step_marks.py)

    def _mark(self, name, stream):
        if self.debug_marks is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(stream)
            self.debug_marks.append((name, ev))

    def _lr_l2c(self, batch_size):
        """(learning rate of this iteration - every train op of it reads the same global_step, cs/train.py:223-236 -, weight of the l2 term)."""
        return (exponential_decay(self.lr0, self.global_step, batch_size * self.world, self.lr_decay_examples, self.lr_decay),
                self.reg_pen * 1e-8)

    def _fuse_moe_update(self, apply, moe, precision, dp=False):
        """(fuse, fused_names) of a single-tower step (SingleTowerGraph, vlad_graphs.GridDistillGraph): whether its update takes the MoE
        head's two matrices through MoeHead's fused clip + Adam pass (their gradient recomputed from its rank-B factors) - whenever the step
        also applies -, and the variables that pass updates (the bias gradient comes from the same factors).  dp: data parallel."""
        fuse = bool(apply and self.fused_moe_update and moe is not None and moe.can_fuse_update() and moe.prefer_fused_update(dp)
                    and precision == "bf16")
        return fuse, ((moe.GATES, moe.EXPERTS, moe.EBIAS) if fuse else ())

    def _update_tower(self, tw, moe, B, fuse, fused_names, route_rs=False, dp=None):
        """The train op of a single-tower step behind tw.backward: the fused MoE update (route_rs: on the owners' slabs of a bf16
        reduce-scatter) and clip_by_norm + TF-Adam on the tower's other variables, or the latter on all of them; global_step += 1.
        dp: the GradReducer of a data-parallel step, None on one rank."""
        lr, l2c = self._lr_l2c(B)
        if fuse:
            tw.begin_update()
            if route_rs:
                moe.sharded_update(tw.adam_lr_t(lr), self.clip, l2c, dp)
            else:
                moe.fused_update(tw.adam_lr_t(lr), self.clip, l2c, dp=dp)
            tw.apply_group([k for k in tw.names if k not in fused_names], lr, self.clip, l2c)
        else:
            tw.apply_gradients(lr, self.clip, l2c)
        self.global_step += 1

    def _on_main(self, inputs, num_frames_host, body):
        """Runs ``body(host frame counts)`` on the graph's own main stream, ordered after the caller's current stream on entry
        and before it on exit (so callers see ordinary single-stream semantics).  ``inputs``: the caller's tensors the step reads
        (the first three are x_raw, labels_u8, num_frames; None entries are skipped).

        num_frames_host: the same frame counts on the host (numpy / CPU tensor / list), as the input pipeline
        has them before the H2D copy.  The launch geometry of the row-planned L1 stacks depends on them; without
        it they are read back from the device, which stalls the host on everything queued before."""
        if num_frames_host is None:
            num_frames_host = inputs[2].cpu()
        nh = np.asarray(num_frames_host, dtype=np.int64).reshape(-1)
        caller = torch.cuda.current_stream(self.device)
        if caller == self._main:
            return body(nh)
        self._main.wait_stream(caller)
        with torch.cuda.stream(self._main):
            out = body(nh)
        for t in inputs:
            if t is not None:
                t.record_stream(self._main)
        caller.wait_stream(self._main)
        return out

    @staticmethod
    def _keep_alive(stream, views, plans):
        """The students' input views and plan tuples (n, len_l1, len_l2, row plan): allocated on `main`, consumed on ``stream``."""
        for xs, sp in zip(views, plans):
            used = (xs if isinstance(xs, tuple) else (xs,)) + sp[:3]
            if sp[3] is not None:
                used += (sp[3].pos, sp[3].inv, sp[3].lens)
            for t in used:
                if t is not None:
                    t.record_stream(stream)


class _TrainGraph(_StepGraph):
    """The training graphs over H-LSTM towers (DistillGraph, SerialStudentsGraph): their streams, the deferred updates, and the step
    against a frozen teacher.  A subclass names its towers (_towers) and counts its train ops (_apply_gradients)."""

    def _make_streams(self):
        """Four streams that measurably overlap (streams.py) - the step never runs on the default stream - and the step's events."""
        self._opt_t = self._opt_s = None
        if self.device.type != "cuda":
            return
        self._main, self._side, self._aux_t, self._aux_s = concurrent_streams(self.device, 4)
        if os.environ.get("EVC_SINGLE_STREAM") == "1":     # profiling aid: the same launches, all on ONE stream (solo kernel times)
            self._side = self._aux_t = self._aux_s = self._main
        # experiment: the optimizer launches on a CU-masked stream of their own - EVC_OPT_CU_MASK=<CUs per XCD>[:<first>]
        m = os.environ.get("EVC_OPT_CU_MASK")
        if m:
            from .streams import cu_masked_stream
            f = [int(v) for v in m.split(":")]
            self._opt_t = self._opt_s = cu_masked_stream(self.device, f[0], f[1] if len(f) > 1 else 0)      # (shared by both towers)
        self._ev_fwd, self._ev_student, self._ev_in = torch.cuda.Event(), torch.cuda.Event(), torch.cuda.Event()

    def flush(self):
        """Enqueue and join the deferred updates of the last step (defer_updates): afterwards every weight, moment and operand
        shadow of every tower is current in the order of the caller's stream.  Cheap no-op when nothing is pending."""
        if self.device.type != "cuda":
            return
        cur = torch.cuda.current_stream(self.device)
        for tw in self._towers():
            tw.wait_deferred(cur)

    def apply_gradients(self, batch_size, lr=None):
        """Runs whichever train op has not been applied inside step() and counts global_step on (_apply_gradients)."""
        self.flush()
        self._apply_gradients(batch_size, lr)

    def _serial_step(self, students, xt, tp, xss, sps, labels_u8, dps, apply, loss_section, teacher_forwards=None):
        """One iteration of ``students`` against the frozen teacher, after the input stage (teacher view ``xt`` and plan ``tp``, per
        student a view, a plan tuple and a dL/dpred buffer).  Returns `out`, the students' dicts as the list out["students"].
        ``teacher_forwards`` (EnsembleDistillGraph): a callable that runs the forwards of SEVERAL frozen teachers one after another on
        `main` in place of the one teacher's, and returns (list of states, list of predictions), which ``loss_section`` and `out` then
        receive as they are; None: the launches of the one-teacher step, unchanged.

        Schedule: the teacher's forward (tape-free, the step's longest chain) ONCE on `main`, the students' forwards next to it on
        `side` from the start of the step, one after the other - neither reads the other -; ``loss_section(t_state, t_pred, fwd, ds)``
        on `side` once all forwards are done (one launch + its finish, every dpred / dstate written once); then each student's backward
        and update exactly as in mode "student" (aux stream, early apply, defer_updates), student after student; `main` joins at the
        end.  The teacher's backward, weight gradients, update and tape of the parallel step do not exist here."""
        B = labels_u8.shape[0]
        main = torch.cuda.current_stream(self.device)
        for s in students:
            s.run_deferred()
        self.losses.zero_()
        mark = self._mark
        mark("start", main)
        lr, l2c = self._lr_l2c(B)
        two_streams = self.overlap_towers
        side = self._side if two_streams else main
        l1, l2, plan_t = tp
        if two_streams:
            self._ev_in.record(main)
            side.wait_event(self._ev_in)
        t_state, t_pred = self.teacher.forward(xt, l1, l2, plan_t) if teacher_forwards is None else teacher_forwards()
        mark("teacher_fwd_done", main)
        if two_streams:
            self._ev_fwd.record(main)
        with torch.cuda.stream(side):
            mark("student_start", side)
            fwd = [s.forward(xs, l1s, l2s, plan_s) for s, xs, (_, l1s, l2s, plan_s) in zip(students, xss, sps)]
            mark("student_fwd_done", side)
            if two_streams:
                side.wait_event(self._ev_fwd)
            if self._ds_serial is None or self._ds_serial[0].shape != fwd[0][0].shape:
                self._ds_serial = [torch.empty_like(f[0]) for f in fwd]
            loss_section(t_state, t_pred, fwd, self._ds_serial)
            mark("losses_done", side)
            early_s = (lr, self.clip, l2c) if (apply and self.overlap_towers and self._aux_s is not None) else None
            for s, ds, dp in zip(students, self._ds_serial, dps):
                drain(s.backward_phases(ds, dp, aux=self._aux_s if self.overlap_towers else None, early_apply=early_s,
                                        defer=self.defer_updates, opt=self._opt_s))      # every phase to its end
            mark("student_done", side)
            if two_streams:
                self._ev_student.record(side)
                self._keep_alive(side, xss, sps)
        if two_streams:
            main.wait_event(self._ev_student)
        rows = self.losses.view(-1, 4)
        outs = [dict(student_predictions=f[1], student_state=f[0], num_frames_student=sp[0], student_loss_state=rows[k, 1],
                     pred_loss=rows[k, 2], student_label_loss=rows[k, 3]) for k, (f, sp) in enumerate(zip(fwd, sps))]
        out = dict(predictions=t_pred, teacher_state=t_state, loss=rows[0, 0], students=outs)
        self._student_applied = early_s is not None
        if apply:
            self._apply_gradients(B, lr)
        out["global_step"] = self.global_step
        return out


class DistillGraph(_TrainGraph):
    """mode: 'teacher_student' (train.py), 'teacher' (teacher only, BASELINE cfg 2),
    'student' (train_finetune.py), 'serial' (the paper's Serial training: the student against a FROZEN teacher -
    forward-only 'model' tower, no tape / gradient / Adam state, never written; one train op)."""

    LOSS_SLOTS = ("label_loss", "student_loss_state", "pred_loss", "student_label_loss")
    # host issue orders of the two towers' backward phases (HLstmTower.backward_phases: MoE head, L2 layer 1, L2 layer 0, L1 layer 1,
    # L1 layer 0 each): letters name the tower whose next phase is issued; whatever is left afterwards is drained student first
    ISSUE_ORDERS = {"sequential": "sssss", "interleaved": "tsstsstst"}
    MODES = ("teacher_student", "teacher", "student", "serial")
    DISTILL_LOSSES = ("rep", "pred", "ce")      # the student's loss terms in mode "serial" (the paper's ablation); all three = cs/train.py:406

    def __init__(self, batch_size, every_n=10, mode="teacher_student", feature_size=1152, vocab_size=4716,
                 max_frames=300, num_inputs_to_lstm=20, num_inputs_l1_student=5, lstm_cells=1024, lstm_layers=2,
                 num_mixtures=2, base_learning_rate=0.001, learning_rate_decay=1.0,
                 learning_rate_decay_examples=4000000, regularization_penalty=2.0, clip_gradient_norm=1.0,
                 count_rep_twice=True, device="cuda:0", seed=7, process_group=None, overlap_towers=True,
                 precision="bf16", student_sampling="uniform", sampling_seed=0, distill_losses=DISTILL_LOSSES, label_loss=None):
        assert mode in self.MODES
        # the label loss L_CE of both towers (losses.BaseLoss instance, class name, None = CrossEntropyLoss: --label_loss)
        self.label_loss = _resolve_label_loss(label_loss, vocab_size)
        if mode == "serial" and not losses_mod.is_default(self.label_loss):
            raise ValueError("DistillGraph(mode='serial') has CrossEntropyLoss built into its loss section (evc_distill_losses), not %s"
                             % type(self.label_loss).__name__)
        self.distill_losses = check_distill_losses(distill_losses)
        if self.distill_losses != self.DISTILL_LOSSES and mode != "serial":
            raise ValueError("distill_losses selects the student's loss terms of mode 'serial' only (mode %r trains on all of its losses)" % mode)
        self.mode, self.B, self.every_n = mode, batch_size, every_n
        # which frames the student sees (ops.STUDENT_SAMPLING; input_views): "uniform" is the grid s * every_n of the reference
        self.student_sampling, self.sampling_seed = ops.check_student_sampling(student_sampling), int(sampling_seed)
        self.max_frames, self.C1, self.C2 = max_frames, num_inputs_to_lstm, num_inputs_l1_student
        self.lr0, self.lr_decay, self.lr_decay_examples = base_learning_rate, learning_rate_decay, learning_rate_decay_examples
        self.reg_pen, self.clip = regularization_penalty, clip_gradient_norm
        self.rep_w = 2.0 if count_rep_twice else 1.0
        self.device = torch.device(device)
        self.pg = process_group
        self.reducer = GradReducer(process_group)
        self.world, self.dp = self.reducer.world, self.reducer.active
        if mode == "serial" and (self.world > 1 or self.dp):
            raise ValueError("DistillGraph(mode='serial') is not data parallel yet (process group of %d ranks): train the student "
                             "against the frozen teacher on one device" % self.world)
        # The student's collectives get a communicator of their own: one process group executes its collectives in
        # issue order, so on a shared group the teacher's early factor all-gather (host-issued after the student's
        # backward) would queue behind the student's last gradient all-reduce and hold the teacher's whole update
        # chain back.  (new_group is collective: every rank constructs the graph.)
        self.reducer_s = self.reducer
        if self.dp and mode == "teacher_student" and not serial_comm():
            ranks = list(range(torch.distributed.get_world_size(process_group))) if process_group is None else None
            self.reducer_s = GradReducer(torch.distributed.new_group(ranks) if ranks is not None else process_group)
        self.global_step = 0
        self.teacher = self.student = None
        self.train_teacher = mode in ("teacher_student", "teacher")       # "serial": the teacher is a constant of the step
        if mode != "student":
            self.teacher = HLstmTower(batch_size, max_frames, num_inputs_to_lstm, feature_size, vocab_size, lstm_cells,
                                      lstm_layers, num_mixtures, device, self.train_teacher, "model", seed)
            if not self.train_teacher:
                self.teacher.store.drop_training_state()
        if mode != "teacher":
            validate_every_n(every_n, num_inputs_l1_student, max_frames)
            self.student = HLstmTower(batch_size, max_frames // every_n, num_inputs_l1_student, feature_size, vocab_size, lstm_cells,
                                      lstm_layers, num_mixtures, device, True, "model_student", seed + 1)
        if self.dp:                      # row-shard the MoE optimizer state now, while nothing is in flight on any stream
            for tw, red in ((self.teacher, self.reducer), (self.student, self.reducer_s)):
                if tw is not None:
                    tw.moe.shard(red.shard_world, red.rank)
        self.precision = precision       # engine.TowerBase.precision: "bf16" | "high" (1e-3 at trained magnitudes) | "split" (uniform)
        student_light(self.student, precision)
        if precision != "bf16":
            for tw in self._towers():
                tw.set_precision(precision)
        # both towers take their input in one pass; row_plans: sort the L1 chunk rows by length and skip the padding rows (ops.RowPlan)
        # (the uniform split-bf16 layers run on every row)
        self.frames = FramePlan(self.teacher, self.student, every_n, self.C1, self.C2, max_frames, precision != "split",
                                self.student_sampling, self.sampling_seed)
        self.losses = torch.zeros(8, dtype=F32, device=self.device)
        self._losses_reduced = torch.zeros(8, dtype=F32, device=self.device)   # data parallel: SUM over the ranks, per step
        self._dp_t = self._dp_s = self._ds_s = self._ds_serial = None
        self._teacher_applied = self._student_applied = False
        self.overlap_towers = overlap_towers
        # True: the student's forward starts next to the teacher's forward instead of after it.  Measured 0.1 ms/step
        # faster, but the teacher's fused forward steps then share the chip (67 -> 84 us per launch): off by default so
        # that the step's dominant kernel runs - and is measured - alone.
        self.student_forward_early = False
        # True: the student's forward starts when the teacher's L1 level has been enqueued, next to the teacher's L2 chain /
        # MoE head (latency-bound launches).  Measured 13.01 -> 12.88 ms/step with the teacher's L1 steps unaffected.
        self.student_forward_after_l1 = True
        # Cross-step deferral (one process): the MoE-head and L2-level updates of step k are enqueued at the start of step k+1,
        # under its L1 forward, instead of under step k's BPTT chain (HLstmTower.backward(defer=True)).  Whoever reads the
        # weights between two steps calls flush() first (state_dict() / consolidate() / apply_gradients() do).
        self.defer_updates = os.environ.get("EVC_DEFER_UPDATES", "0") == "1"
        # one communicator for both towers (EVC_DP_SERIAL_COMM=1): issue the backward phases in readiness order, so that collectives
        # funnelled through one stream do not wait behind the other tower's later ones; EVC_ISSUE_ORDER overrides (A/B runs)
        self.issue_order = os.environ.get("EVC_ISSUE_ORDER", "interleaved" if (self.dp and serial_comm()) else "sequential")
        if self.issue_order not in self.ISSUE_ORDERS:
            raise ValueError("EVC_ISSUE_ORDER must be one of %s" % sorted(self.ISSUE_ORDERS))
        self._make_streams()
        # Single-tower graphs (cfg 2 teacher only, cfg 5 student only) use two of the four streams: the tower's collectives + optimizer launches
        # take a THIRD one (the other tower's idle aux stream) instead of queueing on the aux stream between the weight-gradient products - under
        # data parallelism that stream is the step's critical path and every byte on the wire was exposed (cfg 5 as rank 0 of 8 with stand-in
        # collectives at 300 GB/s: 5.67 ms; profiles/r06_dp_sim_world.txt).  Under data parallelism only.
        if self.device.type == "cuda" and self.dp and os.environ.get("EVC_SINGLE_STREAM") != "1" and self._opt_t is None:
            if mode == "student":
                self._opt_s = self._aux_t
            elif mode == "teacher":
                self._opt_t = self._aux_s

    S = property(lambda self: self.frames.S)
    last_frame_table = property(lambda self: self.frames.last_frame_table)
    row_plans = property(lambda self: self.frames.row_plans, lambda self, on: setattr(self.frames, "row_plans", on))

    def _towers(self):
        return [tw for tw in (self.teacher, self.student) if tw is not None]

    # ---- data-parallel gradient reduction -------------------------------------
    def _reduce_tower(self, tower, moe_first):
        st = tower.store
        moe_lo = st.offsets[tower.GATES]
        if moe_first:
            self.reducer.reduce(st.grad, moe_lo, st.total, f32=True)
        else:
            self.reducer.reduce(st.grad, 0, moe_lo, f32=False)

    def label_grads(self):
        """The dL/dpred buffers the last step filled ({"teacher": ..., "student": ...}, whichever exist; the student's holds its label
        loss's and L_PRED's gradient).  For tests and debugging."""
        out = {}
        if self.teacher is not None and self.train_teacher and self._dp_t is not None:
            out["teacher"] = self._dp_t
        if self.student is not None and self._dp_s is not None:
            out["student"] = self._dp_s
        return out

    # ---- one training iteration -----------------------------------------------
    def step(self, x_raw, labels_u8, num_frames, apply=True, num_frames_host=None):
        """One iteration on the graph's own main stream (_on_main: stream semantics, num_frames_host)."""
        body = self._step_frozen_teacher if self.mode == "serial" else self._step
        return self._on_main((x_raw, labels_u8, num_frames), num_frames_host, lambda nh: body(x_raw, labels_u8, num_frames, apply, nh))

    def _student_label_loss(self, s_pred, labels_u8, B, sc):
        """The student's loss section where no teacher tower has a say in dL/dpred yet: L_CE and its gradient (OfflineDistillGraph puts
        ops.distill_losses_sparse here when the step was handed the batch's teacher lists)."""
        self.label_loss.fused(s_pred, labels_u8, self.losses[3:4], self._dp_s, grad_scale=sc["ce"] / B)

    def _step(self, x_raw, labels_u8, num_frames, apply=True, nh=None):
        """x_raw [B,300,F] f32 (or uint8), labels_u8 [B,V] uint8, num_frames [B] int32.
        Returns a dict mirroring the graph collections the reference's loop
        fetches (cs/train.py:336-344,420-425,516-517); tensors stay on device.

        Schedule: the teacher's backward and the whole student tower are independent once the
        teacher's forward is done (teacher tensors are constants in the student loss), so the
        student runs on a second HIP stream: its many small launches (M = batch L2 steps, 30-frame
        L1) fill the CUs that the teacher's under-filled launches leave idle."""
        B = x_raw.shape[0]
        V = labels_u8.shape[1]
        dev = self.device
        if self.dp and B != self.B:
            # every rank must step on the same number of videos: the factor all-gathers move round_up(B, 32) rows per
            # rank and the per-rank loss scales 1/(world*B) only add up to the global-batch mean for equal B
            raise ValueError("data-parallel step on %d videos, the graph was built for %d per rank (ragged batches are "
                             "not allowed under data parallelism: drop the remainder)" % (B, self.B))
        if self._dp_t is None or self._dp_t.shape[0] != B:
            self._dp_t = torch.empty((B, V), dtype=F32, device=dev)
            self._dp_s = torch.empty((B, V), dtype=F32, device=dev)
        need_student = self.student is not None
        main = torch.cuda.current_stream(dev)
        fp = self.frames
        tp, sp = frame_counts_and_plans(fp, num_frames, nh, self.teacher is not None, need_student)
        # "random" student frames: a new draw per training iteration (global_step counts one per train op, cs/train.py:332,416), other videos
        # on every rank - stateless, so a run is reproducible from its seed and a restored global_step
        fp.sampling_draw = self.global_step // ((self.teacher is not None) + (self.student is not None))
        fp.sampling_row0 = self.reducer.rank * B
        xt, xs = input_views(fp, x_raw, num_frames, tp, sp, need_student)     # (student only: the sub-sampled frames alone are read)
        for tw in self._towers():     # step k-1's deferred MoE / L2-level updates: now, under this step's L1 forward
            tw.run_deferred()
        self.losses.zero_()
        out = {}
        mark = self._mark
        mark("start", main)
        sc = dp_loss_scales(self.world)
        lr, l2c = self._lr_l2c(B)
        self._teacher_applied = self._student_applied = False
        two_streams = self.teacher is not None and need_student and self.overlap_towers
        side = self._side if two_streams else main
        early_student = two_streams and self.student_forward_early
        # "after_l1": the student's forward starts when the teacher's L1 level is done - next to the teacher's L2 chain
        # and MoE head (small launches), not next to its L1 steps (the roofline kernel keeps the chip to itself)
        mid_student = two_streams and not early_student and self.student_forward_after_l1
        s_state = s_pred = gen_s = early_s = None
        n_s, l1s, l2s, plan_s = sp if need_student else (None,) * 4

        def student_forward():                  # (on `side`)
            nonlocal s_state, s_pred
            mark("student_start", side)
            s_state, s_pred = self.student.forward(xs, l1s, l2s, plan_s)
            self._student_label_loss(s_pred, labels_u8, B, sc)
            mark("student_fwd_done", side)

        def student_forward_from_inputs():
            # The student's forward needs only its own inputs and weights: it can start next to the teacher's forward
            # (whose L2 / MoE tail is a chain of small launches that leaves most CUs idle);
            # only its distillation losses wait for the teacher's outputs.
            self._ev_in.record(main)
            side.wait_event(self._ev_in)
            with torch.cuda.stream(side):
                student_forward()

        if early_student:
            student_forward_from_inputs()
        if self.teacher is not None:
            l1, l2, plan_t = tp
            t_state, t_pred = self.teacher.forward(xt, l1, l2, plan_t, after_l1=student_forward_from_inputs if mid_student else None)
            self.label_loss.fused(t_pred, labels_u8, self.losses[0:1], self._dp_t, grad_scale=sc["ce"] / B)
            if two_streams:
                self._ev_fwd.record(main)
            mark("teacher_fwd_done", main)
        if need_student:
            if two_streams:
                side.wait_event(self._ev_fwd)
            with torch.cuda.stream(side):
                if not early_student and not mid_student:
                    student_forward()
                ds = None
                if self.teacher is not None:
                    if self._ds_s is None or self._ds_s.shape != s_state.shape:
                        self._ds_s = torch.empty_like(s_state)
                    ops.kl_pred_loss(t_pred, self.teacher.rowsum, s_pred, self.student.rowsum, self.losses[2:3], self._dp_s,
                                     grad_scale=sc["kl"], accumulate_grad=True)
                    ops.rep_loss(t_state, s_state, self.losses[1:2], self._ds_s, grad_scale=self.rep_w * sc["rep"])
                    ds = self._ds_s
                early_s = (lr, self.clip, l2c) if (apply and self.overlap_towers and self._aux_s is not None) else None
                st_s = self.student.store
                gen_s = self.student.backward_phases(
                    ds, self._dp_s, on_moe_grads_ready=None if early_s else (lambda: self._reduce_tower(self.student, True)),
                    aux=self._aux_s if self.overlap_towers else None, early_apply=early_s,
                    reduce_fn=(lambda lo, hi, f32=False: self.reducer_s.reduce_async(st_s.grad, lo, hi, f32=f32)) if (early_s and self.dp) else None,
                    dp=self.reducer_s if (early_s and self.dp) else None, defer=self.defer_updates and not self.dp, opt=self._opt_s)
        gen_t = None
        if self.teacher is not None:
            # weight-gradient GEMMs and the per-group clip+Adam go to an aux stream, under the BPTT chain
            # (the tower's outputs t_state / t_pred are separate buffers, untouched by the update)
            early_t = (lr, self.clip, l2c) if (apply and self.overlap_towers and self._aux_t is not None) else None
            st_t = self.teacher.store
            gen_t = self.teacher.backward_phases(
                None, self._dp_t, on_moe_grads_ready=None if early_t else (lambda: self._reduce_tower(self.teacher, True)),
                aux=self._aux_t if self.overlap_towers else None, early_apply=early_t,
                reduce_fn=(lambda lo, hi, f32=False: self.reducer.reduce_async(st_t.grad, lo, hi, f32=f32)) if (early_t and self.dp) else None,
                dp=self.reducer if (early_t and self.dp) else None, defer=self.defer_updates and not self.dp, opt=self._opt_t)
        # Host issue order of the two backward passes (same launches, same streams, same results): "sequential" = the student's
        # whole backward, then the teacher's; "interleaved" = phase by phase in the order in which the phases become ready on the
        # GPU (measured timeline, profiles/r04_timeline_default.txt) - what a ONE-communicator placement of the collectives needs
        # so that no tower's early collective queues behind the other tower's late one.
        gens = {"s": (gen_s, side), "t": (gen_t, main)}
        live = {k for k, (g_, _) in gens.items() if g_ is not None}
        order = self.ISSUE_ORDERS[self.issue_order] if (gen_s is not None and gen_t is not None) else ""
        def resume(who):
            g_, st_ = gens[who]
            with torch.cuda.stream(st_):
                if next(g_, self) is self:             # exhausted
                    live.discard(who)
        for who in order:                              # the scripted part (written for two LSTM layers per level) ...
            if who in live:
                resume(who)
        for who in ("s", "t"):                         # ... then each tower to its end, whatever --lstm_layers says: a tower needs
            while who in live:                         # 2 * lstm_layers + 2 resumptions, and an unfinished generator would silently
                resume(who)                            # skip the lowest layers' BPTT, weight gradients, Adam and the final stream joins
        assert not live
        if need_student:
            with torch.cuda.stream(side):
                if not early_s:
                    self._reduce_tower(self.student, False)
                self._student_applied = early_s is not None
                mark("student_done", side)
                if two_streams:
                    self._ev_student.record(side)
                    self._keep_alive(side, [xs], [sp])
            out.update(student_predictions=s_pred, student_state=s_state, num_frames_student=n_s,
                       student_loss_state=self.losses[1], pred_loss=self.losses[2], student_label_loss=self.losses[3])
        if self.teacher is not None:
            if not early_t:
                self._reduce_tower(self.teacher, False)
            mark("teacher_bwd_done", main)
            out.update(predictions=t_pred, teacher_state=t_state, loss=self.losses[0])
            self._teacher_applied = early_t is not None
        if two_streams:
            main.wait_event(self._ev_student)
        self.reducer.wait()
        if self.dp:
            # the loss values of the global batch, as part of the step (8 floats, in stream order behind the teacher's
            # collectives): loss_report() then needs no collective and may be called by any one rank, at any time
            self._losses_reduced.copy_(self.losses)
            self.reducer.all_reduce_small(self._losses_reduced)
        if apply:
            self._apply_gradients(B, lr)
        out["global_step"] = self.global_step
        return out

    def _step_frozen_teacher(self, x_raw, labels_u8, num_frames, apply=True, nh=None):
        """mode "serial": the input stage of _step (one pass for both towers), then _serial_step for the one student with the loss
        section ops.distill_losses.  Same inputs and `out` keys as _step."""
        B, V = x_raw.shape[0], labels_u8.shape[1]
        if self._dp_s is None or self._dp_s.shape[0] != B:
            self._dp_s = torch.empty((B, V), dtype=F32, device=self.device)
        fp = self.frames
        tp, sp = frame_counts_and_plans(fp, num_frames, nh, True, True)
        fp.sampling_draw, fp.sampling_row0 = self.global_step, 0          # one train op per iteration: a new "random" draw per step
        xt, xs = input_views(fp, x_raw, num_frames, tp, sp, True)
        on = self.distill_losses

        def loss_section(t_state, t_pred, fwd, ds):
            (s_state, s_pred), = fwd
            ops.distill_losses(t_pred, self.teacher.rowsum, s_pred, self.student.rowsum, labels_u8, t_state, s_state, self.losses,
                               self._dp_s, ds[0], g_ce=(1.0 / B) if "ce" in on else 0.0, g_kl=1.0 if "pred" in on else 0.0,
                               g_rep=self.rep_w if "rep" in on else 0.0)

        out = self._serial_step([self.student], xt, tp, [xs], [sp], labels_u8, [self._dp_s], apply, loss_section)
        out.update(out.pop("students")[0])
        return out

    def _apply_gradients(self, batch_size, lr=None):
        """Each train op increments global_step (cs/train.py:332,416 -> += 2 per iteration, README.md:116,121)."""
        l2c = self.reg_pen * 1e-8
        if lr is None:
            lr = self._lr_l2c(batch_size)[0]
        if self.teacher is not None and self.train_teacher:
            if not self._teacher_applied:
                self.teacher.apply_gradients(lr, self.clip, l2c)
            self.global_step += 1
        if self.student is not None:
            if not self._student_applied:
                self.student.apply_gradients(lr, self.clip, l2c)
            self.global_step += 1
        self._teacher_applied = self._student_applied = False

    def consolidate(self):
        """Collective (every rank calls it; a no-op on one rank): the row-sharded f32 MoE weights and Adam moments
        (MoeHead.shard) are all-gathered so that every rank holds the complete model again - before a checkpoint,
        state_dict(), or any update that does not go through the fused data-parallel path."""
        self.flush()
        for tw, red in ((self.teacher, self.reducer), (self.student, self.reducer_s)):
            if tw is not None:
                tw.moe.consolidate(red)

    @property
    def losses_for_report(self):
        """Device tensor loss_report() reads (a caller that logs one step behind the GPU clones it after the step)."""
        return self._losses_reduced if self.dp else self.losses

    def loss_report(self, losses=None):
        """Host floats in the order the reference logs them (cs/train.py:528-533), for the global batch.  Not a
        collective (under data parallelism step() has already summed the values over the ranks).  losses: a copy of
        losses_for_report taken after an earlier step (device or host tensor)."""
        v = (self.losses_for_report if losses is None else losses).tolist()
        rep = {k: v[i] for i, k in enumerate(self.LOSS_SLOTS)}
        if self.dp:   # sums over the ranks -> global-batch means (L_PRED is a batch sum)
            rep = {"label_loss": v[0] / self.world, "student_loss_state": v[1] / self.world, "pred_loss": v[2],
                   "student_label_loss": v[3] / self.world}
        return rep


class OfflineDistillGraph(DistillGraph):
    """Offline distillation: the student alone against the sparse lists of 1 .. 8 teacher prediction files (train
    --teacher_preds_pattern).  It IS DistillGraph(mode="student") - the finetune step: the same input pass, row plans, backward, update
    and streams, no teacher tower in memory - whose L_CE launch gives way to ops.distill_losses_sparse when step() is handed the
    batch's lists (teacher_lists = (idx [F, B, kp] int32, val [F, B, kp] f32) device tensors, inference.PriorTables.gather_device);
    without lists the step takes exactly the launches of mode "student".  teacher_mode "max" | "mean" and teacher_weights [F] (mean only)
    combine the files as ensemble_topk_rows combines prior files; distill_losses: a subset of ("pred", "ce") - a prediction file holds no
    state, so there is no L_REP.  global_step += 1 per iteration; "random" student frames are drawn anew per step."""

    OFFLINE_LOSSES = ("pred", "ce")
    MAX_FILES = ops.DISTILL_MAX_FILES

    def __init__(self, batch_size, every_n=10, teacher_mode="mean", teacher_weights=None, distill_losses=OFFLINE_LOSSES, **kw):
        if kw.pop("mode", "student") != "student":
            raise ValueError("OfflineDistillGraph is the mode 'student' graph: it has no teacher tower")
        on = check_distill_losses(distill_losses)
        if "rep" in on:
            raise ValueError("distill_losses %s: a prediction file carries no state, so offline distillation has no L_REP (pred, ce)"
                             % ",".join(on))
        if teacher_mode not in ops.ENSEMBLE_MODES:
            raise ValueError("teacher_mode %r (max | mean)" % (teacher_mode,))
        if teacher_weights is not None and teacher_mode != "mean":
            raise ValueError("teacher_weights are read in teacher_mode 'mean' only")
        super().__init__(batch_size, every_n=every_n, mode="student", **kw)
        if not losses_mod.is_default(self.label_loss):
            raise ValueError("OfflineDistillGraph has CrossEntropyLoss built into its loss section (evc_distill_losses_sparse), not %s"
                             % type(self.label_loss).__name__)
        if self.world > 1 or self.dp:
            raise ValueError("OfflineDistillGraph is not data parallel yet (process group of %d ranks): train the student on one device"
                             % self.world)
        self.offline_losses = on
        self.teacher_mode = teacher_mode
        self.teacher_weights = None if teacher_weights is None else np.asarray(teacher_weights, np.float32).reshape(-1)
        self._teacher_lists = None

    def step(self, x_raw, labels_u8, num_frames, apply=True, num_frames_host=None, teacher_lists=None):
        """DistillGraph.step; teacher_lists: None (the student-only step), or the (idx, val) lists of exactly these videos."""
        if teacher_lists is None:
            return super().step(x_raw, labels_u8, num_frames, apply, num_frames_host)
        idx, val = teacher_lists
        if self.teacher_weights is not None and self.teacher_weights.size != idx.shape[0]:
            raise ValueError("%d teacher_weights for the lists of %d files" % (self.teacher_weights.size, idx.shape[0]))
        self._teacher_lists = (idx, val)
        try:
            return self._on_main((x_raw, labels_u8, num_frames, idx, val), num_frames_host,
                                 lambda nh: self._step(x_raw, labels_u8, num_frames, apply, nh))
        finally:
            self._teacher_lists = None

    def _student_label_loss(self, s_pred, labels_u8, B, sc):
        if self._teacher_lists is None:
            return super()._student_label_loss(s_pred, labels_u8, B, sc)
        idx, val = self._teacher_lists
        on = self.offline_losses
        # losses[0] = CE of the combined teacher row, [2] = L_PRED, [3] = the student's L_CE; the scales of the serial step
        ops.distill_losses_sparse(idx, val, labels_u8, s_pred, self.losses, self._dp_s, mode=self.teacher_mode, weights=self.teacher_weights,
                                  g_ce=(sc["ce"] / B) if "ce" in on else 0.0, g_kl=sc["kl"] if "pred" in on else 0.0)

    def state_dict(self):
        """The variables a checkpoint of this graph holds: the student tower alone."""
        self.flush()
        return self.student.state_dict()


class SerialStudentView:
    """Student k of a SerialStudentsGraph as train.save_checkpoint / restore_checkpoint see a DistillGraph(mode="serial"): the
    shared frozen teacher, this student, its losses and frames, the common global_step."""

    mode = "serial"

    def __init__(self, graph, k, with_teacher=True):
        self._graph, self.k = graph, k
        self.teacher, self.student = graph.teacher if with_teacher else None, graph.students[k]
        self.distill_losses, self.student_sampling, self.every_n = graph.distill_losses[k], graph.student_sampling[k], graph.every_n[k]

    @property
    def global_step(self):
        return self._graph.global_step

    @global_step.setter
    def global_step(self, v):
        self._graph.global_step = int(v)

    def consolidate(self):
        self._graph.consolidate()


class SerialStudentsGraph(_TrainGraph):
    """Serial distillation of K students (1 <= K <= 8) against ONE forward of a frozen teacher per iteration: what K
    DistillGraph(mode="serial") runs on the same batches compute, with the teacher's forward, the batch's input pass for the teacher
    and the teacher's share of the loss section done once.  Each student has its own every_n, frame selection and loss subset; all
    share the batch, the seed of their initial weights (seed + 1: student k starts where the student of a serial DistillGraph with
    the same seed starts), the hyper-parameters and global_step (+= 1 per iteration: every student sees the learning-rate schedule
    of a run of its own).  One device, precision "bf16"."""

    LOSS_SLOTS = DistillGraph.LOSS_SLOTS
    MAX_STUDENTS = ops.DISTILL_MAX_STUDENTS

    def __init__(self, batch_size, every_n=(10,), student_sampling=None, distill_losses=None, feature_size=1152, vocab_size=4716,
                 max_frames=300, num_inputs_to_lstm=20, num_inputs_l1_student=5, lstm_cells=1024, lstm_layers=2, num_mixtures=2,
                 base_learning_rate=0.001, learning_rate_decay=1.0, learning_rate_decay_examples=4000000,
                 regularization_penalty=2.0, clip_gradient_norm=1.0, count_rep_twice=True, device="cuda:0", seed=7,
                 process_group=None, overlap_towers=True, precision="bf16", sampling_seed=0):
        every_n = [int(e) for e in every_n]
        K = len(every_n)
        if not 1 <= K <= self.MAX_STUDENTS:
            raise ValueError("SerialStudentsGraph: %d students (1 .. %d)" % (K, self.MAX_STUDENTS))
        student_sampling = ["uniform"] * K if student_sampling is None else list(student_sampling)
        distill_losses = [DistillGraph.DISTILL_LOSSES] * K if distill_losses is None else list(distill_losses)
        if len(student_sampling) != K or len(distill_losses) != K:
            raise ValueError("SerialStudentsGraph: %d every_n values, %d student_sampling words, %d distill_losses subsets: one of each "
                             "per student" % (K, len(student_sampling), len(distill_losses)))
        world = 1
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            world = torch.distributed.get_world_size(process_group)
        if world > 1:
            raise ValueError("SerialStudentsGraph is not data parallel (process group of %d ranks): train the students against the "
                             "frozen teacher on one device" % world)
        if precision != "bf16":
            raise ValueError("SerialStudentsGraph: precision %r (bf16 only: the input image of the other layouts is decided over the towers "
                             "that share it)" % (precision,))
        for e in every_n:
            validate_every_n(e, num_inputs_l1_student, max_frames)
        self.every_n = tuple(every_n)
        self.student_sampling = tuple(ops.check_student_sampling(w) for w in student_sampling)
        self.distill_losses = tuple(check_distill_losses(w) for w in distill_losses)
        self.K, self.B, self.sampling_seed = K, batch_size, int(sampling_seed)
        self.max_frames, self.C1, self.C2 = max_frames, num_inputs_to_lstm, num_inputs_l1_student
        self.lr0, self.lr_decay, self.lr_decay_examples = base_learning_rate, learning_rate_decay, learning_rate_decay_examples
        self.reg_pen, self.clip = regularization_penalty, clip_gradient_norm
        self.rep_w = 2.0 if count_rep_twice else 1.0
        self.device = torch.device(device)
        self.precision, self.row_plans = precision, True
        self.world, self.dp = 1, False
        self.global_step = 0
        self.teacher = HLstmTower(batch_size, max_frames, num_inputs_to_lstm, feature_size, vocab_size, lstm_cells, lstm_layers,
                                  num_mixtures, device, False, "model", seed)
        self.teacher.store.drop_training_state()
        self.students = [HLstmTower(batch_size, max_frames // e, num_inputs_l1_student, feature_size, vocab_size, lstm_cells,
                                    lstm_layers, num_mixtures, device, True, "model_student", seed + 1) for e in self.every_n]
        # one input pass per tower: the frozen teacher, and each student with its own every_n and frame selection
        self._t_frames = FramePlan(teacher=self.teacher, C1=self.C1, C2=self.C2, max_frames=max_frames)
        self._s_frames = [FramePlan(None, s, e, self.C1, self.C2, max_frames, True, w, self.sampling_seed)
                          for s, e, w in zip(self.students, self.every_n, self.student_sampling)]
        self.losses = torch.zeros((K, 4), dtype=F32, device=self.device)
        self._dp_s = self._ds_serial = None
        self._student_applied = False       # (all K students: their updates run inside the step together or not at all)
        self.overlap_towers = overlap_towers
        self.defer_updates = os.environ.get("EVC_DEFER_UPDATES", "0") == "1"
        self._make_streams()

    def _towers(self):
        return self.students

    def student_view(self, k, with_teacher=True):
        """with_teacher=False: the student alone (restoring student k > 0 must not load the shared teacher again)."""
        return SerialStudentView(self, k, with_teacher)

    @property
    def last_frame_tables(self):
        """Per student: the source-frame table of the last batch (None for a `uniform` student, which needs none)."""
        return [p.last_frame_table for p in self._s_frames]

    def step(self, x_raw, labels_u8, num_frames, apply=True, num_frames_host=None):
        """One iteration of every student on this batch (DistillGraph.step's stream semantics and arguments)."""
        return self._on_main((x_raw, labels_u8, num_frames), num_frames_host, lambda nh: self._step(x_raw, labels_u8, num_frames, apply, nh))

    def _step(self, x_raw, labels_u8, num_frames, apply, nh):
        """The input stage - one pass per tower -, then _serial_step for the K students with the loss section ops.distill_losses_multi."""
        B, V = x_raw.shape[0], labels_u8.shape[1]
        if self._dp_s is None or self._dp_s[0].shape[0] != B:
            self._dp_s = [torch.empty((B, V), dtype=F32, device=self.device) for _ in range(self.K)]
        tp, _ = frame_counts_and_plans(self._t_frames, num_frames, nh, True, False)
        xt, _ = input_views(self._t_frames, x_raw, num_frames, tp, None, False)
        sps, xss = [], []
        # the keys of the content-aware strategies depend on the batch alone: once, for every student that ranks by them
        keys = ops.frame_change_keys(x_raw, num_frames) if any(scored_sampling(p) for p in self._s_frames) else None
        for p in self._s_frames:
            p.sampling_draw, p.sampling_row0 = self.global_step, 0      # one train op per iteration: a new "random" draw per step
            _, sp = frame_counts_and_plans(p, num_frames, nh, False, True)
            sps.append(sp)
            xss.append(input_views(p, x_raw, num_frames, None, sp, True, keys=keys)[1])
        on = self.distill_losses

        def loss_section(t_state, t_pred, fwd, ds):
            ops.distill_losses_multi(t_pred, self.teacher.rowsum, labels_u8, t_state, [f[1] for f in fwd],
                                     [s.rowsum for s in self.students], [f[0] for f in fwd], self.losses, self._dp_s, ds,
                                     g_ce=[(1.0 / B) if "ce" in o else 0.0 for o in on], g_kl=[1.0 if "pred" in o else 0.0 for o in on],
                                     g_rep=[self.rep_w if "rep" in o else 0.0 for o in on])

        return self._serial_step(self.students, xt, tp, xss, sps, labels_u8, self._dp_s, apply, loss_section)

    def _apply_gradients(self, batch_size, lr=None):
        """Every student's train op; global_step += 1 for the iteration."""
        l2c = self.reg_pen * 1e-8
        if lr is None:
            lr = self._lr_l2c(batch_size)[0]
        if not self._student_applied:
            for s in self.students:
                s.apply_gradients(lr, self.clip, l2c)
        self.global_step += 1
        self._student_applied = False

    def consolidate(self):
        """One rank: nothing is sharded; the deferred updates are joined (as DistillGraph.consolidate does first)."""
        self.flush()

    @property
    def losses_for_report(self):
        return self.losses

    def loss_report(self, losses=None):
        """A list of K dicts keyed by LOSS_SLOTS (host floats).  losses: a copy of losses_for_report taken after an earlier step."""
        v = (self.losses if losses is None else losses).reshape(self.K, 4).tolist()
        return [{name: v[k][i] for i, name in enumerate(self.LOSS_SLOTS)} for k in range(self.K)]


class EnsembleDistillGraph(_TrainGraph):
    """Serial distillation of ONE student against J frozen teachers (1 <= J <= 8) per iteration: the teachers' predictions are combined
    as an ensemble combines them (``teacher_mode`` "max" | "mean" with ``teacher_weights``), their states by ``rep_weights``, and the
    student is trained against the combination (ops.distill_losses_ensemble).  ``teachers``: a list of (tower, every_n, student_sampling)
    as EnsembleGraph's members - 'teacher' = an all-frames tower (scope `model`; every_n and the word are ignored), 'student' = a
    few-frame tower (scope `model_student`) at its own every_n and frame selection: teacher-assistant distillation.  Entry 0 is a
    'teacher' tower: it is `self.teacher`, the model/* of the checkpoint.  The student is built as DistillGraph(mode="serial") builds
    its own (seed + 1, its own FramePlan); with one teacher and weight 1 the step computes what that graph computes.  global_step += 1
    per iteration.  One device, precision "bf16"."""

    LOSS_SLOTS = DistillGraph.LOSS_SLOTS
    MAX_TEACHERS = ops.DISTILL_MAX_TEACHERS
    mode = "ensemble"

    def __init__(self, batch_size, teachers=(("teacher", 1, "uniform"),), every_n=10, teacher_mode="mean", teacher_weights=None,
                 rep_weights=None, student_sampling="uniform", distill_losses=DistillGraph.DISTILL_LOSSES, feature_size=1152,
                 vocab_size=4716, max_frames=300, num_inputs_to_lstm=20, num_inputs_l1_student=5, lstm_cells=1024, lstm_layers=2,
                 num_mixtures=2, base_learning_rate=0.001, learning_rate_decay=1.0, learning_rate_decay_examples=4000000,
                 regularization_penalty=2.0, clip_gradient_norm=1.0, count_rep_twice=True, device="cuda:0", seed=7, process_group=None,
                 overlap_towers=True, precision="bf16", sampling_seed=0):
        teachers = [tuple(t) + (1, "uniform")[len(t) - 1:] for t in teachers]
        J = len(teachers)
        if not 1 <= J <= self.MAX_TEACHERS:
            raise ValueError("EnsembleDistillGraph: %d teachers (1 .. %d)" % (J, self.MAX_TEACHERS))
        for tower, _, _ in teachers:
            if tower not in ("teacher", "student"):
                raise ValueError("EnsembleDistillGraph: tower %r (teacher | student)" % (tower,))
        if teachers[0][0] != "teacher":
            raise ValueError("EnsembleDistillGraph: entry 0 is a %r tower: the checkpoint's model/* is entry 0, a 'teacher' tower" % (teachers[0][0],))
        if teacher_mode not in ops.ENSEMBLE_MODES:
            raise ValueError("EnsembleDistillGraph: teacher_mode %r (max | mean)" % (teacher_mode,))
        if teacher_weights is not None and teacher_mode != "mean":
            raise ValueError("EnsembleDistillGraph: teacher_weights are read in teacher_mode 'mean' only")
        w = np.full(J, np.float32(1) / np.float32(J), np.float32) if teacher_weights is None else np.asarray(teacher_weights, np.float32).reshape(-1)
        r = np.asarray([1.0] + [0.0] * (J - 1) if rep_weights is None else rep_weights, np.float32).reshape(-1)
        if w.size != J or r.size != J:
            raise ValueError("EnsembleDistillGraph: %d teacher_weights and %d rep_weights for %d teachers" % (w.size, r.size, J))
        world = 1
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            world = torch.distributed.get_world_size(process_group)
        if world > 1:
            raise ValueError("EnsembleDistillGraph is not data parallel (process group of %d ranks): train the student against the "
                             "frozen teachers on one device" % world)
        if precision != "bf16":
            raise ValueError("EnsembleDistillGraph: precision %r (bf16 only: the input image of the other layouts is decided over the towers "
                             "that share it)" % (precision,))
        self.distill_losses = check_distill_losses(distill_losses)
        if not r.any():
            raise ValueError("EnsembleDistillGraph: every rep_weight is 0: L_REP and its gradient need a combined state (leave the term out "
                             "of the training with distill_losses instead)")
        validate_every_n(every_n, num_inputs_l1_student, max_frames)
        for tower, e, _ in teachers:
            if tower == "student":
                validate_every_n(int(e), num_inputs_l1_student, max_frames)
        self.teacher_towers = tuple(t[0] for t in teachers)
        self.teacher_every_n = tuple(1 if t[0] == "teacher" else int(t[1]) for t in teachers)
        self.teacher_sampling = tuple("uniform" if t[0] == "teacher" else ops.check_student_sampling(t[2]) for t in teachers)
        self.teacher_mode = teacher_mode
        self.teacher_weights = None if teacher_mode == "max" else w
        self.rep_weights = r
        self.J, self.B, self.every_n = J, batch_size, every_n
        self.student_sampling, self.sampling_seed = ops.check_student_sampling(student_sampling), int(sampling_seed)
        self.max_frames, self.C1, self.C2 = max_frames, num_inputs_to_lstm, num_inputs_l1_student
        self.lr0, self.lr_decay, self.lr_decay_examples = base_learning_rate, learning_rate_decay, learning_rate_decay_examples
        self.reg_pen, self.clip = regularization_penalty, clip_gradient_norm
        self.rep_w = 2.0 if count_rep_twice else 1.0
        self.device = torch.device(device)
        self.precision, self.row_plans = precision, True
        self.world, self.dp = 1, False
        self.global_step = 0
        self.teachers = []
        for tower, e in zip(self.teacher_towers, self.teacher_every_n):
            if tower == "teacher":
                tw = HLstmTower(batch_size, max_frames, num_inputs_to_lstm, feature_size, vocab_size, lstm_cells, lstm_layers, num_mixtures,
                                device, False, "model", seed)
            else:
                tw = HLstmTower(batch_size, max_frames // e, num_inputs_l1_student, feature_size, vocab_size, lstm_cells, lstm_layers,
                                num_mixtures, device, False, "model_student", seed + 1)
            tw.store.drop_training_state()
            self.teachers.append(tw)
        self.teacher = self.teachers[0]
        self.student = HLstmTower(batch_size, max_frames // every_n, num_inputs_l1_student, feature_size, vocab_size, lstm_cells, lstm_layers,
                                  num_mixtures, device, True, "model_student", seed + 1)
        # one all-frames input pass for every 'teacher' tower; one pass each for the 'student'-tower teachers and the trained student
        self._t_frames = FramePlan(teacher=self.teacher, C1=self.C1, C2=self.C2, max_frames=max_frames)
        self._a_frames = [None if tower == "teacher" else FramePlan(None, tw, e, self.C1, self.C2, max_frames, True, word, self.sampling_seed)
                          for tower, tw, e, word in zip(self.teacher_towers, self.teachers, self.teacher_every_n, self.teacher_sampling)]
        self.frames = FramePlan(None, self.student, every_n, self.C1, self.C2, max_frames, True, self.student_sampling, self.sampling_seed)
        # [0:4] the LOSS_SLOTS, [4:4 + J] every teacher's own CE (evc_distill_losses_ensemble's teacher_ce); 12 floats = three rows of four
        self.losses = torch.zeros(4 + self.MAX_TEACHERS, dtype=F32, device=self.device)
        self._dp_s = self._ds_serial = self._pred_comb = None
        self._student_applied = False
        self.overlap_towers = overlap_towers
        self.defer_updates = os.environ.get("EVC_DEFER_UPDATES", "0") == "1"
        self._make_streams()

    S = property(lambda self: self.frames.S)
    last_frame_table = property(lambda self: self.frames.last_frame_table)

    def _towers(self):
        return [self.student]

    def teacher_meta(self):
        """What a checkpoint records of the teachers besides their sources: towers, every_n, sampling, mode, weights, rep weights."""
        return dict(towers=list(self.teacher_towers), every_n=list(self.teacher_every_n), sampling=list(self.teacher_sampling),
                    mode=self.teacher_mode, weights=None if self.teacher_weights is None else [float(x) for x in self.teacher_weights],
                    rep_weights=[float(x) for x in self.rep_weights])

    def step(self, x_raw, labels_u8, num_frames, apply=True, num_frames_host=None):
        """One iteration (DistillGraph.step's stream semantics and arguments)."""
        return self._on_main((x_raw, labels_u8, num_frames), num_frames_host, lambda nh: self._step(x_raw, labels_u8, num_frames, apply, nh))

    def _step(self, x_raw, labels_u8, num_frames, apply, nh):
        """The input stage - one all-frames pass shared by the 'teacher' towers, one pass per 'student'-tower teacher and one for the
        trained student -, then _serial_step: the J teacher forwards one after another on `main`, the student's forward on `side` from the
        start, the loss section ops.distill_losses_ensemble on `side` once all are done, the student's backward and update as ever.
        `out`: DistillGraph's keys, "predictions" being the combined row the student is trained against; "teacher_predictions" /
        "teacher_states": the J teachers' own, "teacher_label_losses": their CE."""
        B, V = x_raw.shape[0], labels_u8.shape[1]
        if self._dp_s is None or self._dp_s.shape[0] != B:
            self._dp_s = torch.empty((B, V), dtype=F32, device=self.device)
            self._pred_comb = torch.empty((B, V), dtype=F32, device=self.device)
        tp, _ = frame_counts_and_plans(self._t_frames, num_frames, nh, True, False)
        xt, _ = input_views(self._t_frames, x_raw, num_frames, tp, None, False)
        # the keys of the content-aware strategies depend on the batch alone: once, for every tower that ranks by them
        plans = [p for p in self._a_frames if p is not None] + [self.frames]
        keys = ops.frame_change_keys(x_raw, num_frames) if any(scored_sampling(p) for p in plans) else None
        a_in = []
        for p in self._a_frames:
            if p is None:
                a_in.append(None)
                continue
            p.sampling_draw, p.sampling_row0 = 0, 0                       # a frozen tower sees the frames it is served with: draw 0, as EvalGraph
            _, sp_a = frame_counts_and_plans(p, num_frames, nh, False, True)
            a_in.append((input_views(p, x_raw, num_frames, None, sp_a, True, keys=keys)[1], sp_a))
        fp = self.frames
        fp.sampling_draw, fp.sampling_row0 = self.global_step, 0          # one train op per iteration: a new "random" draw per step
        _, sp = frame_counts_and_plans(fp, num_frames, nh, False, True)
        xs = input_views(fp, x_raw, num_frames, None, sp, True, keys=keys)[1]
        on = self.distill_losses

        def teacher_forwards():
            states, preds = [], []
            for tw, a in zip(self.teachers, a_in):
                if a is None:
                    st, pr = tw.forward(xt, tp[0], tp[1], tp[2])
                else:
                    st, pr = tw.forward(a[0], a[1][1], a[1][2], a[1][3])
                states.append(st)
                preds.append(pr)
            return states, preds

        def loss_section(t_states, t_preds, fwd, ds):
            (s_state, s_pred), = fwd
            ops.distill_losses_ensemble(t_preds, [st if rw != 0 else None for st, rw in zip(t_states, self.rep_weights)], labels_u8, s_pred,
                                        s_state, self.losses[0:4], self._dp_s, ds[0], mode=self.teacher_mode, weights=self.teacher_weights,
                                        rep_weights=self.rep_weights, g_ce=(1.0 / B) if "ce" in on else 0.0,
                                        g_kl=1.0 if "pred" in on else 0.0, g_rep=self.rep_w if "rep" in on else 0.0,
                                        teacher_ce=self.losses[4:4 + self.J], pred_comb=self._pred_comb)

        out = self._serial_step([self.student], xt, tp, [xs], [sp], labels_u8, [self._dp_s], apply, loss_section, teacher_forwards)
        out.update(out.pop("students")[0])
        out.update(teacher_predictions=out["predictions"], teacher_states=out.pop("teacher_state"), predictions=self._pred_comb,
                   teacher_label_losses=self.losses[4:4 + self.J])
        out["teacher_state"] = out["teacher_states"][0]
        return out

    def _apply_gradients(self, batch_size, lr=None):
        """The student's train op; global_step += 1 for the iteration."""
        l2c = self.reg_pen * 1e-8
        if lr is None:
            lr = self._lr_l2c(batch_size)[0]
        if not self._student_applied:
            self.student.apply_gradients(lr, self.clip, l2c)
        self.global_step += 1
        self._student_applied = False

    def consolidate(self):
        """One rank: nothing is sharded; the deferred updates are joined (as DistillGraph.consolidate does first)."""
        self.flush()

    @property
    def losses_for_report(self):
        return self.losses

    def loss_report(self, losses=None):
        """Host floats keyed by LOSS_SLOTS ("label_loss": the CE of the combined prediction), plus "teacher_<j>_label_loss" for each of
        the J teachers.  losses: a copy of losses_for_report taken after an earlier step."""
        v = (self.losses if losses is None else losses).reshape(-1).tolist()
        rep = {k: v[i] for i, k in enumerate(self.LOSS_SLOTS)}
        rep.update({"teacher_%d_label_loss" % j: v[4 + j] for j in range(self.J)})
        return rep


class EvalGraph(_StepGraph):
    """Forward-only graph of cs/validate.py:109-189 (teacher built too, so that the
    student_state_loss ||teacher_state - student_state||^2 can be logged) and of
    cs/eval_finetune.py:108-175 (``student_only``).  Towers are built with
    training=False (no backward tape); ``restore`` takes a TF-named state dict.
    ``teacher_only``: the teacher alone (no student allocated) - the forward the inference binary serves from a
    train.py checkpoint (cs/train.py:338 puts the teacher's predictions in "predictions"); step() then returns
    predictions / teacher_state / teacher_predictions and computes no loss."""

    def __init__(self, batch_size, every_n=10, student_only=False, feature_size=1152, vocab_size=4716, max_frames=300,
                 num_inputs_to_lstm=20, num_inputs_l1_student=5, lstm_cells=1024, lstm_layers=2, num_mixtures=2,
                 device="cuda:0", precision="bf16", teacher_only=False, student_sampling="uniform", sampling_seed=0, label_loss=None):
        self.label_loss = _resolve_label_loss(label_loss, vocab_size)       # the loss reported as out["loss"] (--label_loss)
        if student_only and teacher_only:
            raise ValueError("EvalGraph: student_only and teacher_only exclude each other")
        # the student's frames (ops.STUDENT_SAMPLING); evaluation draws "random" frames with draw 0: the same frames for the same batching
        self.student_sampling, self.sampling_seed = ops.check_student_sampling(student_sampling), int(sampling_seed)
        if not teacher_only:
            validate_every_n(every_n, num_inputs_l1_student, max_frames)
        self.every_n, self.max_frames, self.C1, self.C2 = every_n, max_frames, num_inputs_to_lstm, num_inputs_l1_student
        self.S = max_frames // every_n
        self.device = torch.device(device)
        self.teacher = None
        if not student_only:
            self.teacher = HLstmTower(batch_size, max_frames, num_inputs_to_lstm, feature_size, vocab_size, lstm_cells,
                                      lstm_layers, num_mixtures, device, False, "model", 7)
        self.student = None
        if not teacher_only:
            self.student = HLstmTower(batch_size, self.S, num_inputs_l1_student, feature_size, vocab_size, lstm_cells,
                                      lstm_layers, num_mixtures, device, False, "model_student", 8)
        self.precision = precision
        student_light(self.student, precision)
        if precision != "bf16":
            for tw in (self.teacher, self.student):
                if tw is not None:
                    tw.set_precision(precision)
        self.losses = torch.zeros(4, dtype=F32, device=self.device)
        self._main, self._side = concurrent_streams(self.device, 4)[:2]
        self._ev_in, self._ev_out = torch.cuda.Event(), torch.cuda.Event()
        self.row_plans = precision != "split"
        self.frames = FramePlan(self.teacher, self.student, every_n, self.C1, self.C2, max_frames, self.row_plans,
                                self.student_sampling, self.sampling_seed)

    last_frame_table = property(lambda self: self.frames.last_frame_table)

    def restore(self, state_dict):
        """saver_teacher / saver_student .restore (cs/validate.py:350-384): the 11 variables of each tower by name."""
        for tw in (self.teacher, self.student):
            if tw is not None:
                tw.load_state_dict(state_dict)

    def step(self, x_raw, labels_u8, num_frames, num_frames_host=None, keys=None):
        """``keys``: the batch's ops.frame_change_keys, computed on the caller's stream by an owner of several graphs (EnsembleGraph)."""
        return self._on_main((x_raw, labels_u8, num_frames, keys), num_frames_host, lambda nh: self._step(x_raw, labels_u8, num_frames, nh, keys))

    def _step(self, x_raw, labels_u8, num_frames, nh, keys=None):
        """Returns predictions (student), student_label_loss, student_state_loss (teacher_student only) - the
        tensors cs/validate.py:240 fetches.  The two towers are independent: they run on two streams."""
        if self.student is None:
            return self._step_teacher(x_raw, num_frames, nh)
        main = torch.cuda.current_stream(self.device)
        tp, sp = frame_counts_and_plans(self.frames, num_frames, nh, self.teacher is not None, True)
        xt, xs = input_views(self.frames, x_raw, num_frames, tp, sp, True, keys=keys)
        self.losses.zero_()
        out = {}
        self._ev_in.record(main)
        self._side.wait_event(self._ev_in)
        n_s, l1s, l2s, plan_s = sp
        with torch.cuda.stream(self._side):
            s_state, s_pred = self.student.forward(xs, l1s, l2s, plan_s)
            self.label_loss.fused(s_pred, labels_u8, self.losses[0:1])
            self._ev_out.record(self._side)
            self._keep_alive(self._side, [xs], [sp])
        if self.teacher is not None:
            l1, l2, plan_t = tp
            t_state, t_pred = self.teacher.forward(xt, l1, l2, plan_t)
            out.update(teacher_state=t_state, teacher_predictions=t_pred)
        main.wait_event(self._ev_out)
        if self.teacher is not None:
            ops.rep_loss(t_state, s_state, self.losses[1:2])
            out["student_state_loss"] = self.losses[1]
        out.update(predictions=s_pred, student_state=s_state, num_frames=n_s, student_label_loss=self.losses[0],
                   loss=self.losses[0])
        return out

    def _step_teacher(self, x_raw, num_frames, nh):
        """teacher_only: the teacher's forward alone (same input views, row plans and precision handling as _step)."""
        tp, _ = frame_counts_and_plans(self.frames, num_frames, nh, True, False)
        xt, _ = input_views(self.frames, x_raw, num_frames, tp, None, False)
        l1, l2, plan_t = tp
        t_state, t_pred = self.teacher.forward(xt, l1, l2, plan_t)
        return dict(predictions=t_pred, teacher_state=t_state, teacher_predictions=t_pred)


def member_graph(batch_size, member, kw):
    """The forward-only graph of one ensemble member / cascade stage: ``member`` = (tower, every_n[, student_sampling[, nextvlad]]), kw =
    EvalGraph's keywords.  Without a fourth element (or with None there) an EvalGraph that is teacher_only / student_only; with one - a
    dict of NeXtVladEvalGraph's size keywords - a NeXtVladEvalGraph of that tower, which takes feature_size, vocab_size, max_frames,
    num_mixtures, device, precision and label_loss from kw."""
    tower, every_n = member[0], member[1]
    if len(member) > 3 and member[3] is not None:
        from .vlad_graphs import NeXtVladEvalGraph
        shared = {k: kw[k] for k in ("feature_size", "vocab_size", "max_frames", "num_mixtures", "device", "precision", "label_loss") if k in kw}
        return NeXtVladEvalGraph(batch_size, tower=tower, every_n=every_n, student_sampling=member[2] or "uniform", **shared, **member[3])
    mkw = dict(kw)
    if len(member) > 2 and member[2] is not None:     # (tower, every_n, student_sampling): this member's own frame selection
        mkw["student_sampling"] = member[2]
    return EvalGraph(batch_size, every_n=every_n, student_only=tower == "student", teacher_only=tower == "teacher", **mkw)


class EnsembleGraph:
    """N forward-only members for one input: each an EvalGraph that is ``teacher_only`` or ``student_only`` at its own every_n, all on
    one device with one --precision and one set of model sizes (``members``: list of (tower, every_n[, student_sampling]), tower
    'teacher' | 'student'; the other arguments are EvalGraph's, student_sampling / sampling_seed among them); a member with a fourth
    element is a NeXtVladEvalGraph (member_graph).  step() runs every member on the same input tensors and returns their prediction tensors,
    each the buffer of that member's own tower, so all of them are alive together for ops.ensemble_topk_rows."""

    def __init__(self, batch_size, members, **kw):
        if not members:
            raise ValueError("EnsembleGraph: no members")
        self.members = []
        for member in members:
            tower, every_n = member[0], member[1]
            if tower not in ("teacher", "student"):
                raise ValueError("EnsembleGraph: tower %r (teacher | student)" % (tower,))
            self.members.append(member_graph(batch_size, member, kw))

    def restore(self, state_dicts):
        """Each member restores its own checkpoint (the 11 variables of its tower by name)."""
        if len(state_dicts) != len(self.members):
            raise ValueError("EnsembleGraph.restore: %d state dicts for %d members" % (len(state_dicts), len(self.members)))
        for g, sd in zip(self.members, state_dicts):
            g.restore(sd)

    def step(self, x_raw, labels_u8, num_frames, num_frames_host=None):
        if num_frames_host is None:
            num_frames_host = num_frames.cpu()
        # the keys of the content-aware strategies depend on the batch alone: once, for every member that ranks by them
        keys = ops.frame_change_keys(x_raw, num_frames) if any(scored_sampling(g.frames) for g in self.members) else None
        return [g.step(x_raw, labels_u8, num_frames, num_frames_host=num_frames_host, keys=keys if scored_sampling(g.frames) else None)["predictions"]
                for g in self.members]


class SingleTowerGraph(_StepGraph):
    """Teacher-only training step for dict-returning models (DbofModel,
    FrameLevelLogisticModel).  The reference's train.py cannot run these
    (it unpacks the H-LSTM tuple, cs/train.py:282 - SURVEY.md Appendix D-8);
    this follows the upstream starter-code semantics it was forked from:
    final_loss = regularization_penalty*reg + CE, one train op, global_step += 1.

    Update: the MoE head's two weight matrices go through MoeHead.fused_update (gradient recomputed from its
    rank-B factors inside the clip + Adam pass) whenever the step also applies; the other variables through
    clip_by_norm + TF-Adam on the materialised gradients.
    Data parallel: the gradients of each backward stage (MoE bias -> hidden layer -> cluster layer) are all-reduced on
    a side stream as soon as the stage is final, under the rest of the backward pass; the MoE weights need no gradient
    all-reduce at all (factor all-gather + row-sharded update, as in DistillGraph); batch-norm statistics and the
    batch-norm scale/offset gradients of cluster_bn / hidden1_bn are global through the all-reduced f64 sums."""

    def __init__(self, tower, base_learning_rate=0.001, learning_rate_decay=1.0, learning_rate_decay_examples=4000000,
                 regularization_penalty=2.0, clip_gradient_norm=1.0, process_group=None, label_loss=None):
        self.tower, self.device = tower, tower.device
        self.label_loss = _resolve_label_loss(label_loss, getattr(tower, "V", None))      # --label_loss (None = CrossEntropyLoss)
        self.lr0, self.lr_decay, self.lr_decay_examples = base_learning_rate, learning_rate_decay, learning_rate_decay_examples
        self.reg_pen, self.clip, self.pg = regularization_penalty, clip_gradient_norm, process_group
        self.reducer = GradReducer(process_group)
        self.world, self.dp = self.reducer.world, self.reducer.active
        self.global_step = 0
        self.losses = torch.zeros(4, dtype=F32, device=self.device)
        self._dp = None
        self.moe = getattr(tower, "moe", None)
        self.fused_moe_update = True
        if self.dp and self.moe is not None and self.moe.can_fuse_update():
            self.moe.shard(self.reducer.shard_world, self.reducer.rank)      # while nothing is in flight
        self._aux = torch.cuda.Stream(device=self.device) if self.device.type == "cuda" else None

    def consolidate(self):
        """Collective (no-op on one rank): complete f32 MoE weights / moments on every rank (before a checkpoint)."""
        if self.moe is not None:
            self.moe.consolidate(self.reducer)

    def label_grads(self):
        """The dL/dpred buffer the last step filled, as {"teacher": ...} (the one tower).  For tests and debugging."""
        return {} if self._dp is None else {"teacher": self._dp}

    def step(self, x_raw, labels_u8, num_frames, uniform=None, apply=True, num_frames_host=None):
        """x_raw [B,T,F] float32 or uint8 (as the reader delivers it: Dequantize is fused into the input kernels).
        num_frames_host: the frame counts on the host, for a NeXtVladTower / NetVladTower in grid mode (its packed rows are laid out from them
        without a device sync; no draw is made in that mode)."""
        B, V = labels_u8.shape
        if self._dp is None or self._dp.shape[0] != B:
            self._dp = torch.empty((B, V), dtype=F32, device=self.device)
        tw = self.tower
        if self.dp and B != tw.B:
            raise ValueError("data-parallel step on %d videos, the tower was built for %d per rank (ragged batches are not "
                             "allowed under data parallelism: drop the remainder)" % (B, tw.B))
        kw = tw.step_kwargs(self.global_step)        # (what the tower's forward derives from the step: a dropout mask, "random" frames)
        if tw.frames == "grid":
            pred = tw.forward(x_raw, num_frames, num_frames_host=num_frames_host, **kw)
        elif tw.takes_uniform_draw:
            if uniform is None:     # (SampleRandomSequence draws one start per video: column 0 is used)
                uniform = torch.rand((B, tw.S), dtype=F32, device=self.device)
            self.last_uniform = uniform              # the tf.random_uniform draw of this step (SampleRandomFrames)
            pred = tw.forward(x_raw, num_frames, uniform, **kw)
        else:
            pred = tw.forward(x_raw, num_frames)
        self.losses.zero_()
        self.label_loss.fused(pred, labels_u8, self.losses[0:1], self._dp, grad_scale=1.0 / (B * self.world))
        fuse, fused_names = self._fuse_moe_update(apply, self.moe, tw.precision, self.dp)
        if self.moe is not None and not fuse and getattr(self.moe, "_stale", False):
            raise RuntimeError("the MoE weights are sharded over the ranks (fused data-parallel update); call consolidate() "
                               "on every rank before a step that does not apply through it")
        # data parallel: the exchange that carries the MoE gradient is chosen by shape (MoeHead.dp_route): factor all-gather (fused update) or
        # bf16 reduce-scatter of the materialised gradient onto the owners' slabs (sharded_update) - either way no all-reduce of those segments
        route_rs = bool(fuse and self.dp and self.moe.dp_route(self.reducer.shard_world) == "reduce_scatter")
        main = torch.cuda.current_stream(self.device)
        stages = tw.grad_stages()
        skip =tuple(getattr(tw, "global_grad_names", ())) + fused_names

        def on_stage(i):
            # data parallel: SUM of this stage's per-rank gradients on the side stream, in stream order behind the kernels
            # that produced them; batch-norm gradients that are already global and the fused MoE weights stay out
            if not self.dp:
                return
            self._aux.wait_stream(main)
            with torch.cuda.stream(self._aux):
                for lo, hi in tw.grad_ranges(exclude=skip, only=stages[i]):
                    self.reducer.reduce_async(tw.store.grad, lo, hi)

        tw.backward(self._dp, moe_weight_grads=(not fuse) or route_rs, on_stage=on_stage)
        if self.dp:
            main.wait_stream(self._aux)
        if apply:
            self._update_tower(tw, self.moe, B, fuse, fused_names, route_rs, self.reducer if self.dp else None)
        return {"predictions": pred, "loss": self.losses[0], "global_step": self.global_step}


# The VLAD families' graphs and checkpoint checks live in vlad_graphs (which builds on this module); their public names stay importable
# from here.
_VLAD_GRAPHS = ("GridDistillGraph", "GridEvalGraph", "NeXtVladDistillGraph", "NetVladDistillGraph", "NeXtVladEvalGraph", "NetVladEvalGraph",
                "check_vlad_checkpoint", "check_nextvlad_checkpoint", "check_netvlad_checkpoint", "netvlad_checkpoint_gating")


def __getattr__(name):
    if name in _VLAD_GRAPHS:
        from . import vlad_graphs
        return getattr(vlad_graphs, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
