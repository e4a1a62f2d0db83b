"""What --student_sampling costs a training step on one MI355X: the step under `uniform` (the existing input pass) against the step under
`first` and under `random` (selection table + gathering pass), in one process on one box.

Two graphs at real dimensions (300 x 1152 f32 frames, n ~ U{120..300}, H = 1024, 2 layers, 4716 classes, bf16): BASELINE cfg 5 (student
only, every_n = 30, B = 1024) and the headline graph (teacher + student, every_n = 10, B = 256).  Per graph the three steps are warmed
up and then timed alternately, `--windows` windows of `--steps` steps each between two device events; reported: median of the windows
with min and max, and the ratio to the `uniform` step of the same run.  Then the two new launches on their own, at the shapes of that
graph (device events around `--reps` back-to-back launches), next to the existing student-only input pass.  One JSON line per graph.

    python scripts/frame_select_bench.py [--steps 10] [--windows 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from efficientvideoclassification_youtube8m_amd import ops  # noqa: E402
from efficientvideoclassification_youtube8m_amd.distill import DistillGraph  # noqa: E402

T, F, V = 300, 1152, 4716
WORDS = ("uniform", "first", "random")


def inputs(B, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    q = torch.randint(0, 256, (B, T, F), generator=g, device=dev, dtype=torch.uint8)
    n = torch.randint(120, T + 1, (B,), generator=g, device=dev, dtype=torch.int32)
    x = q.float() * (4.0 / 255.0) + (4.0 / 512.0 - 2.0)
    x[torch.arange(T, device=dev)[None, :] >= n[:, None]] = 0.0
    labels = torch.zeros((B, V), dtype=torch.uint8, device=dev)
    labels.scatter_(1, torch.randint(0, V, (B, 3), generator=g, device=dev), 1)
    return x.contiguous(), labels, n, n.cpu().numpy()


def stats(v, digits=4):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def timed(fn, reps):
    """Milliseconds per call of `reps` back-to-back calls between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run_config(name, mode, every_n, B, steps, windows, warmup, reps, dev):
    x, labels, n, nh = inputs(B, dev, 17)
    graphs = {w: DistillGraph(B, every_n=every_n, mode=mode, device=dev, seed=7, student_sampling=w, sampling_seed=1) for w in WORDS}
    for g in graphs.values():
        for _ in range(warmup):
            g.step(x, labels, n, num_frames_host=nh)
    ms = {w: [] for w in WORDS}
    for _ in range(windows):
        for w in WORDS:                                   # alternating: every window times all three on the same box state
            g = graphs[w]
            ms[w].append(timed(lambda: g.step(x, labels, n, num_frames_host=nh), steps))
    for g in graphs.values():
        g.flush()
    C2, S = 5, T // every_n
    src = ops.student_frame_select(n, T, every_n, "random", seed=1)
    launches = {
        "table_first_ms": [timed(lambda: ops.student_frame_select(n, T, every_n, "first"), reps) for _ in range(windows)],
        "table_random_ms": [timed(lambda: ops.student_frame_select(n, T, every_n, "random", seed=1), reps) for _ in range(windows)],
        "gather_pass_ms": [timed(lambda: ops.l2norm_chunk_sel(x, src, every_n, C2), reps) for _ in range(windows)],
        "existing_student_only_pass_ms": [timed(lambda: ops.l2norm_chunk(x, 20, every_n, C2, teacher_view=False), reps) for _ in range(windows)],
    }
    med = {w: statistics.median(ms[w]) for w in WORDS}
    return {"what": "frame_select_step", "config": name, "mode": mode, "every_n": every_n, "batch": B, "student_frames": S, "precision": "bf16",
            "input": "f32", "steps": steps, "windows": windows, "warmup": warmup,
            "ms_per_step": {w: stats(ms[w]) for w in WORDS},
            "over_uniform_median": {w: round(med[w] / med["uniform"], 4) for w in WORDS if w != "uniform"},
            "extra_ms_median": {w: round(med[w] - med["uniform"], 4) for w in WORDS if w != "uniform"},
            "launches": dict({k: stats(v, 5) for k, v in launches.items()}, reps=reps,
                             note="the allocation of the output tensors is inside the timed call, as in the step")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    if a.windows < 3:
        ap.error("--windows: at least 3 (the spread is part of the result)")
    dev = "cuda:0"
    torch.cuda.set_device(0)
    ops.check_device(0)
    for name, mode, every_n, B in (("cfg5_student_only_every_n30_b1024", "student", 30, 1024), ("headline_cfg3_b256", "teacher_student", 10, 256)):
        print(json.dumps(run_config(name, mode, every_n, B, a.steps, a.windows, a.warmup, a.reps, dev)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
