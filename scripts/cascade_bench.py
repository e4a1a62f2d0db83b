"""A two-stage confidence cascade (cascade.CascadeGraph: student at every_n = 30, then the teacher) against each tower alone, on one MI355X.

Synthetic uint8 frames (n ~ U{120..300}, 1152 features, 4716 classes, H = 1024, 2 layers), --precision bf16, randomly initialised towers,
B = 256 and B = 1024, pure fraction mode at f = 0, 0.1, 0.3, 0.5 and 1: exactly ceil(f B) videos escalate whatever the towers predict, so
the figures do not depend on what a trained model would be sure of.  THIS MEASURES THROUGHPUT ONLY: what a cascade is worth in GAP
cannot be measured here, because the data is synthetic.

Per setting one batch is stepped ``--calls`` times per window, ``--windows`` windows (at least 20); the window's time is a host clock around
the calls ending in a device synchronise, the figure the median over the windows (min and max beside it).  The split of a batch comes from
device events recorded by the graph around every stage and gate (median over all calls):
  stage0_ms  the student's step;  gate_ms  ops.cascade_confidence_rows + ops.cascade_pick_rows + the two copies to pinned memory;
  idle_ms    from the gate's end to the teacher's first launch: the device waits for the host (its wake-up, the gate's result, the row plan);
  stage1_ms  the teacher's step on the escalated rows + the last confidence launch;  host_wait_ms  the host's time inside the one wait.
The student alone and the teacher alone (the cascade's own two graphs, stepped directly, every row live) are timed in the same process,
their windows alternating with the cascade's, and so is ``teacher_rows_ms``: the teacher alone on a batch whose other rows have
num_frames = 0 (the FIRST ceil(f B) rows, ``teacher_rows_frames`` frames in all - the gate escalates other rows, whose frames are
``stage_frames[1]``), the t_teacher(rows = f B) of the model  t = t_student + t_gate + t_wait + t_teacher(rows = f B);  ``model_ms`` is that sum
with the measured parts (t_wait = idle_ms), ``measured_minus_model_ms`` what the model leaves out.  One JSON line per setting.

    python scripts/cascade_bench.py [--windows 20] [--calls 4] [--batches 256,1024]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from efficientvideoclassification_youtube8m_amd import ops  # noqa: E402
from efficientvideoclassification_youtube8m_amd.cascade import CascadeGraph  # noqa: E402
from efficientvideoclassification_youtube8m_amd.flags import FLAGS  # noqa: E402
from efficientvideoclassification_youtube8m_amd.train import synthetic_batches  # noqa: E402

FRACTIONS = (0.0, 0.1, 0.3, 0.5, 1.0)
EVERY_N = 30


def window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def stats(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def split(marks):
    """{segment: ms} of one step from the graph's (name, event) marks; the last mark ends the step."""
    names = {"stage0": "stage0_ms", "gate0": "gate_ms", "wait0": "idle_ms", "stage1": "stage1_ms", "gate1": "stage1_ms"}
    out = {}
    for (name, ev), (_, nxt) in zip(marks[:-1], marks[1:]):
        out[names[name]] = out.get(names[name], 0.0) + ev.elapsed_time(nxt)
    return out


def run_batch_size(B, windows, calls, dev):
    q, y, n, nh = next(synthetic_batches(B, 1152, dev, B, 1, 4321))
    base = CascadeGraph(B, [("student", EVERY_N), ("teacher", 1)], fractions=[0.0], device=dev, precision="bf16")
    student, teacher = base.graphs

    def cascade_at(f):
        """The same two graphs behind another fraction (no second set of towers on the device)."""
        base.fractions = [f]
        return base

    # the teacher alone on ceil(f B) live rows: the least confident rows of the student's gate are as good as any - take the first ones
    def masked_counts(f):
        m = min(B, int(math.ceil(f * B)))
        keep = np.arange(B) < m
        nh_m = np.where(keep, nh, 0)
        return torch.from_numpy(nh_m.astype(np.int32)).to(dev), nh_m

    sides = {"student_alone": lambda: student.step(q, y, n, num_frames_host=nh), "teacher_alone": lambda: teacher.step(q, y, n, num_frames_host=nh)}
    masked = {f: masked_counts(f) for f in FRACTIONS if 0.0 < f < 1.0}
    for f, (n_m, nh_m) in masked.items():
        sides["teacher_rows_%g" % f] = (lambda n_m=n_m, nh_m=nh_m: teacher.step(q, y, n_m, num_frames_host=nh_m))
    for f in FRACTIONS:
        sides["cascade_%g" % f] = (lambda f=f: cascade_at(f).step(q, y, n, num_frames_host=nh))
    for fn in sides.values():                                            # warm-up: code objects, allocator, every shape the windows use
        window(fn, 2)
    times = {k: [] for k in sides}
    for _ in range(windows):                                             # alternate all sides window by window
        for k, fn in sides.items():
            times[k].append(window(fn, calls))
    alone = {k: stats(v) for k, v in times.items() if not k.startswith("cascade_")}
    lines = [dict(what="towers_alone", batch=B, windows=windows, calls_per_window=calls,
                  **{k + "_ms": v for k, v in alone.items()},
                  student_alone_videos_per_s=round(B / alone["student_alone"]["median"] * 1e3, 1),
                  teacher_alone_videos_per_s=round(B / alone["teacher_alone"]["median"] * 1e3, 1))]
    for f in FRACTIONS:                                                  # the split: a run of its own, events on
        g = cascade_at(f)
        segs = {}
        host_wait, rows, frames = [], None, None
        for _ in range(max(10, calls)):
            g.marks = []
            out = g.step(q, y, n, num_frames_host=nh)
            end = torch.cuda.Event(enable_timing=True)
            end.record()
            end.synchronize()
            for k, v in split(g.marks + [("end", end)] if g.marks[-1][0] != "end" else g.marks).items():
                segs.setdefault(k, []).append(v)
            host_wait.append(out["gate_wait_s"] * 1e3)
            rows, frames = out["stage_rows"], out["stage_frames"]
        g.marks = None
        med = {k: round(statistics.median(v), 3) for k, v in segs.items()}
        t = stats(times["cascade_%g" % f])
        t_rows = 0.0 if f == 0.0 else (alone["teacher_alone"] if f == 1.0 else alone["teacher_rows_%g" % f])["median"]
        model = alone["student_alone"]["median"] + med.get("gate_ms", 0.0) + med.get("idle_ms", 0.0) + t_rows
        rows_frames = int(masked[f][1].sum()) if f in masked else (0 if f == 0.0 else int(nh.sum()))
        lines.append(dict(what="cascade", batch=B, fraction=f, stage_rows=rows, stage_frames=frames, teacher_rows_frames=rows_frames, ms_per_batch=t, videos_per_s=round(B / t["median"] * 1e3, 1),
                          split_ms=med, host_wait_ms=round(statistics.median(host_wait), 3), teacher_rows_ms=t_rows, model_ms=round(model, 3),
                          measured_minus_model_ms=round(t["median"] - model, 3),
                          over_teacher_alone=round(alone["teacher_alone"]["median"] / t["median"], 3)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--batches", default="256,1024")
    a = ap.parse_args()
    if a.windows < 20:
        ap.error("--windows: at least 20 (the figure is a median)")
    FLAGS.reset()
    dev = "cuda:0"
    torch.cuda.set_device(0)
    ops.check_device(0)
    print("# " + " ".join(["python", "scripts/cascade_bench.py"] + sys.argv[1:]) + " on one MI355X: student (every_n 30) -> teacher cascade in pure fraction "
          "mode against each tower alone, alternating in one process; host clock around synchronised windows, ms per batch, split by device events; "
          "random weights, 300 x 1152 uint8 frames, n ~ U{120..300}, H 1024, 2 layers, 4716 classes, bf16.  Throughput only: synthetic data says "
          "nothing about GAP", flush=True)
    for B in [int(b) for b in a.batches.split(",")]:
        for line in run_batch_size(B, a.windows, a.calls, dev):
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
