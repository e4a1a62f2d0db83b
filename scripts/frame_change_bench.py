"""What --student_sampling change / segment_change cost on one MI355X: the two new launches alone (score pass, scored table) for uint8 and
f32 frames, and the training step under `uniform`, `random`, `change` and `segment_change`, in one process on one box.

Launches: evc_frame_change_keys at (B, T, F) = (256, 300, 1152) and (1024, 300, 1152) with n ~ U{120..300}; `--reps` back-to-back calls between
two device events, `--windows` windows, median [min - max]; the bytes the pass has to move (the live frames once, plus the keys) and the
achieved TB/s.  The input is larger than it would be in a step's L2 but not larger than the 256 MiB Infinity Cache for the uint8 shapes (88 /
354 MB) and the small f32 one, so the back-to-back figure may be served from that cache: a second figure rotates over enough distinct input
buffers that their total exceeds 1 GiB (each call then reads bytes that left every cache).
Steps: the graphs of scripts/frame_select_bench.py (BASELINE cfg 5: student only, every_n = 30, B = 1024; the headline: teacher + student,
every_n = 10, B = 256; bf16, f32 frames), the four steps warmed up and then timed alternately.  One JSON line per record.

    python scripts/frame_change_bench.py [--steps 10] [--windows 5] [--what launches,steps]
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
WORDS = ("uniform", "random", "change", "segment_change")
STREAM_TBS = 6.0          # the streaming rate the kernel guides give for one MI355X (HBM, reads)


def inputs(B, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    q = torch.randint(0, 256, (B, T, F), generator=g, device=dev, dtype=torch.uint8)
    n = torch.randint(120, T + 1, (B,), generator=g, device=dev, dtype=torch.int32)
    labels = torch.zeros((B, V), dtype=torch.uint8, device=dev)
    labels.scatter_(1, torch.randint(0, V, (B, 3), generator=g, device=dev), 1)
    return q, labels, n, n.cpu().numpy()


def dequantized(q, n):
    x = q.float() * (4.0 / 255.0) + (4.0 / 512.0 - 2.0)
    x[torch.arange(T, device=q.device)[None, :] >= n[:, None]] = 0.0
    return x.contiguous()


def stats(v, digits=4):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def timed(fn, reps):
    """Milliseconds per call of `reps` back-to-back calls between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run_launches(B, dev, windows, reps):
    q, _, n, nh = inputs(B, dev, 17)
    live = int(nh.clip(0, T).sum())
    for name, x in (("uint8", q), ("f32", dequantized(q, n))):
        esz = x.element_size()
        moved = live * F * esz + B * T * 4                                   # the live frames once + the keys
        copies = [x] + [x.clone() for _ in range(max(1, -(-(1 << 30) // (x.numel() * esz))))]          # > 1 GiB in all
        keys = ops.frame_change_keys(x, n)
        for _ in range(3):
            ops.frame_change_keys(x, n)
        same = [timed(lambda i: ops.frame_change_keys(x, n), reps) for _ in range(windows)]
        rot = [timed(lambda i: ops.frame_change_keys(copies[i % len(copies)], n), reps) for _ in range(windows)]
        tables = {}
        for every_n in (10, 30):
            for w in ("change", "segment_change"):
                tables["%s_every_n%d_ms" % (w, every_n)] = stats(
                    [timed(lambda i: ops.student_frame_select_scored(n, keys, T, every_n, w), reps) for _ in range(windows)], 5)
            tables["random_every_n%d_ms" % every_n] = stats(
                [timed(lambda i: ops.student_frame_select(n, T, every_n, "random", seed=1), reps) for _ in range(windows)], 5)
        ms_same, ms_rot = statistics.median(same), statistics.median(rot)
        print(json.dumps({"what": "frame_change_launches", "batch": B, "frames": name, "live_frames": live, "bytes_moved": moved,
                          "keys_same_buffer_ms": stats(same, 5), "keys_rotating_buffers_ms": stats(rot, 5), "buffers": len(copies),
                          "tb_per_s_same_buffer": round(moved / ms_same / 1e9, 3), "tb_per_s_rotating": round(moved / ms_rot / 1e9, 3),
                          "guide_streaming_tb_per_s": STREAM_TBS, "floor_ms_at_guide_rate": round(moved / STREAM_TBS / 1e9, 5),
                          "tables": tables, "reps": reps, "windows": windows,
                          "note": "the allocation of the output tensor is inside the timed call, as in the step"}), flush=True)
        del copies
        torch.cuda.empty_cache()


def run_steps(name, mode, every_n, B, steps, windows, warmup, dev):
    q, labels, n, nh = inputs(B, dev, 17)
    x = dequantized(q, n)
    del q
    graphs = {w: DistillGraph(B, every_n=every_n, mode=mode, device=dev, seed=7, student_sampling=w, sampling_seed=1) for w in WORDS}
    for g in graphs.values():
        for _ in range(warmup):
            g.step(x, labels, n, num_frames_host=nh)
    ms = {w: [] for w in WORDS}
    for _ in range(windows):
        for w in WORDS:                                   # alternating: every window times all four on the same box state
            g = graphs[w]
            ms[w].append(timed(lambda i: g.step(x, labels, n, num_frames_host=nh), steps))
    for g in graphs.values():
        g.flush()
    med = {w: statistics.median(ms[w]) for w in WORDS}
    print(json.dumps({"what": "frame_change_step", "config": name, "mode": mode, "every_n": every_n, "batch": B, "student_frames": T // every_n,
                      "precision": "bf16", "input": "f32", "steps": steps, "windows": windows, "warmup": warmup,
                      "ms_per_step": {w: stats(ms[w]) for w in WORDS},
                      "over_uniform_median": {w: round(med[w] / med["uniform"], 4) for w in WORDS if w != "uniform"},
                      "extra_ms_median": {w: round(med[w] - med["uniform"], 4) for w in WORDS if w != "uniform"}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--what", default="launches,steps")
    a = ap.parse_args()
    if a.windows < 3:
        ap.error("--windows: at least 3 (the spread is part of the result)")
    dev = "cuda:0"
    torch.cuda.set_device(0)
    ops.check_device(0)
    what = a.what.split(",")
    if "launches" in what:
        for B in (256, 1024):
            run_launches(B, dev, a.windows, a.reps)
    if "steps" in what:
        for name, mode, every_n, B in (("cfg5_student_only_every_n30_b1024", "student", 30, 1024), ("headline_cfg3_b256", "teacher_student", 10, 256)):
            run_steps(name, mode, every_n, B, a.steps, a.windows, a.warmup, dev)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
