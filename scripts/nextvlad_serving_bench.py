"""Serving the NeXtVLAD family (distill.NeXtVladEvalGraph) on one MI355X, one stream, uint8 input.

    python scripts/nextvlad_serving_bench.py [--out profiles/nextvlad_serving_bench.txt] [--reps 20] [--batches 256,1024]

Configuration of DESIGN.md 7.13: F = 1152, expansion 2, G = 8, K = 128, H = 2048, gating reduction 8, 4716 classes, n_b ~ U{120..300},
random weights (GAP on synthetic data means nothing: only throughput is reported).  Method of DESIGN.md 7.14: HIP events around every
call, 10 warm-up calls, then 3 windows; the figure of a line is the median of the three window medians, the windows' own medians are
printed next to it (their spread is the run-to-run noise).  Nothing is gated on these numbers.

(a) one served tower, videos/s, every_n = 1 / 10 / 30;
(b) validate's two-tower step (student at every_n = 10 served, teacher at every_n = 1 run too);
(c) a student (every_n = 30) -> teacher (every_n = 1) cascade with exactly 10 / 30 / 50 % of the batch escalated (--cascade_fractions
    alone: the least confident rows), with compact on and off, next to the teacher alone on the whole batch; "stage 2" is the time
    between CascadeGraph's marks stage1 and gate1 (the escalated rows' teacher step).  The keep rule of the compaction: stage 2 with
    compact on must be faster than with compact off by more than the spread of the window medians, at 10 % and at 30 %.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
V, T = 4716, 300
WARMUP, WINDOWS = 10, 3


def median(v):
    s = sorted(v)
    return s[len(s) // 2]


def windows(fn, reps, inner=None):
    """Medians (ms) of WINDOWS windows of ``reps`` calls of fn after WARMUP untimed ones.  inner: a callable returning the (start, end)
    events of a part of the call just made; then (whole-call medians, part medians)."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    whole, part = [], []
    for _ in range(WINDOWS):
        ev, pe = [], []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            ev.append((a, b))
            if inner is not None:
                pe.append(inner())
        torch.cuda.synchronize()
        whole.append(median([a.elapsed_time(b) for a, b in ev]))
        if inner is not None:
            part.append(median([a.elapsed_time(b) for a, b in pe]))
    return (whole, part) if inner is not None else whole


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nextvlad_serving_bench.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="256,1024")
    args = ap.parse_args()
    from efficientvideoclassification_youtube8m_amd import ops
    from efficientvideoclassification_youtube8m_amd.cascade import CascadeGraph
    from efficientvideoclassification_youtube8m_amd.distill import NeXtVladEvalGraph
    ops.check_device(0)
    F, lam, G, K, H, rho = 1152, 2, 8, 128, 2048, 8
    sizes = dict(cluster_size=K, hidden_size=H, groups=G, expansion=lam, gating_reduction=rho)
    shared = dict(feature_size=F, vocab_size=V, max_frames=T, num_mixtures=2, device=DEV, precision="bf16")
    lines = ["Serving the NeXtVLAD family on one MI355X, one stream, uint8 input [B, %d, %d], %d classes (scripts/nextvlad_serving_bench.py)" % (T, F, V),
             "F = %d, expansion %d, G = %d, K = %d, H = %d, gating reduction %d, n_b ~ U{120..300}, random weights; EVC_DETERMINISTIC %s"
             % (F, lam, G, K, H, rho, "on" if ops.DETERMINISTIC else "off"),
             "HIP events around every call, %d warm-up calls, then %d windows of %d; ms = median of the window medians [each window's median]"
             % (WARMUP, WINDOWS, args.reps),
             "GAP / mAP on synthetic data mean nothing: throughput only.", ""]

    def line(text):
        lines.append(text)
        print(text, flush=True)

    fmt = lambda m: "%9.3f   [%s]" % (median(m), " ".join("%.3f" % v for v in m))
    verdicts = []
    for B in [int(b) for b in args.batches.split(",")]:
        gen = torch.Generator(device=DEV)
        gen.manual_seed(B)
        x = torch.randint(0, 256, (B, T, F), generator=gen, device=DEV, dtype=torch.uint8)
        n = torch.randint(120, T + 1, (B,), generator=gen, device=DEV, dtype=torch.int32)
        y = (torch.rand((B, V), generator=gen, device=DEV) < 3.0 / V).to(torch.uint8)
        nh = n.cpu().numpy()
        line("B = %d" % B)
        line("(a) one served tower: NeXtVladEvalGraph(tower='teacher').step")
        line("%-58s %9s" % ("", "ms"))
        alone = None
        for every_n in (1, 10, 30):
            g = NeXtVladEvalGraph(B, tower="teacher", every_n=every_n, **shared, **sizes)
            m = windows(lambda: g.step(x, y, n, num_frames_host=nh), args.reps)
            line("%-58s %s   %9.0f videos/s" % ("every_n = %d (R = %d)" % (every_n, g.teacher.R), fmt(m), B / median(m) * 1e3))
            if every_n == 1:
                alone = m
            del g
        line("(b) validate's two-tower step: NeXtVladEvalGraph(tower='both'), student every_n = 10 served, teacher every_n = 1")
        g = NeXtVladEvalGraph(B, tower="both", every_n=10, teacher_every_n=1, **shared, **sizes)
        m = windows(lambda: g.step(x, y, n, num_frames_host=nh), args.reps)
        line("%-58s %s   %9.0f videos/s" % ("two towers + label loss + rep loss", fmt(m), B / median(m) * 1e3))
        del g
        line("(c) cascade student (every_n = 30) -> teacher (every_n = 1); the teacher alone on the whole batch: %.3f ms" % median(alone))
        line("%-34s %-36s %s" % ("escalated, compact", "whole step ms", "stage 2 ms"))
        for frac in (0.1, 0.3, 0.5):
            stage2 = {}
            for compact in (True, False):
                torch.cuda.empty_cache()
                stages = [("student", 30, "uniform", dict(sizes, compact=compact)), ("teacher", 1, "uniform", dict(sizes, compact=compact))]
                c = CascadeGraph(B, stages, confidence="top1", fractions=[frac], **shared)
                c.marks = []

                def step():
                    del c.marks[:]
                    return c.step(x, y, n, num_frames_host=nh)

                def part():
                    ev = dict(c.marks)
                    return ev["stage1"], ev["gate1"]

                rows = step()["stage_rows"]
                whole, s2 = windows(step, args.reps, part)
                stage2[compact] = s2
                line("%-34s %-36s %s" % ("%2.0f %% (%d of %d rows), compact %s" % (100 * frac, rows[1], B, "on " if compact else "off"),
                                         fmt(whole).strip(), fmt(s2).strip()))
                del c
            on, off = stage2[True], stage2[False]
            faster = max(on) < min(off)
            verdicts.append((B, frac, faster))
            line("   stage 2 at %2.0f %%: compact on %.3f .. %.3f ms, off %.3f .. %.3f ms -> compact is %s beyond the spread of the window medians"
                 % (100 * frac, min(on), max(on), min(off), max(off), "FASTER" if faster else "NOT faster"))
        line("")
        del x, n, y
    keep = all(f for _, frac, f in verdicts if frac in (0.1, 0.3))
    line("keep rule (stage 2 faster beyond the spread at 10 %% and at 30 %%, every batch size above): %s" % ("KEEP the compaction" if keep else "NOT met"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
