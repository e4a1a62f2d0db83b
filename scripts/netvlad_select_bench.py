"""NetVLAD grid towers on selected frames (--student_sampling): evc_frames_gather_packed_tab on a table that names the
grid's frames against evc_frames_gather_packed on the same rows (alternating windows, either order) at every_n = 10 and 30; the training
step under last / random / segment_change next to the grid step at the same every_n; the distillation step under last next to the grid's.
One MI355X, one stream, uint8 input.  Nothing is asserted on these numbers.

    timeout -k 10 900 python scripts/netvlad_select_bench.py [--out profiles/netvlad_select_bench.txt] [--steps 30] [--rounds 3]

B = 256, F = 1152, K = 64, H = 1024, 4716 classes, n_b ~ U{120..300} - the configuration and the method of scripts/netvlad_grid_bench.py /
netvlad_distill_bench.py: `--warmup` untimed calls first, then `--rounds` windows of `--steps` calls on the same batch, HIP events around
every call, the host never waits inside a window; the figure is the median of the window medians, printed next to each window's median
and their spread.  An A / B pair alternates its windows (A B A B A B), and is run again in the other order.

The grid step against another commit: `--sections step --words uniform --package_root CHECKOUT` imports the package (and the library
built next to it) from CHECKOUT and times the grid step alone.  The last section of profiles/netvlad_select_bench.txt holds the `step,`
rows of four such runs in one session - a checkout of the parent commit, this tree, the parent, this tree - appended to the full run.
"""
import argparse
import gc
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
V, T = 4716, 300


def window(call, steps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record()
    for i in range(steps):
        call()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in zip(ev[:-1], ev[1:]))
    return ms[len(ms) // 2]


def summary(medians):
    s = sorted(medians)
    return dict(median=s[len(s) // 2], rounds=medians, spread=s[-1] - s[0])


def time_calls(call, warmup, steps, rounds):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    return summary([window(call, steps) for _ in range(rounds)])


def time_pair(first, second, warmup, steps, rounds):
    """Alternating windows first, second, first, second, ...: (summary of first, summary of second)."""
    for _ in range(warmup):
        first()
        second()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(rounds):
        a.append(window(first, steps))
        b.append(window(second, steps))
    return summary(a), summary(b)


def row(name, rows, peak, r):
    return "%-58s %7s %8s %9.3f %8.3f   %s" % (name, rows if rows else "-", "%.0f" % peak if peak else "-", r["median"], r["spread"],
                                               " ".join("%.3f" % m for m in r["rounds"]))


def fresh():
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "netvlad_select_bench.txt"))
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sections", default="gather,step,distill", help="which of gather,step,distill to run")
    ap.add_argument("--words", default="uniform,last,random,segment_change", help="the words of the step section")
    ap.add_argument("--package_root", default=ROOT,
                    help="import the package from this checkout (with --sections step --words uniform: the grid step of another commit, "
                         "for an A / B between two processes)")
    args = ap.parse_args()
    sections, words = args.sections.split(","), args.words.split(",")
    sys.path.insert(0, os.path.abspath(args.package_root))
    from efficientvideoclassification_youtube8m_amd import ops
    from efficientvideoclassification_youtube8m_amd.distill import NetVladDistillGraph, SingleTowerGraph
    from efficientvideoclassification_youtube8m_amd.towers import NetVladTower
    ops.check_device(0)
    B, F, K, H = 256, 1152, 64, 1024
    w = (args.warmup, args.steps, args.rounds)
    import efficientvideoclassification_youtube8m_amd as pkg
    gen =torch.Generator(device=DEV)
    gen.manual_seed(0)
    x = torch.randint(0, 256, (B, T, F), generator=gen, device=DEV, dtype=torch.uint8)
    n = torch.randint(120, T + 1, (B,), generator=gen, device=DEV, dtype=torch.int32)
    y = (torch.rand((B, V), generator=gen, device=DEV) < 3.0 / V).to(torch.uint8)
    n_host = n.cpu().numpy()
    head = "%-58s %7s %8s %9s %8s   %s" % ("", "rows", "peak MB", "median ms", "spread", "median of each window")
    lines = ["NetVLAD grid towers on selected frames on one MI355X, one stream, uint8 input [%d, %d, %d], %d classes (scripts/netvlad_select_bench.py)"
             % (B, T, F, V),
             "B = %d, F = %d, K = %d, H = %d, n_b ~ U{120..300} (mean %.1f); EVC_DETERMINISTIC %s"
             % (B, F, K, H, float(n_host.mean()), "on" if ops.DETERMINISTIC else "off"),
             "every figure: %d warm-up calls, then %d windows of %d calls, HIP events around every call; median ms = the median of the "
             "window medians, spread = largest - smallest window median" % (args.warmup, args.rounds, args.steps),
             "package: %s" % os.path.relpath(os.path.dirname(os.path.abspath(pkg.__file__)), ROOT), ""]
    kw = dict(cluster_size=K, hidden_size=H, device=DEV)

    def say(line):
        lines.append(line)
        print(line, flush=True)

    # 1. the gather through a table that names the grid's frames against the grid gather, on the same rows
    say("evc_frames_gather_packed_tab on a table holding j * every_n (stride ceil(T / every_n)) against evc_frames_gather_packed on the same "
        "rows, f32 + bf16 outputs, normalisation on, alternating windows")
    say(head)
    for every_n in (10, 30) if "gather" in sections else ():
        fresh()
        plan = ops.GridPlan(n_host, every_n, T)
        R, Rp = plan.R, plan.Rp
        S = -(-T // every_n)
        src = np.full((B, S), -1, np.int32)
        for b in range(B):
            src[b, :plan.k[b]] = np.arange(plan.k[b]) * every_n
        srcd, off = torch.from_numpy(src).to(DEV), torch.from_numpy(plan.row_off).to(DEV)
        out = torch.empty((Rp, F), device=DEV)
        out_bf = torch.empty((Rp, F), dtype=torch.bfloat16, device=DEV)

        def grid():
            ops.frames_gather_packed(x, n, off, every_n, R, Rp, out, out_bf, normalize=True)

        def tab():
            ops.frames_gather_packed_tab(x, n, off, srcd, R, Rp, out, out_bf, normalize=True)

        for order in ("grid first", "tab first"):
            a, b = time_pair(grid, tab, *w) if order == "grid first" else time_pair(tab, grid, *w)[::-1]
            say(row("evc_frames_gather_packed, every_n = %d (%s)" % (every_n, order), R, 0, a))
            say(row("evc_frames_gather_packed_tab, every_n = %d (%s)" % (every_n, order), R, 0, b))

    # 2. the training step: the grid against the words
    say("")
    say("the training step (SingleTowerGraph.step) on the grid (--student_sampling uniform: the launches of DESIGN.md 7.18) and under a word")
    say(head)
    for every_n in (10, 30) if "step" in sections else ():
        for word in words:
            fresh()
            skw = {} if word == "uniform" else dict(sampling=word)         # (uniform: the constructor call of a commit without the words)
            tw = NetVladTower(B, T, F, V, frames="grid", every_n=every_n, **skw, **kw)
            graph = SingleTowerGraph(tw)
            s = time_calls(lambda: graph.step(x, y, n, num_frames_host=n_host), *w)
            say(row("step, every_n = %d, %s" % (every_n, word), tw.R, torch.cuda.max_memory_allocated() / 1e6, s))
            del graph, tw

    # 3. the distillation step: teacher on every real frame, the student on the grid and on "last"
    say("")
    say("the distillation step (NetVladDistillGraph.step, teacher every_n = 1) with the student on the grid (DESIGN.md 7.19) and on last")
    say(head)
    for every_n in (10, 30) if "distill" in sections else ():
        for word in ("uniform", "last"):
            fresh()
            skw = {} if word == "uniform" else dict(student_sampling=word)
            g = NetVladDistillGraph(B, every_n=every_n, teacher_every_n=1, feature_size=F, vocab_size=V, max_frames=T, cluster_size=K, hidden_size=H,
                                    device=DEV, **skw)
            d = time_calls(lambda: g.step(x, y, n, num_frames_host=n_host), *w)
            say(row("distillation step, every_n = %d, %s" % (every_n, word), g.teacher.R + g.student.R, torch.cuda.max_memory_allocated() / 1e6, d))
            del g
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
