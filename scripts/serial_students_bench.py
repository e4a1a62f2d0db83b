"""K students against one teacher forward (SerialStudentsGraph) against K runs of the single-student serial step, on one MI355X,
bf16 forward on uint8 frames:

  * ms/step (mean, median, max - as bench.py reports them: HIP events on the caller's stream after every step) and
    torch.cuda.max_memory_allocated of DistillGraph mode "serial" (the yardstick: K students one after another cost K times
    this), mode "student", and SerialStudentsGraph with K = 1, 2, 3 students of the same every_n, at (B, every_n) = (1024, 30) and
    (256, 10); same inputs, same process, one after the other;
  * the loss section alone on one stream: evc_distill_losses_multi at K = 3 against 3 x evc_distill_losses, B = 256 and 1024.

    python scripts/serial_students_bench.py [--out profiles/serial_students_bench.txt] [--steps 20] [--warmup 3]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import StepClock, step_stats, synthetic_inputs      # noqa: E402  (the benchmark's own inputs and statistics)

T, F, V = 300, 1152, 4716
DEV = "cuda:0"


def time_graph(make, steps, warmup, pool_in, n_host):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()               # the resident input pool: the same for every graph
    g = make()
    pool = len(pool_in)
    for i in range(pool):                              # settle: every batch of the pool once (first uses of kernel instantiations)
        g.step(pool_in[i][0], pool_in[i][2], pool_in[i][1], num_frames_host=n_host[i])
    torch.cuda.synchronize()
    it = 0
    for _ in range(warmup):
        g.step(pool_in[it % pool][0], pool_in[it % pool][2], pool_in[it % pool][1], num_frames_host=n_host[it % pool])
        it += 1
    torch.cuda.synchronize()
    clock = StepClock()
    clock.tick()
    for _ in range(steps):
        g.step(pool_in[it % pool][0], pool_in[it % pool][2], pool_in[it % pool][1], num_frames_host=n_host[it % pool])
        it += 1
        clock.tick()
    g.flush()
    clock.close()
    torch.cuda.synchronize()
    per = clock.per_step_ms()
    st = step_stats(per, span_ms_per_step=clock.span_ms() / steps)
    rep = g.loss_report()
    rep = rep if isinstance(rep, list) else [rep]
    res = dict(mean=clock.span_ms() / steps, median=st["ms_per_step_median"], max=st["ms_per_step_max"], stall=st["stall_suspected"],
               peak_mib=(torch.cuda.max_memory_allocated() - base) / 2.0 ** 20, finite=all(np.isfinite(v) for r in rep for v in r.values()))
    del g
    torch.cuda.empty_cache()
    return res


def time_losses(B, D, reps, K=3):
    from efficientvideoclassification_youtube8m_amd import ops
    gen = torch.Generator(device=DEV)
    gen.manual_seed(B)
    pt = torch.rand((B, V), generator=gen, device=DEV) * (1 - 2e-6) + 1e-6
    pss = [torch.rand((B, V), generator=gen, device=DEV) * (1 - 2e-6) + 1e-6 for _ in range(K)]
    y = (torch.rand((B, V), generator=gen, device=DEV) < 0.001).to(torch.uint8)
    st = torch.randn((B, D), generator=gen, device=DEV)
    sss = [torch.randn((B, D), generator=gen, device=DEV) for _ in range(K)]
    rt, rss = pt.sum(1), [p.sum(1) for p in pss]
    losses = torch.zeros((K, 4), dtype=torch.float32, device=DEV)
    dps, dss = [torch.empty_like(p) for p in pss], [torch.empty_like(s) for s in sss]

    def multi():
        ops.distill_losses_multi(pt, rt, y, st, pss, rss, sss, losses, dps, dss, g_ce=1.0 / B, g_kl=1.0, g_rep=2.0)

    def singles():
        for k in range(K):
            ops.distill_losses(pt, rt, pss[k], rss[k], y, st, sss[k], losses[k], dps[k], dss[k], g_ce=1.0 / B, g_kl=1.0, g_rep=2.0)

    out = {}
    for name, fn in (("multi", multi), ("singles", singles)):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        ev[0].record()
        for i in range(reps):
            fn()
            ev[i + 1].record()
        torch.cuda.synchronize()
        us = sorted(1e3 * a.elapsed_time(b) for a, b in zip(ev[:-1], ev[1:]))
        out[name] = dict(mean=1e3 * ev[0].elapsed_time(ev[-1]) / reps, median=us[len(us) // 2], max=us[-1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "serial_students_bench.txt"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pool", type=int, default=4)
    ap.add_argument("--only", default="", help="B,every_n,K: that SerialStudentsGraph alone, no table (for a kernel trace)")
    args = ap.parse_args()
    from efficientvideoclassification_youtube8m_amd import ops
    from efficientvideoclassification_youtube8m_amd.distill import DistillGraph, SerialStudentsGraph
    ops.check_device(0)
    if args.only:
        B, every_n, K = (int(v) for v in args.only.split(","))
        pool_in = [synthetic_inputs(B, T, F, V, 1234 + 1000 * i, DEV, False, as_uint8=True) for i in range(args.pool)]
        n_host = [p[1].cpu().numpy() for p in pool_in]
        r = time_graph(lambda: SerialStudentsGraph(B, every_n=(every_n,) * K, device=DEV, seed=7), args.steps, args.warmup, pool_in, n_host)
        print("B %d every_n %d K %d: median %.3f ms" % (B, every_n, K, r["median"]))
        return
    lines = ["K students against ONE forward of the frozen teacher per batch (SerialStudentsGraph, K students of the same every_n) against the",
             "single-student serial step (DistillGraph mode 'serial', the yardstick: K students one after another cost K x its step) and the",
             "student alone ('student'); one MI355X, bf16 forward, uint8 frames resident in HBM, %d timed steps after %d warm-up steps," %
             (args.steps, args.warmup),
             "HIP events after every step (scripts/serial_students_bench.py); EVC_DETERMINISTIC %s" % ("on" if ops.DETERMINISTIC else "off"),
             "peak MiB = torch.cuda.max_memory_allocated over construction + all steps, without the resident input pool",
             "vs K x serial = median / (K x the serial step's median): below 1.00 the shared forward pays", ""]
    lines.append("%-6s %-8s %-22s %10s %10s %10s %10s %14s" % ("B", "every_n", "graph", "mean ms", "median ms", "max ms", "peak MiB", "vs K x serial"))
    verdicts = []
    for B, every_n in ((1024, 30), (256, 10)):
        pool_in = [synthetic_inputs(B, T, F, V, 1234 + 1000 * i, DEV, False, as_uint8=True) for i in range(args.pool)]
        n_host = [p[1].cpu().numpy() for p in pool_in]
        rows = [("serial", 1, lambda: DistillGraph(B, every_n=every_n, mode="serial", device=DEV, seed=7)),
                ("student", 0, lambda: DistillGraph(B, every_n=every_n, mode="student", device=DEV, seed=7))]
        for K in (1, 2, 3):
            rows.append(("serial students K=%d" % K, K, (lambda K=K: SerialStudentsGraph(B, every_n=(every_n,) * K, device=DEV, seed=7))))
        serial = None
        for name, K, make in rows:
            r = time_graph(make, args.steps, args.warmup, pool_in, n_host)
            assert r["finite"], (B, every_n, name)
            if name == "serial":
                serial = r["median"]
            ratio = "%13.2fx" % (r["median"] / (K * serial)) if K else "%14s" % "-"
            lines.append("%-6d %-8d %-22s %10.3f %10.3f %10.3f %10.0f %s%s" % (
                B, every_n, name, r["mean"], r["median"], r["max"], r["peak_mib"], ratio,
                "  (a step > 3 x the median or a gap behind the window: read the median)" if r["stall"] else ""))
            print(lines[-1], flush=True)
            if K == 3:
                verdicts.append("(%d, %d): K = 3 step %.3f ms against 3 x %.3f = %.3f ms: %s" % (
                    B, every_n, r["median"], serial, 3 * serial, "BELOW (accepted)" if r["median"] < 3 * serial else "NOT below"))
        del pool_in
        torch.cuda.empty_cache()
    lines += ["", "acceptance (K = 3 step below 3 x the single serial step, medians):"] + verdicts
    lines += ["", "the loss section alone, one stream, V = %d, D = 4096, %d calls each; us per call (every dpred_s and dstate_s written):" % (V, 200),
              "%-6s %-52s %10s %10s %10s" % ("B", "launches", "mean us", "median us", "max us")]
    for B in (256, 1024):
        r = time_losses(B, 4096, 200)
        for name, what in (("singles", "3 x (evc_distill_losses + its finish launch)"), ("multi", "evc_distill_losses_multi, K = 3, + its finish launch")):
            lines.append("%-6d %-52s %10.1f %10.1f %10.1f" % (B, what, r[name]["mean"], r[name]["median"], r[name]["max"]))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
