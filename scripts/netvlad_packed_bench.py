"""NetVLAD tower over packed ragged frames (--netvlad_frames grid): the two packed aggregation entries alone at
every_n = 1, the training step at every_n = 1 (every real frame: the teacher's input), 10 and 30 (the fewer-frames students') next to
the sampled mode at S = 30 in the same process, and the forward-only tower in videos / s.  One MI355X, one stream, uint8 input.  Nothing
is asserted on these numbers.

    timeout -k 10 900 python scripts/netvlad_packed_bench.py [--out profiles/netvlad_packed_bench.txt] [--steps 30] [--rounds 3]

B = 256, F = 1152, K = 64, H = 1024, 4716 classes, n_b ~ U{120..300}.  Every figure: `--warmup` untimed calls first, then `--rounds`
windows of `--steps` calls on the same batch, HIP events around every call, the host never waits inside a window; mean / median / max
over all timed calls and the median of each window (their spread is the run-to-run noise inside this process).  Training step =
SingleTowerGraph.step (forward, loss, backward, clip + Adam).  Rows = packed frame rows of the batch (R; the TN product runs on R
rounded up to 32); peak MB = torch.cuda.max_memory_allocated() over the configuration's life, the input batch included.
"""
import argparse
import gc
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
V, T = 4716, 300


def time_calls(call, warmup, steps, rounds):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    all_ms, medians = [], []
    for _ in range(rounds):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        ev[0].record()
        for i in range(steps):
            call()
            ev[i + 1].record()
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in zip(ev[:-1], ev[1:])]
        all_ms += ms
        medians.append(sorted(ms)[len(ms) // 2])
    s = sorted(all_ms)
    return dict(mean=sum(s) / len(s), median=s[len(s) // 2], max=s[-1], rounds=medians)


def row(name, rows, peak, r):
    return "%-30s %7d %8s %9.3f %9.3f %9.3f   %s" % (name, rows, "%.0f" % peak if peak else "-", r["mean"], r["median"], r["max"],
                                                    " ".join("%.3f" % m for m in r["rounds"]))


def fresh():
    gc.collect()                                     # (a tower and its batch-norms reference each other: the previous configuration's buffers)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "netvlad_packed_bench.txt"))
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    from efficientvideoclassification_youtube8m_amd import ops
    from efficientvideoclassification_youtube8m_amd.distill import SingleTowerGraph
    from efficientvideoclassification_youtube8m_amd.towers import NetVladTower
    ops.check_device(0)
    B, S, F, K, H = 256, 30, 1152, 64, 1024
    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    x = torch.randint(0, 256, (B, T, F), generator=gen, device=DEV, dtype=torch.uint8)
    n = torch.randint(120, T + 1, (B,), generator=gen, device=DEV, dtype=torch.int32)
    y = (torch.rand((B, V), generator=gen, device=DEV) < 3.0 / V).to(torch.uint8)
    n_host = n.cpu().numpy()
    head = "%-30s %7s %8s %9s %9s %9s   %s" % ("", "rows", "peak MB", "mean ms", "median ms", "max ms", "median of each window")
    lines = ["NetVLAD tower over packed ragged frames on one MI355X, one stream, uint8 input [%d, %d, %d], %d classes (scripts/netvlad_packed_bench.py)"
             % (B, T, F, V),
             "B = %d, F = %d, K = %d, H = %d, n_b ~ U{120..300} (mean %.1f); EVC_DETERMINISTIC %s"
             % (B, F, K, H, float(n_host.mean()), "on" if ops.DETERMINISTIC else "off"),
             "every figure: %d warm-up calls, then %d windows of %d calls, HIP events around every call" % (args.warmup, args.rounds, args.steps), ""]
    kw = dict(cluster_size=K, hidden_size=H, device=DEV)

    # the two packed entries alone, on the operands a training step at every_n = 1 leaves in the tower
    fresh()
    tw = NetVladTower(B, T, F, V, frames="grid", every_n=1, **kw)
    graph = SingleTowerGraph(tw)
    graph.step(x, y, n, num_frames_host=n_host)
    bi, st, R, mk = tw.bn_in, tw.store, tw.R, tw.plan.max_k
    stats = (bi.mean, bi.var, bi.gamma(), bi.beta())
    lines += ["the packed aggregation entries alone at every_n = 1 (R = %d rows, longest video %d)" % (R, mk), head]
    r = time_calls(lambda: ops.netvlad_aggregate_packed_fwd(tw.a, tw.r, tw.row_off, B, T, K, F, R, mk, *stats, st.p(tw.C2), tw.Vv, tw.asum),
                   args.warmup, args.steps, args.rounds)
    flop = 2.0 * R * K * F
    lines.append(row("evc_netvlad_aggregate_packed_fwd", R, 0, r) + "   (%.1f TFLOP/s f32)" % (flop / r["median"] / 1e9))
    print(lines[-1], flush=True)
    r = time_calls(lambda: ops.netvlad_aggregate_packed_bwd(tw.a, tw.r, tw.row_off, B, T, K, F, R, mk, *stats, st.p(tw.C2), tw.dV, tw.da, tw.dx,
                                                            ws=tw.agg_ws), args.warmup, args.steps, args.rounds)
    lines.append(row("evc_netvlad_aggregate_packed_bwd", R, 0, r) + "   (%.1f TFLOP/s f32)" % (2 * flop / r["median"] / 1e9))
    print(lines[-1], flush=True)
    del graph, tw, bi, st, stats

    lines += ["", "training step", head]
    for name, frames, every_n in (("grid --every_n 1", "grid", 1), ("grid --every_n 10", "grid", 10), ("grid --every_n 30", "grid", 30),
                                  ("sampled --iterations %d" % S, "sampled", 1)):
        fresh()
        tw = NetVladTower(B, T, F, V, iterations=S, frames=frames, every_n=every_n, **kw)
        graph = SingleTowerGraph(tw)
        if frames == "grid":
            r = time_calls(lambda: graph.step(x, y, n, num_frames_host=n_host), args.warmup, args.steps, args.rounds)
        else:
            r = time_calls(lambda: graph.step(x, y, n), args.warmup, args.steps, args.rounds)
        lines.append(row(name, tw.R, torch.cuda.max_memory_allocated() / 1e6, r))
        print(lines[-1], flush=True)
        del graph, tw

    lines += ["", "forward-only tower (training=False, the moving statistics)", head]
    for every_n in (1, 10, 30):
        fresh()
        tw = NetVladTower(B, T, F, V, frames="grid", every_n=every_n, training=False, **kw)
        r = time_calls(lambda: tw.forward(x, n, is_training=False, num_frames_host=n_host), args.warmup, args.steps, args.rounds)
        lines.append(row("grid --every_n %d" % every_n, tw.R, torch.cuda.max_memory_allocated() / 1e6, r) + "   (%.0f videos / s)" % (B / r["median"] * 1e3))
        print(lines[-1], flush=True)
        del tw
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
