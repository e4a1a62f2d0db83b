"""NeXtVLAD tower over packed ragged frames (--nextvlad_frames grid): the training step at every_n = 1 (every real
frame: the teacher's input), 10 and 30 (the fewer-frames students'), and the sampled mode at S = 30 in the same process.  One
MI355X, one stream, uint8 input.  Nothing is asserted on these numbers.

    timeout -k 10 900 python scripts/nextvlad_packed_bench.py [--out profiles/nextvlad_packed_bench.txt] [--steps 30] [--rounds 3]

B = 256, F = 1152, expansion 2, G = 8, K = 128, H = 2048, gating reduction 8, 4716 classes, n_b ~ U{120..300} through
SingleTowerGraph.step (forward, loss, backward, clip + Adam): `--warmup` untimed steps first, then `--rounds` windows of `--steps`
steps on the same batch, HIP events around every step, the host never waits inside a window; mean / median / max over all timed
steps and the median of each window.  Rows = packed frame rows of the batch (R; the TN products run on R rounded up to 32); peak
MB = torch.cuda.max_memory_allocated() over the configuration's life, the input batch included.
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


def time_steps(step, warmup, steps, rounds):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    all_ms, medians = [], []
    for _ in range(rounds):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        ev[0].record()
        for i in range(steps):
            step()
            ev[i + 1].record()
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in zip(ev[:-1], ev[1:])]
        all_ms += ms
        medians.append(sorted(ms)[len(ms) // 2])
    s = sorted(all_ms)
    return dict(mean=sum(s) / len(s), median=s[len(s) // 2], max=s[-1], rounds=medians)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nextvlad_packed_bench.txt"))
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    from efficientvideoclassification_youtube8m_amd import ops
    from efficientvideoclassification_youtube8m_amd.distill import SingleTowerGraph
    from efficientvideoclassification_youtube8m_amd.towers import NeXtVladTower
    ops.check_device(0)
    B, S, F, lam, G, K, H, rho = 256, 30, 1152, 2, 8, 128, 2048, 8
    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    x = torch.randint(0, 256, (B, T, F), generator=gen, device=DEV, dtype=torch.uint8)
    n = torch.randint(120, T + 1, (B,), generator=gen, device=DEV, dtype=torch.int32)
    y = (torch.rand((B, V), generator=gen, device=DEV) < 3.0 / V).to(torch.uint8)
    n_host = n.cpu().numpy()
    lines = ["NeXtVLAD tower over packed ragged frames on one MI355X, one stream, uint8 input [%d, %d, %d], %d classes (scripts/nextvlad_packed_bench.py)"
             % (B, T, F, V),
             "B = %d, F = %d, expansion %d, G = %d, K = %d, H = %d, gating reduction %d, n_b ~ U{120..300} (mean %.1f); EVC_DETERMINISTIC %s"
             % (B, F, lam, G, K, H, rho, float(n_host.mean()), "on" if ops.DETERMINISTIC else "off"),
             "training step = SingleTowerGraph.step (forward, loss, backward, clip + Adam): %d warm-up steps, then %d windows of %d steps, HIP events"
             % (args.warmup, args.rounds, args.steps), "around every step", "",
             "%-26s %7s %8s %9s %9s %9s   %s" % ("frames", "rows", "peak MB", "mean ms", "median ms", "max ms", "median of each window")]
    kw = dict(cluster_size=K, hidden_size=H, groups=G, expansion=lam, gating_reduction=rho, device=DEV)
    for name, frames, every_n in (("grid --every_n 1", "grid", 1), ("grid --every_n 10", "grid", 10), ("grid --every_n 30", "grid", 30),
                                  ("sampled --iterations %d" % S, "sampled", 1)):
        gc.collect()                                 # (a tower and its batch-norms reference each other: the previous configuration's buffers)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        tw = NeXtVladTower(B, T, F, V, iterations=S, frames=frames, every_n=every_n, **kw)
        graph = SingleTowerGraph(tw)
        if frames == "grid":
            r = time_steps(lambda: graph.step(x, y, n, num_frames_host=n_host), args.warmup, args.steps, args.rounds)
        else:
            r = time_steps(lambda: graph.step(x, y, n), args.warmup, args.steps, args.rounds)
        peak = torch.cuda.max_memory_allocated() / 1e6
        lines.append("%-26s %7d %8.0f %9.3f %9.3f %9.3f   %s" % (name, tw.R, peak, r["mean"], r["median"], r["max"],
                                                              " ".join("%.3f" % m for m in r["rounds"])))
        print(lines[-1], flush=True)
        del graph, tw
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
