"""Serial distillation over the NeXtVLAD towers (distill.NeXtVladDistillGraph) on one MI355X, one stream, uint8 input.

    python scripts/nextvlad_distill_bench.py [--out profiles/nextvlad_distill_bench.txt] [--steps 20] [--reps 30]

Configuration of DESIGN.md 7.13: B = 256, F = 1152, expansion 2, G = 8, K = 128, H = 2048, gating reduction 8, 4716 classes,
n_b ~ U{120..300}.  HIP events around every call, 10 warm-up calls, then 3 windows; the figure of a line is the median of the three
window medians, the windows' own medians are printed next to it (their spread is the run-to-run noise).

(a) the two forward aggregation entries - evc_nextvlad_aggregate_packed_fwd (vector ALU) and evc_nextvlad_aggregate_packed_fwd_mfma -
    on the frozen teacher's own a / xe / row_off at every_n = 1, in the same process, called alternately, in both orders;
(b) the frozen teacher's forward alone, and the student's SingleTowerGraph.step alone at every_n = 10 and 30;
(c) the distillation step at every_n = 10 and 30 with its peak memory, next to the sum of its two parts from (b).
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


def windows(fns, reps):
    """Times the callables of ``fns`` called one after the other, round after round: per callable the medians (ms) of WINDOWS windows
    of ``reps`` rounds, after WARMUP untimed rounds."""
    for _ in range(WARMUP):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    meds = [[] for _ in fns]
    for _ in range(WINDOWS):
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)] for _ in range(reps)]
        for r in range(reps):
            ev[r][0].record()
            for i, fn in enumerate(fns):
                fn()
                ev[r][i + 1].record()
        torch.cuda.synchronize()
        for i in range(len(fns)):
            meds[i].append(median([ev[r][i].elapsed_time(ev[r][i + 1]) for r in range(reps)]))
    return meds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nextvlad_distill_bench.txt"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    from efficientvideoclassification_youtube8m_amd import ops
    from efficientvideoclassification_youtube8m_amd.distill import NeXtVladDistillGraph, SingleTowerGraph
    from efficientvideoclassification_youtube8m_amd.towers import NeXtVladTower
    ops.check_device(0)
    B, F, lam, G, K, H, rho = 256, 1152, 2, 8, 128, 2048, 8
    D = lam * F // G
    sizes = dict(cluster_size=K, hidden_size=H, groups=G, expansion=lam, gating_reduction=rho)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    x = torch.randint(0, 256, (B, T, F), generator=gen, device=DEV, dtype=torch.uint8)
    n = torch.randint(120, T + 1, (B,), generator=gen, device=DEV, dtype=torch.int32)
    y = (torch.rand((B, V), generator=gen, device=DEV) < 3.0 / V).to(torch.uint8)
    nh = n.cpu().numpy()
    lines = ["NeXtVLAD serial distillation on one MI355X, one stream, uint8 input [%d, %d, %d], %d classes (scripts/nextvlad_distill_bench.py)"
             % (B, T, F, V),
             "B = %d, F = %d, expansion %d, G = %d (D = %d), K = %d, H = %d, gating reduction %d, n_b ~ U{120..300}; EVC_DETERMINISTIC %s"
             % (B, F, lam, G, D, K, H, rho, "on" if ops.DETERMINISTIC else "off"),
             "HIP events around every call, %d warm-up calls, then %d windows; ms = median of the window medians [each window's median]"
             % (WARMUP, WINDOWS), ""]

    def line(text):
        lines.append(text)
        print(text, flush=True)

    fmt = lambda m: "%9.3f   [%s]" % (median(m), " ".join("%.3f" % v for v in m))

    # ---- (a) the two aggregation entries on the frozen teacher's buffers
    teacher = NeXtVladTower(B, T, F, V, device=DEV, training=False, seed=7, frames="grid", every_n=1, **sizes)
    teacher.forward(x, n, num_frames_host=nh, is_training=False)
    plan = teacher.plan
    V1, s1 = torch.empty_like(teacher.Vv), torch.empty_like(teacher.asum)
    V2, s2 = torch.empty_like(teacher.Vv), torch.empty_like(teacher.asum)
    c2 = teacher.store.p(teacher.C2)
    agg_args = (teacher.a, teacher.xe, teacher.row_off, B, T, G, K, D, plan.R, plan.max_k, c2)
    vec = lambda: ops.nextvlad_aggregate_packed_fwd(*agg_args, V1, s1)
    mfma = lambda: ops.nextvlad_aggregate_packed_fwd_mfma(*agg_args, V2, s2)
    flops = 2.0 * plan.R * G * K * D
    line("(a) forward aggregation at every_n = 1: R = %d rows (%d pairs), max_k = %d, %.1f GFLOP" % (plan.R, plan.R * G, plan.max_k, flops / 1e9))
    line("%-58s %9s" % ("entry (called alternately; order of the pair)", "ms"))
    res = {}
    for order, fns in (("vector, mfma", (vec, mfma)), ("mfma, vector", (mfma, vec))):
        meds = windows(fns, args.reps)
        for name, m in zip(order.split(", "), meds):
            res.setdefault(name, []).append(m)
            line("%-58s %s   %5.1f TFLOP/s" % ("evc_nextvlad_aggregate_packed_fwd%s (%s)" % ("_mfma" if name == "mfma" else "", order), fmt(m),
                                                flops / (median(m) * 1e-3) / 1e12))
    torch.cuda.synchronize()
    line("same bits: V %s, asum %s" % (torch.equal(V1, V2), torch.equal(s1, s2)))
    lo = {k: min(min(m) for m in v) for k, v in res.items()}
    hi = {k: max(max(m) for m in v) for k, v in res.items()}
    line("window medians: vector %.3f .. %.3f ms, mfma %.3f .. %.3f ms -> the mfma entry is %s beyond their spread"
         % (lo["vector"], hi["vector"], lo["mfma"], hi["mfma"], "FASTER" if hi["mfma"] < lo["vector"] else "NOT faster"))
    line("")

    # ---- (b) the parts alone
    line("(b) the parts alone")
    line("%-58s %9s" % ("", "ms"))
    m_t = windows((lambda: teacher.forward(x, n, num_frames_host=nh, is_training=False),), args.steps)[0]
    line("%-58s %s" % ("frozen teacher forward, every_n = 1 (R = %d)" % plan.R, fmt(m_t)))
    del teacher, V1, V2, s1, s2, agg_args, c2
    parts = {}
    for every_n in (10, 30):
        tw = NeXtVladTower(B, T, F, V, device=DEV, seed=8, frames="grid", every_n=every_n, **sizes)
        graph = SingleTowerGraph(tw)
        m = windows((lambda: graph.step(x, y, n, num_frames_host=nh),), args.steps)[0]
        parts[every_n] = median(m)
        line("%-58s %s" % ("student SingleTowerGraph.step, every_n = %d (R = %d)" % (every_n, tw.R), fmt(m)))
        del tw, graph
    line("")

    # ---- (c) the distillation step
    line("(c) NeXtVladDistillGraph.step (teacher forward + student forward + evc_distill_losses + student backward + update)")
    line("%-58s %9s" % ("", "ms"))
    for every_n in (10, 30):
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        g = NeXtVladDistillGraph(B, every_n=every_n, teacher_every_n=1, feature_size=F, vocab_size=V, max_frames=T, device=DEV, **sizes)
        m = windows((lambda: g.step(x, y, n, num_frames_host=nh),), args.steps)[0]
        peak = torch.cuda.max_memory_allocated() / 2 ** 30
        line("%-58s %s   sum of its parts %.3f ms   peak memory %.2f GiB"
             % ("distillation step, every_n = %d" % every_n, fmt(m), median(m_t) + parts[every_n], peak))
        del g
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
