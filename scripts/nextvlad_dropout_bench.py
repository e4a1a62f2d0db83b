"""NeXtVLAD dropout before the hidden layer: what it costs in the training step, and the two new entries next to
their byte floors and to the evc_bn_apply call the forward entry replaces.  One MI355X, one stream, uint8 input.

    python scripts/nextvlad_dropout_bench.py [--out profiles/nextvlad_dropout_bench.txt] [--steps 30] [--rounds 3] [--reps 50]

Step: SingleTowerGraph.step at the shape of scripts/nextvlad_bench.py (B = 256, S = 30, F = 1152, expansion 2, G = 8, K = 128,
H = 2048, gating reduction 8) and by its protocol: `--warmup` untimed steps, then `--rounds` windows of `--steps` steps per rate, HIP
events around every step, the host never waits inside a window.  ONE tower in one process: the windows alternate between rate 0 (the
launches of a tower without the feature) and rate 0.5 (NeXtVladTower.set_dropout between windows), so both rates see the
same clocks, allocator and weights' addresses.
Kernel floor: bytes it must move / 6.29 TB/s (the measured float4-copy rate of HBM3E); every operand once.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from nextvlad_bench import DEV, HBM, T, V, time_calls  # noqa: E402

RATES = (0.0, 0.5)


def window(graph, batch, steps):
    x, y, n = batch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record()
    for i in range(steps):
        graph.step(x, y, n)
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in zip(ev[:-1], ev[1:])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nextvlad_dropout_bench.txt"))
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    from efficientvideoclassification_youtube8m_amd import ops
    from efficientvideoclassification_youtube8m_amd.distill import SingleTowerGraph
    from efficientvideoclassification_youtube8m_amd.towers import NeXtVladTower
    ops.check_device(0)
    B, S, F, lam, G, K, H, rho = 256, 30, 1152, 2, 8, 128, 2048, 8
    E, D = lam * F, lam * F // G
    C = K * D
    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    x = torch.randint(0, 256, (B, T, F), generator=gen, device=DEV, dtype=torch.uint8)
    n = torch.randint(120, T + 1, (B,), generator=gen, device=DEV, dtype=torch.int32)
    y = (torch.rand((B, V), generator=gen, device=DEV) < 3.0 / V).to(torch.uint8)
    lines = ["NeXtVLAD dropout on one MI355X, one stream, uint8 input [%d, %d, %d], %d classes (scripts/nextvlad_dropout_bench.py)" % (B, T, F, V),
             "B = %d, S = %d, F = %d, expansion %d (E = %d), G = %d (D = %d), K = %d (K*D = %d), H = %d, gating reduction %d; EVC_DETERMINISTIC %s"
             % (B, S, F, lam, E, G, D, K, C, H, rho, "on" if ops.DETERMINISTIC else "off"),
             "training step = SingleTowerGraph.step, one tower: %d warm-up steps per rate, then %d rounds of one window of %d steps per rate,"
             % (args.warmup, args.rounds, args.steps),
             "the rates alternating (0, 0.5, 0, 0.5, ...), HIP events around every step", "",
             "%-34s %9s %9s %9s   %s" % ("step", "mean ms", "median ms", "max ms", "median of each window")]
    tw = NeXtVladTower(B, T, F, V, iterations=S, cluster_size=K, hidden_size=H, groups=G, expansion=lam, gating_reduction=rho, device=DEV,
                       dropout=0.5, dropout_seed=1)
    graph = SingleTowerGraph(tw)
    batch = (x, y, n)
    for rate in RATES:
        tw.set_dropout(rate)
        for _ in range(args.warmup):
            graph.step(*batch)
    torch.cuda.synchronize()
    ms = {r: [] for r in RATES}
    med = {r: [] for r in RATES}
    for _ in range(args.rounds):
        for rate in RATES:
            tw.set_dropout(rate)
            w = window(graph, batch, args.steps)
            ms[rate] += w
            med[rate].append(sorted(w)[len(w) // 2])
    stats = {}
    for rate in RATES:
        s = sorted(ms[rate])
        stats[rate] = dict(mean=sum(s) / len(s), median=s[len(s) // 2], max=s[-1])
        lines.append("%-34s %9.3f %9.3f %9.3f   %s" % ("--nextvlad_dropout %g" % rate, stats[rate]["mean"], stats[rate]["median"], stats[rate]["max"],
                                                       " ".join("%.3f" % m for m in med[rate])))
        print(lines[-1], flush=True)
    d = stats[0.5]["median"] - stats[0.0]["median"]
    lines.append("rate 0.5 - rate 0, medians: %+.3f ms (%+.2f %%); the spread of the window medians above is the noise of this comparison"
                 % (d, 100.0 * d / stats[0.0]["median"]))
    print(lines[-1], flush=True)

    # ---- the two entries, and the call the forward entry replaces, on the tower's own buffers of the last step
    bv = tw.bn_v
    Tk, scale = ops.dropout_threshold(0.5)
    dY = torch.randn((B, C), device=DEV)
    n_el = float(B) * C
    vec = 16.0 * C                                           # the four per-column vectors
    kernels = [
        ("evc_bn_apply (bf16 out; replaced)", lambda: ops.bn_apply(tw.U, B, C, bv.mean, bv.var, bv.gamma(), bv.beta(), False, y_bf16=tw.Y_bf), 6.0 * n_el + vec),
        ("evc_nextvlad_dropout_fwd", lambda: ops.nextvlad_dropout_fwd(tw.U, B, C, bv.mean, bv.var, bv.gamma(), bv.beta(), Tk, scale, 1, 0, 7, tw.Y_bf),
         6.0 * n_el + vec),
        ("evc_nextvlad_dropout_bwd", lambda: ops.nextvlad_dropout_bwd(dY, B, C, Tk, scale, 1, 0, 7), 8.0 * n_el),
    ]
    lines += ["", "the entries on the tower's buffers, [%d, %d] elements, %d calls each after 5 warm-up calls, HIP events around every call;" % (B, C, args.reps),
              "floor = bytes / 6.29 TB/s.  (Back-to-back calls on 38 - 75 MB: the operands partly stay in the 256 MB last-level cache, which a call",
              "inside the step does not enjoy; the step rows above are the cost in place.)",
              "%-36s %9s %9s %9s %9s %9s %8s" % ("kernel", "mean us", "median us", "max us", "MB", "floor us", "x floor")]
    for name, fn, nbytes in kernels:
        t = time_calls(fn, args.reps)
        floor = 1e6 * nbytes / HBM
        lines.append("%-36s %9.1f %9.1f %9.1f %9.1f %9.1f %7.1fx" % (name, t["mean"], t["median"], t["max"], nbytes / 1e6, floor, t["median"] / floor))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
