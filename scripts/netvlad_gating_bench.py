"""The NetVLAD context gate (--netvlad_gating): the fused gate entries (evc_bn_gate_fwd, evc_bn_gate_bwd_partial +
_finalize) against the chain of older entries they replace, forward and backward, alternating and in either order; the training step
at every_n = 10 and 1 with the gate on (fused / chain) against the gate off, in one process; the forward-only tower; peak memory.  One
MI355X, one stream, uint8 input.  Nothing is asserted on these numbers; whether the fused path beats the chain by more than the spread is
evaluated and printed.

    timeout -k 10 900 python scripts/netvlad_gating_bench.py [--out profiles/netvlad_gating_bench.txt] [--steps 30] [--rounds 3]

B = 256, F = 1152, K = 64, H = 1024, 4716 classes, n_b ~ U{120..300}.  Every figure: `--warmup` untimed calls first, then `--rounds`
windows of `--steps` calls on the same batch, HIP events around every call, the host never waits inside a window; the figure is the
median of the window medians, printed next to their spread and each window's median.  An A / B pair alternates its windows (A B A B A B),
and is run again in the other order.  peak MB = torch.cuda.max_memory_allocated() over the configuration's life, the input batch included.
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


def time_group(calls, warmup, steps, rounds):
    """Alternating windows of every call in turn (A B C A B C ...): one summary per call."""
    for _ in range(warmup):
        for c in calls:
            c()
    torch.cuda.synchronize()
    out = [[] for _ in calls]
    for _ in range(rounds):
        for i, c in enumerate(calls):
            out[i].append(window(c, steps))
    return [summary(o) for o in out]


def row(name, rows, peak, r):
    return "%-52s %7s %8s %9.3f %8.3f   %s" % (name, rows if rows else "-", "%.0f" % peak if peak else "-", r["median"], r["spread"],
                                               " ".join("%.3f" % m for m in r["rounds"]))


def fresh():
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "netvlad_gating_bench.txt"))
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    from efficientvideoclassification_youtube8m_amd import ops
    from efficientvideoclassification_youtube8m_amd.distill import SingleTowerGraph
    from efficientvideoclassification_youtube8m_amd.towers import NetVladTower
    ops.check_device(0)
    B, F, K, H = 256, 1152, 64, 1024
    w = (args.warmup, args.steps, args.rounds)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    x = torch.randint(0, 256, (B, T, F), generator=gen, device=DEV, dtype=torch.uint8)
    n = torch.randint(120, T + 1, (B,), generator=gen, device=DEV, dtype=torch.int32)
    y = (torch.rand((B, V), generator=gen, device=DEV) < 3.0 / V).to(torch.uint8)
    n_host = n.cpu().numpy()
    head = "%-52s %7s %8s %9s %8s   %s" % ("", "rows", "peak MB", "median ms", "spread", "median of each window")
    lines = ["NetVLAD context gate on one MI355X, one stream, uint8 input [%d, %d, %d], %d classes (scripts/netvlad_gating_bench.py)" % (B, T, F, V),
             "B = %d, F = %d, K = %d, H = %d, n_b ~ U{120..300} (mean %.1f); EVC_DETERMINISTIC %s"
             % (B, F, K, H, float(n_host.mean()), "on" if ops.DETERMINISTIC else "off"),
             "every figure: %d warm-up calls, then %d windows of %d calls, HIP events around every call; median ms = the median of the "
             "window medians, spread = largest - smallest window median" % (args.warmup, args.rounds, args.steps), ""]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    # 1. the entries alone on [B, H]
    fresh()
    gl, h, d, d2 = (torch.randn((B, H), generator=gen, device=DEV) for _ in range(4))
    h.clamp_(0.0, 6.0)
    mean, beta = 0.1 * torch.randn(H, generator=gen, device=DEV), 0.1 * torch.randn(H, generator=gen, device=DEV)
    var, gamma = 1.0 + torch.rand(H, generator=gen, device=DEV), 1.0 + 0.1 * torch.randn(H, generator=gen, device=DEV)
    st = (mean, var, gamma, beta)
    ws = torch.zeros(2 * H, dtype=torch.float64, device=DEV)
    out, dh, gn, dgn = (torch.empty((B, H), device=DEV) for _ in range(4))
    dgl_bf = torch.empty((B, H), dtype=torch.bfloat16, device=DEV)
    dg, db = torch.empty(H, device=DEV), torch.empty(H, device=DEV)

    def fwd_chain():
        ops.bn_apply(gl, B, H, *st, False, y_f32=gn)
        ops.nextvlad_gate_fwd(h, gn, out)

    def fwd_fused():
        ops.bn_gate_fwd(gl, h, B, H, *st, out)

    def bwd_chain():
        ops.nextvlad_gate_bwd_add(h, gn, d, d2, dh, dgl=dgn)
        ops.bn_bwd_partial(gl, dgn, B, H, *st, False, ws)
        ops.bn_bwd_finalize(gl, dgn, B, B, H, *st, False, ws, dx_bf16=dgl_bf, dgamma=dg, dbeta=db)

    def bwd_fused():
        ops.bn_gate_bwd_partial(gl, h, d, d2, B, H, *st, ws, dh)
        ops.bn_gate_bwd_finalize(gl, h, d, d2, B, B, H, *st, ws, dgl_bf16=dgl_bf, dgamma=dg, dbeta=db)

    say("the gate's entries alone at R = %d, C = %d (with d2; bf16 dgl): the chain of older entries against the fused ones, alternating "
        "windows, in both orders" % (B, H))
    say(head)
    verdict = {}
    for what, chain, fused_ in (("forward", fwd_chain, fwd_fused), ("backward", bwd_chain, bwd_fused)):
        res = []
        for order in ("chain first", "fused first"):
            a, b = time_group([chain, fused_], *w) if order == "chain first" else time_group([fused_, chain], *w)[::-1]
            res.append((a, b))
            say(row("%s, chain (%s)" % (what, order), B, 0, a))
            say(row("%s, fused (%s)" % (what, order), B, 0, b))
        noise = max(r["spread"] for ab in res for r in ab)
        gains = [ab[0]["median"] - ab[1]["median"] for ab in res]
        verdict[what] = all(g > noise for g in gains)
        say("%s: the fused entries are faster by %s ms (chain first / fused first); the largest spread between window medians is %.3f ms: %s"
            % (what, " / ".join("%.3f" % g for g in gains), noise,
               "faster in both orders by more than the spread" if verdict[what] else "NOT faster in both orders by more than the spread"))

    # 2. the training step: gate off, gate on through the chain, gate on through the fused entries - alternating windows of the three
    kw = dict(cluster_size=K, hidden_size=H, device=DEV, frames="grid")
    for every_n in (10, 1):
        say("")
        say("the training step (SingleTowerGraph.step) at every_n = %d: gate off / gate on, chain / gate on, fused - alternating windows" % every_n)
        say(head)
        graphs, peaks = [], []
        for gating, fused_gate in ((False, True), (True, False), (True, True)):
            fresh()
            NetVladTower.fused_gate = fused_gate
            try:
                tw = NetVladTower(B, T, F, V, every_n=every_n, gating=gating, **kw)
            finally:
                NetVladTower.fused_gate = True
            tw.fused_gate = fused_gate
            g = SingleTowerGraph(tw)
            g.step(x, y, n, num_frames_host=n_host)
            torch.cuda.synchronize()
            peaks.append(torch.cuda.max_memory_allocated() / 1e6)       # (this configuration alone: the earlier ones' towers are alive too)
            graphs.append(g)
        base = peaks[0]
        calls = [(lambda g=g: g.step(x, y, n, num_frames_host=n_host)) for g in graphs]
        for order, idx in (("off, chain, fused", (0, 1, 2)), ("fused, chain, off", (2, 1, 0))):
            res = time_group([calls[i] for i in idx], *w)
            for i, r in zip(idx, res):
                say(row("%s (order: %s)" % (("gate off", "gate on, chain", "gate on, fused")[i], order), graphs[i].tower.R, 0, r))
        say("peak MB while each was built and stepped once (towers built earlier in this list still allocated): off %.0f, chain %.0f, fused %.0f"
            % tuple(peaks))
        del graphs, calls, g, tw
        fresh()
        for name, gating, fused_gate in (("gate off", False, True), ("gate on, chain", True, False), ("gate on, fused", True, True)):
            fresh()
            NetVladTower.fused_gate = fused_gate
            try:
                tw = NetVladTower(B, T, F, V, every_n=every_n, gating=gating, **kw)
            finally:
                NetVladTower.fused_gate = True
            tw.fused_gate = fused_gate
            g = SingleTowerGraph(tw)
            for _ in range(3):
                g.step(x, y, n, num_frames_host=n_host)
            torch.cuda.synchronize()
            say("%-52s %7d %8.0f   (alone in memory)" % ("peak, " + name, tw.R, torch.cuda.max_memory_allocated() / 1e6))
            del g, tw

    # 3. the forward-only tower
    say("")
    say("the forward-only tower (training=False, every_n = 1): gate off / chain / fused, alternating windows")
    say(head)
    towers = []
    for gating, fused_gate in ((False, True), (True, False), (True, True)):
        NetVladTower.fused_gate = fused_gate
        try:
            tw = NetVladTower(B, T, F, V, every_n=1, gating=gating, training=False, **kw)
        finally:
            NetVladTower.fused_gate = True
        tw.fused_gate = fused_gate
        towers.append(tw)
    res = time_group([(lambda tw=tw: tw.forward(x, n, is_training=False, num_frames_host=n_host)) for tw in towers], *w)
    for name, tw, r in zip(("gate off", "gate on, chain", "gate on, fused"), towers, res):
        say(row("forward only, " + name, tw.R, 0, r))
    say("")
    say("fused faster than the chain by more than the spread, in both orders: forward %s, backward %s"
        % ("yes" if verdict["forward"] else "no", "yes" if verdict["backward"] else "no"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
