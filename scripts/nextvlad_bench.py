"""NeXtVLAD tower (towers.NeXtVladTower, csrc/evc_nextvlad.hip): the training step and every new kernel next to its own floor, and
the NetVLAD tower's step at its defaults in the same process for orientation.  One MI355X, one stream, uint8 input.

    python scripts/nextvlad_bench.py [--out profiles/nextvlad_bench.txt] [--steps 30] [--rounds 3] [--reps 50]

Step: B = 256, S = 30, F = 1152, expansion 2, G = 8, K = 128, H = 2048, gating reduction 8 through SingleTowerGraph.step (forward, loss,
backward, clip + Adam).  `--warmup` untimed steps first (code objects, allocator, clocks), then `--rounds` windows of `--steps`
steps, HIP events around every step, the host never waits inside a window; mean / median / max over all timed steps and the
median of each window (their spread is the run-to-run noise of this box).
Kernel floor: max(bytes it must move / 6.29 TB/s (the measured float4-copy rate of HBM3E), FLOPs / 157.3 TFLOP/s (the f32 vector =
f32 MFMA peak)); the bytes count every operand once, scratch excluded.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
HBM, F32_PEAK = 6.29e12, 157.3e12
V, T = 4716, 300


def time_calls(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    us = sorted(1e3 * a.elapsed_time(b) for a, b in zip(ev[:-1], ev[1:]))
    return dict(mean=1e3 * ev[0].elapsed_time(ev[-1]) / reps, median=us[len(us) // 2], max=us[-1])


def time_steps(graph, batch, warmup, steps, rounds):
    x, y, n = batch
    for _ in range(warmup):
        graph.step(x, y, n)
    torch.cuda.synchronize()
    all_ms, medians = [], []
    for _ in range(rounds):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        ev[0].record()
        for i in range(steps):
            graph.step(x, y, n)
            ev[i + 1].record()
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in zip(ev[:-1], ev[1:])]
        all_ms += ms
        medians.append(sorted(ms)[len(ms) // 2])
    s = sorted(all_ms)
    return dict(mean=sum(s) / len(s), median=s[len(s) // 2], max=s[-1], rounds=medians)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nextvlad_bench.txt"))
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    from efficientvideoclassification_youtube8m_amd import ops
    from efficientvideoclassification_youtube8m_amd.distill import SingleTowerGraph
    from efficientvideoclassification_youtube8m_amd.towers import NetVladTower, NeXtVladTower
    ops.check_device(0)
    B, S, F, lam, G, K, H, rho = 256, 30, 1152, 2, 8, 128, 2048, 8
    E, D, R = lam * F, lam * F // G, B * S
    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    x = torch.randint(0, 256, (B, T, F), generator=gen, device=DEV, dtype=torch.uint8)
    n = torch.randint(120, T + 1, (B,), generator=gen, device=DEV, dtype=torch.int32)
    y = (torch.rand((B, V), generator=gen, device=DEV) < 3.0 / V).to(torch.uint8)
    lines = ["NeXtVLAD tower on one MI355X, one stream, uint8 input [%d, %d, %d], %d classes (scripts/nextvlad_bench.py)" % (B, T, F, V),
             "B = %d, S = %d, F = %d, expansion %d (E = %d), G = %d (D = %d), K = %d, H = %d, gating reduction %d; EVC_DETERMINISTIC %s"
             % (B, S, F, lam, E, G, D, K, H, rho, "on" if ops.DETERMINISTIC else "off"),
             "training step = SingleTowerGraph.step (forward, loss, backward, clip + Adam): %d warm-up steps, then %d windows of %d steps, HIP events"
             % (args.warmup, args.rounds, args.steps), "around every step", "",
             "%-34s %9s %9s %9s   %s" % ("step", "mean ms", "median ms", "max ms", "median of each window")]
    tw = NeXtVladTower(B, T, F, V, iterations=S, cluster_size=K, hidden_size=H, groups=G, expansion=lam, gating_reduction=rho, device=DEV)
    graph = SingleTowerGraph(tw)
    r = time_steps(graph, (x, y, n), args.warmup, args.steps, args.rounds)
    lines.append("%-34s %9.3f %9.3f %9.3f   %s" % ("NeXtVLADModel (sizes above)", r["mean"], r["median"], r["max"], " ".join("%.3f" % m for m in r["rounds"])))
    print(lines[-1], flush=True)

    # ---- every new kernel on the tower's own buffers of the last step
    st, bc = tw.store, tw.bn_cl
    GK, BKD, BH = G * K, B * K * D, B * H
    P = S * G
    scratch_dout, scratch_dh = torch.randn_like(tw.h), torch.empty_like(tw.h)     # (the gate's reverse mode on buffers of its own: the tower's stay as the step left them)
    kernels = [
        ("evc_nextvlad_assign_fwd", lambda: ops.nextvlad_assign_fwd(tw.act, R, G, K, bc.mean, bc.var, bc.gamma(), bc.beta(), tw.attl, tw.a),
         8.0 * R * GK + 4.0 * R * G, 6.0 * R * GK),
        ("evc_nextvlad_assign_bwd", lambda: ops.nextvlad_assign_bwd(tw.act, R, G, K, bc.mean, bc.var, bc.gamma(), bc.beta(), tw.attl, tw.da, tw.dz, tw.datt,
                                                                    datt_logit_bf16=tw.datt_bf),
         12.0 * R * GK + 10.0 * R * G, 10.0 * R * GK),
        ("evc_nextvlad_aggregate_fwd", lambda: ops.nextvlad_aggregate_fwd(tw.a, tw.xe, B, S, G, K, D, st.p(tw.C2), tw.Vv, tw.asum),
         4.0 * R * GK + 4.0 * R * E + 4.0 * BKD, 2.0 * B * P * K * D),
        ("evc_nextvlad_aggregate_bwd", lambda: ops.nextvlad_aggregate_bwd(tw.a, tw.xe, B, S, G, K, D, st.p(tw.C2), tw.dV, tw.da, tw.dxe, ws=tw.agg_ws),
         8.0 * R * GK + 8.0 * R * E + 4.0 * BKD, 4.0 * B * P * K * D),
        ("evc_netvlad_dcenters (dc2)", lambda: ops.netvlad_dcenters(tw.asum, tw.dV, B, K, D, st.g(tw.C2)), 4.0 * BKD, 2.0 * BKD),
        ("evc_nextvlad_normalize_fwd", lambda: ops.nextvlad_normalize_fwd(tw.Vv, B, K, D, tw.U, tw.nrm), 8.0 * BKD, 3.0 * BKD),
        ("evc_nextvlad_normalize_bwd", lambda: ops.nextvlad_normalize_bwd(tw.Vv, tw.nrm, tw.dU, B, K, D, tw.dV), 12.0 * BKD, 5.0 * BKD),
        ("evc_nextvlad_gate_fwd", lambda: ops.nextvlad_gate_fwd(tw.h, tw.gl, tw.out), 12.0 * BH, 4.0 * BH),
        ("evc_nextvlad_gate_bwd", lambda: ops.nextvlad_gate_bwd(tw.h, tw.gl, scratch_dout, scratch_dh, dgl_bf16=tw.dgl_bf), 18.0 * BH, 8.0 * BH),
        ("evc_nextvlad_center_cast", lambda: ops.nextvlad_center_cast(tw.xe, R, E, st.p(tw.EB), tw.xe_bf), 6.0 * R * E, 1.0 * R * E),
        ("evc_nextvlad_bias_logits (Wc)", lambda: ops.nextvlad_bias_logits(st.p(tw.EB), st.p(tw.CW), GK, E, tw.cbias), 4.0 * GK * E, 2.0 * GK * E),
        ("evc_nextvlad_colsum (dbe)", lambda: ops.nextvlad_colsum(tw.dxe, R, E, st.g(tw.EB), ws=tw.colsum_ws), 4.0 * R * E, 1.0 * R * E),
    ]
    lines += ["", "kernels of csrc/evc_nextvlad.hip on the buffers of the last step, %d calls each after 5 warm-up calls, HIP events around every call;" % args.reps,
              "floor = max(bytes / 6.29 TB/s, FLOPs / 157.3 TFLOP/s)",
              "%-30s %9s %9s %9s %9s %9s %9s %8s" % ("kernel", "mean us", "median us", "max us", "MB", "MFLOP", "floor us", "x floor")]
    for name, fn, nbytes, flops in kernels:
        t = time_calls(fn, args.reps)
        floor = 1e6 * max(nbytes / HBM, flops / F32_PEAK)
        lines.append("%-30s %9.1f %9.1f %9.1f %9.1f %9.0f %9.1f %7.1fx" % (name, t["mean"], t["median"], t["max"], nbytes / 1e6, flops / 1e6, floor, t["median"] / floor))
        print(lines[-1], flush=True)
    del graph, tw
    torch.cuda.empty_cache()

    # ---- the NetVLAD tower at its defaults, same batch, for orientation
    tv = NetVladTower(B, T, F, V, iterations=S, device=DEV)
    gv = SingleTowerGraph(tv)
    r = time_steps(gv, (x, y, n), args.warmup, args.steps, args.rounds)
    lines += ["", "%-34s %9s %9s %9s   %s" % ("step (orientation)", "mean ms", "median ms", "max ms", "median of each window"),
              "%-34s %9.3f %9.3f %9.3f   %s" % ("NetVLADModel (K = 64, H = 1024)", r["mean"], r["median"], r["max"], " ".join("%.3f" % m for m in r["rounds"]))]
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
