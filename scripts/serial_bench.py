"""Serial distillation against the parallel step and the student alone, on one MI355X, bf16 forward on uint8 frames:

  * ms/step (mean, median, max - as bench.py reports them: HIP events on the caller's stream after every step) and
    torch.cuda.max_memory_allocated of DistillGraph mode "serial" / "teacher_student" / "student" at (B, every_n) = (256, 10) and
    (1024, 30), same inputs, same process, one after the other;
  * the loss section alone on one stream: evc_distill_losses + its finish launch against the four launches of the parallel step
    (evc_ce_loss teacher, evc_ce_loss student, evc_kl_pred_loss, evc_rep_loss) at B = 256 and B = 1024.

    python scripts/serial_bench.py [--out profiles/serial_distill_bench.txt] [--steps 20] [--warmup 3]
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


def time_graph(mode, B, every_n, steps, warmup, pool_in, n_host):
    from efficientvideoclassification_youtube8m_amd.distill import DistillGraph
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()               # the resident input pool: the same for every mode
    g = DistillGraph(B, every_n=every_n, mode=mode, device=DEV, seed=7)
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
    res = dict(mean=clock.span_ms() / steps, median=st["ms_per_step_median"], max=st["ms_per_step_max"], stall=st["stall_suspected"],
               peak_mib=(torch.cuda.max_memory_allocated() - base) / 2.0 ** 20, finite=all(np.isfinite(v) for v in rep.values()))
    del g
    torch.cuda.empty_cache()
    return res


def time_losses(B, D, reps):
    from efficientvideoclassification_youtube8m_amd import ops
    gen = torch.Generator(device=DEV)
    gen.manual_seed(B)
    pt, ps = (torch.rand((B, V), generator=gen, device=DEV) * (1 - 2e-6) + 1e-6 for _ in range(2))
    y = (torch.rand((B, V), generator=gen, device=DEV) < 0.001).to(torch.uint8)
    st, ss = (torch.randn((B, D), generator=gen, device=DEV) for _ in range(2))
    rt, rs = pt.sum(1), ps.sum(1)
    losses = torch.zeros(8, dtype=torch.float32, device=DEV)
    dpt, dps, dss = torch.empty_like(pt), torch.empty_like(ps), torch.empty_like(ss)

    def fused():
        ops.distill_losses(pt, rt, ps, rs, y, st, ss, losses, dps, dss, g_ce=1.0 / B, g_kl=1.0, g_rep=2.0)

    def four():
        ops.ce_loss(pt, y, losses[0:1], dpt, grad_scale=1.0 / B)
        ops.ce_loss(ps, y, losses[3:4], dps, grad_scale=1.0 / B)
        ops.kl_pred_loss(pt, rt, ps, rs, losses[2:3], dps, grad_scale=1.0, accumulate_grad=True)
        ops.rep_loss(st, ss, losses[1:2], dss, grad_scale=2.0)

    out = {}
    for name, fn in (("fused", fused), ("four", four)):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "serial_distill_bench.txt"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pool", type=int, default=4)
    args = ap.parse_args()
    from efficientvideoclassification_youtube8m_amd import ops
    ops.check_device(0)
    lines = ["serial distillation (DistillGraph mode 'serial': frozen teacher forward + student step) against the parallel step",
             "('teacher_student') and the student alone ('student'); one MI355X, bf16 forward, uint8 frames resident in HBM,",
             "%d timed steps after %d warm-up steps, HIP events after every step (scripts/serial_bench.py); EVC_DETERMINISTIC %s" %
             (args.steps, args.warmup, "on" if ops.DETERMINISTIC else "off"),
             "peak MiB = torch.cuda.max_memory_allocated over construction + all steps, without the resident input pool", ""]
    lines.append("%-6s %-8s %-16s %10s %10s %10s %10s %8s" % ("B", "every_n", "mode", "mean ms", "median ms", "max ms", "peak MiB", "vs par."))
    for B, every_n in ((256, 10), (1024, 30)):
        pool_in = [synthetic_inputs(B, T, F, V, 1234 + 1000 * i, DEV, False, as_uint8=True) for i in range(args.pool)]
        n_host = [p[1].cpu().numpy() for p in pool_in]
        res = {m: time_graph(m, B, every_n, args.steps, args.warmup, pool_in, n_host) for m in ("teacher_student", "serial", "student")}
        for m in ("teacher_student", "serial", "student"):
            r = res[m]
            assert r["finite"], (B, every_n, m)
            lines.append("%-6d %-8d %-16s %10.3f %10.3f %10.3f %10.0f %7.2fx%s" % (
                B, every_n, m, r["mean"], r["median"], r["max"], r["peak_mib"], r["median"] / res["teacher_student"]["median"],
                "  (a step > 3 x the median or a gap behind the window: read the median)" if r["stall"] else ""))
            print(lines[-1], flush=True)
        del pool_in
        torch.cuda.empty_cache()
    lines += ["", "the loss section alone, one stream, V = %d, D = 4096, %d calls each; us per call (dpred_s and dstate_s written):" % (V, 200),
              "%-6s %-44s %10s %10s %10s" % ("B", "launches", "mean us", "median us", "max us")]
    for B in (256, 1024):
        r = time_losses(B, 4096, 200)
        for name, what in (("four", "evc_ce_loss x2 + evc_kl_pred_loss + evc_rep_loss"), ("fused", "evc_distill_losses + its finish launch")):
            lines.append("%-6d %-44s %10.1f %10.1f %10.1f" % (B, what, r[name]["mean"], r[name]["median"], r[name]["max"]))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
