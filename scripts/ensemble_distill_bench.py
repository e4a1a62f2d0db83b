"""One student against J frozen teachers (EnsembleDistillGraph) against the single-teacher serial step, on one MI355X, bf16 forward on
uint8 frames, by the method of scripts/serial_students_bench.py:

  * ms/step (mean, median, max - as bench.py reports them: HIP events on the caller's stream after every step) and
    torch.cuda.max_memory_allocated of DistillGraph mode "serial" (the yardstick, measured in a window before and a window after the
    others: the spread between the two is what "equal" means in this run), and EnsembleDistillGraph with J = 1, 2, 3 teacher towers and
    with one teacher tower + one every_n = 10 student tower, at (B, every_n) = (1024, 30) and (256, 10); same inputs, same process, one
    after the other;
  * the loss section alone on one stream at V = 4716, D = 4096: evc_distill_losses_ensemble at J = 2 against the composition it replaces,
    ops.ensemble_topk_rows(dense) then evc_distill_losses_multi with K = 1.

    python scripts/ensemble_distill_bench.py [--out profiles/ensemble_distill_bench.txt] [--steps 20] [--warmup 3]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench import synthetic_inputs      # noqa: E402  (the benchmark's own inputs)
from serial_students_bench import time_graph      # noqa: E402  (the same windows and statistics)

T, F, V = 300, 1152, 4716
DEV = "cuda:0"


def time_losses(B, D, reps, J=2):
    from efficientvideoclassification_youtube8m_amd import ops
    gen = torch.Generator(device=DEV)
    gen.manual_seed(B)
    pts = [torch.rand((B, V), generator=gen, device=DEV) * (1 - 2e-6) + 1e-6 for _ in range(J)]
    ps = torch.rand((B, V), generator=gen, device=DEV) * (1 - 2e-6) + 1e-6
    y = (torch.rand((B, V), generator=gen, device=DEV) < 0.001).to(torch.uint8)
    sts = [torch.randn((B, D), generator=gen, device=DEV) for _ in range(J)]
    ss = torch.randn((B, D), generator=gen, device=DEV)
    rs = ps.sum(1)
    losses = torch.zeros(4 + J, dtype=torch.float32, device=DEV)
    dp, ds, comb = torch.empty_like(ps), torch.empty_like(ss), torch.empty_like(ps)

    def ensemble():
        ops.distill_losses_ensemble(pts, sts, y, ps, ss, losses[0:4], dp, ds, mode="mean", g_ce=1.0 / B, g_kl=1.0, g_rep=2.0,
                                    teacher_ce=losses[4:], pred_comb=comb)

    def ensemble_bare():
        ops.distill_losses_ensemble(pts, sts, y, ps, ss, losses[0:4], dp, ds, mode="mean", g_ce=1.0 / B, g_kl=1.0, g_rep=2.0)

    def composition():
        c = ops.ensemble_topk_rows(pts, 0, mode="mean", dense=True)[2]
        ops.distill_losses_multi(c, rs, y, sts[0], [ps], [rs], [ss], losses[0:4].view(1, 4), [dp], [ds], g_ce=1.0 / B, g_kl=1.0, g_rep=2.0)

    out = {}
    for name, fn in (("composition", composition), ("ensemble", ensemble), ("ensemble_bare", ensemble_bare)):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_distill_bench.txt"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pool", type=int, default=4)
    args = ap.parse_args()
    from efficientvideoclassification_youtube8m_amd import ops
    from efficientvideoclassification_youtube8m_amd.distill import DistillGraph, EnsembleDistillGraph
    ops.check_device(0)
    lines = ["ONE student against J frozen teachers per batch (EnsembleDistillGraph) against the single-teacher serial step (DistillGraph mode",
             "'serial', measured twice: before and after the others); one MI355X, bf16 forward, uint8 frames resident in HBM, %d timed steps" % args.steps,
             "after %d warm-up steps, HIP events after every step (scripts/ensemble_distill_bench.py); EVC_DETERMINISTIC %s" %
             (args.warmup, "on" if ops.DETERMINISTIC else "off"),
             "peak MiB = torch.cuda.max_memory_allocated over construction + all steps, without the resident input pool",
             "- serial = median minus the first serial window's median; the teachers are untrained towers (the time does not depend on the weights)", ""]
    lines.append("%-6s %-8s %-34s %10s %10s %10s %10s %10s" % ("B", "every_n", "graph", "mean ms", "median ms", "max ms", "peak MiB", "- serial"))
    for B, every_n in ((1024, 30), (256, 10)):
        pool_in = [synthetic_inputs(B, T, F, V, 1234 + 1000 * i, DEV, False, as_uint8=True) for i in range(args.pool)]
        n_host = [p[1].cpu().numpy() for p in pool_in]
        serial = lambda: DistillGraph(B, every_n=every_n, mode="serial", device=DEV, seed=7)
        rows = [("serial (first window)", serial)]
        for J in (1, 2, 3):
            rows.append(("ensemble J=%d teacher towers" % J,
                         (lambda J=J: EnsembleDistillGraph(B, teachers=[("teacher",)] * J, every_n=every_n, device=DEV, seed=7))))
        rows.append(("ensemble teacher + every_n=10 student",
                     lambda: EnsembleDistillGraph(B, teachers=[("teacher",), ("student", 10, "uniform")], every_n=every_n, device=DEV, seed=7)))
        rows.append(("serial (second window)", serial))
        first = None
        for name, make in rows:
            r = time_graph(make, args.steps, args.warmup, pool_in, n_host)
            assert r["finite"], (B, every_n, name)
            if first is None:
                first = r["median"]
            lines.append("%-6d %-8d %-34s %10.3f %10.3f %10.3f %10.0f %+10.3f%s" % (
                B, every_n, name, r["mean"], r["median"], r["max"], r["peak_mib"], r["median"] - first,
                "  (a step > 3 x the median or a gap behind the window: read the median)" if r["stall"] else ""))
            print(lines[-1], flush=True)
        del pool_in
        torch.cuda.empty_cache()
    lines += ["", "the loss section alone, one stream, V = %d, D = 4096, J = 2 (mean), %d calls each; us per call (dpred_s and dstate_s written):" % (V, 200),
              "%-6s %-76s %10s %10s %10s" % ("B", "launches", "mean us", "median us", "max us")]
    for B in (256, 1024):
        r = time_losses(B, 4096, 200)
        for name, what in (("composition", "evc_ensemble_topk_rows (dense exit) + evc_distill_losses_multi K = 1 + its finish"),
                           ("ensemble", "evc_distill_losses_ensemble + its finish, teacher_ce and pred_comb written"),
                           ("ensemble_bare", "evc_distill_losses_ensemble + its finish, neither of the two")):
            lines.append("%-6d %-76s %10.1f %10.1f %10.1f" % (B, what, r[name]["mean"], r[name]["median"], r[name]["max"]))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
