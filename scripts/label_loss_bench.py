"""The label losses of --label_loss (evc_label_loss, every kind) next to evc_ce_loss on the same tensors, in the same process, on one
MI355X: median us per call with the gradient written, one stream, HIP events around every call.

    python scripts/label_loss_bench.py [--out profiles/label_loss_bench.txt] [--reps 200]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V = 4716
DEV = "cuda:0"
KINDS = ("WITH_SPARSITY", "TOP50", "CLASS_IMBALANCE", "POSITIVES", "NEW", "HINGE", "SOFTMAX")


def time_calls(fn, reps):
    for _ in range(10):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_loss_bench.txt"))
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    from efficientvideoclassification_youtube8m_amd import ops
    ops.check_device(0)
    lines = ["label losses (evc_label_loss: main launch + fixed-order finish launch; NEW: + the batch-minimum launch in front) next to",
             "evc_ce_loss on the same tensors; one MI355X, one stream, V = %d, gradient written, %d calls each after 10 warm-up calls," % (V, args.reps),
             "HIP events around every call (scripts/label_loss_bench.py); EVC_DETERMINISTIC %s" % ("on" if ops.DETERMINISTIC else "off"),
             "bytes: pred 4 + labels 1 + dpred 4 per element (CLASS_IMBALANCE: + the [V] weights, cached; NEW: pred + labels read twice)", "",
             "%-6s %-18s %10s %10s %10s %9s %9s" % ("B", "kind", "mean us", "median us", "max us", "vs CE", "GB/s")]
    for B in (256, 1024):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(B)
        p = torch.rand((B, V), generator=gen, device=DEV) * 0.96 + 0.02
        y = (torch.rand((B, V), generator=gen, device=DEV) < 3.0 / V).to(torch.uint8)
        w = torch.rand((V,), generator=gen, device=DEV) * 100 + 1
        dp = torch.empty_like(p)
        loss = torch.zeros(1, dtype=torch.float32, device=DEV)
        ce = time_calls(lambda: ops.ce_loss(p, y, loss, dp, grad_scale=1.0 / B), args.reps)
        rows = [("evc_ce_loss", ce)]
        for kind in KINDS:
            k = getattr(ops, "LOSS_" + kind)
            cw = w if kind == "CLASS_IMBALANCE" else None
            rows.append((kind, time_calls(lambda: ops.label_loss(k, p, y, loss, dp, grad_scale=1.0 / B, class_weights=cw), args.reps)))
        for name, r in rows:
            lines.append("%-6d %-18s %10.1f %10.1f %10.1f %8.2fx %9.0f" % (B, name, r["mean"], r["median"], r["max"], r["median"] / ce["median"],
                                                                         9.0 * B * V / (r["median"] * 1e-6) / 1e9))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
