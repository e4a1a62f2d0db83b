"""The fused ensemble launch (ops.ensemble_topk_rows) against the torch chain it replaces, on one MI355X.

Device-resident f32 prediction matrices (B = 1024 rows, V = 4716 classes, uniform in [0, 1), k = 20) of M = 2 and 4 members, both modes:
  - fused: one launch of evc_ensemble_topk_rows -> [B, k] values and indices;
  - torch: torch.stack(members) -> amax over the members (max) / weighted sum over the members (mean) -> torch.topk(k).
Each side is warmed up, then timed ``--windows`` times (at least 20) with device events around ``--calls`` back-to-back calls; the
figure is the median window over the calls in it, with min and max.  The two sides alternate window by window.  The fused launch reads
M B V 4 bytes and writes B k 8: ``fused_read_GBps`` is that over the median time (what the algorithm needs, not what the chip moved).
The selections are compared first: the same classes on every row (random rows without ties).  Prints one JSON line per measurement.

    python scripts/ensemble_bench.py [--windows 25] [--calls 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from efficientvideoclassification_youtube8m_amd import ops  # noqa: E402

B, V, K = 1024, 4716, 20


def torch_chain(members, mode, w_dev):
    stacked = torch.stack(members)
    combined = stacked.amax(0) if mode == "max" else (stacked * w_dev[:, None, None]).sum(0)
    return torch.topk(combined, K, dim=1)


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def run_config(M, mode, windows, calls, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(100 + M)
    members = [torch.rand((B, V), dtype=torch.float32, device=dev, generator=g) for _ in range(M)]
    w = [1.0 / M] * M
    w_dev = torch.tensor(w, dtype=torch.float32, device=dev)
    weights = None if mode == "max" else w

    def fused():
        return ops.ensemble_topk_rows(members, K, mode=mode, weights=weights)

    def chain():
        return torch_chain(members, mode, w_dev)
    same = bool(torch.equal(fused()[1].long().sort(1).values, chain()[1].sort(1).values))
    for fn in (fused, chain):                                            # warm-up: code objects, allocator, clocks
        window(fn, calls)
        window(fn, calls)
    t_fused, t_chain = [], []
    for _ in range(windows):                                             # alternate the two sides
        t_fused.append(window(fused, calls))
        t_chain.append(window(chain, calls))
    sf, sc = stats(t_fused), stats(t_chain)
    return {"what": "ensemble_topk", "members": M, "mode": mode, "batch": B, "classes": V, "top_k": K, "windows": windows, "calls_per_window": calls,
            "fused_ms": sf, "torch_chain_ms": sc, "torch_over_fused_median": round(sc["median"] / sf["median"], 3),
            "fused_read_GBps": round(M * B * V * 4 / (sf["median"] * 1e-3) / 1e9, 1), "same_classes_selected": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=25)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    if a.windows < 20:
        ap.error("--windows: at least 20 (the figure is a median)")
    dev = "cuda:0"
    torch.cuda.set_device(0)
    ops.check_device(0)
    for M in (2, 4):
        for mode in ("max", "mean"):
            print(json.dumps(run_config(M, mode, a.windows, a.calls, dev)), flush=True)


if __name__ == "__main__":
    main()
