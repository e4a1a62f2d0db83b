"""Evaluation-loop throughput (validate.py's per-batch work without the reader) on one MI355X: today's host metrics against
--metrics_on_device.

Device-resident uint8 batches at real dimensions (n ~ U{120..300}, 1024 + 128 features, H = 1024, 2 layers, 4716 classes, random
weights, 1 - 8 positive labels per video), the validate graph (teacher + student at every_n = 10) and the student-only graph of
eval_finetune, bf16, B = 512 and 1024.  Two loops per configuration, each the shape of validate.evaluation_loop (batch k's
host work runs under batch k+1's forward):
  A. fetch of the [B, 4716] predictions and labels + EvaluationMetrics.accumulate (the default path);
  B. ops.eval_select_rows behind the head + fetch of its six small tensors + EvaluationMetrics.accumulate_selected.
Both are warmed up, then run alternately `--windows` times each in this process; every window ends in a device synchronise.
One JSON line per configuration: videos/s of A and B (median, min, max over the windows), their ratio, the selection's device
time per batch (device events around ops.eval_select_rows: the kernel and the 19 KB memset of class_pos), and the bytes fetched
per batch by each path (computed from the shapes).

    python scripts/eval_bench.py [--iters 8] [--windows 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from efficientvideoclassification_youtube8m_amd import eval_util, ops, utils  # noqa: E402
from efficientvideoclassification_youtube8m_amd.distill import EvalGraph  # noqa: E402

F, H, V, K = 1152, 1024, 4716, 20


def batches(B, count, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    out = []
    for _ in range(count):
        q = torch.randint(0, 256, (B, 300, F), dtype=torch.uint8, device=dev, generator=g)
        n = torch.randint(120, 301, (B,), dtype=torch.int32, device=dev, generator=g)
        labels = torch.zeros((B, V), dtype=torch.uint8, device=dev)
        cls = torch.randint(0, V, (B, 8), device=dev, generator=g)
        keep = torch.arange(8, device=dev)[None, :] < torch.randint(1, 9, (B, 1), device=dev, generator=g)
        labels.scatter_(1, torch.where(keep, cls, cls[:, :1]), 1)        # 1 - 8 positives per row (fewer where classes repeat)
        out.append((q, labels, n, n.cpu().numpy()))
    return out


def fetched_bytes(B):
    """Bytes copied device -> host per batch, from the shapes of the two fetches (loss scalars included)."""
    a = B * V * 4 + B * V * 1 + 4
    b = B * K * (4 + 4 + 1) + B * (4 + 4) + V * 4 + 4
    return a, b


def run_config(student_only, B, iters, windows, dev):
    g = EvalGraph(B, every_n=10, student_only=student_only, feature_size=F, vocab_size=V, lstm_cells=H, device=dev, precision="bf16")
    data = batches(B, 2, dev, 17)
    fetcher = utils.AsyncFetcher(dev)
    evl = eval_util.EvaluationMetrics(V, K)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]

    def account_a(handle):
        got = fetcher.result(handle)
        evl.accumulate(got["predictions"], got["labels"].astype(np.float32), float(got["loss"].reshape(-1)[0]))

    def account_b(handle):
        got = fetcher.result(handle)
        evl.accumulate_selected(got["top_val"], got["top_idx"], got["top_lab"], got["n_pos"], got["perr_hits"], got["class_pos"],
                                float(got["loss"].reshape(-1)[0]))

    def loop(on_device, n_it):
        """One window; returns (seconds, kernel milliseconds summed over the window - loop B only)."""
        evl.clear()
        account = account_b if on_device else account_a
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pending = None
        for it in range(n_it):
            q, labels, n, nh = data[it % len(data)]
            out = g.step(q, labels, n, num_frames_host=nh)
            if on_device:
                ev[it][0].record()
                fetch = ops.eval_select_rows(out["predictions"], labels, K)
                ev[it][1].record()
                fetch["loss"] = out["loss"].reshape(1)
            else:
                fetch = {"predictions": out["predictions"], "labels": labels, "loss": out["loss"].reshape(1)}
            handle = fetcher.fetch(fetch)
            if pending is not None:
                account(pending)
            pending = handle
        account(pending)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dt, (sum(a.elapsed_time(b) for a, b in ev[:n_it]) if on_device else 0.0)

    loop(False, 2)
    loop(True, 2)
    t_a, t_b, k_ms = [], [], []
    for _ in range(windows):
        t_a.append(loop(False, iters)[0])
        dt, ms = loop(True, iters)
        t_b.append(dt)
        k_ms.append(ms / iters)
    vids = B * iters
    rate_a, rate_b = [vids / t for t in t_a], [vids / t for t in t_b]
    bytes_a, bytes_b = fetched_bytes(B)

    def stats(r):
        return {"median": round(statistics.median(r), 1), "min": round(min(r), 1), "max": round(max(r), 1)}
    return {"what": "eval_loop", "graph": "student_only" if student_only else "validate", "every_n": 10, "precision": "bf16", "batch": B,
            "top_k": K, "iters": iters, "windows": windows,
            "A_host_metrics_videos_per_s": stats(rate_a), "B_metrics_on_device_videos_per_s": stats(rate_b),
            "B_over_A_median": round(statistics.median(rate_b) / statistics.median(rate_a), 3),
            "A_ms_per_batch": round(1e3 * statistics.median(t_a) / iters, 3), "B_ms_per_batch": round(1e3 * statistics.median(t_b) / iters, 3),
            "select_ms_per_batch": round(statistics.median(k_ms), 4),
            "A_fetched_bytes_per_batch": bytes_a, "B_fetched_bytes_per_batch": bytes_b}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--windows", type=int, default=3)
    a = ap.parse_args()
    if a.windows < 3:
        ap.error("--windows: at least 3 (the spread is part of the result)")
    dev = "cuda:0"
    torch.cuda.set_device(0)
    ops.check_device(0)
    for student_only in (False, True):
        for B in (512, 1024):
            print(json.dumps(run_config(student_only, B, a.iters, a.windows, dev)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
