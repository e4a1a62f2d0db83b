"""Offline distillation (OfflineDistillGraph: the student alone against teacher prediction files) against the two steps it stands
between, on one MI355X, bf16 forward on uint8 frames, by the method of scripts/serial_students_bench.py:

  * ms/step (mean, median, max - as bench.py reports them: HIP events on the caller's stream after every step) and
    torch.cuda.max_memory_allocated of DistillGraph mode "student" (the finetune step, the yardstick: measured in a window before and a
    window after the others - the spread between the two is what "equal" means in this run), of the new step with F = 1 file of kp = 20
    and F = 3 files of kp = 100 entries per video, and of DistillGraph mode "serial" on pred,ce, at (B, every_n) = (1024, 30) and
    (256, 10); same inputs, same process, one after the other.  The reader is excluded (frames resident in HBM).  The new step is
    measured twice: with the host gather of every batch's lists inside the step (inference.PriorTables.gather_device: dictionary
    lookups, np.take into pinned buffers, non_blocking copies - what train --teacher_preds_pattern does per step) and with the lists
    staged on the device beforehand; the difference is the host's share.
  * the loss section alone on one stream at V = 4716: evc_distill_losses_sparse against evc_distill_losses_ensemble (J = 1, no state
    gradient) fed the scattered dense row, with and without the launch that scatters it (evc_ensemble_topk_rows' dense exit).

    python scripts/offline_distill_bench.py [--out profiles/offline_distill_bench.txt] [--steps 20] [--warmup 3]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench import synthetic_inputs      # noqa: E402  (the benchmark's own inputs)
from serial_students_bench import time_graph      # noqa: E402  (the same windows and statistics)

T, F, V = 300, 1152, 4716
DEV = "cuda:0"
FILES = ((1, 20), (3, 100))         # (files, entries per video)


def synthetic_tables(ids, files, kp, seed):
    """What read_prediction_file returns for `files` files listing kp distinct classes with confidences in (0, 1) for every id."""
    rng = np.random.default_rng(seed)
    tables = []
    for _ in range(files):
        keys = rng.random((len(ids), V), dtype=np.float32)
        cls = np.argpartition(keys, kp, axis=1)[:, :kp].astype(np.int32)           # kp distinct classes per video
        conf = rng.uniform(1e-3, 1.0, (len(ids), kp)).astype(np.float32)
        tables.append({vid: (cls[i], conf[i]) for i, vid in enumerate(ids)})
    return tables


class WithLists:
    """An OfflineDistillGraph behind the step(x, labels, n, num_frames_host) of the other graphs: the lists of the batch come from the
    host tables at every step (staged = None) or from device tensors staged before the window."""

    def __init__(self, graph, tables, ids_of, staged):
        self.g, self.tables, self.ids_of, self.staged = graph, tables, ids_of, staged

    def step(self, x, labels, n, num_frames_host=None):
        key = x.data_ptr()
        lists = self.staged[key] if self.staged is not None else self.tables.gather_device(self.ids_of[key], DEV)
        return self.g.step(x, labels, n, num_frames_host=num_frames_host, teacher_lists=lists)

    def flush(self):
        self.g.flush()

    def loss_report(self):
        return self.g.loss_report()


def time_losses(B, files, kp, reps):
    from efficientvideoclassification_youtube8m_amd import ops
    gen = torch.Generator(device=DEV)
    gen.manual_seed(B + kp)
    ps = torch.rand((B, V), generator=gen, device=DEV) * (1 - 2e-6) + 1e-6
    y = (torch.rand((B, V), generator=gen, device=DEV) < 0.001).to(torch.uint8)
    idx = torch.stack([torch.rand((B, V), generator=gen, device=DEV).topk(kp, dim=1).indices.to(torch.int32) for _ in range(files)]).contiguous()
    val = torch.rand((files, B, kp), generator=gen, device=DEV) * 0.998 + 1e-3
    zeros, state = torch.zeros((B, V), device=DEV), torch.zeros((B, 4), device=DEV)
    losses = torch.zeros(4, dtype=torch.float32, device=DEV)
    dp = torch.empty_like(ps)
    w = np.full(files, np.float32(1) / np.float32(files), np.float32)
    wz = np.concatenate([np.zeros(1, np.float32), w])
    dense = ops.ensemble_topk_rows([zeros], 0, mode="mean", weights=wz, priors=(idx, val), dense=True)[2]

    def sparse():
        ops.distill_losses_sparse(idx, val, y, ps, losses, dp, mode="mean", weights=w, g_ce=1.0 / B, g_kl=1.0)

    def dense_fed():
        ops.distill_losses_ensemble([dense], [state], y, ps, state, losses, dp, None, mode="mean", weights=[1.0], g_ce=1.0 / B, g_kl=1.0, g_rep=0.0)

    def scatter_then_dense():
        d = ops.ensemble_topk_rows([zeros], 0, mode="mean", weights=wz, priors=(idx, val), dense=True)[2]
        ops.distill_losses_ensemble([d], [state], y, ps, state, losses, dp, None, mode="mean", weights=[1.0], g_ce=1.0 / B, g_kl=1.0, g_rep=0.0)

    out = {}
    for name, fn in (("sparse", sparse), ("dense_fed", dense_fed), ("scatter_then_dense", scatter_then_dense)):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "offline_distill_bench.txt"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pool", type=int, default=4)
    args = ap.parse_args()
    from efficientvideoclassification_youtube8m_amd import ops
    from efficientvideoclassification_youtube8m_amd.distill import DistillGraph, OfflineDistillGraph
    from efficientvideoclassification_youtube8m_amd.inference import PriorTables
    ops.check_device(0)
    lines = ["Offline distillation (OfflineDistillGraph: the student alone against F teacher prediction files of kp entries per video) against",
             "the student-only step (DistillGraph mode 'student', the train_finetune step; measured twice: before and after the others) and",
             "the serial step on pred,ce (DistillGraph mode 'serial': the frozen teacher runs forward on every batch); one MI355X, bf16 forward,",
             "uint8 frames resident in HBM (the reader is excluded), %d timed steps after %d warm-up steps, HIP events after every step" %
             (args.steps, args.warmup),
             "(scripts/offline_distill_bench.py); EVC_DETERMINISTIC %s" % ("on" if ops.DETERMINISTIC else "off"),
             "gathered = the lists of every batch looked up on the host inside the step (PriorTables.gather_device: one dictionary lookup per",
             "video, one np.take per file into pinned buffers, non_blocking copies), as train --teacher_preds_pattern runs; staged = the same",
             "lists on the device before the window; gathered - staged is the host's share of the step",
             "peak MiB = torch.cuda.max_memory_allocated over construction + all steps, without the resident input pool",
             "- student = median minus the first student-only window's median; untrained towers and random lists (the time does not depend on",
             "the values)", ""]
    lines.append("%-6s %-8s %-44s %10s %10s %10s %10s %10s" % ("B", "every_n", "graph", "mean ms", "median ms", "max ms", "peak MiB", "- student"))
    notes = []
    for B, every_n in ((1024, 30), (256, 10)):
        pool_in = [synthetic_inputs(B, T, F, V, 1234 + 1000 * i, DEV, False, as_uint8=True) for i in range(args.pool)]
        n_host = [p[1].cpu().numpy() for p in pool_in]
        ids = [["b%dv%d" % (i, v) for v in range(B)] for i in range(args.pool)]
        ids_of = {p[0].data_ptr(): ids[i] for i, p in enumerate(pool_in)}
        student = lambda: DistillGraph(B, every_n=every_n, mode="student", device=DEV, seed=7)
        rows = [("student only (first window)", student)]
        for files, kp in FILES:
            tables = PriorTables(["file%d.csv" % f for f in range(files)], V, tables=synthetic_tables(sum(ids, []), files, kp, files * 1000 + kp))
            assert tables.kp == kp
            staged = {key: tuple(torch.from_numpy(a).to(DEV) for a in tables.gather(v)) for key, v in ids_of.items()}
            offline = lambda: OfflineDistillGraph(B, every_n=every_n, device=DEV, seed=7)
            rows.append(("offline F=%d kp=%d, lists gathered per step" % (files, kp),
                         lambda offline=offline, tables=tables: WithLists(offline(), tables, ids_of, None)))
            rows.append(("offline F=%d kp=%d, lists staged on the device" % (files, kp),
                         lambda offline=offline, tables=tables, staged=staged: WithLists(offline(), tables, ids_of, staged)))
        rows.append(("serial on pred,ce", lambda: DistillGraph(B, every_n=every_n, mode="serial", distill_losses=("pred", "ce"), device=DEV, seed=7)))
        rows.append(("student only (second window)", student))
        first, medians = None, {}
        for name, make in rows:
            r = time_graph(make, args.steps, args.warmup, pool_in, n_host)
            assert r["finite"], (B, every_n, name)
            medians[name] = r["median"]
            if first is None:
                first = r["median"]
            lines.append("%-6d %-8d %-44s %10.3f %10.3f %10.3f %10.0f %+10.3f%s" % (
                B, every_n, name, r["mean"], r["median"], r["max"], r["peak_mib"], r["median"] - first,
                "  (a step > 3 x the median or a gap behind the window: read the median)" if r["stall"] else ""))
            print(lines[-1], flush=True)
        # what the rows say: the spread of this run is the distance between the two student-only windows (the same graph, the same inputs)
        lo, hi = sorted((medians["student only (first window)"], medians["student only (second window)"]))
        notes.append("B = %d, every_n = %d: the two student-only windows stand %.3f ms apart (median): this run's spread" % (B, every_n, hi - lo))
        for files, kp in FILES:
            gathered = medians["offline F=%d kp=%d, lists gathered per step" % (files, kp)]
            staged_ms = medians["offline F=%d kp=%d, lists staged on the device" % (files, kp)]
            where = "inside the band of the two student-only windows" if lo <= gathered <= hi else (
                "%.3f ms above the slower student-only window: outside the spread" % (gathered - hi) if gathered > hi else
                "%.3f ms below the faster student-only window: outside the spread" % (lo - gathered))
            notes.append("  F = %d, kp = %d: the step with its host gather is %s; gathered - staged = %+.3f ms (the host's share; host-bound "
                         "would show as a share of the order of the step), serial on pred,ce - this step = %+.3f ms" %
                         (files, kp, where, gathered - staged_ms, medians["serial on pred,ce"] - gathered))
        del pool_in, rows, staged
        torch.cuda.empty_cache()
    lines += [""] + notes
    lines += ["", "the loss section alone, one stream, V = %d, mode mean, %d calls each; us per call (dpred_s written, no state gradient):" % (V, 200),
              "%-6s %-4s %-4s %-78s %10s %10s %10s" % ("B", "F", "kp", "launches", "mean us", "median us", "max us")]
    for B in (256, 1024):
        for files, kp in FILES:
            r = time_losses(B, files, kp, 200)
            for name, what in (("sparse", "evc_distill_losses_sparse + its finish"),
                               ("dense_fed", "evc_distill_losses_ensemble J = 1 + its finish, fed the scattered dense row"),
                               ("scatter_then_dense", "evc_ensemble_topk_rows (dense exit: the scatter) + evc_distill_losses_ensemble J = 1 + its finish")):
                lines.append("%-6d %-4d %-4d %-78s %10.1f %10.1f %10.1f" % (B, files, kp, what, r[name]["mean"], r[name]["median"], r[name]["max"]))
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
