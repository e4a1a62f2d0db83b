"""Inference throughput of the served towers (inference.py's per-batch work) on one MI355X.

Device-resident uint8 batches (n ~ U{120..300}, 1024 + 128 features, H = 1024, 2 layers, 4716 classes, random weights) for the
student at every_n = 10 and 30 and the teacher, in bf16 and high, at B = 256 and 1024:
  - forward + ops.topk_rows + fetch of [B, k] values and indices (the inference loop without the reader): videos/s, frames read/s
    (300 frames per video: the uint8 batch the forward reads), and the top-k kernel's share (device events around it);
  - the same forward with the full [B, 4716] predictions fetched and numpy argpartition + sort on the host (what format_lines
    does in the reference): the comparison that justifies the kernel;
  - a file-fed run through inference.main per tower (after a warm-up run) on a synthetic TFRecord set in a temp directory, with
    its host-side breakdown.
Prints one JSON line per measurement.

    python scripts/inference_bench.py [--iters 10] [--file_videos 4096]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from efficientvideoclassification_youtube8m_amd import inference, ops, readers, utils  # noqa: E402
from efficientvideoclassification_youtube8m_amd.distill import EvalGraph  # noqa: E402
from efficientvideoclassification_youtube8m_amd.flags import FLAGS  # noqa: E402

F, H, V, K = 1152, 1024, 4716, 20


def batches(B, count, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    out = []
    for _ in range(count):
        q = torch.randint(0, 256, (B, 300, F), dtype=torch.uint8, device=dev, generator=g)
        n = torch.randint(120, 301, (B,), dtype=torch.int32, device=dev, generator=g)
        out.append((q, n, n.cpu().numpy()))
    return out


def host_topk(p, k):
    idx = np.argpartition(p, -k, axis=1)[:, -k:]
    val = np.take_along_axis(p, idx, 1)
    o = np.argsort(-val, axis=1, kind="stable")
    return np.take_along_axis(val, o, 1), np.take_along_axis(idx, o, 1)


def run_config(tower, every_n, precision, B, iters, dev):
    g = EvalGraph(B, every_n=every_n, student_only=tower == "student", teacher_only=tower == "teacher", feature_size=F,
                  vocab_size=V, lstm_cells=H, device=dev, precision=precision)
    labels = torch.zeros((B, V), dtype=torch.uint8, device=dev)
    data = batches(B, 2, dev, 17)
    fetcher = utils.AsyncFetcher(dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]

    def device_loop(n_it, timed):
        pending, tk_ms = None, 0.0
        for it in range(n_it):
            q, n, nh = data[it % len(data)]
            pred = g.step(q, labels, n, num_frames_host=nh)["predictions"]
            if timed:
                ev[it][0].record()
            v, i = ops.topk_rows(pred, K)
            if timed:
                ev[it][1].record()
            h = fetcher.fetch({"values": v, "indices": i})
            if pending is not None:
                fetcher.result(pending)
            pending = h
        fetcher.result(pending)
        torch.cuda.synchronize()
        if timed:
            tk_ms = sum(a.elapsed_time(b) for a, b in ev[:n_it])
        return tk_ms

    def host_loop(n_it):
        pending = None
        for it in range(n_it):
            q, n, nh = data[it % len(data)]
            pred = g.step(q, labels, n, num_frames_host=nh)["predictions"]
            h = fetcher.fetch({"predictions": pred})
            if pending is not None:
                host_topk(fetcher.result(pending)["predictions"], K)
            pending = h
        host_topk(fetcher.result(pending)["predictions"], K)
        torch.cuda.synchronize()

    device_loop(3, False)
    host_loop(2)
    t0 = time.perf_counter()
    tk_ms = device_loop(iters, True)
    t_dev = time.perf_counter() - t0
    t0 = time.perf_counter()
    host_loop(iters)
    t_host = time.perf_counter() - t0
    vids = B * iters
    return {"what": "device_resident", "tower": tower, "every_n": every_n if tower == "student" else None, "precision": precision,
            "batch": B, "top_k": K, "iters": iters,
            "videos_per_s": round(vids / t_dev, 1), "frames_read_per_s": round(vids * 300 / t_dev, 1),
            "ms_per_batch": round(1e3 * t_dev / iters, 3), "topk_ms_per_batch": round(tk_ms / iters, 4),
            "topk_share": round(tk_ms / 1e3 / t_dev, 5),
            "host_topk_videos_per_s": round(vids / t_host, 1), "host_topk_ms_per_batch": round(1e3 * t_host / iters, 3)}


def file_fed(data_dir, dev, tower):
    """inference.main on a synthetic TFRecord set: the whole product path, reader included."""
    with tempfile.TemporaryDirectory() as d:
        g = EvalGraph(8, every_n=10, student_only=tower == "student", teacher_only=tower == "teacher", feature_size=F, vocab_size=V,
                      lstm_cells=H, device=dev)
        sd = {"global_step": 0}
        for tw in (g.teacher, g.student):
            if tw is not None:
                sd.update({k: v.cpu() for k, v in tw.state_dict().items()})
        ckdir = os.path.join(d, "ck")
        os.makedirs(ckdir)
        torch.save(sd, os.path.join(ckdir, "model.ckpt-0.pt"))
        del g
        FLAGS.reset()
        st = inference.main(["--input_data_pattern", os.path.join(data_dir, "test*.tfrecord"), "--train_dir", ckdir + "/",
                             "--output_file", os.path.join(d, "pred.csv"), "--frame_features", "True", "--feature_names", "rgb, audio",
                             "--feature_sizes", "1024, 128", "--model", "HierarchicalLstmModel", "--gpu", "0", "--batch_size", "1024",
                             "--num_inputs_to_lstm", "20", "--lstm_layers", "2", "--lstm_cells", str(H), "--every_n", "10",
                             "--num_readers", "8", "--top_k", str(K)])
        size = os.path.getsize(os.path.join(d, "pred.csv"))
        FLAGS.reset()
    st = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items() if k != "checkpoint"}
    st.update(what="file_fed", videos_per_s=round(st["videos"] / st["seconds"], 1), csv_bytes=size)
    return st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--file_videos", type=int, default=4096)
    ap.add_argument("--skip_file_fed", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    torch.cuda.set_device(0)
    ops.check_device(0)
    for B in (256, 1024):
        for tower, every_n in (("student", 10), ("student", 30), ("teacher", 10)):
            for precision in ("bf16", "high"):
                print(json.dumps(run_config(tower, every_n, precision, B, a.iters, dev)), flush=True)
                torch.cuda.empty_cache()
    if not a.skip_file_fed:
        with tempfile.TemporaryDirectory() as d:
            t0 = time.perf_counter()
            readers.write_synthetic_frame_dataset(d, 4, a.file_videos // 4, feature_sizes=(1024, 128), seed=3, prefix="test")
            print(json.dumps({"what": "file_fed_dataset", "videos": a.file_videos, "files": 4, "write_s": round(time.perf_counter() - t0, 1)}),
                  flush=True)
            for tower in ("student", "teacher"):
                file_fed(d, dev, tower)                                   # warm-up: first launches, reader threads, page cache
                print(json.dumps(file_fed(d, dev, tower)), flush=True)


if __name__ == "__main__":
    main()
