"""NetVLAD serial distillation (--model NetVLADModel --teacher_dir): the frozen teacher's input pass as two launches
(evc_frames_gather_packed + evc_bn_apply) against evc_frames_gather_packed_bn, alternating and in either order; the frozen teacher's
forward with each input pass; the student's training step alone and the distillation step at every_n = 10 / 30 next to the sum of its
parts; hidden1_bn's backward with and without the second gradient.  One MI355X, one stream, uint8 input.  Nothing is asserted on these
numbers; the keep-or-drop rule of the fused input pass is evaluated and printed.

    timeout -k 10 900 python scripts/netvlad_distill_bench.py [--out profiles/netvlad_distill_bench.txt] [--steps 30] [--rounds 3]

B = 256, F = 1152, K = 64, H = 1024, 4716 classes, n_b ~ U{120..300}.  Every figure: `--warmup` untimed calls first, then `--rounds`
windows of `--steps` calls on the same batch, HIP events around every call, the host never waits inside a window; the figure is the
median of the window medians, printed next to each window's median (their spread is the run-to-run noise inside this process).  An A / B
pair alternates its windows (A B A B A B), and is run again in the other order.  peak MB = torch.cuda.max_memory_allocated() over the
configuration's life, the input batch included.
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


def time_calls(call, warmup, steps, rounds):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    return summary([window(call, steps) for _ in range(rounds)])


def time_pair(first, second, warmup, steps, rounds):
    """Alternating windows first, second, first, second, ...: (summary of first, summary of second)."""
    for _ in range(warmup):
        first()
        second()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(rounds):
        a.append(window(first, steps))
        b.append(window(second, steps))
    return summary(a), summary(b)


def row(name, rows, peak, r):
    return "%-44s %7s %8s %9.3f %8.3f   %s" % (name, rows if rows else "-", "%.0f" % peak if peak else "-", r["median"], r["spread"],
                                               " ".join("%.3f" % m for m in r["rounds"]))


def fresh():
    gc.collect()                                     # (a tower and its batch-norms reference each other: the previous configuration's buffers)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "netvlad_distill_bench.txt"))
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    from efficientvideoclassification_youtube8m_amd import ops
    from efficientvideoclassification_youtube8m_amd.distill import NetVladDistillGraph, SingleTowerGraph
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
    head = "%-44s %7s %8s %9s %8s   %s" % ("", "rows", "peak MB", "median ms", "spread", "median of each window")
    lines = ["NetVLAD serial distillation on one MI355X, one stream, uint8 input [%d, %d, %d], %d classes (scripts/netvlad_distill_bench.py)"
             % (B, T, F, V),
             "B = %d, F = %d, K = %d, H = %d, n_b ~ U{120..300} (mean %.1f); EVC_DETERMINISTIC %s"
             % (B, F, K, H, float(n_host.mean()), "on" if ops.DETERMINISTIC else "off"),
             "every figure: %d warm-up calls, then %d windows of %d calls, HIP events around every call; median ms = the median of the "
             "window medians, spread = largest - smallest window median" % w, ""]
    kw = dict(cluster_size=K, hidden_size=H, device=DEV)

    def say(line):
        lines.append(line)
        print(line, flush=True)

    # 1. the teacher's input pass on its rows at every_n = 1: two launches against one
    fresh()
    tt = NetVladTower(B, T, F, V, frames="grid", every_n=1, training=False, **kw)
    tt.forward(x, n, is_training=False, num_frames_host=n_host)
    bi, R, Rp, off = tt.bn_in, tt.R, tt.Rp, tt.row_off[:B + 1]
    stats = (bi.mean, bi.var, bi.gamma(), bi.beta())

    def pair():
        ops.frames_gather_packed(x, n, off, 1, R, Rp, tt.r, normalize=True)
        ops.bn_apply(tt.r, R, F, *stats, False, y_bf16=tt.r_bn)
        if Rp > R:
            tt.r_bn[R:Rp].zero_()

    def fused():
        ops.frames_gather_packed_bn(x, n, off, 1, R, Rp, *stats, tt.r, tt.r_bn, normalize=True)

    say("the frozen teacher's input pass at every_n = 1 (R = %d rows): evc_frames_gather_packed + evc_bn_apply (+ the zero fill of rows "
        "R .. Rp when there are any) against evc_frames_gather_packed_bn, alternating windows" % R)
    say(head)
    res = {}
    for order in ("pair first", "fused first"):
        a, b = time_pair(pair, fused, *w) if order == "pair first" else time_pair(fused, pair, *w)[::-1]
        res[order] = (a, b)
        say(row("two launches (%s)" % order, R, 0, a))
        say(row("evc_frames_gather_packed_bn (%s)" % order, R, 0, b))
    noise = max(r["spread"] for ab in res.values() for r in ab)
    gains = [ab[0]["median"] - ab[1]["median"] for ab in res.values()]
    keep = all(gain > noise for gain in gains)
    say("keep-or-drop: the fused pass is faster by %s ms (pair first / fused first), the largest spread between window medians of either "
        "contender is %.3f ms: %s" % (" / ".join("%.3f" % gain for gain in gains), noise,
                                      "KEEP (faster in both orders by more than that spread)" if keep else "DROP (not faster in both orders by more than that spread)"))

    # 2. the frozen teacher's forward with each input pass
    say("")
    say("the frozen teacher's forward alone (training=False, every_n = 1), with each input pass, alternating windows")
    say(head)

    def fwd(flag):
        def call():
            tt.fused_input_pass = flag
            tt.forward(x, n, is_training=False, num_frames_host=n_host)
        return call

    a, b = time_pair(fwd(False), fwd(True), *w)
    t_fwd = b
    say(row("forward, two launches", R, 0, a))
    say(row("forward, evc_frames_gather_packed_bn", R, torch.cuda.max_memory_allocated() / 1e6, b))
    del tt, bi, stats, off

    # 3. the student's step alone, the distillation step, the sum of the parts
    say("")
    say("the student's training step alone (SingleTowerGraph.step), the distillation step (NetVladDistillGraph.step, teacher every_n = 1) "
        "and teacher forward + student step")
    say(head)
    for every_n in (10, 30):
        fresh()
        tw = NetVladTower(B, T, F, V, frames="grid", every_n=every_n, **kw)
        graph = SingleTowerGraph(tw)
        s = time_calls(lambda: graph.step(x, y, n, num_frames_host=n_host), *w)
        say(row("student step alone, every_n = %d" % every_n, tw.R, torch.cuda.max_memory_allocated() / 1e6, s))
        del graph, tw
        fresh()
        g = NetVladDistillGraph(B, every_n=every_n, teacher_every_n=1, feature_size=F, vocab_size=V, max_frames=T, cluster_size=K, hidden_size=H,
                                device=DEV)
        d = time_calls(lambda: g.step(x, y, n, num_frames_host=n_host), *w)
        say(row("distillation step, every_n = %d" % every_n, g.teacher.R + g.student.R, torch.cuda.max_memory_allocated() / 1e6, d))
        say("%-44s %7s %8s %9.3f" % ("  teacher forward + student step", "", "", t_fwd["median"] + s["median"]))
        del g

    # 4. hidden1_bn's backward with and without the second gradient
    say("")
    say("hidden1_bn's backward (evc_bn_bwd_partial + _finalize, relu6 on, bf16 dx) at R = %d, C = %d: plain against the _add entries with dy2, "
        "alternating windows" % (B, H))
    say(head)
    fresh()
    hid, dy, dy2 = (torch.randn((B, H), generator=gen, device=DEV) for _ in range(3))
    mean, beta = torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
    var, gamma = torch.ones(H, device=DEV), torch.ones(H, device=DEV)
    ws = torch.zeros(2 * H, dtype=torch.float64, device=DEV)
    dxb = torch.empty((B, H), dtype=torch.bfloat16, device=DEV)
    dg, db = torch.empty(H, device=DEV), torch.empty(H, device=DEV)

    def plain():
        ops.bn_bwd_partial(hid, dy, B, H, mean, var, gamma, beta, True, ws)
        ops.bn_bwd_finalize(hid, dy, B, B, H, mean, var, gamma, beta, True, ws, dx_bf16=dxb, dgamma=dg, dbeta=db)

    def added():
        ops.bn_bwd_partial_add(hid, dy, dy2, B, H, mean, var, gamma, beta, True, ws)
        ops.bn_bwd_finalize_add(hid, dy, dy2, B, B, H, mean, var, gamma, beta, True, ws, dx_bf16=dxb, dgamma=dg, dbeta=db)

    a, b = time_pair(plain, added, *w)
    say(row("evc_bn_bwd_partial + _finalize", B, 0, a))
    say(row("evc_bn_bwd_partial_add + _finalize_add (dy2)", B, 0, b))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
