"""The fused MoE update (moe_update_kernel: rank-B gradient + clip + Adam + shadows) against the HBM roofline, and same-box A/B of builds.

    python scripts/moe_update_bench.py [LIB ...] [--alternations N] [--launches L]

Every LIB is a build of libevc_hip.so (default: the package's own).  All of them are loaded into this one process and timed ALTERNATELY on the
same device and the same buffers: N alternations, each L launches per library, every launch between its own pair of events.  Reported per
library and shape: median and minimum per launch of every alternation, the range of the alternation medians, and TB/s at 28 B per parameter
(p, m, v read and written, two bf16 shadows written; the factor product's operands are noise).  Shapes: the headline's gates (14148 x 4096)
and experts (9432 x 4096) matrices at 256 rows through evc_moe_grad_update_apply (the update pass alone, as the step runs it), and cfg 4's
(K = 1024, 512 rows) through evc_moe_grad_update (norm pass + update pass, as cfg 4 runs it).
Before timing, one launch of every library from identical inputs: p, m, v, both shadows and the |W|^2 partials are compared bit for bit
with the first library's.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from efficientvideoclassification_youtube8m_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("libs", nargs="*", default=[_lib.LIB_PATH])
ap.add_argument("--alternations", type=int, default=5)
ap.add_argument("--launches", type=int, default=20)
args = ap.parse_args()

dev = "cuda:0"
torch.zeros(1, device=dev)          # torch's HIP runtime first (see _lib.load)
NAMES = ("evc_moe_grad_update_apply", "evc_moe_grad_update_phase")


def bind(path):
    lib = C.CDLL(os.path.abspath(path))
    for n in NAMES:
        getattr(lib, n).argtypes = _lib.SIGNATURES[n]
        getattr(lib, n).restype = C.c_int
    lib.evc_last_error.restype = C.c_char_p
    return lib


libs = [(p, bind(p)) for p in args.libs]
ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731


def launch(lib, apply, b):
    if apply:
        rc = lib.evc_moe_grad_update_apply(ptr(b["dlog"]), b["dlog"].stride(0), ptr(b["x"]), b["x"].stride(0), b["rows"], b["V"], b["K"],
                                           ptr(b["p"]), ptr(b["m"]), ptr(b["v"]), ptr(b["pb"]), ptr(b["pT"]), b["pT"].stride(0), None, None, None, 0, 0,
                                           2e-8, ptr(b["sums"]), ptr(b["ws"]), 1.0, 1e-3, 0.9, 0.999, 1e-8, ptr(b["wsq"]), stream())
    else:
        rc = lib.evc_moe_grad_update_phase(ptr(b["dlog"]), b["dlog"].stride(0), ptr(b["x"]), b["x"].stride(0), b["rows"], b["V"], b["K"],
                                           ptr(b["p"]), ptr(b["m"]), ptr(b["v"]), ptr(b["pb"]), ptr(b["pT"]), b["pT"].stride(0),
                                           2e-8, ptr(b["sums"]), ptr(b["ws"]), 1.0, 1e-3, 0.9, 0.999, 1e-8, 0, stream())
    if rc != 0:
        raise RuntimeError(lib.evc_last_error().decode())


def buffers(V, K, rows, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    Vp = (V + 63) // 64 * 64
    dlog = torch.zeros(rows, Vp, dtype=torch.bfloat16, device=dev)
    dlog[:, :V] = (torch.randn(rows, V, device=dev, generator=g) * 1e-3).to(torch.bfloat16)
    b = {"V": V, "K": K, "rows": rows, "dlog": dlog, "x": (torch.randn(rows, K, device=dev, generator=g) * 0.1).to(torch.bfloat16)}
    b["p"], b["m"], b["v"] = (torch.randn(V, K, device=dev, generator=g) * 0.01 for _ in range(3))
    b["v"].abs_()
    b["pb"] = torch.zeros(V, K, dtype=torch.bfloat16, device=dev)
    b["pT"] = torch.zeros(K, Vp, dtype=torch.bfloat16, device=dev)
    b["sums"] = torch.full((2,), 4.0, device=dev)          # |g|^2 = 4 against clip 1: the clip bites
    b["ws"] = torch.zeros(2 * ((V + 127) // 128) * ((K + 127) // 128), device=dev)
    b["wsq"] = torch.zeros(2, device=dev)
    return b


STATE = ("p", "m", "v", "pb", "pT", "ws", "wsq", "sums")
for label, V, K, rows, apply in (("gates", 14148, 4096, 256, True), ("experts", 9432, 4096, 256, True),
                                 ("cfg4 gates", 14148, 1024, 512, False), ("cfg4 experts", 9432, 1024, 512, False)):
    b = buffers(V, K, rows, 7)
    start = {k: b[k].clone() for k in STATE}
    first = None
    for path, lib in libs:                                  # same inputs, one launch each: bit-for-bit against the first library
        for k in STATE:
            b[k].copy_(start[k])
        launch(lib, apply, b)
        torch.cuda.synchronize()
        got = {k: b[k].clone() for k in STATE}
        if first is None:
            first = got
        else:
            diff = [k for k in STATE if not torch.equal(got[k].view(torch.uint8), first[k].view(torch.uint8))]
            print("%-12s %s vs %s after one launch: %s" % (label, os.path.basename(path), os.path.basename(libs[0][0]),
                                                           "bit-identical (%s)" % ", ".join(STATE) if not diff else "DIFFERENT in " + ", ".join(diff)))
    del start, first
    n = V * K
    meds = {p: [] for p, _ in libs}
    for a in range(args.alternations):
        for path, lib in libs:
            launch(lib, apply, b)                           # warm-up of this library's code
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.launches)]
            for e0, e1 in ev:
                e0.record()
                launch(lib, apply, b)
                e1.record()
            torch.cuda.synchronize()
            us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
            med = statistics.median(us)
            meds[path].append(med)
            print("%-12s V=%5d K=%4d rows=%3d  %-22s alternation %d: median %.1f us  min %.1f us  (%.2f TB/s at 28 B/param, median)"
                  % (label, V, K, rows, os.path.basename(path), a + 1, med, us[0], n * 28 / med / 1e6))
    for path, _ in libs:
        mm = meds[path]
        print("%-12s %-22s medians %.1f .. %.1f us, median of medians %.1f us = %.2f TB/s"
              % (label, os.path.basename(path), min(mm), max(mm), statistics.median(mm), n * 28 / statistics.median(mm) / 1e6))
    del b
    torch.cuda.empty_cache()
