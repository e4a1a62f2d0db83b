"""fwd_launch_record.py CSRC_DIR OUT_DIR: what the ten forward entries of CSRC_DIR/evc_lstm_fwd.hip enqueue, without a GPU.

The file is compiled for the host only and linked against scripts/fwd_launch_record.hip instead of the HIP runtime; the entries are then called with
fake, distinct pointers over a grid of shapes and forms (1 652 calls), one process per EVC_FORCE_TILE = 0 (unforced) ... 11, and every memset,
hoisted product and kernel launch is written to OUT_DIR/launches_<k>.txt with its geometry and arguments (of a two-tile launch's absent role and
of ldzx without zx nothing: the kernels read neither).  Two versions of the file enqueue the same work exactly when their logs are equal:

    python scripts/fwd_launch_record.py <parent checkout>/efficientvideoclassification_youtube8m_amd/csrc /tmp/a
    python scripts/fwd_launch_record.py efficientvideoclassification_youtube8m_amd/csrc /tmp/b && diff -r /tmp/a /tmp/b
"""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def build(csrc, out):
    """libfwd.so = host-only objects of evc_lstm_fwd.hip and the stand-in + placeholders for the fat binaries they refer to."""
    flags = ["--cuda-host-only", "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-w", "-I" + csrc, "-I" + os.path.join(csrc, "..", "..", "include")]
    objs = []
    for src in (os.path.join(csrc, "evc_lstm_fwd.hip"), os.path.join(ROOT, "scripts", "fwd_launch_record.hip")):
        objs.append(os.path.join(out, os.path.basename(src) + ".o"))
        subprocess.run([HIPCC] + flags + ["-c", src, "-o", objs[-1]], check=True)
    undefined = subprocess.run(["nm", "-u"] + objs, check=True, capture_output=True, text=True).stdout
    with open(os.path.join(out, "fatbin.c"), "w") as f:
        for i, sym in enumerate(sorted(set(re.findall(r"__hip_fatbin_[0-9a-f]+", undefined)))):
            f.write('char fatbin_%d[64] __asm__("%s");\n' % (i, sym))
    lib = os.path.join(out, "libfwd.so")
    subprocess.run(["g++", "-shared", "-fPIC"] + objs + [os.path.join(out, "fatbin.c"), "-o", lib], check=True)
    return lib


def drive(path):
    sys.path.insert(0, ROOT)
    from efficientvideoclassification_youtube8m_amd._lib import SIGNATURES
    lib = C.CDLL(path)
    for n, a in SIGNATURES.items():
        if "lstm" in n and "fwd" in n:
            f = getattr(lib, n)
            f.argtypes, f.restype = a, C.c_int
    _next = [0]

    def P():
        _next[0] += 1
        return 0x100000000 + _next[0] * 0x10000000
    def call(name, label, *args):
        lib.shim_note(("== %s %s" % (name, label)).encode())
        rc = getattr(lib, name)(*args, None)
        lib.shim_note(("rc %d" % rc).encode())
    def plans(T, M):
        yield "plain", None, None
        yield "planned", P(), (C.c_int32 * T)(*[M, (2 * M // 3) if T > 2 else M, 0][:T] if T > 1 else [M])
        yield "planned-full", P(), (C.c_int32 * T)(*([M] * T))
        yield "bad-plan", P(), (C.c_int32 * T)(*([M // 2] + [M] * (T - 1)))
    T = 3
    MS = (32, 330, 1000, 2000, 3700, 3800, 5120)
    for M, H, Kin in itertools.product(MS, (128, 1024), (64, 1152)):
        for lab, rm, rps in plans(T, M):
            _next[0] = 0
            st = (P(), P(), 2 * H)
            for hoist in (0, 1):
                call("evc_lstm_layer_fwd", "%d %d %d %s hoist=%d" % (M, H, Kin, lab, hoist), P(), P(), P(), P(), T, M, Kin, H, hoist, P(), P(), *st, P(), P(), rm, rps)
            for wide in (0, 1):
                call("evc_lstm_layer_fwd_f16", "%d %d %d %s wide=%d" % (M, H, Kin, lab, wide), P(), Kin + 8 * wide, P(), P(), P(), T, M, Kin, H, P(), wide, P(), *st, P(), P(), rm, rps)
            st2 = (P(), P(), P(), P(), 4 * H)
            call("evc_lstm_level2_fwd", "%d %d %d %s" % (M, H, Kin, lab), P(), P(), P(), P(), P(), P(), T, M, Kin, H, P(), P(), *st2, P(), P(), P(), P(), rm, rps)
            call("evc_lstm_level2_fwd", "%d %d %d %s no tapes" % (M, H, Kin, lab), P(), P(), P(), P(), P(), P(), T, M, Kin, H, P(), P(), *st2, None, None, None, None, rm, rps)
            if Kin == 1152:
                kx = Kin
                for h_lo, xint in itertools.product((0, 1), (0, 1)):
                    rs, cc, gap = (P(), P(), 128 * xint) if xint else (None, None, 0)
                    call("evc_lstm_layer_fwd_f16_fp8lo", "%d %d %s h_lo=%d xint=%d" % (M, H, lab, h_lo, xint), P(), kx * 3 // 2, kx, 2 * kx, kx, P(), P(), 17, h_lo, P(), P(), T, M, H, P(), P(), *st,
                         P(), P(), rm, rps, rs, cc, gap)
                    call("evc_lstm_level2_fwd_high", "%d %d %s h_lo=%d xint=%d" % (M, H, lab, h_lo, xint), P(), kx * 3 // 2, kx, 2 * kx, kx, P(), P(), 17, h_lo, P(), rs, cc, gap,
                         P(), 8 * H * H * (1 - xint), P(), P(), T, M, H, P(), P(), P(), P(), *st2, P(), P(), P(), P(), rm, rps)
                for kx8 in (0, kx):
                    call("evc_lstm_layer_fwd_f16_dith", "%d %d %s kx8=%d" % (M, H, lab, kx8), P(), kx * 3 // 2, kx, 2 * kx, kx8, P(), 4 * H * (kx + H), P() if kx8 else None, kx8 + 16, 24, P(), P(),
                         T, M, H, P(), P(), *st, P(), P(), rm, rps)
    for M, H, Kin in itertools.product((32, 70, 256, 1024, 2000, 3700, 3800), (128, 512, 1024), (64, 1152)):
        _next[0] = 0
        st, st2 = (P(), P(), 2 * H), (P(), P(), P(), P(), 4 * H)
        call("evc_lstm_layer_fwd_hp", "%d %d %d" % (M, H, Kin), P(), P(), 2 * Kin, P(), 2 * H, P(), P(), T, M, Kin, H, P(), P(), P(), *st, P(), P())
        call("evc_lstm_stack2_fwd", "%d %d %d" % (M, H, Kin), P(), P(), P(), P(), P(), P(), T, M, Kin, H, P(), P(), P(), *st2, P(), P(), P(), P())
        for seg, ext in itertools.product((1, 3), (0, 1)):
            call("evc_lstm_stack2_fwd_f16", "%d %d %d seg=%d ext=%d" % (M, H, Kin, seg, ext), P(), seg, P(), ext, P(), P(), P(), P(), T, M, Kin, H, P(), P(), P(), P(), P(), *st2, P(), P(), P(), P())
        for seg, h_lo in itertools.product((1, 2), (0, 1)):
            call("evc_lstm_stack2_fwd_f16_fp8lo", "%d %d %d seg=%d h_lo=%d" % (M, H, Kin, seg, h_lo), P(), seg, P(), P(), P(), P(), P(), 17, h_lo, P(), P(), T, M, Kin, H, P(), P(), P(), P(), P(),
                 *st2, P(), P(), P(), P())


if __name__ == "__main__":
    if sys.argv[1] == "--drive":
        drive(sys.argv[2])
    else:
        csrc, out = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
        os.makedirs(out, exist_ok=True)
        lib = build(csrc, out)
        for k in range(12):
            log = os.path.join(out, "launches_%d.txt" % k)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--drive", lib], check=True, env=dict(os.environ, EVC_FORCE_TILE=str(k), SHIM_LOG=log))
            print("tile %2d: %d calls, %d launches" % (k, sum(l.startswith("==") for l in open(log)), sum(l.startswith("launch") for l in open(log))))
        for f in os.listdir(out):
            if not f.startswith("launches_"):
                os.remove(os.path.join(out, f))
