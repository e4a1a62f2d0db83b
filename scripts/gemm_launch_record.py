"""gemm_launch_record.py CSRC_DIR OUT_DIR [--keep]: what the NT and TN product entries of CSRC_DIR/evc_gemm.hip and evc_gemm_tn.hip enqueue, without a GPU.

Both files are compiled for the host only and linked against scripts/gemm_launch_record.hip instead of the HIP runtime; the entries are then called
with fake pointers over a grid of shapes, flags, strides and refusals, one process per EVC_FORCE_TILE = 0 (unforced) ... 11 crossed with
EVC_DETERMINISTIC unset / 1 (both are read once per process), and every memset, LDS attribute and kernel launch is written to
OUT_DIR/launches_<tile>_<det>.txt with its geometry, every field of its operand and store structs, the call's return code and its error text.  Two
versions of the files enqueue the same work exactly when their logs are equal:

    python scripts/gemm_launch_record.py <parent checkout>/efficientvideoclassification_youtube8m_amd/csrc /tmp/a
    python scripts/gemm_launch_record.py efficientvideoclassification_youtube8m_amd/csrc /tmp/b && diff -r /tmp/a /tmp/b
"""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ENTRIES = ("evc_gemm_nt", "evc_gemm_nt_sqnorm", "evc_gemm_nt_split", "evc_gemm_nt_f16_fp8", "evc_gemm_nt_f16_fp8_dyn", "evc_gemm_tn", "evc_gemm_tn2",
           "evc_gemm_tn2_rows", "evc_gemm_tn_slabs", "evc_gemm_tn2_slabs", "evc_sum_slabs", "evc_gemm_tn2_rows_skip", "evc_gemm_tn2_slabs_skip")


def build(csrc, out):
    """libgemm.so = host-only objects of the two product files and the stand-in + placeholders for the fat binaries they refer to."""
    flags = ["--cuda-host-only", "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-w", "-I" + csrc, "-I" + os.path.join(csrc, "..", "..", "include")]
    objs = []
    for src in (os.path.join(csrc, "evc_gemm.hip"), os.path.join(csrc, "evc_gemm_tn.hip"), os.path.join(ROOT, "scripts", "gemm_launch_record.hip")):
        objs.append(os.path.join(out, os.path.basename(src) + ".o"))
        subprocess.run([HIPCC] + flags + ["-c", src, "-o", objs[-1]], check=True)
    undefined = subprocess.run(["nm", "-u"] + objs, check=True, capture_output=True, text=True).stdout
    with open(os.path.join(out, "fatbin.c"), "w") as f:
        for i, sym in enumerate(sorted(set(re.findall(r"__hip_fatbin_[0-9a-f]+", undefined)))):
            f.write('char fatbin_%d[64] __asm__("%s");\n' % (i, sym))
    lib = os.path.join(out, "libgemm.so")
    subprocess.run(["g++", "-shared", "-fPIC"] + objs + [os.path.join(out, "fatbin.c"), "-o", lib], check=True)
    return lib


def bind(path):
    sys.path.insert(0, ROOT)
    from efficientvideoclassification_youtube8m_amd._lib import SIGNATURES
    lib = C.CDLL(path)
    for n in ENTRIES + ("evc_gemm_tn_plan",):
        f = getattr(lib, n)
        f.argtypes, f.restype = SIGNATURES[n], C.c_int
    lib.shim_err.restype = C.c_char_p
    return lib


def drive_skip(lib):
    """The skip entries, each launch behind the answer of evc_gemm_tn_plan for the same arguments ("plan tile=.. splits=.. live_walk=.."): over the
    live-slab tables of the evc_gemm_tn2_rows grid and the plain walk, k_skip = 0, one step, slab 0, everything."""
    A, B, Cp, B2 = [0x100000000 * (i + 1) for i in (0, 1, 2, 10)]

    def table(v):
        return (C.c_int32 * len(v))(*v) if v is not None else None

    def note(text):
        lib.shim_note(text.encode())
        lib.shim_clear_err()

    for M, N1, N2, sr in itertools.product((128, 1024, 4096), (128, 256, 1024), (0, 256), (32, 256, 2048)):
        tabs = [("plain", None, 5), ("live", [sr] * 5, 5), ("dead", [0] * 5, 5), ("part", [sr, sr // 2, 1, 0, 0], 5), ("odd", [-3, sr + 7, 40, 0, sr], 5),
                ("17", [1] * 17 + [0] * 3, 20), ("16", [sr] * 16 + [0] * 4, 20), ("one", [5], 1), ("long", [sr] * 3 + [sr // 2] * 40, 43)]
        for (lab, v, ns), kf in itertools.product(tabs, (0, 1, "slab", "all", "over", -1)):
            ks = {"slab": sr // 32, "all": sr // 32 * ns, "over": sr // 32 * ns + 1}.get(kf, kf)
            label = "%d %d+%d sr=%d %s k_skip=%d" % (M, N1, N2, sr, lab, ks)
            tile, splits, walk = C.c_int(-1), C.c_int(-1), C.c_int(-1)
            note("== evc_gemm_tn_plan " + label)
            rc = lib.evc_gemm_tn_plan(M, N1, N1, N2 + 8, N2, M, sr, ns, table(v), ks, C.byref(tile), C.byref(splits), C.byref(walk))
            lib.shim_note(("rc %d %s\nplan tile=%d splits=%d live_walk=%d" % (rc, lib.shim_err().decode(), tile.value, splits.value, walk.value)).encode())
            for acc, H in ((0, 0), (1, M // 4)):
                note("== evc_gemm_tn2_rows_skip %s acc=%d H=%d" % (label, acc, H))
                rc = lib.evc_gemm_tn2_rows_skip(A, M, B, N1, N1, B2 if N2 else None, N2 + 8, N2, N1, Cp, N1 + N2, M, sr, ns, table(v), ks, H, acc, None)
                lib.shim_note(("rc %d %s" % (rc, lib.shim_err().decode())).encode())
    for M, N, K, ns, ks in itertools.product((256, 4096), (136, 1152), (1024, 10240), (1, 3, 32), (0, 1, 8, 31, 32, 320, 321)):
        for n2, H in ((0, 0), (256, M // 4)):
            note("== evc_gemm_tn2_slabs_skip %d %d+%d %d nslab=%d k_skip=%d H=%d" % (M, N, n2, K, ns, ks, H))
            rc = lib.evc_gemm_tn2_slabs_skip(A, M, B, N, N, B2 if n2 else None, n2 + 8, n2, N + 64, Cp, N + n2 + 64, M * (N + n2 + 64), M, K, ks, H, ns, None)
            lib.shim_note(("rc %d %s" % (rc, lib.shim_err().decode())).encode())


def drive(path):
    lib = bind(path)
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    lib.shim_gemm_nt_f16.argtypes, lib.shim_gemm_nt_f16.restype = [vp, i64, vp, i64, vp, i64, i32, i32, i32, vp], C.c_int
    # fake operands, 4 GiB apart
    A, B, Cp, BIAS, P_, SUMS, WS, A8, B8, AMAX, B2 = [0x100000000 * (i + 1) for i in range(11)]

    def call(name, label, *args):
        lib.shim_note(("== %s %s" % (name, label)).encode())
        lib.shim_clear_err()
        rc = getattr(lib, name)(*args, None)
        lib.shim_note(("rc %d %s" % (rc, lib.shim_err().decode())).encode())

    MS = (1, 64, 200, 256, 257, 300, 512, 513, 600, 1000, 1280, 2000, 4716, 5120, 14148, 56640)
    NS = (5, 64, 128, 130, 256, 264, 300, 1024, 1152, 4096, 14148)
    KS = (0, 64, 192, 1024, 2048, 4096, 8192, 16384)
    # ---- evc_gemm_nt: every flag combination (the refused out_bf16 + accumulate pair included), ldc = N and N + 1
    for M, N, K in itertools.product(MS, NS, KS):
        for bias, ob, acc in itertools.product((0, 1), repeat=3):
            call("evc_gemm_nt", "%d %d %d bias=%d ob=%d acc=%d" % (M, N, K, bias, ob, acc), A, K, B, K, Cp, N, M, N, K, BIAS if bias else None, ob, acc)
        for ob in (0, 1):
            call("evc_gemm_nt", "%d %d %d ldc=N+1 ob=%d" % (M, N, K, ob), A, K, B, K, Cp, N + 1, M, N, K, None, ob, 0)
    # its refusals: bad shapes, K not a multiple of 64, misaligned pointers and strides, operands of 4 GiB or more
    for M, N, K, lda, ldb, da, db in ((0, 64, 64, 64, 64, 0, 0), (64, 0, 64, 64, 64, 0, 0), (64, 64, -64, 64, 64, 0, 0), (64, 64, 96, 96, 96, 0, 0), (64, 64, 64, 60, 64, 0, 0),
                                      (64, 64, 64, 64, 68, 0, 0), (64, 64, 64, 64, 64, 2, 0), (64, 64, 64, 64, 64, 0, 8), (1 << 24, 64, 64, 64, 64, 0, 0),
                                      (64, 1 << 24, 64, 64, 64, 0, 0), (64, 64, 64, 1 << 23, 64, 0, 0), (64, 64, 64, 64, 1 << 23, 0, 0), (56640, 64, 64, 65536, 64, 0, 0),
                                      (64, 56640, 64, 64, 65536, 0, 0), ((1 << 24) - 1, 64, 64, 64, 64, 0, 0)):
        call("evc_gemm_nt", "refusal %d %d %d lda=%d ldb=%d +%d +%d" % (M, N, K, lda, ldb, da, db), A + da, lda, B + db, ldb, Cp, N, M, N, K, None, 0, 0)
    # ---- evc_gemm_nt_sqnorm: inside each clause of its precondition and just outside, P present / absent / misaligned
    f32 = C.c_float
    for M, N, K in itertools.product((512, 513, 600, 1000, 5120), (256, 264, 300, 1024, 4096), (1024, 4096, 8128, 8192)):
        slots = 2 * 8 * ((M + 127) // 128) * ((N + 127) // 128)
        for ldc, dc in ((N, 0), (N + 1, 0), (N + 4, 0), (N, 4)):
            for p, dp, l2 in ((0, 0, 0.0), (1, 0, 0.5), (1, 4, 0.5), (0, 0, 0.5)):
                call("evc_gemm_nt_sqnorm", "%d %d %d ldc=%d +%d P=%d +%d l2=%g" % (M, N, K, ldc, dc, p, dp, l2), A, K, B, K, Cp + dc, ldc, M, N, K, P_ + dp if p else None, f32(l2),
                     SUMS, WS, slots)
        call("evc_gemm_nt_sqnorm", "%d %d %d short ws" % (M, N, K), A, K, B, K, Cp, N, M, N, K, None, f32(0), SUMS, WS, slots - 1)
        call("evc_gemm_nt_sqnorm", "%d %d %d no sums" % (M, N, K), A, K, B, K, Cp, N, M, N, K, None, f32(0), None, WS, slots)
        call("evc_gemm_nt_sqnorm", "%d %d %d no ws" % (M, N, K), A, K, B, K, Cp, N, M, N, K, None, f32(0), SUMS, None, slots)
    # ---- evc_gemm_nt_split and the internal f16 product over the same M and N
    for M, N, K in itertools.product(MS, NS, (64, 1024, 2048, 4096)):
        for bias in (0, 1):
            call("evc_gemm_nt_split", "%d %d %d bias=%d" % (M, N, K, bias), A, 2 * K, B, 2 * K + 8, Cp, N, M, N, K, BIAS if bias else None)
        call("shim_gemm_nt_f16", "%d %d %d" % (M, N, K), A, K, B, K + 8, Cp, N, M, N, K)
    for M, N, K, lda, ldb, da in ((0, 64, 64, 128, 128, 0), (64, 64, 0, 128, 128, 0), (64, 64, 96, 192, 192, 0), (64, 64, 64, 120, 128, 0), (64, 64, 64, 128, 124, 0),
                                  (64, 64, 64, 128, 128, 2), (1 << 24, 64, 64, 128, 128, 0), (64, 64, 64, 1 << 23, 128, 0), (56640, 64, 64, 65536, 128, 0)):
        call("evc_gemm_nt_split", "refusal %d %d %d lda=%d ldb=%d +%d" % (M, N, K, lda, ldb, da), A + da, lda, B, ldb, Cp, N, M, N, K, None)
        call("shim_gemm_nt_f16", "refusal %d %d %d lda=%d ldb=%d +%d" % (M, N, K, lda, ldb, da), A + da, lda, B, ldb, Cp, N, M, N, K)
    # ---- evc_gemm_nt_f16_fp8 and its _dyn form
    for M, N, (K16, K8) in itertools.product((1, 200, 256, 257, 512, 513, 2000, 5120), (5, 64, 130, 1024, 4096, 14148), ((64, 512), (512, 1024), (1024, 2048), (4096, 8192), (8192, 16384))):
        for bias in (0, 1):
            call("evc_gemm_nt_f16_fp8", "%d %d %d %d bias=%d" % (M, N, K16, K8, bias), A, K16, A8, K8, B, K16, B8, K8 + 16, Cp, N, M, N, K16, K8, -24, BIAS if bias else None)
        call("evc_gemm_nt_f16_fp8_dyn", "%d %d %d %d" % (M, N, K16, K8), A, K16, A8, K8, B, K16, B8, K8, Cp, N + 1, M, N, K16, K8, -24, AMAX, 17, None)
    for se in (-61, -60, 60, 61):
        call("evc_gemm_nt_f16_fp8", "scale_exp=%d" % se, A, 64, A8, 512, B, 64, B8, 512, Cp, 64, 64, 64, 64, 512, se, None)
    for hx, am in ((-31, AMAX), (-30, AMAX), (30, AMAX), (31, AMAX), (0, None)):
        call("evc_gemm_nt_f16_fp8_dyn", "a8_hi_exp=%d amax=%s" % (hx, bool(am)), A, 64, A8, 512, B, 64, B8, 512, Cp, 64, 64, 64, 64, 512, 0, am, hx, None)
    for lab, a16, lda, a8, lda8, b16, b8, c, M, K16, K8 in (("K16=96", A, 96, A8, 512, B, B8, Cp, 64, 96, 512), ("K8=384", A, 64, A8, 384, B, B8, Cp, 64, 64, 384),
                                                          ("K8=576", A, 64, A8, 576, B, B8, Cp, 64, 64, 576), ("M=0", A, 64, A8, 512, B, B8, Cp, 0, 64, 512),
                                                          ("A16 NULL", None, 64, A8, 512, B, B8, Cp, 64, 64, 512), ("B8 NULL", A, 64, A8, 512, B, None, Cp, 64, 64, 512),
                                                          ("C NULL", A, 64, A8, 512, B, B8, None, 64, 64, 512), ("lda=60", A, 60, A8, 512, B, B8, Cp, 64, 64, 512),
                                                          ("lda8=520", A, 64, A8, 520, B, B8, Cp, 64, 64, 512), ("lda8<K8", A, 64, A8, 496, B, B8, Cp, 64, 64, 512),
                                                          ("A8+8", A, 64, A8 + 8, 512, B, B8, Cp, 64, 64, 512), ("M=2^24", A, 64, A8, 512, B, B8, Cp, 1 << 24, 64, 512),
                                                          ("lda=2^23", A, 1 << 23, A8, 512, B, B8, Cp, 64, 64, 512), ("lda8=2^24", A, 64, A8, 1 << 24, B, B8, Cp, 64, 64, 512)):
        call("evc_gemm_nt_f16_fp8", "refusal " + lab, a16, lda, a8, lda8, b16, 64, b8, 512, c, 64, M, 64, K16, K8, 0, None)
    # ---- TN products
    TM, TN_, TK = (8, 128, 256, 1024, 4096, 4104), (8, 128, 136, 256, 1152, 2176), (32, 1024, 1280, 2048, 4096, 10240, 16384)
    for M, N, K in itertools.product(TM, TN_, TK):
        for H, acc in itertools.product((0, M // 4, M // 4 + 1), (0, 1)):
            call("evc_gemm_tn", "%d %d %d H=%d acc=%d" % (M, N, K, H, acc), A, M, B, N + 8, Cp, N, M, N, K, H, acc)
        call("evc_gemm_tn", "%d %d %d ldc=N+1" % (M, N, K), A, M, B, N, Cp, N + 1, M, N, K, 0, 0)
    for M, N, K, lda, ldb, da, db in ((4, 64, 64, 64, 64, 0, 0), (64, 4, 64, 64, 64, 0, 0), (60, 64, 64, 64, 64, 0, 0), (64, 60, 64, 64, 64, 0, 0), (64, 64, 0, 64, 64, 0, 0),
                                      (64, 64, 96, 64, 64, 0, 0), (64, 64, 80, 64, 64, 0, 0), (64, 64, 64, 60, 64, 0, 0), (64, 64, 64, 64, 60, 0, 0), (64, 64, 64, 64, 64, 2, 0),
                                      (64, 64, 64, 64, 64, 0, 2)):
        call("evc_gemm_tn", "refusal %d %d %d lda=%d ldb=%d +%d +%d" % (M, N, K, lda, ldb, da, db), A + da, lda, B + db, ldb, Cp, N, M, N, K, 0, 0)
    # two column segments: adjacent in C and not, N1 not a multiple of 256, missing segments, a misaligned second segment
    for M, K, N1, N2 in itertools.product((128, 1024, 4096), (1024, 2048, 10240), (256, 1024, 128, 384), (128, 256, 1152)):
        for gap, acc, H in itertools.product((0, 64), (0, 1), (0, M // 4)):
            call("evc_gemm_tn2", "%d %d+%d %d gap=%d acc=%d H=%d" % (M, N1, N2, K, gap, acc, H), A, M, B, N1, N1, B2, N2 + 8, N2, N1 + gap, Cp, N1 + N2 + gap, M, K, H, acc)
    for lab, b1, b2, n1, n2, ldb2, col2 in (("B1 NULL", None, B2, 256, 256, 256, 256), ("B2 NULL", B, None, 256, 256, 256, 256), ("N1=0", B, B2, 0, 256, 256, 0),
                                            ("N2=0", B, B2, 256, 0, 256, 256), ("B2+2", B, B2 + 2, 256, 256, 256, 256), ("ldb2=260", B, B2, 256, 256, 260, 256),
                                            ("c_col2<N1", B, B2, 256, 256, 256, 128)):
        call("evc_gemm_tn2", "refusal " + lab, A, 64, b1, 256, n1, b2, ldb2, n2, col2, Cp, 1024, 64, 1024, 0, 1)
    # live-slab tables (host memory): all live, all dead, partly live, negative and over-full entries, 17 non-empty slabs, past the 32-bit byte offset
    def table(v):
        return (C.c_int32 * len(v))(*v)
    for M, N1, N2, sr in itertools.product((128, 1024, 4096), (128, 256, 1024), (0, 256), (32, 256, 2048)):
        tabs = [("live", [sr] * 5), ("dead", [0] * 5), ("part", [sr, sr // 2, 1, 0, 0]), ("odd", [-3, sr + 7, 40, 0, sr]), ("17", [1] * 17 + [0] * 3), ("16", [sr] * 16 + [0] * 4),
                ("one", [5])]
        for lab, v in tabs:
            for acc, H in ((0, 0), (1, M // 4)):
                call("evc_gemm_tn2_rows", "%d %d+%d sr=%d %s acc=%d H=%d" % (M, N1, N2, sr, lab, acc, H), A, M, B, N1, N1, B2 if N2 else None, N2, N2, N1, Cp, N1 + N2, M, sr, len(v), table(v),
                     H, acc)
    call("evc_gemm_tn2_rows", "4 GiB", A, 16384, B, 128, 128, None, 0, 0, 128, Cp, 128, 128, 4096, 32, table([4096] * 8 + [0] * 24), 0, 0)
    call("evc_gemm_tn2_rows", "just under 4 GiB", A, 16376, B, 128, 128, None, 0, 0, 128, Cp, 128, 128, 4096, 32, table([4096] * 8 + [0] * 24), 0, 0)
    call("evc_gemm_tn2_rows", "65536 steps", A, 128, B, 128, 128, None, 0, 0, 128, Cp, 128, 128, 131072, 16, table([64] * 16), 0, 0)
    call("evc_gemm_tn2_rows", "slab_rows=48", A, 128, B, 128, 128, None, 0, 0, 128, Cp, 128, 128, 48, 4, table([48, 0, 0, 0]), 0, 0)
    for lab, b1, n1, sr, ns, tab, b2, n2, col2, acc in (("B1 NULL", None, 128, 32, 4, table([1] * 4), None, 0, 0, 0), ("N1=0", B, 0, 32, 4, table([1] * 4), None, 0, 0, 0),
                                                        ("slab_rows=0", B, 128, 0, 4, table([1] * 4), None, 0, 0, 0), ("nslabs=0", B, 128, 32, 0, table([1] * 4), None, 0, 0, 0),
                                                        ("no table", B, 128, 32, 4, None, None, 0, 0, 0), ("2^31 rows", B, 128, 1 << 20, 1 << 11, table([1] * 4), None, 0, 0, 0),
                                                        ("N2=0", B, 256, 32, 4, table([1] * 4), B2, 0, 256, 0), ("apart", B, 256, 32, 4, table([1] * 4), B2, 256, 320, 0),
                                                        ("apart acc", B, 256, 32, 4, table([1] * 4), B2, 256, 320, 1)):
        call("evc_gemm_tn2_rows", "refusal " + lab, A, 128, b1, 256, n1, b2, 256, n2, col2, Cp, 1024, 128, sr, ns, tab, 0, acc)
    # K split into slabs
    for M, N, K, ns in itertools.product((8, 256, 4096, 4104), (8, 136, 1152, 2176), (32, 1024, 10240), (1, 3, 32, 33, 0)):
        call("evc_gemm_tn_slabs", "%d %d %d nslab=%d" % (M, N, K, ns), A, M, B, N, Cp, M, N, K, ns)
        for n2, H in itertools.product((0, 256), (0, M // 4, 3)):
            call("evc_gemm_tn2_slabs", "%d %d+%d %d nslab=%d H=%d" % (M, N, n2, K, ns, H), A, M, B, N, N, B2 if n2 else None, n2 + 8, n2, N + 64, Cp, N + n2 + 64, M * (N + n2 + 64), M, K, H, ns)
    call("evc_gemm_tn_slabs", "empty slab", A, 64, B, 64, Cp, 64, 64, 160, 4)
    call("evc_gemm_tn2_slabs", "empty slab", A, 64, B, 64, 64, None, 0, 0, 0, Cp, 64, 64 * 64, 64, 160, 0, 4)
    for lab, M, N, K, lda, ldb, da in (("M=60", 60, 64, 64, 64, 64, 0), ("K=96", 64, 64, 96, 64, 64, 0), ("K=80", 64, 64, 80, 64, 64, 0), ("lda=60", 64, 64, 64, 60, 64, 0),
                                       ("ldb=60", 64, 64, 64, 64, 60, 0), ("A+2", 64, 64, 64, 64, 64, 2)):
        call("evc_gemm_tn_slabs", "refusal " + lab, A + da, lda, B, ldb, Cp, M, N, K, 1)
        call("evc_gemm_tn2_slabs", "refusal " + lab, A + da, lda, B, ldb, N, None, 0, 0, 0, Cp, N, M * N, M, K, 0, 1)
    for lab, s_, stride, n1, b2, n2, ldb2, col2 in (("no slabs", None, 64 * 1024, 256, B2, 256, 256, 256), ("short stride", Cp, 64 * 1024 - 4, 256, B2, 256, 256, 256),
                                                    ("N1=128", Cp, 64 * 1024, 128, B2, 256, 256, 128), ("N2=0", Cp, 64 * 1024, 256, B2, 0, 256, 256),
                                                    ("B2+2", Cp, 64 * 1024, 256, B2 + 2, 256, 256, 256), ("ldb2=260", Cp, 64 * 1024, 256, B2, 256, 260, 256),
                                                    ("c_col2<N1", Cp, 64 * 1024, 256, B2, 256, 256, 128), ("N1=4", Cp, 64 * 1024, 4, None, 0, 0, 0)):
        call("evc_gemm_tn2_slabs", "refusal " + lab, A, 64, B, 256, n1, b2, ldb2, n2, col2, s_, 1024, stride, 64, 1024, 0, 2)
    for M, N, ns, acc in itertools.product((1, 8, 4096), (4, 1152, 2176), (1, 3, 32), (0, 1)):
        call("evc_sum_slabs", "%d %d nslab=%d acc=%d" % (M, N, ns, acc), WS, M * (N + 4), ns, M, N, N + 4, Cp, N, acc)
    for lab, s_, stride, ns, M, N, ld, c, ldc in (("no slabs", None, 64, 1, 8, 8, 8, Cp, 8), ("no C", WS, 64, 1, 8, 8, 8, None, 8), ("nslab=0", WS, 64, 0, 8, 8, 8, Cp, 8),
                                                  ("M=0", WS, 64, 1, 0, 8, 8, Cp, 8), ("N=6", WS, 64, 1, 8, 6, 8, Cp, 8), ("ld=6", WS, 64, 1, 8, 8, 6, Cp, 8),
                                                  ("ldc=10", WS, 64, 1, 8, 8, 8, Cp, 10), ("stride=66", WS, 66, 1, 8, 8, 8, Cp, 8), ("slabs+4", WS + 4, 64, 1, 8, 8, 8, Cp, 8),
                                                  ("C+8", WS, 64, 1, 8, 8, 8, Cp + 8, 8)):
        call("evc_sum_slabs", "refusal " + lab, s_, stride, ns, M, N, ld, c, ldc, 0)
    # ---- the skip entries and the plan query, behind everything else: the log of a tree without them is the head of this one
    drive_skip(lib)


if __name__ == "__main__":
    if sys.argv[1] == "--drive":
        drive(sys.argv[2])
    elif sys.argv[1] == "--drive-skip":      # that part alone (tests/test_cpu_tn_plan.py)
        drive_skip(bind(sys.argv[2]))
    else:
        csrc, out = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
        os.makedirs(out, exist_ok=True)
        lib = build(csrc, out)
        for k, det in itertools.product(range(12), (0, 1)):
            log = os.path.join(out, "launches_%d_%d.txt" % (k, det))
            env = dict(os.environ, EVC_FORCE_TILE=str(k), SHIM_LOG=log)
            env.pop("EVC_DETERMINISTIC", None)
            if det:
                env["EVC_DETERMINISTIC"] = "1"
            subprocess.run([sys.executable, os.path.abspath(__file__), "--drive", lib], check=True, env=env)
            print("tile %2d det %d: %d calls, %d launches, %d refusals" % (k, det, sum(l.startswith("==") for l in open(log)), sum(l.startswith("launch") for l in open(log)),
                                                                         sum(l.startswith("rc ") and not l.startswith("rc 0") for l in open(log))))
        for f in os.listdir(out):
            if not f.startswith("launches_") and "--keep" not in sys.argv:      # (--keep: libgemm.so stays, for --drive-skip)
                os.remove(os.path.join(out, f))
