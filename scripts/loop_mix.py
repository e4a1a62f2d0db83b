#!/usr/bin/env python
"""Instruction mix of the MFMA loops of one .hip file (no GPU: hipcc cross-compiles).

    python scripts/loop_mix.py efficientvideoclassification_youtube8m_amd/csrc/evc_gemm_tn.hip [--count PREFIX ...] [--json] [-- extra hipcc flags]

Compiles the file device-only to assembly in a temporary directory (nothing is written into the tree) and prints, per kernel and per loop
whose own basic blocks hold MFMAs, how many instructions of each class one trip through the loop's text carries:

    mfma      v_mfma*
    valu      every other v_*
    ds        ds_*  (ds_asm: those inside inline-asm blocks - in the TN loops the transposing reads)
    salu      s_*   (waits and barriers included; barrier: s_barrier* alone)
    vmem      global_* / buffer_* / flat_*
    scratch   scratch_*  (a spill or its reload inside the loop)
    asm       inline-asm blocks (empty ones - compiler fences - included)

plus the kernel's .vgpr_count / .vgpr_spill_count / .sgpr_spill_count from the code object metadata.  Instructions are classified by mnemonic
PREFIX only; --count PREFIX adds a column that counts the mnemonics starting with PREFIX.  Loops and their blocks are taken from the
compiler's own block comments ("=>This Inner Loop Header", "in Loop: Header=BBx_y"): a block counts towards the innermost loop that holds
it.  A loop's text is every path through it - an if / else inside the loop counts both arms.

The ratio to look at is valu / mfma: a v_mfma_f32_16x16x32_bf16 holds the SIMD's vector issue for 8 of its 16 cycles and a plain VALU
instruction costs 4, so a loop above ~2 VALU per MFMA cannot keep the matrix pipe busy whatever the memory system does.
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc") or "hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S"]      # the compile flags of csrc/build.sh, to assembly

_FUNC = re.compile(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$")
_BLOCK = re.compile(r"^(?:(\.LBB\d+_\d+):|; %bb\.\d+:)\s*(;.*)?$")
_IN_LOOP = re.compile(r"in Loop: Header=(BB\d+_\d+)")
_INSN = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")
CLASSES = ("mfma", "valu", "ds", "ds_asm", "salu", "barrier", "vmem", "scratch", "asm")


def compile_to_asm(path, extra):
    with tempfile.TemporaryDirectory(prefix="loop_mix_") as tmp:
        out = os.path.join(tmp, "device.s")
        r = subprocess.run([HIPCC] + FLAGS + list(extra) + [os.path.abspath(path), "-o", out], capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("hipcc failed:\n" + r.stderr[-4000:])
        with open(out) as f:
            return f.read()


def classify(m):
    """Class of a mnemonic, by prefix."""
    if m.startswith("v_mfma"):
        return "mfma"
    if m.startswith("v_"):
        return "valu"
    if m.startswith("ds_"):
        return "ds"
    if m.startswith("s_"):
        return "salu"
    if m.startswith(("global_", "buffer_", "flat_")):
        return "vmem"
    if m.startswith("scratch_"):
        return "scratch"
    return None


def metadata(text):
    """kernel name -> {vgpr_count, vgpr_spill_count, sgpr_spill_count} from the amdhsa.kernels notes."""
    # (the keys of a kernel's entry are sorted: .agpr_count ... .sgpr_spill_count, .symbol, ... .vgpr_count, .vgpr_spill_count)
    meta, before, cur = {}, {}, None
    for line in text.splitlines():
        m = re.match(r"^-?\s*\.(\w+):\s+(.*)$", line.strip())
        if not m:
            continue
        k, v = m.group(1), m.group(2).strip().strip("'\"")
        if k in ("agpr_count", "sgpr_spill_count"):
            before[k] = int(v)
        elif k == "symbol" and v.endswith(".kd"):
            cur = meta[v[:-3]] = before
            before = {}
        elif k in ("vgpr_count", "vgpr_spill_count") and cur is not None:
            cur[k] = int(v)
    return meta


def loop_mix(text, prefixes=()):
    """[{kernel, loop, depth counts...}] for every loop whose own blocks hold MFMAs, in file order, and the metadata by kernel."""
    meta = metadata(text)
    kernels = set(meta)
    rows, func, loop, in_asm = [], None, None, False
    loops = {}                                   # (function, header) -> counts

    def bump(key, n=1):
        c = loops.setdefault((func, loop), dict.fromkeys(CLASSES + tuple(prefixes), 0))
        c[key] += n

    lines = text.splitlines()
    for i, line in enumerate(lines):
        m = _FUNC.match(line)
        if m and m.group(1) in kernels:
            func, loop, in_asm = m.group(1), None, False
            continue
        if func is None:
            continue
        if line.startswith(".Lfunc_end"):
            func = None
            continue
        m = _BLOCK.match(line)
        if m:
            note = m.group(2) or ""
            j = i + 1                            # the comment may run on over the next lines
            while j < len(lines) and lines[j].lstrip().startswith(";") and not _BLOCK.match(lines[j]) and "#ASM" not in lines[j]:
                note += lines[j]
                j += 1
            if "Loop Header" in note and m.group(1):
                loop = m.group(1)[2:]
            else:
                h = _IN_LOOP.search(note)
                loop = h.group(1) if h else None
            continue
        if "#ASMSTART" in line:
            in_asm = True
            if loop:
                bump("asm")
            continue
        if "#ASMEND" in line:
            in_asm = False
            continue
        m = _INSN.match(line)
        if not m or loop is None:
            continue
        mn = m.group(1)
        cls = classify(mn)
        if cls:
            bump(cls)
            if cls == "ds" and in_asm:
                bump("ds_asm")
            if mn.startswith("s_barrier"):
                bump("barrier")
        for p in prefixes:
            if mn.startswith(p):
                bump(p)
    for (f, h), c in loops.items():
        if c["mfma"] > 0:
            rows.append(dict(kernel=f, loop=h, **c))
    return rows, meta


def demangle(names):
    """Readable kernel names where a demangler is installed, the mangled ones otherwise."""
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    try:
        r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True) if tool and names else None
        out = r.stdout.splitlines() if r else []
        if names and len(out) == len(names):
            return dict(zip(names, [re.sub(r"\(GemmOperandsT.*$|\([^<>]*\)$", "", re.sub(r"^void ", "", o)) for o in out]))
    except (OSError, subprocess.CalledProcessError):
        pass
    return {n: n for n in names}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("source", help="a .hip file")
    ap.add_argument("--count", action="append", default=[], metavar="PREFIX", help="also count the mnemonics that start with PREFIX (repeatable)")
    ap.add_argument("--json", action="store_true", help="one JSON object instead of the tables")
    ap.add_argument("extra", nargs="*", help="extra hipcc flags (after --)")
    a = ap.parse_args(argv)
    rows, meta = loop_mix(compile_to_asm(a.source, a.extra), tuple(a.count))
    if a.json:
        print(json.dumps({"loops": rows, "kernels": meta}))
        return 0
    short = demangle(sorted(meta))
    cols = list(CLASSES) + list(a.count)
    print("%-66s %-10s %s  valu/mfma" % ("kernel", "loop", " ".join("%7s" % c for c in cols)))
    for r in rows:
        print("%-66s %-10s %s  %.2f" % (short[r["kernel"]][:66], r["loop"], " ".join("%7d" % r[c] for c in cols), r["valu"] / r["mfma"]))
    print()
    print("%-66s %5s %11s %11s" % ("kernel", "vgpr", "vgpr_spill", "sgpr_spill"))
    for k in sorted(meta):
        m = meta[k]
        print("%-66s %5d %11d %11d" % (short[k][:66], m.get("vgpr_count", -1), m.get("vgpr_spill_count", -1), m.get("sgpr_spill_count", -1)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
