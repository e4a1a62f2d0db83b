"""scripts/loop_mix.py on csrc/evc_gemm_tn.hip (no GPU; needs hipcc, which cross-compiles): the instruction mix of the TN loops.

The bound, for every loop that holds both MFMAs and transposing reads: other VALU <= transposing reads / 2 + 4 - one add per fragment (slot base +
lane offset; the fragment's second read, the A / B half of the stage and whatever else is constant ride in the reads' immediates), two reads per
fragment, four instructions for the loop's own bookkeeping - and no scratch access (a spill or its reload) inside the loop.

Every kernel has its loop four times: steady state and tail, each in the copy of the waves that only read and multiply and in the copy of the waves
that also issue the stage's LDS-DMA (gemm_core_tn.h, run()).  Figures (two K steps per trip; VALU / bound; in brackets the tree before the immediates):

    gemm_tn_kernel 256 x 256, all four loops, SEG and plain      24 / 28   (read-only loops 80; LDS-DMA loops 96 plain, 208 and 223 SEG)
    gemm_tn_kernel 128 x 128, all four loops, SEG and plain      12 / 16   (40; 48, 160 and 167)
    moe_update_kernel 128 x 128 (every wave stages)              12 / 16   (36)

The LDS-DMA loops meet the bound because the staging issues buffer loads whose K walk is the instruction's scalar offset (no per-piece VALU add) and
the segment switch of the SEG walk is held in scalar registers (gemm_core_tn.h: tn_load_lds16, advance()).
"""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import loop_mix  # noqa: E402

SRC = os.path.join(ROOT, "efficientvideoclassification_youtube8m_amd", "csrc", "evc_gemm_tn.hip")
TR = "ds_read_b64_tr"

needs_hipcc = pytest.mark.skipif(not (os.path.exists(loop_mix.HIPCC) or shutil.which(loop_mix.HIPCC)), reason="hipcc is absent")


@pytest.fixture(scope="module")
def mix():
    """One compile for the module, through the command line as a user runs it."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "loop_mix.py"), SRC, "--count", TR, "--json"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout)
    loops = [l for l in out["loops"] if l["mfma"] > 0 and l[TR] > 0]
    for l in loops:
        print("%-100s %-9s mfma %3d valu %3d reads %3d vmem %2d scratch %d" % (l["kernel"][:100], l["loop"], l["mfma"], l["valu"], l[TR], l["vmem"], l["scratch"]))
    return out, loops


def _over(loops):
    return ["%s %s: %d other VALU > %d reads / 2 + 4 = %d" % (l["kernel"], l["loop"], l["valu"], l[TR], l[TR] // 2 + 4)
            for l in loops if l["valu"] > l[TR] // 2 + 4]


@needs_hipcc
def test_every_tn_kernel_has_its_loops(mix):
    """Four gemm_tn_kernel and two moe_update_kernel instantiations; the transposing reads are all inside inline asm, two per fragment."""
    out, loops = mix
    kernels = sorted({l["kernel"] for l in loops})
    assert sum("gemm_tn_kernel" in k for k in kernels) == 4 and sum("moe_update_kernel" in k for k in kernels) == 2, kernels
    for k in kernels:
        n = sum(l["kernel"] == k for l in loops)
        assert n == (4 if "gemm_tn_kernel" in k else 2), (k, n)
        assert set(out["kernels"][k]) >= {"vgpr_count", "vgpr_spill_count"}
    for l in loops:
        assert l[TR] == l["ds_asm"] == l["ds"] and l[TR] % 2 == 0 and l["barrier"] == 2, l


@needs_hipcc
def test_no_spill_inside_a_loop(mix):
    _, loops = mix
    assert not [l for l in loops if l["scratch"]], [(l["kernel"], l["loop"], l["scratch"]) for l in loops if l["scratch"]]


@needs_hipcc
def test_read_only_loops_one_add_per_fragment(mix):
    """The loops of the waves that issue no LDS-DMA: nothing but the read addresses is computed on the VALU."""
    _, loops = mix
    part = [l for l in loops if l["vmem"] == 0]
    assert len(part) == 8, len(part)
    assert not _over(part), "\n".join(_over(part))


@needs_hipcc
def test_lds_dma_loops_one_add_per_fragment(mix):
    """The loops that also issue the LDS-DMA, same bound (see the module docstring for the figures)."""
    _, loops = mix
    part = [l for l in loops if l["vmem"] > 0]
    assert len(part) == 12, len(part)
    assert not _over(part), "\n".join(_over(part))


def test_parser_on_a_hand_written_listing():
    """The parser alone (no compiler): blocks count towards the innermost loop that holds them, by the compiler's block comments."""
    text = "\n".join([
        "k1:                                     ; @k1",
        "; %bb.0:",
        "\tv_add_u32_e32 v1, s0, v0",
        ".LBB0_1:                                ; =>This Loop Header: Depth=1",
        "\tv_mfma_f32_16x16x32_bf16 v[0:3], v[4:7], v[8:11], v[0:3]",
        "\tv_add_u32_e32 v1, s0, v0",
        "\t;;#ASMSTART",
        "\tds_read_b64_tr_b16 v[4:5], v1 offset:0x800",
        "\t;;#ASMEND",
        "\ts_barrier",
        ".LBB0_2:                                ;   Parent Loop BB0_1 Depth=1",
        "                                        ; =>  This Inner Loop Header: Depth=2",
        "\tv_mov_b32_e32 v9, v8",
        "\ts_cbranch_scc1 .LBB0_2",
        "; %bb.3:                                ;   in Loop: Header=BB0_1 Depth=1",
        "\tscratch_load_dword v7, off, off",
        "\ts_cbranch_scc1 .LBB0_1",
        "; %bb.4:",
        "\tv_mov_b32_e32 v9, v8",
        "\ts_endpgm",
        ".Lfunc_end0:",
        "amdhsa.kernels:",
        "  - .agpr_count:     0",
        "    .name:           k1",
        "    .sgpr_spill_count: 0",
        "    .symbol:         k1.kd",
        "    .vgpr_count:     12",
        "    .vgpr_spill_count: 1",
    ])
    rows, meta = loop_mix.loop_mix(text, ("ds_read_b64_tr",))
    assert meta == {"k1": {"agpr_count": 0, "sgpr_spill_count": 0, "vgpr_count": 12, "vgpr_spill_count": 1}}
    assert len(rows) == 1
    r = rows[0]
    assert (r["kernel"], r["loop"]) == ("k1", "BB0_1")
    assert (r["mfma"], r["valu"], r["ds"], r["ds_asm"], r["ds_read_b64_tr"], r["salu"], r["barrier"], r["scratch"], r["asm"]) == (1, 1, 1, 1, 1, 2, 1, 1, 1)
