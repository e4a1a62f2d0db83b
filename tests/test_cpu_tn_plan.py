"""evc_gemm_tn_plan against what the launch does, without a GPU: scripts/gemm_launch_record.py builds the TN host code against a recording
stand-in for the HIP runtime and drives the skip entries over its shape grid, each launch behind the plan query's answer for the same
arguments.  Checked per launch: the plan's tile and splits are the launch's; no atomic split of either column segment is empty; they keep at
least 32 K steps in every tile; a skip never reaches past the walk.  Under EVC_FORCE_TILE=11 and EVC_DETERMINISTIC=1 too (read once per
process: one driver process each)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "scripts", "gemm_launch_record.py")
LDS = {163840: 1, 81920: 11}          # dynamic LDS of the 256 x 256 / 128 x 128 ring tile -> the tile id evc_gemm_tn_plan reports


@pytest.fixture(scope="module")
def recorder(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tn_plan"))
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gemm_launch_record as rec
    return rec.build(os.path.join(ROOT, "efficientvideoclassification_youtube8m_amd", "csrc"), out), out


def _blocks(log):
    """[(header line, lines up to and including its rc line)]"""
    blocks, cur = [], None
    for line in open(log).read().split("\n"):
        if line.startswith("== "):
            cur = (line, [])
            blocks.append(cur)
        elif cur is not None:
            cur[1].append(line)
    return blocks


@pytest.mark.parametrize("tile,det", [(0, 0), (11, 0), (0, 1)])
def test_plan_query_is_the_launch(recorder, tile, det):
    lib, out = recorder
    log = os.path.join(out, "skip_%d_%d.txt" % (tile, det))
    env = dict(os.environ, EVC_FORCE_TILE=str(tile), SHIM_LOG=log)
    env.pop("EVC_DETERMINISTIC", None)
    if det:
        env["EVC_DETERMINISTIC"] = "1"
    subprocess.run([sys.executable, SCRIPT, "--drive-skip", lib], check=True, env=env)
    plan, launches, split_launches, skipped, refused = None, 0, 0, 0, 0
    for head, body in _blocks(log):
        text = "\n".join(body)
        ok = any(l.startswith("rc 0") for l in body)
        if head.startswith("== evc_gemm_tn_plan "):
            m = re.search(r"plan tile=(-?\d+) splits=(-?\d+) live_walk=(-?\d+)", text)
            plan = (head[len("== evc_gemm_tn_plan "):], ok, int(m.group(1)), int(m.group(2)), int(m.group(3)))
            continue
        slabs = head.startswith("== evc_gemm_tn2_slabs_skip ")
        if not slabs:
            assert plan[0] in head, (head, plan)
            assert ok == plan[1], "the query and the launch disagree on the arguments: %s" % head
        if not ok:
            refused += 1
            assert "launch" not in text and "memset" not in text, head
            continue
        launches += 1
        lds = int(re.search(r"launch \S+ grid=\d+ block=\d+ lds=(\d+)", text).group(1))
        splits, ksteps = (int(x) for x in re.search(r" splits=(\d+) ksteps=(-?\d+)", text).groups())
        nk = int(re.search(r" nk=(-?\d+)", text).group(1))
        stride = int(re.search(r"slab_stride=(\d+)", text).group(1))
        if not slabs:
            assert (LDS[lds], splits, int("EELb1EEv13GemmOperandsT" in text)) == plan[2:], (head, plan)      # (..ELb1EEv..: the kernel's SEG instance)
            assert ("accumulate=0" in text and splits > 1) == ("memset2d" in text), head
        if nk > 0:
            assert ksteps * (splits - 1) < nk, head
        m = re.search(r"k_skip2=(\d+) ksteps2=(-?\d+)", text)
        if m:
            skipped += 1
            skip, ksteps2 = int(m.group(1)), int(m.group(2))
            assert 0 < skip <= nk, head
            if stride:                     # slabs keep the ranges of the unskipped walk (bit-identical partial sums); the skip only cuts their front
                assert ksteps2 == ksteps, head
            elif nk - skip > 0:
                assert ksteps2 * (splits - 1) < nk - skip and ksteps2 * splits >= nk - skip, head
            if splits > 1 and not stride:
                assert ksteps2 >= 32, head
        if splits > 1 and not stride:
            split_launches += 1
            assert ksteps >= 32, head
    assert launches > 2000 and skipped > 500 and refused > 100, (launches, skipped, refused)
    assert (split_launches > 0) == (tile == 0 and det == 0)
