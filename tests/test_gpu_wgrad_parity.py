"""The weight-gradient TN products (csrc/evc_gemm_tn.hip), every element, on every path of the dispatch: operands whose product is exact in
f32 against the integer product, bit for bit, and dz-like operands against the float64 product within the any-order bound of
tests/_wgrad_ref.py; the slab entries slab by slab, the slab sum, the bias-gradient column sums and engine.LstmStack._wgrad_tn.  C always
lives inside a larger buffer of sentinels.  pytest -m gpu; every check prints its path (by plan_tn) and `exact` or its worst err/d and
where (pytest -s shows the lines; a failure carries them).

Measured on an MI355X: profiles/wgrad_parity_ratios.txt.
"""
import os
import subprocess
import sys

import pytest
import torch

import _wgrad_parity_child as ch
import _wgrad_ref as wr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FAULT_CODES = (-6, -11, -9, 134, 139, 137, 124)


@pytest.fixture(autouse=True)
def _fresh_results():
    """A GPU fault ends the session: nothing more is started on a device that a kernel of this file has just faulted."""
    ch.RESULTS.clear()
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:   # a sticky HIP error
        pytest.exit("GPU error after a weight-gradient parity test, stopping: %s" % e, returncode=3)


def _assert_inside():
    assert ch.RESULTS, "nothing was checked"
    assert not ch.failures(), "\n".join(ch.failures())


def _child(mode, **env_add):
    env = dict(os.environ)
    env.pop("EVC_FORCE_TILE", None)
    env.pop("EVC_DETERMINISTIC", None)
    env.update(env_add)
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_wgrad_parity_child.py"), mode], env=env, capture_output=True, text=True,
                           timeout=120, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        pytest.exit("weight-gradient parity child %s %s hung, stopping: %s" % (mode, env_add, (e.stdout or b"")[-2000:]), returncode=3)
    print(r.stdout)
    if r.returncode in FAULT_CODES:
        pytest.exit("weight-gradient parity child %s %s died with %d, stopping:\n%s" % (mode, env_add, r.returncode, r.stdout[-2000:] + r.stderr[-3000:]), returncode=3)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-4000:] + r.stderr[-3000:]
    return r.stdout


NATURAL = [c for c in wr.CASES if c.group == "natural"]


def test_the_switches_are_off_in_this_process():
    """The in-process cases claim the default dispatch: both switches are read once per process by the library."""
    assert os.environ.get("EVC_FORCE_TILE", "0") in ("", "0") and os.environ.get("EVC_DETERMINISTIC", "0") in ("", "0")


@pytest.mark.parametrize("case", NATURAL, ids=[c.name for c in NATURAL])
def test_tn_product_every_element(case):
    """Cases 2 - 7 on the branch the dispatch picks: plain and accumulate, both data kinds, twice."""
    ch.run_case(case)
    _assert_inside()
    assert len(ch.RESULTS) == len(case.kinds) * len(case.accs)


def test_forced_128_tile_branch():
    """EVC_FORCE_TILE=11 (a child: the switch is read once): nk 1 .. 8 and 11 around the 5-deep ring, the 8 x 8 and the ragged 264 x 40 tile,
    two column segments, every row plan, and the branch's negative controls."""
    out = _child("tile11", EVC_FORCE_TILE="11")
    n = sum(len(c.kinds) * len(c.accs) for c in wr.CASES if c.group == "tile11")
    assert out.count("\nratio ") + out.startswith("ratio ") == n + 6
    assert all("| tn128 " in line for line in out.splitlines() if line.startswith("ratio "))


def test_deterministic_switch():
    """EVC_DETERMINISTIC=1 (a child): the K >= 2080 cases with splits 1 and no segment walk - the garbage in B's dead rows meets zeros -,
    ops.gemm_tn_det with the segment gap, ops.colsum_bf16 on its two entries, and _wgrad_tn's two deterministic routes."""
    out = _child("det", EVC_DETERMINISTIC="1")
    n = sum(len(c.kinds) * len(c.accs) for c in wr.DET_CASES)
    assert out.count("\nratio ") + out.startswith("ratio ") == n + 2 + 6 + 2
    assert "splits=1 x" in out and " seg " not in out


@pytest.mark.parametrize("branch", ["strip", "tile256"])
def test_negative_controls_fail_where_predicted(branch):
    """The kernel untouched, the reference fed a changed input (one K row of A negated; rows[t] lowered by 32 in one slab; c_col2 off by 8):
    the exact kind flags exactly the elements the change moves, the wide kind sits above its limit there (factor printed)."""
    ch.negative_controls(branch)
    _assert_inside()


@pytest.mark.parametrize("nslab", [1, 3, 97])
@pytest.mark.parametrize("two", [False, True], ids=["evc_gemm_tn_slabs", "evc_gemm_tn2_slabs"])
def test_slab_entries_every_slab_on_its_own(two, nslab):
    for kind in ("exact", "wide"):
        ch.run_slabs(two, nslab, kind)
    _assert_inside()


def test_refusals_write_nothing():
    """An nslab that leaves an empty slab; a row plan whose K is no multiple of 32."""
    ch.slab_refusal()
    ch.rows_refusal()
    _assert_inside()
    assert len(ch.RESULTS) == 3


def test_sum_slabs_in_slab_order():
    for kind in ("exact", "wide"):
        for acc in (0, 1):
            ch.run_sum_slabs(kind, acc)
    _assert_inside()


@pytest.mark.parametrize("R", ch.COLSUM_R)
def test_colsum_bf16(R):
    """The bias gradient: integers bit for bit (atomics commute on them), dz-like values within R U sum |x|; the memset covers exactly C floats."""
    for C in ch.COLSUM_C:
        for kind in ("exact", "wide"):
            for H in (0, C // 4):
                ch.run_colsum(R, C, kind, H, "atomic")
                for ws in ((max(1, R // 64 - 1), R // 64 + 7) if R >= 128 else (1, 3)):       # partial rows below and above R / 64
                    ch.run_colsum(R, C, kind, H, "det", ws)
    _assert_inside()


@pytest.mark.parametrize("H,kin,rows,live", [(256, 256, 256, None), (256, 256, 256, ([40, 64, 0, 17], 64)), (64, 72, 160, None), (64, 72, 2080, None)],
                         ids=["fused", "fused live", "two launches", "two launches split"])
def test_engine_wgrad_tn_routes(H, kin, rows, live):
    ch.run_engine(H, kin, rows, live)
    _assert_inside()


def test_engine_wgrad_tn_layer0_route():
    """kin - n1 = 128, rows = 16384, (n1 + H) % 2048 == 0: the 2048-column launch with the gap plus the 128-column strip.  The route's own
    condition admits no smaller shape; 16 slabs of 1024 rows with 40 .. 70 live rows each keep the host product small.  |i| <= 2."""
    live = ([40 + 2 * t for t in range(16)], 1024)
    ch.run_engine(1024, 1152, 16384, live, qmax=2)
    _assert_inside()
