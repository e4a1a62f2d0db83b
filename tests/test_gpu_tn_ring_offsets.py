"""The TN loop's transposing reads address their ring slot, their A / B half of the stage and their second group of four k rows partly through the
read instruction's immediate offset (csrc/gemm_core_tn.h: one lane-offset register per fragment).  A wrong slot, a wrong j = 1 offset or a wrong
A / B base moves a whole 4-row group of a fragment, so the smallest launches show it: the exact integer operands of tests/_wgrad_ref.py, the
whole sentinel-framed buffer bit for bit, the first differing element named.

  264 x 264 on the 256 x 256 tile and 264 x 72 on the 128 x 128 strip tile (N <= 128, one segment), nk = 1 .. 27 K steps each: every residue of the
      ring depth (5) times the fragment double buffer (2), and the launches that never reach the steady loop (nk <= 5)
  one two-segment launch whose second segment skips its first K steps (k_skip)
  one row-planned launch per tile: six slabs of 128 rows with [128, 96, 96, 64, 64, 32] live ones - 4, 3, 3, 2, 2, 1 steps, so every segment
      jump lands on another ring slot

pytest -m gpu; a few seconds in all.
"""
import os

import numpy as np
import pytest
import torch

import _wgrad_parity_child as ch
import _wgrad_ref as wr

pytestmark = pytest.mark.gpu

NKS = tuple(range(1, 28))
LIVE = [128, 96, 96, 64, 64, 32]
TILES = {"tile256": (264, 264), "strip": (264, 72)}


@pytest.fixture(autouse=True)
def _fresh_results():
    """A GPU fault ends the session: nothing more is started on a device that a kernel of this file has just faulted."""
    ch.RESULTS.clear()
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:   # a sticky HIP error
        pytest.exit("GPU error after a TN ring-offset test, stopping: %s" % e, returncode=3)


def _run(case, accs=(0,)):
    """The case on the exact kind; the plan must be the one the case claims (tile, one split, segment walk or not)."""
    for acc in accs:
        plan = case.plan(acc)
        assert (plan["branch"], plan["splits"], plan["seg"]) == (case.claim["branch"], 1, case.claim["seg"]), (case.name, wr.path_name(plan))
    ch.run_case(case, kinds=("exact",), accs=accs)


def _assert_inside(n):
    assert len(ch.RESULTS) == n, "%d checks ran, %d expected" % (len(ch.RESULTS), n)
    assert not ch.failures(), "\n".join(ch.failures())


def test_the_switches_are_off_in_this_process():
    assert os.environ.get("EVC_FORCE_TILE", "0") in ("", "0") and os.environ.get("EVC_DETERMINISTIC", "0") in ("", "0")


@pytest.mark.parametrize("branch", sorted(TILES))
def test_every_ring_residue(branch):
    """nk = 1 .. 27, plain stores: one workgroup per tile walks all nk steps."""
    M, N = TILES[branch]
    for nk in NKS:
        _run(wr.Case("%s %dx%d ring nk=%d" % (branch, M, N, nk), M, N, nk * 32, branch=branch))
    _assert_inside(len(NKS))


@pytest.mark.parametrize("branch", sorted(TILES))
def test_row_plan_segment_jumps(branch):
    """15 live steps of 24: the walk leaves a slab after 4, 3, 3, 2, 2 steps - ring slots 4, 2, 0, 2, 4 - plain and accumulate."""
    M, N = TILES[branch]
    _run(wr.Case("%s %dx%d rows %s" % (branch, M, N, LIVE), M, N, 128 * len(LIVE), rows=LIVE, slab_rows=128, branch=branch, seg=True), accs=(0, 1))
    _assert_inside(2)


def test_two_segments_with_k_skip():
    """264 x (256 + 264) over 13 K steps, the second segment's tiles start at step 3 (B2 is zero in the steps they skip: the entry's contract): their
    first read slot holds step 3, the first segment's step 0, in one launch."""
    from efficientvideoclassification_youtube8m_amd import ops
    ops.check_device(0)
    k_skip, nk = 3, 13
    case = wr.Case("tile256 264x(256+264) nk=%d k_skip=%d" % (nk, k_skip), 264, 256, nk * 32, N2=264, branch="tile256")
    assert ops.gemm_tn_plan(case.M, case.N1, case.K, case.lda, case.ldb1, N2=case.N2, ldb2=case.ldb2, k_skip=k_skip) == (1, 1, False)
    st = torch.cuda.current_stream().cuda_stream
    for acc in (0, 1):
        d = wr.make_data(case, "exact", acc)
        d.B2[:k_skip * 32, :case.N2] = 0.0
        plan = case.plan(acc)
        exp, lim = wr.reference(case, d)
        A, B1, B2 = ch.dev_bf16(d.A), ch.dev_bf16(d.B1), ch.dev_bf16(d.B2)
        outs = []
        for ks in (k_skip, 0):
            buf = torch.from_numpy(d.buf0).to(ch.DEV)
            ch._lib().call("evc_gemm_tn2_rows_skip", A.data_ptr(), case.lda, B1.data_ptr(), case.ldb1, case.N1, B2.data_ptr(), case.ldb2, case.N2, case.c_col2,
                           buf.data_ptr() + 4 * d.c0, case.ldc, case.M, case.K, 1, None, ks, 0, acc, st)
            torch.cuda.synchronize()
            outs.append(buf.cpu().numpy())
        for ks, got in zip((k_skip, 0), outs):
            msg = wr.check(case, d, got, exp, lim, plan)[3]
            ch.record("%s walked with k_skip=%d" % (case.name, ks), wr.path_name(plan), "exact", acc, 0.0, "", msg)
    _assert_inside(4)
    assert np.array_equal(wr.bits(outs[0]), wr.bits(outs[1]))
