"""The refusals of the ten forward entry points of csrc/evc_lstm_fwd.hip: a call with one argument broken raises, and it raises BEFORE the
first enqueue - the h buffers (what every entry clears first) keep a sentinel bit for bit - and leaves the library able to repeat the
well-formed call with the bits it gave before.  The well-formed calls are tests/_lstm_fwd_entries.py's, at T = 2."""
import ctypes as C

import pytest
import torch

import _lstm_fwd_entries as fe
from efficientvideoclassification_youtube8m_amd import _lib, ops

pytestmark = pytest.mark.gpu

SENTINEL = 0xA7


def _broken(call):
    """(label, replaced arguments) for every rule the entry has an argument for."""
    a, k = call.args, call.keys
    T, M, H = a["T"], a["M"], a["H"]
    cases = []
    if "rows_per_step" in a:
        cases += [("rows_per_step increases", dict(rows_per_step=(C.c_int32 * T)(M // 2, M))),
                  ("rows_per_step[0] > M", dict(rows_per_step=(C.c_int32 * T)(M + 1, M)))]
    cases += [("gates without c_all", {k["c_all"]: None}),
              ("c_state + 4 bytes", {k["c_state"]: a[k["c_state"]] + 4}),
              ("ld_state % 4", dict(ld_state=a["ld_state"] + 2)),
              ("H off its rule", dict(H=H + 32)),          # neither a multiple of 64 nor of 128
              # gate records off their 16 bytes.  evc_lstm_layer_fwd_hp, evc_lstm_stack2_fwd_f16 and evc_lstm_stack2_fwd_f16_fp8lo gained this check
              # with the shared refusal helpers (their siblings always had it): the one case that differs from the library before them
              ("gates + 8 bytes", {k["gates"]: a[k["gates"]].data_ptr() + 8})]
    return cases


@pytest.mark.parametrize("name", fe.ENTRIES)
def test_refusals_precede_the_first_enqueue(name):
    ops.check_device(0)
    call = fe.build(name, T=2)
    call.run()
    before = call.bits()
    assert any(bool((before[r] != fe.FILL).any()) for r in call.rings)          # the call did write
    for r in call.rings:
        call.outs[r].view(torch.uint8).fill_(SENTINEL)
    for label, over in _broken(call):
        with pytest.raises(_lib.EvcError):
            call.run(**over)
        torch.cuda.synchronize()
        for r in call.rings:
            assert bool((call.outs[r].view(torch.uint8) == SENTINEL).all()), "%s: '%s' was refused after %s had been touched" % (name, label, r)
    call.refill()
    call.run()
    after = call.bits()
    for kk in before:
        assert torch.equal(before[kk], after[kk]), "%s: %s differs after the refused calls" % (name, kk)
