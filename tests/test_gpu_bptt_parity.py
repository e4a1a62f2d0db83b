"""The BPTT step kernels (csrc/evc_lstm_bwd.hip): every element of dz against a float64 replay of the kernel's own tape, within the
bound derived in tests/_bptt_ref.py - on every tile pick of evc_lstm_layer_bwd, its fused form (dz_above / w_above), both forms of
evc_lstm_stack2_bwd, a saturated synthetic tape and EVC_BWD_DC_BF16=1.  pytest -m gpu; every check prints its worst err/bound and
where it is (pytest -s shows the lines; a failure carries them).

Measured on an MI355X: profiles/bptt_parity_ratios.txt.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _bptt_parity_child as ch
import _bptt_ref as br

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
        pytest.exit("GPU error after a BPTT parity test, stopping: %s" % e, returncode=3)


def _assert_inside():
    assert ch.RESULTS, "nothing was checked"
    assert not ch.failures(), ch.failures()


def _child(mode, **env_add):
    env = dict(os.environ)
    env.pop("EVC_FORCE_TILE", None)
    env.pop("EVC_BWD_DC_BF16", None)
    env.update(env_add)
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_bptt_parity_child.py"), mode], env=env, capture_output=True, text=True,
                           timeout=300, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        pytest.exit("BPTT parity child %s %s hung, stopping: %s" % (mode, env_add, (e.stdout or b"")[-2000:]), returncode=3)
    print(r.stdout)
    if r.returncode in FAULT_CODES:
        pytest.exit("BPTT parity child %s %s died with %d, stopping:\n%s" % (mode, env_add, r.returncode, r.stdout[-2000:] + r.stderr[-3000:]), returncode=3)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-4000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("tile", ["1", "2", "3", "4", "5", "6", "7"])
def test_layer_bwd_dz_on_every_tile_pick(tile):
    """EVC_FORCE_TILE 1..7 -> the 192, 160 and 128-row ring tiles, v1 64, v1 32, the skinny kernel, the 64 x 64 ring: the three plain-form
    cases of _bptt_ref.LAYER_CASES (two row tiles with a ragged last one and two column tiles; a row plan whose active prefix ends inside
    a tile and leaves a tile beyond it; H = 64), and for 1..3 the fused-form cases.  One process per tile: the choice is read once."""
    out = _child("tile", EVC_FORCE_TILE=tile)
    assert out.count("\nratio ") + out.startswith("ratio ") == len(br.LAYER_CASES) + (2 * len(br.FUSED_CASES) if int(tile) <= 3 else 0)


@pytest.mark.parametrize("M,Kin,H,planned,above,want_db", br.LAYER_CASES)
def test_layer_bwd_dz_on_the_chosen_tile(M, Kin, H, planned, above, want_db):
    ch.plain_case(M, Kin, H, planned, above, want_db)
    _assert_inside()


@pytest.mark.parametrize("M,H,planned", br.FUSED_CASES)
def test_fused_layer_bwd_dz(M, H, planned):
    """The fused form: the upper layer's dz (a plain call on layer 1, checked too) contracted in layer 0's steps; at a row's last step the
    final-state gradient is added to the product.  At every t some row has its last step (check_lens)."""
    ch.fused_case(M, H, planned)
    _assert_inside()


@pytest.mark.parametrize("M,H,planned", br.STACK2_CASES)
def test_stack2_bwd_dz_both_layers(M, H, planned):
    """evc_lstm_stack2_bwd: the skinny pair launches (M <= 512) and the 128 x 128 pair kernel (M = 520: five row tiles, the last with 8
    rows; its row plan keeps all 520 slots), both db requested.  M <= 512 also against the layer-after-layer calls (layer 1 plain, then
    layer 0 with dz_above), which run the same skinny body there: dz1 bit for bit, dz0 within the two bounds added.  For M = 520 that
    comparison is test_pair_kernel_equals_the_layer_calls_on_the_same_tile."""
    c = ch.make_case("stack2", M, br.STACK2_KIN, H, 2, planned)
    assert (c.P > 512) == (M > 512)
    ch.stack2_case(c, cross=M <= 512)
    _assert_inside()


def test_pair_kernel_equals_the_layer_calls_on_the_same_tile():
    """M = 520 (plain layout and row plan, H = 128 and 256): evc_lstm_stack2_bwd's 128 x 128 pair kernel against the layer-after-layer
    calls, dz1 bit for bit and dz0 within the two bounds added.  Left to itself evc_lstm_layer_bwd runs 520 rows on the skinny kernel,
    whose K range is split over four waves: another f32 summation order than the ring's (measured: 59 of 1 064 960 and 418 of 2 129 920
    dz1 elements of the plain-layout cases then differ, each call inside its own bound), so this comparison runs with EVC_FORCE_TILE=3, the
    128-row ring tile on both sides (read once per process: a child)."""
    out = _child("pair128", EVC_FORCE_TILE="3")
    assert out.count("dz1 elements that differ: 0") == 4


def test_saturated_tape_plain_and_skinny_pair():
    """A written tape: gates of exactly 0 and 1, |j| = 1, |c| up to 20, NaN in slab 0 of c_all and in every record of an inactive row."""
    c = ch.saturated_case(2)
    runs = ch.run_layer(c, above=True)
    rep = ch.replay_plain(c, runs[0], above=True)
    assert np.isfinite(rep["dz"]).all() and np.isfinite(rep["bound"]).all()
    ch.check_dz("saturated plain", c, runs[0], rep, runs)
    ch.stack2_case(c, tag="saturated ", cross=False)
    _assert_inside()


def test_bf16_carry_switch():
    """EVC_BWD_DC_BF16=1 (read once per process): the plain M = 200, H = 256 case and the M = 520, H = 128 pair case."""
    out = _child("dc_bf16", EVC_BWD_DC_BF16="1")
    assert out.count("ratio ") == 3


def test_negative_control_a_dropped_k_chunk_in_the_operand_is_reported():
    """The checker on the GPU path, kernel untouched: one 32-wide K chunk of Wh zeroed in the kernel's operand only."""
    M, Kin, H = br.LAYER_CASES[0][:3]
    c = ch.make_case("layer", M, Kin, H, 1, False)
    w = c.w_il[0].clone()
    w[Kin:, 7 * 32:8 * 32] = 0
    o = ch.run_layer(c, above=True, w_il=w)[0]
    rep = ch.replay_plain(c, o, above=True)
    r, at = br.worst_ratio(ch._f64(o.dz), rep["dz"], rep["bound"], rep["active"])
    print("ratio negative control (K chunk 7 of Wh zeroed)             %s" % br.describe(r, at))
    assert r > 1.0 and at[0] < br.T_STEPS - 1 and c.lens[at[1]] - 1 > at[0]     # where the recurrent product is used
    o = ch.run_layer(c, above=True)[0]
    rep = ch.replay_plain(c, o, above=True)
    assert br.worst_ratio(ch._f64(o.dz), rep["dz"], rep["bound"], rep["active"])[0] <= 1.0
