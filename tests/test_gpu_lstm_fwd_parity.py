"""The forward LSTM step kernels (csrc/evc_lstm_fwd.hip, lstm_fwd_epilogue): every element of everything a step stores - the packed gate
records, c_all, hbuf (and the bf16 copy of the f16 form), c_state / h_state - against a float64 replay of the same step fed the kernel's own
h_{t-1}, within the bound derived in tests/_lstm_fwd_ref.py.  Covered: evc_lstm_layer_fwd on every forward tile pick (EVC_FORCE_TILE 1..11)
and hoisted, evc_lstm_layer_fwd_f16 (h_wide = 0), evc_lstm_level2_fwd (the two-tiles-per-workgroup kernel and its two-launch fallback),
evc_lstm_stack2_fwd (both pair kernels), a saturated case, and a negative control.  Buffers are prefilled with NaN and carry sentinel tails;
every entry runs twice and must repeat bit for bit.  pytest -m gpu; every check prints its worst err/limit per output and where it is
(pytest -s shows the lines; a failure carries them).

Out of scope: the "high"-precision forms (evc_lstm_layer_fwd_f16_fp8lo, _f16_dith, _hp, evc_lstm_level2_fwd_high, evc_lstm_stack2_fwd_f16*):
their operands are composite images, and they have oracle and bit-equality tests of their own.

Measured on an MI355X: profiles/fwd_parity_ratios.txt.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _lstm_fwd_parity_child as ch
import _lstm_fwd_ref as fr

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
        pytest.exit("GPU error after a forward parity test, stopping: %s" % e, returncode=3)


def _assert_inside(nlines):
    assert len(ch.RESULTS) == nlines, (len(ch.RESULTS), nlines)
    assert not ch.failures(), ch.failures()


def _child(mode, tile, nlines):
    env = dict(os.environ)
    env["EVC_FORCE_TILE"] = tile
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_lstm_fwd_parity_child.py"), mode], env=env, capture_output=True, text=True,
                           timeout=300, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        pytest.exit("forward parity child %s tile=%s hung, stopping: %s" % (mode, tile, (e.stdout or b"")[-2000:]), returncode=3)
    print(r.stdout)
    if r.returncode in FAULT_CODES:
        pytest.exit("forward parity child %s tile=%s died with %d, stopping:\n%s" % (mode, tile, r.returncode, r.stdout[-2000:] + r.stderr[-3000:]),
                    returncode=3)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-4000:] + r.stderr[-3000:]
    assert r.stdout.count("\nratio ") + r.stdout.startswith("ratio ") == nlines       # a silently skipped case fails
    return r.stdout


@pytest.mark.parametrize("tile", [str(k) for k in range(1, 12)])
def test_layer_fwd_on_every_tile_pick(tile):
    """EVC_FORCE_TILE 1..11 -> the 256-row ring tile, v1 128 x 32, v1 64 x 16, 320, 288, 224 (6 + 8 row fragments), 192, 160, v2 128, v2 64,
    240 (7 + 8): the three shapes of _lstm_fwd_ref.SHAPES plain and under a row plan (two row tiles with a ragged second one on every tile
    height; an active prefix that ends inside a tile; H = 64 = one unit tile with the bias clamp at its end), and one hoisted x-projection.
    One process per tile: the choice is read once."""
    _child("layer", tile, ch.N_LAYER_LINES)


def test_layer_fwd_on_the_chosen_tile():
    ch.layer_cases()
    _assert_inside(ch.N_LAYER_LINES)


def test_layer_fwd_f16_on_the_chosen_tile():
    """evc_lstm_layer_fwd_f16, h_wide = 0: the f16 hbuf at 2^-11, its bf16 copy at 2^-8 (both roundings of the same f32 h_t), and the tape."""
    ch.layer_cases(fmt="f16")
    _assert_inside(ch.N_F16_LINES)


@pytest.mark.parametrize("tile", ["1", "2", "3", "11"])
def test_layer_fwd_f16_on_forced_tiles(tile):
    _child("f16", tile, ch.N_F16_LINES)


@pytest.mark.parametrize("tile", ["1", "6", "11", "7"])
def test_level2_fwd_both_layers(tile):
    """evc_lstm_level2_fwd against replay_level2 (layer 1's x_t = the kernel's layer-0 slab t+1), plain and planned.  Tiles 1, 6, 11 = 256, 224
    and 240 rows take lstm_fwd_walk2_kernel: the first and the last launch carry one role only, and under the plan the two roles of a launch
    have different row counts (layer 1 runs the earlier step).  Tile 7 (192 rows) takes the fallback of two separate launches."""
    _child("level2", tile, ch.N_LEVEL2_LINES)


def test_level2_fwd_on_the_chosen_tile():
    ch.level2_cases()
    _assert_inside(ch.N_LEVEL2_LINES)


@pytest.mark.parametrize("tile", ["2", "3"])
def test_stack2_fwd_on_both_pair_kernels(tile):
    """evc_lstm_stack2_fwd, M = 70 and M = 200: tile 2 = the v1 128 x 32 pair kernel, 3 = the 64 x 16 ring pair kernel.  Layer 0's x-part
    arrives through zx_ws; the replay bounds the whole contraction and does not care."""
    _child("stack2", tile, ch.N_STACK2_LINES)


def test_stack2_fwd_on_the_chosen_tile():
    ch.stack2_cases()
    _assert_inside(ch.N_STACK2_LINES)


def test_saturated_case_layer_and_stack2():
    """Weights and bias scaled until |z| reaches 40 - 90: gates of exactly 0 and 1 in bf16, |c| growing with t; all finite, all inside."""
    c, run, rep, _ = ch.layer_case(*fr.SAT_SHAPE, False, saturated=True)
    assert 40.0 <= np.abs(rep["z"][rep["active"]]).max() <= 90.0
    for L in run.layers:
        h = ch.decode_h(c, L)[1:]
        assert np.isfinite(h[rep["active"]]).all()
    ch.pair_case("stack2", *fr.SAT_SHAPE, False, saturated=True)
    _assert_inside(15)


def test_negative_control_a_zeroed_k_chunk_in_the_operand_is_reported():
    """The checker on the GPU path, kernel untouched: one 64-wide K chunk of the recurrent weights zeroed in the kernel's operand only.  The
    replay, which holds the true weights, must find the gates outside the bound at some t >= 1 on a row that is live there; nothing at t = 0,
    where the recurrent product does not exist; and the unmodified operand passes."""
    M, Kin, H = fr.SHAPES[0]
    c = ch.device_case(fr.make_case(M, Kin, H, False))
    w = c.wT_d[0].clone()
    w[:, Kin + 64:Kin + 128] = 0
    run = ch.run_layer(c, wT=w)
    rep = fr.replay_layer(c.x, ch.decode_h(c, run.layers[0]), c.W[0], c.bias[0], c.lens)
    res = ch.check_layer_out("negative control (h units 64..127 of Wh zeroed)", c, run, rep)
    r, at = fr.worst_ratio(res)["gates"]
    assert r > 1.0 and at[0] >= 1 and c.lens[at[1]] > at[0]
    assert not (res["gates"][0] > 1.0).any()
    ch.RESULTS.clear()
    run = ch.run_layer(c)
    rep = fr.replay_layer(c.x, ch.decode_h(c, run.layers[0]), c.W[0], c.bias[0], c.lens)
    ch.check_layer_out("negative control, operand restored", c, run, rep)
    _assert_inside(5)
