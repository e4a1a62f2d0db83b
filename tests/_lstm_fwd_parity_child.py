"""The GPU side of tests/test_gpu_lstm_fwd_parity.py: everything the forward LSTM step kernels store (gate records, c_all, hbuf and its
bf16 copy, the final state) against the float64 step replay of tests/_lstm_fwd_ref.py.

Imported by the test for the cases that run in its own process, and run as a fresh process where the tile switch is read once per process:

    EVC_FORCE_TILE=k python tests/_lstm_fwd_parity_child.py layer     evc_lstm_layer_fwd: the three shapes, plain and planned, and one hoisted
    EVC_FORCE_TILE=k python tests/_lstm_fwd_parity_child.py f16       evc_lstm_layer_fwd_f16 (h_wide = 0): the three shapes, plain and planned
    EVC_FORCE_TILE=k python tests/_lstm_fwd_parity_child.py level2    evc_lstm_level2_fwd: two shapes, plain and planned, both layers
    EVC_FORCE_TILE=k python tests/_lstm_fwd_parity_child.py stack2    evc_lstm_stack2_fwd: M = 70 and M = 200, both layers

Every check prints one line `ratio <case> <output> <worst err/limit> at t=.. slot=.. unit=..` per output before anything is asserted; `ok`
ends a clean run.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import _lstm_fwd_ref as fr  # noqa: E402

DEV = "cuda:0"
TAIL = 4096                     # sentinel elements behind every output buffer
TAIL16, TAIL32 = 0x1234, 0x12345678
LEVEL2_SHAPES = fr.SHAPES[:2]


def _ops():
    from efficientvideoclassification_youtube8m_amd import ops
    ops.check_device(0)
    return ops


def forced_tile():
    k = int(os.environ.get("EVC_FORCE_TILE", "0") or 0)
    return fr.TILES.get(k)


# ---------------------------------------------------------------------------- operands on the device
def device_case(c):
    """The case's operands on the device (bf16, or f16 for an f16 case), and - planned - the project's own RowPlan, which must be
    the host plan the replay uses."""
    if hasattr(c, "x_d"):
        return c
    ops = _ops()
    dt = torch.bfloat16 if c.fmt == "bf16" else torch.float16
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dt).to(DEV)
    c.x_d = dev(c.x)
    c.wT_d = [dev(w.T) for w in c.W]
    c.bias_d = [torch.from_numpy(b.astype(np.float32)).to(DEV) for b in c.bias]
    for a, b in ((c.x_d, c.x), (c.wT_d[0], c.W[0].T)):
        assert np.array_equal(a.float().cpu().double().numpy(), b)     # the device holds exactly the replay's operands
    lens_rows_d = torch.from_numpy(c.lens_rows).to(DEV)
    if c.planned:
        c.plan = ops.RowPlan(lens_rows_d, c.lens_rows, c.T)
        assert c.plan.P == c.P and list(c.plan.rows) == c.rows
        assert np.array_equal(c.plan.inv.cpu().numpy()[:c.P], c.inv[:c.P]) and np.array_equal(c.plan.lens.cpu().numpy()[:c.P], c.lens)
        c.lens_d = c.plan.lens[:c.P]
    else:
        c.plan, c.lens_d = None, lens_rows_d
    return c


class Guarded:
    """A buffer of `n` elements prefilled with a NaN bit pattern, with TAIL sentinel elements behind it."""

    def __init__(self, shape, bits, view=None):
        n = int(np.prod(shape))
        idt = torch.int16 if bits == 16 else torch.int32
        self.flat = torch.full((n + TAIL,), TAIL16 if bits == 16 else TAIL32, dtype=idt, device=DEV)
        self.flat[:n] = fr.NAN16 if bits == 16 else (int(fr.NAN_REC) if view is None else int(fr.NAN32))
        self.n = n
        body = self.flat[:n].view(*shape)
        self.t = body if view is None else body.view(view)
        self.udt = np.uint16 if bits == 16 else np.uint32

    def numpy(self):
        return self.flat[:self.n].cpu().numpy().view(self.udt).reshape(tuple(self.t.shape))

    def guard_ok(self):
        return bool((self.flat[self.n:] == (TAIL16 if self.flat.dtype == torch.int16 else TAIL32)).all())


class LayerOut:
    """What one layer writes: hbuf, (f16: the bf16 copy,) gate records, c_all - all guarded, all prefilled with NaN."""

    def __init__(self, c, f16=False):
        T, P, H = c.T, c.P, c.H
        self.hbuf = Guarded((T + 1, P, H), 16, torch.float16 if f16 else torch.bfloat16)
        self.hbf = Guarded((T + 1, P, H), 16, torch.bfloat16) if f16 else None
        self.gates = Guarded((T, P, H, 2), 32)
        self.c_all = Guarded((T + 1, P, H), 16, torch.bfloat16)

    def all(self):
        return [b for b in (self.hbuf, self.hbf, self.gates, self.c_all) if b is not None]


class Run:
    def __init__(self, c, nlayers, f16=False):
        self.layers = [LayerOut(c, f16) for _ in range(nlayers)]
        self.S = Guarded((c.M, 2 * c.H * nlayers), 32, torch.float32)

    def all(self):
        return [b for L in self.layers for b in L.all()] + [self.S]


def call_twice(c, nlayers, fn, f16=False):
    """fn(run) fills fresh guarded outputs; twice: the forward has no atomics, every buffer must repeat bit for bit, every sentinel survive."""
    runs = []
    for _ in range(2):
        r = Run(c, nlayers, f16)
        fn(r)
        torch.cuda.synchronize()
        runs.append(r)
    for a, b in zip(runs[0].all(), runs[1].all()):
        assert a.guard_ok() and b.guard_ok(), "a sentinel behind an output buffer was overwritten"
        assert torch.equal(a.flat, b.flat), "an output differs between two calls"
    return runs[0]


def run_layer(c, hoist=False, wT=None):
    ops = _ops()
    device_case(c)
    T, P, H, Kin = c.T, c.P, c.H, c.Kin
    f16 = c.fmt == "f16"
    w = c.wT_d[0] if wT is None else wT
    zx = torch.full((T * P * 4 * H,), float("nan"), dtype=torch.float32, device=DEV) if hoist else None

    def fn(r):
        L, S = r.layers[0], r.S.t
        if f16:
            ops.lstm_layer_fwd_f16(c.x_d, w, c.bias_d[0], c.lens_d, T, P, Kin, H, L.hbuf.t, L.hbf.t, S[:, :H], S[:, H:], 2 * H,
                                   gates=L.gates.t, c_all=L.c_all.t, plan=c.plan)
        else:
            ops.lstm_layer_fwd(c.x_d, w, c.bias_d[0], c.lens_d, T, P, Kin, H, L.hbuf.t, S[:, :H], S[:, H:], 2 * H,
                               gates=L.gates.t, c_all=L.c_all.t, hoist=hoist, zx_ws=zx, plan=c.plan)
    return call_twice(c, 1, fn, f16)


def run_pair(c, entry):
    """evc_lstm_level2_fwd (entry = "level2": row plans) or evc_lstm_stack2_fwd (entry = "stack2": layer 0's x-part through zx_ws)."""
    ops = _ops()
    device_case(c)
    T, P, H, Kin = c.T, c.P, c.H, c.Kin
    zx = torch.full((T * P * 4 * H,), float("nan"), dtype=torch.float32, device=DEV)

    def fn(r):
        L0, L1 = r.layers
        args = (c.x_d, c.wT_d[0], c.bias_d[0], c.wT_d[1], c.bias_d[1], c.lens_d, T, P, Kin, H)
        kw = dict(gates=(L0.gates.t, L1.gates.t), c_all=(L0.c_all.t, L1.c_all.t))
        if entry == "level2":
            ops.lstm_level2_fwd(*args, L0.hbuf.t, L1.hbuf.t, r.S.t, plan=c.plan, **kw)
        else:
            assert c.plan is None
            ops.lstm_stack2_fwd(*args, zx, L0.hbuf.t, L1.hbuf.t, r.S.t, **kw)
    return call_twice(c, 2, fn)


# ---------------------------------------------------------------------------- the checks
RESULTS = []          # (name, ratio) of every check of this process


def report(name, output, ratio, at, rep):
    RESULTS.append((name + " " + output, ratio))
    print("ratio %-46s %-9s %s" % (name, output, fr.describe(output, ratio, at, tile=forced_tile(), rep=rep)), flush=True)


def decode_h(c, L):
    bits = L.hbuf.numpy()
    return fr.f16_to_f64(bits) if c.fmt == "f16" else fr.bf16_to_f64(bits)


def check_layer_out(name, c, run, rep, layer=0, nlayers=1):
    """Every element of layer `layer`'s outputs against `rep`; one ratio line per output.  Returns the ratio arrays."""
    L, H = run.layers[layer], c.H
    S = run.S.numpy().view(np.float32)
    res = fr.check_layer(rep, L.hbuf.numpy(), L.gates.numpy().view(np.int32), L.c_all.numpy(), S[:, 2 * layer * H:(2 * layer + 1) * H],
                         S[:, (2 * layer + 1) * H:(2 * layer + 2) * H], hbuf_bf16=L.hbf.numpy() if L.hbf is not None else None,
                         h_f16=c.fmt == "f16")
    for k, (r, at) in fr.worst_ratio(res).items():
        report(name, k, r, at, rep)
    return res


def plan_kw(c):
    return dict(row_map=c.inv, rows_per_step=c.rows, n_state_rows=c.M)


def layer_case(M, Kin, H, planned, fmt="bf16", hoist=False, tag="", saturated=False):
    c = fr.make_case(M, Kin, H, planned, fmt=fmt, saturated=saturated)
    run = run_layer(c, hoist=hoist)
    rep = fr.replay_layer(c.x, decode_h(c, run.layers[0]), c.W[0], c.bias[0], c.lens, **plan_kw(c))
    if saturated:
        assert all(np.isfinite(rep[k]).all() for k in ("gates", "gates_bound", "c", "c_bound", "h", "h_bound"))
    name = "%s%s %s%s" % (tag, "layer_fwd" + ("_f16" if fmt == "f16" else ""), c.name, " hoist" if hoist else "")
    return c, run, rep, check_layer_out(name, c, run, rep)


def pair_case(entry, M, Kin, H, planned, tag="", saturated=False):
    c = fr.make_case(M, Kin, H, planned, nlayers=2, saturated=saturated)
    run = run_pair(c, entry)
    r0, r1 = fr.replay_level2(c.x, decode_h(c, run.layers[0]), decode_h(c, run.layers[1]), c.W[0], c.bias[0], c.W[1], c.bias[1], c.lens,
                              **plan_kw(c))
    for l, rep in enumerate((r0, r1)):
        check_layer_out("%s%s_fwd %s layer %d" % (tag, entry, c.name, l), c, run, rep, layer=l, nlayers=2)
    return c, run


def layer_cases(fmt="bf16", tag=""):
    for (M, Kin, H) in fr.SHAPES:
        for planned in (False, True):
            layer_case(M, Kin, H, planned, fmt=fmt, tag=tag)
    if fmt == "bf16":
        layer_case(*fr.HOIST_SHAPE, False, hoist=True, tag=tag)


N_LAYER_LINES = (2 * len(fr.SHAPES) + 1) * 5          # gates, c_all, hbuf, c_state, h_state
N_F16_LINES = 2 * len(fr.SHAPES) * 6                  # ... + hbuf_bf16
N_LEVEL2_LINES = 2 * len(LEVEL2_SHAPES) * 2 * 5
N_STACK2_LINES = len(fr.STACK2_SHAPES) * 2 * 5


def level2_cases(tag=""):
    for (M, Kin, H) in LEVEL2_SHAPES:
        for planned in (False, True):
            pair_case("level2", M, Kin, H, planned, tag=tag)


def stack2_cases(tag=""):
    for (M, Kin, H) in fr.STACK2_SHAPES:
        pair_case("stack2", M, Kin, H, False, tag=tag)


def failures():
    return [(n, r) for n, r in RESULTS if not r <= 1.0]


def main(mode):
    tag = "tile=%s " % os.environ["EVC_FORCE_TILE"]
    if mode == "layer":
        layer_cases(tag=tag)
    elif mode == "f16":
        layer_cases(fmt="f16", tag=tag)
    elif mode == "level2":
        level2_cases(tag=tag)
    elif mode == "stack2":
        stack2_cases(tag=tag)
    else:
        sys.exit("mode?")
    bad = failures()
    if bad:
        sys.exit("outside the bound: %s" % bad)
    print("ok")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "")
