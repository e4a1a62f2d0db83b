"""The NetVLAD context gate (--netvlad_gating) on the device: evc_bn_gate_fwd / _bwd_partial / _bwd_finalize bit for bit
against the chain of older entries they replace, the gated tower against the float64 restatement tests/_netvlad_gating_ref.py (grid
and sampled frames, training and forward only), the distillation step with gated and ungated towers, and - in a child process under
EVC_DETERMINISTIC=1 - fused against chain in the tower, gate off against no keyword, and train.main / validate.main end to end.
pytest -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _netvlad_gating_ref as gx
from oracle import model_math as mm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
NEW = ("gating_weights", "gating_bn/beta", "gating_bn/gamma")


def _np(t):
    return t.detach().cpu().double().numpy()


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


# ---------------------------------------------------------------------------- 1. the three entries against the chain
def _gate_case(R, C, seed):
    rng = np.random.default_rng(seed)
    gl = _d(rng.standard_normal((R, C)) * 2.0 + 0.5)
    h = _d(np.clip(rng.standard_normal((R, C)) * 2.0 + 1.5, 0.0, 6.0))                 # a relu6 output: zeros, sixes and values between
    d, d2 = _d(rng.standard_normal((R, C)) * 0.1), _d(rng.standard_normal((R, C)) * 0.1)
    mean, var = _d(0.5 + 0.2 * rng.standard_normal(C)), _d(4.0 * np.exp(0.2 * rng.standard_normal(C)))      # away from (0, 1)
    gamma, beta = _d(np.exp(0.2 * rng.standard_normal(C))), _d(0.2 * rng.standard_normal(C))
    return gl, h, d, d2, mean, var, gamma, beta


def _guarded(n, dtype=torch.float32, shift=0):
    """A NaN-filled buffer of n elements with one guard element behind it (and `shift` in front: a base that is not 16-byte aligned)."""
    full = torch.full((shift + n + 1,), NAN, dtype=dtype, device=DEV)
    return full, full[shift:shift + n]


def _run_gate(ops, fused, gl, h, d, d2, mean, var, gamma, beta, shift=0):
    R, C = gl.shape
    n = R * C
    bufs = {k: _guarded(n, shift=shift) for k in ("out", "dh", "dgl")}
    bufs["dgl_bf"] = _guarded(n, torch.bfloat16)
    bufs["dgamma"], bufs["dbeta"] = _guarded(C), _guarded(C)
    bufs["ws"] = _guarded(2 * C, torch.float64)
    v = {k: (b[1].view(R, C) if k in ("out", "dh", "dgl", "dgl_bf") else b[1]) for k, b in bufs.items()}
    st = (mean, var, gamma, beta)
    if fused:
        ops.bn_gate_fwd(gl, h, R, C, *st, v["out"])
        ops.bn_gate_bwd_partial(gl, h, d, d2, R, C, *st, v["ws"], v["dh"])
        ops.bn_gate_bwd_finalize(gl, h, d, d2, R, R, C, *st, v["ws"], dgl_f32=v["dgl"], dgl_bf16=v["dgl_bf"], dgamma=v["dgamma"], dbeta=v["dbeta"])
    else:
        gn, dgn = torch.full((R, C), NAN, device=DEV), torch.full((R, C), NAN, device=DEV)
        ops.bn_apply(gl, R, C, *st, False, y_f32=gn)
        ops.nextvlad_gate_fwd(h, gn, v["out"])
        ops.nextvlad_gate_bwd_add(h, gn, d, d2, v["dh"], dgl=dgn)
        ops.bn_bwd_partial(gl, dgn, R, C, *st, False, v["ws"])
        ops.bn_bwd_finalize(gl, dgn, R, R, C, *st, False, v["ws"], dx_f32=v["dgl"], dx_bf16=v["dgl_bf"], dgamma=v["dgamma"], dbeta=v["dbeta"])
    torch.cuda.synchronize()
    for k, (full, view) in bufs.items():
        assert torch.isnan(full[-1]) and torch.isnan(full[:full.numel() - view.numel() - 1].float()).all(), k       # the guards
        assert torch.isfinite(view.float()).all(), k
    return {k: b[1].clone() for k, b in bufs.items() if k != "ws"}


# (R, C): a single element; a column tail in the second 64-column block and C % 4 != 0 (the scalar forward); more rows than the four row
# lanes, C % 4 == 0 (the 16-byte forward; with shift, the scalar forward on the same shape); the last R at which the partial pass
# launches ONE row block per column group (R < 512), so that the f64 column sums have one adder and one order.
@pytest.mark.parametrize("with_d2", [True, False])
@pytest.mark.parametrize("R,C,shift", [(1, 1, 0), (7, 65, 0), (33, 128, 0), (33, 128, 1), (511, 200, 0)])
def test_fused_gate_entries_are_the_chain_bit_for_bit(R, C, shift, with_d2):
    """evc_bn_gate_fwd / _bwd_partial / _bwd_finalize against evc_bn_apply, evc_nextvlad_gate_fwd, evc_nextvlad_gate_bwd_add and
    evc_bn_bwd_partial / _finalize: torch.equal in out, dh, dgl f32 / bf16, dgamma, dbeta; statistics away from (0, 1); outputs prefilled
    with NaN, a guard element behind each; every call made twice for equal bits.  And the f32 outputs against float64."""
    from efficientvideoclassification_youtube8m_amd import ops
    gl, h, d, d2, mean, var, gamma, beta = _gate_case(R, C, 100 * R + C)
    args = (gl, h, d, d2 if with_d2 else None, mean, var, gamma, beta)
    a, a2 = _run_gate(ops, True, *args, shift=shift), _run_gate(ops, True, *args, shift=shift)
    b = _run_gate(ops, False, *args)
    for k in a:
        assert torch.equal(a[k], a2[k]), "two calls differ in " + k
        assert torch.equal(a[k], b[k]), "%s: %d of %d elements differ from the chain" % (k, int((a[k] != b[k]).sum()), a[k].numel())
    g64 = gx.sigmoid((_np(gl) - _np(mean)) / np.sqrt(_np(var) + 1e-3) * _np(gamma) + _np(beta))
    e64 = _np(d) + (_np(d2) if with_d2 else 0.0)
    assert np.abs(_np(a["out"]).reshape(R, C) - _np(h) * g64).max() < 1e-5 and np.abs(_np(a["dh"]).reshape(R, C) - e64 * g64).max() < 1e-6
    if R > 1:
        assert a["dgl"].any() and a["dgamma"].any()


def test_gate_entries_refuse_before_any_launch():
    """R < 1, C < 1 (EVC_ERR_BAD_SHAPE, -1) and a NULL operand (EVC_ERR_BAD_ARG, -5; d2 alone may be NULL): nothing is written."""
    from efficientvideoclassification_youtube8m_amd import _lib, ops
    R, C = 5, 8
    gl, h, d, d2, mean, var, gamma, beta = _gate_case(R, C, 1)
    out, dh, dgl = (torch.full((R, C), 3.0, device=DEV) for _ in range(3))
    ws = torch.full((2 * C,), 3.0, dtype=torch.float64, device=DEV)
    st = (mean, var, gamma, beta)
    for r, c in ((0, C), (R, 0), (-1, C)):
        with pytest.raises(_lib.EvcError, match=r"evc_bn_gate_fwd failed \(-1\)"):
            ops.bn_gate_fwd(gl, h, r, c, *st, out)
        with pytest.raises(_lib.EvcError, match=r"evc_bn_gate_bwd_partial failed \(-1\)"):
            ops.bn_gate_bwd_partial(gl, h, d, d2, r, c, *st, ws, dh)
        with pytest.raises(_lib.EvcError, match=r"evc_bn_gate_bwd_finalize failed \(-1\)"):
            ops.bn_gate_bwd_finalize(gl, h, d, d2, r, r, c, *st, ws, dgl_f32=dgl)
    with pytest.raises(_lib.EvcError, match=r"evc_bn_gate_bwd_finalize failed \(-1\)"):
        ops.bn_gate_bwd_finalize(gl, h, d, d2, R, R - 1, C, *st, ws, dgl_f32=dgl)
    for i in range(7):                                               # gl, h, the four vectors, out
        a = [gl, h, mean, var, gamma, beta, out]
        a[i] = None
        with pytest.raises(_lib.EvcError, match=r"evc_bn_gate_fwd failed \(-5\).*NULL operand"):
            ops.bn_gate_fwd(a[0], a[1], R, C, *a[2:6], a[6])
    for i in range(9):                                               # gl, h, d, the four vectors, ws, dh
        a = [gl, h, d, mean, var, gamma, beta, ws, dh]
        a[i] = None
        with pytest.raises(_lib.EvcError, match=r"evc_bn_gate_bwd_partial failed \(-5\).*NULL operand"):
            ops.bn_gate_bwd_partial(a[0], a[1], a[2], d2, R, C, *a[3:7], a[7], a[8])
        if i < 8:
            with pytest.raises(_lib.EvcError, match=r"evc_bn_gate_bwd_finalize failed \(-5\).*NULL operand"):
                ops.bn_gate_bwd_finalize(a[0], a[1], a[2], d2, R, R, C, *a[3:7], a[7], dgl_f32=dgl)
    torch.cuda.synchronize()
    assert all(bool((t == 3.0).all()) for t in (out, dh, dgl, ws))


# ---------------------------------------------------------------------------- 2. / 5. / 6. two towers bit for bit, train.main: a process of its own
@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """tests/_netvlad_gating_child.py, once, in a fresh process under EVC_DETERMINISTIC=1 (the library reads it once per process)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    work = str(tmp_path_factory.mktemp("netvlad_gating"))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "_netvlad_gating_child.py"), work],
                       env=dict(os.environ, EVC_DETERMINISTIC="1"), capture_output=True, text=True, timeout=600)
    lines = [line for line in r.stdout.splitlines() if not line.startswith("Key: ")]
    print("\n".join(lines)[-8000:])
    return r, "\n".join(lines)


def test_fused_gate_tower_is_the_chain_tower_bit_for_bit(child):
    """NetVladTower.fused_gate True against False at B = 8, T = 40, F = 128, K = 64, H = 64, every_n = 1: state, predictions and every
    gradient, with and without dstate, and the evaluation forward."""
    r, out = child
    assert "deterministic 1" in out and "fused: ok" in out, out[-3000:] + r.stderr[-3000:]
    for ds in (0, 1):
        for name in ("predictions", "state") + tuple("grad " + k for k in NEW + ("hidden1_weights", "cluster_weights", "input_bn/gamma")):
            assert any(line.split() == ("fused dstate=%d %s equal" % (ds, name)).split() for line in out.splitlines()), (ds, name)
    assert "DIFFERS" not in out.split("fused: ok")[0]


def test_gate_off_is_the_tower_without_the_keyword(child):
    """gating=False: no new variable or buffer, and over two training steps the bits of a tower built without the keyword; no launch of
    the gate's entries."""
    r, out = child
    assert "gate_off: ok" in out, out[-3000:] + r.stderr[-3000:]
    for step in (0, 1):
        for what in ("predictions", "gradient store", "master weights"):
            assert any(line.split() == ("gate_off step %d %s equal" % (step, what)).split() for line in out.splitlines()), (step, what)


def test_gating_through_train_main(child):
    """train.main with --netvlad_gating True for 4 steps, then --teacher_dir for 4 steps: metadata, model/* the teacher's bits, a fresh
    forward-only tower bit for bit, resume, a flag / checkpoint mismatch refused, validate.main equal to eval_util (also on device)."""
    r, out = child
    assert "workflow: ok" in out and r.returncode == 0, out[-3000:] + r.stderr[-3000:]
    for words in ("model/* holds the teacher's bits", "reproduces the student's evaluation predictions bit for bit",
                  "validate.main equals eval_util on those predictions, --metrics_on_device True too",
                  "resume works, a flag / checkpoint mismatch is refused"):
        assert words in out, words


# ---------------------------------------------------------------------------- 3. / 4. the tower against float64
B4, F4, K4, H4, V4, T4 = 32, 128, 64, 128, 33, 60
_BATCH = {}


def _batch(n4=0):
    """The shared batch: video 4 with n4 frames (empty by default), video 11 with 3; q its uint8 form, x the f32 one, zero past the end."""
    if n4 not in _BATCH:
        q, x, n, labels = mm.synthetic_batch(B4, seed=B4, max_frames=T4, feature_size=F4, vocab_size=V4, dtype=np.float32)
        n[4], n[11] = n4, 3
        x[np.arange(T4)[None, :] >= n[:, None]] = 0.0
        _BATCH[n4] = dict(q=q, x=x, n=n, labels=labels, xn=mm.l2_normalize(x.astype(np.float64), 2))
    return _BATCH[n4]


def _params(tw, moving=False):
    pre = tw.scope + "/"
    sd = {k[len(pre):]: _np(v) for k, v in tw.state_dict().items()}
    M = {k: sd.pop(k) for k in list(sd) if "/moving_" in k}
    return (sd, M) if moving else sd


def _perturb(tw, rng, moving=False):
    for k in tw.names:
        if k.endswith("/gamma") or k.endswith("/beta"):
            z = torch.from_numpy(rng.standard_normal(tw.store.p(k).shape).astype(np.float32) * 0.2).to(DEV)
            tw.store.p(k).copy_(tw.store.p(k) * torch.exp(z) if k.endswith("/gamma") else tw.store.p(k) + z)
    if moving:
        for k, v in tw.buffers.items():
            z = torch.from_numpy(rng.standard_normal(v.shape).astype(np.float32) * 0.2).to(DEV)
            v.copy_(v * torch.exp(z) if k.endswith("variance") else v + z)
    tw.refresh_shadows()


def _tf_grad(tw, k):
    got = tw.store.g(k)
    got = _np(got.t() if got.dim() == 2 else got)
    if k == tw.HW:
        got = got.reshape(tw.Kc, tw.F, tw.Hd).transpose(1, 0, 2).reshape(tw.F * tw.Kc, tw.Hd)
    return got


def _grad_figures(tag, tw, want, missed):
    assert set(want) == set(tw.names) and all(k in want for k in NEW)
    for k, w in want.items():
        got = _tf_grad(tw, k)
        l2 = float(np.linalg.norm(got - w) / (np.linalg.norm(w) + 1e-30))
        mx = float(np.abs(got - w).max())
        print("%s   grad %-28s rel l2 %.3e  max abs %.3e  (|ref|max %.3e)" % (tag, k, l2, mx, float(np.abs(w).max())))
        if not (l2 < 0.12 or mx < 1e-3):
            missed.append(("grad " + k, (l2, mx), (0.12, 1e-3)))


@pytest.mark.parametrize("mode,u8", [("grid", True), ("grid", False), ("sampled", True), ("sampled", False)])
def test_gated_tower_against_float64(mode, u8):
    """The gated tower's training forward and backward (L_CE) against tests/_netvlad_gating_ref.py at B = 32, F = 128, K = 64, H = 128,
    V = 33, T = 60: grid mode at every_n = 10 with video 4 empty and video 11 of 3 frames; sampled mode at S = 17 on the same batch
    (a sampled tower has no frame to draw from an empty video: video 4 keeps one frame there).  uint8 and f32 input.  The bounds
    test_gpu_netvlad_packed.py / test_gpu_netvlad_distill.py apply to this tower, none new: a 2e-2, Y_bf 2e-2, predictions 5e-3, every
    gradient tensor - the gate's three included - relative L2 0.12 or max abs 1e-3; the state is reported.  Every figure is printed
    before the first assertion; the observed maxima are recorded in DESIGN.md 7.21."""
    from efficientvideoclassification_youtube8m_amd.towers import NetVladTower
    bt = _batch(1 if mode == "sampled" else 0)
    rng = np.random.default_rng(B4 + K4)
    n = bt["n"]
    S = 17
    if mode == "sampled":
        tw = NetVladTower(B4, T4, F4, V4, iterations=S, cluster_size=K4, hidden_size=H4, device=DEV, seed=3, gating=True)
    else:
        tw = NetVladTower(B4, T4, F4, V4, cluster_size=K4, hidden_size=H4, device=DEV, seed=3, frames="grid", every_n=10, gating=True)
    assert tw.fused_gate and tw.gating
    _perturb(tw, rng)
    P = _params(tw)
    assert P["gating_weights"].shape == (H4, H4) and P["gating_bn/gamma"].shape == (H4,)
    xin, nd = torch.from_numpy(bt["q"] if u8 else bt["x"]).to(DEV), torch.from_numpy(n).to(DEV)
    if mode == "sampled":
        u = rng.random((B4, S)).astype(np.float32)
        pred = tw.forward(xin, nd, torch.from_numpy(u).to(DEV))
        idx = mm.sample_random_frames_index(u, n)
        assert np.array_equal(tw.idx.cpu().numpy(), idx)
        frames = [np.asarray(idx[b], np.int64) for b in range(B4)]
        ref_pred, c = gx.fwd(bt["xn"], n, 1, P, frames=frames)
    else:
        pred = tw.forward(xin, nd, num_frames_host=n)
        ref_pred, c = gx.fwd(bt["xn"], n, 10, P)
        assert tw.R == c["r"].shape[0] == 181 and not tw.Vv[4].any()
    R = c["r"].shape[0]
    tag = "%s u8=%d" % (mode, u8)
    Yk = lambda Y: Y.reshape(B4, F4, K4).transpose(0, 2, 1).reshape(B4, K4 * F4)
    figures = (("a", np.abs(_np(tw.a[:R]) - c["a"]).max(), 2e-2), ("Y_bf", np.abs(tw.Y_bf[:B4].float().cpu().numpy() - Yk(c["Y"])).max(), 2e-2),
               ("h6", np.abs(_np(tw.h6) - c["h6"]).max(), None), ("gl", np.abs(_np(tw.gl) - c["gl"]).max(), None),
               ("state", np.abs(_np(tw.state) - c["state"]).max(), None), ("pred", np.abs(_np(pred) - ref_pred).max(), 5e-3))
    missed = []
    for what, e, bound in figures:
        print("%s %-6s err %.2e%s" % (tag, what, e, "" if bound is None else "  (bound %.0e)" % bound))
        if bound is not None and not e < bound:
            missed.append((what, e, bound))
    assert tw.state.data_ptr() == tw.gated.data_ptr() and not torch.equal(tw.state, tw.h6)
    dp = mm.cross_entropy_grad(ref_pred, bt["labels"])
    tw.backward(torch.from_numpy(dp.astype(np.float32)).to(DEV))
    torch.cuda.synchronize()
    assert tw.h6_bf.shape[0] == tw.Bk and not tw.h6_bf[B4:].any() and not tw.dgl_bf[B4:].any()
    _grad_figures(tag, tw, gx.bwd(dp, c), missed)
    assert not missed, missed


def test_forward_only_gated_tower_against_float64():
    """A training=False gated grid tower on perturbed moving statistics (gating_bn's included) against the float64 evaluation forward
    under the predictions bound, then a shorter second batch in the same buffers (the rows= path of the head behind the gate)."""
    from efficientvideoclassification_youtube8m_amd.towers import NetVladTower
    bt = _batch()
    rng = np.random.default_rng(7)
    tw = NetVladTower(B4, T4, F4, V4, cluster_size=K4, hidden_size=H4, device=DEV, seed=5, frames="grid", every_n=10, gating=True, training=False)
    assert tw.store.grad is None and tw.store.m is None and not hasattr(tw, "dgl_bf")
    _perturb(tw, rng, moving=True)
    P, M = _params(tw, moving=True)
    assert "gating_bn/moving_variance" in M
    names = ("r", "hid", "h6", "h6_bf", "gl", "gated")
    ptrs = {k: getattr(tw, k).data_ptr() for k in names}
    missed = []
    for b in (B4, 20):
        n = bt["n"][:b]
        pred = tw.forward(torch.from_numpy(bt["q"][:b]).to(DEV), torch.from_numpy(n).to(DEV), num_frames_host=n, is_training=False)
        want, state, c = gx.eval_fwd(bt["xn"][:b], n, 10, P, M)
        torch.cuda.synchronize()
        assert tuple(pred.shape) == (b, V4) and tuple(tw.state.shape) == (b, H4) and tuple(tw.pred.shape) == (b, V4)
        e, es = np.abs(_np(pred) - want).max(), np.abs(_np(tw.state) - state).max()
        print("forward only b=%d: pred err %.2e (bound 5e-03)  state err %.2e" % (b, e, es))
        if not e < 5e-3:
            missed.append((b, e))
        assert ptrs == {k: getattr(tw, k).data_ptr() for k in names}
        assert np.array_equal(_np(tw.buffers["gating_bn/moving_mean"]), M["gating_bn/moving_mean"])        # evaluation leaves them alone
    assert not missed, missed


# ---------------------------------------------------------------------------- the distillation step
def _graph(on, gating, teacher_gating):
    from efficientvideoclassification_youtube8m_amd.distill import NetVladDistillGraph
    g = NetVladDistillGraph(B4, every_n=10, teacher_every_n=1, feature_size=F4, vocab_size=V4, max_frames=T4, cluster_size=K4,
                            hidden_size=H4, device=DEV, seed=3, distill_losses=on, gating=gating, teacher_gating=teacher_gating)
    rng = np.random.default_rng(B4 + K4 + int(teacher_gating))
    _perturb(g.student, rng)
    _perturb(g.teacher, rng, moving=True)
    assert (g.student.gating, g.teacher.gating) == (gating, teacher_gating)
    return g


@pytest.mark.parametrize("teacher_gating", [False, True])
def test_distillation_step_against_float64(teacher_gating):
    """step(apply=False) with rep,pred,ce: a gated student on every 10th frame against an ungated and a gated frozen teacher on every
    frame, at the sizes and under the bounds of test_gpu_netvlad_distill.py's test_step_against_float64 (the four losses 2e-2 relative
    + 1e-6, predictions 5e-3, student a / Y_bf 2e-2, every student gradient relative L2 0.12 or max abs 1e-3; the states and dstate
    reported).  L_REP and dstate are on `state`, the gated vector."""
    bt = _batch()
    g = _graph(("rep", "pred", "ce"), True, teacher_gating)
    (teacher, moving), student = _params(g.teacher, moving=True), _params(g.student)
    assert ("gating_weights" in teacher) == teacher_gating and "gating_weights" in student
    ref = gx.distill_step(bt["xn"], bt["n"], bt["labels"], teacher, moving, student, 1, 10)
    y = torch.from_numpy(bt["labels"].astype(np.uint8)).to(DEV)
    t_before = g.teacher.store.master.clone()
    out = g.step(torch.from_numpy(bt["q"]).to(DEV), y, torch.from_numpy(bt["n"]).to(DEV), apply=False, num_frames_host=bt["n"])
    torch.cuda.synchronize()
    assert torch.equal(g.teacher.store.master, t_before) and g.global_step == 0
    ts, tt = g.student, g.teacher
    assert out["student_state"].data_ptr() == ts.gated.data_ptr()
    assert out["teacher_state"].data_ptr() == (tt.gated if teacher_gating else tt.h6).data_ptr()
    sc = ref["student_cache"]
    R = sc["r"].shape[0]
    assert ts.R == R == 181 and tt.R == 1803
    tag = "teacher_gating=%d" % teacher_gating
    rep, missed = g.loss_report(), []
    for k in g.LOSS_SLOTS:
        print("%s loss %-20s got %.6f  float64 %.6f  rel %.2e" % (tag, k, rep[k], float(ref[k]), abs(rep[k] - ref[k]) / abs(ref[k])))
        if not abs(rep[k] - ref[k]) <= 2e-2 * abs(ref[k]) + 1e-6:
            missed.append((k, rep[k], float(ref[k])))
    Yk = lambda Y: Y.reshape(B4, F4, K4).transpose(0, 2, 1).reshape(B4, K4 * F4)
    figures = (("teacher pred", np.abs(_np(out["predictions"]) - ref["teacher_predictions"]).max(), 5e-3),
               ("teacher state", np.abs(_np(out["teacher_state"]) - ref["teacher_state"]).max(), None),
               ("student a", np.abs(_np(ts.a[:R]) - sc["a"]).max(), 2e-2),
               ("student Y_bf", np.abs(ts.Y_bf[:B4].float().cpu().numpy() - Yk(sc["Y"])).max(), 2e-2),
               ("student state", np.abs(_np(out["student_state"]) - ref["student_state"]).max(), None),
               ("student pred", np.abs(_np(out["student_predictions"]) - ref["student_predictions"]).max(), 5e-3),
               ("dstate", np.abs(_np(g.state_grad()) - ref["dstate"]).max(), None))
    for what, e, bound in figures:
        print("%s %-14s err %.2e%s" % (tag, what, e, "" if bound is None else "  (bound %.0e)" % bound))
        if bound is not None and not e < bound:
            missed.append((what, e, bound))
    _grad_figures(tag, ts, ref["student_grads"], missed)
    assert not missed, missed


def test_pred_only_has_a_zero_state_gradient_behind_the_gate():
    """--distill_losses pred with a gated student: dstate is exactly zero and the gradient store equals a backward without dstate
    (B = 32 < 512: the column sums of both batch norms have one order)."""
    bt = _batch()
    g = _graph(("pred",), True, False)
    y = torch.from_numpy(bt["labels"].astype(np.uint8)).to(DEV)
    g.step(torch.from_numpy(bt["q"]).to(DEV), y, torch.from_numpy(bt["n"]).to(DEV), apply=False, num_frames_host=bt["n"])
    torch.cuda.synchronize()
    assert not g.state_grad().any()
    with_state = g.student.store.grad.clone()
    g.student.backward(g.label_grads()["student"])
    torch.cuda.synchronize()
    assert torch.equal(g.student.store.grad, with_state)
    with pytest.raises(ValueError, match=r"dstate \(32, 64\): the state of this tower is \(32, 128\)"):
        g.student.backward(g.label_grads()["student"], dstate=torch.zeros((B4, 64), device=DEV))
