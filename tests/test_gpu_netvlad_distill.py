"""Serial distillation over the NetVLAD towers: evc_bn_bwd_partial_add / _finalize_add bit for bit against the plain
entries fed the summed gradient, evc_frames_gather_packed_bn bit for bit against the two launches it replaces, the frozen tower as an
evaluation forward, the step against the float64 restatement tests/_netvlad_distill_ref.py, and train --teacher_dir / validate for
--model NetVLADModel end to end.  pytest -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _netvlad_distill_ref as dx
from oracle import model_math as mm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _np(t):
    return t.detach().cpu().double().numpy()


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


# ---------------------------------------------------------------------------- 1. the batch-norm backward with a second gradient
def _bn_case(R, C, seed):
    rng = np.random.default_rng(seed)
    x = _d(rng.standard_normal((R, C)) * 2.0 + 1.0)                  # pre-activations on both sides of 0 and of 6 after the scale
    dy, dy2 = _d(rng.standard_normal((R, C)) * 0.1), _d(rng.standard_normal((R, C)) * 0.1)
    mean, var = _d(0.2 * rng.standard_normal(C)), _d(np.exp(0.2 * rng.standard_normal(C)))
    gamma, beta = _d(2.0 * np.exp(0.2 * rng.standard_normal(C))), _d(1.0 + 0.2 * rng.standard_normal(C))
    return x, dy, dy2, mean, var, gamma, beta


def _bn_bwd(ops, add, x, dy, dy2, mean, var, gamma, beta, relu6):
    """Both passes; every output prefilled with NaN, one guard element behind each."""
    R, C = x.shape
    ws = torch.full((2 * C + 1,), NAN, dtype=torch.float64, device=DEV)
    dxf = torch.full((R * C + 1,), NAN, device=DEV)
    dxb = torch.full((R * C + 1,), NAN, dtype=torch.bfloat16, device=DEV)
    dg, db = torch.full((C + 1,), NAN, device=DEV), torch.full((C + 1,), NAN, device=DEV)
    if add:
        ops.bn_bwd_partial_add(x, dy, dy2, R, C, mean, var, gamma, beta, relu6, ws)
        ops.bn_bwd_finalize_add(x, dy, dy2, R, R, C, mean, var, gamma, beta, relu6, ws, dx_f32=dxf, dx_bf16=dxb, dgamma=dg, dbeta=db)
    else:
        ops.bn_bwd_partial(x, dy, R, C, mean, var, gamma, beta, relu6, ws)
        ops.bn_bwd_finalize(x, dy, R, R, C, mean, var, gamma, beta, relu6, ws, dx_f32=dxf, dx_bf16=dxb, dgamma=dg, dbeta=db)
    torch.cuda.synchronize()
    for t, n in ((dxf, R * C), (dxb, R * C), (dg, C), (db, C), (ws, 2 * C)):
        assert torch.isnan(t[n]) and torch.isfinite(t[:n].float()).all()
    return dxf[:R * C], dxb[:R * C], dg[:C], db[:C]


# (R, C): a single element; a column tail in the second 64-column block; more rows than the four row lanes; the last R at which
# evc_bn_bwd_partial launches ONE row block per column group (R < 512), so that the f64 column sums have one adder and one order.
@pytest.mark.parametrize("relu6", [True, False])
@pytest.mark.parametrize("R,C", [(1, 1), (7, 65), (33, 128), (511, 200)])
def test_bn_bwd_add_is_the_plain_entry_on_the_summed_gradient(R, C, relu6):
    """dx_f32, dx_bf16, dgamma, dbeta of the _add entries on (dy, dy2): torch.equal with the plain entries fed the f32 sum dy + dy2;
    dy2 = None: torch.equal with the plain entries on dy."""
    from efficientvideoclassification_youtube8m_amd import ops
    x, dy, dy2, mean, var, gamma, beta = _bn_case(R, C, 100 * R + C)
    if relu6 and R * C > 1:
        y = (x - mean) * torch.rsqrt(var + 1e-3) * gamma + beta
        inside = (y > 0) & (y < 6)
        assert inside.any() and not inside.all()                     # the mask has both values
    base = _bn_bwd(ops, False, x, dy, None, mean, var, gamma, beta, relu6)
    for got, want in zip(_bn_bwd(ops, True, x, dy, None, mean, var, gamma, beta, relu6), base):
        assert torch.equal(got, want)
    summed = _bn_bwd(ops, False, x, dy + dy2, None, mean, var, gamma, beta, relu6)
    added = _bn_bwd(ops, True, x, dy, dy2, mean, var, gamma, beta, relu6)
    for name, got, want in zip(("dx_f32", "dx_bf16", "dgamma", "dbeta"), added, summed):
        assert torch.equal(got, want), (name, R, C, relu6)
    if R * C > 1:
        assert not torch.equal(added[3], base[3])                    # (dy2 is not ignored)


def test_bn_bwd_add_refuses_max_pool_routing():
    """dy2 together with argmax: EVC_ERR_BAD_ARG from both entries, nothing launched (ws and the outputs keep their fill)."""
    from efficientvideoclassification_youtube8m_amd import _lib, ops
    R, C, S = 8, 16, 4
    x, dy, dy2, mean, var, gamma, beta = _bn_case(R, C, 1)
    am = torch.zeros((R // S, C), dtype=torch.int32, device=DEV)
    ws = torch.full((2 * C,), 3.0, dtype=torch.float64, device=DEV)
    dxf = torch.full((R, C), 3.0, device=DEV)
    with pytest.raises(_lib.EvcError, match=r"evc_bn_bwd_partial_add failed \(-5\).*dy2 with argmax"):
        ops.bn_bwd_partial_add(x, dy[:R // S], dy2, R, C, mean, var, gamma, beta, True, ws, am, S)
    with pytest.raises(_lib.EvcError, match=r"evc_bn_bwd_finalize_add failed \(-5\).*dy2 with argmax"):
        ops.bn_bwd_finalize_add(x, dy[:R // S], dy2, R, R, C, mean, var, gamma, beta, True, ws, am, S, dx_f32=dxf)
    torch.cuda.synchronize()
    assert bool((ws == 3.0).all()) and bool((dxf == 3.0).all())
    # without dy2 the _add entries route as the plain ones do
    ops.bn_bwd_partial_add(x, dy[:R // S], None, R, C, mean, var, gamma, beta, True, ws, am, S)
    want = torch.empty_like(ws)
    ops.bn_bwd_partial(x, dy[:R // S], R, C, mean, var, gamma, beta, True, want, am, S)
    assert torch.equal(ws, want)


# ---------------------------------------------------------------------------- 2. the fused input pass
def _stats(F, rng):
    """Statistics, scale and offset perturbed as DESIGN.md 7.14 perturbs them: 0.2 N(0,1) on mean and beta, exp(0.2 N(0,1)) on variance
    and gamma."""
    return (_d(0.2 * rng.standard_normal(F)), _d(np.exp(0.2 * rng.standard_normal(F))), _d(np.exp(0.2 * rng.standard_normal(F))),
            _d(0.2 * rng.standard_normal(F)))


# (4, 12, 8, ..): an empty video first, a one-row video last, F / 4 = 2 lanes.  (3, 40, 260, ..): F / 4 = 65, one float4 past the wave -
# the row loop takes a second trip -, an empty video in the middle.  (2, 300, 1152, ..): the shipped row length.  (8, 300, 1152, 1, ..):
# 2 251 rows, 2.6 M elements - a batch norm that read the unrounded product v * inv (a fused v * inv - mean) differs from bn_apply by an
# f32 ulp, which moves about one bf16 in 45 000: only this many elements show it (it happened, and the three small cases passed).
@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("B,T,F,every_n,n", [(4, 12, 8, 1, [0, 5, 12, 1]), (3, 40, 260, 3, [40, 0, 7]), (2, 300, 1152, 10, [300, 151]),
                                             (8, 300, 1152, 1, [300] * 7 + [151])])
def test_fused_input_pass_is_the_two_launches_bit_for_bit(B, T, F, every_n, n, u8):
    """evc_frames_gather_packed_bn against evc_frames_gather_packed followed by evc_bn_apply: torch.equal in r (rows < R; its rows
    R .. Rp are zeros too) and r_bn (rows < Rp, the zero rows included); rows >= Rp keep their NaN prefill.  normalize on."""
    from efficientvideoclassification_youtube8m_amd import ops
    rng = np.random.default_rng(B * 1000 + F)
    n = np.asarray(n, np.int32)
    plan = ops.GridPlan(n, every_n, T)
    R, Rp = plan.R, plan.Rp
    assert 0 < R < Rp
    q = rng.integers(0, 256, (B, T, F), dtype=np.uint8)
    x = torch.from_numpy(q).to(DEV) if u8 else _d(rng.standard_normal((B, T, F)))
    nd, off = torch.from_numpy(n).to(DEV), torch.from_numpy(plan.row_off).to(DEV)
    mean, var, gamma, beta = _stats(F, rng)
    r = torch.full((Rp + 3, F), NAN, device=DEV)
    r_bn = torch.full((Rp + 3, F), NAN, dtype=torch.bfloat16, device=DEV)
    ops.frames_gather_packed_bn(x, nd, off, every_n, R, Rp, mean, var, gamma, beta, r, r_bn, normalize=True)
    want_r = torch.full((Rp + 3, F), NAN, device=DEV)
    want_bn = torch.full((Rp + 3, F), NAN, dtype=torch.bfloat16, device=DEV)
    ops.frames_gather_packed(x, nd, off, every_n, R, Rp, want_r, normalize=True)
    ops.bn_apply(want_r, R, F, mean, var, gamma, beta, False, y_bf16=want_bn)
    want_bn[R:Rp].zero_()
    torch.cuda.synchronize()
    assert torch.isfinite(r[:Rp]).all() and torch.isfinite(r_bn[:Rp].float()).all()
    assert torch.equal(r[:R], want_r[:R]) and not r[R:Rp].any()
    assert torch.equal(r_bn[:Rp], want_bn[:Rp]) and not r_bn[R:Rp].any() and r_bn[:R].any()
    assert torch.isnan(r[Rp:]).all() and torch.isnan(r_bn[Rp:].float()).all()
    norms = r[:R].double().norm(dim=1)
    assert bool(((norms - 1.0).abs() < 1e-5).all())                  # (normalize is on; no row of these inputs is all zero)


def test_fused_input_pass_refuses_before_any_launch():
    """F % 4 != 0 and Rp - R >= 32 (EVC_ERR_BAD_SHAPE), a misaligned f32 input, output or per-column vector (EVC_ERR_BAD_ALIGN): no
    launch, the outputs keep their fill."""
    from efficientvideoclassification_youtube8m_amd import _lib, ops
    rng = np.random.default_rng(3)
    B, T, every_n = 2, 8, 1
    n = np.array([8, 3], np.int32)
    plan = ops.GridPlan(n, every_n, T)
    R, Rp = plan.R, plan.Rp
    nd, off = torch.from_numpy(n).to(DEV), torch.from_numpy(plan.row_off).to(DEV)

    def run(F, code, Rp_=Rp, shift=None):
        x = _d(rng.standard_normal((B, T, F)))
        rows = max(Rp_, Rp) + 1
        vecs = list(_stats(F, rng))
        r = torch.full((rows * F + 4,), 3.0, device=DEV)
        r_bn = torch.full((rows, F), 3.0, dtype=torch.bfloat16, device=DEV)
        out = r[:rows * F].view(rows, F)
        if shift == "out":
            out = r[1:1 + rows * F].view(rows, F)
        elif shift == "x":
            x = torch.cat([x.reshape(-1), x.reshape(-1)[:1]])[1:].view(B, T, F)
        elif shift is not None:
            vecs[shift] = torch.cat([vecs[shift], vecs[shift][:1]])[1:]
        with pytest.raises(_lib.EvcError, match=r"evc_frames_gather_packed_bn failed \(%d\)" % code):
            ops.frames_gather_packed_bn(x, nd, off, every_n, R, Rp_, *vecs, out, r_bn, normalize=True)
        torch.cuda.synchronize()
        assert bool((r == 3.0).all()) and bool((r_bn == 3.0).all())

    run(6, -1)
    run(8, -1, Rp_=R + 32)
    for shift in ("out", "x", 0, 1, 2, 3):
        run(8, -2, shift=shift)


# ---------------------------------------------------------------------------- 3. / 6. two towers compared bit for bit: a process of its own
@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """tests/_netvlad_distill_child.py, once, in a fresh process under EVC_DETERMINISTIC=1 (the library reads it once per process): the
    hidden layer's product is joined over K by f32 atomics otherwise, and two towers' f32 states then agree only up to that order."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    work = str(tmp_path_factory.mktemp("netvlad_distill"))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "_netvlad_distill_child.py"), work],
                       env=dict(os.environ, EVC_DETERMINISTIC="1"), capture_output=True, text=True, timeout=600)
    lines = [line for line in r.stdout.splitlines() if not line.startswith("Key: ")]
    print("\n".join(lines)[-6000:])
    return r, "\n".join(lines)


def test_frozen_tower_is_an_evaluation_forward(child):
    """A training=False grid tower's V, asum, state and predictions equal forward(is_training=False) of a training tower holding the same
    weights and moving statistics bit for bit, at every_n = 1, B = 8, T = 40, F = 128, K = 64, H = 64 - the one through the fused input
    pass, the other through the two launches."""
    r, out = child
    assert "deterministic 1" in out and "frozen: ok" in out, out[-3000:] + r.stderr[-3000:]
    for name in ("r", "r_bn", "V", "asum", "state", "predictions"):
        assert any(line.split() == ["frozen", name, "equal"] for line in out.splitlines()), name


# ---------------------------------------------------------------------------- 4. / 5. the step against float64
_SHARED = {}
B4, F4, K4, H4, V4, T4 = 32, 128, 64, 128, 33, 60


def _params(tw):
    pre = tw.scope + "/"
    return {k[len(pre):]: _np(v) for k, v in tw.state_dict().items()}


def _graph(on):
    """The graph of test 4 (teacher on every real frame, student on every 10th; one video empty, one of 3 frames).  Both towers' batch
    norms get perturbed scales and offsets, the teacher's moving statistics are its initial ones perturbed (0.2 N(0,1) on mean and beta,
    exp(0.2 N(0,1)) on variance and gamma) - not batch moments.  The batch, both towers' weights and the float64
    reference are made once and shared."""
    from efficientvideoclassification_youtube8m_amd.distill import NetVladDistillGraph
    g = NetVladDistillGraph(B4, every_n=10, teacher_every_n=1, feature_size=F4, vocab_size=V4, max_frames=T4, cluster_size=K4,
                            hidden_size=H4, device=DEV, seed=3, distill_losses=on)
    if not _SHARED:
        rng = np.random.default_rng(B4 + K4)
        q, x, n, labels = mm.synthetic_batch(B4, seed=B4, max_frames=T4, feature_size=F4, vocab_size=V4, dtype=np.float32)
        n[4], n[11] = 0, 3
        x[np.arange(T4)[None, :] >= n[:, None]] = 0.0
        y = torch.from_numpy(labels.astype(np.uint8)).to(DEV)
        dev = {True: (torch.from_numpy(q).to(DEV), y, torch.from_numpy(n).to(DEV)), False: (torch.from_numpy(x).to(DEV), y, torch.from_numpy(n).to(DEV))}
        for tw in (g.teacher, g.student):
            for k in tw.names:
                if k.endswith("/gamma") or k.endswith("/beta"):
                    z = torch.from_numpy(rng.standard_normal(tw.store.p(k).shape).astype(np.float32) * 0.2).to(DEV)
                    tw.store.p(k).copy_(tw.store.p(k) * torch.exp(z) if k.endswith("/gamma") else tw.store.p(k) + z)
            tw.refresh_shadows()
        for k, v in g.teacher.buffers.items():
            z = torch.from_numpy(rng.standard_normal(v.shape).astype(np.float32) * 0.2).to(DEV)
            v.copy_(v * torch.exp(z) if k.endswith("variance") else v + z)
        sds = (g.teacher.state_dict(), g.student.state_dict())
        teacher, student = _params(g.teacher), _params(g.student)
        moving = {k: teacher.pop(k) for k in list(teacher) if "/moving_" in k}
        for k in list(student):
            if "/moving_" in k:
                student.pop(k)
        xn = mm.l2_normalize(x.astype(np.float64), 2)
        _SHARED.update(n=n, labels=labels, dev=dev, sds=sds, xn=xn, teacher=teacher, moving=moving, student=student, ref={})
    sh = _SHARED
    g.teacher.load_state_dict(sh["sds"][0])
    g.student.load_state_dict(sh["sds"][1])
    if on not in sh["ref"]:
        sh["ref"][on] = dx.distill_step(sh["xn"], sh["n"], sh["labels"], sh["teacher"], sh["moving"], sh["student"], 1, 10, on=on)
    return g, sh, sh["ref"][on]


def _tf_grad(tw, k):
    got = tw.store.g(k)
    got = _np(got.t() if got.dim() == 2 else got)
    if k == tw.HW:
        got = got.reshape(tw.Kc, tw.F, tw.Hd).transpose(1, 0, 2).reshape(tw.F * tw.Kc, tw.Hd)
    return got


@pytest.mark.parametrize("u8", [True, False])
def test_step_against_float64(u8):
    """step(apply=False) with rep,pred,ce at B = 32, F = 128, K = 64, H = 128, V = 33, T = 60, teacher every_n = 1 (R = 1803), student
    every_n = 10 (R = 181); video 4 is empty, video 11 has 3 frames; uint8 and f32 input.  Bounds of DESIGN.md 7.18 / 7.14, none new: the
    four loss values 2e-2 relative (+ 1e-6); the teacher's predictions 5e-3; the student's a 2e-2, Y_bf 2e-2, predictions 5e-3; every
    student gradient tensor relative L2 0.12, or max abs 1e-3 where the reference gradient is zero up to rounding.  The one new
    operation, the f32 add in front of hidden1_bn's mask, is pinned exactly by test_bn_bwd_add_is_the_plain_entry_on_the_summed_gradient.
    Every figure is printed before the first assertion; the observed maxima are recorded in DESIGN.md 7.19."""
    g, sh, ref = _graph(("rep", "pred", "ce"))
    assert g.teacher.store.grad is None and g.teacher.store.m is None and g.student.training and not g.teacher.training
    t_before = g.teacher.store.master.clone()
    out = g.step(*sh["dev"][u8], apply=False, num_frames_host=sh["n"])
    torch.cuda.synchronize()
    assert g.global_step == 0 and out["global_step"] == 0
    assert set(out) >= {"predictions", "teacher_state", "loss", "student_predictions", "student_state", "num_frames_student",
                        "student_loss_state", "pred_loss", "student_label_loss", "global_step"}
    assert torch.equal(g.teacher.store.master, t_before)
    ts, tt = g.student, g.teacher
    sc, tc = ref["student_cache"], ref["teacher_cache"]
    R, Rt = sc["r"].shape[0], tc["r"].shape[0]
    assert ts.R == R == 181 and tt.R == Rt == 1803 and np.array_equal(ts.plan.k, sc["k"]) and np.array_equal(out["num_frames_student"].numpy(), sc["k"])
    assert not ts.Vv[4].any() and not tt.Vv[4].any()                 # the empty video
    rep = g.loss_report()
    missed = []
    for k in g.LOSS_SLOTS:
        print("u8=%d loss %-20s got %.6f  float64 %.6f  rel %.2e" % (u8, k, rep[k], float(ref[k]), abs(rep[k] - ref[k]) / abs(ref[k])))
        if not abs(rep[k] - ref[k]) <= 2e-2 * abs(ref[k]) + 1e-6:
            missed.append((k, rep[k], float(ref[k])))
    Yk = lambda Y: Y.reshape(B4, F4, K4).transpose(0, 2, 1).reshape(B4, K4 * F4)          # reference order f*K+k -> cluster-major
    figures = (("teacher a", np.abs(_np(tt.a[:Rt]) - tc["a"]).max(), None),
               ("teacher Y_bf", np.abs(tt.Y_bf[:B4].float().cpu().numpy() - Yk(tc["Y"])).max(), None),
               ("teacher pred", np.abs(_np(out["predictions"]) - ref["teacher_predictions"]).max(), 5e-3),
               ("teacher state", np.abs(_np(out["teacher_state"]) - ref["teacher_state"]).max(), None),
               ("student a", np.abs(_np(ts.a[:R]) - sc["a"]).max(), 2e-2),
               ("student Y_bf", np.abs(ts.Y_bf[:B4].float().cpu().numpy() - Yk(sc["Y"])).max(), 2e-2),
               ("student state", np.abs(_np(out["student_state"]) - ref["student_state"]).max(), None),
               ("student pred", np.abs(_np(out["student_predictions"]) - ref["student_predictions"]).max(), 5e-3),
               ("dstate", np.abs(_np(g.state_grad()) - ref["dstate"]).max(), None))
    for what, e, bound in figures:
        print("u8=%d %-14s err %.2e%s" % (u8, what, e, "" if bound is None else "  (bound %.0e)" % bound))
        if bound is not None and not e < bound:
            missed.append((what, e, bound))
    assert set(ref["student_grads"]) == set(ts.names)
    for k, want in ref["student_grads"].items():
        got = _tf_grad(ts, k)
        l2 = float(np.linalg.norm(got - want) / (np.linalg.norm(want) + 1e-30))
        mx = float(np.abs(got - want).max())
        print("u8=%d   grad %-28s rel l2 %.3e  max abs %.3e  (|ref|max %.3e)" % (u8, k, l2, mx, float(np.abs(want).max())))
        if not (l2 < 0.12 or mx < 1e-3):
            missed.append(("grad " + k, (l2, mx), (0.12, 1e-3)))
    assert not missed, missed


def test_pred_only_has_a_zero_state_gradient():
    """--distill_losses pred: dstate is exactly zero and the gradient store is that of backward(dpred) without dstate (B = 32 < 512:
    hidden1_bn's column sums have one order)."""
    g, sh, ref = _graph(("pred",))
    g.step(*sh["dev"][True], apply=False, num_frames_host=sh["n"])
    assert not g.state_grad().any() and not ref["dstate"].any()
    with_state = g.student.store.grad.clone()
    g.student.backward(g.label_grads()["student"])
    torch.cuda.synchronize()
    assert torch.equal(g.student.store.grad, with_state)
    rep = g.loss_report()
    for k in g.LOSS_SLOTS:                                           # a loss left out is still reported
        assert abs(rep[k] - ref[k]) <= 2e-2 * abs(ref[k]) + 1e-6, (k, rep[k], float(ref[k]))
    with pytest.raises(ValueError, match=r"dstate \(32, 64\): the state of this tower is \(32, 128\)"):
        g.student.backward(g.label_grads()["student"], dstate=torch.zeros((B4, 64), device=DEV))


def test_distillation_through_train_main(child):
    """train.main on synthetic data at test_step_against_float64's sizes: a teacher for 4 steps on every real frame, then --teacher_dir
    with --every_n 10 for 4 steps (finite losses, model/* the teacher checkpoint's bits, the four metadata entries, a fresh forward-only
    tower from model_student/* reproducing the evaluation predictions bit for bit), validate.main on the result (the student's metrics,
    equal to eval_util on the host; student_state_loss logged), a resume, --student_init_from_teacher and a size mismatch."""
    r, out = child
    assert "workflow: ok" in out and r.returncode == 0, out[-3000:] + r.stderr[-3000:]
    assert "reproduces the student's evaluation predictions bit for bit" in out and "student_state_loss" in out


# ---------------------------------------------------------------------------- 7. two runs
def test_two_runs_give_the_same_bits():
    """tests/_netvlad_distill_twice.py in a fresh process under EVC_DETERMINISTIC=1: losses, gradient store and master weights of two
    graphs on the same seeds and batch, after each of two steps."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "_netvlad_distill_twice.py")],
                       env=dict(os.environ, EVC_DETERMINISTIC="1"), capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "step 1: master weights" in r.stdout and "DIFFERS" not in r.stdout and "deterministic 1" in r.stdout
