"""Serial distillation over the NeXtVLAD towers: the f32-MFMA aggregation entry bit for bit against the entry the
training towers call, evc_nextvlad_gate_bwd_add, the frozen tower as an evaluation forward, the student's gradients against the float64
restatement tests/_nextvlad_distill_ref.py, and train --teacher_dir for --model NeXtVLADModel end to end.  pytest -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _nextvlad_distill_ref as dx
from oracle import model_math as mm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _np(t):
    return t.detach().cpu().double().numpy()


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


# P_b = k_b G.  (4, 18, 20): no row, 4 pairs (less than one load batch of 8), 64, 68, 132, 160 pairs; K and D below one 32 x 32 block.
# (3, 7, 12): the empty video first and last, odd L_b = 15 and 6.  (1, 40, 100): K across the 32-row blocks of a workgroup's waves, D
# across the 96-column workgroup tile (second tile: 4 live columns), L_b = 1, 2, 3, 63, 64, 65, 0 and - on the LAST video, whose
# unused second contraction slot would be the first row at R - 129.  (8, 128, 288): the shipped tile shape, 3 workgroups per video.
@pytest.mark.parametrize("G,K,D,ks", [(4, 18, 20, (0, 1, 16, 17, 33, 40)), (3, 7, 12, (0, 5, 2, 0)),
                                      (1, 40, 100, (1, 2, 3, 63, 64, 65, 0, 129)), (8, 128, 288, (30, 7))])
def test_mfma_aggregation_is_the_existing_entry_bit_for_bit(G, K, D, ks):
    """evc_nextvlad_aggregate_packed_fwd_mfma: torch.equal with evc_nextvlad_aggregate_packed_fwd on V and asum, twice with equal
    bits, and against numpy float64 at 1e-4 x max(1, |ref|max) (the bound of test_packed_aggregation_in_f32_against_numpy).  Every row
    of a and xe at and beyond R is NaN and the outputs are prefilled with NaN: all of V[B,K,D] / asum[B,K] is written and finite -
    nothing beyond a video's rows entered a sum, not even times zero - and the guard row behind them keeps its NaN."""
    from efficientvideoclassification_youtube8m_amd import ops
    rng = np.random.default_rng(5 + G)
    B, T = len(ks), 160
    k = np.array(ks)
    off = np.concatenate([[0], np.cumsum(k)]).astype(np.int32)
    R, max_k = int(off[-1]), int(k.max())
    big = lambda ref: max(1.0, float(np.abs(ref).max()))
    a = rng.random((R, G, K)) * rng.random((R, G, 1))
    xe = rng.standard_normal((R, G, D)); c2 = rng.standard_normal((K, D))
    asum_ref = np.zeros((B, K)); V_ref = np.zeros((B, K, D))
    for b in range(B):
        asum_ref[b] = a[off[b]:off[b + 1]].sum((0, 1))
        V_ref[b] = np.einsum("rgk,rgd->kd", a[off[b]:off[b + 1]], xe[off[b]:off[b + 1]]) - asum_ref[b][:, None] * c2
    d_a = torch.full((R + 9, G * K), NAN, device=DEV); d_a[:R] = _d(a.reshape(R, G * K))
    d_xe = torch.full((R + 9, G * D), NAN, device=DEV); d_xe[:R] = _d(xe.reshape(R, G * D))
    d_c2, d_off = _d(c2), torch.from_numpy(off).to(DEV)
    outs = {}
    for name, fn in (("vector", ops.nextvlad_aggregate_packed_fwd), ("mfma", ops.nextvlad_aggregate_packed_fwd_mfma)):
        V = torch.full((B + 1, K, D), NAN, device=DEV); asum = torch.full((B + 1, K), NAN, device=DEV)
        fn(d_a, d_xe, d_off, B, T, G, K, D, R, max_k, d_c2, V, asum)
        first = (V.clone(), asum.clone())
        fn(d_a, d_xe, d_off, B, T, G, K, D, R, max_k, d_c2, V, asum)
        torch.cuda.synchronize()
        assert torch.equal(V[:B], first[0][:B]) and torch.equal(asum[:B], first[1][:B]), name           # two runs, the same bits
        assert torch.isnan(V[B]).all() and torch.isnan(asum[B]).all(), name
        assert torch.isfinite(V[:B]).all() and torch.isfinite(asum[:B]).all(), name
        outs[name] = (V[:B], asum[:B])
    Vm, sm = outs["mfma"]
    err_v, err_s = np.abs(_np(Vm) - V_ref).max(), np.abs(_np(sm) - asum_ref).max()
    nv, ns = int((Vm != outs["vector"][0]).sum()), int((sm != outs["vector"][1]).sum())
    print("mfma aggregate G=%d K=%d D=%d: V err %.2e (|ref| %.1f)  asum err %.2e  elements differing from the vector entry: V %d  asum %d"
          % (G, K, D, err_v, big(V_ref), err_s, nv, ns))
    assert torch.equal(Vm, outs["vector"][0]) and torch.equal(sm, outs["vector"][1])
    assert err_v < 1e-4 * big(V_ref) and err_s < 1e-4 * big(asum_ref)
    for b in np.flatnonzero(k == 0):
        assert not Vm[b].any() and not sm[b].any()                   # zeros, not merely small


def test_mfma_entry_refuses_bad_shapes():
    """The refusals of test_packed_entries_refuse_bad_shapes hold for the new entry; nothing is launched."""
    from efficientvideoclassification_youtube8m_amd import _lib, ops
    B, T, G, K, R = 2, 8, 2, 8, 6
    off = torch.tensor([0, 2, 6], dtype=torch.int32, device=DEV)
    for D, max_k in ((6, 4), (8, 9), (8, 2)):                        # D % 4 != 0; max_k > T; R > B * max_k
        a = torch.zeros((R, G * K), device=DEV); xe = torch.zeros((R, G * D), device=DEV); c2 = torch.zeros((K, D), device=DEV)
        V = torch.full((B, K, D), 3.0, device=DEV); asum = torch.full((B, K), 3.0, device=DEV)
        with pytest.raises(_lib.EvcError, match=r"evc_nextvlad_aggregate_packed_fwd_mfma failed \(-1\)"):
            ops.nextvlad_aggregate_packed_fwd_mfma(a, xe, off, B, T, G, K, D, R, max_k, c2, V, asum)
        torch.cuda.synchronize()
        assert bool((V == 3.0).all()) and bool((asum == 3.0).all())


@pytest.mark.parametrize("n", [1, 7, 4096 + 3])
def test_gate_bwd_add(n):
    """dout2 = None: the bits of evc_nextvlad_gate_bwd.  With dout2: evc_nextvlad_gate_bwd fed the torch f32 sum dout + dout2, bit for
    bit in dh, dgl and dgl_bf16."""
    from efficientvideoclassification_youtube8m_amd import ops
    g = torch.Generator(device=DEV); g.manual_seed(n)
    h, gl, dout, dout2 = (torch.randn(n, device=DEV, generator=g) * s for s in (1.0, 2.0, 0.1, 0.1))

    def run(fn, *grads):
        dh, dgl = torch.full((n + 1,), NAN, device=DEV), torch.full((n + 1,), NAN, device=DEV)
        dgl_bf = torch.full((n + 1,), NAN, dtype=torch.bfloat16, device=DEV)
        fn(h, gl, *grads, dh, dgl, dgl_bf)
        torch.cuda.synchronize()
        assert torch.isnan(dh[n]) and torch.isnan(dgl[n]) and torch.isnan(dgl_bf[n])
        assert torch.isfinite(dh[:n]).all() and torch.isfinite(dgl[:n]).all()
        return dh[:n], dgl[:n], dgl_bf[:n]

    base = run(ops.nextvlad_gate_bwd, dout)
    for got, want in zip(run(ops.nextvlad_gate_bwd_add, dout, None), base):
        assert torch.equal(got, want)
    summed = run(ops.nextvlad_gate_bwd, dout + dout2)
    added = run(ops.nextvlad_gate_bwd_add, dout, dout2)
    for got, want in zip(added, summed):
        assert torch.equal(got, want)
    assert not torch.equal(added[0], base[0])


SMALL = dict(max_frames=300, feature_size=128, vocab_size=40, cluster_size=16, hidden_size=128, groups=4, expansion=2, gating_reduction=2,
             device=DEV)


def _perturb_moving(tw, rng):
    for k, v in tw.buffers.items():
        r = torch.from_numpy(rng.random(v.shape).astype(np.float32)).to(DEV)
        v.copy_(v * (1.0 + 0.1 * r) if k.endswith("variance") else v + 0.05 * (r - 0.5))


def test_frozen_tower_is_an_evaluation_forward():
    """A training=False grid tower (every real frame, ragged n, uint8 input) with a trained tower's weights and perturbed moving
    statistics: predictions and state are the bits of the trained tower's forward(is_training=False) - which aggregates on the vector
    ALU, the frozen tower on the MFMA - and it holds neither a gradient store nor moments nor backward buffers."""
    from efficientvideoclassification_youtube8m_amd.towers import NeXtVladTower
    B = 8
    rng = np.random.default_rng(2)
    q, x, n, labels = mm.synthetic_batch(B, seed=9, feature_size=128, vocab_size=40, dtype=np.float32)
    n[0], n[3] = 1, 300
    qd, nd = torch.from_numpy(q).to(DEV), torch.from_numpy(n).to(DEV)
    trained = NeXtVladTower(B, frames="grid", every_n=1, seed=3, **SMALL)
    trained.forward(qd, nd, num_frames_host=n)                       # batch moments into the moving statistics
    _perturb_moving(trained, rng)
    want_pred = trained.forward(qd, nd, num_frames_host=n, is_training=False).clone()
    want_state = trained.state.clone()
    frozen = NeXtVladTower(B, frames="grid", every_n=1, seed=11, training=False, **SMALL)
    assert frozen.store.grad is None and frozen.store.m is None and frozen.store.v is None and not hasattr(frozen, "dxe")
    frozen.load_state_dict(trained.state_dict())
    got = frozen.forward(qd, nd, num_frames_host=n, is_training=False)
    torch.cuda.synchronize()
    assert frozen.state.shape == (B, 128) and torch.equal(frozen.Vv, trained.Vv) and torch.equal(frozen.asum, trained.asum)
    assert torch.equal(got, want_pred) and torch.equal(frozen.state, want_state)
    assert not torch.equal(got, trained.forward(qd, nd, num_frames_host=n, is_training=True))     # (the statistics matter)
    with pytest.raises(AssertionError, match="training-mode forward"):
        frozen.backward(torch.zeros_like(got))


_SHARED = {}
B4, F4, LAM, G4, K4, H4, RHO, V4, T4 = 32, 192, 2, 8, 24, 128, 2, 33, 300


def _params(tw):
    pre = tw.scope + "/"
    return {k[len(pre):]: _np(v) for k, v in tw.state_dict().items()}


def _graph(on):
    """The graph of test 4 (teacher on every real frame, student on every 10th), perturbed as the existing tower test perturbs: the
    batch-norm scales, offsets and the biases of both towers, and the teacher's moving statistics.  The batch, both towers' weights
    and the float64 reference are made once and shared."""
    from efficientvideoclassification_youtube8m_amd.distill import NeXtVladDistillGraph
    g = NeXtVladDistillGraph(B4, every_n=10, teacher_every_n=1, feature_size=F4, vocab_size=V4, max_frames=T4, cluster_size=K4,
                             hidden_size=H4, groups=G4, expansion=LAM, gating_reduction=RHO, device=DEV, seed=3, distill_losses=on)
    if not _SHARED:
        rng = np.random.default_rng(B4 + K4)
        q, x, n, labels = mm.synthetic_batch(B4, seed=B4, feature_size=F4, vocab_size=V4, dtype=np.float32)
        dev = (torch.from_numpy(q).to(DEV), torch.from_numpy(labels.astype(np.uint8)).to(DEV), torch.from_numpy(n).to(DEV))
        for tw in (g.teacher, g.student):
            for k in tw.names:
                if k.endswith("/gamma") or k.endswith("/beta") or k in (tw.EB, tw.AB):
                    tw.store.p(k).add_(torch.from_numpy(rng.standard_normal(tw.store.p(k).shape).astype(np.float32) * 0.2).to(DEV))
            tw.refresh_shadows()
        # the teacher's moving statistics, perturbed as the scales and offsets are: 0.2 N(0, 1) on their initial values - added to
        # the mean (0), and, a variance having to stay positive, as the factor exp(0.2 N(0, 1)) on the variance (1)
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
    K, D, H = tw.Kc, tw.D, tw.Hd
    if k == tw.HW:
        got = got.reshape(K, D, H).transpose(1, 0, 2).reshape(D * K, H)
    elif k.startswith("vlad_bn/"):
        got = got.reshape(K, D).T.reshape(-1)
    return got


def test_student_gradients_against_float64():
    """step(apply=False) with rep,pred,ce at B = 32, F = 192, lambda = 2, G = 8, K = 24, H = 128, rho = 2, V = 33, T = 300 on the synthetic
    batch's own lengths, uint8 input, teacher every_n = 1, student every_n = 10.  The four loss values within 2e-2 relative + 1e-6 (the
    bound of the H-LSTM serial-distillation loss test); the teacher's predictions 5e-3, the student's a 2e-2, Y_bf 2e-2, predictions
    5e-3 and every student gradient tensor relative L2 0.12 or max abs 1e-3 (the bounds of
    test_grid_tower_forward_backward_against_reference: the arithmetic in front of each quantity is unchanged, and the one new
    operation, the f32 add at `out`, is pinned exactly by test_gate_bwd_add).  Every figure is printed before the first assertion.

    Measured on an MI355X (teacher R = 6506, student R = 665; L_REP 227.6, L_PRED 6.54, L_CE 15.97): losses within 9.6e-4 relative;
    teacher predictions 3.5e-3 (its a 5.6e-5, Y_bf 3.8e-3, state 2.2e-2); student a 1.5e-3, Y_bf 1.18e-2, predictions 1.9e-3, state
    1.8e-2, dstate 2.8e-3; largest relative L2 of a gradient 0.089 (gating_weights_1), except vlad_bn/beta, whose true gradient is zero up
    to rounding and which is within 8.8e-4 absolute - a thin margin: that residual is the bf16 rounding of dhid summed over the batch,
    and it grows with the gradient that flows, here mostly dstate.  The teacher's moving statistics are its initial ones perturbed as
    the scales and offsets are.  With its batch moments on this batch instead (moved by a few per cent; L_REP 662) the teacher's
    predictions were 8.4e-3 and vlad_bn/beta 2.0e-3 off: at every_n = 1 the descriptors of i.i.d. synthetic videos are nearly equal,
    vlad_bn's batch variance is far below its epsilon, and an evaluation forward on such statistics multiplies every common error of
    U by about 31."""
    g, sh, ref = _graph(("rep", "pred", "ce"))
    assert g.teacher.store.grad is None and g.teacher.store.m is None and g.student.training and not g.teacher.training
    t_before = g.teacher.store.master.clone()
    out = g.step(*sh["dev"], apply=False, num_frames_host=sh["n"])
    torch.cuda.synchronize()
    assert g.global_step == 0 and out["global_step"] == 0
    assert set(out) >= {"predictions", "teacher_state", "loss", "student_predictions", "student_state", "num_frames_student",
                        "student_loss_state", "pred_loss", "student_label_loss", "global_step"}
    assert torch.equal(g.teacher.store.master, t_before)
    ts = g.student
    B, G, K, D = B4, G4, K4, ts.D
    sc = ref["student_cache"]
    R = sc["r"].shape[0]
    assert ts.R == R and np.array_equal(ts.plan.k, sc["k"]) and g.teacher.R == int(np.minimum(sh["n"], T4).sum())
    rep = g.loss_report()
    missed = []
    for k in g.LOSS_SLOTS:
        print("loss %-20s got %.6f  float64 %.6f  rel %.2e" % (k, rep[k], float(ref[k]), abs(rep[k] - ref[k]) / abs(ref[k])))
        if not abs(rep[k] - ref[k]) <= 2e-2 * abs(ref[k]) + 1e-6:
            missed.append((k, rep[k], float(ref[k])))
    Yk = sc["Y"].reshape(B, D, K).transpose(0, 2, 1).reshape(B, K * D)
    tt, tc = g.teacher, ref["teacher_cache"]
    Rt = tc["r"].shape[0]
    Yt = tc["Y"].reshape(B, D, K).transpose(0, 2, 1).reshape(B, K * D)
    figures = (("teacher a", np.abs(_np(tt.a[:Rt]).reshape(Rt, G, K) - tc["a"]).max(), None),
               ("teacher Y_bf", np.abs(tt.Y_bf[:B].float().cpu().numpy() - Yt).max(), None),
               ("teacher pred", np.abs(_np(out["predictions"]) - ref["teacher_predictions"]).max(), 5e-3),
               ("teacher state", np.abs(_np(out["teacher_state"]) - ref["teacher_state"]).max(), None),
               ("student a", np.abs(_np(ts.a[:R]).reshape(R, G, K) - sc["a"]).max(), 2e-2),
               ("student Y_bf", np.abs(ts.Y_bf[:B].float().cpu().numpy() - Yk).max(), 2e-2),
               ("student state", np.abs(_np(out["student_state"]) - ref["student_state"]).max(), None),
               ("student pred", np.abs(_np(out["student_predictions"]) - ref["student_predictions"]).max(), 5e-3),
               ("dstate", np.abs(_np(g.state_grad()) - ref["dstate"]).max(), None))
    for what, e, bound in figures:
        print("%-14s err %.2e%s" % (what, e, "" if bound is None else "  (bound %.0e)" % bound))
        if bound is not None and not e < bound:
            missed.append((what, e, bound))
    assert set(ref["student_grads"]) == set(ts.names)
    for k, want in ref["student_grads"].items():
        got = _tf_grad(ts, k)
        l2 = float(np.linalg.norm(got - want) / (np.linalg.norm(want) + 1e-30))
        mx = float(np.abs(got - want).max())
        print("  grad %-28s rel l2 %.3e  max abs %.3e" % (k, l2, mx))
        if not (l2 < 0.12 or mx < 1e-3):
            missed.append(("grad " + k, (l2, mx), (0.12, 1e-3)))
    assert not missed, missed


def test_pred_only_has_a_zero_state_gradient():
    """--distill_losses pred: dstate is exactly zero and the gradient store is that of backward(dpred) without dstate."""
    g, sh, ref = _graph(("pred",))
    g.step(*sh["dev"], apply=False, num_frames_host=sh["n"])
    assert not g.state_grad().any() and not ref["dstate"].any()
    with_state = g.student.store.grad.clone()
    g.student.backward(g.label_grads()["student"])
    torch.cuda.synchronize()
    assert torch.equal(g.student.store.grad, with_state)
    rep = g.loss_report()
    for k in g.LOSS_SLOTS:                                           # a loss left out is still reported
        assert abs(rep[k] - ref[k]) <= 2e-2 * abs(ref[k]) + 1e-6, (k, rep[k], float(ref[k]))


def test_distillation_through_train_main(tmp_path):
    """train.main on synthetic data at the sizes of test_grid_through_train_main: a teacher for 4 steps on every real frame, then
    --teacher_dir with --every_n 10 for 4 steps, a resume, and a student started from the teacher's weights."""
    from efficientvideoclassification_youtube8m_amd import train
    from efficientvideoclassification_youtube8m_amd.distill import NeXtVladDistillGraph
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    from efficientvideoclassification_youtube8m_amd.towers import NeXtVladTower
    tdir, sdir, idir = (str(tmp_path / d) + "/" for d in ("teacher", "student", "init"))
    common = ["--train_data_pattern", "synthetic", "--frame_features", "True", "--feature_names", "rgb, audio", "--model", "NeXtVLADModel",
              "--batch_size", "16", "--nextvlad_frames", "grid", "--nextvlad_cluster_size", "16", "--nextvlad_groups", "4",
              "--nextvlad_hidden_size", "128", "--nextvlad_gating_reduction", "2", "--feature_sizes", "64, 64", "--synthetic_videos", "64",
              "--num_epochs", "1", "--base_learning_rate", "0.01"]
    kw = dict(max_frames=300, feature_size=128, vocab_size=train.NUM_CLASSES, cluster_size=16, hidden_size=128, groups=4, expansion=2,
              gating_reduction=2, device=DEV)
    try:
        FLAGS.reset()
        res = train.main(common + ["--train_dir", tdir, "--every_n", "1", "--start_new_model", "True"])
        assert res["iterations"] == 4
        tck = train.latest_checkpoint(tdir)
        tsd = torch.load(tck)
        assert tsd["nextvlad_frames"] == "grid" and tsd["every_n"] == 1
        FLAGS.reset()
        res = train.main(common + ["--train_dir", sdir, "--every_n", "10", "--start_new_model", "True", "--teacher_dir", tdir])
        g = res["graph"]
        assert isinstance(g, NeXtVladDistillGraph) and res["iterations"] == 4 and g.global_step == 4
        assert (g.every_n, g.teacher_every_n, g.teacher.every_n, g.student.every_n) == (10, 1, 1, 10)
        hist = [h[1] for h in res["history"]]
        total = [2.0 * h["student_loss_state"] + h["pred_loss"] + h["student_label_loss"] for h in hist]
        print("nextvlad distillation losses", hist, "totals", total)
        assert all(np.isfinite(v) for h in hist for v in h.values()) and total[-1] < total[0]             # it trains
        sd = torch.load(train.latest_checkpoint(sdir))
        assert (sd["nextvlad_frames"], sd["every_n"], sd["teacher_every_n"], sd["distill_losses"]) == ("grid", 10, 1, "rep,pred,ce")
        assert sd["distill_mode"] == "serial" and "model/adam" not in sd and "model_student/adam" in sd
        names = [k for k, v in tsd.items() if k.startswith("model/") and torch.is_tensor(v)]
        assert len(names) == 28
        for k in names:
            assert torch.equal(sd[k], tsd[k]), k                                                           # the teacher: never written
            ks = "model_student/" + k[len("model/"):]
            assert sd[ks].shape == tsd[k].shape and sd[ks].dtype == tsd[k].dtype, ks                       # the single tower's names and shapes
        # a fresh grid tower from model_student/* against the trained student, in evaluation mode on one batch
        q, x, n, labels = mm.synthetic_batch(16, seed=4, feature_size=128, vocab_size=train.NUM_CLASSES, dtype=np.float32)
        qd, nd = torch.from_numpy(q).to(DEV), torch.from_numpy(n).to(DEV)
        last = g.student.forward(qd, nd, num_frames_host=n, is_training=False).clone()
        fresh = NeXtVladTower(16, frames="grid", every_n=10, seed=9, **kw)
        fresh.load_state_dict(sd, prefix="model_student")
        assert torch.equal(fresh.forward(qd, nd, num_frames_host=n, is_training=False), last)
        # resume: both towers from --train_dir; --teacher_dir (an empty directory here) only selects the mode
        FLAGS.reset()
        res = train.main(common + ["--train_dir", sdir, "--every_n", "10", "--teacher_dir", str(tmp_path / "nothing_here") + "/",
                                   "--max_steps", "1", "--student_init_from_teacher", "True"])
        assert res["iterations"] == 1 and res["graph"].global_step == 5 and res["graph"].student.adam_t == 5
        sd5 = torch.load(train.latest_checkpoint(sdir))
        assert sd5["global_step"] == 5 and sd5["teacher_every_n"] == 1
        assert all(torch.equal(sd5[k], tsd[k]) for k in names)
        assert not torch.equal(sd5["model_student/expansion_weights"], sd["model_student/expansion_weights"])
        # a new student from the teacher's weights and moving statistics: before its first step (no batch: --synthetic_videos 0) it is
        # the teacher's weights run on the student's frames
        FLAGS.reset()
        res = train.main([a if a != "64" else "0" for a in common] +
                         ["--train_dir", idir, "--every_n", "10", "--start_new_model", "True", "--teacher_dir", tdir,
                          "--student_init_from_teacher", "True"])
        gi = res["graph"]
        assert res["iterations"] == 0 and gi.global_step == 0
        on_student_frames = NeXtVladTower(16, frames="grid", every_n=10, seed=9, **kw)
        on_student_frames.load_state_dict(tsd)
        assert torch.equal(gi.student.forward(qd, nd, num_frames_host=n, is_training=False),
                           on_student_frames.forward(qd, nd, num_frames_host=n, is_training=False))
        # sizes that are not the checkpoint's
        FLAGS.reset()
        with pytest.raises(ValueError, match=r"model/cluster_weights of model.ckpt-4.pt has shape \(256, 64\), the size flags.*\(256, 128\)"):
            train.main([a if a != "16" or common[i - 1] != "--nextvlad_cluster_size" else "32" for i, a in enumerate(common)] +
                       ["--train_dir", str(tmp_path / "x") + "/", "--every_n", "10", "--start_new_model", "True", "--teacher_dir", tdir])
    finally:
        FLAGS.reset()


def test_two_runs_give_the_same_bits():
    """tests/_nextvlad_distill_twice.py in a fresh process under EVC_DETERMINISTIC=1: losses, gradient store and master weights of
    two graphs on the same seeds and batch, after each of two steps."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "_nextvlad_distill_twice.py")],
                       env=dict(os.environ, EVC_DETERMINISTIC="1"), capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "step 1: master weights" in r.stdout and "DIFFERS" not in r.stdout and "deterministic 1" in r.stdout
