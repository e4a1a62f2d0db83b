"""NeXtVLAD tower (extension: the reference's NeXtVLADModel is an empty stub - no reference math; the binding definition is
DESIGN.md 7.12) against its float64 restatement tests/_nextvlad_ref.py (itself checked against finite differences on the CPU):
the kernels of csrc/evc_nextvlad.hip alone in f32, their refusals, the tower's forward and gradients, and the public interface
(create_model, train.main).  pytest -m gpu."""
import numpy as np
import pytest
import torch

import _nextvlad_ref as nx
from oracle import model_math as mm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _np(t):
    return t.detach().cpu().double().numpy()


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _sig(x):
    return mm.sigmoid(np.asarray(x, np.float64))


def _twice(fn, *outs):
    """fn() fills `outs`; a second call on the same inputs must give the same bits (fixed-order sums, no atomics)."""
    fn()
    first = [o.clone() for o in outs]
    fn()
    torch.cuda.synchronize()
    for o, f in zip(outs, first):
        assert torch.equal(o, f)


# K, G and D/4 odd or not a power of two; the S*G = 1024 edge; and a K that is no multiple of 4 (the aggregation backward's
# transposed dV is padded to 4 columns there and da is stored element by element)
@pytest.mark.parametrize("B,S,G,K,D", [(5, 7, 3, 24, 20), (2, 64, 16, 8, 4), (3, 5, 2, 7, 12)])
def test_nextvlad_kernels_in_f32_against_numpy(B, S, G, K, D):
    """csrc/evc_nextvlad.hip alone (no GEMM, no bf16): assignment fwd/bwd, aggregation fwd/bwd, the centre gradient through
    evc_netvlad_dcenters, normalisation fwd/bwd, context gate fwd/bwd, the column sum - against numpy float64 to f32 accuracy.
    Bounds as in test_netvlad_kernels_in_f32_against_numpy: 1e-6 absolute for softmax-type outputs (values <= 1 from one exp and
    one reciprocal, ~2 ulp each), 1e-5 for their reverse mode, 1e-4 (1e-3 for da) x max(1, |ref|max) for the sums; the gate is
    h times a sigmoid with ~2e-6 relative error, |h| < 5: 1e-5 x max(1, |ref|max)."""
    from efficientvideoclassification_youtube8m_amd import ops
    rng = np.random.default_rng(2 + S)
    R, E = B * S, G * D
    big = lambda ref: max(1.0, float(np.abs(ref).max()))
    # ---- assignment
    act = rng.standard_normal((R, G * K)); mean = rng.standard_normal(G * K) * 0.1; var = rng.random(G * K) + 0.5
    ga = 1 + 0.2 * rng.standard_normal(G * K); be = 0.2 * rng.standard_normal(G * K)
    ld = G + 3                                                        # a padded row of attention logits
    attl = rng.standard_normal((R, ld)); ab = 0.3 * rng.standard_normal(G)
    attl[3, 1] = -40.0                                                # a sigmoid that all but underflows: att ~ 4e-18
    y = ((act - mean) / np.sqrt(var + 1e-3) * ga + be).reshape(R, G, K)
    e = np.exp(y - y.max(2, keepdims=True)); p_ref = e / e.sum(2, keepdims=True)
    att_ref = _sig(attl[:, :G] + ab)
    a_ref = p_ref * att_ref[:, :, None]
    d_act, d_mean, d_var, d_ga, d_be, d_attl, d_ab = _d(act), _d(mean), _d(var), _d(ga), _d(be), _d(attl), _d(ab)
    a = torch.empty((R, G * K), device=DEV)
    _twice(lambda: ops.nextvlad_assign_fwd(d_act, R, G, K, d_mean, d_var, d_ga, d_be, d_attl, a, att_bias=d_ab), a)
    assert np.abs(_np(a).reshape(R, G, K) - a_ref).max() < 1e-6
    da = rng.standard_normal((R, G, K)); d_da = _d(da)
    dz = torch.empty((R, G * K), device=DEV); datt = torch.empty((R, G), device=DEV)
    datt_bf = torch.zeros((R, 64), dtype=torch.bfloat16, device=DEV)
    _twice(lambda: ops.nextvlad_assign_bwd(d_act, R, G, K, d_mean, d_var, d_ga, d_be, d_attl, d_da, dz, datt, att_bias=d_ab,
                                           datt_logit_bf16=datt_bf), dz, datt, datt_bf)
    t_ref = (p_ref * da).sum(2)
    dz_ref = p_ref * att_ref[:, :, None] * (da - t_ref[:, :, None])
    datt_ref = t_ref * att_ref * (1 - att_ref)
    assert torch.isfinite(dz).all() and torch.isfinite(datt).all()
    assert np.abs(_np(dz).reshape(R, G, K) - dz_ref).max() < 1e-5 * big(dz_ref)
    assert np.abs(_np(datt) - datt_ref).max() < 1e-5 * big(datt_ref)
    assert np.abs(_np(dz).reshape(R, G, K)[3, 1]).max() < 1e-15 and abs(float(datt[3, 1])) < 1e-15      # the -40 group: ~1e-18, not NaN
    assert torch.equal(datt_bf[:, :G], datt.bfloat16()) and not datt_bf[:, G:].any()
    # ---- aggregation
    xe = rng.standard_normal((R, E)); c2 = rng.standard_normal((K, D))
    a4 = a_ref.reshape(B, S, G, K); x4 = xe.reshape(B, S, G, D)
    asum_ref = a4.sum((1, 2))
    V_ref = np.einsum("bsgk,bsgd->bkd", a4, x4) - asum_ref[:, :, None] * c2[None]
    d_a, d_xe, d_c2 = _d(a_ref), _d(xe), _d(c2)
    V = torch.empty((B, K, D), device=DEV); asum = torch.empty((B, K), device=DEV)
    _twice(lambda: ops.nextvlad_aggregate_fwd(d_a, d_xe, B, S, G, K, D, d_c2, V, asum), V, asum)
    assert np.abs(_np(V) - V_ref).max() < 1e-4 * big(V_ref) and np.abs(_np(asum) - asum_ref).max() < 1e-4 * big(asum_ref)
    # ---- normalisation
    U = torch.empty((B, K, D), device=DEV); nrm = torch.empty((B, K), device=DEV)
    d_V = _d(V_ref)
    _twice(lambda: ops.nextvlad_normalize_fwd(d_V, B, K, D, U, nrm), U, nrm)
    n_ref = np.maximum(np.sqrt((V_ref ** 2).sum(2)), 1e-12); U_ref = V_ref / n_ref[:, :, None]
    assert np.abs(_np(U) - U_ref).max() < 1e-6 and np.abs(_np(nrm) - n_ref).max() < 1e-4 * big(n_ref)
    dU = rng.standard_normal((B, K, D)); dV = torch.empty((B, K, D), device=DEV)
    d_n, d_dU = _d(n_ref), _d(dU)
    _twice(lambda: ops.nextvlad_normalize_bwd(d_V, d_n, d_dU, B, K, D, dV), dV)
    dV_ref = (dU - U_ref * (U_ref * dU).sum(2, keepdims=True)) / n_ref[:, :, None]
    assert np.abs(_np(dV) - dV_ref).max() < 1e-4 * big(dV_ref)
    # ---- aggregation backward, centre gradient
    d_dV = _d(dV_ref)
    da_o = torch.empty((R, G * K), device=DEV); dxe_o = torch.full((R, E), 7.0, device=DEV)       # (dxe is written, not accumulated)
    _twice(lambda: ops.nextvlad_aggregate_bwd(d_a, d_xe, B, S, G, K, D, d_c2, d_dV, da_o, dxe_o), da_o, dxe_o)
    da_ref = np.einsum("bkd,bsgd->bsgk", dV_ref, x4) - np.einsum("bkd,kd->bk", dV_ref, c2)[:, None, None, :]
    dxe_ref = np.einsum("bsgk,bkd->bsgd", a4, dV_ref)
    assert np.abs(_np(da_o).reshape(B, S, G, K) - da_ref).max() < 1e-3 * big(da_ref)
    assert np.abs(_np(dxe_o).reshape(B, S, G, D) - dxe_ref).max() < 1e-4 * big(dxe_ref)
    dc2 = torch.empty((K, D), device=DEV)
    d_asum = _d(asum_ref)
    _twice(lambda: ops.netvlad_dcenters(d_asum, d_dV, B, K, D, dc2), dc2)
    dc2_ref = -np.einsum("bk,bkd->kd", asum_ref, dV_ref)
    assert np.abs(_np(dc2) - dc2_ref).max() < 1e-4 * big(dc2_ref)
    # ---- context gate, column sum
    H = 37
    h = rng.standard_normal((B, H)); gl = 2 * rng.standard_normal((B, H)); dout = rng.standard_normal((B, H))
    d_h, d_gl, d_dout = _d(h), _d(gl), _d(dout)
    out = torch.empty((B, H), device=DEV); dh = torch.empty((B, H), device=DEV); dgl = torch.empty((B, H), device=DEV)
    dgl_bf = torch.empty((B, H), dtype=torch.bfloat16, device=DEV)
    _twice(lambda: ops.nextvlad_gate_fwd(d_h, d_gl, out), out)
    _twice(lambda: ops.nextvlad_gate_bwd(d_h, d_gl, d_dout, dh, dgl, dgl_bf), dh, dgl, dgl_bf)
    gate = _sig(gl)
    for got, ref in ((out, h * gate), (dh, dout * gate), (dgl, dout * h * gate * (1 - gate))):
        assert np.abs(_np(got) - ref).max() < 1e-5 * big(ref)
    assert torch.equal(dgl_bf, dgl.bfloat16())
    cs = torch.empty(E, device=DEV)
    _twice(lambda: ops.nextvlad_colsum(d_xe, R, E, cs), cs)
    assert np.abs(_np(cs) - xe.sum(0)).max() < 1e-4 * big(xe.sum(0))
    tall = rng.standard_normal((600 + S, 70))                         # >= 512 rows: 32 partial rows, then their sum in order
    d_tall = _d(tall); cs2 = torch.empty(70, device=DEV)
    _twice(lambda: ops.nextvlad_colsum(d_tall, tall.shape[0], 70, cs2), cs2)
    assert np.abs(_np(cs2) - tall.sum(0)).max() < 1e-4 * big(tall.sum(0))
    # ---- the centred bf16 operand of the logit products, the constant it leaves to the products' bias, the rank-one gradient term
    bias = rng.standard_normal(E); d_bias = _d(bias)
    xc = torch.empty((R, E), dtype=torch.bfloat16, device=DEV)
    _twice(lambda: ops.nextvlad_center_cast(d_xe, R, E, d_bias, xc), xc)
    assert torch.equal(xc, (d_xe - d_bias[None, :]).bfloat16())       # one f32 subtraction, rounded to nearest even
    W = rng.standard_normal((G, E)); add = rng.standard_normal(G); d_W = _d(W); d_add = _d(add)
    bl = torch.full((G + 5,), 9.0, device=DEV)
    _twice(lambda: ops.nextvlad_bias_logits(d_bias, d_W, G, E, bl, add=d_add), bl)
    bl_ref = W @ bias + add
    assert np.abs(_np(bl[:G]) - bl_ref).max() < 1e-4 * big(bl_ref) and not bl[G:].any()
    dWc = rng.standard_normal((G + 2, E)); du = rng.standard_normal(G); dW = torch.empty((G, E), device=DEV)
    d_dWc, d_du = _d(dWc), _d(du)
    _twice(lambda: ops.nextvlad_wgrad_uncenter(d_dWc, d_du, d_bias, G, E, dW), dW)
    dW_ref = dWc[:G] + du[:, None] * bias[None, :]
    assert np.abs(_np(dW) - dW_ref).max() < 1e-5 * big(dW_ref)        # one fma per element


def test_nextvlad_refusals():
    """Shapes the tiles cannot take are refused with EVC_ERR_BAD_SHAPE before anything is launched (the outputs keep their
    fill), and the tower constructor names the offending size."""
    from efficientvideoclassification_youtube8m_amd import _lib, ops
    from efficientvideoclassification_youtube8m_amd.towers import NeXtVladTower
    for S, G, D in ((65, 1, 8), (41, 25, 8), (4, 2, 6)):             # S > 64, S*G = 1025, D % 4 != 0
        B, K = 2, 8
        R = B * S
        a = torch.zeros((R, G * K), device=DEV); xe = torch.zeros((R, G * D), device=DEV); c2 = torch.zeros((K, D), device=DEV)
        V = torch.full((B, K, D), 3.0, device=DEV); asum = torch.full((B, K), 3.0, device=DEV)
        da = torch.full((R, G * K), 3.0, device=DEV); dxe = torch.full((R, G * D), 3.0, device=DEV)
        with pytest.raises(_lib.EvcError, match=r"evc_nextvlad_aggregate_fwd failed \(-1\)"):
            ops.nextvlad_aggregate_fwd(a, xe, B, S, G, K, D, c2, V, asum)
        with pytest.raises(_lib.EvcError, match=r"evc_nextvlad_aggregate_bwd failed \(-1\)"):
            ops.nextvlad_aggregate_bwd(a, xe, B, S, G, K, D, c2, V.clone(), da, dxe)
        torch.cuda.synchronize()
        for t in (V, asum, da, dxe):
            assert bool((t == 3.0).all())
    with pytest.raises(_lib.EvcError, match=r"evc_nextvlad_assign_fwd failed \(-1\)"):
        z = torch.zeros((4, 1025), device=DEV)
        ops.nextvlad_assign_fwd(z, 4, 1, 1025, z[0], z[0], z[0], z[0], z, z.clone())
    kw = dict(max_frames=300, feature_size=64, vocab_size=10, iterations=8, cluster_size=16, hidden_size=128, device=DEV)
    with pytest.raises(ValueError, match="groups=3"):
        NeXtVladTower(8, groups=3, expansion=2, gating_reduction=2, **kw)            # E = 128 is not a multiple of 3
    with pytest.raises(ValueError, match="= 32 must be a multiple of 64"):
        NeXtVladTower(8, groups=4, expansion=2, gating_reduction=4, **kw)            # H / rho = 32
    with pytest.raises(ValueError, match="iterations=65"):
        NeXtVladTower(8, groups=4, expansion=2, gating_reduction=2, **dict(kw, iterations=65))
    with pytest.raises(ValueError, match="= 72 must be a multiple of 32"):
        NeXtVladTower(9, groups=4, expansion=2, gating_reduction=2, **kw)            # R = 72 in training


def _params(tw):
    pre = tw.scope + "/"
    return {k[len(pre):]: _np(v) for k, v in tw.state_dict().items()}


@pytest.mark.parametrize("B,F,lam,G,K,H,rho,V,S,u8", [(16, 64, 2, 4, 16, 128, 2, 40, 10, False), (32, 192, 2, 8, 24, 128, 2, 33, 30, True)])
def test_nextvlad_forward_backward_against_reference(B, F, lam, G, K, H, rho, V, S, u8):
    """The tower against tests/_nextvlad_ref.py.  Bounds are the NetVLAD test's, for the same reason: bf16 operands through
    the GEMMs in front of each compared quantity, and relu6 masks that may flip within bf16 rounding of 0 / 6.

    Measured on an MI355X (first / second shape): a 1.4e-3 / 1.7e-3, Y (the bf16 operand Y_bf) 1.63e-2 / 1.07e-2, pred 2.2e-3 / 2.2e-3, largest
    relative L2 of a gradient 0.114 (attention_biases) / 0.034.  Y is the tight one: vlad_bn normalises over B
    videos whose descriptors differ little on synthetic frames - the batch variance of U (median 1.4e-4) lies below epsilon =
    1e-3 - so Y is U's deviation times gamma / sqrt(var + eps), up to 49 with the perturbed gamma.  With the logit products'
    operand rounded as bf16(xe), bias included, Y was 1.85e-2 / 2.02e-2 and the second shape missed the bound; the tower
    contracts bf16(xe - be) and adds be.W as the products' f32 bias for that reason."""
    from efficientvideoclassification_youtube8m_amd import ops
    from efficientvideoclassification_youtube8m_amd.towers import NeXtVladTower
    rng = np.random.default_rng(B + K)
    q, x, n, labels = mm.synthetic_batch(B, seed=B, feature_size=F, vocab_size=V, dtype=np.float32)
    mk = lambda seed: NeXtVladTower(B, 300, F, V, iterations=S, cluster_size=K, hidden_size=H, groups=G, expansion=lam,
                                    gating_reduction=rho, device=DEV, seed=seed)
    tw = mk(3)
    E, D, Hg = lam * F, lam * F // G, H // rho
    for k in tw.names:                                   # non-trivial batch-norm scale / offset and biases
        if k.endswith("/gamma") or k.endswith("/beta") or k in (tw.EB, tw.AB):
            tw.store.p(k).add_(torch.from_numpy(rng.standard_normal(tw.store.p(k).shape).astype(np.float32) * 0.2).to(DEV))
    P = _params(tw)
    tf_shapes = {"expansion_weights": (F, E), "expansion_biases": (E,), "attention_weights": (E, G), "attention_biases": (G,),
                 "cluster_weights": (E, G * K), "cluster_weights2": (D, K), "hidden1_weights": (K * D, H),
                 "gating_weights_1": (H, Hg), "gating_weights_2": (Hg, H)}
    for s, c in zip(nx.BN_NAMES, (G * K, K * D, H, Hg)):
        for v in ("beta", "gamma", "moving_mean", "moving_variance"):
            tf_shapes["%s/%s" % (s, v)] = (c,)
    for k, shp in tf_shapes.items():
        assert P[k].shape == shp, (k, P[k].shape, shp)
    # TF order: row d*K + k of hidden1_weights (entry d*K + k of vlad_bn/*) is the internal cluster-major column k*D + d
    hw = _np(tw.store.p(tw.HW))                                                    # [H][k*D + d]
    assert np.array_equal(P["hidden1_weights"].reshape(D, K, H), hw.T.reshape(K, D, H).transpose(1, 0, 2))
    assert np.array_equal(P["vlad_bn/gamma"].reshape(D, K), _np(tw.store.p("vlad_bn/gamma")).reshape(K, D).T)
    u = rng.random((B, S)).astype(np.float32)
    xin = torch.from_numpy(q).to(DEV) if u8 else torch.from_numpy(x).to(DEV)
    pred = tw.forward(xin, torch.from_numpy(n).to(DEV), torch.from_numpy(u).to(DEV))
    xn = mm.l2_normalize(x.astype(np.float64), 2)
    ref_pred, cache = nx.nextvlad_fwd(xn, n, u, P)
    assert np.array_equal(tw.idx.cpu().numpy(), mm.sample_random_frames_index(u, n))
    err_a = np.abs(_np(tw.a).reshape(B * S, G, K) - cache["a"]).max()
    Yk = cache["Y"].reshape(B, D, K).transpose(0, 2, 1).reshape(B, K * D)          # reference order d*K+k -> cluster-major
    # The tower's Y is Y_bf, the hidden GEMM's bf16 operand: the bound is asserted on it, as the NetVLAD test does.  Y in f32
    # from the tower's own U and vlad_bn statistics, by the kernel the tower calls, is printed next to it, and Y_bf must be
    # exactly its rounding.
    bv = tw.bn_v
    Yf = torch.empty((B, K * D), device=DEV)
    ops.bn_apply(tw.U, B, K * D, bv.mean, bv.var, bv.gamma(), bv.beta(), False, y_f32=Yf)
    assert torch.equal(tw.Y_bf[:B], Yf.bfloat16()) and not tw.Y_bf[B:].any()
    err_y_f32 = np.abs(_np(Yf) - Yk).max()
    err_y = np.abs(tw.Y_bf[:B].float().cpu().numpy() - Yk).max()
    err = np.abs(_np(pred) - ref_pred).max()
    print("nextvlad a err %.2e  Y err %.2e (before the rounding to bf16 %.2e, |Y|max %.2f)  pred err %.2e" % (err_a, err_y, err_y_f32, np.abs(Yk).max(), err))
    # every bound is evaluated (and every figure printed) before the first one fails the test
    missed = [(w, e, b) for w, e, b in (("a", err_a, 2e-2), ("Y", err_y, 2e-2), ("pred", err, 5e-3)) if not e < b]
    dp =mm.cross_entropy_grad(ref_pred, labels)
    tw.backward(torch.from_numpy(dp.astype(np.float32)).to(DEV))
    gref = nx.nextvlad_bwd(dp, cache)
    assert set(gref) == set(tw.names)
    for k, g in gref.items():
        got = tw.store.g(k)
        got = _np(got.t() if got.dim() == 2 else got)
        if k == tw.HW:
            got = got.reshape(K, D, H).transpose(1, 0, 2).reshape(D * K, H)
        elif k.startswith("vlad_bn/"):
            got = got.reshape(K, D).T.reshape(-1)
        l2 = float(np.linalg.norm(got - g) / (np.linalg.norm(g) + 1e-30))
        mx = float(np.abs(got - g).max())
        print("  grad %-28s rel l2 %.3e  max abs %.3e" % (k, l2, mx))
        # (relu6 masks can flip on values within bf16 rounding of 0 / 6: judge each tensor by its relative L2 error)
        if not (l2 < 0.12 or mx < 1e-3):
            missed.append(("grad " + k, (l2, mx), (0.12, 1e-3)))
    # state_dict round trip into a tower with other initial weights
    tw2 = mk(9)
    assert not torch.equal(tw2.store.master, tw.store.master)
    tw2.load_state_dict(tw.state_dict())
    assert torch.equal(tw2.store.master, tw.store.master)
    assert not missed, missed


def test_nextvlad_through_create_model_and_train_main(tmp_path):
    from efficientvideoclassification_youtube8m_amd import frame_level_models, train
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    FLAGS.reset()
    FLAGS.parse(["--nextvlad_cluster_size", "16", "--nextvlad_groups", "4", "--nextvlad_hidden_size", "128",
                 "--nextvlad_gating_reduction", "2", "--iterations", "8"])
    B, F, V = 8, 64, 20
    q, x, n, labels = mm.synthetic_batch(B, seed=4, feature_size=F, vocab_size=V, dtype=np.float32)
    m = frame_level_models.NeXtVLADModel()
    out = m.create_model(torch.from_numpy(x).to(DEV), V, torch.from_numpy(n).to(DEV), normalize_input=True)
    assert set(out) == {"predictions"} and tuple(out["predictions"].shape) == (B, V)
    assert 0.0 <= float(out["predictions"].min()) and float(out["predictions"].max()) <= 1.0
    assert m.create_model(None, V, None) is None and m.create_model_inference(None, V, 10, None) is None     # the reference's stubs
    FLAGS.reset()
    common = ["--train_data_pattern", "synthetic", "--frame_features", "True", "--feature_names", "rgb, audio", "--model", "NeXtVLADModel",
              "--batch_size", "16", "--iterations", "10", "--nextvlad_cluster_size", "16", "--nextvlad_groups", "4",
              "--nextvlad_hidden_size", "128", "--nextvlad_gating_reduction", "2", "--feature_sizes", "64, 64", "--synthetic_videos", "64",
              "--num_epochs", "1", "--start_new_model", "True", "--base_learning_rate", "0.01"]
    res = train.main(common + ["--train_dir", str(tmp_path) + "/"])
    FLAGS.reset()
    assert res["iterations"] == 4 and res["graph"].global_step == 4
    losses = [h[1]["loss"] for h in res["history"]]
    print("nextvlad train losses", losses)
    assert all(np.isfinite(l) for l in losses) and losses[-1] < losses[0]            # it trains
    sd = torch.load(train.latest_checkpoint(str(tmp_path) + "/"))
    assert sd["model/hidden1_weights"].shape == (64 * 16, 128) and sd["model/cluster_weights2"].shape == (64, 16)     # D = 256 / 4
    with pytest.raises(ValueError, match="NeXtVladTower has no such forward mode"):
        train.main(common + ["--train_dir", str(tmp_path) + "/p/", "--precision", "high"])
    FLAGS.reset()
