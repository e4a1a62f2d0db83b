"""NeXtVLAD (extension) on the CPU: the float64 restatement tests/_nextvlad_ref.py checked against itself
(hand-written reverse mode vs central finite differences), and the host interface that needs no device."""
import numpy as np
import pytest
import torch

import _nextvlad_ref as nx
from oracle import model_math as mm


def test_nextvlad_ref_backward_matches_finite_differences():
    """Every parameter tensor, several random entries each, in training-mode batch-norm; the bound is the one
    tests/test_oracle_model.py uses for NetVLAD.  The seed is chosen so that no relu6 input lies within the step of 0 or 6
    (asserted: a kink inside the difference stencil would make the comparison meaningless)."""
    rng = np.random.default_rng(5)
    F, lam, G, K, H, rho, S, B, V, T = 8, 2, 4, 3, 8, 2, 5, 4, 6, 12
    P = nx.init_params(rng, F, lam, G, K, H, rho, V)
    for k in P:
        if k.endswith("gamma") or k.endswith("beta"):
            P[k] = P[k] + 0.2 * rng.standard_normal(P[k].shape)
    x = rng.standard_normal((B, T, F))
    n = rng.integers(1, T + 1, B)
    u = rng.random((B, S)).astype(np.float32)
    y = rng.random((B, V)) > 0.6

    def loss(Q):
        p, _ = nx.nextvlad_fwd(x, n, u, Q)
        return mm.cross_entropy_loss(p, y)

    pred, cache = nx.nextvlad_fwd(x, n, u, P)
    eps = 1e-6
    g1 = cache["g1bn"]
    margin = min(np.abs(g1).min(), np.abs(g1 - 6).min())
    assert margin > 1e-3, margin                   # far more than any relu6 input moves under a 1e-6 parameter step
    grads = nx.nextvlad_bwd(mm.cross_entropy_grad(pred, y), cache)
    assert set(grads) == set(P)
    for k in P:
        flat = P[k].reshape(-1)
        for j in rng.choice(flat.size, size=min(6, flat.size), replace=False):
            old = flat[j]
            flat[j] = old + eps
            lp = loss(P)
            flat[j] = old - eps
            lm = loss(P)
            flat[j] = old
            fd = (lp - lm) / (2 * eps)
            got = grads[k].reshape(-1)[j]
            assert abs(fd - got) <= 1e-5 * max(1.0, abs(fd)) + 1e-7, (k, j, fd, got)


def test_nextvlad_flags_exist_with_their_defaults():
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    FLAGS.reset()
    assert (FLAGS.nextvlad_expansion, FLAGS.nextvlad_groups, FLAGS.nextvlad_cluster_size, FLAGS.nextvlad_hidden_size,
            FLAGS.nextvlad_gating_reduction) == (2, 8, 64, 1024, 8)
    FLAGS.parse(["--nextvlad_groups", "4", "--nextvlad_cluster_size", "16"])
    assert FLAGS.nextvlad_groups == 4 and FLAGS.nextvlad_cluster_size == 16
    FLAGS.reset()


def test_nextvlad_create_model_stub_call_and_no_cpu_path():
    from efficientvideoclassification_youtube8m_amd import _lib, frame_level_models
    from efficientvideoclassification_youtube8m_amd.flags import FLAGS
    FLAGS.reset()
    m = frame_level_models.NeXtVLADModel()
    assert m.create_model(None, 1, None) is None                       # the reference's stub call
    assert m.create_model_inference(None, 1, 10, None) is None
    if not torch.cuda.is_available():
        with pytest.raises(_lib.EvcError):                             # the library's error, not an eager fallback
            m.create_model(torch.zeros((2, 12, 64)), 6, torch.full((2,), 12), iterations=4, cluster_size=16, hidden_size=128,
                           groups=4, gating_reduction=2)
        assert m.towers == {}
