"""Kernel-level parity: each HIP entry point (through the C ABI) against the
numpy oracle on seeded inputs.  Run on the MI355X box: pytest -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import model_math as mm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from efficientvideoclassification_youtube8m_amd import ops as _ops
    _ops.check_device(0)
    return _ops


def _raises(fn, *a):
    try:
        fn(*a)
        return False
    except ValueError:
        return True


def bf16_round(a):
    return torch.from_numpy(np.asarray(a, np.float32)).bfloat16().double().numpy()


def to_bf16(a):
    return torch.from_numpy(np.asarray(a, np.float32)).bfloat16().to(DEV)


@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (200, 300, 128), (512, 4096, 1024), (64, 64, 2176),
                                   (1, 5, 64), (1000, 130, 192), (4716, 64, 256),
                                   (512, 300, 16384),    # long K, few tiles -> split-K with f32 atomics on 128x128 tiles ...
                                   (600, 264, 8192)])    # ... and, above 512 rows, on 256x256 tiles
def test_gemm_nt(ops, M, N, K):
    rng = np.random.default_rng(M * 7 + N)
    A = bf16_round(rng.standard_normal((M, K)))
    B = bf16_round(rng.standard_normal((N, K)) * 0.1)
    bias = rng.standard_normal(N).astype(np.float32)
    ref = A @ B.T + bias
    out = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
    ops.gemm_nt(to_bf16(A), to_bf16(B), M, N, K, out, bias=torch.from_numpy(bias).to(DEV))
    got = out.cpu().double().numpy()
    scale = np.abs(A) @ np.abs(B.T) + 1.0
    assert np.max(np.abs(got - ref) / scale) < 3e-6          # f32 accumulation of exact bf16 products
    # accumulate + bf16 output paths
    ops.gemm_nt(to_bf16(A), to_bf16(B), M, N, K, out, accumulate=True)
    assert np.max(np.abs(out.cpu().double().numpy() - (2 * ref - bias)) / scale) < 4e-6
    outb = torch.empty((M, N), dtype=torch.bfloat16, device=DEV)
    ops.gemm_nt(to_bf16(A), to_bf16(B), M, N, K, outb)
    assert np.max(np.abs(outb.float().cpu().double().numpy() - (ref - bias)) / scale) < 8e-3


@pytest.mark.parametrize("M,T,Kin,H,hoist", [(256, 5, 64, 64, False), (256, 5, 64, 64, True), (200, 4, 128, 128, False),
                                             (1536, 3, 192, 256, False), (1536, 3, 192, 256, True), (70, 6, 64, 128, True),
                                             (640, 3, 64, 128, False)])
def test_lstm_layer_fwd_and_bwd(ops, M, T, Kin, H, hoist):
    """One BasicLSTMCell layer over T steps with ragged lengths (incl. 0 and T):
    final state, per-step h, and the BPTT dz / dx / dW against
    the oracle run on the same bf16-rounded operands."""
    rng = np.random.default_rng(M + T + Kin + H)
    x = bf16_round(rng.standard_normal((M, T, Kin)) * 0.5)
    kernel = bf16_round(mm.glorot_uniform(rng, (Kin + H, 4 * H)) * 2.0)
    bias = (rng.standard_normal(4 * H) * 0.1).astype(np.float32).astype(np.float64)
    lens = rng.integers(0, T + 1, size=M).astype(np.int32)
    lens[:3] = [0, T, 1]
    s_ref, cache = mm.multi_rnn_seq_fwd(x, lens, [(kernel, bias)])

    xt = to_bf16(np.ascontiguousarray(x.transpose(1, 0, 2)))         # [T][M][Kin]
    wT = to_bf16(np.ascontiguousarray(kernel.T))                       # [4H][Kin+H]
    # backward shadow: TF layout with the 4H axis gate-interleaved (column u*4+g <- g*H+u)
    w_il = to_bf16(np.ascontiguousarray(kernel.reshape(Kin + H, 4, H).transpose(0, 2, 1).reshape(Kin + H, 4 * H)))
    b = torch.from_numpy(bias.astype(np.float32)).to(DEV)
    ln = torch.from_numpy(lens).to(DEV)
    hbuf = torch.full((T + 1, M, H), float("nan"), dtype=torch.bfloat16, device=DEV)
    S = torch.full((M, 2 * H), float("nan"), dtype=torch.float32, device=DEV)
    gates = torch.empty((T, M, H, 2), dtype=torch.int32, device=DEV)
    c_all = torch.full((T + 1, M, H), float("nan"), dtype=torch.bfloat16, device=DEV)
    KP = ops.round_up(T * M, 64)
    zx = torch.empty((T * M, 4 * H), dtype=torch.float32, device=DEV) if hoist else None
    ops.lstm_layer_fwd(xt, wT, b, ln, T, M, Kin, H, hbuf, S[:, :H], S[:, H:], 2 * H, gates, c_all, hoist=hoist, zx_ws=zx)
    got = S.cpu().double().numpy()
    assert np.isfinite(got).all()
    # h is re-quantised to bf16 between steps (the kernel's operand precision): 2^-9 relative per step
    assert np.max(np.abs(got - s_ref)) < 6e-3, np.max(np.abs(got - s_ref))
    assert np.all(got[0] == 0)                                          # len 0 -> zero state
    hb = hbuf.float().cpu().numpy()
    assert np.all(hb[0] == 0)
    for t in range(T):
        assert np.all(hb[t + 1][lens <= t] == 0)                        # zero output past the length

    # ---- backward ----
    dS = rng.standard_normal((M, 2 * H))
    dh_above = bf16_round(rng.standard_normal((T, M, H)) * 0.3)      # the upper layer's dX arrives as bf16
    dx_ref, grads_ref = _bwd_ref(x, lens, kernel, bias, dS, dh_above)
    dSt = torch.from_numpy(dS.astype(np.float32)).to(DEV)
    dha = to_bf16(dh_above)
    dz4 = torch.full((T, M, 4 * H), float("nan"), dtype=torch.bfloat16, device=DEV)
    dcw = torch.empty((M, H), dtype=torch.float32, device=DEV)
    dbk = torch.zeros(4 * H, dtype=torch.float32, device=DEV)           # bias gradient accumulated by the step kernels
    ops.lstm_layer_bwd(w_il, ln, T, M, Kin, H, gates, c_all, dSt[:, :H], dSt[:, H:], 2 * H, dha, dcw, dz4, db=dbk)
    dzf = dz4.float().cpu().double().numpy()
    assert np.isfinite(dzf).all()
    for t in range(T):
        assert np.all(dzf[t][lens <= t] == 0)
    dz_tf = dz4.view(T, M, H, 4).permute(0, 1, 3, 2).reshape(T * M, 4 * H).contiguous()   # TF gate order
    dzT = torch.empty((4 * H, KP), dtype=torch.bfloat16, device=DEV)     # de-interleaving transpose
    ops.transpose_to_bf16(dz4.reshape(T * M, 4 * H), T * M, 4 * H, dzT, KP, interleave_H=-H)
    assert torch.equal(dzT[:, :T * M], dz_tf.t()) and bool((dzT[:, T * M:] == 0).all())
    # dx = dz . Wx^T through the generic GEMM with the interleaved K order
    dxo = torch.empty((T * M, Kin), dtype=torch.float32, device=DEV)
    ops.gemm_nt(dz4.reshape(T * M, 4 * H), w_il, T * M, Kin, 4 * H, dxo)
    dx_got = dxo.cpu().double().numpy().reshape(T, M, Kin).transpose(1, 0, 2)
    sc = np.abs(dx_ref).max() + 1e-6
    assert np.max(np.abs(dx_got - dx_ref)) / sc < 2e-2
    # dW^T = dz^T . [x | h_prev]
    hT = torch.empty((H, KP), dtype=torch.bfloat16, device=DEV)
    ops.transpose_to_bf16(hbuf[:T].reshape(T * M, H), T * M, H, hT, KP)
    xT = torch.empty((Kin, KP), dtype=torch.bfloat16, device=DEV)
    ops.transpose_to_bf16(xt.reshape(T * M, Kin), T * M, Kin, xT, KP)
    dWT = torch.empty((4 * H, Kin + H), dtype=torch.float32, device=DEV)
    ops.gemm_nt(dzT, xT, 4 * H, Kin, KP, dWT)
    ops.gemm_nt(dzT, hT, 4 * H, H, KP, dWT[:, Kin:], ldc=Kin + H)
    dW_got = dWT.cpu().double().numpy().T
    dW_ref = grads_ref[0][0]
    sc = np.abs(dW_ref).max() + 1e-6
    assert np.max(np.abs(dW_got - dW_ref)) / sc < 2e-2
    db = torch.empty(4 * H, dtype=torch.float32, device=DEV)
    ops.rowsum_bf16(dzT, 4 * H, KP, db)
    sc = np.abs(grads_ref[0][1]).max() + 1e-6
    assert np.max(np.abs(db.cpu().double().numpy() - grads_ref[0][1])) / sc < 2e-2
    assert np.max(np.abs(dbk.cpu().double().numpy() - grads_ref[0][1])) / sc < 2e-2      # in-kernel sum (f32, unrounded dz)
    assert (dbk - db).abs().max().item() / sc < 5e-3
    # the shadow-weight builder produces exactly this interleaved layout
    sb = torch.empty((Kin + H, 4 * H), dtype=torch.bfloat16, device=DEV)
    ops.transpose_to_bf16(wT, 4 * H, Kin + H, sb, 4 * H, interleave_H=H)
    assert torch.equal(sb, w_il)


@pytest.mark.parametrize("M,T,Kin,H", [(256, 5, 64, 64), (200, 4, 128, 128), (1536, 3, 192, 256), (640, 3, 64, 128), (70, 6, 64, 128)])
def test_lstm_layer_fwd_f16(ops, M, T, Kin, H):
    """evc_lstm_layer_fwd_f16: the fused step on IEEE f16 operands (one f16 MFMA product per depth) against the oracle on the same
    f16-rounded x and kernel.  h is re-quantised to f16 between steps - 2^-12 relative, 8x finer than the bf16 step, whose bound
    in test_lstm_layer_fwd_and_bwd is 6e-3 - so the states must sit within 8e-4; the bf16 copy of h (the operand of the
    backward products) is the bf16 rounding of the same values.  Of the tape only c_all is looked at here, and only for being finite on
    live rows; every element of gates, c_all, both h images and the state is compared in tests/test_gpu_lstm_fwd_parity.py."""
    rng = np.random.default_rng(M + T + Kin + H + 1)
    f16r = lambda a: torch.from_numpy(np.asarray(a, np.float32)).half().double().numpy()
    x = f16r(rng.standard_normal((M, T, Kin)) * 0.5)
    kernel = f16r(mm.glorot_uniform(rng, (Kin + H, 4 * H)) * 2.0)
    bias = (rng.standard_normal(4 * H) * 0.1).astype(np.float32).astype(np.float64)
    lens = rng.integers(0, T + 1, size=M).astype(np.int32)
    lens[:3] = [0, T, 1]
    s_ref, cache = mm.multi_rnn_seq_fwd(x, lens, [(kernel, bias)])
    x16 = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2)).astype(np.float32)).half().to(DEV)
    w16 = torch.from_numpy(np.ascontiguousarray(kernel.T).astype(np.float32)).half().to(DEV)
    b = torch.from_numpy(bias.astype(np.float32)).to(DEV)
    ln = torch.from_numpy(lens).to(DEV)
    h16 = torch.full((T + 1, M, H), float("nan"), dtype=torch.float16, device=DEV)
    hbf = torch.full((T + 1, M, H), float("nan"), dtype=torch.bfloat16, device=DEV)
    S = torch.full((M, 2 * H), float("nan"), dtype=torch.float32, device=DEV)
    gates = torch.empty((T, M, H, 2), dtype=torch.int32, device=DEV)
    c_all = torch.full((T + 1, M, H), float("nan"), dtype=torch.bfloat16, device=DEV)
    ops.lstm_layer_fwd_f16(x16, w16, b, ln, T, M, Kin, H, h16, hbf, S[:, :H], S[:, H:], 2 * H, gates, c_all)
    got = S.cpu().double().numpy()
    assert np.isfinite(got).all()
    err = np.max(np.abs(got - s_ref))
    assert err < 8e-4, err
    assert np.all(got[0] == 0)
    h16n, hbfn = h16.float().cpu().numpy(), hbf.float().cpu().numpy()
    assert np.all(h16n[0] == 0) and np.all(hbfn[0] == 0)
    for t in range(T):
        dead = lens <= t
        assert np.all(h16n[t + 1][dead] == 0) and np.all(hbfn[t + 1][dead] == 0)
        # both images are roundings of the same f32 h_t
        assert np.max(np.abs(h16n[t + 1] - hbfn[t + 1])) <= 2.0 ** -8
    # the cell history is finite wherever a row is live (its values: test_gpu_lstm_fwd_parity.py)
    c_hist = c_all.float().cpu().numpy()
    for t in range(T):
        live = lens > t
        if live.any():
            assert np.isfinite(c_hist[t + 1][live]).all()


def test_cast_f16_and_l2norm_f16_images(ops):
    """evc_cast_f32_to_f16 rounds to nearest even like torch's .half(); evc_l2norm_chunk_fwd with aux_f16 = 1 writes, next to the
    bf16 images, IEEE f16 images of the SAME normalised values (teacher and student views, uint8 and f32 inputs)."""
    g = torch.Generator(device="cpu")
    g.manual_seed(5)
    w = (torch.rand((130, 72), generator=g) * 2 - 1) * torch.logspace(-9, 1, 72)[None, :]
    out = torch.empty((130, 72), dtype=torch.float16, device=DEV)
    ops.cast_f16(w.to(DEV), out)
    assert torch.equal(out.cpu(), w.half())
    B, T, F, C1, C2, every_n = 3, 60, 64, 4, 2, 10
    q, x, n, _ = mm.synthetic_batch(B, seed=3, max_frames=T, feature_size=F, vocab_size=8, dtype=np.float32)
    for inp, nf in ((torch.from_numpy(x).to(DEV), None), (torch.from_numpy(q).to(DEV), torch.from_numpy(n).to(DEV))):
        (t_bf, t_16), (s_bf, s_16) = ops.l2norm_chunk(inp, C1, every_n, C2, num_frames=nf, split="f16")
        (t_bf2, t_lo), _ = ops.l2norm_chunk(inp, C1, every_n, C2, num_frames=nf, split=True)
        assert t_16.dtype == torch.float16 and s_16.dtype == torch.float16 and torch.equal(t_bf, t_bf2)
        ref = mm.l2_normalize(x.astype(np.float64))
        view = ref.reshape(B, C1, T // C1, F).transpose(2, 1, 0, 3).reshape(T // C1, C1 * B, F)
        assert np.max(np.abs(t_16.float().cpu().numpy() - view)) < 2.0 ** -11 * np.abs(view).max() * 1.01 + 1e-7
        # hi + lo (bf16 halves) and the f16 image describe the same f32 values
        assert float((t_bf.float() + t_lo.float() - t_16.float()).abs().max()) < 2.0 ** -11
        # K-extension segments: [f16(x) | (x - f16(x))*64 | f16(x)/64] - the first two sum (descaled) to x within f16's subnormal step
        (_, t_w), (_, s_w) = ops.l2norm_chunk(inp, C1, every_n, C2, num_frames=nf, split="f16", f16_segments=3)
        assert t_w.shape == t_16.shape[:2] + (3 * F,) and s_w.shape == s_16.shape[:2] + (3 * F,)
        assert torch.equal(t_w[:, :, :F], t_16) and torch.equal(s_w[:, :, :F], s_16)
        assert float((t_w[:, :, 2 * F:].float() * 64.0 - t_16.float()).abs().max()) <= 64 * 2.0 ** -25   # (f16(x)/64 may be subnormal: step 2^-24)
        rec = t_w[:, :, :F].double().cpu().numpy() + t_w[:, :, F:2 * F].double().cpu().numpy() / 64.0
        assert np.max(np.abs(rec - view)) < 3e-7          # ~2^-22: f32 normalisation arithmetic of the kernel, not the f16 images
        (_, t_w2), _ = ops.l2norm_chunk(inp, C1, every_n, C2, num_frames=nf, split="f16", f16_segments=2)
        assert torch.equal(t_w2, t_w[:, :, :2 * F])
        sub = ref[:, ::every_n][:, :T // every_n]
        S2 = T // every_n
        sview = sub.reshape(B, C2, S2 // C2, F).transpose(2, 1, 0, 3).reshape(S2 // C2, C2 * B, F)
        assert np.max(np.abs(s_16.float().cpu().numpy() - sview)) < 2.0 ** -11 * np.abs(sview).max() * 1.01 + 1e-7



@pytest.mark.parametrize("M,N,K", [(4, 300, 128), (256, 4716 * 3, 1024), (700, 512, 256), (5120, 1024, 512), (1280, 384, 192)])
def test_gemm_nt_split_wide(ops, M, N, K):
    """evc_gemm_nt_split: (A_hi + A_lo) . (B_hi + B_lo)^T as one K-extended launch of the plain bf16 loop (segment 1: [lo | hi]
    rows against [hi | lo] rows, segment 2: hi against hi through GemmOperands::B2) from the wide images of
    evc_cast_f32_to_bf16_wide - against the float64 product of the f32 operands: ~2^-16 relative to |A|.|B|, where one bf16
    product sits at 2^-8."""
    rng = np.random.default_rng(M + N + K)
    A = (rng.standard_normal((M, K)) * 3.0).astype(np.float32)
    B = (rng.standard_normal((N, K)) * 0.1).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    Aw = torch.empty((M, 2 * K), dtype=torch.bfloat16, device=DEV)
    Bw = torch.empty((N, 2 * K), dtype=torch.bfloat16, device=DEV)
    ops.cast_bf16_wide(torch.from_numpy(A).to(DEV), Aw, lo_first=True)
    ops.cast_bf16_wide(torch.from_numpy(B).to(DEV), Bw, lo_first=False)
    At = torch.from_numpy(A)
    hi = At.bfloat16()
    assert torch.equal(Aw[:, K:].cpu(), hi) and torch.equal(Aw[:, :K].cpu(), (At - hi.float()).bfloat16())
    Bt = torch.from_numpy(B)
    assert torch.equal(Bw[:, :K].cpu(), Bt.bfloat16()) and torch.equal(Bw[:, K:].cpu(), (Bt - Bt.bfloat16().float()).bfloat16())
    out = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
    ops.gemm_nt_split_wide(Aw, Bw, M, N, K, out, bias=torch.from_numpy(bias).to(DEV))
    ref = A.astype(np.float64) @ B.astype(np.float64).T + bias
    scale = np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64).T + 1.0
    err = np.max(np.abs(out.cpu().double().numpy() - ref) / scale)
    assert err < 4e-5, err
    # one bf16 product of the same operands for scale
    o1 = torch.empty((M, N), dtype=torch.float32, device=DEV)
    ops.gemm_nt(Aw[:, K:], Bw[:, :K], M, N, K, o1, bias=torch.from_numpy(bias).to(DEV), lda=2 * K, ldb=2 * K)
    assert np.max(np.abs(o1.cpu().double().numpy() - ref) / scale) > 5 * err


@pytest.mark.parametrize("M,T,Kin,H", [(256, 5, 256, 64), (40, 6, 128, 128), (96, 4, 64, 192), (1100, 3, 128, 128)])
def test_lstm_layer_fwd_hp_split_layers(ops, M, T, Kin, H):
    """evc_lstm_layer_fwd_hp (the "high" precision L2 level): split-bf16 operands as K-extensions - hoisted x-projection through
    evc_gemm_nt_split, recurrent part [lo(h) | hi(h)] . [Wh_hi | Wh_lo]^T + hi(h) . Wh_hi^T - against the float64 oracle on the
    UNROUNDED f32 operands: final states and every h_t to 1e-4 (the plain bf16 step on rounded operands: 6e-3)."""
    rng = np.random.default_rng(M * 3 + T + Kin + H)
    x = (rng.standard_normal((M, T, Kin)) * 0.7).astype(np.float32)
    kernel = (mm.glorot_uniform(rng, (Kin + H, 4 * H)) * 2.5).astype(np.float32)
    bias = (rng.standard_normal(4 * H) * 0.1).astype(np.float32)
    lens = rng.integers(0, T + 1, size=M).astype(np.int32)
    lens[:3] = [0, T, 1]
    s_ref, cache = mm.multi_rnn_seq_fwd(x.astype(np.float64), lens, [(kernel.astype(np.float64), bias.astype(np.float64))])
    xt = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2))).to(DEV).reshape(T * M, Kin)
    x_w = torch.empty((T * M, 2 * Kin), dtype=torch.bfloat16, device=DEV)
    ops.cast_bf16_wide(xt, x_w, lo_first=True)
    wT = torch.from_numpy(np.ascontiguousarray(kernel.T)).to(DEV)            # [4H][Kin+H]
    wx = torch.empty((4 * H, 2 * Kin), dtype=torch.bfloat16, device=DEV)
    wh = torch.empty((4 * H, 2 * H), dtype=torch.bfloat16, device=DEV)
    ops.cast_bf16_wide(wT[:, :Kin], wx, lo_first=False)
    ops.cast_bf16_wide(wT[:, Kin:], wh, lo_first=False)
    b = torch.from_numpy(bias).to(DEV)
    ln = torch.from_numpy(lens).to(DEV)
    zx = torch.empty((T * M, 4 * H), dtype=torch.float32, device=DEV)
    hbuf = torch.full((T + 1, M, H), float("nan"), dtype=torch.bfloat16, device=DEV)
    hw = torch.full((T + 1, M, 2 * H), float("nan"), dtype=torch.bfloat16, device=DEV)
    S = torch.full((M, 2 * H), float("nan"), dtype=torch.float32, device=DEV)
    gates = torch.empty((T, M, H, 2), dtype=torch.int32, device=DEV)
    c_all = torch.full((T + 1, M, H), float("nan"), dtype=torch.bfloat16, device=DEV)
    ops.lstm_layer_fwd_hp(x_w, wx, wh, b, ln, T, M, Kin, H, zx, hbuf, hw, S[:, :H], S[:, H:], 2 * H, gates, c_all)
    got = S.cpu().double().numpy()
    assert np.isfinite(got).all()
    err = np.max(np.abs(got - s_ref))
    assert err < 1e-4, err
    assert np.all(got[0] == 0)
    hwn = hw.float().cpu().numpy()
    hsum = hwn[:, :, :H] + hwn[:, :, H:]                                # lo + hi
    assert np.all(hwn[0] == 0) and torch.equal(hw[:, :, H:], hbuf)      # the plain image is the hi half
    # h_t of the oracle: replay the cell on its cached per-step states is not exposed - check the recurrence instead: every
    # live h_t equals tanh(c_t) * sigmoid(o) to split precision through the final h of rows that end at step t
    for t in range(T):
        dead = lens <= t
        assert np.all(hwn[t + 1][dead] == 0)
        ends = lens == t + 1
        if ends.any():
            assert np.max(np.abs(hsum[t + 1][ends] - s_ref[ends][:, H:])) < 1e-4


@pytest.mark.parametrize("M,T,Kin,H,ext", [(256, 5, 256, 64, False), (40, 6, 128, 128, True), (96, 20, 512, 128, False), (96, 20, 512, 128, True)])
def test_lstm_stack2_fwd_f16_weight_lo_extension(ops, M, T, Kin, H, ext):
    """evc_lstm_stack2_fwd_f16 (the "high" precision L2 level): two layers in wavefront order on IEEE f16 operands, layer 0 plain
    (hoisted f16 x-projection), layer 1 with its weights K-extended by their low-order halves ([h | h/64] . [W | W_lo*64]^T) - against
    the float64 oracle on f16-rounded x and layer-0 kernel and the UNROUNDED f32 layer-1 kernel: the states must sit within 8e-4
    (activations re-quantised to f16 between steps), the wide images must be [f16(h) | f16(h)/64] and the bf16 copies roundings of the
    same values; with the layer-1 kernel merely f16-rounded in the oracle the distance grows (the extension is doing its job)."""
    rng = np.random.default_rng(M + T + Kin + H + 7)
    f16r = lambda a: torch.from_numpy(np.asarray(a, np.float32)).half().double().numpy()
    x = f16r(rng.standard_normal((M, T, Kin)) * 0.5)
    k0 = f16r(mm.glorot_uniform(rng, (Kin + H, 4 * H)) * 2.0)
    k1 = (mm.glorot_uniform(rng, (2 * H, 4 * H)) * 2.0).astype(np.float32)
    b0 = (rng.standard_normal(4 * H) * 0.1).astype(np.float32)
    b1 = (rng.standard_normal(4 * H) * 0.1).astype(np.float32)
    lens = rng.integers(0, T + 1, size=M).astype(np.int32)
    lens[:3] = [0, T, 1]
    layers = [(k0, b0.astype(np.float64)), (k1.astype(np.float64), b1.astype(np.float64))]
    s_ref, _ = mm.multi_rnn_seq_fwd(x, lens, layers)
    s_rounded, _ = mm.multi_rnn_seq_fwd(x, lens, [layers[0], (f16r(k1), layers[1][1])])
    x16 = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2)).astype(np.float32)).half().to(DEV)
    w0 = torch.from_numpy(np.ascontiguousarray(k0.T).astype(np.float32)).half().to(DEV)
    x16p, w0p = x16, w0                              # plain images: the reference call for layer 0 below
    if ext:      # layer 0 K-extended as well: input in 3 segments, recurrent weights + low halves (x and k0 are f16-exact here, so
        #          the extra segments are zeros / scaled copies and the result must not move)
        x16 = torch.empty((T * M, 3 * Kin), dtype=torch.float16, device=DEV)
        ops.cast_f16_segs(x16p.float().reshape(T * M, Kin), 3, x16)
        assert torch.equal(x16[:, :Kin], x16p.reshape(T * M, Kin)) and not bool(x16[:, Kin:2 * Kin].any())
        x16 = x16.view(T, M, 3 * Kin)
        w0 = torch.empty((4 * H, 3 * Kin + 2 * H), dtype=torch.float16, device=DEV)
        ops.cast_f16_wide(w0p.float(), Kin, H, 3, w0, h_ext=True)
    w1 = torch.empty((4 * H, 4 * H), dtype=torch.float16, device=DEV)
    k1T = torch.from_numpy(np.ascontiguousarray(k1.T)).to(DEV)
    ops.cast_f16_wlo(k1T, H, H, w1)
    hi = k1T.half()
    assert torch.equal(w1[:, :H], hi[:, :H]) and torch.equal(w1[:, 2 * H:3 * H], hi[:, H:])
    assert torch.equal(w1[:, H:2 * H], ((k1T[:, :H] - hi[:, :H].float()) * 64.0).half())
    zx = torch.empty((T * M, 4 * H), dtype=torch.float32, device=DEV)
    hw = [torch.full((T + 1, M, 2 * H), float("nan"), dtype=torch.float16, device=DEV) for _ in range(2)]
    hb = [torch.full((T + 1, M, H), float("nan"), dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    S = torch.full((M, 4 * H), float("nan"), dtype=torch.float32, device=DEV)
    gates = [torch.empty((T, M, H, 2), dtype=torch.int32, device=DEV) for _ in range(2)]
    c_all = [torch.full((T + 1, M, H), float("nan"), dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    ops.lstm_stack2_fwd_f16(x16, w0, torch.from_numpy(b0).to(DEV), w1, torch.from_numpy(b1).to(DEV), torch.from_numpy(lens).to(DEV),
                            T, M, Kin, H, zx, hw[0], hw[1], hb[0], hb[1], S, gates, c_all, x_segments=3 if ext else 1, h0_ext=ext)
    got = S.cpu().double().numpy()
    assert np.isfinite(got).all()
    err = np.max(np.abs(got - s_ref))
    assert err < 8e-4, err
    assert np.all(got[0] == 0)
    for l in range(2):
        hwn, hbn = hw[l].float().cpu().numpy(), hb[l].float().cpu().numpy()
        assert np.all(hwn[0] == 0) and np.all(hbn[0] == 0)
        assert np.max(np.abs(hwn[:, :, H:] * 64.0 - hwn[:, :, :H])) <= 64 * 2.0 ** -25          # the scaled copy (subnormal step 2^-24)
        assert np.max(np.abs(hwn[:, :, :H] - hbn)) <= 2.0 ** -8                                 # two roundings of the same h
        for t in range(T):
            assert np.all(hwn[t + 1][lens <= t] == 0) and np.all(hbn[t + 1][lens <= t] == 0)
    # the same steps through two plain bf16-free references: per-layer f16 kernel for layer 0 gives the same layer-0 states
    S0 = torch.full((M, 2 * H), float("nan"), dtype=torch.float32, device=DEV)
    h16 = torch.empty((T + 1, M, H), dtype=torch.float16, device=DEV)
    hbf = torch.empty((T + 1, M, H), dtype=torch.bfloat16, device=DEV)
    ops.lstm_layer_fwd_f16(x16p, w0p, torch.from_numpy(b0).to(DEV), torch.from_numpy(lens).to(DEV), T, M, Kin, H, h16, hbf, S0[:, :H], S0[:, H:], 2 * H)
    # (hoisted vs fused x-projection: the accumulation order differs by ~1e-7, which now and then flips the f16 rounding of an
    #  h entry - one f16 ulp, 2.4e-4 at |h| ~ 0.5 - and that flip travels on through the remaining steps)
    assert float((S0 - S[:, :2 * H]).abs().max()) < 8e-4
    print("stack2 f16: state err %.2e (oracle with f16-rounded layer-1 kernel: %.2e away from the exact one)" % (err, np.max(np.abs(s_rounded - s_ref))))


def _e4m3(a, scale):
    """torch's OCP e4m3fn rounding (nearest even, the reference for the hardware's v_cvt_pk_fp8_f32) of a * scale, clamped to +-448."""
    return (a.float() * scale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)


def test_fp8_low_order_weight_cast_and_input_rows(ops):
    """evc_cast_f32_to_fp8_lo = e4m3(clamp((w - f16(w)) 2^17)) bit for bit against torch's float8_e4m3fn (values over eleven decades,
    including ones whose low-order half underflows e4m3 and ones that clamp), and with hi_cols its three-block rows [lo(Wx) | e4m3(Wx 2^6) |
    lo(Wh)]; evc_l2norm_chunk_fwd aux_mode 5 writes rows [f16(x) | e4m3(x 2^7) | e4m3((x - f16(x)) 2^18)]: the first part is the f16 image,
    the bytes are the e4m3 images of the normalised values and of their f16 remainders (compared through torch's rounding of the f16 +
    low-order reconstruction of the two-segment image, allowing one code step where the f32 value sits on a rounding boundary)."""
    g = torch.Generator(device="cpu")
    g.manual_seed(11)
    w = (torch.rand((132, 256), generator=g) * 2 - 1) * torch.logspace(-9, 1, 256)[None, :]
    w[5, :8] = torch.tensor([3.99, -3.99, 7.5, -100.0, 0.0, 1.0, -1.0, 2.0 ** -20])
    zero_ok = lambda got, ref: bool(((got == ref) | (((got & 0x7f) == 0) & ((ref & 0x7f) == 0))).all())    # +0 / -0 codes of exact zeros
    out = torch.zeros((132, 256), dtype=torch.uint8, device=DEV)
    ops.cast_fp8_lo(w.to(DEV), out)
    ref = _e4m3(w - w.half().float(), 2.0 ** ops.FP8_W_SCALE_EXP).view(torch.uint8)
    got = out.cpu()
    assert zero_ok(got, ref), int((got != ref).sum())
    assert int((got & 0x7f).max()) <= 0x7e                      # never the NaN code
    out3 = torch.zeros((132, 256 + 64), dtype=torch.uint8, device=DEV)
    ops.cast_fp8_lo(w.to(DEV), out3, hi_cols=64)
    g3 = out3.cpu()
    assert torch.equal(g3[:, :64], got[:, :64]) and torch.equal(g3[:, 128:], got[:, 64:])
    assert zero_ok(g3[:, 64:128], _e4m3(w[:, :64], 2.0 ** ops.FP8_WX_HI_EXP).view(torch.uint8))
    B, T, F, C1, C2, every_n = 3, 60, 128, 4, 2, 10
    q, x, n, _ = mm.synthetic_batch(B, seed=3, max_frames=T, feature_size=F, vocab_size=8, dtype=np.float32)
    for inp, nf in ((torch.from_numpy(x).to(DEV), None), (torch.from_numpy(q).to(DEV), torch.from_numpy(n).to(DEV))):
        (t_bf, t_w2), (s_bf, s_w2) = ops.l2norm_chunk(inp, C1, every_n, C2, num_frames=nf, split="f16", f16_segments=2)
        (t_bf5, t_5), (s_bf5, s_5) = ops.l2norm_chunk(inp, C1, every_n, C2, num_frames=nf, split="f16", fp8_tail=True)
        assert t_5.shape == t_w2.shape[:2] + (2 * F,) and s_5.shape == s_w2.shape[:2] + (2 * F,)
        assert torch.equal(t_bf, t_bf5) and torch.equal(s_bf, s_bf5)
        for w2, w5 in ((t_w2, t_5), (s_w2, s_5)):
            assert torch.equal(w5[:, :, :F], w2[:, :, :F])
            b8 = w5[:, :, F:].contiguous().view(torch.uint8)
            assert b8.shape[-1] == 2 * F
            xlo = w2[:, :, F:].float() / 64.0                              # x - f16(x) to f16's precision of the remainder
            xv = w2[:, :, :F].float() + xlo                                # the normalised f32 values to ~2^-22
            for part, want in ((b8[:, :, :F], _e4m3(xv, 128.0)), (b8[:, :, F:], _e4m3(xlo, 2.0 ** 18))):
                d = (part.to(torch.int16) - want.view(torch.uint8).to(torch.int16)).abs()
                d = torch.where((part & 0x7f) + (want.view(torch.uint8) & 0x7f) == 0, torch.zeros_like(d), d)       # +0 / -0
                assert int(d.max()) <= 1 and float((d > 0).float().mean()) < 3e-2, (int(d.max()), float((d > 0).float().mean()))


@pytest.mark.parametrize("M,T,Kin,H,nseg", [(96, 6, 512, 512, 1), (256, 20, 1024, 512, 2), (40, 5, 256, 640, 2)])
def test_lstm_stack2_fwd_f16_fp8_low_order_weights(ops, M, T, Kin, H, nseg):
    """evc_lstm_stack2_fwd_f16_fp8lo (the "high" precision L2 level with e4m3 low-order halves): two layers in wavefront order, layer 0 =
    hoisted f16 x-projection (input in nseg segments) + [f16(h0)] . f16(Wh0)^T + e4m3 correction, layer 1 = [h0 | h1] . [Wx | Wh]^T in f16 +
    e4m3 corrections of both weight blocks - against the float64 oracle on the UNROUNDED f32 kernels (x f16-exact): within the f16 activation
    bound (8e-4) and no further from it than evc_lstm_stack2_fwd_f16 with every weight K-extended by f16 low-order halves; h rows are
    [f16(h) | e4m3(h 2^7)], the bf16 copies roundings of the same values."""
    rng = np.random.default_rng(M + T + Kin + H + 17)
    f16r = lambda a: torch.from_numpy(np.asarray(a, np.float32)).half().double().numpy()
    x = f16r(rng.standard_normal((M, T, Kin)) * 0.5)
    k0 = (mm.glorot_uniform(rng, (Kin + H, 4 * H)) * 2.0).astype(np.float32)
    k0[:Kin] = f16r(k0[:Kin]).astype(np.float32)          # (the input weights are not extended in either form: keep them f16-exact)
    k1 = (mm.glorot_uniform(rng, (2 * H, 4 * H)) * 2.0).astype(np.float32)
    b0 = (rng.standard_normal(4 * H) * 0.1).astype(np.float32)
    b1 = (rng.standard_normal(4 * H) * 0.1).astype(np.float32)
    lens = rng.integers(0, T + 1, size=M).astype(np.int32)
    lens[:3] = [0, T, 1]
    s_ref, _ = mm.multi_rnn_seq_fwd(x, lens, [(k0.astype(np.float64), b0.astype(np.float64)), (k1.astype(np.float64), b1.astype(np.float64))])
    x16p = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2)).astype(np.float32)).half().to(DEV)
    x16 = torch.empty((T * M, nseg * Kin), dtype=torch.float16, device=DEV)
    ops.cast_f16_segs(x16p.float().reshape(T * M, Kin), nseg, x16)
    x16 = x16.view(T, M, nseg * Kin)
    k0T, k1T = torch.from_numpy(np.ascontiguousarray(k0.T)).to(DEV), torch.from_numpy(np.ascontiguousarray(k1.T)).to(DEV)
    bd0, bd1, ln = torch.from_numpy(b0).to(DEV), torch.from_numpy(b1).to(DEV), torch.from_numpy(lens).to(DEV)
    zx = torch.empty((T * M, 4 * H), dtype=torch.float32, device=DEV)
    hb = [torch.full((T + 1, M, H), float("nan"), dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    # e4m3 form
    w0 = torch.empty((4 * H, nseg * Kin + H), dtype=torch.float16, device=DEV)
    ops.cast_f16_wide(k0T, Kin, H, nseg, w0, h_ext=False)
    w0_8 = torch.empty((4 * H, H), dtype=torch.uint8, device=DEV)
    ops.cast_fp8_lo(k0T[:, Kin:], w0_8)
    w1 = torch.empty((4 * H, 2 * H), dtype=torch.float16, device=DEV)
    ops.cast_f16(k1T, w1)
    w1_8 = torch.empty((4 * H, 2 * H), dtype=torch.uint8, device=DEV)
    ops.cast_fp8_lo(k1T, w1_8)
    hr = [torch.full((T + 1, M, 3 * H // 2), float("nan"), dtype=torch.float16, device=DEV) for _ in range(2)]
    S = torch.full((M, 4 * H), float("nan"), dtype=torch.float32, device=DEV)
    ops.lstm_stack2_fwd_f16_fp8lo(x16, w0, w0_8, bd0, w1, w1_8, bd1, ln, T, M, Kin, H, zx, hr[0], hr[1], hb[0], hb[1], S, x_segments=nseg)
    got = S.cpu().double().numpy()
    assert np.isfinite(got).all() and np.all(got[0] == 0)
    err = np.max(np.abs(got - s_ref))
    for l in range(2):
        hn, hbn = hr[l][:, :, :H].float(), hb[l].float()
        assert bool((hn[0] == 0).all()) and float((hn - hbn).abs().max()) <= 2.0 ** -8
        h8 = hr[l][:, :, H:].contiguous().view(torch.uint8)
        d = (h8.to(torch.int16) - (hn * 128.0).to(torch.float8_e4m3fn).view(torch.uint8).to(torch.int16)).abs()
        assert int(d.max()) <= 1 and float((d > 0).float().mean()) < 2e-2
        for t in range(T):
            dead = torch.from_numpy(lens <= t).to(DEV)
            assert bool((hn[t + 1][dead] == 0).all()) and bool((h8[t + 1][dead] == 0).all())
    # h_lo (round 6): the activations' low-order halves corrected as well - rows [f16(h) | e4m3(h 2^7) | e4m3((h - f16(h)) 2^18)] against
    # [lo(Wh0) | hi(Wh0)] / [lo(Wx1) | hi(Wx1) | lo(Wh1) | hi(Wh1)]: the "f16 activation bound" above goes too
    w0_8l = torch.empty((4 * H, 2 * H), dtype=torch.uint8, device=DEV)
    ops.cast_fp8_lo(k0T[:, Kin:], w0_8l, hi_tail=True)
    assert torch.equal(w0_8l[:, :H], w0_8) and torch.equal(w0_8l[:, H:], (k0T[:, Kin:] * 64.0).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8))
    w1_8l = torch.empty((4 * H, 4 * H), dtype=torch.uint8, device=DEV)
    ops.cast_fp8_lo(k1T, w1_8l, hi_cols=H, hi_tail=True)
    assert torch.equal(w1_8l[:, :H], w1_8[:, :H]) and torch.equal(w1_8l[:, 2 * H:3 * H], w1_8[:, H:])
    hrl = [torch.full((T + 1, M, 2 * H), float("nan"), dtype=torch.float16, device=DEV) for _ in range(2)]
    hbl = [torch.full((T + 1, M, H), float("nan"), dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    Sl = torch.full((M, 4 * H), float("nan"), dtype=torch.float32, device=DEV)
    ops.lstm_stack2_fwd_f16_fp8lo(x16, w0, w0_8l, bd0, w1, w1_8l, bd1, ln, T, M, Kin, H, zx, hrl[0], hrl[1], hbl[0], hbl[1], Sl, x_segments=nseg, h_lo=True)
    got_lo = Sl.cpu().double().numpy()
    assert np.isfinite(got_lo).all() and np.all(got_lo[0] == 0)
    err_lo = np.max(np.abs(got_lo - s_ref))
    for l in range(2):
        l8 = hrl[l][:, :, 3 * H // 2:].contiguous().view(torch.float8_e4m3fn).float()
        assert bool(torch.isfinite(l8).all()) and float(l8.abs().max()) <= 64.0 and bool((l8[0] == 0).all())
        assert float((hrl[l][:, :, :H].float() - hr[l][:, :, :H].float()).abs().max()) < 1e-2         # (the same recurrence, closer to the oracle)
    print("stack2 f16 + e4m3 low-order halves of the weights: state err %.2e; + of the activations (h_lo) %.2e" % (err, err_lo))
    assert err_lo < 0.6 * err and err_lo < 3e-4, (err_lo, err)
    # f16 K-extension form on the same kernels
    w0e = torch.empty((4 * H, nseg * Kin + 2 * H), dtype=torch.float16, device=DEV)
    ops.cast_f16_wide(k0T, Kin, H, nseg, w0e, h_ext=True)
    w1e = torch.empty((4 * H, 4 * H), dtype=torch.float16, device=DEV)
    ops.cast_f16_wlo(k1T, H, H, w1e)
    hw = [torch.full((T + 1, M, 2 * H), float("nan"), dtype=torch.float16, device=DEV) for _ in range(2)]
    S2 = torch.full((M, 4 * H), float("nan"), dtype=torch.float32, device=DEV)
    ops.lstm_stack2_fwd_f16(x16, w0e, bd0, w1e, bd1, ln, T, M, Kin, H, zx, hw[0], hw[1], hb[0], hb[1], S2, x_segments=nseg, h0_ext=True)
    err_ext = np.max(np.abs(S2.cpu().double().numpy() - s_ref))
    print("stack2 f16 + e4m3 low-order halves: state err %.2e (f16 K-extensions %.2e)" % (err, err_ext))
    assert err < 8e-4 and err <= err_ext * 1.3 + 2e-5, (err, err_ext)


@pytest.mark.parametrize("M,N,K", [(256, 1416, 512), (64, 4716 * 3, 4096), (200, 700, 1024), (600, 520, 512), (512, 1024, 8192)])
def test_gemm_nt_f16_fp8_product_with_low_order_corrections(ops, M, N, K):
    """evc_gemm_nt_f16_fp8 = f16(x) . f16(W)^T + 2^-24 [e4m3(x 2^6) | e4m3(x_lo 2^17)] . [e4m3(W_lo 2^18) | e4m3(W 2^7)]^T + bias in one launch (the
    "high" precision MoE head), operands from evc_cast_f32_to_f16_fp8x / evc_cast_f32_to_f16 / evc_cast_f32_to_fp8_lo(hi_cols = K): against the
    float64 product of the f32 operands it must be >= 10x closer than the plain f16 product (the corrections remove the 2^-12 operand
    rounding to ~2^-16) and within 1e-4 of the largest |logit|; the activation rows have the documented layout; batch-row (M <= 256) and
    256 x 256 tiles, ragged N."""
    rng = np.random.default_rng(M + N + K)
    x = (rng.standard_normal((M, K)) * 1.3).astype(np.float32)
    w = (rng.standard_normal((N, K)) * 0.04).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    ref = x.astype(np.float64) @ w.astype(np.float64).T + bias
    xd, wd, bd = torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV), torch.from_numpy(bias).to(DEV)
    rows = torch.empty((M, 2 * K), dtype=torch.float16, device=DEV)
    ops.cast_f16_fp8x(xd, rows)
    assert torch.equal(rows[:, :K], xd.half())
    b8 = rows[:, K:].contiguous().view(torch.uint8)
    e = ops.FP8_MOE
    zero_ok = lambda got, want: bool(((got == want) | (((got & 0x7f) == 0) & ((want & 0x7f) == 0))).all())
    assert zero_ok(b8[:, :K], _e4m3(xd, 2.0 ** e["x_hi_exp"]).view(torch.uint8))
    assert zero_ok(b8[:, K:], _e4m3(xd - xd.half().float(), 2.0 ** e["x_lo_exp"]).view(torch.uint8))
    w16 = torch.empty((N, K), dtype=torch.float16, device=DEV)
    ops.cast_f16(wd, w16)
    w8 = torch.empty((N, 2 * K), dtype=torch.uint8, device=DEV)
    ops.cast_fp8_lo(wd, w8, hi_cols=K, scale_exp=e["w_lo_exp"], hi_exp=e["w_hi_exp"])
    out = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
    ops.gemm_nt_f16_fp8(rows, w16, w8, M, N, K, out, bias=bd)
    got = out.cpu().double().numpy()
    assert np.isfinite(got).all()
    err = np.max(np.abs(got - ref))
    plain = xd.half().double().cpu().numpy() @ wd.half().double().cpu().numpy().T + bias
    err16 = np.max(np.abs(plain - ref))
    # the numpy restatement of the same operand roundings (oracle/lowprec.py, float64 accumulation): the kernel differs from it only by
    # its f32 accumulation
    from oracle import lowprec as lp
    emu = lp.corrected_product(x, w, e["x_hi_exp"], e["x_lo_exp"], e["w_lo_exp"], e["w_hi_exp"]) + bias
    d_emu = np.max(np.abs(got - emu))
    print("gemm_nt_f16_fp8 %dx%dx%d: max err %.2e (plain f16 product %.2e; vs the numpy restatement %.2e), |z| max %.1f" % (
        M, N, K, err, err16, d_emu, np.abs(ref).max()))
    assert err < 1e-4 * max(1.0, np.abs(ref).max()) and err * 10 < err16, (err, err16)
    assert d_emu < 2e-5 * max(1.0, np.abs(ref).max()), d_emu


@pytest.mark.parametrize("amp,M,N,K", [(1.3, 64, 712, 512), (9.0, 64, 712, 512), (30.0, 256, 1416, 4096), (400.0, 200, 520, 1024), (5000.0, 64, 520, 512)])
def test_gemm_nt_f16_fp8_dynamic_range_of_the_activation_operand(ops, amp, M, N, K):
    """The MoE head's input is the L2 state [c | h]: its cell-state half is unbounded and the fixed e4m3(x 2^6) image saturates at |x| = 7 (towers
    trained for 512 steps: |c| ~ 16) - the correction of the weights' f16 rounding is then partly lost, silently.  evc_absmax_partials +
    evc_cast_f32_to_f16_fp8x_dyn + evc_gemm_nt_f16_fp8_dyn shift both e4m3 images of x down by the d bits the batch's largest |x| needs and
    scale the products back: (a) the image bytes are e4m3(x 2^(6 - d)) / e4m3(x_lo 2^(17 - d)) with d from oracle.lowprec.fp8_range_drop - no
    byte saturated; (b) the product equals the numpy restatement of the same roundings; (c) against the float64 product it is >= 10x closer
    than plain f16 and within 1e-4 |z| max at ANY amplitude, while the fixed-scale entry loses that once |x| > 7; (d) d = 0 (|x| <= 7)
    reproduces the fixed-scale entry bit for bit."""
    from oracle import lowprec as lp
    rng = np.random.default_rng(int(amp * 10) + M + N + K)
    x = (rng.standard_normal((M, K)) * 0.3).astype(np.float32)
    x[:, : K // 2] *= np.float32(amp / np.abs(x[:, : K // 2]).max())          # the "cell state" half reaches +-amp, the "h" half stays small
    w = (rng.standard_normal((N, K)) * 0.04).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    ref = x.astype(np.float64) @ w.astype(np.float64).T + bias
    zmax = np.abs(ref).max()
    xd, wd, bd = torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV), torch.from_numpy(bias).to(DEV)
    e = ops.FP8_MOE
    ws = torch.full((ops.AMAX_SLOTS,), float("nan"), dtype=torch.float32, device=DEV)
    ops.absmax_partials(xd, ws)
    assert float(ws.max()) == float(np.abs(x).max()) and float(ws.min()) >= 0.0
    d = lp.fp8_range_drop(np.abs(x).max(), e["x_hi_exp"])
    top = float(np.abs(x).max()) * 2.0 ** (e["x_hi_exp"] - d)
    assert (d == 0) == (np.abs(x).max() <= 7.0) and top <= 448.0 and (d == 0 or 2.0 * top > 448.0)      # the fewest bits that fit
    rows = torch.empty((M, 2 * K), dtype=torch.float16, device=DEV)
    ops.cast_f16_fp8x(xd, rows, amax_ws=ws)
    assert torch.equal(rows[:, :K], xd.half())
    b8 = rows[:, K:].contiguous().view(torch.uint8)
    zero_ok = lambda got, want: bool(((got == want) | (((got & 0x7f) == 0) & ((want & 0x7f) == 0))).all())
    assert zero_ok(b8[:, :K], _e4m3(xd, 2.0 ** (e["x_hi_exp"] - d)).view(torch.uint8))
    assert zero_ok(b8[:, K:], _e4m3(xd - xd.half().float(), 2.0 ** (e["x_lo_exp"] - d)).view(torch.uint8))
    w16 = torch.empty((N, K), dtype=torch.float16, device=DEV)
    ops.cast_f16(wd, w16)
    w8 = torch.empty((N, 2 * K), dtype=torch.uint8, device=DEV)
    ops.cast_fp8_lo(wd, w8, hi_cols=K, scale_exp=e["w_lo_exp"], hi_exp=e["w_hi_exp"])
    out = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
    ops.gemm_nt_f16_fp8(rows, w16, w8, M, N, K, out, bias=bd, amax_ws=ws)
    got = out.cpu().double().numpy()
    err = np.max(np.abs(got - ref))
    plain = xd.half().double().cpu().numpy() @ wd.half().double().cpu().numpy().T + bias
    err16 = np.max(np.abs(plain - ref))
    emu = lp.corrected_product_dyn(x, w, e["x_hi_exp"], e["x_lo_exp"], e["w_lo_exp"], e["w_hi_exp"]) + bias
    d_emu = np.max(np.abs(got - emu))
    # the fixed-scale entries on the same operands
    rows_f = torch.empty_like(rows)
    ops.cast_f16_fp8x(xd, rows_f)
    out_f = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
    ops.gemm_nt_f16_fp8(rows_f, w16, w8, M, N, K, out_f, bias=bd)
    err_fixed = np.max(np.abs(out_f.cpu().double().numpy() - ref))
    print("dynamic e4m3 range, |x| max %.0f (d = %d), |z| max %.1f: err %.2e (fixed 2^6 scale %.2e, plain f16 %.2e; vs the numpy restatement %.2e)"
          % (amp, d, zmax, err, err_fixed, err16, d_emu))
    assert np.isfinite(got).all()
    assert err < 1e-4 * max(1.0, zmax) and err * 10 < err16, (err, err16)
    assert d_emu < 2e-5 * max(1.0, zmax), d_emu
    if d == 0:
        assert torch.equal(out, out_f) and torch.equal(rows, rows_f)
    elif amp >= 30:
        assert err_fixed > 3 * err, (err_fixed, err)          # what the fixed scale loses to saturation


@pytest.mark.parametrize("M,T,Kin,H,tile", [(512, 4, 384, 384, 0), (1100, 3, 1152, 512, 0), (700, 5, 384, 384, 6), (390, 3, 512, 384, 7), (330, 3, 384, 384, 8), (730, 4, 384, 384, 11)])
def test_lstm_layer_fwd_f16_fp8_low_order_weights(M, T, Kin, H, tile):
    """evc_lstm_layer_fwd_f16_fp8lo (two stacked layers: layer 0 on input rows [f16(x) | e4m3(x 2^7) | e4m3(x_lo 2^18)], layer 1 on layer 0's
    h rows [f16(h) | e4m3(h 2^7)]): per step z = [x | h] . [Wx | Wh]^T in f16 + 2^-24 [x8 | x_lo8 | h8] . [e4m3(Wx_lo 2^17) | e4m3(Wx 2^6) |
    e4m3(Wh_lo 2^17)]^T on the MX-scaled fp8 MFMA.  Against the float64 oracle with EXACT weights and exact x: what is left is the f16 rounding of h (the
    same bound as the f16 layer with extended weights, 8e-4) - and next to the plain f16 layer on the same kernel it must be the
    closer one.  Every ring tile the launcher can pick (EVC_FORCE_TILE in a child process: 256 / 224 / 192 / 160 rows), rows that end
    early, a row plan.  Tile 11 = 240 rows split 7 + 8 row fragments between the two wave rows (gemm_core_v3.h, uneven split)."""
    code = _FP8LO_CHILD % dict(M=M, T=T, Kin=Kin, H=H)
    env = dict(os.environ)
    if tile:
        env["EVC_FORCE_TILE"] = str(tile)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout.strip().splitlines()[-1])


_FP8LO_CHILD = r"""
import numpy as np, torch
from oracle import model_math as mm
from efficientvideoclassification_youtube8m_amd import ops
DEV = "cuda:0"
M, T, Kin, H = %(M)d, %(T)d, %(Kin)d, %(H)d
rng = np.random.default_rng(M + T + Kin + H)
x = (rng.standard_normal((M, T, Kin)) * 0.05).astype(np.float32)
x /= np.maximum(1.0, np.abs(x).max())
k0 = (mm.glorot_uniform(rng, (Kin + H, 4 * H)) * 3.0).astype(np.float32)
k1 = (mm.glorot_uniform(rng, (2 * H, 4 * H)) * 3.0).astype(np.float32)
b0 = (rng.standard_normal(4 * H) * 0.1).astype(np.float32)
b1 = (rng.standard_normal(4 * H) * 0.1).astype(np.float32)
lens = rng.integers(0, T + 1, size=M).astype(np.int32)
lens[:3] = [0, T, 1]
s_ref, _ = mm.multi_rnn_seq_fwd(x.astype(np.float64), lens, [(k0.astype(np.float64), b0.astype(np.float64)), (k1.astype(np.float64), b1.astype(np.float64))])
# input rows [f16(x) | e4m3(x 2^7) | e4m3((x - f16(x)) 2^18)], time-major; next to them the two-segment f16 rows [f16(x) | (x - f16(x)) 64]
xt = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2))).to(DEV)
rows = torch.zeros((T, M, 2 * Kin), dtype=torch.float16, device=DEV)
hi = xt.half()
rows[:, :, :Kin] = hi
rows[:, :, Kin:3 * Kin // 2] = (xt * 128.0).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.float16)
rows[:, :, 3 * Kin // 2:] = ((xt - hi.float()) * 2.0 ** 18).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.float16)
rows2 = torch.zeros((T, M, 2 * Kin), dtype=torch.float16, device=DEV)
rows2[:, :, :Kin] = hi
rows2[:, :, Kin:] = ((xt - hi.float()) * 64.0).half()
ln = torch.from_numpy(lens).to(DEV)
def run(plan, hlo=False):
    S = torch.full((M, 4 * H), float("nan"), dtype=torch.float32, device=DEV)
    inp, ldx, kx16, x8_off, kx8 = rows, 2 * Kin, Kin, 2 * Kin, 2 * Kin
    wrow = 2 * H if hlo else 3 * H // 2           # h rows: [f16(h) | e4m3(h 2^7)] (+ e4m3((h - f16(h)) 2^18) with h_lo)
    lens_run, Mrun = ln, M
    if plan is not None:          # slot order: rows sorted by length, the length-0 rows dropped
        live = plan.rows[0]
        inp = torch.zeros((T, plan.P, 2 * Kin), dtype=torch.float16, device=DEV)
        inp[:, :live] = rows[:, plan.inv[:live].long()]
        lens_run, Mrun = plan.lens, plan.P
        S.zero_()
    for l, (k, b) in enumerate(((k0, b0), (k1, b1))):
        kT = torch.from_numpy(np.ascontiguousarray(k.T)).to(DEV)
        nin = k.shape[0] - H
        w16 = torch.empty((4 * H, nin + H), dtype=torch.float16, device=DEV)
        ops.cast_f16(kT, w16)
        if hlo:                   # [lo(Wx) | hi(Wx) | lo(Wh) | hi(Wh)]: both activation operands' low-order halves are contracted against full-value images
            w8 = torch.empty((4 * H, 2 * (nin + H)), dtype=torch.uint8, device=DEV)
            ops.cast_fp8_lo(kT, w8, hi_cols=nin, hi_tail=True)
            assert torch.equal(w8[:, :2 * nin], ops.cast_fp8_lo(kT, torch.empty((4 * H, 2 * nin + H), dtype=torch.uint8, device=DEV), hi_cols=nin)[:, :2 * nin])
            assert torch.equal(w8[:, 2 * nin:2 * nin + H], ops.cast_fp8_lo(kT, torch.empty((4 * H, nin + H), dtype=torch.uint8, device=DEV))[:, nin:])
            assert torch.equal(w8[:, 2 * nin + H:], (kT[:, nin:] * 64.0).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8))
        else:
            w8 = torch.empty((4 * H, kx8 + H), dtype=torch.uint8, device=DEV)
            ops.cast_fp8_lo(kT, w8, hi_cols=kx8 - nin)
        h16 = torch.full((T + 1, Mrun, wrow), float("nan"), dtype=torch.float16, device=DEV)
        hbf = torch.full((T + 1, Mrun, H), float("nan"), dtype=torch.bfloat16, device=DEV)
        ops.lstm_layer_fwd_f16_fp8lo(inp, ldx, kx16, x8_off, kx8, w16, w8, torch.from_numpy(b).to(DEV), lens_run, T, Mrun, H, h16, hbf,
                                     S[:, 2 * l * H:], S[:, (2 * l + 1) * H:], 4 * H, plan=plan, h_lo=hlo)
        if plan is None:          # (with a plan the rows beyond a step's active prefix are never written)
            hn = h16[:, :, :H].float()
            assert float((hn - hbf.float()).abs().max()) <= 2.0 ** -8
            h8 = h16[:, :, H:3 * H // 2].contiguous().view(torch.uint8)
            if hlo:               # the low-order image: |h - f16(h)| 2^18 <= 64, finite, never the NaN code, and not all zero
                l8 = h16[:, :, 3 * H // 2:].contiguous().view(torch.float8_e4m3fn).float()
                assert bool(torch.isfinite(l8).all()) and float(l8.abs().max()) <= 64.0 and float((l8 != 0).float().mean()) > 0.3
            want = (hn * 128.0).to(torch.float8_e4m3fn).view(torch.uint8)       # (from the f16 image: one code step of slack on boundaries)
            d = (h8.to(torch.int16) - want.to(torch.int16)).abs()
            assert int(d.max()) <= 1 and float((d > 0).float().mean()) < 2e-2, (int(d.max()), float((d > 0).float().mean()))
        inp, ldx, kx16, x8_off, kx8 = h16[1:], wrow, H, 2 * H, (2 * H if hlo else H)
    return S.cpu().double().numpy()
got = run(None)
assert np.isfinite(got).all() and np.all(got[0] == 0)
err = float(np.max(np.abs(got - s_ref)))
# the plain f16 layers on the same kernels (x exact through its two segments there too)
S = torch.full((M, 4 * H), float("nan"), dtype=torch.float32, device=DEV)
inp, ldx, kx = rows2, 2 * Kin, 2 * Kin
for l, (k, b) in enumerate(((k0, b0), (k1, b1))):
    kT = torch.from_numpy(np.ascontiguousarray(k.T)).to(DEV)
    nin = k.shape[0] - H
    w16 = torch.empty((4 * H, kx + H), dtype=torch.float16, device=DEV)
    ops.cast_f16_wide(kT, nin, H, kx // nin, w16, h_ext=False)
    h16 = torch.full((T + 1, M, H), float("nan"), dtype=torch.float16, device=DEV)
    hbf = torch.full((T + 1, M, H), float("nan"), dtype=torch.bfloat16, device=DEV)
    ops.lstm_layer_fwd_f16(inp, w16, torch.from_numpy(b).to(DEV), ln, T, M, kx, H, h16, hbf, S[:, 2 * l * H:], S[:, (2 * l + 1) * H:], 4 * H, ldx=ldx)
    inp, ldx, kx = h16[1:], H, H
err16 = float(np.max(np.abs(S.cpu().double().numpy() - s_ref)))
# a row plan: rows sorted by length, the padding rows dropped - the same states in the original row order
gp = run(ops.RowPlan(ln, lens, T))
assert float(np.max(np.abs(gp - got))) < 1e-6
# h_lo (round 6): the low-order half of h corrected as well - what was "left" above (the f16 rounding of h) goes too
got_lo = run(None, hlo=True)
assert np.isfinite(got_lo).all() and np.all(got_lo[0] == 0)
err_lo = float(np.max(np.abs(got_lo - s_ref)))
gp_lo = run(ops.RowPlan(ln, lens, T), hlo=True)
assert float(np.max(np.abs(gp_lo - got_lo))) < 1e-6
print("fp8lo two-layer stack M=%%d T=%%d Kin=%%d H=%%d: state err %%.2e (plain f16 layers %%.2e; with h_lo %%.2e)" %% (M, T, Kin, H, err, err16, err_lo))
assert err < 8e-4 and err <= err16 * 1.05, (err, err16)
assert err_lo < 0.5 * err and err_lo < 2e-4, (err_lo, err)
"""


@pytest.mark.parametrize("M,N,K,l2", [(14148, 4096, 1024, 2e-8), (9432, 4096, 1024, 0.0), (2000, 1024, 256, 0.5), (1400, 512, 4096, 1e-3)])
def test_gemm_nt_with_the_clip_norm_from_the_same_pass(ops, M, N, K, l2):
    """evc_gemm_nt_sqnorm (round 6; the MoE weight gradient materialised at 1024 rows, cfg 5): the product is bit-identical to evc_gemm_nt's and
    the norm rows it leaves - {|C + l2 P|^2, |P|^2} from the tiles' stores - equal evc_grad_sqnorm's over the stored product (f32 sums in another
    order: 1e-5 relative), with and without the l2 term; shapes it does not take are refused."""
    torch.manual_seed(M + N + K)
    A = (torch.randn(M, K, device=DEV) * 0.3).to(torch.bfloat16)
    Bm = (torch.randn(N, K, device=DEV) * 0.3).to(torch.bfloat16)
    P = torch.randn(M, N, device=DEV) * 2.0
    ref = torch.full((M, N), float("nan"), device=DEV)
    ops.gemm_nt(A, Bm, M, N, K, ref)
    rs = torch.zeros(2, device=DEV)
    ops.grad_sqnorm(ref, P if l2 else None, l2, rs)
    out = torch.full((M, N), float("nan"), device=DEV)
    sums = torch.zeros(2, device=DEV)
    ops.gemm_nt_sqnorm(A, Bm, M, N, K, out, P if l2 else None, l2, sums)
    assert torch.equal(out, ref)
    want = ((ref.double() + l2 * P.double()) ** 2).sum().item()
    assert abs(sums[0].item() - want) <= 2e-5 * want and abs(sums[0].item() - rs[0].item()) <= 2e-5 * want, (sums, rs, want)
    if l2:
        wp = (P.double() ** 2).sum().item()
        assert abs(sums[1].item() - wp) <= 2e-5 * wp and abs(rs[1].item() - wp) <= 2e-5 * wp
    else:
        assert sums[1].item() == 0.0
    assert not ops.gemm_nt_sqnorm_ok(300, 4096, 1024) and not ops.gemm_nt_sqnorm_ok(2000, 1000, 1024)
    assert not ops.gemm_nt_sqnorm_ok(M, N, K) or os.environ.get("EVC_FUSED_GRAD_NORM") == "1"      # (measured slower on cfg 5: off unless asked for)
    with pytest.raises(Exception):
        ops.gemm_nt_sqnorm(A[:300], Bm, 300, N, K, out[:300], None, 0.0, sums)


@pytest.mark.parametrize("every_n,plans", [(10, False), (10, True), (30, True)])
def test_l2norm_chunk_int_images_of_the_uint8_frames(ops, every_n, plans):
    """evc_l2norm_chunk_int (round 6): the reader's uint8 frames as EXACT integers for the "high" layer 0 - per view the usual bf16 image, rows
    [f16(2q - 255) | e4m3(x_hat 2^7)] and one f32 per frame row, rs = (2/255) / |x|: rs (c + 255/256) reproduces the l2-normalised dequantised
    frame (cs/utils.py:22-25, cs/train.py:253-256) to f32 rounding; padded frames are all-zero rows with rs = 0; the e4m3 part equals the one of
    the f32-input rows (aux_mode 5); student-only (teacher_view=False) gives the same student images."""
    B, T, F, C2 = 6, 300, 1152, 5
    q, x, n, _ = mm.synthetic_batch(B, seed=50 + every_n, dtype=np.float32)
    n[0], n[1] = 300, 29
    qd, nd = torch.from_numpy(q).to(DEV), torch.from_numpy(n).to(DEV)
    S = T // every_n
    p1 = p2 = None
    if plans:
        _, l1, _ = ops.frame_counts(nd, 1, 20, 15)
        _, l1s, _ = ops.frame_counts(nd, every_n, C2, S // C2, subsampled=True)
        p1 = ops.RowPlan(l1, ops.host_frame_counts(n, 1, 20, 15)[1], 15)
        p2 = ops.RowPlan(l1s, ops.host_frame_counts(n, every_n, C2, S // C2, subsampled=True)[1], S // C2)
    (b1, i1, r1), (b2, i2, r2) = ops.l2norm_chunk_int(qd, nd, 20, every_n, C2, plan1=p1, plan2=p2)
    (f1, m1), (f2, m2) = ops.l2norm_chunk(qd, 20, every_n, C2, num_frames=nd, split="f16", f16_segments=1, fp8_tail=True, plan1=p1, plan2=p2)
    for bf, ii, rs, fb, m5, plan, rows_all in ((b1, i1, r1, f1, m1, p1, 20 * B), (b2, i2, r2, f2, m2, p2, C2 * B)):
        live = plan.rows[0] if plan is not None else rows_all
        assert torch.equal(bf[:, :live], fb[:, :live])                                      # the bf16 image is the usual one
        c = ii[:, :live, :F].float()
        assert bool((c == c.round()).all()) and float(c.abs().max()) <= 255.0
        x8 = ii[:, :live, F:].contiguous().view(torch.uint8)
        x8_5 = m5[:, :live, F:3 * F // 2].contiguous().view(torch.uint8)
        assert torch.equal(x8, x8_5)                                                          # e4m3(x_hat 2^7): the same bytes as the f32-input rows
        xhat = rs[:, :live, None] * (c + 255.0 / 256.0)
        dead = rs[:, :live] == 0
        assert bool((c[dead] == 0).all())                                                     # padded frames: zero integers, zero scale
        ref16 = m5[:, :live, :F].float()                                                      # f16(x_hat) of the f32-input rows
        assert float((xhat - ref16)[~dead].abs().max()) <= 2.0 ** -11 * 1.001               # (|x_hat| <= 1: half an f16 ulp)
        assert bool(((c[~dead] % 2).abs() == 1).all())                                        # odd integers 2q - 255
    # exact reconstruction against numpy on the plain layout
    if not plans:
        xr = mm.dequantize(q.astype(np.float64))            # (from q: n[0] was raised to 300 above, synthetic_batch's x is zero beyond ITS count)
        xr[np.arange(T)[None, :] >= n[:, None]] = 0.0
        nrm = np.sqrt((xr ** 2).sum(-1, keepdims=True))
        xh = np.where(nrm > 0, xr / np.maximum(nrm, 1e-6), 0.0)                               # [B, T, F]
        got = (r1[:, :, None] * (i1[:, :, :F].float() + 255.0 / 256.0)).cpu().double().numpy()  # [15][20 B][F], row = chunk * B + b
        want = xh.reshape(B, 20, 15, F).transpose(2, 1, 0, 3).reshape(15, 20 * B, F)
        assert np.abs(got - want).max() < 2e-7
    only = ops.l2norm_chunk_int(qd, nd, 20, every_n, C2, plan2=p2, teacher_view=False)
    live2 = p2.rows[0] if p2 is not None else C2 * B
    assert only[0] is None and all(torch.equal(a[:, :live2], b[:, :live2]) for a, b in zip(only[1], (b2, i2, r2)))


def test_lstm_layer_fwd_integer_frames_are_exact(ops):
    """evc_lstm_layer_fwd_f16_fp8lo with x_int (round 6): layer 0 contracts the integers 2q - 255 against f16(Wx), rescales its accumulators by the
    frame's factor behind the x-part (LOOP_ROW_SCALE) and starts them from (255/256) colsum(f16(Wx)); with the weights' and h's low-order halves in
    e4m3 (h_lo) what is left against the float64 oracle on the EXACT dequantised, l2-normalised frames and exact weights is the corrections' own
    quantisation: closer than the f32-input form (x rounded to f16, its low-order half in e4m3), row plans included."""
    M, T, F, H = 700, 5, 384, 384
    rng = np.random.default_rng(77)
    q = rng.integers(0, 256, size=(M, T, F), dtype=np.uint8)
    lens = rng.integers(0, T + 1, size=M).astype(np.int32)
    lens[:3] = [0, T, 1]
    xr = mm.dequantize(q.astype(np.float64))
    xh = xr / np.sqrt((xr ** 2).sum(-1, keepdims=True))
    k0 = (mm.glorot_uniform(rng, (F + H, 4 * H)) * 3.0).astype(np.float32)
    b0 = (rng.standard_normal(4 * H) * 0.1).astype(np.float32)
    s_ref, _ = mm.multi_rnn_seq_fwd(xh, lens, [(k0.astype(np.float64), b0.astype(np.float64))])
    xt = torch.from_numpy(np.ascontiguousarray(xh.transpose(1, 0, 2)).astype(np.float32)).to(DEV)          # [T][M][F]
    qt = torch.from_numpy(np.ascontiguousarray(q.transpose(1, 0, 2))).to(DEV)
    kT = torch.from_numpy(np.ascontiguousarray(k0.T)).to(DEV)
    w16 = torch.empty((4 * H, F + H), dtype=torch.float16, device=DEV)
    ops.cast_f16(kT, w16)
    w8 = torch.empty((4 * H, 2 * (F + H)), dtype=torch.uint8, device=DEV)
    ops.cast_fp8_lo(kT, w8, hi_cols=F, hi_tail=True)
    bd, ln = torch.from_numpy(b0).to(DEV), torch.from_numpy(lens).to(DEV)
    # f32-input rows [f16(x) | e4m3(x 2^7) | e4m3(x_lo 2^18)] and integer rows [f16(2q - 255) | e4m3(x 2^7)] + row scales
    rows5 = torch.zeros((T, M, 2 * F), dtype=torch.float16, device=DEV)
    hi = xt.half()
    rows5[:, :, :F] = hi
    x8 = (xt * 128.0).clamp(-448, 448).to(torch.float8_e4m3fn)
    rows5[:, :, F:3 * F // 2] = x8.view(torch.float16)
    rows5[:, :, 3 * F // 2:] = ((xt - hi.float()) * 2.0 ** 18).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.float16)
    rows6 = torch.zeros((T, M, 3 * F // 2), dtype=torch.float16, device=DEV)
    rows6[:, :, :F] = (2.0 * qt.float() - 255.0).half()
    rows6[:, :, F:] = x8.view(torch.float16)
    nrm = torch.from_numpy(np.ascontiguousarray(np.sqrt((xr ** 2).sum(-1)).T)).to(DEV)                    # [T][M]
    rs = ((2.0 / 255.0) / nrm).float().contiguous()
    cc = w16[:, :F].sum(dim=1, dtype=torch.float32) * (255.0 / 256.0)
    cc[2 * H:3 * H] -= 1.0
    cc = cc.contiguous()

    def run(int_form, plan=None):
        src = rows6 if int_form else rows5
        S = torch.zeros((M, 2 * H), dtype=torch.float32, device=DEV)
        inp, lens_run, Mrun, rs_run = src, ln, M, rs
        if plan is not None:
            live = plan.rows[0]
            inp = torch.zeros((T, plan.P, src.shape[-1]), dtype=torch.float16, device=DEV)
            inp[:, :live] = src[:, plan.inv[:live].long()]
            rs_run = torch.zeros((T, plan.P), dtype=torch.float32, device=DEV)
            rs_run[:, :live] = rs[:, plan.inv[:live].long()]
            lens_run, Mrun = plan.lens, plan.P
        h16 = torch.full((T + 1, Mrun, 2 * H), float("nan"), dtype=torch.float16, device=DEV)
        hbf = torch.full((T + 1, Mrun, H), float("nan"), dtype=torch.bfloat16, device=DEV)
        if int_form:
            ops.lstm_layer_fwd_f16_fp8lo(inp, 3 * F // 2, F, 2 * F, F, w16, w8, bd, lens_run, T, Mrun, H, h16, hbf, S[:, :H], S[:, H:], 2 * H, plan=plan,
                                         h_lo=True, x_int=(rs_run, cc), b8_gap=F)
        else:
            ops.lstm_layer_fwd_f16_fp8lo(inp, 2 * F, F, 2 * F, 2 * F, w16, w8, bd, lens_run, T, Mrun, H, h16, hbf, S[:, :H], S[:, H:], 2 * H, plan=plan, h_lo=True)
        return S.cpu().double().numpy()
    e_f32 = np.abs(run(False) - s_ref).max()
    got = run(True)
    e_int = np.abs(got - s_ref).max()
    plan = ops.RowPlan(ln, lens, T)
    assert np.abs(run(True, plan) - got).max() < 1e-6
    print("layer 0 on integer frames: state err %.2e (f32-input form with the e4m3 x_lo correction: %.2e)" % (e_int, e_f32))
    assert np.isfinite(got).all() and np.all(got[0] == 0)
    assert e_int < 1.5e-4 and e_int <= e_f32 * 1.05, (e_int, e_f32)


def test_f16_dither_images_equal_the_oracle_bit_for_bit(ops):
    """evc_cast_f32_to_f16_dither against oracle/lowprec.py::f16_dither_images: every bit of every image - values over eleven decades (f16
    subnormals and values that underflow f16 among them), exact f16 values, zeros of both signs, a strided image stack, T = 1."""
    from oracle import lowprec as lp
    rng = np.random.default_rng(23)
    w = (rng.standard_normal((260, 384)) * np.logspace(-9, 1, 384)[None, :]).astype(np.float32)
    w[3, :10] = [0.0, -0.0, 1.0, -1.0, 2.0 ** -24, -2.0 ** -24, 3e-8, -3e-8, 6.1e-5, 65000.0]
    wd = torch.from_numpy(w).to(DEV)
    for T, seed in ((15, 1), (1, 9), (6, 4)):
        out = torch.full((T,) + w.shape, float("nan"), dtype=torch.float16, device=DEV)
        ops.cast_f16_dither(wd, out, seed)
        ref = lp.f16_dither_images(w, T, seed)
        got = out.cpu().numpy()
        assert np.array_equal(got.view(np.uint16), ref.view(np.uint16)), (T, seed, int((got.view(np.uint16) != ref.view(np.uint16)).sum()))
    pad = torch.full((4, w.size + 64), float("nan"), dtype=torch.float16, device=DEV)      # images 8 rows apart: the pad stays untouched
    ops._lib.call("evc_cast_f32_to_f16_dither", wd.data_ptr(), w.size, 4, pad.stride(0), 3, pad.data_ptr(), 0, 0, ops._stream())
    got = pad.cpu().numpy()
    assert np.array_equal(got[:, :w.size].reshape((4,) + w.shape).view(np.uint16), lp.f16_dither_images(w, 4, 3).view(np.uint16))
    assert np.isnan(got[:, w.size:].astype(np.float32)).all()
    # only the columns from col0 on dithered (a kernel whose input block keeps its correction): the others are the round-to-nearest image in every step
    out = torch.full((5,) + w.shape, float("nan"), dtype=torch.float16, device=DEV)
    ops.cast_f16_dither(wd, out, 2, col0=128)
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint16), lp.f16_dither_images(w, 5, 2, col0=128).view(np.uint16))
    assert np.array_equal(got[:, :, :128].view(np.uint16), np.broadcast_to(w.astype(np.float16)[None, :, :128], (5, 260, 128)).view(np.uint16))


@pytest.mark.parametrize("M,T,Kin,H,tile", [(512, 4, 384, 384, 0), (1100, 15, 1152, 512, 0), (700, 5, 384, 384, 6), (390, 3, 512, 384, 7), (730, 6, 384, 384, 11)])
def test_lstm_layer_fwd_f16_on_time_dithered_weight_images(M, T, Kin, H, tile):
    """evc_lstm_layer_fwd_f16_dith, two stacked layers: layer 0 on input rows [f16(x) | e4m3(x 2^7) | e4m3(x_lo 2^18)] - f16 stages on image t of
    evc_cast_f32_to_f16_dither + the e4m3 stages of the input's low-order half against the e4m3(Wx 2^6) block of evc_cast_f32_to_fp8_lo's rows -
    layer 1 on layer 0's PLAIN f16 h rows and its own images (kx8 = 0).  Against (a) a float64 step-by-step restatement with the SAME per-step
    images (oracle/lowprec.py::f16_dither_images), f16-rounded h operands and the e4m3 correction: what is left is the f32 accumulation and
    f16 ties of h (1.5e-4; the same restatement on images one step late must be farther); (b) the float64 oracle on the exact weights: within the f16 bound (8e-4).  Ring tiles forced in a child process,
    rows that end early, a row plan, one image for every step (stride 0) = the plain f16 layer bit for bit."""
    code = _DITH_CHILD % dict(M=M, T=T, Kin=Kin, H=H)
    env = dict(os.environ)
    if tile:
        env["EVC_FORCE_TILE"] = str(tile)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout.strip().splitlines()[-1])


_DITH_CHILD = r"""
import numpy as np, torch
from oracle import model_math as mm
from oracle import lowprec as lp
from efficientvideoclassification_youtube8m_amd import ops
DEV = "cuda:0"
M, T, Kin, H = %(M)d, %(T)d, %(Kin)d, %(H)d
rng = np.random.default_rng(M + T + Kin + H + 5)
x = (rng.standard_normal((M, T, Kin)) * 0.05).astype(np.float32)
x /= np.maximum(1.0, np.abs(x).max())
gain = 3.0 if T <= 6 else 1.0      # (long chains on amplifying weights turn one f16 tie of h into 1e-3 on the final state: the comparison with the restatement would measure that)
k0 = (mm.glorot_uniform(rng, (Kin + H, 4 * H)) * gain).astype(np.float32)
k1 = (mm.glorot_uniform(rng, (2 * H, 4 * H)) * gain).astype(np.float32)
b0 = (rng.standard_normal(4 * H) * 0.1).astype(np.float32)
b1 = (rng.standard_normal(4 * H) * 0.1).astype(np.float32)
lens = rng.integers(0, T + 1, size=M).astype(np.int32)
lens[:3] = [0, T, 1]
s_ref, _ = mm.multi_rnn_seq_fwd(x.astype(np.float64), lens, [(k0.astype(np.float64), b0.astype(np.float64)), (k1.astype(np.float64), b1.astype(np.float64))])
sig = lambda v: 1.0 / (1.0 + np.exp(-v))
f16r = lp.f16_round
def emulate(images):
    # float64 restatement of what the two launches contract: per step image t of each kernel ([4H][C] layout -> TF layout), f16 operands, layer 0's e4m3 term
    inp = x.astype(np.float64)
    state = []
    for l, (k, b) in enumerate(((k0, b0), (k1, b1))):
        nin = k.shape[0] - H
        c, h = np.zeros((M, H)), np.zeros((M, H))
        outs = np.zeros((M, T, H))
        w8 = lp.e4m3_round(k[:nin].astype(np.float64) * 2.0 ** ops.FP8_WX_HI_EXP) if l == 0 else None
        for t in range(T):
            wt = images[l][t].astype(np.float64).T                       # [C][4H]
            xt = inp[:, t]
            z = f16r(xt) @ wt[:nin] + f16r(h) @ wt[nin:] + b
            if l == 0:
                z = z + (lp.e4m3_round((xt - f16r(xt)) * 2.0 ** 18) @ w8) * 2.0 ** -(18 + ops.FP8_WX_HI_EXP)
            i, j, f, o = np.split(z, 4, axis=1)
            cn = c * sig(f + 1.0) + sig(i) * np.tanh(j)
            hn = np.tanh(cn) * sig(o)
            act = (lens > t)[:, None]
            c, h = np.where(act, cn, c), np.where(act, hn, h)
            outs[:, t] = np.where(act, hn, 0.0)
        inp = outs
        state += [c, h]
    return np.concatenate(state, 1)
xt = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2))).to(DEV)
rows = torch.zeros((T, M, 2 * Kin), dtype=torch.float16, device=DEV)
hi = xt.half()
rows[:, :, :Kin] = hi
rows[:, :, Kin:3 * Kin // 2] = (xt * 128.0).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.float16)
rows[:, :, 3 * Kin // 2:] = ((xt - hi.float()) * 2.0 ** 18).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.float16)
ln = torch.from_numpy(lens).to(DEV)
kTs = [torch.from_numpy(np.ascontiguousarray(k.T)).to(DEV) for k in (k0, k1)]
def run(plan, n_img):
    S = torch.full((M, 4 * H), float("nan"), dtype=torch.float32, device=DEV)
    inp, ldx, kx16, x8_off, kx8 = rows, 2 * Kin, Kin, 3 * Kin, Kin
    lens_run, Mrun = ln, M
    if plan is not None:
        live = plan.rows[0]
        inp = torch.zeros((T, plan.P, 2 * Kin), dtype=torch.float16, device=DEV)
        inp[:, :live] = rows[:, plan.inv[:live].long()]
        lens_run, Mrun = plan.lens, plan.P
        S.zero_()
    imgs = []
    for l, (k, b) in enumerate(((k0, b0), (k1, b1))):
        kT = kTs[l]
        nin = k.shape[0] - H
        w16 = torch.empty((n_img, 4 * H, nin + H), dtype=torch.float16, device=DEV)
        if n_img == 1:
            ops.cast_f16(kT, w16[0])
        else:
            ops.cast_f16_dither(kT, w16, 3 + l)
        imgs.append(w16)
        w8 = None
        if l == 0:
            w8full = torch.empty((4 * H, nin + H + nin), dtype=torch.uint8, device=DEV)
            ops.cast_fp8_lo(kT, w8full, hi_cols=nin)
            w8 = w8full[:, nin:2 * nin]
        h16 = torch.full((T + 1, Mrun, H), float("nan"), dtype=torch.float16, device=DEV)
        hbf = torch.full((T + 1, Mrun, H), float("nan"), dtype=torch.bfloat16, device=DEV)
        ops.lstm_layer_fwd_f16_dith(inp, ldx, kx16, x8_off, kx8, w16, w8, w8full.stride(0) if l == 0 else 0, 18 + ops.FP8_WX_HI_EXP,
                                    torch.from_numpy(b).to(DEV), lens_run, T, Mrun, H, h16, hbf, S[:, 2 * l * H:], S[:, (2 * l + 1) * H:], 4 * H, plan=plan)
        if plan is None:
            assert float((h16.float() - hbf.float()).abs().max()) <= 2.0 ** -8
        inp, ldx, kx16, x8_off, kx8 = h16[1:], H, H, 0, 0
    return S.cpu().double().numpy(), imgs
got, imgs = run(None, T)
assert np.isfinite(got).all() and np.all(got[0] == 0)
want = emulate([im.cpu().numpy() for im in imgs])
d_emu = float(np.max(np.abs(got - want)))
err = float(np.max(np.abs(got - s_ref)))
gp, _ = run(ops.RowPlan(ln, lens, T), T)
assert float(np.max(np.abs(gp - got))) < 1e-6
# one image for every step: the round-to-nearest f16 image = layer 0 with its e4m3 input term, layer 1 the plain f16 layer
g1, im1 = run(None, 1)
w1 = emulate([np.repeat(im.cpu().numpy(), T, 0) for im in im1])
d1 = float(np.max(np.abs(g1 - w1)))
# the restatement on the WRONG images (every layer's images one step late) must be the farther one: step t really contracts image t
d_late = float(np.max(np.abs(got - emulate([np.roll(im.cpu().numpy(), 1, 0) for im in imgs]))))
print("dithered two-layer stack M=%%d T=%%d Kin=%%d H=%%d: vs the restatement on the same images %%.2e (images one step late: %%.2e; one image: %%.2e), vs the exact-weight oracle %%.2e" %% (M, T, Kin, H, d_emu, d_late, d1, err))
assert d_emu < 1.5e-4 and d1 < 1.5e-4 and d_emu < d_late, (d_emu, d1, d_late)
assert err < 8e-4, err
"""


@pytest.mark.parametrize("M,T,Kin,H", [(256, 6, 64, 64), (1536, 4, 192, 256), (640, 15, 128, 128)])
def test_lstm_layer_fwd_f16_recurrent_weights_extended(ops, M, T, Kin, H):
    """evc_lstm_layer_fwd_f16 with h_wide = 1: the recurrent weights K-extended by their low-order halves - h rows [f16(h) |
    f16(h)/64] against kernel rows [f16(Wx) | f16(Wh) | (Wh - f16(Wh))*64] (evc_cast_f32_to_f16_wide, h_ext) - next to the plain f16
    layer on the same f32 kernel, both against the float64 oracle with the x-part f16-rounded and the h-part EXACT: the extended
    layer must be the closer one and within the f16 activation bound; its wide image must be [h | h/64]; a strided x (ldx > Kin)
    reads the same rows."""
    rng = np.random.default_rng(M + T + Kin + H + 11)
    f16r = lambda a: torch.from_numpy(np.asarray(a, np.float32)).half().double().numpy()
    x = f16r(rng.standard_normal((M, T, Kin)) * 0.5)
    kernel = (mm.glorot_uniform(rng, (Kin + H, 4 * H)) * 3.0).astype(np.float32)
    k_ref = kernel.astype(np.float64).copy()
    k_ref[:Kin] = f16r(kernel[:Kin])
    bias = (rng.standard_normal(4 * H) * 0.1).astype(np.float32)
    lens = rng.integers(0, T + 1, size=M).astype(np.int32)
    lens[:3] = [0, T, 1]
    s_ref, _ = mm.multi_rnn_seq_fwd(x, lens, [(k_ref, bias.astype(np.float64))])
    # x with a row stride of Kin + 64 (as a wide h image of a layer below would have)
    xs = torch.zeros((T, M, Kin + 64), dtype=torch.float16, device=DEV)
    xs[:, :, :Kin] = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2)).astype(np.float32)).half().to(DEV)
    kT = torch.from_numpy(np.ascontiguousarray(kernel.T)).to(DEV)
    b, ln = torch.from_numpy(bias).to(DEV), torch.from_numpy(lens).to(DEV)
    errs = {}
    for wide in (True, False):
        w = torch.empty((4 * H, Kin + (2 if wide else 1) * H), dtype=torch.float16, device=DEV)
        ops.cast_f16_wide(kT, Kin, H, 1, w, h_ext=wide)
        h16 = torch.full((T + 1, M, (2 if wide else 1) * H), float("nan"), dtype=torch.float16, device=DEV)
        hbf = torch.full((T + 1, M, H), float("nan"), dtype=torch.bfloat16, device=DEV)
        S = torch.full((M, 2 * H), float("nan"), dtype=torch.float32, device=DEV)
        ops.lstm_layer_fwd_f16(xs, w, b, ln, T, M, Kin, H, h16, hbf, S[:, :H], S[:, H:], 2 * H, ldx=Kin + 64, h_wide=wide)
        got = S.cpu().double().numpy()
        assert np.isfinite(got).all() and np.all(got[0] == 0)
        errs[wide] = float(np.max(np.abs(got - s_ref)))
        hn = h16.float().cpu().numpy()
        assert np.max(np.abs(hn[:, :, :H] - hbf.float().cpu().numpy())) <= 2.0 ** -8
        if wide:
            assert np.max(np.abs(hn[:, :, H:] * 64.0 - hn[:, :, :H])) <= 64 * 2.0 ** -25
            hi = kT.half()
            assert torch.equal(w[:, :Kin + H], hi) and torch.equal(w[:, Kin + H:], ((kT[:, Kin:] - hi[:, Kin:].float()) * 64.0).half())
    print("f16 layer, exact-Wh oracle: state err with the recurrent weights extended %.2e, plain f16 %.2e" % (errs[True], errs[False]))
    assert errs[True] < 8e-4 and errs[True] <= errs[False] * 1.05


@pytest.mark.parametrize("M,T,Kin,H", [(256, 5, 128, 64), (70, 6, 64, 128), (512, 3, 256, 128), (1200, 2, 64, 64)])
def test_lstm_stack2_wavefront_fwd(ops, M, T, Kin, H):
    """evc_lstm_stack2_fwd (layer 0 step t+1 and layer 1 step t in one launch) against the float64 oracle's 2-layer
    MultiRNNCell and against two evc_lstm_layer_fwd calls: layer 0 bit-identical, layer 1 equal up to the rounding of
    the hoisted vs fused x-projection."""
    rng = np.random.default_rng(M + T + Kin + H)
    x = bf16_round(rng.standard_normal((M, T, Kin)) * 0.5)
    k0 = bf16_round(mm.glorot_uniform(rng, (Kin + H, 4 * H)) * 2.0)
    k1 = bf16_round(mm.glorot_uniform(rng, (2 * H, 4 * H)) * 2.0)
    b0 = (rng.standard_normal(4 * H) * 0.1).astype(np.float32).astype(np.float64)
    b1 = (rng.standard_normal(4 * H) * 0.1).astype(np.float32).astype(np.float64)
    lens = rng.integers(0, T + 1, size=M).astype(np.int32)
    lens[:3] = [0, T, 1]
    s_ref, _ = mm.multi_rnn_seq_fwd(x, lens, [(k0, b0), (k1, b1)])
    xt = to_bf16(np.ascontiguousarray(x.transpose(1, 0, 2)))
    w0, w1 = to_bf16(np.ascontiguousarray(k0.T)), to_bf16(np.ascontiguousarray(k1.T))
    bb0, bb1 = (torch.from_numpy(b.astype(np.float32)).to(DEV) for b in (b0, b1))
    ln = torch.from_numpy(lens).to(DEV)

    def bufs():
        hb = [torch.full((T + 1, M, H), float("nan"), dtype=torch.bfloat16, device=DEV) for _ in range(2)]
        S = torch.full((M, 4 * H), float("nan"), dtype=torch.float32, device=DEV)
        g = [torch.zeros((T, M, H, 2), dtype=torch.int32, device=DEV) for _ in range(2)]
        c = [torch.full((T + 1, M, H), float("nan"), dtype=torch.bfloat16, device=DEV) for _ in range(2)]
        return hb, S, g, c

    zx = torch.empty((T * M, 4 * H), dtype=torch.float32, device=DEV)
    hb, S, g, c = bufs()
    ops.lstm_stack2_fwd(xt, w0, bb0, w1, bb1, ln, T, M, Kin, H, zx, hb[0], hb[1], S, g, c)
    got = S.cpu().double().numpy()
    assert np.isfinite(got).all()
    assert np.max(np.abs(got - s_ref)) < 8e-3, np.max(np.abs(got - s_ref))
    assert np.all(got[0] == 0)
    # the same stack, one layer after the other
    hb2, S2, g2, c2 = bufs()
    ops.lstm_layer_fwd(xt, w0, bb0, ln, T, M, Kin, H, hb2[0], S2[:, :H], S2[:, H:], 4 * H, g2[0], c2[0], hoist=True, zx_ws=zx)
    ops.lstm_layer_fwd(hb2[0][1:], w1, bb1, ln, T, M, H, H, hb2[1], S2[:, 2 * H:], S2[:, 3 * H:], 4 * H, g2[1], c2[1], hoist=True, zx_ws=zx)
    assert torch.equal(hb[0], hb2[0]) and torch.equal(S[:, :2 * H], S2[:, :2 * H]) and torch.equal(g[0], g2[0])
    assert torch.equal(torch.nan_to_num(c[0][1:].float()), torch.nan_to_num(c2[0][1:].float()))   # rows past their length are not written
    assert (S[:, 2 * H:] - S2[:, 2 * H:]).abs().max().item() < 4e-3
    assert (hb[1].float() - hb2[1].float()).abs().max().item() < 2e-2      # a bf16 ulp or two of values up to 1
    for t in range(T):
        assert bool((hb[1][t + 1][ln <= t] == 0).all())
    # inference form: no tape
    hb3, S3, _, _ = bufs()
    ops.lstm_stack2_fwd(xt, w0, bb0, w1, bb1, ln, T, M, Kin, H, zx, hb3[0], hb3[1], S3)
    assert torch.equal(S3, S)


def _bwd_ref(x, lens, kernel, bias, dS, dh_above):
    """Oracle BPTT with an upper-layer gradient on the per-step outputs: emulate
    the upper layer by a 2-layer stack is overkill, so extend the oracle's
    single-layer BPTT by injecting dh_above where the step is active."""
    layers = [(kernel, bias)]
    _, cache = mm.multi_rnn_seq_fwd(x, lens, layers)
    steps, lengths, xshape, H = cache
    M, T, F = xshape
    dc = dS[:, :H].copy()
    dh = dS[:, H:].copy()
    dK = np.zeros_like(kernel)
    db = np.zeros_like(bias)
    dx = np.zeros((M, T, F))
    for t in range(T - 1, -1, -1):
        act = (t < lengths)[:, None].astype(np.float64)
        inp, h_prev, c_prev, (i, j, f, o, tc) = steps[t][0]
        dh_new = act * (dh + dh_above[t])
        dc_new = act * dc + dh_new * o * (1 - tc * tc)
        dz = np.concatenate([dc_new * j * i * (1 - i), dc_new * i * (1 - j * j), dc_new * c_prev * f * (1 - f),
                             dh_new * tc * o * (1 - o)], axis=1)
        xin = np.concatenate([inp, h_prev], axis=1)
        dK += xin.T @ dz
        db += dz.sum(0)
        dxin = dz @ kernel.T
        dx[:, t] = dxin[:, :F]
        dh = (1 - act) * dh + dxin[:, F:]
        dc = (1 - act) * dc + dc_new * f
    return dx, [(dK, db)]


def test_l2norm_chunk_and_counts(ops):
    rng = np.random.default_rng(5)
    B, T, F = 6, 300, 1152
    q, x, n, _ = mm.synthetic_batch(B, seed=3, dtype=np.float32)
    xr = torch.from_numpy(x).to(DEV)
    o1, o2 = ops.l2norm_chunk(xr, 20, every_n=10, num_chunks_student=5)
    ref = mm.l2_normalize(x.astype(np.float64), 2)
    # teacher view [15][20*B][F], row m = chunk*B + b
    r1 = ref.reshape(B, 20, 15, F).transpose(2, 1, 0, 3).reshape(15, 20 * B, F)
    assert np.max(np.abs(o1.float().cpu().numpy() - r1)) < 2 ** -8 * np.abs(r1).max()
    rs = mm.subsample_frames(ref, 10)
    r2 = rs.reshape(B, 5, 6, F).transpose(2, 1, 0, 3).reshape(6, 5 * B, F)
    assert np.max(np.abs(o2.float().cpu().numpy() - r2)) < 2 ** -8 * np.abs(r2).max()
    # the student rows are bit-identical copies of the teacher's rows for frames 0,10,20,...
    t1 = o1.reshape(15, 20, B, F)
    for s in range(30):
        fr = s * 10
        assert torch.equal(o2.reshape(6, 5, B, F)[s % 6, s // 6], t1[fr % 15, fr // 15])
    # uint8 input path: dequantise + zero padding + normalise
    qd = torch.from_numpy(q).to(DEV)
    nd = torch.from_numpy(n).to(DEV)
    u1, _ = ops.l2norm_chunk(qd, 20, num_frames=nd)
    # (dequantisation may contract to an FMA on the device: allow one bf16 ulp)
    d_max = (u1.float() - o1.float()).abs().max().item()
    o_max = o1.float().abs().max().item()
    frac = (u1 != o1).float().mean().item()
    assert d_max <= 2 ** -7 * o_max and frac < 0.01, (d_max, o_max, frac)
    # integer part: bit-exact
    from efficientvideoclassification_youtube8m_amd.distill import validate_every_n
    admissible = [e for e in range(1, 301) if not _raises(validate_every_n, e)]
    assert admissible == [1, 2, 3, 4, 5, 6, 10, 12, 15, 20, 30, 60]        # every every_n the reference's graph builds for
    for every_n in admissible:                                             # ... each for EVERY frame count 0..300, device and host twin
        nn = torch.arange(0, 301, dtype=torch.int32, device=DEV)
        S = 300 // every_n
        C = 20 if every_n == 1 else 5
        Lc = S // C if S % C == 0 else 1
        n_used, l1, l2 = ops.frame_counts(nn, every_n, C, Lc)
        ref_n = mm.student_num_frames(np.arange(301), every_n) if every_n > 1 else np.arange(301)
        # the reference's expression itself (cs/train.py:270-272: tf.cast(tf.cast(n, float64) / 300 * int(300 / every_n), int64)), in numpy
        lit = (np.arange(301).astype(np.float64) / 300.0 * int(300 / every_n)).astype(np.int64)
        if every_n > 1:
            assert np.array_equal(ref_n, lit)
        assert np.array_equal(n_used.cpu().numpy(), ref_n)
        rl1, rl2 = mm.hlstm_chunk_lengths(ref_n, C, Lc)
        assert np.array_equal(l1.cpu().numpy().reshape(C, 301), rl1.T)
        assert np.array_equal(l2.cpu().numpy(), rl2)
        hn, hl1, hl2 = ops.host_frame_counts(np.arange(301), every_n, C, Lc)
        assert np.array_equal(hn, ref_n) and np.array_equal(np.asarray(hl1).reshape(C, 301), rl1.T) and np.array_equal(hl2, rl2)
        if every_n > 1:                                                    # the student's call (subsampled formula on device and host)
            ns, _, _ = ops.frame_counts(nn, every_n, C, Lc, 300, subsampled=True)
            assert np.array_equal(ns.cpu().numpy(), lit)
            assert np.array_equal(ops.host_frame_counts(np.arange(301), every_n, C, Lc, 300, subsampled=True)[0], lit)
    # the student input at every_n = 1 (the reference's default) still goes through float64 (n/300)*300: n-1 for some n
    nn = torch.arange(0, 301, dtype=torch.int32, device=DEV)
    n_used, l1, l2 = ops.frame_counts(nn, 1, 5, 60, subsampled=True)
    ref_n = mm.student_num_frames(np.arange(301), 1)
    assert (ref_n != np.arange(301)).sum() == 12 and ref_n[55] == 54
    assert np.array_equal(n_used.cpu().numpy(), ref_n)
    assert np.array_equal(ops.host_frame_counts(np.arange(301), 1, 5, 60, subsampled=True)[0], ref_n)
    rl1, rl2 = mm.hlstm_chunk_lengths(ref_n, 5, 60)
    assert np.array_equal(l1.cpu().numpy().reshape(5, 301), rl1.T) and np.array_equal(l2.cpu().numpy(), rl2)


@pytest.mark.parametrize("R,C,S", [(48, 70, 8), (1920, 256, 30)])
def test_batchnorm_relu6_pool_kernels(ops, R, C, S):
    """slim.batch_norm training statistics / apply / backward, relu6 and the fused max-pool
    routing, each against the oracle in f32-level tolerance (no bf16 in these kernels)."""
    rng = np.random.default_rng(R + C)
    B = R // S
    x = (rng.standard_normal((R, C)) * 2 + 0.5).astype(np.float32)
    gamma = (1 + 0.3 * rng.standard_normal(C)).astype(np.float32)
    beta = (0.5 * rng.standard_normal(C) + 1.0).astype(np.float32)
    xd, gd, bd = (torch.from_numpy(a).to(DEV) for a in (x, gamma, beta))
    ws = torch.empty(2 * C, dtype=torch.float64, device=DEV)
    mean = torch.empty(C, dtype=torch.float32, device=DEV)
    var = torch.empty(C, dtype=torch.float32, device=DEV)
    ops.bn_stats(xd, R, C, ws, mean, var)
    x64 = x.astype(np.float64)
    assert np.allclose(mean.cpu().numpy(), x64.mean(0), rtol=1e-5, atol=1e-6)
    assert np.allclose(var.cpu().numpy(), x64.var(0), rtol=1e-5, atol=1e-6)
    y_ref, cache = mm.batch_norm_train_fwd(x64, gamma.astype(np.float64), beta.astype(np.float64))
    y = torch.empty((R, C), dtype=torch.float32, device=DEV)
    ops.bn_apply(xd, R, C, mean, var, gd, bd, False, y_f32=y)
    assert np.abs(y.cpu().numpy() - y_ref).max() < 1e-4
    # plain BN backward
    dy = rng.standard_normal((R, C)).astype(np.float32)
    dyd = torch.from_numpy(dy).to(DEV)
    dx_ref, dg_ref, db_ref = mm.batch_norm_train_bwd(dy.astype(np.float64), cache)
    dx = torch.empty((R, C), dtype=torch.float32, device=DEV)
    dg = torch.empty(C, dtype=torch.float32, device=DEV)
    db = torch.empty(C, dtype=torch.float32, device=DEV)
    ops.bn_bwd_partial(xd, dyd, R, C, mean, var, gd, bd, False, ws)
    ops.bn_bwd_finalize(xd, dyd, R, R, C, mean, var, gd, bd, False, ws, dx_f32=dx, dgamma=dg, dbeta=db)
    assert np.abs(dx.cpu().numpy() - dx_ref).max() < 1e-4 * max(1.0, np.abs(dx_ref).max())
    assert np.allclose(dg.cpu().numpy(), dg_ref, rtol=1e-4, atol=1e-4)
    assert np.allclose(db.cpu().numpy(), db_ref, rtol=1e-4, atol=1e-4)
    # relu6 + max-pool forward, then routed backward; masks taken from the oracle's own y
    a6 = mm.relu6(y_ref).reshape(B, S, C)
    pooled = torch.empty((B, C), dtype=torch.float32, device=DEV)
    am = torch.empty((B, C), dtype=torch.int32, device=DEV)
    ops.bn_relu6_framepool_fwd(xd, B, S, C, mean, var, gd, bd, pooled, None, am)
    assert np.abs(pooled.cpu().numpy() - a6.max(1)).max() < 1e-4
    amr = a6.argmax(1)
    safe = np.sort(a6, axis=1)[:, -1] - np.sort(a6, axis=1)[:, -2] > 1e-3        # unambiguous maxima
    assert np.array_equal(am.cpu().numpy()[safe], amr[safe])
    dpool = rng.standard_normal((B, C)).astype(np.float32)
    da = np.zeros((B, S, C))
    amg = am.cpu().numpy()
    bi, ci = np.meshgrid(np.arange(B), np.arange(C), indexing="ij")
    da[bi, amg, ci] = dpool
    inside = (y_ref > 1e-3) & (y_ref < 6 - 1e-3)
    edge = ~inside & ~((y_ref < -1e-3) | (y_ref > 6 + 1e-3))
    dyb = da.reshape(R, C) * inside
    dx_ref, dg_ref, db_ref = mm.batch_norm_train_bwd(dyb, cache)
    ops.bn_bwd_partial(xd, torch.from_numpy(dpool).to(DEV), R, C, mean, var, gd, bd, True, ws, argmax=am, S=S)
    ops.bn_bwd_finalize(xd, torch.from_numpy(dpool).to(DEV), R, R, C, mean, var, gd, bd, True, ws, argmax=am, S=S,
                        dx_f32=dx, dgamma=dg, dbeta=db)
    cols_ok = ~(edge & (da.reshape(R, C) != 0)).any(0)                               # columns with no boundary-valued routed entry
    assert cols_ok.mean() > 0.9
    assert np.abs(dx.cpu().numpy() - dx_ref)[:, cols_ok].max() < 1e-4 * max(1.0, np.abs(dx_ref).max())
    assert np.allclose(dg.cpu().numpy()[cols_ok], dg_ref[cols_ok], rtol=1e-4, atol=1e-4)
    assert np.allclose(db.cpu().numpy()[cols_ok], db_ref[cols_ok], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("M,N,K,il", [(256, 256, 64, 0), (512, 264, 160, 0), (1024, 1152, 4096, 0), (4096, 1152, 10240, 1024),
                                      (264, 8, 32, 0), (512, 1024, 8192, 128)])
def test_gemm_tn_and_colsum(ops, M, N, K, il):
    """C = A^T B with both operands row-major over K (ds_read_b64_tr_b16 transpose reads), incl.
    split-K atomics (long K), ragged M/N tiles and the gate de-interleaving row map."""
    rng = np.random.default_rng(M + N + K)
    A = bf16_round(rng.standard_normal((K, M)) * 0.5)
    B = bf16_round(rng.standard_normal((K, N)) * 0.5)
    ref = A.T @ B
    if il:
        H = M // 4
        ref = ref.reshape(H, 4, N).transpose(1, 0, 2).reshape(M, N)       # row u*4+g -> g*H+u
    out = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
    ops.gemm_tn(to_bf16(A), to_bf16(B), M, N, K, out, row_interleave_H=(M // 4 if il else 0))
    got = out.cpu().double().numpy()
    scale = (np.abs(A.T) @ np.abs(B)).max() + 1.0
    assert np.isfinite(got).all()
    assert np.max(np.abs(got - ref)) / scale < 3e-6
    ops.gemm_tn(to_bf16(A), to_bf16(B), M, N, K, out, row_interleave_H=(M // 4 if il else 0), accumulate=True)
    assert np.max(np.abs(out.cpu().double().numpy() - 2 * ref)) / scale < 6e-6
    cs = torch.empty(M, dtype=torch.float32, device=DEV)
    ops.colsum_bf16(to_bf16(A), K, M, cs, deinterleave_H=(M // 4 if il else 0))
    cref = A.sum(0)
    if il:
        cref = cref.reshape(M // 4, 4).T.reshape(M)
    assert np.max(np.abs(cs.cpu().double().numpy() - cref)) < 1e-3 * (np.abs(A).sum(0).max() + 1)


@pytest.mark.parametrize("M,N1,N2,P,rows,il", [
    (1024, 256, 256, 512, [500, 470, 470, 300, 33, 1], 256),                 # two column segments, split K, partial last steps
    (4096, 1024, 1024, 3776, [3700, 3650, 3600, 3590, 3580, 3570, 3560, 3550, 3540, 3530, 3520, 3510, 3500, 3490, 3460], 1024),   # the teacher's L1 shape
    (512, 128, 0, 1024, [1000, 0, 900, 0, 0, 64, 32], 0),                    # one segment, narrow strip, empty slabs
    (512, 384, 0, 256, [256, 250, 31], 0),                                    # short contraction (128 x 128 tiles, no split)
    (1024, 256, 256, 64, [64] * 4, 0),                                        # nothing dead: the plain walk
    (512, 256, 0, 96, [90] * 17 + [40], 0),                                   # more than 16 non-empty slabs: the plain walk over every row
])
def test_gemm_tn_over_time_slabs_skips_the_dead_rows(ops, M, N1, N2, P, rows, il):
    """evc_gemm_tn2_rows (ops.gemm_tn / gemm_tn2 with live_rows): K = T slabs of P rows of which the first rows[t] are live - the weight-gradient
    products of a row-planned LSTM level.  The dead rows of A are zeros (what the BPTT steps leave), the dead rows of B are finite garbage: the
    product must equal the reference over the live rows (plain, accumulate), i.e. the full-K product, whether the walk skips (<= 16 non-empty
    slabs) or not; rows between rows[t] and the next multiple of 32 are contracted (A is zero there)."""
    T = len(rows)
    K = T * P
    rng = np.random.default_rng(M + N1 + N2 + P + T)
    A = bf16_round(rng.standard_normal((K, M)) * 0.5)
    live = np.zeros(K, bool)
    for t, r in enumerate(rows):
        live[t * P:t * P + r] = True
    A[~live] = 0.0
    Bs = [bf16_round(rng.standard_normal((K, n)) * 0.5) for n in (N1, N2) if n]
    for b in Bs:
        b[~live] = bf16_round(rng.standard_normal(((~live).sum(), b.shape[1])) * 100.0)      # garbage where A is zero
    ref = np.concatenate([A.T @ b for b in Bs], axis=1)
    if il:
        ref = ref.reshape(M // 4, 4, N1 + N2).transpose(1, 0, 2).reshape(M, N1 + N2)
    scale = (np.abs(A.T) @ np.abs(np.concatenate(Bs, axis=1))).max() + 1.0
    out = torch.full((M, N1 + N2), float("nan"), dtype=torch.float32, device=DEV)
    a = to_bf16(A)
    bs = [to_bf16(b) for b in Bs]
    def run(acc):
        if N2:
            ops.gemm_tn2(a, bs[0], N1, bs[1], N2, M, K, out, row_interleave_H=il, accumulate=acc, live_rows=(rows, P))
        else:
            ops.gemm_tn(a, bs[0], M, N1, K, out, row_interleave_H=il, accumulate=acc, live_rows=(rows, P))
    run(False)
    got = out.cpu().double().numpy()
    assert np.isfinite(got).all()
    assert np.max(np.abs(got - ref)) / scale < 3e-6, np.max(np.abs(got - ref)) / scale
    run(True)
    assert np.max(np.abs(out.cpu().double().numpy() - 2 * ref)) / scale < 6e-6
    with pytest.raises(Exception):                                            # slab_rows must be a multiple of 32 and K = T slabs
        ops.gemm_tn(a, bs[0], M, N1, K, out, live_rows=(rows, P + 1))


@pytest.mark.parametrize("M,N1,N2,K,il", [(512, 256, 256, 64, 0), (1024, 256, 264, 2560, 256), (4096, 1024, 1024, 8192, 1024),
                                           (1024, 512, 128, 1024, 0)])
def test_gemm_tn2_two_column_segments(ops, M, N1, N2, K, il):
    """evc_gemm_tn2: C[:, :N1] = A^T B1, C[:, N1:] = A^T B2 in one launch (the x- and h-part of a layer's weight gradient),
    plain / accumulate / split-K forms, ragged second segment, gate de-interleave; B1 and B2 with different row strides."""
    rng = np.random.default_rng(M + N1 + N2 + K)
    A = bf16_round(rng.standard_normal((K, M)) * 0.5)
    B1 = bf16_round(rng.standard_normal((K, N1 + 8)) * 0.5)[:, :N1]       # row stride N1 + 8
    B2 = bf16_round(rng.standard_normal((K, N2)) * 0.5)
    ref = np.concatenate([A.T @ B1, A.T @ B2], axis=1)
    if il:
        ref = ref.reshape(M // 4, 4, N1 + N2).transpose(1, 0, 2).reshape(M, N1 + N2)
    b1 = to_bf16(np.ascontiguousarray(bf16_round(np.concatenate([B1, np.zeros((K, 8))], axis=1))))[:, :N1]
    out = torch.full((M, N1 + N2), float("nan"), dtype=torch.float32, device=DEV)
    ops.gemm_tn2(to_bf16(A), b1, N1, to_bf16(B2), N2, M, K, out, row_interleave_H=il)
    got = out.cpu().double().numpy()
    scale = (np.abs(A.T) @ np.abs(np.concatenate([B1, B2], axis=1))).max() + 1.0
    assert np.isfinite(got).all()
    assert np.max(np.abs(got - ref)) / scale < 3e-6
    ops.gemm_tn2(to_bf16(A), b1, N1, to_bf16(B2), N2, M, K, out, row_interleave_H=il, accumulate=True)
    assert np.max(np.abs(out.cpu().double().numpy() - 2 * ref)) / scale < 6e-6
    with pytest.raises(Exception):                                       # the segment boundary must fall on a tile boundary
        ops.gemm_tn2(to_bf16(A), b1[:, :128], 128, to_bf16(B2), N2, M, K, out[:, :128 + N2])
    # segments that are not adjacent in C, the gap filled by a narrow strip product (engine._wgrad_tn: layer 0 of the L1 stacks)
    G = 128
    B3 = bf16_round(rng.standard_normal((K, G)) * 0.5)
    wide = torch.zeros((M, N1 + G + N2), dtype=torch.float32, device=DEV)
    ops.gemm_tn2(to_bf16(A), b1, N1, to_bf16(B2), N2, M, K, wide, row_interleave_H=il, accumulate=True, c_col2=N1 + G)
    ops.gemm_tn(to_bf16(A), to_bf16(B3), M, G, K, wide[:, N1:N1 + G], row_interleave_H=il, ldc=N1 + G + N2, accumulate=True)
    ref3 = A.T @ B3
    if il:
        ref3 = ref3.reshape(M // 4, 4, G).transpose(1, 0, 2).reshape(M, G)
    want = np.concatenate([ref[:, :N1], ref3, ref[:, N1:]], axis=1)
    assert np.max(np.abs(wide.cpu().double().numpy() - want)) / scale < 6e-6
    with pytest.raises(Exception):                                       # a gap needs accumulate
        ops.gemm_tn2(to_bf16(A), b1, N1, to_bf16(B2), N2, M, K, wide, c_col2=N1 + G)


@pytest.mark.parametrize("M,T", [(40, 15), (5120, 15), (1280, 6), (7000, 31)])
def test_sort_rows_and_host_counts(ops, M, T):
    """evc_sort_rows_by_len = numpy's stable argsort by descending length (integer work: exact)."""
    rng = np.random.default_rng(M + T)
    lens = rng.integers(0, T + 1, size=M).astype(np.int32)
    lens[rng.random(M) < 0.3] = 0
    ld = torch.from_numpy(lens).to(DEV)
    plan = ops.RowPlan(ld, lens, T)
    inv_ref = np.argsort(-lens.astype(np.int64), kind="stable")
    assert np.array_equal(plan.inv.cpu().numpy(), inv_ref)
    pos = plan.pos.cpu().numpy()
    assert np.array_equal(pos[inv_ref], np.arange(M)) and np.array_equal(plan.lens.cpu().numpy(), lens[inv_ref])
    assert plan.rows == [int((lens > t).sum()) for t in range(T)]
    assert plan.P == min(M, max(32, (plan.rows[0] + 31) // 32 * 32))
    # host twin of the frame-count kernel (bit-exact)
    n = rng.integers(0, 301, size=64).astype(np.int32)
    for every_n, C, Lc in ((1, 20, 15), (10, 5, 6), (6, 5, 10), (3, 5, 20)):
        got = ops.frame_counts(torch.from_numpy(n).to(DEV), every_n, C, Lc)
        ref = ops.host_frame_counts(n, every_n, C, Lc)
        for g, r in zip(got, ref):
            assert np.array_equal(g.cpu().numpy(), r)


def test_l2norm_chunk_with_row_plans(ops):
    B, T, F = 6, 300, 1152
    q, x, n, _ = mm.synthetic_batch(B, seed=8, dtype=np.float32)
    n[0], n[1] = 300, 7
    qd, nd = torch.from_numpy(q).to(DEV), torch.from_numpy(n).to(DEV)
    _, l1, _ = ops.frame_counts(nd, 1, 20, 15)
    _, l1s, _ = ops.frame_counts(nd, 10, 5, 6)
    p1 = ops.RowPlan(l1, ops.host_frame_counts(n, 1, 20, 15)[1], 15)
    p2 = ops.RowPlan(l1s, ops.host_frame_counts(n, 10, 5, 6)[1], 6)
    assert p1.P < 20 * B and p1.P % 32 == 0
    r1, r2 = ops.l2norm_chunk(qd, 20, 10, 5, num_frames=nd)                        # plain layout
    o1, o2 = ops.l2norm_chunk(qd, 20, 10, 5, num_frames=nd, plan1=p1, plan2=p2)   # slot layout
    assert o1.shape == (15, p1.P, F) and o2.shape == (6, p2.P, F)
    inv1, inv2 = p1.inv.cpu().numpy(), p2.inv.cpu().numpy()
    live1, live2 = p1.rows[0], p2.rows[0]
    assert torch.equal(o1[:, :live1], r1[:, torch.from_numpy(inv1[:live1]).to(DEV).long()])
    assert torch.equal(o2[:, :live2], r2[:, torch.from_numpy(inv2[:live2]).to(DEV).long()])
    assert bool((r1[:, torch.from_numpy(inv1[live1:]).to(DEV).long()] == 0).all())     # what was dropped is all padding


@pytest.mark.parametrize("every_n,u8", [(30, False), (30, True), (10, False), (1, True), (60, False)])
@pytest.mark.parametrize("split", [False, "f16", "fp8", "wide"])
def test_l2norm_chunk_student_only_reads_the_subsampled_frames(ops, every_n, u8, split):
    """evc_l2norm_chunk_fwd with out1 == NULL (student-only graphs, cs/train_finetune.py:243-318; round 6): the student view - and its second
    image in every "high" / "split" layout - is bit-identical to the one the two-view call writes, with and without a row plan; the frames
    between the sub-sampled ones are never read (NaN there changes nothing: at every_n = 30 the launch touches 1/30 of the tensor)."""
    B, T, F, C2 = 5, 300, 1152, 5
    q, x, n, _ = mm.synthetic_batch(B, seed=40 + every_n, dtype=np.float32)
    n[0], n[1] = 300, 31
    x[np.arange(T)[None, :] >= n[:, None]] = 0.0
    src = torch.from_numpy(q if u8 else x).to(DEV)
    nd = torch.from_numpy(n).to(DEV)
    S = T // every_n
    kw = dict(num_frames=nd if u8 else None)
    if split == "fp8":
        kw.update(split="f16", f16_segments=1, fp8_tail=True)
    elif split:
        kw.update(split=split, f16_segments=2 if split == "f16" else 1)
    _, l1s, _ = ops.frame_counts(nd, every_n, C2, S // C2, subsampled=True)
    plan = ops.RowPlan(l1s, ops.host_frame_counts(n, every_n, C2, S // C2, subsampled=True)[1], S // C2)
    for p2 in (None, plan):
        both = ops.l2norm_chunk(src, 20, every_n, C2, plan2=p2, **kw)
        only = ops.l2norm_chunk(src, 20, every_n, C2, plan2=p2, teacher_view=False, **kw)
        assert only[0] is None
        live = p2.rows[0] if p2 is not None else C2 * B          # (slots past the live rows are never written: compare the live ones)
        for a, b in zip(both[1] if split else (both[1],), only[1] if split else (only[1],)):
            assert a.shape == b.shape and torch.equal(a[:, :live], b[:, :live])
    if not u8:       # poison every frame the student does not use
        xp = src.clone()
        mask = torch.ones(T, dtype=torch.bool, device=DEV)
        mask[torch.arange(0, S * every_n, every_n, device=DEV)] = False
        xp[:, mask] = float("nan")
        got = ops.l2norm_chunk(xp, 20, every_n, C2, teacher_view=False, **kw)[1]
        ref = ops.l2norm_chunk(src, 20, every_n, C2, teacher_view=False, **kw)[1]
        for a, b in zip(got if split else (got,), ref if split else (ref,)):
            assert torch.equal(a, b)


@pytest.mark.parametrize("M,T,Kin,H", [(640, 5, 64, 128), (5120, 4, 128, 128), (200, 6, 64, 64)])
def test_lstm_layer_with_row_plan_matches_plain(ops, M, T, Kin, H):
    """Forward + BPTT on length-sorted rows (padding rows skipped) give the plain-layout results."""
    rng = np.random.default_rng(M + T)
    lens = rng.integers(0, T + 1, size=M).astype(np.int32)
    lens[rng.random(M) < 0.3] = 0
    lens[:2] = [T, 0]
    x = to_bf16(rng.standard_normal((T, M, Kin)) * 0.5)
    wT = to_bf16(mm.glorot_uniform(rng, (4 * H, Kin + H)) * 2.0)
    w_il = torch.empty((Kin + H, 4 * H), dtype=torch.bfloat16, device=DEV)
    ops.transpose_to_bf16(wT, 4 * H, Kin + H, w_il, 4 * H, interleave_H=H)
    b = torch.from_numpy((rng.standard_normal(4 * H) * 0.1).astype(np.float32)).to(DEV)
    ln = torch.from_numpy(lens).to(DEV)
    dS = torch.from_numpy(rng.standard_normal((M, 2 * H)).astype(np.float32)).to(DEV)
    dha = to_bf16(rng.standard_normal((T, M, H)) * 0.3)

    def run(plan):
        P = plan.P if plan is not None else M
        if plan is not None:
            idx = plan.inv[:P].long()
            xs, dh, lens_d = x[:, idx].contiguous(), dha[:, idx].contiguous(), plan.lens
        else:
            xs, dh, lens_d = x, dha, ln
        hbuf = torch.zeros((T + 1, P, H), dtype=torch.bfloat16, device=DEV)
        S = torch.zeros((M, 2 * H), dtype=torch.float32, device=DEV)
        gates = torch.empty((T, P, H, 2), dtype=torch.int32, device=DEV)
        c_all = torch.full((T + 1, P, H), float("nan"), dtype=torch.bfloat16, device=DEV)
        ops.lstm_layer_fwd(xs, wT, b, lens_d, T, P, Kin, H, hbuf, S[:, :H], S[:, H:], 2 * H, gates, c_all, plan=plan)
        dz4 = torch.full((T, P, 4 * H), float("nan"), dtype=torch.bfloat16, device=DEV)
        dcw = torch.empty((P, H), dtype=torch.float32, device=DEV)
        ops.lstm_layer_bwd(w_il, lens_d, T, P, Kin, H, gates, c_all, dS[:, :H], dS[:, H:], 2 * H, dh, dcw, dz4, plan=plan)
        assert bool(torch.isfinite(dz4.float()).all())
        dW = torch.empty((4 * H, Kin), dtype=torch.float32, device=DEV)
        if (T * P) % 32 == 0:
            ops.gemm_tn(dz4.view(T * P, 4 * H), xs.reshape(T * P, Kin), 4 * H, Kin, T * P, dW, row_interleave_H=H)
        return S, hbuf, dz4, dW

    S0, h0, dz0, dW0 = run(None)
    plan = ops.RowPlan(ln, lens, T)
    S1, h1, dz1, dW1 = run(plan)
    assert torch.equal(S0, S1)                                  # same per-row arithmetic, original row order
    live = plan.rows[0]
    idx = plan.inv[:live].long()
    for t in range(T):
        rt = plan.rows[t]
        assert torch.equal(h1[t + 1, :rt], h0[t + 1, idx[:rt]])
        # the BPTT tile (and with it the K summation order) may differ between the two row counts: 1 bf16 ulp
        a, b = dz1[t, :rt].float(), dz0[t, idx[:rt]].float()
        assert (a - b).abs().max().item() <= 2.0 ** -7 * b.abs().max().item() + 1e-12
        assert bool((dz1[t, rt:] == 0).all())                   # every dz row is written: zeros beyond the active prefix
    if (T * plan.P) % 32 == 0 and (T * M) % 32 == 0:
        sc = dW0.abs().max().item() + 1e-6
        assert (dW0 - dW1).abs().max().item() / sc < 1e-3      # dz within one bf16 ulp, different summation order


@pytest.mark.parametrize("M,T,Kin,H,planned", [(4096, 4, 192, 128, True), (5120, 5, 128, 128, True), (3840, 3, 128, 256, False), (600, 4, 128, 128, True)])
def test_lstm_level2_fwd_two_tiles_per_workgroup_equals_two_layer_calls(ops, M, T, Kin, H, planned):
    """Round 5: a two-layer many-row level as T + 1 launches (evc_lstm_level2_fwd) - layer 0's step s and layer 1's step s-1 in one launch
    whose workgroups walk both tiles, the second tile's first ring stages issued under the first tile's gate tail - against two
    evc_lstm_layer_fwd calls: the same arithmetic in the same order, so h, the states, the gate records and the cell history must be
    IDENTICAL - on row plans whose live rows pick the 256- / 240- / 224-row ring tiles (walk), with launches that fall back to two separate
    ones (600 rows: smaller tiles), with a step count that leaves layer 1's last step alone in its launch, and in the evaluation form
    (no tape)."""
    rng = np.random.default_rng(M + T)
    lens = rng.integers(1, T + 1, size=M).astype(np.int32)
    lens[rng.random(M) < (0.25 if planned else 0.0)] = 0
    lens[:2] = [T, T if not planned else 0]
    x = to_bf16(rng.standard_normal((T, M, Kin)) * 0.5)
    w0 = to_bf16(mm.glorot_uniform(rng, (4 * H, Kin + H)) * 2.0)
    w1 = to_bf16(mm.glorot_uniform(rng, (4 * H, 2 * H)) * 2.0)
    b0 = torch.from_numpy((rng.standard_normal(4 * H) * 0.1).astype(np.float32)).to(DEV)
    b1 = torch.from_numpy((rng.standard_normal(4 * H) * 0.1).astype(np.float32)).to(DEV)
    ln = torch.from_numpy(lens).to(DEV)
    plan = ops.RowPlan(ln, lens, T) if planned else None
    P = plan.P if plan is not None else M
    xs = x[:, plan.inv[:P].long()].contiguous() if plan is not None else x
    lens_d = plan.lens if plan is not None else ln
    for tape in (True, False):
        outs = []
        for walk in (False, True):
            hb = [torch.full((T + 1, P, H), float("nan"), dtype=torch.bfloat16, device=DEV) for _ in range(2)]
            S = torch.full((M, 4 * H), float("nan"), dtype=torch.float32, device=DEV)
            gates = [torch.full((T, P, H, 2), -1, dtype=torch.int32, device=DEV) if tape else None for _ in range(2)]
            c_all = [torch.full((T + 1, P, H), float("nan"), dtype=torch.bfloat16, device=DEV) if tape else None for _ in range(2)]
            if walk:
                ops.lstm_level2_fwd(xs, w0, b0, w1, b1, lens_d, T, P, Kin, H, hb[0], hb[1], S, gates, c_all, plan=plan)
            else:
                ops.lstm_layer_fwd(xs, w0, b0, lens_d, T, P, Kin, H, hb[0], S[:, 0:], S[:, H:], 4 * H, gates[0], c_all[0], plan=plan)
                ops.lstm_layer_fwd(hb[0][1:], w1, b1, lens_d, T, P, H, H, hb[1], S[:, 2 * H:], S[:, 3 * H:], 4 * H, gates[1], c_all[1], plan=plan)
            torch.cuda.synchronize()
            outs.append((hb, S, gates, c_all))
        (ha, Sa, ga, ca), (hw, Sw, gw, cw) = outs
        rows = plan.rows if plan is not None else [M] * T
        live = np.nonzero(lens > 0)[0]
        assert torch.equal(Sa[torch.from_numpy(live).to(DEV)].view(torch.int32), Sw[torch.from_numpy(live).to(DEV)].view(torch.int32)) and bool(torch.isfinite(Sw[torch.from_numpy(live).to(DEV)]).all())
        for l in range(2):
            assert bool((hw[l][0] == 0).all())
            for t in range(T):
                rt = rows[t]
                assert torch.equal(ha[l][t + 1, :rt].view(torch.int16), hw[l][t + 1, :rt].view(torch.int16)), (l, t)
                if tape:
                    assert torch.equal(ga[l][t, :rt], gw[l][t, :rt]) and torch.equal(ca[l][t + 1, :rt].view(torch.int16), cw[l][t + 1, :rt].view(torch.int16)), (l, t)


@pytest.mark.parametrize("M,T,F,H,planned,int_form,h_lo", [(4096, 4, 384, 256, True, True, True), (5120, 5, 384, 128, True, False, True), (3840, 3, 384, 256, False, True, True),
                                                            (3840, 3, 512, 128, False, False, False), (600, 4, 384, 128, True, True, True)])
def test_lstm_level2_fwd_high_equals_the_two_layer_calls(ops, M, T, F, H, planned, int_form, h_lo):
    """Round 6: the "high" mode's two-layer L1 level as T + 1 two-tile launches (evc_lstm_level2_fwd_high) - tile a = layer 0's step s on f16 + e4m3 stages
    (integer frames with the accumulator rescale, or f32-input rows; h rows with or without the low-order image), tile b = the dithered upper layer's step
    s-1 on plain f16 stages, each in its own loop mode - against evc_lstm_layer_fwd_f16_fp8lo + evc_lstm_layer_fwd_f16_dith: the same arithmetic in the
    same order, so every h row image, the bf16 copies, the states, the gate records and the cell history must be IDENTICAL - on row plans, with launches
    that fall back to separate ones (600 rows), and in the evaluation form (no tape)."""
    rng = np.random.default_rng(M + T + H)
    lens = rng.integers(1, T + 1, size=M).astype(np.int32)
    lens[rng.random(M) < (0.25 if planned else 0.0)] = 0
    lens[:2] = [T, T if not planned else 0]
    q = rng.integers(0, 256, size=(T, M, F), dtype=np.uint8)
    xr = mm.dequantize(q.astype(np.float64))
    nrm = np.sqrt((xr ** 2).sum(-1))
    xt = torch.from_numpy((xr / nrm[..., None]).astype(np.float32)).to(DEV)
    qt = torch.from_numpy(q).to(DEV)
    k0 = torch.from_numpy(np.ascontiguousarray((mm.glorot_uniform(rng, (F + H, 4 * H)) * 2.0).astype(np.float32).T)).to(DEV)
    k1 = torch.from_numpy(np.ascontiguousarray((mm.glorot_uniform(rng, (2 * H, 4 * H)) * 2.0).astype(np.float32).T)).to(DEV)
    b0 = torch.from_numpy((rng.standard_normal(4 * H) * 0.1).astype(np.float32)).to(DEV)
    b1 = torch.from_numpy((rng.standard_normal(4 * H) * 0.1).astype(np.float32)).to(DEV)
    w16 = torch.empty((4 * H, F + H), dtype=torch.float16, device=DEV)
    ops.cast_f16(k0, w16)
    w8 = torch.empty((4 * H, (2 * F + 2 * H) if h_lo else (2 * F + H)), dtype=torch.uint8, device=DEV)
    ops.cast_fp8_lo(k0, w8, hi_cols=F, hi_tail=h_lo)
    w16d = torch.empty((T, 4 * H, 2 * H), dtype=torch.float16, device=DEV)
    ops.cast_f16_dither(k1, w16d, 1234)
    x8 = (xt * 128.0).clamp(-448, 448).to(torch.float8_e4m3fn)
    if int_form:
        src = torch.zeros((T, M, 3 * F // 2), dtype=torch.float16, device=DEV)
        src[:, :, :F] = (2.0 * qt.float() - 255.0).half()
        src[:, :, F:] = x8.view(torch.float16)
        rs = torch.from_numpy(((2.0 / 255.0) / nrm).astype(np.float32)).to(DEV).contiguous()
        cc = w16[:, :F].sum(dim=1, dtype=torch.float32) * (255.0 / 256.0)
        cc[2 * H:3 * H] -= 1.0
        cc = cc.contiguous()
        x8_off, kx8, gap = 2 * F, F, F
    else:
        src = torch.zeros((T, M, 2 * F), dtype=torch.float16, device=DEV)
        hi = xt.half()
        src[:, :, :F] = hi
        src[:, :, F:3 * F // 2] = x8.view(torch.float16)
        src[:, :, 3 * F // 2:] = ((xt - hi.float()) * 2.0 ** 18).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.float16)
        rs = cc = None
        x8_off, kx8, gap = 2 * F, 2 * F, 0
    ln = torch.from_numpy(lens).to(DEV)
    plan = ops.RowPlan(ln, lens, T) if planned else None
    P = plan.P if plan is not None else M
    inp, lens_d, rs_run = src, ln, rs
    if plan is not None:
        live_rows = plan.rows[0]
        inp = torch.zeros((T, P, src.shape[-1]), dtype=torch.float16, device=DEV)
        inp[:, :live_rows] = src[:, plan.inv[:live_rows].long()]
        if rs is not None:
            rs_run = torch.zeros((T, P), dtype=torch.float32, device=DEV)
            rs_run[:, :live_rows] = rs[:, plan.inv[:live_rows].long()]
        lens_d = plan.lens
    xi = (rs_run, cc) if int_form else None
    wrow = 2 * H if h_lo else 3 * H // 2
    for tape in (True, False):
        outs = []
        for walk in (False, True):
            h0 = torch.full((T + 1, P, wrow), float("nan"), dtype=torch.float16, device=DEV)
            h1 = torch.full((T + 1, P, H), float("nan"), dtype=torch.float16, device=DEV)
            hb = [torch.full((T + 1, P, H), float("nan"), dtype=torch.bfloat16, device=DEV) for _ in range(2)]
            S = torch.full((M, 4 * H), float("nan"), dtype=torch.float32, device=DEV)
            gates = [torch.full((T, P, H, 2), -1, dtype=torch.int32, device=DEV) if tape else None for _ in range(2)]
            c_all = [torch.full((T + 1, P, H), float("nan"), dtype=torch.bfloat16, device=DEV) if tape else None for _ in range(2)]
            if walk:
                ops.lstm_level2_fwd_high(inp, inp.shape[-1], F, x8_off, kx8, w16, w8, b0, w16d, b1, lens_d, T, P, H, h0, hb[0], h1, hb[1], S, gates, c_all, plan=plan,
                                         h_lo=h_lo, x_int=xi, b8_gap=gap)
            else:
                ops.lstm_layer_fwd_f16_fp8lo(inp, inp.shape[-1], F, x8_off, kx8, w16, w8, b0, lens_d, T, P, H, h0, hb[0], S[:, 0:], S[:, H:], 4 * H, gates[0], c_all[0],
                                             plan=plan, h_lo=h_lo, x_int=xi, b8_gap=gap)
                ops.lstm_layer_fwd_f16_dith(h0[1:], wrow, H, 0, 0, w16d, None, 0, 7 + ops.FP8_W_SCALE_EXP, b1, lens_d, T, P, H, h1, hb[1], S[:, 2 * H:], S[:, 3 * H:], 4 * H,
                                            gates[1], c_all[1], plan=plan)
            torch.cuda.synchronize()
            outs.append((h0, h1, hb, S, gates, c_all))
        (h0a, h1a, ha, Sa, ga, ca), (h0w, h1w, hw, Sw, gw, cw) = outs
        rows = plan.rows if plan is not None else [M] * T
        live = torch.from_numpy(np.nonzero(lens > 0)[0]).to(DEV)
        assert torch.equal(Sa[live].view(torch.int32), Sw[live].view(torch.int32)) and bool(torch.isfinite(Sw[live]).all())
        assert bool((h0w[0] == 0).all()) and bool((h1w[0] == 0).all()) and bool((hw[0][0] == 0).all()) and bool((hw[1][0] == 0).all())
        for t in range(T):
            rt = rows[t]
            assert torch.equal(h0a[t + 1, :rt].view(torch.int16), h0w[t + 1, :rt].view(torch.int16)), ("h0 rows", t)
            assert torch.equal(h1a[t + 1, :rt].view(torch.int16), h1w[t + 1, :rt].view(torch.int16)), ("h1 rows", t)
            for l in range(2):
                assert torch.equal(ha[l][t + 1, :rt].view(torch.int16), hw[l][t + 1, :rt].view(torch.int16)), (l, t)
                if tape:
                    assert torch.equal(ga[l][t, :rt], gw[l][t, :rt]) and torch.equal(ca[l][t + 1, :rt].view(torch.int16), cw[l][t + 1, :rt].view(torch.int16)), (l, t)
    assert float(Sw[live].abs().max()) > 0.05


@pytest.mark.parametrize("M,N1,N2,K,il", [(512, 256, 128, 4096, 128), (256, 192, 0, 2048, 0), (1024, 512, 256, 8192, 256)])
def test_gemm_tn_det_slabs_equal_the_product_and_repeat_bit_for_bit(ops, M, N1, N2, K, il):
    """EVC_DETERMINISTIC=1 weight gradients (round 5): the TN product with its K split kept, the partial products stored as slabs
    (evc_gemm_tn2_slabs: two column segments, gate de-interleave, C's row stride) and added in slab order (evc_sum_slabs) instead of joined
    with atomics - against a float64 product of the same bf16 operands, accumulating onto what C holds, and IDENTICAL bits on a second run."""
    rng = np.random.default_rng(M + K)
    A = to_bf16(rng.standard_normal((K, M)) * 0.1)
    B1 = to_bf16(rng.standard_normal((K, N1)) * 0.1)
    B2 = to_bf16(rng.standard_normal((K, N2)) * 0.1) if N2 else None
    c2 = N1 + 64 if N2 else None                                       # the second segment lands 64 columns behind the first (layer 0: 1152 vs 1024)
    ldc = (c2 + N2) if N2 else N1
    C0 = torch.from_numpy(rng.standard_normal((M, ldc)).astype(np.float32)).to(DEV)
    outs = []
    for _ in range(2):
        C = C0.clone()
        ops.gemm_tn_det(A, B1, M, N1, K, C, row_interleave_H=il, accumulate=True, ldc=ldc, B2=B2, N2=N2, c_col2=c2)
        torch.cuda.synchronize()
        outs.append(C)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    ref = C0.double().cpu().numpy().copy()
    prod1 = A.double().cpu().numpy().T @ B1.double().cpu().numpy()
    rows = (np.arange(M) % 4) * il + np.arange(M) // 4 if il else np.arange(M)         # row u*4+g of the product -> row g*H+u
    ref[rows, :N1] += prod1
    if N2:
        ref[rows, c2:c2 + N2] += A.double().cpu().numpy().T @ B2.double().cpu().numpy()
    got = outs[0].double().cpu().numpy()
    assert np.abs(got - ref).max() < 2e-4 * np.abs(ref).max() + 1e-4
    if N2:
        assert np.array_equal(got[:, N1:c2], C0.double().cpu().numpy()[:, N1:c2])    # the gap between the segments is untouched


def test_clip_adam_small_equals_the_per_tensor_launches(ops):
    """Round 5: per-tensor clip_by_norm + TF-Adam of several small tensors in ONE launch (evc_clip_adam_small: workgroup i = tensor i, norm by a
    block sum) against evc_grad_sqnorm + evc_clip_adam_step per tensor and against the float64 formula - sizes that are not multiples of 4 or 256,
    a tensor whose norm is below the clip threshold and one above it, 16 tensors (the limit) and the error for 17."""
    rng = np.random.default_rng(8)
    sizes = [1152, 8192, 1, 1024, 4716 * 2, 257, 3, 64, 100, 1000, 5, 8193, 2, 640, 77, 4096]
    lr_t, clip, b1, b2, eps = 1.3e-3, 1.0, 0.9, 0.999, 1e-8
    P = [torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV) for n in sizes]
    G = [torch.from_numpy((rng.standard_normal(n) * (0.3 if i % 2 else 0.003)).astype(np.float32)).to(DEV) for i, n in enumerate(sizes)]
    Mo = [torch.from_numpy((rng.standard_normal(n) * 1e-2).astype(np.float32)).to(DEV) for n in sizes]
    Vo = [torch.from_numpy((rng.random(n) * 1e-4).astype(np.float32)).to(DEV) for n in sizes]
    a = [[t.clone() for t in L] for L in (P, Mo, Vo)]
    b = [[t.clone() for t in L] for L in (P, Mo, Vo)]
    sa = torch.full((len(sizes), 2), float("nan"), device=DEV)
    sb = torch.zeros((len(sizes), 2), device=DEV)
    ops.clip_adam_small(a[0], G, a[1], a[2], [sa[i] for i in range(len(sizes))], clip, lr_t, b1, b2, eps)
    for i in range(len(sizes)):
        ops.grad_sqnorm(G[i], None, 0.0, sb[i])
        ops.clip_adam_step(b[0][i], G[i], b[1][i], b[2][i], 0.0, sb[i], clip, lr_t, b1, b2, eps)
    torch.cuda.synchronize()
    assert torch.allclose(sa[:, 0], sb[:, 0], rtol=2e-6, atol=0) and bool((sa[:, 1] == 0).all())
    for i, n in enumerate(sizes):
        g64 = G[i].double().cpu().numpy()
        nrm = np.sqrt((g64 ** 2).sum())
        gc = g64 * (clip / max(nrm, clip))
        m64 = b1 * Mo[i].double().cpu().numpy() + (1 - b1) * gc
        v64 = b2 * Vo[i].double().cpu().numpy() + (1 - b2) * gc * gc
        p64 = P[i].double().cpu().numpy() - lr_t * m64 / (np.sqrt(v64) + eps)
        for got, other, want in ((a[0][i], b[0][i], p64), (a[1][i], b[1][i], m64), (a[2][i], b[2][i], v64)):
            assert np.abs(got.double().cpu().numpy() - want).max() <= 2e-6 * (np.abs(want).max() + 1e-6) + 1e-9, (i, n)
            assert (got - other).abs().max().item() <= 1e-6 * (other.abs().max().item() + 1e-6) + 1e-9, (i, n)
    assert (nrm_big := float(np.sqrt(sb[1, 0].item()))) > clip and float(np.sqrt(sb[0, 0].item())) < clip, nrm_big     # both sides of the clip
    with pytest.raises(AssertionError):                               # 17 tensors: the table of one launch holds 16
        ops.clip_adam_small(a[0] + [a[0][0]], G + [G[0]], a[1] + [a[1][0]], a[2] + [a[2][0]], [sa[i] for i in range(16)] + [sa[0]], clip, lr_t)


def test_kl_pred_loss_against_oracle_and_degenerate_rows(ops):
    """L_PRED (cs/train.py:398-402): Categorical KL of the renormalised probabilities, summed over the batch, with
    its gradient wrt the student probabilities; rows where the reference would produce NaN/inf stay finite."""
    rng = np.random.default_rng(3)
    B, V = 6, 500
    pt = rng.random((B, V)).astype(np.float32) ** 4
    ps = rng.random((B, V)).astype(np.float32) ** 2 + 1e-3
    pt[0, :50] = 0.0                                   # exact zeros in the teacher: 0 * log 0 := 0
    def kl_ref(p, q):                                  # mm.pred_kl_loss with 0 * log 0 := 0
        P, Q = p / p.sum(1, keepdims=True), q / q.sum(1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.where(P > 0, P * (np.log(P) - np.log(Q)), 0.0).sum())

    loss_ref = kl_ref(pt.astype(np.float64), ps.astype(np.float64))
    full = pt.copy()
    full[0, :50] = 1e-3
    assert abs(kl_ref(full.astype(np.float64), ps.astype(np.float64)) - mm.pred_kl_loss(full.astype(np.float64), ps.astype(np.float64))) < 1e-9
    ptd, psd = torch.from_numpy(pt).to(DEV), torch.from_numpy(ps).to(DEV)
    loss = torch.zeros(1, device=DEV)
    dps = torch.empty((B, V), device=DEV)
    ops.kl_pred_loss(ptd, ptd.sum(1), psd, psd.sum(1), loss, dps)
    assert abs(loss.item() - loss_ref) < 1e-4 * abs(loss_ref)
    # gradient: finite differences of the oracle on a few entries
    for (b, c) in ((1, 3), (4, 499), (0, 10)):
        e = 1e-4 * ps[b, c]
        up, dn = ps.astype(np.float64).copy(), ps.astype(np.float64).copy()
        up[b, c] += e
        dn[b, c] -= e
        fd = (kl_ref(pt.astype(np.float64), up) - kl_ref(pt.astype(np.float64), dn)) / (2 * e)
        assert abs(dps[b, c].item() - fd) < 2e-3 * abs(fd) + 1e-6
    # degenerate: a collapsed teacher row (sum underflows) and student probabilities that are exactly 0
    pt2, ps2 = pt.copy(), ps.copy()
    pt2[2] = 1e-44
    ps2[3, :7] = 0.0
    ptd, psd = torch.from_numpy(pt2).to(DEV), torch.from_numpy(ps2).to(DEV)
    loss.zero_()
    ops.kl_pred_loss(ptd, ptd.sum(1), psd, psd.sum(1), loss, dps)
    assert np.isfinite(loss.item()) and bool(torch.isfinite(dps).all())
    assert bool((dps[2] == 0).all())                   # the undefined row contributes nothing


def test_clip_adam_vector_and_scalar_paths_and_gradient_only_norm(ops):
    """evc_clip_adam_step takes 16-byte accesses when every pointer allows it and a scalar path otherwise: same
    numbers; evc_grad_sqnorm with p == NULL reads the gradient only and leaves sums[1] alone."""
    torch.manual_seed(3)
    n = 4099                                             # not a multiple of 4: scalar tail in the vector path
    base = [torch.randn(n + 1, device=DEV) * s for s in (0.1, 1.0, 1e-3)] + [torch.rand(n + 1, device=DEV) * 1e-4]
    outs = []
    for off in (0, 1):                                   # offset 1 breaks the 16-byte alignment -> scalar path
        p, g, m, v = (t[:n].clone() for t in base)
        if off:
            p, g, m, v = (torch.cat([t.new_zeros(1), t])[1:] for t in (p, g, m, v))        # storage offset 1: 4-byte aligned only
            assert all(t.data_ptr() % 16 != 0 for t in (p, g, m, v))
        else:
            p, g, m, v = (t.clone() for t in (p, g, m, v))
            assert all(t.data_ptr() % 16 == 0 for t in (p, g, m, v))
        pb = torch.zeros(n + 8, dtype=torch.bfloat16, device=DEV)[:n]
        sums = torch.zeros(2, device=DEV)
        ops.grad_sqnorm(g.clone(), None, 0.0, sums)      # (the norm pass itself requires 16-byte aligned tensors)
        assert sums[1].item() == 0.0
        assert abs(sums[0].item() - float((g.double() ** 2).sum())) < 1e-3 * sums[0].item()
        ops.clip_adam_step(p, g, m, v, 0.0, sums, 1.0, 1e-3, p_bf16=pb)
        outs.append((p.clone(), m.clone(), v.clone(), pb.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # with a regulariser the weights are read too
    p, g = base[0][:n].clone(), base[1][:n].clone()
    sums = torch.zeros(2, device=DEV)
    ops.grad_sqnorm(g, p, 0.5, sums)
    assert abs(sums[0].item() - float(((g + 0.5 * p).double() ** 2).sum())) < 1e-3 * sums[0].item()
    assert abs(sums[1].item() - float((p.double() ** 2).sum())) < 1e-3 * sums[1].item()
    with pytest.raises(Exception):
        ops.grad_sqnorm(g, None, 0.5, sums)              # p == NULL needs l2_coeff == 0


@pytest.mark.parametrize("H,nin,images", [(64, 64, "bf16"), (128, 384, "l1_fp8_layer0"), (128, 128, "l1_fp8_upper"), (128, 512, "l2_fp8_layer0"),
                                          (128, 128, "f16_plain"), (1024, 1152, "l1_fp8_layer0"),
                                          (128, 384, "lohi_l1"), (128, 512, "lohi_l2_layer0"), (128, 128, "lohi_l2_layer1"), (1024, 1152, "lohi_l1")])
def test_fused_lstm_adam_equals_the_per_tensor_launches_and_writes_every_operand_image(ops, H, nin, images):
    """evc_sqnorm2_partials + evc_lstm_adam_fused (one layer's kernel + bias: clip, TF-Adam, bf16 forward shadow, transposed
    gate-interleaved backward shadow, f16 / e4m3 images of the "high" layouts - all from one pass) against evc_grad_sqnorm +
    evc_clip_adam_step + evc_transpose_to_bf16 + the cast kernels: identical bits for everything that does not depend on the
    summation order of the norm (a clipping step: both norms >> 1), every image identical to the cast of the new weights."""
    torch.manual_seed(11)
    R, C = 4 * H, nin + H
    p0 = torch.randn(R, C, device=DEV) * 0.05
    g0 = torch.randn(R, C, device=DEV) * 0.02          # |g| >> 1: the clip is active
    m0, v0 = torch.randn(R, C, device=DEV) * 1e-3, torch.rand(R, C, device=DEV) * 1e-5
    pb0, gb0 = torch.randn(R, device=DEV) * 0.1, torch.randn(R, device=DEV) * 0.5
    mb0, vb0 = torch.randn(R, device=DEV) * 1e-3, torch.rand(R, device=DEV) * 1e-5
    lr_t, clip = 3e-4, 1.0
    kw, nseg, col0, hi_cols = {}, 1, 0, 0
    F16 = torch.float16
    tail = images.startswith("lohi")          # round 6: [lo | hi] images of every part (the h_lo forms of the forward kernels)
    if images != "bf16":
        nseg = {"l2_fp8_layer0": 2, "lohi_l2_layer0": 2}.get(images, 1)
        kw.update(p_f16=torch.zeros(R, nseg * nin + H, dtype=F16, device=DEV), nin=nin, nseg=nseg)
        if images != "f16_plain":
            col0 = nin if images in ("l2_fp8_layer0", "lohi_l2_layer0") else 0
            hi_cols = nin if images in ("l1_fp8_layer0", "lohi_l1", "lohi_l2_layer1") else 0
            kw.update(p_fp8=torch.zeros(R, 2 * (C - col0) if tail else C - col0 + hi_cols, dtype=torch.uint8, device=DEV), fp8_col0=col0, fp8_hi_cols=hi_cols,
                      fp8_hi_tail=tail)
    # fused
    p, g, m, v, pb, gb, mb, vb = (t.clone() for t in (p0, g0, m0, v0, pb0, gb0, mb0, vb0))
    sh_f = torch.zeros(R, C, dtype=torch.bfloat16, device=DEV)
    sh_b = torch.zeros(C, R, dtype=torch.bfloat16, device=DEV)
    sums = torch.zeros(2, 2, device=DEV)
    ws = torch.empty(1028, device=DEV)
    ops.lstm_adam_fused(p, g, m, v, pb, gb, mb, vb, ws, sums[0], sums[1], clip, lr_t, sh_f, sh_b, **kw)
    # per-tensor launches
    q, qm, qv, qb, qmb, qvb = (t.clone() for t in (p0, m0, v0, pb0, mb0, vb0))
    rsums = torch.zeros(2, 2, device=DEV)
    ops.grad_sqnorm(g0, None, 0.0, rsums[0])
    ops.grad_sqnorm(gb0, None, 0.0, rsums[1])
    rf = torch.zeros_like(sh_f)
    ops.clip_adam_step(q, g0, qm, qv, 0.0, rsums[0], clip, lr_t, p_bf16=rf)
    ops.clip_adam_step(qb, gb0, qmb, qvb, 0.0, rsums[1], clip, lr_t)
    torch.cuda.synchronize()
    assert torch.allclose(sums[:, 0], rsums[:, 0], rtol=2e-6) and float(sums[0, 0]) > 10 and float(sums[1, 0]) > 10
    for a, b, name in ((p, q, "p"), (m, qm, "m"), (v, qv, "v"), (pb, qb, "pb"), (mb, qmb, "mb"), (vb, qvb, "vb")):
        assert (a - b).abs().max().item() <= 4e-6 * b.abs().max().item(), name      # (the two norms differ in their last bits: scale -> m, v)
    # every image is the cast of the NEW weights p, bit for bit
    assert torch.equal(sh_f, p.bfloat16())
    want_b = torch.zeros_like(sh_b)
    ops.transpose_to_bf16(sh_f, R, C, want_b, R, interleave_H=H)
    assert torch.equal(sh_b, want_b)
    if "p_f16" in kw:
        w16 = torch.zeros_like(kw["p_f16"])
        if nseg == 1:
            ops.cast_f16(p, w16)
        else:
            ops.cast_f16_wide(p, nin, H, nseg, w16, h_ext=False)
        assert torch.equal(kw["p_f16"], w16)
    if "p_fp8" in kw:
        w8 = torch.zeros_like(kw["p_fp8"])
        ops.cast_fp8_lo(p[:, col0:], w8, hi_cols=hi_cols, hi_tail=tail)
        assert torch.equal(kw["p_fp8"], w8)
        if tail:                  # [lo(A) | hi(A) | lo(B) | hi(B)]: the hi blocks are e4m3(W 2^6) of the same columns
            Cc = C - col0
            hi_want = (p[:, col0:] * 64.0).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
            assert torch.equal(w8[:, hi_cols:2 * hi_cols], hi_want[:, :hi_cols]) and torch.equal(w8[:, Cc + hi_cols:], hi_want[:, hi_cols:])
    # run-to-run identical (no atomics anywhere)
    p2, m2, v2, pb2, mb2, vb2 = (t.clone() for t in (p0, m0, v0, pb0, mb0, vb0))
    s2 = torch.zeros(2, 2, device=DEV)
    ops.lstm_adam_fused(p2, g0, m2, v2, pb2, gb0, mb2, vb2, ws, s2[0], s2[1], clip, lr_t, torch.zeros_like(sh_f), torch.zeros_like(sh_b),
                        **{k: (torch.zeros_like(t) if torch.is_tensor(t) else t) for k, t in kw.items()})
    assert torch.equal(p2, p) and torch.equal(m2, m) and torch.equal(v2, v) and torch.equal(pb2, pb) and torch.equal(s2, sums)


@pytest.mark.parametrize("R,C,images", [(200, 68, False), (4716, 1152, False), (1024, 8192, True), (8192, 1152, True)])
def test_fused_adam_for_plain_2d_weights(ops, R, C, images):
    """evc_adam2d_fused (the pass of evc_lstm_adam_fused for a plain [R][C] weight without a bias: DBoF cluster / hidden weights, the
    logistic matrix) against grad_sqnorm + clip_adam_step + transpose (+ casts): same update up to the norm's summation order, the
    bf16 forward shadow, the transposed backward shadow with ZERO pad columns and the f16 / e4m3 images bit-equal to casts of the new weights."""
    torch.manual_seed(R + C)
    p0, g0 = torch.randn(R, C, device=DEV) * 0.05, torch.randn(R, C, device=DEV) * 0.02
    m0, v0 = torch.randn(R, C, device=DEV) * 1e-3, torch.rand(R, C, device=DEV) * 1e-5
    Rp = (R + 63) // 64 * 64
    kw = {}
    if images:
        kw = dict(p_f16=torch.zeros(R, C, dtype=torch.float16, device=DEV), p_fp8=torch.zeros(R, 2 * C, dtype=torch.uint8, device=DEV),
                  fp8_hi_cols=C, fp8_lo_exp=19, fp8_hi_exp=8)
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    sh_f = torch.zeros(R, C, dtype=torch.bfloat16, device=DEV)
    sh_b = torch.full((C, Rp), 7.0, dtype=torch.bfloat16, device=DEV)          # (stale values: the pad columns must come out zero)
    sums, ws = torch.zeros(2, device=DEV), torch.empty(1028, device=DEV)
    ops.adam2d_fused(p, g0, m, v, ws, sums, 1.0, 3e-4, sh_f, sh_b, **kw)
    q, qm, qv, rs, rf = p0.clone(), m0.clone(), v0.clone(), torch.zeros(2, device=DEV), torch.zeros_like(sh_f)
    ops.grad_sqnorm(g0, None, 0.0, rs)
    ops.clip_adam_step(q, g0, qm, qv, 0.0, rs, 1.0, 3e-4, p_bf16=rf)
    torch.cuda.synchronize()
    assert abs(float(sums[0]) - float(rs[0])) <= 2e-6 * float(rs[0]) and float(sums[0]) > 1.0
    for a, b in ((p, q), (m, qm), (v, qv)):
        assert (a - b).abs().max().item() <= 4e-6 * b.abs().max().item()
    assert torch.equal(sh_f, p.bfloat16())
    assert torch.equal(sh_b[:, :R], p.t().bfloat16()) and bool((sh_b[:, R:] == 0).all())
    if images:
        w16, w8 = torch.zeros_like(kw["p_f16"]), torch.zeros_like(kw["p_fp8"])
        ops.cast_f16(p, w16)
        ops.cast_fp8_lo(p, w8, hi_cols=C, scale_exp=19, hi_exp=8)
        assert torch.equal(kw["p_f16"], w16) and torch.equal(kw["p_fp8"], w8)


@pytest.mark.parametrize("B,F,C", [(320, 128, 2304), (260, 256, 1024), (36, 192, 8192)])
def test_dbof_cluster_tile_walk_equals_one_tile_per_workgroup(ops, B, F, C, monkeypatch):
    """Round 5: evc_dbof_cluster_pool_fwd walks several row tiles of one W_c column panel per workgroup (the next tile's first ring stages
    issued under the current tile's epilogue, the tape transposed through 4 KB per wave behind the ring) when there are >= 512 tiles.  Forced
    here at smaller shapes (EVC_DBOF_WALK=2) against the one-tile-per-workgroup kernel (EVC_DBOF_WALK=0): the same arithmetic in the same
    order, so the tape, the selected activations, the frame slots and the statistics partials must be IDENTICAL - ragged walks (40 row
    tiles over 16 walkers, 17 over 8), K of two, four and three stages, column panels that do not fill the last XCD."""
    S = 30
    rng = np.random.default_rng(B + C)
    Mp, P_in, P_cl = ops.dbof_workspace(B, S)
    rows = torch.from_numpy(ops.dbof_row_index(B, S).numpy().reshape(-1)).to(DEV)
    r_bn = torch.zeros((Mp, F), dtype=torch.bfloat16, device=DEV)
    r_bn[rows] = torch.from_numpy(rng.standard_normal((B * S, F)).astype(np.float32)).to(DEV).bfloat16()
    W = torch.from_numpy((rng.standard_normal((C, F)) / np.sqrt(F)).astype(np.float32)).to(DEV).bfloat16()
    ga = (1 + 0.3 * rng.standard_normal(C)).astype(np.float32)
    ga[::3] *= -1
    ga_d = torch.from_numpy(ga).to(DEV)
    outs = []
    for mode in ("2", "0", "2"):
        monkeypatch.setenv("EVC_DBOF_WALK", mode)
        act = torch.full((Mp, C), 7.0, dtype=torch.bfloat16, device=DEV)
        part = torch.full((P_cl, 2, C), float("nan"), device=DEV)
        xsel = torch.full((B, C), float("nan"), device=DEV)
        arg = torch.full((B, C), 255, dtype=torch.uint8, device=DEV)
        ops.dbof_cluster_pool_fwd(r_bn, W, B, S, F, C, ga_d, xsel, arg, act=act, part=part)
        xs2 = torch.full((B, C), float("nan"), device=DEV)
        ar2 = torch.full((B, C), 255, dtype=torch.uint8, device=DEV)
        ops.dbof_cluster_pool_fwd(r_bn, W, B, S, F, C, ga_d, xs2, ar2)              # evaluation form: no tape, no partials
        torch.cuda.synchronize()
        outs.append((act, part, xsel, arg, xs2, ar2))
    for a, b in ((outs[0], outs[1]), (outs[0], outs[2])):
        for name, x, y in zip(("act", "part", "xsel", "arg", "xsel (eval)", "arg (eval)"), a, b):
            assert torch.equal(x.view(torch.uint8) if x.dtype != torch.uint8 else x, y.view(torch.uint8) if y.dtype != torch.uint8 else y), name
    act, part, xsel, arg = outs[0][:4]
    ref = r_bn.float() @ W.float().t()                                             # the tape against a plain product of the same bf16 operands
    assert (act.float() - ref).abs().max().item() <= 2 ** -8 * ref.abs().max().item() + 1e-4
    assert torch.isfinite(xsel).all() and int(arg.max()) < S and torch.equal(outs[0][2], outs[0][4]) and torch.equal(outs[0][3], outs[0][5])


@pytest.mark.parametrize("B,S,F,C,u8", [(6, 8, 64, 128, False), (9, 30, 128, 320, True), (37, 30, 1152, 512, True)])
def test_dbof_fused_kernels_against_oracle(ops, B, S, F, C, u8):
    """csrc/evc_dbof.hip piece by piece (cs/frame_level_models.py:126-167, cs/model_utils.py:39-58,77-78): gather into the
    padded frame layout + column sums, input batch-norm, the cluster GEMM's statistics / max-pool epilogue (both signs of
    gamma), pool finish, the in-place max-pool/relu6/batch-norm backward, the slab TN product and the weight-gradient finish."""
    rng = np.random.default_rng(B * 1000 + C)
    T = 40
    q = rng.integers(0, 256, (B, T, F), dtype=np.uint8)
    n = rng.integers(1, T + 1, B).astype(np.int32)
    n[0] = T
    if B > 3:
        n[3] = 0                                             # an empty video: every sample is frame 0 = padding
    x = mm.dequantize(q.astype(np.float64)) * (np.arange(T)[None, :, None] < n[:, None, None])
    u = rng.random((B, S)).astype(np.float32)
    xin_d = torch.from_numpy(q).to(DEV) if u8 else torch.from_numpy(x.astype(np.float32)).to(DEV)
    nd, ud = torch.from_numpy(n).to(DEV), torch.from_numpy(u).to(DEV)
    Mp, P_in, P_cl = ops.dbof_workspace(B, S)
    assert Mp == (B + 3) // 4 * 128
    rows = ops.dbof_row_index(B, S).numpy()                   # [B, S] -> padded row
    assert len(set(rows.reshape(-1).tolist())) == B * S and rows.max() < Mp

    # ---- gather ----
    r = torch.full((Mp, F), float("nan"), device=DEV)
    idx = torch.empty((B, S), dtype=torch.int32, device=DEV)
    part = torch.empty((P_in, 2, F), device=DEV)
    ops.dbof_gather(xin_d, ud, nd, r, idx, part)
    ref_idx = mm.sample_random_frames_index(u, n)
    assert np.array_equal(idx.cpu().numpy(), ref_idx)        # int32 truncation, bit-exact
    g = mm.l2_normalize(x[np.arange(B)[:, None], np.clip(ref_idx, 0, T - 1)], 2)          # [B, S, F]
    rr = r.cpu().numpy()
    assert np.abs(rr[rows] - g).max() < 2e-6
    live = np.zeros(Mp, bool)
    live[rows.reshape(-1)] = True
    assert np.isnan(rr[~live]).all()                          # empty frame slots are neither written nor read
    ws = torch.empty(2 * F, dtype=torch.float64, device=DEV)
    ops.bn_partials_reduce(part, P_in, F, ws)
    g2 = g.reshape(-1, F)
    assert np.allclose(ws.cpu().numpy()[:F], g2.sum(0), atol=1e-4) and np.allclose(ws.cpu().numpy()[F:], (g2 ** 2).sum(0), atol=1e-4)
    mean, var = torch.empty(F, device=DEV), torch.empty(F, device=DEV)
    mov_m, mov_v = torch.zeros(F, device=DEV), torch.ones(F, device=DEV)
    ops.bn_finalize_ema(ws, B * S, F, mean, var, mov_m, mov_v)
    assert np.allclose(mean.cpu().numpy(), g2.mean(0), atol=1e-6) and np.allclose(var.cpu().numpy(), g2.var(0), atol=1e-7)
    assert np.allclose(mov_m.cpu().numpy(), 0.001 * g2.mean(0), atol=1e-8) and np.allclose(mov_v.cpu().numpy(), 1 - 0.001 * (1 - g2.var(0)), atol=1e-7)

    # ---- input batch-norm ----
    ga_in = (1 + 0.3 * rng.standard_normal(F)).astype(np.float32)
    be_in = (0.2 * rng.standard_normal(F)).astype(np.float32)
    r_bn = torch.full((Mp, F), 7.0, dtype=torch.bfloat16, device=DEV)
    xhat = torch.full((Mp, F), 7.0, dtype=torch.bfloat16, device=DEV)
    ops.dbof_input_bn_apply(r, B, S, F, mean, var, torch.from_numpy(ga_in).to(DEV), torch.from_numpy(be_in).to(DEV), r_bn, None, xhat)
    xh_ref = (g2 - g2.mean(0)) / np.sqrt(g2.var(0) + 1e-3)
    xh = xhat.float().cpu().numpy()
    rb = r_bn.float().cpu().numpy()
    assert np.abs(xh[rows].reshape(-1, F) - xh_ref).max() <= 2 ** -8 * np.abs(xh_ref).max() + 1e-6
    assert np.abs(rb[rows].reshape(-1, F) - (xh_ref * ga_in + be_in)).max() <= 2 ** -8 * (np.abs(xh_ref).max() * 1.9 + 1)
    assert not xh[~live].any() and not rb[~live].any()        # empty slots contribute nothing to the contractions

    # ---- cluster GEMM + statistics + selection (both gamma signs) ----
    W = (rng.standard_normal((C, F)) / np.sqrt(F)).astype(np.float32)
    Wd = torch.from_numpy(W).to(DEV).bfloat16()
    ga_cl = (1 + 0.3 * rng.standard_normal(C)).astype(np.float32)
    ga_cl[::3] *= -1                                          # negative scales select the MINIMUM over the frames
    be_cl = (0.5 * rng.standard_normal(C) + 1.0).astype(np.float32)
    ga_d, be_d = torch.from_numpy(ga_cl).to(DEV), torch.from_numpy(be_cl).to(DEV)
    act = torch.full((Mp, C), 7.0, dtype=torch.bfloat16, device=DEV)
    part_cl = torch.full((P_cl, 2, C), float("nan"), device=DEV)
    xsel = torch.empty((B, C), device=DEV)
    arg = torch.empty((B, C), dtype=torch.uint8, device=DEV)
    ops.dbof_cluster_pool_fwd(r_bn, Wd, B, S, F, C, ga_d, xsel, arg, act=act, part=part_cl)
    a_ref = rb.astype(np.float64) @ Wd.float().cpu().numpy().astype(np.float64).T                # exact product of the bf16 operands
    a_live = a_ref[rows]                                                                         # [B, S, C]
    got_act = act.float().cpu().numpy()
    assert np.abs(got_act - a_ref).max() <= 2 ** -8 * np.abs(a_ref).max() + 1e-5
    wsc = torch.empty(2 * C, dtype=torch.float64, device=DEV)
    ops.bn_partials_reduce(part_cl, P_cl, C, wsc)
    assert np.allclose(wsc.cpu().numpy()[:C], a_live.sum((0, 1)), atol=2e-3) and np.allclose(wsc.cpu().numpy()[C:], (a_live ** 2).sum((0, 1)), rtol=1e-5, atol=2e-3)
    sgn = np.where(ga_cl >= 0, 1.0, -1.0)
    sel_ref = (a_live * sgn).max(1) * sgn                                                        # max for gamma >= 0, min otherwise
    xs = xsel.cpu().numpy()
    assert np.abs(xs - sel_ref).max() < 2e-5 * max(1.0, np.abs(sel_ref).max())
    ar = arg.cpu().numpy().astype(np.int64)
    assert ar.max() < S
    picked = np.take_along_axis(a_live, ar[:, None, :], 1)[:, 0, :]
    assert np.abs(picked - sel_ref).max() < 2e-5 * max(1.0, np.abs(sel_ref).max())               # the slot holds the selected value
    mean_c, var_c = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    ops.bn_finalize_ema(wsc, B * S, C, mean_c, var_c)
    a2 = a_live.reshape(-1, C)
    assert np.allclose(mean_c.cpu().numpy(), a2.mean(0), atol=1e-5) and np.allclose(var_c.cpu().numpy(), a2.var(0), rtol=1e-4, atol=1e-6)
    # evaluation form: nothing kept, no statistics - same selection
    xsel2, arg2 = torch.empty_like(xsel), torch.empty_like(arg)
    ops.dbof_cluster_pool_fwd(r_bn, Wd, B, S, F, C, ga_d, xsel2, arg2)
    assert torch.equal(xsel2, xsel) and torch.equal(arg2, arg)

    # ---- pooled = relu6(bn(selected)) = max over frames of relu6(bn(act)) ----
    pooled = torch.empty((B, C), device=DEV)
    pooled_bf = torch.empty((B, C), dtype=torch.bfloat16, device=DEV)
    ops.dbof_pool_finish(xsel, B, C, mean_c, var_c, ga_d, be_d, pooled, pooled_bf)
    mu, rstd = a2.mean(0), 1 / np.sqrt(a2.var(0) + 1e-3)
    y = mm.relu6((a_live - mu) * rstd * ga_cl + be_cl)
    assert np.abs(pooled.cpu().numpy() - y.max(1)).max() < 1e-4
    assert torch.equal(pooled_bf, pooled.bfloat16())

    # ---- backward: d(act) in place ----
    dpooled = rng.standard_normal((B, C)).astype(np.float32)
    dp_d = torch.from_numpy(dpooled).to(DEV)
    wsb = torch.empty(2 * C, dtype=torch.float64, device=DEV)
    ops.bn_bwd_partial(xsel, dp_d, B, C, mean_c, var_c, ga_d, be_d, True, wsb)
    pl = pooled.cpu().numpy()
    dmask = dpooled * ((pl > 0) & (pl < 6))
    xh_sel = (xs - mu) * rstd
    assert np.allclose(wsb.cpu().numpy()[:C], dmask.sum(0), atol=1e-4) and np.allclose(wsb.cpu().numpy()[C:], (dmask * xh_sel).sum(0), atol=1e-3)
    dgam, dbet = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    ops.dbof_dact(act, dp_d, pooled, arg, mean_c, var_c, ga_d, wsb, B * S, B, S, C, dgam, dbet)
    d_full = np.zeros((B, S, C))
    np.put_along_axis(d_full, ar[:, None, :], dmask[:, None, :], 1)
    xh_act = (got_act[rows] - mu) * rstd                       # the kernel reads the bf16 activation it stored
    R = B * S
    dact_ref = ga_cl * rstd * (d_full - dmask.sum(0) / R - xh_act * (dmask * xh_sel).sum(0) / R)
    dact = act.float().cpu().numpy()
    assert np.abs(dact[rows] - dact_ref).max() <= 2 ** -8 * np.abs(dact_ref).max() + 1e-6
    assert not dact[~live].any()
    assert np.allclose(dbet.cpu().numpy(), dmask.sum(0), atol=1e-4) and np.allclose(dgam.cpu().numpy(), (dmask * xh_sel).sum(0), atol=1e-3)

    # ---- G = dact^T . xhat in slabs, then dWc / dgamma_in ----
    G_ref = dact.astype(np.float64).T @ xh.astype(np.float64)
    Wm = torch.from_numpy(W).to(DEV)
    for nslab in (1, 3):
        if Mp // 32 < nslab * 2:
            continue
        slabs = torch.full((nslab, C, F), float("nan"), device=DEV)
        ops.gemm_tn_slabs(act, xhat, C, F, Mp, slabs, nslab)
        assert np.abs(slabs.sum(0).cpu().numpy() - G_ref).max() <= 1e-4 * np.abs(G_ref).max() + 1e-5
        dW, dg_in, db_in = torch.empty((C, F), device=DEV), torch.full((F,), 9.0, device=DEV), torch.full((F,), 9.0, device=DEV)
        ops.dbof_wgrad_finish(slabs, nslab, C, F, Wm, torch.from_numpy(ga_in).to(DEV), dW, dg_in, db_in)
        assert np.abs(dW.cpu().numpy() - ga_in * G_ref).max() <= 1e-4 * np.abs(G_ref).max() * 2 + 1e-5
        assert np.abs(dg_in.cpu().numpy() - (W * G_ref).sum(0)).max() <= 1e-4 * np.abs((W * G_ref).sum(0)).max() + 1e-4
        assert not db_in.cpu().numpy().any()
    with pytest.raises(Exception, match="at most 32"):
        ops.dbof_workspace(B, 33)


NT_STORE_WORKER = r'''
import sys, numpy as np, torch
sys.path.insert(0, %(root)r)
from efficientvideoclassification_youtube8m_amd import ops
torch.manual_seed(0)
dev = "cuda:0"
worst = 0.0
for (M, N, K) in ((512, 512, 128), (777, 1000, 192), (300, 264, 64), (2000, 72, 256), (256, 4096, 1024)):
    A = (torch.randn(M, K, device=dev) * 0.5).bfloat16()
    B = (torch.randn(N, K, device=dev) * 0.5).bfloat16()
    bias = torch.randn(N, device=dev)
    ref = A.double() @ B.double().t()
    for out_dtype in (torch.float32, torch.bfloat16):
        for use_bias in (False, True):
            # row stride: the natural one, and one that breaks the 16-byte row alignment (element-wise fallback)
            for ld in (N, N + 1):
                buf = torch.full((M, ld), 7.0, dtype=out_dtype, device=dev)
                ops.gemm_nt(A, B, M, N, K, buf, bias=bias if use_bias else None, ldc=ld)
                want = ref + (bias.double() if use_bias else 0.0)
                got = buf[:, :N].double()
                tol = (2 ** -8 if out_dtype == torch.bfloat16 else 1e-5) * want.abs().max().item() + 1e-4
                err = (got - want).abs().max().item()
                assert err <= tol, (M, N, K, str(out_dtype), use_bias, ld, err, tol)
                if ld > N:
                    assert bool((buf[:, N:] == 7.0).all()), "wrote outside the N columns"
                worst = max(worst, err)
    acc = torch.randn(M, N, device=dev)
    want = acc.double() + ref
    ops.gemm_nt(A, B, M, N, K, acc, accumulate=True)
    assert (acc.double() - want).abs().max().item() <= 1e-5 * want.abs().max().item() + 1e-4
print("ok", worst)
'''


@pytest.mark.parametrize("tile", ["0", "1", "4", "5", "6", "7"])
def test_gemm_nt_ring_tile_store_paths(tile):
    """The ring-tile NT kernels store a plain overwrite of C through a per-wave LDS transpose (whole rows of the sub-tile, 16
    bytes per lane) and fall back to element-wise stores for split-K / accumulate / unaligned rows / the ragged right edge:
    f32 and bf16 outputs, bias, ragged M and N, odd row strides, on the 256x256 (EVC_FORCE_TILE=1), 224x256 (=4), 128x128 (=5), 320x256 (=6), 160x128 (=7: both 128-column tiles on the 64-wide K stages of gemm_core_v3.h) and
    automatically chosen (=0: also the 256x64 batch-row form) tiles.  One process per forced tile (the choice is read once)."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("EVC_FORCE_TILE", None)
    if tile != "0":
        env["EVC_FORCE_TILE"] = tile
    r = subprocess.run([sys.executable, "-c", NT_STORE_WORKER % {"root": root}], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.parametrize("tile", ["1", "2", "3", "4", "5", "6", "7", "8", "9", "10", "11"])
def test_lstm_steps_on_every_ring_tile(tile):  # (BPTT: 7 -> the 64 x 64 ring tile of gemm_core_v3.h)
    """The fused LSTM step kernels on every ring-tile height (EVC_FORCE_TILE pins the choice: forward 1 -> 256 rows, 4 -> 320,
    5 -> 288, 6 -> 224, 7 -> 192, 8 -> 160, 9 -> 128, 10 -> 64, 11 -> 240 = 7 + 8 row fragments on the two wave rows; BPTT 1 -> 192, 2 -> 160, 3 -> 128) against the oracle - the
    160 / 224 / 288-row tiles have surplus staging lanes (dummy LDS sink), and the forward loop stages through four producer
    waves.  One process per tile (the choice is read once per process)."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, EVC_FORCE_TILE=tile)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_kernels.py"), "-x", "-q", "-m", "gpu", "-k",
                        "(test_lstm_layer_fwd_and_bwd and (1536 or 640 or 200)) or test_lstm_layer_with_row_plan_matches_plain "
                        "or (test_lstm_layer_fwd_f16 and (1536 or 640 or 200))"],
                       env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
