"""Thin torch-tensor wrappers over the C ABI (one call per kernel family).

Tensors are only containers for device memory here: every wrapper extracts raw
device pointers and enqueues on torch's current HIP stream.  No wrapper has a
CPU or eager-PyTorch fallback; CPU tensors are rejected.
"""
from __future__ import annotations

import ctypes as C

import os

import torch

from . import _lib

BF16 = torch.bfloat16
F16 = torch.float16
F32 = torch.float32


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.EvcError("evc ops need device tensors (got a CPU tensor); there is no CPU path")
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


MARKS = None     # set to a list to collect (name, stream handle, timing event) at the engine's mark() points (scripts/step_timeline.py)


def mark(name):
    """Timeline aid: a timing event on the current stream, kept in ops.MARKS when that is a list (else nothing happens)."""
    if MARKS is not None:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        MARKS.append((name, torch.cuda.current_stream().cuda_stream, ev))


def round_up(x, m):
    return (x + m - 1) // m * m


def check_device(dev=0):
    _lib.call("evc_check_device", dev)


# ---------------------------------------------------------------------------
def gemm_nt(A, B, M, N, K, out, bias=None, accumulate=False, lda=None, ldb=None, ldc=None):
    """out[M,N] (+)= A[M,K] @ B[N,K]^T (+ bias).  A, B bf16 K-contiguous."""
    assert A.dtype == BF16 and B.dtype == BF16
    lda = A.stride(0) if lda is None else lda
    ldb = B.stride(0) if ldb is None else ldb
    ldc = out.stride(0) if ldc is None else ldc
    _lib.call("evc_gemm_nt", _p(A), lda, _p(B), ldb, _p(out), ldc, M, N, K, _p(bias),
              1 if out.dtype == BF16 else 0, 1 if accumulate else 0, _stream())
    return out


def gemm_kn(A, B, M, N, K, out, A2=None, B2=None, K2=0, bias=None, accumulate=False, splits=0, b_rows=0, b_rows2=0, lda=None, ldb=None, ldc=None):
    """out[M,N] (+)= A[M,K] @ B[K,N] (+ A2[M,K2] @ B2[K2,N]) (+ bias): B bf16 with the CONTRACTION index as its row (evc_gemm_kn; M <= 256).
    b_rows (0: K): the rows B really has - the rows up to K are read as its last row, A's columns there must be zero.  splits: 0 = by shape
    (gemm_kn_splits), else forced."""
    assert A.dtype == BF16 and B.dtype == BF16 and (A2 is None) == (B2 is None) == (K2 == 0)
    _lib.call("evc_gemm_kn", _p(A), A.stride(0) if lda is None else lda, _p(B), B.stride(0) if ldb is None else ldb, K, b_rows,
              _p(A2), A2.stride(0) if A2 is not None else 0, _p(B2), B2.stride(0) if B2 is not None else 0, K2, b_rows2,
              _p(out), out.stride(0) if ldc is None else ldc, M, N, _p(bias), 1 if out.dtype == BF16 else 0, 1 if accumulate else 0, splits, _stream())
    return out


def gemm_kn_splits(N, K, K2=0, out_bf16=False):
    """K splits evc_gemm_kn takes by itself for this shape in this process (no GPU needed)."""
    s = C.c_int(0)
    _lib.call("evc_gemm_kn_plan", N, K, K2, 1 if out_bf16 else 0, C.byref(s))
    return s.value


def _slab_rows_arg(live_rows, K):
    """(slab_rows, nslabs, host int32 array) of evc_gemm_tn2_rows from live_rows = (rows per slab [T], rows of one slab)."""
    rows, slab = live_rows
    assert slab % 32 == 0 and K == slab * len(rows), (K, slab, len(rows))
    return slab, len(rows), (C.c_int32 * len(rows))(*[int(r) for r in rows])


def gemm_nt_sqnorm(A, B, M, N, K, out, p, l2_coeff, sums, ws=None):
    """out [M,N] f32 = A[M,K] @ B[N,K]^T and sums[0] += |out + l2_coeff * p|^2 from the same pass (evc_gemm_nt_sqnorm; p laid out as out, or None with
    l2_coeff 0; sums zeroed by the caller; ws: gemm_nt_sqnorm_ws(M, N) floats of scratch - per-wave partials summed in index order, no atomics)."""
    assert A.dtype == BF16 and B.dtype == BF16 and out.dtype == F32 and out.is_contiguous() and (p is None or (p.dtype == F32 and p.shape == out.shape and p.is_contiguous()))
    need = gemm_nt_sqnorm_ws(M, N)
    if ws is None:                      # (callers on several streams keep their own: engine.MoeHead.sq_part)
        ws = torch.empty(need, dtype=F32, device=out.device)
    assert ws.dtype == F32 and ws.numel() >= need and ws.is_contiguous()
    _lib.call("evc_gemm_nt_sqnorm", _p(A), A.stride(0), _p(B), B.stride(0), _p(out), out.stride(0), M, N, K, _p(p), float(l2_coeff), _p(sums), _p(ws), ws.numel(),
              _stream())
    return out


def gemm_nt_sqnorm_ws(M, N):
    """Floats of scratch evc_gemm_nt_sqnorm needs: one {|C + l2 P|^2, |P|^2} slot per wave of every tile."""
    return 16 * ((M + 127) // 128) * ((N + 127) // 128)


def gemm_nt_sqnorm_ok(M, N, K):
    """Shapes evc_gemm_nt_sqnorm takes (one pass of ring tiles storing whole rows) - and whether to use it: OFF unless EVC_FUSED_GRAD_NORM=1.  Measured on
    cfg 5 (the one configuration that materialises its MoE gradient), same box, alternating (profiles/r06_fused_grad_norm_ab.txt): 3.72-3.75 ms per step
    with the norm from the product's stores against 3.61-3.63 with the separate evc_grad_sqnorm pass - reading P and squaring in the store epilogue costs
    the two products more than the 0.19 ms pass it removes (with same-address atomics instead of per-wave partials: 3.95)."""
    return M > 512 and N % 256 == 0 and K % 64 == 0 and K < 8192 and os.environ.get("EVC_FUSED_GRAD_NORM", "0") == "1"


def _tn_rows_args(live_rows, K, k_skip):
    """(slab_rows, nslabs, rows table or None) of evc_gemm_tn2_rows_skip / evc_gemm_tn_plan: the live-row table, or K rows as one plain walk."""
    if live_rows is not None:
        return _slab_rows_arg(live_rows, K)
    return K, 1, None


def gemm_tn_plan(M, N1, K, lda, ldb1, N2=0, ldb2=0, live_rows=None, k_skip=0):
    """(tile, splits, live_walk) that gemm_tn / gemm_tn2 would launch with for these shapes (evc_gemm_tn_plan: the launch's own choice, nothing
    enqueued).  splits == 1: the launch stores each element of its columns once - accumulate=False needs no zeroed `out`.  live_walk: the K walk
    follows live_rows and reads no dead row from the next multiple of 32 on."""
    slab, ns, arr = _tn_rows_args(live_rows, K, k_skip)
    tile, splits, walk = C.c_int(0), C.c_int(0), C.c_int(0)
    _lib.call("evc_gemm_tn_plan", lda, ldb1, N1, ldb2, N2, M, slab, ns, arr, k_skip, C.byref(tile), C.byref(splits), C.byref(walk))
    return tile.value, splits.value, bool(walk.value)


def gemm_tn(A, B, M, N, K, out, row_interleave_H=0, accumulate=False, lda=None, ldb=None, ldc=None, live_rows=None, k_skip=0):
    """out[M,N] (+)= A[K,M]^T @ B[K,N] (both row-major over K), f32 out.  live_rows = (rows [T], slab_rows): K = T slabs of slab_rows rows
    of which the first rows[t] are live (a row-planned level) - the dead rows are skipped (evc_gemm_tn2_rows).  k_skip: the first k_skip * 32
    rows of B are zeros and are not walked (evc_gemm_tn2_rows_skip)."""
    assert A.dtype == BF16 and B.dtype == BF16 and out.dtype == F32
    lda, ldb, ldc = A.stride(0) if lda is None else lda, B.stride(0) if ldb is None else ldb, out.stride(0) if ldc is None else ldc
    if k_skip:
        slab, ns, arr = _tn_rows_args(live_rows, K, k_skip)
        _lib.call("evc_gemm_tn2_rows_skip", _p(A), lda, _p(B), ldb, N, None, 0, 0, 0, _p(out), ldc, M, slab, ns, arr, k_skip, row_interleave_H,
                  1 if accumulate else 0, _stream())
        return out
    if live_rows is not None:
        slab, ns, arr = _slab_rows_arg(live_rows, K)
        _lib.call("evc_gemm_tn2_rows", _p(A), lda, _p(B), ldb, N, None, 0, 0, 0, _p(out), ldc, M, slab, ns, arr, row_interleave_H, 1 if accumulate else 0, _stream())
        return out
    _lib.call("evc_gemm_tn", _p(A), lda, _p(B), ldb, _p(out), ldc, M, N, K, row_interleave_H, 1 if accumulate else 0, _stream())
    return out


def gemm_tn_det(A, B, M, N, K, out, row_interleave_H=0, accumulate=False, ldc=None, B2=None, N2=0, c_col2=None, k_skip=0):
    """out[:, :N] (and out[:, c_col2:c_col2+N2] from B2) (+)= A^T @ B without atomics and with the K split kept (EVC_DETERMINISTIC=1): partial
    products into slabs (evc_gemm_tn2_slabs), added in slab order (evc_sum_slabs).  Scratch from the stream-aware caching allocator.
    k_skip: the first k_skip * 32 rows of the last segment (B2, or B) are zeros and are not walked (evc_gemm_tn2_slabs_skip: same slabs, same bits)."""
    assert A.dtype == BF16 and B.dtype == BF16 and out.dtype == F32
    ldc = out.stride(0) if ldc is None else ldc
    ntot = (c_col2 + N2) if B2 is not None else N
    tiles = ((M + 255) // 256) * ((N + N2 + 255) // 256)
    nslab = max(1, min(256 // max(1, tiles), K // 1024))
    while nslab > 1 and ((K // 32 + nslab - 1) // nslab) * (nslab - 1) >= K // 32:
        nslab -= 1
    ws = torch.empty((nslab, M, ntot), dtype=F32, device=out.device)
    args = (_p(A), A.stride(0), _p(B), B.stride(0), N, _p(B2), B2.stride(0) if B2 is not None else 0, N2,
            (c_col2 if c_col2 is not None else N), _p(ws), ntot, M * ntot, M, K)
    if k_skip:
        _lib.call("evc_gemm_tn2_slabs_skip", *args, k_skip, row_interleave_H, nslab, _stream())
    else:
        _lib.call("evc_gemm_tn2_slabs", *args, row_interleave_H, nslab, _stream())
    for c0, w in ((0, N),) + (((c_col2, N2),) if B2 is not None else ()):
        _lib.call("evc_sum_slabs", _p(ws[0, :, c0:]), M * ntot, nslab, M, w, ntot, _p(out[:, c0:]), ldc, 1 if accumulate else 0, _stream())
    return out


def gemm_tn2(A, B1, N1, B2, N2, M, K, out, row_interleave_H=0, accumulate=False, ldc=None, c_col2=None, live_rows=None, k_skip=0):
    """out[:, :N1] (+)= A[K,M]^T @ B1[K,N1], out[:, c_col2:c_col2+N2] (+)= A^T @ B2[K,N2] in one launch (N1 % 256 == 0;
    c_col2 defaults to N1: adjacent segments).  live_rows: as in gemm_tn.  k_skip: the first k_skip * 32 rows of B2 are zeros and are not
    walked (evc_gemm_tn2_rows_skip)."""
    assert A.dtype == BF16 and B1.dtype == BF16 and B2.dtype == BF16 and out.dtype == F32
    ldc, c_col2 = out.stride(0) if ldc is None else ldc, N1 if c_col2 is None else c_col2
    if k_skip:
        slab, ns, arr = _tn_rows_args(live_rows, K, k_skip)
        _lib.call("evc_gemm_tn2_rows_skip", _p(A), A.stride(0), _p(B1), B1.stride(0), N1, _p(B2), B2.stride(0), N2, c_col2, _p(out), ldc, M, slab, ns, arr, k_skip,
                  row_interleave_H, 1 if accumulate else 0, _stream())
        return out
    if live_rows is not None:
        slab, ns, arr = _slab_rows_arg(live_rows, K)
        _lib.call("evc_gemm_tn2_rows", _p(A), A.stride(0), _p(B1), B1.stride(0), N1, _p(B2), B2.stride(0), N2, c_col2,
                  _p(out), ldc, M, slab, ns, arr, row_interleave_H, 1 if accumulate else 0, _stream())
        return out
    _lib.call("evc_gemm_tn2", _p(A), A.stride(0), _p(B1), B1.stride(0), N1, _p(B2), B2.stride(0), N2, c_col2,
              _p(out), ldc, M, K, row_interleave_H, 1 if accumulate else 0, _stream())
    return out


def fill_f32(t, value):
    """Contiguous f32 fill (one streaming kernel; hipMemset2D on a pitched view is several times slower)."""
    assert t.dtype == F32 and t.is_contiguous()
    _lib.call("evc_fill_f32", _p(t), t.numel(), float(value), _stream())


def fill_f32_cols(t, value):
    """Fill of a column range t = m[:, c0:c1] of a row-major f32 matrix, in one kernel (evc_fill_f32_cols)."""
    assert t.dtype == F32 and t.dim() == 2 and t.stride(1) == 1
    _lib.call("evc_fill_f32_cols", _p(t), t.stride(0), t.shape[0], t.shape[1], float(value), _stream())


class _Once:
    """bool() of a question asked of the loaded library, on first use (importing this module must not load the library)."""

    def __init__(self, ask):
        self.ask, self.v = ask, None

    def __bool__(self):
        if self.v is None:
            self.v = bool(self.ask())
        return self.v


# the TN products' plan query, skip entries and column fill: missing only from a library of an older tree named by EVC_LIB (_lib.NEWER)
TN_PLAN = _Once(lambda: _lib.has("evc_gemm_tn_plan"))
GEMM_KN = _Once(lambda: _lib.has("evc_gemm_kn"))      # the K-major-B product (the MoE head's dX from the forward weight image), likewise

DETERMINISTIC = os.environ.get("EVC_DETERMINISTIC", "0") not in ("", "0")     # (the library reads the same variable: csrc/evc_common.h)


def colsum_bf16(x, R, C, out, deinterleave_H=0):
    if DETERMINISTIC and R >= 128:      # no atomics: partial rows + a fixed-order finish (evc_colsum_bf16_det)
        # (workspace from the caching allocator, which is stream-aware: the two towers call this concurrently on two streams)
        ws = torch.empty((128, C), dtype=F32, device=x.device)
        _lib.call("evc_colsum_bf16_det", _p(x), x.stride(0), R, C, deinterleave_H, _p(out), _p(ws), 128, _stream())
        return out
    _lib.call("evc_colsum_bf16", _p(x), x.stride(0), R, C, deinterleave_H, _p(out), _stream())
    return out


def transpose_to_bf16(x, R, C, out, Rpad, ld_in=None, interleave_H=0):
    """out[c][r] = x[r][c]; out is [C, >=Rpad] bf16 with columns [R,Rpad) zeroed.
    interleave_H: write input row g*H+u to output column u*4+g (gate-interleaved K order)."""
    ld_in = x.stride(0) if ld_in is None else ld_in
    _lib.call("evc_transpose_to_bf16", _p(x), 1 if x.dtype == F32 else 0, ld_in, R, C, _p(out), out.stride(0), Rpad,
              interleave_H, _stream())
    return out


def cast_bf16(x, out=None):
    x2 = x.reshape(-1, x.shape[-1]) if x.dim() > 1 else x.reshape(1, -1)
    if out is None:
        out = torch.empty(x.shape, dtype=BF16, device=x.device)
    o2 = out.reshape(x2.shape)
    _lib.call("evc_cast_f32_to_bf16", _p(x2), x2.stride(0), x2.shape[0], x2.shape[1], _p(o2), o2.stride(0), _stream())
    return out


def cast_f16(x, out):
    """out = f16(x), round to nearest even, for a 2-D f32 tensor (the f16 weight shadows of lstm_layer_fwd_f16)."""
    assert x.dtype == F32 and out.dtype == F16 and x.dim() == 2
    _lib.call("evc_cast_f32_to_f16", _p(x), x.stride(0), x.shape[0], x.shape[1], _p(out), out.stride(0), _stream())
    return out


def cast_f16_wide(w, Kin, H, nseg, out, h_ext=False):
    """f16 image of an LSTM kernel w [R][Kin+H] f32 for K-extended operands: out [R][nseg*Kin + (2 if h_ext else 1)*H] =
    [f16(Wx) | f16(Wx)/64 | (Wx - f16(Wx))*64 | f16(Wh) | (Wh - f16(Wh))*64] (first nseg x blocks; the last block with h_ext)."""
    assert w.dtype == F32 and out.dtype == F16 and w.shape[1] == Kin + H and out.is_contiguous()
    assert out.shape == (w.shape[0], nseg * Kin + (2 if h_ext else 1) * H)
    _lib.call("evc_cast_f32_to_f16_wide", _p(w), w.stride(0), w.shape[0], Kin, H, nseg, 1 if h_ext else 0, _p(out), _stream())
    return out


def cast_f16_segs(x, nseg, out):
    """K-extended f16 image of a 2-D f32 activation matrix: out [R][nseg*C] = [f16(x) | (x - f16(x))*64 | f16(x)/64] (first nseg)."""
    assert x.dtype == F32 and out.dtype == F16 and out.shape == (x.shape[0], nseg * x.shape[1]) and out.is_contiguous()
    _lib.call("evc_cast_f32_to_f16_segs", _p(x), x.stride(0), x.shape[0], x.shape[1], nseg, _p(out), _stream())
    return out


def cast_f16_wlo(w, Kin, H, out):
    """f16 image of an LSTM kernel w [R][Kin+H] f32 with both parts K-extended by the weights' low-order halves:
    out [R][2Kin + 2H] = [f16(Wx) | (Wx - f16(Wx))*64 | f16(Wh) | (Wh - f16(Wh))*64] (upper layer of lstm_stack2_fwd_f16)."""
    assert w.dtype == F32 and out.dtype == F16 and w.shape[1] == Kin + H and out.shape == (w.shape[0], 2 * (Kin + H)) and out.is_contiguous()
    _lib.call("evc_cast_f32_to_f16_wlo", _p(w), w.stride(0), w.shape[0], Kin, H, _p(out), _stream())
    return out


FP8_W_SCALE_EXP = 17       # e4m3((W - f16(W)) * 2^17): |W| < 4 never clamps, weights above ~2^-13 keep 3-4 bits of their low-order half
FP8_WX_HI_EXP = 6          # e4m3(Wx * 2^6) against e4m3((x - f16(x)) * 2^18): the same 2^24 as 2^7 * 2^17


def cast_fp8_lo(w, out, hi_cols=0, scale_exp=FP8_W_SCALE_EXP, hi_exp=FP8_WX_HI_EXP, hi_tail=False):
    """out uint8 = e4m3(clamp((w - f16(w)) * 2^scale_exp)): the low-order halves of a weight matrix next to its f16 image (the wT8 operand of
    lstm_layer_fwd_f16_fp8lo).  hi_cols > 0: out [R][C + hi_cols] = [lo(W[:, :hi_cols]) | e4m3(W[:, :hi_cols] * 2^hi_exp) | lo(W[:, hi_cols:])] -
    the layer that reads the input frames contracts the input's low-order half against the full-value image.
    hi_tail (round 6): EVERY column gets its full-value image - out [R][2C] = [lo(A) | hi(A) | lo(B) | hi(B)], A = W[:, :hi_cols], B = the rest
    (evc_cast_f32_to_fp8_lohi: the weight rows of the h_lo forms, whose activations' low-order halves are corrected too)."""
    assert w.dtype == F32 and out.dtype == torch.uint8 and w.dim() == 2
    if hi_tail:
        assert out.shape == (w.shape[0], 2 * w.shape[1])
        _lib.call("evc_cast_f32_to_fp8_lohi", _p(w), w.stride(0), w.shape[0], w.shape[1], scale_exp, hi_cols, hi_exp, _p(out), out.stride(0), _stream())
        return out
    assert out.shape == (w.shape[0], w.shape[1] + hi_cols)
    _lib.call("evc_cast_f32_to_fp8_lo", _p(w), w.stride(0), w.shape[0], w.shape[1], scale_exp, hi_cols, hi_exp, _p(out), out.stride(0), _stream())
    return out


FP8_MOE = dict(x_hi_exp=6, x_lo_exp=17, w_lo_exp=18, w_hi_exp=7)     # e4m3 scales of the "high" MoE head: |state| < 7, |W| < 3.5 never clamp; 6 + 18 = 17 + 7 = 24


AMAX_SLOTS = 64     # EVC_AMAX_SLOTS (csrc/evc_common.h)


def absmax_partials(x, ws):
    """ws [64] f32 = partial maxima of |x| over a 2-D f32 tensor (evc_absmax_partials: plain stores, nothing to zero)."""
    assert x.dtype == F32 and x.dim() == 2 and ws.dtype == F32 and ws.numel() == AMAX_SLOTS and ws.is_contiguous()
    _lib.call("evc_absmax_partials", _p(x), x.stride(0), x.shape[0], x.shape[1], _p(ws), _stream())
    return ws


def cast_f16_fp8x(x, out, hi_exp=FP8_MOE["x_hi_exp"], lo_exp=FP8_MOE["x_lo_exp"], amax_ws=None):
    """out [R][2C] f16 containers = rows [f16(x) | e4m3(x 2^hi_exp) (C bytes) | e4m3((x - f16(x)) 2^lo_exp) (C bytes)]: the A operands of gemm_nt_f16_fp8.
    amax_ws (absmax_partials(x)): dynamic range - both e4m3 images are shifted down by the d bits the largest |x| needs to stay below 448
    (evc_cast_f32_to_f16_fp8x_dyn; gemm_nt_f16_fp8 takes the same amax_ws / hi_exp and scales its products back up)."""
    assert x.dtype == F32 and x.dim() == 2 and out.dtype == F16 and out.shape == (x.shape[0], 2 * x.shape[1]) and out.is_contiguous()
    if amax_ws is not None:
        _lib.call("evc_cast_f32_to_f16_fp8x_dyn", _p(x), x.stride(0), x.shape[0], x.shape[1], hi_exp, lo_exp, _p(amax_ws), _p(out), _stream())
        return out
    _lib.call("evc_cast_f32_to_f16_fp8x", _p(x), x.stride(0), x.shape[0], x.shape[1], hi_exp, lo_exp, _p(out), _stream())
    return out


def gemm_nt_f16_fp8(a_rows, w16, w8, M, N, K, out, bias=None, scale_exp=-24, amax_ws=None, a_hi_exp=FP8_MOE["x_hi_exp"]):
    """out [M][N] f32 = f16(x) . f16(W)^T + 2^scale_exp [e4m3(x ..) | e4m3(x_lo ..)] . w8^T (+ bias): a_rows [M][2K] from cast_f16_fp8x, w16 [N][K]
    f16, w8 [N][2K] uint8 = [e4m3(W_lo ..) | e4m3(W ..)] (evc_gemm_nt_f16_fp8: the "high" precision MoE head).  amax_ws / a_hi_exp: what
    cast_f16_fp8x(amax_ws=...) wrote a_rows with (evc_gemm_nt_f16_fp8_dyn)."""
    assert a_rows.dtype == F16 and a_rows.shape == (M, 2 * K) and w16.dtype == F16 and w16.shape == (N, K) and w8.dtype == torch.uint8 and w8.shape == (N, 2 * K)
    assert out.dtype == F32 and a_rows.is_contiguous() and w16.is_contiguous() and w8.is_contiguous()
    if amax_ws is not None:
        _lib.call("evc_gemm_nt_f16_fp8_dyn", _p(a_rows), 2 * K, a_rows.data_ptr() + 2 * K, 4 * K, _p(w16), K, _p(w8), 2 * K, _p(out), out.stride(0),
                  M, N, K, 2 * K, scale_exp, _p(amax_ws), a_hi_exp, _p(bias), _stream())
        return out
    _lib.call("evc_gemm_nt_f16_fp8", _p(a_rows), 2 * K, a_rows.data_ptr() + 2 * K, 4 * K, _p(w16), K, _p(w8), 2 * K, _p(out), out.stride(0),
              M, N, K, 2 * K, scale_exp, _p(bias), _stream())
    return out


def cast_bf16_wide(x, out, lo_first):
    """Wide split-bf16 image of a 2-D f32 tensor: out rows [lo | hi] (lo_first: the A operand of gemm_nt_split_wide) or
    [hi | lo] (its B operand)."""
    R, Cc = x.shape
    assert x.dtype == F32 and out.dtype == BF16 and out.shape[0] == R and out.shape[1] >= 2 * Cc
    _lib.call("evc_cast_f32_to_bf16_wide", _p(x), x.stride(0), R, Cc, _p(out), out.stride(0), 1 if lo_first else 0, _stream())
    return out


def gemm_nt_split_wide(A_lohi, B_hilo, M, N, K, out, bias=None):
    """out[M,N] f32 = (A_hi + A_lo) @ (B_hi + B_lo)^T (+ bias) to ~2^-16 as ONE K-extended launch (evc_gemm_nt_split):
    A_lohi rows [lo(K) | hi(K)], B_hilo rows [hi(K) | lo(K)]."""
    assert A_lohi.dtype == BF16 and B_hilo.dtype == BF16 and out.dtype == F32
    _lib.call("evc_gemm_nt_split", _p(A_lohi), A_lohi.stride(0), _p(B_hilo), B_hilo.stride(0), _p(out), out.stride(0), M, N, K,
              _p(bias), _stream())
    return out


def cast_bf16_split(x, hi, lo):
    """hi = bf16(x), lo = bf16(x - hi) for a 2-D f32 tensor (split-bf16 operands)."""
    R, Cc = x.shape
    _lib.call("evc_cast_f32_to_bf16_split", _p(x), x.stride(0), R, Cc, _p(hi), _p(lo), hi.stride(0), _stream())
    return hi, lo


def gemm_nt_split(A_hi, A_lo, B_hi, B_lo, M, N, K, out, bias=None):
    """out = (A_hi + A_lo) @ (B_hi + B_lo)^T to ~2^-16: hi.hi + hi.lo + lo.hi (the lo.lo term is below f32 noise)."""
    gemm_nt(A_hi, B_hi, M, N, K, out, bias=bias)
    gemm_nt(A_hi, B_lo, M, N, K, out, accumulate=True)
    gemm_nt(A_lo, B_hi, M, N, K, out, accumulate=True)
    return out


def rowsum_bf16(x, R, C, out):
    _lib.call("evc_rowsum_bf16", _p(x), x.stride(0), R, C, _p(out), _stream())
    return out


# ---------------------------------------------------------------------------
class RowPlan:
    """Row order of one LSTM stack for one batch (evc_sort_rows_by_len): rows sorted by sequence length,
    longest first, so that the rows active at step t are the prefix [0, rows[t]) and the length-0 rows
    (frames beyond num_frames) drop out of every kernel.

    pos / inv / lens  device int32 [M]: slot of each row, row of each slot, length of each slot
    P                 rows kept per time slab (rows[0] rounded up to 32, at most M): all [T][M][..] buffers
                      of the stack are used as [T][P][..]
    rows              host list [T]: rows[t] = #{len > t}, computed from the HOST copy of the lengths (the
                      launch geometry depends on it; a device->host read would stall the stream)
    """

    def __init__(self, lens_dev, lens_host, T):
        import numpy as np
        lens_host = np.asarray(lens_host)
        M = int(lens_dev.shape[0])
        assert lens_host.shape == (M,)
        self.M, self.T = M, T
        hist = np.bincount(np.clip(lens_host, 0, T), minlength=T + 1)
        self.rows = [int(M - hist[:t + 1].sum()) for t in range(T)]         # rows with len > t
        self.P = min(M, max(32, round_up(self.rows[0], 32)))
        self.rows_c = (C.c_int32 * T)(*self.rows)
        dev = lens_dev.device
        self.pos = torch.empty(M, dtype=torch.int32, device=dev)
        self.inv = torch.empty(M, dtype=torch.int32, device=dev)
        self.lens = torch.empty(M, dtype=torch.int32, device=dev)
        _lib.call("evc_sort_rows_by_len", _p(lens_dev), M, T, _p(self.pos), _p(self.inv), _p(self.lens), _stream())


def host_frame_counts(num_frames_host, every_n, num_chunks, chunk_len, max_frames=300, subsampled=None):
    """Host (numpy) twin of evc_frame_counts, bit-identical: (n_used int64 [B], len_l1 int32 [C*B], len_l2 int32 [B]).
    subsampled: the student formula of cs/train.py:264 (default: every_n > 1; the student graph passes True also at
    every_n = 1, where float64 (n/300)*300 truncates to n-1 for some n)."""
    import numpy as np
    n = np.asarray(num_frames_host).astype(np.int64)
    if (every_n > 1) if subsampled is None else subsampled:
        S = max_frames // every_n
        n = np.trunc(n.astype(np.float64) / float(max_frames) * float(S)).astype(np.int64)
    l1 = np.clip(n[None, :] - chunk_len * np.arange(num_chunks, dtype=np.int64)[:, None], 0, chunk_len).astype(np.int32).reshape(-1)
    l2 = np.ceil(n.astype(np.float32) / np.float32(chunk_len)).astype(np.int32)
    return n, l1, l2


def l2norm_chunk(x_raw, num_chunks, every_n=None, num_chunks_student=None, num_frames=None, normalize=True, split=False,
                 plan1=None, plan2=None, f16_segments=1, fp8_tail=False, teacher_view=True):
    """a1+a2.  x_raw [B,T,F] f32 (or uint8 with num_frames).  Returns the
    teacher view [Lc][C*B][F] bf16 and (if every_n) the student view; with row plans the views are
    [Lc][plan.P][F] in slot order.  split: True -> (bf16, bf16 low half) pairs; "f16" -> (bf16, IEEE f16 image) pairs (the
    operands of the "high" precision L1 forward; the bf16 image stays the operand of the backward products) - the f16 image
    has rows of f16_segments*F: [f16(x) | (x - f16(x))*64 | f16(x)/64], the K-extended x operand of lstm_layer_fwd_f16;
    "wide" -> (bf16, wide bf16 image with rows [lo | hi] of 2F) pairs, the input of lstm_layer_fwd_hp.
    fp8_tail (with split "f16", f16_segments 1): the f16 image's rows are 2F halfwords = [f16(x) | e4m3(x 2^7) (F bytes) | e4m3((x - f16(x)) 2^18)
    (F bytes)], the x rows of lstm_layer_fwd_f16_fp8lo (evc_l2norm_chunk_fwd aux_mode 5).
    teacher_view=False (student-only graphs; needs every_n): the first view is None and only the sub-sampled frames of x_raw are read."""
    B, T, F = x_raw.shape
    dev = x_raw.device
    assert teacher_view or every_n, "l2norm_chunk: no view requested"
    rows1 = (plan1.P if plan1 is not None else num_chunks * B) if teacher_view else 0
    out1 = torch.empty((T // num_chunks, rows1, F), dtype=BF16, device=dev) if teacher_view else None
    out2 = None
    rows2 = 0
    if every_n:
        S = T // every_n
        rows2 = plan2.P if plan2 is not None else num_chunks_student * B
        out2 = torch.empty((S // num_chunks_student, rows2, F), dtype=BF16, device=dev)
    is_u8 = x_raw.dtype == torch.uint8
    aux_dt = F16 if split == "f16" else BF16
    nseg = f16_segments if split == "f16" else (2 if split == "wide" else 1)
    aux_mode = nseg if split == "f16" else (4 if split == "wide" else 0)
    wrow = nseg * F
    if fp8_tail:
        assert split == "f16" and f16_segments == 1 and F % 32 == 0, "fp8_tail: the f16 image + two e4m3 images, F % 32 == 0"
        aux_mode, wrow = 5, 2 * F
    lo1 = torch.empty(out1.shape[:2] + (wrow,), dtype=aux_dt, device=dev) if (split and out1 is not None) else None
    lo2 = torch.empty(out2.shape[:2] + (wrow,), dtype=aux_dt, device=dev) if (split and out2 is not None) else None
    _lib.call("evc_l2norm_chunk_fwd", None if is_u8 else _p(x_raw), _p(x_raw) if is_u8 else None, _p(num_frames),
              B, T, F, num_chunks, _p(out1), every_n or 1, num_chunks_student or 1, _p(out2), 1 if normalize else 0,
              _p(lo1), _p(lo2), aux_mode, _p(plan1.pos) if (plan1 is not None and teacher_view) else None, rows1,
              _p(plan2.pos) if plan2 is not None else None, rows2, _stream())
    if split:      # image pairs for the "high" / "split" precision forward
        return ((out1, lo1) if out1 is not None else None), ((out2, lo2) if out2 is not None else None)
    return out1, out2


def frame_counts(num_frames, every_n, num_chunks, chunk_len, max_frames=300, subsampled=None):
    """a2 integer part.  Returns (n_used int64 [B], len_l1 int32 [C*B], len_l2 int32 [B])."""
    sub = (every_n > 1) if subsampled is None else subsampled
    B = num_frames.shape[0]
    dev = num_frames.device
    n_out = torch.empty(B, dtype=torch.int64, device=dev)
    l1 = torch.empty(num_chunks * B, dtype=torch.int32, device=dev)
    l2 = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.call("evc_frame_counts", _p(num_frames), B, every_n, 1 if sub else 0, max_frames, num_chunks, chunk_len, _p(n_out), _p(l1), _p(l2), _stream())
    return n_out, l1, l2


# Which frames the student sees (--student_sampling); the position in the tuple is the EVC_SELECT_* code of evc_student_frame_select.
STUDENT_SAMPLING = ("uniform", "first", "middle", "last", "first_middle_last", "random")


# The strategies that read the video: the table is ranked by one key per frame (frame_change_keys); the EVC_SELECT_* codes go on from
# STUDENT_SAMPLING's, for evc_student_frame_select_scored.
STUDENT_SAMPLING_SCORED = ("change", "segment_change")


def check_student_sampling(word, flag="student_sampling"):
    """The word itself, or a ValueError that names the choices (raised before anything touches the device)."""
    if word not in STUDENT_SAMPLING and word not in STUDENT_SAMPLING_SCORED:
        raise ValueError("%s: %r (%s)" % (flag, word, " | ".join(STUDENT_SAMPLING + STUDENT_SAMPLING_SCORED)))
    return word


def student_frame_select(num_frames, T, every_n, strategy, seed=0, draw=0, row0=0):
    """The student's source-frame table (evc_student_frame_select): src [B, T // every_n] int32 on the device, -1 = no frame.  num_frames [B]
    int32 (device); strategy a word of STUDENT_SAMPLING; seed / draw / row0 only matter under "random" (draw: the training iteration,
    row0: index of this batch's first video in the global batch)."""
    if check_student_sampling(strategy, "student_frame_select") in STUDENT_SAMPLING_SCORED:
        raise ValueError("student_frame_select: %r ranks the frames by their content, so the frames are needed: frame_change_keys, then "
                         "student_frame_select_scored" % (strategy,))
    code = STUDENT_SAMPLING.index(strategy)
    assert num_frames.dtype == torch.int32 and num_frames.dim() == 1 and num_frames.is_contiguous()
    B = num_frames.shape[0]
    src = torch.empty((B, T // max(1, every_n)), dtype=torch.int32, device=num_frames.device)
    _lib.call("evc_student_frame_select", _p(num_frames), B, T, every_n, code, int(seed) & 0xFFFFFFFF, int(draw) & 0xFFFFFFFF, int(row0), _p(src), _stream())
    return src


def frame_change_keys(x_raw, num_frames):
    """One key per frame, its squared change from the frame before (evc_frame_change_keys): x_raw [B, T, F] float32 or uint8 RAW frames
    (contiguous, device), num_frames [B] int32 -> keys [B, T], the uint32 keys as the bit patterns of an int32 tensor (what
    student_frame_select_scored takes; .cpu().numpy().view(numpy.uint32) to look at them).  Depends on the data only."""
    assert x_raw.dim() == 3 and x_raw.is_contiguous() and x_raw.dtype in (torch.float32, torch.uint8)
    assert num_frames.dtype == torch.int32 and num_frames.dim() == 1 and num_frames.is_contiguous() and num_frames.shape[0] == x_raw.shape[0]
    B, T, F = x_raw.shape
    keys = torch.empty((B, T), dtype=torch.int32, device=x_raw.device)
    is_u8 = x_raw.dtype == torch.uint8
    _lib.call("evc_frame_change_keys", None if is_u8 else _p(x_raw), _p(x_raw) if is_u8 else None, _p(num_frames), B, T, F, _p(keys), _stream())
    return keys


def student_frame_select_scored(num_frames, keys, T, every_n, strategy):
    """The student's source-frame table under a word of STUDENT_SAMPLING_SCORED (evc_student_frame_select_scored): src [B, T // every_n]
    int32 on the device, -1 = no frame, from keys [B, T] (frame_change_keys)."""
    if strategy not in STUDENT_SAMPLING_SCORED:
        raise ValueError("student_frame_select_scored: %r (%s)" % (strategy, " | ".join(STUDENT_SAMPLING_SCORED)))
    code = len(STUDENT_SAMPLING) + STUDENT_SAMPLING_SCORED.index(strategy)
    assert num_frames.dtype == torch.int32 and num_frames.dim() == 1 and num_frames.is_contiguous()
    B = num_frames.shape[0]
    assert keys.dtype == torch.int32 and tuple(keys.shape) == (B, T) and keys.is_contiguous()
    src = torch.empty((B, T // max(1, every_n)), dtype=torch.int32, device=num_frames.device)
    _lib.call("evc_student_frame_select_scored", _p(num_frames), _p(keys), B, T, every_n, code, _p(src), _stream())
    return src


def l2norm_chunk_sel(x_raw, src, every_n, num_chunks_student, num_frames=None, normalize=True, split=False, plan2=None, f16_segments=1,
                     fp8_tail=False):
    """The student view of l2norm_chunk(..., teacher_view=False) from the frames a table names (evc_l2norm_chunk_sel_fwd): slot j of video b
    holds frame src[b, j] of x_raw (student_frame_select; -1: a zero row).  Same arguments and the same return form as that view: the bf16
    image, or with split the pair (bf16 image, second image)."""
    B, T, F = x_raw.shape
    dev = x_raw.device
    S = T // every_n
    assert src.dtype == torch.int32 and tuple(src.shape) == (B, S) and src.is_contiguous() and x_raw.is_contiguous()
    rows2 = plan2.P if plan2 is not None else num_chunks_student * B
    out2 = torch.empty((S // num_chunks_student, rows2, F), dtype=BF16, device=dev)
    is_u8 = x_raw.dtype == torch.uint8
    aux_dt = F16 if split == "f16" else BF16
    nseg = f16_segments if split == "f16" else (2 if split == "wide" else 1)
    aux_mode = nseg if split == "f16" else (4 if split == "wide" else 0)
    wrow = nseg * F
    if fp8_tail:
        assert split == "f16" and f16_segments == 1 and F % 32 == 0, "fp8_tail: the f16 image + two e4m3 images, F % 32 == 0"
        aux_mode, wrow = 5, 2 * F
    lo2 = torch.empty(out2.shape[:2] + (wrow,), dtype=aux_dt, device=dev) if split else None
    _lib.call("evc_l2norm_chunk_sel_fwd", None if is_u8 else _p(x_raw), _p(x_raw) if is_u8 else None, _p(num_frames), _p(src), B, T, F, every_n,
              num_chunks_student, _p(out2), 1 if normalize else 0, _p(lo2), aux_mode, _p(plan2.pos) if plan2 is not None else None, rows2, _stream())
    return (out2, lo2) if split else out2


def l2norm_chunk_int_sel(x_u8, num_frames, src, every_n, num_chunks_student, plan2=None):
    """The student view of l2norm_chunk_int(..., teacher_view=False) from the frames a table names (evc_l2norm_chunk_sel_int):
    (bf16 image, integer image, row scales)."""
    B, T, F = x_u8.shape
    S = T // every_n
    assert x_u8.dtype == torch.uint8 and F % 32 == 0 and x_u8.is_contiguous()
    assert src.dtype == torch.int32 and tuple(src.shape) == (B, S) and src.is_contiguous()
    dev = x_u8.device
    rows2 = plan2.P if plan2 is not None else num_chunks_student * B
    L2 = S // num_chunks_student
    out2 = torch.empty((L2, rows2, F), dtype=BF16, device=dev)
    int2 = torch.empty((L2, rows2, 3 * F // 2), dtype=F16, device=dev)
    rs2 = torch.zeros((L2, rows2), dtype=F32, device=dev)
    _lib.call("evc_l2norm_chunk_sel_int", _p(x_u8), _p(num_frames), _p(src), B, T, F, every_n, num_chunks_student, _p(out2), _p(int2), _p(rs2),
              _p(plan2.pos) if plan2 is not None else None, rows2, _stream())
    return out2, int2, rs2


# ---------------------------------------------------------------------------
def _plan_args(plan):
    return (_p(plan.inv), plan.rows_c) if plan is not None else (None, None)


def lstm_layer_fwd(x, wT, bias, lens, T, M, Kin, H, hbuf, c_state, h_state, ld_state,
                   gates=None, c_all=None, hoist=False, zx_ws=None, plan=None):
    """With a RowPlan: M = plan.P, lens = plan.lens, all [T][M][..] operands in slot order."""
    _lib.call("evc_lstm_layer_fwd", _p(x), _p(wT), _p(bias), _p(lens), T, M, Kin, H, 1 if hoist else 0, _p(zx_ws),
              _p(hbuf), _p(c_state), _p(h_state), ld_state, _p(gates), _p(c_all), *_plan_args(plan), _stream())


def lstm_layer_fwd_f16(x16, wT16, bias, lens, T, M, Kin, H, hbuf16, hbuf_bf, c_state, h_state, ld_state,
                       gates=None, c_all=None, plan=None, ldx=None, h_wide=False):
    """lstm_layer_fwd on IEEE f16 operands (one f16 MFMA product per depth); hbuf16 f16 (h_wide: rows [h | h/64] of 2H against a
    kernel whose h-part is [Wh | Wh_lo*64]), hbuf_bf the bf16 copy of h; ldx: row stride of x16 (default Kin)."""
    assert x16.dtype == F16 and wT16.dtype == F16 and hbuf16.dtype == F16 and hbuf_bf.dtype == BF16
    assert wT16.shape[1] == Kin + (2 if h_wide else 1) * H
    _lib.call("evc_lstm_layer_fwd_f16", _p(x16), Kin if ldx is None else ldx, _p(wT16), _p(bias), _p(lens), T, M, Kin, H, _p(hbuf16),
              1 if h_wide else 0, _p(hbuf_bf), _p(c_state), _p(h_state), ld_state, _p(gates), _p(c_all), *_plan_args(plan), _stream())


def lstm_layer_fwd_f16_fp8lo(x16, ldx, kx16, x8_off, kx8, wT16, wT8, bias, lens, T, M, H, hbuf16, hbuf_bf, c_state, h_state, ld_state,
                             gates=None, c_all=None, plan=None, w8_scale_exp=FP8_W_SCALE_EXP, h_lo=False, x_int=None, b8_gap=0):
    """lstm_layer_fwd_f16 with the weights' low-order halves contracted in fp8 (evc_lstm_layer_fwd_f16_fp8lo): x16 rows of ldx halfwords
    (kx16 halfwords of f16 operand at the row start, kx8 e4m3 bytes at byte offset x8_off), wT16 [4H][kx16 + H] f16, wT8 [4H][kx8 + H]
    uint8 (cast_fp8_lo), hbuf16 [(T+1)][M][3H/2] f16 containers = rows [f16(h) | e4m3(h 2^7)], hbuf_bf the bf16 copy of h.
    h_lo: the low-order half of h corrected too - hbuf16 [(T+1)][M][2H] containers = rows [f16(h) | e4m3(h 2^7) | e4m3((h - f16(h)) 2^18)],
    wT8 [4H][kx8 + 2H] with the h-part [lo(Wh) | hi(Wh)] (cast_fp8_lo(hi_tail=True)).
    x_int = (row_scale [T][M] f32, col_const [4H] f32): the integer-frame form (x16 rows from l2norm_chunk_int: exact integers + e4m3(x_hat 2^7));
    b8_gap: bytes of wT8's rows between the x-part this launch contracts and the h-part (the hi(Wx) block)."""
    assert x16.dtype == F16 and wT16.dtype == F16 and wT8.dtype == torch.uint8 and hbuf16.dtype == F16 and hbuf_bf.dtype == BF16
    assert wT16.shape == (4 * H, kx16 + H) and wT8.shape == (4 * H, kx8 + b8_gap + (2 if h_lo else 1) * H) and wT16.is_contiguous() and wT8.is_contiguous()
    rs, cc = x_int if x_int is not None else (None, None)
    assert x_int is None or (rs.dtype == F32 and cc.dtype == F32 and rs.numel() >= T * M and cc.numel() == 4 * H and rs.is_contiguous() and cc.is_contiguous())
    assert hbuf16.shape[-1] == (2 * H if h_lo else 3 * H // 2)
    _lib.call("evc_lstm_layer_fwd_f16_fp8lo", _p(x16), ldx, kx16, x8_off, kx8, _p(wT16), _p(wT8), w8_scale_exp, 1 if h_lo else 0, _p(bias), _p(lens), T, M, H,
              _p(hbuf16), _p(hbuf_bf), _p(c_state), _p(h_state), ld_state, _p(gates), _p(c_all), *_plan_args(plan), _p(rs), _p(cc), b8_gap, _stream())


def l2norm_chunk_int(x_u8, num_frames, num_chunks, every_n=None, num_chunks_student=None, plan1=None, plan2=None, teacher_view=True):
    """l2norm_chunk for the "high" mode on the reader's uint8 frames (evc_l2norm_chunk_int): per view (bf16 image, integer image, row scales) -
    integer image rows of 3F/2 containers [f16(2q - 255) | e4m3(x_hat 2^7)], row scales [steps][rows] f32 with x_hat = rs (c + 255/256)."""
    B, T, F = x_u8.shape
    assert x_u8.dtype == torch.uint8 and F % 32 == 0 and (teacher_view or every_n)
    dev = x_u8.device
    rows1 = (plan1.P if plan1 is not None else num_chunks * B) if teacher_view else 0
    L1 = T // num_chunks
    out1 = torch.empty((L1, rows1, F), dtype=BF16, device=dev) if teacher_view else None
    int1 = torch.empty((L1, rows1, 3 * F // 2), dtype=F16, device=dev) if teacher_view else None
    rs1 = torch.zeros((L1, rows1), dtype=F32, device=dev) if teacher_view else None
    out2 = int2 = rs2 = None
    rows2 = 0
    if every_n:
        S = T // every_n
        rows2 = plan2.P if plan2 is not None else num_chunks_student * B
        L2 = S // num_chunks_student
        out2 = torch.empty((L2, rows2, F), dtype=BF16, device=dev)
        int2 = torch.empty((L2, rows2, 3 * F // 2), dtype=F16, device=dev)
        rs2 = torch.zeros((L2, rows2), dtype=F32, device=dev)
    _lib.call("evc_l2norm_chunk_int", _p(x_u8), _p(num_frames), B, T, F, num_chunks, _p(out1), every_n or 1, num_chunks_student or 1, _p(out2),
              _p(int1), _p(int2), _p(rs1), _p(rs2), _p(plan1.pos) if (plan1 is not None and teacher_view) else None, rows1,
              _p(plan2.pos) if plan2 is not None else None, rows2, _stream())
    return ((out1, int1, rs1) if teacher_view else None), ((out2, int2, rs2) if every_n else None)


def lstm_layer_fwd_f16_dith(x16, ldx, kx16, x8_off, kx8, wT16_steps, wT8, ldb8, scale8_exp, bias, lens, T, M, H, hbuf16, hbuf_bf, c_state, h_state,
                            ld_state, gates=None, c_all=None, plan=None):
    """lstm_layer_fwd_f16 on time-dithered weight images (evc_lstm_layer_fwd_f16_dith): wT16_steps [T'][4H][kx16 + H] f16 from cast_f16_dither
    (T' >= T; T' == 1: one image for every step), x16 rows of ldx halfwords with kx8 e4m3 bytes at byte offset x8_off (kx8 = 0: none) against
    the first kx8 bytes of wT8's rows (row stride ldb8; a view into a cast_fp8_lo image), every e4m3 product scaled by 2^-scale8_exp;
    hbuf16 [(T+1)][M][H] plain f16 rows, hbuf_bf the bf16 copy of h."""
    assert x16.dtype == F16 and wT16_steps.dtype == F16 and hbuf16.dtype == F16 and hbuf_bf.dtype == BF16
    assert wT16_steps.dim() == 3 and wT16_steps.shape[1:] == (4 * H, kx16 + H) and wT16_steps.is_contiguous() and wT16_steps.shape[0] in (1, ) + tuple(range(T, 4097))
    assert (kx8 == 0) == (wT8 is None) and (wT8 is None or wT8.dtype == torch.uint8)
    stride = 0 if wT16_steps.shape[0] == 1 else wT16_steps.stride(0)
    _lib.call("evc_lstm_layer_fwd_f16_dith", _p(x16), ldx, kx16, x8_off, kx8, _p(wT16_steps), stride, _p(wT8), ldb8, scale8_exp, _p(bias), _p(lens), T, M, H,
              _p(hbuf16), _p(hbuf_bf), _p(c_state), _p(h_state), ld_state, _p(gates), _p(c_all), *_plan_args(plan), _stream())


def lstm_level2_fwd_high(x16, ldx, kx16, x8_off, kx8, wT16_0, wT8_0, bias0, wT16_1_steps, bias1, lens, T, M, H, h0_rows, hbuf0, h1_rows, hbuf1, S,
                         gates=(None, None), c_all=(None, None), plan=None, w8_scale_exp=FP8_W_SCALE_EXP, h_lo=False, x_int=None, b8_gap=0):
    """The two-layer L1 level of the "high" mode as T + 1 two-tile launches (evc_lstm_level2_fwd_high): lstm_layer_fwd_f16_fp8lo for layer 0 (same
    arguments) + lstm_layer_fwd_f16_dith(kx8 = 0) for layer 1 on wT16_1_steps [T'][4H][2H], bit for bit.  h0_rows [(T+1)][M][2H or 3H/2] f16 containers,
    h1_rows [(T+1)][M][H] f16, hbuf0 / hbuf1 the bf16 copies; S [rows][4H] f32 = [c0 | h0 | c1 | h1]."""
    assert x16.dtype == F16 and wT16_0.dtype == F16 and wT8_0.dtype == torch.uint8 and wT16_1_steps.dtype == F16
    assert h0_rows.dtype == F16 and h1_rows.dtype == F16 and hbuf0.dtype == BF16 and hbuf1.dtype == BF16
    assert wT16_0.shape == (4 * H, kx16 + H) and wT8_0.shape == (4 * H, kx8 + b8_gap + (2 if h_lo else 1) * H) and wT16_0.is_contiguous() and wT8_0.is_contiguous()
    assert wT16_1_steps.dim() == 3 and wT16_1_steps.shape[1:] == (4 * H, 2 * H) and wT16_1_steps.is_contiguous() and (wT16_1_steps.shape[0] == 1 or wT16_1_steps.shape[0] >= T)
    assert h0_rows.shape[-1] == (2 * H if h_lo else 3 * H // 2) and h1_rows.shape[-1] == H
    rs, cc = x_int if x_int is not None else (None, None)
    assert x_int is None or (rs.dtype == F32 and cc.dtype == F32 and rs.numel() >= T * M and cc.numel() == 4 * H and rs.is_contiguous() and cc.is_contiguous())
    stride = 0 if wT16_1_steps.shape[0] == 1 else wT16_1_steps.stride(0)
    _lib.call("evc_lstm_level2_fwd_high", _p(x16), ldx, kx16, x8_off, kx8, _p(wT16_0), _p(wT8_0), w8_scale_exp, 1 if h_lo else 0, _p(bias0), _p(rs), _p(cc), b8_gap,
              _p(wT16_1_steps), stride, _p(bias1), _p(lens), T, M, H, _p(h0_rows), _p(hbuf0), _p(h1_rows), _p(hbuf1),
              _p(S[:, 0:]), _p(S[:, H:]), _p(S[:, 2 * H:]), _p(S[:, 3 * H:]), S.stride(0),
              _p(gates[0]), _p(c_all[0]), _p(gates[1]), _p(c_all[1]), *_plan_args(plan), _stream())


def cast_f16_dither(p, out, seed, col0=0):
    """out [T][...p.shape] f16: the T time-dithered f16 images of the f32 tensor p (evc_cast_f32_to_f16_dither; oracle/lowprec.py::f16_dither_images).
    col0 > 0 (p 2-D): only the columns from col0 on are dithered, the others hold their round-to-nearest value in every image."""
    assert p.dtype == F32 and p.is_contiguous() and out.dtype == F16 and out.is_contiguous() and out.shape[1:] == p.shape
    assert col0 == 0 or (p.dim() == 2 and 0 < col0 <= p.shape[1])
    _lib.call("evc_cast_f32_to_f16_dither", _p(p), p.numel(), out.shape[0], out.stride(0) if out.shape[0] > 1 else p.numel(), int(seed) & 0xFFFFFFFF, _p(out),
              p.shape[1] if col0 else 0, col0, _stream())


def lstm_level2_fwd(x, wT0, bias0, wT1, bias1, lens, T, M, Kin, H, hbuf0, hbuf1, S, gates=(None, None), c_all=(None, None), plan=None):
    """Two-layer L1 level in bf16, layer 0's step s and layer 1's step s-1 per launch (evc_lstm_level2_fwd): the results of two
    lstm_layer_fwd calls, bit for bit.  S [rows][4H] f32 = [c0 | h0 | c1 | h1]; with a RowPlan M = plan.P, lens = plan.lens."""
    assert x.dtype == BF16 and wT0.dtype == BF16 and wT1.dtype == BF16 and hbuf0.dtype == BF16 and hbuf1.dtype == BF16
    _lib.call("evc_lstm_level2_fwd", _p(x), _p(wT0), _p(bias0), _p(wT1), _p(bias1), _p(lens), T, M, Kin, H, _p(hbuf0), _p(hbuf1),
              _p(S[:, 0:]), _p(S[:, H:]), _p(S[:, 2 * H:]), _p(S[:, 3 * H:]), S.stride(0),
              _p(gates[0]), _p(c_all[0]), _p(gates[1]), _p(c_all[1]), *_plan_args(plan), _stream())


def lstm_stack2_fwd(x, wT0, bias0, wT1, bias1, lens, T, M, Kin, H, zx_ws, hbuf0, hbuf1, S, gates=(None, None), c_all=(None, None)):
    """Two-layer stack, M ~ batch rows, wavefront order (evc_lstm_stack2_fwd).  S [M][4H] f32 = [c0 | h0 | c1 | h1]."""
    _lib.call("evc_lstm_stack2_fwd", _p(x), _p(wT0), _p(bias0), _p(wT1), _p(bias1), _p(lens), T, M, Kin, H, _p(zx_ws),
              _p(hbuf0), _p(hbuf1), _p(S[:, 0:]), _p(S[:, H:]), _p(S[:, 2 * H:]), _p(S[:, 3 * H:]), S.stride(0),
              _p(gates[0]), _p(c_all[0]), _p(gates[1]), _p(c_all[1]), _stream())


def lstm_stack2_fwd_f16(x16, wT0_16, bias0, wT1_wlo, bias1, lens, T, M, Kin, H, zx_ws, h0_wide, h1_wide, hbuf0, hbuf1, S,
                        gates=(None, None), c_all=(None, None), x_segments=1, h0_ext=False):
    """Two-layer stack, M ~ batch rows, wavefront order, IEEE f16 operands with the upper layer's weights K-extended by their
    low-order halves (evc_lstm_stack2_fwd_f16).  h*_wide [(T+1)][M][2H] f16, hbuf* [(T+1)][M][H] bf16; S [M][4H] f32."""
    assert x16.dtype == F16 and wT0_16.dtype == F16 and wT1_wlo.dtype == F16 and h0_wide.dtype == F16 and hbuf0.dtype == BF16
    assert x16.shape[-1] == x_segments * Kin and wT0_16.shape[1] == x_segments * Kin + (2 if h0_ext else 1) * H
    _lib.call("evc_lstm_stack2_fwd_f16", _p(x16), x_segments, _p(wT0_16), 1 if h0_ext else 0, _p(bias0), _p(wT1_wlo), _p(bias1), _p(lens),
              T, M, Kin, H, _p(zx_ws),
              _p(h0_wide), _p(h1_wide), _p(hbuf0), _p(hbuf1), _p(S[:, 0:]), _p(S[:, H:]), _p(S[:, 2 * H:]), _p(S[:, 3 * H:]), S.stride(0),
              _p(gates[0]), _p(c_all[0]), _p(gates[1]), _p(c_all[1]), _stream())


def lstm_stack2_fwd_f16_fp8lo(x16, wT0_16, wT0_8, bias0, wT1_16, wT1_8, bias1, lens, T, M, Kin, H, zx_ws, h0_rows, h1_rows, hbuf0, hbuf1, S,
                              gates=(None, None), c_all=(None, None), x_segments=1, w8_scale_exp=FP8_W_SCALE_EXP, h_lo=False):
    """lstm_stack2_fwd_f16 with the low-order halves of layer 0's recurrent weights and of layer 1's weights as e4m3 operands behind the f16
    stages of the same launches (evc_lstm_stack2_fwd_f16_fp8lo).  wT0_16 [4H][x_segments Kin + H], wT0_8 [4H][H], wT1_16 / wT1_8 [4H][2H];
    h*_rows [(T+1)][M][3H/2] f16 containers = rows [f16(h) | e4m3(h 2^7)]; hbuf* [(T+1)][M][H] bf16; S [M][4H] f32.
    h_lo: rows [f16(h) | e4m3(h 2^7) | e4m3((h - f16(h)) 2^18)] (2H containers), wT0_8 [4H][2H] = [lo(Wh0) | hi(Wh0)], wT1_8 [4H][4H] = [lo(Wx1) | hi(Wx1)
    | lo(Wh1) | hi(Wh1)] (cast_fp8_lo(hi_tail=True)): the activations' low-order halves corrected as well."""
    k8 = 2 if h_lo else 1
    assert x16.dtype == F16 and wT0_16.dtype == F16 and wT1_16.dtype == F16 and wT0_8.dtype == torch.uint8 and wT1_8.dtype == torch.uint8
    assert x16.shape[-1] == x_segments * Kin and wT0_16.shape == (4 * H, x_segments * Kin + H) and wT0_8.shape == (4 * H, k8 * H)
    assert wT1_16.shape == (4 * H, 2 * H) and wT1_8.shape == (4 * H, 2 * k8 * H) and h0_rows.dtype == F16 and hbuf0.dtype == BF16
    assert h0_rows.shape[-1] == h1_rows.shape[-1] == (2 * H if h_lo else 3 * H // 2)
    assert all(t.is_contiguous() for t in (wT0_16, wT0_8, wT1_16, wT1_8))
    _lib.call("evc_lstm_stack2_fwd_f16_fp8lo", _p(x16), x_segments, _p(wT0_16), _p(wT0_8), _p(bias0), _p(wT1_16), _p(wT1_8), w8_scale_exp, 1 if h_lo else 0, _p(bias1),
              _p(lens), T, M, Kin, H, _p(zx_ws), _p(h0_rows), _p(h1_rows), _p(hbuf0), _p(hbuf1),
              _p(S[:, 0:]), _p(S[:, H:]), _p(S[:, 2 * H:]), _p(S[:, 3 * H:]), S.stride(0),
              _p(gates[0]), _p(c_all[0]), _p(gates[1]), _p(c_all[1]), _stream())


def lstm_layer_fwd_hp(x_lohi, wx_hilo, wh_hilo, bias, lens, T, M, Kin, H, zx_ws, hbuf, hbuf_lohi, c_state, h_state, ld_state,
                      gates=None, c_all=None):
    """Split-bf16 layer for the M ~ batch stacks (evc_lstm_layer_fwd_hp): wide [lo | hi] activations, [hi | lo] weights."""
    _lib.call("evc_lstm_layer_fwd_hp", _p(x_lohi), _p(wx_hilo), wx_hilo.stride(0), _p(wh_hilo), wh_hilo.stride(0), _p(bias), _p(lens),
              T, M, Kin, H, _p(zx_ws), _p(hbuf), _p(hbuf_lohi), _p(c_state), _p(h_state), ld_state, _p(gates), _p(c_all), _stream())


def lstm_layer_bwd(w_il, lens, T, M, Kin, H, gates, c_all, dS_c, dS_h, ld_dS, dh_above, dc_ws, dz4, plan=None, db=None,
                   dz_above=None, w_above=None, dz_dead_unread=False):
    """db [4H] f32: the bias gradient is accumulated into it (zero it first) - no separate column-sum pass.
    dz_above / w_above (instead of dh_above): the upper layer's gate gradients and backward-layout kernel - its dX is
    contracted inside this layer's steps.
    dz_dead_unread (row plans): nothing reads slab t of dz4 from row round_up(plan.rows[t], 32) on - those tiles are left unwritten
    (evc_lstm_layer_bwd_live)."""
    if dz_dead_unread:
        _lib.call("evc_lstm_layer_bwd_live", _p(w_il), _p(lens), T, M, Kin, H, _p(gates), _p(c_all), _p(dS_c), _p(dS_h), ld_dS,
                  _p(dh_above), _p(dc_ws), _p(dz4), _p(db), *_plan_args(plan), _p(dz_above), _p(w_above), 1, _stream())
        return
    _lib.call("evc_lstm_layer_bwd", _p(w_il), _p(lens), T, M, Kin, H, _p(gates), _p(c_all), _p(dS_c), _p(dS_h), ld_dS,
              _p(dh_above), _p(dc_ws), _p(dz4), _p(db), *_plan_args(plan), _p(dz_above), _p(w_above), _stream())


def lstm_stack2_bwd(w_il0, w_il1, lens, T, M, Kin0, H, gates, c_all, dS, dc_ws, dz, db, plan=None):
    """Two-layer stack, BPTT in wavefront order (evc_lstm_stack2_bwd).  gates / c_all / dc_ws / dz / db: per-layer pairs."""
    _lib.call("evc_lstm_stack2_bwd", _p(w_il0), _p(w_il1), _p(lens), T, M, Kin0, H, _p(gates[0]), _p(c_all[0]), _p(gates[1]),
              _p(c_all[1]), _p(dS), dS.stride(0), _p(dc_ws[0]), _p(dc_ws[1]), _p(dz[0]), _p(dz[1]), _p(db[0]), _p(db[1]),
              *_plan_args(plan), _stream())


TOPK_MAX_K = 256         # evc_topk_rows: 1 <= k <= min(cols, 256), cols <= 32768


def topk_rows(x, k):
    """Per-row top-k of a 2-D f32 tensor (rows contiguous, any row stride) on the current stream (evc_topk_rows): (values [B, k] f32,
    indices [B, k] int32), value descending and column ascending - -0 ties with +0, NaN above +inf, ties at the k-th place admit the
    lowest columns; the values are the input's own bits.  The selection of the inference binary (cs/inference_ensemble.py:63-74)."""
    if x.dtype != F32 or x.dim() != 2 or (x.shape[0] > 0 and x.shape[1] > 1 and x.stride(1) != 1):
        raise _lib.EvcError("topk_rows: needs a 2-D float32 tensor with contiguous rows (got %s %s)" % (x.dtype, tuple(x.shape)))
    B, cols = x.shape
    kk = max(int(k), 0)
    values = torch.empty((B, kk), dtype=F32, device=x.device)
    indices = torch.empty((B, kk), dtype=torch.int32, device=x.device)
    ld = x.stride(0) if B > 1 else cols
    _lib.call("evc_topk_rows", _p(x), ld, B, cols, int(k), _p(values), _p(indices), _stream())
    return values, indices


def eval_select_rows(predictions, labels, k):
    """What eval_util.EvaluationMetrics.accumulate_selected needs from one batch, selected on the current stream
    (evc_eval_select_rows): predictions [B, C] f32 and labels [B, C] uint8 (rows contiguous, any row stride) -> dict of device tensors
    top_val [B, k] f32 / top_idx [B, k] int32 (= topk_rows(predictions, k)), top_lab [B, k] uint8 (the labels of those columns),
    n_pos [B] int32 (positives per row), perr_hits [B] int32 (positives with a value > 0 among each row's first n_pos columns in the
    order of topk_rows) and class_pos [C] int32 (positives per class)."""
    x, y = predictions, labels
    if x.dtype != F32 or x.dim() != 2 or (x.shape[0] > 0 and x.shape[1] > 1 and x.stride(1) != 1):
        raise _lib.EvcError("eval_select_rows: needs 2-D float32 predictions with contiguous rows (got %s %s)" % (x.dtype, tuple(x.shape)))
    if y.dtype != torch.uint8 or y.dim() != 2 or tuple(y.shape) != tuple(x.shape) or (y.shape[0] > 0 and y.shape[1] > 1 and y.stride(1) != 1):
        raise _lib.EvcError("eval_select_rows: needs uint8 labels of the predictions' shape %s with contiguous rows (got %s %s)"
                            % (tuple(x.shape), y.dtype, tuple(y.shape)))
    if y.device != x.device:
        raise _lib.EvcError("eval_select_rows: predictions on %s, labels on %s" % (x.device, y.device))
    B, cols = x.shape
    kk = max(int(k), 0)
    out = {"top_val": torch.empty((B, kk), dtype=F32, device=x.device), "top_idx": torch.empty((B, kk), dtype=torch.int32, device=x.device),
           "top_lab": torch.empty((B, kk), dtype=torch.uint8, device=x.device), "n_pos": torch.empty((B,), dtype=torch.int32, device=x.device),
           "perr_hits": torch.empty((B,), dtype=torch.int32, device=x.device),
           "class_pos": torch.zeros((cols,), dtype=torch.int32, device=x.device)}
    _lib.call("evc_eval_select_rows", _p(x), x.stride(0) if B > 1 else cols, _p(y), y.stride(0) if B > 1 else cols, B, cols, int(k),
              _p(out["top_val"]), _p(out["top_idx"]), _p(out["top_lab"]), _p(out["n_pos"]), _p(out["perr_hits"]), _p(out["class_pos"]),
              _stream())
    return out


ENSEMBLE_MAX_MEMBERS = 8   # evc_ensemble_topk_rows: 1 <= M <= 8 dense members, 0 <= P <= 8 sparse prior lists of 1 <= kp <= 256 entries
ENSEMBLE_MAX_PRIORS = 8
ENSEMBLE_MAX_KP = 256
ENSEMBLE_MODES = {"max": 0, "mean": 1}


def ensemble_topk_rows(preds, k, mode="max", weights=None, priors=None, dense=False):
    """The members' predictions combined and selected in one launch on the current stream (evc_ensemble_topk_rows).  preds: list of M
    2-D f32 device tensors of one shape (rows contiguous, any row stride); priors: None or (idx [P, B, kp] int32, val [P, B, kp] f32)
    on the device - the sparse (class, confidence) lists of P earlier prediction files for these rows, padded with idx = -1, classes
    distinct within a list.  mode "max": per class the largest value in the order of topk_rows, the lowest member on ties, then the
    prior files in order; "mean": w[0] x_0 + w[1] x_1 + ... + w[M + p] val_p left to right, one f32 rounding per operation, weights
    [M + P] (default np.float32(1) / np.float32(M + P) each).  Returns (values [B, k] f32, indices [B, k] int32) of the combined row in
    the order of topk_rows, and with dense=True also the combined [B, C] tensor; k = 0 needs dense=True and selects nothing."""
    import numpy as np
    preds = list(preds)
    M = len(preds)
    if not 1 <= M <= ENSEMBLE_MAX_MEMBERS:
        raise _lib.EvcError("ensemble_topk_rows: %d members (1 .. %d)" % (M, ENSEMBLE_MAX_MEMBERS))
    if mode not in ENSEMBLE_MODES:
        raise _lib.EvcError("ensemble_topk_rows: mode %r (max | mean)" % (mode,))
    x0 = preds[0]
    for x in preds:
        if not torch.is_tensor(x) or not x.is_cuda:
            raise _lib.EvcError("ensemble_topk_rows: evc ops need device tensors (got a CPU tensor); there is no CPU path")
        if x.dtype != F32 or x.dim() != 2 or (x.shape[0] > 0 and x.shape[1] > 1 and x.stride(1) != 1):
            raise _lib.EvcError("ensemble_topk_rows: needs 2-D float32 tensors with contiguous rows (got %s %s)" % (x.dtype, tuple(x.shape)))
        if tuple(x.shape) != tuple(x0.shape) or x.device != x0.device:
            raise _lib.EvcError("ensemble_topk_rows: members differ: %s on %s, %s on %s" % (tuple(x0.shape), x0.device, tuple(x.shape), x.device))
    B, cols = x0.shape
    P, kp, pidx, pval = 0, 0, None, None
    if priors is not None:
        pidx, pval = priors
        if (not pidx.is_cuda or not pval.is_cuda or pidx.device != x0.device or pval.device != x0.device or pidx.dtype != torch.int32
                or pval.dtype != F32 or pidx.dim() != 3 or tuple(pidx.shape) != tuple(pval.shape) or pidx.shape[1] != B
                or not pidx.is_contiguous() or not pval.is_contiguous()):
            raise _lib.EvcError("ensemble_topk_rows: priors are a contiguous (idx [P, %d, kp] int32, val [P, %d, kp] float32) pair on %s" % (B, B, x0.device))
        P, kp = int(pidx.shape[0]), int(pidx.shape[2])
        if P == 0:
            pidx = pval = None
        elif P > ENSEMBLE_MAX_PRIORS or not 1 <= kp <= ENSEMBLE_MAX_KP:
            raise _lib.EvcError("ensemble_topk_rows: %d prior lists of %d entries (at most %d of 1 .. %d)" % (P, kp, ENSEMBLE_MAX_PRIORS, ENSEMBLE_MAX_KP))
    if weights is None:
        w = np.full(M + P, np.float32(1) / np.float32(M + P), np.float32)
    else:
        if mode != "mean":
            raise _lib.EvcError("ensemble_topk_rows: weights are read in mode 'mean' only")
        w = np.ascontiguousarray(np.asarray(weights, np.float32).reshape(-1))
        if w.size != M + P:
            raise _lib.EvcError("ensemble_topk_rows: %d weights for %d members + %d prior lists" % (w.size, M, P))
    kk = int(k)
    if kk == 0 and not dense:
        raise _lib.EvcError("ensemble_topk_rows: k = 0 without dense=True asks for nothing")
    values = torch.empty((B, max(kk, 0)), dtype=F32, device=x0.device)
    indices = torch.empty((B, max(kk, 0)), dtype=torch.int32, device=x0.device)
    out = torch.empty((B, cols), dtype=F32, device=x0.device) if dense else None
    ptrs = (C.c_void_p * M)(*[x.data_ptr() for x in preds])
    lds = (C.c_int64 * M)(*[x.stride(0) if B > 1 else cols for x in preds])
    ws = (C.c_float * (M + P))(*w.tolist())
    _lib.call("evc_ensemble_topk_rows", ptrs, lds, ws, M, _p(pidx), _p(pval), P, kp, B, cols, ENSEMBLE_MODES[mode], kk,
              _p(values) if kk != 0 else None, _p(indices) if kk != 0 else None, _p(out), cols, _stream())
    return (values, indices, out) if dense else (values, indices)


CASCADE_CONFIDENCE = {"top1": 0, "margin": 1}   # the EVC_CONF_* codes of evc_cascade_confidence_rows
CASCADE_MAX_STAGES = 8
CASCADE_MAX_ROWS = 16384   # evc_cascade_pick_rows: the keys of one batch in LDS


def _cascade_vector(name, what, t, rows, dtype, device):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.EvcError("%s: evc ops need device tensors (got a CPU tensor for %s); there is no CPU path" % (name, what))
    if t.dtype != dtype or t.dim() != 1 or t.shape[0] != rows or not t.is_contiguous() or t.device != device:
        raise _lib.EvcError("%s: %s must be a contiguous %s [%d] on %s (got %s %s on %s)" % (name, what, dtype, rows, device, t.dtype, tuple(t.shape), t.device))


def cascade_confidence_rows(pred, kind, stage, conf, merged, stage_of, active=None):
    """The gate's first half on the current stream (evc_cascade_confidence_rows).  pred [B, C] f32 (rows contiguous, any row stride): the
    predictions of stage `stage`; active: None (every row) or uint8 [B], the rows that stage ran.  For those rows, in place: conf [B] f32 = the
    confidence (kind "top1": the row's largest value; "margin": largest - second largest, duplicates counted, one f32 subtraction; NaN for
    a row that holds one), merged [B, C] f32 = the row's bits, stage_of [B] uint8 = stage.  Every other row of the three is left untouched.
    Returns conf."""
    name = "cascade_confidence_rows"
    if kind not in CASCADE_CONFIDENCE:
        raise ValueError("%s: kind %r (%s)" % (name, kind, " | ".join(CASCADE_CONFIDENCE)))
    for what, x in (("pred", pred), ("merged", merged)):
        if not torch.is_tensor(x) or not x.is_cuda:
            raise _lib.EvcError("%s: evc ops need device tensors (got a CPU tensor for %s); there is no CPU path" % (name, what))
        if x.dtype != F32 or x.dim() != 2 or (x.shape[0] > 0 and x.shape[1] > 1 and x.stride(1) != 1):
            raise _lib.EvcError("%s: %s must be a 2-D float32 tensor with contiguous rows (got %s %s)" % (name, what, x.dtype, tuple(x.shape)))
    if tuple(merged.shape) != tuple(pred.shape) or merged.device != pred.device:
        raise _lib.EvcError("%s: pred %s on %s, merged %s on %s" % (name, tuple(pred.shape), pred.device, tuple(merged.shape), merged.device))
    B, cols = pred.shape
    _cascade_vector(name, "conf", conf, B, F32, pred.device)
    _cascade_vector(name, "stage_of", stage_of, B, torch.uint8, pred.device)
    if active is not None:
        _cascade_vector(name, "active", active, B, torch.uint8, pred.device)
    if not 0 <= int(stage) <= 255:
        raise ValueError("%s: stage %r (0 .. 255)" % (name, stage))
    _lib.call("evc_cascade_confidence_rows", _p(pred), pred.stride(0) if B > 1 else cols, _p(active), B, cols, CASCADE_CONFIDENCE[kind],
              int(stage), _p(conf), _p(merged), merged.stride(0) if B > 1 else cols, _p(stage_of), _stream())
    return conf


def cascade_pick_rows(conf, num_frames, threshold, max_rows=-1, active=None):
    """The gate's second half on the current stream (evc_cascade_pick_rows): which rows go on to the next stage.  conf [B] f32, num_frames [B]
    int32 (the batch's original counts), active None or uint8 [B].  Candidates: active rows for which conf >= threshold is false (NaN
    always); with max_rows >= 0 at most that many are kept, the least confident first (NaN, then conf ascending with -0 = +0, then the
    lower row).  Returns (active_next uint8 [B], num_frames_next int32 [B] = the counts of the kept rows and 0 elsewhere, count int32 [1])."""
    name = "cascade_pick_rows"
    if not torch.is_tensor(conf) or not conf.is_cuda:
        raise _lib.EvcError("%s: evc ops need device tensors (got a CPU tensor for conf); there is no CPU path" % name)
    if conf.dim() != 1:
        raise _lib.EvcError("%s: conf must be a float32 vector (got %s %s)" % (name, conf.dtype, tuple(conf.shape)))
    B = int(conf.shape[0])
    _cascade_vector(name, "conf", conf, B, F32, conf.device)
    _cascade_vector(name, "num_frames", num_frames, B, torch.int32, conf.device)
    if active is not None:
        _cascade_vector(name, "active", active, B, torch.uint8, conf.device)
    active_next = torch.empty(B, dtype=torch.uint8, device=conf.device)
    num_frames_next = torch.empty(B, dtype=torch.int32, device=conf.device)
    count = torch.zeros(1, dtype=torch.int32, device=conf.device) if B == 0 else torch.empty(1, dtype=torch.int32, device=conf.device)
    _lib.call("evc_cascade_pick_rows", _p(conf), _p(active), _p(num_frames), B, float(threshold), int(max_rows), _p(active_next),
              _p(num_frames_next), _p(count), _stream())
    return active_next, num_frames_next, count


# ---------------------------------------------------------------------------
def moe_tail_fwd(gate_logits, expert_logits, B, V, M, pred, rowsum):
    _lib.call("evc_moe_tail_fwd", _p(gate_logits), _p(expert_logits), B, V, M, _p(pred), _p(rowsum), _stream())


def moe_tail_bwd(gate_logits, expert_logits, dpred, B, V, M, dgate, dexpert):
    _lib.call("evc_moe_tail_bwd", _p(gate_logits), _p(expert_logits), _p(dpred), B, V, M, _p(dgate), dgate.stride(0),
              _p(dexpert), dexpert.stride(0), _stream())


def _ld_or_0(t):
    return t.stride(0) if t is not None else 0


def moe_grad_update(dlogits, x, rows, V, K, p, m, v, p_bf16, pT_bf16, l2_coeff, sums, partial_ws, clip_norm, lr_t,
                    beta1=0.9, beta2=0.999, eps=1e-8, phase=0, p_wide=None, p_f16=None, p_fp8=None):
    """Fused weight-gradient + per-tensor clip + TF-Adam of one MoE weight matrix (evc_moe_grad_update); phase 1 / 2:
    the norm pass / the update pass alone, for a row slab of a matrix sharded over ranks (evc_moe_grad_update_phase).
    p_wide [V][2K] bf16 / p_f16 [V][K] f16 + p_fp8 [V][2K] uint8 (phase 0 only): also receive the forward operand images of the new weights
    (evc_moe_grad_update_wide: the wide [hi | lo] split image / the f16 image and [e4m3(W_lo) | e4m3(W)])."""
    if p_wide is not None or p_f16 is not None:
        assert phase == 0 and (p_wide is None or (p_wide.dtype == BF16 and p_wide.shape == (V, 2 * K) and p_wide.is_contiguous()))
        assert (p_f16 is None) == (p_fp8 is None)
        if p_f16 is not None:
            assert p_f16.dtype == F16 and p_f16.shape == (V, K) and p_fp8.dtype == torch.uint8 and p_fp8.shape == (V, 2 * K) and p_f16.is_contiguous() and p_fp8.is_contiguous()
        _lib.call("evc_moe_grad_update_wide", _p(dlogits), dlogits.stride(0), _p(x), x.stride(0), rows, V, K, _p(p), _p(m), _p(v),
                  _p(p_bf16), _p(pT_bf16), _ld_or_0(pT_bf16), _p(p_wide), _p(p_f16), _p(p_fp8), FP8_MOE["w_lo_exp"], FP8_MOE["w_hi_exp"],
                  l2_coeff, _p(sums), _p(partial_ws), clip_norm, lr_t, beta1, beta2, eps, _stream())
        return
    _lib.call("evc_moe_grad_update_phase", _p(dlogits), dlogits.stride(0), _p(x), x.stride(0), rows, V, K, _p(p), _p(m), _p(v),
              _p(p_bf16), _p(pT_bf16), _ld_or_0(pT_bf16), l2_coeff, _p(sums), _p(partial_ws), clip_norm, lr_t, beta1, beta2, eps,
              phase, _stream())


def gram_slabs(A, R, Kc, S, slabs):
    """slabs[s] [R][R] f32 = A[:, slab s] . A[:, slab s]^T over S slabs of the first Kc columns of A (bf16, evc_gram_slabs)."""
    assert A.dtype == BF16 and slabs.dtype == F32 and slabs.numel() >= S * R * R
    _lib.call("evc_gram_slabs", _p(A), A.stride(0), R, Kc, S, _p(slabs), _stream())


def moe_grad_norms(gram_a, SA, gram_x, SX, R, dlogits, logits, bias, B, V, l2_coeff, wsq, part_ws, sums):
    """sums[0] += |dlogits^T x + l2 W|^2 from the two Gram matrices, the forward logits and the carried |W|^2 (evc_moe_grad_norms);
    sums[1] += |W|^2."""
    assert part_ws.numel() >= 256 + 4 * B and logits.dtype == F32
    _lib.call("evc_moe_grad_norms", _p(gram_a), SA, _p(gram_x), SX, R, _p(dlogits), dlogits.stride(0), _p(logits), logits.stride(0),
              _p(bias), B, V, l2_coeff, _p(wsq), _p(part_ws), _p(sums), _stream())


def moe_grad_update_apply(dlogits, x, rows, V, K, p, m, v, p_bf16, pT_bf16, l2_coeff, sums, partial_ws, clip_norm, lr_t, wsq_out,
                          beta1=0.9, beta2=0.999, eps=1e-8, p_wide=None, p_f16=None, p_fp8=None):
    """The update pass of evc_moe_grad_update alone (clip scale from sums[0]) + wsq_out[0] = sum of the new weights squared."""
    assert (p_f16 is None) == (p_fp8 is None)
    _lib.call("evc_moe_grad_update_apply", _p(dlogits), dlogits.stride(0), _p(x), x.stride(0), rows, V, K, _p(p), _p(m), _p(v),
              _p(p_bf16), _p(pT_bf16), _ld_or_0(pT_bf16), _p(p_wide), _p(p_f16), _p(p_fp8), FP8_MOE["w_lo_exp"], FP8_MOE["w_hi_exp"],
              l2_coeff, _p(sums), _p(partial_ws), clip_norm, lr_t, beta1, beta2, eps, _p(wsq_out), _stream())


def ce_loss(pred, labels_u8, loss, dpred=None, grad_scale=1.0, accumulate_grad=False):
    B, V = pred.shape
    if DETERMINISTIC:      # fixed-order loss sum from per-block partials (scratch from the stream-aware caching allocator)
        ws = torch.empty(256, dtype=F32, device=pred.device)
        _lib.call("evc_ce_loss_ordered", _p(pred), _p(labels_u8), B, V, grad_scale, _p(loss), _p(dpred), 1 if accumulate_grad else 0, _p(ws), _stream())
        return
    _lib.call("evc_ce_loss", _p(pred), _p(labels_u8), B, V, grad_scale, _p(loss), _p(dpred), 1 if accumulate_grad else 0, _stream())


# evc_label_loss kinds (include/evc.h EVC_LOSS_*): the label losses of cs/losses.py besides CrossEntropyLoss
LOSS_WITH_SPARSITY, LOSS_TOP50, LOSS_CLASS_IMBALANCE, LOSS_POSITIVES, LOSS_NEW, LOSS_HINGE, LOSS_SOFTMAX = 1, 2, 3, 4, 5, 6, 7
LABEL_LOSS_MAX_V = 32768


def label_loss(kind, pred, labels_u8, loss, dpred=None, grad_scale=1.0, accumulate_grad=False, class_weights=None):
    """loss[0] += mean_b row_loss_b of label loss ``kind`` (LOSS_*), dpred (= | +=) grad_scale * d(sum_b row_loss_b)/dpred
    (evc_label_loss: the contract of ce_loss; class_weights [V] f32 with LOSS_CLASS_IMBALANCE only).  Fixed summation order in every
    mode; scratch from the stream-aware caching allocator.  What the library refuses raises _lib.EvcError before any launch."""
    B, V = pred.shape
    assert pred.dtype == F32 and labels_u8.dtype == torch.uint8 and loss.dtype == F32 and labels_u8.shape == (B, V)
    assert pred.is_contiguous() and labels_u8.is_contiguous()
    assert dpred is None or (dpred.dtype == F32 and dpred.shape == (B, V) and dpred.is_contiguous())
    assert class_weights is None or (class_weights.dtype == F32 and class_weights.numel() == V and class_weights.is_contiguous())
    ws = torch.empty(max(B, 0) + 320, dtype=F32, device=pred.device)
    _lib.call("evc_label_loss", int(kind), _p(pred), _p(labels_u8), B, V, float(grad_scale), _p(class_weights), _p(loss), _p(dpred),
              1 if accumulate_grad else 0, _p(ws), _stream())


def kl_pred_loss(pred_t, rowsum_t, pred_s, rowsum_s, loss, dpred_s=None, grad_scale=1.0, accumulate_grad=False):
    B, V = pred_t.shape
    if DETERMINISTIC:      # the row sums joined in row order (scratch from the stream-aware caching allocator)
        ws = torch.empty(B, dtype=F32, device=pred_t.device)
        _lib.call("evc_kl_pred_loss_ordered", _p(pred_t), _p(rowsum_t), _p(pred_s), _p(rowsum_s), B, V, grad_scale, _p(loss), _p(dpred_s),
                  1 if accumulate_grad else 0, _p(ws), _stream())
        return
    _lib.call("evc_kl_pred_loss", _p(pred_t), _p(rowsum_t), _p(pred_s), _p(rowsum_s), B, V, grad_scale, _p(loss), _p(dpred_s),
              1 if accumulate_grad else 0, _stream())


def rep_loss(state_t, state_s, loss, dstate_s=None, grad_scale=1.0, accumulate_grad=False):
    B, D = state_t.shape
    if DETERMINISTIC:
        ws = torch.empty(256, dtype=F32, device=state_t.device)
        _lib.call("evc_rep_loss_ordered", _p(state_t), _p(state_s), B, D, grad_scale, _p(loss), _p(dstate_s), 1 if accumulate_grad else 0, _p(ws), _stream())
        return
    _lib.call("evc_rep_loss", _p(state_t), _p(state_s), B, D, grad_scale, _p(loss), _p(dstate_s), 1 if accumulate_grad else 0, _stream())


def distill_losses(pred_t, rowsum_t, pred_s, rowsum_s, labels_u8, state_t, state_s, losses, dpred_s=None, dstate_s=None,
                   g_ce=1.0, g_kl=1.0, g_rep=1.0):
    """The four losses of the serial distillation step in one launch + its finish (evc_distill_losses): losses[0:4] += (teacher CE,
    L_REP, L_PRED, student CE) - DistillGraph.LOSS_SLOTS -, dpred_s = g_ce dCE_s + g_kl dL_PRED (written once), dstate_s = g_rep dL_REP.
    The scales are the grad_scale arguments of ce_loss / kl_pred_loss / rep_loss; a scale of 0 leaves its term out of the gradient (its
    value is still reported).  Fixed summation order in every mode; scratch from the stream-aware caching allocator."""
    B, V = pred_t.shape
    D = state_t.shape[1]
    assert pred_s.shape == (B, V) and labels_u8.shape == (B, V) and state_s.shape == (B, D) and state_t.shape[0] == B
    assert rowsum_t.numel() >= B and rowsum_s.numel() >= B and losses.numel() >= 4
    assert pred_t.dtype == F32 and pred_s.dtype == F32 and state_t.dtype == F32 and state_s.dtype == F32 and labels_u8.dtype == torch.uint8
    for t in (pred_t, pred_s, labels_u8, state_t, state_s, losses):
        assert t.is_contiguous()
    for t, shp in ((dpred_s, (B, V)), (dstate_s, (B, D))):
        assert t is None or (t.dtype == F32 and t.shape == shp and t.is_contiguous())
    ws = torch.empty(3 * B + 256, dtype=F32, device=pred_t.device)
    _lib.call("evc_distill_losses", _p(pred_t), _p(rowsum_t), _p(pred_s), _p(rowsum_s), _p(labels_u8), _p(state_t), _p(state_s), B, V, D,
              float(g_ce), float(g_kl), float(g_rep), _p(losses), _p(dpred_s), _p(dstate_s), _p(ws), _stream())


DISTILL_MAX_STUDENTS = 8   # evc_distill_losses_multi: 1 <= K <= 8 students against one teacher


def distill_losses_multi(pred_t, rowsum_t, labels_u8, state_t, preds_s, rowsums_s, states_s, losses, dpreds_s=None, dstates_s=None,
                         g_ce=1.0, g_kl=1.0, g_rep=1.0):
    """distill_losses for K students against one teacher in one launch + its finish (evc_distill_losses_multi): the teacher's
    share of every element is computed once for all K (the prediction rows are read twice: double row sums first).  preds_s / rowsums_s / states_s: lists of K tensors; dpreds_s / dstates_s: None or lists
    of K tensors-or-None; g_ce / g_kl / g_rep: one number for all students or a sequence of K; losses [K, 4] += each student's four values
    (row k, DistillGraph.LOSS_SLOTS order; slot 0, the teacher's CE, is the same in every row).  Student k's outputs are the bits a
    K = 1 call on it alone gives, wherever it stands in the lists."""
    import ctypes as C
    K = len(preds_s)
    if not 1 <= K <= DISTILL_MAX_STUDENTS:
        raise ValueError("distill_losses_multi: %d students (1 .. %d)" % (K, DISTILL_MAX_STUDENTS))
    B, V = pred_t.shape
    D = state_t.shape[1]
    dpreds_s = [None] * K if dpreds_s is None else list(dpreds_s)
    dstates_s = [None] * K if dstates_s is None else list(dstates_s)
    assert len(rowsums_s) == len(states_s) == len(dpreds_s) == len(dstates_s) == K
    assert labels_u8.shape == (B, V) and state_t.shape[0] == B and rowsum_t.numel() >= B and tuple(losses.shape) == (K, 4)
    assert pred_t.dtype == F32 and state_t.dtype == F32 and labels_u8.dtype == torch.uint8 and losses.dtype == F32
    for t in (pred_t, labels_u8, state_t, losses):
        assert t.is_contiguous()
    for k in range(K):
        assert preds_s[k].shape == (B, V) and states_s[k].shape == (B, D) and rowsums_s[k].numel() >= B
        assert preds_s[k].dtype == F32 and states_s[k].dtype == F32 and preds_s[k].is_contiguous() and states_s[k].is_contiguous()
        for t, shp in ((dpreds_s[k], (B, V)), (dstates_s[k], (B, D))):
            assert t is None or (t.dtype == F32 and t.shape == shp and t.is_contiguous())
    scales = []
    for g in (g_ce, g_kl, g_rep):
        g = [float(g)] * K if isinstance(g, (int, float)) else [float(x) for x in g]
        assert len(g) == K
        scales.append((C.c_float * K)(*g))
    arr = lambda ts: (C.c_void_p * K)(*[_p(t) for t in ts])
    ws = torch.empty((1 + 2 * K) * B + 256 * K, dtype=F32, device=pred_t.device)
    _lib.call("evc_distill_losses_multi", _p(pred_t), _p(rowsum_t), _p(labels_u8), _p(state_t), K, arr(preds_s), arr(rowsums_s),
              arr(states_s), scales[0], scales[1], scales[2], arr(dpreds_s), arr(dstates_s), B, V, D, _p(losses), _p(ws), _stream())


DISTILL_MAX_TEACHERS = 8   # evc_distill_losses_ensemble: one student against 1 <= J <= 8 teachers


def distill_losses_ensemble(preds_t, states_t, labels_u8, pred_s, state_s, losses, dpred_s=None, dstate_s=None, mode="mean", weights=None,
                            rep_weights=None, g_ce=1.0, g_kl=1.0, g_rep=1.0, teacher_ce=None, pred_comb=None):
    """distill_losses for one student against J teachers in one launch + its finish (evc_distill_losses_ensemble).  preds_t: list of J
    [B, V] f32 tensors, combined as ensemble_topk_rows(dense=True) combines them (mode "max" | "mean"; weights [J], mean only, default
    np.float32(1) / np.float32(J) each); states_t: list of J [B, D] tensors, or None where rep_weights[j] == 0 (rep_weights default
    1, 0, ..., 0: the state of entry 0); the combined state is rep_weights[j] * states_t[j] summed left to right in f32.  losses[0:4] +=
    (CE of the combined row, L_REP, L_PRED, student CE); teacher_ce [J] (optional) += each teacher's own CE; pred_comb [B, V] (optional)
    receives the combined row.  For a given combined row and state the outputs do not depend on J."""
    import ctypes as C
    import numpy as np
    preds_t = list(preds_t)
    J = len(preds_t)
    if not 1 <= J <= DISTILL_MAX_TEACHERS:
        raise ValueError("distill_losses_ensemble: %d teachers (1 .. %d)" % (J, DISTILL_MAX_TEACHERS))
    if mode not in ENSEMBLE_MODES:
        raise ValueError("distill_losses_ensemble: mode %r (max | mean)" % (mode,))
    if weights is None:
        w = np.full(J, np.float32(1) / np.float32(J), np.float32)
    else:
        if mode != "mean":
            raise ValueError("distill_losses_ensemble: weights are read in mode 'mean' only")
        w = np.asarray(weights, np.float32).reshape(-1)
    r = np.asarray([1.0] + [0.0] * (J - 1) if rep_weights is None else rep_weights, np.float32).reshape(-1)
    states_t = [None] * J if states_t is None else list(states_t)
    if w.size != J or r.size != J or len(states_t) != J:
        raise ValueError("distill_losses_ensemble: %d weights, %d rep_weights, %d states for %d teachers" % (w.size, r.size, len(states_t), J))
    B, V = pred_s.shape
    D = state_s.shape[1]
    if not r.any() and (g_rep != 0.0 or dstate_s is not None):
        raise ValueError("distill_losses_ensemble: every rep_weight is 0: no combined state for L_REP's gradient (g_rep = 0 and no dstate_s only)")
    assert labels_u8.shape == (B, V) and state_s.shape[0] == B and losses.numel() >= 4
    assert pred_s.dtype == F32 and state_s.dtype == F32 and labels_u8.dtype == torch.uint8 and losses.dtype == F32
    for t in (pred_s, labels_u8, state_s, losses):
        assert t.is_cuda and t.is_contiguous()
    for j in range(J):
        assert preds_t[j].shape == (B, V) and preds_t[j].dtype == F32 and preds_t[j].is_contiguous() and preds_t[j].is_cuda
        if r[j] != 0:
            if states_t[j] is None:
                raise ValueError("distill_losses_ensemble: teacher %d has rep_weight %g and no state" % (j, r[j]))
            assert states_t[j].shape == (B, D) and states_t[j].dtype == F32 and states_t[j].is_contiguous()
    for t, shp in ((dpred_s, (B, V)), (dstate_s, (B, D)), (pred_comb, (B, V))):
        assert t is None or (t.dtype == F32 and t.shape == shp and t.is_contiguous())
    assert teacher_ce is None or (teacher_ce.dtype == F32 and teacher_ce.numel() >= J and teacher_ce.is_contiguous())
    arr = lambda ts: (C.c_void_p * J)(*[_p(t) for t in ts])
    ws = torch.empty((3 + J) * B + 256, dtype=F32, device=pred_s.device)
    _lib.call("evc_distill_losses_ensemble", J, arr(preds_t), arr([s if r[j] != 0 else None for j, s in enumerate(states_t)]),
              (C.c_float * J)(*w.tolist()), (C.c_float * J)(*r.tolist()), ENSEMBLE_MODES[mode], _p(labels_u8), _p(pred_s), _p(state_s),
              B, V, D, float(g_ce), float(g_kl), float(g_rep), _p(losses), _p(teacher_ce), _p(pred_comb), _p(dpred_s), _p(dstate_s), _p(ws),
              _stream())


DISTILL_MAX_FILES = 8      # evc_distill_losses_sparse: one student against 1 <= F <= 8 sparse lists of 1 <= kp <= 256 entries, V <= 32768
DISTILL_SPARSE_MAX_V = 32768


def distill_losses_sparse(prior_idx, prior_val, labels_u8, pred_s, losses, dpred_s=None, mode="mean", weights=None, g_ce=1.0, g_kl=1.0,
                          pred_comb=None):
    """The loss section of the offline distillation step in one launch + its finish (evc_distill_losses_sparse): one student against
    the sparse (class, confidence) lists of F prediction files.  prior_idx [F, B, kp] int32 / prior_val [F, B, kp] f32 on the device, as
    ensemble_topk_rows takes its priors (idx = -1 pads, classes distinct within a list); they are scattered into one combined row per
    video exactly as ensemble_topk_rows(dense=True) scatters them over one all-zero member (mode "max" | "mean"; weights [F], mean only,
    default np.float32(1) / np.float32(F) each).  losses[0] += CE of the combined row, losses[2] += L_PRED, losses[3] += student CE
    (DistillGraph.LOSS_SLOTS; slot 1, L_REP, is left alone: a prediction file holds no state); dpred_s [B, V] (optional) = g_ce dCE_s +
    g_kl dL_PRED, written once; pred_comb [B, V] (optional) receives the combined row."""
    import ctypes as C
    import numpy as np
    if mode not in ENSEMBLE_MODES:
        raise ValueError("distill_losses_sparse: mode %r (max | mean)" % (mode,))
    for t in (prior_idx, prior_val, labels_u8, pred_s, losses):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise _lib.EvcError("distill_losses_sparse: evc ops need device tensors (got a CPU tensor); there is no CPU path")
    if (prior_idx.dtype != torch.int32 or prior_val.dtype != F32 or prior_idx.dim() != 3 or tuple(prior_idx.shape) != tuple(prior_val.shape)
            or not prior_idx.is_contiguous() or not prior_val.is_contiguous()):
        raise ValueError("distill_losses_sparse: the lists are a contiguous (idx [F, B, kp] int32, val [F, B, kp] float32) pair")
    F, B, kp = (int(x) for x in prior_idx.shape)
    if not 1 <= F <= DISTILL_MAX_FILES or not 1 <= kp <= ENSEMBLE_MAX_KP:
        raise ValueError("distill_losses_sparse: %d lists of %d entries (1 .. %d of 1 .. %d)" % (F, kp, DISTILL_MAX_FILES, ENSEMBLE_MAX_KP))
    if pred_s.dim() != 2 or pred_s.shape[0] != B:
        raise ValueError("distill_losses_sparse: pred_s %s for lists of %d rows" % (tuple(pred_s.shape), B))
    V = int(pred_s.shape[1])
    if not 1 <= V <= DISTILL_SPARSE_MAX_V:
        raise ValueError("distill_losses_sparse: %d classes (1 .. %d: the combined row is built in LDS)" % (V, DISTILL_SPARSE_MAX_V))
    if weights is None:
        w = np.full(F, np.float32(1) / np.float32(F), np.float32)
    else:
        if mode != "mean":
            raise ValueError("distill_losses_sparse: weights are read in mode 'mean' only")
        w = np.asarray(weights, np.float32).reshape(-1)
        if w.size != F:
            raise ValueError("distill_losses_sparse: %d weights for %d lists" % (w.size, F))
    assert labels_u8.shape == (B, V) and losses.numel() >= 4
    assert pred_s.dtype == F32 and labels_u8.dtype == torch.uint8 and losses.dtype == F32
    for t in (pred_s, labels_u8, losses):
        assert t.is_contiguous()
    for t in (dpred_s, pred_comb):
        assert t is None or (t.is_cuda and t.dtype == F32 and t.shape == (B, V) and t.is_contiguous())
    ws = torch.empty(3 * max(B, 1), dtype=F32, device=pred_s.device)
    _lib.call("evc_distill_losses_sparse", F, _p(prior_idx), _p(prior_val), kp, (C.c_float * F)(*w.tolist()), ENSEMBLE_MODES[mode],
              _p(labels_u8), _p(pred_s), B, V, float(g_ce), float(g_kl), _p(losses), _p(pred_comb), _p(dpred_s), _p(ws), _stream())


def clip_adam_small(ps, gs, ms, vs, sums, clip_norm, lr_t, beta1=0.9, beta2=0.999, eps=1e-8):
    """Per-tensor clip + TF-Adam of up to 16 small tensors (no l2 term) in one launch (evc_clip_adam_small): sums[i] receives {|g_i|^2, 0}."""
    import ctypes as C
    k = len(ps)
    assert 1 <= k <= 16 and len(gs) == len(ms) == len(vs) == len(sums) == k
    arr = lambda ts: (C.c_void_p * k)(*[_p(t) for t in ts])
    n = (C.c_int64 * k)(*[t.numel() for t in ps])
    _lib.call("evc_clip_adam_small", k, arr(ps), arr(gs), arr(ms), arr(vs), n, arr(sums), clip_norm, lr_t, beta1, beta2, eps, _stream())


def grad_sqnorm(g, p, l2_coeff, sums):
    _lib.call("evc_grad_sqnorm", _p(g), _p(p), l2_coeff, g.numel(), _p(sums), _stream())


def lstm_adam_fused(p, g, m, v, pb, gb, mb, vb, part_ws, sums_w, sums_b, clip_norm, lr_t, p_bf16, pT_bf16, beta1=0.9, beta2=0.999, eps=1e-8,
                    p_f16=None, nin=0, nseg=1, p_fp8=None, fp8_col0=0, fp8_hi_cols=0, fp8_lo_exp=FP8_W_SCALE_EXP, fp8_hi_exp=FP8_WX_HI_EXP, fp8_hi_tail=False):
    """Clip + TF-Adam of one LSTM layer's kernel p [4H][C] and bias pb [4H] with every operand image of the new kernel written from the same
    pass (evc_sqnorm2_partials + evc_lstm_adam_fused): bf16 forward shadow, gate-interleaved transposed bf16 backward shadow, and in "high"
    precision the f16 image (cast_f16 / cast_f16_wide without h_ext) and the e4m3 low-order image (cast_fp8_lo of the columns from fp8_col0)."""
    R, C = p.shape
    assert R % 64 == 0 and p.is_contiguous() and g.is_contiguous() and part_ws.numel() >= 1025 and pT_bf16.shape[0] == C
    assert p_f16 is None or (p_f16.dtype == F16 and p_f16.shape == (R, nseg * nin + (C - nin)) and p_f16.is_contiguous())
    assert p_fp8 is None or (p_fp8.dtype == torch.uint8 and p_fp8.shape == (R, 2 * (C - fp8_col0) if fp8_hi_tail else C - fp8_col0 + fp8_hi_cols) and p_fp8.is_contiguous())
    _lib.call("evc_sqnorm2_partials", _p(g), g.numel(), _p(gb), gb.numel(), _p(part_ws), _stream())
    _lib.call("evc_lstm_adam_fused", _p(p), _p(g), _p(m), _p(v), _p(pb), _p(gb), _p(mb), _p(vb), R // 4, C, _p(part_ws), _p(sums_w), _p(sums_b),
              clip_norm, lr_t, beta1, beta2, eps, _p(p_bf16), _p(pT_bf16), pT_bf16.stride(0), _p(p_f16), p_f16.stride(0) if p_f16 is not None else 0,
              nin, nseg, _p(p_fp8), p_fp8.stride(0) if p_fp8 is not None else 0, fp8_col0, fp8_hi_cols, fp8_lo_exp, fp8_hi_exp, 1 if fp8_hi_tail else 0, _stream())


def adam2d_fused(p, g, m, v, part_ws, sums_w, clip_norm, lr_t, p_bf16, pT_bf16, beta1=0.9, beta2=0.999, eps=1e-8,
                 p_f16=None, p_fp8=None, fp8_hi_cols=0, fp8_lo_exp=FP8_W_SCALE_EXP, fp8_hi_exp=FP8_WX_HI_EXP):
    """lstm_adam_fused for a plain 2-D weight p [R][C] without a bias (evc_sqnorm2_partials + evc_adam2d_fused): clip + TF-Adam, bf16 forward shadow,
    transposed bf16 backward shadow (pad columns zeroed) and the optional f16 / e4m3 images, one pass over the weights."""
    R, C = p.shape
    assert p.is_contiguous() and g.is_contiguous() and part_ws.numel() >= 1025 and pT_bf16.shape[0] == C and pT_bf16.stride(0) >= round_up(R, 64)
    assert p_f16 is None or (p_f16.dtype == F16 and p_f16.shape == (R, C) and p_f16.is_contiguous())
    assert p_fp8 is None or (p_fp8.dtype == torch.uint8 and p_fp8.shape == (R, C + fp8_hi_cols) and p_fp8.is_contiguous())
    _lib.call("evc_sqnorm2_partials", _p(g), g.numel(), None, 0, _p(part_ws), _stream())
    _lib.call("evc_adam2d_fused", _p(p), _p(g), _p(m), _p(v), R, C, _p(part_ws), _p(sums_w), clip_norm, lr_t, beta1, beta2, eps, _p(p_bf16), _p(pT_bf16),
              pT_bf16.stride(0), _p(p_f16), C if p_f16 is not None else 0, _p(p_fp8), p_fp8.stride(0) if p_fp8 is not None else 0, fp8_hi_cols,
              fp8_lo_exp, fp8_hi_exp, _stream())


def clip_adam_step(p, g, m, v, l2_coeff, sums, clip_norm, lr_t, beta1=0.9, beta2=0.999, eps=1e-8, p_bf16=None):
    _lib.call("evc_clip_adam_step", _p(p), _p(g), _p(m), _p(v), p.numel(), l2_coeff, _p(sums), clip_norm, lr_t, beta1, beta2, eps,
              _p(p_bf16), _stream())


def meanpool(x, num_frames, avg_f32, avg_bf16=None, normalize=False):
    B, T, F = x.shape
    is_u8 = x.dtype == torch.uint8
    _lib.call("evc_meanpool_fwd", None if is_u8 else _p(x), _p(x) if is_u8 else None, _p(num_frames), B, T, F, 1 if normalize else 0, _p(avg_f32), _p(avg_bf16), _stream())


def sigmoid_(z):
    _lib.call("evc_sigmoid_fwd", _p(z), z.numel(), _stream())
    return z


def sigmoid_bwd(p, dp, dz):
    _lib.call("evc_sigmoid_bwd", _p(p), _p(dp), p.numel(), _p(dz), _stream())


def sample_frames_gather(x, u, num_frames, out, idx_out=None, normalize=False):
    B, T, F = x.shape
    S = u.shape[1]
    is_u8 = x.dtype == torch.uint8
    _lib.call("evc_sample_frames_gather", None if is_u8 else _p(x), _p(x) if is_u8 else None, _p(u), _p(num_frames), B, T, F, S,
              1 if normalize else 0, _p(out), _p(idx_out), _stream())


def sample_sequence_gather(x, u, num_frames, S, out, idx_out=None, normalize=False):
    """SampleRandomSequence (cs/model_utils.py:11-36): u [B] one draw per video, S consecutive frames."""
    B, T, F = x.shape
    is_u8 = x.dtype == torch.uint8
    _lib.call("evc_sample_sequence_gather", None if is_u8 else _p(x), _p(x) if is_u8 else None, _p(u), _p(num_frames), B, T, F, S,
              1 if normalize else 0, _p(out), _p(idx_out), _stream())


def relu6_fwd(x, y_f32=None, y_bf16=None):
    _lib.call("evc_relu6_fwd", _p(x), x.numel(), _p(y_f32), _p(y_bf16), _stream())


def relu6_bwd(x, dy, dx_f32=None, dx_bf16=None):
    _lib.call("evc_relu6_bwd", _p(x), _p(dy), x.numel(), _p(dx_f32), _p(dx_bf16), _stream())


def framepool_mean_fwd(y, B, S, Cc, pooled_f32=None, pooled_bf16=None):
    _lib.call("evc_framepool_mean_fwd", _p(y), B, S, Cc, _p(pooled_f32), _p(pooled_bf16), _stream())


def framepool_mean_bwd(dpooled, B, S, Cc, dy):
    _lib.call("evc_framepool_mean_bwd", _p(dpooled), B, S, Cc, _p(dy), _stream())


def bn_stats(x, R, Cc, ws, mean, var):
    _lib.call("evc_bn_stats", _p(x), R, Cc, _p(ws), _p(mean), _p(var), _stream())


def bn_stats_partial(x, R, Cc, ws):
    _lib.call("evc_bn_stats_partial", _p(x), R, Cc, _p(ws), _stream())


def bn_stats_finalize(ws, R_total, Cc, mean, var):
    _lib.call("evc_bn_stats_finalize", _p(ws), R_total, Cc, _p(mean), _p(var), _stream())


def ema_update(moving, batch_value, decay=0.999):
    _lib.call("evc_ema_update", _p(moving), _p(batch_value), decay, moving.numel(), _stream())


def bn_apply(x, R, Cc, mean, var, gamma, beta, relu6, y_f32=None, y_bf16=None):
    _lib.call("evc_bn_apply", _p(x), R, Cc, _p(mean), _p(var), _p(gamma), _p(beta), 1 if relu6 else 0, _p(y_f32), _p(y_bf16), _stream())


def bn_bwd_partial(x, dy, R, Cc, mean, var, gamma, beta, relu6, ws, argmax=None, S=1):
    _lib.call("evc_bn_bwd_partial", _p(x), _p(dy), R, Cc, _p(mean), _p(var), _p(gamma), _p(beta), 1 if relu6 else 0,
              _p(argmax), S, _p(ws), _stream())


def bn_bwd_finalize(x, dy, R, R_total, Cc, mean, var, gamma, beta, relu6, ws, argmax=None, S=1,
                    dx_f32=None, dx_bf16=None, dgamma=None, dbeta=None):
    _lib.call("evc_bn_bwd_finalize", _p(x), _p(dy), R, R_total, Cc, _p(mean), _p(var), _p(gamma), _p(beta),
              1 if relu6 else 0, _p(argmax), S, _p(ws), _p(dx_f32), _p(dx_bf16), _p(dgamma), _p(dbeta), _stream())


def bn_bwd_partial_add(x, dy, dy2, R, Cc, mean, var, gamma, beta, relu6, ws, argmax=None, S=1):
    """bn_bwd_partial on the gradient dy + dy2 (dy2 [R, Cc] f32 or None: the plain entry's launch and bits)."""
    _lib.call("evc_bn_bwd_partial_add", _p(x), _p(dy), _p(dy2), R, Cc, _p(mean), _p(var), _p(gamma), _p(beta), 1 if relu6 else 0,
              _p(argmax), S, _p(ws), _stream())


def bn_bwd_finalize_add(x, dy, dy2, R, R_total, Cc, mean, var, gamma, beta, relu6, ws, argmax=None, S=1,
                        dx_f32=None, dx_bf16=None, dgamma=None, dbeta=None):
    """bn_bwd_finalize on the gradient dy + dy2, after bn_bwd_partial_add on the same pair."""
    _lib.call("evc_bn_bwd_finalize_add", _p(x), _p(dy), _p(dy2), R, R_total, Cc, _p(mean), _p(var), _p(gamma), _p(beta),
              1 if relu6 else 0, _p(argmax), S, _p(ws), _p(dx_f32), _p(dx_bf16), _p(dgamma), _p(dbeta), _stream())


def bn_gate_fwd(gl, h, R, Cc, mean, var, gamma, beta, out):
    """out = h * sigmoid(bn(gl)): bn_apply and nextvlad_gate_fwd in one pass, their bits."""
    _lib.call("evc_bn_gate_fwd", _p(gl), _p(h), R, Cc, _p(mean), _p(var), _p(gamma), _p(beta), _p(out), _stream())


def bn_gate_bwd_partial(gl, h, d, d2, R, Cc, mean, var, gamma, beta, ws, dh):
    """bn_bwd_partial on dy = e * h * g * (1 - g), e = d (+ d2, None allowed), g recomputed from gl; stores dh = e * g."""
    _lib.call("evc_bn_gate_bwd_partial", _p(gl), _p(h), _p(d), _p(d2), R, Cc, _p(mean), _p(var), _p(gamma), _p(beta), _p(ws), _p(dh), _stream())


def bn_gate_bwd_finalize(gl, h, d, d2, R, R_total, Cc, mean, var, gamma, beta, ws, dgl_f32=None, dgl_bf16=None, dgamma=None, dbeta=None):
    """bn_bwd_finalize on the same dy, after bn_gate_bwd_partial on the same operands."""
    _lib.call("evc_bn_gate_bwd_finalize", _p(gl), _p(h), _p(d), _p(d2), R, R_total, Cc, _p(mean), _p(var), _p(gamma), _p(beta), _p(ws),
              _p(dgl_f32), _p(dgl_bf16), _p(dgamma), _p(dbeta), _stream())


def bn_relu6_framepool_fwd(act, B, S, Cc, mean, var, gamma, beta, pooled_f32, pooled_bf16, argmax):
    _lib.call("evc_bn_relu6_framepool_fwd", _p(act), B, S, Cc, _p(mean), _p(var), _p(gamma), _p(beta), _p(pooled_f32),
              _p(pooled_bf16), _p(argmax), _stream())


def framepool_max_fwd(y, B, S, Cc, pooled_f32, pooled_bf16, argmax):
    _lib.call("evc_framepool_max_fwd", _p(y), B, S, Cc, _p(pooled_f32), _p(pooled_bf16), _p(argmax), _stream())


def framepool_max_bwd(dpooled, argmax, B, S, Cc, dy):
    _lib.call("evc_framepool_max_bwd", _p(dpooled), _p(argmax), B, S, Cc, _p(dy), _stream())


# ---------------------------------------------------------------------------
# DbofModel fused path (csrc/evc_dbof.hip)
def dbof_workspace(B, S):
    """(padded_rows, gather_part_rows, gemm_part_rows) of the padded frame layout for B videos x S sampled frames."""
    a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
    _lib.call("evc_dbof_workspace", B, S, C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def dbof_row_index(B, S, device=None):
    """int64 [B, S]: row of frame s of video b in the padded frame layout (tests / debugging; the kernels compute it)."""
    b = torch.arange(B, device=device)[:, None]
    s = torch.arange(S, device=device)[None, :]
    return (b >> 2) * 128 + (s >> 2) * 16 + (b & 3) * 4 + (s & 3)


def dbof_gather(x, u, num_frames, r, idx_out=None, part=None, normalize=True):
    B, T, F = x.shape
    S = u.shape[1]
    is_u8 = x.dtype == torch.uint8
    assert is_u8 or x.dtype == F32
    _lib.call("evc_dbof_gather", None if is_u8 else _p(x), _p(x) if is_u8 else None, _p(u), _p(num_frames), B, T, F, S,
              1 if normalize else 0, _p(r), _p(idx_out), _p(part), _stream())


def bn_partials_reduce(part, P, Cc, ws):
    _lib.call("evc_bn_partials_reduce", _p(part), P, Cc, _p(ws), _stream())


def bn_finalize_ema(ws, R_total, Cc, mean, var, moving_mean=None, moving_var=None, decay=0.999):
    _lib.call("evc_bn_finalize_ema", _p(ws), R_total, Cc, _p(mean), _p(var), _p(moving_mean), _p(moving_var), decay, _stream())


def dbof_input_bn_apply(r, B, S, F, mean, var, gamma, beta, r_bn, r_bn_lo=None, xhat=None):
    _lib.call("evc_dbof_input_bn_apply", _p(r), B, S, F, _p(mean), _p(var), _p(gamma), _p(beta), _p(r_bn), _p(r_bn_lo), _p(xhat),
              _stream())


def dbof_cluster_pool_fwd(r_bn, wT, B, S, F, Cc, gamma, xsel, arg, act=None, part=None, r_bn_lo=None, wT_lo=None):
    _lib.call("evc_dbof_cluster_pool_fwd", _p(r_bn), _p(r_bn_lo), _p(wT), _p(wT_lo), B, S, F, Cc, _p(gamma), _p(act), _p(part),
              _p(xsel), _p(arg), _stream())


FP8_DBOF_CLUSTER = dict(x_hi_exp=5, x_lo_exp=16, w_lo_exp=19, w_hi_exp=8)   # batch-normalised frames |y| < 14, cluster weights |W| < 1.75: 5 + 19 = 16 + 8 = 24


def dbof_input_bn_apply_f16fp8(r, B, S, F, mean, var, gamma, beta, r_rows, xhat=None, e=FP8_DBOF_CLUSTER):
    """dbof_input_bn_apply writing rows [f16(y) | e4m3(y 2^x_hi_exp) | e4m3((y - f16(y)) 2^x_lo_exp)] (r_rows [Mp][2F] f16 containers)."""
    assert r_rows.dtype == F16 and r_rows.shape[1] == 2 * F and r_rows.is_contiguous()
    _lib.call("evc_dbof_input_bn_apply_f16fp8", _p(r), B, S, F, _p(mean), _p(var), _p(gamma), _p(beta), _p(r_rows), e["x_hi_exp"], e["x_lo_exp"],
              _p(xhat), _stream())


def dbof_cluster_pool_fwd_f16fp8(r_rows, wT16, wT8, B, S, F, Cc, gamma, xsel, arg, act=None, part=None, e=FP8_DBOF_CLUSTER):
    """dbof_cluster_pool_fwd on f16 + e4m3 operands (evc_dbof_cluster_pool_fwd_f16fp8): wT16 [C][F] f16, wT8 [C][2F] uint8 from
    cast_fp8_lo(W, hi_cols=F, scale_exp=w_lo_exp, hi_exp=w_hi_exp)."""
    assert r_rows.dtype == F16 and wT16.dtype == F16 and wT16.shape == (Cc, F) and wT8.dtype == torch.uint8 and wT8.shape == (Cc, 2 * F)
    assert e["x_hi_exp"] + e["w_lo_exp"] == e["x_lo_exp"] + e["w_hi_exp"]
    _lib.call("evc_dbof_cluster_pool_fwd_f16fp8", _p(r_rows), _p(wT16), _p(wT8), -(e["x_hi_exp"] + e["w_lo_exp"]), B, S, F, Cc, _p(gamma),
              _p(act), _p(part), _p(xsel), _p(arg), _stream())


def dbof_pool_finish(xsel, B, Cc, mean, var, gamma, beta, pooled_f32, pooled_bf16=None, pooled_lo=None):
    _lib.call("evc_dbof_pool_finish", _p(xsel), B, Cc, _p(mean), _p(var), _p(gamma), _p(beta), _p(pooled_f32), _p(pooled_bf16),
              _p(pooled_lo), _stream())


def dbof_dact(act, dpooled, pooled, arg, mean, var, gamma, ws, R_total, B, S, Cc, dgamma=None, dbeta=None):
    _lib.call("evc_dbof_dact", _p(act), _p(dpooled), _p(pooled), _p(arg), _p(mean), _p(var), _p(gamma), _p(ws), R_total, B, S, Cc,
              _p(dgamma), _p(dbeta), _stream())


def gemm_tn_slabs(A, B, M, N, K, slabs, nslab):
    """slabs[s] [M,N] f32 = partial product of A[K,M]^T @ B[K,N] over the s-th K range."""
    assert A.dtype == BF16 and B.dtype == BF16 and slabs.dtype == F32
    _lib.call("evc_gemm_tn_slabs", _p(A), A.stride(0), _p(B), B.stride(0), _p(slabs), M, N, K, nslab, _stream())


def dbof_wgrad_finish(slabs, nslab, Cc, F, W, gamma_in, dW, dgamma_in, dbeta_in=None, part_ws=None):
    if part_ws is None:
        part_ws = torch.empty(((Cc + 7) // 8, F), dtype=F32, device=dW.device)
    _lib.call("evc_dbof_wgrad_finish", _p(slabs), nslab, Cc, F, _p(W), _p(gamma_in), _p(dW), _p(dgamma_in), _p(dbeta_in), _p(part_ws),
              _stream())


# ---------------------------------------------------------------------------
# NetVLAD aggregation (csrc/evc_netvlad.hip; extension, see towers.NetVladTower)
def netvlad_softmax_fwd(act, R, K, mean, var, gamma, beta, a):
    _lib.call("evc_netvlad_softmax_fwd", _p(act), R, K, _p(mean), _p(var), _p(gamma), _p(beta), _p(a), _stream())


def netvlad_softmax_bwd(a, da, R, K, dz):
    _lib.call("evc_netvlad_softmax_bwd", _p(a), _p(da), R, K, _p(dz), _stream())


def netvlad_aggregate_fwd(a, r, B, S, K, F, mean, var, gamma, beta, c2, V, asum):
    _lib.call("evc_netvlad_aggregate_fwd", _p(a), _p(r), B, S, K, F, _p(mean), _p(var), _p(gamma), _p(beta), _p(c2), _p(V), _p(asum), _stream())


def netvlad_aggregate_bwd(a, r, B, S, K, F, mean, var, gamma, beta, c2, dV, da, dx):
    _lib.call("evc_netvlad_aggregate_bwd", _p(a), _p(r), B, S, K, F, _p(mean), _p(var), _p(gamma), _p(beta), _p(c2), _p(dV), _p(da), _p(dx),
              _stream())


def netvlad_aggregate_packed_fwd(a, r, row_off, B, T, K, F, R, max_k, mean, var, gamma, beta, c2, V, asum):
    """netvlad_aggregate_fwd over packed rows: video b's a / r rows are row_off[b] .. row_off[b+1] (device int32 [B+1],
    GridPlan.row_off), any number of them up to T; on the f32 matrix cores, for training and forward-only towers alike."""
    assert row_off.dtype == torch.int32 and row_off.numel() == B + 1
    assert a.numel() >= R * K and r.numel() >= R * F and V.numel() >= B * K * F and asum.numel() >= B * K
    _lib.call("evc_netvlad_aggregate_packed_fwd", _p(a), _p(r), _p(row_off), B, T, K, F, R, max_k, _p(mean), _p(var), _p(gamma), _p(beta),
              _p(c2), _p(V), _p(asum), _stream())


def netvlad_aggregate_packed_bwd_ws(B, K, F):
    """Floats of scratch evc_netvlad_aggregate_packed_bwd needs: dV transposed [B][F][K rounded up to 4] and q [B][K]."""
    return B * F * round_up(K, 4) + B * K


def netvlad_aggregate_packed_bwd(a, r, row_off, B, T, K, F, R, max_k, mean, var, gamma, beta, c2, dV, da, dx, ws=None):
    """netvlad_aggregate_bwd over packed rows: the R live rows of da and dx are written, nothing beyond them."""
    assert row_off.dtype == torch.int32 and row_off.numel() == B + 1
    assert a.numel() >= R * K and r.numel() >= R * F and da.numel() >= R * K and dx.numel() >= R * F and dV.numel() >= B * K * F
    if ws is None:
        ws = torch.empty(netvlad_aggregate_packed_bwd_ws(B, K, F), dtype=F32, device=da.device)
    _lib.call("evc_netvlad_aggregate_packed_bwd", _p(a), _p(r), _p(row_off), B, T, K, F, R, max_k, _p(mean), _p(var), _p(gamma), _p(beta),
              _p(c2), _p(dV), _p(da), _p(dx), _p(ws), ws.numel(), _stream())


def netvlad_dcenters(asum, dV, B, K, F, dc2):
    _lib.call("evc_netvlad_dcenters", _p(asum), _p(dV), B, K, F, _p(dc2), _stream())


def netvlad_normalize_fwd(V, B, K, F, n1, n2, Y_bf16, Y_f32=None):
    _lib.call("evc_netvlad_normalize_fwd", _p(V), B, K, F, _p(n1), _p(n2), _p(Y_f32), _p(Y_bf16), _stream())


def netvlad_normalize_bwd(V, n1, n2, dY, B, K, F, dV):
    _lib.call("evc_netvlad_normalize_bwd", _p(V), _p(n1), _p(n2), _p(dY), B, K, F, _p(dV), _stream())


# ---------------------------------------------------------------------------
# NeXtVLAD aggregation (csrc/evc_nextvlad.hip; extension, see towers.NeXtVladTower and DESIGN.md 7.12)
def nextvlad_assign_fwd(act, R, G, K, mean, var, gamma, beta, att_logits, a, att_bias=None):
    """a [R,G,K] = softmax_k(cluster_bn(act)) * sigmoid(att_logits[:, :G] (+ att_bias)); att_logits f32 [R, ld >= G]."""
    _lib.call("evc_nextvlad_assign_fwd", _p(act), R, G, K, _p(mean), _p(var), _p(gamma), _p(beta), _p(att_logits), att_logits.stride(0),
              _p(att_bias), _p(a), _stream())


def nextvlad_assign_bwd(act, R, G, K, mean, var, gamma, beta, att_logits, da, dz, datt_logit, att_bias=None, datt_logit_bf16=None):
    """dz [R,G*K] and datt_logit [R,G] from da; the softmax is recomputed from act.  datt_logit_bf16 [R, ld >= G] bf16: a copy
    as the operand of the attention weight-gradient products (its columns >= G are left alone)."""
    _lib.call("evc_nextvlad_assign_bwd", _p(act), R, G, K, _p(mean), _p(var), _p(gamma), _p(beta), _p(att_logits), att_logits.stride(0),
              _p(att_bias), _p(da), _p(dz), _p(datt_logit), _p(datt_logit_bf16),
              datt_logit_bf16.stride(0) if datt_logit_bf16 is not None else 0, _stream())


def nextvlad_aggregate_fwd(a, xe, B, S, G, K, D, c2, V, asum):
    _lib.call("evc_nextvlad_aggregate_fwd", _p(a), _p(xe), B, S, G, K, D, _p(c2), _p(V), _p(asum), _stream())


def nextvlad_aggregate_bwd_ws(B, K, D):
    """Floats of scratch evc_nextvlad_aggregate_bwd needs: dV transposed [B][D][K rounded up to 4] and q [B][K]."""
    return B * D * round_up(K, 4) + B * K


def nextvlad_aggregate_bwd(a, xe, B, S, G, K, D, c2, dV, da, dxe, ws=None):
    if ws is None:
        ws = torch.empty(nextvlad_aggregate_bwd_ws(B, K, D), dtype=F32, device=da.device)
    _lib.call("evc_nextvlad_aggregate_bwd", _p(a), _p(xe), B, S, G, K, D, _p(c2), _p(dV), _p(da), _p(dxe), _p(ws), ws.numel(), _stream())


class GridPlan:
    """Packed rows of a ragged batch, from the frame counts on the host: video b contributes the frames j * every_n,
    j < k[b] = ceil(min(n_b, max_frames) / every_n) (n_b <= 0: none), as the rows row_off[b] .. row_off[b+1] in time order.
    k, row_off: int32 numpy [B], [B+1]; R = row_off[B]; Rp = R rounded up to 32 (row count of the TN products); max_k = max_b k[b]."""

    def __init__(self, num_frames_host, every_n, max_frames):
        import numpy as np
        every_n, max_frames = int(every_n), int(max_frames)
        if every_n < 1 or every_n > max_frames:
            raise ValueError("every_n=%d must lie in 1 .. max_num_frames=%d" % (every_n, max_frames))
        n = np.clip(np.asarray(num_frames_host).reshape(-1).astype(np.int64), 0, max_frames)
        k = (n + every_n - 1) // every_n
        self.every_n, self.B = every_n, int(n.shape[0])
        self.k = k.astype(np.int32)
        self.row_off = np.zeros(self.B + 1, np.int32)
        np.cumsum(k, out=self.row_off[1:])
        self.R = int(self.row_off[-1])
        self.Rp = round_up(self.R, 32)
        self.max_k = int(k.max()) if self.B else 0


def grid_capacity(B, max_frames, every_n):
    """Rows the packed buffers of a batch of B videos are allocated for: every video at full length, rounded up to 32."""
    return round_up(B * ((max_frames + every_n - 1) // every_n), 32)


def frames_gather_packed(x, num_frames, row_off, every_n, R, Rp, out, out_bf16=None, normalize=False):
    """out [>= Rp, F] f32 (and out_bf16, the same rows as bf16): row row_off[b] + j = frame j * every_n of video b with
    sample_frames_gather's arithmetic; rows R .. Rp zeros.  row_off: device int32 [B+1] (GridPlan.row_off)."""
    B, T, F = x.shape
    is_u8 = x.dtype == torch.uint8
    assert x.is_contiguous() and out.is_contiguous() and out.dtype == F32 and out.shape[0] >= Rp and out.shape[1] == F
    assert out_bf16 is None or (out_bf16.is_contiguous() and out_bf16.dtype == BF16 and out_bf16.shape[0] >= Rp and out_bf16.shape[1] == F)
    assert row_off.dtype == torch.int32 and row_off.numel() == B + 1 and num_frames.dtype == torch.int32 and num_frames.numel() == B
    _lib.call("evc_frames_gather_packed", None if is_u8 else _p(x), _p(x) if is_u8 else None, _p(num_frames), _p(row_off), B, T, F, every_n, R, Rp,
              1 if normalize else 0, _p(out), _p(out_bf16), _stream())


def frames_gather_packed_bn(x, num_frames, row_off, every_n, R, Rp, mean, var, gamma, beta, out, out_bn, normalize=False):
    """frames_gather_packed and bn_apply(relu6=False, y_bf16=out_bn) behind it in one launch, for statistics known before the batch
    (DESIGN.md 7.19): out [>= Rp, F] f32 and out_bn [>= Rp, F] bf16, bit for bit the two launches' outputs; rows R .. Rp zeros in both."""
    B, T, F = x.shape
    is_u8 = x.dtype == torch.uint8
    assert x.is_contiguous() and out.is_contiguous() and out.dtype == F32 and out.shape[0] >= Rp and out.shape[1] == F
    assert out_bn.is_contiguous() and out_bn.dtype == BF16 and out_bn.shape[0] >= Rp and out_bn.shape[1] == F
    assert row_off.dtype == torch.int32 and row_off.numel() == B + 1 and num_frames.dtype == torch.int32 and num_frames.numel() == B
    for v in (mean, var, gamma, beta):
        assert v.dtype == F32 and v.numel() == F and v.is_contiguous()
    _lib.call("evc_frames_gather_packed_bn", None if is_u8 else _p(x), _p(x) if is_u8 else None, _p(num_frames), _p(row_off), B, T, F, every_n,
              R, Rp, 1 if normalize else 0, _p(mean), _p(var), _p(gamma), _p(beta), _p(out), _p(out_bn), _stream())


def check_row_selection(sel, B):
    """The host validation of a row selection before any launch reads it: ``sel`` (any integer sequence) must be strictly ascending and
    lie in 0 .. B - 1, and not be empty.  Returns it as an int32 numpy array.  The kernels trust what this accepted."""
    import numpy as np
    s = np.asarray(sel)
    if s.ndim != 1 or s.size == 0 or not np.issubdtype(s.dtype, np.integer):
        raise ValueError("row selection: a non-empty 1-D integer sequence is needed (got shape %s, dtype %s)" % (s.shape, s.dtype))
    s = s.astype(np.int64)
    if s.min() < 0 or s.max() >= B:
        raise ValueError("row selection: entries must lie in 0 .. %d (got %d .. %d)" % (B - 1, int(s.min()), int(s.max())))
    bad = np.flatnonzero(np.diff(s) <= 0)
    if bad.size:
        i = int(bad[0]) + 1
        raise ValueError("row selection: entries must be strictly ascending (entry %d is %d after %d)" % (i, int(s[i]), int(s[i - 1])))
    return s.astype(np.int32)


def frames_gather_packed_sel(x, num_frames, row_off, sel, every_n, R, Rp, out=None, out_bf16=None, normalize=False):
    """frames_gather_packed for the videos sel[0 .. b') of the unchanged batch x [B, T, F]: packed video j is source
    video sel[j].  row_off: device int32 [b' + 1] (GridPlan over the selected counts); sel: device int32 [b'], accepted by
    check_row_selection on the host before this call.  out (f32) may be None: the bf16 rows alone."""
    B, T, F = x.shape
    bs = sel.numel()
    is_u8 = x.dtype == torch.uint8
    assert x.is_contiguous() and sel.dtype == torch.int32 and sel.is_contiguous()
    assert out is None or (out.is_contiguous() and out.dtype == F32 and out.shape[0] >= Rp and out.shape[1] == F)
    assert out_bf16 is None or (out_bf16.is_contiguous() and out_bf16.dtype == BF16 and out_bf16.shape[0] >= Rp and out_bf16.shape[1] == F)
    assert row_off.dtype == torch.int32 and row_off.numel() == bs + 1 and num_frames.dtype == torch.int32 and num_frames.numel() == B
    _lib.call("evc_frames_gather_packed_sel", None if is_u8 else _p(x), _p(x) if is_u8 else None, _p(num_frames), _p(row_off), _p(sel), B, bs,
              T, F, every_n, R, Rp, 1 if normalize else 0, _p(out), _p(out_bf16), _stream())


SELECT_MAX_T = 1024     # the frames per video the source-frame tables hold (evc_student_frame_select, evc_student_frame_select_scored)


class SelectPlan:
    """GridPlan's fields for the packed rows of frames a source-frame table names: video b contributes the k[b] frames in
    the first k[b] slots of its table row, as the rows row_off[b] .. row_off[b+1].  The counts are the table kernels' own
    (evc_student_frame_select, _scored; host_frame_counts(subsampled=True)): n_b clipped to 0 .. T, k[b] = trunc(float64(n_b) / T * S)
    with S = T // every_n - the frames an H-LSTM student with the same word and every_n sees.  That can be one fewer than GridPlan's
    ceil(n_b / every_n), and it is 0 for a video shorter than every_n.  B * S is at most grid_capacity(B, T, every_n)."""

    def __init__(self, num_frames_host, every_n, max_frames):
        import numpy as np
        every_n, T = int(every_n), int(max_frames)
        if every_n < 1 or every_n > T:
            raise ValueError("every_n=%d must lie in 1 .. max_num_frames=%d" % (every_n, T))
        if T > SELECT_MAX_T:
            raise ValueError("max_num_frames=%d: the source-frame tables hold at most %d frames per video" % (T, SELECT_MAX_T))
        self.S = T // every_n
        n = np.clip(np.asarray(num_frames_host).reshape(-1).astype(np.int64), 0, T)
        k = np.trunc(n.astype(np.float64) / float(T) * float(self.S)).astype(np.int64)
        self.every_n, self.B = every_n, int(n.shape[0])
        self.k = k.astype(np.int32)
        self.row_off = np.zeros(self.B + 1, np.int32)
        np.cumsum(k, out=self.row_off[1:])
        self.R = int(self.row_off[-1])
        self.Rp = round_up(self.R, 32)
        self.max_k = int(k.max()) if self.B else 0


def frames_gather_packed_tab(x, num_frames, row_off, src, R, Rp, out=None, out_bf16=None, normalize=False):
    """frames_gather_packed on the frames a table names (evc_frames_gather_packed_tab): row row_off[b] + j = frame
    src[b, j] of video b; src device int32 [B, S] (student_frame_select / student_frame_select_scored), an entry outside 0 .. T - 1
    - and for uint8 input one >= num_frames[b] - a zero row.  row_off: device int32 [B+1] (SelectPlan.row_off).  out (f32) or out_bf16
    may be None, not both; rows R .. Rp zeros."""
    B, T, F = x.shape
    is_u8 = x.dtype == torch.uint8
    assert x.is_contiguous() and src.dtype == torch.int32 and src.is_contiguous() and src.dim() == 2 and src.shape[0] == B
    assert out is None or (out.is_contiguous() and out.dtype == F32 and out.shape[0] >= Rp and out.shape[1] == F)
    assert out_bf16 is None or (out_bf16.is_contiguous() and out_bf16.dtype == BF16 and out_bf16.shape[0] >= Rp and out_bf16.shape[1] == F)
    assert row_off.dtype == torch.int32 and row_off.numel() == B + 1 and num_frames.dtype == torch.int32 and num_frames.numel() == B
    _lib.call("evc_frames_gather_packed_tab", None if is_u8 else _p(x), _p(x) if is_u8 else None, _p(num_frames), _p(row_off), _p(src), B, T, F,
              src.shape[1], R, Rp, 1 if normalize else 0, _p(out), _p(out_bf16), _stream())


def scatter_rows(src, sel, dst):
    """dst[sel[j]] = src[j] for the rows of src (2-D f32, rows contiguous, any row stride); the other rows of dst keep their contents.
    sel: device int32 [src.shape[0]], accepted by check_row_selection(sel, dst.shape[0]) on the host before this call."""
    assert src.dim() == 2 and dst.dim() == 2 and src.dtype == F32 and dst.dtype == F32 and src.shape[1] == dst.shape[1]
    assert src.shape[1] <= 1 or (src.stride(1) == 1 and dst.stride(1) == 1)
    assert sel.dtype == torch.int32 and sel.is_contiguous() and sel.numel() == src.shape[0] and src.shape[0] <= dst.shape[0]
    _lib.call("evc_scatter_rows", _p(src), src.stride(0), _p(sel), src.shape[0], dst.shape[0], src.shape[1], _p(dst), dst.stride(0), _stream())
    return dst


def nextvlad_aggregate_packed_fwd(a, xe, row_off, B, T, G, K, D, R, max_k, c2, V, asum):
    """nextvlad_aggregate_fwd over packed rows: video b's a / xe rows are row_off[b] .. row_off[b+1] (device int32 [B+1])."""
    assert row_off.dtype == torch.int32 and row_off.numel() == B + 1
    assert a.numel() >= R * G * K and xe.numel() >= R * G * D and V.numel() >= B * K * D and asum.numel() >= B * K
    _lib.call("evc_nextvlad_aggregate_packed_fwd", _p(a), _p(xe), _p(row_off), B, T, G, K, D, R, max_k, _p(c2), _p(V), _p(asum), _stream())


def nextvlad_aggregate_packed_fwd_mfma(a, xe, row_off, B, T, G, K, D, R, max_k, c2, V, asum):
    """nextvlad_aggregate_packed_fwd on the f32 matrix cores: same arguments, same bits; forward-only callers."""
    assert row_off.dtype == torch.int32 and row_off.numel() == B + 1
    assert a.numel() >= R * G * K and xe.numel() >= R * G * D and V.numel() >= B * K * D and asum.numel() >= B * K
    _lib.call("evc_nextvlad_aggregate_packed_fwd_mfma", _p(a), _p(xe), _p(row_off), B, T, G, K, D, R, max_k, _p(c2), _p(V), _p(asum), _stream())


def nextvlad_aggregate_packed_bwd(a, xe, row_off, B, T, G, K, D, R, max_k, c2, dV, da, dxe, ws=None):
    """nextvlad_aggregate_bwd over packed rows: the R live rows of da and dxe are written, nothing beyond them."""
    assert row_off.dtype == torch.int32 and row_off.numel() == B + 1
    assert a.numel() >= R * G * K and xe.numel() >= R * G * D and da.numel() >= R * G * K and dxe.numel() >= R * G * D and dV.numel() >= B * K * D
    if ws is None:
        ws = torch.empty(nextvlad_aggregate_bwd_ws(B, K, D), dtype=F32, device=da.device)
    _lib.call("evc_nextvlad_aggregate_packed_bwd", _p(a), _p(xe), _p(row_off), B, T, G, K, D, R, max_k, _p(c2), _p(dV), _p(da), _p(dxe), _p(ws),
              ws.numel(), _stream())


def nextvlad_normalize_fwd(V, B, K, D, U, norms):
    _lib.call("evc_nextvlad_normalize_fwd", _p(V), B, K, D, _p(U), _p(norms), _stream())


def nextvlad_normalize_bwd(V, norms, dU, B, K, D, dV):
    _lib.call("evc_nextvlad_normalize_bwd", _p(V), _p(norms), _p(dU), B, K, D, _p(dV), _stream())


def nextvlad_gate_fwd(h, gl, out):
    _lib.call("evc_nextvlad_gate_fwd", _p(h), _p(gl), h.numel(), _p(out), _stream())


def nextvlad_gate_bwd(h, gl, dout, dh, dgl=None, dgl_bf16=None):
    _lib.call("evc_nextvlad_gate_bwd", _p(h), _p(gl), _p(dout), h.numel(), _p(dh), _p(dgl), _p(dgl_bf16), _stream())


def nextvlad_gate_bwd_add(h, gl, dout, dout2, dh, dgl=None, dgl_bf16=None):
    """nextvlad_gate_bwd on the incoming gradient dout + dout2 (one f32 add; dout2 None: nextvlad_gate_bwd's bits)."""
    assert dout2 is None or (dout2.numel() == h.numel() and dout2.dtype == F32 and dout2.is_contiguous())
    _lib.call("evc_nextvlad_gate_bwd_add", _p(h), _p(gl), _p(dout), _p(dout2), h.numel(), _p(dh), _p(dgl), _p(dgl_bf16), _stream())


def nextvlad_colsum(x, R, C, out, ws=None):
    """out[c] = sum_r x[r, c] (f32, fixed order).  Tall inputs go through 32 partial rows in `ws` (32 * C floats; from the
    stream-aware caching allocator when not given)."""
    if ws is None and R >= 512:
        ws = torch.empty(32 * C, dtype=F32, device=x.device)
    _lib.call("evc_nextvlad_colsum", _p(x), x.stride(0), R, C, _p(out), _p(ws), ws.numel() if ws is not None else 0, _stream())


def nextvlad_center_cast(xe, R, E, be, out_bf16):
    """out [R,E] bf16 = xe - be: the centred operand of the cluster / attention products (contiguous rows)."""
    assert xe.is_contiguous() and out_bf16.is_contiguous() and out_bf16.dtype == BF16
    _lib.call("evc_nextvlad_center_cast", _p(xe), R, E, _p(be), _p(out_bf16), _stream())


def nextvlad_bias_logits(be, W, N, E, out, add=None):
    """out[n] = be . W[n] (+ add[n]) for n < N, zeros up to out.numel(): the constant the expansion bias adds to every logit (f32)."""
    assert W.is_contiguous() and W.dtype == F32
    _lib.call("evc_nextvlad_bias_logits", _p(be), _p(W), N, E, _p(add), _p(out), out.numel(), _stream())


def check_dropout_rate(rate, what="dropout"):
    """The DROP rate as a Python float; a value outside [0, 1) (or not a number) is a ValueError that names it."""
    r = float(rate)
    if not (0.0 <= r < 1.0):
        raise ValueError("%s=%r: the drop rate must lie in [0, 1)" % (what, rate))
    return r


def dropout_threshold(keep):
    """(T, scale) of the dropout entries for a keep probability in (0, 1]: T = floor(keep * 2^32) as a uint32 (an element is kept
    iff its Philox word is below T; keep = 1 is refused, it has no such T - a rate of 0 launches nothing) and scale = float32(1 / keep)."""
    import numpy as np
    keep = float(keep)
    T = int(keep * 4294967296.0) if 0.0 < keep < 1.0 else 0        # (the product is exact in float64; int() is floor here)
    if not (0 < T <= 0xFFFFFFFF):
        raise ValueError("dropout: keep probability %r has no 32-bit threshold (it must lie in (0, 1) and keep * 2^32 >= 1)" % keep)
    return T, float(np.float32(1.0 / keep))


def nextvlad_dropout_fwd(U, B, Cc, mean, var, gamma, beta, T, scale, seed, rank, step, y_bf16):
    """y_bf16 [>= B, Cc] = bf16(vlad_bn(U) * scale) where kept, +0 where dropped: bn_apply, the stateless mask of
    (seed, rank, step, element) and the bf16 store in one pass.  T, scale: dropout_threshold(keep)."""
    assert U.is_contiguous() and U.dtype == F32 and U.numel() >= B * Cc
    assert y_bf16.is_contiguous() and y_bf16.dtype == BF16 and y_bf16.numel() >= B * Cc
    _lib.call("evc_nextvlad_dropout_fwd", _p(U), B, Cc, _p(mean), _p(var), _p(gamma), _p(beta), T, scale, seed & 0xFFFFFFFF,
              rank & 0xFFFFFFFF, step & 0xFFFFFFFFFFFFFFFF, _p(y_bf16), _stream())


def nextvlad_dropout_bwd(dY, B, Cc, T, scale, seed, rank, step):
    """dY [B, Cc] f32 in place: dY * scale where the forward of the same (seed, rank, step) kept the element, 0 where it dropped it."""
    assert dY.is_contiguous() and dY.dtype == F32 and dY.numel() >= B * Cc
    _lib.call("evc_nextvlad_dropout_bwd", _p(dY), B, Cc, T, scale, seed & 0xFFFFFFFF, rank & 0xFFFFFFFF, step & 0xFFFFFFFFFFFFFFFF, _stream())


def nextvlad_wgrad_uncenter(dWc, du, be, N, E, dW):
    """dW [N,E] = dWc[:N] + du[:, None] * be[None, :] (the rank-one term a product against the centred operand leaves out)."""
    _lib.call("evc_nextvlad_wgrad_uncenter", _p(dWc), _p(du), _p(be), N, E, _p(dW), _stream())
