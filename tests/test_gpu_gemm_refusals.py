"""The refusals of the NT and TN product entry points of csrc/evc_gemm.hip and csrc/evc_gemm_tn.hip: a call with one argument broken returns the
documented EVC_ERR_* code, and the error text names the entry the caller used (the slab entries say evc_gemm_tn_slabs / evc_gemm_tn2_slabs, not
evc_gemm_tn).  Every case is refused before the first enqueue, so nothing is launched: 64 x 64 x 64 operands carved out of one small buffer."""
import ctypes as C
import re

import pytest
import torch

from efficientvideoclassification_youtube8m_amd import _lib, ops

pytestmark = pytest.mark.gpu

SHAPE, ALIGN, ARG = -1, -2, -5          # EVC_ERR_BAD_SHAPE, EVC_ERR_BAD_ALIGN, EVC_ERR_BAD_ARG (include/evc.h)
KB = 1024
# byte offsets into the buffer: A, B (and their e4m3 images), C / slabs, a second B segment, bias / P / sums / workspaces
A, B, CC, B2, A8, B8, F = 0, 64 * KB, 128 * KB, 192 * KB, 256 * KB, 320 * KB, 384 * KB

# well-formed arguments per entry, in the order of the C signature (pointers as byte offsets, None = NULL) ...
GOOD = {
    "evc_gemm_nt": dict(A=A, lda=64, B=B, ldb=64, C=CC, ldc=64, M=64, N=64, K=64, bias=None, out_bf16=0, accumulate=0),
    "evc_gemm_nt_sqnorm": dict(A=A, lda=64, B=B, ldb=64, C=CC, ldc=256, M=640, N=256, K=64, P=F, l2_coeff=0.5, sums=F + 8 * KB, part_ws=F + 16 * KB,
                               part_ws_floats=160),
    "evc_gemm_nt_split": dict(A=A, lda=128, B=B, ldb=128, C=CC, ldc=64, M=64, N=64, K=64, bias=None),
    "evc_gemm_nt_f16_fp8": dict(A16=A, lda=64, A8=A8, lda8=512, B16=B, ldb=64, B8=B8, ldb8=512, C=CC, ldc=64, M=64, N=64, K16=64, K8=512, scale_exp=-24,
                                bias=None),
    "evc_gemm_nt_f16_fp8_dyn": dict(A16=A, lda=64, A8=A8, lda8=512, B16=B, ldb=64, B8=B8, ldb8=512, C=CC, ldc=64, M=64, N=64, K16=64, K8=512, scale_exp=-24,
                                    amax_ws=F, a8_hi_exp=17, bias=None),
    "evc_gemm_tn": dict(A=A, lda=64, B=B, ldb=64, C=CC, ldc=64, M=64, N=64, K=64, row_interleave_H=0, accumulate=0),
    "evc_gemm_tn2": dict(A=A, lda=64, B1=B, ldb1=256, N1=256, B2=B2, ldb2=64, N2=64, c_col2=256, C=CC, ldc=320, M=64, K=64, row_interleave_H=0, accumulate=0),
    "evc_gemm_tn2_rows": dict(A=A, lda=64, B1=B, ldb1=256, N1=256, B2=B2, ldb2=64, N2=64, c_col2=256, C=CC, ldc=320, M=64, slab_rows=32, nslabs=2,
                              rows_per_slab="table", row_interleave_H=0, accumulate=0),
    "evc_gemm_tn_slabs": dict(A=A, lda=64, B=B, ldb=64, slabs=CC, M=64, N=64, K=64, nslab=2),
    "evc_gemm_tn2_slabs": dict(A=A, lda=64, B1=B, ldb1=256, N1=256, B2=B2, ldb2=64, N2=64, c_col2=256, slabs=CC, ldc=320, slab_stride=64 * 320, M=64, K=64,
                               row_interleave_H=0, nslab=2),
    "evc_sum_slabs": dict(slabs=CC, slab_stride=64 * 64, nslab=2, M=64, N=64, ld=64, C=F, ldc=64, accumulate=0),
}
POINTERS = {"A", "B", "C", "bias", "P", "sums", "part_ws", "A16", "A8", "B16", "B8", "amax_ws", "B1", "B2", "slabs"}

# ... and (entry, the arguments that break one rule, the code it must return)
NT_OPERANDS = [(dict(K=96, lda=96, ldb=96), SHAPE), (dict(M=0), SHAPE), (dict(N=-8), SHAPE), (dict(lda=60), ALIGN), (dict(ldb=68), ALIGN), (dict(A=A + 2), ALIGN),
               (dict(B=B + 8), ALIGN), (dict(M=1 << 24), SHAPE), (dict(lda=1 << 23), SHAPE), (dict(N=1 << 17, ldb=1 << 15), SHAPE)]
TN_OPERANDS = [(dict(M=60), SHAPE), (dict(M=4), SHAPE), (dict(K=80), SHAPE), (dict(K=0), SHAPE), (dict(lda=60), ALIGN), (dict(A=A + 2), ALIGN)]
TN_SEGMENT2 = [(dict(N1=128, c_col2=128), SHAPE), (dict(ldb2=60), SHAPE), (dict(B2=B2 + 2), SHAPE)]
CASES = (
    [("evc_gemm_nt", o, c) for o, c in NT_OPERANDS + [(dict(K=-64), SHAPE), (dict(out_bf16=1, accumulate=1), ARG)]]
    + [("evc_gemm_nt_sqnorm", o, c) for o, c in NT_OPERANDS[:1] + NT_OPERANDS[3:7] + [
        (dict(sums=None), ARG), (dict(part_ws=None), ARG), (dict(P=None), ARG), (dict(part_ws_floats=159), ARG), (dict(M=512), ARG), (dict(N=264, ldc=264), ARG),
        (dict(K=8192, lda=8192, ldb=8192), ARG), (dict(ldc=258), ARG), (dict(C=CC + 4), ARG), (dict(P=F + 4), ARG)]]
    + [("evc_gemm_nt_split", o, c) for o, c in [(dict(K=96, lda=192, ldb=192), SHAPE), (dict(K=0), SHAPE), (dict(M=0), SHAPE), (dict(lda=120), ALIGN), (dict(ldb=124), ALIGN),
                                                 (dict(A=A + 2), ALIGN), (dict(M=1 << 24), SHAPE), (dict(lda=1 << 23), SHAPE)]]
    + [(e, o, c) for e in ("evc_gemm_nt_f16_fp8", "evc_gemm_nt_f16_fp8_dyn") for o, c in [
        (dict(K16=96, lda=96, ldb=96), SHAPE), (dict(K8=384), SHAPE), (dict(K8=576, lda8=576, ldb8=576), SHAPE), (dict(M=0), SHAPE), (dict(A16=None), ARG), (dict(B8=None), ARG),
        (dict(C=None), ARG), (dict(lda=60), ALIGN), (dict(lda8=520), ALIGN), (dict(ldb8=496), ALIGN), (dict(A8=A8 + 8), ALIGN), (dict(scale_exp=61), ARG),
        (dict(scale_exp=-61), ARG), (dict(M=1 << 24), SHAPE), (dict(lda=1 << 23), SHAPE), (dict(lda8=1 << 24), SHAPE)]]
    + [("evc_gemm_nt_f16_fp8_dyn", o, ARG) for o in (dict(amax_ws=None), dict(a8_hi_exp=31), dict(a8_hi_exp=-31))]
    + [("evc_gemm_tn", o, c) for o, c in TN_OPERANDS + [(dict(N=60), SHAPE), (dict(ldb=60), ALIGN), (dict(B=B + 2), ALIGN), (dict(row_interleave_H=17), SHAPE)]]
    + [("evc_gemm_tn2", o, c) for o, c in TN_OPERANDS + TN_SEGMENT2 + [
        (dict(c_col2=128, accumulate=1), SHAPE), (dict(N2=60), SHAPE), (dict(ldb1=60), ALIGN), (dict(B1=B + 2), ALIGN), (dict(row_interleave_H=17), SHAPE), (dict(B1=None), ARG), (dict(B2=None), ARG),
        (dict(N1=0), ARG), (dict(N2=0), ARG), (dict(c_col2=320, ldc=384), ARG)]]
    + [("evc_gemm_tn2_rows", o, c) for o, c in TN_OPERANDS[:2] + TN_OPERANDS[4:] + TN_SEGMENT2 + [
        (dict(c_col2=128, accumulate=1), SHAPE), (dict(slab_rows=40), SHAPE), (dict(row_interleave_H=17), SHAPE), (dict(B1=None), ARG), (dict(N1=0), ARG), (dict(slab_rows=0), ARG), (dict(nslabs=0), ARG),
        (dict(rows_per_slab=None), ARG), (dict(slab_rows=1 << 20, nslabs=1 << 11), ARG), (dict(N2=0), ARG), (dict(c_col2=320, ldc=384), ARG)]]
    + [("evc_gemm_tn_slabs", o, c) for o, c in TN_OPERANDS + [(dict(N=60), SHAPE), (dict(ldb=60), ALIGN), (dict(nslab=0), SHAPE), (dict(nslab=3), SHAPE),
                                                                 (dict(K=160, nslab=4), SHAPE)]]
    + [("evc_gemm_tn2_slabs", o, c) for o, c in TN_OPERANDS + TN_SEGMENT2 + [
        (dict(c_col2=128), SHAPE), (dict(N1=4, B2=None), SHAPE), (dict(ldb1=60), ALIGN), (dict(nslab=0), SHAPE), (dict(nslab=3), SHAPE), (dict(K=160, nslab=4), SHAPE), (dict(slabs=None), ALIGN),
        (dict(slab_stride=64 * 320 - 4), ALIGN), (dict(row_interleave_H=17), SHAPE), (dict(N2=0), SHAPE)]]
    + [("evc_sum_slabs", o, SHAPE) for o in (dict(slabs=None), dict(C=None), dict(nslab=0), dict(M=0), dict(N=6), dict(ld=6), dict(ldc=10), dict(slab_stride=66),
                                            dict(slabs=CC + 4), dict(C=F + 8))]
)


def arguments(entry, over, base):
    """The ctypes argument list of `entry`: GOOD[entry] with `over` applied, pointers rebased onto `base`, stream NULL."""
    table = (C.c_int32 * 2)(32, 0)
    args = []
    for key, v in dict(GOOD[entry], **over).items():
        if key == "rows_per_slab":
            v = table if v == "table" else None
        elif key in POINTERS and v is not None:
            v = base + v
        args.append(v)
    return args + [None], table


@pytest.fixture(scope="module")
def buffer():
    ops.check_device(0)
    return torch.zeros(512 * KB, dtype=torch.uint8, device="cuda:0")


@pytest.mark.parametrize("entry", sorted(GOOD))
def test_refusals_return_their_code_and_name_the_entry(entry, buffer):
    cases = [(o, c) for e, o, c in CASES if e == entry]
    assert cases
    for over, code in cases:
        args, keep = arguments(entry, over, buffer.data_ptr())
        with pytest.raises(_lib.EvcError) as err:
            _lib.call(entry, *args)
        assert re.match(r"%s failed \(%d\): %s: " % (entry, code, entry), str(err.value)), "%s with %s: %s" % (entry, over, err.value)
