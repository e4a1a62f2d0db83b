"""The K-major-B product evc_gemm_kn (csrc/evc_gemm_kn.hip): C[M][N] (+)= A[M][K] . B[K][N] with B stored as it is contracted.

Per element against the float64 product of the same bf16 values, in the bound form of tests/_wgrad_ref.py ("wide" data): in any order of the
f32 additions  |c - ref| <= (K + splits + 1) U (sum_k |a_k b_k| + |C0|), U = 2^-24 - nothing in it is measured.  Bit equality with
evc_gemm_nt on a contiguous transposed copy of B wherever both run unsplit: evc_gemm_kn with splits = 1 forced; evc_gemm_nt splits K only for
N >= 1024 or K >= 4096 (choose_nt, csrc/evc_gemm.hip) and takes K % 64 == 0 only, so of the shapes below those with K = 2048.
Shapes: M in {70, 256}, N in {64, 192} (one column tile and three), K in {328, 2048} (328 = 5 stages of 64 and a tail of 8).  pytest -m gpu."""
import ctypes as C
import functools
import itertools

import pytest
import torch

from efficientvideoclassification_youtube8m_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
BF16 = torch.bfloat16
SHAPES = list(itertools.product((70, 256), (64, 192), (328, 2048)))
SENT = float("nan")          # a C that must not be read is full of these; margins keep them


@functools.lru_cache(maxsize=None)
def _operands(M, N, K, seed=0):
    """A [M][K], B [K][N] (bf16, on the device), C0 [M][N] f32, and on the host in float64: A . B, |A| . |B|."""
    g = torch.Generator(device="cpu").manual_seed(1000 * M + 10 * N + K + seed)
    a = (torch.randn(M, K, generator=g) * torch.pow(10.0, torch.rand(M, K, generator=g) * 3 - 3)).to(BF16)
    b = torch.randn(K, N, generator=g).to(BF16)
    b[:, ::5] *= 1e-3
    c0 = torch.randn(M, N, generator=g)
    a64, b64 = a.double(), b.double()
    return a.to(DEV), b.to(DEV), c0.to(DEV), a64 @ b64, a64.abs() @ b64.abs()


def _strided(t, ld, fill=0.0):
    """t's values in rows of stride ld, the margin holding `fill` (NaN: operands never read it into a finite result unseen)."""
    full = torch.full((t.shape[0], ld), fill, dtype=t.dtype, device=t.device)
    full[:, :t.shape[1]] = t
    return full


def _run(M, N, K, ldb, ldc, accumulate, splits, seg2=None):
    a, b, c0, ref, absref = _operands(M, N, K)
    kw = {}
    if seg2 is not None:                   # a second K segment of its own operands
        a2, b2, _, ref2, abs2 = _operands(M, N, seg2, seed=7)
        ref, absref = ref + ref2, absref + abs2
        kw = dict(A2=_strided(a2, seg2 + 8, SENT), B2=_strided(b2, ldb, SENT), K2=seg2)
    As, Bs = _strided(a, K + 16, SENT), _strided(b, ldb, SENT)
    Cf = torch.full((M + 2, ldc), SENT, dtype=torch.float32, device=DEV)
    if accumulate:
        Cf[:M, :N] = c0
    ops.gemm_kn(As, Bs, M, N, K, Cf, accumulate=accumulate, splits=splits, **kw)
    torch.cuda.synchronize()
    got = Cf[:M, :N].double().cpu()
    base = c0.double().cpu() if accumulate else torch.zeros_like(ref)
    depth = K + (seg2 or 0)
    bound = (depth + splits + 1) * U * (absref + base.abs())
    err = (got - (ref + base)).abs()
    ratio = float((err / bound).max())
    print("M=%d N=%d K=%d%s ldb=%d ldc=%d acc=%d splits=%d: max err / bound = %.3f" % (M, N, K, "+%d" % seg2 if seg2 else "", ldb, ldc, accumulate, splits, ratio))
    assert torch.isfinite(got).all(), "a sentinel reached the result"
    assert ratio <= 1.0, ratio
    assert torch.isnan(Cf[M:]).all() and torch.isnan(Cf[:, N:]).all(), "stored outside C"
    return Cf


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_per_element_against_float64(M, N, K):
    """ldb > N, ldc > N (rows 16-byte aligned and not), accumulate on and off, one K split and three forced; the non-accumulating runs start
    from a C full of NaN."""
    for accumulate, splits in itertools.product((False, True), (1, 3)):
        _run(M, N, K, N + 8, N + 4, accumulate, splits)
    _run(M, N, K, N + 24, N + 1, False, 1)          # element-wise store (unaligned rows)
    _run(M, N, K, N, N, False, 1)                   # contiguous


@pytest.mark.parametrize("M,N", list(itertools.product((70, 256), (64, 192))))
def test_two_segments(M, N):
    """K1 = 192 then K2 = 136 in one launch; with three splits of two stages the middle one walks the last stage of segment 1 and the first of
    segment 2, the last one ends in the 8-wide tail."""
    for accumulate, splits in itertools.product((False, True), (1, 3)):
        _run(M, N, 192, N + 8, N + 4, accumulate, splits, seg2=136)


def test_ragged_last_column_tile():
    """N = 72: the second column tile holds 8 valid columns - its other chunks are clamped onto them and its stores are masked."""
    for accumulate, splits in ((False, 1), (True, 1), (False, 2)):
        _run(70, 72, 328, 80, 76, accumulate, splits)


def test_fewer_b_rows_than_k():
    """b_rows < K: the rows up to K are read as B's last row (B ends there: the allocation has no further row) against zero columns of A."""
    M, N, K, rows = 70, 192, 2048, 1990
    a, b, _, _, _ = _operands(M, N, K)
    a = a.clone()
    a[:, rows:] = 0
    bs = b[:rows].clone()
    ref = a[:, :rows].double().cpu() @ bs.double().cpu()
    absref = a[:, :rows].double().cpu().abs() @ bs.double().cpu().abs()
    for splits in (1, 2):
        out = torch.full((M, N), SENT, dtype=torch.float32, device=DEV)
        ops.gemm_kn(a, bs, M, N, K, out, splits=splits, b_rows=rows)
        err = (out.double().cpu() - ref).abs()
        assert float((err / ((K + splits + 1) * U * absref)).max()) <= 1.0


def test_bits_of_gemm_nt_on_the_transposed_copy():
    """Unsplit on both sides (see the module docstring): the same K order, MFMA shape and accumulator layout, so the same bits - plain and
    accumulating."""
    compared = 0
    for M, N, K in SHAPES:
        if K % 64:
            continue                       # evc_gemm_nt refuses it
        assert N < 1024 and K < 4096       # evc_gemm_nt runs these unsplit
        a, b, c0, _, _ = _operands(M, N, K)
        bt = b.t().contiguous()
        for accumulate in (False, True):
            got, want = (c0.clone() if accumulate else torch.full((M, N), SENT, dtype=torch.float32, device=DEV) for _ in range(2))
            ops.gemm_kn(a, b, M, N, K, got, accumulate=accumulate, splits=1)
            ops.gemm_nt(a, bt, M, N, K, want, accumulate=accumulate)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (M, N, K, accumulate, float((got - want).abs().max()))
            compared += 1
    assert compared >= 2


def test_plan_query_matches_the_batch_row_rule():
    """The split count the entry takes by itself: until ~256 workgroups, >= 16 stages each (none under EVC_DETERMINISTIC)."""
    assert ops.gemm_kn_splits(64, 2048, out_bf16=True) == 1
    if not ops.DETERMINISTIC:
        assert ops.gemm_kn_splits(4096, 14208) == 4 and ops.gemm_kn_splits(4096, 14208, 9472) == 4 and ops.gemm_kn_splits(64, 2048) == 2
        assert ops.gemm_kn_splits(64, 328) == 1
    else:
        assert ops.gemm_kn_splits(4096, 14208) == 1


SHAPE, ALIGN, ARG = -1, -2, -5          # EVC_ERR_BAD_SHAPE, EVC_ERR_BAD_ALIGN, EVC_ERR_BAD_ARG (include/evc.h)
GOOD = dict(A1="A", lda1=64, B1="B", ldb1=64, K1=64, b_rows1=0, A2=None, lda2=0, B2=None, ldb2=0, K2=0, b_rows2=0, C="C", ldc=64, M=64, N=64, bias=None,
            out_bf16=0, accumulate=0, splits=0)
REFUSALS = [
    (dict(A1=None), ARG), (dict(B1=None), ARG), (dict(C=None), ARG), (dict(K2=64), ARG), (dict(K2=64, A2="A"), ARG), (dict(K2=-8), ARG),
    (dict(out_bf16=1, accumulate=1), ARG), (dict(splits=-1), ARG), (dict(splits=2), ARG), (dict(K1=256, lda1=256, splits=3, out_bf16=1), ARG),
    (dict(M=0), SHAPE), (dict(N=0), SHAPE), (dict(K1=0), SHAPE), (dict(M=257), SHAPE), (dict(K1=60), SHAPE), (dict(N=60), SHAPE),
    (dict(K2=60, A2="A", B2="B", lda2=64, ldb2=64), SHAPE), (dict(b_rows1=65), SHAPE), (dict(b_rows1=-1), SHAPE), (dict(lda1=56), SHAPE), (dict(ldb1=56), SHAPE),
    (dict(ldc=60), SHAPE), (dict(lda1=1 << 23), SHAPE), (dict(ldb1=1 << 23), SHAPE), (dict(K1=1 << 20, lda1=1 << 20, ldb1=4096), SHAPE),      # (the last: B spans 8 GiB)
    (dict(lda1=68), ALIGN), (dict(ldb1=68), ALIGN), (dict(A1="A+2"), ALIGN), (dict(B1="B+8"), ALIGN),
    (dict(K2=64, A2="A+2", B2="B", lda2=64, ldb2=64), ALIGN), (dict(K2=64, A2="A", B2="B", lda2=64, ldb2=68), ALIGN),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_refusals(case):
    """One broken argument: the documented code, an error text that names the entry, and nothing enqueued - C keeps its fill."""
    change, code = REFUSALS[case]
    buf = torch.zeros(3 * 64 * 64, dtype=BF16, device=DEV)
    cbuf = torch.full((64 * 64,), 3.5, dtype=torch.float32, device=DEV)
    base = {"A": buf.data_ptr(), "B": buf.data_ptr() + 2 * 64 * 64, "C": cbuf.data_ptr()}

    def ptr(v):
        if v is None:
            return None
        name, _, off = v.partition("+")
        return base[name] + int(off or 0)

    args = dict(GOOD, **change)
    lib = _lib.load()
    rc = lib.evc_gemm_kn(*[ptr(v) if k in ("A1", "B1", "A2", "B2", "C", "bias") else v for k, v in args.items()], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == code, (change, rc, lib.evc_last_error().decode())
    assert "evc_gemm_kn" in lib.evc_last_error().decode()
    assert bool((cbuf == 3.5).all())
    # the well-formed call from the same buffers is accepted
    rc = lib.evc_gemm_kn(*[ptr(v) if k in ("A1", "B1", "A2", "B2", "C", "bias") else v for k, v in GOOD.items()], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and bool((cbuf == 0).all())


def test_signature_order():
    """GOOD lists the arguments in the order of the C signature (the refusal cases are passed positionally)."""
    assert len(GOOD) + 1 == len(_lib.SIGNATURES["evc_gemm_kn"]) and _lib.SIGNATURES["evc_gemm_kn"][-1] is C.c_void_p
