"""Host side of the weight-gradient (TN product) parity tests: operands whose product is exact in f32, the plain references, a mirror of
the dispatch, the checker and planted faults.  Used by tests/test_cpu_wgrad_ref.py (no GPU) and tests/test_gpu_wgrad_parity.py.

The products  C[M][N] (+)= A^T . B  (A [K][lda], B [K][ldb] bf16, C f32; csrc/evc_gemm_tn.hip) are checked in two data kinds.

exact   A = SA ia, B = SB ib with integers |i| <= q = min(255, floor(sqrt(2^24 / (2 K)))) (K = contracted rows) and SA = 2^-9, SB = 2^4; C0 (for
        accumulate) = SA SB times integers below 2^22.  Every product is an integer times SA SB, every partial sum in ANY order is such an
        integer below K q^2 + 2^22 < 2^24, so every f32 addition - inside the MFMA, across split-K atomics, across slabs, onto C0 - is
        exact and the result is the integer product's f32 image bit for bit.  The reference is the integer product (int_product); the
        assertion is bit equality of every element of the buffer, sentinels included.
wide    A = bf16(normal 10^uniform(-6, -1)) (as dz looks), zeros in the dead rows; B = bf16(normal), every fifth column scaled by 1e-3;
        magnitudes >= 1e-15 so that no product is subnormal in f32.  Reference: the float64 product of the same bf16 values.  Limit, in
        any order of the f32 additions (the form of tests/_optim_ref.py): d = (K + splits + 1) U (sum_k |a_k b_k| + |C0|), U = 2^-24, K the
        rows actually walked.  Nothing in d is measured.

Dead rows (row plans, evc_gemm_tn2_rows): A is zero there, B holds +-2^100 in the rows no 32-row step of a live prefix covers; rows between
rows[t] and the next multiple of 32 are ordinary in B and zero in A.  The reference contracts the live rows only.
"""
import zlib

import numpy as np

U = 2.0 ** -24
SA, SB = 2.0 ** -9, 2.0 ** 4
SENT = np.float32(-7.25)             # sentinel around C
GARBAGE = 2.0 ** 100                 # B in the skipped rows
FRONT = 4                            # sentinel floats in front of C (16 bytes: an aligned C stays aligned)
BACK_ROWS = 2                        # sentinel rows behind row M

# (BM, BU, WR, WC) of the two tile configurations (CfgTn128, CfgPlainV2 in csrc)
TILE = {"tn128": (128, 128, 2, 4), "strip": (128, 128, 2, 4), "tile256": (256, 256, 2, 4)}


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the dispatch mirror
# ---------------------------------------------------------------------------------------------------------------------------------------
def plan_tn(M, N, K, N1=0, B2=False, rows_per_slab=None, slab_rows=0, deterministic=False, forced_tile=0, accumulate=False, ldc=None,
            c_col2=None, c_aligned=True, lda=8, ldb=8, ldb2=8):
    """A line-by-line Python mirror of gemm_tn_impl (csrc/evc_gemm_tn.hip: the segment table, the three branches, splits, the memset), of
    gemm_tn_kernel's split -> (seg0, seg_off0) walk and of its choice between the four stores.  IT MIRRORS THOSE LINES AND MUST MOVE WITH
    THEM: its only purpose is that every test case can assert that it reaches the path it is named after.

    M, N, K as the C ABI takes them (N = N1 + N2 with two segments, K = slab_rows * nslabs for the row-plan entry).  Returns
    branch: tn128 | strip | tile256;  seg: the segment walk runs;  segs: [(first step, steps)];  nk: K steps walked;  splits;
    ksteps_per_split;  walk: per split (segment or None, first step within it / absolute first step, steps - may be <= 0);  memset: the
    N columns are cleared first;  stores: per column tile, per wave column: vec | rmw | elementwise | atomic | none (no valid column)."""
    nk = K // 32
    segs, seg = [], False
    if rows_per_slab is not None and slab_rows > 0 and slab_rows % 32 == 0 and K % slab_rows == 0 and not deterministic:
        nslabs, slab_steps = K // slab_rows, slab_rows // 32
        ld_max = max(lda, ldb)
        ok = nslabs * slab_steps < 65536 and K * (ldb2 if B2 and ldb2 > ld_max else ld_max) * 2 < (1 << 32)
        total = 0
        for t in range(nslabs):
            if not ok:
                break
            r = min(max(int(rows_per_slab[t]), 0), slab_rows)
            steps = (r + 31) // 32
            if steps == 0:
                continue
            if len(segs) == 16:
                ok = False
                break
            segs.append((t * slab_steps, steps))
            total += steps
        if ok and 0 < total < K // 32:
            seg, nk, K = True, total, total * 32
    if not seg:
        segs = []
    if forced_tile == 11 or (forced_tile == 0 and K <= 2048 and ceil_div(M, 128) * ceil_div(N, 128) >= 192):
        branch, splits = "tn128", 1
        tm, tn = ceil_div(M, 128), ceil_div(N, 128)
        per = nk
    elif forced_tile == 0 and N <= 128 and not B2:
        branch = "strip"
        tm, tn = ceil_div(M, 128), 1
        splits = min(256 // tm, K // 1024)
        if splits < 1 or deterministic:
            splits = 1
        while splits > 1 and ceil_div(nk, splits) * (splits - 1) >= nk:
            splits -= 1
        per = ceil_div(nk, splits)
    else:
        branch = "tile256"
        tm, tn = ceil_div(M, 256), ceil_div(N, 256)
        splits = min(256 // (tm * tn), K // 1024)
        if splits < 1 or deterministic:
            splits = 1
        per = ceil_div(nk, splits)
    walk = []
    for s in range(splits):
        if seg:                                         # gemm_tn_kernel, SEG
            off, sg = s * per, 0
            steps = min(per, nk - off)
            for i in range(15):
                adv = sg == i and i + 1 < len(segs) and off >= segs[i][1]
                off -= segs[i][1] if adv else 0
                sg += 1 if adv else 0
            walk.append((sg, off, steps))
        else:
            k0 = s * per if splits > 1 else 0
            walk.append((None, k0, min(per, nk - k0) if splits > 1 else nk))
    BM, BU, WR, WC = TILE[branch]
    WU = BU // WC
    ldc = N if ldc is None else ldc
    plain = splits == 1 and not accumulate
    stores = []
    for t in range(tn):
        n0, sN = t * BU, N
        if B2:
            if n0 >= N1:
                sN = c_col2 + (N - N1)
                n0 = c_col2 + (n0 - N1)
            else:
                sN = N1
        row = []
        for wc in range(WC):
            aligned = ldc % 4 == 0 and c_aligned and n0 + wc * WU + WU <= sN
            if n0 + wc * WU >= sN:
                row.append("none")
            elif plain and aligned:
                row.append("vec")
            elif splits == 1 and accumulate and aligned:
                row.append("rmw")
            elif plain:
                row.append("elementwise")
            else:
                row.append("atomic")
        stores.append(tuple(row))
    return {"branch": branch, "seg": seg, "segs": segs, "nk": nk, "splits": splits, "ksteps_per_split": per, "walk": walk,
            "memset": splits > 1 and not accumulate, "tiles_m": tm, "tiles_n": tn, "BM": BM, "BU": BU, "WM": BM // WR, "WU": WU,
            "stores": stores, "store_set": frozenset(p for r in stores for p in r if p != "none")}


def walk_steps(plan, split):
    """The absolute K steps (of 32 rows) that split `split` stages, in order: the mirror of gemm_mainloop_tn's K walk (gemm_core_tn.h: a_k /
    seg_left / advance()).  A split with a non-positive step count stages nothing."""
    sg, off, steps = plan["walk"][split]
    if steps <= 0:
        return []
    if sg is None:
        return list(range(off, off + steps))
    segs = plan["segs"]
    out, left, k = [], segs[sg][1] - off, segs[sg][0] + off
    for _ in range(steps):
        out.append(k)
        left -= 1
        if left == 0:
            sg += 1
            if sg < len(segs):
                k, left = segs[sg]
            else:
                k, left = 0, 0                         # (the kernel reads table entry 0 here; no step follows)
        else:
            k += 1
    return out


def path_name(plan):
    return "%s%s splits=%d x %d %s" % (plan["branch"], " seg" if plan["seg"] else "", plan["splits"], plan["ksteps_per_split"],
                                       "+".join(sorted(plan["store_set"])))


# ---------------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """One call of evc_gemm_tn / evc_gemm_tn2 / evc_gemm_tn2_rows.  N2 > 0: two column segments; rows / slab_rows: the row-plan entry;
    forced: EVC_FORCE_TILE of the process that runs it; det: EVC_DETERMINISTIC=1.  claim: what plan_tn must say (checked on the CPU)."""

    def __init__(self, name, M, N1, K, N2=0, H=0, c_col2=None, ldc_extra=8, base_off=0, rows=None, slab_rows=0, forced=0, det=False,
                 accs=(0, 1), kinds=("exact", "wide"), branch=None, seg=False, splits=1, stores=None, group=""):
        self.name, self.M, self.N1, self.N2, self.K, self.H = name, M, N1, N2, K, H
        self.N = N1 + N2
        self.c_col2 = (N1 if c_col2 is None else c_col2) if N2 else 0
        self.ncols = self.c_col2 + N2 if N2 else N1                  # columns of C the call owns (the gap included)
        self.ldc = self.ncols + ldc_extra
        self.base_off, self.rows, self.slab_rows, self.forced, self.det = base_off, rows, slab_rows, forced, det
        self.accs, self.kinds, self.group = accs, kinds, group
        self.lda = M + 8
        self.ldb1, self.ldb2 = N1 + 8, N2 + 24
        self.claim = {"branch": branch, "seg": seg, "splits": splits, "stores": stores}
        if rows is not None:
            assert K == slab_rows * len(rows)

    def plan(self, acc):
        return plan_tn(self.M, self.N, self.K, N1=self.N1 if self.N2 else 0, B2=self.N2 > 0, rows_per_slab=self.rows, slab_rows=self.slab_rows,
                       deterministic=self.det, forced_tile=self.forced, accumulate=bool(acc), ldc=self.ldc, c_col2=self.c_col2,
                       c_aligned=self.base_off % 4 == 0, lda=self.lda, ldb=self.ldb1, ldb2=self.ldb2)

    def live_mask(self):
        """[K] bool: the rows of A that may be non-zero, and [K] bool: the rows of B that a 32-row step of a live prefix covers."""
        if self.rows is None:
            return np.ones(self.K, bool), np.ones(self.K, bool)
        r = np.arange(self.K) % self.slab_rows
        cl = np.repeat(np.clip(np.asarray(self.rows), 0, self.slab_rows), self.slab_rows)
        return r < cl, r < (cl + 31) // 32 * 32

    def contracted(self, acc):
        """Rows the call walks: the live steps x 32 under the segment walk, all rows otherwise."""
        return self.plan(acc)["nk"] * 32


# row plans of the segment-walk cases: (name, slab_rows, rows, seg claimed)
_S16 = [5, 12, 7, 9, 6, 11, 8, 10, 5, 3, 4, 5, 3, 4, 5, 32]         # live steps of 16 slabs of 32: 129 steps -> 4 splits of 33 starting at
#                                                                   0 (segment 0), 33 (first step of segment 4), 66 (inside segment 7), 99 (inside segment 15)
ROW_PLANS = [
    ("one-step segments", 64, [32, 5, 17, 32, 1, 20, 9, 30], True),
    ("first slab empty", 128, [0, 100, 64, 33], True),
    ("clamped rows", 128, [-5, 200, 40, 128], True),
    ("16 slabs split", 1024, [s * 32 - (7 if s < 32 else 0) for s in _S16], True),
    ("17 slabs", 32, [20] * 17, False),
    ("nothing dead", 64, [64, 64, 33], False),
    ("all dead", 64, [0, 0, 0], False),
    ("slab_rows 48", 48, [20, 48], False),            # slab_rows % 32 != 0 with K % 32 == 0: no segment walk, the plain product
]


def _cases():
    c = []
    V, E, A_, R = "vec", "elementwise", "atomic", "rmw"

    def add(*a, **k):
        c.append(Case(*a, **k))
    # 1. tn128 forced (EVC_FORCE_TILE=11)
    for nk in (1, 2, 3, 4, 5, 6, 7, 8, 11):
        add("tn128f 136x136 nk=%d" % nk, 136, 136, nk * 32, forced=11, branch="tn128", group="tile11")
    add("tn128f 8x8x32", 8, 8, 32, forced=11, branch="tn128", group="tile11")
    add("tn128f 264x40x96", 264, 40, 96, forced=11, branch="tn128", group="tile11")
    for n2 in (8, 136):
        add("tn128f 136x(256+%d) nk=6" % n2, 136, 256, 192, N2=n2, forced=11, branch="tn128", group="tile11")
    # 2. tn128 by itself: 13 x 16 tiles
    add("tn128 1544x1928x160", 1544, 1928, 160, branch="tn128", group="natural")
    # 3. strip
    for K, sp in ((32, 1), (160, 1), (2080, 2), (3104, 3)):
        add("strip 264x72x%d" % K, 264, 72, K, branch="strip", splits=sp, group="natural")
    add("strip 8x8x40992", 8, 8, 40992, branch="strip", splits=39, group="natural")
    # 4. tile256
    for nk in (1, 2, 4, 5, 6, 9):
        add("tile256 264x264 nk=%d" % nk, 264, 264, nk * 32, branch="tile256", group="natural")
    for K, sp in ((2080, 2), (3104, 3)):
        add("tile256 264x264x%d" % K, 264, 264, K, branch="tile256", splits=sp, group="natural")
    for n2 in (8, 264):
        for K, sp in ((192, 1), (2080, 2)):
            add("tile256 264x(256+%d)x%d" % (n2, K), 264, 256, K, N2=n2, branch="tile256", splits=sp, group="natural")
            add("tile256 264x(256+%d)x%d gap" % (n2, K), 264, 256, K, N2=n2, c_col2=256 + 64, accs=(1,), branch="tile256", splits=sp, group="natural")
    add("tile256 8x136x40992", 8, 136, 40992, branch="tile256", splits=40, group="natural")
    # 5. row interleave
    for H in (66, 64):
        for n, br in ((72, "strip"), (264, "tile256")):
            for K, sp in ((160, 1), (2080, 2)):
                add("%s il H=%d %dx%dx%d" % (br, H, 4 * H, n, K), 4 * H, n, K, H=H, branch=br, splits=sp, group="natural")
    # 6. unaligned C
    for M, n, K, br, sp in ((264, 264, 64, "tile256", 1), (264, 264, 2080, "tile256", 2), (264, 72, 2080, "strip", 2)):
        add("%s %dx%dx%d ldc=N+2" % (br, M, n, K), M, n, K, ldc_extra=2, branch=br, splits=sp, group="natural")
        add("%s %dx%dx%d base+1" % (br, M, n, K), M, n, K, base_off=1, branch=br, splits=sp, group="natural")
    # 7. the segment walk, on each branch, with one and two column segments (the strip branch takes one segment only)
    for pname, slab, rows, segc in ROW_PLANS:
        K = slab * len(rows)
        big = pname == "16 slabs split"
        for tag, M, n1, n2, br, forced in (("tn128f", 136, 136, 0, "tn128", 11), ("tn128f", 136, 256, 8, "tn128", 11), ("strip", 264, 72, 0, "strip", 0),
                                           ("tile256", 264, 264, 0, "tile256", 0), ("tile256", 264, 256, 8, "tile256", 0)):
            sp = 4 if (big and br != "tn128") else 1
            add("%s rows %dx%s: %s" % (tag, M, "%d+%d" % (n1, n2) if n2 else n1, pname), M, n1, K, N2=n2, rows=rows, slab_rows=slab, forced=forced,
                branch=br, seg=segc, splits=sp, group="tile11" if forced else "natural")
    # the 40-split case again with live rows: 61 slabs of 672 rows (21 steps), 16 of them live
    rows = [0] * 61
    for i, t in enumerate(range(2, 61, 3)[:16]):
        rows[t] = 672 - 3 * i
    add("tile256 8x136x40992 live", 8, 136, 40992, rows=rows, slab_rows=672, branch="tile256", seg=True, splits=10, group="natural")
    return c


CASES = _cases()


def det_cases():
    """9.: the cases of 3, 4 and 7 with K >= 2080 under EVC_DETERMINISTIC=1: splits 1, no segment walk."""
    out = []
    for c in CASES:
        if c.K >= 2080 and c.forced == 0 and c.H == 0 and c.ldc == c.ncols + 8 and c.base_off == 0:
            d = Case("det " + c.name, c.M, c.N1, c.K, N2=c.N2, c_col2=c.c_col2 if c.N2 else None, rows=c.rows, slab_rows=c.slab_rows, det=True,
                     accs=c.accs, branch=c.claim["branch"], seg=False, splits=1, group="det")
            out.append(d)
    return out


DET_CASES = det_cases()
ALL_CASES = CASES + DET_CASES


def case_by_name(name):
    for c in ALL_CASES:
        if c.name == name:
            return c
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------------------
def to_bf16(x):
    """float -> the nearest bf16 value (round to nearest even), as float32."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32)


def bf16_bits(x):
    """float32 values that ARE bf16 values -> their 16-bit patterns (int16 view, for torch.bfloat16 tensors)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    assert not (u & 0xFFFF).any(), "not a bf16 value"
    return (u >> 16).astype(np.uint16).view(np.int16)


def q_of(K):
    return int(min(255, np.floor(np.sqrt(2.0 ** 24 / (K * 2.0)))))


class Data:
    pass


def make_data(case, kind, acc, seed=None):
    """Operands and the prefilled C buffer of one call.  A [K][lda], B1 [K][ldb1], B2 [K][ldb2] float32 holding bf16 values (the columns
    behind M / N hold 3.0: a loop that contracted them would show); buf0: the flat f32 buffer - FRONT + base_off sentinels, (M + BACK_ROWS)
    rows of ldc floats with C0 (accumulate) or NaN (plain) in the columns the call owns and sentinels elsewhere (the segment gap too)."""
    rng = np.random.default_rng(zlib.crc32(("%s|%s|%d" % (case.name, kind, acc)).encode()) if seed is None else seed)
    d = Data()
    M, K = case.M, case.K
    liveA, liveB = case.live_mask()
    Kc = case.contracted(acc)
    d.q = q_of(Kc)

    def operand(n, ld, is_a):
        x = np.full((K, ld), 3.0, np.float32)
        if kind == "exact":
            v = rng.integers(-d.q, d.q + 1, (K, n)).astype(np.float32) * np.float32(SA if is_a else SB)
        else:
            v = rng.standard_normal((K, n))
            if is_a:
                v = v * 10.0 ** rng.uniform(-6, -1, (K, n))
            else:
                v[:, ::5] *= 1e-3
            v = np.where(np.abs(v) < 1e-15, np.copysign(1e-15, v), v)
            v = to_bf16(v)
        if is_a:
            v[~liveA] = 0.0
        else:
            g = np.where(rng.integers(0, 2, (K, n)) > 0, GARBAGE, -GARBAGE).astype(np.float32)
            v = np.where(liveB[:, None], v, g)
        x[:, :n] = v
        return x
    d.A = operand(M, case.lda, True)
    d.B1 = operand(case.N1, case.ldb1, False)
    d.B2 = operand(case.N2, case.ldb2, False) if case.N2 else None
    d.c0 = FRONT + case.base_off
    buf = np.full(d.c0 + (M + BACK_ROWS) * case.ldc, SENT, np.float32)
    C = buf[d.c0:].reshape(M + BACK_ROWS, case.ldc)
    for c0, w in owned_columns(case):
        if not acc:
            C[:M, c0:c0 + w] = np.nan
        elif kind == "exact":
            C[:M, c0:c0 + w] = rng.integers(-2 ** 22, 2 ** 22 + 1, (M, w)).astype(np.float32) * np.float32(SA * SB)
        else:
            C[:M, c0:c0 + w] = (rng.standard_normal((M, w)) * 1e-2).astype(np.float32)
    d.buf0 = buf
    d.kind, d.acc = kind, acc
    return d


def owned_columns(case):
    return [(0, case.N1)] + ([(case.c_col2, case.N2)] if case.N2 else [])


def out_rows(M, H):
    """Row of C that row m of the product goes to: the gate de-interleave u*4+g -> g*H+u."""
    m = np.arange(M)
    return (m % 4) * H + m // 4 if H else m


# ---------------------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------------------
def int_product(ia, ib):
    """The integer product ia^T ib as int64.  Computed by float64 BLAS: with sum |ia||ib| < 2^53 every float64 partial sum is an exact
    integer, so this IS the int64 product (tests/test_cpu_wgrad_ref.py compares it with numpy's int64 matmul)."""
    ia, ib = np.asarray(ia, np.float64), np.asarray(ib, np.float64)
    assert (ia == np.rint(ia)).all() and (ib == np.rint(ib)).all()
    assert float(np.abs(ia).sum(0).max()) * float(np.abs(ib).max(initial=0)) < 2.0 ** 53
    p = ia.T @ ib
    assert (p == np.rint(p)).all()
    return p.astype(np.int64)


def products(case, d, rows=None):
    """Per column segment: the product over the live rows (or the given K rows) as float64 - for the exact kind the integer product scaled
    by SA SB (exact in float64) - and sum_k |a_k b_k|."""
    liveA, _ = case.live_mask()
    idx = np.flatnonzero(liveA)
    if rows is not None:
        idx = np.intersect1d(idx, np.asarray(rows, np.int64))
    A = d.A[idx, :case.M].astype(np.float64)
    out = []
    for B, n in ((d.B1, case.N1), (d.B2, case.N2)):
        if not n:
            continue
        Bv = B[idx, :n].astype(np.float64)
        if d.kind == "exact":
            P = int_product(A / SA, Bv / SB).astype(np.float64) * (SA * SB)
        else:
            P = A.T @ Bv
        out.append((P, np.abs(A).T @ np.abs(Bv)))
    return out


def reference(case, d, prods=None, depth=None):
    """The expected buffer as float64 (sentinels and the gap untouched), and the wide kind's limit d (zero outside C's owned columns).
    depth: the factor of U in d, (rows walked + splits + 1) by plan_tn unless given."""
    prods = products(case, d) if prods is None else prods
    acc = d.acc
    plan = case.plan(acc)
    exp = d.buf0.astype(np.float64)
    lim = np.zeros_like(exp)
    M, ldc = case.M, case.ldc
    E = exp[d.c0:].reshape(M + BACK_ROWS, ldc)
    L = lim[d.c0:].reshape(M + BACK_ROWS, ldc)
    orow = out_rows(M, case.H)
    depth = plan["nk"] * 32 + plan["splits"] + 1 if depth is None else depth
    for (c0, w), (P, S) in zip(owned_columns(case), prods):
        C0 = E[orow, c0:c0 + w] if acc else np.zeros((M, w))
        L[orow, c0:c0 + w] = depth * U * (S + np.abs(C0))
        E[orow, c0:c0 + w] = C0 + P
    return exp, lim


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def where_is(case, plan, d, flat):
    """Names the element at a flat buffer index: row / column of C, and the tile, wave, split and segment that own it."""
    if flat < d.c0:
        return "front sentinel %d" % flat
    r, c = divmod(int(flat) - d.c0, case.ldc)
    if r >= case.M:
        return "row %d col %d (behind row M=%d)" % (r, c, case.M)
    H = case.H
    m = (r % H) * 4 + r // H if H else r
    own = None
    for s, (c0, w) in enumerate(owned_columns(case)):
        if c0 <= c < c0 + w:
            own = (s, c - c0)
    if own is None:
        return "row %d col %d (%s)" % (r, c, "segment gap" if c < case.ncols else "columns [N, ldc)")
    s, cc = own
    n = cc + (case.N1 if s else 0)
    BM, BU, WM, WU = plan["BM"], plan["BU"], plan["WM"], plan["WU"]
    sp = "all %d splits" % plan["splits"] if plan["splits"] > 1 else "one split"
    return "row %d col %d = product row %d col %d: tile (%d, %d) wave (%d, %d) store %s, %s, column segment %d%s" % (
        r, c, m, n, m // BM, n // BU, m % BM // WM, n % BU // WU, plan["stores"][n // BU][n % BU // WU], sp, s,
        ", %d K segments" % len(plan["segs"]) if plan["seg"] else "")


def check(case, d, got, exp, lim=None, plan=None):
    """got (flat float32 buffer) against the reference.  exact kind: every element bit for bit.  wide kind: |got - exp| <= lim inside C's owned
    columns, every other element (sentinels, gap, rows behind M) bit for bit.  Returns (bad: flat bool mask, worst err/lim or 0.0, where the
    worst / first bad element is, message)."""
    plan = case.plan(d.acc) if plan is None else plan
    got = np.ascontiguousarray(got, np.float32)
    e32 = exp.astype(np.float32)
    if d.kind == "exact":
        assert np.array_equal(e32.astype(np.float64), exp, equal_nan=True), "the reference is not exact in f32"
        bad = bits(got) != bits(e32)
        ratio, at = 0.0, None
    else:
        inside = lim > 0
        err = np.abs(got.astype(np.float64) - exp)
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(inside, err / np.where(inside, lim, 1.0), 0.0)
        r = np.where(np.isnan(r), np.inf, r)
        bad = np.where(inside, r > 1.0, bits(got) != bits(e32))
        at = int(np.argmax(r))
        ratio = float(r[at])
    msg = ""
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        msg = "%s [%s, %s]: %d elements differ; first at flat %d: %s: got %r want %r" % (
            case.name, path_name(plan), d.kind, int(bad.sum()), i, where_is(case, plan, d, i), float(got[i]), float(exp[i]))
    at = int(np.flatnonzero(bad)[0]) if (at is None and bad.any()) else at
    return bad, ratio, at, msg


def sentinels_intact(case, d, got):
    """True if every element outside C's owned columns still holds what buf0 held."""
    keep = np.ones(d.buf0.shape, bool)
    K2 = keep[d.c0:].reshape(case.M + BACK_ROWS, case.ldc)
    for c0, w in owned_columns(case):
        K2[:case.M, c0:c0 + w] = False
    return bool((bits(got)[keep] == bits(d.buf0)[keep]).all())


# ---------------------------------------------------------------------------------------------------------------------------------------
# f32 emulations (premises)
# ---------------------------------------------------------------------------------------------------------------------------------------
def f32_orders(a, b, c0, splits, rng):
    """sum_k a[k][:, None] b[k][None, :] + c0 in f32 in three orders: one element after the other; 32-row steps in order inside `splits`
    splits that are joined onto c0 in shuffled order; pairwise tree.  a [K][m], b [K][n] float32, c0 [m][n] float32."""
    K = a.shape[0]
    prod = (a[:, :, None] * b[:, None, :]).astype(np.float32)        # every product is exact in f32 for the exact kind; rounded once otherwise
    seq = c0.copy()
    for k in range(K):
        seq = seq + prod[k]
    nk = ceil_div(K, 32)
    per = ceil_div(nk, splits)
    parts = []
    for s in range(splits):
        acc = np.zeros_like(c0)
        for k in range(s * per * 32, min((s + 1) * per * 32, K)):
            acc = acc + prod[k]
        parts.append(acc)
    spl = c0.copy()
    for s in rng.permutation(splits):
        spl = spl + parts[s]
    t = prod
    while t.shape[0] > 1:
        if t.shape[0] % 2:
            t = np.concatenate([t, np.zeros_like(t[:1])])
        t = t[0::2] + t[1::2]
    tree = (t[0] if t.shape[0] else np.zeros_like(c0)) + c0
    return seq.astype(np.float32), spl.astype(np.float32), tree.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# a model of the launch for the planted faults
# ---------------------------------------------------------------------------------------------------------------------------------------
FAULTS = ("dropped step", "doubled step", "segment start + 1", "last split lost", "second split late", "gate rows swapped",
          "de-interleave skipped in one tile", "second segment at N1", "second segment read with ldb1", "ragged chunk from its neighbour",
          "C0 dropped", "C0 kept", "slab added twice", "memset of ldc columns")


def model(case, d, fault=None, slabs=0):
    """What the launch computes, tile by tile, split by split, from plan_tn's walk - in float64, which is exact for the exact kind - with one
    planted fault.  slabs > 0: the deterministic form (partial images per split of `slabs` slabs, added in slab order).  Returns the flat
    buffer.  Without a fault it must reproduce reference() (the CPU test asserts that: it ties plan_tn's walk to the live rows)."""
    acc = d.acc
    plan = case.plan(acc)
    M, H, ldc = case.M, case.H, case.ldc
    buf = d.buf0.astype(np.float64)
    C = buf[d.c0:].reshape(M + BACK_ROWS, ldc)
    splits, per = plan["splits"], plan["ksteps_per_split"]
    if slabs:
        nk = case.K // 32
        per = ceil_div(nk, slabs)
        split_steps = [list(range(s * per, min((s + 1) * per, nk))) for s in range(slabs)]
        segs = None
    else:
        segs = list(plan["segs"])
        if fault == "segment start + 1":
            segs[1] = (segs[1][0] + 1, segs[1][1])
        p2 = dict(plan, segs=segs)
        split_steps = [walk_steps(p2, s) for s in range(splits)]
    if fault == "last split lost":
        split_steps[-1] = []
    if fault == "second split late":
        split_steps[1] = split_steps[1][1:]
    if plan["memset"] and not slabs:
        C[:M, :(ldc if fault == "memset of ldc columns" else case.N)] = 0.0
    plain = bool(slabs) or (splits == 1 and not acc)
    if fault == "C0 dropped":
        plain = True
    if fault == "C0 kept":
        plain = False
    BM, BU = plan["BM"], plan["BU"]
    g_swap = {1: 2, 2: 1} if fault == "gate rows swapped" else {}
    A = d.A.astype(np.float64)
    B1f = d.B1.astype(np.float64)
    B2f = d.B2.astype(np.float64) if case.N2 else None
    total = np.zeros((M + BACK_ROWS, ldc))
    wrote = np.zeros((M + BACK_ROWS, ldc), bool)
    parts = [np.zeros((M + BACK_ROWS, ldc)) for _ in split_steps]
    for tm in range(plan["tiles_m"]):
        m0, m1 = tm * BM, min(tm * BM + BM, M)
        for tn in range(plan["tiles_n"]):
            n0 = tn * BU
            if case.N2 and n0 >= case.N1:
                B, ldb, nb, nseg, ccol = B2f, case.ldb2, n0 - case.N1, case.N2, case.c_col2
                if fault == "second segment at N1":
                    ccol = case.N1
                if fault == "second segment read with ldb1":
                    B = B2f.reshape(-1)[:case.K * case.ldb1].reshape(case.K, case.ldb1)
            else:
                B, ldb, nb, nseg, ccol = B1f, case.ldb1, n0, case.N1, 0
            n1 = min(nb + BU, nseg)
            cols = np.arange(nb, n1)
            src = cols.copy()
            if fault == "ragged chunk from its neighbour" and n1 == nseg and nseg % BU:
                src[-8:] -= 8
            m = np.arange(m0, m1)
            g, u = m % 4, m // 4
            if H:
                g = np.array([g_swap.get(int(x), int(x)) for x in g])
                orow = g * H + u
            else:
                orow = m
            if fault == "de-interleave skipped in one tile" and tm == plan["tiles_m"] - 1 and tn == 0:
                orow = m
            for s, steps in enumerate(split_steps):
                steps = list(steps)
                if (tm, tn, s) == (0, 0, splits - 1 if not slabs else 0):
                    if fault == "dropped step":
                        del steps[len(steps) // 2]
                    if fault == "doubled step":
                        steps.insert(0, steps[len(steps) // 2])
                P = np.zeros((m1 - m0, n1 - nb))
                for k in steps:
                    P += A[k * 32:k * 32 + 32, m0:m1].T @ B[k * 32:k * 32 + 32, src]
                parts[s][np.ix_(orow, ccol + cols)] += P
            wrote[np.ix_(orow, ccol + cols)] = True
    if slabs:
        order = list(range(slabs))
        if fault == "slab added twice":
            order.insert(1, 0)
        for s in order:
            total += parts[s]
        plain = not acc
    else:
        for p in parts:
            total += p
    if plain:
        C[wrote] = total[wrote]
    else:
        C[wrote] = C[wrote] + total[wrote]
    return buf
