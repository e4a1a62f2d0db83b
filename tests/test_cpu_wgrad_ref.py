"""The host side of the weight-gradient parity tests (tests/_wgrad_ref.py), without a GPU: the premises of the two data kinds, that the
case list reaches every path of the dispatch, and that the checker catches planted faults at the elements they must move."""
import numpy as np
import pytest

import _wgrad_ref as wr

RUNS = [(c, acc) for c in wr.ALL_CASES for acc in c.accs]
IDS = ["%s acc=%d" % (c.name, acc) for c, acc in RUNS]


def _sample(case, d, rng, n=24):
    """A sample of the product for the f32 emulations: up to n rows and n columns, the first and the last ones always among them."""
    def pick(m):
        if m <= n:
            return np.arange(m)
        return np.unique(np.concatenate([[0, 1, m - 2, m - 1], rng.choice(m, n - 4, replace=False)]))
    live = np.flatnonzero(case.live_mask()[0])
    mi = pick(case.M)
    B = d.B2 if case.N2 else d.B1
    ni = pick(case.N2 if case.N2 else case.N1)
    c0 = case.c_col2 if case.N2 else 0
    C = d.buf0[d.c0:].reshape(case.M + wr.BACK_ROWS, case.ldc)
    orow = wr.out_rows(case.M, case.H)
    C0 = C[np.ix_(orow[mi], c0 + ni)] if d.acc else np.zeros((len(mi), len(ni)), np.float32)
    return d.A[np.ix_(live, mi)], B[np.ix_(live, ni)], C0.astype(np.float32)


@pytest.mark.parametrize("case,acc", RUNS, ids=IDS)
def test_exactness_premise(case, acc):
    """sum |ia||ib| + |C0| / (SA SB) < 2^24 for the whole product, and - on a sample of rows and columns, over all live K rows - f32 sums
    in three orders give the integer product bit for bit."""
    d = wr.make_data(case, "exact", acc)
    exp, _ = wr.reference(case, d)
    prods = wr.products(case, d)
    C = d.buf0[d.c0:].reshape(case.M + wr.BACK_ROWS, case.ldc).astype(np.float64)
    orow = wr.out_rows(case.M, case.H)
    for (c0, w), (P, S) in zip(wr.owned_columns(case), prods):
        C0 = np.abs(C[orow, c0:c0 + w]) if acc else 0.0
        assert ((S + C0) / (wr.SA * wr.SB)).max() < 2.0 ** 24
    assert np.array_equal(exp.astype(np.float32).astype(np.float64), exp, equal_nan=True)
    rng = np.random.default_rng(5)
    a, b, c0 = _sample(case, d, rng, 16 if case.K > 8192 else 24)
    want = (wr.int_product(a / wr.SA, b / wr.SB) * (wr.SA * wr.SB) + c0.astype(np.float64)).astype(np.float32)
    for name, got in zip(("sequential", "steps and splits", "tree"), wr.f32_orders(a, b, c0, max(case.plan(acc)["splits"], 3), rng)):
        assert np.array_equal(wr.bits(got), wr.bits(want)), name


@pytest.mark.parametrize("case,acc", RUNS, ids=IDS)
def test_bound_premise(case, acc):
    """The wide kind: f32 sums in the same three orders stay inside d, on a sample."""
    d = wr.make_data(case, "wide", acc)
    rng = np.random.default_rng(6)
    a, b, c0 = _sample(case, d, rng, 16 if case.K > 8192 else 24)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    want = a64.T @ b64 + c0
    plan = case.plan(acc)
    lim = (plan["nk"] * 32 + plan["splits"] + 1) * wr.U * (np.abs(a64).T @ np.abs(b64) + np.abs(c0))
    assert np.abs(a64[a64 != 0]).min(initial=1.0) >= 1e-15 and np.abs(b64).min(initial=1.0) >= 1e-15
    for name, got in zip(("sequential", "steps and splits", "tree"), wr.f32_orders(a, b, c0, max(plan["splits"], 3), rng)):
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= lim).all(), (name, float((err / np.maximum(lim, 1e-300)).max()))


def test_int_product_is_the_int64_product():
    rng = np.random.default_rng(1)
    for K, q in ((32, 255), (4128, 45), (40992, 14)):
        ia, ib = rng.integers(-q, q + 1, (K, 24)), rng.integers(-q, q + 1, (K, 40))
        assert np.array_equal(wr.int_product(ia, ib), ia.astype(np.int64).T @ ib.astype(np.int64))
    assert wr.q_of(128) == 255 and wr.q_of(40992) == 14 and wr.q_of(32) == 255


# every (branch, segment walk, splits > 1, store) the dispatch can reach.  Not in the list, because the code cannot get there:
#   tn128 with splits > 1        the branch launches one workgroup per tile whatever K is (StoreParamsT s1{..., 1, p.nk, 0})
#   vec / rmw / elementwise with splits > 1   gemm_tn_kernel: `plain` needs splits == 1 (or a slab store), the read-modify-write store too: a split
#                                product is always joined by atomics
#   strip with two column segments   the strip branch is taken with !B2 only
REACHABLE = {(b, s, m, st) for b in ("tn128", "strip", "tile256") for s in (False, True) for m in (False,) for st in ("vec", "rmw", "elementwise", "atomic")} | \
            {(b, s, True, "atomic") for b in ("strip", "tile256") for s in (False, True)}


def test_coverage_every_case_takes_its_path_and_every_path_has_a_case():
    seen = {}
    for c, acc in RUNS:
        p = c.plan(acc)
        assert (p["branch"], p["seg"], p["splits"]) == (c.claim["branch"], c.claim["seg"], c.claim["splits"]), (c.name, acc, wr.path_name(p))
        if c.det:
            assert p["splits"] == 1 and not p["seg"]
        assert sum(len(wr.walk_steps(p, s)) for s in range(p["splits"])) == p["nk"]
        for st in p["store_set"]:
            seen.setdefault((p["branch"], p["seg"], p["splits"] > 1, st), c.name)
    assert set(seen) <= REACHABLE, set(seen) - REACHABLE
    assert not REACHABLE - set(seen), "no case for %s" % sorted(REACHABLE - set(seen))
    # the named paths of single cases
    p = wr.case_by_name("tn128 1544x1928x160").plan(0)
    assert (p["tiles_m"], p["tiles_n"]) == (13, 16) and p["stores"][15] == ("elementwise", "none", "none", "none") and p["stores"][0] == ("vec",) * 4
    p = wr.case_by_name("strip 8x8x40992").plan(0)
    assert p["splits"] == 39 and p["walk"][-1] == (None, 38 * 33, 27)
    p = wr.case_by_name("tile256 8x136x40992").plan(0)
    assert p["splits"] == 40 and p["ksteps_per_split"] == 33 and p["walk"][-1] == (None, 1287, -6) and wr.walk_steps(p, 39) == []
    p = wr.case_by_name("tile256 rows 264x264: 16 slabs split").plan(0)
    assert len(p["segs"]) == 16 and [w[:2] for w in p["walk"]] == [(0, 0), (4, 0), (7, 8), (15, 2)]    # a first step, mid-segment, inside segment 15
    p = wr.case_by_name("tile256 rows 264x264: one-step segments").plan(0)
    assert [s[1] for s in p["segs"]] == [1] * 8
    assert wr.case_by_name("tile256 rows 264x264: first slab empty").plan(0)["segs"][0][0] == 4
    assert [s[1] for s in wr.case_by_name("tile256 rows 264x264: clamped rows").plan(0)["segs"]] == [4, 2, 4]
    for n in ("tile256 264x264x64", "tile256 264x264x2080", "strip 264x72x2080"):
        for tag in (" ldc=N+2", " base+1"):
            c = wr.case_by_name(n + tag)
            assert c.plan(0)["store_set"] == ({"elementwise"} if c.K == 64 else {"atomic"})
            assert c.plan(1)["store_set"] == {"atomic"}                  # accumulate with splits = 1 goes through atomics here too
    for H in (66, 64):
        assert wr.case_by_name("tile256 il H=%d %dx264x160" % (H, 4 * H)).plan(1)["store_set"] == {"rmw", "atomic"}


@pytest.mark.parametrize("case,acc", RUNS, ids=IDS)
def test_the_model_of_the_launch_reproduces_the_reference(case, acc):
    """plan_tn's walk, contracted tile by tile, is the product over the live rows: the mirror and the row plans agree."""
    d = wr.make_data(case, "exact", acc)
    exp, _ = wr.reference(case, d)
    bad, _, _, msg = wr.check(case, d, wr.model(case, d).astype(np.float32), exp)
    assert not bad.any(), msg


def _fault_case(fault):
    """(case name, accumulate, slabs) on which a fault is planted."""
    return {"dropped step": ("tile256 264x264x2080", 0, 0), "doubled step": ("strip 264x72x3104", 1, 0),
            "segment start + 1": ("tile256 rows 264x256+8: first slab empty", 0, 0), "last split lost": ("tile256 264x264x3104", 0, 0),
            "second split late": ("strip 264x72x2080", 1, 0), "gate rows swapped": ("tile256 il H=66 264x264x160", 0, 0),
            "de-interleave skipped in one tile": ("tile256 il H=66 264x264x160", 1, 0), "second segment at N1": ("tile256 264x(256+8)x192 gap", 1, 0),
            "second segment read with ldb1": ("tile256 264x(256+264)x192", 0, 0), "ragged chunk from its neighbour": ("tn128f 264x40x96", 0, 0),
            "C0 dropped": ("tile256 264x264 nk=5", 1, 0), "C0 kept": ("tile256 264x264 nk=5", 0, 0), "slab added twice": ("tile256 264x264x3104", 1, 3),
            "memset of ldc columns": ("strip 264x72x2080", 0, 0)}[fault]


def _predicted(fault, case, d, exp):
    """The elements a fault must move, worked out from the operands and the reference - not from the model."""
    M, H, ldc = case.M, case.H, case.ldc
    plan = case.plan(d.acc)
    pred = np.zeros(exp.shape, bool)
    P2 = pred[d.c0:].reshape(M + wr.BACK_ROWS, ldc)
    E = exp[d.c0:].reshape(M + wr.BACK_ROWS, ldc)
    A = d.A[:, :M].astype(np.float64)
    orow = wr.out_rows(M, H)

    def step_product(k, B, n):
        return A[k * 32:k * 32 + 32].T @ B[k * 32:k * 32 + 32, :n].astype(np.float64)
    BM, BU = plan["BM"], plan["BU"]
    if fault in ("dropped step", "doubled step"):                 # tile (0, 0), last split, its middle step
        st = wr.walk_steps(plan, plan["splits"] - 1)
        D = step_product(st[len(st) // 2], d.B1, case.N1)[:BM, :BU]
        P2[np.ix_(orow[:min(BM, M)], np.arange(D.shape[1]))] = D != 0
    elif fault == "segment start + 1":                            # segment 1 loses its first step; the step behind its end is dead: zeros in A
        k = plan["segs"][1][0]
        for (c0, w), B in zip(wr.owned_columns(case), (d.B1, d.B2)):
            P2[np.ix_(orow, c0 + np.arange(w))] = step_product(k, B, w) != 0
    elif fault in ("last split lost", "second split late"):
        st = wr.walk_steps(plan, plan["splits"] - 1) if fault == "last split lost" else wr.walk_steps(plan, 1)[:1]
        D = sum(step_product(k, d.B1, case.N1) for k in st)
        P2[np.ix_(orow, np.arange(case.N1))] = D != 0
    elif fault == "gate rows swapped":                            # gates 1 and 2 of every unit
        u = np.arange(H)
        P2[H + u, :case.N1] = P2[2 * H + u, :case.N1] = E[H + u, :case.N1] != E[2 * H + u, :case.N1]
    elif fault == "de-interleave skipped in one tile":            # the last row tile, column tile 0, under accumulate: its rows land at row m
        P = wr.products(case, d)[0][0]
        F = np.zeros_like(E)
        m = np.arange((plan["tiles_m"] - 1) * BM, M)
        cols = np.arange(min(BU, case.N1))
        F[np.ix_(orow[m], cols)] -= P[np.ix_(m, cols)]
        F[np.ix_(m, cols)] += P[np.ix_(m, cols)]
        P2[:] = F != 0
    elif fault == "second segment at N1":
        P = wr.products(case, d)[1][0]
        F = np.zeros_like(E)
        F[np.ix_(orow, case.c_col2 + np.arange(case.N2))] -= P
        F[np.ix_(orow, case.N1 + np.arange(case.N2))] += P
        P2[:] = F != 0
    elif fault == "second segment read with ldb1":
        Bw = d.B2.reshape(-1)[:case.K * case.ldb1].reshape(case.K, case.ldb1)[:, :case.N2].astype(np.float64)
        P2[np.ix_(orow, case.c_col2 + np.arange(case.N2))] = (A.T @ Bw) != wr.products(case, d)[1][0]
    elif fault == "ragged chunk from its neighbour":
        n = case.N1
        P2[np.ix_(orow, np.arange(n - 8, n))] = E[np.ix_(orow, np.arange(n - 16, n - 8))] != E[np.ix_(orow, np.arange(n - 8, n))]
    elif fault == "C0 dropped":
        C0 = d.buf0[d.c0:].reshape(M + wr.BACK_ROWS, ldc)
        P2[:M, :case.N1] = C0[:M, :case.N1] != 0
    elif fault == "C0 kept":                                      # NaN + product
        P2[:M, :case.N1] = True
    elif fault == "slab added twice":                             # slab 0 of 3: K steps [0, 33)
        D = sum(step_product(k, d.B1, case.N1) for k in range(33))
        P2[np.ix_(orow, np.arange(case.N1))] = D != 0
    elif fault == "memset of ldc columns":
        P2[:M, case.N:ldc] = True
    return pred


@pytest.mark.parametrize("fault", wr.FAULTS)
def test_power_planted_faults_are_caught_where_predicted(fault):
    name, acc, slabs = _fault_case(fault)
    case = wr.case_by_name(name)
    d = wr.make_data(case, "exact", acc)
    exp, _ = wr.reference(case, d)
    clean, _, _, msg = wr.check(case, d, wr.model(case, d, slabs=slabs).astype(np.float32), exp)
    assert not clean.any(), msg
    bad, _, _, msg = wr.check(case, d, wr.model(case, d, fault, slabs=slabs).astype(np.float32), exp)
    pred = _predicted(fault, case, d, exp)
    assert pred.any() and np.array_equal(bad, pred), (int(bad.sum()), int(pred.sum()), msg)
    assert wr.where_is(case, case.plan(acc), d, int(np.flatnonzero(bad)[0])) in msg
    if fault in ("dropped step", "last split lost", "gate rows swapped", "C0 dropped", "second segment read with ldb1"):     # the wide kind sees these too
        d = wr.make_data(case, "wide", acc)
        exp, lim = wr.reference(case, d)
        assert not wr.check(case, d, wr.model(case, d, slabs=slabs).astype(np.float32), exp, lim)[0].any()
        bad, ratio, _, _ = wr.check(case, d, wr.model(case, d, fault, slabs=slabs).astype(np.float32), exp, lim)
        assert ratio > 1.0 and bad.any() and not (bad & ~_predicted(fault, case, d, exp)).any()


def test_fault_list_is_complete():
    assert len(wr.FAULTS) >= 14 and len(set(wr.FAULTS)) == len(wr.FAULTS)


def test_sentinel_check_sees_a_single_changed_float():
    case = wr.case_by_name("tile256 264x(256+8)x192 gap")
    d = wr.make_data(case, "exact", 1)
    exp, _ = wr.reference(case, d)
    got = exp.astype(np.float32)
    assert wr.sentinels_intact(case, d, got) and not wr.check(case, d, got, exp)[0].any()
    for flat in (0, d.c0 - 1, d.c0 + 300, d.c0 + case.M * case.ldc, d.c0 + case.ldc - 1):
        g = got.copy()
        g[flat] = 0.0
        assert not wr.sentinels_intact(case, d, g)
        bad = wr.check(case, d, g, exp)[0]
        assert bad.sum() == 1 and bad[flat]
