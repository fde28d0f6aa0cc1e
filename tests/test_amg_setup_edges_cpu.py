"""CPU suite of tests/amg_setup_synth.py, the inputs and the reference of tests/test_gpu_amg_setup_edges.py: every synthetic
case has the shape it is named for, the bit-exact restatement `setup_bits` of the device's numeric set-up chain
(csrc/amg_setup.hpp) lies within the level-local bounds of tests/amg_refresh_ref.level_bounds of an independent longdouble
chain, agrees with `fem.amg_refresh` wherever the two orders of summation coincide, and every edge is visible: a restatement
with the fault a case is there for differs from `setup_bits` in at least one bit of what a read-back sees on that case, and
in none on a case without the edge.

Measured here (printed by the tests): |setup_bits - setup_ld| against the level bounds, worst over all cases and both
matrices: ω and ω/d 0.32 of (kA + 2) u, P 0.35 of its bound, A_{l+1} 0.12 of its bound (the chains, kA = 3; the long-row
cases stay below 0.003: the bounds grow with the longest row, the error does not). Against `fem.amg_refresh` on the mesh
pairs: ω, g, ω/d and P bit-equal, A_{l+1} at most 0.014 of its bound."""
import numpy as np
import pytest
import scipy.sparse as sp

import amg_refresh_ref as rr
import amg_setup_synth as sz

NT = sz.NT


def _blocks(n):
    return (n + NT - 1) // NT


def _top_two(A):
    r = sz.ratios(A)
    o = np.argsort(-r, kind="stable")
    return int(o[0]), int(o[1]), float(r[o[0]]), float(r[o[1]]), float(r[o[2]])


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("r", sz.GERSH_ROWS)
def test_gershgorin_position_cases(r):
    """1 025 rows = four full blocks and a block of one row; the strict maximum of the ratio in row r, the runner-up in
    another wave and another block at least 10 % lower, every other row lower still — in both matrices"""
    A0, A1, aggs = sz.case(f"gersh_{r}")
    assert A0.shape[0] == 1025 and _blocks(1025) == 5 and 1025 % NT == 1
    for w, A in enumerate((A0, A1)):
        i, j, a, b, c = _top_two(A)
        assert i == r and j == sz.gersh_second(r) and b <= 0.9 * a and c < 0.9 * b
        assert i // NT != j // NT and (i % NT) // 64 != (j % NT) // 64
        assert abs(sz.bits(f"gersh_{r}", w).g[0] - a) <= 4 * sz.U * a      # (scipy's row sum has its own order)
    assert {(r // NT, (r % NT) // 64) for r in sz.GERSH_ROWS} >= {(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (3, 3), (4, 0)}
    assert {r % 64 for r in sz.GERSH_ROWS} >= {0, 63}


@pytest.mark.parametrize("name", list(sz.BIG))
def test_more_than_256_partials(name):
    """256, 257 and 301 workgroup partials on level 0 (k_as_omega makes a second pass from 257 on); the maximum and the
    runner-up on the sides of partial 256 the name says; four levels down to at most 200 rows, every level a chain"""
    n, peak, second = sz.BIG[name]
    A0, A1, aggs = sz.case(name)
    assert A0.shape[0] == n and _blocks(n) == {65536: 256, 65537: 257, 76801: 301}[n]
    for A in (A0, A1):
        i, j, a, b, c = _top_two(A)
        assert (i, j) == (peak, second) and b <= 0.9 * a and c < 0.9 * b
    if name.endswith("_hi"):
        assert peak // NT >= NT and second // NT < NT
    if name.endswith("_lo"):
        assert peak // NT < NT and second // NT >= NT
    B = sz.bits(name)
    assert B.nlevels in (4, 5) and B.sizes[-1] <= 200 and B.sizes[1] == (n + 7) // 8
    assert all(np.diff(a.indptr).max() == 3 for a in B.A)
    assert max(_blocks(m) for m in B.sizes[1:]) <= NT
    assert {_blocks(v[0]) for v in sz.BIG.values()} == {256, 257, 301}


def test_long_rows(fem):
    """the head row of the arrows: 1 024, 1 025 and 2 049 entries (one thread's sum in k_as_gersh, one thread's walk in
    k_as_product); the head touches every aggregate (a long row of P, and every column of A P); arrow_seg: one segment of
    1 024 entries and R rows of 1 025 and 1 026; giant: the R row of the 1 100-node aggregate"""
    for name, (m, w) in sz.ARROW.items():
        A0, _, aggs = sz.case(name)
        B = sz.bits(name)
        nc = (m + w - 1) // w
        assert np.diff(A0.indptr)[0] == m == A0.shape[0] and np.diff(A0.indptr)[1:].max() == 2
        assert np.diff(B.P[0].indptr)[0] == nc == B.sizes[1] and np.diff(B.AP[0].indptr)[0] == nc
        assert np.diff(sz.transposed(B.P[0]).indptr)[0] == m             # column 0 of P: every node touches the head
        assert B.A[1].nnz == nc * nc
    assert {m for m, _ in sz.ARROW.values()} == {1024, 1025, 2049} and max((m + w - 1) // w for m, w in sz.ARROW.values()) > 512
    A0, _, aggs = sz.case("arrow_seg")
    prow, pcol, ln, own = sz.segment_lengths(A0, aggs[0])
    assert np.diff(A0.indptr)[0] == 1025 and ln.max() == 1024 and prow[np.argmax(ln)] == 0 and pcol[np.argmax(ln)] == 1
    assert np.diff(sz.transposed(sz.bits("arrow_seg").P[0]).indptr).tolist()[:2] == [1025, 1026]   # node 0 touches both; node 1025 aggregate 1
    B = sz.bits("giant", fem=fem)
    assert np.diff(sz.transposed(B.P[0]).indptr).max() >= 1100 and np.diff(B.A[0].indptr).max() <= 7


def test_segments_case():
    """segments of 1, 2 and kA entries; the own aggregate first and last in its row of P; an own segment that is the
    diagonal entry alone; a row of P of one entry"""
    A0, _, aggs = sz.case("segments")
    agg = aggs[0]
    prow, pcol, ln, own = sz.segment_lengths(A0, agg)
    kA = int(np.diff(A0.indptr).max())
    assert kA == 10 and {1, 2, kA} <= set(ln.tolist()) and ln.min() >= 1
    k = int(np.flatnonzero(ln == kA)[0])
    assert prow[k] == sz.SEG_STAR and own[k]
    pl = np.diff(sz.bits("segments").P[0].indptr)
    first = {int(i) for i, o, p in zip(prow, own, np.arange(prow.size)) if o and pl[i] > 1 and p == sz.bits("segments").P[0].indptr[i]}
    last = {int(i) for i, o, p in zip(prow, own, np.arange(prow.size)) if o and pl[i] > 1 and p == sz.bits("segments").P[0].indptr[i + 1] - 1}
    assert 1 in first and 2 in last and (first - last) and (last - first)
    lone = np.flatnonzero((prow == sz.SEG_LONE) & own)
    assert lone.size == 1 and ln[lone[0]] == 1 and pl[sz.SEG_LONE] == 3   # its neighbours 8 and 10 lie in other aggregates
    assert pl.min() == 1


def test_search_case_has_every_hit_and_miss():
    """for A P and for R (A P): right-hand rows of 1, 2 and at least 1 025 entries, the wanted column their first, last and an
    interior entry, and absent below the first, above the last and between two entries — counted from the patterns"""
    B = sz.bits("search")
    P, AP = B.P[0], B.AP[0]
    assert np.diff(P.indptr).max() >= 1025 and np.diff(AP.indptr).max() >= 1025
    for tag, L, R, C in (("A P", B.A[0], P, AP), ("R (A P)", sz.transposed(P), AP, B.M[0])):
        cen = sz.search_census(L, R, C)
        print(tag, {f"{k[0]}:{k[1]}": v for k, v in cen.items() if v})
        missing = [k for k in sz.FEASIBLE if cen[k] == 0]
        assert not missing, (tag, missing)
        assert all(v == 0 for k, v in cen.items() if k not in sz.FEASIBLE)
    # the long right-hand rows of the arrows are searched too (hits only: the head touches every aggregate)
    Ba = sz.bits("arrow_2049")
    cen = sz.search_census(Ba.A[0], Ba.P[0], Ba.AP[0])
    assert cen[(2, "first")] and cen[(2, "last")] and cen[(2, "between")]


def test_coarsest_level_and_level_count():
    """one level with n = 1 and n = 65; two levels with a coarsest level of 1, 2, 16, 17, 64 and 65 rows: as_row_of with
    n = 1, k_as_sym_dense on one workgroup (256 = 16² entries exactly) and on two (17²), k_as_dense on one workgroup and (the
    129-row coarsest level of the Gershgorin cases, 385 entries) on two"""
    assert sz.bits("one_1").sizes == [1] and sz.bits("one_65").sizes == [65]
    dense, symd = set(), set()
    for name in ["one_1", "one_65", "gersh_0"] + [f"coarse_{k}" for k in sz.COARSE_NC]:
        B = sz.bits(name)
        if name.startswith("coarse"):
            assert B.sizes == [3 * int(name[7:]), int(name[7:])]
        dense.add(_blocks(B.A[-1].nnz)); symd.add(_blocks(B.sizes[-1] ** 2))
    assert {1, 2} <= dense and {1, 2} <= symd and 16 * 16 == NT
    assert sz.bits("gersh_0").A[-1].nnz == 385


def test_level_block_cases():
    """three levels with 255, 256 and 257 rows on level 1; the entry counts of P_0 (k_as_gather), A_0 P_0 and A_1 (k_as_product's
    grids, k_as_sym) lie on both sides of a multiple of 256 across the three"""
    counts = {"P": [], "AP": [], "A1": []}
    for k in sz.LEVEL_NC:
        B = sz.bits(f"level_{k}")
        assert B.sizes == [8 * k, k, (k + 7) // 8]
        counts["P"].append(B.P[0].nnz); counts["AP"].append(B.AP[0].nnz); counts["A1"].append(B.A[1].nnz)
    print(counts)
    for what, c in counts.items():
        m = (max(c) // NT) * NT
        assert min(c) < m < max(c) and m - min(c) < 32 and max(c) - m < 32, (what, c)
    assert {_blocks(k) for k in sz.LEVEL_NC} == {1, 2} and 256 in sz.LEVEL_NC


@pytest.mark.parametrize("levels", [2, 3])
def test_breakdown_case_fails_on_level_1_alone(levels):
    """the matrix of the failure test: a positive diagonal on level 0, finite values everywhere, entry (1, 1) of level 1 not
    positive in the restatement"""
    A0, bad, aggs = sz.breakdown(levels)
    assert np.array_equal(A0.indices, bad.indices) and (bad.diagonal() > 0).all() and (A0 != bad).nnz == 2
    assert abs(bad - bad.T).max() == 0.0
    B = sz.setup_bits(bad, aggs)
    assert B.nlevels == levels and all(np.isfinite(v).all() for v in B.values())
    d1 = B.A[1].diagonal()
    assert d1[1] < 0 and (np.delete(d1, 1) > 0).all()
    G = sz.setup_bits(A0, aggs)
    assert all((a.diagonal() > 0).all() for a in G.A)


# ------------------------------------------------------------------ bounds, the mesh route, values
@pytest.mark.parametrize("name", sz.NAMES)
def test_setup_bits_within_the_bounds_of_the_longdouble_chain(fem, name):
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    A0, A1, aggs = sz.case(name, fem)
    for w, A in enumerate((A0, A1)):
        B = sz.bits(name, w, fem=fem)
        assert np.array_equal(B.A[0].data, A.data)
        sz.check_ld(B, aggs, sz.setup_ld(A, aggs, B), f"{name} [{w}]")
        for a in B.A[1:]:
            assert abs(a - a.T).max() == 0.0


MESH = [(12, dict(max_levels=2, max_coarse=10)), (12, dict(max_levels=3, max_coarse=4)), (34, {})]


@pytest.mark.parametrize("N,kw", MESH)
def test_agreement_with_the_mesh_route(fem, N, kw):
    """on the mesh pairs setup_bits against fem.amg_refresh where the two orders coincide: on level 0 ω, g, ω/d and P are
    bit-equal (scipy sums a row of A and of A T in stored order too) and A_1 lies within its bound (the host multiplies
    (P' A) P); the levels below start from that A_1 and are held level by level, like a hierarchy read back"""
    A0, A1, _ = rr.pair(fem, N)
    aggs = fem.prepare_amg_precond(A0, **kw).agg
    assert len(aggs) == (kw.get("max_levels", 2) - 1)
    for A in (A0, A1):
        H, B = fem.amg_refresh(aggs, A), sz.setup_bits(A, aggs)
        assert B.sizes == H.sizes
        # level 0, where both routes start from the same A_0: bit-equal but for the product
        assert B.omega[0] == H.omega[0] and np.array_equal(B.wd[0], H.omega_over_d[0])
        assert B.g[0] == float(np.max(sz.ratios(B.A[0])))
        assert np.array_equal(B.P[0].data, H.P[0].data)
        for l in range(len(aggs)):
            for X, Y in ((B.P[l], H.P[l]), (B.A[l + 1], H.A[l + 1])):
                assert np.array_equal(X.indptr, Y.indptr) and np.array_equal(X.indices, Y.indices)
        Bd = rr.level_bounds(B.A[0], B.P[0], aggs[0])
        dA = np.abs(B.A[1].data - H.A[1].data)
        bA = rr.on_pattern(Bd["G_bound"], B.A[1])
        print(f"N = {N} {kw}: A_1 of setup_bits against fem.amg_refresh: {np.max(np.divide(dA, bA, out=np.zeros_like(dA), where=bA > 0)):.4f} of the bound")
        assert (dA <= bA).all()
        # deeper levels start from an A_l that differs by that rounding: level by level from the restatement's own A_l
        rr.check_levels(B, aggs, f"N = {N} {kw}")
        sz.check_ld(B, aggs, sz.setup_ld(A, aggs, B), f"N = {N} {kw}")


def test_values_are_normal_and_finite(fem):
    tiny = np.finfo(np.float64).tiny
    for name in sz.NAMES:
        for w in (0, 1):
            for v in sz.bits(name, w, fem=fem).values():
                assert np.isfinite(v).all() and np.all((v == 0.0) | (np.abs(v) >= tiny)), (name, w)
            B = sz.bits(name, w, fem=fem)
            for X in B.AP + B.M:
                assert np.isfinite(X.data).all() and np.all((X.data == 0.0) | (np.abs(X.data) >= tiny)), (name, w)
            assert all(0.0 < g < 4.0 for g in B.g)


# ------------------------------------------------------------------ defects
# (defect, case): the fault and a case that is there for it
SEEN_BY = (
    [("omega_tail", "big_65537_hi"), ("omega_tail", "big_76801_hi")] +
    [("gersh_wave", f"gersh_{r}") for r in (192, 255, 1023)] +
    [("gersh_last_block", "gersh_1024"), ("gersh_last_block", "big_65537_hi")] +
    [("seg_short", n) for n in ("segments", "arrow_seg", "search", "coarse_1")] +
    [(d, n) for d in ("search_last", "search_first") for n in ("search", "arrow_1024", "arrow_1025", "arrow_2049", "giant", "coarse_1", "level_256")] +
    [("sym_half", n) for n in ("search", "arrow_2049", "level_257", "big_65536")])
# (defect, case): a case without the edge: not one bit moves
UNSEEN_BY = (
    [("omega_tail", n) for n in ("big_65536", "big_65537_lo", "big_76801_lo", "gersh_1024", "search")] +
    [("gersh_wave", n) for n in ("segments", "coarse_16", "one_65")] +
    [("gersh_last_block", "big_65536")] +
    [(d, "one_65") for d in ("seg_short", "search_last", "search_first", "sym_half")] + [("sym_half", "coarse_1")])


@pytest.mark.parametrize("defect,name", SEEN_BY)
def test_every_edge_is_visible(fem, defect, name):
    seen = [not sz.same(sz.bits(name, w, fem=fem), sz.bits(name, w, defect, fem=fem)) for w in (0, 1)]
    assert all(seen), (defect, name, seen)
    if defect in ("omega_tail", "gersh_wave", "gersh_last_block"):       # a lost maximum moves ω in its leading digits
        a, b = sz.bits(name, 0, fem=fem).omega[0], sz.bits(name, 0, defect, fem=fem).omega[0]
        assert b >= a / 0.9


@pytest.mark.parametrize("defect,name", UNSEEN_BY)
def test_a_defect_leaves_other_cases_alone(fem, defect, name):
    for w in (0, 1):
        assert sz.same(sz.bits(name, w, fem=fem), sz.bits(name, w, defect, fem=fem)), (defect, name, w)


def test_defects_cover_the_list():
    assert {d for d, _ in SEEN_BY} == set(sz.DEFECTS) == {d for d, _ in UNSEEN_BY} and len(sz.DEFECTS) == 7
