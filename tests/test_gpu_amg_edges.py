"""GPU suite (-m gpu) of the AMG cycle kernels (csrc/amg.hpp: k_amg_down / _restrict / _prolong / _post / _post_dot,
k_amg_coarse / _coarse_dom) at the edges of their row-block partition and of the coarse GEMV, bit for bit against
`amg_synth.cycle_bits`, the cycle restated on the host in the device's order of operations. The hierarchies, their variants
("pzp": restrict, coarse, prolong alone; "smooth": down and post alone) and their right-hand sides are those of
tests/amg_synth.py; tests/test_amg_edges_cpu.py asserts on the host that each has the block shape it is named for and that
the fault each case is there for changes at least one bit of the restatement.

Bars:
  * cycle: `M.ldiv(r)` equals `cycle_bits(H, r)` under np.array_equal, for every hierarchy, variant and right-hand side; a
    second apply, an apply on a torch tensor and an operator created from 1-based arrays give the same bits. A mismatch
    prints the first differing indices with their row blocks and the error in units of amg_synth.bound.
  * plan route (`device_setup=True, aggregates=`): the levels read back within tests/amg_refresh_ref.level_bounds, at create
    and after set_values(D A D); the apply equals cycle_bits of the hierarchy read back.
  * interior `Pl` on edge blocks: the bars of tests/test_gpu_interior_amg.py (S-apply within 1e-7 max|Sx| of the exact one,
    true residual within 2 reltol ‖b‖_d, iteration count equal to the restatement's, repeated applies and chunk sizes equal
    bit for bit), and for interior_solutions(0, b_I), the solve with data in every row of every block: its count equal to
    the restatement's and its solution within interior_amg_ref.solution_bars of the restated one, per subdomain.
    tests/test_interior_amg_cpu.py::test_counts_are_not_marginal covers the counts of both cases and both solves.

Measured on an MI355X (printed by the tests before they assert):
  * cycle: every case bit-identical — all 33 hierarchies of amg_synth.NAMES in every variant (332 applies), each also on the
    second apply, through a device pointer and from 1-based arrays; N = 40 lognormal and the N = 12 three-level mesh
    hierarchy bit-identical too. No stage fell back to the bound: the device cycle IS the host order of amg_synth.cycle_bits,
    long-row path, unpaired path, empty rows and blocks, GEMV lane and row tails included. No kernel was changed.
  * plan route, fraction of the level bounds used, at create | after set_values: ω, g, ω/d relative error at most 2.3e-15
    (bars 6.7e-16 .. 4.6e-13; exactly 0 on diag1025); P: arrow2100_2049 0.002 | 0.003, odd_start 0.010 | 0.007, diag1025 0 | 0,
    one_aggregate 0 | 0.074; A_1: below 0.001 everywhere; coarse inverse ||I - Z A||_F 2.1 .. 2.8 times numpy's (bar 8);
    32 applies bit-identical to cycle_bits of the hierarchy read back.
  * interior `Pl`: edge_long 3 iterations = the restatement's [3, 1, 2] (stopping residuals 9.5e-11 / 0 / 1.9e-9 of tol, the
    ones before 2.9e4 / 1e9 / 1.1e7), edge_rows 6 = [6, 0, 6] (0.548 of tol after 18.8), the same counts after set_values;
    S-apply error at most 1.2e-16 of max|Sx| (bar 1e-7); true residuals 2.2e-16 / 0 / 9.5e-17 and 7.3e-10 / 0 / 7.5e-10 of
    ‖b‖_d (bar 2e-9); every repeated apply, both chunk settings of the interior CG and set_chunk(0) bit-identical.
    interior_solutions(0, b_I): edge_long 4 iterations = the restatement's [4, 1, 2], edge_rows 6 = [6, 0, 6]; solution against
    the restated one, per subdomain: 1.3e-16 / 0 / 7.1e-17 (bars 3.6e-11 / 2.7e-12 / 2.1e-11) and 1.8e-16 / 0 / 1.9e-16 (bars
    5.6e-13 / 1.9e-14 / 5.6e-13); the seeded faults of the CPU suite that keep the count move it by 4.7e-11 at the least.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import amg_ref as ar
import amg_synth as az
import interior_amg_ref as ir
import sparse_synth as ss
from amg_refresh_ref import check_coarse as _check_coarse, check_levels as _check_levels
from interior_amg_ref import close as _close, new_values as _new_values, op as _op, residuals as _residuals

pytestmark = pytest.mark.gpu


def _report(tag, H, r, got, want):
    """a mismatch: the first differing indices, their row blocks in A_0, and the error against the derived bound"""
    bad = np.flatnonzero(got != want)
    blk = az.row_blocks(az.sorted_csr(H.A[0]).indptr)
    b = az.block_of_rows(blk, bad[:8])
    d = np.abs(got - az.cycle_ld(H, r)).astype(np.float64)
    bd = az.bound(H, r)
    ratio = float(np.max(np.divide(d, bd, out=np.zeros_like(d), where=bd > 0)))
    print(f"{tag}: {bad.size} of {got.size} entries differ; first {bad[:8].tolist()} in row blocks {b.tolist()} "
          f"{[tuple(blk[k]) for k in np.unique(b)]}; got {got[bad[:4]].tolist()} want {want[bad[:4]].tolist()}; "
          f"|got - cycle_ld| / bound = {ratio:.3f}, outside the bound: {int((d > bd).sum())}")


def _check_bits(pkg, ctx, H, tag, rhs, one_based=True):
    """the four statements of the bar for one hierarchy; returns the number of applies compared"""
    import torch
    api = pkg.api
    M = api.AMGPreconditioner(ctx, H)
    M1 = api.AMGPreconditioner(ctx, H, index_base=1) if one_based else None
    ok, count = True, 0
    try:
        assert M.n == H.sizes[0]
        for k, r in enumerate(rhs):
            want = az.cycle_bits(H, r)
            got = M.ldiv(r)
            count += 1
            if not np.array_equal(got, want):
                _report(f"{tag} rhs {k}", H, r, got, want)
                ok = False
                continue
            assert np.isfinite(got).all()
            assert np.array_equal(M.ldiv(r), got), (tag, k, "second apply")
            t = M.ldiv(torch.from_numpy(r).to("cuda"))
            assert np.array_equal(t.cpu().numpy(), got), (tag, k, "device pointer")
            if M1 is not None:
                assert np.array_equal(M1.ldiv(r), got), (tag, k, "1-based arrays")
    finally:
        M.close()
        if M1 is not None:
            M1.close()
    assert ok, f"{tag}: the device cycle is not the host order bit for bit (see the lines printed above)"
    return count


@pytest.mark.parametrize("name", az.NAMES)
def test_cycle_bit_for_bit(pkg, ctx, fem, name):
    n = 0
    for v in az.variants(fem, name):
        H = az.hierarchy(fem, name, v)
        n += _check_bits(pkg, ctx, H, f"{name} ({v})", az.rhs(name, H.sizes[0]))
    print(f"{name} {az.hierarchy(fem, name).sizes}: {n} applies bit-identical to cycle_bits (and second, device-pointer, 1-based)")


def test_holes_rows_are_written_exactly(pkg, ctx, fem):
    """the rows of `holes` without entries: with Z = 0 the cycle leaves y = ω/d b + ω/d (b - 0) there, whatever the buffers
    held before (an apply to another vector in between)"""
    H = az.hierarchy(fem, "holes", "smooth")
    n = H.sizes[0]
    empty = np.diff(H.A[0].indptr) == 0
    assert empty.sum() > ss.HOLES_INNER
    wd = H.omega_over_d[0]
    M = pkg.api.AMGPreconditioner(ctx, H)
    try:
        r, other = az.rhs("holes", n)[0], az.rhs("lead_long", n)[0]
        M.ldiv(other)
        got = M.apply(r, out=np.full(n, np.nan))
        x = wd * r
        assert np.array_equal(got[empty], (x + wd * (r - 0.0))[empty]) and not np.isnan(got).any()
    finally:
        M.close()


def test_mesh_hierarchies_bit_for_bit(pkg, ctx, fem):
    """the hierarchies tests/test_gpu_amg.py holds to 1e-12: N = 40 lognormal and the N = 12 three-level one"""
    A12 = ar.system(fem, 12, "example01")[0]
    for tag, H in (("N40 lognormal", ar.case(fem, 40, "lognormal")[2]),
                   ("N12 three levels", fem.prepare_amg_precond(A12, max_levels=3, max_coarse=4))):
        n = _check_bits(pkg, ctx, H, tag, az.rhs(tag, H.sizes[0]))
        print(f"{tag} {H.sizes}: {n} applies bit-identical")


def _dad(A):
    n = A.shape[0]
    D = sp.diags(1.0 + 0.3 * np.sin(np.arange(n) / 17.0))
    return az.sorted_csr(D @ sp.csr_matrix(A) @ D)


PLAN_CASES = {"arrow2100_2049": lambda: (ss.arrow(2100, 2049), az.groups(2100, 2)),
              "odd_start": lambda: (ss.odd_start(), az.groups(1300, 2)),
              "diag1025": lambda: (ss.diag(1025), az.groups(1025, 2)),
              "one_aggregate": lambda: (ss.tridiag(1500), np.zeros(1500, dtype=np.int64))}


@pytest.mark.parametrize("case", list(PLAN_CASES))
def test_plan_route_on_the_edge_patterns(pkg, ctx, fem, case):
    """the device set-up on frozen hand-made aggregates (pairs of consecutive rows; `one_aggregate`: every node in one, a
    coarsest level of one row and an R row of 1500 entries): level bounds at create and after set_values, the apply bit for
    bit the restatement on the hierarchy read back"""
    A, agg = PLAN_CASES[case]()
    A = az.sorted_csr(A)
    n = A.shape[0]
    M = pkg.api.AMGPreconditioner(ctx, A, device_setup=True, aggregates=[agg])
    try:
        for tag, V in ((f"{case} (create)", A), (f"{case} (set_values)", _dad(A))):
            if V is not A:
                M.set_values(V)
            H = M.device_hierarchy()
            assert H.sizes == [n, int(agg.max()) + 1] and np.array_equal(H.A[0].data, V.data)
            if case == "arrow2100_2049":
                assert np.diff(H.A[0].indptr)[0] == 2049 and np.diff(H.P[0].indptr)[0] > az.TILE
                assert np.diff(az.transposed(H.P[0]).indptr)[0] == 2049
            _check_levels(H, [agg], tag)
            with np.errstate(invalid="ignore"):              # n_c = 1: both residuals are exactly zero, the printed ratio 0 / 0
                _check_coarse(H, tag)
            rhs = az.rhs("arrow_2049" if case.startswith("arrow") else case if case in az.NAMES else "tridiag3000", n)
            for k, r in enumerate(rhs):
                got, want = M.ldiv(r), az.cycle_bits(H, r)
                if not np.array_equal(got, want):
                    _report(f"{tag} rhs {k}", H, r, got, want)
                assert np.array_equal(got, want), (tag, k)
                assert np.array_equal(M.ldiv(r), got)
            print(f"{tag}: levels {H.sizes}, {len(rhs)} applies bit-identical to cycle_bits of the hierarchy read back")
    finally:
        M.close()


@pytest.mark.parametrize("name", ir.EDGE_NAMES)
def test_interior_pl_on_edge_blocks(pkg, ctx, fem, monkeypatch, name):
    """`Pl` = AMG of the interior CG with row blocks cut at subdomain boundaries (k_amg_post_dot's per-block partials of r'z,
    k_amg_coarse_dom) on edge_long — a row longer than the tile alone in its block, a subdomain of one row, 1023 rows in one
    block at an odd offset and two rows after it — and edge_rows — 1023 rows, an empty interior, 1025 rows, blocks of two
    and five rows before the boundaries; aggregates in pairs within each subdomain. The S-applies have right-hand sides
    that are multiples of e_0 per subdomain; interior_solutions(0, b_I) with its random b_I has data in every row, and
    tests/test_amg_edges_cpu.py shows that leaving out the partial of any one block, or a row pass, moves its largest count
    or its solution beyond interior_amg_ref.solution_bars."""
    api = pkg.api
    C = ir.case(fem, name)
    H = C.hierarchy(fem)
    sizes, aggs = ir.pair_aggregates(C.A_II)
    assert sizes == list(H.sizes)
    x = C.x()
    _, its, hist, tol = C.solve(fem, x)
    exact = C.exact_apply(x)
    monkeypatch.setenv("MI355_ICG_CHUNK", "1")
    S1 = _op(api, ctx, C)
    monkeypatch.delenv("MI355_ICG_CHUNK")
    Sdef = _op(api, ctx, C)
    try:
        st = S1.interior_amg(sizes=sizes, aggregates=aggs)
        assert st["levels"] == 2 and st["coarse_n"] == sizes[1]
        it0 = S1.interior_iterations()
        y1 = S1 * x
        got = S1.interior_iterations() - it0
        e = _close(y1, exact)
        print(f"{name}: levels {H.sizes}, iterations device {got}, restatement {its.tolist()}, margins (stop, before) / tol "
              f"{[(float(f'{a:.3g}'), float(f'{b:.3g}')) for a, b in ir.margins(hist, tol)]}; S-apply error {e:.2e} of max|Sx|")
        assert got == int(its.max())
        assert e <= 1e-7
        assert np.array_equal(S1 * x, y1)
        Sdef.interior_amg(sizes=sizes, aggregates=aggs)
        yd = Sdef * x
        assert np.array_equal(yd, y1) and np.array_equal(Sdef * x, yd)
        try:
            ctx.set_chunk(0)
            y0 = Sdef * x
        finally:
            ctx.set_chunk(8)
        assert np.array_equal(y0, y1) and np.array_equal(Sdef * x, y1)
        # interior_solutions(0, b_I), random b_I: data in every row of every block, so every partial of r'z counts
        bI = C.b_I()
        vb, its_b, hist_b, tol_b = C.solve_b(fem)
        it0 = S1.interior_iterations()
        u = S1.interior_solutions(np.zeros(C.n_Γ), bI)
        got_b = S1.interior_iterations() - it0
        print(f"{name}: interior_solutions(0, b_I): iterations device {got_b}, restatement {its_b.tolist()}")
        assert got_b == int(its_b.max())
        assert np.array_equal(Sdef.interior_solutions(np.zeros(C.n_Γ), bI), u) and np.array_equal(S1.interior_solutions(np.zeros(C.n_Γ), bI), u)
        _, offs = C.stacked()
        bars = ir.solution_bars(C, fem, its_b)
        for d, (rn, bn) in enumerate(_residuals(C, u, bI)):
            s = slice(int(offs[d]), int(offs[d + 1]))
            dev = np.linalg.norm(u[s] - vb[s]) / np.linalg.norm(vb[s]) if s.stop > s.start else 0.0
            print(f"{name}: subdomain {d}: ‖b - A u‖ / ‖b‖ = {rn / bn if bn else 0.0:.2e}; ‖u - u_restated‖ / ‖u_restated‖ = {dev:.2e} "
                  f"(bar {bars[d]:.2e})")
            assert rn <= 2.0 * ir.RELTOL * bn, d
            assert dev <= bars[d], d
        x2 = C.x(True)
        _, its2, _, _ = C.solve(fem, x2, second=True)
        S1.set_values(*_new_values(C))
        it0 = S1.interior_iterations()
        y2 = S1 * x2
        got2 = S1.interior_iterations() - it0
        e2 = _close(y2, C.exact_apply(x2, second=True))
        print(f"{name}: after set_values: iterations device {got2}, restatement {its2.tolist()}; S-apply error {e2:.2e}")
        assert got2 == int(its2.max())
        assert e2 <= 1e-7
        assert np.array_equal(S1 * x2, y2)
    finally:
        S1.close(); Sdef.close()
