"""CPU checks of the AMG `Pl` of the interior CG: the host side (`fem.prepare_interior_amg`) and the numpy restatement
(tests/interior_amg_ref.py) the GPU suite compares with (tests/test_gpu_interior_amg.py)."""
import numpy as np
import pytest
import scipy.sparse as sp

import interior_amg_ref as ir


def _canon(agg):
    """aggregate ids renumbered by first occurrence: equal arrays <=> equal partitions"""
    _, first, inv = np.unique(agg, return_index=True, return_inverse=True)
    rank = np.empty(first.size, dtype=np.int64)
    rank[np.argsort(first)] = np.arange(first.size)
    return rank[inv]


@pytest.mark.parametrize("name", ["ragged", "n12_3", "empty"])
def test_stacked_aggregation_is_the_blocks_own(fem, name):
    """`amg_aggregate` looks at neighbours only: on blockdiag(A_IIdd) every block gets the aggregates it gets alone, no
    aggregate holds nodes of two blocks, and prepare_interior_amg returns the sizes and aggregates of prepare_amg_precond on
    the stacked matrix."""
    C = ir.case(fem, name)
    sizes, aggs = fem.prepare_interior_amg(C.A_II, **C.kw)
    H = C.hierarchy(fem)
    assert sizes == list(H.sizes) and len(aggs) == len(H.agg) and all(np.array_equal(a, b) for a, b in zip(aggs, H.agg))
    assert sizes[0] == sum(A.shape[0] for A in C.A_II) and len(sizes) >= 2
    _, offs = C.stacked()
    seen = np.zeros(sizes[1], dtype=bool)
    for d, A in enumerate(C.A_II):
        own = aggs[0][offs[d]:offs[d + 1]]
        if own.size == 0:
            continue
        A = sp.csr_matrix(A); A.sort_indices()
        assert np.array_equal(_canon(own), _canon(fem.amg_aggregate(A))), (name, d)
        ids = np.unique(own)
        assert not seen[ids].any(), (name, d, "an aggregate of an earlier block")
        seen[ids] = True
    assert seen.all()


def test_restated_s_apply_on_ragged_and_fewer_iterations_than_diagonal(fem):
    """The restated matrix-free S-apply with the AMG `Pl` stays within 1e-7 max|Sx| of the exact one (the bar of
    test_gpu_parity.py for this solve; here: 4e-11), every subdomain's solve meets 2 reltol ‖b‖_d in the true residual
    (the cap check 2 of the GPU suite uses), and every subdomain needs fewer iterations than with the diagonal `Pl`."""
    C = ir.case(fem, "ragged")
    x = C.x()
    v, its, hist, tol = C.solve(fem, x)
    exact = C.exact_apply(x)
    err = np.abs(C.s_apply(x, v) - exact).max() / np.abs(exact).max()
    _, its_d, _, _ = C.solve(fem, x, pl="diagonal")
    print(f"ragged: S-apply error {err:.2e} of max|Sx|; iterations AMG {its.tolist()}, diagonal {its_d.tolist()}")
    assert err <= 1e-7
    assert (its < its_d).all() and its.max() <= 15
    A, offs = C.stacked()
    rhs = C.interior_rhs(x)
    r = rhs - A @ v
    for d in range(offs.size - 1):
        s = slice(offs[d], offs[d + 1])
        assert np.linalg.norm(r[s]) <= 2.0 * ir.RELTOL * np.linalg.norm(rhs[s]), d


@pytest.mark.parametrize("second", [False, True], ids=["first", "after_set_values"])
@pytest.mark.parametrize("name", ir.NAMES + ir.EDGE_NAMES)
def test_counts_are_not_marginal(fem, name, second):
    """Every case the GPU suites use for an iteration-count equality (tests/test_gpu_interior_amg.py; the edge cases of
    tests/test_gpu_amg_edges.py): in the restatement each subdomain stops with
    ‖r‖ <= 0.95 tol, after a step that left ‖r‖ >= 1.05 tol. The true residual meets the cap 2 reltol ‖b‖_d."""
    C = ir.case(fem, name)
    x = C.x(second)
    v, its, hist, tol = C.solve(fem, x, second)
    m = ir.margins(hist, tol)
    print(f"{name} second={second}: sizes {C.hierarchy(fem, second).sizes}, iterations {its.tolist()}, "
          f"(stop, before) / tol {[(round(a, 3), round(b, 3)) for a, b in m]}")
    assert len(m) == sum(A.shape[0] > 0 for A in C.A_II)
    for a, b in m:
        assert a <= 0.95 and b >= 1.05, (name, second, a, b)
    A, offs = C.stacked(second)
    rhs = C.interior_rhs(x, second)
    r = rhs - A @ v
    for d in range(offs.size - 1):
        s = slice(offs[d], offs[d + 1])
        assert np.linalg.norm(r[s]) <= 2.0 * ir.RELTOL * np.linalg.norm(rhs[s]), (name, d)
    exact = C.exact_apply(x, second)
    assert np.abs(C.s_apply(x, v, second) - exact).max() <= 1e-7 * np.abs(exact).max()
    if not second:      # the right-hand side of the GPU suite's interior_solutions(0, b_I): the same cap
        bI = C.b_I()
        vb = ir.pcg_domains(A, offs, bI, ir.amg_pl(C.hierarchy(fem)))[0]
        rb = bI - A @ vb
        for d in range(offs.size - 1):
            s = slice(offs[d], offs[d + 1])
            assert np.linalg.norm(rb[s]) <= 2.0 * ir.RELTOL * np.linalg.norm(bI[s]), (name, d)
        if name in ir.EDGE_NAMES:   # ... and on the edge cases its iteration count is compared too: the same margins
            _, its_b, hist_b, tol_b = C.solve_b(fem)
            mb = ir.margins(hist_b, tol_b)
            print(f"{name} interior_solutions(0, b_I): iterations {its_b.tolist()}, (stop, before) / tol "
                  f"{[(float(f'{a:.3g}'), float(f'{b:.3g}')) for a, b in mb]}")
            assert len(mb) == sum(A.shape[0] > 0 for A in C.A_II)
            for a, b in mb:
                assert a <= 0.95 and b >= 1.05, (name, a, b)


def test_level_counts_of_the_cases(fem):
    """the cases take the paths they are there for: three levels with interiors below a row block, the dense inverse alone,
    a subdomain boundary beside a row-block boundary, an empty interior"""
    sz = {n: ir.case(fem, n).hierarchy(fem).sizes for n in ir.NAMES}
    assert sz["ragged"] == [2162, 400, 50] and sz["n12_3"] == [81, 19, 4] and sz["n12_1"] == [81]
    assert len(sz["blocks2"]) == 2 and sz["blocks2"][0] == 2048 and len(sz["empty"]) == 3
    assert [A.shape[0] for A in ir.case(fem, "blocks2").A_II] == [1023, 1025]
    assert [A.shape[0] for A in ir.case(fem, "empty").A_II] == [300, 0, 500]


def test_prepare_interior_amg_refusals(fem):
    C = ir.case(fem, "n12_3")
    with pytest.raises(ValueError, match="non-empty"):
        fem.prepare_interior_amg([])
    with pytest.raises(ValueError, match="non-empty"):
        fem.prepare_interior_amg([sp.csr_matrix((0, 0))])
    with pytest.raises(ValueError, match="max_levels"):
        fem.prepare_interior_amg(C.A_II, max_levels=0)
    neg = [sp.csr_matrix(A).copy() for A in C.A_II]
    neg[1] = neg[1] - 2.0 * sp.diags(neg[1].diagonal())
    with pytest.raises(ValueError, match="diagonal"):
        fem.prepare_interior_amg(neg, max_coarse=16)
    with pytest.raises(ValueError, match="stalled"):
        fem.prepare_interior_amg([sp.identity(40, format="csr"), sp.identity(30, format="csr")], max_coarse=8)
    big = ir.case(fem, "blocks2")
    with pytest.raises(ValueError, match="4096"):
        fem.prepare_interior_amg(big.A_II + big.A_II + big.A_II, max_levels=1)
    bad = [sp.csr_matrix(A).copy() for A in C.A_II]
    bad[0].data[0] = np.nan
    with pytest.raises(ValueError, match="finite"):
        fem.prepare_interior_amg(bad)
