"""Host checks of the smoothed-aggregation set-up (`fem.prepare_amg_precond`) and of the V-cycle's numpy restatement
(tests/amg_ref.py), so that the GPU tests of tests/test_gpu_amg.py compare against a checked reference: the Galerkin
product, symmetry and definiteness of every level, symmetry of the cycle, the exact one-level form, the refusals, and the
iteration counts of `pcg(A, b, 0, Π_amg)` under their caps."""
import numpy as np
import pytest
import scipy.sparse as sp

import amg_ref as ar


@pytest.mark.parametrize("N,coeff", [(40, "example01"), (40, "lognormal"), (100, "example01")])
def test_levels_galerkin_symmetric_definite(fem, N, coeff):
    A, b, H, _ = ar.case(fem, N, coeff)
    assert H.nlevels >= 2 and H.sizes[0] == A.shape[0] and H.sizes[-1] <= 256
    assert len(H.P) == len(H.omega) == len(H.omega_over_d) == H.nlevels - 1
    assert np.isclose(H.operator_complexity, sum(a.nnz for a in H.A) / A.nnz, rtol=1e-15)
    assert H.operator_complexity < 1.5
    for l in range(H.nlevels - 1):
        Al, P = H.A[l], H.P[l]
        assert P.shape == (H.sizes[l], H.sizes[l + 1])
        G = (P.T @ Al @ P).toarray()
        err = np.linalg.norm(G - H.A[l + 1].toarray()) / np.linalg.norm(G)
        print(f"N = {N} {coeff} level {l}: |P'AP - A_next| / |P'AP| = {err:.2e}")
        assert err <= 1e-13
        d = Al.diagonal()
        g = np.max(np.asarray(abs(Al).sum(axis=1)).ravel() / d)
        assert H.omega[l] == 4.0 / (3.0 * g) and np.array_equal(H.omega_over_d[l], H.omega[l] / d)
    for l, Al in enumerate(H.A):
        assert abs(Al - Al.T).max() == 0.0 if l else abs(Al - Al.T).max() <= 1e-15 * abs(Al).max()
        if Al.shape[0] <= 2000:
            assert np.linalg.eigvalsh(Al.toarray())[0] > 0, l
    Ac = H.A[-1].toarray()
    assert np.array_equal(H.coarse_inv, H.coarse_inv.T)
    assert np.linalg.norm(H.coarse_inv @ Ac - np.eye(Ac.shape[0])) <= 1e-9 * np.linalg.cond(Ac)


def test_aggregation_passes(fem):
    """by hand on paths: node 0 seeds {0, 1}; node 2 has an aggregated neighbour and waits; node 3 seeds {3, 2, 4}; on 6 nodes
    node 5 is left over and joins its neighbour 4's aggregate in pass 2, on 7 nodes node 6 seeds {6, 5}. An isolated node
    has no neighbour that is taken: it is a seed of its own. A star: the first leaf takes the hub, the others join it."""
    path = lambda n: sp.diags([-np.ones(n - 1), 2 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csr")
    assert fem.amg_aggregate(path(6)).tolist() == [0, 0, 1, 1, 1, 1]
    assert fem.amg_aggregate(path(7)).tolist() == [0, 0, 1, 1, 1, 2, 2]
    assert fem.amg_aggregate(sp.block_diag([path(6), sp.identity(1)], format="csr")).tolist() == [0, 0, 1, 1, 1, 1, 2]
    star = sp.csr_matrix(np.array([[4, 0, 0, -1.0], [0, 4, 0, -1], [0, 0, 4, -1], [-1, -1, -1, 4]]))
    assert fem.amg_aggregate(star).tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("N,coeff", [(40, "example01"), (100, "lognormal")])
def test_cycle_is_symmetric(fem, N, coeff):
    _, b, H, _ = ar.case(fem, N, coeff)
    rng = np.random.default_rng(2)
    for _ in range(3):
        u, v = rng.standard_normal((2, b.size))
        uMv, vMu = u @ ar.cycle(H, v), v @ ar.cycle(H, u)
        print(f"N = {N} {coeff}: |u'Mv - v'Mu| / |u'Mv| = {abs(uMv - vMu) / abs(uMv):.2e}")
        assert abs(uMv - vMu) <= 1e-12 * abs(uMv)
        assert u @ ar.cycle(H, u) > 0


def test_one_level_is_the_exact_solve(fem):
    A, b = ar.system(fem, 20, "example01")
    H = fem.prepare_amg_precond(A, max_levels=1)
    assert H.nlevels == 1 and H.P == [] and H.sizes == [A.shape[0]] and H.operator_complexity == 1.0
    x = ar.cycle(H, b)
    assert np.linalg.norm(A @ x - b) <= 1e-12 * np.linalg.norm(b)
    want = np.linalg.solve(A.toarray(), b)
    assert np.linalg.norm(x - want) <= 1e-12 * np.linalg.norm(want)
    H2 = fem.prepare_amg_precond(A, max_levels=2, max_coarse=64)
    H3 = fem.prepare_amg_precond(A, max_levels=3, max_coarse=8)
    assert (H2.nlevels, H3.nlevels) == (2, 3)


def test_stall_and_size_refusals(fem):
    D = sp.identity(300, format="csr") * 2.0                       # no off-diagonal entry: every node its own aggregate
    with pytest.raises(ValueError, match="stalled"):
        fem.prepare_amg_precond(D)
    A, _ = ar.system(fem, 80, "example01")                         # 6 084 rows
    with pytest.raises(ValueError, match="4096"):
        fem.prepare_amg_precond(A, max_levels=1)
    with pytest.raises(ValueError, match="max_levels"):
        fem.prepare_amg_precond(A, max_levels=0)
    bad = A.copy(); bad.data[3] = np.nan
    with pytest.raises(ValueError, match="finite"):
        fem.prepare_amg_precond(bad)
    assert fem.prepare_amg_precond(A).nlevels == 3                 # and the same matrix is accepted with the defaults


@pytest.mark.parametrize("N,coeff,cap", ar.LOOP_CASES)
def test_iteration_counts(fem, N, coeff, cap):
    """`it` of the restatement under its caps (the prototype's counts plus two: a correct variant of the aggregation may differ
    by an aggregate), and the last two residuals at least 5 % away from the stop threshold, so that the device's rounding
    cannot move `it`. Jacobi's count on the same system is printed beside it."""
    A, b, H, (x, it, res) = ar.case(fem, N, coeff)
    tol = 1e-7 * np.linalg.norm(b)
    print(f"N = {N} {coeff}: levels {H.sizes}, complexity {H.operator_complexity:.3f}, it = {it} (cap {cap}), "
          f"res[it]/tol = {res[it - 1] / tol:.3f}, res[it-1]/tol = {res[it - 2] / tol:.3f}")
    assert it <= cap and len(res) == it
    assert res[it - 1] <= 0.95 * tol and res[it - 2] >= 1.05 * tol
    assert np.linalg.norm(A @ x - b) <= 2e-7 * np.linalg.norm(b)
    dinv = 1.0 / A.diagonal()
    itj = ar.pcg(A, b, np.zeros(b.size), lambda r: dinv * r)[1]
    print(f"  Jacobi-PCG on the same system: it = {itj}")
    assert 4 * it <= itj


def test_synthetic_hierarchies_are_well_formed(fem):
    """the hand-made hierarchies of the GPU edge tests: SPD levels, a symmetric cycle, the shapes they are there for"""
    for n in (1023, 1024, 1025):
        A = ar.grid_like(n)
        assert A.shape == (n, n) and abs(A - A.T).max() == 0 and np.linalg.eigvalsh(A.toarray())[0] > 0
    H = ar.giant_aggregate_hierarchy(fem)
    R = sp.csr_matrix(H.P[0].T)
    assert np.diff(R.indptr).max() > 1024 and np.diff(H.P[0].indptr).min() == 1
    u, v = np.random.default_rng(0).standard_normal((2, H.sizes[0]))
    a, b = u @ ar.cycle(H, v), v @ ar.cycle(H, u)
    assert abs(a - b) <= 1e-12 * abs(a) and u @ ar.cycle(H, u) > 0
