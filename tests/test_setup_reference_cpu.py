"""CPU checks of tests/setup_synth.py: the synthetic set-up problems have the level structure they promise, the
long-double reference is right to the last bits of float64 (against mpmath), the host level elimination meets the κ bar
against it, and the numpy copy of the device's Gauss-Jordan inversion separates the algorithm's rounding from the
pivot-block mirroring that lost it (setup_gj.hpp, gj_invert_block64)."""
import numpy as np
import pytest
import scipy.sparse as sp

import setup_synth as ss


def test_reference_against_mpmath():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    s = ss.ladder([12, 9, 11, 8], degree=[1, 2, 5], density=0.2, n_gamma=7, gamma_deg=2, seed=5, contrast=1e3)
    assert s.A_II.shape[0] == 40
    ref = ss.reference(s)
    A = mp.matrix(s.A_II.toarray().tolist())
    B = mp.matrix(s.A_IΓ.toarray().tolist())
    G = mp.matrix(s.A_ΓΓ.toarray().tolist())
    Ai = mp.inverse(A)
    S = G - B.T * (Ai * B)
    w = B.T * (Ai * mp.matrix(s.b_I.tolist()))
    uf = Ai * mp.matrix(s.f.tolist())
    S64 = np.array([[float(S[i, j]) for j in range(S.cols)] for i in range(S.rows)])
    w64 = np.array([float(w[i, 0]) for i in range(w.rows)])
    u64 = np.array([float(uf[i, 0]) for i in range(uf.rows)])
    assert np.max(np.abs(ref.S - S64)) <= 2 * ss.EPS * np.max(np.abs(S64))
    assert np.max(np.abs(ref.w - w64)) <= 2 * ss.EPS * np.max(np.abs(w64))
    assert np.max(np.abs(ref.u - u64)) <= 2 * ss.EPS * np.max(np.abs(u64))


@pytest.mark.parametrize("widths,degree,density,n_gamma,gamma_deg,island", [
    ([65, 64, 1, 33, 128, 2], [1, 4, 5, 12], 0.05, 17, 3, 0),
    ([129, 63, 257], 4, 0.01, 300, 2, 0),
    ([6] * 12, 1, 0.0, 15, 1, 0),
    ([40], 1, 0.1, 1, 1, 0),
    ([33, 200, 129], 12, 0.02, 16, 4, 7),
])
def test_generator_levels(widths, degree, density, n_gamma, gamma_deg, island):
    s = ss.ladder(widths, degree=degree, density=density, n_gamma=n_gamma, gamma_deg=gamma_deg, seed=11, island=island)
    levels = ss.bfs_levels(s.A_II, s.A_IΓ)
    assert [len(l) for l in levels] == widths
    n = s.A_II.shape[0]
    assert n == sum(widths) + island
    for M in (s.A_II, s.A_IΓ, s.A_ΓΓ):            # CSC, canonical (no duplicates)
        assert isinstance(M, sp.csc_matrix) and M.has_canonical_format
    assert abs(s.A_II - s.A_II.T).max() == 0
    assert np.linalg.eigvalsh(s.A_II.toarray())[0] > 0
    # coupling degrees: columns of C_k (level k+1 rows per level-k node) and of B longer than the pick kernel's 4 registers
    A = sp.csr_matrix(s.A_II)
    if np.max(degree) > 4:
        deg = [A[levels[k + 1]][:, levels[k]].getnnz(axis=1).max() for k in range(len(levels) - 1)]
        assert max(deg) == np.max(degree)
    if n_gamma == 1:
        assert s.A_IΓ.getnnz(axis=0)[0] == widths[0]
    if island:
        assert sum(len(l) for l in levels) == n - island


def test_direct_inverse_family_is_what_it_says():
    s = ss.direct_inverse(65, 1e8)
    ref = ss.reference(s)
    assert ref.kappas == pytest.approx([1e8], rel=1e-6)
    Tinv = 2.0 * np.eye(65) - ref.S
    assert np.max(np.abs(s.A_II.toarray() @ Tinv - np.eye(65))) <= 1e-7        # κ eps ‖T‖ ‖T^-1‖ at most
    assert ref.S_scale == pytest.approx(np.max(np.abs(Tinv)))


@pytest.mark.parametrize("case", ["ladder", "direct"])
def test_host_level_elimination_meets_the_bar(pkg, case):
    fem = pkg.fem
    s = (ss.ladder([65, 64, 1, 33, 128, 2], degree=[1, 4, 5, 12], density=0.05, n_gamma=17, gamma_deg=3, seed=1, contrast=1e4)
         if case == "ladder" else ss.direct_inverse(129, 1e6))
    ref = ss.reference(s)
    S, w = fem.local_schur_by_level_elimination(s.A_II, s.A_IΓ, s.A_ΓΓ, s.b_I)
    S = np.asarray(S)
    r = np.max(np.abs(S - ref.S)) / ref.S_scale / (ref.kappa * ref.nmax * ss.EPS)
    rw = np.max(np.abs(np.asarray(w).ravel() - ref.w)) / np.max(np.abs(ref.w)) / (ref.kappa * ref.nmax * ss.EPS)
    print(f"host levels {case}: κ_max {ref.kappa:.3g}, S err/(κ n eps) {r:.3g}, w {rw:.3g}")
    assert r <= 50 and rw <= 50


@pytest.mark.parametrize("n", [65, 96, 129])
def test_gj_emulation_pivot_mirroring(n):
    """The device's blocked Gauss-Jordan (numpy copy) meets the κ bar at κ = 1e6; with the pivot inverses mirrored to
    symmetry (the kernels before this fix) it does not: the loss at κ = 1e6 - 1e8 came from that mirror, not the algorithm."""
    s = ss.direct_inverse(n, 1e6)
    ref = ss.reference(s)
    Tinv = 2.0 * np.eye(n) - ref.S
    scale = np.max(np.abs(Tinv)) * 1e6 * n * ss.EPS
    r_fix = np.max(np.abs(ss.gj_emulate(s.A_II.toarray()) - Tinv)) / scale
    r_old = np.max(np.abs(ss.gj_emulate(s.A_II.toarray(), mirror_pivots=True) - Tinv)) / scale
    print(f"emulated Gauss-Jordan n={n} κ=1e6: err/(κ n eps) {r_fix:.3g}, with mirrored pivots {r_old:.3g}")
    assert r_fix <= 1.0
    if n in (65, 96):
        assert r_old > 20.0
