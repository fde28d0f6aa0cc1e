"""CPU suite of the LORASC preconditioner: the host restatement of `apply_lorasc` (tests/lorasc_ref.py) against the block
formula, `fem.prepare_lorasc_precond` (the `:exact` branch of EPDD.jl:1541-1617), and the properties of the inputs that
tests/test_gpu_lorasc.py relies on — the checker's own noise, the n_Γ of the workgroup-edge partitions, the shapes of the
A_IΓd columns."""
import numpy as np
import pytest
import scipy.sparse as sp

import lorasc_ref as lr


@pytest.fixture(scope="module")
def cases(fem):
    return lr.gpu_cases(fem)


def test_restatement_equals_block_formula(cases):
    """dense M^-1 from the statement-by-statement apply == [I -A_II^-1 A_IΓ; 0 I] diag(A_II^-1, A_ΓΓ^-1 + E diag(coef) E')
    [I 0; -A_ΓI A_II^-1 I] on micro, without correction, as written (coef = 1) and with a coefficient vector"""
    c = cases["micro"]
    _, E, coef = lr.apply_inputs(c, 25, True)
    for Ek, ck in ((None, None), (E, None), (E, coef)):
        got, want = lr.dense_minv(c, Ek, ck), lr.block_formula_minv(c, Ek, ck)
        assert np.linalg.norm(got - want) <= 1e-11 * np.linalg.norm(want)
        assert np.linalg.norm(got - got.T) <= 1e-11 * np.linalg.norm(got)


def test_blocks_are_the_blocks_of_A(cases):
    """A in `not_dirichlet` order, cut by pos_I / pos_Γ, is [A_IId, A_IΓd; A_IΓd', A_ΓΓ]: the maps the operator is given"""
    for c in cases.values():
        perm = np.concatenate(list(c.pos_I) + [c.pos_Γ])
        assert np.array_equal(np.sort(perm), np.arange(c.n))
        Ap = c.A[perm][:, perm]
        B = sp.bmat([[sp.block_diag(c.A_IId), sp.vstack(c.A_IΓd)], [sp.vstack(c.A_IΓd).T, c.A_ΓΓ]])
        assert abs(Ap - B).max() <= 1e-13 * abs(B).max(), c.name


def test_checker_noise_is_100x_below_the_gpu_bar(cases):
    """on every input of the GPU suite the plain and the refined restatement differ by less than 1e-12 ||z||"""
    for c in cases.values():
        for nev, with_coef in lr.APPLY_VARIANTS:
            x, E, coef = lr.apply_inputs(c, nev, with_coef)
            plain, fine = lr.apply_lorasc(c, x, E, coef, refine=0), lr.apply_lorasc(c, x, E, coef, refine=2)
            assert np.linalg.norm(plain - fine) < 1e-12 * np.linalg.norm(fine), (c.name, nev, with_coef)


def test_edge_inputs_have_the_shapes_the_gpu_suite_needs(cases):
    """n_Γ mod 256 of the three edge partitions; Γ columns with one interior row; the hub of the unstructured mesh, where
    the slices meet, is a Γ column without any interior row; in the 1 x 2 strip every Γ column holds entries of both subdomains, and no interior row
    belongs to both (the row sets of the stacked A_IΓd are disjoint)"""
    assert cases["tail1"].n_Γ % 256 == 1 and cases["full"].n_Γ % 256 == 0 and cases["short1"].n_Γ % 256 == 255
    for name in ("micro", "ragged", "unstructured"):
        per = np.array([np.diff(sp.csc_matrix(a).indptr) for a in cases[name].A_IΓd])
        assert (per == 1).any(), name
    cnt = cases["unstructured"].P.sub.node_Γ_cnt                   # the hub: the pie slices meet there; all its neighbours
    per = np.array([np.diff(sp.csc_matrix(a).indptr) for a in cases["unstructured"].A_IΓd])   # are Γ nodes -> an empty column
    assert int(cnt.max()) >= 5 and per[:, int(np.argmax(cnt))].sum() == 0
    per = np.array([np.diff(sp.csc_matrix(a).indptr) for a in cases["strip"].A_IΓd])
    assert per.shape[0] == 2 and (per > 0).all()


def test_prepare_lorasc_precond_properties(fem, cases):
    """E' A_ΓΓ E = I and S E = A_ΓΓ E diag(σ) to 1e-10; the same pairs as the Cholesky-reduced reference"""
    c = cases["micro"]
    S, A = lr.dense_schur(c), c.A_ΓΓ.toarray()
    ε = 0.5
    E, Σ = fem.prepare_lorasc_precond(S, c.A_ΓΓ, nvec=25, ε=ε)
    Er, Σr = lr.prepare_lorasc_precond_ref(S, c.A_ΓΓ, nvec=25, ε=ε)
    nev = E.shape[1]
    assert 0 < nev < 25 and nev == Er.shape[1]
    σ = ε / (1.0 + Σ)                                    # Σ = (ε - σ)/σ
    assert np.abs(E.T @ A @ E - np.eye(nev)).max() <= 1e-10
    assert np.abs(S @ E - A @ E * σ).max() <= 1e-10 * np.abs(A @ E).max()
    assert np.allclose(Σ, Σr, rtol=1e-9)
    Ecall, Σcall = fem.prepare_lorasc_precond(lambda v: S @ v, c.A_ΓΓ, nvec=25, ε=ε)
    assert np.allclose(Σcall, Σ, rtol=1e-9) and Ecall.shape == E.shape


def test_prepare_lorasc_precond_selection_rule(fem):
    """a hand-made spectrum (A_ΓΓ = I, S = diag): nev in the middle, nev == nvec, and nev == 0 -> nev = nvec with Σ = σ"""
    n, ε = 12, 0.01
    A = np.eye(n)
    spec = np.array([0.002, 0.004, 0.008, 0.02, 0.05, 0.1, 0.3, 0.5, 0.7, 1.0, 1.5, 2.0])
    S = np.diag(spec[::-1].copy())                       # not sorted on the way in
    E, Σ = fem.prepare_lorasc_precond(S, A, nvec=5, ε=ε)
    assert E.shape == (n, 3) and np.allclose(Σ, (ε - spec[:3]) / spec[:3], rtol=1e-12)
    assert np.allclose(np.abs(E[::-1][:3]), np.eye(3), atol=1e-12)
    E, Σ = fem.prepare_lorasc_precond(S, A, nvec=2, ε=ε)                      # nev == nvec: kept (the reference warns)
    assert E.shape == (n, 2) and np.allclose(Σ, (ε - spec[:2]) / spec[:2], rtol=1e-12)
    E, Σ = fem.prepare_lorasc_precond(S, A, nvec=4, ε=1e-3)                   # nev == 0 -> nvec, Σ left as σ
    assert E.shape == (n, 4) and np.allclose(Σ, spec[:4], rtol=1e-12)
    E, Σ = fem.prepare_lorasc_precond(S, A, nvec=4, ε=0.0)                    # ε <= 0: no correction
    assert E.shape == (n, 0) and Σ.size == 0
    for nvec, eps in ((5, ε), (2, ε), (4, 1e-3)):
        Er, Σr = lr.prepare_lorasc_precond_ref(S, A, nvec=nvec, ε=eps)
        Ef, Σf = fem.prepare_lorasc_precond(S, A, nvec=nvec, ε=eps)
        assert Er.shape == Ef.shape and np.allclose(Σr, Σf, rtol=1e-12)
