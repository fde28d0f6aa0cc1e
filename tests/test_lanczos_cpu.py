"""CPU suite: the numpy restatement of the device eigensolver (tests/lanczos_ref.py) meets, against dense `eigh`, the bars that
tests/test_gpu_lanczos.py holds `mi_eigsolve` to, on every case of tests/lanczos_synth.py; the table's records (restarts,
orthonormality defect, gap) are the restatement's; every gap is wide enough for a subspace comparison. Also: the
`fem.prepare_lorasc_precond(eigs=...)` hook against the default path on `micro`, and the binding of the new prototype.

Bars (tol = 1e-10, absolute):
  values        |θ_i - λ_i| <= 10 tol: for a (B-)unit Ritz vector an eigenvalue lies within the residual norm; 10 for the
                rounding in the estimate
  residual      ||A x_i - θ_i B x_i|| (B^-1 norm) <= 10 tol
  orthonormality  max |X' B X - I| <= 2e-13 for the restatement itself (it attains 4e-16 .. 1.4e-13, the latter after the 1570
                restarts of synth4097; the table's O_ref); the device is held to max(100 O_ref, 1e-13)
  subspace      sin of the largest principal angle to the eigh subspace <= 10 tol / gap (Davis-Kahan)
The restart count is sensitive to the summation order of the BLAS underneath numpy in its last digit or two: the record is
checked to +-25 % (+-2), which the device's maxiter = 4 R_ref + 8 absorbs."""
import ctypes as C
import re

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import lanczos_ref as lz
import lanczos_synth as syn
from conftest import ROOT

TOL = syn.TOL


def _solve_case(c, dense, B, Binv, v0):
    A = dense
    return lz.eigsolve(lambda x: A @ x, A.shape[0], c.nev, c.which, c.krylovdim, TOL, c.maxiter, v0,
                       None if B is None else (lambda x: B @ x), Binv)


def check_against_eigh(c, r, Ad, Bd, o_bar):
    """the four bars; returns the measured figures"""
    lam, X = lz.dense_eigh(Ad, Bd)
    lw, Xw, gap = lz.wanted(lam, X, c.nev, c.which)
    verr = float(np.max(np.abs(r.vals - lw)))
    res = float(np.max(lz.true_residuals(Ad, Bd, r.vals, r.vecs)))
    O = lz.ortho_defect(r.vecs, Bd)
    ang = lz.sin_largest_angle(r.vecs, Xw, Bd)
    print(f"  {c.id}: restarts {r.numiter} (table {c.R_ref}), applies {r.numops}, converged {r.converged}; |θ-λ| {verr:.2e}, residual {res:.2e} "
          f"(bars {10 * TOL:.0e}); orthonormality {O:.2e} (bar {o_bar:.1e}); sin θ {ang:.2e} (bar {10 * TOL / gap:.2e}); gap {gap:.3e}")
    assert r.converged == c.nev
    assert np.all(np.isfinite(r.vals)) and np.all(np.isfinite(r.vecs))
    assert verr <= 10 * TOL and res <= 10 * TOL
    assert O <= o_bar
    assert ang <= 10 * TOL / gap
    assert np.all(r.normres <= TOL)
    return lw, gap, O


def _problem(c, fem, probs):
    if c.group in ("schur", "count"):
        P = probs[c.prob[:-1]]
        S, A_gg, v0 = syn.schur_inputs(fem, P, c.prob)
        return S, None if A_gg is None else A_gg.toarray(), A_gg, v0
    A, B, v0 = syn.problem(c.prob)
    return A.toarray(), None if B is None else B.toarray(), B, v0


@pytest.fixture(scope="module")
def probs(micro, toy):
    return {"micro": micro, "toy": toy}


@pytest.mark.parametrize("c", syn.CASES + (syn.TOY_DEFLATION,), ids=[c.id for c in syn.CASES + (syn.TOY_DEFLATION,)])
def test_restatement_meets_the_bars_and_the_table_records_it(fem, probs, c):
    Ad, Bd, Bs, v0 = _problem(c, fem, probs)
    Binv = None if Bs is None else spla.splu(sp.csc_matrix(Bs)).solve
    r = _solve_case(c, Ad, Bs, Binv, v0)
    if c.group == "count":                       # nev = 14 on toy: values, residuals and the count only (no subspace is compared with it)
        lam = lz.dense_eigh(Ad)[0]
        assert r.converged == c.nev and np.max(np.abs(r.vals - lam[:c.nev])) <= 10 * TOL
        assert abs(r.numiter - c.R_ref) <= max(2, c.R_ref // 4)
        return
    lw, gap, O = check_against_eigh(c, r, Ad, Bd, 2e-13)
    assert gap >= syn.GAP_MIN * abs(lw[-1]), f"{c.id}: gap {gap:.3e} below {syn.GAP_MIN} |λ_nev| = {syn.GAP_MIN * abs(lw[-1]):.3e}: replace the case"
    assert abs(gap - c.gap) <= 1e-3 * c.gap, (gap, c.gap)
    assert abs(r.numiter - c.R_ref) <= max(2, c.R_ref // 4), (r.numiter, c.R_ref)
    assert r.numiter <= c.maxiter
    assert O <= max(10 * c.O_ref, 1e-15) and c.O_ref <= 2e-13, (O, c.O_ref)


def test_table_covers_what_the_gpu_file_needs():
    rows = {int(c.prob[5:]) for c in syn.group("rows")}
    assert rows == {255, 256, 257, 1024, 1025, 4097}
    cols = {(c.nev, c.krylovdim, c.which) for c in syn.group("cols")}
    assert cols == {(a, b, w) for a, b in ((1, 8), (7, 16), (8, 17), (10, 20), (18, 36)) for w in ("SR", "LR")}
    t = syn.COLUMN_TILE
    assert {c.krylovdim for c in syn.group("tile")} == {3 * t - 1, 3 * t, 3 * t + 1}
    assert {(c.prob, c.nev, c.krylovdim) for c in syn.group("gen")} == {(p, a, b) for p in ("gdiag257", "gtri257") for a, b in ((6, 12), (10, 20))}
    assert {(c.krylovdim) for c in syn.group("window")} == {36, 37, 40} and all(c.prob == "synth37" for c in syn.group("window"))
    assert all(c.R_ref == 0 for c in syn.group("first")) and syn.group("first")
    src = open(ROOT + "/julia-phd-krylov-spdes_amd/csrc/lanczos_kernels.hpp").read()
    assert re.search(r"constexpr int LZ_CT = (\d+);", src).group(1) == str(t)


@pytest.mark.parametrize("nev", syn.BREAKDOWN_NEV)
def test_restatement_breakdown(nev):
    """v0 is an eigenvector (beta = 0 at step 0); a fresh vector continues; the basis is invariant again after four columns"""
    A, _, v0 = syn.problem("diag37")
    d = A.diagonal()
    assert set(d[[0, 5, 9]]) == {1.0}
    r = lz.eigsolve(lambda x: A @ x, 37, nev, "SR", 0, TOL, 8, v0)
    assert r.converged == nev and r.numiter == 0 and np.all(np.isfinite(r.vals)) and np.all(np.isfinite(r.vecs))
    assert all(np.min(np.abs(d - t)) <= 1e-13 for t in r.vals)
    assert np.max(lz.true_residuals(A.toarray(), None, r.vals, r.vecs)) <= 10 * TOL
    if nev == 2:
        assert np.allclose(r.vals, [1.0, 1.0], rtol=0, atol=1e-13)      # the two smallest of {d0, d5, d9}


@pytest.mark.parametrize("maxiter", [0, 1])
def test_restatement_out_of_restarts(maxiter):
    """maxiter restarts are no error: converged < nev, Ritz values from above (interlacing), estimates that are the residuals"""
    c = syn.BY_ID["rows-synth257-6-12-SR"]
    A, _, v0 = syn.problem(c.prob)
    Ad = A.toarray()
    r = lz.eigsolve(lambda x: A @ x, 257, c.nev, "SR", c.krylovdim, TOL, maxiter, v0)
    lam = lz.dense_eigh(Ad)[0][:c.nev]
    true = lz.true_residuals(Ad, None, r.vals, r.vecs)
    assert r.numiter == maxiter and r.converged < c.nev
    assert np.all(r.vals >= lam - 10 * TOL)
    assert np.all(r.normres <= 2 * true) and np.all(true <= 2 * r.normres)


def test_prepare_lorasc_precond_eigs_hook(fem, micro):
    """eigs = the restatement on the pencil (S, A_ΓΓ) of micro: the same selection as the default dense path, E' A_ΓΓ E = I,
    the same subspace and Σ; ε where the selection cuts (0.2) and where it falls back to nev = nvec (0.01)"""
    S, A_gg, v0 = syn.schur_inputs(fem, micro, "microP")
    lu = spla.splu(A_gg)
    calls = []

    def eigs(k):
        r = lz.eigsolve(lambda x: S @ x, S.shape[0], k, "SR", 2 * k, 1e-12, 100, v0, lambda x: A_gg @ x, lu.solve)
        assert r.converged == k
        calls.append(k)
        return r.vals, r.vecs
    for ε in (0.2, 0.01):
        E0, Σ0 = fem.prepare_lorasc_precond(S, A_gg, nvec=25, ε=ε)
        E1, Σ1 = fem.prepare_lorasc_precond(None, A_gg, nvec=25, ε=ε, eigs=eigs)
        assert E1.shape == E0.shape and Σ1.shape == Σ0.shape and E1.flags.f_contiguous
        assert np.allclose(Σ1, Σ0, rtol=1e-9, atol=0)
        assert lz.ortho_defect(E1, A_gg.toarray()) <= 1e-12
        assert lz.sin_largest_angle(E1, E0, A_gg.toarray()) <= 1e-7
    assert calls == [25, 25]
    E, Σ = fem.prepare_lorasc_precond(None, A_gg, nvec=25, ε=0.0, eigs=eigs)
    assert E.shape == (S.shape[0], 0) and Σ.size == 0 and calls == [25, 25]
    with pytest.raises(ValueError):
        fem.prepare_lorasc_precond(None, A_gg, nvec=25, ε=0.2, eigs=lambda k: (np.zeros(k - 1), np.zeros((S.shape[0], k))))


def test_new_prototype_is_bound(pkg):
    """mi_eigsolve: declared in the header, in the ctypes table with the prototype's 15 parameters, exported by the library;
    NULL handles are MI_ERR_BAD_ARG with a message; the version moved with the feature"""
    text = open(ROOT + "/include/mi355schur.h").read()
    assert "#define MI_EIG_SR 0" in text and "#define MI_EIG_LR 1" in text
    m = re.search(r"int mi_eigsolve\(([^;]*?)\);", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S)
    assert m and len(m.group(1).split(",")) == 15
    sig = pkg._lib.SIGNATURES["mi_eigsolve"]
    assert len(sig) == 15 and sig[4] is C.c_int and sig[6] is C.c_double
    assert (pkg._lib.MI_EIG_SR, pkg._lib.MI_EIG_LR) == (0, 1)
    L = pkg._lib.load()
    assert L.mi_eigsolve(None, None, None, 1, 0, 0, 1e-10, 1, None, None, None, None, None, None, None) == pkg._lib.MI_ERR_BAD_ARG
    assert L.mi_last_error()
    assert L.mi_version() >= 300
    assert callable(pkg.api.eigsolve) and callable(pkg.api.geneigsolve)
