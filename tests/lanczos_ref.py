"""Thick-restart Lanczos with full re-orthogonalisation, restated in numpy: the reference of tests/test_lanczos_cpu.py and
tests/test_gpu_lanczos.py for `mi_eigsolve` (csrc/lanczos.hpp). Nothing of this file is compiled into the library.

Standard problem A x = λ x, window m = krylovdim (clamped to n), basis V (n x (m+1)), projected matrix T (m x m):
  step j : w = A v_j; h = V[:, :j+1]' w; w -= V h; a second identical pass h2 (CGS2); T[:j+1, j] = T[j, :j+1] = h + h2;
           beta = ||w||; v_{j+1} = w / beta
  after step m-1: T = Y Θ Y', ascending (SR) or descending (LR); rho_i = |beta Y[m-1, i]|; nconv = leading pairs with
           rho_i <= tol (at most nev); done if nconv >= nev, or `maxiter` restarts were made, or m == n
  restart: k = min(nev + (m - nev)//2, m - 1); V[:, :k] = V[:, :m] Y[:, :k]; v_k = v_m; T = diag(θ_1..θ_k); go on at j = k
Generalized problem A x = λ B x (B SPD, as operators B and Binv): Lanczos on B^-1 A in the B inner product with Q = B V:
  u = A v_j; w = Binv u; h = V'u; w -= V h; u = B w (applied: the recurrence u -= Q h loses B-orthogonality steadily);
  h2 = V'u; w -= V h2; u -= Q h2; beta = sqrt(w'u); v_{j+1} = w / beta; q_{j+1} = u / beta
Break-down, beta <= 64 eps max|T|: with j + 1 >= nev the call ends on the exact pairs of V[:, :j+1]; otherwise a fresh
vector, (B-)orthogonalised twice, continues the basis. With m == n the last step does not normalise."""
from dataclasses import dataclass

import numpy as np

EPS = np.finfo(np.float64).eps


@dataclass
class Result:
    vals: np.ndarray
    vecs: np.ndarray
    normres: np.ndarray
    converged: int
    numiter: int          # restarts
    numops: int           # applies of A


class NonFinite(ArithmeticError):
    pass


def _cgs2(V, Q, w, u, ncols, B):
    """two passes of classical Gram-Schmidt of w (u = B w) against V[:, :ncols]; returns (w, u, h + h2)"""
    x = w if B is None else u
    h = V[:, :ncols].T @ x
    w = w - V[:, :ncols] @ h
    if B is not None:
        u = B(w)
    x = w if B is None else u
    h2 = V[:, :ncols].T @ x
    w = w - V[:, :ncols] @ h2
    if B is not None:
        u = u - Q[:, :ncols] @ h2
    return w, u, h + h2


def eigsolve(A, n, nev, which="SR", krylovdim=0, tol=1e-12, maxiter=100, v0=None, B=None, Binv=None, fresh_seed=0):
    """A, B, Binv: callables on vectors. Returns a Result; `vecs` is n x nev with vecs' B vecs = I."""
    assert 1 <= nev <= n and which in ("SR", "LR") and (B is None) == (Binv is None)
    m = min(krylovdim if krylovdim else max(2 * nev, 8), n)
    assert m >= nev + 1 or m == n
    V = np.zeros((n, m + 1))
    Q = np.zeros((n, m + 1)) if B is not None else None
    T = np.zeros((m, m))
    w = np.array(np.random.default_rng(0).uniform(-1, 1, n) if v0 is None else v0, dtype=np.float64)
    u = B(w) if B is not None else w
    beta = np.sqrt(w @ u)
    if not np.isfinite(beta) or beta <= 0:
        raise NonFinite("start vector")
    V[:, 0] = w / beta
    if B is not None:
        Q[:, 0] = u / beta
    j, restarts, numops, tmax, m_eff, fresh = 0, 0, 0, 0.0, m, np.random.default_rng(1000 + fresh_seed)
    while True:
        finish = False
        while j < m:
            if B is None:
                w = A(V[:, j])
                u = None
            else:
                u = A(V[:, j])
                w = Binv(u)
            numops += 1
            w, u, t = _cgs2(V, Q, w, u, j + 1, B)
            T[:j + 1, j] = t
            T[j, :j + 1] = t
            beta = np.sqrt(w @ (w if B is None else u))
            tmax = max(tmax, np.max(np.abs(t))) if np.all(np.isfinite(t)) else np.nan
            if not np.isfinite(beta) or not np.isfinite(tmax):
                raise NonFinite(f"step {j}")
            if m == n and j == n - 1:                     # the basis spans everything: beta is rounding noise
                j += 1
                break
            if beta <= 64 * EPS * tmax:                   # V[:, :j+1] is invariant
                if j + 1 >= nev:
                    m_eff, finish = j + 1, True
                    break
                w = fresh.uniform(-1, 1, n)
                u = B(w) if B is not None else None
                w, u, _ = _cgs2(V, Q, w, u, j + 1, B)
                b2 = np.sqrt(w @ (w if B is None else u))
                V[:, j + 1] = w / b2
                if B is not None:
                    Q[:, j + 1] = u / b2
                j += 1
                continue
            V[:, j + 1] = w / beta
            if B is not None:
                Q[:, j + 1] = u / beta
            j += 1
        θ, Y = np.linalg.eigh(T[:m_eff, :m_eff])
        if which == "LR":
            θ, Y = θ[::-1], Y[:, ::-1]
        rho = np.abs(beta * Y[m_eff - 1, :])
        nconv = 0
        while nconv < nev and rho[nconv] <= tol:
            nconv += 1
        if finish or nconv >= nev or restarts >= maxiter or m_eff == n:
            break
        k = min(nev + (m - nev) // 2, m - 1)
        V[:, :k] = V[:, :m] @ Y[:, :k]
        V[:, k] = V[:, m]
        if B is not None:
            Q[:, :k] = Q[:, :m] @ Y[:, :k]
            Q[:, k] = Q[:, m]
        T[:] = 0.0
        T[np.arange(k), np.arange(k)] = θ[:k]
        tmax = float(np.max(np.abs(θ[:k])))
        j = k
        restarts += 1
    X = V[:, :m_eff] @ Y[:, :nev]
    return Result(θ[:nev].copy(), X, rho[:nev].copy(), nconv, restarts, numops)


# ------------------------------------------------------------------ what the bars are measured with
def dense_eigh(A, B=None):
    """ascending (λ, X) of the dense symmetric matrix or pencil"""
    import scipy.linalg as sla
    A = (A + A.T) / 2
    return sla.eigh(A) if B is None else sla.eigh(A, (B + B.T) / 2)


def wanted(lam, X, nev, which):
    """(λ[:nev], X[:, :nev], gap) in the order mi_eigsolve returns them; gap = |λ_{nev+1} - λ_nev| (inf when nev == n)"""
    if which == "LR":
        lam, X = lam[::-1], X[:, ::-1]
    gap = abs(lam[nev] - lam[nev - 1]) if nev < lam.size else np.inf
    return lam[:nev], X[:, :nev], gap


def true_residuals(A, B, vals, X):
    """||A x_i - θ_i B x_i|| in the B^-1 norm (the 2-norm for the standard problem); A, B dense"""
    R = A @ X - (X if B is None else B @ X) * vals[None, :]
    if B is None:
        return np.linalg.norm(R, axis=0)
    return np.sqrt(np.maximum(np.einsum("ij,ij->j", R, np.linalg.solve(B, R)), 0.0))


def ortho_defect(X, B=None):
    G = X.T @ (X if B is None else B @ X)
    return float(np.max(np.abs(G - np.eye(X.shape[1]))))


def sin_largest_angle(X, Xref, B=None):
    """sine of the largest principal angle between span(X) and span(Xref), in the B inner product"""
    if B is not None:
        L = np.linalg.cholesky((B + B.T) / 2)
        X, Xref = L.T @ X, L.T @ Xref
    Qx, Qr = np.linalg.qr(X)[0], np.linalg.qr(Xref)[0]
    return float(np.linalg.norm(Qx - Qr @ (Qr.T @ Qx), 2))
