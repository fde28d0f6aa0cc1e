"""Host reference of the LORASC preconditioner for tests/test_lorasc_cpu.py and tests/test_gpu_lorasc.py.

`apply_lorasc` restates the reference's function (EPDD.jl:1908-1976) statement by statement in numpy / scipy, the way
oracle/ restates the solvers; SuperLU stands in for CHOLMOD in the two solves, either plain or with iterative refinement
on long-double residuals (the form the GPU suite compares against: its own error is far below the GPU bar, which the CPU
suite asserts). `dense_minv` is M^-1 column by column from it, `prepare_lorasc_precond_ref` the `:exact` branch of
`prepare_lorasc_precond` (EPDD.jl:1541-1617) by a Cholesky reduction to a standard symmetric eigenproblem."""
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from conftest import f_m1, lognormal_coeff, one, u0734, unstructured_mesh


class Solve:
    """x = A \\ r through SuperLU; `refine` sweeps of iterative refinement with the residual formed in long double."""

    def __init__(self, A, refine: int = 0):
        A = sp.csc_matrix(A)
        A.sum_duplicates()
        self.lu = spla.splu(A)
        self.refine = refine
        c = A.tocoo()
        self.r, self.c, self.v = c.row, c.col, c.data.astype(np.longdouble)
        self.n = A.shape[0]

    def _residual(self, b, x):
        out = np.asarray(b, dtype=np.longdouble).copy()
        xl = np.asarray(x, dtype=np.longdouble)
        if out.ndim == 1:
            np.subtract.at(out, self.r, self.v * xl[self.c])
        else:
            np.subtract.at(out, self.r, self.v[:, None] * xl[self.c])
        return out

    def __call__(self, b):
        x = self.lu.solve(np.asarray(b, dtype=np.float64))
        for _ in range(self.refine):
            x = (x.astype(np.longdouble) + self.lu.solve(self._residual(b, x).astype(np.float64))).astype(np.float64)
        return x


@dataclass
class Case:
    name: str
    P: object                  # fem.SchurProblem on the local blocks (the set-up plan's input)
    A_IId: list
    A_IΓd: list                # Γ-global columns
    A_ΓΓ: sp.spmatrix
    A: sp.csr_matrix           # the full matrix, rows in not_dirichlet order
    b: np.ndarray
    pos_I: list
    pos_Γ: np.ndarray
    coeff: object = None

    @property
    def n(self):
        return self.A.shape[0]

    @property
    def n_Γ(self):
        return int(self.pos_Γ.size)

    def solves(self, refine: int):
        key = ("solves", refine)
        if key not in self.__dict__:
            self.__dict__[key] = ([Solve(M, refine) for M in self.A_IId], Solve(self.A_ΓΓ, refine))
        return self.__dict__[key]


def make_case(fem, name, N, px, py, coeff=one, mesh=None, partition=None):
    P = fem.build_schur_problem(N, px, py, coeff, f_m1, u0734, assemble=False, mesh=mesh, partition=partition)
    m = P.mesh
    A_IId, A_IΓd, A_ΓΓ, _, _ = fem.prepare_global_schur(m.cells, m.points, P.epart, P.sub, coeff, f_m1, u0734)
    A, b = fem.do_isotropic_elliptic_assembly(m.cells, m.points, P.dinds, m.point_marker, coeff, f_m1, u0734)
    g2l = P.dinds.not_dirichlet_g2l
    return Case(name, P, A_IId, A_IΓd, sp.csc_matrix(A_ΓΓ), sp.csr_matrix(A), b, [g2l[nd] for nd in P.sub.node_Id],
                g2l[P.sub.node_Γ], coeff)


# (N, px, py) of the partitions whose n_Γ leaves a one-thread tail in the last 256-thread workgroup, fills it, and is
# one short of filling it (asserted in test_lorasc_cpu.py)
EDGE_PARTITIONS = {"tail1": (67, 4, 2), "full": (67, 3, 3), "short1": (46, 4, 4)}


def gpu_cases(fem, which=None):
    """The inputs of the GPU suite, by name (built on demand)."""
    def ragged():
        mesh = fem.get_mesh(50)
        return make_case(fem, "ragged", 50, 3, 2, lognormal_coeff(fem, mesh.points, 7))

    def unstructured():
        mesh, epart, npart = unstructured_mesh(fem)
        return make_case(fem, "unstructured", mesh.N, 1, 1, one, mesh=mesh, partition=(epart, npart))

    makers = {"micro": lambda: make_case(fem, "micro", 40, 2, 2), "ragged": ragged, "unstructured": unstructured,
              "strip": lambda: make_case(fem, "strip", 30, 1, 2)}
    for k, (N, px, py) in EDGE_PARTITIONS.items():
        makers[k] = (lambda N=N, px=px, py=py, k=k: make_case(fem, k, N, px, py))
    return {k: makers[k]() for k in (which or makers)}


def apply_lorasc(case: Case, x, E=None, coef=None, refine: int = 0):
    """EPDD.jl:1908-1976 on a vector or on the columns of a matrix; `coef=None` is the reference as written (ones)."""
    x = np.asarray(x, dtype=np.float64)
    chol_A_IId, chol_A_ΓΓ = case.solves(refine)
    ndom = len(case.A_IId)
    x_Id = [x[case.pos_I[d]] for d in range(ndom)]                 # :1922-1926
    x_Γ = x[case.pos_Γ].copy()                                     # :1929-1933
    z_Γ = x_Γ.copy()
    for d in range(ndom):                                          # :1935-1942
        x_Id[d] = chol_A_IId[d](x_Id[d])
        z_Γ = z_Γ - case.A_IΓd[d].T @ x_Id[d]
    x_Γ = chol_A_ΓΓ(z_Γ)                                           # :1950
    if E is not None:
        E = np.asarray(E, dtype=np.float64).reshape(case.n_Γ, -1)
        for k in range(E.shape[1]):                                # :1954-1957
            val = E[:, k] @ z_Γ
            c = 1.0 if coef is None else coef[k]
            x_Γ = x_Γ + (c * val) * (E[:, k] if x.ndim == 1 else E[:, k][:, None])
    for d in range(ndom):                                          # :1959-1961
        x_Id[d] = x_Id[d] - chol_A_IId[d](case.A_IΓd[d] @ x_Γ)
    u = np.empty_like(x)
    for d in range(ndom):                                          # :1964-1968
        u[case.pos_I[d]] = x_Id[d]
    u[case.pos_Γ] = x_Γ                                            # :1971-1973
    return u


def dense_minv(case: Case, E=None, coef=None, refine: int = 0):
    """M^-1 as a dense matrix: `apply_lorasc` on the columns of the identity."""
    return np.asfortranarray(apply_lorasc(case, np.eye(case.n), E, coef, refine))


def block_formula_minv(case: Case, E=None, coef=None):
    """M^-1 = [I -A_II^-1 A_IΓ; 0 I] diag(A_II^-1, A_ΓΓ^-1 + E diag(coef) E') [I 0; -A_ΓI A_II^-1 I], dense algebra, in
    the (I_1, ..., I_ndom, Γ) ordering, then permuted to the rows of A."""
    n_I = [a.shape[0] for a in case.A_IId]
    nI, nΓ = sum(n_I), case.n_Γ
    A_II = sp.block_diag(case.A_IId).toarray()
    A_IΓ = sp.vstack(case.A_IΓd).toarray()
    iA = np.linalg.inv(A_II)
    mid = np.linalg.inv(case.A_ΓΓ.toarray())
    if E is not None:
        E = np.asarray(E).reshape(nΓ, -1)
        c = np.ones(E.shape[1]) if coef is None else np.asarray(coef)
        mid = mid + (E * c) @ E.T
    U = np.block([[np.eye(nI), -iA @ A_IΓ], [np.zeros((nΓ, nI)), np.eye(nΓ)]])
    D = np.block([[iA, np.zeros((nI, nΓ))], [np.zeros((nΓ, nI)), mid]])
    L = np.block([[np.eye(nI), np.zeros((nI, nΓ))], [-A_IΓ.T @ iA, np.eye(nΓ)]])
    perm = np.concatenate(list(case.pos_I) + [case.pos_Γ])
    out = np.empty((nI + nΓ, nI + nΓ))
    out[np.ix_(perm, perm)] = U @ D @ L
    return out


def dense_schur(case: Case):
    """S = A_ΓΓ - Σ_d A_IΓd' A_IId^-1 A_IΓd (the operator of Example03:101 as a matrix)."""
    S = case.A_ΓΓ.toarray()
    for Aii, Aig in zip(case.A_IId, case.A_IΓd):
        S = S - Aig.T @ spla.splu(sp.csc_matrix(Aii)).solve(Aig.toarray())
    return (S + S.T) / 2


def prepare_lorasc_precond_ref(S, A_ΓΓ, nvec=25, ε=0.01):
    """EPDD.jl:1541-1617, `:exact`: the nvec smallest pairs of S e = σ A_ΓΓ e with E' A_ΓΓ E = I (L^-1 S L^-T v = σ v,
    e = L^-T v), sorted (:1588-1590), then the selection loop (:1593-1610)."""
    A = A_ΓΓ.toarray() if sp.issparse(A_ΓΓ) else np.asarray(A_ΓΓ)
    L = np.linalg.cholesky(A)
    C = np.linalg.solve(L, np.linalg.solve(L, S).T).T
    w, V = np.linalg.eigh((C + C.T) / 2)
    nvec = min(nvec, A.shape[0])
    Σ, E = w[:nvec].copy(), np.linalg.solve(L.T, V[:, :nvec])
    nev = 0
    for k, σ in enumerate(Σ):
        if σ < ε:
            Σ[k] = (ε - σ) / σ
            nev += 1
        else:
            break
    if nev == 0:
        nev = nvec
    return E[:, :nev], Σ[:nev]


ALL_CASES = ("micro", "ragged", "unstructured", "strip", "tail1", "full", "short1")
# (nev, random positive coef?) of the apply tests; 257 crosses the 256-thread edge of the t / partials loops
APPLY_VARIANTS = ((0, False), (1, False), (1, True), (25, False), (25, True), (257, False), (257, True))


def apply_inputs(case: Case, nev: int, with_coef: bool):
    """The random x, E (n_Γ x nev, need not be eigenvectors for an apply test) and coef of one apply test."""
    rng = np.random.default_rng(sum(case.name.encode()) * 1000 + nev * 2 + int(with_coef))
    x = rng.standard_normal(case.n)
    E = rng.standard_normal((case.n_Γ, nev)) / np.sqrt(case.n_Γ) if nev else None
    coef = 0.5 + rng.random(nev) if (with_coef and nev) else None
    return x, E, coef
