"""Inputs and the case table of the eigensolver tests (tests/test_lanczos_cpu.py, tests/test_gpu_lanczos.py): data and
builders only; the numpy restatement is tests/lanczos_ref.py.

Problems, by name:
  synth<n> / mild<n>   eig_synth.matrix(n) / matrix_mild(n) as CSR operators, v0 = eig_synth.rhs(n) (dense, random: no
                       eigenvector is missed)
  diag37               eig_synth.diagonal_system(37): eigenvalues 1, 2, 4 only — a start vector with three non-zeros spans an
                       invariant subspace of dimension 3
  gdiag<n> / gtri<n>   the pencil (eig_synth.matrix(n), B): B = diag(0.5 + 4 U(0,1)) (mi_diag_create as B and as B^-1), and that
                       diagonal plus -0.2 off-diagonals (SparseMatrixCSC + SparseDirectPreconditioner)
  microS / toyS        the assembled Schur complement of conftest.micro / toy (LocalSchurs), nev = ndom + 10 (Example03:206)
  microP / toyP        the LORASC pencil (S, A_ΓΓ) (EPDD.jl:1546-1549), nvec = 25, krylovdim = 50

Every case records what the restatement does on it at tol = TOL: its restart count R_ref (the device run gets
maxiter = 4 R_ref + 8, so that a stagnating run fails instead of spinning), its orthonormality defect O_ref
(max |X' B X - I|) and the gap |λ_{nev+1} - λ_nev| to the first eigenvalue not asked for. test_lanczos_cpu.py checks the
records against the restatement and that gap >= 1e-3 |λ_nev| for every case."""
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

import eig_synth as es
import sparse_synth as ss

TOL = 1e-10
GAP_MIN = 1e-3
COLUMN_TILE = 4       # csrc/lanczos_kernels.hpp LZ_CT: columns whose loads are issued together


@dataclass(frozen=True)
class Case:
    group: str
    prob: str
    nev: int
    krylovdim: int
    which: str
    R_ref: int            # restarts of the restatement
    O_ref: float          # its max |X' B X - I|
    gap: float            # |λ_{nev+1} - λ_nev| (mirrored for LR)

    @property
    def id(self):
        return f"{self.group}-{self.prob}-{self.nev}-{self.krylovdim}-{self.which}"

    @property
    def maxiter(self):
        return 4 * self.R_ref + 8


def b_diagonal(n):
    return 0.5 + 4.0 * np.random.default_rng(4400 + n).uniform(0.0, 1.0, n)


def pencil_B(prob):
    """(B as CSR, kind) of a generalized synthetic problem"""
    n = int(prob.lstrip("gdiatr"))
    d = b_diagonal(n)
    if prob.startswith("gdiag"):
        return ss._csr(sp.diags(d)), "diag"
    off = -0.2 * np.ones(n - 1)
    return ss._csr(sp.diags([off, d, off], [-1, 0, 1])), "tri"


def problem(prob):
    """(A CSR, B CSR or None, v0) of a synthetic problem"""
    if prob == "diag37":
        A = es.diagonal_system(37)[0]
        v0 = np.zeros(37)
        v0[[0, 5, 9]] = 1.0
        return A, None, v0
    if prob.startswith("synth"):
        n = int(prob[5:])
        return es.matrix(n), None, es.rhs(n)
    if prob.startswith("mild"):
        n = int(prob[4:])
        return es.matrix_mild(n), None, es.rhs(n)
    if prob.startswith("g"):
        B, _ = pencil_B(prob)
        n = B.shape[0]
        return es.matrix(n), B, es.rhs(n)
    raise KeyError(prob)


def schur_inputs(fem, P, prob):
    """(S dense, A_ΓΓ CSC or None, v0) of microS / toyS / microP / toyP on the SchurProblem P of that mesh"""
    from conftest import f_m1, one, u0734
    n = P.sub.n_Γ
    S = np.zeros((n, n))
    for Sd, g in zip(P.Sd, P.sub.gather_idx):
        S[np.ix_(g, g)] += Sd
    A_gg = None
    if prob.endswith("P"):
        A_gg = sp.csc_matrix(fem.prepare_global_schur(P.mesh.cells, P.mesh.points, P.epart, P.sub, one, f_m1, u0734)[2])
    return S, A_gg, es.rhs(n)


# group, prob, nev, krylovdim, which, R_ref, O_ref, gap — the last three as tests/lanczos_ref.py gives them (test_lanczos_cpu.py)
_TABLE = (
    # row-slice edges: 1024 rows are one workgroup, 1025 two, 4097 five with a ragged tail; 255 / 257: a last double2 that is
    # half padding (odd n) and a last wave that is partly idle
    ("rows", "synth255", 6, 12, "SR", 112, 1.1e-14, 4.573e-02),
    ("rows", "synth256", 6, 12, "SR", 120, 1.4e-14, 4.555e-02),
    ("rows", "synth257", 6, 12, "SR", 119, 1.6e-14, 4.538e-02),
    ("rows", "synth1024", 6, 12, "SR", 368, 2.8e-14, 1.160e-02),
    ("rows", "synth1025", 6, 12, "SR", 420, 6.3e-14, 1.158e-02),
    ("rows", "synth4097", 6, 12, "SR", 1570, 1.4e-13, 2.916e-03),
    # column edges, SR and LR
    ("cols", "synth257", 1, 8, "SR", 66, 4.4e-16, 4.528e-02),
    ("cols", "synth257", 1, 8, "LR", 16, 2.6e-15, 2.886e-01),
    ("cols", "synth257", 7, 16, "SR", 47, 6.2e-15, 4.529e-02),
    ("cols", "synth257", 7, 16, "LR", 19, 4.2e-15, 1.465e-01),
    ("cols", "synth257", 8, 17, "SR", 47, 8.7e-15, 4.518e-02),
    ("cols", "synth257", 8, 17, "LR", 21, 5.8e-15, 1.386e-01),
    ("cols", "synth257", 10, 20, "SR", 44, 1.5e-14, 4.496e-02),
    ("cols", "synth257", 10, 20, "LR", 21, 5.3e-15, 1.260e-01),
    ("cols", "synth257", 18, 36, "SR", 21, 6.2e-15, 4.392e-02),
    ("cols", "synth257", 18, 36, "LR", 11, 6.3e-15, 9.489e-02),
    # the window one short of, equal to and one past a multiple of COLUMN_TILE (every step count 1 .. krylovdim occurs in the
    # first window of every case; these make the LAST group of the full window 3, 4 and 1 columns wide)
    ("tile", "synth257", 5, 11, "LR", 42, 5.7e-15, 1.673e-01),
    ("tile", "synth257", 5, 12, "LR", 28, 3.1e-15, 1.673e-01),
    ("tile", "synth257", 5, 13, "LR", 25, 3.6e-15, 1.673e-01),
    # krylovdim one below n (a restart), above n and equal to n (clamped: one exact window whose last step must not normalise)
    ("window", "synth37", 18, 36, "SR", 1, 1.7e-15, 2.070e-01),
    ("window", "synth37", 18, 40, "SR", 0, 1.6e-15, 2.070e-01),
    ("window", "synth37", 18, 37, "LR", 0, 1.1e-15, 2.287e-01),
    # generalized, both forms of B
    ("gen", "gdiag257", 6, 12, "SR", 302, 3.2e-14, 2.087e-02),
    ("gen", "gdiag257", 10, 20, "SR", 111, 1.3e-14, 1.083e-02),
    ("gen", "gtri257", 6, 12, "SR", 268, 1.2e-14, 2.554e-02),
    ("gen", "gtri257", 10, 20, "SR", 104, 1.6e-14, 1.143e-02),
    # Schur operators. toy at nev = ndom + 10 = 14 cuts between 0.50975516 and 0.50998986 (SR; relative gap 4.6e-4) and between
    # 5.59070905 and 5.5890956 (LR; 2.9e-4): below GAP_MIN, so the subspace cases of toy run at nev = 13 (gaps 0.21 and 4.3e-3)
    ("schur", "microS", 14, 28, "SR", 9, 4.1e-15, 7.276e-03),
    ("schur", "microS", 14, 28, "LR", 14, 3.6e-15, 2.450e-02),
    ("schur", "toyS", 13, 26, "SR", 18, 5.3e-15, 8.815e-02),
    ("schur", "toyS", 13, 26, "LR", 46, 1.3e-14, 2.402e-02),
    ("schur", "microP", 25, 50, "SR", 1, 3.6e-15, 2.253e-02),
    ("schur", "toyP", 25, 50, "SR", 4, 4.2e-15, 2.974e-02),
)

# Convergence inside the first window (nrestart == 0): the largest eigenvalue of synth257 with a 60-column window
FIRST_WINDOW = ("first", "synth257", 1, 60, "LR", 0, 6.7e-16, 2.886e-01)
# toy at Example03:206's nev = ndom + 10 = 14, for the defpcg iteration-count comparison only (no subspace is compared: see above)
TOY_DEFLATION = ("count", "toyS", 14, 28, "SR", 21, 7.5e-15, 2.347e-04)
# Break-down: diag37 with v0 = e0 + e5 + e9. d0 = d5 = d9 = 1, so v0 IS an eigenvector: beta = 0 at step 0, a fresh vector
# continues the basis; it meets the three distinct eigenvalues 1, 2, 4, so the basis is invariant again after four columns.
BREAKDOWN_NEV = (2, 4)


CASES = tuple(Case(*row) for row in _TABLE + (FIRST_WINDOW,))
TOY_DEFLATION = Case(*TOY_DEFLATION)
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def group(g):
    return [c for c in CASES if c.group == g]
