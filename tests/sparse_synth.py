"""Synthetic symmetric matrices for the sparse kernels (CSR SpMV, two-launch sparse PCG, device interior CG) at the
edges of their row-block partition (csrc/spmv_blocks.hpp: blocks of <= SPMV_TILE = 1024 non-zeros, NT = 256 threads).

Not a conftest: tests/test_sparse_edges_cpu.py and tests/test_gpu_sparse_edges.py import it. Everything runs on the host.
P1-FEM matrices hold ~7 non-zeros per row, so a row block has ~146 rows: fewer than one workgroup. The matrices here
have 0, 1, 2, 3 or > 1024 non-zeros per row instead.

  diag(n)            12 distinct positive values: CG ends within 12 iterations. 1024 rows per block (4 row passes).
  tridiag(n, shift)  stencil (-1, 2 + shift, -1): κ < (4 + shift) / shift. ~341 rows per block, odd block ends.
  arrow(n, m)        row and column 0 hold m entries, diagonal |v| + n (diagonally dominant).
  odd_start()        row 0: one entry, row 1: exactly 1024 -> a block that fits the tile at k0 = 1.
  holes()            a tridiagonal scattered over rows with empty rows (and columns) in between; apply only.
  interior sets      lists of subdomains (A_II, A_IΓ, A_ΓΓ) with trivial interface wiring, see interior_set().
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp

SPMV_TILE = 1024
NT = 256
FUSED_MAX_N = 8192

DIAG_VALUES = 1.0 + 0.25 * np.arange(12)          # 1 .. 3.75: κ = 3.75


def _csr(A):
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A


def diag(n, values=DIAG_VALUES, seed=0):
    rng = np.random.default_rng(1000 + seed + n)
    d = np.asarray(values)[rng.integers(0, len(values), size=n)]
    return _csr(sp.diags(d, format="csr"))


def tridiag(n, shift=1.0):
    off = -np.ones(max(n - 1, 0))
    return _csr(sp.diags([off, np.full(n, 2.0 + shift), off], [-1, 0, 1], format="csr"))


def arrow(n, m, seed=6):
    """A[0, :m] = A[:m, 0] = v[:m]; diagonal |v| + n. Row 0 has exactly m entries (v has no zeros)."""
    assert 1 <= m <= n
    v = np.random.default_rng(seed + m).standard_normal(n)
    v[v == 0.0] = 1.0
    i = np.arange(1, m)
    rows = np.concatenate([np.zeros(m - 1, dtype=np.int64), i, np.arange(n)])
    cols = np.concatenate([i, np.zeros(m - 1, dtype=np.int64), np.arange(n)])
    vals = np.concatenate([v[1:m], v[1:m], np.abs(v) + n])
    return _csr(sp.coo_matrix((vals, (rows, cols)), shape=(n, n)))


def odd_start(n=1300):
    """Row 0: its diagonal only (k0 of the next block = 1). Row 1: columns 1..1024, exactly SPMV_TILE entries."""
    v = np.random.default_rng(7).standard_normal(SPMV_TILE)
    j = np.arange(2, SPMV_TILE + 1)
    rows = np.concatenate([np.ones(j.size, dtype=np.int64), j, np.arange(n)])
    cols = np.concatenate([j, np.ones(j.size, dtype=np.int64), np.arange(n)])
    vals = np.concatenate([v[1:], v[1:], np.full(n, float(n))])
    return _csr(sp.coo_matrix((vals, (rows, cols)), shape=(n, n)))


HOLES_LEAD, HOLES_INNER, HOLES_TRAIL = 5, 1500, 7


def holes():
    """tridiag(2400) on the `live` rows/columns: a leading run of empty rows, single and double holes in between, an
    inner run of 1500 (> SPMV_TILE) empty rows, a trailing run. Returns (A, live)."""
    live, r = [], HOLES_LEAD
    for k in range(2400):
        if k == 1200:
            r += HOLES_INNER
        live.append(r)
        r += 1 + (k % 3 == 0) + (k % 7 == 0)              # 0, 1 or 2 empty rows after this one
    n = live[-1] + 1 + HOLES_TRAIL
    live = np.array(live)
    T = sp.coo_matrix(tridiag(live.size))
    A = sp.coo_matrix((T.data, (live[T.row], live[T.col])), shape=(n, n))
    return _csr(A), live


def apply_cases():
    """name -> matrix, every apply case of the table"""
    out = {}
    for n in (1, 1023, 1024, 1025, 5000, 8193, 16385):
        out[f"diag{n}"] = diag(n)
    for n in (3000, 9001, 800000):
        out[f"tridiag{n}"] = tridiag(n)
    for m in (1023, 1024, 1025, 2048, 2049):
        out[f"arrow5000_{m}"] = arrow(5000, m)
    out["arrow9000_9000"] = arrow(9000, 9000)
    out["odd_start"] = odd_start()
    out["holes"] = holes()[0]
    return out


SOLVER_CASES = ("diag8193", "diag16385", "tridiag9001", "tridiag800000", "arrow9000_9000")


def solver_rhs(n, seed=0):
    return np.random.default_rng(4000 + seed + n % 997).standard_normal(n)


# ------------------------------------------------------------------ interior-CG subdomain sets
@dataclass
class InteriorSet:
    """Subdomains with trivial interface wiring: subdomain d owns the Γ nodes 2d, 2d + 1 (node_Γ_cnt = 1), A_IΓ holds the
    single entry (0, 0) = 1 and A_ΓΓ = c I. With u_Γ = 0, `interior_solutions(u_Γ, b_I)` is A_II \\ b_I itself."""
    A_II: list
    A_IΓ: list
    A_ΓΓ: list
    gather_idx: list
    node_Γ_cnt: np.ndarray
    b_I: list                      # per subdomain
    kappa: list                    # an upper bound of κ(A_II) known from the construction (1 for an empty interior)
    reltol: float
    n_i: list = field(default_factory=list)

    @property
    def n_Γ(self):
        return self.node_Γ_cnt.size

    @property
    def breaks(self):
        return np.concatenate([[0], np.cumsum(self.n_i)[:-1]]).astype(np.int64)

    def stacked(self):
        return _csr(sp.block_diag(self.A_II, format="csr")) if sum(self.n_i) else sp.csr_matrix((0, 0))


GAMMA_C = 100.0   # A_ΓΓ = c I. |S_d v| ~ c |v| while the interior term is at most |v| / λ_min(A_II) <= 20 |v| for every
                  # block here, so an interior error of κ reltol |u*| stays under the Schur bar 0.5 reltol max|S v|.


def interior_set(blocks, kappa, reltol, rhs_seed=3, zero_rhs=()):
    ndom = len(blocks)
    rng = np.random.default_rng(rhs_seed)
    A_IΓ, A_ΓΓ, gi, b = [], [], [], []
    for d, A in enumerate(blocks):
        n = A.shape[0]
        ig = sp.lil_matrix((n, 2))
        if n:
            ig[0, 0] = 1.0
        A_IΓ.append(sp.csc_matrix(ig))
        A_ΓΓ.append(sp.csc_matrix(GAMMA_C * sp.identity(2)))
        gi.append(np.array([2 * d, 2 * d + 1], dtype=np.int64))
        b.append(np.zeros(n) if d in zero_rhs else rng.standard_normal(n))
    return InteriorSet([sp.csc_matrix(A) for A in blocks], A_IΓ, A_ΓΓ, gi, np.ones(2 * ndom), b, list(kappa), reltol,
                       [A.shape[0] for A in blocks])


def gershgorin_kappa(A):
    """κ bound of a diagonally dominant symmetric matrix: max(a_ii + R_i) / min(a_ii - R_i)"""
    A = sp.csr_matrix(A)
    d = A.diagonal()
    R = np.asarray(abs(A).sum(axis=1)).ravel() - np.abs(d)
    assert (d - R).min() > 0
    return float((d + R).max() / (d - R).min())


# 8 equally spaced eigenvalues 1 .. 1000 (142.7 apart), κ = 1e3. CG needs all 8 = n_i steps and its 8th step leaves an error
# of ~1e-14 |u*|. (A geometric spectrum 10^(3k/7) also takes 8 steps, but finite-precision CG then ends 2e-8 away.)
CAPPED_EIGS = np.linspace(1.0, 1000.0, 8)


def capped_matrix():
    Q = np.linalg.qr(np.random.default_rng(8).standard_normal((8, 8)))[0]
    A = (Q * CAPPED_EIGS) @ Q.T
    return _csr((A + A.T) / 2), Q


MIXED_ZERO_RHS = 1     # the subdomain of `mixed` whose right-hand side is zero


def interior_sets(names=("mixed", "longrow", "capped", "wide")):
    out = {}
    if "mixed" in names:
        # n_i = [1, 2, 300, 5000, 0]: 1 x 1; tridiagonal, zero right-hand side; diagonal with 12 values in [1, 100]
        # (ends within 12 iterations); tridiagonal with shift 0.05, κ < 81 (~100 iterations); empty interior
        wide_vals = np.linspace(1.0, 100.0, 12)
        blocks = [diag(1), tridiag(2, 1.0), diag(300, wide_vals), tridiag(5000, 0.05), sp.csr_matrix((0, 0))]
        out["mixed"] = interior_set(blocks, [1.0, 5.0, 100.0, 81.0, 1.0], 1e-9, zero_rhs=(MIXED_ZERO_RHS,))
    if "longrow" in names:
        A = arrow(3000, 3000)
        out["longrow"] = interior_set([A], [gershgorin_kappa(A)], 1e-9)
    if "capped" in names:
        A, Q = capped_matrix()
        s = interior_set([A], [1e3], 1e-14)
        s.b_I = [Q @ np.ones(8)]                   # every eigenvector takes part: no early exact termination
        out["capped"] = s
    if "wide" in names:
        out["wide"] = interior_set([tridiag(300000, 1.0)], [5.0], 1e-9)
    return out


# ------------------------------------------------------------------ the partition file of tests/cpp/spmv_blocks_check.cpp
def write_rowptr(path, indptr, breaks=()):
    indptr = np.asarray(indptr, dtype=np.int32)
    breaks = np.asarray(breaks, dtype=np.int32)
    with open(path, "wb") as f:
        np.array([indptr.size - 1, breaks.size], dtype="<i4").tofile(f)
        indptr.astype("<i4").tofile(f)
        breaks.astype("<i4").tofile(f)
