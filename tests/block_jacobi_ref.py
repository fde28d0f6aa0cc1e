"""Host reference of the block-Jacobi preconditioner (`mi_block_jacobi_*`, csrc/block_jacobi.hpp) for
tests/test_block_jacobi_cpu.py and tests/test_gpu_block_jacobi.py.

  slices(n, nb)            the reference's slice rule (BJPreconditioner.jl:1-32), 0-based half-open
  default_seeds(A, nb)     the default seed rule of block_jacobi.hpp in numpy (block-local indices per block)
  shapes(A, nb, seeds)     per block (n_G, levels, widest level, components)
  Ref(A, nb, refine)       y[slice] = B_d \\ x[slice] per block through SuperLU refined on long-double residuals
                           (lorasc_ref.Solve), and the dense blockdiag(B_d^-1) for the oracle
  sweep(A, nb, seeds, r)   numpy copy of the device's ONE-sweep recursion: levels by setup_synth.bfs_levels, inverses by
                           setup_synth.gj_emulate
  ladder_matrix(...)       a full SPD matrix whose block has exactly the requested seeds and level widths
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.csgraph as csgraph

import setup_synth as ss
from lorasc_ref import Solve

EPS = np.finfo(np.float64).eps


def slices(n, nb):
    bsize = n // nb
    return [(d * bsize, (d + 1) * bsize if d + 1 < nb else n) for d in range(nb)]


def default_seeds(A, nb):
    A = sp.csc_matrix(A)
    n = A.shape[0]
    out = []
    for lo, hi in slices(n, nb):
        B = A[lo:hi, lo:hi]
        ncomp, lab = csgraph.connected_components(B, directed=False)
        rows = sp.csr_matrix(A[lo:hi, :])
        low = np.array([np.any(rows.indices[rows.indptr[v]:rows.indptr[v + 1]] < lo) for v in range(hi - lo)])
        high = np.array([np.any(rows.indices[rows.indptr[v]:rows.indptr[v + 1]] >= hi) for v in range(hi - lo)])
        seed = np.zeros(hi - lo, dtype=bool)
        for c in range(ncomp):
            nodes = np.flatnonzero(lab == c)
            if low[nodes].any():
                seed[nodes[low[nodes]]] = True
            elif high[nodes].any():
                seed[nodes[high[nodes]]] = True
            else:
                seed[nodes.min()] = True
        out.append(np.flatnonzero(seed))
    return out


def split(B, G):
    """(I, levels): the non-seed nodes (ascending) and the plan's breadth-first levels as positions in I"""
    m = B.shape[0]
    I = np.setdiff1d(np.arange(m), G)
    B = sp.csc_matrix(B)
    levels = ss.bfs_levels(B[I][:, I], B[I][:, G]) if I.size else []
    return I, levels


def shapes(A, nb, seeds=None):
    A = sp.csc_matrix(A)
    seeds = default_seeds(A, nb) if seeds is None else seeds
    out = []
    for (lo, hi), G in zip(slices(A.shape[0], nb), seeds):
        B = A[lo:hi, lo:hi]
        I, levels = split(B, G)
        assert sum(len(l) for l in levels) == I.size, "a node is not reached"
        out.append((len(G), len(levels), max([len(l) for l in levels], default=0), csgraph.connected_components(B, directed=False)[0]))
    return out


class Ref:
    def __init__(self, A, nb, refine=2):
        self.A, self.nb = sp.csc_matrix(A), nb
        self.sl = slices(self.A.shape[0], nb)
        self.solves = [Solve(self.A[lo:hi, lo:hi], refine) for lo, hi in self.sl]

    def __call__(self, x):
        y = np.empty_like(np.asarray(x, dtype=np.float64))
        for (lo, hi), s in zip(self.sl, self.solves):
            y[lo:hi] = s(x[lo:hi])
        return y

    def dense_minv(self):
        n = self.A.shape[0]
        M = np.zeros((n, n))
        for (lo, hi), s in zip(self.sl, self.solves):
            M[lo:hi, lo:hi] = s(np.eye(hi - lo))
        return np.asfortranarray((M + M.T) / 2)


def sweep(A, nb, r, seeds=None):
    """The device's recursion in numpy: Z_m = A_mm^-1, Z_k = (A_kk - C_k' Z_{k+1} C_k)^-1, S_G = B_GG - B' Z_0 B;
    forward g_k = r_k - C_k' Z_{k+1} g_{k+1}; u_G = S_G^-1 (r_G - B' Z_0 g_0); u_0 = Z_0 (g_0 - B u_G);
    u_{k+1} = Z_{k+1} (g_{k+1} - C_k u_k). Every inverse by the device's blocked Gauss-Jordan (gj_emulate)."""
    A = sp.csc_matrix(A)
    seeds = default_seeds(A, nb) if seeds is None else seeds
    z = np.empty(A.shape[0])
    for (lo, hi), G in zip(slices(A.shape[0], nb), seeds):
        B = A[lo:hi, lo:hi].toarray()
        rb = r[lo:hi]
        I, levels = split(sp.csc_matrix(B), G)
        L = [I[l] for l in levels]                        # block-local nodes per level
        m = len(L)
        Z, g = [None] * m, [None] * m
        for k in range(m - 1, -1, -1):
            T, gk = B[np.ix_(L[k], L[k])], rb[L[k]].copy()
            if k + 1 < m:
                C = B[np.ix_(L[k + 1], L[k])]
                T = T - C.T @ Z[k + 1] @ C
                gk = gk - C.T @ (Z[k + 1] @ g[k + 1])
            Z[k], g[k] = ss.gj_emulate(T), gk
        S, t = B[np.ix_(G, G)], rb[G].copy()
        if m:
            Bc = B[np.ix_(L[0], G)]
            S = S - Bc.T @ Z[0] @ Bc
            t = t - Bc.T @ (Z[0] @ g[0])
        uG = ss.gj_emulate(np.triu(S) + np.triu(S, 1).T) @ t
        zb = np.empty(hi - lo)
        zb[G] = uG
        u = None
        for k in range(m):
            rhs = g[k] - (Bc @ uG if k == 0 else B[np.ix_(L[k], L[k - 1])] @ u)
            u = Z[k] @ rhs
            zb[L[k]] = u
        z[lo:hi] = zb
    return z


def ladder_matrix(widths, n_gamma, seed=0, shift=1.0, **kw):
    """(A, seeds): A = [A_II A_IΓ; A_IΓ' A_ΓΓ] of setup_synth.ladder (SPD by diagonal dominance, κ small through `shift`), the
    Γ nodes as the explicit seeds: n_G = n_gamma and levels of exactly `widths`."""
    s = ss.ladder(widths, n_gamma=n_gamma, seed=seed, shift=shift, **kw)
    nI = s.A_II.shape[0]
    A = sp.bmat([[s.A_II, s.A_IΓ], [s.A_IΓ.T, s.A_ΓΓ + 4.0 * sp.identity(n_gamma)]], format="csc")
    return A, np.arange(nI, nI + n_gamma)


# (n_G, level-0 width) of the kernel-edge cases: the 64-row tile and the 256-thread tail of k_bj_gamma (tiles n_G) and
# k_bj_back0 (tiles n_0), on the diagonal and with unequal sizes (the B-column and B-row loops)
EDGE_PAIRS = [(w, w) for w in (1, 63, 64, 65, 255, 256, 257)] + [(1, 257), (257, 1), (64, 255), (255, 65)]


def edge_matrix(ng, n0):
    return ladder_matrix([n0, 5], n_gamma=ng, seed=ng + 1000 * n0, degree=2)


def edge_bar(A, nb, n_g, max_level):
    """50 κ₂(B) m eps, m = max(n_G, widest level), the largest over the blocks (DESIGN §6b's rule)"""
    return max(50 * kappa2(A[lo:hi, lo:hi]) * max(int(g), int(w)) * EPS for (lo, hi), g, w in zip(slices(A.shape[0], nb), n_g, max_level))


def kappa2(A):
    ev = np.linalg.eigvalsh(A.toarray() if sp.issparse(A) else A)
    return float(ev[-1] / ev[0])
