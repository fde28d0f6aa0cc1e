"""Synthetic inputs for the device Schur set-up (`mi_schur_setup_*`) and an extended-precision reference.

Not a conftest: test modules import it. Everything here runs on the host.

  ladder(...)         A_IIdd, A_IΓdd, A_ΓΓdd of one subdomain whose breadth-first levels from Γ have exactly the requested
                      widths, coupling degrees, in-level density and Γ couplings (SPD by diagonal dominance).
  direct_inverse(...) one level T = Q diag(λ) Q', B = I, A_ΓΓ = 2 ‖T^-1‖ I: S_d = A_ΓΓ - T^-1 shows the Gauss-Jordan inverse.
  refined_solve(...)  A^-1 R from SuperLU refined with long-double residuals (also the reference of tests/spd_graphs.py).
  reference(...)      S_d, w_d and A_II^-1 f from refined_solve, and κ(T_k) of every level.
  gj_emulate(...)     numpy copy of the device's blocked Gauss-Jordan inversion (64-wide pivot blocks inverted by 4 x 4
                      block steps with gj_inv4's arithmetic), to tell the algorithm's rounding from a kernel's.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

EPS = np.finfo(np.float64).eps


@dataclass
class Synth:
    A_II: sp.csc_matrix
    A_IΓ: sp.csc_matrix
    A_ΓΓ: sp.csc_matrix
    b_I: np.ndarray
    f: np.ndarray                       # a second interior right-hand side (interior_solve)
    widths: list = field(default_factory=list)   # the BFS level widths the generator promised (island excluded)
    tag: str = ""


def _csc(M, n, m):
    M = sp.csc_matrix(M, shape=(n, m))
    M.sum_duplicates()
    M.sort_indices()
    return M


def bfs_levels(A_II, A_IΓ):
    """The plan's breadth-first levels (setup_plan.hpp): seeds = rows of A_IΓ holding an entry, each level sorted."""
    A = sp.csr_matrix(A_II)
    seen = np.full(A.shape[0], -1)
    front = np.unique(sp.csc_matrix(A_IΓ).indices)
    seen[front] = 0
    levels = []
    while front.size:
        levels.append(front)
        nxt = set()
        for v in front:
            for u in A.indices[A.indptr[v]:A.indptr[v + 1]]:
                if seen[u] < 0:
                    seen[u] = len(levels)
                    nxt.add(int(u))
        front = np.array(sorted(nxt), dtype=np.int64)
    return levels


def ladder(widths, degree=3, density=0.0, n_gamma=8, gamma_deg=1, seed=0, contrast=1.0, shift=0.0, island=0, value_seed=None,
           tag=""):
    """One subdomain with BFS levels of exactly `widths` (level 0 = the nodes coupled to Γ).

    degree: level-k nodes each level-(k+1) node couples to (int, or a list to draw from per node, e.g. [1, 4, 5, 12]);
    density: probability of a coupling between two nodes of the same level; n_gamma / gamma_deg: size of Γ and Γ
    couplings per level-0 node; contrast: coupling weights are exp(U(-1, 1) log(contrast) / 2); shift: added to the
    diagonal of the diagonally dominant A_II (0: dominant only where Γ couplings are, conditioning grows with depth);
    island: size of an interior component that touches neither Γ nor the levels. `value_seed` redraws the values on the
    same sparsity (default: `seed`)."""
    rs = np.random.default_rng(seed)                             # structure
    rv = np.random.default_rng(seed + 7919 if value_seed is None else value_seed)   # values
    widths = [int(w) for w in widths]
    n_lev = sum(widths)
    n = n_lev + island
    off = np.concatenate(([0], np.cumsum(widths)))
    perm = rs.permutation(n)                                     # node number of (level order position)
    rows, cols = [], []

    def couple(a, b):
        rows.append(perm[a]); cols.append(perm[b])

    degs = np.atleast_1d(np.asarray(degree))
    for k in range(len(widths) - 1):
        for q in range(widths[k + 1]):
            d = int(rs.choice(degs)) if degs.size > 1 else int(degs[0])
            for p in rs.choice(widths[k], size=min(d, widths[k]), replace=False):
                couple(off[k + 1] + q, off[k] + p)
    for k, w in enumerate(widths):
        if density > 0 and w > 1:
            m = sp.random(w, w, density=density, random_state=rs.integers(2**31), format="coo")
            for a, b in zip(m.row, m.col):
                if a < b:
                    couple(off[k] + a, off[k] + b)
    for a in range(island - 1):                                  # a path: one connected island
        couple(n_lev + a, n_lev + a + 1)
    wts = np.exp(rv.uniform(-1, 1, len(rows)) * np.log(contrast) / 2) if rows else np.zeros(0)
    r = np.array(rows, dtype=np.int64); c = np.array(cols, dtype=np.int64)
    O = sp.coo_matrix((-wts, (r, c)), shape=(n, n)).tocsr()
    O = O + O.T
    O.sum_duplicates()
    # Γ couplings of level 0 (B = A_IΓ[L_0, :]): every level-0 node at least one
    gr, gc = [], []
    for q in range(widths[0] if widths else 0):
        for g in rs.choice(n_gamma, size=min(gamma_deg, n_gamma), replace=False):
            gr.append(perm[q]); gc.append(g)
    gw = np.exp(rv.uniform(-1, 1, len(gr)) * np.log(contrast) / 2)
    B = _csc(sp.coo_matrix((-gw, (gr, gc)), shape=(n, n_gamma)), n, n_gamma)
    absrow = np.asarray(abs(O).sum(axis=1)).ravel() + np.asarray(abs(B).sum(axis=1)).ravel()
    diag = absrow + shift * (np.mean(wts) if wts.size else 1.0)
    if island:
        diag[perm[n_lev:]] += 1.0
    A_II = _csc(O + sp.diags(diag), n, n)
    gdiag = np.asarray(abs(B).sum(axis=0)).ravel() + 1.0
    A_ΓΓ = _csc(sp.diags(gdiag) + sp.diags(-0.1 * np.ones(max(0, n_gamma - 1)), 1) + sp.diags(-0.1 * np.ones(max(0, n_gamma - 1)), -1),
                n_gamma, n_gamma)
    s = Synth(A_II, B, A_ΓΓ, rv.standard_normal(n), rv.standard_normal(n), widths, tag or f"ladder{widths}")
    got = [len(l) for l in bfs_levels(A_II, B)]
    assert got == widths, (got, widths)
    return s


def orthogonal(n, seed):
    return np.linalg.qr(np.random.default_rng(seed).standard_normal((n, n)))[0]


def direct_inverse(n0, kappa, seed=None):
    """One level, T = A_II = Q diag(geomspace(1, κ)) Q' dense, B = I (interior node i -> Γ node i), A_ΓΓ = 2 ‖T^-1‖ I = 2 I:
    S_d = A_ΓΓ - T^-1."""
    Q = orthogonal(n0, n0 if seed is None else seed)
    lam = np.geomspace(1.0, kappa, n0) if n0 > 1 else np.array([1.0])
    T = (Q * lam) @ Q.T
    T = (T + T.T) / 2
    rv = np.random.default_rng(n0 + 17)
    return Synth(_csc(T, n0, n0), _csc(sp.identity(n0), n0, n0), _csc(2.0 * sp.identity(n0), n0, n0), rv.standard_normal(n0),
                 rv.standard_normal(n0), [n0], f"direct n0={n0} κ={kappa:g}")


def empty_interior(n_gamma=5, seed=3):
    rv = np.random.default_rng(seed)
    G = rv.standard_normal((n_gamma, n_gamma))
    G = G + G.T + 2 * n_gamma * np.eye(n_gamma)
    return Synth(_csc(sp.csc_matrix((0, 0)), 0, 0), _csc(sp.csc_matrix((0, n_gamma)), 0, n_gamma), _csc(G, n_gamma, n_gamma),
                 np.zeros(0), np.zeros(0), [], "n_I = 0")


def refined_solve(A, R, max_it=8):
    """A^-1 R (R dense, columns) by SuperLU in float64, refined with residuals in long double until the correction is below
    1e-18 relative (or stops shrinking). Returns long-double columns."""
    lu = spla.splu(sp.csc_matrix(A), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=1.0)
    Al = sp.csr_matrix(A).astype(np.longdouble)
    Rl = np.asarray(R, dtype=np.longdouble)
    X = lu.solve(np.asarray(R, dtype=np.float64)).astype(np.longdouble)
    last = np.inf
    for _ in range(max_it):
        r = Rl - Al @ X
        d = lu.solve(np.asarray(r, dtype=np.float64)).astype(np.longdouble)
        X = X + d
        rel = float(np.max(np.abs(d)) / max(np.max(np.abs(X)), 1e-300))
        if rel < 1e-18 or rel >= last:
            break
        last = rel
    return X


def level_kappas(s: Synth):
    """κ(T_k) for every level of the float64 level recursion T_m = A_mm, T_k = A_kk - C_k' T_{k+1}^-1 C_k (host, eigvalsh)."""
    levels = bfs_levels(s.A_II, s.A_IΓ)
    A = sp.csr_matrix(s.A_II)
    ks = []
    T = None
    for k in range(len(levels) - 1, -1, -1):
        Akk = A[levels[k]][:, levels[k]].toarray()
        if T is not None:
            Ck = A[levels[k + 1]][:, levels[k]].toarray()
            Akk = Akk - Ck.T @ np.linalg.solve(T, Ck)
        T = (Akk + Akk.T) / 2
        ev = np.linalg.eigvalsh(T)
        ks.append(float(ev[-1] / ev[0]) if ev[0] > 0 else np.inf)
    return ks[::-1]                                              # index = level


@dataclass
class Ref:
    S: np.ndarray               # A_ΓΓ - A_IΓ' A_II^-1 A_IΓ (float64 of the long-double result)
    S_scale: float              # max |A_IΓ' A_II^-1 A_IΓ|
    w: np.ndarray
    u: np.ndarray               # A_II^-1 f (every interior node, island included)
    kappa: float                # largest κ(T_k)
    nmax: int                   # largest level width
    kappas: list


def reference(s: Synth) -> Ref:
    nI, nG = s.A_IΓ.shape
    Gd = s.A_ΓΓ.toarray()
    if nI == 0:
        return Ref(Gd.copy(), 0.0, np.zeros(nG), np.zeros(0), 1.0, 0, [])
    B = s.A_IΓ.toarray()
    X = refined_solve(s.A_II, np.column_stack([B, s.b_I, s.f]))
    Bl = B.astype(np.longdouble)
    BX = Bl.T @ X[:, :nG]
    S = Gd.astype(np.longdouble) - BX
    ks = level_kappas(s)
    return Ref(np.asarray(S, dtype=np.float64), float(np.max(np.abs(BX))) if nG else 0.0,
               np.asarray(Bl.T @ X[:, nG], dtype=np.float64), np.asarray(X[:, nG + 1], dtype=np.float64),
               max(ks) if ks else 1.0, max(s.widths) if s.widths else 0, ks)


def bar(ref: Ref, C=50.0):
    """The accuracy bar err / scale <= C κ_max n eps of one subdomain (n: its largest level width)."""
    return C * ref.kappa * max(ref.nmax, 1) * EPS


def split_blocks(Sd, sizes):
    out, off = [], 0
    for n in sizes:
        out.append(np.asarray(Sd[off:off + n * n]).reshape(n, n).T)
        off += n * n
    return out


def split_vec(v, sizes):
    out, off = [], 0
    for n in sizes:
        out.append(np.asarray(v[off:off + n]))
        off += n
    return out


# ---------------------------------------------------------------- numpy copy of the device's Gauss-Jordan inversion
def gj_inv4(m):
    """gj_inv4 (setup_gj.hpp): 4 x 4 inverse by the 2 x 2 block formula with explicit 2 x 2 inverses."""
    m = np.asarray(m, dtype=np.float64).reshape(4, 4)
    da = 1.0 / (m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0])
    Ai = np.array([[m[1, 1] * da, -m[0, 1] * da], [-m[1, 0] * da, m[0, 0] * da]])
    X = Ai @ m[:2, 2:]
    V = m[2:, :2] @ Ai
    S = m[2:, 2:] - m[2:, :2] @ X
    ds = 1.0 / (S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0])
    Si = np.array([[S[1, 1] * ds, -S[0, 1] * ds], [-S[1, 0] * ds, S[0, 0] * ds]])
    P = np.empty((4, 4))
    P[:2, :2] = Ai + X @ (Si @ V)
    P[:2, 2:] = -(X @ Si)
    P[2:, :2] = -(Si @ V)
    P[2:, 2:] = Si
    return P


def _gj_steps(M, b, inv):
    """Block Gauss-Jordan without pivoting, pivot blocks of b rows inverted by `inv`: the update of k_gj_update /
    gj_invert_block64 (row panel P A_Kj, column panel -A_iK P, trailing A_ij - A_iK (P A_Kj), pivot block P)."""
    M = np.array(M, dtype=np.float64)
    n = M.shape[0]
    for k0 in range(0, n, b):
        K = slice(k0, min(n, k0 + b))
        bs = K.stop - k0
        Mb = np.eye(b)
        Mb[:bs, :bs] = M[K, K]
        P = inv(Mb)[:bs, :bs]
        R = P @ M[K, :]
        R[:, K] = P
        D = M.copy()
        D[:, K] = 0.0
        D = D - M[:, K] @ R
        D[K, :] = R
        M = D
    return M


def gj_emulate(T, mirror_pivots=False):
    """The device's inversion of an SPD T: 64-wide pivot blocks, each inverted by 4 x 4 block steps (gj_inv4).
    `mirror_pivots`: replace the lower triangle of every pivot inverse by the upper one (what the kernels did before)."""
    def inv64(Mb):
        P = _gj_steps(Mb, 4, gj_inv4)
        return np.triu(P) + np.triu(P, 1).T if mirror_pivots else P
    return _gj_steps(T, 64, inv64)
