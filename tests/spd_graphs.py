"""Sparse SPD test matrices for the sparse direct preconditioner (csrc/spd_direct*.hpp): chains, a star, a disconnected
pair, a grid Laplacian, the A_ΓΓ of FEM problems, and a graph whose separator is too large. Shared by
tests/test_spd_direct_cpu.py and tests/test_gpu_spd_direct.py.

For tests/test_spd_direct_edges_cpu.py and tests/test_gpu_spd_direct_edges.py also:
  edge_cases()        matrices at the edges of the piece size P and of the separator size |Σ| (the LDS / step-per-launch
                      branches of s^-1, the limit, an orphan Σ node, single-node pieces, pieces without Σ neighbours, n = 0)
                      with the shape each is named for; the CPU suite asserts every shape with the host plan checker.
  spd_kappa(...)      a family with a prescribed condition number on a given pattern (small margin, or D A D scaling).
  reference(...)      A^-1 R from SuperLU refined with long-double residuals (setup_synth.refined_solve).
  dissection_copy()   fp64 numpy restatement of the device algorithm in the device's order: what the algorithm itself loses."""
import numpy as np
import scipy.linalg
import scipy.sparse as sp

import setup_synth as ss

EPS = np.finfo(np.float64).eps
P_MAX, SIGMA_MAX = 128, 2048


def spd_from_graph(G, seed=0):
    """SPD matrix on the pattern of G (+ diagonal): random negative couplings, diagonal = row sum + a random margin."""
    G = sp.csr_matrix(G)
    n = G.shape[0]
    rng = np.random.default_rng(seed)
    U = sp.triu(G, 1).tocoo()
    w = rng.uniform(0.5, 1.5, U.nnz)
    off = sp.coo_matrix((-w, (U.row, U.col)), shape=(n, n))
    off = (off + off.T).tocsr()
    d = -np.asarray(off.sum(axis=1)).ravel() + rng.uniform(0.1, 1.0, n)
    A = (off + sp.diags(d)).tocsc()
    A.sort_indices()
    return A


def chain(n):
    return sp.diags([np.ones(n - 1), np.ones(n - 1)], [-1, 1], shape=(n, n)) if n > 1 else sp.csr_matrix((1, 1))


def star(leaves):
    n = leaves + 1
    r = np.zeros(leaves, dtype=np.int64)
    c = np.arange(1, n)
    G = sp.coo_matrix((np.ones(leaves), (r, c)), shape=(n, n))
    return G + G.T


def grid(m):
    c = chain(m)
    return sp.kron(sp.identity(m), c) + sp.kron(c, sp.identity(m))


def disconnected_pair():
    return sp.block_diag([chain(40), grid(9)])


def random_dense_graph(n, deg, seed=3):
    """An expander-like random graph: no small separator (|Σ| far above the limit for n = 6000, deg = 12)."""
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(n), deg // 2)
    c = rng.integers(0, n, r.size)
    keep = r != c
    G = sp.coo_matrix((np.ones(keep.sum()), (r[keep], c[keep])), shape=(n, n)).tocsr()
    G = G + G.T
    G.data[:] = 1.0
    return G


def synthetic_cases():
    """name -> SPD scipy CSC matrix"""
    out = {}
    for n in (1, 63, 64, 65, 1000):
        out[f"chain{n}"] = spd_from_graph(chain(n), n)
    out["star"] = spd_from_graph(star(150), 5)
    out["pair"] = spd_from_graph(disconnected_pair(), 6)
    out["grid30"] = spd_from_graph(grid(30), 7)
    return out


def global_gg(fem, mesh, epart, sub, coeff, f, uexact):
    """A_ΓΓ of `prepare_global_schur` (EPDD.jl:212-369), CSC"""
    A = fem.prepare_global_schur(mesh.cells, mesh.points, epart, sub, coeff, f, uexact)[2]
    A = sp.csc_matrix(A)
    A.sort_indices()
    return A


def write_graph(path, A):
    A = sp.csc_matrix(A)
    A.sort_indices()
    with open(path, "w") as fh:
        fh.write(f"{A.shape[0]} {A.nnz}\n")
        fh.write(" ".join(map(str, A.indptr)) + "\n")
        fh.write(" ".join(map(str, A.indices)) + "\n")


def dissection_solve(A, piece_of, r):
    """z = A \\ r by the three formulas of the plan (dense numpy): y = D^-1 r_P, z_Σ = s^-1 (r_Σ - B y), z_P = y - D^-1 B' z_Σ."""
    A = sp.csr_matrix(A)
    piece_of = np.asarray(piece_of)
    Pn, Sn = np.flatnonzero(piece_of >= 0), np.flatnonzero(piece_of < 0)
    D = A[Pn][:, Pn].toarray()
    assert np.all(D[piece_of[Pn][:, None] != piece_of[Pn][None, :]] == 0)     # D is block diagonal over the pieces
    B = A[Sn][:, Pn].toarray()
    Ass = A[Sn][:, Sn].toarray()
    y = np.linalg.solve(D, r[Pn]) if Pn.size else np.zeros(0)
    s = Ass - B @ np.linalg.solve(D, B.T) if Pn.size else Ass
    zs = np.linalg.solve(s, r[Sn] - B @ y) if Sn.size else np.zeros(0)
    z = np.empty_like(r)
    z[Sn] = zs
    if Pn.size:
        z[Pn] = y - np.linalg.solve(D, B.T @ zs)
    return z


# ---------------------------------------------------------------- edges of the piece size and of the separator size
def strip(width, length):
    """`width` chains of `length` nodes joined rung by rung (a ladder for width = 2): node = row + width * position"""
    return sp.kron(chain(length), sp.identity(width)) + sp.kron(sp.identity(length), chain(width))


def spider():
    """hub 0, arms 1..3, two leaves per arm: at P = 1 the cover takes the hub and the arms, the leaves are the pieces, and
    the hub has no piece next to it (an orphan Σ node)"""
    e = [(0, 1), (0, 2), (0, 3), (1, 4), (1, 5), (2, 6), (2, 7), (3, 8), (3, 9)]
    r, c = np.array(e).T
    G = sp.coo_matrix((np.ones(len(e)), (r, c)), shape=(10, 10))
    return G + G.T


def empty():
    return sp.csc_matrix((0, 0))


def _spd(G, seed):
    G = sp.csc_matrix(G)
    return spd_from_graph(G, seed) if G.shape[0] else sp.csc_matrix((0, 0), dtype=np.float64)


def edge_cases():
    """name -> (SPD CSC matrix, P, shape). `shape`: what tests/cpp/spd_direct_check.cpp reports at that P (status, pieces,
    sigma, and orphans / single-node pieces / pieces without Σ neighbours where the case is about them); every entry is
    asserted by tests/test_spd_direct_edges_cpu.py. status 2 = SIGMA_TOO_LARGE (the library's MI_ERR_BAD_ARG)."""
    out = {}

    def add(name, G, P, seed, **shape):
        out[name] = (_spd(G, seed), P, dict({"status": 0}, **shape))

    # |Σ| around 88 | 89 (sd_lds_bytes: from 89 on k_sd_invert needs more than the 64 KiB of LDS a kernel gets without
    # hipFuncSetAttribute), 90 | 91 and 128 | 129 (LDS kernel | one launch per step); a chain at P = 4 splits into pieces
    # of 3 nodes and single separator nodes: tridiagonal s
    for n, ns in ((356, 88), (360, 89), (364, 90), (365, 91), (512, 127), (516, 128), (517, 129)):
        add(f"chain{n}_P4", chain(n), 4, n, pieces=ns + 1, sigma=ns)
    # the same edges (and |Σ| = 100, between them) with an s that is not tridiagonal: strips of width 3 and 4 at P = 8
    for w, L, ns, npc in ((3, 86, 90, 33), (3, 87, 91, 33), (4, 68, 100, 34), (3, 123, 128, 46), (4, 87, 129, 44)):
        add(f"strip{w}x{L}_P8", strip(w, L), 8, 20 + L, pieces=npc, sigma=ns)
    add("grid40_P64", grid(40), 64, 40, pieces=27, sigma=253)
    add("chain4097_P1", chain(4097), 1, 41, pieces=2049, sigma=2048, singles=2049)
    add("chain4099_P1", chain(4099), 1, 42, status=2, sigma=2049)
    add("spider_P1", spider(), 1, 43, pieces=6, sigma=4, orphans=1)
    add("grid16_P128", grid(16), 128, 16, pieces=2, sigma=16)
    add("grid16_P100", grid(16), 100, 16, pieces=3, sigma=21)
    add("grid8_P1", grid(8), 1, 8, pieces=32, sigma=32, singles=32)
    add("star150_P64", star(150), 64, 5, pieces=88, sigma=1, singles=87)
    add("three_chains_P64", sp.block_diag([chain(10), chain(64), chain(1)]), 64, 44, pieces=3, sigma=0, isolated=3)
    add("chain10_grid9_P64", sp.block_diag([chain(10), grid(9)]), 64, 45, pieces=3, sigma=7, isolated=1)
    add("n0_P64", empty(), 64, 0, pieces=0, sigma=0)
    add("n1_P64", chain(1), 64, 1, pieces=1, sigma=0, isolated=1)
    return out



# ---------------------------------------------------------------- a prescribed condition number on a given pattern
KAPPAS = (1e2, 1e4, 1e6, 1e8, 1e10)


def kappa2(A):
    """κ_2 of a symmetric positive definite matrix: dense eigvalsh, or the tridiagonal solver where A is tridiagonal"""
    A = sp.csc_matrix(A)
    if A.shape[0] == 0:
        return 1.0
    C = A.tocoo()
    if A.shape[0] > 1 and np.all(np.abs(C.row - C.col) <= 1):
        ev = scipy.linalg.eigvalsh_tridiagonal(A.diagonal(), A.diagonal(1))
    else:
        ev = np.linalg.eigvalsh(A.toarray())
    return float(ev[-1] / ev[0]) if ev[0] > 0 else np.inf


def spd_kappa(G, kappa, seed=0, kind="margin"):
    """SPD matrix on the pattern of G (+ diagonal) with κ_2 close to `kappa` (within a factor 3; callers assert it).

    kind "margin":  the weighted graph Laplacian L of spd_from_graph (λ_min = 0 on a connected graph) plus a diagonal
                    margin δ u_i, u_i in [0.7, 1.3], δ = λ_max(L) / κ: λ_min lies in [0.7 δ, 1.3 δ].
    kind "scaling": D A D with A = spd_from_graph(G) (κ of order 10..100) and D = diag(exp(σ v_i)), v_i in [-1, 1]
                    fixed by the seed; σ is found by bisection on the dense κ_2 (κ_2 grows with σ)."""
    G = sp.csr_matrix(G)
    n = G.shape[0]
    rng = np.random.default_rng(seed)
    if kind == "margin":
        U = sp.triu(G, 1).tocoo()
        w = rng.uniform(0.5, 1.5, U.nnz)
        off = sp.coo_matrix((-w, (U.row, U.col)), shape=(n, n))
        off = (off + off.T).tocsr()
        lap = -np.asarray(off.sum(axis=1)).ravel()
        lmax = np.linalg.eigvalsh((off + sp.diags(lap)).toarray())[-1]
        A = (off + sp.diags(lap + lmax / kappa * rng.uniform(0.7, 1.3, n))).tocsc()
    elif kind == "scaling":
        A0 = spd_from_graph(G, seed)
        v = rng.uniform(-1.0, 1.0, n)

        def scaled(sig):
            d = np.exp(sig * v)
            A = A0.copy()
            A.data = A0.data * d[A0.indices] * np.repeat(d, np.diff(A0.indptr))
            return A

        lo, hi = 0.0, 0.25 * np.log(kappa)                 # κ(D)^2 = exp(4 σ): start where the scaling alone gives κ
        while kappa2(scaled(hi)) < kappa:
            lo, hi = hi, 1.5 * hi
        for _ in range(40):                                # κ within 30 % of the target is enough
            mid = 0.5 * (lo + hi)
            k = kappa2(scaled(mid))
            if max(k / kappa, kappa / k) <= 1.3:
                break
            lo, hi = (mid, hi) if k < kappa else (lo, mid)
        A = scaled(mid)
    else:
        raise ValueError(kind)
    A = sp.csc_matrix(A)
    A.sort_indices()
    return A


# ---------------------------------------------------------------- reference and the numpy copy of the device algorithm
def reference(A, R=None):
    """A^-1 R (default R = I: the whole inverse) from SuperLU refined with long-double residuals, as float64"""
    n = A.shape[0]
    if n == 0:
        return np.zeros((0, 0) if R is None else np.shape(R))
    R = np.eye(n) if R is None else np.asarray(R, dtype=np.float64)
    X = ss.refined_solve(sp.csc_matrix(A), R.reshape(n, -1))
    return np.asarray(X, dtype=np.float64).reshape(R.shape)


def gj_inverse(M):
    """sd_gj_lds / k_sd_gj_step (spd_direct.hpp): in-place inverse by scalar Gauss-Jordan without pivoting. Returns
    (inverse, ok); ok is the kernels' pivot test, every pivot finite and above n eps times its original diagonal entry."""
    M = np.array(M, dtype=np.float64)
    n = M.shape[0]
    dg = M.diagonal().copy()
    ok = True
    for k in range(n):
        p = M[k, k]
        ok = ok and bool(np.isfinite(p) and p > n * EPS * dg[k])
        ip = 1.0 / p
        row, col = M[k, :].copy(), M[:, k].copy()
        rk = row * ip
        M -= np.outer(col, rk)
        M[k, :] = rk
        M[:, k] = -col * ip
        M[k, k] = ip
    return M, ok


def probe_sign(n):
    j = np.arange(n, dtype=np.uint64)
    return np.where((j * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF) & np.uint64(0x10000), 1.0, -1.0)


def certificate(s, Z):
    """(probe residual, bar) of the certificate of s^-1: ||v - Z (s v)||_inf against 4 |Σ| eps ||Z||_inf ||s||_inf, v = ±1"""
    n = s.shape[0]
    v = probe_sign(n)
    res = float(np.max(np.abs(v - Z @ (s @ v)))) if n else 0.0
    return res, 4.0 * n * EPS * float(np.abs(s).sum(axis=1).max(initial=0.0)) * float(np.abs(Z).sum(axis=1).max(initial=0.0))


def split_of(plan):
    """(list of the pieces' node arrays in piece order, Σ nodes) from a node -> piece map (the checker's `piece_of`, or
    its whole result)"""
    piece_of = np.asarray(plan["piece_of"] if isinstance(plan, dict) else plan, dtype=np.int64)
    npc = int(piece_of.max(initial=-1)) + 1
    return [np.flatnonzero(piece_of == i) for i in range(npc)], np.flatnonzero(piece_of < 0)


def dissection_copy(A, plan, r, info=None):
    """z = A \\ r as the device computes it (spd_direct.hpp), in fp64 numpy and in the device's order: D_i^-1 and s^-1 by
    unpivoted scalar Gauss-Jordan, G_i = D_i^-1 B_i', patch_i = B_i G_i, s = A_ΣΣ - (the patches summed in ascending
    piece order), then y_i = D_i^-1 r_i, t = r_Σ - Σ G_i' r_i (ascending piece), z_Σ = s^-1 t, z_i = y_i - G_i z_Σi.
    `r`: a vector or a matrix of columns (the identity gives the whole inverse). `info`, a dict, receives `pivots_ok`
    (the kernels' pivot test) and `certificate` = (probe residual, bar). Not bitwise the device: the dot products inside
    a step are numpy's. It measures what the algorithm loses; it is not a bar for correctness."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    pieces, Sn = split_of(plan)
    r = np.asarray(r, dtype=np.float64)
    if n == 0:
        return np.zeros_like(r)
    R = r.reshape(n, -1)
    ns = Sn.size
    where = np.full(n, -1)
    where[Sn] = np.arange(ns)
    s = A[Sn][:, Sn].toarray()
    acc = np.zeros((ns, ns))
    fac, ok = [], True
    for nodes in pieces:
        Bt = A[nodes].tocsc()[:, Sn]                               # B_i' restricted to Σ, n_i x |Σ|
        si = np.unique(Bt.tocoo().col)                             # Σ_i by structure (stored entries), ascending
        Bt = Bt[:, si].toarray()
        Dinv, good = gj_inverse(A[nodes][:, nodes].toarray())
        ok = ok and good
        Gi = Dinv @ Bt
        acc[np.ix_(si, si)] += Bt.T @ Gi
        fac.append((nodes, si, Dinv, Gi))
    s = s - acc
    Z, good = gj_inverse(s) if ns else (s, True)
    if info is not None:
        info["pivots_ok"] = bool(ok and good)
        info["certificate"] = certificate(s, Z)
        info["s"], info["Z"] = s, Z
    z = np.zeros_like(R)
    t = R[Sn].copy()
    ys = []
    for nodes, si, Dinv, Gi in fac:
        ys.append(Dinv @ R[nodes])
        t[si] -= Gi.T @ R[nodes]
    zs = Z @ t
    z[Sn] = zs
    for (nodes, si, Dinv, Gi), y in zip(fac, ys):
        z[nodes] = y - Gi @ zs[si]
    return z.reshape(r.shape)


# ---------------------------------------------------------------- what the CPU and the GPU edge suites share
def sd_lds_bytes(m):
    """dynamic LDS of k_sd_factor / k_sd_invert for an m x m block (spd_direct.hpp): m x (m + 1) doubles and three vectors"""
    return 8 * (m * (m + 1) + 3 * m)


def rhs_of(n, seed=11):
    """the right-hand sides of the accuracy checks: every unit vector for n <= 300 (the whole inverse), else 4 random columns"""
    return np.eye(n) if n <= 300 else np.random.default_rng(seed).standard_normal((n, 4))


# graphs of the κ ladder: name -> (graph, P). grid(16): |Σ| = 16 at P = 64; the chains: |Σ| = 128 | 129 at P = 4, a
# tridiagonal s; the strip: |Σ| = 128 with an s that is not
LADDER_GRAPHS = {"grid16": (grid(16), 64), "chain516": (chain(516), 4), "chain517": (chain(517), 4), "strip3x123": (strip(3, 123), 8)}


def inclusions(points, contrast):
    """a two-valued coefficient: `contrast` inside four discs, 1 outside"""
    x, y = points
    inc = np.zeros(x.shape, dtype=bool)
    for cx, cy, r in ((0.3, 0.3, 0.12), (0.7, 0.55, 0.15), (0.35, 0.75, 0.1), (0.62, 0.2, 0.08)):
        inc |= (x - cx) ** 2 + (y - cy) ** 2 <= r * r
    return np.where(inc, float(contrast), 1.0)


def ragged_gg(fem, f, uexact, contrast):
    """A_ΓΓ of the `ragged` problem (N = 50, 3 x 2 boxes) with the inclusions coefficient"""
    mesh = fem.get_mesh(50)
    epart, npart = fem.mesh_partition(mesh, 3, 2)
    d = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
    sub = fem.set_subdomains(mesh.cells, mesh.cell_neighbors, epart, npart, d.dirichlet_g2l)
    return global_gg(fem, mesh, epart, sub, inclusions(mesh.points, contrast), f, uexact)
