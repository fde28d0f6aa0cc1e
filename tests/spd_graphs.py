"""Sparse SPD test matrices for the sparse direct preconditioner (csrc/spd_direct*.hpp): chains, a star, a disconnected
pair, a grid Laplacian, the A_ΓΓ of FEM problems, and a graph whose separator is too large. Shared by
tests/test_spd_direct_cpu.py and tests/test_gpu_spd_direct.py."""
import numpy as np
import scipy.sparse as sp


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
