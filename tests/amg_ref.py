"""numpy restatement of the smoothed-aggregation V-cycle on a `fem.AmgHierarchy`, the reference of the AMG
tests: one pre- and one post-sweep of Jacobi damped by ω_l, the coarsest level by its dense inverse. Also the numpy `pcg`
(cg.jl:67-109) the in-loop tests compare with, the test systems, and synthetic hierarchies for the kernels' edges.
tests/test_amg_cpu.py holds this file and the set-up to their bars; the GPU tests compare against it."""
import numpy as np
import scipy.sparse as sp

from conftest import a_example01, f_m1, lognormal_coeff, u3

EPS = 1e-7


def cycle(H, b, l=0):
    """M^-1 b: the V(1,1) cycle from level l"""
    if l == H.nlevels - 1:
        return H.coarse_inv @ b
    A, P, wd = H.A[l], H.P[l], H.omega_over_d[l]
    x = wd * b                               # pre-smoothing from x = 0
    r = b - A @ x
    e = cycle(H, P.T @ r, l + 1)
    x = x + P @ e
    return x + wd * (b - A @ x)              # post-smoothing


def dense_minv(H):
    n = H.sizes[0]
    return np.column_stack([cycle(H, e) for e in np.eye(n)])


def pcg(A, b, x, M, maxit=0, eps=EPS):
    """cg.jl:67-109 in numpy; M: r -> z. Returns (x, it, res_norm[:it])."""
    n = b.size
    x = np.array(x, dtype=np.float64)
    maxit = maxit or n
    it = 1
    r = b - A @ x
    rTr = r @ r
    z = M(r)
    rTz = r @ z
    p = z.copy()
    res = [np.sqrt(rTr)]
    tol = eps * np.linalg.norm(b)
    while it < maxit and res[-1] > tol:
        Ap = A @ p
        α = rTz / (p @ Ap)
        β = 1.0 / rTz
        x += α * p
        r -= α * Ap
        rTr = r @ r
        z = M(r)
        rTz = r @ z
        β *= rTz
        p = z + β * p
        it += 1
        res.append(np.sqrt(rTr))
    return x, it, np.asarray(res)


def system(fem, N, coeff):
    """(A, b) of the Example01 flow on the N x N mesh; coeff: "example01" (0.1 + 1e-4 x y) or "lognormal"
    (synthetic_kl, default_rng(481456))"""
    mesh = fem.get_mesh(N)
    d = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
    a = a_example01 if coeff == "example01" else lognormal_coeff(fem, mesh.points)
    A, b = fem.do_isotropic_elliptic_assembly(mesh.cells, mesh.points, d, mesh.point_marker, a, f_m1, u3)
    return sp.csr_matrix(A), b


# the in-loop cases and the caps on `it` of the restatement (prototype's counts plus two)
LOOP_CASES = [(100, "example01", 16), (100, "lognormal", 16), (40, "example01", 13), (40, "lognormal", 11)]

_cache = {}


def case(fem, N, coeff):
    """(A, b, hierarchy, restatement's pcg result), computed once per session"""
    key = (N, coeff)
    if key not in _cache:
        A, b = system(fem, N, coeff)
        H = fem.prepare_amg_precond(A)
        _cache[key] = (A, b, H, pcg(A, b, np.zeros(b.size), lambda r: cycle(H, r)))
    return _cache[key]


def grid_like(n, seed=0):
    """An SPD matrix of exactly n rows from the mesh's 7-point stencil pattern: the N x N-grid matrix of at least n rows cut
    to its leading n x n block (a principal submatrix of an SPD matrix), values jittered symmetrically by a few per cent."""
    m = int(np.ceil(np.sqrt(n)))
    idx = np.arange(m * m).reshape(m, m)
    I, J = [], []
    for di, dj in ((0, 1), (1, 0), (1, 1)):
        a, b = idx[:m - di, :m - dj].ravel(), idx[di:, dj:].ravel()
        I += [a, b]; J += [b, a]
    I, J = np.concatenate(I), np.concatenate(J)
    rng = np.random.default_rng(seed)
    w = sp.coo_matrix((np.ones(I.size), (I, J)), shape=(m * m, m * m)).tocsr()
    w = sp.triu(w, 1).tocsr()
    w.data = 1.0 + 0.05 * rng.random(w.nnz)
    w = w + w.T
    L = sp.diags(np.asarray(w.sum(axis=1)).ravel() + 0.05) - w
    return sp.csr_matrix(sp.csr_matrix(L)[:n, :n])


def giant_aggregate_hierarchy(fem, n=1500, seed=3):
    """A two-level hierarchy whose first aggregate holds more than SPMV_TILE = 1024 nodes — the row of R = P' for it is
    longer than a tile — and whose P has rows of a single entry: an unsmoothed (tentative) prolongator on an SPD matrix.
    Built by hand in the form prepare_amg_precond leaves."""
    A = grid_like(n, seed)
    big = 1100
    agg = np.concatenate((np.zeros(big, dtype=np.int64), 1 + (np.arange(n - big) // 8)))
    nc = int(agg.max()) + 1
    cnt = np.bincount(agg, minlength=nc).astype(np.float64)
    P = sp.csr_matrix((1.0 / np.sqrt(cnt[agg]), (np.arange(n), agg)), shape=(n, nc))
    d = A.diagonal()
    g = float(np.max(np.asarray(abs(A).sum(axis=1)).ravel() / d))
    w = 4.0 / (3.0 * g)
    M = (P.T @ A @ P).tocsr()
    Ac = sp.csr_matrix((M + M.T) * 0.5)
    Ac.sort_indices()
    D = Ac.toarray()
    inv = np.linalg.inv((D + D.T) * 0.5)
    inv = np.asfortranarray((inv + inv.T) * 0.5)
    return fem.AmgHierarchy([A, Ac], [P], [w], [w / d], inv, [n, nc], float(A.nnz + Ac.nnz) / A.nnz)
