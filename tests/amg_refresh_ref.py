"""What the tests of the device AMG refresh share (tests/test_amg_refresh_cpu.py, tests/test_gpu_amg_refresh.py): the matrix
pairs (A0 = `example01`, A1 = lognormal, one mesh), the frozen aggregates of the synthetic cases, the level-local bounds of
the numeric chain, and the restatement's solves, computed once per session."""
import numpy as np
import scipy.sparse as sp

import amg_ref as ar

U = 2.0 ** -52

_pairs, _solves = {}, {}


def pair(fem, N):
    """(A0, A1, b1): the `example01` and the lognormal matrix of the N x N mesh in sorted CSR, and the lognormal right-hand side"""
    if N not in _pairs:
        A0, _ = ar.system(fem, N, "example01")
        A1, b1 = ar.system(fem, N, "lognormal")
        for M in (A0, A1):
            M.sum_duplicates(); M.sort_indices()
        assert np.array_equal(A0.indptr, A1.indptr) and np.array_equal(A0.indices, A1.indices)
        _pairs[N] = (A0, A1, b1)
    return _pairs[N]


def synthetic_pair(n):
    """two SPD matrices on the pattern of ar.grid_like(n): different jitter seeds"""
    A0, A1 = ar.grid_like(n, 0), ar.grid_like(n, 7)
    for M in (A0, A1):
        M.sum_duplicates(); M.sort_indices()
    assert np.array_equal(A0.indices, A1.indices)
    return A0, A1


def giant_aggregates(fem):
    """(A0, A1, [agg]) of ar.giant_aggregate_hierarchy: the first aggregate holds 1100 nodes, the others 8"""
    H = ar.giant_aggregate_hierarchy(fem)
    P = sp.csr_matrix(H.P[0])
    assert np.diff(P.indptr).max() == 1
    A0, A1 = synthetic_pair(H.sizes[0])
    return A0, A1, [P.indices.astype(np.int64)]


def refreshed_solve(fem, N):
    """(H1, (x, it, res)): fem.amg_refresh on the aggregates of A0 for A1, and the restatement's pcg(A1, b1, 0, cycle(H1))"""
    if N not in _solves:
        A0, A1, b1 = pair(fem, N)
        H1 = fem.amg_refresh(fem.prepare_amg_precond(A0), A1)
        _solves[N] = (H1, ar.pcg(A1, b1, np.zeros(b1.size), lambda r: ar.cycle(H1, r)))
    return _solves[N]


def ones(M):
    M = sp.csr_matrix(M)
    return sp.csr_matrix((np.ones(M.indices.size), M.indices.copy(), M.indptr.copy()), shape=M.shape)


def tentative(agg, nc):
    cnt = np.bincount(agg, minlength=nc).astype(np.float64)
    return sp.csr_matrix((1.0 / np.sqrt(cnt[agg]), (np.arange(agg.size), agg)), shape=(agg.size, nc))


def keys(M):
    return np.repeat(np.arange(M.shape[0], dtype=np.int64), np.diff(M.indptr)) * M.shape[1] + M.indices


def on_pattern(V, S):
    """the values of V at the stored entries of S (sorted CSR, in storage order), 0 where V stores nothing; every stored
    entry of V must be one of S"""
    V, S = sp.csr_matrix(V), sp.csr_matrix(S)
    V.sum_duplicates(); V.sort_indices()
    assert S.has_sorted_indices
    kv, ks = keys(V), keys(S)
    pos = np.searchsorted(ks, kv)
    assert pos.size == 0 or (pos.max() < ks.size and np.array_equal(ks[pos], kv)), "an entry outside the pattern"
    out = np.zeros(ks.size)
    out[pos] = V.data
    return out


def level_bounds(Al, P, agg):
    """The host's own numbers of one level from the level's own A_l (and, for the product, the given P_l), with the entry-wise
    bounds of the numeric chain; kA, kR the longest rows of A_l and R_l = P_l':
      g, ω/d   relative (kA + 2) u
      P        (kA + 4) u (|T| + |wd| |A_l| |T|)
      A_{l+1}  (kR + kA + 4) u (|P|' |A_l| |P|),   against sym(P' A_l P)"""
    Al, P = sp.csr_matrix(Al), sp.csr_matrix(P)
    n, nc = P.shape
    kA, kR = int(np.diff(Al.indptr).max()), int(np.diff(sp.csr_matrix(P.T).indptr).max())
    d = Al.diagonal()
    g = float(np.max(np.asarray(abs(Al).sum(axis=1)).ravel() / d))
    w = 4.0 / (3.0 * g)
    wd = w / d
    T = tentative(agg, nc)
    Ph = sp.csr_matrix(T - sp.diags(wd) @ (Al @ T))
    Pb = sp.csr_matrix((kA + 4) * U * (abs(T) + sp.diags(abs(wd)) @ (abs(Al) @ abs(T))))
    M = sp.csr_matrix(P.T @ Al @ P)
    Gb = sp.csr_matrix((kR + kA + 4) * U * (abs(P).T @ abs(Al) @ abs(P)))
    return dict(kA=kA, kR=kR, g=g, omega=w, wd=wd, rel=(kA + 2) * U, P=Ph, P_bound=Pb, G=sp.csr_matrix((M + M.T) * 0.5), G_bound=Gb)


def check_levels(H, aggs, tag):
    """every smoothed level of a hierarchy read back from the device within `level_bounds`; prints the fractions used"""
    for l in range(H.nlevels - 1):
        Al, P, An = H.A[l], H.P[l], H.A[l + 1]
        B = level_bounds(Al, P, aggs[l])
        g_dev = 4.0 / (3.0 * H.omega[l])
        e_w, e_g = abs(H.omega[l] - B["omega"]) / B["omega"], abs(g_dev - B["g"]) / B["g"]
        e_wd = np.max(np.abs(H.omega_over_d[l] - B["wd"]) / np.abs(B["wd"]))
        dP = np.abs(P.data - on_pattern(B["P"], P))
        bP = on_pattern(B["P_bound"], P)
        dA = np.abs(An.data - on_pattern(B["G"], An))
        bA = on_pattern(B["G_bound"], An)
        use = lambda d, b: np.max(np.divide(d, b, out=np.zeros_like(d), where=b > 0), initial=0.0)
        print(f"{tag} level {l}: n = {Al.shape[0]}, kA = {B['kA']}, kR = {B['kR']}; ω rel. {e_w:.2e}, g rel. {e_g:.2e}, ω/d rel. {e_wd:.2e} "
              f"(bar {B['rel']:.2e}); P: {use(dP, bP):.3f} of its bound; A_{l + 1}: {use(dA, bA):.3f} of its bound")
        assert e_w <= B["rel"] and e_g <= B["rel"] and e_wd <= B["rel"], (tag, l)
        assert (dP <= bP).all(), (tag, l, "P")
        assert (dA <= bA).all(), (tag, l, "A_next")
        assert abs(An - An.T).max() == 0.0, (tag, l, "A_next is not exactly symmetric")


def check_coarse(H, tag):
    """the coarse inverse read back against numpy's of the device's own A_L: ||I - Z A||_F <= 8 ||I - Z_np A||_F + n_c u"""
    Ac = H.A[-1].toarray()
    nc = Ac.shape[0]
    Zn = np.linalg.inv((Ac + Ac.T) * 0.5)
    Zn = (Zn + Zn.T) * 0.5
    r_dev, r_np = np.linalg.norm(np.eye(nc) - H.coarse_inv @ Ac), np.linalg.norm(np.eye(nc) - Zn @ Ac)
    print(f"{tag} coarse inverse: n_c = {nc}, cond = {np.linalg.cond(Ac):.1f}, ||I - Z A||_F device {r_dev:.3e}, numpy {r_np:.3e}, "
          f"ratio {r_dev / r_np:.2f}")
    assert np.array_equal(H.coarse_inv, H.coarse_inv.T)
    assert r_dev <= 8 * r_np + nc * U, (tag, r_dev, r_np)
