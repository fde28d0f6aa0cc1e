"""GPU suite (-m gpu): `mi_eigsolve` (csrc/lanczos.hpp, csrc/lanczos_kernels.hpp) through the C ABI against dense `eigh` of the
host matrix or pencil. Cases, inputs and the restatement's records: tests/lanczos_synth.py; the restatement itself and the
measuring functions: tests/lanczos_ref.py; tests/test_lanczos_cpu.py proves that the restatement meets the same bars.

Every call runs at tol = 1e-10 (absolute) with maxiter = 4 R_ref + 8, R_ref the restatement's restart count: a stagnating
device run fails instead of spinning. Bars, none of them taken from the code under test:
  values          |θ_i - λ_i| <= 10 tol    (an eigenvalue lies within the residual norm of a unit Ritz vector; 10 for rounding)
  residual        ||A x_i - θ_i B x_i|| in the B^-1 norm, computed on the host, <= 10 tol
  orthonormality  max |X' B X - I| <= max(100 O_ref, 1e-13), O_ref the restatement's (a missing second Gram-Schmidt pass shows
                  orders above that)
  subspace        sin of the largest principal angle to the eigh subspace <= 10 tol / gap (Davis-Kahan)
  counts          pcg / defpcg iteration counts with device pairs == with host pairs

Edges. Rows: a workgroup owns tiles of 1024 rows (two double2 per thread): n = 1024 is one workgroup, 1025 two, 4097 five with a
ragged tail; odd n ends in a double2 that is half padding. Columns: the loads of LZ_CT = 4 columns are issued together; every
active-column count 1 .. krylovdim occurs in the first window of every case, and the `tile` group makes the last group of a
full window 3, 4 and 1 columns wide (krylovdim = 11, 12, 13)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import lanczos_ref as lz
import lanczos_synth as syn
import lorasc_ref as lr
import test_gpu_lorasc as tlo
from conftest import lowest_eigvecs

pytestmark = pytest.mark.gpu

TOL = syn.TOL


# ------------------------------------------------------------------ operators
def _diag_op(api, ctx, values):
    """z = values .* r through mi_diag_create (as B: values = d; as B^-1: values = 1 / d)"""
    v = np.ascontiguousarray(values, dtype=np.float64)
    h = C.c_void_p()
    api.check(ctx._L.mi_diag_create(ctx._h, C.c_int64(v.size), v.ctypes.data_as(api.f64p), C.byref(h)))
    return api.Operator(ctx, h)


def synth_ops(api, ctx, prob):
    """(A, B, Binv device operators; A dense, B dense or None; v0)"""
    A, B, v0 = syn.problem(prob)
    ops = [api.SparseMatrixCSC(ctx, A), None, None]
    if B is not None:
        _, kind = syn.pencil_B(prob)
        if kind == "diag":
            d = B.diagonal()
            ops[1], ops[2] = _diag_op(api, ctx, d), _diag_op(api, ctx, 1.0 / d)
        else:
            ops[1], ops[2] = api.SparseMatrixCSC(ctx, B), api.SparseDirectPreconditioner(ctx, sp.csc_matrix(B))
    return ops, A.toarray(), None if B is None else B.toarray(), v0


def schur_ops(api, ctx, fem, P, prob):
    S, A_gg, v0 = syn.schur_inputs(fem, P, prob)
    ops = [api.LocalSchurs(ctx, P.Sd, P.sub.gather_idx, P.sub.node_Γ_cnt), None, None]
    if A_gg is not None:
        ops[1], ops[2] = api.SparseMatrixCSC(ctx, A_gg), api.SparseDirectPreconditioner(ctx, A_gg)
    return ops, S, None if A_gg is None else A_gg.toarray(), v0


def close(ops):
    for op in ops:
        if op is not None:
            op.close()


def solve(api, ops, c, v0, maxiter=None):
    A, B, Binv = ops
    kw = dict(which=c.which, krylovdim=c.krylovdim, tol=TOL, maxiter=c.maxiter if maxiter is None else maxiter, v0=v0)
    return api.eigsolve(A, c.nev, **kw) if B is None else api.geneigsolve(A, B, Binv, c.nev, **kw)


def check(c, got, Ad, Bd):
    vals, X, info = got
    lam, Xh = lz.dense_eigh(Ad, Bd)
    lw, Xw, gap = lz.wanted(lam, Xh, c.nev, c.which)
    verr = float(np.max(np.abs(vals - lw)))
    true = lz.true_residuals(Ad, Bd, vals, X)
    O = lz.ortho_defect(X, Bd)
    ang = lz.sin_largest_angle(X, Xw, Bd)
    o_bar = max(100 * c.O_ref, 1e-13)
    print(f"  {c.id}: restarts {info.numiter} (restatement {c.R_ref}, cap {c.maxiter}), applies {info.numops}, converged {info.converged}; "
          f"|θ-λ| {verr:.2e}, residual {true.max():.2e} (bars {10 * TOL:.0e}); orthonormality {O:.2e} (bar {o_bar:.1e}); "
          f"sin θ {ang:.2e} (bar {10 * TOL / gap:.2e})")
    assert np.all(np.isfinite(vals)) and np.all(np.isfinite(X))
    assert info.converged == c.nev and info.numiter <= c.maxiter
    assert np.all(info.normres <= TOL)
    assert verr <= 10 * TOL
    assert true.max() <= 10 * TOL
    assert O <= o_bar
    assert ang <= 10 * TOL / gap


SYNTH = [c for c in syn.CASES if c.group != "schur"]


@pytest.mark.parametrize("c", SYNTH, ids=[c.id for c in SYNTH])
def test_synthetic_cases_against_eigh(pkg, ctx, c):
    """rows, columns, SR / LR, the column tile, krylovdim below / at / above n, convergence in the first window, both B forms"""
    api = pkg.api
    ops, Ad, Bd, v0 = synth_ops(api, ctx, c.prob)
    try:
        got = solve(api, ops, c, v0)
        check(c, got, Ad, Bd)
        info = got[2]
        if c.group == "first":
            assert info.numiter == 0 and info.numops == c.krylovdim
        if c.group == "window" and c.krylovdim >= Ad.shape[0]:       # one exact window: n applies, no restart, nothing divided by the last beta
            assert info.numiter == 0 and info.numops == Ad.shape[0]
    finally:
        close(ops)


SCHUR = syn.group("schur")


@pytest.mark.parametrize("c", SCHUR, ids=[c.id for c in SCHUR])
def test_schur_operators_and_lorasc_pencil_against_eigh(pkg, ctx, fem, micro, toy, c):
    api = pkg.api
    P = {"micro": micro, "toy": toy}[c.prob[:-1]]
    ops, Ad, Bd, v0 = schur_ops(api, ctx, fem, P, c.prob)
    try:
        check(c, solve(api, ops, c, v0), Ad, Bd)
    finally:
        close(ops)


def test_eager_and_device_pointers_equal_the_replayed_call(pkg, ctx):
    """set_chunk(0) launches the same kernels eagerly; torch tensors select device pointers: bit for bit the host-pointer call"""
    import torch
    api = pkg.api
    for cid in ("cols-synth257-7-16-SR", "gen-gtri257-6-12-SR"):
        c = syn.BY_ID[cid]
        ops, _, _, v0 = synth_ops(api, ctx, c.prob)
        try:
            before = ctx.query("graph_replays")
            vals, X, info = solve(api, ops, c, v0)
            assert ctx.query("graph_replays") - before == info.numiter + 1           # one replay per window, none per step
            ctx.set_chunk(0)
            try:
                before = ctx.query("graph_replays")
                vals0, X0, info0 = solve(api, ops, c, v0)
                assert ctx.query("graph_replays") == before
            finally:
                ctx.set_chunk(8)
            assert np.array_equal(vals0, vals) and np.array_equal(X0, X) and info0.numiter == info.numiter
            vals1, X1, info1 = solve(api, ops, c, torch.from_numpy(v0).cuda())
            assert np.array_equal(vals1, vals) and np.array_equal(X1.cpu().numpy(), X) and info1.numops == info.numops
        finally:
            close(ops)


@pytest.mark.parametrize("maxiter", [0, 1])
def test_out_of_restarts_is_not_an_error(pkg, ctx, maxiter):
    """MI_OK with nconv < nev; Ritz values interlace (θ_i >= λ_i - 10 tol); resid is the true residual norm within a factor 2"""
    api = pkg.api
    c = syn.BY_ID["rows-synth257-6-12-SR"]
    ops, Ad, _, v0 = synth_ops(api, ctx, c.prob)
    try:
        vals, X, info = solve(api, ops, c, v0, maxiter=maxiter)
    finally:
        close(ops)
    lam = lz.dense_eigh(Ad)[0][:c.nev]
    true = lz.true_residuals(Ad, None, vals, X)
    print(f"  maxiter {maxiter}: converged {info.converged}, θ - λ {vals - lam}, resid / true {info.normres / true}")
    assert info.numiter == maxiter and info.converged < c.nev
    assert info.numops == c.krylovdim + maxiter * (c.krylovdim - min(c.nev + (c.krylovdim - c.nev) // 2, c.krylovdim - 1))
    assert np.all(vals >= lam - 10 * TOL)
    assert np.all(info.normres <= 2 * true) and np.all(true <= 2 * info.normres)
    assert lz.ortho_defect(X) <= 1e-13


@pytest.mark.parametrize("nev", syn.BREAKDOWN_NEV)
def test_breakdown(pkg, ctx, nev):
    """diag37, v0 = e0 + e5 + e9 (an eigenvector: d0 = d5 = d9 = 1). nev = 2 returns the two smallest of {d0, d5, d9}; nev = 4
    continues with fresh vectors: finite eigenvalues of the matrix, nconv = nev, true residuals at the bar"""
    api = pkg.api
    A, _, v0 = syn.problem("diag37")
    d = A.diagonal()
    op = api.SparseMatrixCSC(ctx, A)
    try:
        vals, X, info = api.eigsolve(op, nev, "SR", 0, TOL, 8, v0)
    finally:
        op.close()
    print(f"  breakdown nev {nev}: vals {vals}, normres {info.normres}, restarts {info.numiter}, applies {info.numops}")
    assert info.converged == nev and np.all(np.isfinite(vals)) and np.all(np.isfinite(X)) and np.all(np.isfinite(info.normres))
    assert all(np.min(np.abs(d - t)) <= 10 * TOL for t in vals)
    assert np.max(lz.true_residuals(A.toarray(), None, vals, X)) <= 10 * TOL
    assert lz.ortho_defect(X) <= 1e-13
    if nev == 2:
        assert np.allclose(vals, np.sort(d[[0, 5, 9]])[:2], rtol=0, atol=10 * TOL)


def test_lorasc_pairs_from_the_device_give_the_same_pcg_count(pkg, ctx, fem, toy):
    """fem.prepare_lorasc_precond(eigs = api.geneigsolve on (S, A_ΓΓ)) against its dense default on toy (no generalized
    eigenvalue below ε = 0.01: the nev = nvec fallback): E' A_ΓΓ E = I, the same Σ, and pcg(A, b, 0, ΠA_lorasc) takes the
    same number of iterations with either E"""
    api = pkg.api
    c = lr.make_case(fem, "toy", 100, 2, 2)
    cp = syn.BY_ID["schur-toyP-25-50-SR"]
    ops, S, A_gg, v0 = schur_ops(api, ctx, fem, toy, "toyP")
    assert np.array_equal(c.pos_Γ.shape, (S.shape[0],)) and abs(c.A_ΓΓ - sp.csc_matrix(A_gg)).max() == 0

    def eigs(k):
        vals, E, info = api.geneigsolve(*ops, k, "SR", krylovdim=2 * k, tol=TOL, maxiter=cp.maxiter, v0=v0)
        assert info.converged == k
        return vals, E
    try:
        E_dev, Σ_dev = fem.prepare_lorasc_precond(None, c.A_ΓΓ, eigs=eigs)
    finally:
        close(ops)
    E_host, Σ_host = fem.prepare_lorasc_precond(S, c.A_ΓΓ)
    assert E_dev.shape == E_host.shape == (S.shape[0], 25)
    assert np.max(np.abs(Σ_dev - Σ_host)) <= 10 * TOL
    assert lz.ortho_defect(E_dev, A_gg) <= max(100 * cp.O_ref, 1e-13)
    A = api.SparseMatrixCSC(ctx, c.A)
    M = tlo._device(pkg, ctx, c)
    try:
        its = []
        for E in (E_host, E_dev):
            M.set_correction(E, None)
            its.append(api.pcg(A, c.b, np.zeros(c.n), M)[1])
        M.set_correction(None)
        plain = api.pcg(A, c.b, np.zeros(c.n), M)[1]
    finally:
        M.close()
        A.close()
    print(f"  lorasc-pcg on toy: iterations with host pairs {its[0]}, with device pairs {its[1]}, without correction {plain}")
    assert its[0] == its[1] < plain


def test_deflation_basis_from_the_device_gives_the_same_defpcg_count(pkg, ctx, orc, toy):
    """Example03:206-214: W = the ndom + 10 least dominant eigenvectors of S; defpcg(S, b, 0, W, ΠSnn) takes the same number of
    iterations with the device W as with conftest.lowest_eigvecs (nev = 14 on toy: iteration counts only, lanczos_synth.py)"""
    api = pkg.api
    P, c = toy, syn.TOY_DEFLATION
    n = P.sub.n_Γ
    assert c.nev == P.sub.ndom + 10
    S = api.LocalSchurs(ctx, P.Sd, P.sub.gather_idx, P.sub.node_Γ_cnt)
    M = api.NeumannNeumannSchurPreconditioner(ctx, P.ΠSd, P.sub.gather_idx, P.sub.node_Γ_cnt)
    try:
        vals, W_dev, info = api.eigsolve(S, c.nev, "SR", c.krylovdim, TOL, c.maxiter, syn.schur_inputs(None, P, "toyS")[2])
        assert info.converged == c.nev
        W_host = lowest_eigvecs(orc.apply_local_schurs_operator(P.Sd, P.sub.gather_idx, n), n, c.nev)
        it_host = api.defpcg(S, P.b_schur, np.zeros(n), W_host, M)[1]
        it_dev = api.defpcg(S, P.b_schur, np.zeros(n), W_dev, M)[1]
        it_pcg = api.pcg(S, P.b_schur, np.zeros(n), M)[1]
    finally:
        M.close()
        S.close()
    print(f"  defpcg on toy: iterations with host W {it_host}, with device W {it_dev}, pcg {it_pcg}; restarts {info.numiter}")
    assert it_dev == it_host <= it_pcg


def test_poisoned_start_vector_leaves_no_trace(pkg, ctx):
    """v0 with one NaN: the error code of a non-finite state (MI_ERR_SINGULAR, as everywhere in the library); the good call that
    follows on the same handles returns bit for bit what it returns on fresh handles in a fresh context. Also NaN from the
    operator (a matrix entry), and v0 = 0."""
    api = pkg.api
    c = syn.BY_ID["cols-synth257-7-16-SR"]
    A, _, v0 = syn.problem(c.prob)
    bad = v0.copy()
    bad[100] = np.nan
    Abad = A.copy()
    Abad.data[Abad.data.size // 2] = np.nan
    op, opbad = api.SparseMatrixCSC(ctx, A), api.SparseMatrixCSC(ctx, Abad)
    try:
        good = solve(api, [op, None, None], c, v0)
        for o, v in ((op, bad), (op, np.zeros_like(v0)), (opbad, v0)):
            with pytest.raises(api.SingularException) as e:
                solve(api, [o, None, None], c, v)
            assert e.value.code == pkg._lib.MI_ERR_SINGULAR and "finite" in str(e.value)
            again = solve(api, [op, None, None], c, v0)
            assert np.array_equal(again[0], good[0]) and np.array_equal(again[1], good[1]) and again[2].numops == good[2].numops
    finally:
        op.close()
        opbad.close()
    ctx2 = api.Context(0)
    try:
        op2 = api.SparseMatrixCSC(ctx2, A)
        fresh = solve(api, [op2, None, None], c, v0)
        op2.close()
    finally:
        ctx2.close()
    assert np.array_equal(fresh[0], good[0]) and np.array_equal(fresh[1], good[1])


def test_bad_arguments(pkg, ctx):
    api, L = pkg.api, pkg._lib.load()
    BAD = pkg._lib.MI_ERR_BAD_ARG
    n = 257
    A, B, _ = syn.problem("gtri257")
    ops = [api.SparseMatrixCSC(ctx, A), api.SparseMatrixCSC(ctx, B), api.SparseDirectPreconditioner(ctx, sp.csc_matrix(B))]
    small = api.IdentityPreconditioner(ctx, n - 1)
    vals, vecs = np.empty(n), np.empty((n, n), order="F")
    out = [C.c_int64(), C.c_int64(), C.c_int64()]

    def call(a, b, binv, nev, which, kd, tol=TOL, maxiter=3, vals_p=vals.ctypes.data_as(api.f64p), vecs_p=C.c_void_p(vecs.ctypes.data)):
        h = lambda o: o._h if o is not None else None                           # noqa: E731
        return L.mi_eigsolve(h(a), h(b), h(binv), C.c_int64(nev), C.c_int(which), C.c_int64(kd), C.c_double(tol), C.c_int64(maxiter),
                             None, vals_p, vecs_p, None, *[C.byref(o) for o in out])
    try:
        a, b, bi = ops
        bad = {
            "nev < 1": (a, None, None, 0, 0, 0), "nev > n": (a, None, None, n + 1, 0, 0),
            "krylovdim == nev": (a, None, None, 6, 0, 6), "krylovdim < nev": (a, None, None, 6, 0, 3),
            "krylovdim < 0": (a, None, None, 6, 0, -1), "which": (a, None, None, 6, 2, 12),
            "B without Binv": (a, b, None, 6, 0, 12), "Binv without B": (a, None, bi, 6, 0, 12),
            "size of B": (a, small, bi, 6, 0, 12), "size of Binv": (a, b, small, 6, 0, 12),
            "window above 1024": (api.IdentityPreconditioner(ctx, 4096), None, None, 600, 0, 1500),
        }
        for name, args in bad.items():
            L.mi_ctx_set_pointer_mode(ctx._h, 0)
            assert call(*args) == BAD, name
            msg = L.mi_last_error().decode()
            print(f"  {name}: {msg}")
            assert msg.startswith("mi_eigsolve"), name
        assert call(a, None, None, 6, 0, 12, tol=-1.0) == BAD and L.mi_last_error()
        assert call(a, None, None, 6, 0, 12, maxiter=-1) == BAD and L.mi_last_error()
        assert call(a, None, None, 6, 0, 12, vals_p=None) == BAD and L.mi_last_error()
        assert call(a, None, None, 6, 0, 12, vecs_p=None) == BAD and L.mi_last_error()
        assert call(None, None, None, 6, 0, 12) == BAD and L.mi_last_error()
        # the edges that ARE valid: krylovdim = nev + 1; krylovdim = n with nev = n (clamped, one exact window)
        assert call(a, None, None, 6, 0, 7, maxiter=0) == 0
        assert call(a, None, None, n, 1, n) == 0 and out[0].value == n and out[1].value == 0 and out[2].value == n
        lam = np.linalg.eigvalsh(A.toarray())[::-1]
        assert np.max(np.abs(vals - lam)) <= 10 * TOL
    finally:
        close(ops + [small])
