"""GPU suite of the device smoothed-aggregation AMG preconditioner `api.AMGPreconditioner` (`mi_amg_create`, csrc/amg.hpp):
the reference's `AMGPreconditioner{SmoothedAggregation}` as the M of `pcg(A, b, 0, Π_amg)` (Example01:49-61). Applies
against the numpy restatement of the V(1,1) cycle (tests/amg_ref.py) at relative 2-norm 1e-12 — the device differs from it
by the rounding of the coarse GEMV's shuffle tree and nothing else that is known: eps x row length x levels x |smoother| is
of order 1e-14 — on the shapes where the row-block kernels can go wrong; the solvers against the restatement plus a numpy
pcg; symmetry, statistics, refusals, and non-finite input. tests/test_amg_cpu.py holds the restatement to its own bars."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import amg_ref as ar
from test_gpu_parity import RES_FLOOR, RES_RTOL, X_RTOL

pytestmark = pytest.mark.gpu

APPLY_BAR = 1e-12


def _rel(got, want):
    return np.linalg.norm(got - want) / np.linalg.norm(want)


def _rhs(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n), np.eye(n)[0], np.eye(n)[n // 3], np.eye(n)[n - 1]]


def _check_apply(pkg, ctx, H, tag, index_base=0):
    M = pkg.api.AMGPreconditioner(ctx, H, index_base=index_base)
    n = H.sizes[0]
    assert M.n == n
    outs = []
    for k, r in enumerate(_rhs(n, 5)):
        got, want = M.ldiv(r), ar.cycle(H, r)
        err = _rel(got, want)
        print(f"AMG apply {tag} levels {H.sizes} rhs {k}: rel. error {err:.3e} (bar {APPLY_BAR:.0e})")
        assert err <= APPLY_BAR, (tag, k, err)
        assert np.array_equal(M.ldiv(r), got) and np.array_equal(M * r, got)
        assert np.array_equal(pkg.api.apply_amg(M, r), got)
        outs.append(got)
    M.close()
    return outs


@pytest.fixture(scope="module")
def sys34(fem):
    return ar.system(fem, 34, "example01")


@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_apply_around_1024_rows(pkg, ctx, fem, sys34, n):
    """free-node counts 1023 / 1024 / 1025: N = 34 gives 32² = 1024 rows of the mesh itself; one row fewer or more by a
    synthetic SPD matrix of the same stencil"""
    A = sys34[0] if n == 1024 else ar.grid_like(n)
    assert A.shape[0] == n
    _check_apply(pkg, ctx, fem.prepare_amg_precond(A), f"n = {n}")


@pytest.mark.parametrize("N,kw,nlev", [(12, dict(max_levels=1), 1), (12, dict(max_levels=2, max_coarse=10), 2),
                                       (12, dict(max_levels=3, max_coarse=4), 3), (34, dict(max_levels=1), 1),
                                       (34, dict(max_levels=3, max_coarse=32), 3), (100, dict(), 3)])
def test_apply_by_number_of_levels(pkg, ctx, fem, N, kw, nlev):
    """nlevels 1 (the dense inverse alone: `A \\ b`), 2 and 3; N = 12: 100 rows, less than one workgroup; N = 100: the
    default hierarchy of the in-loop tests, many row blocks per level"""
    A, b = ar.system(fem, N, "example01")
    H = fem.prepare_amg_precond(A, **kw)
    assert H.nlevels == nlev
    outs = _check_apply(pkg, ctx, H, f"N = {N} {kw}")
    if nlev == 1:
        r = _rhs(A.shape[0], 5)[0]
        assert np.linalg.norm(A @ outs[0] - r) <= 1e-10 * np.linalg.norm(r)


def test_apply_with_a_giant_aggregate_and_one_based_arrays(pkg, ctx, fem):
    """a P whose rows hold a single entry and an R = P' row of 1100 entries, longer than SPMV_TILE (the tile-by-tile path of
    one row); then the same hierarchy and the N = 34 one through 1-based arrays: the same bits"""
    H = ar.giant_aggregate_hierarchy(fem)
    assert np.diff(sp.csr_matrix(H.P[0].T).indptr).max() > 1024 and np.diff(H.P[0].indptr).max() == 1
    z0 = _check_apply(pkg, ctx, H, "giant aggregate")
    z1 = _check_apply(pkg, ctx, H, "giant aggregate, 1-based", index_base=1)
    assert all(np.array_equal(a, b) for a, b in zip(z0, z1))
    H = fem.prepare_amg_precond(ar.system(fem, 34, "lognormal")[0])
    z0, z1 = _check_apply(pkg, ctx, H, "N = 34"), _check_apply(pkg, ctx, H, "N = 34, 1-based", index_base=1)
    assert all(np.array_equal(a, b) for a, b in zip(z0, z1))


def _assert_solve(got, want, tag):
    (x, it, res), (xo, ito, reso) = got[:3], want[:3]
    m = min(len(res), len(reso))
    print(f"{tag}: it = {it} (restatement {ito}), max rel. history difference {np.max(np.abs(res[:m] - reso[:m]) / reso[:m]):.3e}, "
          f"|x - x_ref| / |x_ref| = {_rel(x, xo):.3e}")
    assert it == ito, f"{tag}: iteration counts differ: {it} vs {ito}"
    assert np.allclose(res, reso, rtol=RES_RTOL, atol=RES_FLOOR * reso[0]), np.max(np.abs(res - reso) / reso)
    assert _rel(x, xo) <= X_RTOL


@pytest.mark.parametrize("N,coeff,cap", ar.LOOP_CASES)
def test_pcg_in_the_loop(pkg, ctx, fem, N, coeff, cap):
    """pcg(A, b, 0, Π_amg) against the restatement + numpy pcg: `it` equal, history within 1e-8 res_k + 1e-12 res_1; the
    eager solve (chunk 0) bit for bit the replayed one; defpcg, initpcg and eigdefpcg(spdim = 12) with 4 random columns and
    eigpcg(nvec = 4, spdim = 12) reach the tolerance. tests/test_amg_cpu.py asserts that the last two residuals of each case
    are 5 % away from the threshold."""
    api = pkg.api
    assert RES_RTOL == 1e-8 and RES_FLOOR == 1e-12
    A, b, H, want = ar.case(fem, N, coeff)
    n = b.size
    Ag, M = api.SparseMatrixCSC(ctx, A), api.AMGPreconditioner(ctx, H)
    x0 = np.zeros(n)
    got = api.pcg(Ag, b, x0, M)
    _assert_solve(got, want, f"pcg N = {N} {coeff}")
    assert got[1] <= cap
    try:
        ctx.set_chunk(0)
        eager = api.pcg(Ag, b, x0, M)
    finally:
        ctx.set_chunk(8)
    assert eager[1] == got[1] and np.array_equal(eager[0], got[0]) and np.array_equal(eager[2], got[2])
    tol = 1e-7 * np.linalg.norm(b)
    W = np.asfortranarray(np.random.default_rng(9).standard_normal((n, 4)))
    for name, out in (("defpcg", api.defpcg(Ag, b, x0, W, M)), ("eigpcg", api.eigpcg(Ag, b, x0, M, 4, 12)),
                      ("initpcg", api.initpcg(Ag, b, x0, M, W)), ("eigdefpcg", api.eigdefpcg(Ag, b, x0, M, W, 12))):
        x, it, res = out[:3]
        print(f"{name} N = {N} {coeff}: it = {it}, res / tol = {res[it - 1] / tol:.3f}")
        assert it <= 2 * cap and res[it - 1] <= tol
        assert np.linalg.norm(A @ x - b) <= 2 * tol
    M.close(); Ag.close()


def test_symmetry_on_the_device(pkg, ctx, fem):
    """u'Mv against v'Mu to 1e-12, and u'Mu > 0"""
    for N, coeff in ((40, "lognormal"), (100, "example01")):
        _, b, H, _ = ar.case(fem, N, coeff)
        M = pkg.api.AMGPreconditioner(ctx, H)
        rng = np.random.default_rng(3)
        for _ in range(3):
            u, v = rng.standard_normal((2, b.size))
            uMv, vMu = u @ M.ldiv(v), v @ M.ldiv(u)
            print(f"N = {N} {coeff}: |u'Mv - v'Mu| / |u'Mv| = {abs(uMv - vMu) / abs(uMv):.2e}")
            assert abs(uMv - vMu) <= 1e-12 * abs(uMv) and u @ M.ldiv(u) > 0
        M.close()


def _want_bytes(H):
    nc = H.sizes[-1]
    alg = 8 * nc * nc + 16 * nc
    kept = 8 * nc * nc
    for l in range(H.nlevels - 1):
        n, n1, a, p = H.sizes[l], H.sizes[l + 1], H.A[l].nnz, H.P[l].nnz
        alg += 2 * (12 * a + 4 * (n + 1)) + 24 * p + 4 * (n + 1) + 4 * (n1 + 1) + 88 * n + 16 * n1
        kept += 12 * a + 24 * p + 8 * n
    dom = 12 * H.A[0].nnz + 4 * (H.sizes[0] + 1) + 32 * H.sizes[0] if H.nlevels > 1 else alg
    return alg, dom, kept


def test_stats_and_bytes(pkg, ctx, fem):
    """mi_amg_stats equals the hierarchy's numbers; mi_op_bytes: two sweeps of every smoothed A_l, P_l and R_l once, 11 doubles
    per fine and 2 per coarse row of every level, the inverse (amg.hpp); dominant = the fine-level k_amg_down; a matrix goes
    through the host set-up with its options"""
    A, b = ar.system(fem, 40, "example01")
    for H in (ar.case(fem, 40, "example01")[2], ar.case(fem, 100, "lognormal")[2], fem.prepare_amg_precond(A, max_levels=1)):
        M = pkg.api.AMGPreconditioner(ctx, H)
        alg, dom, kept = _want_bytes(H)
        assert M.stats() == dict(n_levels=H.nlevels, coarse_n=H.sizes[-1], operator_nnz=H.operator_nnz, bytes_kept=kept)
        assert H.operator_nnz == round(H.operator_complexity * H.A[0].nnz)
        assert M.bytes() == (alg, dom)
        M.apply_dominant(b if H.sizes[0] == b.size else np.ones(H.sizes[0]))
        ctx.synchronize()
        M.close()
    M = pkg.api.AMGPreconditioner(ctx, A, max_levels=3, max_coarse=30)
    assert M.stats()["n_levels"] == 3 and M.hierarchy.nlevels == 3
    r = _rhs(b.size, 1)[0]
    assert _rel(M.ldiv(r), ar.cycle(M.hierarchy, r)) <= APPLY_BAR
    with pytest.raises(TypeError):
        pkg.api.AMGPreconditioner(ctx, M.hierarchy, max_levels=3)


def test_bad_arguments_are_refused(pkg, ctx, fem):
    """MI_ERR_BAD_ARG with a text: level sizes that do not chain, a P_l that is not n_l x n_{l+1}, a value that is not finite
    in A, P, ω/d or the inverse, nlevels < 1, a coarsest level above 4096 rows; a good create works right after each"""
    import copy
    api, L = pkg.api, pkg._lib
    H = ar.case(fem, 40, "example01")[2]
    r = _rhs(H.sizes[0], 2)[0]
    M = api.AMGPreconditioner(ctx, H)
    z0 = M.ldiv(r)
    M.close()

    def refused(Hb, *words):
        with pytest.raises(api.MiError) as e:
            api.AMGPreconditioner(ctx, Hb)
        msg = str(e.value)
        print("  refused:", msg)
        assert e.value.code == L.MI_ERR_BAD_ARG and len(msg) > 30 and all(w in msg for w in words), msg
        M = api.AMGPreconditioner(ctx, H)
        assert np.array_equal(M.ldiv(r), z0)
        M.close()

    n, nc = H.sizes
    Hb = copy.copy(H); Hb.sizes = [n, n]
    refused(Hb, "chain", str(n))
    Hb = copy.copy(H); Hb.sizes = [n, nc - 1]               # P_0 holds a column the next level does not have
    Hb.A = [H.A[0], H.A[1][:nc - 1, :nc - 1]]
    Hb.coarse_inv = np.asfortranarray(H.coarse_inv[:nc - 1, :nc - 1])
    refused(Hb, "P of level 0", f"{n} x {nc - 1}")
    for what, l in (("A", 0), ("A", 1), ("P", 0)):
        Hb = copy.copy(H)
        mats = [m.copy() for m in getattr(H, what)]
        mats[l].data[mats[l].nnz // 2] = np.nan if what == "A" else np.inf
        setattr(Hb, what, mats)
        refused(Hb, f"{what} of level {l}", "finite")
    Hb = copy.copy(H); Hb.omega_over_d = [H.omega_over_d[0].copy()]; Hb.omega_over_d[0][7] = np.nan
    refused(Hb, "omega_over_d", "finite")
    Hb = copy.copy(H); Hb.coarse_inv = H.coarse_inv.copy(order="F"); Hb.coarse_inv[1, 2] = -np.inf
    refused(Hb, "coarse_inv", "finite")
    big = 4097
    Hb = fem.AmgHierarchy([sp.identity(big, format="csr")], [], [], [], np.asfortranarray(np.eye(big)), [big], 1.0)
    refused(Hb, "4097", "4096")
    lib, h = L.load(), L.vp()
    for nlev in (0, -3):
        rc = lib.mi_amg_create(ctx._h, nlev, None, None, None, None, None, None, None, None, None, 0, C.byref(h))
        assert rc == L.MI_ERR_BAD_ARG and b"nlevels" in lib.mi_last_error() and not h.value
    one = np.array([5], dtype=np.int64)
    rc = lib.mi_amg_create(ctx._h, 1, one.ctypes.data_as(L.i64p), None, None, None, None, None, None, None, None, 0, C.byref(h))
    assert rc == L.MI_ERR_BAD_ARG and b"NULL" in lib.mi_last_error() and not h.value
    rc = lib.mi_amg_stats(None, None, None, None, None)
    assert rc == L.MI_ERR_BAD_ARG
    Aop = api.SparseMatrixCSC(ctx, H.A[0])
    a = L.i64()
    assert lib.mi_amg_stats(Aop._h, C.byref(a), None, None, None) == L.MI_ERR_BAD_ARG
    Aop.close()


def test_non_finite_input_leaves_no_trace(pkg, ctx, fem):
    """ldiv on a clean vector, on one with a NaN / Inf, on the clean one again: bit for bit (every level vector is rewritten by
    every apply); pcg(A, b_nan, 0, M) ends as the reference does — it = 1, res_norm = [nan] — between two clean solves that
    are bit-identical, replayed and eager, and equal to a solve on fresh handles in a fresh context"""
    api = pkg.api
    A, b, H, want = ar.case(fem, 40, "lognormal")
    n = b.size
    r = np.random.default_rng(41).standard_normal(n)
    Ag, M = api.SparseMatrixCSC(ctx, A), api.AMGPreconditioner(ctx, H)
    x0 = np.zeros(n)
    try:
        z0 = M.ldiv(r)
        assert _rel(z0, ar.cycle(H, r)) <= APPLY_BAR
        for val, at in ((np.nan, n // 2), (np.inf, 3), (np.nan, n - 1), (-np.inf, 0)):
            rb = r.copy()
            rb[at] = val
            assert not np.all(np.isfinite(M.ldiv(rb)))
            assert np.array_equal(M.ldiv(r), z0), (val, at)
        b_bad = b.copy()
        b_bad[n // 3] = np.nan
        xo, ito, reso = ar.pcg(A, b_bad, x0, lambda v: ar.cycle(H, v), maxit=20)
        assert ito == 1 and np.isnan(reso).all()
        by_chunk = {}
        for chunk in (4, 0):
            ctx.set_chunk(chunk)
            good = api.pcg(Ag, b, x0, M)
            if chunk == 4:
                _assert_solve(good, want, "clean solve")
            xb, itb, resb = api.pcg(Ag, b_bad, x0, M, 20)[:3]
            assert itb == 1 and resb.shape == (1,) and np.isnan(resb[0])
            again = api.pcg(Ag, b, x0, M)
            assert again[1] == good[1] and np.array_equal(again[0], good[0]) and np.array_equal(again[2], good[2]), chunk
            by_chunk[chunk] = good
        assert np.array_equal(by_chunk[0][0], by_chunk[4][0]) and np.array_equal(by_chunk[0][2], by_chunk[4][2])
        ctx.set_chunk(4)
        ctx2 = api.Context(0)
        try:
            ctx2.set_chunk(4)
            A2, M2 = api.SparseMatrixCSC(ctx2, A), api.AMGPreconditioner(ctx2, H)
            assert np.array_equal(M2.ldiv(r), z0)
            fresh = api.pcg(A2, b, x0, M2)
            assert fresh[1] == by_chunk[4][1] and np.array_equal(fresh[0], by_chunk[4][0]) and np.array_equal(fresh[2], by_chunk[4][2])
            M2.close(); A2.close()
        finally:
            ctx2.close()
    finally:
        ctx.set_chunk(8)
        M.close(); Ag.close()
