"""GPU suite of the device block-Jacobi preconditioner `api.BlockJacobiPreconditioner` (`mi_block_jacobi_*`,
csrc/block_jacobi.hpp): the reference's `BJPreconditioner(nb, A)` as the M of pcg / defpcg / eigpcg on the full matrix.
Applies against the refined per-block solve (tests/block_jacobi_ref.py) at the project's bar for the device's exact
elimination against the host (relative 2-norm 1e-10); the edges of the new kernels with explicit seeds at
50 κ₂(B) m eps (DESIGN §6b's rule); the solvers against the oracle with the dense M^-1; reproducibility, new realizations,
the error returns and `mi_op_bytes`. tests/test_block_jacobi_cpu.py asserts on the host what these tests rely on."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import lognormal_coeff, lowest_eigvecs
from test_gpu_parity import RES_FLOOR, RES_RTOL, X_RTOL
import block_jacobi_ref as bjr
import lorasc_ref as lr
import sparse_synth

pytestmark = pytest.mark.gpu

APPLY_BAR = 1e-10
EPS = np.finfo(np.float64).eps
SOLVER_INPUTS = [("micro", 1), ("micro", 2), ("micro", 4), ("micro", 7), ("ragged", 3), ("ragged", 6)]


@pytest.fixture(scope="module")
def mats(fem):
    cs = lr.gpu_cases(fem, which=("micro", "ragged", "unstructured"))
    out = {k: (sp.csc_matrix(c.A), c.b) for k, c in cs.items()}
    out["tridiag"] = (sp.csc_matrix(sparse_synth.tridiag(300)), np.ones(300))
    return out


def _rhs(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n), np.eye(n)[0], np.eye(n)[n // 3], np.eye(n)[n - 1]]


def _rel(got, want):
    return np.linalg.norm(got - want) / np.linalg.norm(want)


@pytest.mark.parametrize("name,nbs", [("micro", (1, 2, 4, 7, "n")), ("ragged", (3, 6)), ("unstructured", (2, 3)), ("tridiag", (1,))])
def test_apply_against_refined_block_solves(pkg, ctx, mats, name, nbs):
    """random and unit right-hand sides: relative 2-norm error <= 1e-10 against the refined per-block solve; two applies
    bit-identical; host and device pointers bit-identical. nb = n: every block 1 x 1, no levels at all; the unstructured
    mesh: dozens of components per block, nearly every node a seed; tridiag: levels of width 1."""
    import torch
    A = mats[name][0]
    n = A.shape[0]
    for nb in nbs:
        nb = n if nb == "n" else nb
        M = pkg.api.BlockJacobiPreconditioner(ctx, nb, A)
        st = M.stats()
        want_shapes = bjr.shapes(A, nb)
        assert [(g, lv, w) for g, lv, w, _ in want_shapes] == list(zip(st["n_g"], st["n_levels"], st["max_level"]))
        ref = bjr.Ref(A, nb, 2)
        for k, r in enumerate(_rhs(n, nb)):
            got = M.ldiv(r)
            err = _rel(got, ref(r))
            print(f"block-Jacobi apply {name} nb = {nb} rhs {k}: rel. error {err:.3e} (bar {APPLY_BAR:.0e}, margin {APPLY_BAR / max(err, 1e-300):.1f}x)")
            assert err <= APPLY_BAR, (name, nb, k, err)
            assert np.array_equal(M.ldiv(r), got)
            assert np.array_equal(M.ldiv(torch.from_numpy(r).cuda()).cpu().numpy(), got)
        M.close()


def _edge_check(pkg, ctx, A, nb, seeds, tag):
    M = pkg.api.BlockJacobiPreconditioner(ctx, nb, A, seeds=seeds)
    st = M.stats()
    n = A.shape[0]
    ref = bjr.Ref(A, nb, 2)
    worst = bjr.edge_bar(A, nb, st["n_g"], st["max_level"])
    for k, r in enumerate(_rhs(n, 7)):
        err = _rel(M.ldiv(r), ref(r))
        print(f"block-Jacobi edge {tag} rhs {k}: rel. error {err:.3e} (bar {worst:.3e})")
        assert err <= worst, (tag, k, err, worst)
    return M, st


@pytest.mark.parametrize("ng,n0", bjr.EDGE_PAIRS)
def test_kernel_edges_of_gamma_and_level_zero(pkg, ctx, ng, n0):
    """n_G and the level-0 width around the 64-row tile and the 256-thread tail of k_bj_gamma / k_bj_back0, equal and
    unequal, a second level behind; bar 50 κ₂(B) m eps, m = max(n_G, widest level)"""
    A, seeds = bjr.edge_matrix(ng, n0)
    assert bjr.kappa2(A) <= 1e4
    M, st = _edge_check(pkg, ctx, A, 1, [seeds], f"n_G = {ng}, n_0 = {n0}")
    assert (st["n_g"][0], st["n_levels"][0], st["max_level"][0]) == (ng, 2, max(n0, 5))


def test_unequal_depth_and_single_level_blocks(pkg, ctx):
    """one operator with a block whose only level is level 0 beside a block of 5 levels (it idles in the early steps)"""
    A1, s1 = bjr.ladder_matrix([10], n_gamma=6, seed=1)
    A2, s2 = bjr.ladder_matrix([2, 2, 2, 2, 2], n_gamma=6, seed=2, degree=1)
    assert A1.shape == A2.shape == (16, 16)
    A = sp.block_diag([A1, A2], format="csc")
    M, st = _edge_check(pkg, ctx, A, 2, [s1, s2], "1 level beside 5")
    assert list(st["n_levels"]) == [1, 5]
    M1, st1 = _edge_check(pkg, ctx, A1, 1, [s1], "only level 0")
    assert list(st1["n_levels"]) == [1]


def test_size_limits_and_refusals(pkg, ctx, mats):
    """n_G = 2048 is accepted; n_G = 2049, a level of 2049, a seedless component, nb = 0 and nb = n + 1, a pattern that is
    not structurally symmetric: MI_ERR_BAD_ARG with a message that names the numbers"""
    api, L = pkg.api, pkg._lib
    A, seeds = bjr.ladder_matrix([4], n_gamma=2048, seed=3)
    M, st = _edge_check(pkg, ctx, A, 1, [seeds], "n_G = 2048")
    assert st["n_g"][0] == 2048

    def refused(*args, **kw):
        with pytest.raises(api.MiError) as e:
            api.BlockJacobiPreconditioner(ctx, *args, **kw)
        assert e.value.code == L.MI_ERR_BAD_ARG and len(str(e.value)) > 30
        return str(e.value)

    A, seeds = bjr.ladder_matrix([4], n_gamma=2049, seed=3)
    msg = refused(1, A, seeds=[seeds])
    assert "2049" in msg and "2048" in msg
    A, seeds = bjr.ladder_matrix([2049], n_gamma=4, seed=3)
    msg = refused(1, A, seeds=[seeds])
    assert "2049" in msg and "2048" in msg
    A1, s1 = bjr.ladder_matrix([10], n_gamma=6, seed=1)
    B = sp.block_diag([A1, A1], format="csc")             # one block, two components, seeds in the first only
    msg = refused(1, B, seeds=[s1])
    assert "no seed" in msg and "16" in msg
    Am = mats["micro"][0]
    n = Am.shape[0]
    assert "nb = 0" in refused(0, Am) and f"nb = {n + 1}" in refused(n + 1, Am)
    lib, i64p = L.load(), L.i64p                          # a seed_ptr that decreases, or does not start at index_base
    Ac = sp.csc_matrix(A1)
    ptr, idx = np.asarray(Ac.indptr, dtype=np.int64), np.asarray(Ac.indices, dtype=np.int64)
    for sq in ([0, 10, 5], [1, 3, 6]):
        sqa, sxa, h = np.asarray(sq, dtype=np.int64), np.arange(6, dtype=np.int64), L.vp()
        rc = lib.mi_block_jacobi_create(ctx._h, 16, ptr.ctypes.data_as(i64p), idx.ctypes.data_as(i64p), Ac.data.ctypes.data_as(L.f64p), 2,
                                        sqa.ctypes.data_as(i64p), sxa.ctypes.data_as(i64p), 0, L.C.byref(h))
        assert rc == L.MI_ERR_BAD_ARG and b"seed_ptr" in lib.mi_last_error() and not h.value
    U = sp.csc_matrix(Am + sp.csc_matrix(([1e-3], ([0], [n - 1])), shape=(n, n)))
    assert "symmetric" in refused(2, U)


def _assert_solve(got, want):
    x, it, res = got[:3]
    xo, ito, reso = want[:3]
    print(f"it = {it} (oracle {ito}), max rel. history difference {np.max(np.abs(res - reso[:len(res)]) / reso[:len(res)]):.3e}")
    assert it == ito, f"iteration counts differ: {it} vs oracle {ito}"
    assert np.allclose(res, reso, rtol=RES_RTOL, atol=RES_FLOOR * reso[0]), np.max(np.abs(res - reso) / reso)
    assert np.linalg.norm(x - xo) <= X_RTOL * np.linalg.norm(xo)


@pytest.mark.parametrize("name,nb", SOLVER_INPUTS)
def test_solvers_against_oracle(pkg, ctx, orc, mats, name, nb):
    """pcg, defpcg (the lowest 6 eigenvectors) and eigpcg on SparseMatrixCSC(A) with M = Π_bj against the oracle with the
    dense M^-1: `it` equal, history within 1e-8 res_k + 1e-12 res_1; nb = 1 is the exact solve: it == 2"""
    api = pkg.api
    A, b = mats[name]
    n = A.shape[0]
    assert RES_RTOL == 1e-8 and RES_FLOOR == 1e-12
    Minv = bjr.Ref(A, nb, 2).dense_minv()
    Mo = orc.neumann_neumann_operator([Minv], [np.arange(n)], np.ones(n, dtype=np.int64))
    Ao, Ag = orc.csc_operator(A), api.SparseMatrixCSC(ctx, A)
    M = api.BlockJacobiPreconditioner(ctx, nb, A)
    x0 = np.zeros(n)
    want = orc.pcg(Ao, b, x0, Mo)
    got = api.pcg(Ag, b, x0, M)
    _assert_solve(got, want)
    assert want[1] < 50 and (nb != 1 or got[1] == 2)
    ϕ = lowest_eigvecs(Ao, n, 6)
    _assert_solve(api.defpcg(Ag, b, x0, ϕ, M), orc.defpcg(Ao, b, x0, ϕ, Mo))
    _assert_solve(api.eigpcg(Ag, b, x0, M, 4, 10), orc.eigpcg(Ao, b, x0, Mo, 4, 10))


def test_eager_and_replayed_solves_are_bit_identical(pkg, ctx, mats):
    api = pkg.api
    A, b = mats["ragged"]
    Ag, M = api.SparseMatrixCSC(ctx, A), api.BlockJacobiPreconditioner(ctx, 3, A)
    x0 = np.zeros(A.shape[0])
    ctx.set_chunk(0)
    eager = api.pcg(Ag, b, x0, M)
    try:
        for chunk in (4, 8):
            ctx.set_chunk(chunk)
            r = api.pcg(Ag, b, x0, M)
            assert eager[1] == r[1] and np.array_equal(eager[0], r[0]) and np.array_equal(eager[2], r[2])
    finally:
        ctx.set_chunk(8)


def test_set_values_lifecycle(pkg, ctx, fem, mats):
    """a new realization == a fresh create, bit for bit (host and device values); an indefinite block is MI_ERR_SINGULAR and
    the old factor still applies, bit for bit; two live operators of different sizes side by side"""
    import torch
    api, L = pkg.api, pkg._lib
    A1 = mats["ragged"][0]
    c2 = lr.make_case(fem, "ragged2", 50, 3, 2, lognormal_coeff(fem, fem.get_mesh(50).points, 8))
    A2 = sp.csc_matrix(c2.A)
    assert np.array_equal(A1.indices, A2.indices) and not np.array_equal(A1.data, A2.data)
    n = A1.shape[0]
    r = np.random.default_rng(4).standard_normal(n)
    other = api.BlockJacobiPreconditioner(ctx, 4, mats["micro"][0])
    ro = np.random.default_rng(5).standard_normal(other.n)
    zo = other.ldiv(ro)
    fresh = api.BlockJacobiPreconditioner(ctx, 3, A2).ldiv(r)
    assert _rel(fresh, bjr.Ref(A2, 3, 2)(r)) <= APPLY_BAR
    M = api.BlockJacobiPreconditioner(ctx, 3, A1)
    before = M.ldiv(r)
    assert not np.array_equal(before, fresh)
    M.set_values(A2)
    assert np.array_equal(M.ldiv(r), fresh)
    M.set_values(torch.from_numpy(A1.data.copy()).cuda())
    assert np.array_equal(M.ldiv(r), before)
    # indefinite in the second block: one diagonal entry negated
    lo, hi = bjr.slices(n, 3)[1]
    bad, j = A1.copy(), lo + 7                            # (on the stored pattern: it holds explicit zeros)
    k = bad.indptr[j] + int(np.flatnonzero(bad.indices[bad.indptr[j]:bad.indptr[j + 1]] == j)[0])
    bad.data[k] = -bad.data[k]
    assert np.array_equal(bad.indices, A1.indices) and np.linalg.eigvalsh(bad[lo:hi, lo:hi].toarray())[0] < 0
    with pytest.raises(api.MiError) as e:
        M.set_values(bad)
    assert e.value.code == L.MI_ERR_SINGULAR, str(e.value)
    assert np.array_equal(M.ldiv(r), before)
    M.set_values(A2)                                      # and it still takes a new realization afterwards
    assert np.array_equal(M.ldiv(r), fresh)
    assert np.array_equal(other.ldiv(ro), zo)


def test_destroy_order_with_the_context(pkg, ctx, mats):
    """an operator closed before its context; one still alive when its context is closed and closed (then collected)
    afterwards; the shared context and a fresh one work on"""
    import gc
    api = pkg.api
    c2 = api.Context(0)
    A = mats["micro"][0]
    M1, M2 = api.BlockJacobiPreconditioner(c2, 2, A), api.BlockJacobiPreconditioner(c2, 7, A)
    r = np.ones(A.shape[0])
    z2 = M2.ldiv(r)
    assert np.isfinite(M1.ldiv(r)).all() and np.isfinite(z2).all()
    M1.close()
    assert np.array_equal(M2.ldiv(r), z2)
    c2.close()                                            # M2 outlives its context
    M2.close()
    del M2, c2
    gc.collect()
    M3 = api.BlockJacobiPreconditioner(ctx, 7, A)
    assert np.array_equal(M3.ldiv(r), z2)
    c3 = api.Context(0)
    assert np.array_equal(api.BlockJacobiPreconditioner(c3, 7, A).ldiv(r), z2)


@pytest.mark.parametrize("name,nb", [("micro", 1), ("micro", 7), ("unstructured", 3)])
def test_op_bytes(pkg, ctx, mats, name, nb):
    """mi_op_bytes: every kept inverse twice, S_G^-1 once, 10 doubles + 2 indices per level node, 5 doubles + 2 indices per
    seed (block_jacobi.hpp); dominant = the widest step's inverses"""
    A = mats[name][0]
    n = A.shape[0]
    M = pkg.api.BlockJacobiPreconditioner(ctx, nb, A)
    st = M.stats()
    n_g = int(st["n_g"].sum())
    n_i = n - n_g
    want = 2 * st["kept_bytes"] + 8 * int((st["n_g"].astype(np.int64) ** 2).sum()) + (10 * 8 + 2 * 4) * n_i + (5 * 8 + 2 * 4) * n_g
    a, d = M.bytes()
    assert a == want, (a, want)
    assert 0 <= d <= st["kept_bytes"] and (d > 0) == (st["n_levels"].max() > 0)
    if nb == 1:
        assert d == 8 * int(st["max_level"][0]) ** 2
