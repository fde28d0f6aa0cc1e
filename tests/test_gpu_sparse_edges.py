"""GPU suite (-m gpu) of the sparse kernels at the edges of their row-block partition: k_spmv_csr, the two-launch sparse PCG
(k_spmv_pcg / k_update_xr_blk / k_csrfold_start) and the device interior CG in both forms, on the synthetic matrices of
tests/sparse_synth.py. tests/test_sparse_edges_cpu.py asserts on the host that every matrix has the block shape it is
named for (row blocks of more than 256 / 512 rows, rows longer than the tile, more than 2048 blocks, XCDs without
blocks, ...), so each case below reaches the branch it was written for.

Bars:
  * apply: bit-identical to the oracle's CSC scatter product (the project's own bar for the SpMV).
  * sparse solvers: test_gpu_parity.assert_history against the oracle; every solve has oracle it <= 20 (asserted on the CPU:
    diag 13 / 2 with Jacobi, tridiag 19, arrow 4..5), so the tight branch applies: `it` equal, res_norm to 1e-8 (+1e-12 res_1).
    The three device forms (two-launch loop, generic loop, eager launches) must agree on `it`.
  * interior CG: per subdomain ||u - u*|| <= 2 κ_d reltol ||u*|| against SuperLU, κ_d from the construction. Both solves stop
    at a recurrence residual <= reltol ||b||, so ||u - u*|| <= ||A^-1|| ||r|| <= κ_d reltol ||u*||; the factor 2 leaves room
    for the gap between recurrence and true residual. The oracle's interior CG alone, measured on the CPU
    (test_oracle_interior_cg_on_the_sets): mixed 0 / 1.2e-8 / 0.011, longrow 0.0021, capped 7.3e-4, wide 0.18 times κ_d reltol.
    `capped` stops on maxiter = n_i = 8, not on the tolerance: its spectrum (8 equally spaced eigenvalues, κ = 1e3) is
    chosen so that the 8th CG step still ends within the bar (a geometric spectrum ends 2e-8 away in the oracle itself).
  * iteration counts (MI355_ICG_CHUNK=1, plain CG): the increase of interior_iterations() equals the oracle's largest
    count over the subdomains to +-1; exactly 8 for `capped`. The oracle restates the unpreconditioned iteration only, so
    runs with the diagonal preconditioner are held to the accuracy bar and to bitwise equality across chunk sizes.

Measured on an MI355X (figures printed by the tests before they assert):
  * apply: every case bit-identical; exact +0.0 in the empty rows of `holes`.
  * sparse solvers: `it` equal to the oracle and between the three loop forms in every solve (no iteration-count
    difference observed). Largest |res - res_oracle| / res_oracle over the entries above the 1e-12 res_1 floor:
    tridiag(9001) 2.5e-14, tridiag(800000) 1.9e-13, arrow(9000, 9000) 1.7e-13, the same in all three forms to two digits
    (bar 1e-8); Jacobi on diag 6e-16. The last entries of the diag solves (CG has ended: ~1e-13 res_1) are below the floor.
  * interior CG, err / (κ_d reltol), plain | diagonal Pl, identical in both forms: mixed 0 / 2.2e-9 / 0.0108 | 0 / 2.1e-9 /
    0.0108; longrow 0.00214 | 1.5e-8; capped 0.00258 | 7.9e-4; wide 0.18 | 0.18. interior_iterations at chunk 1: mixed 95,
    longrow 4, capped 8, wide 22 in both forms = the oracle's counts.
  * S * v on `mixed`: 6.1e-8 of reltol max|want| (bar 0.5).
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import sparse_synth as ss
from test_gpu_parity import RES_FLOOR, RES_RTOL, TIGHT_PREFIX, assert_history

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mats():
    return ss.apply_cases()


APPLY_CASES = [f"diag{n}" for n in (1, 1023, 1024, 1025, 5000, 8193, 16385)] + [f"tridiag{n}" for n in (3000, 9001, 800000)] + \
              [f"arrow5000_{m}" for m in (1023, 1024, 1025, 2048, 2049)] + ["arrow9000_9000", "odd_start", "holes"]


# ------------------------------------------------------------------ apply
@pytest.mark.parametrize("name", APPLY_CASES)
def test_apply_bit_exact(pkg, ctx, orc, mats, name):
    A = mats[name]
    n = A.shape[0]
    x = np.random.default_rng(5).standard_normal(n)
    op = pkg.api.SparseMatrixCSC(ctx, A)
    want = orc.csc_operator(A) * x
    got = op * x
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert np.array_equal(op * x, want)                                   # a second launch on the same operator


def test_apply_writes_exact_zeros_into_empty_rows(pkg, ctx, orc):
    A, live = ss.holes()
    n = A.shape[0]
    x = np.random.default_rng(6).standard_normal(n)
    out = np.full(n, np.nan)
    got = pkg.api.SparseMatrixCSC(ctx, A).apply(x, out=out)
    empty = np.ones(n, dtype=bool)
    empty[live] = False
    assert empty[:ss.HOLES_LEAD].all() and empty[-ss.HOLES_TRAIL:].all() and empty.sum() > ss.HOLES_INNER
    assert not np.isnan(got).any()
    assert np.all(got[empty] == 0.0) and not np.signbit(got[empty]).any()
    assert np.array_equal(got, orc.csc_operator(A) * x)


# ------------------------------------------------------------------ sparse solvers
FORMS = ("two-launch", "generic", "eager")


def run_form(form, ctx, monkeypatch, fn):
    """fn() under one of the three device forms of the sparse loop (MI355_NO_CSRFOLD is read per solve)"""
    if form == "generic":
        monkeypatch.setenv("MI355_NO_CSRFOLD", "1")
    elif form == "eager":
        ctx.set_chunk(0)
    try:
        return fn()
    finally:
        monkeypatch.delenv("MI355_NO_CSRFOLD", raising=False)
        ctx.set_chunk(8)


def history_margin(got, want):
    """the largest res_norm deviation in units of assert_history's bar 1e-8 res_k + 1e-12 res_1 (printed, not asserted)"""
    res, reso = got[2], want[2]
    m = min(res.size, reso.size)
    return float(np.max(np.abs(res[:m] - reso[:m]) / (RES_RTOL * reso[:m] + RES_FLOOR * reso[0]))) if m and reso[0] else 0.0


@pytest.mark.parametrize("name", ss.SOLVER_CASES)
def test_sparse_solvers_in_three_loop_forms(pkg, ctx, orc, mats, monkeypatch, name):
    api = pkg.api
    A = mats[name]
    n = A.shape[0]
    assert n > ss.FUSED_MAX_N                                             # otherwise the fused single-workgroup loop runs
    Ag, Ao = api.SparseMatrixCSC(ctx, A), orc.csc_operator(A)
    dg = A.diagonal()
    Mj, Mi = api.JacobiPreconditioner(ctx, dg), api.IdentityPreconditioner(ctx, n)
    Mjo, Mio = orc.jacobi_operator(dg), orc.identity_operator(n)
    b = ss.solver_rhs(n)
    worst = {}
    for x0 in (np.zeros(n), ss.solver_rhs(n, 1)):
        for maxit in (0, 1, 2):
            solves = (("cg", lambda: api.cg(Ag, b, x0.copy(), maxit=maxit), lambda: orc.cg(Ao, b, x0, maxit=maxit)),
                      ("jacobi", lambda: api.pcg(Ag, b, x0.copy(), Mj, maxit=maxit), lambda: orc.pcg(Ao, b, x0, Mjo, maxit=maxit)),
                      ("identity", lambda: api.pcg(Ag, b, x0.copy(), Mi, maxit=maxit), lambda: orc.pcg(Ao, b, x0, Mio, maxit=maxit)))
            for tag, dev, ref in solves:
                want = ref()                                              # once per solve, shared by the three forms
                assert want[1] <= TIGHT_PREFIX
                its = []
                for form in FORMS:
                    got = run_form(form, ctx, monkeypatch, dev)
                    its.append(got[1])
                    worst[(tag, form)] = max(worst.get((tag, form), 0.0), history_margin(got, want))
                    if got[1] != want[1]:
                        print(f"{name} {tag} {form} x0={'0' if not x0.any() else 'rand'} maxit={maxit}: it {got[1]} vs oracle {want[1]}")
                    assert_history(got, want)
                assert len(set(its)) == 1, (tag, maxit, its)
    for (tag, form), v in sorted(worst.items()):
        print(f"{name} {tag:8s} {form:10s} max |res - res_oracle| / bar = {v:.2e}")


@pytest.mark.parametrize("name", ["diag8193", "tridiag9001"])
def test_sparse_loop_start_up_edges(pkg, ctx, mats, monkeypatch, name):
    """b = 0 (tol = 0, res = 0) and an initial guess that has already converged: it == 1, no loop pass, x unchanged"""
    api = pkg.api
    A = mats[name]
    n = A.shape[0]
    Ag = api.SparseMatrixCSC(ctx, A)
    Mj = api.JacobiPreconditioner(ctx, A.diagonal())
    b = ss.solver_rhs(n)
    xs = spla.splu(sp.csc_matrix(A)).solve(b)
    assert np.linalg.norm(b - A @ xs) <= 1e-12 * np.linalg.norm(b)
    for form in FORMS:
        for solve in (lambda b_, x_: api.cg(Ag, b_, x_), lambda b_, x_: api.pcg(Ag, b_, x_, Mj)):
            x, it, res = run_form(form, ctx, monkeypatch, lambda: solve(np.zeros(n), np.zeros(n)))
            assert it == 1 and res.size == 1 and res[0] == 0.0 and not np.any(x), form
            x, it, res = run_form(form, ctx, monkeypatch, lambda: solve(b, xs.copy()))
            assert it == 1 and res.size == 1 and np.array_equal(x, xs), form
            assert res[0] <= 1e-7 * np.linalg.norm(b)


def test_sparse_loop_res_capacity(pkg, mats):
    """res_norm capacity smaller than `it` in the two-launch loop: MI_ERR_RES_CAPACITY after a completed solve"""
    api, L = pkg.api, pkg._lib.load()
    A = mats["tridiag9001"]
    n = A.shape[0]
    c3 = api.Context(0)
    Ag, Mj = api.SparseMatrixCSC(c3, A), api.JacobiPreconditioner(c3, A.diagonal())
    b = ss.solver_rhs(n)
    ref = api.pcg(Ag, b, np.zeros(n), Mj)
    assert ref[1] > 3
    x, res, it = np.zeros(n), np.zeros(3), C.c_int64()
    c3._mode_for(b, x)
    rc = L.mi_pcg(Ag._h, Mj._h, C.c_void_p(b.ctypes.data), C.c_void_p(x.ctypes.data), 0, 1e-7,
                  res.ctypes.data_as(C.POINTER(C.c_double)), 3, C.byref(it))
    assert rc == pkg._lib.MI_ERR_RES_CAPACITY and it.value == ref[1]
    assert np.array_equal(res, ref[2][:3]) and np.array_equal(x, ref[0])      # the solve itself completed
    with pytest.raises(api.BoundsError):
        pkg._lib.check(rc)
    again = api.pcg(Ag, b, np.zeros(n), Mj)                                    # the context is still usable
    assert again[1] == ref[1] and np.array_equal(again[0], ref[0])


# ------------------------------------------------------------------ interior CG
_sets = {}


def interior_case(orc, name):
    """(set, SuperLU solutions, oracle iteration counts) of one interior set: computed once, shared by every test"""
    if name not in _sets:
        s = ss.interior_sets((name,))[name]
        ustar, its = [], []
        for A, b in zip(s.A_II, s.b_I):
            if A.shape[0] == 0:
                ustar.append(np.zeros(0)); its.append(0)
                continue
            ustar.append(spla.splu(sp.csc_matrix(A)).solve(b))
            its.append(orc.interior_cg(A, b, s.reltol)[1])
        _sets[name] = (s, ustar, its)
    return _sets[name]


def make_op(pkg, ctx, monkeypatch, s, fused, chunk, precond):
    monkeypatch.setenv("MI355_ICG_FUSED", str(fused))                      # read when the operator is created
    monkeypatch.setenv("MI355_ICG_CHUNK", str(chunk))
    try:
        S = pkg.api.MatrixFreeLocalSchurs(ctx, s.A_II, s.A_IΓ, s.A_ΓΓ, s.gather_idx, s.node_Γ_cnt, None, reltol=s.reltol)
    finally:
        monkeypatch.delenv("MI355_ICG_FUSED")
        monkeypatch.delenv("MI355_ICG_CHUNK")
    S.interior_precond(precond)
    return S


@pytest.mark.parametrize("name", ["mixed", "longrow", "capped", "wide"])
def test_interior_cg_edges(pkg, ctx, orc, monkeypatch, name):
    s, ustar, its_o = interior_case(orc, name)
    off = np.concatenate([[0], np.cumsum(s.n_i)])
    b_I = np.concatenate(s.b_I)
    u0 = np.zeros(s.n_Γ)
    out = {}
    for fused in (0, 1):
        for precond in (None, "diagonal"):
            for chunk in (1, 7, 64):
                S = make_op(pkg, ctx, monkeypatch, s, fused, chunk, precond)
                before = S.interior_iterations()
                u = S.interior_solutions(u0, b_I)
                out[(fused, precond, chunk)] = (u, S.interior_iterations() - before)
    for (fused, precond, chunk), (u, iters) in out.items():
        key = (fused, precond, chunk)
        # converged subdomains are frozen: the extra iterations of a longer replay change nothing
        assert np.array_equal(u, out[(fused, precond, 1)][0]), key
        for d in range(len(s.n_i)):
            ud, want = u[off[d]:off[d + 1]], ustar[d]
            if not s.b_I[d].any():
                assert not np.any(ud), (key, d)                            # zero right-hand side (or empty interior): exact zeros
                continue
            err = np.linalg.norm(ud - want) / np.linalg.norm(want)
            if chunk == 1:
                print(f"{name}[{d}] fused={fused} precond={precond}: err / (kappa reltol) = {err / (s.kappa[d] * s.reltol):.3g}")
            assert err <= 2.0 * s.kappa[d] * s.reltol, (key, d, err)
        if chunk == 1 and precond is None:
            print(f"{name} fused={fused}: interior_iterations {iters}, oracle max {max(its_o)} (per subdomain {its_o})")
            assert abs(iters - max(its_o)) <= 1, (key, iters, its_o)
            if name == "capped":
                assert its_o == [8] and iters == 8, (key, iters)
        elif precond is None:
            assert iters % chunk == 0 and iters >= max(its_o) - 1, (key, iters)
    if name == "wide":
        # more than NT pieces: MI355_ICG_FUSED=1 must fall back to the three-launch form, bit for bit
        for precond in (None, "diagonal"):
            for chunk in (1, 7, 64):
                assert np.array_equal(out[(1, precond, chunk)][0], out[(0, precond, chunk)][0]), (precond, chunk)
                assert out[(1, precond, chunk)][1] == out[(0, precond, chunk)][1]
    if name == "mixed":
        assert ss.MIXED_ZERO_RHS == 1 and s.n_i == [1, 2, 300, 5000, 0]
        assert len(set(i for i, n in zip(its_o, s.n_i) if n and i)) == 3    # the others stop at three different iterations


def test_matrix_free_schur_apply_on_mixed(pkg, ctx, orc, monkeypatch):
    """One S * v on `mixed` against the dense Schur complement formed on the host (SuperLU), in both forms"""
    s, _, _ = interior_case(orc, "mixed")
    v = np.random.default_rng(23).standard_normal(s.n_Γ)
    want = np.zeros(s.n_Γ)
    for d, (A, G, GG) in enumerate(zip(s.A_II, s.A_IΓ, s.A_ΓΓ)):
        Sd = GG.toarray()
        if A.shape[0]:
            Sd = Sd - G.T @ spla.splu(sp.csc_matrix(A)).solve(G.toarray())
        want[s.gather_idx[d]] += Sd @ v[s.gather_idx[d]]
    for fused in (0, 1):
        got = make_op(pkg, ctx, monkeypatch, s, fused, 64, None) * v
        print(f"mixed S*v fused={fused}: max |got - want| / (reltol max|want|) = {np.abs(got - want).max() / (s.reltol * np.abs(want).max()):.3g}")
        assert np.abs(got - want).max() <= 0.5 * s.reltol * np.abs(want).max()
