"""GPU suite (-m gpu): handle lifetime — borrowed operators, reused addresses, old graphs (DESIGN.md "Who remembers whom").

A solver graph is keyed by the addresses of A and M and bakes in the launch arguments of every operator nested inside M; a
full-assembly plan remembers the operator it has checked; a combined operator and a LORASC operator apply operators they
do not own; freed device blocks and freed host objects are handed out again, so a new handle regularly lives where an old
one died. Each test closes, refreshes or releases one side of such a relation and requires the other side to behave like
handles created in a NEW context on the same inputs ("fresh"): return codes, error texts and `np.array_equal` only.

No test reads a device pointer: each is valid whether or not an address recurs.

  1  FullAssemblyPlan.update after the checked operator was closed and another took its place
  2  pcg / defpcg / eigpcg after A, M or both were closed and replaced by operators of the same size
  3  two operator pairs of one size interleaved on the shared SolverWorkspace, through a drop of all its graphs
  4  mi_op_destroy of a child under live combinations (raw handles)
  5  a child refreshed under a combination whose solve graphs are captured: set_coupling, set_correction, set_values
  6  the kept levels of a plan under a bound matrix-free operator: release, re-keep, new values
  7  the AMG `Pl` of the interior CG replaced and dropped between solves
  8  a context closed before its operators (api)"""
import numpy as np
import pytest
import scipy.sparse as sp

import amg_synth as asy
import lifetime_cases as lc
import lorasc_ref as lr
import nn_induced_ref as nr

pytestmark = pytest.mark.gpu

MAXIT = 60     # of the solves of test 5: the as-written coupling gives no SPD M, the history is compared, not the limit


@pytest.fixture(scope="module")
def grid20(fem):
    return lc.grid_systems(fem, 20)


@pytest.fixture(scope="module")
def grid24(fem):
    return lc.grid_systems(fem, 24)


@pytest.fixture(scope="module")
def micro(fem):
    return lr.gpu_cases(fem, ["micro"])["micro"]


@pytest.fixture(scope="module")
def schur24(fem):
    return lc.schur_problems(fem, 24)


def _close(*objs):
    for o in objs:
        o.close()


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("order", ["closed_then_moved", "moved_then_closed", "closed_then_same"])
def test_full_assembly_update_after_the_checked_operator_is_gone(pkg, ctx, fem, grid20, order):
    """The plan compares an operator's whole pattern once and remembers which operator that was. `A_op` is checked and
    closed; `moved` (same indptr, same count, one column index changed) is created before or after the close — after it, its
    arrays may be the blocks `A_op` gave back. Either way the update is refused ("pattern") and `moved` keeps the bits of
    scipy(moved) @ x. A same-pattern operator created after the close is accepted and equals a fresh one."""
    api = pkg.api
    _, plan, (a0, a1, _), ((A0, b0), (A1, b1), _) = grid20
    n = plan.n
    x = np.random.default_rng(3).standard_normal(n)
    dev = api.FullAssemblyPlan(ctx, plan)
    A_op = api.SparseMatrixCSC(ctx, A0)
    parts = lc.moved_pattern(A0)
    if order == "moved_then_closed":
        nxt = api.SparseMatrixCSC(ctx, parts)
    assert np.array_equal(dev.update(a1, A_op), b1)                     # checked, remembered
    assert np.array_equal(A_op * x, A1 @ x)
    A_op.close()
    if order == "closed_then_moved":
        nxt = api.SparseMatrixCSC(ctx, parts)
    elif order == "closed_then_same":
        nxt = api.SparseMatrixCSC(ctx, A0)
    if order == "closed_then_same":
        assert np.array_equal(dev.update(a1, nxt), b1)
        with lc.fresh_context(api) as c2:
            fresh = api.SparseMatrixCSC(c2, A1)
            want = fresh * x
            fresh.close()
        assert np.array_equal(nxt * x, want)
    else:
        y0 = nxt * x
        with pytest.raises(api.MiError, match="pattern"):
            dev.update(a1, nxt)
        assert np.array_equal(nxt * x, y0) and np.array_equal(y0, lc.scipy_of(parts) @ x)
    _close(nxt, dev)


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("replaced", ["both", "M", "A"])
def test_solves_after_operators_of_the_same_size_took_their_place(pkg, ctx, fem, grid20, replaced):
    """(A, Jacobi M): pcg, defpcg with 3 vectors, eigpcg, each twice, so that graphs, `predicted` and `zero_x0` exist under
    the addresses of A and M. Then A, M or both are closed and operators of the same size (same size classes in the pool,
    same malloc bins) are created from another coefficient. The same six solves equal those of a fresh context."""
    api = pkg.api
    _, _, _, ((_, _), (A1, b1), (A2, b2)) = grid20
    W = lc.deflation_vectors(b1.size)
    A, M = api.SparseMatrixCSC(ctx, A1), api.JacobiPreconditioner(ctx, A1.diagonal())
    first = lc.trio(api, A, M, b1, W)
    assert first[0][1] > 3 and lc.same_solve(first[0], first[1]) and lc.same_solve(first[2], first[3]) and lc.same_solve(first[4], first[5])
    newA, newM = (A2, b2) if replaced in ("both", "A") else (A1, b1), A2 if replaced in ("both", "M") else A1
    if replaced in ("both", "A"):
        A.close()
    if replaced in ("both", "M"):
        M.close()
    if replaced in ("both", "A"):
        A = api.SparseMatrixCSC(ctx, newA[0])
    if replaced in ("both", "M"):
        M = api.JacobiPreconditioner(ctx, newM.diagonal())
    got = lc.trio(api, A, M, newA[1], W)
    want = lc.fresh_trio(api, newA[0], newM.diagonal(), newA[1], W)
    for k, (g, w) in enumerate(zip(got, want)):
        assert lc.same_solve(g, w), (replaced, k, g[1], w[1])
    assert not np.array_equal(got[0][2], first[0][2])                   # and they are other solves than the first pair's
    _close(M, A)


# ------------------------------------------------------------------ 3
def test_two_pairs_interleaved_on_one_workspace(pkg, ctx, fem, grid20):
    """Two pairs of one n share the context's SolverWorkspace (keyed by n). defpcg(A1, W1) captures graphs; eigpcg(A2) with a
    search space that the workspace does not hold yet re-allocates it and drops every graph; then defpcg(A1, W1) again,
    eigdefpcg(A2, W) and pcg(A1). Every solve equals its first occurrence and the same solve alone in a fresh context."""
    api = pkg.api
    _, _, _, ((_, _), (A1, b1), (A2, b2)) = grid20
    n = b1.size
    x0 = np.zeros(n)
    W1 = lc.deflation_vectors(n, 6)
    big = 2 * lc.SPDIM                                                   # larger than any search space the suite asked for at this n

    def run(c):
        ops = [api.SparseMatrixCSC(c, A1), api.JacobiPreconditioner(c, A1.diagonal()),
               api.SparseMatrixCSC(c, A2), api.JacobiPreconditioner(c, A2.diagonal())]
        return ops

    Ao1, Mo1, Ao2, Mo2 = run(ctx)
    d1 = api.defpcg(Ao1, b1, x0, W1, Mo1)
    e2 = api.eigpcg(Ao2, b2, x0, Mo2, lc.NVEC, big)
    d1b = api.defpcg(Ao1, b1, x0, W1, Mo1)
    ed2 = api.eigdefpcg(Ao2, b2, x0, Mo2, e2[3], big)
    p1 = api.pcg(Ao1, b1, x0, Mo1)
    d1c = api.defpcg(Ao1, b1, x0, W1, Mo1)
    assert lc.same_solve(d1b, d1) and lc.same_solve(d1c, d1)
    assert d1[1] > 3 and e2[1] > 3
    with lc.fresh_context(api) as c2:                                   # each solve alone, in another order
        Fo1, Fm1, Fo2, Fm2 = run(c2)
        wp1 = api.pcg(Fo1, b1, x0, Fm1)
        we2 = api.eigpcg(Fo2, b2, x0, Fm2, lc.NVEC, big)
        wed2 = api.eigdefpcg(Fo2, b2, x0, Fm2, we2[3], big)
        wd1 = api.defpcg(Fo1, b1, x0, W1, Fm1)
        _close(Fm2, Fo2, Fm1, Fo1)
    assert lc.same_solve(d1, wd1) and lc.same_solve(e2, we2) and lc.same_solve(ed2, wed2) and lc.same_solve(p1, wp1)
    _close(Mo2, Ao2, Mo1, Ao1)


# ------------------------------------------------------------------ 4
def test_a_child_cannot_be_destroyed_under_a_live_combination(pkg, ctx, fem):
    """mi_op_combine counts its children: mi_op_destroy(child) is MI_ERR_BAD_ARG and names the borrower while a combination
    holds it. The handles are raw and belong to no wrapper: if the first assertion fails, nothing touches the child or
    the combination again (no apply, no second destroy, no close())."""
    api = pkg.api
    BAD = pkg._lib.MI_ERR_BAD_ARG
    Hs = [asy.hierarchy(fem, "arrow_%d" % asy.ARROW_M[0]), asy.hierarchy(fem, "longP")]
    n = Hs[0].A[0].shape[0]
    diag = np.random.default_rng(95).uniform(0.5, 2.0, n)
    k0, k1, k2 = (lc.steal(op) for op in (api.AMGPreconditioner(ctx, Hs[0]), api.AMGPreconditioner(ctx, Hs[1]),
                                          api.JacobiPreconditioner(ctx, diag)))
    ca, cb = [0.25, -1.5], [2.0, 0.5, -0.75]
    rc, Pa = lc.raw_combine(pkg, ctx, [k0, k1], ca)
    assert rc == 0
    rc, msg = lc.raw_destroy(pkg, k0)
    assert rc == BAD, "mi_op_destroy(child) succeeded under a live combination"     # nothing below runs on a library without the count
    assert "1 place(s)" in msg and "combined operator" in msg and "mi_op_combine" in msg, msg
    rc, Pb = lc.raw_combine(pkg, ctx, [k1, k2, k1], cb)                  # k1: a second combination, twice
    assert rc == 0
    rc, msg = lc.raw_destroy(pkg, k1)
    assert rc == BAD and "3 place(s)" in msg, (rc, msg)
    # the refusals changed nothing: both combinations are the host expression on the children's applies
    r = np.random.default_rng(96).standard_normal(n)
    t0, t1, t2 = (lc.raw_apply(pkg, ctx, k, r) for k in (k0, k1, k2))
    assert np.array_equal(lc.raw_apply(pkg, ctx, Pa, r), lc.host_expression(ca, [t0, t1]))
    assert np.array_equal(lc.raw_apply(pkg, ctx, Pb, r), lc.host_expression(cb, [t1, t2, t1]))
    # release: a child goes when the last combination that holds it has gone
    assert lc.raw_destroy(pkg, Pa) == (0, "")
    assert lc.raw_destroy(pkg, k0) == (0, "")
    rc, msg = lc.raw_destroy(pkg, k1)
    assert rc == BAD and "2 place(s)" in msg, (rc, msg)
    rc, msg = lc.raw_destroy(pkg, k2)
    assert rc == BAD and "1 place(s)" in msg, (rc, msg)
    assert np.array_equal(lc.raw_apply(pkg, ctx, Pb, r), lc.host_expression(cb, [t1, t2, t1]))
    assert lc.raw_destroy(pkg, Pb) == (0, "")
    assert lc.raw_destroy(pkg, k1) == (0, "") and lc.raw_destroy(pkg, k2) == (0, "")


def test_the_api_refuses_to_close_a_borrowed_child(pkg, ctx, fem, grid20):
    """api: `child.close()` under a live InterpolatingPreconditioner raises and keeps the handle; after `Π.close()` it goes"""
    api = pkg.api
    _, _, _, ((_, _), (A1, b1), _) = grid20
    J1, J2 = api.JacobiPreconditioner(ctx, A1.diagonal()), api.JacobiPreconditioner(ctx, 2.0 * A1.diagonal())
    Π = api.InterpolatingPreconditioner(ctx, [0.5, 0.5], [J1, J2])
    r = np.random.default_rng(1).standard_normal(b1.size)
    z = Π * r
    with pytest.raises(api.MiError, match="combined operator"):
        J1.close()
    assert J1._h is not None and np.array_equal(Π * r, z)
    Π.close()
    _close(J1, J2)
    assert J1._h is None and J2._h is None


# ------------------------------------------------------------------ 5
def _hist_differs(a, b):
    m = min(len(a[2]), len(b[2]))
    return a[1] != b[1] or not np.array_equal(a[2][:m], b[2][:m])


def _nni(pkg, c, fem, case, coupling):
    api, P = pkg.api, case.P
    setup = api.SchurSetup(c, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd)
    setup.keep_levels()
    setup.run()
    M = api.NeumannNeumannInducedPreconditioner(c, P.A_IΓdd, (case.pos_I, case.pos_Γ), P.sub.gather_idx, P.sub.node_Γ_cnt,
                                                nr.prepare(fem, case), setup, coupling=coupling)
    return M, setup


def test_set_coupling_of_a_child_under_captured_graphs(pkg, ctx, fem, micro):
    """Π = 0.7 NN-induced + 0.3 Jacobi on the full system of `micro`; pcg twice (graphs keyed by Π hold the operand arrays of
    the child's launch 6); set_coupling on the child; the next solve is the one of a fresh context whose child was created
    with that coupling, and another solve than the first; back again: the first solve."""
    api, c = pkg.api, micro
    x0 = np.zeros(c.n)
    coef = [0.7, 0.3]

    def solve_fresh(coupling):
        with lc.fresh_context(api) as c2:
            A2 = api.SparseMatrixCSC(c2, c.A)
            M2, s2 = _nni(pkg, c2, fem, c, coupling)
            J2 = api.JacobiPreconditioner(c2, c.A.diagonal())
            Π2 = api.InterpolatingPreconditioner(c2, coef, [M2, J2])
            out = api.pcg(A2, c.b, x0, Π2, MAXIT)
            _close(Π2, J2, M2, s2, A2)
        return out

    A = api.SparseMatrixCSC(ctx, c.A)
    M, setup = _nni(pkg, ctx, fem, c, "assembled")
    J = api.JacobiPreconditioner(ctx, c.A.diagonal())
    Π = api.InterpolatingPreconditioner(ctx, coef, [M, J])
    first = api.pcg(A, c.b, x0, Π, MAXIT)
    assert lc.same_solve(api.pcg(A, c.b, x0, Π, MAXIT), first) and first[1] > 3
    M.set_coupling("reference")
    second = api.pcg(A, c.b, x0, Π, MAXIT)
    assert lc.same_solve(second, solve_fresh("reference"))
    assert _hist_differs(second, first)
    M.set_coupling("assembled")
    assert lc.same_solve(api.pcg(A, c.b, x0, Π, MAXIT), first)
    assert lc.same_solve(first, solve_fresh("assembled"))
    _close(Π, J, M, setup, A)


def _lorasc(pkg, c, case, E):
    api, P = pkg.api, case.P
    setup = api.SchurSetup(c, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd)
    setup.keep_levels()
    setup.run()
    gg = api.SparseDirectPreconditioner(c, case.A_ΓΓ)
    return api.LorascPreconditioner(c, case.A_IΓd, (case.pos_I, case.pos_Γ), setup, gg, E), gg, setup


def test_set_correction_and_new_values_of_a_child_under_captured_graphs(pkg, ctx, fem, micro):
    """Π = 0.7 LORASC + 0.3 Jacobi; pcg twice; set_correction with MORE vectors (nev and the address of a re-allocated E are
    arguments of the captured launches), with fewer again, and a new realization of every matrix in place (plan re-run,
    A_ΓΓ values, A_IΓ values, A values): each state equals a fresh context created in it."""
    api, c = pkg.api, micro
    c2 = lr.make_case(fem, "micro2", 40, 2, 2, lc.lognormal_coeff(fem, c.P.mesh.points, 4))
    assert c2.n == c.n and all(a.nnz == b.nnz for a, b in zip(c.A_IΓd, c2.A_IΓd)) and c.A.nnz == c2.A.nnz and c.A_ΓΓ.nnz == c2.A_ΓΓ.nnz
    x0 = np.zeros(c.n)
    coef = [0.7, 0.3]
    rng = np.random.default_rng(12)
    E3 = rng.standard_normal((c.n_Γ, 3)) / np.sqrt(c.n_Γ)
    E9 = rng.standard_normal((c.n_Γ, 9)) / np.sqrt(c.n_Γ)

    def solve_fresh(case, E):
        with lc.fresh_context(api) as cf:
            Af = api.SparseMatrixCSC(cf, case.A)
            Mf, gf, sf = _lorasc(pkg, cf, case, E)
            Jf = api.JacobiPreconditioner(cf, c.A.diagonal())
            Πf = api.InterpolatingPreconditioner(cf, coef, [Mf, Jf])
            out = api.pcg(Af, case.b, x0, Πf, MAXIT)
            _close(Πf, Jf, Mf, gf, sf, Af)
        return out

    A = api.SparseMatrixCSC(ctx, c.A)
    M, gg, setup = _lorasc(pkg, ctx, c, E3)
    J = api.JacobiPreconditioner(ctx, c.A.diagonal())
    Π = api.InterpolatingPreconditioner(ctx, coef, [M, J])
    first = api.pcg(A, c.b, x0, Π, MAXIT)
    assert lc.same_solve(api.pcg(A, c.b, x0, Π, MAXIT), first) and first[1] > 3
    assert lc.same_solve(first, solve_fresh(c, E3))
    M.set_correction(E9)
    second = api.pcg(A, c.b, x0, Π, MAXIT)
    assert lc.same_solve(second, solve_fresh(c, E9)) and _hist_differs(second, first)
    M.set_correction(E3)
    assert lc.same_solve(api.pcg(A, c.b, x0, Π, MAXIT), first)
    # a new realization, every array in place: the captured graphs stay and see the new values
    P2 = c2.P
    setup.run(lc.csc_data(P2.A_IIdd), lc.csc_data(P2.A_IΓdd), lc.csc_data(P2.A_ΓΓdd))
    gg.set_values(sp.csc_matrix(c2.A_ΓΓ).data)
    M.set_values(lc.csc_data(c2.A_IΓd))
    A.set_values(c2.A)
    third = api.pcg(A, c2.b, x0, Π, MAXIT)
    assert lc.same_solve(third, solve_fresh(c2, E3)) and _hist_differs(third, first)
    _close(Π, J, M, gg, setup, A)


@pytest.mark.parametrize("kind", ["amg", "block_jacobi"])
def test_set_values_of_a_child_under_captured_graphs(pkg, ctx, fem, grid24, kind):
    """Π = 0.6 child + 0.4 Jacobi with an AMG or a block-Jacobi child; pcg twice; child.set_values(A2); the next solve equals
    a fresh context whose child was made from A2 (the AMG child on the aggregates of A1, which a refresh keeps); and back."""
    api = pkg.api
    _, _, _, ((_, _), (A1, b1), (A2, _)) = grid24
    x0 = np.zeros(b1.size)
    coef = [0.6, 0.4]
    aggs = []

    def child(c, A):
        if kind == "block_jacobi":
            return api.BlockJacobiPreconditioner(c, 4, A)
        if not aggs:
            M = api.AMGPreconditioner(c, A, device_setup=True, max_coarse=40)
            aggs.append(M.aggregates)
            return M
        M = api.AMGPreconditioner(c, A1, device_setup=True, aggregates=aggs[0])
        M.set_values(A)
        return M

    def solve_fresh(Ach):
        with lc.fresh_context(api) as c2:
            Af, Mf, Jf = api.SparseMatrixCSC(c2, A1), child(c2, Ach), api.JacobiPreconditioner(c2, A1.diagonal())
            Πf = api.InterpolatingPreconditioner(c2, coef, [Mf, Jf])
            out = api.pcg(Af, b1, x0, Πf)
            _close(Πf, Jf, Mf, Af)
        return out

    A, M, J = api.SparseMatrixCSC(ctx, A1), child(ctx, A1), api.JacobiPreconditioner(ctx, A1.diagonal())
    Π = api.InterpolatingPreconditioner(ctx, coef, [M, J])
    first = api.pcg(A, b1, x0, Π)
    assert lc.same_solve(api.pcg(A, b1, x0, Π), first) and first[1] > 3
    M.set_values(A2)
    second = api.pcg(A, b1, x0, Π)
    assert lc.same_solve(second, solve_fresh(A2)) and _hist_differs(second, first)
    M.set_values(A1)
    assert lc.same_solve(api.pcg(A, b1, x0, Π), first)
    assert lc.same_solve(first, solve_fresh(A1))
    _close(Π, J, M, A)


# ------------------------------------------------------------------ 6
def _matfree(api, c, P, reltol=1e-9):
    return api.MatrixFreeLocalSchurs(c, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd, P.sub.gather_idx, P.sub.node_Γ_cnt, None, reltol=reltol)


def test_kept_levels_released_under_a_bound_matrix_free_operator(pkg, ctx, fem, schur24, micro):
    """What the table allows: `keep_levels(plan, 0)` is accepted while matrix-free operators are bound to the plan, because no
    launch of theirs is captured anywhere — S is never part of a solve graph and every level solve checks the plan first.
    So after the release `S * x` and `pcg(S, ...)` are refused by text, nothing runs on the released storage, and with the
    levels kept and run again `S * x` has its bits back. The operators whose level solves ARE captured refuse the release:
    a Neumann-Neumann induced operator bound to its plan is named, and keeps its bits.
    New values under the bound S: plan.run + S.set_values between two pcg(S, ...) equals a fresh pair on the new values."""
    api = pkg.api
    Lb = pkg._lib.load()
    BAD = pkg._lib.MI_ERR_BAD_ARG
    P1, P2 = schur24
    n_Γ = P1.sub.n_Γ
    x = np.random.default_rng(8).standard_normal(n_Γ)
    x0 = np.zeros(n_Γ)
    vals2 = (lc.csc_data(P2.A_IIdd), lc.csc_data(P2.A_IΓdd), lc.csc_data(P2.A_ΓΓdd))

    def pair(c, P):
        setup = api.SchurSetup(c, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd)
        setup.keep_levels()
        setup.run()
        S = _matfree(api, c, P)
        S.use_level_solver(setup)
        return S, setup, api.IdentityPreconditioner(c, n_Γ)

    S, setup, I = pair(ctx, P1)
    y0 = S * x
    s1 = api.pcg(S, P1.b_schur, x0, I)
    assert s1[1] > 3 and lc.same_solve(api.pcg(S, P1.b_schur, x0, I), s1)
    # release under the bound operator: accepted, and refused by text from then on
    assert Lb.mi_schur_setup_keep_levels(setup._h, 0) == 0
    for call in (lambda: S * x, lambda: api.pcg(S, P1.b_schur, x0, I)):
        with pytest.raises(api.MiError, match="level solves need"):
            call()
    setup.keep_levels()
    with pytest.raises(api.MiError, match="level solves need"):         # kept, but no run after it
        S * x
    setup.run()
    assert np.array_equal(S * x, y0) and lc.same_solve(api.pcg(S, P1.b_schur, x0, I), s1)
    # new values under the bound S
    setup.run(*vals2)
    S.set_values(*vals2)
    s2 = api.pcg(S, P2.b_schur, x0, I)
    with lc.fresh_context(api) as c2:
        S2, setup2, I2 = pair(c2, P2)
        want = api.pcg(S2, P2.b_schur, x0, I2)
        y2 = S2 * x
        S2.use_level_solver(None)
        y2_cg = S2 * x                                                  # its own interior CG
        _close(I2, S2, setup2)
    assert lc.same_solve(s2, want) and np.array_equal(S * x, y2) and _hist_differs(s2, s1)
    # unbound: the release needs nobody's leave, and S is back on its own interior CG, on the new values
    S.use_level_solver(None)
    assert Lb.mi_schur_setup_keep_levels(setup._h, 0) == 0
    assert np.array_equal(S * x, y2_cg) and not np.array_equal(y2_cg, y2)
    _close(I, S, setup)
    # captured level solves: the release is refused and names the borrower
    M, plan = _nni(pkg, ctx, fem, micro, "assembled")
    r = nr.apply_input(micro)
    z = M.ldiv(r)
    assert Lb.mi_schur_setup_keep_levels(plan._h, 0) == BAD
    msg = Lb.mi_last_error().decode()
    assert "1 live Neumann-Neumann induced operator(s) solve with the kept levels" in msg, msg
    assert np.array_equal(M.ldiv(r), z)
    M.close()
    assert Lb.mi_schur_setup_keep_levels(plan._h, 0) == 0
    plan.close()


# ------------------------------------------------------------------ 7
def test_interior_amg_replaced_and_dropped_between_solves(pkg, ctx, fem, schur24):
    """The AMG `Pl` of the interior CG is owned by the operator; selecting another hierarchy or none is allowed at any time
    (the stream is idle between solves) and drops the interior CG's own graph, whose launches hold the old hierarchy's
    arrays. After each change pcg(S, ...) and S * x equal a fresh operator that was given that `Pl` from the start."""
    api = pkg.api
    P1, _ = schur24
    n_Γ = P1.sub.n_Γ
    x = np.random.default_rng(9).standard_normal(n_Γ)
    x0 = np.zeros(n_Γ)
    STATES = (("amg", 100), ("amg", 16), ("none", None), ("amg", 100), ("diagonal", None))

    def select(S, state):
        kind, mc = state
        if kind == "amg":
            S.interior_amg(P1.A_IIdd, max_coarse=mc)
        else:
            S.interior_precond(kind)

    def run(S, I):
        return api.pcg(S, P1.b_schur, x0, I, 25), S * x

    want = {}
    with lc.fresh_context(api) as c2:
        for state in sorted(set(STATES), key=str):
            S2, I2 = _matfree(api, c2, P1), api.IdentityPreconditioner(c2, n_Γ)
            select(S2, state)
            want[state] = run(S2, I2)
            _close(I2, S2)
    assert not np.array_equal(want[("amg", 100)][1], want[("amg", 16)][1])   # the states are told apart by their bits
    assert not np.array_equal(want[("amg", 100)][1], want[("none", None)][1])
    S, I = _matfree(api, ctx, P1), api.IdentityPreconditioner(ctx, n_Γ)
    for state in STATES:
        select(S, state)
        for _ in range(2):                                              # the second solve replays the interior CG's graph
            got = run(S, I)
            assert lc.same_solve(got[0], want[state][0]) and np.array_equal(got[1], want[state][1]), state
    _close(I, S)


# ------------------------------------------------------------------ 8
def test_a_context_closed_before_its_operators(pkg, fem, grid20):
    """Every handle holds its context by address, uncounted: the C ABI's rule is "operators before their context". The api
    keeps the rule for its users: after `ctx.close()` the wrappers' close() and finalizers call nothing."""
    api = pkg.api
    _, _, _, ((_, _), (A1, b1), _) = grid20
    c2 = api.Context(0)
    A, M = api.SparseMatrixCSC(c2, A1), api.JacobiPreconditioner(c2, A1.diagonal())
    Π = api.InterpolatingPreconditioner(c2, [1.0], [M])
    assert api.pcg(A, b1, np.zeros(b1.size), Π)[1] > 3
    c2.close()
    assert c2._h is None
    for op in (M, Π, A):                                                # any order: nothing reaches the library
        op.close()
        assert op._h is None
