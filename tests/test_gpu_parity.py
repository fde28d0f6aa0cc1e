"""GPU suite (-m gpu): the HIP path, called through the C ABI, against the CPU oracle on the same
inputs and against the committed golden fixtures.

Tolerances (all arithmetic fp64):
  * element-wise kernels (axpy, axpby) and the CSR SpMV: BIT-EXACT vs the oracle (same operation
    order, library built with -ffp-contract=off);
  * reductions (dot, dense GEMV rows) reorder sums: rel. 1e-13 on a single apply;
  * solvers: `it` equal; res_norm entries |Δ| <= 1e-8*res_k + 1e-12*res_1 on the first 20 entries
    (= all of them for every preconditioned solve; see assert_history for long CG runs) (relative, with a floor
    twelve orders under the initial residual: entries near convergence are themselves ~1e-10*res_1
    and carry the rounding of every earlier update); solution rel. l2 diff <= 1e-6.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN, a_example01, f_m1, lognormal_coeff, lowest_eigvecs, u0734, u3

pytestmark = pytest.mark.gpu

RES_RTOL = 1e-8
RES_FLOOR = 1e-12      # times res_norm[1]
X_RTOL = 1e-6


TIGHT_PREFIX = 20
EQUAL_IT_UPTO = 50     # `it` must equal the oracle's for every solve of at most this many iterations


def assert_history(got, want, apply=None, b=None):
    """Short solves (it <= TIGHT_PREFIX, i.e. every well-preconditioned case incl. the 1M-DoF headline): `it`
    EQUAL and every res_norm entry within RES_RTOL (+floor).
    Long solves: CG in finite precision amplifies summation-order differences (the oracle sums left to right,
    the GPU in lane-strided trees) — between any two BLAS builds as well. There the first TIGHT_PREFIX entries
    are still held to RES_RTOL, later entries of the common part to a factor 2, `it` to +-max(1, 2 %), and the
    answer is checked independently through the true residual ||b - A x|| with the oracle's operator."""
    x, it, res = got
    xo, ito, reso = want
    if max(it, ito) <= TIGHT_PREFIX:
        assert it == ito, f"iteration counts differ: {it} vs oracle {ito}"
        assert np.allclose(res, reso, rtol=RES_RTOL, atol=RES_FLOOR * reso[0]), np.max(np.abs(res - reso) / reso)
        assert np.linalg.norm(x - xo) <= X_RTOL * np.linalg.norm(xo)
        return
    if max(it, ito) <= EQUAL_IT_UPTO:                             # solves of up to 50 iterations: `it` EQUAL (north_star)
        assert it == ito, f"iteration counts differ: {it} vs oracle {ito}"
    assert abs(it - ito) <= max(1, ito // 50), f"iteration counts differ: {it} vs oracle {ito}"
    k, m = TIGHT_PREFIX, min(it, ito)
    assert np.allclose(res[:k], reso[:k], rtol=RES_RTOL, atol=RES_FLOOR * reso[0]), \
        np.max(np.abs(res[:k] - reso[:k]) / reso[:k])
    ratio = res[k:m] / reso[k:m]
    assert ratio.size == 0 or (ratio.max() < 2.0 and ratio.min() > 0.5), (ratio.min(), ratio.max())
    assert apply is not None and b is not None, "long runs need the true-residual check"
    bn = np.linalg.norm(b)
    assert np.linalg.norm(b - apply(x)) <= 2.0 * max(res[-1], 1e-7 * bn)
    assert np.linalg.norm(x - xo) <= 1e-4 * np.linalg.norm(xo)


def gpu_ops(pkg, ctx, P):
    api = pkg.api
    return (api.LocalSchurs(ctx, P.Sd, P.sub.gather_idx, P.sub.node_Γ_cnt),
            api.NeumannNeumannSchurPreconditioner(ctx, P.ΠSd, P.sub.gather_idx, P.sub.node_Γ_cnt))


def orc_ops(orc, P):
    return (orc.apply_local_schurs_operator(P.Sd, P.sub.gather_idx, P.sub.n_Γ),
            orc.neumann_neumann_operator(P.ΠSd, P.sub.gather_idx, P.sub.node_Γ_cnt))


# ------------------------------------------------------------------ BLAS-1
@pytest.mark.parametrize("n", [1, 63, 64, 1000, 3989, 248004])
def test_blas1(ctx, n):
    rng = np.random.default_rng(n)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    assert np.isclose(ctx.dot(x, y), np.dot(x, y), rtol=1e-12, atol=1e-12 * np.sqrt(n))
    assert np.isclose(ctx.norm2(x), np.linalg.norm(x), rtol=1e-13)
    a, b = 0.37, -1.25
    assert np.array_equal(ctx.axpy(a, x, y.copy()), y + a * x)            # bit-exact, no FMA
    assert np.array_equal(ctx.axpby(a, x, b, y.copy()), a * x + b * y)


# ------------------------------------------------------------------ CSR SpMV: bit-exact
def test_spmv_bit_exact_vs_oracle(pkg, ctx, orc, fem, toy):
    mesh = fem.get_mesh(120)
    d = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
    A, b = fem.do_isotropic_elliptic_assembly(mesh.cells, mesh.points, d, mesh.point_marker, a_example01, f_m1, u3)
    rng = np.random.default_rng(5)
    for M in (A, toy.A_IIdd[1], sp.identity(5, format="csr"), sp.csr_matrix((7, 7))):
        n = M.shape[0]
        x = rng.standard_normal(n)
        got = pkg.api.SparseMatrixCSC(ctx, M) * x
        want = orc.csc_operator(M) * x          # stdlib CSC scatter order
        assert np.array_equal(got, want)


def test_spmv_long_row_and_one_based(pkg, ctx, orc):
    # an arrow matrix: row/column 0 is dense with n > SPMV_TILE entries (the single-long-row path)
    n = 5000
    rng = np.random.default_rng(6)
    v = rng.standard_normal(n)
    A = sp.lil_matrix((n, n))
    A[0, :] = v
    A[:, 0] = v.reshape(-1, 1)
    A.setdiag(np.abs(v) + n)
    A = sp.csr_matrix(A)
    x = rng.standard_normal(n)
    want = orc.csc_operator(A) * x
    assert np.array_equal(pkg.api.SparseMatrixCSC(ctx, A) * x, want)
    # Julia-style 1-based arrays through index_base=1
    A.sort_indices()
    op1 = pkg.api.SparseMatrixCSC(ctx, (A.indptr + 1, A.indices + 1, A.data, n), index_base=1)
    assert np.array_equal(op1 * x, want)


# ------------------------------------------------------------------ Schur / NN applies
@pytest.mark.parametrize("case", ["micro", "toy", "ragged"])
def test_assembled_applies_vs_oracle(pkg, ctx, orc, case, micro, toy, ragged):
    P = {"micro": micro, "toy": toy, "ragged": ragged}[case]
    S, M = gpu_ops(pkg, ctx, P)
    So, Mo = orc_ops(orc, P)
    rng = np.random.default_rng(8)
    for _ in range(2):
        v = rng.standard_normal(P.sub.n_Γ)
        ys, yo = S * v, So * v
        assert np.allclose(ys, yo, rtol=0, atol=1e-13 * np.abs(yo).max())
        zs, zo = M.ldiv(v), Mo * v
        assert np.allclose(zs, zo, rtol=0, atol=1e-13 * np.abs(zo).max())
    # reference-named free functions
    assert np.array_equal(pkg.api.apply_local_schurs(S, v), ys)
    assert np.array_equal(pkg.api.apply_neumann_neumann_schur(M, v), zs)


def test_applies_vs_golden(pkg, ctx):
    for name in ("micro", "toy"):
        G = np.load(f"{GOLDEN}/{name}.npz")
        nd = 4
        Sd = [G[f"Sd_{d}"] for d in range(nd)]
        Pi = [G[f"PiSd_{d}"] for d in range(nd)]
        gi = [G[f"gather_idx_{d}"] for d in range(nd)]
        S = pkg.api.LocalSchurs(ctx, Sd, gi, G["node_gamma_cnt"])
        M = pkg.api.NeumannNeumannSchurPreconditioner(ctx, Pi, gi, G["node_gamma_cnt"])
        assert np.allclose(S * G["v"], G["S_v"], rtol=0, atol=1e-13 * np.abs(G["S_v"]).max())
        assert np.allclose(M.ldiv(G["v"]), G["M_v"], rtol=0, atol=1e-13 * np.abs(G["M_v"]).max())
        b, x0 = G["b_schur"], np.zeros(int(G["n_gamma"]))
        for tag, got in (("cg", pkg.api.cg(S, b, x0)), ("pcg", pkg.api.pcg(S, b, x0, M)),
                         ("defpcg", pkg.api.defpcg(S, b, x0, G["W"], M))):
            assert_history(got, (G[f"{tag}_x"], int(G[f"{tag}_it"]), G[f"{tag}_res_norm"]),
                           lambda v: S * v, b)


def test_domain_slices_sum_to_full_apply(pkg, ctx, ragged):
    """A rank's operator applies only its slice of subdomains; the slices add up to the full sum
    (what the RCCL all-reduce computes across GPUs)."""
    P = ragged
    rng = np.random.default_rng(9)
    v = rng.standard_normal(P.sub.n_Γ)
    full = pkg.api.LocalSchurs(ctx, P.Sd, P.sub.gather_idx, P.sub.node_Γ_cnt) * v
    acc = np.zeros_like(full)
    for lo, hi in ((0, 2), (2, 2), (2, 5), (5, 6)):                     # includes an empty slice
        acc += pkg.api.LocalSchurs(ctx, P.Sd, P.sub.gather_idx, P.sub.node_Γ_cnt, dom_slice=(lo, hi)) * v
    assert np.allclose(acc, full, rtol=0, atol=1e-13 * np.abs(full).max())


def test_matrix_free_and_global_schur_vs_oracle(pkg, ctx, orc, fem, ragged):
    P = ragged
    n = P.sub.n_Γ
    Sm = pkg.api.MatrixFreeLocalSchurs(ctx, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd, P.sub.gather_idx, P.sub.node_Γ_cnt, P.solvers)
    Smo = orc.apply_local_schurs_matfree_operator(P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd, P.sub.gather_idx, n, P.solvers)
    rng = np.random.default_rng(10)
    v = rng.standard_normal(n)
    want = Smo * v
    got = Sm * v
    # sparse products are bit-exact; the interior solve is the same host callback
    assert np.array_equal(got, want)
    coeff = lognormal_coeff(fem, P.mesh.points, 7)
    A_IIg, A_IΓg, A_ΓΓ, b_Id, b_Γ = fem.prepare_global_schur(P.mesh.cells, P.mesh.points, P.epart, P.sub, coeff, f_m1, u0734)
    Sg = pkg.api.GlobalSchur(ctx, A_IIg, A_IΓg, A_ΓΓ, P.solvers)
    Sgo = orc.apply_global_schur_operator(A_IIg, A_IΓg, A_ΓΓ, P.solvers)
    assert np.array_equal(pkg.api.apply_global_schur(Sg, v), Sgo * v)
    # the same operator with the interior CG on the device (no callback): against the oracle's restatement of that inexact
    # solve, at the reference's default reltol = sqrt(eps) and at a tight one
    for reltol in (float(np.sqrt(np.finfo(float).eps)), 1e-12):
        Sgd = pkg.api.GlobalSchur(ctx, A_IIg, A_IΓg, A_ΓΓ, None, reltol=reltol)
        Sgdo = orc.apply_global_schur_operator(A_IIg, A_IΓg, A_ΓΓ, orc.interior_cg_solvers(A_IIg, reltol))
        yd, yo = Sgd * v, Sgdo * v
        assert np.abs(yd - yo).max() <= 0.5 * reltol * np.abs(yo).max() + 1e-12 * np.abs(yo).max()
    assert np.abs(yd - Sgo * v).max() <= 1e-9 * np.abs(yd).max()
    # get_schur_rhs (EPDD.jl:798-821) and get_subdomain_solutions (:1014-1025) in their Γ-global forms, host callback: exact solves
    bI = np.concatenate(b_Id)
    assert np.allclose(Sg.schur_rhs(bI, b_Γ), fem.get_schur_rhs(b_Id, A_IIg, A_IΓg, b_Γ, solvers=P.solvers), rtol=1e-12, atol=1e-14)
    uI = Sg.interior_solutions(v, bI)
    ref = np.concatenate(fem.get_subdomain_solutions(v, A_IIg, A_IΓg, b_Id, P.solvers))
    assert np.allclose(uI, ref, rtol=1e-12, atol=1e-13 * np.abs(ref).max())
    assert np.linalg.norm(Sgd.interior_solutions(v, bI) - ref) <= 1e-9 * np.linalg.norm(ref)
    # Example03:175 identity on the device path
    Sa = pkg.api.LocalSchurs(ctx, P.Sd, P.sub.gather_idx, P.sub.node_Γ_cnt)
    assert np.allclose(Sa * v, got, rtol=0, atol=1e-11 * np.abs(got).max())
    # pcg on the matrix-free operator (eager loop, host callback every apply)
    M = pkg.api.NeumannNeumannSchurPreconditioner(ctx, P.ΠSd, P.sub.gather_idx, P.sub.node_Γ_cnt)
    Mo = orc.neumann_neumann_operator(P.ΠSd, P.sub.gather_idx, P.sub.node_Γ_cnt)
    assert_history(pkg.api.pcg(Sm, P.b_schur, np.zeros(n), M), orc.pcg(Smo, P.b_schur, np.zeros(n), Mo))


def test_failing_interior_callback_names_the_global_subdomain_and_leaves_no_trace(pkg, ctx, fem, ragged):
    """The host callback returns an error for one subdomain: `apply`, `schur_rhs` and `interior_solutions` of both
    matrix-free operators return MI_ERR_CALLBACK naming the GLOBAL subdomain (a slice 2..4 fails on its local subdomain 1),
    and once the callback works again the same handles give the bits they gave before."""
    api, P = pkg.api, ragged
    n, k, (lo, hi) = P.sub.n_Γ, 3, (2, 5)
    failing = {"on": False}

    def guard(d, solve):
        def f(rhs):
            if failing["on"] and d == k:
                raise RuntimeError("interior solver %d fails" % d)
            return solve(rhs)
        return f

    solvers = [guard(d, s) for d, s in enumerate(P.solvers)]
    Sm = api.MatrixFreeLocalSchurs(ctx, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd, P.sub.gather_idx, P.sub.node_Γ_cnt, solvers, dom_slice=(lo, hi))
    coeff = lognormal_coeff(fem, P.mesh.points, 7)
    A_IIg, A_IΓg, A_ΓΓ, b_Id, b_Γ = fem.prepare_global_schur(P.mesh.cells, P.mesh.points, P.epart, P.sub, coeff, f_m1, u0734)
    Sg = api.GlobalSchur(ctx, A_IIg, A_IΓg, A_ΓΓ, solvers)
    v = np.random.default_rng(12).standard_normal(n)
    for S, bI in ((Sm, np.concatenate(P.b_Id[lo:hi])), (Sg, np.concatenate(b_Id))):
        calls = (lambda: S * v, lambda: S.schur_rhs(bI, b_Γ), lambda: S.interior_solutions(v, bI))
        before = [c() for c in calls]
        failing["on"] = True
        for c in calls:
            with pytest.raises(pkg._lib.MiError) as e:
                c()
            assert e.value.code == pkg._lib.MI_ERR_CALLBACK and "subdomain %d" % k in str(e.value), str(e.value)
        failing["on"] = False
        for c, want in zip(calls, before):
            assert np.array_equal(c(), want)


# ------------------------------------------------------------------ solvers
@pytest.mark.parametrize("case", ["micro", "toy", "ragged"])
def test_schur_solvers_vs_oracle(pkg, ctx, orc, case, micro, toy, ragged):
    P = {"micro": micro, "toy": toy, "ragged": ragged}[case]
    api = pkg.api
    S, M = gpu_ops(pkg, ctx, P)
    So, Mo = orc_ops(orc, P)
    n, b = P.sub.n_Γ, P.b_schur
    x0 = np.zeros(n)
    assert_history(api.cg(S, b, x0), orc.cg(So, b, x0), So, b)
    assert_history(api.pcg(S, b, x0, M), orc.pcg(So, b, x0, Mo))
    W = lowest_eigvecs(So, n, P.sub.ndom + 10)                            # Example03:206
    assert_history(api.defcg(S, b, x0, W), orc.defcg(So, b, x0, W), So, b)
    assert_history(api.defpcg(S, b, x0, W, M), orc.defpcg(So, b, x0, W, Mo))
    # non-zero initial guess
    x1 = np.random.default_rng(11).standard_normal(n)
    assert_history(api.pcg(S, b, x1, M), orc.pcg(So, b, x1, Mo))
    assert_history(api.defpcg(S, b, x1, W, M), orc.defpcg(So, b, x1, W, Mo))


def test_full_system_pcg_config2_small(pkg, ctx, orc, fem):
    """Example01 flow (config 2) at N=150: CSR SpMV + BLAS-1 kernels only, multi-workgroup reductions."""
    mesh = fem.get_mesh(150)
    d = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
    A, b = fem.do_isotropic_elliptic_assembly(mesh.cells, mesh.points, d, mesh.point_marker, a_example01, f_m1, u3)
    n = b.size
    api = pkg.api
    Ag, Ao = api.SparseMatrixCSC(ctx, A), orc.csc_operator(A)
    x0 = np.zeros(n)
    assert_history(api.cg(Ag, b, x0), orc.cg(Ao, b, x0), Ao, b)
    assert_history(api.pcg(Ag, b, x0, api.JacobiPreconditioner(ctx, A.diagonal())),
                   orc.pcg(Ao, b, x0, orc.jacobi_operator(A.diagonal())), Ao, b)
    assert_history(api.pcg(Ag, b, x0, api.IdentityPreconditioner(ctx, n)),
                   orc.pcg(Ao, b, x0, orc.identity_operator(n)), Ao, b)


def test_stop_rule_edges(pkg, ctx, orc, micro):
    P = micro
    api = pkg.api
    S, M = gpu_ops(pkg, ctx, P)
    So, Mo = orc_ops(orc, P)
    n, b = P.sub.n_Γ, P.b_schur
    x0 = np.zeros(n)
    for maxit in (1, 2, 3, 7):
        assert_history(api.pcg(S, b, x0, M, maxit=maxit), orc.pcg(So, b, x0, Mo, maxit=maxit))
        assert_history(api.cg(S, b, x0, maxit=maxit), orc.cg(So, b, x0, maxit=maxit))
    xs, its, _ = orc.pcg(So, b, x0, Mo)
    x, it, res = api.pcg(S, b, xs, M)                                     # converged initial guess: no loop pass
    assert it == 1 and res.size == 1
    x, it, res = api.cg(S, np.zeros(n), x0)                               # b = 0: tol = 0, res = 0 -> it = 1
    assert it == 1 and res[0] == 0.0 and not np.any(x)
    assert_history(api.pcg(S, b, x0, M, eps=1e-12), orc.pcg(So, b, x0, Mo, eps=1e-12))


def test_results_do_not_depend_on_chunking_or_pointer_mode(pkg, ctx, toy):
    import torch
    api = pkg.api
    P = toy
    S, M = gpu_ops(pkg, ctx, P)
    n, b = P.sub.n_Γ, P.b_schur
    ref = None
    try:
        for chunk in (0, 1, 5, 8, 64):
            ctx.set_chunk(chunk)
            got = api.pcg(S, b, np.zeros(n), M)
            if ref is None:
                ref = got
            assert got[1] == ref[1] and np.array_equal(got[2], ref[2]) and np.array_equal(got[0], ref[0])
    finally:
        ctx.set_chunk(8)
    bt = torch.from_numpy(b).cuda()
    xt = torch.zeros(n, dtype=torch.float64, device="cuda")
    x, it, res = api.pcg(S, bt, xt, M)
    assert x is xt and it == ref[1] and np.array_equal(res, ref[2])       # x mutated in place, like the reference
    assert np.array_equal(xt.cpu().numpy(), ref[0])
    yt = S * bt
    assert np.array_equal(yt.cpu().numpy(), S * b)


def test_error_conventions(pkg, ctx, toy):
    api = pkg.api
    P = toy
    S, M = gpu_ops(pkg, ctx, P)
    n, b = P.sub.n_Γ, P.b_schur
    # rank-deficient W with an exactly zero pivot (two equal columns give U[2,2] == 0 only if fl(1/a)*a == 1 for
    # a = b'Sb, in LAPACK as here: value-dependent; a zero column is singular for every value)
    W = np.asfortranarray(np.column_stack([b, np.zeros(n)]))
    with pytest.raises(api.SingularException):
        api.defpcg(S, b, np.zeros(n), W, M)
    x, it, res = api.pcg(S, b, np.zeros(n), M)                            # the context is still usable
    assert it > 1
    with pytest.raises(ValueError):
        api.pcg(S, b[:-1], np.zeros(n), M)
    with pytest.raises(api.MiError):                                      # gather index out of range
        api.LocalSchurs(ctx, P.Sd, [g + 10**6 for g in P.sub.gather_idx], P.sub.node_Γ_cnt)
    with pytest.raises(api.MiError):                                      # repeated Γ index in one subdomain
        bad = [g.copy() for g in P.sub.gather_idx]
        bad[0][1] = bad[0][0]
        api.LocalSchurs(ctx, P.Sd, bad, P.sub.node_Γ_cnt)


def test_rccl_single_rank_communicator(pkg, ctx, orc, micro):
    """world_size 1 on the one GPU of the box: the RCCL binding, communicator set-up and an
    all-reduce captured inside the iteration graph all execute; the result must not change.
    MI355_FORCE_REDUCE keeps the collectives although the single rank holds every subdomain."""
    import os
    api = pkg.api
    P = micro
    c2 = api.Context(0)
    c2.comm_init(c2.unique_id(), 0, 1)
    v = np.arange(5, dtype=np.float64)
    assert np.array_equal(c2.allreduce_sum(v.copy()), v)
    So, Mo = orc_ops(orc, P)
    n = P.sub.n_Γ
    os.environ["MI355_FORCE_REDUCE"] = "1"
    try:
        S, M = gpu_ops(pkg, c2, P)                       # "sharded": Γ-sums through the all-reduced slot table
    finally:
        del os.environ["MI355_FORCE_REDUCE"]
    Mr = api.NeumannNeumannSchurPreconditioner(c2, P.ΠSd, P.sub.gather_idx, P.sub.node_Γ_cnt)   # replicated: no collective
    got = api.pcg(S, P.b_schur, np.zeros(n), M)
    assert_history(got, orc.pcg(So, P.b_schur, np.zeros(n), Mo))
    # Summing with the other ranks' zeros is exact, so a sharded loop is bit-identical to the same loop form without a
    # communicator: the 4-launch loop when the preconditioner is sharded too, the folded loop (S launch + one captured
    # all-reduce + ΠS launch) when it is replicated on every rank.
    S1, M1 = gpu_ops(pkg, ctx, P)
    ref_fold = api.pcg(S1, P.b_schur, np.zeros(n), M1)
    os.environ["MI355_NO_FOLD"] = "1"
    try:
        ref = api.pcg(S1, P.b_schur, np.zeros(n), M1)
    finally:
        del os.environ["MI355_NO_FOLD"]
    # both "sharded": the folded loop with an exchange behind each launch (round 3; per-row partial dots: re-associated) ...
    assert got[1] == ref_fold[1] and np.allclose(got[2], ref_fold[2], rtol=1e-9, atol=1e-13 * ref_fold[2][0])
    # ... and, on request, the 4-launch loop: bit-identical to the same loop form without a communicator
    os.environ["MI355_NO_FOLD_SHARDED_NN"] = "1"
    try:
        got4 = api.pcg(S, P.b_schur, np.zeros(n), M)
    finally:
        del os.environ["MI355_NO_FOLD_SHARDED_NN"]
    assert got4[1] == ref[1] and np.array_equal(got4[2], ref[2]) and np.array_equal(got4[0], ref[0])
    gf = api.pcg(S, P.b_schur, np.zeros(n), Mr)   # (a "sharded" S may be tiled differently: partial dots re-associated)
    assert gf[1] == ref_fold[1] and np.allclose(gf[2], ref_fold[2], rtol=1e-9, atol=1e-13 * ref_fold[2][0])
    v = np.random.default_rng(1).standard_normal(n)
    assert np.array_equal(S * v, S1 * v) and np.array_equal(M.ldiv(v), M1.ldiv(v)) and np.array_equal(Mr.ldiv(v), M1.ldiv(v))
    # a fully replicated pair on a context with a communicator is free to use the folded loop
    Sr = api.LocalSchurs(c2, P.Sd, P.sub.gather_idx, P.sub.node_Γ_cnt)
    assert_history(api.pcg(Sr, P.b_schur, np.zeros(n), Mr), orc.pcg(So, P.b_schur, np.zeros(n), Mo))


# ------------------------------------------------------------------ folded PCG (2 launches / iteration) vs the other loop forms
def test_folded_unfolded_and_eager_loops_agree(pkg, ctx, orc, fem):
    """pcg(S, b, x, ΠSnn) has three device forms: folded into the GEMVs (default), 4 launches with fused
    single-workgroup kernels (what a communicator or deflation selects), and multi-workgroup kernels.
    All must reproduce the oracle; here on strips (multiplicity 2 everywhere, slot width 2), on a 4x2
    partition (cross points, width 4) and with a non-zero initial guess."""
    import os
    import subprocess
    import sys
    api = pkg.api
    for (N, px, py, seed) in ((60, 3, 1, 3), (90, 4, 2, 5)):
        mesh = fem.get_mesh(N)
        P = fem.build_schur_problem(N, px, py, lognormal_coeff(fem, mesh.points, seed), f_m1, u0734)
        S, M = gpu_ops(pkg, ctx, P)
        So, Mo = orc_ops(orc, P)
        n, b = P.sub.n_Γ, P.b_schur
        for x0 in (np.zeros(n), np.random.default_rng(seed).standard_normal(n)):
            want = orc.pcg(So, b, x0, Mo)
            assert_history(api.pcg(S, b, x0, M), want)
            assert_history(api.pcg(S, b, x0, M, maxit=4), orc.pcg(So, b, x0, Mo, maxit=4))
    # the same solve with the fold / the fused kernels switched off (environment is read per solve)
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r + '/tests');"
            "import __graft_entry__ as g; from conftest import *; pkg = g.load_package(); fem, api = pkg.fem, pkg.api;"
            "P = fem.build_schur_problem(40, 2, 2, one, f_m1, u0734); ctx = api.Context(0);"
            "S = api.LocalSchurs(ctx, P.Sd, P.sub.gather_idx, P.sub.node_Γ_cnt);"
            "M = api.NeumannNeumannSchurPreconditioner(ctx, P.ΠSd, P.sub.gather_idx, P.sub.node_Γ_cnt);"
            "x, it, res = api.pcg(S, P.b_schur, np.zeros(P.sub.n_Γ), M); print(it, ' '.join(repr(float(v)) for v in res))")
    from conftest import ROOT
    outs = []
    for env in ({}, {"MI355_NO_FOLD": "1"}, {"MI355_NO_FOLD": "1", "MI355_NO_FUSED": "1"}):
        r = subprocess.run([sys.executable, "-c", code % (ROOT, ROOT)], env={**os.environ, **env},
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        tok = r.stdout.split()
        outs.append((int(tok[0]), np.array([float(t) for t in tok[1:]])))
    G = np.load(f"{GOLDEN}/micro.npz")
    for it, res in outs:
        assert it == int(G["pcg_it"])
        assert np.allclose(res, G["pcg_res_norm"], rtol=RES_RTOL, atol=RES_FLOOR * res[0])


def test_folded_deflated_loop(pkg, ctx, orc, fem, toy, ragged, monkeypatch):
    """defpcg(S, b, x, W, ΠSnn) in its folded form (3 launches per iteration: ΠS GEMV with the WtA*z partials, the small
    mu / W*mu kernel, S GEMV with the p-update) against the 5-launch form it replaces and against the oracle, for one,
    many and the maximum number of deflation vectors, zero and non-zero initial guesses. The environment is read at every
    solve."""
    api = pkg.api
    for P, nvecs in ((toy, (1, 14, 64)), (ragged, (3, 16))):
        S, M = gpu_ops(pkg, ctx, P)
        So, Mo = orc_ops(orc, P)
        n, b = P.sub.n_Γ, P.b_schur
        Wall = lowest_eigvecs(So, n, max(nvecs))
        for nvec in nvecs:
            W = np.asfortranarray(Wall[:, :nvec])
            for x0 in (np.zeros(n), np.random.default_rng(nvec).standard_normal(n)):
                want = orc.defpcg(So, b, x0, W, Mo)
                monkeypatch.delenv("MI355_NO_FOLD_DEFL", raising=False)
                folded = api.defpcg(S, b, x0, W, M)
                monkeypatch.setenv("MI355_NO_FOLD_DEFL", "1")
                unfolded = api.defpcg(S, b, x0, W, M)
                monkeypatch.delenv("MI355_NO_FOLD_DEFL")
                assert_history(folded, want)
                assert_history(unfolded, want)
                assert folded[1] == unfolded[1]
        # capped solves and the singular-WtAW convention (defcg.jl:273 `WtAW \\ mu`) are the same in the folded form
        W = np.asfortranarray(Wall[:, :4])
        assert_history(api.defpcg(S, b, np.zeros(n), W, M, maxit=3), orc.defpcg(So, b, np.zeros(n), W, Mo, maxit=3))
        Wsing = np.asfortranarray(np.column_stack([W[:, 0], W[:, 1], np.zeros(n)]))      # a zero column: U[3,3] == 0 exactly
        with pytest.raises(api.SingularException):
            api.defpcg(S, b, np.zeros(n), Wsing, M)


# ------------------------------------------------------------------ matrix-free operator with the interior CG on the device
def test_matrix_free_device_interior_cg(pkg, ctx, orc, ragged):
    """`apply_local_schurs(A_IIdd, A_IΓdd, A_ΓΓdd, ...; reltol)` with `IterativeSolvers.cg` as the interior solve
    (EPDD.jl:648-650): the device CG (batched over subdomains) against the oracle's restatement of the same iteration,
    and against the exact (direct interior solve) operator within the interior tolerance."""
    api = pkg.api
    P = ragged
    n = P.sub.n_Γ
    rng = np.random.default_rng(21)
    v = rng.standard_normal(n)
    for reltol in (1e-9, 1e-5):
        Sd = api.MatrixFreeLocalSchurs(ctx, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd, P.sub.gather_idx, P.sub.node_Γ_cnt, None, reltol=reltol)
        So = orc.apply_local_schurs_matfree_operator(P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd, P.sub.gather_idx, n,
                                                     orc.interior_cg_solvers(P.A_IIdd, reltol))
        got, want = Sd * v, So * v
        # Same iteration, different summation order inside the dots. Both are inexact solves that stop at
        # ||r|| <= reltol*||rhs||, so they agree to the order of that tolerance, not to rounding (measured:
        # 0.05*reltol between them, 0.07*reltol from the exact operator).
        assert np.allclose(got, want, rtol=0, atol=0.5 * reltol * np.abs(want).max())
    Sx = api.LocalSchurs(ctx, P.Sd, P.sub.gather_idx, P.sub.node_Γ_cnt)
    Sdev = api.MatrixFreeLocalSchurs(ctx, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd, P.sub.gather_idx, P.sub.node_Γ_cnt, None)
    exact = Sx * v
    assert np.allclose(Sdev * v, exact, rtol=0, atol=1e-7 * np.abs(exact).max())       # Example03:175 with inexact solves
    assert not np.any(Sdev * np.zeros(n))                                                # rhs = 0: zero iterations
    # NN-PCG on the inexact operator converges like on the exact one (Example03 runs exactly this with S_local)
    M = api.NeumannNeumannSchurPreconditioner(ctx, P.ΠSd, P.sub.gather_idx, P.sub.node_Γ_cnt)
    x, it, res = api.pcg(Sdev, P.b_schur, np.zeros(n), M)
    xe, ite, rese = api.pcg(Sx, P.b_schur, np.zeros(n), M)
    assert abs(it - ite) <= 1 and np.linalg.norm(x - xe) <= 1e-5 * np.linalg.norm(xe)


def test_whole_solve_graph_entry_exit_and_speculation(pkg, ctx, orc, toy, monkeypatch):
    """Undeflated solves replay ONE graph (entry kernel .. exit kernel, arguments through a pinned block) and the host waits
    for the exit's last store. The folded loop adds an entry built for x0 == 0 (chosen when the previous solve with the
    same operators had a zero guess, verified on the device, replayed in the general form otherwise) and hands the results
    over from the launch that meets the stop rule. All of it must be invisible: same x, it, history as the step-by-step
    path (MI355_NO_WHOLE_GRAPH=1), bit for bit, through every transition — zero guess, non-zero guess (mis-speculation),
    zero again, -0.0, a solve that needs more iterations than the replay holds, maxit hit, torch device vectors."""
    import torch
    api = pkg.api
    P = toy
    S, M = gpu_ops(pkg, ctx, P)
    n, b = P.sub.n_Γ, P.b_schur
    rng = np.random.default_rng(5)
    x1 = rng.standard_normal(n)
    negz = np.zeros(n); negz[::3] = -0.0
    cases = [dict(x=np.zeros(n)), dict(x=np.zeros(n)), dict(x=x1), dict(x=x1), dict(x=np.zeros(n)), dict(x=negz), dict(x=np.zeros(n), eps=1e-3),
             dict(x=np.zeros(n), eps=1e-12), dict(x=np.zeros(n), maxit=3), dict(x=x1, maxit=2), dict(x=np.zeros(n))]
    def run():
        out = []
        for c in cases:
            x, it, res = api.pcg(S, b, c["x"].copy(), M, maxit=c.get("maxit", 0), eps=c.get("eps", 1e-7))
            out.append((x.copy(), it, res.copy()))
        xt = torch.zeros(n, dtype=torch.float64, device="cuda")
        x, it, res = api.pcg(S, torch.from_numpy(b).cuda(), xt, M)
        out.append((x.cpu().numpy(), it, np.asarray(res).copy()))
        x, it, res = api.cg(S, b, np.zeros(n))                       # fused 4-launch loop: general entry, exit kernel in the graph
        out.append((x.copy(), it, res.copy()))
        return out
    got = run()
    monkeypatch.setenv("MI355_NO_WHOLE_GRAPH", "1")
    ref = run()
    monkeypatch.delenv("MI355_NO_WHOLE_GRAPH")
    for (x, it, res), (xr, itr, resr) in zip(got, ref):
        assert it == itr and np.array_equal(x, xr) and np.array_equal(res, resr)
    So, Mo = orc_ops(orc, P)
    assert_history(got[0], orc.pcg(So, b, np.zeros(n), Mo))
    assert_history(got[2], orc.pcg(So, b, x1.copy(), Mo))


def test_interior_cg_two_launch_form_and_diagonal_precond(pkg, ctx, orc, fem, ragged, monkeypatch):
    """MI355_ICG_FUSED=1 runs the interior CG in 2 launches per iteration (k_icg_spmv / k_icg_update_blk: the direction is
    formed on the fly from gathered (u, z) pairs; slower than the 3-launch default at 1 M DoF, kept as an opt-in). Both restate the same iteration
    (IterativeSolvers.cg, EPDD.jl:648-650), so they agree to the order of the interior tolerance, with the same bar as
    against the oracle. `interior_precond("diagonal")` is the `precond` keyword with Pl = Diagonal(A_IIdd): same answer
    to the interior tolerance, fewer iterations; new block values refresh the diagonal."""
    api = pkg.api
    P = ragged
    n = P.sub.n_Γ
    v = np.random.default_rng(22).standard_normal(n)
    args = (ctx, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd, P.sub.gather_idx, P.sub.node_Γ_cnt, None)
    for reltol in (1e-9, 1e-5):
        S3 = api.MatrixFreeLocalSchurs(*args, reltol=reltol)
        monkeypatch.setenv("MI355_ICG_FUSED", "1")
        S2 = api.MatrixFreeLocalSchurs(*args, reltol=reltol)
        monkeypatch.delenv("MI355_ICG_FUSED")
        So = orc.apply_local_schurs_matfree_operator(P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd, P.sub.gather_idx, n,
                                                     orc.interior_cg_solvers(P.A_IIdd, reltol))
        want = So * v
        bar = 0.5 * reltol * np.abs(want).max()
        y2, y3 = S2 * v, S3 * v
        assert np.allclose(y2, want, rtol=0, atol=bar) and np.allclose(y3, want, rtol=0, atol=bar)
        assert np.array_equal(S2 * v, y2)                                  # replays are deterministic
    exact = api.LocalSchurs(ctx, P.Sd, P.sub.gather_idx, P.sub.node_Γ_cnt) * v
    for fused in ("0", "1"):
        monkeypatch.setenv("MI355_ICG_FUSED", fused)
        Sp, Sj = api.MatrixFreeLocalSchurs(*args), api.MatrixFreeLocalSchurs(*args)
        monkeypatch.delenv("MI355_ICG_FUSED")
        Sj.interior_precond("diagonal")
        yp, yj = Sp * v, Sj * v
        assert np.allclose(yp, exact, rtol=0, atol=1e-7 * np.abs(exact).max())
        assert np.allclose(yj, exact, rtol=0, atol=1e-7 * np.abs(exact).max())
        assert 0 < Sj.interior_iterations() <= Sp.interior_iterations()
        assert not np.any(Sj * np.zeros(n))
        Sj.interior_precond(None)
        assert np.array_equal(Sj * v, yp)                                  # back to the plain iteration, bit for bit
    with pytest.raises(pkg.api.MiError):
        api.MatrixFreeLocalSchurs(*args[:-1], P.solvers).interior_precond("diagonal")   # host-callback interior solve: nothing to precondition
    # global-Schur form of the same solve (EPDD.jl:596-625)
    coeff = lognormal_coeff(fem, P.mesh.points, 7)
    A_IIg, A_IΓg, A_ΓΓ, _, _ = fem.prepare_global_schur(P.mesh.cells, P.mesh.points, P.epart, P.sub, coeff, f_m1, u0734)
    G = api.GlobalSchur(ctx, A_IIg, A_IΓg, A_ΓΓ, None)
    yg = G * v
    G.interior_precond("diagonal")
    assert np.allclose(G * v, yg, rtol=0, atol=1e-6 * np.abs(yg).max())


def test_deflation_with_many_vectors(pkg, ctx, orc, toy):
    """nvec > 64 takes the generic projection kernels (k_multi_dot_partial + k_lu_solve) instead of the one-wave
    solve inside the fused p-update; nvec = 1 and nvec = 64 sit on the edges of the in-kernel path."""
    api = pkg.api
    P = toy
    S, M = gpu_ops(pkg, ctx, P)
    So, Mo = orc_ops(orc, P)
    n, b = P.sub.n_Γ, P.b_schur
    Q = np.linalg.qr(np.random.default_rng(17).standard_normal((n, 70)))[0]
    for nvec in (1, 64, 70):
        W = np.asfortranarray(Q[:, :nvec])
        assert_history(api.defpcg(S, b, np.zeros(n), W, M), orc.defpcg(So, b, np.zeros(n), W, Mo))
        assert_history(api.defcg(S, b, np.zeros(n), W), orc.defcg(So, b, np.zeros(n), W), So, b)


@pytest.mark.parametrize("N,px,py,seed", [(12, 2, 1, 1), (17, 1, 3, 2), (23, 3, 3, 3), (31, 5, 2, 4), (41, 2, 5, 5),
                                           (64, 7, 1, 6), (37, 4, 4, 7)])
def test_shapes_sweep(pkg, ctx, orc, fem, N, px, py, seed):
    """Odd sizes on purpose: n_Γd not a multiple of 16 (row padding), subdomains with fewer rows than a workgroup
    tile, strips (multiplicity 2) and cross points (4), floating subdomains, very small Γ."""
    api = pkg.api
    mesh = fem.get_mesh(N)
    P = fem.build_schur_problem(N, px, py, lognormal_coeff(fem, mesh.points, seed), f_m1, u0734)
    n, b = P.sub.n_Γ, P.b_schur
    S, M = gpu_ops(pkg, ctx, P)
    So, Mo = orc_ops(orc, P)
    v = np.random.default_rng(seed).standard_normal(n)
    assert np.allclose(S * v, So * v, rtol=0, atol=1e-13 * np.abs(So * v).max())
    assert np.allclose(M.ldiv(v), Mo * v, rtol=0, atol=1e-13 * np.abs(Mo * v).max())
    # NN-PCG needs more than 20 iterations on the 10-16 subdomain cases ("Pcg performs worse for larger ndom",
    # Example03:26): pass the oracle operator for the long-run branch of assert_history
    assert_history(api.pcg(S, b, np.zeros(n), M), orc.pcg(So, b, np.zeros(n), Mo), So, b)
    assert_history(api.pcg(S, b, v, M), orc.pcg(So, b, v, Mo), So, b)
    assert_history(api.cg(S, b, np.zeros(n)), orc.cg(So, b, np.zeros(n)), So, b)
    nev = min(n - 1, P.sub.ndom + 3)
    W = lowest_eigvecs(So, n, nev)
    assert_history(api.defpcg(S, b, np.zeros(n), W, M), orc.defpcg(So, b, np.zeros(n), W, Mo), So, b)


def test_res_capacity_and_borrowed_stream(pkg, ctx, micro):
    """C-ABI corners: res_cap smaller than `it` -> MI_ERR_RES_CAPACITY after a completed solve (the reference's
    BoundsError on res_norm[it]); a borrowed hipStream_t (torch's) gives the same bits as the context's own."""
    import ctypes as C
    import torch
    api, L = pkg.api, pkg._lib.load()
    P = micro
    n, b = P.sub.n_Γ, P.b_schur
    c3 = api.Context(0)
    S, M = gpu_ops(pkg, c3, P)
    ref = api.pcg(S, b, np.zeros(n), M)
    # capacity 3 < it
    x = np.zeros(n)
    res = np.zeros(3)
    it = C.c_int64()
    c3._mode_for(b, x)
    rc = L.mi_pcg(S._h, M._h, C.c_void_p(b.ctypes.data), C.c_void_p(x.ctypes.data), 0, 1e-7,
                  res.ctypes.data_as(C.POINTER(C.c_double)), 3, C.byref(it))
    assert rc == pkg._lib.MI_ERR_RES_CAPACITY and it.value == ref[1]
    assert np.array_equal(res, ref[2][:3]) and np.array_equal(x, ref[0])      # the solve itself completed
    with pytest.raises(api.BoundsError):
        pkg._lib.check(rc)
    # borrowed stream
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c3.use_torch_stream()
        got = api.pcg(S, b, np.zeros(n), M)
        bt = torch.from_numpy(b).cuda()
        xt = torch.zeros(n, dtype=torch.float64, device="cuda")
        api.pcg(S, bt, xt, M)
        st.synchronize()
    assert got[1] == ref[1] and np.array_equal(got[2], ref[2]) and np.array_equal(got[0], ref[0])
    assert np.array_equal(xt.cpu().numpy(), ref[0])
    assert L.mi_ctx_set_stream(c3._h, None) == 0                               # back to the context's own stream
    again = api.pcg(S, b, np.zeros(n), M)
    assert np.array_equal(again[0], ref[0])


def test_initial_guess_zero_shortcut_and_nonzero_guesses(pkg, ctx, orc, ragged):
    """The set-up `r = b - A*x0` skips streaming A when x0 is identically zero (device flag set by the solve's entry
    kernel). Alternate zero / non-zero / signed-zero / partly-zero guesses on the same operators: every solve must match
    the oracle from the same guess — a stale flag would show as a wrong first residual."""
    api = pkg.api
    P = ragged
    S, M = gpu_ops(pkg, ctx, P)
    So, Mo = orc_ops(orc, P)
    n, b = P.sub.n_Γ, P.b_schur
    rng = np.random.default_rng(12)
    part = np.zeros(n); part[n // 2] = 1e-300
    guesses = [np.zeros(n), rng.standard_normal(n), np.zeros(n), -np.zeros(n), part, np.zeros(n), rng.standard_normal(n)]
    for x0 in guesses:
        for solver, osolver, args, oargs in ((api.pcg, orc.pcg, (M,), (Mo,)), (api.cg, orc.cg, (), ())):
            got = solver(S, b, x0.copy(), *args)
            want = osolver(So, b, x0.copy(), *oargs)
            assert np.isclose(got[2][0], want[2][0], rtol=1e-12), "first residual: wrong x0 handling"
            if not x0.any() or max(got[1], want[1]) > TIGHT_PREFIX:
                assert_history(got, want, apply=So, b=b)
                continue
            # a random guess makes res_1 ~ 1e3 ||b||: the solve runs nine orders down from res_1 and the last entries sit
            # at the floor of assert_history's bar (|Δ| ~ 1e-12 res_1); hold `it`, the history to 1e-6 (+1e-11 res_1)
            # and the true residual instead
            assert abs(got[1] - want[1]) <= max(1, want[1] // 50)
            m = min(got[1], want[1])
            assert np.allclose(got[2][:m], want[2][:m], rtol=1e-6, atol=1e-11 * want[2][0])
            assert np.linalg.norm(b - So(got[0])) <= 2.0 * max(got[2][-1], 1e-7 * np.linalg.norm(b))
    import torch
    bt = torch.from_numpy(b).cuda()
    for x0 in guesses[:3]:
        xt = torch.from_numpy(x0.copy()).cuda()
        got = api.pcg(S, bt, xt, M)
        want = orc.pcg(So, b, x0.copy(), Mo)
        assert got[1] == want[1] and np.isclose(got[2][0], want[2][0], rtol=1e-12)


def test_apply_local_schur_single_subdomain(pkg, ctx, ragged):
    """a7 (EPDD.jl:639-654): one subdomain in its own Γ_d numbering, against the assembled S_d of the same subdomain
    (host callback: sparse-direct interior solve; device: interior CG to reltol 1e-11)."""
    api = pkg.api
    P = ragged
    rng = np.random.default_rng(21)
    for d in (0, P.sub.ndom - 1):
        xd = rng.standard_normal(P.sub.n_Γd[d])
        want = P.Sd[d] @ xd
        for solver, tol in ((P.solvers[d], 1e-10), (None, 1e-7)):
            S_d = api.LocalSchur(ctx, P.A_IIdd[d], P.A_IΓdd[d], P.A_ΓΓdd[d], solver, reltol=1e-11)
            got = api.apply_local_schur(S_d, xd)
            assert np.linalg.norm(got - want) <= tol * np.linalg.norm(want)


@pytest.mark.parametrize("world,replicate_precond", [(2, True), (2, False), (4, True), (3, False), (8, True)])
def test_sharded_operators_with_in_process_ranks(pkg, orc, fem, world, replicate_precond):
    """SURVEY.md §8(e) on ONE GPU: `world` contexts of this process, one thread each, joined by the loopback communicator
    (RCCL refuses two ranks on a device). Every rank builds its slice of the subdomains (`dom_slice`), S is sharded, the
    NN blocks are replicated (bench.py's default) or sharded too; all ranks must return the SAME bits, equal to the
    single-context loop of the same form (the sums over ranks are unions: x + 0), and match the oracle."""
    import os
    import threading
    api = pkg.api
    N, px, py = 90, 4, 2
    mesh = fem.get_mesh(N)
    coeff = lognormal_coeff(fem, mesh.points, 5)
    P = fem.build_schur_problem(N, px, py, coeff, f_m1, u0734)
    ndom, n, b = P.sub.ndom, P.sub.n_Γ, P.b_schur
    gi, cnt = P.sub.gather_idx, P.sub.node_Γ_cnt
    group = api.LoopbackGroup(world)
    out, errs = [None] * world, []
    # NN blocks sharded too: here the 4-launch loop (bit-identical to the same loop on one context); the folded form with
    # an exchange behind both launches is tests/test_gpu_multirank.py's
    if not replicate_precond:
        os.environ["MI355_NO_FOLD_SHARDED_NN"] = "1"

    def rank_main(r):
        try:
            ctx = api.Context(0)
            ctx.loopback_init(group, r)
            lo, hi = api.shard_domains(ndom, r, world)
            Sd = [P.Sd[d] if lo <= d < hi else None for d in range(ndom)]
            S = api.LocalSchurs(ctx, Sd, gi, cnt, dom_slice=(lo, hi))
            if replicate_precond:
                M = api.NeumannNeumannSchurPreconditioner(ctx, P.ΠSd, gi, cnt, dom_slice=(0, ndom))
            else:
                Pd = [P.ΠSd[d] if lo <= d < hi else None for d in range(ndom)]
                M = api.NeumannNeumannSchurPreconditioner(ctx, Pd, gi, cnt, dom_slice=(lo, hi))
            y = S * b                                            # a sharded apply: every rank gets the full Γ vector
            res = api.pcg(S, b, np.zeros(n), M)
            res_cg = api.cg(S, b, np.zeros(n), maxit=25)
            ymf = None
            if world == 2:                                       # the matrix-free operator, sharded the same way
                Smf = api.MatrixFreeLocalSchurs(ctx, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd, gi, cnt, P.solvers, dom_slice=(lo, hi))
                ymf = Smf * b
            out[r] = (y, res, res_cg, ymf)
        except Exception as e:                                   # noqa: BLE001
            errs.append((r, repr(e)))

    threads = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    os.environ.pop("MI355_NO_FOLD_SHARDED_NN", None)
    assert not errs, errs
    assert all(o is not None for o in out), "a rank did not finish"
    for r in range(1, world):                                    # ranks stay bit-identical
        assert np.array_equal(out[r][0], out[0][0])
        assert out[r][1][1] == out[0][1][1] and np.array_equal(out[r][1][2], out[0][1][2]) and np.array_equal(out[r][1][0], out[0][1][0])
        assert np.array_equal(out[r][2][0], out[0][2][0])
    # single context, same (unfolded) loop: identical bits; and the oracle to the usual bar
    ctx1 = api.Context(0)
    S1 = api.LocalSchurs(ctx1, P.Sd, gi, cnt)
    M1 = api.NeumannNeumannSchurPreconditioner(ctx1, P.ΠSd, gi, cnt)
    assert np.array_equal(out[0][0], S1 * b)
    # S sharded + NN replicated runs the FOLDED loop across the ranks (one all-reduce after the S launch); with the NN
    # blocks sharded too the 4-launch loop runs: compare with the same loop form on one context
    if not replicate_precond:
        os.environ["MI355_NO_FOLD"] = "1"
    try:
        ref = api.pcg(S1, b, np.zeros(n), M1)
        ref_cg = api.cg(S1, b, np.zeros(n), maxit=25)
    finally:
        os.environ.pop("MI355_NO_FOLD", None)
    if replicate_precond:
        # folded loop: a sharded S cuts its blocks into smaller tiles than the single-GPU operator, so the per-tile
        # partials of p'Ap are associated differently — rounding-level differences, `it` equal
        assert out[0][1][1] == ref[1] and np.allclose(out[0][1][2], ref[2], rtol=1e-9, atol=1e-13 * ref[2][0])
        assert np.linalg.norm(out[0][1][0] - ref[0]) <= 1e-9 * np.linalg.norm(ref[0])
    else:
        assert out[0][1][1] == ref[1] and np.array_equal(out[0][1][2], ref[2]) and np.array_equal(out[0][1][0], ref[0])
    assert np.array_equal(out[0][2][2], ref_cg[2])
    if world == 2:    # matrix-free: per-rank partial Γ-sums are added by the all-reduce (same value, another rounding order)
        assert np.array_equal(out[0][3], out[1][3])
        assert np.allclose(out[0][3], out[0][0], rtol=1e-9, atol=1e-11 * np.abs(out[0][0]).max())
    So, Mo = orc_ops(orc, P)
    assert_history(out[0][1], orc.pcg(So, b, np.zeros(n), Mo))


def test_sharded_deflated_and_recycling_solvers_with_in_process_ranks(pkg, orc, fem):
    """defpcg / eigpcg / eigdefpcg on 2 in-process ranks (S sharded, NN replicated): these run the 4-launch loop with an
    all-reduce of the slot table after every S-apply (also for `WtA = (A W)'` and eigpcg's `A*V`). All ranks identical,
    and equal to the single-context run: bit for bit for defpcg (same kernels, union of slot tables), to the recycled-space
    bar for the eig solvers' vectors."""
    import threading
    from test_gpu_eig import assert_space
    api = pkg.api
    N, px, py, world = 60, 3, 2, 2
    mesh = fem.get_mesh(N)
    P = fem.build_schur_problem(N, px, py, lognormal_coeff(fem, mesh.points, 9), f_m1, u0734)
    ndom, n, b = P.sub.ndom, P.sub.n_Γ, P.b_schur
    gi, cnt = P.sub.gather_idx, P.sub.node_Γ_cnt
    So, Mo = orc_ops(orc, P)
    nvec, spdim = int(1.25 * ndom), 3 * ndom
    W = orc.eigpcg(So, b, np.zeros(n), Mo, nvec, spdim)[3]
    b2 = So(np.random.default_rng(2).standard_normal(n))
    group = api.LoopbackGroup(world)
    out, errs = [None] * world, []

    def solves(S, M):
        return (api.defpcg(S, b2, np.zeros(n), W, M), api.eigpcg(S, b, np.zeros(n), M, nvec, spdim),
                api.eigdefpcg(S, b2, np.zeros(n), M, W, spdim))

    def rank_main(r):
        try:
            ctx = api.Context(0)
            ctx.loopback_init(group, r)
            lo, hi = api.shard_domains(ndom, r, world)
            S = api.LocalSchurs(ctx, [P.Sd[d] if lo <= d < hi else None for d in range(ndom)], gi, cnt, dom_slice=(lo, hi))
            M = api.NeumannNeumannSchurPreconditioner(ctx, P.ΠSd, gi, cnt, dom_slice=(0, ndom))
            out[r] = solves(S, M)
        except Exception as e:                                   # noqa: BLE001
            errs.append((r, repr(e)))

    threads = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errs, errs
    assert all(o is not None for o in out)
    for k in range(3):                                           # ranks identical
        assert out[0][k][1] == out[1][k][1] and np.array_equal(out[0][k][2], out[1][k][2]) and np.array_equal(out[0][k][0], out[1][k][0])
    ctx1 = api.Context(0)
    ref = solves(api.LocalSchurs(ctx1, P.Sd, gi, cnt), api.NeumannNeumannSchurPreconditioner(ctx1, P.ΠSd, gi, cnt))
    assert out[0][0][1] == ref[0][1] and np.allclose(out[0][0][2], ref[0][2], rtol=1e-9, atol=1e-13 * ref[0][2][0])
    for k in (1, 2):
        assert out[0][k][1] == ref[k][1] and np.allclose(out[0][k][2], ref[k][2], rtol=1e-8, atol=1e-12 * ref[k][2][0])
        assert_space(So, out[0][k][3], ref[k][3])
    assert_history(out[0][0][:3], orc.defpcg(So, b2, np.zeros(n), W, Mo))
