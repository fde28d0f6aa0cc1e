"""GPU suite (-m gpu): the matrix-free covariance kernel (csrc/cov_kernels.hpp), the operator C = M K M (csrc/kl.hpp) and the
Karhunen-Loève drivers of api.py, through the C ABI, against tests/kl_ref.py (dense numpy restatement of the reference).

Tolerance of the kernel cases — derived, not measured (kl_ref.kernel_bound): with t_ij the magnitude of the exponent,
    |Y - Y_ref|_i <= 2 eps Σ_j (ns + 4 min(t_ij, 745) + 16) K_ij |X_j|,   eps = 2^-52
(the summation; the rounding of the exponent amplified by exp; exp's own ulp and the products; 2 for the restatement's own
rounding). A wrong index or a dropped tail breaks it by many orders of magnitude.

Edges come from mi_cov_tiling: row_tile rows per workgroup, src_chunk sources per LDS chunk, col_block columns per thread,
and the split of the sources over workgroups when the rows alone do not fill the device. Kernel cases run twice: with host
pointers (staged, compact) and with device pointers, where the kernel itself sees ldx > ns and ldy > nt."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sla

import kl_ref as ref
import lanczos_ref as lz

pytestmark = pytest.mark.gpu

EPS = ref.EPS
TOL = 1e-10
SENT = -7.25e300            # sentinel in the padding rows of X and Y


def _model(pkg, name):
    return {"SExp": pkg._lib.MI_COV_SEXP, "Exp": pkg._lib.MI_COV_EXP}[name]


def raw_cov(pkg, ctx, model, sig2, L, pt, ps, X, ldx, ldy, device):
    """mi_cov_apply on X (ns x m) embedded in leading dimension ldx, Y in ldy; padding rows hold SENT. Returns (Y, Xpad, Ypad)
    after the call. `pt is ps` passes one pointer for both."""
    Lb = pkg._lib.load()
    nt, ns, m = pt.shape[1], ps.shape[1], X.shape[1]
    Xp = np.full((m, ldx), SENT); Xp[:, :ns] = X.T            # row c of this C-ordered array = column c, leading dimension ldx
    Yp = np.full((m, ldy), SENT)
    ptm = np.ascontiguousarray(pt.T)
    psm = ptm if ps is pt else np.ascontiguousarray(ps.T)
    args = lambda a, b, x, y: (ctx._h, C.c_int(_model(pkg, model)), C.c_double(sig2), C.c_double(L), C.c_int64(nt), a, C.c_int64(ns), b,   # noqa: E731
                               C.c_int64(m), x, C.c_int64(ldx), y, C.c_int64(ldy))
    if not device:
        assert Lb.mi_ctx_set_pointer_mode(ctx._h, 0) == 0
        rc = Lb.mi_cov_apply(*args(C.c_void_p(ptm.ctypes.data), C.c_void_p(psm.ctypes.data), C.c_void_p(Xp.ctypes.data), C.c_void_p(Yp.ctypes.data)))
        assert rc == 0, Lb.mi_last_error()
        return Yp[:, :nt].T.copy(), Xp, Yp
    import torch
    tp, tX, tY = torch.from_numpy(ptm).cuda(), torch.from_numpy(Xp).cuda(), torch.from_numpy(Yp).cuda()
    tq = tp if ps is pt else torch.from_numpy(psm).cuda()
    torch.cuda.synchronize()
    assert Lb.mi_ctx_set_pointer_mode(ctx._h, 1) == 0
    try:
        rc = Lb.mi_cov_apply(*args(C.c_void_p(tp.data_ptr()), C.c_void_p(tq.data_ptr()), C.c_void_p(tX.data_ptr()), C.c_void_p(tY.data_ptr())))
        assert rc == 0, Lb.mi_last_error()
        ctx.synchronize()
    finally:
        Lb.mi_ctx_set_pointer_mode(ctx._h, 0)
    Xp, Yp = tX.cpu().numpy(), tY.cpu().numpy()
    return Yp[:, :nt].T.copy(), Xp, Yp


def check_case(pkg, ctx, model, sig2, L, pt, ps, X, tag):
    """both pointer modes: the bound, untouched padding, equal bits between the modes and from call to call"""
    nt, ns = pt.shape[1], ps.shape[1]
    Yref = ref.dense_K(model, sig2, L, pt, ps) @ X
    bound = ref.kernel_bound(model, sig2, L, pt, ps, X)
    got = []
    for device in (False, True):
        Y, Xp, Yp = raw_cov(pkg, ctx, model, sig2, L, pt, ps, X, ns + 3, nt + 5, device)
        err = np.abs(Y - Yref)
        worst = float(np.max(err / np.maximum(bound, 1e-300)))
        print(f"  {tag} {'device' if device else 'host'} pointers: nt {nt} ns {ns} m {X.shape[1]} splits {pkg.api.cov_tiling(nt, ns, X.shape[1])[3]}: "
              f"max err {err.max():.2e}, err / bound {worst:.3f}")
        assert np.all(np.isfinite(Y)) and np.all(err <= bound), (tag, worst)
        assert np.all(Xp[:, ns:] == SENT) and np.all(Yp[:, nt:] == SENT) and np.array_equal(Xp[:, :ns], X.T)
        got.append(Y)
    assert np.array_equal(got[0], got[1])
    again = raw_cov(pkg, ctx, model, sig2, L, pt, ps, X, ns + 3, nt + 5, True)[0]
    assert np.array_equal(again, got[1])
    return got[0]


def mixed(rng, ns, m):
    """mixed sign with exact zeros"""
    X = rng.standard_normal((ns, m))
    X[rng.random((ns, m)) < 0.2] = 0.0
    return X


def test_kernel_row_and_source_edges(pkg, ctx):
    rt, sc, cb, _ = pkg.api.cov_tiling(1, 1, 1)
    rng = np.random.default_rng(0)
    ms = [1, 2, cb - 1, cb, cb + 1, 2 * cb + 3]
    k = 0
    for nt in (1, rt - 1, rt, rt + 1):
        for ns in (1, sc - 1, sc, sc + 1, 2 * sc + 3):
            m = ms[k % len(ms)]; k += 1
            model = "SExp" if k % 2 else "Exp"
            check_case(pkg, ctx, model, 1.7, 0.3, rng.random((2, nt)), rng.random((2, ns)), mixed(rng, ns, m), f"edge[{model}]")


def test_kernel_column_edges_split_and_unsplit(pkg, ctx):
    rt, sc, cb, _ = pkg.api.cov_tiling(1, 1, 1)
    rng = np.random.default_rng(1)
    nt, ns = rt + 1, 2 * sc + 3
    pt, ps = rng.random((2, nt)), rng.random((2, ns))
    for m in (1, 2, cb - 1, cb, cb + 1, 2 * cb + 3):
        assert pkg.api.cov_tiling(nt, ns, m)[3] > 1 and ns % sc != 0        # the last split is ragged
        check_case(pkg, ctx, "SExp", 1.0, 0.25, pt, ps, mixed(rng, ns, m), "split")
    # enough column blocks to fill the grid: no split, two source chunks in one workgroup
    m = 256 * cb + 1
    assert pkg.api.cov_tiling(3, sc + 1, m)[3] == 1
    check_case(pkg, ctx, "Exp", 0.5, 0.4, rng.random((2, 3)), rng.random((2, sc + 1)), mixed(rng, sc + 1, m), "unsplit")
    assert pkg.api.cov_tiling(nt, sc, 1)[3] == 1
    check_case(pkg, ctx, "SExp", 1.0, 0.25, pt, ps[:, :sc].copy(), mixed(rng, sc, 1), "unsplit")


def test_kernel_values_coincident_far_and_duplicated_points(pkg, ctx):
    rng = np.random.default_rng(2)
    n = 700
    p = rng.random((2, n))
    # targets == sources (one pointer), L = 0.02 on the unit square: far pairs underflow
    t = ref.exponent("SExp", 1.0, 0.02, p, p)
    assert (t > ref.T_CAP).mean() > 0.25
    X = mixed(rng, n, 3)
    check_case(pkg, ctx, "SExp", 2.5, 0.02, p, p, X, "far")
    # coincident points give exactly sig2: K e_j at the same point
    e = np.zeros((n, 1)); e[123, 0] = 1.0
    for model in ("SExp", "Exp"):
        Y = check_case(pkg, ctx, model, 2.5, 0.02, p, p, e, "unit")
        assert Y[123, 0] == 2.5 and Y.max() == 2.5
    # Exp with duplicated points: sqrt(0), equal rows
    q = p.copy(); q[:, 1::2] = q[:, 0:-1:2]
    Y = check_case(pkg, ctx, "Exp", 1.0, 0.3, q, q, X, "dup")
    assert np.array_equal(Y[0::2], Y[1::2]) and np.all(np.isfinite(Y))


# ------------------------------------------------------------------ operator
def _spmv_err(Mabs, v):
    """2 x the rounding of a CSR row sum of at most 7 products (P1 mass matrix), entrywise: 2 * 8 eps |M| |v|"""
    return 16 * EPS * (Mabs @ np.abs(v))


def c_apply_bound(M, K, pts, model, sig2, L, x):
    """the kernel bound carried through the two SpMVs of y = M (K (M x))"""
    Mabs = np.abs(M)
    u = M @ x
    du = _spmv_err(Mabs, x)
    dv = ref.kernel_bound(model, sig2, L, pts, pts, u)[:, 0] + K @ du
    return Mabs @ dv + _spmv_err(Mabs, K @ np.abs(u))


def test_operator_against_dense_C_and_symmetry(pkg, ctx, fem):
    api = pkg.api
    mesh, M, K, Cd, lam, V = ref.problem400(fem)
    n = 400
    op = api.CovarianceOperator(ctx, mesh.points, fem.get_mass_matrix(mesh.cells, mesh.points), "SExp", ref.SIG2, ref.L_GLOBAL)
    try:
        assert op.n == n and op.bytes()[1] == 48 * n and op.bytes()[0] > op.bytes()[1]
        rng = np.random.default_rng(5)
        x, y = mixed(rng, n, 1)[:, 0], rng.standard_normal(n)
        Cx, Cy = op * x, op * y
        bx, by = c_apply_bound(M, K, mesh.points, "SExp", ref.SIG2, ref.L_GLOBAL, x), c_apply_bound(M, K, mesh.points, "SExp", ref.SIG2, ref.L_GLOBAL, y)
        print(f"  C x: max err {np.abs(Cx - Cd @ x).max():.2e}, err / bound {np.max(np.abs(Cx - Cd @ x) / bx):.3f}")
        assert np.all(np.abs(Cx - Cd @ x) <= bx) and np.all(np.abs(Cy - Cd @ y) <= by)
        assert np.array_equal(op * x, Cx)                                        # bitwise from call to call
        sym = abs(x @ Cy - y @ Cx)
        bar = np.abs(x) @ by + np.abs(y) @ bx + 2 * n * EPS * (np.abs(x) @ (Cd @ np.abs(y)))
        print(f"  |x'Cy - y'Cx| = {sym:.2e} (bar {bar:.2e})")
        assert sym <= bar
        import torch
        xd = torch.from_numpy(x).cuda()
        assert np.array_equal((op * xd).cpu().numpy(), Cx)                       # device pointers: the same bits
        op.apply_dominant(x, 2)
        assert op.time_dominant(x, 3) > 0
    finally:
        op.close()


def test_panel_apply_inside_defcg_equals_single_applies(pkg, ctx, fem):
    """defcg forms A W through Operator::apply_multi: the covariance operator answers with its panel kernel (10 columns: a
    panel of col_block and one of 2), a CSR copy of the dense C with single applies. Same solver, same W, six iterations;
    the two operators differ by O(eps) relative, W'CW of a random W has a condition number far below 1e8, so x and the
    residual history agree to 1e-6 relative — a wrong column or leading dimension in the panel path is an O(1) difference."""
    import scipy.sparse as sp
    api = pkg.api
    mesh, M, K, Cd, lam, V = ref.problem400(fem)
    rng = np.random.default_rng(9)
    b, W = rng.standard_normal(400), np.asfortranarray(rng.standard_normal((400, 10)))
    assert np.linalg.cond(W.T @ Cd @ W) < 1e8
    op = api.CovarianceOperator(ctx, mesh.points, fem.get_mass_matrix(mesh.cells, mesh.points), "SExp", ref.SIG2, ref.L_GLOBAL)
    dense = api.SparseMatrixCSC(ctx, sp.csr_matrix(Cd))
    try:
        x1, it1, r1 = api.defcg(op, b, np.zeros(400), W, maxit=6)[:3]
        x2, it2, r2 = api.defcg(dense, b, np.zeros(400), W, maxit=6)[:3]
    finally:
        op.close()
        dense.close()
    dx = np.linalg.norm(x1 - x2) / np.linalg.norm(x2)
    print(f"  defcg, 10 deflation vectors: it {it1} / {it2}, |x_panel - x_single| / |x| = {dx:.2e}")
    assert it1 == it2 and dx <= 1e-6 and np.allclose(r1, r2, rtol=1e-6, atol=0)
    assert abs(W.T @ (b - Cd @ x1)).max() <= 1e-6 * np.linalg.norm(b)         # the deflation property the panel product feeds


@pytest.mark.parametrize("nev", [1, 4, 8])
def test_solve_kl_against_eigh(pkg, ctx, fem, nev):
    """400 nodes, L = 0.3: the dense spectrum has gaps >= 1.7e-2 behind λ_1, λ_4 and λ_8. The operator is replayed inside
    mi_eigsolve's graphs."""
    api = pkg.api
    mesh, M, K, Cd, lam, V = ref.problem400(fem)
    gap = lam[nev - 1] - lam[nev]
    assert gap >= 1.7e-2
    before = ctx.query("graph_replays")
    Λ, Φ = api.solve_kl(ctx, mesh.cells, mesh.points, nev, "SExp", ref.SIG2, ref.L_GLOBAL, relative=0.99, tol=TOL, verbose=False)
    assert ctx.query("graph_replays") > before
    assert Λ.shape == (nev,) and Φ.shape == (400, nev)                          # Σ_1..8 λ = 0.80 < 0.99: nothing truncated
    verr, O, ang = np.abs(Λ - lam[:nev]).max(), lz.ortho_defect(Φ, M), lz.sin_largest_angle(Φ, V[:, :nev], M)
    print(f"  nev {nev}: |θ-λ| {verr:.2e} (bar {10 * TOL:.0e}), |Φ'MΦ - I| {O:.2e}, sin θ {ang:.2e} (bar {10 * TOL / gap:.2e})")
    assert verr <= 10 * TOL and O <= 10 * TOL and ang <= 10 * TOL / gap


def test_solve_kl_truncates_like_the_reference(pkg, ctx, fem):
    mesh, M, K, Cd, lam, V = ref.problem400(fem)
    Λ, Φ = pkg.api.solve_kl(ctx, mesh.cells, mesh.points, 8, "SExp", ref.SIG2, ref.L_GLOBAL, relative=0.5, tol=TOL, verbose=False)
    assert Λ.size == 4 and Φ.shape == (400, 4) and np.abs(Λ - lam[:4]).max() <= 10 * TOL


# ------------------------------------------------------------------ domain-decomposition pipeline
@pytest.fixture(scope="module")
def dd(pkg, ctx, fem):
    """400 nodes, 4 x 4 boxes, L = 0.1, local nev = 6: the device's local solves, once"""
    mesh = fem.get_mesh(ref.N_SIDE)
    epart, _ = fem.mesh_partition(mesh, 4, 4)
    rel_local, rel_global = fem.suggest_parameters(400)
    subs = [pkg.api.solve_local_kl(ctx, mesh.cells, mesh.points, epart, 6, d, "SExp", 1.0, 0.1, relative=rel_local, tol=TOL, verbose=False)
            for d in range(16)]
    return mesh, epart, subs, rel_local, rel_global


def test_dd_local_pairs(pkg, fem, dd):
    mesh, epart, subs, rel_local, _ = dd
    cells, points = mesh.cells, mesh.points
    for d, s in enumerate(subs):
        l2g, elems, center = ref.set_subdomain(cells, points, epart, d)
        assert np.array_equal(s.inds_l2g, l2g) and np.array_equal(s.elems, elems)
        Md = ref.dense_mass(cells, points, l2g, elems)
        Cd = Md @ ref.dense_K("SExp", 1.0, 0.1, points[:, l2g], points[:, l2g]) @ Md
        lam, V = ref.eigh_desc(Cd, Md)
        Area = ref.energy(cells, points, elems)[0]
        nvec = ref.keep(lam[:6], rel_local * Area * 1.0)[0]
        k = s.Φ.shape[1]
        gap = lam[k - 1] - lam[k]
        verr, O, ang = np.abs(s.λ - lam[:6]).max(), lz.ortho_defect(s.Φ, Md), lz.sin_largest_angle(s.Φ, V[:, :k], Md)
        if d in (0, 5, 15):
            print(f"  idom {d}: n {l2g.size}, kept {k}/6, |θ-λ| {verr:.2e}, |Φ'MΦ - I| {O:.2e}, sin θ {ang:.2e} (bar {10 * TOL / gap:.2e})")
        assert k == nvec and abs(s.energy - Area) <= 1e-14
        assert verr <= 10 * TOL and O <= 10 * TOL and ang <= 10 * TOL / gap


def test_dd_reduced_assembly_global_modes_and_draw(pkg, ctx, fem, dd):
    api = pkg.api
    mesh, epart, subs, _, rel_global = dd
    points, L, sig2 = mesh.points, 0.1, 1.0
    Φd, centerd = [s.Φ for s in subs], [s.center for s in subs]
    md = [P.shape[1] for P in Φd]
    off = np.concatenate([[0], np.cumsum(md)])
    K = api.do_global_mass_covariance_reduced_assembly(ctx, points, subs, Φd, centerd, "SExp", sig2, L, forget=-1.0)
    assert K.shape == (off[-1], off[-1]) and np.array_equal(K, K.T)
    worst = 0.0
    for i in range(16):
        for j in range(i, 16):
            Mi, Mj = subs[i].M.toarray(), subs[j].M.toarray()
            Pi, Pj = points[:, subs[i].inds_l2g], points[:, subs[j].inds_l2g]
            want = ref.reduced_block("SExp", sig2, L, points, subs[i].inds_l2g, Mi, Φd[i], subs[j].inds_l2g, Mj, Φd[j])
            # Φ_i' M_i (kernel bound on K (M_j Φ_j)) + the host products in either association: (n_i + n_j + 16) roundings
            # of |Φ_i|' |M_i| K |M_j| |Φ_j|, twice (both sides)
            Kd = ref.dense_K("SExp", sig2, L, Pi, Pj)
            A, B = np.abs(Φd[i]).T @ np.abs(Mi), np.abs(Mj) @ np.abs(Φd[j])
            bar = A @ ref.kernel_bound("SExp", sig2, L, Pi, Pj, Mj @ Φd[j]) + 4 * (Mi.shape[0] + Mj.shape[0] + 16) * EPS * (A @ Kd @ B)
            got = K[off[i]:off[i + 1], off[j]:off[j + 1]]
            if i == j:
                got, want, bar = np.triu(got), np.triu(want), np.triu(bar) + 1e-300
            worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(bar, 1e-300))))
            assert np.all(np.abs(got - want) <= bar), (i, j)
    print(f"  reduced K {K.shape}: worst err / bound {worst:.3f}")
    # forget = 1e-6: exactly the blocks whose centres are further apart than L sqrt(ln 1e6) are zero, the others keep their bits
    Kf = api.do_global_mass_covariance_reduced_assembly(ctx, points, subs, Φd, centerd, "SExp", sig2, L, forget=1e-6)
    far = L * np.sqrt(np.log(1e6))
    nzero = 0
    for i in range(16):
        for j in range(16):
            dist = float(np.hypot(*(centerd[i] - centerd[j])))
            assert abs(dist - far) > 1e-9
            blk = Kf[off[i]:off[i + 1], off[j]:off[j + 1]]
            if dist > far:
                nzero += 1
                assert np.all(blk == 0.0)
            else:
                assert np.array_equal(blk, K[off[i]:off[i + 1], off[j]:off[j + 1]])
    assert 0 < nzero < 256 and np.array_equal(Kf, Kf.T)
    # global reduced problem on the device's K
    energy = sum(s.energy for s in subs)
    l2gd = [s.inds_l2g for s in subs]
    Λ, Ψ = fem.solve_global_reduced_kl(400, K, energy, [s.elems for s in subs], l2gd, Φd, relative=rel_global, verbose=False)
    w, Φr = sla.eigh(K)
    w, Φr = w[::-1], Φr[:, ::-1]
    nvec = Λ.size
    assert 0 < nvec <= int((w > 0).sum()) and np.abs(Λ - w[:nvec]).max() <= 1e-12 * w[0]
    wpos = w[:int((w >= 0).sum())]                                # trim_and_order drops the negative values only
    reached = np.flatnonzero(np.cumsum(wpos) >= rel_global * energy)
    want_nvec = int(reached[0]) + 1 if reached.size else wpos.size  # KLDD.jl:797-801: until the energy is reached, else all
    assert nvec == want_nvec
    wu, Φu = fem.trim_and_order(*sla.eigh(K, lower=False))
    assert np.abs(Ψ - ref.project_on_mesh(400, Φu[:, :nvec], l2gd, Φd)).max() <= 1e-13
    kl = fem.SyntheticKL(Λ, Ψ)
    ξ, g = fem.draw(kl, np.random.default_rng(42))
    assert np.array_equal(ξ, np.random.default_rng(42).standard_normal(nvec))
    assert np.abs(g - ref.draw(Λ, Ψ, ξ)).max() <= 1e-13 * max(1.0, np.abs(g).max()) and np.all(np.isfinite(g))
    print(f"  global: {nvec}/{w.size} modes kept, Λ_1 {Λ[0]:.4f}, |g|_max {np.abs(g).max():.3f}")


# ------------------------------------------------------------------ arguments
def test_bad_arguments_leave_y_untouched(pkg, ctx, fem):
    Lb = pkg._lib.load()
    BAD = pkg._lib.MI_ERR_BAD_ARG
    assert Lb.mi_ctx_set_pointer_mode(ctx._h, 0) == 0
    n, m = 5, 2
    p = np.ascontiguousarray(np.random.default_rng(0).random((n, 2)))
    X = np.ones((m, n)); Y = np.full((m, n), SENT)
    vp, i64, f64 = C.c_void_p, C.c_int64, C.c_double
    P, XP, YP = vp(p.ctypes.data), vp(X.ctypes.data), vp(Y.ctypes.data)
    good = dict(ctx=ctx._h, model=0, sig2=1.0, L=0.1, nt=n, pt=P, ns=n, ps=P, m=m, X=XP, ldx=n, Y=YP, ldy=n)

    def call(**kw):
        a = dict(good, **kw)
        return Lb.mi_cov_apply(a["ctx"], C.c_int(a["model"]), f64(a["sig2"]), f64(a["L"]), i64(a["nt"]), a["pt"], i64(a["ns"]), a["ps"],
                               i64(a["m"]), a["X"], i64(a["ldx"]), a["Y"], i64(a["ldy"]))
    cases = [dict(model=2), dict(model=-1), dict(L=0.0), dict(L=-0.1), dict(sig2=-1.0), dict(L=np.nan), dict(L=np.inf), dict(sig2=np.nan),
             dict(sig2=np.inf), dict(nt=0), dict(ns=0), dict(m=0), dict(nt=-1), dict(ldx=n - 1), dict(ldy=n - 1), dict(pt=None), dict(ps=None),
             dict(X=None), dict(ctx=None)]
    for kw in cases:
        assert call(**kw) == BAD, kw
        msg = Lb.mi_last_error().decode()
        assert msg.startswith("mi_cov_apply"), (kw, msg)
        assert np.all(Y == SENT), kw
    assert call(Y=None) == BAD and Lb.mi_last_error().decode().startswith("mi_cov_apply")
    pn = p.copy(); pn[3, 1] = np.nan
    assert call(pt=vp(pn.ctypes.data)) == BAD and "finite" in Lb.mi_last_error().decode() and np.all(Y == SENT)
    assert call() == 0 and np.all(Y != SENT)
    # mi_kl_cov_create
    mesh = fem.get_mesh(4)
    M = fem.get_mass_matrix(mesh.cells, mesh.points)
    pts = np.ascontiguousarray(mesh.points.T)
    ptr, idx, val = M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data.astype(np.float64)
    f64p, i64p = pkg._lib.f64p, pkg._lib.i64p
    gk = dict(ctx=ctx._h, model=0, sig2=1.0, L=0.1, n=16, pts=pts.ctypes.data_as(f64p), ptr=ptr.ctypes.data_as(i64p), idx=idx.ctypes.data_as(i64p),
              val=val.ctypes.data_as(f64p))

    def create(**kw):
        a = dict(gk, **kw)
        h = C.c_void_p(12345)
        rc = Lb.mi_kl_cov_create(a["ctx"], C.c_int(a["model"]), f64(a["sig2"]), f64(a["L"]), i64(a["n"]), a["pts"], a["ptr"], a["idx"], a["val"],
                                 C.byref(h))
        return rc, h
    vbad = val.copy(); vbad[3] = np.inf
    for kw in [dict(model=7), dict(L=0.0), dict(sig2=-2.0), dict(L=np.nan), dict(n=0), dict(n=15), dict(pts=None), dict(ptr=None),
               dict(idx=None), dict(val=None), dict(val=vbad.ctypes.data_as(f64p)), dict(ctx=None)]:
        rc, h = create(**kw)
        assert rc == BAD and not h.value, kw
        assert Lb.mi_last_error().decode().startswith("mi_kl_cov_create"), (kw, Lb.mi_last_error())
    rc, h = create()
    assert rc == 0 and h.value
    assert Lb.mi_op_destroy(h) == 0
