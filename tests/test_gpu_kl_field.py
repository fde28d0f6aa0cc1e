"""GPU suite (-m gpu): the realization sampler (csrc/kl_field.hpp) through the C ABI and api.KLField, against
tests/kl_field_ref.py (numpy restatement of the reference).

Dense form — G carries the bits of the host loop `g += (sqrt(Λ[α]) * ξ[α]) * Ψ[:, α]` (same operations in the same order, no
contraction), column by column and whatever the batch; A = exp(G) is within 4 * 2^-52 relative (the device's exp and the
host's are each within 1 ulp of the truth; doubled). Factored form and coordinates — derived rounding bounds
(kl_field_ref.dd_bound, coords_bound); a wrong owner list or a dropped tail misses them by many orders of magnitude.

Edges come from mi_kl_field_tiling: row_tile nodes per workgroup, mode_chunk modes per LDS chunk, real_block realizations per
pass, and the row splits of the coordinates launch. Kernel cases run with host pointers (staged, compact) and with device
pointers, where the kernels themselves see the padded leading dimensions."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sla

import kl_field_ref as ref

pytestmark = pytest.mark.gpu

EPS = ref.EPS
SENT = -7.25e300            # sentinel in the padding rows of Ψ, Ξ, G and A
vp, i64 = C.c_void_p, C.c_int64


def create_dense(pkg, ctx, Λ, Ψ, pad=0):
    """mi_kl_field_create on Ψ embedded in leading dimension n + pad (the padding holds SENT)"""
    Lb = pkg._lib.load()
    n, m = Ψ.shape
    Ψp = np.full((m, n + pad), SENT); Ψp[:, :n] = Ψ.T                     # row α of this C-ordered array = column α
    Λc = np.ascontiguousarray(Λ, dtype=np.float64)
    h = vp()
    rc = Lb.mi_kl_field_create(ctx._h, i64(n), i64(m), Λc.ctypes.data_as(pkg._lib.f64p), Ψp.ctypes.data_as(pkg._lib.f64p), i64(n + pad), C.byref(h))
    assert rc == 0, Lb.mi_last_error()
    assert np.all(Ψp[:, n:] == SENT)
    return h


def raw_set(pkg, ctx, h, n, Ξ, device, want_g=True, want_a=True, pads=(3, 5, 2)):
    """mi_kl_field_set with Ξ (m x nreal), G and A embedded in padded leading dimensions; -> (G, A) or None for an output that
    was not asked for. Asserts that every padding row still holds SENT and that Ξ is unchanged."""
    Lb = pkg._lib.load()
    m, nreal = Ξ.shape
    ldxi, ldg, lda = m + pads[0], n + pads[1], n + pads[2]
    Ξp = np.full((nreal, ldxi), SENT); Ξp[:, :m] = Ξ.T
    Gp, Ap = np.full((nreal, ldg), SENT), np.full((nreal, lda), SENT)
    if device:
        import torch
        tΞ, tG, tA = torch.from_numpy(Ξp).cuda(), torch.from_numpy(Gp).cuda(), torch.from_numpy(Ap).cuda()
        torch.cuda.synchronize()
        ptr = lambda t: vp(t.data_ptr())                                  # noqa: E731
    else:
        tΞ, tG, tA = Ξp, Gp, Ap
        ptr = lambda a: vp(a.ctypes.data)                                 # noqa: E731
    assert Lb.mi_ctx_set_pointer_mode(ctx._h, 1 if device else 0) == 0
    try:
        rc = Lb.mi_kl_field_set(h, i64(nreal), ptr(tΞ), i64(ldxi), ptr(tG) if want_g else None, i64(ldg), ptr(tA) if want_a else None, i64(lda))
        assert rc == 0, Lb.mi_last_error()
        ctx.synchronize()
    finally:
        Lb.mi_ctx_set_pointer_mode(ctx._h, 0)
    if device:
        Ξp, Gp, Ap = tΞ.cpu().numpy(), tG.cpu().numpy(), tA.cpu().numpy()
    assert np.array_equal(Ξp[:, :m], Ξ.T, equal_nan=True) and np.all(Ξp[:, m:] == SENT) and np.all(Gp[:, n:] == SENT) and np.all(Ap[:, n:] == SENT)
    if not want_g:
        assert np.all(Gp == SENT)
    if not want_a:
        assert np.all(Ap == SENT)
    return (Gp[:, :n].T.copy() if want_g else None), (Ap[:, :n].T.copy() if want_a else None)


def check_dense(pkg, ctx, n, m, nreal, seed, tag):
    rng = np.random.default_rng(seed)
    Λ, Ψ = ref.small_modes(rng, n, m)
    Ξ = rng.standard_normal((m, nreal))
    Gref = np.column_stack([ref.set_field(Λ, Ψ, Ξ[:, r]) for r in range(nreal)])
    Aref = np.exp(Gref)
    h = create_dense(pkg, ctx, Λ, Ψ, pad=7)
    try:
        got = []
        for device in (False, True):
            G, A = raw_set(pkg, ctx, h, n, Ξ, device)
            rel = float(np.max(np.abs(A - Aref) / Aref))
            print(f"  {tag} {'device' if device else 'host'} pointers: n {n} m {m} nreal {nreal}: G bit-equal {np.array_equal(G, Gref)}, "
                  f"max |A - A_ref| / A_ref = {rel:.2e} (bar {ref.EXP_RTOL:.2e})")
            assert np.array_equal(G, Gref), tag
            assert np.all(np.abs(A - Aref) <= ref.EXP_RTOL * Aref), (tag, rel)
            Gonly, none = raw_set(pkg, ctx, h, n, Ξ, device, want_a=False)
            none2, Aonly = raw_set(pkg, ctx, h, n, Ξ, device, want_g=False)
            assert none is None and none2 is None and np.array_equal(Gonly, G) and np.array_equal(Aonly, A)
            got.append((G, A))
        assert np.array_equal(got[0][1], got[1][1])                              # exp: the same bits in both modes
        # any column of the batch equals its single-column call
        r = nreal - 1
        G1, A1 = raw_set(pkg, ctx, h, n, Ξ[:, r:r + 1].copy(), True)
        assert np.array_equal(G1[:, 0], got[1][0][:, r]) and np.array_equal(A1[:, 0], got[1][1][:, r])
    finally:
        assert pkg._lib.load().mi_kl_field_destroy(h) == 0


def test_dense_row_edges(pkg, ctx):
    rt, mc, rb, _ = pkg.api.kl_field_tiling(1, 1)
    for k, n in enumerate((1, rt - 1, rt, rt + 1, 2 * rt + 1)):
        check_dense(pkg, ctx, n, 3, 2, 10 + k, "rows")


def test_dense_mode_edges(pkg, ctx):
    rt, mc, rb, _ = pkg.api.kl_field_tiling(1, 1)
    for k, m in enumerate((1, 2, mc - 1, mc, mc + 1)):
        check_dense(pkg, ctx, rt + 1, m, 1, 20 + k, "modes")


def test_dense_realization_edges(pkg, ctx):
    rt, mc, rb, _ = pkg.api.kl_field_tiling(1, 1)
    for k, nreal in enumerate((1, 2, rb - 1, rb, rb + 1, 2 * rb + 1)):
        check_dense(pkg, ctx, rt + 1, mc + 1, nreal, 30 + k, "realizations")


def test_dense_overflow_and_nan_follow_numpy(pkg, ctx):
    rt = pkg.api.kl_field_tiling(1, 1)[0]
    rng = np.random.default_rng(40)
    n, m = rt + 1, 4
    Λ, Ψ = ref.small_modes(rng, n, m)
    Ψ[:, 0] = np.abs(Ψ[:, 0]) + 0.5
    Ξ = rng.standard_normal((m, 3))
    Ξ[0, 0] = 5000.0 / np.sqrt(Λ[0])                                     # g > 709.78 on every node: exp overflows
    Ξ[2, 1] = np.nan
    with np.errstate(all="ignore"):
        Gref = np.column_stack([ref.set_field(Λ, Ψ, Ξ[:, r]) for r in range(3)])
        Aref = np.exp(Gref)
    assert Gref[:, 0].min() > 709.78 and np.all(np.isinf(Aref[:, 0])) and np.all(np.isnan(Gref[:, 1])) and np.all(np.isfinite(Aref[:, 2]))
    h = create_dense(pkg, ctx, Λ, Ψ)
    try:
        for device in (False, True):
            G, A = raw_set(pkg, ctx, h, n, Ξ, device)                    # rc == 0 inside: no error is returned
            assert np.array_equal(G, Gref, equal_nan=True)
            assert np.array_equal(np.isinf(A), np.isinf(Aref)) and np.array_equal(np.isnan(A), np.isnan(Aref)) and np.all(A[:, 0] > 0)
            assert np.all(np.abs(A[:, 2] - Aref[:, 2]) <= ref.EXP_RTOL * Aref[:, 2])
    finally:
        pkg._lib.load().mi_kl_field_destroy(h)


# ------------------------------------------------------------------ factored form
@pytest.mark.parametrize("index_base", [0, 1])
def test_factored_form_on_a_2x2_split(pkg, ctx, fem, index_base):
    import torch
    rt, mc, rb, _ = pkg.api.kl_field_tiling(1, 1)
    mesh, l2gd, elemsd, Φd, Φ, Λ, rng = ref.split_problem(fem, md=(1, 3, 7, 2))
    n = mesh.points.shape[1]
    cnt = np.bincount(np.concatenate(l2gd), minlength=n)
    assert set(cnt) == {1, 2, 4} and l2gd[0].size == rt + 1 and min(l.size for l in l2gd) < rt
    f = pkg.api.KLField.from_dd(ctx, n, Λ, Φ, Φd, l2gd, index_base=index_base)
    try:
        st = f.stats()
        assert st["bytes_kept"] >= 8 * (sum(P.size for P in Φd) + Φ.size) and st["bytes_kept"] < 8 * n * Λ.size + 8 * Φ.size + 64 * n
        for nreal in (1, 2, 3, rb + 1):                                   # 1, 2, 4 and real_block accumulators in use
            Ξ = rng.standard_normal((Λ.size, nreal))
            want = np.column_stack([ref.dd_field(n, Λ, Φ, Φd, l2gd, Ξ[:, r]) for r in range(nreal)])
            bound = np.column_stack([ref.dd_bound(n, Λ, Φ, Φd, l2gd, Ξ[:, r]) for r in range(nreal)])
            G, A = f.set_and_coefficient(Ξ)
            err = np.abs(G - want)
            print(f"  factored, base {index_base}, nreal {nreal}: max err {err.max():.2e}, err / bound {np.max(err / bound):.3f}")
            assert np.all(err <= bound)
            assert np.all(np.abs(A - np.exp(G)) <= ref.EXP_RTOL * np.exp(G))
            Gd, Ad = f.set_and_coefficient(torch.from_numpy(Ξ).cuda())
            assert np.array_equal(Gd.cpu().numpy(), G) and np.array_equal(Ad.cpu().numpy(), A)      # across pointer modes
            assert np.array_equal(f.set(Ξ), G) and np.array_equal(f.coefficient(Ξ), A)               # call to call, single outputs
            assert np.array_equal(f.set(Ξ[:, -1]), G[:, -1])                                          # a column alone
        Mop = pkg.api.SparseMatrixCSC(ctx, fem.get_mass_matrix(mesh.cells, mesh.points))
        with pytest.raises(pkg.api.MiError) as e:
            f.coords(Mop, np.zeros(n))                                                                # "not provided"
        Mop.close()
        assert e.value.code == pkg._lib.MI_ERR_BAD_ARG and "factored" in str(e.value)
    finally:
        f.close()


# ------------------------------------------------------------------ coordinates
def _m_orthonormal(rng, M, m):
    X = rng.standard_normal((M.shape[0], m))
    return X @ np.linalg.inv(sla.cholesky(X.T @ (M @ X)))                 # Ψ' M Ψ = I


def roundtrip_bound(ξ, Λ, Ψ, M):
    """|coords(M, set(ξ)) - ξ|: the sum of the two bounds — the coordinates bound on g, and the rounding of g itself
    ((m + 2) roundings per node, doubled) carried through Ψ' |M| / sqrt(Λ)"""
    c = np.sqrt(Λ) * ξ
    g = ref.set_field(Λ, Ψ, ξ)
    dg = 2 * (Λ.size + 2) * EPS * (np.abs(Ψ) @ np.abs(c))
    return ref.coords_bound(g, Λ, Ψ, M) + (np.abs(Ψ).T @ (abs(M) @ dg)) / np.sqrt(Λ)


def test_coordinates_at_split_edges_and_round_trip(pkg, ctx, fem):
    import torch
    api = pkg.api
    rt, mc, rb, _ = api.kl_field_tiling(1, 1)
    side = int(round(np.sqrt(rt)))
    assert side * side == rt
    mesh0, l2gd, elemsd, _, _, _, _ = ref.split_problem(fem)
    g2l = np.full(mesh0.points.shape[1], -1, dtype=np.int64); g2l[l2gd[0]] = np.arange(l2gd[0].size)
    masses = [fem.get_mass_matrix(*(lambda me: (me.cells, me.points))(fem.get_mesh(N))) for N in (side, side + 1, side + 7)]
    masses.insert(1, fem.do_local_mass_assembly(mesh0.cells, mesh0.points, g2l, elemsd[0]))          # rt + 1 nodes
    assert [M.shape[0] for M in masses[:2]] == [rt, rt + 1]
    # several row tiles per split (the strided row loop of a workgroup): many column blocks, eleven row tiles
    masses.append(fem.get_mass_matrix(*(lambda me: (me.cells, me.points))(fem.get_mesh(int(np.sqrt(11 * rt))))))
    seen, strided = set(), 0
    for k, M in enumerate(masses):
        n = M.shape[0]
        m = (1, rb + 1, rb, 3, 125 * rb)[k]
        seen.add(api.kl_field_tiling(n, m)[3])
        strided += api.kl_field_tiling(n, m)[3] < -(-n // rt)
        rng = np.random.default_rng(50 + k)
        Ψ = _m_orthonormal(rng, M, m)
        Λ = np.sort(rng.random(m) + 0.1)[::-1]
        ξ = rng.standard_normal(m)
        g = rng.standard_normal(n)
        f, Mop = api.KLField(ctx, Λ, Ψ), api.SparseMatrixCSC(ctx, M)
        try:
            restate = ref.kl_coordinates if n * m <= 10 ** 5 else ref.kl_coordinates_blas
            got, want, bound = f.coords(Mop, g), restate(g, Λ, Ψ, M), ref.coords_bound(g, Λ, Ψ, M)
            err = np.abs(got - want)
            print(f"  coordinates n {n} m {m} splits {api.kl_field_tiling(n, m)[3]}: max err {err.max():.2e}, err / bound {np.max(err / bound):.3f}")
            assert np.all(err <= bound)
            assert np.array_equal(f.coords(Mop, g), got)                                          # call to call
            assert np.array_equal(f.coords(Mop, torch.from_numpy(g).cuda()).cpu().numpy(), got)   # device pointers
            back = f.coords(Mop, f.set(ξ))
            rb_ = roundtrip_bound(ξ, Λ, Ψ, M)
            print(f"    round trip: max |ξ' - ξ| {np.abs(back - ξ).max():.2e}, worst / bound {np.max(np.abs(back - ξ) / rb_):.3f}")
            assert np.all(np.abs(back - ξ) <= rb_)
        finally:
            f.close(); Mop.close()
    assert {1, 2, 3} <= seen and strided == 1


# ------------------------------------------------------------------ arguments
def test_bad_arguments_leave_outputs_untouched(pkg, ctx, fem):
    Lb, lib = pkg._lib.load(), pkg._lib
    BAD, f64p, i64p = lib.MI_ERR_BAD_ARG, lib.f64p, lib.i64p
    assert Lb.mi_ctx_set_pointer_mode(ctx._h, 0) == 0
    rng = np.random.default_rng(60)
    mesh = fem.get_mesh(4)
    Mh = fem.get_mass_matrix(mesh.cells, mesh.points)
    n, m = 16, 3
    Λ = np.array([0.9, 0.5, 0.2]); Ψ = np.asfortranarray(rng.standard_normal((n, m)))
    dp = lambda a: a.ctypes.data_as(f64p)                                     # noqa: E731
    ip = lambda a: a.ctypes.data_as(i64p)                                     # noqa: E731

    def refused(rc, prefix):
        msg = Lb.mi_last_error().decode()
        assert rc == BAD and msg.startswith(prefix) and len(msg) > len(prefix) + 5, (rc, msg)

    # ---- mi_kl_field_create
    def create(**kw):
        a = dict(ctx=ctx._h, n=n, m=m, lam=dp(Λ), psi=dp(Ψ), ld=n)
        a.update(kw)
        h = vp(12345)
        rc = Lb.mi_kl_field_create(a["ctx"], i64(a["n"]), i64(a["m"]), a["lam"], a["psi"], i64(a["ld"]), C.byref(h))
        return rc, h
    neg, nan, inf = np.array([0.9, -0.5, 0.2]), np.array([0.9, np.nan, 0.2]), np.array([np.inf, 0.5, 0.2])
    grp = pkg.api.LoopbackGroup(2)
    grp.set_mode(1)
    rank0 = pkg.api.Context(0)
    rank0.loopback_init(grp, 0)
    for kw in [dict(n=0), dict(m=0), dict(n=-1), dict(n=2 ** 30 + 1), dict(ld=n - 1), dict(lam=None), dict(psi=None), dict(ctx=None),
               dict(lam=dp(neg)), dict(lam=dp(nan)), dict(lam=dp(inf)), dict(ctx=rank0._h)]:
        rc, h = create(**kw)
        refused(rc, "mi_kl_field_create")
        assert not h.value, kw
    assert Lb.mi_kl_field_create(ctx._h, i64(n), i64(m), dp(Λ), dp(Ψ), i64(n), None) == BAD
    # ---- mi_kl_field_create_dd
    maps = [np.arange(0, 10), np.arange(8, 16)]
    n_d, md = np.array([10, 8], dtype=np.int64), np.array([2, 1], dtype=np.int64)
    inds = np.concatenate(maps).astype(np.int64)
    Φd, Φ = rng.standard_normal(10 * 2 + 8 * 1), np.asfortranarray(rng.standard_normal((3, m)))

    def create_dd(**kw):
        a = dict(ctx=ctx._h, n=n, m=m, lam=dp(Λ), ndom=2, n_d=ip(n_d), md=ip(md), inds=ip(inds), base=0, phid=dp(Φd), phi=dp(Φ), ld=3)
        a.update(kw)
        h = vp(12345)
        rc = Lb.mi_kl_field_create_dd(a["ctx"], i64(a["n"]), i64(a["m"]), a["lam"], i64(a["ndom"]), a["n_d"], a["md"], a["inds"], C.c_int(a["base"]),
                                      a["phid"], a["phi"], i64(a["ld"]), C.byref(h))
        return rc, h
    md0 = np.array([2, 0], dtype=np.int64)
    out_of_range, repeated = inds.copy(), inds.copy()
    out_of_range[3] = 16; repeated[4] = 2
    orphan = np.concatenate([np.arange(0, 10), np.arange(7, 15)]).astype(np.int64)      # node 15 is owned by nobody
    for kw in [dict(n=0), dict(m=0), dict(ndom=0), dict(md=ip(md0)), dict(inds=ip(out_of_range)), dict(inds=ip(inds), base=1),
               dict(inds=ip(repeated)), dict(inds=ip(orphan)), dict(ld=2), dict(lam=dp(neg)), dict(lam=None), dict(n_d=None), dict(md=None),
               dict(inds=None), dict(phid=None), dict(phi=None), dict(ctx=None), dict(ctx=rank0._h), dict(base=2)]:
        rc, h = create_dd(**kw)
        refused(rc, "mi_kl_field_create_dd")
        assert not h.value, kw
    rank0.close()
    # ---- mi_kl_field_set / mi_kl_field_coords on good handles
    rc, h = create()
    assert rc == 0 and h.value
    rc, hdd = create_dd()
    assert rc == 0 and hdd.value
    rc, hzero = create(lam=dp(np.array([0.9, 0.0, 0.2])))                   # Λ_α = 0 is fine for a set ...
    assert rc == 0 and hzero.value
    Mop, M5 = pkg.api.SparseMatrixCSC(ctx, Mh), pkg.api.SparseMatrixCSC(ctx, fem.get_mass_matrix(*(lambda me: (me.cells, me.points))(fem.get_mesh(5))))
    diag = pkg.api.JacobiPreconditioner(ctx, np.ones(n))
    try:
        Ξ = np.ones((2, m)); G = np.full((2, n), SENT); A = np.full((2, n), SENT)

        def call_set(**kw):
            a = dict(h=h, nreal=2, xi=vp(Ξ.ctypes.data), ldxi=m, g=vp(G.ctypes.data), ldg=n, a=vp(A.ctypes.data), lda=n)
            a.update(kw)
            return Lb.mi_kl_field_set(a["h"], i64(a["nreal"]), a["xi"], i64(a["ldxi"]), a["g"], i64(a["ldg"]), a["a"], i64(a["lda"]))
        for kw in [dict(nreal=0), dict(nreal=-2), dict(nreal=2 ** 30 + 1), dict(ldxi=m - 1), dict(ldg=n - 1), dict(lda=n - 1), dict(xi=None),
                   dict(h=None), dict(g=None, a=None)]:
            refused(call_set(**kw), "mi_kl_field_set")
            assert np.all(G == SENT) and np.all(A == SENT), kw
        assert call_set(g=None, ldg=0) == 0 and np.all(G == SENT) and np.all(A != SENT)     # the leading dimension of a NULL output is not looked at
        assert call_set(h=hzero) == 0 and np.all(np.isfinite(G))
        g = np.ones(n); ξ = np.full(m, SENT)

        def call_coords(**kw):
            a = dict(h=h, M=Mop._h, g=vp(g.ctypes.data), xi=vp(ξ.ctypes.data))
            a.update(kw)
            return Lb.mi_kl_field_coords(a["h"], a["M"], a["g"], a["xi"])
        for kw in [dict(h=None), dict(M=None), dict(g=None), dict(xi=None), dict(M=M5._h), dict(M=diag._h), dict(h=hdd), dict(h=hzero)]:
            refused(call_coords(**kw), "mi_kl_field_coords")                # ... hzero: and refused by the coordinates only
            assert np.all(ξ == SENT), kw
        assert call_coords() == 0 and np.all(ξ != SENT)
        many = 65535 * 8 + 1                                                 # one grid row per block of 8 modes: refused, not launched
        rc, hmany = create(n=1, m=many, lam=dp(np.ones(many)), psi=dp(np.ones(many)), ld=1)
        assert rc == 0 and hmany.value
        ξm = np.full(many, SENT)
        refused(call_coords(h=hmany, xi=vp(ξm.ctypes.data)), "mi_kl_field_coords")
        assert np.all(ξm == SENT) and Lb.mi_kl_field_destroy(hmany) == 0
        a, b = i64(), i64()
        assert Lb.mi_kl_field_stats(h, C.byref(a), C.byref(b)) == 0 and a.value == 8 * (n * m + m) and b.value > a.value
    finally:
        for x in (h, hdd, hzero):
            assert Lb.mi_kl_field_destroy(x) == 0
        Mop.close(); M5.close(); diag.close()


# ------------------------------------------------------------------ stream order
def test_set_in_front_of_assembly_without_a_synchronise(pkg, ctx, fem):
    """device pointers: mi_kl_field_set, then mi_assembly_run on its A, both enqueued on the context's stream with nothing
    between them; the assembled values have the bits of assembling the same A read back and uploaded again"""
    import torch
    Lb = pkg._lib.load()
    N = 24
    mesh = fem.get_mesh(N)
    dinds = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
    epart, npart = fem.mesh_partition(mesh, 2, 2)
    sub = fem.set_subdomains(mesh.cells, mesh.cell_neighbors, epart, npart, dinds.dirichlet_g2l)
    plan = fem.make_assembly_plan(mesh.cells, mesh.points, epart, sub, lambda x, y: -1.0 + 0 * x, lambda x, y: 0.734 + 0 * x)
    kl = fem.synthetic_kl(mesh.points)
    ξ, g_host = fem.draw(kl, np.random.default_rng(481456))
    n = N * N
    dev = pkg.api.AssemblyPlan(ctx, plan)
    f = pkg.api.KLField(ctx, kl.Λ, kl.Ψ)
    try:
        tξ = torch.from_numpy(ξ).cuda()
        tA = torch.empty(n, dtype=torch.float64, device="cuda")
        tV = torch.empty(plan.n_entries, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert Lb.mi_ctx_set_pointer_mode(ctx._h, 1) == 0
        try:
            assert Lb.mi_kl_field_set(f._h, i64(1), vp(tξ.data_ptr()), i64(kl.Λ.size), None, i64(n), vp(tA.data_ptr()), i64(n)) == 0
            assert Lb.mi_assembly_run(dev._h, vp(tA.data_ptr()), vp(tV.data_ptr())) == 0
            ctx.synchronize()
        finally:
            Lb.mi_ctx_set_pointer_mode(ctx._h, 0)
        A = tA.cpu().numpy()
        assert np.all(np.abs(A - np.exp(g_host)) <= ref.EXP_RTOL * np.exp(g_host))
        assert np.array_equal(tV.cpu().numpy(), dev.run(A))
        # the same through api.KLField with a torch tensor, one output each (what example07 --device-field does)
        a_t, g_t = f.coefficient(tξ), f.set(tξ)
        assert a_t.is_cuda and g_t.is_cuda and a_t.shape == (n,) and g_t.shape == (n,)
        assert np.array_equal(a_t.cpu().numpy(), A) and np.array_equal(g_t.cpu().numpy(), g_host)
        assert np.array_equal(dev.run(a_t).cpu().numpy(), tV.cpu().numpy())
    finally:
        f.close(); dev.close()


# ------------------------------------------------------------------ samplers
def test_mcmc_sampler_with_a_device_field_equals_the_host_one(pkg, ctx):
    rng = np.random.default_rng(70)
    Λ, Ψ = ref.small_modes(rng, 300, 3)
    f = pkg.api.KLField(ctx, Λ, Ψ)
    try:
        host = pkg.api.McmcSampler(Λ, Ψ, ref.ScriptedRng(ref.mcmc_script()))
        devs = pkg.api.McmcSampler(Λ, None, ref.ScriptedRng(ref.mcmc_script()), field=f)
        assert np.array_equal(host.ξ, devs.ξ) and np.array_equal(host.g, devs.g)
        for want in (1, 3, 1):
            assert host.draw() == want and devs.draw() == want
            assert np.array_equal(host.ξ, devs.ξ) and np.array_equal(host.g, devs.g)
            assert np.all(np.abs(devs.a - host.a) <= ref.EXP_RTOL * host.a)
    finally:
        f.close()
