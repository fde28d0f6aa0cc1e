"""GPU suite (-m gpu): the quantizer kernels (csrc/vq.hpp) through the C ABI and the api, against tests/vq_ref.py (the loop
form of the reference) with np.array_equal throughout, and the combined operator of mi_op_combine against the host
expression on its children's own device applies.

The sizes come from mi_vq_tiling — point_tile samples per workgroup, cent_tile centroids staged at a time, k_chunk
coordinates per LDS chunk, the centroid splits of a launch that the samples alone do not fill, sum_chunk samples per chunk of
the ordered sums — so they move with the kernel. Raw calls embed X and C in padded leading dimensions whose padding rows
hold a sentinel, and run with host pointers (staged, compact) and with device pointers, where the kernels see the padding."""
import ctypes as C

import numpy as np
import pytest

import amg_ref as ar
import amg_synth as asy
import vq_ref as ref

pytestmark = pytest.mark.gpu

SENT = -7.25e300
vp, i64 = C.c_void_p, C.c_int64
_T = {}


def tiling(pkg, d=3, ns=1000, P=10):
    key = (d, ns, P)
    if key not in _T:
        _T[key] = pkg.api.vq_tiling(d, ns, P)
    return _T[key]


def padded(M, pad):
    """(buffer, view): M (d x n) embedded column by column in leading dimension d + pad; the padding rows hold SENT"""
    d, n = M.shape
    buf = np.full((n, d + pad), SENT)
    buf[:, :d] = M.T
    return buf


def raw_assign(pkg, ctx, X, Cn, device, pads=(3, 5), want=(True, True, True)):
    """mi_vq_assign with X and C in padded leading dimensions -> (assign, dist2, objv), None where not asked for. Asserts
    that the padding and the inputs are unchanged."""
    Lb = pkg._lib.load()
    d, ns = X.shape
    P = Cn.shape[1]
    Xp, Cp = padded(X, pads[0]), padded(Cn, pads[1])
    a, c = np.full(ns, -5, dtype=np.int64), np.full(ns, SENT)
    if device:
        import torch
        tX, tC, ta, tc = (torch.from_numpy(v).cuda() for v in (Xp, Cp, a, c))
        torch.cuda.synchronize()
        ptr = lambda t: vp(t.data_ptr())                                  # noqa: E731
    else:
        tX, tC, ta, tc = Xp, Cp, a, c
        ptr = lambda v: vp(v.ctypes.data)                                 # noqa: E731
    assert Lb.mi_ctx_set_pointer_mode(ctx._h, 1 if device else 0) == 0
    objv = C.c_double(-1.0)
    try:
        rc = Lb.mi_vq_assign(ctx._h, i64(d), i64(ns), ptr(tX), i64(d + pads[0]), i64(P), ptr(tC), i64(d + pads[1]),
                             ptr(ta) if want[0] else None, ptr(tc) if want[1] else None, C.byref(objv) if want[2] else None)
        assert rc == 0, Lb.mi_last_error()
    finally:
        Lb.mi_ctx_set_pointer_mode(ctx._h, 0)
    if device:
        Xb, Cb, a, c = (t.cpu().numpy() for t in (tX, tC, ta, tc))
    else:
        Xb, Cb = tX, tC
    assert np.array_equal(Xb, padded(X, pads[0]), equal_nan=True) and np.array_equal(Cb, padded(Cn, pads[1]), equal_nan=True)
    if not want[0]:
        assert np.all(a == -5)
    if not want[1]:
        assert np.all(c == SENT)
    return (a if want[0] else None), (c if want[1] else None), (objv.value if want[2] else None)


def host_pointers(pkg, ctx):
    """a raw call on numpy arrays follows: the api leaves the context in the mode of its last call, which may be the device's"""
    assert pkg._lib.load().mi_ctx_set_pointer_mode(ctx._h, 0) == 0


def data(seed, d, ns, P):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((d, ns)), rng.standard_normal((d, P))


def check_assign(pkg, ctx, X, Cn, device=False, tag=""):
    sum_chunk = tiling(pkg)[4]
    a, c, objv = raw_assign(pkg, ctx, X, Cn, device)
    ar_, cr = ref.assign(X, Cn)
    print(f"{tag} d x ns x P = {X.shape[0]} x {X.shape[1]} x {Cn.shape[1]}: differing assignments {int(np.sum(a != ar_))}, "
          f"differing dist2 {int(np.sum(c != cr))}, objv {objv!r} vs {ref.objective(cr, sum_chunk)!r}")
    assert np.array_equal(a, ar_) and np.array_equal(c, cr)
    assert objv == ref.objective(cr, sum_chunk)
    return a, c


# ------------------------------------------------------------------ assign
def _edge_shapes(pkg):
    pt, ct, kc = tiling(pkg)[:3]
    base = (pt + 1, ct + 1, kc + 1)
    shapes = [base]
    shapes += [(ns, base[1], base[2]) for ns in (1, pt - 1, pt, 2 * pt + 1)]
    shapes += [(base[0], P, base[2]) for P in (1, ct - 1, ct, 2 * ct + 1)]
    shapes += [(base[0], base[1], d) for d in (1, kc - 1, kc, 2 * kc + 3)]
    return shapes


@pytest.mark.parametrize("idx", range(13))
def test_assign_at_tile_edges(pkg, ctx, idx):
    """(ns, P, d) = (point_tile + 1, cent_tile + 1, k_chunk + 1) and one size at a time at 1, tile - 1, tile, 2 tile + 1 (+3)"""
    ns, P, d = _edge_shapes(pkg)[idx]
    X, Cn = data(100 + idx, d, ns, P)
    check_assign(pkg, ctx, X, Cn, device=bool(idx % 2), tag=f"edge {idx}")


def _first_split_P(pkg, d):
    for P in range(1, 4097):
        if tiling(pkg, d, 1, P)[3] >= 2:
            return P
    raise AssertionError("no P up to 4096 splits the centroids of a single sample")


@pytest.mark.parametrize("device", [False, True])
def test_assign_one_sample_with_split_centroids(pkg, ctx, device):
    d = tiling(pkg)[2] + 1
    P = _first_split_P(pkg, d)
    assert tiling(pkg, d, 1, P)[3] >= 2 and tiling(pkg, d, 1, P - 1)[3] == 1
    X, Cn = data(7, d, 1, P)
    check_assign(pkg, ctx, X, Cn, device, tag=f"ns = 1, P = {P}, splits = {tiling(pkg, d, 1, P)[3]}")
    # many splits: every split boundary of a larger launch
    P2 = 40 * tiling(pkg)[1] + 3
    assert tiling(pkg, d, 1, P2)[3] >= 8
    X, Cn = data(8, d, 1, P2)
    check_assign(pkg, ctx, X, Cn, device, tag=f"ns = 1, P = {P2}, splits = {tiling(pkg, d, 1, P2)[3]}")


def test_assign_ties_go_to_the_lower_index(pkg, ctx):
    """a duplicated centroid on both sides of a cent_tile boundary, of a wave's share of it, and of a split boundary; a sample
    equal to a centroid has dist2 == 0.0"""
    pt, ct, kc = tiling(pkg)[:3]
    d = kc + 1
    for ns in (1, pt + 1):
        P = 6 * ct
        splits = tiling(pkg, d, ns, P)[3]
        X, Cn = data(20 + ns, d, ns, P)
        Cn *= 10.0                                       # far away, so that the duplicates below are the winners
        per = -(-(P // ct) // splits) * ct               # centroids per split
        if ns == 1:
            assert splits >= 2
        lo_hi = [(ct - 1, ct), (3, 2 * ct + 5), (per - 1, per), (0, P - 1), (ct // 4 - 1, ct // 4)]
        for lo, hi in lo_hi:
            Cd = Cn.copy()
            Cd[:, lo] = X[:, 0] + 0.25
            Cd[:, hi] = Cd[:, lo]
            a, c = check_assign(pkg, ctx, X, Cd, device=True, tag=f"tie {lo} / {hi}")
            assert a[0] == lo
        Cd = Cn.copy()
        Cd[:, P - 2] = X[:, ns - 1]
        a, c = check_assign(pkg, ctx, X, Cd, tag="sample on a centroid")
        assert a[ns - 1] == P - 2 and c[ns - 1] == 0.0


def test_assign_nan_distances_follow_the_reference_scan(pkg, ctx):
    """a NaN distance to centroid 0 stays (the scan starts there), a NaN distance to another centroid never wins"""
    pt, ct, kc = tiling(pkg)[:3]
    X, Cn = data(30, 3, 5, 2 * ct + 1)
    for col in (0, 1, ct, 2 * ct):
        Cd = Cn.copy()
        Cd[1, col] = np.nan
        a, c, _ = raw_assign(pkg, ctx, X, Cd, device=True, want=(True, True, False))
        ar_, cr = ref.assign(X, Cd)
        assert np.array_equal(a, ar_) and np.array_equal(c, cr, equal_nan=True)
        assert np.all(np.isnan(c)) == (col == 0)


@pytest.mark.parametrize("device", [False, True])
def test_assign_optional_outputs(pkg, ctx, device):
    X, Cn = data(40, 5, 70, 9)
    full = raw_assign(pkg, ctx, X, Cn, device)
    for want in [(False, True, True), (True, False, True), (True, True, False), (False, False, True), (True, False, False)]:
        got = raw_assign(pkg, ctx, X, Cn, device, want=want)
        for g, f, w in zip(got, full, want):
            assert (g is None) if not w else np.array_equal(g, f)


def test_api_assign_find_precond_and_distortion(pkg, ctx):
    import torch
    api = pkg.api
    sum_chunk = tiling(pkg)[4]
    X, Cn = data(50, 6, 300, 40)
    ar_, cr = ref.assign(X, Cn)
    a, c, objv = api.vq_assign(ctx, X, Cn)
    assert np.array_equal(a, ar_) and np.array_equal(c, cr) and objv == ref.objective(cr, sum_chunk)
    ta, tc, tobjv = api.vq_assign(ctx, torch.from_numpy(X).cuda(), torch.from_numpy(Cn).cuda())
    assert np.array_equal(ta.cpu().numpy(), ar_) and np.array_equal(tc.cpu().numpy(), cr) and tobjv == objv
    assert api.get_distortion(ctx, X, Cn) == ref.objective(cr, sum_chunk) / 300
    rng = np.random.default_rng(51)
    for P in (5, 40 * tiling(pkg)[1] + 3):                # nKL_trunc < nKL; the second one splits the centroids
        x, hXt = rng.standard_normal(19), rng.standard_normal((7, P))
        assert api.find_precond(ctx, x, hXt) == ref.find_precond(x, hXt)
    hXt[:, 3] = x[:7]
    x[7:] = 0.0
    assert api.find_precond(ctx, x, hXt) == 3


def test_assign_refusals(pkg, ctx):
    Lb = pkg._lib.load()
    host_pointers(pkg, ctx)
    BAD = pkg._lib.MI_ERR_BAD_ARG
    X, Cn = np.zeros((5, 4)), np.zeros((3, 4))           # 4 x 5 and 4 x 3, column-major
    p = lambda v: vp(v.ctypes.data)                      # noqa: E731
    call = lambda d, ns, ldx, P, ldc: Lb.mi_vq_assign(ctx._h, i64(d), i64(ns), p(X), i64(ldx), i64(P), p(Cn), i64(ldc), None, None, None)  # noqa: E731
    assert call(4, 5, 4, 3, 4) == 0
    for args in [(0, 5, 4, 3, 4), (4, 0, 4, 3, 4), (4, 5, 4, 0, 4), (4, 5, 3, 3, 4), (4, 5, 4, 3, 3), (4, 2 ** 31, 4, 3, 4), (4, 5, 4, 2 ** 31, 4)]:
        assert call(*args) == BAD, args
    assert Lb.mi_vq_assign(ctx._h, i64(4), i64(5), None, i64(4), i64(3), p(Cn), i64(4), None, None, None) == BAD
    assert call(4, 2, 4, 3, 4) == 0                      # P > ns is allowed here ...
    cnt = np.zeros(3, dtype=np.int64)
    assert Lb.mi_vq_kmeans(ctx._h, i64(4), i64(2), p(X), i64(4), i64(3), p(Cn), i64(4), C.c_double(1e-8), i64(10), None, p(cnt), None, None,
                           None, None) == BAD            # ... and not here
    u, pk = np.zeros(3), np.zeros(3, dtype=np.int64)
    assert Lb.mi_vq_seed(ctx._h, i64(4), i64(2), p(X), i64(4), i64(3), p(u), p(pk), p(Cn), i64(4)) == BAD


# ------------------------------------------------------------------ update
@pytest.mark.parametrize("device", [False, True])
def test_update_cluster_sizes_0_1_2_and_all(pkg, ctx, device):
    api = pkg.api
    pt = tiling(pkg)[0]
    d, ns, P = 19, 2 * pt + 45, 5
    X, Cn = data(60, d, ns, P)
    cases = []
    a = np.full(ns, 3, dtype=np.int64)                   # sizes 0 (cluster 4), 1, 2 and the rest
    a[17], a[5], a[ns - 1] = 0, 1, 1
    a[[2, 40]] = 2
    a[a == 2] = 2
    cases.append(a)
    cases.append(np.full(ns, 2, dtype=np.int64))         # one cluster holds every sample
    cases.append(np.random.default_rng(61).integers(0, P, ns))
    for a in cases:
        want_C, want_n = ref.update(X, a, Cn)
        if device:
            import torch
            tC = torch.from_numpy(np.ascontiguousarray(Cn.T)).cuda().t()
            gC, gn = api.vq_update(ctx, torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t(), torch.from_numpy(a).cuda(), tC)
            gC, gn = gC.cpu().numpy(), gn.cpu().numpy()
        else:
            gC, gn = api.vq_update(ctx, X, a, np.array(Cn, order="F"))
        assert np.array_equal(gn, want_n) and np.array_equal(gC, want_C)
        for p in np.nonzero(want_n == 0)[0]:
            assert np.array_equal(gC[:, p], Cn[:, p])    # the empty cluster's centre is unchanged to the bit
    assert 0 in ref.update(X, cases[0], Cn)[1] and ns in ref.update(X, cases[1], Cn)[1]


def test_update_padded_and_many_clusters(pkg, ctx):
    """more clusters than one workgroup owns, more coordinates than one workgroup has threads, padded leading dimensions"""
    Lb = pkg._lib.load()
    host_pointers(pkg, ctx)
    d, ns, P = 300, 700, 530
    X, Cn = data(62, d, ns, P)
    a = np.random.default_rng(63).integers(0, P, ns)
    a[a == 257] = 0
    Xp, Cp, cnt = padded(X, 2), padded(Cn, 7), np.full(P, -1, dtype=np.int64)
    p = lambda v: vp(v.ctypes.data)                      # noqa: E731
    assert Lb.mi_vq_update(ctx._h, i64(d), i64(ns), p(Xp), i64(d + 2), i64(P), p(a), p(Cp), i64(d + 7), p(cnt)) == 0, Lb.mi_last_error()
    want_C, want_n = ref.update(X, a, Cn)
    assert np.array_equal(cnt, want_n) and np.array_equal(Cp[:, :d].T, want_C) and np.all(Cp[:, d:] == SENT)
    assert np.array_equal(Xp, padded(X, 2))
    bad = a.copy()
    bad[11] = P
    before = Cp.copy()
    assert Lb.mi_vq_update(ctx._h, i64(d), i64(ns), p(Xp), i64(d + 2), i64(P), p(bad), p(Cp), i64(d + 7), p(cnt)) == pkg._lib.MI_ERR_BAD_ARG
    assert np.array_equal(Cp, before) and np.array_equal(cnt, want_n)


# ------------------------------------------------------------------ objective and seed
def test_objective_at_sum_chunk_edges(pkg, ctx):
    sc = tiling(pkg)[4]
    for ns in (sc - 1, sc, sc + 1, 3 * sc + 2):
        X, Cn = data(70 + ns % 7, 2, ns, 3)
        _, c, objv = raw_assign(pkg, ctx, X, Cn, device=False)
        assert np.array_equal(c, ref.assign(X, Cn)[1])
        assert objv == ref.objective(c, sc), ns
        assert raw_assign(pkg, ctx, X, Cn, device=True, want=(False, False, True))[2] == objv


@pytest.mark.parametrize("device", [False, True])
def test_seed_picks_the_reference_samples(pkg, ctx, device):
    api = pkg.api
    sc = tiling(pkg)[4]
    d, ns, P = 3, 3 * sc + 2, 9
    X = np.random.default_rng(80).standard_normal((d, ns))
    u = np.random.default_rng(81).random(P)
    u[1], u[2], u[3] = 0.0, np.nextafter(1.0, 0.0), 0.0
    for u0 in (u[0], 0.0, np.nextafter(1.0, 0.0)):
        u[0] = u0
        want_p, want_C = ref.seed(X, P, u, sc)
        if device:
            import torch
            pk, Cn = api.kmpp_seed(ctx, torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t(), P, torch.from_numpy(u).cuda())
            pk, Cn = pk.cpu().numpy(), Cn.cpu().numpy()
        else:
            pk, Cn = api.kmpp_seed(ctx, X, P, u)
        print(f"u0 = {u0!r}: picked {pk.tolist()}, reference {want_p.tolist()}")
        assert np.array_equal(pk, want_p) and np.array_equal(Cn, want_C)
        assert len(set(pk.tolist())) == P


def test_seed_of_identical_points_is_refused(pkg, ctx):
    api = pkg.api
    X = np.ones((3, 40))
    Cn = np.full((3, 2), SENT, order="F")
    Lb = pkg._lib.load()
    host_pointers(pkg, ctx)
    u, pk = np.array([0.3, 0.6]), np.full(2, -9, dtype=np.int64)
    p = lambda v: vp(v.ctypes.data)                      # noqa: E731
    Xf = np.asfortranarray(X)
    rc = Lb.mi_vq_seed(ctx._h, i64(3), i64(40), p(Xf), i64(3), i64(2), p(u), p(pk), p(Cn), i64(3))
    assert rc == pkg._lib.MI_ERR_BAD_ARG and np.all(Cn == SENT) and np.all(pk == -9)
    with pytest.raises(pkg._lib.MiError):
        api.kmpp_seed(ctx, X, 2, u)
    pk1, C1 = api.kmpp_seed(ctx, X, 1, u)               # one centre needs no distance
    assert pk1[0] == 12 and np.array_equal(C1, X[:, :1])


# ------------------------------------------------------------------ kmeans
KM_SHAPES = [(2, 257, 5), (7, 300, 65), (3, 1000, 17)]
_km = {}


def km_ref(pkg, shape, **kw):
    key = (shape, tuple(sorted(kw.items())))
    if key not in _km:
        d, ns, P = shape
        X = np.random.default_rng(sum(shape)).standard_normal((d, ns))
        _km[key] = (X, ref.kmeans(X, X[:, :P].copy(), tiling(pkg)[4], **kw))
    return _km[key]


def _same(res, want):
    assert (res.iterations, res.converged, res.totalcost) == (want["iterations"], want["converged"], want["totalcost"])
    for f in ("assignments", "counts", "centers", "costs"):
        got = getattr(res, f)
        got = got.cpu().numpy() if hasattr(got, "cpu") else got
        assert np.array_equal(got, want[f]), f


@pytest.mark.parametrize("shape", KM_SHAPES)
def test_kmeans_equals_the_loop_form(pkg, ctx, shape):
    api = pkg.api
    X, want = km_ref(pkg, shape)
    P = shape[2]
    print(f"{shape}: {want['iterations']} iterations, changes of the objective {want['changes']}")
    assert want["converged"] and 1 < want["iterations"] < 1000
    res = api.kmeans(ctx, X, P, init=X[:, :P])
    _same(res, want)
    _same(api.kmeans(ctx, X, P, init=np.arange(P)), want)          # sample indices; a second run: equal bits
    import torch
    _same(api.kmeans(ctx, torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t(), P, init=np.arange(P)), want)


def test_kmeans_stops_at_maxiter(pkg, ctx):
    shape = max(KM_SHAPES, key=lambda s: km_ref(pkg, s)[1]["iterations"])
    X, want = km_ref(pkg, shape, maxiter=2)
    assert want["iterations"] == 2 and not want["converged"]
    res = pkg.api.kmeans(ctx, X, shape[2], init=X[:, :shape[2]], maxiter=2)
    assert res.iterations == 2 and res.converged is False
    _same(res, want)


def test_kmeans_with_two_identical_initial_centres(pkg, ctx):
    """centres 1 and 4 both start on sample 1, an outlier that is a cluster of its own: the tie gives it to centre 1, whose mean
    is the sample again, so centre 4 stays a duplicate, stays empty and keeps its bits through every iteration. (A duplicated
    centre whose twin moves away would be left behind as a centre of its own and collect members from the next assignment on.)"""
    X = np.random.default_rng(90).standard_normal((3, 200))
    X[:, 1] = [40.0, -35.0, 50.0]
    C0 = X[:, :6].copy()
    C0[:, 4] = C0[:, 1]
    want = ref.kmeans(X, C0, tiling(pkg)[4])
    res = pkg.api.kmeans(ctx, X, 6, init=C0)
    _same(res, want)
    assert want["iterations"] > 1 and res.counts[1] == 1
    assert res.counts[4] == 0 and np.array_equal(res.centers[:, 4], C0[:, 4]) and not np.any(res.assignments == 4)


def test_kmeans_refuses_a_nan_and_leaves_the_centres(pkg, ctx):
    Lb = pkg._lib.load()
    host_pointers(pkg, ctx)
    X = np.asfortranarray(np.random.default_rng(91).standard_normal((3, 100)))
    X[1, 57] = np.nan
    Cn = np.array(X[:, :4], order="F")
    before = Cn.copy()
    p = lambda v: vp(v.ctypes.data)                      # noqa: E731
    it, conv, objv = i64(-1), C.c_int(-1), C.c_double(-1.0)
    rc = Lb.mi_vq_kmeans(ctx._h, i64(3), i64(100), p(X), i64(3), i64(4), p(Cn), i64(3), C.c_double(1e-8), i64(100), None, None, None,
                         C.byref(objv), C.byref(it), C.byref(conv))
    assert rc == pkg._lib.MI_ERR_BAD_ARG and np.array_equal(Cn, before)
    import torch
    tX, tC = torch.from_numpy(np.ascontiguousarray(X.T)).cuda(), torch.from_numpy(np.ascontiguousarray(before.T)).cuda()
    with pytest.raises(pkg._lib.MiError):
        pkg.api.kmeans(ctx, tX.t(), 4, init=tC.t())
    assert np.array_equal(tC.cpu().numpy().T, before)


def test_kmeans_from_kmpp_and_get_quantizer(pkg, ctx, fem):
    """the whole flow: k-means++ on uniforms of a seeded generator, then Lloyd; the host mirror gives the same bits"""
    api = pkg.api
    sc = tiling(pkg)[4]
    X = np.random.default_rng(92).standard_normal((4, 400))
    res = api.kmeans(ctx, X, 7, init="kmpp", rng=np.random.default_rng(93))
    u = np.random.default_rng(93).random(7)
    want = ref.kmeans(X, ref.seed(X, 7, u, sc)[1], sc)
    _same(res, want)
    host = fem.kmeans(X, fem.kmpp_seed(X, 7, u)[1])
    assert np.array_equal(host.centers, res.centers) and host.iterations == res.iterations
    Λ = np.array([0.5, 0.3, 0.15, 0.05])
    Xq, cen, a, c = api.get_quantizer(ctx, 300, 5, Λ, "L2-full", rng=np.random.default_rng(94))
    assert Xq.shape == (4, 300) and cen.shape == (4, 5) and a.shape == c.shape == (300,)
    a2, c2, _ = api.vq_assign(ctx, fem.scale_data(Xq, Λ, "L2"), fem.scale_data(cen, Λ, "L2"))
    assert np.mean(a2 == a) > 0.99                       # the centres went through ./ sqrt(Λ) and back: ties aside, the same cells


# ------------------------------------------------------------------ combine
@pytest.fixture(scope="module")
def kids(pkg, ctx, fem):
    api = pkg.api
    Hs = [asy.hierarchy(fem, "arrow_%d" % asy.ARROW_M[0]), asy.hierarchy(fem, "longP")]
    n = Hs[0].A[0].shape[0]
    assert Hs[1].A[0].shape[0] == n
    diag = np.random.default_rng(95).uniform(0.5, 2.0, n)
    return n, [api.AMGPreconditioner(ctx, Hs[0]), api.AMGPreconditioner(ctx, Hs[1]), api.JacobiPreconditioner(ctx, diag)]


def _host_expression(coef, ts):
    z = np.zeros_like(ts[0])
    for c, t in zip(coef, ts):
        z = z + c * t
    return z


@pytest.mark.parametrize("k", [1, 2, 3])
def test_combined_apply_is_the_host_expression_on_the_childrens_applies(pkg, ctx, kids, k):
    import torch
    api = pkg.api
    n, ops = kids
    rng = np.random.default_rng(96 + k)
    coef = rng.standard_normal(k)
    r = rng.standard_normal(n)
    ts = [op * r for op in ops[:k]]
    Π = api.InterpolatingPreconditioner(ctx, coef, ops[:k])
    assert Π.n == n
    z = Π * r
    assert np.array_equal(z, _host_expression(coef, ts))
    zt = Π * torch.from_numpy(r).cuda()
    assert np.array_equal(zt.cpu().numpy(), z)
    coef2 = rng.standard_normal(k)
    Π.set_coefficients(coef2)
    assert np.array_equal(Π * r, _host_expression(coef2, ts))
    Π.close()
    for op, t in zip(ops[:k], ts):                      # destroying the combination leaves the children usable
        assert np.array_equal(op * r, t)


def test_combination_of_one_solves_like_its_child(pkg, ctx, fem):
    api = pkg.api
    A, b, H, _ = ar.case(fem, 40, "example01")
    Ag, M = api.SparseMatrixCSC(ctx, A), api.AMGPreconditioner(ctx, H)
    x0 = np.zeros(b.size)
    x, it, res = api.pcg(Ag, b, x0.copy(), M)
    Π = api.InterpolatingPreconditioner(ctx, [1.0], [M])
    xc, itc, resc = api.pcg(Ag, b, x0.copy(), Π)
    assert itc == it and np.array_equal(resc, res) and np.array_equal(xc, x)


def test_set_coefficients_between_two_solves(pkg, ctx, fem):
    api = pkg.api
    A, b, H, _ = ar.case(fem, 40, "example01")
    A2, _, H2, _ = ar.case(fem, 40, "lognormal")
    Ag = api.SparseMatrixCSC(ctx, A)
    ops = [api.AMGPreconditioner(ctx, H), api.AMGPreconditioner(ctx, H2), api.JacobiPreconditioner(ctx, A.diagonal())]
    c1, c2 = [0.6, 0.3, 0.1], [0.1, 0.2, 0.7]
    Π = api.InterpolatingPreconditioner(ctx, c1, ops)
    x0 = np.zeros(b.size)
    first = api.pcg(Ag, b, x0.copy(), Π)
    Π.set_coefficients(c2)
    second = api.pcg(Ag, b, x0.copy(), Π)
    Π.set_coefficients(c1)
    again = api.pcg(Ag, b, x0.copy(), Π)
    assert first[1] == again[1] and np.array_equal(first[2], again[2]) and np.array_equal(first[0], again[0])
    assert not np.array_equal(second[2][:min(len(second[2]), len(first[2]))], first[2][:min(len(second[2]), len(first[2]))])
    for out in (first, second):
        assert np.linalg.norm(A @ out[0] - b) <= 1e-5 * np.linalg.norm(b)
    # the other solvers take it like any other M
    W = np.asfortranarray(np.random.default_rng(97).standard_normal((b.size, 3)))
    assert np.linalg.norm(A @ api.defpcg(Ag, b, x0.copy(), W, Π)[0] - b) <= 1e-5 * np.linalg.norm(b)
    assert np.linalg.norm(A @ api.eigpcg(Ag, b, x0.copy(), Π, 3, 10)[0] - b) <= 1e-5 * np.linalg.norm(b)


def test_combine_refusals(pkg, ctx, kids):
    api = pkg.api
    Lb = pkg._lib.load()
    host_pointers(pkg, ctx)
    BAD = pkg._lib.MI_ERR_BAD_ARG
    n, ops = kids
    small = api.JacobiPreconditioner(ctx, np.ones(n - 1))
    f64p = pkg._lib.f64p

    def combine(hs, coef):
        arr = (vp * max(len(hs), 1))(*hs)
        cf = np.ascontiguousarray(coef, dtype=np.float64)
        h = vp()
        return Lb.mi_op_combine(ctx._h, i64(len(hs)), arr, cf.ctypes.data_as(f64p), C.byref(h)), h

    assert combine([], [1.0])[0] == BAD                                  # k = 0
    assert combine([ops[2]._h] * 17, np.ones(17))[0] == BAD              # k = 17
    rc, h = combine([ops[2]._h] * 16, np.ones(16))
    assert rc == 0 and Lb.mi_op_destroy(h) == 0
    assert combine([ops[0]._h, small._h], [0.5, 0.5])[0] == BAD          # mixed sizes
    for bad in (np.nan, np.inf):
        assert combine([ops[0]._h, ops[1]._h], [0.5, bad])[0] == BAD     # a non-finite coefficient
    with pytest.raises(ValueError, match="finite"):
        api.InterpolatingPreconditioner(ctx, [0.5, np.inf], ops[:2])
    Π = api.InterpolatingPreconditioner(ctx, [0.5, 0.5], ops[:2])
    with pytest.raises(ValueError, match="finite"):
        Π.set_coefficients([np.nan, 1.0])
    cf = np.array([np.nan, 1.0])
    assert Lb.mi_op_combine_set_coefficients(Π._h, cf.ctypes.data_as(f64p)) == BAD
    assert Lb.mi_op_combine_set_coefficients(ops[0]._h, cf.ctypes.data_as(f64p)) == BAD   # not a combination
    r = np.random.default_rng(98).standard_normal(n)
    assert np.array_equal(Π * r, _host_expression([0.5, 0.5], [ops[0] * r, ops[1] * r]))  # the refused calls changed nothing


def test_centroidal_preconds_and_the_interpolation_flow(pkg, ctx, fem):
    """Example12/14 in small: quantize, one AMG hierarchy per centroid, solve a fresh realization with the nearest one and
    with a Shepard combination; both converge"""
    api = pkg.api
    mesh = fem.get_mesh(24)
    dinds = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
    kl = fem.synthetic_kl(mesh.points, m_side=3)
    field = api.KLField(ctx, kl.Λ, kl.Ψ)

    def assemble(a, rhs=False):
        A, b = fem.do_isotropic_elliptic_assembly(mesh.cells, mesh.points, dinds, mesh.point_marker, a, ar.f_m1, ar.u3)
        return (A, b) if rhs else A

    A0 = assemble(np.ones(mesh.points[0].size))
    rng = np.random.default_rng(99)
    X, cen, _, _ = api.get_quantizer(ctx, 200, 4, kl.Λ, "L2-full", rng=rng)
    Πs = api.get_centroidal_preconds(ctx, cen, field, assemble, A0)
    assert len(Πs) == 4
    ξ = rng.standard_normal(kl.Λ.size)
    A, b = assemble(field.coefficient(ξ), rhs=True)
    Ag = api.SparseMatrixCSC(ctx, A)
    p = api.find_precond(ctx, fem.scale_data(ξ, kl.Λ, "L2"), fem.scale_data(cen, kl.Λ, "L2"))
    assert p == ref.find_precond(fem.scale_data(ξ, kl.Λ, "L2"), fem.scale_data(cen, kl.Λ, "L2"))
    x, it, _ = api.pcg(Ag, b, np.zeros(b.size), Πs[p])
    Π = api.InterpolatingPreconditioner(ctx, fem.shepard_coefficients(ξ, cen, kl.Λ), Πs)
    xi, iti, _ = api.pcg(Ag, b, np.zeros(b.size), Π)
    print(f"nearest centroid {p}: {it} iterations; Shepard combination of 4: {iti}")
    for sol in (x, xi):
        assert np.linalg.norm(A @ sol - b) <= 1e-5 * np.linalg.norm(b)
