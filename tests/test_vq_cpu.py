"""CPU suite of the quantizer: fem.py's host functions against tests/vq_ref.py (the loop form) bit for bit, the tiling as a
pure host function, the deterministic grid, CLVQ and the Shepard weights. No device call is made here."""
import ctypes as C

import numpy as np
import pytest

import vq_ref as ref

i64 = C.c_int64


def _tiling(pkg, d, ns, P):
    return pkg.api.vq_tiling(d, ns, P)


def _data(seed, d, ns):
    return np.random.default_rng(seed).standard_normal((d, ns))


def test_tiling_needs_no_device_and_is_a_function_of_the_sizes(pkg, fem):
    L = pkg._lib.load()
    a, b = _tiling(pkg, 170, 100_000, 10_000), _tiling(pkg, 170, 100_000, 10_000)
    assert a == b and all(v >= 1 for v in a)
    point_tile, cent_tile, k_chunk, splits, sum_chunk = a
    assert sum_chunk == fem.VQ_SUM_CHUNK
    assert _tiling(pkg, 3, 100_000, 10_000)[:3] == (point_tile, cent_tile, k_chunk)     # the tile sizes are constants
    assert _tiling(pkg, 170, 1, 1)[3] == 1
    assert _tiling(pkg, 170, 1, 10_000)[3] >= 2                                         # the ns = 1 shape of find_precond is split
    assert L.mi_vq_tiling(i64(3), i64(5), i64(2), None, None, None, None, None) == 0     # every output may be NULL
    BAD = pkg._lib.MI_ERR_BAD_ARG
    for d, ns, P in [(0, 5, 2), (3, 0, 2), (3, 5, 0), (3, 2 ** 31, 2), (3, 5, 2 ** 31)]:
        assert L.mi_vq_tiling(i64(d), i64(ns), i64(P), None, None, None, None, None) == BAD


@pytest.mark.parametrize("d,ns,P", [(1, 1, 1), (3, 70, 9), (17, 300, 33)])
def test_assign_and_objective_carry_the_bits_of_the_loop(fem, d, ns, P):
    X, Cn = _data(1, d, ns), _data(2, d, P)
    Cn[:, P // 2] = Cn[:, 0]                       # a tie between two centroids: the lower index
    X[:, ns // 2] = Cn[:, P - 1]                   # a sample on a centroid
    a, c = fem.vq_assign(X, Cn, block=64)
    ar, cr = ref.assign(X, Cn)
    assert np.array_equal(a, ar) and np.array_equal(c, cr)
    assert c[ns // 2] == 0.0
    if P > 1:
        assert a[ns // 2] == P - 1 and not np.any(a == P // 2)
    for chunk in (1, 7, 256):
        assert fem.vq_objective(c, chunk) == ref.objective(cr, chunk)
    assert fem.get_distortion(X, Cn) == ref.objective(cr, fem.VQ_SUM_CHUNK) / ns


def test_scan_keeps_a_nan_at_centroid_zero_and_skips_it_elsewhere(fem):
    X = _data(3, 2, 4)
    Cn = _data(4, 2, 3)
    C0, C1 = Cn.copy(), Cn.copy()
    C0[0, 0], C1[0, 1] = np.nan, np.nan
    for Cx in (C0, C1):
        a, c = fem.vq_assign(X, Cx)
        ar, cr = ref.assign(X, Cx)
        assert np.array_equal(a, ar) and np.array_equal(c, cr, equal_nan=True)
    assert np.all(fem.vq_assign(X, C0)[0] == 0) and np.all(np.isnan(fem.vq_assign(X, C0)[1]))
    assert not np.any(fem.vq_assign(X, C1)[0] == 1)


def test_update_seed_and_kmeans_carry_the_bits_of_the_loop(fem):
    X = _data(5, 3, 300)
    a = np.random.default_rng(6).integers(0, 7, 300)
    a[a == 4] = 0                                   # cluster 4 is empty
    Cn = _data(7, 3, 7)
    got, want = fem.vq_update(X, a, Cn), ref.update(X, a, Cn)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[1][4] == 0 and np.array_equal(got[0][:, 4], Cn[:, 4])
    u = np.random.default_rng(8).random(9)
    u[1], u[2] = 0.0, np.nextafter(1.0, 0.0)
    for chunk in (16, 256):
        got, want = fem.kmpp_seed(X, 9, u, chunk), ref.seed(X, 9, u, chunk)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert len(set(got[0])) == 9
    with pytest.raises(ValueError, match="distinct"):
        fem.kmpp_seed(np.ones((2, 5)), 2, u)
    assert ref.seed(np.ones((2, 5)), 2, u, 256) is None
    for d, ns, P in [(2, 257, 5), (3, 120, 17)]:
        X = _data(9 + d, d, ns)
        r, w = fem.kmeans(X, X[:, :P]), ref.kmeans(X, X[:, :P], fem.VQ_SUM_CHUNK)
        assert (r.iterations, r.converged, r.totalcost) == (w["iterations"], w["converged"], w["totalcost"])
        assert 1 < r.iterations < 1000 and r.converged
        for f in ("centers", "assignments", "costs", "counts"):
            assert np.array_equal(getattr(r, f), w[f]), f
    r = fem.kmeans(X, X[:, :P], maxiter=2)
    assert r.iterations == 2 and not r.converged
    with pytest.raises(ValueError, match="finite"):
        fem.kmeans(np.where(np.arange(ns) == 3, np.nan, X), X[:, :P])


def test_find_precond_pads_the_centroids_with_zeros(fem):
    rng = np.random.default_rng(10)
    x, hXt = rng.standard_normal(9), rng.standard_normal((4, 6))
    assert fem.find_precond(x, hXt) == ref.find_precond(x, hXt)
    hXt[:, 3] = x[:4]
    x[4:] = 0.0
    assert fem.find_precond(x, hXt) == 3


@pytest.mark.parametrize("nKL", [0, 1, 3])
def test_deterministic_grid(fem, nKL):
    Λ, s = np.array([4.0, 9.0, 16.0, 25.0]), 1.5
    P = 2 ** nKL + 2
    hη, hξ = fem.get_deterministic_grid(P, nKL, Λ, s)
    assert hη.shape == hξ.shape == (nKL, P)
    assert np.all(hξ[:, 0] == 0.0)
    want = np.zeros((nKL, P))
    for p in range(1, 2 ** nKL + 1):                 # bitstring(p)[end-(nKL-1):end], '0' -> -s
        bits = format(p, "064b")[64 - nKL:] if nKL else ""
        for k in range(nKL):
            want[k, p] = -s if bits[k] == "0" else s
    assert np.array_equal(hξ, want)
    assert np.array_equal(hη, np.sqrt(Λ[:nKL])[:, None] * hξ)
    if nKL:
        assert len({tuple(c) for c in hξ[:, 1:2 ** nKL + 1].T}) == 2 ** nKL     # every corner once
        assert np.all(hξ[:, 2 ** nKL] == -s)                                    # p = 2^nKL: its last nKL bits are zero
        with pytest.raises(ValueError):
            fem.get_deterministic_grid(2 ** nKL, nKL, Λ, s)


def test_clvq_and_gain_sequence(fem):
    X = _data(11, 3, 150)
    γ = fem.get_gain_sequence(1.0, 0.1, 0.2, 0.51, 150)
    assert γ.shape == (150,) and γ[0] == 1.0 * 0.1 / (1.0 + 0.2) and np.all(np.diff(γ) < 0)
    inds = np.array([5, 17, 3, 99])
    H = fem.clvq(X, 4, γ, inds)
    assert np.array_equal(H, ref.clvq(X, X[:, inds], γ))
    assert np.array_equal(fem.clvq(X, 4, γ, X[:, inds]), H)


def test_scaling_round_trip_and_shepard(pkg, fem):
    rng = np.random.default_rng(12)
    Λ = np.array([0.06, 0.05, 0.03, 0.01])
    ξ = rng.standard_normal((4, 6))
    from scipy.special import ndtr
    assert np.array_equal(fem.scale_data(ξ, Λ, "L2"), ξ * np.sqrt(Λ)[:, None])
    assert np.array_equal(fem.scale_data(ξ[:, 0], Λ, "cdf"), ndtr(ξ[:, 0]) * np.sqrt(Λ))
    assert fem.scale_data(ξ, Λ, "L2-10%").shape == (2, 6)          # cumsum(Λ) reaches 0.1 at the second mode
    for dist in ("L2", "L2-full", "cdf", "cdf-full", "L2-10%"):
        Y = fem.scale_data(ξ, Λ, dist)
        assert np.allclose(fem.unscale_centers(Y, Λ, dist), ξ[:Y.shape[0]], rtol=1e-9, atol=1e-12)
    assert fem.get_scaled_data(7, Λ, "L2", np.random.default_rng(1)).shape == (4, 7)
    I = rng.standard_normal((4, 5))
    for dist in ("L2-full", "cdf-full"):
        c = fem.shepard_coefficients(ξ[:, 0], I, Λ, dist)
        assert c.shape == (5,) and np.all(c > 0) and abs(c.sum() - 1.0) <= 5 * 2.0 ** -52
    # the quirk: the difference is weighted with Λ, not sqrt.(Λ)
    d2 = np.array([np.dot((I[:, i] - ξ[:, 0]) * Λ, (I[:, i] - ξ[:, 0]) * Λ) for i in range(5)])
    assert np.allclose(fem.shepard_coefficients(ξ[:, 0], I, Λ), (1 / d2) / (1 / d2).sum(), rtol=1e-13)
    I[:, 2] = ξ[:, 0]
    assert not np.all(np.isfinite(fem.shepard_coefficients(ξ[:, 0], I, Λ)))
    with pytest.raises(ValueError, match="finite"):
        pkg.api.InterpolatingPreconditioner._coef([0.5, np.inf])
