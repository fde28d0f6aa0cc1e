"""GPU suite of the device AMG set-up on frozen aggregates: `api.AMGPreconditioner(ctx, A, device_setup=True)`
(`mi_amg_plan_create`, csrc/amg_plan.hpp + csrc/amg_setup.hpp) and `.set_values` (`mi_amg_set_values`). Every case is created
on A0 and then given `set_values(A1)`.

Level-local check of `device_hierarchy()`: every level is recomputed on the host from the device's own A_l (and, for the
Galerkin product, from the device's own P_l), so no error accumulates across levels. With kA, kR the longest rows of A_l
and R_l and u = 2^-52 (tests/amg_refresh_ref.level_bounds):
    |ω_dev - ω_host| <= (kA + 2) u ω, the same for g = 4 / (3 ω) and, entry by entry, for ω/d
    |P_dev - P_host| <= (kA + 4) u (|T| + |wd| |A_l| |T|)                       entry by entry
    |A_{l+1,dev} - sym(P' A_l P)_host| <= (kR + kA + 4) u (|P|' |A_l| |P|)       entry by entry, A_{l+1} exactly symmetric
(row sums of at most kA terms, one division, one product and one difference; the products sum at most kA resp. kR terms of
products of rounded factors; both sides are within half the bound of the exact value). Coarse inverse against numpy's of the
device's own A_L: ||I - Z_dev A_L||_F <= 8 ||I - Z_np A_L||_F + n_c u (the 8 for the unpivoted elimination's larger constant).
The apply against the numpy cycle on the hierarchy read back (the bar and the right-hand sides of tests/test_gpu_amg.py: the
hierarchy is identical on both sides). The solves against the restatement with `fem.amg_refresh`."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import amg_ref as ar
import amg_refresh_ref as rr
from amg_refresh_ref import check_coarse as _check_coarse, check_levels as _check_levels
from test_gpu_amg import APPLY_BAR, _assert_solve, _rel, _rhs

pytestmark = pytest.mark.gpu

U = rr.U


def _inputs(fem, case):
    """(A0, A1, constructor keywords)"""
    if case.startswith("N"):
        N, kw = {"N12_2": (12, dict(max_levels=2, max_coarse=10)), "N12_3": (12, dict(max_levels=3, max_coarse=4)),
                 "N12_1": (12, dict(max_levels=1)), "N34": (34, {}), "N100": (100, {})}[case]
        A0, A1, _ = rr.pair(fem, N)
        return A0, A1, kw
    if case == "giant":
        A0, A1, aggs = rr.giant_aggregates(fem)
        return A0, A1, dict(aggregates=aggs)
    A0, A1 = rr.synthetic_pair(int(case[4:]))
    return A0, A1, {}


def _same_hierarchy(Ha, Hb):
    same = lambda X, Y: np.array_equal(X.indptr, Y.indptr) and np.array_equal(X.indices, Y.indices) and np.array_equal(X.data, Y.data)
    return (Ha.sizes == Hb.sizes and all(same(a, b) for a, b in zip(Ha.A, Hb.A)) and all(same(a, b) for a, b in zip(Ha.P, Hb.P))
            and Ha.omega == Hb.omega and all(np.array_equal(a, b) for a, b in zip(Ha.omega_over_d, Hb.omega_over_d))
            and np.array_equal(Ha.coarse_inv, Hb.coarse_inv))


def _check_apply(M, H, tag):
    outs = []
    for k, r in enumerate(_rhs(H.sizes[0], 5)):
        got, want = M.ldiv(r), ar.cycle(H, r)
        err = _rel(got, want)
        print(f"{tag} apply rhs {k}: rel. error {err:.3e} (bar {APPLY_BAR:.0e})")
        assert err <= APPLY_BAR, (tag, k, err)
        assert np.array_equal(M.ldiv(r), got)
        outs.append(got)
    return outs


@pytest.mark.parametrize("case", ["N12_2", "N12_3", "N12_1", "N34", "grid1023", "grid1025", "giant", "N100"])
def test_refresh_levels_inverse_and_apply(pkg, ctx, fem, case):
    """created on A0, refreshed to A1: the level-local bounds, the coarse inverse, the apply; two refreshes with the same
    values read back bit-identical; the plan's bytes are in the statistics"""
    A0, A1, kw = _inputs(fem, case)
    M = pkg.api.AMGPreconditioner(ctx, A0, device_setup=True, **kw)
    try:
        aggs = M.aggregates
        H0 = M.device_hierarchy()
        want_levels = {"N12_2": 2, "N12_3": 3, "N12_1": 1, "giant": 2, "N100": 3}.get(case)
        assert want_levels is None or H0.nlevels == want_levels
        if case == "giant":
            R = sp.csr_matrix(H0.P[0].T)
            assert np.diff(R.indptr).max() >= 1100 and np.diff(H0.P[0].indptr).min() == 1 and np.diff(H0.A[1].indptr).max() > 8
        _check_levels(H0, aggs, f"{case} (create)")
        M.set_values(A1)
        H1 = M.device_hierarchy()
        assert np.array_equal(H1.A[0].data, A1.data) and H1.sizes == H0.sizes
        _check_levels(H1, aggs, case)
        _check_coarse(H1, case)
        _check_apply(M, H1, case)
        M.set_values(A1.data)
        assert _same_hierarchy(M.device_hierarchy(), H1), "two refreshes with the same values differ"
        st = M.stats()
        assert st["n_levels"] == H1.nlevels and st["coarse_n"] == H1.sizes[-1] and st["operator_nnz"] == sum(a.indices.size for a in H1.A)
        nc = H1.sizes[-1]
        cycle = 8 * nc * nc + sum(12 * H1.A[l].indices.size + 24 * H1.P[l].indices.size + 8 * H1.sizes[l] for l in range(H1.nlevels - 1))
        assert st["bytes_kept"] > cycle
        prof = M.refresh_profile()                            # the timed refresh is a refresh on the values held: nothing moves
        assert len(prof) == 6 and all(v >= 0.0 for v in prof.values()) and sum(prof.values()) > 0.0
        assert _same_hierarchy(M.device_hierarchy(), H1)
    finally:
        M.close()


def test_one_based_arrays_give_the_same_bits(pkg, ctx, fem):
    A0, A1, _ = rr.pair(fem, 34)
    out = []
    for base in (0, 1):
        M = pkg.api.AMGPreconditioner(ctx, A0, index_base=base, device_setup=True)
        M.set_values(A1)
        out.append((M.device_hierarchy(), [M.ldiv(r) for r in _rhs(A0.shape[0], 5)]))
        M.close()
    assert _same_hierarchy(out[0][0], out[1][0])
    assert all(np.array_equal(a, b) for a, b in zip(out[0][1], out[1][1]))


def test_read_back_of_a_host_hierarchy(pkg, ctx, fem):
    """the accessors on an operator of mi_amg_create return what it was given (ω one rounding away)"""
    H = ar.case(fem, 40, "lognormal")[2]
    M = pkg.api.AMGPreconditioner(ctx, H)
    G = M.device_hierarchy()
    M.close()
    assert G.sizes == H.sizes and np.array_equal(G.coarse_inv, H.coarse_inv)
    for a, b in list(zip(G.A, H.A)) + list(zip(G.P, H.P)):
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and np.array_equal(a.data, b.data)
    for l in range(H.nlevels - 1):
        assert np.array_equal(G.omega_over_d[l], H.omega_over_d[l]) and abs(G.omega[l] - H.omega[l]) <= 2 * U * H.omega[l]


@pytest.mark.parametrize("N,coeff,cap", [c for c in ar.LOOP_CASES if c[1] == "lognormal"])
def test_pcg_after_a_refresh(pkg, ctx, fem, N, coeff, cap):
    """pcg(A1, b, 0, M) after set_values: `it` of the restatement on fem.amg_refresh, history within 1e-8 res_k + 1e-12 res_1;
    the eager solve bit for bit the replayed one; a solve before the refresh, the refresh, a solve on the same objects: the
    bits of a solve on an operator created for A1 (the graphs see the new values and nothing stale); set_values(A0) again
    restores the first apply's bits"""
    api = pkg.api
    A0, A1, b = rr.pair(fem, N)
    H1, want = rr.refreshed_solve(fem, N)
    assert want[1] <= cap
    n = b.size
    x0 = np.zeros(n)
    r = _rhs(n, 11)[0]
    Ag, M = api.SparseMatrixCSC(ctx, A1), api.AMGPreconditioner(ctx, A0, device_setup=True)
    M2 = None
    try:
        z_first = M.ldiv(r)
        stale = api.pcg(Ag, b, x0, M)
        M.set_values(A1)
        got = api.pcg(Ag, b, x0, M)
        print(f"N = {N}: it = {got[1]} after the refresh, {stale[1]} with the hierarchy of A0")
        _assert_solve(got, want, f"pcg after set_values N = {N}")
        assert stale[1] > got[1]
        try:
            ctx.set_chunk(0)
            eager = api.pcg(Ag, b, x0, M)
        finally:
            ctx.set_chunk(8)
        assert eager[1] == got[1] and np.array_equal(eager[0], got[0]) and np.array_equal(eager[2], got[2])
        M2 = api.AMGPreconditioner(ctx, A1, device_setup=True)
        assert all(np.array_equal(a, c) for a, c in zip(M2.aggregates, M.aggregates))
        fresh = api.pcg(Ag, b, x0, M2)
        assert fresh[1] == got[1] and np.array_equal(fresh[0], got[0]) and np.array_equal(fresh[2], got[2])
        assert np.array_equal(M2.ldiv(r), M.ldiv(r))
        M.set_values(A0)
        assert np.array_equal(M.ldiv(r), z_first)
        again = api.pcg(Ag, b, x0, M)
        assert again[1] == stale[1] and np.array_equal(again[0], stale[0]) and np.array_equal(again[2], stale[2])
    finally:
        if M2 is not None:
            M2.close()
        M.close(); Ag.close()


def test_refusals_and_failures_leave_the_previous_hierarchy(pkg, ctx, fem):
    """set_values on an operator of mi_amg_create: MI_ERR_BAD_ARG (TypeError from the Python class); a wrong-length array is
    caught in Python; a NaN in nzval is refused, a negated diagonal entry gives MI_ERR_SINGULAR; a communicator context is
    refused at create. After each failed call the next apply gives the previous bits."""
    api, L = pkg.api, pkg._lib
    lib = L.load()
    A0, A1, _ = rr.pair(fem, 34)
    n = A0.shape[0]
    r = _rhs(n, 3)[0]
    Mh = api.AMGPreconditioner(ctx, fem.prepare_amg_precond(A0))
    zh = Mh.ldiv(r)
    with pytest.raises(TypeError, match="device_setup"):
        Mh.set_values(A1)
    v = np.ascontiguousarray(A1.data)
    rc = lib.mi_amg_set_values(Mh._h, v.ctypes.data_as(C.c_void_p))
    msg = lib.mi_last_error().decode()
    print("  refused:", msg)
    assert rc == L.MI_ERR_BAD_ARG and "mi_amg_create" in msg and len(msg) > 40
    assert np.array_equal(Mh.ldiv(r), zh)
    Aop = api.SparseMatrixCSC(ctx, A0)
    assert lib.mi_amg_set_values(Aop._h, v.ctypes.data_as(C.c_void_p)) == L.MI_ERR_BAD_ARG
    assert lib.mi_amg_level_sizes(Aop._h, 0, None, None, None, None) == L.MI_ERR_BAD_ARG
    assert lib.mi_amg_level_sizes(Mh._h, 7, None, None, None, None) == L.MI_ERR_BAD_ARG
    Aop.close(); Mh.close()

    M = api.AMGPreconditioner(ctx, A0, device_setup=True)
    try:
        M.set_values(A1)
        z1, H1 = M.ldiv(r), M.device_hierarchy()
        with pytest.raises(ValueError, match="entries"):
            M.set_values(A1.data[:-1])
        assert np.array_equal(M.ldiv(r), z1)
        bad = A1.data.copy(); bad[bad.size // 2] = np.nan
        with pytest.raises(api.MiError) as e:
            M.set_values(bad)
        print("  refused:", e.value)
        assert "finite" in str(e.value) and len(str(e.value)) > 40
        assert np.array_equal(M.ldiv(r), z1)
        neg = A1.copy()
        rows = np.repeat(np.arange(n), np.diff(neg.indptr))
        k = np.flatnonzero(rows == neg.indices)[n // 2]
        neg.data[k] = -neg.data[k]
        with pytest.raises(api.MiError) as e:
            M.set_values(neg)
        print("  refused:", e.value)
        assert e.value.code == L.MI_ERR_SINGULAR and "diagonal" in str(e.value)
        assert np.array_equal(M.ldiv(r), z1)
        assert _same_hierarchy(M.device_hierarchy(), H1)
        aggs = M.aggregates
    finally:
        M.close()
    with pytest.raises(api.MiError) as e:                    # a matrix that is not positive definite at create
        api.AMGPreconditioner(ctx, neg, device_setup=True, aggregates=aggs)
    assert e.value.code == L.MI_ERR_SINGULAR
    grp = api.LoopbackGroup(2)
    grp.set_mode(1)
    rank0 = api.Context(0)
    rank0.loopback_init(grp, 0)
    with pytest.raises(api.MiError) as e:
        api.AMGPreconditioner(rank0, A0, device_setup=True)
    assert e.value.code == L.MI_ERR_BAD_ARG and "rank 0 of 2" in str(e.value) and len(str(e.value)) > 40
    rank0.close()
