"""GPU suite of `Pl` = AMG in the device interior CG (`mi_schur_interior_amg`; csrc/interior_amg.hpp, the ICG_PL_EXT
instantiations of the k_icg_* kernels of csrc/kernels.hpp, k_amg_post_dot / k_amg_coarse_dom of csrc/amg.hpp), against the numpy restatement of
tests/interior_amg_ref.py. The cases, their seeds and why an iteration count is comparable at all: that file and
tests/test_interior_amg_cpu.py::test_counts_are_not_marginal.

Bars: the S-apply and schur_rhs within 1e-7 max|.| of the exact (dense / sparse direct) answer, the bar
tests/test_gpu_parity.py has for this inexact solve; the true residual of an interior solve within 2 reltol ‖b‖_d per
subdomain (the recurrence's residual meets reltol ‖b‖_d; the 2 caps its rounding drift, and the restatement meets it on
the CPU); iteration counts equal; repeated applies equal bit for bit."""
import numpy as np
import pytest
import scipy.sparse as sp

import interior_amg_ref as ir
from interior_amg_ref import close as _close, new_values as _new_values, op as _op, residuals as _residuals

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ir.NAMES)
def test_interior_amg_against_the_restatement(pkg, ctx, fem, monkeypatch, name):
    api = pkg.api
    C = ir.case(fem, name)
    H = C.hierarchy(fem)
    x = C.x()
    _, its, _, _ = C.solve(fem, x)
    exact = C.exact_apply(x)
    Sx = api.LocalSchurs(ctx, C.Sd(), C.gather_idx, C.node_Γ_cnt)
    monkeypatch.setenv("MI355_ICG_CHUNK", "1")
    S1 = _op(api, ctx, C)
    S1b = _op(api, ctx, C)
    monkeypatch.delenv("MI355_ICG_CHUNK")
    Sdef = _op(api, ctx, C)
    monkeypatch.setenv("MI355_ICG_FUSED", "1")
    Sfused = _op(api, ctx, C)
    monkeypatch.delenv("MI355_ICG_FUSED")
    Splain2 = _op(api, ctx, C, second=True)
    ops = [Sx, S1, S1b, Sdef, Sfused, Splain2]
    try:
        st = S1.interior_amg(C.A_II, **C.kw)
        assert st["levels"] == H.nlevels and st["coarse_n"] == H.sizes[-1] and st["bytes_kept"] > 0
        # 1. the count of one apply, one iteration per replay
        it0 = S1.interior_iterations()
        y1 = S1 * x
        got = S1.interior_iterations() - it0
        print(f"{name}: levels {H.sizes}, iterations device {got}, restatement {its.tolist()}")
        assert got == int(its.max())
        # 3. against the exact operator
        e3 = _close(y1, exact)
        e3x = _close(Sx * x, exact)
        print(f"{name}: S-apply error {e3:.2e} of max|Sx| (dense S_d on the device: {e3x:.2e})")
        assert e3 <= 1e-7 and e3x <= 1e-12
        # 4. repeated applies, chunk 1 and the default chunk; the chunk does not change the bits either
        assert np.array_equal(S1 * x, y1)
        Sdef.interior_amg(C.A_II, **C.kw)
        yd = Sdef * x
        assert np.array_equal(Sdef * x, yd) and np.array_equal(yd, y1)
        # MI355_ICG_FUSED is ignored while the AMG is selected: the 3-launch form, the same bits
        Sfused.interior_amg(C.A_II, **C.kw)
        assert np.array_equal(Sfused * x, y1)
        # 5. 1-based aggregates
        S1b.interior_amg(sizes=H.sizes, aggregates=H.agg, index_base=1)
        assert np.array_equal(S1b * x, y1)
        # 2. the true residual of interior_solutions(0, b_I), every subdomain
        bI = C.b_I()
        u = Sdef.interior_solutions(np.zeros(C.n_Γ), bI)
        for d, (rn, bn) in enumerate(_residuals(C, u, bI)):
            print(f"{name}: subdomain {d}: ‖b - A u‖ / ‖b‖ = {rn / bn if bn else 0.0:.2e}")
            assert rn <= 2.0 * ir.RELTOL * bn, d
        # 9. schur_rhs against the host get_schur_rhs (sparse direct interior solves)
        want = fem.get_schur_rhs(C.b_Id, C.A_II, C.A_IΓ, C.b_Γ, C.gather_idx, C.host_solvers())
        got_rhs = Sdef.schur_rhs(bI, C.b_Γ)
        scale = max(np.abs(want).max(), np.abs(C.b_Γ).max())
        assert np.abs(got_rhs - want).max() <= 1e-7 * scale
        # 10. a NaN in x ends the apply; the next apply is the one of before
        xn = x.copy()
        xn[0] = np.nan
        it0 = Sdef.interior_iterations()
        yn = Sdef * xn
        it1 = Sdef.interior_iterations()
        assert np.array_equal(Sdef * x, yd)
        assert np.isnan(yn).any() and it1 - it0 <= Sdef.interior_iterations() - it1     # no more replays than the clean apply
        # 6. new values: the hierarchy is redone on the device; the count is the restatement's on fem.amg_refresh
        x2 = C.x(True)
        _, its2, _, _ = C.solve(fem, x2, second=True)
        S1.set_values(*_new_values(C))
        it0 = S1.interior_iterations()
        y2 = S1 * x2
        got2 = S1.interior_iterations() - it0
        print(f"{name}: after set_values: iterations device {got2}, restatement {its2.tolist()}")
        assert got2 == int(its2.max())
        exact2 = C.exact_apply(x2, second=True)
        assert _close(y2, exact2) <= 1e-7
        assert np.array_equal(S1 * x2, y2)
        # 7. back to the plain iteration, bit for bit
        yp = Splain2 * x2
        S1.interior_precond(None)
        with pytest.raises(api.MiError):
            S1.interior_amg_stats()
        assert np.array_equal(S1 * x2, yp)
        S1.interior_precond("diagonal")
        Splain2.interior_precond("diagonal")
        assert np.array_equal(S1 * x2, Splain2 * x2)
    finally:
        for S in ops:
            S.close()


def test_interior_amg_on_global_schur(pkg, ctx, fem, monkeypatch):
    """the same on `apply_global_schur` (EPDD.jl:596-625), ragged: count, exactness, repeatability, the way back, schur_rhs"""
    from conftest import f_m1, lognormal_coeff, u0734
    api = pkg.api
    C = ir.case(fem, "ragged")
    P = fem.build_schur_problem(50, 3, 2, lognormal_coeff(fem, fem.get_mesh(50).points, 7), f_m1, u0734, assemble=False, precond=False)
    A_IIg, A_IΓg, A_ΓΓ, b_Id, b_Γ = fem.prepare_global_schur(P.mesh.cells, P.mesh.points, P.epart, P.sub, lognormal_coeff(fem, P.mesh.points, 7),
                                                           f_m1, u0734)
    x = C.x()
    _, its, _, _ = C.solve(fem, x)
    exact = C.exact_apply(x)
    monkeypatch.setenv("MI355_ICG_CHUNK", "1")
    G = api.GlobalSchur(ctx, A_IIg, A_IΓg, A_ΓΓ, None, reltol=ir.RELTOL)
    monkeypatch.delenv("MI355_ICG_CHUNK")
    Gp = api.GlobalSchur(ctx, A_IIg, A_IΓg, A_ΓΓ, None, reltol=ir.RELTOL)
    try:
        yp = Gp * x
        st = G.interior_amg(A_IIg)
        assert st["levels"] == 3 and st["coarse_n"] == 50
        it0 = G.interior_iterations()
        y = G * x
        assert G.interior_iterations() - it0 == int(its.max())
        assert _close(y, exact) <= 1e-7
        assert np.array_equal(G * x, y)
        bI = np.concatenate(b_Id)
        want = fem.get_schur_rhs(b_Id, A_IIg, A_IΓg, b_Γ)
        assert np.abs(G.schur_rhs(bI, b_Γ) - want).max() <= 1e-7 * max(np.abs(want).max(), np.abs(b_Γ).max())
        u = G.interior_solutions(np.zeros(C.n_Γ), bI)
        for d, (rn, bn) in enumerate(_residuals(C, u, bI, blocks=A_IIg)):
            assert rn <= 2.0 * ir.RELTOL * bn, d
        G.interior_precond(None)
        assert np.array_equal(G * x, yp)
    finally:
        G.close(); Gp.close()


def test_refusals_leave_the_selected_pl(pkg, ctx, fem):
    """MI_ERR_BAD_ARG: a host-callback operator, a loopback-sharded operator, an aggregate id out of range, an aggregate
    across two subdomains, level sizes that do not chain; stats without a selected AMG. After a refused call on an operator
    with the AMG selected, that AMG still answers."""
    api, L = pkg.api, pkg._lib
    C = ir.case(fem, "n12_3")
    H = C.hierarchy(fem)
    x = C.x()
    args = (C.A_II, C.A_IΓ, C.A_ΓΓ, C.gather_idx, C.node_Γ_cnt)
    Sh = api.MatrixFreeLocalSchurs(ctx, *args, C.host_solvers())
    with pytest.raises(api.MiError) as e:
        Sh.interior_amg(C.A_II, **C.kw)
    assert e.value.code == L.MI_ERR_BAD_ARG and "interior solve on the device" in str(e.value)
    Sh.close()
    grp = api.LoopbackGroup(2)
    grp.set_mode(1)
    rank0 = api.Context(0)
    rank0.loopback_init(grp, 0)
    Ss = api.MatrixFreeLocalSchurs(rank0, *args, None, reltol=ir.RELTOL, dom_slice=(0, 2))
    with pytest.raises(api.MiError) as e:
        Ss.interior_amg(C.A_II, **C.kw)
    print("  refused:", e.value)
    assert e.value.code == L.MI_ERR_BAD_ARG and "sharded" in str(e.value)
    Ss.close(); rank0.close()

    S = _op(api, ctx, C)
    try:
        with pytest.raises(api.MiError):
            S.interior_amg_stats()
        S.interior_amg(C.A_II, **C.kw)
        y = S * x
        bad = [a.copy() for a in H.agg]
        bad[0][3] = H.sizes[1]                                   # one past the last aggregate
        with pytest.raises(api.MiError) as e:
            S.interior_amg(sizes=H.sizes, aggregates=bad)
        print("  refused:", e.value)
        assert e.value.code == L.MI_ERR_BAD_ARG and "aggregate" in str(e.value)
        assert np.array_equal(S * x, y)
        _, offs = C.stacked()
        cross = [a.copy() for a in H.agg]
        cross[0][offs[1]] = cross[0][0]                          # the first node of subdomain 1 joins an aggregate of subdomain 0
        with pytest.raises(api.MiError) as e:
            S.interior_amg(sizes=H.sizes, aggregates=cross)
        print("  refused:", e.value)
        assert e.value.code == L.MI_ERR_BAD_ARG and "subdomains" in str(e.value)
        with pytest.raises(api.MiError) as e:
            S.interior_amg(sizes=[H.sizes[0] + 1] + list(H.sizes[1:]), aggregates=[np.append(H.agg[0], 0)] + list(H.agg[1:]))
        assert e.value.code == L.MI_ERR_BAD_ARG and "chain" in str(e.value)
        assert np.array_equal(S * x, y)
        assert S.interior_amg_stats()["levels"] == H.nlevels
    finally:
        S.close()


@pytest.mark.parametrize("name", ["n12_3", "n12_1"])
def test_singular_set_values_leaves_the_previous_answers(pkg, ctx, fem, name):
    """a diagonal entry of A_II that is not positive: set_values returns MI_ERR_SINGULAR before it stores anything — the
    operator answers as before, and a later good set_values works"""
    api, L = pkg.api, pkg._lib
    C = ir.case(fem, name)
    x = C.x()
    S = _op(api, ctx, C)
    try:
        S.interior_amg(C.A_II, **C.kw)
        y = S * x
        neg = [sp.csc_matrix(A).copy() for A in C.A_II]
        for M in neg:
            M.sort_indices()
        M, j = neg[1], neg[1].shape[0] // 2                          # one diagonal entry of subdomain 1 negated, pattern kept
        k = M.indptr[j] + int(np.searchsorted(M.indices[M.indptr[j]:M.indptr[j + 1]], j))
        assert M.indices[k] == j and M.data[k] > 0
        M.data[k] = -M.data[k]
        ii = ir.csc_values(neg)
        assert ii.size == ir.csc_values(C.A_II).size
        with pytest.raises(api.MiError) as e:
            S.set_values(ii, None, None)
        print("  refused:", e.value)
        assert e.value.code == L.MI_ERR_SINGULAR
        assert np.array_equal(S * x, y)
        S.set_values(*_new_values(C))
        x2 = C.x(True)
        exact2 = C.exact_apply(x2, second=True)
        assert _close(S * x2, exact2) <= 1e-7
    finally:
        S.close()
