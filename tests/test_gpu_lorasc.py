"""GPU suite of the device LORASC preconditioner `api.LorascPreconditioner` (`mi_lorasc_*`): the M of
`pcg(A, b, zeros, ΠA_lorasc)` and `defpcg(A, b, zeros, ϕ, ΠA_lorasc)` (Example03:245-268). Applies against the refined
host restatement of `apply_lorasc` (tests/lorasc_ref.py) at the project's bar for the device's exact elimination against
the host (relative 2-norm 1e-10); the edges of the new kernels; determinism; new realizations; the solvers
against the oracle with the dense restated M^-1 as its preconditioner; the error returns; the example's `--lorasc` leg.

Measured margins of the apply test (MI355X, worst case over all inputs and variants): see DESIGN §6c."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT, lognormal_coeff, lowest_eigvecs
from test_gpu_parity import RES_FLOOR, RES_RTOL, X_RTOL, assert_history
import lorasc_ref as lr

pytestmark = pytest.mark.gpu

APPLY_BAR = 1e-10


@pytest.fixture(scope="module")
def cases(fem):
    return lr.gpu_cases(fem)


def _csc_data(mats):
    out = []
    for m in mats:
        m = sp.csc_matrix(m)
        m.sort_indices()
        out.append(m.data)
    return np.concatenate(out)


def _device(pkg, ctx, c, E=None, coef=None, index_base=0):
    api, P = pkg.api, c.P
    setup = api.SchurSetup(ctx, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd)
    setup.keep_levels()
    setup.run()
    gg = api.SparseDirectPreconditioner(ctx, c.A_ΓΓ)
    return api.LorascPreconditioner(ctx, c.A_IΓd, (c.pos_I, c.pos_Γ), setup, gg, E, coef, index_base=index_base)


@pytest.fixture(scope="module")
def devs(pkg, ctx, cases):
    """one device operator per input, shared by the tests that only apply it (they leave it without a correction)"""
    return {k: _device(pkg, ctx, c) for k, c in cases.items()}


@pytest.mark.parametrize("name", lr.ALL_CASES)
def test_apply_against_refined_restatement(pkg, ctx, cases, devs, name):
    """random x; nev = 0, 1, 25, 257 (random E), coef = NULL and random positive: relative 2-norm error <= 1e-10 against the
    refined restatement; two applies bit-identical; host and device pointers bit-identical. The inputs cover the kernels'
    edges: n_Γ mod 256 = 1, 0, 255 (tail1, full, short1), Γ columns with one interior row, the empty hub column of the
    unstructured mesh, the 1 x 2 strip whose Γ columns all hold both subdomains."""
    import torch
    c, M = cases[name], devs[name]
    worst = 0.0
    for nev, with_coef in lr.APPLY_VARIANTS:
        x, E, coef = lr.apply_inputs(c, nev, with_coef)
        M.set_correction(E, coef)
        want = lr.apply_lorasc(c, x, E, coef, refine=2)
        got = M.ldiv(x)
        err = np.linalg.norm(got - want) / np.linalg.norm(want)
        worst = max(worst, err)
        print(f"lorasc apply {name}: n = {c.n}, n_Γ = {c.n_Γ}, nev = {nev}, coef = {'random' if with_coef else 'NULL'}: "
              f"rel. error {err:.3e} (bar {APPLY_BAR:.0e}, margin {APPLY_BAR / max(err, 1e-300):.1f}x)")
        assert err <= APPLY_BAR, (name, nev, with_coef, err)
        assert np.array_equal(M.ldiv(x), got), (name, nev)
        assert np.array_equal(pkg.api.apply_lorasc(M, torch.from_numpy(x).cuda()).cpu().numpy(), got), (name, nev)
    M.set_correction(None)
    print(f"lorasc apply {name}: worst rel. error {worst:.3e}")


def test_index_base_one_and_create_with_correction(pkg, ctx, cases):
    """a create with E and coef == a create without and set_correction; index_base 1 == index_base 0; bit for bit"""
    c = cases["micro"]
    x, E, coef = lr.apply_inputs(c, 25, True)
    M0 = _device(pkg, ctx, c)
    M0.set_correction(E, coef)
    M1 = _device(pkg, ctx, c, E, coef)
    Mb = _device(pkg, ctx, c, E, coef, index_base=1)
    z = M0.ldiv(x)
    assert np.array_equal(M1.ldiv(x), z) and np.array_equal(Mb.ldiv(x), z)
    a, d = M1.bytes()
    assert a > 2 * d > 0


def test_new_realization_equals_fresh_create(pkg, ctx, fem, cases):
    """plan re-run + mi_spd_direct_set_values + mi_lorasc_set_values + mi_lorasc_set_correction == a fresh create on the new
    realization, bit for bit (host and device values)"""
    import torch
    c1 = cases["ragged"]
    c2 = lr.make_case(fem, "ragged2", 50, 3, 2, lognormal_coeff(fem, c1.P.mesh.points, 8))
    x, E, coef = lr.apply_inputs(c2, 25, True)
    fresh = _device(pkg, ctx, c2, E, coef).ldiv(x)
    assert np.linalg.norm(fresh - lr.apply_lorasc(c2, x, E, coef, refine=2)) <= APPLY_BAR * np.linalg.norm(fresh)
    M = _device(pkg, ctx, c1, *lr.apply_inputs(c1, 1, False)[1:])
    before = M.ldiv(x)
    assert not np.array_equal(before, fresh)
    P2 = c2.P
    M.setup.run(_csc_data(P2.A_IIdd), _csc_data(P2.A_IΓdd), _csc_data(P2.A_ΓΓdd))
    M.A_ΓΓ_solver.set_values(sp.csc_matrix(c2.A_ΓΓ).data)
    M.set_values(_csc_data(c2.A_IΓd))
    M.set_correction(E, coef)
    assert np.array_equal(M.ldiv(x), fresh)
    P1 = c1.P                                            # back and forth through device pointers
    M.setup.run(_csc_data(P1.A_IIdd), _csc_data(P1.A_IΓdd), _csc_data(P1.A_ΓΓdd))
    M.A_ΓΓ_solver.set_values(sp.csc_matrix(c1.A_ΓΓ).data)
    M.set_values(torch.from_numpy(_csc_data(c1.A_IΓd)).cuda())
    M.set_correction(*lr.apply_inputs(c1, 1, False)[1:])
    assert np.array_equal(M.ldiv(x), before)


def _assert_solve(got, want, apply, b):
    """DESIGN §3's solver rows by the oracle's iteration count: up to 50 iterations `it` equal and the whole history within
    1e-8 res_k + 1e-12 res_1; the long-solve row (test_gpu_parity.assert_history) otherwise"""
    x, it, res = got
    xo, ito, reso = want
    print(f"it = {it} (oracle {ito}), max rel. history difference {np.max(np.abs(res - reso[:len(res)]) / reso[:len(res)]):.3e}")
    if max(it, ito) <= 50:
        assert it == ito, f"iteration counts differ: {it} vs oracle {ito}"
        assert np.allclose(res, reso, rtol=RES_RTOL, atol=RES_FLOOR * reso[0]), np.max(np.abs(res - reso) / reso)
        assert np.linalg.norm(x - xo) <= X_RTOL * np.linalg.norm(xo)
    else:
        assert_history(got, want, apply=apply, b=b)


def _oracle_M(orc, c, E, coef=None):
    Minv = lr.dense_minv(c, E, coef)
    return orc.neumann_neumann_operator([Minv], [np.arange(c.n)], np.ones(c.n, dtype=np.int64))


@pytest.mark.parametrize("name", ["micro", "ragged"])
def test_pcg_with_lorasc_against_oracle(pkg, ctx, orc, fem, cases, name):
    """pcg(A, b, 0, ΠA_lorasc) without correction, with the eigenvectors of fem.prepare_lorasc_precond as the reference
    applies them (coef = NULL) and with coef = Σ; a solve replayed from graphs == the eager solve, bit for bit"""
    api = pkg.api
    c = cases[name]
    E, Σ = fem.prepare_lorasc_precond(lr.dense_schur(c), c.A_ΓΓ, nvec=25, ε=0.2)
    assert 0 < E.shape[1] < 25
    A, Ao = api.SparseMatrixCSC(ctx, c.A), orc.csc_operator(c.A)
    x0 = np.zeros(c.n)
    M = _device(pkg, ctx, c)
    its = []
    for Ek, ck in ((None, None), (E, None), (E, Σ)):
        M.set_correction(Ek, ck)
        want = orc.pcg(Ao, c.b, x0, _oracle_M(orc, c, Ek, ck))
        got = api.pcg(A, c.b, x0, M)
        _assert_solve(got, want, Ao, c.b)
        assert got[1] == want[1]
        its.append(got[1])
    assert its[1] < its[0]                                # the correction as written already helps
    M.set_correction(E, None)
    ctx.set_chunk(0)
    eager = api.pcg(A, c.b, x0, M)
    ctx.set_chunk(4)
    replay = api.pcg(A, c.b, x0, M)
    ctx.set_chunk(8)
    replay8 = api.pcg(A, c.b, x0, M)
    for r in (replay, replay8):
        assert eager[1] == r[1] and np.array_equal(eager[0], r[0]) and np.array_equal(eager[2], r[2])


def test_defpcg_with_lorasc_against_oracle(pkg, ctx, orc, fem, cases):
    """defpcg(A, b, 0, ϕ, ΠA_lorasc), ϕ = the least dominant eigenvectors of A (Example03:258-262)"""
    api = pkg.api
    c = cases["micro"]
    E, _ = fem.prepare_lorasc_precond(lr.dense_schur(c), c.A_ΓΓ, nvec=25, ε=0.2)
    A, Ao = api.SparseMatrixCSC(ctx, c.A), orc.csc_operator(c.A)
    ϕ = lowest_eigvecs(Ao, c.n, len(c.A_IId) + 10)
    x0 = np.zeros(c.n)
    M = _device(pkg, ctx, c, E)
    _assert_solve(api.defpcg(A, c.b, x0, ϕ, M), orc.defpcg(Ao, c.b, x0, ϕ, _oracle_M(orc, c, E)), Ao, c.b)


def test_errors_do_not_fault(pkg, ctx, cases):
    """every MI_ERR_BAD_ARG of mi_lorasc_create returns the code and a message; a bound plan / A_ΓΓ operator cannot be
    destroyed, and the operator still applies afterwards"""
    api, L = pkg.api, pkg._lib
    c = cases["micro"]
    P = c.P
    M = _device(pkg, ctx, c)
    setup, gg = M.setup, M.A_ΓΓ_solver
    x = np.random.default_rng(5).standard_normal(c.n)
    z = M.ldiv(x)

    def refused(*args, **kw):
        with pytest.raises(api.MiError) as e:
            api.LorascPreconditioner(ctx, *args, **kw)
        assert e.value.code == L.MI_ERR_BAD_ARG and len(str(e.value)) > 40
        return str(e.value)

    maps = (c.pos_I, c.pos_Γ)
    dup = [p.copy() for p in c.pos_I]
    dup[1][0] = dup[0][0]
    assert "permutation" in refused(c.A_IΓd, (dup, c.pos_Γ), setup, gg)
    far = c.pos_Γ.copy()
    far[3] = c.n
    assert "out of range" in refused(c.A_IΓd, (c.pos_I, far), setup, gg)
    moved = [np.r_[c.pos_I[0], c.pos_I[1][:1]], c.pos_I[1][1:]] + list(c.pos_I[2:])
    assert "n_i" in refused(c.A_IΓd, (moved, c.pos_Γ), setup, gg)
    plain = api.SchurSetup(ctx, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd)
    assert "level" in refused(c.A_IΓd, maps, plain, gg)
    plain.keep_levels()                                   # kept, but no run after it
    assert "level" in refused(c.A_IΓd, maps, plain, gg)
    jac = api.JacobiPreconditioner(ctx, np.ones(c.n_Γ))
    assert "sparse direct" in refused(c.A_IΓd, maps, setup, jac)
    small = api.SparseDirectPreconditioner(ctx, sp.csc_matrix(c.A_ΓΓ)[:-1, :-1])
    msg = refused(c.A_IΓd, maps, setup, small)
    assert str(c.n_Γ) in msg and str(c.n_Γ - 1) in msg
    tall = sp.csc_matrix(c.A_IΓd[0]).copy()
    tall.resize((tall.shape[0] + 4, tall.shape[1]))
    tall = sp.csc_matrix(tall + sp.csc_matrix(([1.0], ([tall.shape[0] - 2], [0])), shape=tall.shape))
    assert "out of range" in refused([tall] + list(c.A_IΓd[1:]), maps, setup, gg)
    msg = refused(c.A_IΓd, maps, setup, gg, E=np.zeros((c.n_Γ, 1025)))
    assert "1025" in msg and "1024" in msg
    with pytest.raises(api.MiError) as e:
        M.set_correction(np.zeros((c.n_Γ, 1025)))
    assert e.value.code == L.MI_ERR_BAD_ARG and "1025" in str(e.value) and "1024" in str(e.value)
    # the bound plan and A_ΓΓ operator
    lib = L.load()
    assert lib.mi_schur_setup_destroy(setup._h) == L.MI_ERR_BAD_ARG and b"LORASC" in lib.mi_last_error()
    assert lib.mi_op_destroy(gg._h) == L.MI_ERR_BAD_ARG and b"LORASC" in lib.mi_last_error()
    assert lib.mi_schur_setup_keep_levels(setup._h, 0) == L.MI_ERR_BAD_ARG
    assert np.array_equal(M.ldiv(x), z)
    M.close()                                             # released: both can go now
    assert lib.mi_schur_setup_destroy(setup._h) == 0 and lib.mi_op_destroy(gg._h) == 0
    setup._h = gg._h = None


def test_example03_lorasc_leg(orc, fem, cases):
    """examples/example03_domain_decomposition.py --lorasc at N = 40: exit 0 and the printed `it` equals the oracle's"""
    c = cases["micro"]
    E, _ = fem.prepare_lorasc_precond(lr.dense_schur(c), c.A_ΓΓ)       # the example's defaults: nvec = 25, ε = 0.01
    want = orc.pcg(orc.csc_operator(c.A), c.b, np.zeros(c.n), _oracle_M(orc, c, E))
    cmd = [sys.executable, os.path.join(ROOT, "examples", "example03_domain_decomposition.py"), "--N", "40", "--lorasc"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"lorasc-pcg: n = (\d+), ndom = 4, iter = (\d+)", r.stdout)
    assert m, r.stdout[-2000:]
    assert int(m.group(1)) == c.n and int(m.group(2)) == want[1], (m.groups(), want[1])
