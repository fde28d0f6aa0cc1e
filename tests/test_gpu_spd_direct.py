"""GPU suite of the sparse direct preconditioner `api.SparseDirectPreconditioner` (`mi_spd_direct_*`): `M \\ r` with a
sparse SPD M, the `pcg(S, b_schur, zeros(S.N), A_ΓΓ)` of Example07:412/416. Applies against SuperLU, the errors, solves
against the oracle (`M` = neumann_neumann_operator([inv(A_ΓΓ)], [0:n_Γ], 1), which is exactly A_ΓΓ \\ r) under the rules
of test_gpu_parity.assert_history, other solvers, graph replay, and the example's second loop."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from conftest import ROOT, f_m1, lognormal_coeff, one, u0734, unstructured_mesh
from test_gpu_parity import assert_history, gpu_ops, orc_ops
import spd_graphs as sg

pytestmark = pytest.mark.gpu


def _fem_cases(fem):
    out = {}
    mesh = fem.get_mesh(50)
    epart, npart = fem.mesh_partition(mesh, 3, 2)
    d = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
    sub = fem.set_subdomains(mesh.cells, mesh.cell_neighbors, epart, npart, d.dirichlet_g2l)
    out["ragged"] = sg.global_gg(fem, mesh, epart, sub, lognormal_coeff(fem, mesh.points, 7), f_m1, u0734)
    mesh, epart, npart = unstructured_mesh(fem)
    d = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
    sub = fem.set_subdomains(mesh.cells, mesh.cell_neighbors, epart, npart, d.dirichlet_g2l)
    out["unstructured"] = sg.global_gg(fem, mesh, epart, sub, one, f_m1, u0734)
    return out


@pytest.fixture(scope="module")
def cases(fem):
    out = sg.synthetic_cases()
    out.update(_fem_cases(fem))
    return out


def _one_based(A):
    A = sp.csc_matrix(A)
    return (A.indptr + 1, A.indices + 1, A.data, A.shape[0])


def test_apply_against_splu(pkg, ctx, cases):
    """z = M \\ r against SuperLU at 1e-12 for index_base 0 and 1, host and device pointers; two applies bit-identical"""
    import torch
    api = pkg.api
    rng = np.random.default_rng(1)
    for name, A in cases.items():
        r = rng.standard_normal(A.shape[0])
        want = spla.splu(sp.csc_matrix(A)).solve(r)
        for base in (0, 1):
            M = api.SparseDirectPreconditioner(ctx, A if base == 0 else _one_based(A), index_base=base)
            z = M.ldiv(r)
            assert np.linalg.norm(z - want) <= 1e-12 * np.linalg.norm(want), (name, base, M.stats)
            zd = M.ldiv(torch.from_numpy(r).cuda()).cpu().numpy()
            assert np.array_equal(zd, z), (name, base)
            assert np.array_equal(M.ldiv(r), z), (name, base)


def test_set_values_equals_fresh_create(pkg, ctx, cases):
    """new values through set_values (host and device) == a create on them, bit for bit; the pattern is kept"""
    import torch
    api = pkg.api
    rng = np.random.default_rng(2)
    for name in ("chain1000", "grid30", "ragged", "unstructured", "star"):
        A = sp.csc_matrix(cases[name])
        A2 = A.copy()                                   # D A D, D > 0 diagonal: still SPD, same stored pattern
        d = 1.0 + 0.3 * rng.random(A.shape[0])
        A2.data = A.data * d[A.indices] * np.repeat(d, np.diff(A.indptr))
        r = rng.standard_normal(A.shape[0])
        M = api.SparseDirectPreconditioner(ctx, A)
        fresh = api.SparseDirectPreconditioner(ctx, A2).ldiv(r)
        M.set_values(A2.data)
        assert np.array_equal(M.ldiv(r), fresh), name
        M.set_values(torch.from_numpy(A.data).cuda())
        M.set_values(torch.from_numpy(A2.data).cuda())
        assert np.array_equal(M.ldiv(r), fresh), name


def test_errors_do_not_fault(pkg, ctx, cases):
    """an indefinite matrix -> MI_ERR_SINGULAR (piece pivot, or the separator's Schur complement); a failed set_values keeps
    the previous factor; a separator above the limit -> MI_ERR_BAD_ARG naming both numbers; a non-symmetric pattern -> BAD_ARG"""
    api, L = pkg.api, pkg._lib
    A = sp.csc_matrix(cases["chain1000"]).copy()
    A.setdiag(A.diagonal() * np.where(np.arange(1000) == 500, -1.0, 1.0))
    with pytest.raises(api.SingularException):
        api.SparseDirectPreconditioner(ctx, A)
    # the hub of a star is the separator: s = a_hh - Σ b^2 / a_ll < 0
    n = 151
    G = sp.csc_matrix(sg.star(150))
    hub = sp.csc_matrix(-G + sp.diags(np.r_[1.0, np.full(150, 1.0)]))
    with pytest.raises(api.SingularException):
        api.SparseDirectPreconditioner(ctx, hub)
    good = sp.csc_matrix(-G + sp.diags(np.r_[200.0, np.full(150, 1.5)]))
    good.sort_indices()
    M = api.SparseDirectPreconditioner(ctx, good)
    assert M.stats == (M.stats[0], 1)
    r = np.random.default_rng(3).standard_normal(n)
    z = M.ldiv(r)
    hub.sort_indices()
    with pytest.raises(api.SingularException):
        M.set_values(hub.data)
    assert np.array_equal(M.ldiv(r), z)
    dense = sg.spd_from_graph(sg.random_dense_graph(6000, 12), 1)
    with pytest.raises(api.MiError) as e:
        api.SparseDirectPreconditioner(ctx, dense)
    assert e.value.code == L.MI_ERR_BAD_ARG and "2048" in str(e.value) and "separator has" in str(e.value)
    with pytest.raises(api.MiError) as e:
        api.SparseDirectPreconditioner(ctx, sp.csc_matrix(np.array([[2.0, 1.0], [0.0, 2.0]])))
    assert e.value.code == L.MI_ERR_BAD_ARG
    assert np.array_equal(M.ldiv(r), z)                   # the context is still healthy


def _gg_problem(fem, P, coeff):
    return sg.global_gg(fem, P.mesh, P.epart, P.sub, coeff, f_m1, u0734)


def _run_pcg_case(pkg, ctx, orc, P, A_gg):
    api = pkg.api
    S, _ = gpu_ops(pkg, ctx, P)
    So, _ = orc_ops(orc, P)
    n = P.sub.n_Γ
    M = api.SparseDirectPreconditioner(ctx, A_gg)
    Mo = orc.neumann_neumann_operator([np.asfortranarray(np.linalg.inv(A_gg.toarray()))], [np.arange(n)], np.ones(n, dtype=np.int64))
    x0 = np.zeros(n)
    got = api.pcg(S, P.b_schur, x0, M)
    want = orc.pcg(So, P.b_schur, x0, Mo)
    assert_history(got, want, apply=So, b=P.b_schur)
    return got[1], M


@pytest.mark.parametrize("case,cpu_it", [("micro", 17), ("toy", 29), ("ragged", 28)])
def test_pcg_with_A_GG_against_oracle(pkg, ctx, orc, fem, case, cpu_it, micro, toy, ragged):
    P = {"micro": micro, "toy": toy, "ragged": ragged}[case]
    coeff = lognormal_coeff(fem, P.mesh.points, 7) if case == "ragged" else one
    it, _ = _run_pcg_case(pkg, ctx, orc, P, _gg_problem(fem, P, coeff))
    assert it == cpu_it


def test_pcg_with_A_GG_unstructured(pkg, ctx, orc, fem):
    mesh, epart, npart = unstructured_mesh(fem)
    P = fem.build_schur_problem(mesh.N, 1, 1, one, f_m1, u0734, mesh=mesh, partition=(epart, npart))
    _run_pcg_case(pkg, ctx, orc, P, _gg_problem(fem, P, one))


def test_other_solvers_and_graph_replay(pkg, ctx, orc, fem, ragged):
    """defpcg and eigpcg with this M against the oracle; a chunked (graph-replayed) pcg == an eager one, bit for bit"""
    api = pkg.api
    P = ragged
    A = _gg_problem(fem, P, lognormal_coeff(fem, P.mesh.points, 7))
    S, _ = gpu_ops(pkg, ctx, P)
    So, _ = orc_ops(orc, P)
    n = P.sub.n_Γ
    M = api.SparseDirectPreconditioner(ctx, A)
    Mo = orc.neumann_neumann_operator([np.asfortranarray(np.linalg.inv(A.toarray()))], [np.arange(n)], np.ones(n, dtype=np.int64))
    x0 = np.zeros(n)
    W = np.asfortranarray(np.linalg.qr(np.random.default_rng(4).standard_normal((n, 6)))[0])
    assert_history(api.defpcg(S, P.b_schur, x0, W, M), orc.defpcg(So, P.b_schur, x0, W, Mo), apply=So, b=P.b_schur)
    x, it, res, V = api.eigpcg(S, P.b_schur, x0, M, 4, 12)
    xo, ito, reso = orc.eigpcg(So, P.b_schur, x0, Mo, 4, 12)[:3]
    assert_history((x, it, res), (xo, ito, reso), apply=So, b=P.b_schur)
    ctx.set_chunk(0)
    eager = api.pcg(S, P.b_schur, x0, M)
    ctx.set_chunk(4)
    replay = api.pcg(S, P.b_schur, x0, M)
    ctx.set_chunk(8)
    assert eager[1] == replay[1] and np.array_equal(eager[0], replay[0]) and np.array_equal(eager[2], replay[2])


def test_pcg_with_A_GG_config3(pkg, ctx, orc, fem, full):
    """config 3 (N = 1000, 4x2 boxes, lognormal S): M = A_ΓΓ_0 (a = 1) and M = A_ΓΓ_t (this realization)"""
    P = full
    for coeff in (one, lognormal_coeff(fem, P.mesh.points)):
        _run_pcg_case(pkg, ctx, orc, P, _gg_problem(fem, P, coeff))


def test_pcg_with_A_GG_160_subdomains(pkg, ctx, orc, fem):
    """n_Γ = 9 417: N = 400, 16 x 10 boxes (|Σ| ~ 300)"""
    P = fem.build_schur_problem(400, 16, 10, one, f_m1, u0734)
    it, M = _run_pcg_case(pkg, ctx, orc, P, _gg_problem(fem, P, one))
    assert P.sub.n_Γ == 9417 and M.stats[1] <= 2048


def test_example07_second_loop(tmp_path):
    """examples/example07_stochastic.py --gg: host and device set-up paths give iteration counts within max(1, 2 %)"""
    its = {}
    for tag, extra in (("host", []), ("device", ["--device-assembly", "--device-setup"])):
        out = str(tmp_path / f"{tag}.npz")
        cmd = [sys.executable, os.path.join(ROOT, "examples", "example07_stochastic.py"), "--N", "60", "--px", "3", "--py", "2",
               "--nreals", "3", "--gg", "--out", out] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        z = np.load(out)
        its[tag] = (z["iters_gg0"], z["iters_ggt"])
        assert len(z["iters_gg0"]) == 3 and len(z["iters_ggt"]) == 3 and min(z["iters_ggt"]) > 0
    for a, b in zip(its["host"], its["device"]):
        for x, y in zip(a, b):
            assert abs(int(x) - int(y)) <= max(1, int(0.02 * x)), (its,)
