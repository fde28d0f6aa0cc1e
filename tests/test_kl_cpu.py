"""CPU suite: the host side of the Karhunen-Loève layer (fem.py, io.py) and the pure host function mi_cov_tiling against
tests/kl_ref.py, the numpy restatement of Fem/KarhunenLoeve.jl and Fem/KarhunenLoeveDomainDecomposition.jl ("KLDD.jl").

The identity everything on the device rests on: the reference's two element loops build R = M K and C = R M, so C = M K M
(M the consistent P1 mass matrix, K the nodal covariance). It is checked here on a 5 x 5-node mesh, for the global matrix and
for one rectangular (idom, jdom) block, to 1e-14 max|C|: both sides sum O(10) terms of equal sign per entry."""
import ctypes as C

import numpy as np
import pytest

import kl_ref as ref


def test_the_two_element_loops_are_M_K_M(fem):
    mesh = fem.get_mesh(5)
    cells, points = mesh.cells, mesh.points
    for model in ("SExp", "Exp"):
        cov = ref.cov_scalar(model, 1.3, 0.4)
        nodes, elems = np.arange(25), np.arange(cells.shape[1])
        Cl = ref.loops_C(cells, points, cov, nodes, elems, nodes, elems)
        M = ref.dense_mass(cells, points)
        Cm = M @ ref.dense_K(model, 1.3, 0.4, points, points) @ M
        print(f"  {model}: max|C_loops - M K M| / max|C| = {np.abs(Cl - Cm).max() / np.abs(Cm).max():.2e}")
        assert np.abs(Cl - Cm).max() <= 1e-14 * np.abs(Cm).max()


def test_a_rectangular_block_is_Mi_K_Mj(fem):
    mesh = fem.get_mesh(5)
    cells, points = mesh.cells, mesh.points
    epart, _ = fem.mesh_partition(mesh, 2, 2)
    ni, ei, _ = ref.set_subdomain(cells, points, epart, 0)
    nj, ej, _ = ref.set_subdomain(cells, points, epart, 3)
    cov = ref.cov_scalar("SExp", 1.0, 0.5)
    Cl = ref.loops_C(cells, points, cov, ni, ei, nj, ej)
    Mi, Mj = ref.dense_mass(cells, points, ni, ei), ref.dense_mass(cells, points, nj, ej)
    Cm = Mi @ ref.dense_K("SExp", 1.0, 0.5, points[:, ni], points[:, nj]) @ Mj
    assert Cl.shape == (ni.size, nj.size) and ni.size != 25
    assert np.abs(Cl - Cm).max() <= 1e-14 * np.abs(Cm).max()


def test_mass_matrices(fem):
    mesh = fem.get_mesh(7)
    cells, points = mesh.cells, mesh.points
    M = fem.get_mass_matrix(cells, points)
    assert abs(M - M.T).max() == 0
    assert np.abs(M.toarray() - ref.dense_mass(cells, points)).max() <= 1e-17
    lumped = np.zeros(points.shape[1])
    np.add.at(lumped, cells.ravel(), np.tile(ref.areas(cells, points) / 3, 3))
    assert np.abs(np.asarray(M.sum(axis=1)).ravel() - lumped).max() <= 1e-16       # row sums = lumped areas
    assert abs(M.sum() - 1.0) <= 1e-14
    epart, _ = fem.mesh_partition(mesh, 3, 2)
    for idom in (0, 4):
        l2g, g2l, elems, center = fem.kl_set_subdomain(cells, points, epart, idom)
        rl2g, relems, rcenter = ref.set_subdomain(cells, points, epart, idom)
        assert np.array_equal(l2g, rl2g) and np.array_equal(elems, relems) and np.allclose(center, rcenter, rtol=0, atol=1e-15)
        assert np.array_equal(g2l[l2g], np.arange(l2g.size)) and (g2l >= 0).sum() == l2g.size
        Md = fem.do_local_mass_assembly(cells, points, g2l, elems)
        assert np.abs(Md.toarray() - ref.dense_mass(cells, points, rl2g, relems)).max() <= 1e-17


def test_truncation_on_400_nodes(fem):
    """get_mesh(20), L = 0.3, σ² = 1: λ_1..4 = 0.2117, 0.1381, 0.1375, 0.0897; relative = 0.5 keeps 4 of 8 (0.487 before the
    fourth, 0.577 after), relative = 0.99 keeps all 8."""
    mesh, M, K, Cd, lam, V = ref.problem400(fem)
    print(f"  λ_1..8 = {lam[:8]}")
    assert np.allclose(lam[:4], [0.2117, 0.1381, 0.1375, 0.0897], rtol=0, atol=5e-5)
    Area, cen = fem.kl_energy(mesh.cells, mesh.points)
    rArea, rcen = ref.energy(mesh.cells, mesh.points)
    assert abs(Area - rArea) <= 1e-14 and np.allclose(cen, rcen, rtol=0, atol=1e-14) and abs(Area - 1.0) <= 1e-14
    cc = float(fem.cov("SExp", cen[0], cen[1], cen[0], cen[1], ref.SIG2, ref.L_GLOBAL))
    assert cc == ref.SIG2
    nvec, achieved = fem.kl_keep(lam[:8], 0.5 * Area * cc)
    rn, cum = ref.keep(lam[:8], 0.5 * Area * cc)
    assert nvec == rn == 4 and abs(cum[2] - 0.487) < 1e-3 and abs(cum[3] - 0.577) < 1e-3 and achieved == cum[3]
    assert fem.kl_keep(lam[:8], 0.99 * Area * cc)[0] == 8
    assert fem.kl_keep(np.array([0.3, 0.1, -1e-18, 0.2]), 10.0)[0] == 2          # stops at the first value that is not positive


def test_trim_and_order_and_project_on_mesh(fem):
    Λ = np.array([-2e-17, -1e-18, 0.5, 1.5, 3.0])
    Φ = np.arange(15.0).reshape(3, 5)
    Λt, Φt = fem.trim_and_order(Λ, Φ)
    assert np.array_equal(Λt, [3.0, 1.5, 0.5]) and np.array_equal(Φt, Φ[:, [4, 3, 2]])
    # two subdomains on 5 nodes sharing nodes 2 and 3; 2 + 1 local modes, 2 reduced modes
    l2g = [np.array([3, 0, 2]), np.array([2, 4, 3, 1])]
    Φd = [np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]), np.array([[7.0], [8.0], [9.0], [10.0]])]
    Φr = np.array([[1.0, -1.0], [0.5, 2.0], [2.0, 0.25]])
    Ψ = fem.project_on_mesh(5, Φr, None, l2g, Φd)
    assert np.array_equal(Ψ, ref.project_on_mesh(5, Φr, l2g, Φd))
    assert Ψ[0, 0] == 3.0 * 1.0 + 4.0 * 0.5                                      # node 0: subdomain 0 only
    assert Ψ[2, 0] == ((5.0 * 1.0 + 6.0 * 0.5) + 7.0 * 2.0) / 2                  # node 2: both, divided by cnt = 2
    assert Ψ[1, 1] == 10.0 * 0.25
    K = np.diag([2.0, 1.0, 0.5]); K[0, 1] = 0.1; K[1, 0] = 99.0                  # only the upper triangle is read
    Λg, Ψg = fem.solve_global_reduced_kl(5, K, 3.0, None, l2g, Φd, relative=0.8, verbose=False)
    w = np.linalg.eigvalsh(np.array([[2.0, 0.1, 0], [0.1, 1.0, 0], [0, 0, 0.5]]))[::-1]
    assert Λg.size == 2 and np.allclose(Λg, w[:2], rtol=0, atol=1e-15) and Ψg.shape == (5, 2)   # 2.01 + 0.99 >= 0.8 * 3
    assert fem.suggest_parameters(100_000) == (.9986, .995) and fem.suggest_parameters(100_001) == (.9993, .995)


def test_cov_tiling_invariants(pkg):
    """mi_cov_tiling through ctypes, no device: splits >= 1, splits = 1 when the rows alone fill the grid, at most one split
    per source chunk, the same answer for the same sizes."""
    L = pkg._lib.load()
    out = [C.c_int64() for _ in range(4)]

    def tiling(nt, ns, m):
        assert L.mi_cov_tiling(C.c_int64(nt), C.c_int64(ns), C.c_int64(m), *[C.byref(o) for o in out]) == 0
        return tuple(o.value for o in out)
    rt, sc, cb, _ = tiling(1, 1, 1)
    assert rt >= 64 and sc >= 1 and cb >= 1
    for nt, ns, m in [(1, 1, 1), (1000, 1000, 1), (1000, 1000, cb), (rt - 1, 2 * sc + 3, cb + 1), (rt * 256, 40000, 1),
                      (rt * 256 - 1, 40000, 1), (40000, 40000, 1), (7, 10 ** 6, 3), (1, sc, 1), (1, sc + 1, 1)]:
        a, b = tiling(nt, ns, m), tiling(nt, ns, m)
        assert a == b and a[:3] == (rt, sc, cb)
        chunks = -(-ns // sc)
        assert 1 <= a[3] <= chunks, (nt, ns, m, a)
    assert tiling(rt * 256, 40000, 1)[3] == 1                    # 256 row tiles: one per CU
    assert tiling(10 ** 6, 10 ** 6, 1)[3] == 1
    assert tiling(1000, 1000, 1)[3] > 1 and tiling(1, sc, 1)[3] == 1 and tiling(1, sc + 1, 1)[3] == 2
    BAD = pkg._lib.MI_ERR_BAD_ARG
    for bad in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (-3, 5, 1)]:
        assert L.mi_cov_tiling(*[C.c_int64(v) for v in bad], None, None, None, None) == BAD
        assert L.mi_last_error().decode().startswith("mi_cov_tiling")
    assert L.mi_cov_tiling(C.c_int64(5), C.c_int64(5), C.c_int64(5), None, None, None, None) == 0      # any output may be NULL
    assert pkg.api.cov_tiling(1000, 1000, 1) == tiling(1000, 1000, 1)


def test_file_names_and_npz_round_trips(pkg, tmp_path):
    io = pkg.io
    assert io.get_root_filename("SExp", 1.0, 0.1, 4000) == "SExp_sig21.0_L0.1_DoF4000"       # Example02:28 with its values
    assert io.get_root_filename("Exp", 2.5, 0.05, 100000) == "Exp_sig22.5_L0.05_DoF100000"
    assert io.get_root_filename("SExp", 1, 10.0, 8000) == "SExp_sig21.0_L10.0_DoF8000"
    rng = np.random.default_rng(3)
    Λ, Ψ = rng.random(5), rng.standard_normal((12, 5))
    root = io.get_root_filename("SExp", 1.0, 0.1, 12)
    pv, pe = io.save_kl(Λ, Ψ, root, str(tmp_path))
    assert pv.endswith("SExp_sig21.0_L0.1_DoF12.kl-eigvals.npz") and pe.endswith(".kl-eigvecs.npz")
    assert np.load(pv).shape == (5,) and np.load(pe).shape == (12, 5) and np.isfortran(np.load(pe))   # NPZ.jl writes NPY, column-major
    Λ2, Ψ2 = io.load_kl(root, str(tmp_path))
    assert np.array_equal(Λ2, Λ) and np.array_equal(Ψ2, Ψ)
    kl = pkg.fem.SyntheticKL(Λ2, Ψ2)
    ξ, g = pkg.fem.draw(kl, np.random.default_rng(11))
    assert np.allclose(g, ref.draw(Λ, Ψ, ξ), rtol=0, atol=1e-14)
    assert np.array_equal(np.load(io.save_greal(g, root, str(tmp_path))), g)
