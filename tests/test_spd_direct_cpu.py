"""CPU suite of the sparse direct preconditioner (`M \\ r` with M = A_ΓΓ, Example07:412/416): the symbolic phase
(csrc/spd_direct_plan.hpp, compiled for the host by tests/cpp/spd_direct_check.cpp) on chains, a star, a disconnected
pair, a grid and the A_ΓΓ of FEM problems; the three-formula solve on its split against SuperLU; and the fem gather map
Σ_d R_d' A_ΓΓdd R_d against `prepare_global_schur`."""
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from conftest import ROOT, f_m1, lognormal_coeff, one, u0734, unstructured_mesh
import spd_graphs as sg

SIGMA_MAX = 2048


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spd") / "spd_direct_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "spd_direct_check.cpp")])
    return exe


def fem_problem(fem, name):
    """(mesh, epart, sub, coeff) of the `ragged` fixture (3x2 boxes, lognormal) or the 6-slice unstructured mesh"""
    if name == "ragged":
        mesh = fem.get_mesh(50)
        epart, npart = fem.mesh_partition(mesh, 3, 2)
        coeff = lognormal_coeff(fem, mesh.points, 7)
    else:
        mesh, epart, npart = unstructured_mesh(fem)
        coeff = one
    d = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
    sub = fem.set_subdomains(mesh.cells, mesh.cell_neighbors, epart, npart, d.dirichlet_g2l)
    return mesh, epart, sub, coeff


@pytest.fixture(scope="module")
def cases(fem):
    out = sg.synthetic_cases()
    for name in ("ragged", "unstructured"):
        mesh, epart, sub, coeff = fem_problem(fem, name)
        out[name] = sg.global_gg(fem, mesh, epart, sub, coeff, f_m1, u0734)
    return out


def run_checker(exe, tmp_path, mats, P=64, sigma_max=SIGMA_MAX):
    files = []
    for name, A in mats.items():
        fn = str(tmp_path / f"{name}.txt")
        sg.write_graph(fn, A)
        files.append(fn)
    out = subprocess.run([exe, str(P), str(sigma_max)] + files, capture_output=True, text=True)
    res = [json.loads(line) for line in out.stdout.splitlines()]
    assert len(res) == len(mats), out.stderr
    return out.returncode, dict(zip(mats, res))


@pytest.mark.parametrize("P", [32, 64, 128])
def test_split_is_a_valid_dissection(checker, tmp_path, cases, P):
    """every node in one piece or Σ, no edge between pieces, pieces <= P nodes, Σ_i / slots / destinations consistent,
    two runs identical"""
    rc, res = run_checker(checker, tmp_path, cases, P)
    for name, r in res.items():
        assert r["ok"] and r["status"] == 0, (name, r["why"])
    assert rc == 0
    # the shapes the design relies on (P = 64): a chain of <= P nodes is one piece; a chain splits at single nodes
    if P == 64:
        assert (res["chain1"]["pieces"], res["chain1"]["sigma"]) == (1, 0)
        assert (res["chain64"]["pieces"], res["chain64"]["sigma"]) == (1, 0)
        assert res["chain65"]["sigma"] == 1 and res["chain1000"]["sigma"] <= 1000 // 64 + 1
        assert res["star"]["sigma"] == 1                          # the hub
        for name in ("ragged", "unstructured"):
            assert res[name]["sigma"] < 0.2 * cases[name].shape[0], (name, res[name]["sigma"])


def test_split_solves_exactly(checker, tmp_path, cases):
    """the three formulas on the split give A \\ r (SuperLU) to 1e-12"""
    _, res = run_checker(checker, tmp_path, cases)
    rng = np.random.default_rng(0)
    for name, A in cases.items():
        r = rng.standard_normal(A.shape[0])
        z = sg.dissection_solve(A, res[name]["piece_of"], r)
        want = spla.splu(sp.csc_matrix(A)).solve(r)
        assert np.linalg.norm(z - want) <= 1e-12 * np.linalg.norm(want), name


def test_separator_limit_is_reported(checker, tmp_path):
    """a graph without a small separator: status SIGMA_TOO_LARGE (the library turns it into MI_ERR_BAD_ARG), no layout"""
    mats = {"dense": sg.spd_from_graph(sg.random_dense_graph(6000, 12), 1)}
    rc, res = run_checker(checker, tmp_path, mats)
    assert res["dense"]["status"] == 2 and res["dense"]["sigma"] > SIGMA_MAX and res["dense"]["ok"]
    rc, res = run_checker(checker, tmp_path, {"chain": sg.spd_from_graph(sg.chain(1000))}, sigma_max=5)
    assert res["chain"]["status"] == 2


def test_bad_patterns_are_refused(checker, tmp_path):
    A = sp.csc_matrix(np.array([[2.0, 1.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 2.0]]))
    rc, res = run_checker(checker, tmp_path, {"nonsym": A})
    assert res["nonsym"]["status"] == 1 and "symmetric" in res["nonsym"]["why"] and rc != 0


@pytest.mark.parametrize("name", ["micro", "ragged", "unstructured"])
def test_gamma_gather_map_matches_global_assembly(fem, orc, name):
    """Σ_d R_d' A_ΓΓdd R_d through fem.gamma_gather_map == prepare_global_schur's A_ΓΓ (same pattern, values to 1e-15)"""
    if name == "micro":
        mesh = fem.get_mesh(40)
        epart, npart = fem.mesh_partition(mesh, 2, 2)
        d = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
        sub = fem.set_subdomains(mesh.cells, mesh.cell_neighbors, epart, npart, d.dirichlet_g2l)
        coeff = one
    else:
        mesh, epart, sub, coeff = fem_problem(fem, name)
    want = sg.global_gg(fem, mesh, epart, sub, coeff, f_m1, u0734)
    A_ΓΓdd = fem.prepare_local_schurs(mesh.cells, mesh.points, epart, sub, coeff, f_m1, u0734)[2]
    gm = fem.gamma_gather_map(A_ΓΓdd, sub.gather_idx, sub.n_Γ)
    flat = np.concatenate([sp.csr_matrix(m).data for m in A_ΓΓdd])
    got = gm.matrix(flat)
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert np.abs(got.data - want.data).max() <= 1e-15 * np.abs(want.data).max()
    # the same map read straight from the output of an assembly plan (what the device set-up path feeds it)
    plan = fem.make_assembly_plan(mesh.cells, mesh.points, epart, sub, f_m1, u0734)
    a = coeff(mesh.points[0], mesh.points[1]) if callable(coeff) else coeff
    vals = orc.run_assembly_plan(plan, a)
    gm2 = fem.gamma_gather_map(plan.patterns["ΓΓ"], sub.gather_idx, sub.n_Γ, offsets=[o for o, _ in plan.layout["ΓΓ"]])
    assert np.array_equal(gm2.indptr, gm.indptr) and np.array_equal(gm2.indices, gm.indices)
    assert np.abs(gm2.values(vals) - want.data).max() <= 1e-15 * np.abs(want.data).max()


def test_save_pcg_iters_A_GG_names(pkg, tmp_path):
    """Example07:423-424 file names with precond="A_GG"; the default keeps the Neumann-Neumann names (Example07:284-285)"""
    io = pkg.io
    p = io.save_pcg_iters([30, 31], "DoF576", 4, "t", 2, str(tmp_path), precond="A_GG")
    assert os.path.basename(p) == "DoF576.A_GG_ndom4_t.pcg-iters.nreals2.npz" and os.path.exists(p)
    assert os.path.basename(io.save_pcg_iters([3], "DoF576", 4, "0", 1, str(tmp_path))) == \
        "DoF576.neumann-neumann_ndom4_0.pcg-iters.nreals1.npz"
