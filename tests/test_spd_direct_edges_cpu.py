"""CPU suite behind tests/test_gpu_spd_direct_edges.py: every case of spd_graphs.edge_cases() has the shape it is named for
(the host plan checker tests/cpp/spd_direct_check.cpp at the case's piece size), the conditioning family spd_kappa has
the condition numbers it promises, the reference agrees with mpmath, and the numpy copy of the device algorithm
(spd_graphs.dissection_copy) agrees with the reference.

Bar of the copy (the GPU suite's bar): per column ||z - z_ref||_2 / ||z_ref||_2 <= 50 κ_2(A) m eps, m = max(P, |Σ|). The
copy stays below 1e-3 of it everywhere (measured: 5e-4 on the edge cases, 2.3e-5 on the κ ladder); its pivot test passes
and its probe residual stays below 10 % of the certificate's bar (measured: 3.7 %) up to κ = 1e10, so neither has a
reason to refuse these matrices on the device.
The copy of chain4097_P1 is not run: the 2048 Gauss-Jordan steps on a 2048 x 2048 matrix take a minute in numpy."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, f_m1, u0734
import spd_graphs as sg

C = 50.0


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spd_edges") / "spd_direct_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "spd_direct_check.cpp")])
    return exe


@pytest.fixture(scope="module")
def plan_of(checker, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("graphs")
    count = [0]

    def run(A, P):
        count[0] += 1
        fn = str(tmp / f"g{count[0]}.txt")
        sg.write_graph(fn, A)
        out = subprocess.run([checker, str(P), str(sg.SIGMA_MAX), fn], capture_output=True, text=True)
        return json.loads(out.stdout)
    return run


@pytest.fixture(scope="module")
def edges():
    return sg.edge_cases()


@pytest.fixture(scope="module")
def plans(edges, plan_of):
    return {name: plan_of(A, P) for name, (A, P, _) in edges.items()}


def col_err(Z, X):
    """largest relative 2-norm error over the columns"""
    Z, X = np.reshape(Z, (X.shape[0], -1)), np.reshape(X, (X.shape[0], -1))
    if X.size == 0:
        return 0.0
    return float(np.max(np.linalg.norm(Z - X, axis=0) / np.linalg.norm(X, axis=0)))


def test_edge_cases_have_their_shapes(edges, plans):
    for name, (A, P, shape) in edges.items():
        r = plans[name]
        assert r["ok"], (name, r["why"])
        assert r["status"] == shape["status"] and r["sigma"] == shape["sigma"], (name, r["status"], r["sigma"])
        if shape["status"] == 0:
            assert r["pieces"] == shape["pieces"], (name, r["pieces"])
        for key in ("singles", "isolated"):
            if key in shape:
                assert r[key] == shape[key], (name, key, r[key])
        assert r["orphans"] >= shape.get("orphans", 0), name
    # the branch each case is named for
    assert [plans[f"chain{n}_P4"]["sigma"] for n in (356, 360, 364, 365, 512, 516, 517)] == [88, 89, 90, 91, 127, 128, 129]
    assert sg.sd_lds_bytes(88) <= 65536 < sg.sd_lds_bytes(89)              # 88 | 89: the 64 KiB of LDS a kernel has by default
    assert sg.sd_lds_bytes(sg.P_MAX) == 135168 <= 160 * 1024               # P = 128 in k_sd_factor, |Σ| = 128 in k_sd_invert
    assert plans["chain4097_P1"]["sigma"] == sg.SIGMA_MAX and plans["chain4099_P1"]["sigma"] == sg.SIGMA_MAX + 1
    assert plans["spider_P1"]["orphans"] == 1 and plans["spider_P1"]["piece_of"][0] == -1     # the hub
    assert all(plans[n]["orphans"] == 0 for n in plans if n != "spider_P1")
    mixed = plans["chain10_grid9_P64"]
    assert 0 < mixed["isolated"] < mixed["pieces"]                        # pieces both with and without Σ neighbours
    assert plans["three_chains_P64"]["isolated"] == plans["three_chains_P64"]["pieces"] == 3
    # P = 100 and 128: pieces larger than a wave and than the default P; at P = 100 pieces above 64 nodes whose size is no
    # multiple of 64 (the `rr += 64` loop of k_sd_apply1 ends in a partial wave) nor of 4 (its `c += 4` loop ends unevenly)
    for name, P in (("grid16_P128", 128), ("grid16_P100", 100)):
        piece_of = np.asarray(plans[name]["piece_of"])
        sizes = np.bincount(piece_of[piece_of >= 0])
        assert 64 < sizes.max() <= P, (name, sizes)
        if P == 100:
            assert any(sz > 64 and sz % 64 and sz % 4 for sz in sizes), sizes


def test_separator_blocks_are_dense_or_tridiagonal(edges, plans):
    """the chains give a tridiagonal s (index coverage); the strips and grids give an s that is not (the accuracy claims)"""
    for name, (A, P, shape) in edges.items():
        if shape["status"] or shape["sigma"] < 2 or name == "chain4097_P1":
            continue
        info = {}
        sg.dissection_copy(A, plans[name], np.ones(A.shape[0]), info)
        i, j = np.nonzero(info["s"])
        bw = int(np.abs(i - j).max())
        if name.startswith("chain") and "grid" not in name:
            assert bw == 1, (name, bw)
        elif name.startswith(("strip", "grid")):
            assert bw >= 5, (name, bw)
    info = {}
    sg.dissection_copy(edges["grid40_P64"][0], plans["grid40_P64"], np.ones(1600), info)
    assert np.count_nonzero(info["s"]) > 8 * 253                           # dense-ish: far more than a band of a few entries


def test_reference_against_mpmath():
    """SuperLU + long-double refinement against a 50-digit LU of mpmath on a 25 x 25 matrix of κ = 1e8: the reference is
    right to a few κ u_longdouble (~1e-11 here), which is more than 1e5 times below the bar 50 κ m eps of every comparison"""
    import mpmath
    A = sg.spd_kappa(sg.grid(5), 1e8, seed=1, kind="margin")
    n = A.shape[0]
    k = sg.kappa2(A)
    X = sg.reference(A)
    with mpmath.workdps(50):
        Xm = mpmath.inverse(mpmath.matrix(A.toarray().tolist()))
        Xm = np.array([[float(Xm[i, j]) for j in range(n)] for i in range(n)])
    err = col_err(X, Xm)
    print(f"reference vs mpmath: κ = {k:.2e}, largest column error {err:.2e}")
    assert err <= 4 * sg.EPS + 16 * k * np.finfo(np.longdouble).eps
    assert err <= 1e-5 * C * k * sg.EPS


def test_copy_against_reference_on_the_edge_cases(edges, plans):
    worst = 0.0
    for name, (A, P, shape) in edges.items():
        n = A.shape[0]
        if shape["status"] or name == "chain4097_P1":
            continue
        R = sg.rhs_of(n)
        info = {}
        Z = sg.dissection_copy(A, plans[name], R, info)
        assert Z.shape == R.shape
        if n == 0:
            continue
        bar = C * sg.kappa2(A) * max(P, shape["sigma"]) * sg.EPS
        err = col_err(Z, sg.reference(A, R))
        res, cbar = info["certificate"]
        print(f"{name}: copy err / bar = {err / bar:.2e}, certificate residual / bar = {res / cbar if cbar else 0:.2e}")
        assert info["pivots_ok"] and res <= cbar, name
        assert err <= bar, (name, err, bar)
        worst = max(worst, err / bar)
        z1 = sg.dissection_copy(A, plans[name], R[:, 0])                   # a vector gives the first column (to BLAS rounding)
        assert z1.shape == (n,) and np.linalg.norm(z1 - Z[:, 0]) <= 1e-13 * np.linalg.norm(z1), name
    assert worst <= 1e-3                                                   # the docstring's figure


def _ladder_graphs(fem):
    out = dict(sg.LADDER_GRAPHS)
    out["ragged"] = (sg.ragged_gg(fem, f_m1, u0734, contrast=1.0), 64)      # the pattern of the FEM A_ΓΓ
    return out


def test_kappa_family_and_its_copy(fem, plan_of):
    """κ_2 of every member within a factor 3 of its target; the copy within the bar, its pivot test and certificate pass"""
    worst_err, worst_cert = 0.0, 0.0
    for gname, (G, P) in _ladder_graphs(fem).items():
        for kind in ("margin", "scaling"):
            for target in sg.KAPPAS:
                A = sg.spd_kappa(G, target, seed=3, kind=kind)
                k = sg.kappa2(A)
                assert target / 3 <= k <= 3 * target, (gname, kind, target, k)
                pl = plan_of(A, P)
                assert pl["ok"] and pl["status"] == 0
                R = sg.rhs_of(A.shape[0])
                info = {}
                Z = sg.dissection_copy(A, pl, R, info)
                bar = C * k * max(P, pl["sigma"]) * sg.EPS
                err = col_err(Z, sg.reference(A, R))
                res, cbar = info["certificate"]
                assert info["pivots_ok"] and res <= cbar, (gname, kind, target, res, cbar)
                assert err <= bar, (gname, kind, target, err, bar)
                worst_err, worst_cert = max(worst_err, err / bar), max(worst_cert, res / cbar)
    print(f"κ ladder: copy err / bar <= {worst_err:.2e}, certificate residual / bar <= {worst_cert:.2e}")
    assert worst_err <= 1e-3 and worst_cert <= 0.1                         # the docstring's figures


def test_fem_contrast_1e6(fem, plan_of):
    """the `ragged` A_ΓΓ with inclusions of contrast 1e6: SPD, κ far above the synthetic cases', the copy within the bar"""
    A = sg.ragged_gg(fem, f_m1, u0734, contrast=1e6)
    k = sg.kappa2(A)
    pl = plan_of(A, 64)
    assert pl["ok"] and pl["status"] == 0 and pl["sigma"] > 0
    R = sg.rhs_of(A.shape[0])
    info = {}
    Z = sg.dissection_copy(A, pl, R, info)
    bar = C * k * max(64, pl["sigma"]) * sg.EPS
    err = col_err(Z, sg.reference(A, R))
    res, cbar = info["certificate"]
    print(f"ragged, contrast 1e6: n = {A.shape[0]}, |Σ| = {pl['sigma']}, κ = {k:.2e}, copy err / bar = {err / bar:.2e}, "
          f"certificate residual / bar = {res / cbar:.2e}")
    assert 1e4 <= k <= 1e10
    assert info["pivots_ok"] and res <= cbar and err <= bar
