"""CPU suite of the SpMV row-block partition (csrc/spmv_blocks.hpp, compiled for the host by
tests/cpp/spmv_blocks_check.cpp) on the synthetic matrices of tests/sparse_synth.py: the invariants every kernel relies
on, and for every case the property it is named for, so that tests/test_gpu_sparse_edges.py reaches the branches it
was written to reach. Also the CPU-side facts that suite's bars rest on: oracle iteration counts <= 20 for the solver
cases, exactly 8 for `capped`, and the oracle's interior CG within 1.1 κ_d reltol of a SuperLU solve."""
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from conftest import ROOT
import sparse_synth as ss

TILE, NT = ss.SPMV_TILE, ss.NT


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spmv") / "spmv_blocks_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "spmv_blocks_check.cpp")])
    return exe


@pytest.fixture(scope="module")
def mats():
    return ss.apply_cases()


@pytest.fixture(scope="module")
def isets():
    return ss.interior_sets()


@pytest.fixture(scope="module")
def parts(checker, mats, isets, tmp_path_factory):
    """name -> (indptr, breaks, blocks [nb, 4], xcd_row [9]) from one run of the driver over every case"""
    tmp = tmp_path_factory.mktemp("rowptr")
    inputs = {name: (A.indptr, np.zeros(0, dtype=np.int64)) for name, A in mats.items()}
    for name, s in isets.items():
        inputs["icg_" + name] = (s.stacked().indptr, s.breaks)
    files = []
    for name, (indptr, breaks) in inputs.items():
        fn = str(tmp / f"{name}.bin")
        ss.write_rowptr(fn, indptr, breaks)
        files.append(fn)
    out = subprocess.run([checker] + files, capture_output=True, text=True, check=True)
    lines = out.stdout.splitlines()
    assert len(lines) == len(inputs)
    res = {}
    for (name, (indptr, breaks)), line in zip(inputs.items(), lines):
        r = json.loads(line)
        assert r["tile"] == TILE and r["n"] == indptr.size - 1
        res[name] = (np.asarray(indptr), np.asarray(breaks), np.array(r["blocks"], dtype=np.int64).reshape(-1, 4),
                     np.array(r["xcd_row"], dtype=np.int64))
    return res


def test_partition_invariants(parts):
    for name, (indptr, breaks, blk, xr) in parts.items():
        n = indptr.size - 1
        r0, r1, k0, k1 = blk.T
        if n == 0:
            assert blk.shape[0] == 0 and np.all(xr == 0), name
            continue
        # rows [0, n) exactly once, in order; the give-back rule never empties a block
        assert r0[0] == 0 and r1[-1] == n and np.array_equal(r0[1:], r1[:-1]), name
        assert np.all(r1 > r0), name
        # k0 / k1 are the row pointers
        assert np.array_equal(k0, indptr[r0]) and np.array_equal(k1, indptr[r1]), name
        # at most SPMV_TILE non-zeros, or a single row
        assert np.all((k1 - k0 <= TILE) | (r1 - r0 == 1)), name
        # no block crosses a break
        for b in breaks:
            assert not np.any((r0 < b) & (r1 > b)), (name, b)
        # xcd_row: the first row of block x * per, n for an XCD without blocks; non-decreasing, ends at n
        nb = blk.shape[0]
        per = (nb + 7) // 8
        assert xr.size == 9 and xr[8] == n and np.all(np.diff(xr) >= 0), name
        for x in range(8):
            assert xr[x] == (r0[x * per] if x * per < nb else n), (name, x)
        # greedy up to the give-back of at most three rows: a block that ends before the next break (or n) could not have
        # taken four more rows
        for b in range(nb):
            later = breaks[breaks > r0[b]]
            lim = min(n, later.min()) if later.size else n
            if r1[b] < lim:
                assert indptr[min(r1[b] + 4, lim)] - k0[b] > TILE, (name, b)


def rows(blk):
    return blk[:, 1] - blk[:, 0]


def nnz(blk):
    return blk[:, 3] - blk[:, 2]


def test_cases_have_the_property_they_are_named_for(parts, mats):
    P = {k: v[2] for k, v in parts.items()}
    X = {k: v[3] for k, v in parts.items()}
    # diag: 1024 rows per block -> four row passes of NT threads (i >= 2 reload in k_spmv_csr, i > 0 in the solvers' SpMV)
    assert P["diag1"].shape[0] == 1
    assert P["diag1023"].shape[0] == 1 and rows(P["diag1023"])[0] == 1023 and nnz(P["diag1023"])[0] % 2 == 1   # paired path, odd tail
    assert P["diag1024"].shape[0] == 1 and rows(P["diag1024"])[0] == 1024
    assert P["diag1025"].shape[0] == 2 and rows(P["diag1025"])[1] == 1
    assert rows(P["diag5000"]).max() > 2 * NT
    # n = 8193: 9 blocks, per = 2, XCDs 5..7 without blocks -> xcd_row == n there; above FUSED_MAX_N
    assert P["diag8193"].shape[0] == 9 and 8193 > ss.FUSED_MAX_N
    assert np.all(X["diag8193"][5:] == 8193) and X["diag8193"][4] < 8193
    # 17 blocks, per = 3: XCD 5 holds two blocks (one of them the 1-row block), XCDs 6 and 7 none
    assert P["diag16385"].shape[0] == 17 and X["diag16385"][5] < 16385 and np.all(X["diag16385"][6:] == 16385)
    # tridiag: > NT rows per block (second row pass), odd block ends so that the give-back rule fires (a block with fewer
    # non-zeros than the greedy 1022..1024) and every block starts at an even offset
    for name in ("tridiag3000", "tridiag9001", "tridiag800000"):
        b = P[name]
        assert rows(b).max() > NT and rows(b).max() <= 2 * NT, name
        assert np.all(b[:, 2] % 2 == 0), name
        assert np.any(nnz(b)[:-1] < TILE - 2), name                 # rows were given back
    assert 9 < P["tridiag9001"].shape[0] and 9001 > ss.FUSED_MAX_N
    # tridiag(800000): more than 8 * NT = 2048 blocks (partials loop of k_update_xr_blk) and more than 4 * NT = 1024 rows
    # in each of the 32 slices of an XCD's rows (row loop of k_update_xr_blk)
    assert P["tridiag800000"].shape[0] > 8 * NT
    assert np.diff(X["tridiag800000"]).min() > 32 * 4 * NT
    # arrow(5000, m): row 0 alone in its block; fits the tile up to m = 1024, the long-row branch from 1025 on
    for m in (1023, 1024, 1025, 2048, 2049):
        b = P[f"arrow5000_{m}"]
        assert rows(b)[0] == 1 and nnz(b)[0] == m, m
    assert nnz(P["arrow9000_9000"])[0] == 9000 and P["arrow9000_9000"].shape[0] > 9
    assert any(nnz(P[f"arrow5000_{m}"])[0] == TILE + 1 for m in (1025,))       # a single-row block of exactly 1025 non-zeros
    # odd_start: a block with odd k0 whose non-zeros fill the tile exactly; then odd k0 with more than NT rows
    b = P["odd_start"]
    assert tuple(b[0]) == (0, 1, 0, 1) and tuple(b[1]) == (1, 2, 1, 1 + TILE)
    assert b[2, 2] % 2 == 1 and rows(b)[2] > NT
    # holes: empty rows first and last, and a block holding the run of more than SPMV_TILE empty rows
    A = mats["holes"]
    rl = np.diff(A.indptr)
    assert np.all(rl[:ss.HOLES_LEAD] == 0) and np.all(rl[-ss.HOLES_TRAIL:] == 0) and rl[ss.HOLES_LEAD] > 0
    assert rows(P["holes"]).max() > ss.HOLES_INNER > TILE
    assert (abs(A - A.T)).nnz == 0
    # interior sets
    b = P["icg_mixed"]
    assert rows(b).max() > NT and rows(b).min() == 1                # row passes i > 0 of k_icg_spmv; the 1 x 1 subdomain
    assert b.shape[0] > 9 + 3                                       # several blocks per XCD, subdomains of 1, 1, 1, many blocks
    b = P["icg_longrow"]
    assert rows(b)[0] == 1 and nnz(b)[0] == 3000
    assert P["icg_capped"].shape[0] == 1
    # wide: more than NT pieces of max(NT, ceil(n / 512)) rows -> the two-launch form must fall back
    n = 300000
    rows_per = max(NT, -(-n // 512))
    xr = X["icg_wide"]
    pieces = sum(-(-(xr[x + 1] - xr[x]) // rows_per) for x in range(8) if xr[x + 1] > xr[x])
    assert pieces > NT


def test_all_matrices_are_symmetric_and_spd_where_solved(mats, isets):
    for name, A in mats.items():
        assert (abs(A - A.T)).nnz == 0, name
    for name in ss.SOLVER_CASES:
        A = mats[name]
        d = A.diagonal()
        R = np.asarray(abs(A).sum(axis=1)).ravel() - d
        assert np.all(d > R), name                                  # strictly diagonally dominant with a positive diagonal
    for s in isets.values():
        for A, kap in zip(s.A_II, s.kappa):
            if A.shape[0] and A.shape[0] <= 300:
                w = np.linalg.eigvalsh(A.toarray())
                assert w[0] > 0 and w[-1] / w[0] <= kap * (1 + 1e-9)
            elif A.shape[0]:
                assert ss.gershgorin_kappa(A) <= kap * (1 + 1e-12)


def test_oracle_iteration_counts_of_the_solver_cases(orc, mats):
    """every sparse solve of the GPU suite stays in the tight branch of assert_history: oracle `it` <= 20"""
    for name in ss.SOLVER_CASES:
        A = mats[name]
        n = A.shape[0]
        Ao = orc.csc_operator(A)
        b = ss.solver_rhs(n)
        for x0 in (np.zeros(n), ss.solver_rhs(n, 1)):
            its = (orc.cg(Ao, b, x0)[1], orc.pcg(Ao, b, x0, orc.jacobi_operator(A.diagonal()))[1],
                   orc.pcg(Ao, b, x0, orc.identity_operator(n))[1])
            print(name, "oracle it (cg, jacobi, identity):", its)
            assert max(its) <= 20, (name, its)
            assert its[0] > 2 and its[2] > 2, (name, its)            # maxit 1, 2 cut cg and pcg(I) short (Jacobi on diag: it = 2)


def test_oracle_interior_cg_on_the_sets(orc, isets):
    """`capped` stops on maxiter = n_i = 8 exactly; the oracle's interior CG alone is within 1.1 κ_d reltol of SuperLU (the
    GPU suite's bar is 2 κ_d reltol); subdomains of `mixed` converge at different iterations"""
    its = {}
    for name, s in isets.items():
        for d, (A, b, kap) in enumerate(zip(s.A_II, s.b_I, s.kappa)):
            if A.shape[0] == 0:
                continue
            x, it = orc.interior_cg(A, b, s.reltol)
            its[(name, d)] = it
            if not b.any():
                assert it == 0 and not x.any()
                continue
            want = spla.splu(sp.csc_matrix(A)).solve(b)
            err = np.linalg.norm(x - want) / np.linalg.norm(want)
            print(f"{name}[{d}] n_i={A.shape[0]} it={it} err/(kappa*reltol)={err / (kap * s.reltol):.3g}")
            assert err <= 1.1 * kap * s.reltol, (name, d, err)
    assert its[("capped", 0)] == 8
    assert its[("mixed", 0)] == 1 and its[("mixed", 2)] <= 12 < its[("mixed", 3)]
