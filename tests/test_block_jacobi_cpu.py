"""CPU suite behind tests/test_gpu_block_jacobi.py (`mi_block_jacobi_*`, csrc/block_jacobi.hpp): the helper's slice rule
against the reference's, the default seed rule's shapes, the noise of the refined reference, a numpy copy of the device's
one-sweep recursion inside the GPU bar on every GPU input (so the bar is attainable), and the oracle's iteration counts
with the dense M^-1 that the GPU solver tests rely on."""
import numpy as np
import pytest
import scipy.sparse as sp

import block_jacobi_ref as bjr
import lorasc_ref as lr
import sparse_synth

APPLY_BAR = 1e-10
GPU_INPUTS = [("micro", 1), ("micro", 2), ("micro", 4), ("micro", 7), ("ragged", 3), ("ragged", 6), ("unstructured", 2),
              ("unstructured", 3), ("tridiag", 1)]
ITERATIONS = {("micro", 1): 2, ("micro", 2): 14, ("micro", 4): 28, ("micro", 7): 38, ("ragged", 3): 34, ("ragged", 6): 44}


@pytest.fixture(scope="module")
def mats(fem):
    cs = lr.gpu_cases(fem, which=("micro", "ragged", "unstructured"))
    out = {k: (sp.csc_matrix(c.A), c.b) for k, c in cs.items()}
    T = sp.csc_matrix(sparse_synth.tridiag(300))
    out["tridiag"] = (T, np.ones(300))
    return out


def test_slices_are_the_reference_s():
    """bsize = n ÷ nb; (i-1) bsize + 1 : i bsize, the last slice to n (BJPreconditioner.jl), here 0-based half-open"""
    s = bjr.slices(1444, 7)
    assert [hi - lo for lo, hi in s] == [206] * 6 + [208] and s[0][0] == 0 and s[-1][1] == 1444
    assert bjr.slices(10, 3) == [(0, 3), (3, 6), (6, 10)]
    assert bjr.slices(7, 7) == [(k, k + 1) for k in range(7)]
    assert bjr.slices(5, 1) == [(0, 5)]
    for n, nb in ((1444, 7), (10, 3), (7, 7), (5, 1)):
        bsize = n // nb                                   # the reference's loop, 1-based inclusive
        want = [((i - 1) * bsize + 1, i * bsize if i < nb else n) for i in range(1, nb + 1)]
        assert [(lo + 1, hi) for lo, hi in bjr.slices(n, nb)] == want


def test_default_seed_shapes(mats):
    """every node is reached (asserted inside shapes), and the shapes on `micro` are those of the issue's table"""
    A = mats["micro"][0]
    assert A.shape[0] == 1444
    assert bjr.shapes(A, 1) == [(1, 37, 75, 1)]
    s4 = bjr.shapes(A, 4)
    assert all(38 <= g <= 39 and lv == 9 for g, lv, w, _ in s4) and max(w for _, _, w, _ in s4) == 39, s4
    for nb in (2, 7):
        sh = bjr.shapes(A, nb)
        assert all(38 <= g <= 39 and w <= 39 for g, lv, w, _ in sh), sh
    su = bjr.shapes(mats["unstructured"][0], 3)
    print("unstructured nb = 3:", su)
    assert mats["unstructured"][0].shape[0] == 676 and all(62 <= nc <= 65 and 208 <= g <= 226 for g, _, _, nc in su), su
    assert bjr.shapes(mats["tridiag"][0], 1) == [(1, 299, 1, 1)]


def test_refined_reference_noise(mats):
    """the refined per-block solve against itself with one more sweep, and its residual in long double: below 1e-12"""
    rng = np.random.default_rng(0)
    for (name, nb) in GPU_INPUTS:
        A = mats[name][0]
        x = rng.standard_normal(A.shape[0])
        y2, y3 = bjr.Ref(A, nb, 2)(x), bjr.Ref(A, nb, 3)(x)
        assert np.linalg.norm(y2 - y3) <= 1e-12 * np.linalg.norm(y3), (name, nb)
        for lo, hi in bjr.slices(A.shape[0], nb):         # normwise backward error of every block, residual in long double
            B = sp.coo_matrix(A[lo:hi, lo:hi])
            res = x[lo:hi].astype(np.longdouble)
            np.subtract.at(res, B.row, B.data.astype(np.longdouble) * y2[lo:hi].astype(np.longdouble)[B.col])
            scale = np.linalg.norm(B.data) * np.linalg.norm(y2[lo:hi]) + np.linalg.norm(x[lo:hi])
            assert float(np.linalg.norm(res.astype(np.float64))) <= 1e-12 * scale, (name, nb, lo)


@pytest.mark.parametrize("name,nb", GPU_INPUTS)
def test_one_sweep_recursion_is_inside_the_gpu_bar(mats, name, nb):
    A = mats[name][0]
    rng = np.random.default_rng(nb)
    ref = bjr.Ref(A, nb, 2)
    for r in (rng.standard_normal(A.shape[0]), np.eye(A.shape[0])[A.shape[0] // 3]):
        want = ref(r)
        err = np.linalg.norm(bjr.sweep(A, nb, r) - want) / np.linalg.norm(want)
        print(f"one-sweep recursion {name} nb = {nb}: rel. error {err:.3e} (bar {APPLY_BAR:.0e})")
        assert err <= APPLY_BAR


@pytest.mark.parametrize("ng,n0", bjr.EDGE_PAIRS)
def test_one_sweep_recursion_is_inside_the_edge_bar(ng, n0):
    """the kernel-edge inputs of the GPU suite: shapes as named, κ₂ <= 1e4, and the recursion inside 50 κ₂(B) m eps"""
    A, seeds = bjr.edge_matrix(ng, n0)
    assert bjr.shapes(A, 1, [seeds]) == [(ng, 2, max(n0, 5), 1)] and bjr.kappa2(A) <= 1e4
    bar = bjr.edge_bar(A, 1, [ng], [max(n0, 5)])
    ref = bjr.Ref(A, 1, 2)
    for r in (np.random.default_rng(7).standard_normal(A.shape[0]), np.eye(A.shape[0])[0]):
        want = ref(r)
        err = np.linalg.norm(bjr.sweep(A, 1, r, [seeds]) - want) / np.linalg.norm(want)
        assert err <= bar, (ng, n0, err, bar)


def test_every_block_one_by_one(mats):
    A = mats["micro"][0]
    n = A.shape[0]
    r = np.random.default_rng(1).standard_normal(n)
    assert bjr.shapes(A, n) == [(1, 0, 0, 1)] * n
    assert np.allclose(bjr.sweep(A, n, r), r / A.diagonal(), rtol=1e-15)


@pytest.mark.parametrize("name,nb", sorted(ITERATIONS))
def test_oracle_iteration_counts(orc, mats, name, nb):
    A, b = mats[name]
    Minv = bjr.Ref(A, nb, 2).dense_minv()
    n = A.shape[0]
    M = orc.neumann_neumann_operator([Minv], [np.arange(n)], np.ones(n, dtype=np.int64))
    _, it, _ = orc.pcg(orc.csc_operator(A), b, np.zeros(n), M)
    assert it == ITERATIONS[(name, nb)], (name, nb, it)
