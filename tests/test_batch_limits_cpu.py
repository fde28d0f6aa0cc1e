"""The inputs of tests/test_gpu_batch_limits.py held, on the CPU, to the conditions that make them edges of the batched and the
multi-workgroup Krylov loop (tests/batch_limit_cases.py): a GPU test must never pass because its input missed the edge.
Every measured figure is printed (run with -s)."""
import numpy as np
import pytest

import amg_setup_synth as asy
import amg_synth as ays
import batch_limit_cases as blc


def test_host_arithmetic_of_the_grids():
    assert blc.vec_grid(1) == 1 and blc.vec_grid(1024) == 1 and blc.vec_grid(1025) == 2
    assert blc.vec_grid(524288) == 512 and blc.passes(524288, 512) == 1
    assert blc.vec_grid(524289) == 512 and blc.passes(524289, 512) == 2
    assert blc.first_graph(0, 8, 2049) == 8 and blc.first_graph(2048, 8, 2049) == 1024 and blc.first_graph(513, 8, 2049) == 512
    assert blc.first_graph(300, 8, 50) == 50 and blc.first_graph(49, 8, 49) == 49 and blc.first_graph(65, 8, 2049) == 64


@pytest.mark.parametrize("n", [1, 2, 3, 300, 340, 341, 342, 343, 683, 2041, 2043, 5801, 5803, 6001, 20001])
def test_closed_form_block_count_is_row_blocks(n):
    assert blc.chain_block_count(n) == ays.row_blocks(asy.chain(n).indptr).shape[0]


def test_big_chains_sit_past_the_caps():
    na, nb = blc.big_n("big_a"), blc.big_n("big_b")
    assert na == 524289 == 4 * 512 * 256 + 1
    assert na - 4 * blc.MAX_PARTS * blc.NT == 1, "the second pass of big_a holds exactly one element"
    for name, n in (("big_a", na), ("big_b", nb)):
        S = asy.chain(n)
        blocks = ays.row_blocks(S.indptr).shape[0]
        assert blocks == blc.chain_block_count(n)
        assert n % 2 == 1 and S.indices.size == 3 * n - 2 and S.indices.size % 2 == 1
        assert blc.vec_grid(n) == 512 and blc.passes(n, 512) == 2
        assert blc.passes(n, blc.CF_VEC_GRID) >= 3, "the two-launch sparse form's grid of 256 takes further passes too"
        print(f"{name}: n = {n}, nnz = {S.indices.size}, row blocks = {blocks}, vec_grid = {blc.vec_grid(n)}, "
              f"passes = {blc.passes(n, 512)} (grid 512), {blc.passes(n, blc.CF_VEC_GRID)} (grid 256)")
        if name == "big_a":
            assert blc.LANE_SET < blocks <= blc.LANE_PASS, "lanes 1 .. 7 of sum_partials, one pass"
        else:
            assert blocks >= blc.LANE_PASS + 1, "a second pass of sum_partials"
            assert ays.row_blocks(asy.chain(n - 2).indptr).shape[0] < blc.LANE_PASS + 1, "not the smallest odd length"


@pytest.mark.parametrize("name", ["big_a", "big_b"])
def test_big_references_stop_clear_of_the_tolerance(orc, name):
    mats, bs, X0 = blc.big(name)
    assert not X0[:, 0].any() and np.count_nonzero(X0[:, 1]) == X0.shape[0], "column 0 zero, column 1 non-zero everywhere"
    for t in range(2):
        ref = blc.big_cg_ref(orc, name, t)
        last, before = blc.margins(ref[2], bs[t])
        print(f"{name}: system {t}: oracle cg it = {ref[1]}, res_norm[it] = {last:.3f} tol, res_norm[it - 1] = {before:.3f} tol")
        assert blc.tight(ref, bs[t]), (ref[1], last, before)
        mine = blc.cg_ref(mats[t], bs[t], X0[:, t])                       # the numpy restatement agrees with the oracle
        assert mine[1] == ref[1] and np.allclose(mine[2], ref[2], rtol=1e-8, atol=1e-12 * ref[2][0])


def test_big_a_bank_reference_stops_clear_of_the_tolerance(fem):
    mats, bs, _ = blc.big("big_a")
    aggs = blc.big_aggregates("big_a")
    sizes = [a.size for a in aggs] + [int(aggs[-1].max()) + 1]
    assert sizes == [524289, 65537, 8193, 1025, 129]
    ref = blc.big_bank_ref(fem, "big_a")
    last, before = blc.margins(ref[2], bs[0])
    print(f"big_a bank: levels {sizes}; restatement pcg it = {ref[1]}, res_norm[it] = {last:.3f} tol, res_norm[it - 1] = {before:.3f} tol")
    assert blc.tight(ref, bs[0]), (ref[1], last, before)


def test_lap2049_counts_on_both_sides_of_the_stage():
    mats, b = blc.lap2049()
    n = blc.LAP_LONG_N
    assert all(np.array_equal(A.indptr, mats[0].indptr) and np.array_equal(A.indices, mats[0].indices) for A in mats)
    its = [blc.cg_ref(A, b)[1] for A in mats]
    print(f"lap2049: numpy cg counts {its} for sigma = {blc.LAP_SIGMA}")
    short = [it for it in its if it <= blc.LOW * blc.BATCH_RES_STAGE]
    long_ = [it for it in its if it >= blc.HIGH * blc.BATCH_RES_STAGE]
    assert len(short) == 2 and len(long_) == 2 and its[0] in short and its[1] in short
    assert its[3] == n, "the unshifted system stops by maxit = n"
    last, _ = blc.margins(blc.cg_ref(mats[3], b)[2], b)
    assert last > 10.0, "... far from converged"
    assert blc.FIRST_CAP - max(short) >= 500, "the short systems are frozen for at least 500 replayed iterations"
    assert blc.first_graph(its[3] - 1, 8, n) == blc.FIRST_CAP


def test_lap301_reaches_the_capacity(orc):
    mats, b, maxit = blc.lap301()
    n = blc.LAP_OVER_N
    assert maxit == n + 5
    tol = blc.EPS * np.linalg.norm(b)
    x, it, res = blc.cg_ref(mats[0], b, maxit=maxit)
    print(f"lap301: restatement it = {it}; res_norm[n] = {res[n - 1] / tol:.4g} tol, res_norm[n + 1] = {res[n] / tol:.4g} tol; "
          f"min over [1, n] = {res[:n].min() / tol:.4g} tol")
    assert it >= n + 1 and np.isfinite(res).all() and (res > 0).all()
    assert res[:n].min() >= 10.0 * tol, "the restatement does not stop before it = n + 1, with a margin no summation order moves"
    with pytest.raises(orc.BoundsError):
        blc.oracle_cg(orc, mats[0], b, maxit=maxit)
    xs, its, ress = blc.cg_ref(mats[1], b, maxit=maxit)
    print(f"lap301: shifted by {blc.LAP_OVER_SIGMA}: it = {its}")
    assert its < blc.LOW * n and ress[-1] <= tol
    for m in range(1, 51):                                   # the sweep of the eviction test: every small maxit is reached
        assert blc.cg_ref(mats[0], b, maxit=m)[1] == m
    assert blc.first_graph(it - 1, 8, 50) == 50 and all(blc.first_graph(m, 8, m) == m for m in range(1, 50))


def test_poisons_are_what_they_say():
    A = blc.laplacian(9)
    v = blc.poisoned_values(A, "A_nan")
    assert np.isnan(v).sum() == 1
    assert not blc.poisoned_values(A, "A_zero").any()
    assert blc.poisoned_values(A, "x0_inf") is None
    x = blc.poison_x0(np.zeros(9), "x0_inf")
    assert np.isposinf(x).sum() == 1 and np.isfinite(x).sum() == 8
    assert not blc.poison_x0(np.zeros(9), "A_nan").any()
