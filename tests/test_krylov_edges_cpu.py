"""Host assertions that tests/test_gpu_krylov_edges.py relies on (no GPU): conditions on the oracle alone under which the
strict parity row (`it` equal, res_norm within 1e-8 res_k + 1e-12 res_1, x within 1e-6) says something about the device
code and not about the conditioning of the case, and that every case of tests/krylov_synth.py has the property it is named
for, so that the GPU file's parametrisation reaches the branch it was written for.

  * every solve of the tables ends within 50 iterations (the strict row applies) and on its tolerance, not on maxit;
  * the stop is decided: the last residual and the one before it are each >= 1e-4 (relative) away from tol = eps |b|, which is
    1e4 x the history bar;
  * the oracle's history differs from a numpy solver with pairwise sums in every dot product (the oracle adds left to right)
    by <= 1 % of the history bar, with `it` equal. Measured: at most 7.9e-4 of the bar (sp8192-defcg-3), smallest stop gap
    3.5e-4 (d1025w6-cg), longest solve 46 iterations (cg from a random x0, n >= 4096);
  * EPT from n, slot width, nloc, the number of tiles from csrc/dense_tiles.hpp through tests/cpp/dense_tiles_check.cpp,
    Gershgorin bounds of the blocks, WtAW non-singular with κ <= 1e6.
No case is skipped or expected to fail."""
import json
import subprocess

import numpy as np
import pytest

import krylov_synth as ks
import shard_synth as ss

FREE_SOLVES = [s for s in ks.all_solves() if s.maxit == 0]
CAPPED_SOLVES = [s for s in ks.all_solves() if s.maxit]


@pytest.fixture(scope="module")
def probs(orc):
    return ks.Problems(orc)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return ss.build_checker(tmp_path_factory.mktemp("dense_tiles"))


def test_tables_cover_the_issue():
    assert ks.SPARSE_N == (1023, 1024, 1025, 2048, 2049, 4096, 4097, 8191, 8192, 8193)
    assert [ks.ept(n) for n in ks.SPARSE_N] == [1, 1, 2, 2, 4, 4, 8, 8, 8, 0]
    assert ks.NVEC_ALL == (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 20, 21, 32, 33, 36, 37, 64, 65)
    by = {}
    for p, kinds, nv in ks.DEFLATED:
        by.setdefault(p, set()).update(nv)
    for p in ("nloc1023", "nloc1024", "nloc1025"):
        assert by[p] == set(ks.NVEC_ALL)
    assert {33, 36, 37, 64} <= by["tiles336"] and {17, 20, 21, 32, 33, 64} <= by["tiles544"]
    assert set(ks.NVEC_EPT8) <= by["d4097w4"] and set(ks.NVEC_EPT8) <= by["sp8192"] and 65 in by["sp8192"] and 65 in by["d4097w4"]
    assert set(ks.NVEC_EPT2) <= by["d1025w4"] and set(ks.NVEC_EPT2) <= by["sp2048"]
    assert ks.ept(ks.size_of("d4097w4")) == ks.ept(ks.size_of("sp8192")) == 8
    assert ks.ept(ks.size_of("d1025w4")) == ks.ept(ks.size_of("sp2048")) == 2
    # replay: one EPT 8 sparse case, one EPT 4 dense case, one deflated dense case
    assert [(s.prob in ks.SPARSE, ks.ept(ks.size_of(s.prob)), s.nvec > 0) for s in ks.REPLAY] == [(True, 8, False), (False, 4, False), (False, 1, True)]
    assert all(len(ks.replay_sequence(s)) == 8 for s in ks.REPLAY)
    assert len({s.id for s in ks.all_solves()}) == len(ks.all_solves())


def test_sparse_operators_are_what_they_are_named_for():
    for prob, n in ks.SPARSE.items():
        A = ks.banded(n)
        assert A.shape == (n, n) and (abs(A - A.T)).max() == 0.0
        d = A.diagonal()
        assert np.isclose(d.min(), 33.0) and np.isclose(d.max(), 3300.0)      # the scaling 1 ... 100 is on the diagonal: Jacobi matters
        assert set(np.round(d / 33.0).astype(int)) == {1, 4, 25, 100}
        # Jacobi-scaled, the matrix is T / 33: Gershgorin 1 -+ 3 / 33
        Dm = 1.0 / np.sqrt(d)
        J = A.multiply(Dm[:, None]).multiply(Dm[None, :]).tocsr()
        off = np.asarray(abs(J).sum(axis=1)).ravel() - J.diagonal()
        assert off.max() <= 3.0 / 33.0 + 1e-12 and np.allclose(J.diagonal(), 1.0)
        assert A.indptr[-1] == 5 * n - 6                                     # five diagonals


@pytest.mark.parametrize("name", list(ks.DENSE))
def test_dense_cases_have_the_property_they_are_named_for(probs, checker, tmp_path, name):
    d = ks.DENSE[name]
    g, cnt, n = probs.maps(name)
    assert n == d.n and cnt.size == n and cnt.min() >= 1
    assert [a.size for a in g] == list(d.sizes) and all(np.unique(a).size == a.size for a in g)
    assert np.array_equal(np.bincount(np.concatenate(g), minlength=n), cnt)
    assert int(cnt.max()) == d.width and d.slot_width == (4 if d.width == 3 else d.width)
    assert max(d.sizes) <= ks.GEMV_PANEL and d.folds == (d.slot_width <= 4)
    if d.width > 1:
        assert np.count_nonzero(cnt > 1) >= 50                               # a real overlap, not the hub node alone
    for S in probs.blocks(name):
        lo, hi = ks.gershgorin(S)
        assert 1.0 <= lo and hi <= 21.0 and np.array_equal(S, S.T)           # κ_d <= 21 <= 1e2, no factorisation needed
    # the tile list the operators will be built with (csrc/dense_tiles.hpp), one context: default 16 x 2 or the forced tiling
    waves, rpw = d.tiling or (16, 2)
    fn = tmp_path / f"{name}.txt"
    fn.write_text(" ".join(str(w) for w in [len(d.sizes), 1, ss.N_CU, 16, 0, *d.sizes, 0, len(d.sizes), waves, rpw]) + "\n")
    R = json.loads(subprocess.run([checker, str(fn)], capture_output=True, text=True, check=True).stdout)["ranks"][0]
    ntiles = len(R["tiles"])
    assert ntiles == R["part_total"] == d.ntiles(waves, rpw)
    assert R["max_ld"] <= ks.GEMV_PANEL and -(-R["max_ld"] // (64 * waves)) <= 8    # the folded launches take it (solvers.hpp)
    if name.startswith("d"):
        tag = int(name[1:name.index("w")])
        assert tag == d.n and name.endswith(f"w{d.width}")
    if name.startswith("nloc"):
        assert d.nloc == int(name[4:]) and ks.ept(d.n) == 1
        assert -(-d.nloc // 1024) == (2 if d.nloc == 1025 else 1)             # k_defl_mu's grid
    if name == "tiles336":
        # second pass over the partials needs ntiles > 16 tpv: tpv = 16 for nvec 33 ... 64
        assert d.tiling == (4, 1) and 256 < ntiles <= 512
    if name == "tiles544":
        assert d.tiling == (4, 1) and 512 < ntiles <= 1024                     # ... and tpv = 32 for nvec 17 ... 32; a third pass for 33 ... 64
    if name == ks.BIG:
        assert ks.FUSED_MAX_N < d.n <= 8300 and d.slot_width <= 4 and max(d.sizes) <= 2048 and d.nloc - d.n <= 200
    if name != ks.BIG:
        assert d.n <= ks.FUSED_MAX_N


def test_dense_table_crosses_widths_and_ept():
    seen = {(ks.ept(d.n), d.width) for d in ks.DENSE.values() if d.name.startswith("d")}
    for e in (1, 2, 4, 8):
        assert (e, 2) in seen and (e, 4) in seen                             # vector loads of 2 and 4 slots at every EPT
    assert (2, 1) in seen and (2, 6) in seen and (8, 3) in seen              # the generic loop at EPT > 1; 3 widened to 4
    sizes = sorted({d.n for d in ks.DENSE.values() if d.name.startswith("d") and d.width in (2, 4)})
    assert sizes == [1024, 1025, 2048, 2049, 4096, 4097]


@pytest.mark.parametrize("s", FREE_SOLVES, ids=lambda s: s.id)
def test_oracle_solve_is_short_decided_and_insensitive_to_summation_order(probs, s):
    x, it, res = probs.solve(s)
    b = probs.b(s.prob)
    tol = s.eps * np.linalg.norm(b)
    assert 2 <= it <= 50
    assert res[-1] <= tol * (1 - ks.STOP_GAP) and res[-2] >= tol * (1 + ks.STOP_GAP)
    xn, itn, resn = ks.numpy_solve(probs, s)
    share = ks.history_margin(resn, res)
    print(f"{s.id}: it {it}, res[-2] / tol {res[-2] / tol:.6g}, res[-1] / tol {res[-1] / tol:.6g}; numpy vs oracle: "
          f"|Δres| / bar {share:.2e}, |Δx| / (1e-6 |x|) {ks.x_margin(xn, x):.2e}")
    assert itn == it
    assert share <= ks.ORDER_SHARE and ks.x_margin(xn, x) <= ks.ORDER_SHARE
    if s.nvec:
        W = probs.W(s)
        A = probs.op(s.prob, "A")
        G = W.T @ np.column_stack([A(W[:, v]) for v in range(s.nvec)])
        assert np.allclose(W.T @ W, np.eye(s.nvec), atol=1e-12)
        assert np.linalg.cond(G) <= 1e6


@pytest.mark.parametrize("s", CAPPED_SOLVES, ids=lambda s: s.id)
def test_capped_solves_end_on_maxit(probs, s):
    x, it, res = probs.solve(s)
    assert it == s.maxit and res[-1] > s.eps * np.linalg.norm(probs.b(s.prob))


@pytest.mark.parametrize("s", ks.REPLAY, ids=lambda s: s.id)
def test_replay_sequence_is_shorter_then_longer(probs, s):
    """the `predicted` map of the device sees a shorter and then a longer solve than the first; b = 0 has nothing to iterate"""
    its = [probs.solve(t, bk)[1] for t, bk in ks.replay_sequence(s)]
    assert its[1] == 2 and its[2] < its[0] < its[3] and its[5] == its[7] == its[0] and its[6] == 1
    assert its[0] >= 4                                                       # chunk sizes it - 1, it, it + 1 are distinct from 0 and 1
