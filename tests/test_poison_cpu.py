"""Host assertions that tests/test_gpu_poison.py relies on (no GPU), on the oracle alone:

  * the outcome table of tests/poison_synth.py (EXPECT) for every solver kind on an SPD tridiagonal system of n = 1025
    (eig_synth.matrix), and for every poisoned call the GPU file makes: either (x, it, res_norm) or one of the two exception
    kinds, nothing else;
  * the breakdown systems: res_norm = [sqrt(n), inf, nan] and it = 3 bit for bit from the oracle (sums left to right) and from
    a numpy solver with pairwise sums, for every n, as CSR and as the dense pair; eigcg the same, eigpcg a BoundsError;
  * every clean solve of the GPU file meets the conditions of tests/test_krylov_edges_cpu.py (it <= 50, the last two residuals
    >= 1e-4 away from tol, oracle within 1 % of the history bar of the numpy solver), so the bitwise comparison of a repeated
    solve is sensitive to state and to nothing else; the eigCG-family calls end on maxit with a Ritz gap >= eig_synth.GAP_MIN;
  * each case has the form property it is named for: EPT, slot width, fold eligibility, more than FUSED_MAX_N rows, the row
    blocks of csrc/spmv_blocks.hpp, every interior system <= 300 rows; the oracle's interior CG ends a NaN right-hand side at
    0 iterations with x = 0;
  * tests/cpp/dense_small_check.cpp with non-finite inputs, plain and under -fsanitize=address,undefined as a stand-alone
    program.
No case is skipped or expected to fail."""
import json
import os
import subprocess

import numpy as np
import pytest

import eig_synth as es
import krylov_synth as ks
import poison_synth as ps
import shard_synth as shs
import sparse_synth as ss
from conftest import ROOT


@pytest.fixture(scope="module")
def probs(orc):
    return ps.Problems(orc)


def describe(out):
    kind, r = out
    return kind if r is None else (r[1], ps.kind_of_value(r[2][0]))


# ------------------------------------------------------------------ the outcome table
@pytest.mark.parametrize("kind", ps.KINDS)
def test_outcome_table_on_the_tridiagonal_system(probs, kind):
    c = ps.eig_call(kind) if kind in ps.EIG_KINDS else ps.Call(ps.EIG, kind, ps.EIG_NVEC if ps.takes_W(kind) else 0)
    A = probs.matrix(ps.EIG)
    assert A.shape == (1025, 1025) and A.nnz == 3 * 1025 - 2 and np.linalg.eigvalsh(A.toarray())[0] > 0
    kind_, r = probs.solve(c)
    assert kind_ == "ok" and np.all(np.isfinite(r[2])) and np.all(np.isfinite(r[0]))
    for p in ps.POISONS_VEC + ps.POISONS_W:
        want = ps.EXPECT[(ps.group_of(kind), p)]
        if want is None:
            assert p not in ps.poisons_of(kind)
            continue
        out = probs.solve(c, p)
        print(f"{kind} {p}: {describe(out)} (table: {want})")
        assert out[0] in ("ok", "singular", "bounds")
        assert describe(out) == want, (kind, p)
        if out[0] == "ok":
            assert out[1][2].size == 1


def gpu_poisoned_calls():
    out = [(c, p) for _, _, calls in ps.SPARSE_GROUP for c in calls for p in ps.POISONS_VEC]
    out += [(c, p) for _, _, calls in ps.DENSE_GROUP for c in calls for p in ps.POISONS_VEC]
    out += [(c, p) for c, _ in ps.DEFL_GROUP for p in ps.poisons_of(c.kind)]
    out += [(c, p) for c in ps.EIG_GROUP for p in ps.poisons_of(c.kind)]
    return out


@pytest.mark.parametrize("c,p", gpu_poisoned_calls(), ids=lambda v: v.id if isinstance(v, ps.Call) else v)
def test_every_poisoned_call_of_the_gpu_file_follows_the_table(probs, c, p):
    out = probs.solve(c, p)
    assert ps.poison_maxit(c) <= 50
    assert describe(out) == ps.EXPECT[(ps.group_of(c.kind), p)], (c.id, p, describe(out))


# ------------------------------------------------------------------ breakdown inside the loop
@pytest.mark.parametrize("c", ps.BREAKDOWN_CALLS, ids=lambda c: c.id)
def test_breakdown_history_is_exact_in_any_summation_order(probs, c):
    n = probs.n(c.prob)
    assert 0 < c.maxit <= 50
    want = ps.breakdown_history(n)
    kind, r = probs.solve(c)
    if c.kind == "eigpcg":
        assert kind == "bounds"                                   # the final extraction at ivec = 3 with nvec = 2
        return
    assert kind == "ok"
    print(f"{c.id}: it {r[1]}, res_norm {r[2]}")
    assert r[1] == 3 and np.array_equal(r[2], want, equal_nan=True)
    assert r[2][0] == np.sqrt(n)
    if not c.kind.startswith("eig"):
        xn, itn, resn = ps.numpy_solve(probs, c, c.maxit)
        assert itn == 3 and np.array_equal(resn, r[2], equal_nan=True) and resn[:2].tobytes() == r[2][:2].tobytes()


def test_breakdown_systems_are_powers_of_two():
    for n in ps.BREAKDOWN_N:
        A = ps.breakdown(n)
        d = A.diagonal()
        assert A.nnz == n and np.count_nonzero(d == 1.0) == np.count_nonzero(d == -1.0) == n // 2
    assert [ks.ept(n) for n in ps.BREAKDOWN_N] == [2, 8, 0] and ps.BREAKDOWN_N[2] > ks.FUSED_MAX_N
    S, Pi, g, cnt, n = ps.breakdown_dense()
    assert n == 1026 and ks.ept(n) == 2 and len(S) == 2 and np.array_equal(g[0], g[1]) and np.all(cnt == 2)
    assert max(B.shape[0] for B in S) <= ks.GEMV_PANEL                  # slot width 2, blocks within the panel: folds
    assembled = sum(np.diag(B) for B in S)
    assert np.array_equal(np.abs(assembled), np.ones(n)) and assembled.sum() == 0.0
    assert all(np.array_equal(B, np.diag(np.diag(B))) for B in S) and all(np.array_equal(P, np.eye(n)) for P in Pi)
    v = np.arange(1.0, n + 1)
    assert np.array_equal(sum((P @ (v / cnt)) / cnt for P in Pi), v / 2)  # Π = I / 2 exactly


# ------------------------------------------------------------------ the clean solves are short, decided and order-insensitive
@pytest.mark.parametrize("c", ps.clean_calls(), ids=lambda c: c.id)
def test_clean_solve_is_short_decided_and_insensitive_to_summation_order(probs, c):
    kind, (x, it, res) = probs.solve(c)
    tol = c.eps * np.linalg.norm(probs.b(c.prob, c.kind))
    assert 2 <= it <= 50
    assert res[-1] <= tol * (1 - ks.STOP_GAP) and res[-2] >= tol * (1 + ks.STOP_GAP)
    if c.prob in ks.SPARSE or c.prob in ks.DENSE:
        xn, itn, resn = ks.numpy_solve(probs.ks, c.as_solve())
    else:
        xn, itn, resn = ps.numpy_solve(probs, c, 0)
    share = ks.history_margin(resn, res)
    print(f"{c.id}: it {it}, res[-2] / tol {res[-2] / tol:.6g}, res[-1] / tol {res[-1] / tol:.6g}; numpy vs oracle: "
          f"|Δres| / bar {share:.2e}, |Δx| / (1e-6 |x|) {ks.x_margin(xn, x):.2e}")
    assert itn == it and share <= ks.ORDER_SHARE and ks.x_margin(xn, x) <= ks.ORDER_SHARE


@pytest.mark.parametrize("c", ps.EIG_GROUP, ids=lambda c: c.id)
def test_clean_eig_calls_end_on_maxit_with_a_gap(orc, probs, c):
    kind, r = probs.solve(c)
    assert kind == "ok" and r[1] == c.maxit <= 50 and np.all(np.isfinite(r[2])) and r[2][-1] > 0
    if c.kind.startswith("eig"):
        assert np.all(np.isfinite(r[3])) and r[3].shape == (1025, ps.EIG_NVEC)
        state = {}
        pre = probs.precond(c)
        es.run(orc, c.kind, probs.op(c.prob, "A"), probs.op(c.prob, pre) if pre else None, probs.b(c.prob, c.kind), probs.x0(c),
               probs.W(c), c.nvec, c.spdim, c.maxit, c.eps, state=state)
        T = es.decisive_T(state)
        if T is not None:
            gap = es.ritz_gap(T, c.nvec)
            print(f"{c.id}: Ritz gap {gap:.3e}")
            assert gap >= es.GAP_MIN
    assert c.spdim > 3                                                 # the breakdown (it = 3) never reaches a restart
    if c.kind in ("eigcg", "eigpcg"):
        # the short call that shows a window left over from an earlier solve: one column, then zeros
        kind, r = probs.solve(ps.eig_start_call(c.kind))
        assert kind == "ok" and r[1] == 1 and np.any(r[3][:, 0]) and not np.any(r[3][:, 1:])


# ------------------------------------------------------------------ each case reaches the form it is named for
@pytest.fixture(scope="module")
def spmv_checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("spmv_blocks")
    exe = str(d / "spmv_blocks_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "spmv_blocks_check.cpp")])
    return exe


@pytest.fixture(scope="module")
def tiles_checker(tmp_path_factory):
    return shs.build_checker(tmp_path_factory.mktemp("dense_tiles"))


def test_dense_pair_takes_the_folded_launches(tiles_checker, tmp_path):
    """the tile list of the two 1026-row blocks from csrc/dense_tiles.hpp (default tiling 16 x 2), as test_krylov_edges_cpu.py
    checks it for krylov_synth's cases: the folded launches take it (slot width 2, padded rows within the panel)"""
    sizes = (ps.BREAKDOWN_DENSE_N,) * 2
    fn = tmp_path / "pair.txt"
    fn.write_text(" ".join(str(w) for w in [len(sizes), 1, shs.N_CU, 16, 0, *sizes, 0, len(sizes), 16, 2]) + "\n")
    R = json.loads(subprocess.run([tiles_checker, str(fn)], capture_output=True, text=True, check=True).stdout)["ranks"][0]
    assert len(R["tiles"]) == R["part_total"] == sum(-(-n // 32) for n in sizes)
    assert R["max_ld"] <= ks.GEMV_PANEL and -(-R["max_ld"] // (64 * 16)) <= 8


def test_cases_have_the_form_property_they_are_named_for(probs):
    assert [ks.ept(probs.n(p)) for p, _, _ in ps.SPARSE_GROUP] == [2, 8, 0]
    assert probs.n(ps.TRI) > ks.FUSED_MAX_N and probs.n("brk9002") > ks.FUSED_MAX_N
    d = ks.DENSE
    assert (ks.ept(d["d1025w4"].n), d["d1025w4"].slot_width, d["d1025w4"].folds) == (2, 4, True)
    assert (ks.ept(d["d4097w4"].n), d["d4097w4"].slot_width, d["d4097w4"].folds) == (8, 4, True)
    assert (ks.ept(d["d2048w1"].n), d["d2048w1"].slot_width) == (2, 1)
    assert d["big8200"].n > ks.FUSED_MAX_N and d["big8200"].folds and d["big8200"].slot_width == 2
    assert d[ps.DEFL_PROB].nloc == 1024 and d[ps.DEFL_PROB].folds and ps.DEFL_NVEC == (5, 21)   # 21: past k_defl_mu's 20 preloaded columns
    assert ps.F32_PROB == "d1025w4"
    # the clean solve around a breakdown runs at the breakdown's n (the context keys its Krylov workspace by n)
    for clean, brk, _ in ps.breakdown_pairs():
        assert probs.n(clean.prob) == probs.n(brk.prob) and probs.is_dense(clean.prob) == probs.is_dense(brk.prob)
    for clean, brk in ps.eig_breakdown_pairs():
        assert probs.n(clean.prob) == probs.n(brk.prob) == 1026
        kind, r = probs.solve(clean)
        assert kind == "ok" and r[1] == clean.maxit and np.all(np.isfinite(r[2])) and np.all(np.isfinite(r[3]))
    S, Pi, g, cnt, n = probs.dense(ps.PAIR)
    gb = probs.dense(ps.BRK_DENSE)[2]
    assert all(np.array_equal(a, b) for a, b in zip(g, gb)) and [B.shape for B in S] == [(1026, 1026)] * 2
    assert all(1.0 <= ks.gershgorin(B)[0] and ks.gershgorin(B)[1] <= 21.0 for B in S)
    for c, _ in ps.DEFL_GROUP:
        assert c.as_solve() in ks.DEFLATED_SOLVES
    assert set(ps.EIG_KINDS) == {c.kind for c in ps.EIG_GROUP} and len(ps.EIG_GROUP) == 6


@pytest.mark.parametrize("prob", [ps.TRI, "brk9002"])
def test_two_launch_cases_have_many_row_blocks(probs, spmv_checker, tmp_path, prob):
    A = probs.matrix(prob)
    fn = tmp_path / "rowptr.bin"
    ss.write_rowptr(fn, A.indptr)
    R = json.loads(subprocess.run([spmv_checker, str(fn)], capture_output=True, text=True, check=True).stdout.splitlines()[0])
    blk = np.array(R["blocks"], dtype=np.int64).reshape(-1, 4)
    assert R["n"] == A.shape[0] and blk.shape[0] >= 8 and np.all(blk[:, 3] - blk[:, 2] <= ss.SPMV_TILE)   # every XCD has row blocks


def test_interior_sets_are_small_and_the_oracle_ends_a_nan_at_zero_iterations(orc):
    for name, (s, dom) in ps.interior_sets().items():
        assert max(s.n_i) <= ps.ICG_MAX_ROWS and s.n_i[dom] > 0, name
        b = s.b_I[dom].copy()
        b[b.size // 2] = np.nan
        x, it = orc.interior_cg(s.A_II[dom], b, s.reltol)
        assert it == 0 and not np.any(x) and not np.isnan(x).any(), (name, it)
        x, it = orc.interior_cg(s.A_II[dom], s.b_I[dom], s.reltol)
        assert 0 < it <= s.n_i[dom] and np.all(np.isfinite(x))
    s, dom = ps.interior_sets()["mixed"]
    assert s.n_i == [1, 2, 300, 300, 0] and dom == 3
    # the poisoned subdomain is the slowest: a form that keeps iterating on NaN shows in interior_iterations()
    its = [orc.interior_cg(A, b, s.reltol)[1] if A.shape[0] else 0 for A, b in zip(s.A_II, s.b_I)]
    assert its[dom] == max(its) and sorted(its)[-2] < its[dom]


# ------------------------------------------------------------------ the small dense routines with non-finite inputs
def _build_dense_small(tmp, flags):
    exe = str(tmp / ("dense_small_check" + ("_san" if flags else "")))
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *flags, os.path.join(ROOT, "tests", "cpp", "dense_small_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "sanitized"])
def test_dense_small_routines_return_on_non_finite_input(tmp_path, flags):
    """sym_eig_upper, svd_left and ritz_restart with NaN, +Inf, -Inf in one diagonal entry, one off-diagonal entry and
    everywhere at (m, nvec) = (3, 1), (6, 2), (24, 10), (70, 33): each call returns (the sweeps are bounded), nev <= m and
    G has m nev entries. The second build is a stand-alone program under the address and undefined-behaviour sanitizers."""
    exe = _build_dense_small(tmp_path, list(flags))
    r = subprocess.run([exe, "nonfinite"], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rows = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(rows) == 4 * 3 * 3 and {(q["m"], q["nvec"]) for q in rows} == {(3, 1), (6, 2), (24, 10), (70, 33)}
    for q in rows:
        assert q["returned"] == 3 and 0 <= q["nev"] <= q["m"] and q["g_size"] == q["m"] * q["nev"], q
