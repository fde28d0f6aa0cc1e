"""Host checks (no GPU) of the AMG refresh on frozen aggregates:

  * `fem.amg_refresh(prepare_amg_precond(A0), A1)` — A0 the `example01` matrix, A1 the lognormal one of the same mesh —
    against a fresh `prepare_amg_precond(A1)`: equal level sizes, equal values wherever the fresh hierarchy stores an entry,
    every extra structural entry within the entry-wise bound of its product (tests/amg_refresh_ref.level_bounds), ω, ω/d and
    the coarse inverse bit for bit;
  * the stale hierarchy is no substitute: pcg(A1, b, 0, Π) takes 8 / 11 iterations with the refreshed hierarchy at N = 34 /
    100 and strictly more with the hierarchy of A0;
  * csrc/amg_plan.hpp through tests/cpp/amg_plan_check.cpp: every pattern against scipy's structural products of all-ones
    matrices, the segments against a numpy sort, the permutations by applying them, on N = 12 and N = 34, the giant
    aggregate, a single aggregate per level and 1-based input; every refusal: a non-zero status and a message of more than
    40 characters that names the offender; the same checker under -fsanitize=address,undefined on the small cases and on
    every refusal."""
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import amg_ref as ar
import amg_refresh_ref as rr
from conftest import ROOT

SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")
KW12 = dict(max_levels=3, max_coarse=4)


@pytest.mark.parametrize("N,kw", [(12, KW12), (34, {}), (100, {})])
def test_refresh_equals_a_fresh_build(fem, N, kw):
    A0, A1, _ = rr.pair(fem, N)
    H0, F = fem.prepare_amg_precond(A0, **kw), fem.prepare_amg_precond(A1, **kw)
    assert H0.agg is not None and len(H0.agg) == H0.nlevels - 1
    assert all(np.array_equal(a, b) for a, b in zip(H0.agg, F.agg)), "the aggregates depend on the values"
    H = fem.amg_refresh(H0, A1)
    assert H.sizes == F.sizes and H.nlevels == F.nlevels
    assert np.array_equal(fem.amg_refresh(H0.agg, A1).coarse_inv, H.coarse_inv)
    for l in range(H.nlevels):
        got, want = H.A[l], F.A[l]
        w_on = rr.on_pattern(want, got)                     # asserts pattern(fresh) ⊆ pattern(refreshed)
        stored = rr.on_pattern(rr.ones(want), got) > 0
        assert np.array_equal(got.data[stored], w_on[stored]), f"A of level {l}"
        extra = ~stored
        if l:
            B = rr.level_bounds(H.A[l - 1], H.P[l - 1], H.agg[l - 1])
            bound = rr.on_pattern(B["G_bound"], got)
            print(f"N = {N} A_{l}: {extra.sum()} extra structural entries of {got.nnz}, max |extra| = "
                  f"{np.max(np.abs(got.data[extra]), initial=0.0):.3e}, smallest bound there {np.min(bound[extra], initial=np.inf):.3e}")
            assert (np.abs(got.data[extra]) <= bound[extra]).all()
            assert abs(got - got.T).max() == 0.0
        else:
            assert not extra.any()
        if l == H.nlevels - 1:
            break
        got, want = H.P[l], F.P[l]
        w_on = rr.on_pattern(want, got)
        stored = rr.on_pattern(rr.ones(want), got) > 0
        assert np.array_equal(got.data[stored], w_on[stored]), f"P of level {l}"
        B = rr.level_bounds(H.A[l], H.P[l], H.agg[l])
        bound = rr.on_pattern(B["P_bound"], got)
        print(f"N = {N} P_{l}: {(~stored).sum()} extra structural entries of {got.nnz}")
        assert (np.abs(got.data[~stored]) <= bound[~stored]).all()
        assert H.omega[l] == F.omega[l] and np.array_equal(H.omega_over_d[l], F.omega_over_d[l])
    assert np.array_equal(H.coarse_inv, F.coarse_inv)


@pytest.mark.parametrize("N,it_want", [(34, 8), (100, 11)])
def test_the_stale_hierarchy_is_no_substitute(fem, N, it_want):
    A0, A1, b1 = rr.pair(fem, N)
    H1, (x, it, res) = rr.refreshed_solve(fem, N)
    H0 = fem.prepare_amg_precond(A0)
    its = ar.pcg(A1, b1, np.zeros(b1.size), lambda r: ar.cycle(H0, r))[1]
    print(f"N = {N}: pcg(A1, b, 0, Π) it = {it} with the refreshed hierarchy, {its} with the stale one")
    assert it == it_want and its > it
    assert np.linalg.norm(A1 @ x - b1) <= 2e-7 * np.linalg.norm(b1)


# --------------------------------------------------------------------------------------------------- the plan checker
def _build(tmp, flags=()):
    exe = str(tmp / ("amg_plan_check" + ("_san" if flags else "")))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", *flags, "-o", exe, os.path.join(ROOT, "tests", "cpp", "amg_plan_check.cpp")])
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("amg_plan"))


@pytest.fixture(scope="module")
def sanitized_checker(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("amg_plan_san"), SANITIZE)


class Case:
    """one input of make_plan, everything 0-based; `write` adds the index base"""

    def __init__(self, A, aggs, sizes=None, rank=0, n_ranks=1, agg_given=None):
        A = sp.csr_matrix(A)
        self.n = A.shape[0]
        self.ptr, self.idx = A.indptr.astype(np.int64), A.indices.astype(np.int64)
        self.aggs = [np.asarray(a, dtype=np.int64) for a in aggs]
        self.sizes = [self.n] + [int(a.max()) + 1 for a in self.aggs] if sizes is None else list(sizes)
        self.rank, self.n_ranks = rank, n_ranks
        self.agg_given = len(self.aggs) if agg_given is None else agg_given

    def write(self, path, base=0):
        def arr(a, shift=0):
            a = np.asarray(a, dtype=np.int64).ravel()
            return " ".join(str(v) for v in [a.size, *(a + shift)])
        rows = [f"{self.n} {len(self.sizes)} {base} {self.rank} {self.n_ranks} {self.agg_given}", arr(self.sizes), arr(self.ptr, base),
                arr(self.idx, base)] + [arr(a, base) for a in self.aggs[:self.agg_given]]
        path.write_text("\n".join(rows) + "\n")
        return path


def run(exe, path):
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.splitlines()[0])


def _mirror(S):
    """entry k = (i, j) of the sorted pattern S -> the position of (j, i)"""
    S = sp.csr_matrix((np.arange(1, S.indices.size + 1, dtype=np.float64), S.indices, S.indptr), shape=S.shape)
    St = sp.csr_matrix(S.T)
    St.sort_indices()
    assert np.array_equal(St.indices, S.indices) and np.array_equal(St.indptr, S.indptr)
    return St.data.astype(np.int64) - 1


def check_plan(doc, c):
    """every array of the plan from scipy's structural products and numpy sorts"""
    assert doc["status"] == 0 and doc["err"] == "" and doc["nlev"] == len(c.sizes) == len(doc["levels"])
    A = sp.csr_matrix((np.ones(c.idx.size), c.idx, c.ptr), shape=(c.n, c.n))
    A.sort_indices()
    nbytes = 0
    for l, L in enumerate(doc["levels"]):
        g = {k: np.asarray(v, dtype=np.int64) for k, v in L.items() if k not in ("n", "nc", "tw")}
        n = A.shape[0]
        assert L["n"] == n == c.sizes[l]
        assert np.array_equal(g["a_ptr"], A.indptr) and np.array_equal(g["a_col"], A.indices), f"pattern of A_{l}"
        rows = np.repeat(np.arange(n), np.diff(A.indptr))
        diag = np.full(n, -1)
        on = np.flatnonzero(rows == A.indices)
        diag[rows[on]] = on
        assert np.array_equal(g["diag"], diag) and np.array_equal(g["sym"], _mirror(A))
        nbytes += 4 * (2 * n + 1 + 2 * A.nnz)
        if l == len(c.sizes) - 1:
            assert L["nc"] == 0 and all(g[k].size == 0 for k in ("agg", "p_ptr", "p_col", "seg_ptr", "seg_src", "r_from", "ap_col"))
            break
        agg, nc = c.aggs[l], c.sizes[l + 1]
        assert L["nc"] == nc and np.array_equal(g["agg"], agg)
        assert np.array_equal(np.asarray(L["tw"]), 1.0 / np.sqrt(np.bincount(agg, minlength=nc).astype(np.float64)))
        T = sp.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, nc))
        P = sp.csr_matrix(T + A @ T)
        P.sort_indices()
        P.data[:] = 1.0
        assert np.array_equal(g["p_ptr"], P.indptr) and np.array_equal(g["p_col"], P.indices), f"pattern of P_{l}"
        # segments: the entries of A ordered by (row, aggregate of the column, position), cut where the P entry changes
        kP = rr.keys(P)
        dest = rows.astype(np.int64) * nc + agg[A.indices]
        order = np.lexsort((np.arange(A.nnz), dest))
        assert np.array_equal(g["seg_src"], order), f"segments of P_{l}"
        assert np.array_equal(g["seg_ptr"], np.searchsorted(dest[order], np.concatenate((kP, [n * nc])))), f"segment pointer of P_{l}"
        assert np.array_equal(np.sort(g["seg_src"]), np.arange(A.nnz))
        # R = P' and the permutation that carries P's values to R's
        Pn = sp.csr_matrix((np.arange(1, P.nnz + 1, dtype=np.float64), P.indices, P.indptr), shape=P.shape)
        R = sp.csr_matrix(Pn.T)
        R.sort_indices()
        assert np.array_equal(g["r_ptr"], R.indptr) and np.array_equal(g["r_col"], R.indices)
        assert np.array_equal(g["r_from"], R.data.astype(np.int64) - 1)
        AP = sp.csr_matrix(A @ P)
        AP.sort_indices()
        assert np.array_equal(g["ap_ptr"], AP.indptr) and np.array_equal(g["ap_col"], AP.indices), f"pattern of A_{l} P_{l}"
        R.data[:] = 1.0
        nxt = sp.csr_matrix(R @ AP)
        nxt.sort_indices()
        nxt.data[:] = 1.0
        nbytes += 4 * (3 * n + nc + 4 + 4 * P.nnz + A.nnz + AP.nnz) + 8 * nc
        A = nxt
    assert doc["bytes"] == nbytes


def _cases(fem):
    out = {}
    A0, _, _ = rr.pair(fem, 12)
    out["N12"] = Case(A0, fem.prepare_amg_precond(A0, **KW12).agg)
    A0, _, _ = rr.pair(fem, 34)
    out["N34"] = Case(A0, fem.prepare_amg_precond(A0).agg)
    Ag, _, aggs = rr.giant_aggregates(fem)
    out["giant"] = Case(Ag, aggs)
    A0, _, _ = rr.pair(fem, 12)
    out["single"] = Case(A0, [np.zeros(A0.shape[0], dtype=np.int64)])
    out["one_level"] = Case(A0, [])
    return out


def test_plan_against_scipy(fem, checker, tmp_path):
    cases = _cases(fem)
    assert len(cases["N12"].sizes) == 3 and np.bincount(cases["giant"].aggs[0]).max() == 1100
    for tag, c in cases.items():
        doc = run(checker, c.write(tmp_path / f"{tag}.txt"))
        check_plan(doc, c)
        print(f"{tag}: levels {c.sizes}, plan bytes {doc['bytes']}")
    for tag in ("N12", "N34"):                                # 1-based input: the same plan
        d0 = run(checker, cases[tag].write(tmp_path / f"{tag}_b0.txt", 0))
        d1 = run(checker, cases[tag].write(tmp_path / f"{tag}_b1.txt", 1))
        assert d0 == d1


def _refusals(fem):
    A0, _, _ = rr.pair(fem, 12)
    n = A0.shape[0]
    good = fem.prepare_amg_precond(A0, **KW12).agg
    nc = int(good[0].max()) + 1
    out = []
    B = sp.lil_matrix(A0); B[0, n - 1] = 1.0                  # (0, n-1) without (n-1, 0)
    out.append(("unsymmetric", Case(sp.csr_matrix(B), good), ["not structurally symmetric", f"(0, {n - 1})"]))
    c = Case(A0, good); c.idx = c.idx.copy(); c.idx[1] = c.idx[0]
    out.append(("duplicate", c, ["duplicates", "row 0"]))
    bad = [good[0].copy(), good[1]]; bad[0][5] = nc
    out.append(("agg_range", Case(A0, bad, sizes=[n, nc, int(good[1].max()) + 1]), ["node 5", f"aggregate {nc}", f"{nc} aggregates"]))
    bad = [good[0].copy(), good[1]]; bad[0][bad[0] == 2] = 1
    out.append(("agg_empty", Case(A0, bad, sizes=[n, nc, int(good[1].max()) + 1]), ["aggregate 2", "empty"]))
    out.append(("chain", Case(A0, good, sizes=[n, n, 3]), ["do not chain", str(n)]))
    out.append(("chain0", Case(A0, good, sizes=[n + 1, nc, 3]), ["do not chain", str(n + 1)]))
    big = 4097
    out.append(("coarse", Case(sp.identity(big, format="csr"), []), ["4097", "4096"]))
    out.append(("ranks", Case(A0, good, rank=1, n_ranks=4), ["rank 1 of 4"]))
    out.append(("agg_null", Case(A0, good, agg_given=1), ["aggregates of level 1", "NULL"]))
    return out


def _check_refusals(exe, fem, tmp_path):
    for tag, c, words in _refusals(fem):
        for base in (0, 1):
            doc = run(exe, c.write(tmp_path / f"{tag}_{base}.txt", base))
            print(f"  {tag} (base {base}): {doc['err']}")
            assert doc["status"] != 0 and len(doc["err"]) > 40 and doc["levels"] == [] and doc["nlev"] == 0, (tag, doc["err"])
            if base == 0:
                assert all(w in doc["err"] for w in words), (tag, doc["err"])


def test_plan_refusals(fem, checker, tmp_path):
    _check_refusals(checker, fem, tmp_path)


def test_plan_checker_under_sanitizers(fem, sanitized_checker, tmp_path):
    """address + undefined-behaviour sanitizers on the stand-alone checker: the small cases, 1-based input, every refusal"""
    cases = _cases(fem)
    for tag in ("N12", "single", "one_level"):
        for base in (0, 1):
            check_plan(run(sanitized_checker, cases[tag].write(tmp_path / f"{tag}_{base}.txt", base)), cases[tag])
    _check_refusals(sanitized_checker, fem, tmp_path)
