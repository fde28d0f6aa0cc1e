"""Host checks (no GPU) of the level set-up plan, csrc/setup_plan.hpp, through tests/cpp/setup_plan_check.cpp, built plain and
with -fsanitize=address,undefined; both builds run every case.

Plan mode, index_base 0 and 1: the seven subdomains of test_gpu_setup_edges.ladders() in one plan and each alone, the two
island cases, direct_inverse(n0, 10) for n0 = 1, 64, 65 and empty_interior(5) alone.
  * the levels are setup_synth.bfs_levels, node for node; an unreached node's slot of `perm` holds 0;
  * with the stored values replaced by distinct integers, the dense A_kk and A_ΓΓ rebuilt from the entry lists and
    C_k = A[L_{k+1}, L_k], B = A_IΓ[L_0, :] rebuilt from the column form equal the scipy slices exactly, and no stored entry
    is used twice: the lists hold exactly the entries inside a level, from a level to the next deeper one, of A_IΓ, of A_ΓΓ;
  * the row form of setup::row_form is the transpose of the column form with strictly ascending columns, its offsets
    those of arrays that are appended to;
  * offsets and totals are the sums of the inputs; a subdomain's record alone equals its record in the mixed plan up to the
    offsets; in the island cases lev_off[nlev] < n_i.
Refusals (status 1 and the exact text): a row index out of range in each block, an A_II that lost one entry of a symmetric
pair across two levels, a negative size, a column pointer that ends below its start. (The plan looks at the ends of a
column-pointer array only, as it always has: a decrease in the middle is the caller's to refuse, mi_block_jacobi_create's
make_split does.)

Split mode (bj::make_split, then the plan of the split): the matrices and block counts of
test_block_jacobi_cpu.py::test_default_seed_shapes and one explicit-seed case: G, I and the component counts are
block_jacobi_ref.default_seeds', and the levels reach every node of every block."""
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csgraph

import block_jacobi_ref as bjr
import lorasc_ref as lr
import setup_synth as ss
import sparse_synth
from conftest import ROOT
from test_gpu_setup_edges import ladders

SANITIZE = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
BAD_ARG = 1


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    san = request.param == "sanitized"
    out = str(tmp_path_factory.mktemp("setup_plan") / ("setup_plan_check" + ("_san" if san else "")))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", *(SANITIZE if san else ("-O2",)), "-o", out,
                           os.path.join(ROOT, "tests", "cpp", "setup_plan_check.cpp")])
    return out


def arr(a, shift=0):
    a = np.asarray(a, dtype=np.int64).ravel()
    return " ".join(str(v) for v in [a.size, *(a + shift)])


def run(exe, path, text):
    path.write_text(text)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.splitlines()[0])


def plan_text(blocks, base, n_g=None, n_i=None):
    """blocks: per subdomain six arrays (ii_ptr, ii_idx, ig_ptr, ig_idx, gg_ptr, gg_idx), 0-based"""
    n_g = [len(b[2]) - 1 for b in blocks] if n_g is None else n_g
    n_i = [max(len(b[0]) - 1, 0) for b in blocks] if n_i is None else n_i
    return "\n".join([f"0 {len(blocks)} {base}", arr(n_g), arr(n_i)] + [arr(a, base) for b in blocks for a in b]) + "\n"


def blocks_of(c):
    out = []
    for M in (c.A_II, c.A_IΓ, c.A_ΓΓ):
        M = sp.csc_matrix(M)
        out += [M.indptr, M.indices]
    return out


@pytest.fixture(scope="module")
def synth():
    """every plan-mode input, generated once (the generators assert their own level widths)"""
    islands = [ss.ladder([33, 70, 20], degree=[1, 5], density=0.05, n_gamma=17, gamma_deg=2, seed=8, island=9, tag="island"),
               ss.ladder([30, 10], degree=2, n_gamma=16, seed=9, tag="island's neighbour")]
    return {"ladders": ladders(), "islands": islands, "direct": [ss.direct_inverse(n0, 10.0) for n0 in (1, 64, 65)],
            "empty": [ss.empty_interior(5)]}


def numbered(M, off):
    """M's pattern with the value off + k + 1 at stored entry k: what the entry lists' `src` points to"""
    M = sp.csc_matrix(M)
    return sp.csc_matrix((off + np.arange(M.nnz) + 1.0, M.indices, M.indptr), shape=M.shape)


def expectation(cases):
    """Everything the plan must say, from scipy and setup_synth.bfs_levels alone (checked before the C++ is looked at)."""
    out, off = [], dict(ii=0, ig=0, gg=0, bi=0, s=0, w=0)
    for c in cases:
        ni, ng = c.A_IΓ.shape
        levels = [np.asarray(l, dtype=np.int64) for l in ss.bfs_levels(c.A_II, c.A_IΓ)] if ni else []
        assert [len(l) for l in levels] == list(c.widths), c.tag
        assert all(np.all(np.diff(l) > 0) for l in levels)
        reached = np.concatenate(levels) if levels else np.zeros(0, dtype=np.int64)
        assert np.unique(reached).size == reached.size <= ni
        assert ni == 0 or abs(c.A_II - c.A_II.T).max() == 0                # symmetric: the transposed twins may stay unused
        Aii, Aig, Agg = numbered(c.A_II, off["ii"]).tocsr(), numbered(c.A_IΓ, off["ig"]).tocsr(), numbered(c.A_ΓΓ, off["gg"])
        e = dict(off=dict(off), ni=ni, ng=ng, levels=levels,
                 Akk=[Aii[l][:, l].toarray() for l in levels],
                 Ck=[Aii[levels[k + 1]][:, levels[k]].toarray() for k in range(len(levels) - 1)],
                 B=Aig[levels[0]].toarray() if levels else np.zeros((0, ng)), G=Agg.toarray())
        out.append(e)
        off["ii"] += c.A_II.nnz; off["ig"] += c.A_IΓ.nnz; off["gg"] += c.A_ΓΓ.nnz
        off["bi"] += ni; off["s"] += ng * ng; off["w"] += ng
    return out, off


def dense_from_list(doc, e0, e1, nr, nc):
    src, dst = np.array(doc["src"][e0:e1], dtype=np.int64), np.array(doc["dst"][e0:e1], dtype=np.int64)
    assert np.unique(dst).size == dst.size and (dst.size == 0 or (dst.min() >= 0 and dst.max() < nr * nc))
    d = np.zeros(nr * nc)
    d[dst] = src + 1.0
    return d.reshape(nr, nc, order="F"), src


def dense_from_columns(doc, p0, nr, nc):
    cp = np.array(doc["c_ptr"][p0:p0 + nc + 1], dtype=np.int64)
    assert cp.size == nc + 1 and np.all(np.diff(cp) >= 0)
    d, used = np.zeros((nr, nc)), []
    for j in range(nc):
        rows, src = np.array(doc["c_row"][cp[j]:cp[j + 1]], dtype=np.int64), np.array(doc["c_src"][cp[j]:cp[j + 1]], dtype=np.int64)
        assert np.all((rows >= 0) & (rows < nr))
        d[rows, j] = src + 1.0
        used.append((rows, src))
    return d, cp, used


def check_row_form(D, q, nr, nc, cp, dense):
    """block q of the record's row forms against the column form it came from"""
    r0 = D["r_off"][q]
    rp = np.array(D["r_ptr"][r0:r0 + nr + 1], dtype=np.int64)
    assert rp.size == nr + 1 and np.all(np.diff(rp) >= 0) and rp[-1] - rp[0] == cp[-1] - cp[0]
    assert rp[0] == (D["r_ptr"][r0 - 1] if r0 else 0)                       # appended: a block starts where the one before ended
    t = np.zeros((nr, nc))
    for i in range(nr):
        cols, src = np.array(D["r_col"][rp[i]:rp[i + 1]], dtype=np.int64), np.array(D["r_src"][rp[i]:rp[i + 1]], dtype=np.int64)
        assert np.all(np.diff(cols) > 0), "a row's columns ascend"
        assert np.all((cols >= 0) & (cols < nc))
        t[i, cols] = src + 1.0
    assert np.array_equal(t, dense)


def check_plan(doc, cases):
    want, tot = expectation(cases)
    assert doc["status"] == 0 and doc["err"] == "" and doc["ndom"] == len(cases) == len(doc["dom"])
    assert [doc[k] for k in ("n_ii", "n_ig", "n_gg", "n_bi", "n_s", "n_w")] == [tot[k] for k in ("ii", "ig", "gg", "bi", "s", "w")]
    assert len(doc["src"]) == len(doc["dst"]) and len(doc["perm"]) == tot["bi"] and len(doc["c_row"]) == len(doc["c_src"])
    e_at, p_at = 0, 0                                                       # the lists and the column pointers are contiguous
    used_ii, used_ig, used_gg = [], [], []
    for D, e, c in zip(doc["dom"], want, cases):
        o, ni, ng, levels = e["off"], e["ni"], e["ng"], e["levels"]
        assert [D[k] for k in ("ii_val_off", "ig_val_off", "gg_val_off", "bi_off", "s_off", "w_off")] == [o[k] for k in ("ii", "ig", "gg", "bi", "s", "w")]
        assert (D["n_i"], D["n_g"], D["nlev"]) == (ni, ng, len(levels)), c.tag
        widths = [len(l) for l in levels]
        assert D["lev_off"] == [0, *np.cumsum(widths)] and D["max_lev"] == max(widths, default=0)
        perm = np.array(doc["perm"][o["bi"]:o["bi"] + ni], dtype=np.int64)
        nreach = sum(widths)
        for k, l in enumerate(levels):                                      # node for node
            assert np.array_equal(perm[D["lev_off"][k]:D["lev_off"][k + 1]] - o["bi"], l), (c.tag, k)
        assert np.all(perm[nreach:] == 0)
        # entry lists: A_kk of every level, then A_ΓΓ
        assert len(D["d_e0"]) == len(levels) + 1 and (not levels or D["d_e0"][0] == e_at)
        for k, w in enumerate(widths):
            got, src = dense_from_list(doc, D["d_e0"][k], D["d_e0"][k + 1], w, w)
            assert np.array_equal(got, e["Akk"][k]), (c.tag, k)
            used_ii.append(src)
        e_at = D["d_e0"][-1] if levels else e_at
        assert D["g_e0"] == e_at
        got, src = dense_from_list(doc, D["g_e0"], D["g_e1"], ng, ng)
        assert np.array_equal(got, e["G"]), c.tag
        used_gg.append(src)
        e_at = D["g_e1"]
        # column form: C_k, then B; their row forms
        assert len(D["cptr_off"]) == max(len(levels) - 1, 0) and len(D["r_off"]) == len(D["cptr_off"]) + 1
        for k in range(len(levels) - 1):
            assert D["cptr_off"][k] == p_at
            got, cp, cols = dense_from_columns(doc, p_at, widths[k + 1], widths[k])
            assert np.array_equal(got, e["Ck"][k]), (c.tag, k)
            assert all(np.all(np.diff(r) > 0) for r, _ in cols), "a column's rows ascend"
            used_ii += [s for _, s in cols]
            check_row_form(D, k, widths[k + 1], widths[k], cp, got)
            p_at += widths[k] + 1
        assert D["bptr_off"] == p_at
        n0 = widths[0] if widths else 0
        got, cp, cols = dense_from_columns(doc, p_at, n0, ng)
        assert np.array_equal(got, e["B"]), c.tag
        used_ig += [s for _, s in cols]
        check_row_form(D, len(D["r_off"]) - 1, n0, ng, cp, got)
        p_at += ng + 1
        if c.tag.startswith("island") and "neighbour" not in c.tag:
            assert D["lev_off"][D["nlev"]] < D["n_i"]
    assert e_at == len(doc["src"]) and p_at == len(doc["c_ptr"])
    # every stored entry is used once at most; the used ones are all of A_IΓ and A_ΓΓ, and of A_II those inside a level or
    # from a level to the next deeper one (the dense blocks above hold each of them: equal counts close the argument)
    for used, n in ((used_ig, tot["ig"]), (used_gg, tot["gg"])):
        u = np.concatenate(used) if used else np.zeros(0)
        assert np.array_equal(np.sort(u), np.arange(n))
    u = np.concatenate(used_ii) if used_ii else np.zeros(0)
    assert np.unique(u).size == u.size == sum(np.count_nonzero(a) for e in want for a in e["Akk"] + e["Ck"])
    return doc


def normalised(doc, d):
    """subdomain d's record and its part of the plan-wide arrays with the offsets taken out"""
    D = doc["dom"][d]
    e0 = D["d_e0"][0] if D["nlev"] else D["g_e0"]
    ii = slice(e0, D["g_e0"]); gg = slice(D["g_e0"], D["g_e1"])
    p0 = D["cptr_off"][0] if D["cptr_off"] else D["bptr_off"]
    p1 = D["bptr_off"] + D["n_g"] + 1
    cp = np.array(doc["c_ptr"][p0:p1], dtype=np.int64)
    c0, c1, cb = cp[0], cp[-1], doc["c_ptr"][D["bptr_off"]]
    csrc = np.array(doc["c_src"][c0:c1], dtype=np.int64)
    csrc[:cb - c0] -= D["ii_val_off"]; csrc[cb - c0:] -= D["ig_val_off"]
    nreach = D["lev_off"][D["nlev"]]
    perm = np.array(doc["perm"][D["bi_off"]:D["bi_off"] + D["n_i"]], dtype=np.int64)
    perm[:nreach] -= D["bi_off"]
    r_src = np.array(D["r_src"], dtype=np.int64)
    nb = D["r_ptr"][D["r_off"][-1]] if D["r_ptr"] else 0                    # entries of the C_k row forms; B's follow
    r_src[:nb] -= D["ii_val_off"]; r_src[nb:] -= D["ig_val_off"]
    return [D["n_g"], D["n_i"], D["nlev"], D["max_lev"], D["lev_off"], [v - e0 for v in D["d_e0"]], D["g_e0"] - e0, D["g_e1"] - e0,
            [v - p0 for v in D["cptr_off"]], D["bptr_off"] - p0, (np.array(doc["src"][ii]) - D["ii_val_off"]).tolist(),
            (np.array(doc["src"][gg]) - D["gg_val_off"]).tolist(), doc["dst"][e0:D["g_e1"]], perm.tolist(), (cp - c0).tolist(),
            doc["c_row"][c0:c1], csrc.tolist(), D["r_off"], D["r_ptr"], D["r_col"], r_src.tolist()]


# --------------------------------------------------------------------------------------------------- plan mode
@pytest.mark.parametrize("base", [0, 1])
def test_ladders_in_one_plan_and_alone(exe, synth, tmp_path, base):
    cases = synth["ladders"]
    assert len(cases) == 7
    mixed = check_plan(run(exe, tmp_path / "mixed.txt", plan_text([blocks_of(c) for c in cases], base)), cases)
    for d, c in enumerate(cases):
        alone = check_plan(run(exe, tmp_path / f"alone{d}.txt", plan_text([blocks_of(c)], base)), [c])
        assert normalised(alone, 0) == normalised(mixed, d), c.tag


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("group", ["islands", "direct", "empty"])
def test_islands_single_levels_and_an_empty_interior(exe, synth, tmp_path, group, base):
    cases = synth[group]
    for sub in ([cases] if group == "islands" else [[c] for c in cases]):
        doc = check_plan(run(exe, tmp_path / "case.txt", plan_text([blocks_of(c) for c in sub], base)), sub)
        if group == "islands":
            D = doc["dom"][0]
            assert D["lev_off"][D["nlev"]] == D["n_i"] - 9 and doc["dom"][1]["lev_off"][2] == doc["dom"][1]["n_i"]
        if group == "empty":
            assert doc["dom"][0]["nlev"] == 0 and doc["n_bi"] == 0 and doc["c_ptr"] == [0] * 6


def outside(what, v, hi):
    return f"{what}: index {v} outside [0, {hi})"


@pytest.mark.parametrize("base", [0, 1])
def test_refusals(exe, tmp_path, base):
    good = ss.ladder([3, 4, 5], degree=2, n_gamma=4, seed=11)
    ni, ng = good.A_IΓ.shape

    def refused(blocks, text, **kw):
        doc = run(exe, tmp_path / "bad.txt", plan_text(blocks, base, **kw))
        assert doc["status"] == BAD_ARG and doc["err"] == text, doc

    ok = [np.array(a, dtype=np.int64) for a in blocks_of(good)]
    assert run(exe, tmp_path / "good.txt", plan_text([ok], base))["status"] == 0
    # a row index out of range in each block (A_II: in a column the levels reach, which is every column here)
    for q, what, hi, bad in ((1, "A_II rowval", ni, ni), (3, "A_IΓ rowval", ni, -1), (5, "A_ΓΓ rowval", ng, ng + 3)):
        b = [a.copy() for a in ok]
        b[q][b[q].size // 2] = bad
        refused([b], outside(what, bad, hi))
        refused([ok, b], outside(what, bad, hi))                            # ... and in a later subdomain
    # one entry of a symmetric pair across two levels removed: chain 0 - 1 - 2 - 3 from Γ and the entry (0, 3) without (3, 0)
    A = sp.lil_matrix((4, 4))
    for i in range(4):
        A[i, i] = 4.0
    for i in range(3):
        A[i, i + 1] = A[i + 1, i] = -1.0
    A[0, 3] = -1.0
    A, B, G = sp.csc_matrix(A), sp.csc_matrix(([1.0], ([0], [0])), shape=(4, 1)), sp.csc_matrix([[2.0]])
    refused([[A.indptr, A.indices, B.indptr, B.indices, G.indptr, G.indices]],
            "setup plan: A_II is not block tridiagonal over the BFS levels (not symmetric?)")
    # sizes and column pointers
    refused([ok], "setup plan: negative size", n_i=[-1])
    refused([ok], "setup plan: negative size", n_g=[-2])
    for q in (0, 2, 4):
        b = [a.copy() for a in ok]
        b[q][-1] = -1                                                       # ends below where it starts
        refused([b], "setup plan: bad colptr")


# --------------------------------------------------------------------------------------------------- split mode
@pytest.fixture(scope="module")
def mats(fem):
    cs = lr.gpu_cases(fem, which=("micro", "unstructured"))
    out = {k: sp.csc_matrix(c.A) for k, c in cs.items()}
    out["tridiag"] = sp.csc_matrix(sparse_synth.tridiag(300))
    return out


def check_split(exe, tmp_path, A, nb, base, seeds=None):
    A = sp.csc_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    want_G = bjr.default_seeds(A, nb) if seeds is None else [np.asarray(s) for s in seeds]
    shapes = bjr.shapes(A, nb, want_G)                                      # asserts that every node is reached
    text = [f"1 {n} {nb} {base} {0 if seeds is None else 1}", arr(A.indptr, base), arr(A.indices, base)]
    if seeds is not None:
        text += [arr(np.concatenate([[0], np.cumsum([len(s) for s in seeds])]), base), arr(np.concatenate(seeds), base)]
    doc = run(exe, tmp_path / "split.txt", "\n".join(text) + "\n")
    assert doc["status"] == 0 and doc["err"] == ""
    for d, (lo, hi) in enumerate(bjr.slices(n, nb)):
        assert doc["G"][d] == list(want_G[d]), (nb, d)
        assert doc["I"][d] == list(np.setdiff1d(np.arange(hi - lo), want_G[d]))
        assert doc["ncomp"][d] == csgraph.connected_components(A[lo:hi, lo:hi], directed=False)[0] == shapes[d][3]
        widths = np.diff(doc["lev_off"][d])
        assert widths.sum() == doc["n_i"][d] == len(doc["I"][d]), "a node of the block is not reached"
        I, levels = bjr.split(A[lo:hi, lo:hi], want_G[d])
        assert list(widths) == [len(l) for l in levels] and (len(levels), max(widths, default=0)) == shapes[d][1:3]


@pytest.mark.parametrize("name,nb", [("micro", 1), ("micro", 4), ("micro", 2), ("micro", 7), ("unstructured", 3), ("tridiag", 1)])
def test_default_seeds_and_levels_of_the_split(exe, mats, tmp_path, name, nb):
    check_split(exe, tmp_path, mats[name], nb, base=nb % 2)


def test_explicit_seeds_of_the_split(exe, tmp_path):
    A, seeds = bjr.ladder_matrix([5, 7, 3], n_gamma=4, seed=2)
    for base in (0, 1):
        check_split(exe, tmp_path, A, 1, base, seeds=[seeds])
