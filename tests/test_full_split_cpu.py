"""Host assertions (no GPU) on csrc/full_split_plan.hpp, the interior/Γ split that the LORASC and the Neumann-Neumann induced
operator share, through tests/cpp/full_split_check.cpp:

  * a hand-written micro case (3 subdomains, 5 Γ nodes, a Γ node with two holders and no segment, a subdomain without
    interior): every array of the plan written out literally, in the gathered and in the identity form;
  * the cases of tests/full_synth.py in both forms and both index bases against a numpy construction written here (sorting,
    not the header's counting fill), and the properties the kernels rely on: segments per Γ node, ascending subdomains, every
    stored entry once per form, ascending columns per row, r_gam = gather[d][r_loc - goff[d]], the permutation;
  * the invariant that lets one builder serve both operators: the gathered plan of (A_IΓdd, gather_idx) and the identity plan
    of the scattered A_IΓd agree entry for entry in the column form and in r_ptr, and row by row in the row form once a row's
    entries are ordered by Γ node (the gathered form orders them by LOCAL column, as the induced apply always has: the gather
    lists of full_synth are shuffled, so the two orders differ inside a row with several entries; on the micro case, whose
    gather lists ascend, the row forms agree entry for entry);
  * every refusal: a non-zero status and a message of more than 40 characters that names the offender;
  * the same checker as a stand-alone program under -fsanitize=address,undefined on the micro case and on every refusal."""
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import full_synth as fs
from conftest import ROOT

CASES = ("w1", "w3", "hub6", "bare", "wg1", "wg255", "wg256", "tiles")
ARRAYS = ("pos_I", "pos_g", "gseg_ptr", "seg_ptr", "c_row", "c_src", "r_ptr", "r_loc", "r_gam", "r_src", "voff", "ioff", "goff")
SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def _build(tmp, flags=()):
    exe = str(tmp / ("full_split_check" + ("_san" if flags else "")))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", *flags, "-o", exe, os.path.join(ROOT, "tests", "cpp", "full_split_check.cpp")])
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("full_split"))


@pytest.fixture(scope="module")
def sanitized_checker(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("full_split_san"), SANITIZE)


class Split:
    """one input of make_plan, everything 0-based; `write` adds the index base"""

    def __init__(self, mats, pos_I, pos_g, gather=None, cnt=None, n=None):
        self.ptr = [np.asarray(sp.csc_matrix(M).indptr, dtype=np.int64) for M in mats]
        self.idx = [np.asarray(sp.csc_matrix(M).indices, dtype=np.int64) for M in mats]
        self.val = [np.asarray(sp.csc_matrix(M).data, dtype=np.float64) for M in mats]
        self.pos_I, self.pos_g = [np.asarray(p, dtype=np.int64) for p in pos_I], np.asarray(pos_g, dtype=np.int64)
        self.n_i = [int(p.size) for p in self.pos_I]
        self.plan_n_i = list(self.n_i)
        self.gather = None if gather is None else [np.asarray(g, dtype=np.int64) for g in gather]
        self.cnt = None if cnt is None else np.asarray(cnt, dtype=np.int64)
        self.n_gd = None if gather is None else [int(g.size) for g in self.gather]
        self.plan_n_gd = None if gather is None else list(self.n_gd)
        self.n = sum(self.n_i) + self.pos_g.size if n is None else n
        self.val_null = [0] * len(mats)

    @property
    def ndom(self):
        return len(self.ptr)

    def nodes(self, d):
        return np.arange(self.pos_g.size) if self.gather is None else self.gather[d]

    def write(self, path, base=0):
        def arr(a, shift=0):
            a = np.asarray(a, dtype=np.int64).ravel()
            return " ".join(str(v) for v in [a.size, *(a + shift)])
        rows = [f"{self.ndom} {self.n} {self.pos_g.size} {base} {int(self.gather is not None)}", arr(self.n_i), arr(self.plan_n_i)]
        if self.gather is not None:
            rows += [arr(self.n_gd), arr(self.plan_n_gd)]
        rows += [arr(p, base) for p in self.pos_I] + [arr(self.pos_g, base)]
        if self.gather is not None:
            rows += [arr(g, base) for g in self.gather] + [arr(self.cnt)]
        for d in range(self.ndom):
            rows += [arr(self.ptr[d], base), arr(self.idx[d], base), str(self.val_null[d])]
        path.write_text("\n".join(rows) + "\n")
        return path


def run(exe, path):
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    doc = json.loads(r.stdout.splitlines()[0])
    for k in ARRAYS:
        doc[k] = np.asarray(doc[k], dtype=np.int64)
    return doc


def plan_of(exe, tmp_path, s, base=0, tag="case"):
    doc = run(exe, s.write(tmp_path / f"{tag}_{base}.txt", base))
    assert doc["status"] == 0 and doc["err"] == "", doc["err"]
    return doc


def expected(s):
    """the plan from sorting: independent of the header's counting fills"""
    ndom, n_g = s.ndom, s.pos_g.size
    voff = np.concatenate(([0], np.cumsum([i.size for i in s.idx])))
    ioff = np.concatenate(([0], np.cumsum(s.n_i)))
    goff = np.zeros(ndom + 1, dtype=np.int64) if s.gather is None else np.concatenate(([0], np.cumsum(s.n_gd)))
    d_of, col, row, src = [], [], [], []
    for d in range(ndom):
        c = np.repeat(np.arange(s.ptr[d].size - 1), np.diff(s.ptr[d]))
        d_of.append(np.full(c.size, d)); col.append(c); row.append(ioff[d] + s.idx[d]); src.append(voff[d] + np.arange(c.size))
    d_of, col, row, src = (np.concatenate(a).astype(np.int64) for a in (d_of, col, row, src))
    gam = np.concatenate([s.nodes(d)[col[d_of == d]] for d in range(ndom)]).astype(np.int64) if src.size else src
    by_col = np.lexsort((src, d_of, gam))                   # Γ node, then subdomain, then stored order
    new_seg = np.r_[True, (gam[by_col][1:] != gam[by_col][:-1]) | (d_of[by_col][1:] != d_of[by_col][:-1])] if src.size else np.zeros(0, bool)
    seg_start = np.flatnonzero(new_seg)
    by_row = np.lexsort((col, row))                         # interior row, then stored column of its subdomain
    return dict(pos_I=np.concatenate(s.pos_I), pos_g=s.pos_g,
                gseg_ptr=np.concatenate(([0], np.cumsum(np.bincount(gam[by_col][seg_start], minlength=n_g)))),
                seg_ptr=np.r_[seg_start, src.size], c_row=row[by_col], c_src=src[by_col],
                r_ptr=np.concatenate(([0], np.cumsum(np.bincount(row, minlength=int(ioff[-1]))))),
                r_loc=(goff[d_of] + col)[by_row], r_gam=gam[by_row], r_src=src[by_row], voff=voff, ioff=ioff, goff=goff)


def assert_plan(doc, want, what):
    for k in ARRAYS:
        assert doc[k].shape == np.asarray(want[k]).shape and np.array_equal(doc[k], want[k]), (what, k, doc[k][:20], np.asarray(want[k])[:20])


# ------------------------------------------------------------------ the micro case, written out
def micro(gathered=True):
    A0 = sp.csc_matrix((np.array([1.0, 2.0, 3.0]), np.array([0, 1, 1]), np.array([0, 2, 2, 3])), shape=(2, 3))    # column 1 empty
    A1 = sp.csc_matrix((0, 2))
    A2 = sp.csc_matrix((np.array([4.0, 5.0, 6.0, 7.0]), np.array([0, 2, 0, 1]), np.array([0, 2, 3, 4])), shape=(3, 3))
    gather = ([0, 1, 2], [1, 3], [2, 3, 4])
    pos_I, pos_g = ([7, 2], [], [9, 0, 4]), [5, 1, 8, 3, 6]
    if gathered:
        return Split([A0, A1, A2], pos_I, pos_g, gather, [1, 2, 2, 2, 1])
    return Split([fs.scatter_columns(A, g, 5) for A, g in zip((A0, A1, A2), gather)], pos_I, pos_g)


MICRO = dict(pos_I=[7, 2, 9, 0, 4], pos_g=[5, 1, 8, 3, 6], gseg_ptr=[0, 1, 1, 3, 4, 5], seg_ptr=[0, 2, 3, 5, 6, 7],
             c_row=[0, 1, 1, 2, 4, 2, 3], c_src=[0, 1, 2, 3, 4, 5, 6], r_ptr=[0, 1, 3, 5, 6, 7], r_loc=[0, 0, 2, 5, 6, 7, 5],
             r_gam=[0, 0, 2, 2, 3, 4, 2], r_src=[0, 1, 2, 3, 5, 6, 4], voff=[0, 3, 3, 7], ioff=[0, 2, 2, 5], goff=[0, 3, 5, 8])


@pytest.mark.parametrize("base", [0, 1])
def test_micro_case_literally(checker, tmp_path, base):
    """Γ node 1 has two holders (subdomains 0 and 1) and no segment; subdomain 1 has no interior and no entries"""
    doc = plan_of(checker, tmp_path, micro(), base, "micro")
    assert (doc["n_I"], doc["n_g"], doc["nnz"], doc["totg"]) == (5, 5, 7, 8)
    assert_plan(doc, MICRO, "micro, gathered form")
    assert_plan(doc, expected(micro()), "micro, gathered form, numpy construction")
    ident = plan_of(checker, tmp_path, micro(False), base, "micro_identity")
    assert (ident["n_I"], ident["n_g"], ident["nnz"], ident["totg"]) == (5, 5, 7, 5)
    want = dict(MICRO, r_loc=MICRO["r_gam"], goff=[0, 0, 0, 0])          # identity form: the local vector is the Γ vector
    assert_plan(ident, want, "micro, identity form")


# ------------------------------------------------------------------ the synthetic partitions
def splits_of(c):
    sub = c.P.sub
    return (Split(c.P.A_IΓdd, c.pos_I, c.pos_Γ, sub.gather_idx, sub.node_Γ_cnt), Split(c.A_IΓd, c.pos_I, c.pos_Γ))


@pytest.fixture(scope="module")
def plans(checker, tmp_path_factory):
    """(gathered, identity) plan of every case at index base 0, with their inputs"""
    tmp = tmp_path_factory.mktemp("full_split_cases")
    out = {}
    for name in CASES:
        sg, si = splits_of(fs.case(name))
        out[name] = (sg, plan_of(checker, tmp, sg, 0, name + "_g"), si, plan_of(checker, tmp, si, 0, name + "_i"))
    return out


@pytest.mark.parametrize("name", CASES)
def test_synthetic_cases_against_numpy_in_both_forms_and_bases(checker, tmp_path, plans, name):
    sg, pg, si, pi = plans[name]
    for s, p, form in ((sg, pg, "gathered"), (si, pi, "identity")):
        assert_plan(p, expected(s), f"{name} {form}")
        assert_plan(plan_of(checker, tmp_path, s, 1, form), p, f"{name} {form}, index base 1 against 0")


@pytest.mark.parametrize("name", CASES)
def test_properties_the_kernels_rely_on(plans, name):
    c = fs.case(name)
    sg, pg, si, pi = plans[name]
    for s, p in ((sg, pg), (si, pi)):
        nnz = int(p["nnz"])
        assert np.array_equal(np.diff(p["gseg_ptr"]), fs.column_segments(c))
        seg_dom = np.searchsorted(p["voff"], p["c_src"][p["seg_ptr"][:-1]], side="right") - 1
        for g in range(c.n_Γ):
            d = seg_dom[p["gseg_ptr"][g]:p["gseg_ptr"][g + 1]]
            assert np.all(np.diff(d) > 0), (name, g, d)
        assert np.array_equal(np.sort(p["c_src"]), np.arange(nnz)) and np.array_equal(np.sort(p["r_src"]), np.arange(nnz))
        inner = np.ones(nnz, dtype=bool)
        inner[p["r_ptr"][:-1][np.diff(p["r_ptr"]) > 0]] = False           # first entry of every non-empty row
        assert np.all(np.diff(p["r_loc"])[inner[1:]] > 0)
        dom = np.searchsorted(p["voff"], p["r_src"], side="right") - 1
        assert np.array_equal(p["r_gam"], np.array([s.nodes(d)[l - p["goff"][d]] for d, l in zip(dom, p["r_loc"])], dtype=np.int64))
        perm = np.concatenate([p["pos_I"], p["pos_g"]])
        assert np.array_equal(perm, np.concatenate(list(c.pos_I) + [c.pos_Γ])) and np.array_equal(np.sort(perm), np.arange(c.n))
    print(f"{name}: nnz {int(pg['nnz'])}, longest row {int(max(np.diff(pg['r_ptr'])))}, most segments {int(max(np.diff(pg['gseg_ptr'])))}")


def by_node_within_rows(p, val):
    """the row form with every row's entries ordered by Γ node: (r_gam, val[r_src])"""
    row = np.repeat(np.arange(p["r_ptr"].size - 1), np.diff(p["r_ptr"]))
    order = np.lexsort((p["r_gam"], row))
    return p["r_gam"][order], val[p["r_src"]][order]


@pytest.mark.parametrize("name", CASES + ("micro",))
def test_gathered_and_identity_plans_agree(checker, tmp_path, plans, name):
    if name == "micro":
        sg, si = micro(), micro(False)
        pg, pi = plan_of(checker, tmp_path, sg, 0, "g"), plan_of(checker, tmp_path, si, 0, "i")
    else:
        sg, pg, si, pi = plans[name]
    val_g, val_i = np.concatenate(sg.val), np.concatenate(si.val)
    for k in ("gseg_ptr", "seg_ptr", "c_row", "r_ptr"):
        assert np.array_equal(pg[k], pi[k]), (name, k)
    assert np.array_equal(val_g[pg["c_src"]], val_i[pi["c_src"]])
    for a, b in zip(by_node_within_rows(pg, val_g), by_node_within_rows(pi, val_i)):
        assert np.array_equal(a, b), name
    if all(np.all(np.diff(g) > 0) for g in sg.gather):                   # ascending gather lists: local order is Γ order
        assert np.array_equal(pg["r_gam"], pi["r_gam"]) and np.array_equal(val_g[pg["r_src"]], val_i[pi["r_src"]])
    else:
        assert name != "micro"


# ------------------------------------------------------------------ refusals
def refusals():
    """name -> (input, substrings of the message); every one starts from the micro case"""
    out = {}

    def case(name, needs, gathered=True):
        s = micro(gathered)
        out[name] = (s, needs)
        return s
    s = case("duplicated position", ("permutation", "7"))
    s.pos_I[2][0] = s.pos_I[0][0]
    s = case("position out of range", ("out of range", "pos_gamma", "10"))
    s.pos_g[3] = s.n
    s = case("n off by one", ("n_gamma", "11", "10"))
    s.n += 1
    s = case("moved interior node", ("n_i[0] = 3", "2"))
    s.pos_I = [np.r_[s.pos_I[0], s.pos_I[2][:1]], s.pos_I[1], s.pos_I[2][1:]]
    s.n_i = [3, 0, 2]
    s = case("short n_gamma_d", ("n_gamma_d[0] = 2", "3"))
    s.gather[0], s.n_gd[0], s.ptr[0], s.idx[0] = s.gather[0][:2], 2, s.ptr[0][:3], s.idx[0][:2]
    s.cnt = np.array([1, 2, 1, 2, 1])
    s = case("repeated gather index", ("gather_idx[2]", "repeats", "2"))
    s.gather[2][1] = 2
    s = case("gather index out of range", ("gather_idx[2][1]", "5"))
    s.gather[2][1] = 5
    s = case("wrong cnt", ("node_gamma_cnt[3] = 3", "2 subdomain"))
    s.cnt[3] += 1
    for gathered in (True, False):
        form = "gathered" if gathered else "identity"
        s = case(f"colptr[0] != base, {form}", ("ig_colptr[2][0] = 1", "index_base"), gathered)
        s.ptr[2] = s.ptr[2] + 1
        s = case(f"decreasing colptr, {form}", ("ig_colptr[0]", "decreases"), gathered)
        s.ptr[0][1] = 4 if gathered else 9
        s = case(f"row out of range, {form}", ("ig_rowval[2]", "out of range", "row 3", "n_i = 3"), gathered)
        s.idx[2][1] = 3
        s = case(f"NULL values, {form}", ("ig_nzval [0]", "NULL"), gathered)
        s.val_null[0] = 1
    return out


REFUSALS = refusals()


@pytest.mark.parametrize("name", sorted(REFUSALS))
@pytest.mark.parametrize("base", [0, 1])
def test_refusals_name_the_offender(checker, tmp_path, name, base):
    s, needs = REFUSALS[name]
    doc = run(checker, s.write(tmp_path / "refused.txt", base))
    print(f"{name}: {doc['err']}")
    assert doc["status"] != 0 and len(doc["err"]) > 40
    if base == 0:
        for t in needs:
            assert t in doc["err"], (name, t, doc["err"])
    assert all(doc[k].size == 0 for k in ARRAYS)


def test_sanitized_checker_runs_clean(sanitized_checker, checker, tmp_path):
    """the stand-alone program under the address and undefined-behaviour sanitizers: the micro case in both forms and bases,
    one synthetic case, and every refusal; the same output as the plain build"""
    files = [micro().write(tmp_path / "m0.txt", 0), micro().write(tmp_path / "m1.txt", 1), micro(False).write(tmp_path / "i0.txt", 0),
             micro(False).write(tmp_path / "i1.txt", 1)]
    files += [s.write(tmp_path / f"hub6_{k}.txt", k) for k, s in enumerate(splits_of(fs.case("hub6")))]
    files += [s.write(tmp_path / f"r{k}_{base}.txt", base) for k, (s, _) in enumerate(REFUSALS.values()) for base in (0, 1)]
    got = subprocess.run([sanitized_checker, *map(str, files)], capture_output=True, text=True, timeout=600)
    assert got.returncode == 0 and got.stderr == "", got.stdout[-2000:] + got.stderr[-4000:]
    plain = subprocess.run([checker, *map(str, files)], capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0 and got.stdout == plain.stdout and len(got.stdout.splitlines()) == len(files)
