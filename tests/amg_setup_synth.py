"""The numeric set-up chain of csrc/amg_setup.hpp restated in the device's own order of operations, and synthetic matrices
with frozen aggregates that put each of its kernels on an edge (k_as_gersh, k_as_omega, k_as_prolong, k_as_gather,
k_as_product, k_as_sym, k_as_dense, k_as_sym_dense; the symbolic side is csrc/amg_plan.hpp).

Not a conftest: tests/test_amg_setup_edges_cpu.py and tests/test_gpu_amg_setup_edges.py import it. Everything runs on the host,
with numpy and scipy alone.

The restatement (`setup_bits`), per smoothed level, as the header and DESIGN §6g "Summation orders" state it (the build has
-ffp-contract=off: a product and a sum are two roundings; every division is a true fp64 division):
    sum_i = Σ_k |a_ik|              left to right in CSR order from +0.0
    ratio_i = sum_i / a_ii,  g = max(0, max_i ratio_i)      (the maximum is order-free)
    ω = 4.0 / (3.0 g),  wd_i = ω / a_ii
    tw[J] = 1.0 / sqrt(|agg J|)
    P[i, J] = (J == agg(i) ? tw[J] : 0.0) − wd_i s,  s = Σ (a_ik tw[J]) over the stored k of row i with agg(col k) = J, in
              ascending column from +0.0; the pattern is pattern(T) ∪ pattern(A T), structural
    (A P)[i, J] = Σ_q a_iq P[col q, J]   in ascending q from +0.0; a (col q, J) that P does not store adds nothing; the
              pattern is the full structural product
    M[I, J] = Σ_i R[I, i] (A P)[i, J]    in ascending i, R = P' with the same values
    A_{l+1}[I, J] = (M[I, J] + M[J, I]) * 0.5
Every ordered sum is vectorised by the position within its group: pass t adds the t-th term of every group that long, so the
order inside a group is left to right and the cost is the number of terms. No `@`, `np.sum` or `reduceat` touches a sum
whose order matters. A term that a seeded fault drops is replaced by +0.0: a running sum that starts at +0.0 never turns
-0.0, so adding +0.0 leaves every bit as it was, exactly like not adding.

`setup_ld` is the same chain in np.longdouble with scipy's own sums, level by level from the restatement's own A_l (and its
P_l for the Galerkin product), the reference `amg_refresh_ref.level_bounds` is measured against (`check_ld`).

DEFECTS, for `setup_bits(..., defect=)`; each states one way a kernel of the chain could be wrong:
    omega_tail        the workgroup partials with index >= 256 are not looked at (k_as_omega without its second pass)
    gersh_wave        the rows of the last wave (threads 192 .. 255) of a row block of 256 are left out of the block's maximum
    gersh_last_block  the rows past the last whole block of 256 are left out
    seg_short         every prolongator segment loses its last entry
    search_last       the search in a right-hand row cannot find that row's last entry
    search_first      the search in a right-hand row cannot find that row's first entry
    sym_half          A_{l+1} = M, without the mirrored half
"""
from __future__ import annotations

import dataclasses

import numpy as np
import scipy.sparse as sp

import amg_refresh_ref as rr

NT = 256                       # AS_NT: rows, entries per workgroup
U = rr.U
DEFECTS = ("omega_tail", "gersh_wave", "gersh_last_block", "seg_short", "search_last", "search_first", "sym_half")


@dataclasses.dataclass
class Setup:
    """what the chain leaves per level: A (nlev), P, AP, M (the unsymmetrised product), ω, g, ω/d (nlev - 1 each)"""
    A: list
    P: list
    AP: list
    M: list
    omega: list
    g: list
    wd: list

    @property
    def nlevels(self):
        return len(self.A)

    @property
    def sizes(self):
        return [a.shape[0] for a in self.A]

    @property
    def omega_over_d(self):                 # the name fem.AmgHierarchy gives it (amg_refresh_ref.check_levels reads either)
        return self.wd

    def values(self):
        """every number a read-back sees, as one list of arrays"""
        return ([a.data for a in self.A] + [p.data for p in self.P] + [np.asarray(self.omega, dtype=np.float64)] +
                [np.asarray(w) for w in self.wd])


def same(a: Setup, b: Setup):
    """bit-equal in everything a read-back sees (A_l, P_l, ω, ω/d)"""
    va, vb = a.values(), b.values()
    return len(va) == len(vb) and all(np.array_equal(x, y) for x, y in zip(va, vb))


def sorted_csr(M):
    M = sp.csr_matrix(M).copy()
    M.sum_duplicates()
    M.sort_indices()
    return M


# ------------------------------------------------------------------ ordered sums
def _ordered(v, start, ln):
    """out[g] = v[start[g]] + v[start[g] + 1] + ... (ln[g] terms), left to right from +0.0"""
    out = np.zeros(ln.size, dtype=v.dtype)
    m = int(ln.max(initial=0))
    by = np.argsort(-ln, kind="stable")
    longer = np.searchsorted(-ln[by], -np.arange(m), side="left")     # groups with ln > t
    for t in range(m):
        rows = by[:longer[t]]
        out[rows] = out[rows] + v[start[rows] + t]
    return out


def _grouped(v, key):
    """(keys, sums): the distinct keys ascending, and per key the sum of its terms in the order given"""
    order = np.argsort(key, kind="stable")
    ks = key[order]
    new = np.ones(ks.size, dtype=bool)
    new[1:] = ks[1:] != ks[:-1]
    start = np.flatnonzero(new)
    ln = np.diff(np.append(start, ks.size))
    return ks[new], _ordered(v[order], start, ln)


def _ptr(rows, n):
    return np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=n)))).astype(np.int64)


def _product(L, R, defect):
    """C = L R on the full structural pattern: c[i, J] = Σ_q l_iq r[col q, J] in ascending q from +0.0 (k_as_product)"""
    nl, ncols = L.shape[0], R.shape[1]
    lptr, lcol, rptr, rcol = (np.asarray(a, dtype=np.int64) for a in (L.indptr, L.indices, R.indptr, R.indices))
    lrow = np.repeat(np.arange(nl, dtype=np.int64), np.diff(lptr))
    rl = np.diff(rptr)[lcol]                                           # length of the right-hand row of every left entry
    le = np.repeat(np.arange(lcol.size, dtype=np.int64), rl)           # the left entry of every term, ascending: (i, q) order
    re = rptr[lcol][le] + (np.arange(le.size, dtype=np.int64) - np.repeat(np.cumsum(rl) - rl, rl))
    term = L.data[le] * R.data[re]
    if defect == "search_last":
        term[re == rptr[lcol[le] + 1] - 1] = 0.0
    if defect == "search_first":
        term[re == rptr[lcol[le]]] = 0.0
    ck, val = _grouped(term, lrow[le] * ncols + rcol[re])
    return sp.csr_matrix((val, ck % ncols, _ptr(ck // ncols, nl)), shape=(nl, ncols))


def transposed(P):
    """R = P' in sorted CSR with the values of P (k_as_gather through the plan's r_from)"""
    P = sp.csr_matrix(P)
    prow = np.repeat(np.arange(P.shape[0], dtype=np.int64), np.diff(P.indptr))
    frm = np.argsort(P.indices, kind="stable")
    return sp.csr_matrix((P.data[frm], prow[frm], _ptr(P.indices, P.shape[1])), shape=(P.shape[1], P.shape[0]))


def _level(A, agg, defect):
    n = A.shape[0]
    nc = int(agg.max()) + 1
    ptr, col, val = A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data
    ln = np.diff(ptr)
    row = np.repeat(np.arange(n, dtype=np.int64), ln)
    # k_as_gersh, k_as_omega
    s = _ordered(np.abs(val), ptr[:-1], ln)
    d = np.zeros(n)
    d[row[col == row]] = val[col == row]                               # a missing diagonal entry reads 0.0
    ratio = s / d
    keep = np.ones(n, dtype=bool)
    if defect == "gersh_wave":
        keep[np.arange(n) % NT >= NT - 64] = False
    if defect == "gersh_last_block":
        keep[(n // NT) * NT:] = False
    if defect == "omega_tail":
        keep[NT * NT:] = False
    g = np.float64(np.fmax.reduce(ratio[keep], initial=0.0))
    omega = np.float64(4.0) / (np.float64(3.0) * g)
    wd = omega / d
    # k_as_prolong on the plan's pattern and segments
    tw = 1.0 / np.sqrt(np.bincount(agg, minlength=nc).astype(np.float64))
    J = agg[col]
    akey = row * nc + J
    term = val * tw[J]
    if defect == "seg_short":
        o = np.argsort(akey, kind="stable")
        last = np.ones(o.size, dtype=bool)
        last[:-1] = akey[o][1:] != akey[o][:-1]
        term[o[last]] = 0.0
    sk, ssum = _grouped(term, akey)
    pk = np.union1d(akey, np.arange(n, dtype=np.int64) * nc + agg)
    seg = np.zeros(pk.size)
    seg[np.searchsorted(pk, sk)] = ssum                                # (a P entry without a segment: T's own, s = +0.0)
    prow, pcol = pk // nc, pk % nc
    pv = np.where(pcol == agg[prow], tw[pcol], 0.0) - wd[prow] * seg
    P = sp.csr_matrix((pv, pcol, _ptr(prow, n)), shape=(n, nc))
    # k_as_gather, k_as_product twice, k_as_sym
    AP = _product(A, P, defect)
    M = _product(transposed(P), AP, defect)
    mrow = np.repeat(np.arange(nc, dtype=np.int64), np.diff(M.indptr))
    mkey = mrow * nc + M.indices
    sym = np.searchsorted(mkey, M.indices.astype(np.int64) * nc + mrow)
    assert np.array_equal(mkey[np.minimum(sym, mkey.size - 1)], M.indices.astype(np.int64) * nc + mrow), "the product pattern is not symmetric"
    nxt = M.data.copy() if defect == "sym_half" else (M.data + M.data[sym]) * 0.5
    return P, AP, M, sp.csr_matrix((nxt, M.indices.copy(), M.indptr.copy()), shape=(nc, nc)), omega, g, wd


def setup_bits(A0, aggs, defect=None) -> Setup:
    """the hierarchy of `A0` (sorted CSR, structurally symmetric) on the frozen aggregates `aggs` (one 0-based array per
    smoothed level) in the device's order of operations; `defect`: one of DEFECTS"""
    assert defect is None or defect in DEFECTS, defect
    A = sorted_csr(A0)
    out = Setup([A], [], [], [], [], [], [])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for agg in aggs:
            agg = np.asarray(agg, dtype=np.int64).ravel()
            assert agg.size == out.A[-1].shape[0]
            P, AP, M, nxt, omega, g, wd = _level(out.A[-1], agg, defect)
            out.P.append(P); out.AP.append(AP); out.M.append(M); out.A.append(nxt)
            out.omega.append(float(omega)); out.g.append(float(g)); out.wd.append(wd)
    return out


# ------------------------------------------------------------------ the longdouble reference
def setup_ld(A0, aggs, bits: Setup | None = None):
    """per smoothed level, in np.longdouble with scipy's own sums, from the restatement's own A_l (and, for the Galerkin
    product, its P_l — as amg_refresh_ref.level_bounds takes them): dict(g, omega, wd, P, G) with G = sym(P_l' A_l P_l)"""
    ld = np.longdouble
    bits = bits or setup_bits(A0, aggs)
    out = []
    for l, agg in enumerate(aggs):
        agg = np.asarray(agg, dtype=np.int64).ravel()
        Al, Pb = bits.A[l].astype(ld), bits.P[l].astype(ld)
        n, nc = Pb.shape
        d = Al.diagonal()
        g = np.max(np.asarray(abs(Al).sum(axis=1)).ravel() / d)
        w = ld(4.0) / (ld(3.0) * g)
        wd = w / d
        T = sp.csr_matrix((ld(1.0) / np.sqrt(np.bincount(agg, minlength=nc).astype(ld))[agg], (np.arange(n), agg)), shape=(n, nc))
        P = sp.csr_matrix(T - sp.diags(wd) @ (Al @ T))
        M = sp.csr_matrix(Pb.T @ Al @ Pb)
        out.append(dict(g=g, omega=w, wd=wd, P=P, G=sp.csr_matrix((M + M.T) * ld(0.5))))
    return out


def _on_pattern(V, S):
    """rr.on_pattern for a matrix of any float type"""
    V, S = sorted_csr(V), sp.csr_matrix(S)
    kv, ks = rr.keys(V), rr.keys(S)
    pos = np.searchsorted(ks, kv)
    assert pos.size == 0 or (pos.max() < ks.size and np.array_equal(ks[pos], kv)), "an entry outside the pattern"
    out = np.zeros(ks.size, dtype=V.dtype)
    out[pos] = V.data
    return out


def check_ld(H, aggs, ref, tag, verbose=True):
    """H (a Setup, or a hierarchy read back from the device: .A, .P, .omega, .omega_over_d) against `ref` = setup_ld(...) within
    the entry-wise bounds of amg_refresh_ref.level_bounds; returns the largest fractions used as dict(rel, P, A)"""
    worst = dict(rel=0.0, P=0.0, A=0.0)
    use = lambda d, b: float(np.max(np.divide(d, b, out=np.zeros_like(d), where=b > 0), initial=0.0))
    for l, agg in enumerate(aggs):
        B = rr.level_bounds(H.A[l], H.P[l], np.asarray(agg, dtype=np.int64))
        R = ref[l]
        e_w = float(abs(H.omega[l] - R["omega"]) / R["omega"])
        e_wd = float(np.max(np.abs(H.omega_over_d[l] - R["wd"]) / np.abs(R["wd"])))
        dP = np.abs(H.P[l].data - _on_pattern(R["P"], H.P[l])).astype(np.float64)
        dA = np.abs(H.A[l + 1].data - _on_pattern(R["G"], H.A[l + 1])).astype(np.float64)
        bP, bA = rr.on_pattern(B["P_bound"], H.P[l]), rr.on_pattern(B["G_bound"], H.A[l + 1])
        fr = dict(rel=max(e_w, e_wd) / B["rel"], P=use(dP, bP), A=use(dA, bA))
        if verbose:
            print(f"{tag} level {l}: n = {H.A[l].shape[0]}, kA = {B['kA']}, kR = {B['kR']}; ω, ω/d: {fr['rel']:.3f} of (kA + 2) u; "
                  f"P: {fr['P']:.3f} of its bound; A_{l + 1}: {fr['A']:.4f} of its bound")
        assert e_w <= B["rel"] and e_wd <= B["rel"], (tag, l, e_w, e_wd)
        assert (dP <= bP).all(), (tag, l, "P")
        assert (dA <= bA).all(), (tag, l, "A_next")
        for k in worst:
            worst[k] = max(worst[k], fr[k])
    return worst


# ------------------------------------------------------------------ patterns, values, aggregates
def groups(n, w):
    """aggregates of w consecutive nodes"""
    return np.arange(n, dtype=np.int64) // w


def chain_levels(n, w, stop):
    """aggregates of w consecutive nodes per level until a level has at most `stop` rows"""
    out = []
    while n > stop:
        out.append(groups(n, w))
        n = (n + w - 1) // w
    return out


def pattern(n, I, J):
    """the symmetric pattern with the edges (I, J) and a full diagonal, as a matrix of ones"""
    I, J = np.asarray(I, dtype=np.int64), np.asarray(J, dtype=np.int64)
    assert (I != J).all()
    r, c = np.concatenate((I, J, np.arange(n))), np.concatenate((J, I, np.arange(n)))
    S = sorted_csr(sp.coo_matrix((np.ones(r.size), (r, c)), shape=(n, n)))
    S.data[:] = 1.0
    return S


def chain(n):
    return pattern(n, np.arange(n - 1), np.arange(1, n))


PEAK, SECOND = 1.05, 1.4          # a_ii / Σ_{j != i} |a_ij| of the row with the largest ratio and of the runner-up


def spd_values(S, seed, peak=None, second=None):
    """A symmetric, strictly diagonally dominant matrix on the pattern S: off-diagonal values ±[0.5, 1.5) (a quarter positive),
    a_ii = c_i Σ_{j != i} |a_ij| with c_i in [2.5, 3.5) — the Gershgorin ratio 1 + 1 / c_i then lies in (1.28, 1.4] — but
    c = PEAK at row `peak` (ratio 1.952) and c = SECOND at row `second` (1.714, 12 % lower); a row without a neighbour gets
    a_ii in [1, 2) (ratio exactly 1)."""
    rng = np.random.default_rng(seed)
    n = S.shape[0]
    Up = sp.triu(S, 1).tocoo()
    w = rng.choice([-1.0, 1.0, -1.0, -1.0], size=Up.nnz) * (0.5 + rng.random(Up.nnz))
    W = sp.coo_matrix((w, (Up.row, Up.col)), shape=(n, n)).tocsr()
    W = W + W.T
    off = np.asarray(abs(W).sum(axis=1)).ravel()
    c = 2.5 + rng.random(n)
    if peak is not None:
        assert off[peak] > 0
        c[peak] = PEAK
    if second is not None:
        assert off[second] > 0
        c[second] = SECOND
    d = np.where(off > 0, c * off, 1.0 + rng.random(n))
    A = sorted_csr(W + sp.diags(d))
    assert np.array_equal(A.indptr, S.indptr) and np.array_equal(A.indices, S.indices)
    return A


def ratios(A):
    A = sp.csr_matrix(A)
    return np.asarray(abs(A).sum(axis=1)).ravel() / A.diagonal()


# ------------------------------------------------------------------ the cases
GERSH_ROWS = (0, 63, 64, 191, 192, 255, 256, 1023, 1024)
GERSH_N = 1025
BIG = {"big_65536": (65536, 65535, 1000), "big_65537_hi": (65537, 65536, 300), "big_65537_lo": (65537, 300, 65536),
       "big_76801_hi": (76801, 70000, 5000), "big_76801_lo": (76801, 5000, 70000)}      # n, row of the maximum, of the runner-up
ARROW = {"arrow_1024": (1024, 8), "arrow_1025": (1025, 2), "arrow_2049": (2049, 4)}     # entries of the head row, nodes per aggregate
COARSE_NC = (1, 2, 16, 17, 64, 65)
LEVEL_NC = (255, 256, 257)
SEARCH_K, SEARCH_KH, SEARCH_LO, SEARCH_HI, SEARCH_GAP, SEARCH_X = 1100, 600, 20, 1070, 500, 300
NAMES = (tuple(f"gersh_{r}" for r in GERSH_ROWS) + tuple(BIG) + tuple(ARROW) + ("arrow_seg", "giant", "segments", "search", "one_1", "one_65")
         + tuple(f"coarse_{k}" for k in COARSE_NC) + tuple(f"level_{k}" for k in LEVEL_NC))


def gersh_second(r):
    """the row of the runner-up: two blocks and two waves away from row r"""
    return ((r // NT + 2) % 4) * NT + (r % NT + 128) % NT


def arrow_pattern(n):
    return pattern(n, np.zeros(n - 1, dtype=np.int64), np.arange(1, n))


def arrow_seg():
    """node 0 alone in aggregate 0, its 1024 neighbours 1 .. 1024 in aggregate 1 (one segment of 1024 entries in row 0, an R
    row of 1025), then a chain 1024 - 1025 - ... - 1040 in aggregates of eight"""
    n = 1041
    I = np.concatenate((np.zeros(1024, dtype=np.int64), np.arange(1024, 1040)))
    J = np.concatenate((np.arange(1, 1025), np.arange(1025, 1041)))
    agg = np.concatenate(([0], np.ones(1024, dtype=np.int64), 2 + np.arange(16) // 8))
    return pattern(n, I, J), [agg]


SEG_STAR, SEG_LONE = 20, 9


def segments():
    """a chain of 20 nodes in aggregates of 1, 2, 3, ... nodes (node SEG_LONE = 9 alone in its aggregate: its own segment is
    its diagonal entry; node 1: own aggregate first in its row of P, node 2: last), then a star: node SEG_STAR = 20 with nine
    leaves, all ten in one aggregate — the longest row of the matrix, kA = 10 entries, in one segment"""
    agg = np.array([0, 0, 1, 1, 1, 2, 2, 2, 2, 3, 4, 4, 5, 5, 5, 6, 6, 6, 6, 6] + [7] * 10, dtype=np.int64)
    I = np.concatenate((np.arange(19), np.full(9, SEG_STAR)))
    J = np.concatenate((np.arange(1, 20), np.arange(21, 30)))
    return pattern(30, I, J), [agg]


def search():
    """SEARCH_K aggregates of four nodes: three on a chain (4k - 4k+1 - 4k+2 - 4(k+1)) and a spare s_k = 4k + 3. The head
    s_600 is joined to the spares of the aggregates [20, 1070] but 500 (a P row and AP rows of more than 1025 entries);
    x = s_300 also to s_5, s_500 and s_1090 (columns below, between and above the head's); s_12 - s_14 alone (AP rows
    {12, 14}); s_1080 a leaf of the chain node 4 * 1082 (a P row {1080, 1082}); every other spare alone (P and AP rows of
    one entry, their own segment the diagonal entry)."""
    K = SEARCH_K
    s = lambda k: 4 * k + 3
    I, J = [], []
    for k in range(K):
        I += [4 * k, 4 * k + 1]; J += [4 * k + 1, 4 * k + 2]
        if k + 1 < K:
            I.append(4 * k + 2); J.append(4 * k + 4)
    for k in range(SEARCH_LO, SEARCH_HI + 1):
        if k not in (SEARCH_GAP, SEARCH_KH):
            I.append(s(SEARCH_KH)); J.append(s(k))
    for k in (5, SEARCH_GAP, 1090):
        I.append(s(SEARCH_X)); J.append(s(k))
    I += [s(12), s(1080)]; J += [s(14), 4 * 1082]
    return pattern(4 * K, I, J), [groups(4 * K, 4)]


_cases, _bits = {}, {}


def case(name, fem=None):
    """(A0, A1, aggs) of NAMES: two SPD matrices on one pattern (different jitter, the same peak rows) and the aggregates;
    `giant` (the 1 100-node aggregate of amg_refresh_ref) needs `fem`"""
    if name in _cases:
        return _cases[name]
    kind, _, arg = name.partition("_")
    peak = second = None
    if name == "giant":
        A0, A1, aggs = rr.giant_aggregates(fem)
        _cases[name] = (sorted_csr(A0), sorted_csr(A1), aggs)
        return _cases[name]
    if kind == "gersh":
        peak = int(arg)
        second = gersh_second(peak)
        S, aggs = chain(GERSH_N), [groups(GERSH_N, 8)]
    elif kind == "big":
        n, peak, second = BIG[name]
        S, aggs = chain(n), chain_levels(n, 8, 200)
    elif name in ARROW:
        m, w = ARROW[name]
        S, aggs = arrow_pattern(m), [groups(m, w)]
    elif name == "arrow_seg":
        S, aggs = arrow_seg()
    elif name == "segments":
        S, aggs = segments()
    elif name == "search":
        S, aggs = search()
    elif kind == "one":
        S, aggs = chain(int(arg)), []
    elif kind == "coarse":
        S, aggs = chain(3 * int(arg)), [groups(3 * int(arg), 3)]
    elif kind == "level":
        n = 8 * int(arg)
        S, aggs = chain(n), [groups(n, 8), groups(int(arg), 8)]
    else:
        raise KeyError(name)
    k = NAMES.index(name)
    _cases[name] = (spd_values(S, [31, k], peak, second), spd_values(S, [32, k], peak, second), aggs)
    return _cases[name]


def bits(name, which=0, defect=None, fem=None) -> Setup:
    """setup_bits of matrix `which` (0, 1) of the case, computed once per session"""
    key = (name, which, defect)
    if key not in _bits:
        c = case(name, fem)
        _bits[key] = setup_bits(c[which], c[2], defect)
    return _bits[key]


# ------------------------------------------------------------------ censuses, counted from the patterns
def segment_lengths(A, agg):
    """per entry of P in storage order: the length of its segment (0: T's own entry without a stored a_ij), and whether it is
    the own aggregate of its row"""
    A = sp.csr_matrix(A)
    n, nc = A.shape[0], int(agg.max()) + 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.indptr))
    akey = row * nc + agg[A.indices]
    pk = np.union1d(akey, np.arange(n, dtype=np.int64) * nc + agg)
    ln = np.bincount(np.searchsorted(pk, akey), minlength=pk.size)
    return pk // nc, pk % nc, ln, (pk % nc) == agg[pk // nc]


OUTCOMES = ("first", "last", "interior", "below", "above", "between")
LENGTHS = (1, 2, 1025)           # right-hand rows of exactly 1, exactly 2, at least 1025 entries


def search_census(L, R, C):
    """Every search k_as_product makes for C = L R: one per (entry (i, J) of C, entry q of row i of L), J looked for in row
    col(q) of R. Returns {(length class, outcome): count} for the right-hand rows of the LENGTHS classes; a hit in a row of
    one entry counts as "first"."""
    L, R, C = sp.csr_matrix(L), sp.csr_matrix(R), sp.csr_matrix(C)
    ncols = R.shape[1]
    rptr = R.indptr.astype(np.int64)
    rkey = rr.keys(R)
    rlen = np.diff(rptr)
    lrow = np.repeat(np.arange(L.shape[0], dtype=np.int64), np.diff(L.indptr))
    out = {}
    for cls in LENGTHS:
        sel = np.flatnonzero((rlen[L.indices] >= cls) if cls == LENGTHS[-1] else (rlen[L.indices] == cls))
        cl = np.diff(C.indptr)[lrow[sel]]                                 # searches of every selected left entry
        q = np.repeat(sel, cl)
        e = C.indptr[lrow[q]] + (np.arange(q.size, dtype=np.int64) - np.repeat(np.cumsum(cl) - cl, cl))
        j, J = L.indices[q].astype(np.int64), C.indices[e].astype(np.int64)
        pos = np.searchsorted(rkey, j * ncols + J)
        hit = (pos < rkey.size) & (rkey[np.minimum(pos, rkey.size - 1)] == j * ncols + J)
        lo, hi = rptr[j], rptr[j + 1]
        what = {"first": hit & (pos == lo), "last": hit & (pos == hi - 1) & (pos != lo), "interior": hit & (pos > lo) & (pos < hi - 1),
                "below": ~hit & (pos == lo), "above": ~hit & (pos == hi), "between": ~hit & (pos > lo) & (pos < hi)}
        assert sum(int(m.sum()) for m in what.values()) == q.size
        for k, m in what.items():
            out[(cls, k)] = int(m.sum())
    return out


FEASIBLE = ([(1, o) for o in ("first", "below", "above")] + [(2, o) for o in ("first", "last", "below", "above", "between")] +
            [(1025, o) for o in OUTCOMES])


# ------------------------------------------------------------------ a failure below level 0
BREAK_PAIR = (11, 12)             # two nodes of aggregate 1 (nodes 8 .. 15)


def breakdown(levels):
    """(A0, A_bad, aggs) on chain(256) with aggregates of eight, `levels` = 2 or 3 levels: A0 is SPD; A_bad is A0 with the
    coupling of the two nodes BREAK_PAIR, both in aggregate 1, set to minus three times the diagonal sum of their aggregate.
    Its diagonal is still positive, so level 0 raises nothing, but the matrix is indefinite and entry (1, 1) of level 1 is
    negative: the failure arises in the numbers the device made itself."""
    n = 256
    aggs = [groups(n, 8), groups(32, 8)][:levels - 1]
    A0 = spd_values(chain(n), [33, levels])
    bad = A0.copy()
    u, v = BREAK_PAIR
    big = -3.0 * A0.diagonal()[8:16].sum()
    for i, j in ((u, v), (v, u)):
        k = bad.indptr[i] + int(np.flatnonzero(bad.indices[bad.indptr[i]:bad.indptr[i + 1]] == j)[0])
        bad.data[k] = big
    return A0, bad, aggs


# ------------------------------------------------------------------ comparing a hierarchy read back
def same_csr(X, Y):
    return np.array_equal(X.indptr, Y.indptr) and np.array_equal(X.indices, Y.indices) and np.array_equal(X.data, Y.data)


def same_hierarchy(Ha, Hb):
    """two hierarchies read back from the device, bit for bit, the coarse inverse included"""
    return (Ha.sizes == Hb.sizes and all(same_csr(a, b) for a, b in zip(Ha.A, Hb.A)) and all(same_csr(a, b) for a, b in zip(Ha.P, Hb.P))
            and Ha.omega == Hb.omega and all(np.array_equal(a, b) for a, b in zip(Ha.omega_over_d, Hb.omega_over_d))
            and np.array_equal(Ha.coarse_inv, Hb.coarse_inv))


def compare(H, B: Setup, tag):
    """A hierarchy read back from the device against the restatement: patterns equal (asserted), then every A_l, P_l, (ω/d)_l
    and ω_l under np.array_equal, and A_{l+1} exactly symmetric. Returns (comparisons made, descriptions of those that
    differ); a difference is printed with its first entries."""
    assert list(H.sizes) == B.sizes, (tag, H.sizes, B.sizes)
    n, bad = 0, []

    def values(what, got, want):
        nonlocal n
        n += 1
        got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
        if got.shape != want.shape or not np.array_equal(got, want):
            k = np.flatnonzero(got != want) if got.shape == want.shape else np.zeros(0, dtype=np.int64)
            rel = np.max(np.abs(got[k] - want[k]) / np.maximum(np.abs(want[k]), np.finfo(np.float64).tiny), initial=0.0)
            print(f"{tag}: {what}: {k.size} of {want.size} values differ; first at {k[:6].tolist()}: got {got[k[:3]].tolist()}, "
                  f"want {want[k[:3]].tolist()}; largest relative difference {rel:.3e}")
            bad.append(what)

    for l in range(B.nlevels):
        X, Y = sp.csr_matrix(H.A[l]), B.A[l]
        assert np.array_equal(X.indptr, Y.indptr) and np.array_equal(X.indices, Y.indices), (tag, f"pattern of A_{l}")
        values(f"A_{l}", X.data, Y.data)
        if l:
            n += 1
            if abs(X - X.T).max() != 0.0:
                bad.append(f"A_{l} is not exactly symmetric")
        if l == B.nlevels - 1:
            break
        X, Y = sp.csr_matrix(H.P[l]), B.P[l]
        assert np.array_equal(X.indptr, Y.indptr) and np.array_equal(X.indices, Y.indices), (tag, f"pattern of P_{l}")
        values(f"P_{l}", X.data, Y.data)
        values(f"(ω/d)_{l}", H.omega_over_d[l], B.wd[l])
        values(f"ω_{l}", float(H.omega[l]), B.omega[l])
    return n, bad
