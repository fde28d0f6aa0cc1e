"""The V(1,1) cycle of csrc/amg.hpp restated in the device's own order of operations, and synthetic hierarchies that put
every kernel of the cycle on the edges of the row-block partition (csrc/spmv_blocks.hpp) and of the coarse GEMV.

Not a conftest: tests/test_amg_edges_cpu.py and tests/test_gpu_amg_edges.py import it. Everything runs on the host.

The restatement (`cycle_bits`). Every sparse kernel forms prod[k] = val[k] * gather(col[k]) and one thread sums a row left
to right in stored order from +0.0 (a row longer than the tile: one running sum over the tiles, the same order); the build
has -ffp-contract=off, so a product and a sum are two roundings. The coarse GEMV keeps 64 lane sums (lane q: columns q,
q + 64, ... ascending from +0.0) and folds them with the `__shfl_down` tree of `wave_sum`: for off = 32 .. 1, lanes
[0, off) add lanes [off, 2 off). None of this depends on the partition into row blocks, so the host needs no blocks to
state it; the blocks (`row_blocks`, a port of spmv_row_blocks that test_amg_edges_cpu.py holds to the C++ code) are used by
the deliberately defective variants (`DEFECTS`) and to name the block of a differing entry.

`cycle_ld` is the same cycle in np.longdouble with numpy's own sums, and `bound` the running-error bar against it:
a row sum of L terms of rounded products errs by at most (L + 1) u Σ|prod|, the epilogues add at most two more roundings,
so a stage errs entrywise by (L + 3) u times its output in the absolute-valued cycle (every matrix, ω/d, Z and vector
replaced by its absolute value, every subtraction by an addition). The absolute-valued operators after a stage map that
stage's absolute output to at most the final absolute output â, so entrywise |cycle_bits - cycle_ld| <= 2 u â Σ_s (L_s + 3),
the sum over all stages of all levels, the 2 for the reference's own rounding and the second-order terms. This is the
coarser form of the stage-by-stage bar Σ_s 2 (L_s + 3) u â_s: every â_s carried to the output is replaced by the final â
that dominates it, so the bar is valid and, where one stage has a far longer row than the others, looser than it need be.

The hierarchies need not be Galerkin-consistent: mi_amg_create takes A_l, P_l, ω/d and the inverse as given. `variant`:
"full" random values, ω/d > 0, symmetric Z; "pzp" ω/d = 0, so z = P Z P' b: restrict, coarse, prolong alone; "smooth" Z = 0:
down and post alone (and the restrict / prolong of zeros). Values are ± 2^[-2, 2): normal range, no subnormals.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import scipy.sparse as sp

import sparse_synth as ss

TILE, NT = ss.SPMV_TILE, ss.NT
U = 2.0 ** -52
VARIANTS = ("full", "pzp", "smooth")
# The faults `cycle_bits(..., defect=)` can be given, one per edge:
#   block_last    the last entry of the last row of every row block is dropped
#   long_tail     the last tile of a row longer than the tile is dropped
#   pair_overrun  a paired (even k0) block of an odd count also takes entry k + 1 = k0 + nnz, the half of its last pair that
#                 belongs to the next block, into its last row (read alone, that half changes no result: it must be summed to show)
#   skip_empty    the epilogue of a row without entries never runs: its x, r, b_{l+1} and y keep what the buffer held (zero)
#   coarse_cols   the GEMV ignores the columns past the last full 64
#   coarse_rows   the GEMV ignores the rows past the last full 4 (their y keeps zero)
DEFECTS = ("block_last", "long_tail", "pair_overrun", "skip_empty", "coarse_cols", "coarse_rows")


def sorted_csr(M):
    M = sp.csr_matrix(M).copy()
    M.sort_indices()
    return M


def transposed(P):
    """R = P' in sorted CSR (the library's stable transpose of a sorted P)"""
    return sorted_csr(sp.csr_matrix(P).T)


# ------------------------------------------------------------------ the row blocks (spmv_blocks.hpp)
def row_blocks(indptr, breaks=()):
    """[nb, 4] (r0, r1, k0, k1): spmv_row_blocks"""
    ptr = np.asarray(indptr).tolist()
    n = len(ptr) - 1
    breaks = [int(b) for b in breaks]
    out, r, nb = [], 0, 0
    while r < n:
        while nb < len(breaks) and breaks[nb] <= r:
            nb += 1
        limit = min(breaks[nb], n) if nb < len(breaks) else n
        e = r + 1
        while e < limit and ptr[e + 1] - ptr[r] <= TILE:
            e += 1
        if e < limit and (ptr[e] & 1):
            for back in (1, 2, 3):
                if e - back <= r:
                    break
                if (ptr[e - back] & 1) == 0:
                    e -= back
                    break
        out.append((r, e, ptr[r], ptr[e]))
        r = e
    return np.array(out, dtype=np.int64).reshape(-1, 4)


def block_of_rows(blk, rows):
    """index of the row block of every row"""
    return np.searchsorted(blk[:, 1], np.asarray(rows), side="right")


def xcd_of_blocks(nb):
    """the launch index blockIdx of every row block: b = (bid & 7) * per + (bid >> 3)"""
    per = (nb + 7) >> 3
    bid = np.arange(8 * per)
    b = (bid & 7) * per + (bid >> 3)
    return bid[b < nb], b[b < nb]


# ------------------------------------------------------------------ the restatement
def _limits(M, defect):
    """[start, stop) of the entries each row sums, as the defective variant would take them"""
    ptr = np.asarray(M.indptr, dtype=np.int64)
    start, stop = ptr[:-1].copy(), ptr[1:].copy()
    if defect in ("block_last", "pair_overrun"):
        for r0, r1, k0, k1 in row_blocks(ptr):
            if defect == "block_last" and k1 > k0:
                last = r0 + int(np.flatnonzero(stop[r0:r1] > start[r0:r1])[-1])   # the row that holds entry k1 - 1
                stop[last] -= 1
            if defect == "pair_overrun" and k0 % 2 == 0 and (k1 - k0) % 2 == 1 and k1 - k0 <= TILE and k1 < ptr[-1]:
                stop[r1 - 1] = k1 + 1                                            # the half of the last pair that is not the block's
    if defect == "long_tail":
        ln = stop - start
        long = ln > TILE
        stop[long] = start[long] + ((ln[long] - 1) // TILE) * TILE
    return start, stop


def row_sums(M, g, defect=None):
    """Σ_k val[k] g[col[k]] per row of the sorted CSR M: products first, then every row strictly left to right from +0.0;
    a loop over the position within the row, vectorised over the rows that are that long. The dtype is g's."""
    M = sp.csr_matrix(M)
    g = np.asarray(g)
    prod = M.data.astype(g.dtype) * g[M.indices]
    start, stop = _limits(M, defect)
    ln = stop - start
    order = np.argsort(-ln, kind="stable")
    longer = np.searchsorted(-ln[order], -np.arange(int(ln.max(initial=0))), side="left")   # rows with ln > j
    out = np.zeros(M.shape[0], dtype=g.dtype)
    for j in range(int(ln.max(initial=0))):
        rows = order[:longer[j]]
        out[rows] = out[rows] + prod[start[rows] + j]
    return out


def coarse_bits(Z, b, defect=None):
    """y = Z b as k_amg_coarse sums it: row i reads column i of the column-major Z"""
    n = b.size
    Z = np.asarray(Z)
    ncol = (n // 64) * 64 if defect == "coarse_cols" else n
    a = np.zeros((n, 64), dtype=b.dtype)
    for j0 in range(0, ncol, 64):
        w = min(64, ncol - j0)
        a[:, :w] = a[:, :w] + Z[j0:j0 + w, :].T.astype(b.dtype) * b[j0:j0 + w]
    off = 32
    while off:
        a[:, :off] = a[:, :off] + a[:, off:2 * off]
        off >>= 1
    y = a[:, 0].copy()
    if defect == "coarse_rows":
        y[(n // 4) * 4:] = 0.0                               # rows of the last, partial workgroup never written
    return y


def _written(M, out, defect):
    """skip_empty: the epilogue never runs for a row without entries; what the buffer held (zeros here) stays"""
    if defect == "skip_empty":
        out = out.copy()
        out[np.diff(sp.csr_matrix(M).indptr) == 0] = 0.0
    return out


def cycle_bits(H, b, l=0, defect=None):
    """M^-1 b, the V(1,1) cycle of amg.hpp in the device's order of operations (float64)"""
    b = np.asarray(b, dtype=np.float64)
    if l == H.nlevels - 1:
        return coarse_bits(H.coarse_inv, b, defect)
    A, P, wd = sorted_csr(H.A[l]), sorted_csr(H.P[l]), np.asarray(H.omega_over_d[l], dtype=np.float64)
    R = transposed(P)
    x = wd * b                                                # k_amg_down: the gathered operand and the stored x
    r = b - row_sums(A, x, defect)
    x, r = _written(A, x, defect), _written(A, r, defect)
    bc = _written(R, row_sums(R, r, defect), defect)          # k_amg_restrict
    e = cycle_bits(H, bc, l + 1, defect)
    x = x + row_sums(P, e, defect)                            # k_amg_prolong (an unwritten x[i] is the x[i] + 0 it would write)
    return _written(A, x + wd * (b - row_sums(A, x, defect)), defect)   # k_amg_post


def _plain_rows(M, g):
    """row sums in longdouble by numpy's reduceat (empty rows: zero)"""
    M = sp.csr_matrix(M)
    prod = M.data.astype(np.longdouble) * g[M.indices]
    out = np.zeros(M.shape[0], dtype=np.longdouble)
    full = np.flatnonzero(np.diff(M.indptr) > 0)
    if full.size:
        out[full] = np.add.reduceat(prod, M.indptr[full])
    return out


def cycle_ld(H, b, l=0, absolute=False):
    """the cycle in np.longdouble with plain sums; `absolute`: the absolute-valued cycle of `bound`"""
    f = (lambda v: np.abs(np.asarray(v, dtype=np.longdouble))) if absolute else (lambda v: np.asarray(v, dtype=np.longdouble))
    sgn = 1 if absolute else -1
    b = f(b)
    if l == H.nlevels - 1:
        return f(H.coarse_inv).T @ b
    A, P, wd = sorted_csr(H.A[l]), sorted_csr(H.P[l]), f(H.omega_over_d[l])
    if absolute:
        A, P = abs(A), abs(P)
    x = wd * b
    r = b + sgn * _plain_rows(A, x)
    e = cycle_ld(H, _plain_rows(transposed(P), r), l + 1, absolute)
    x = x + _plain_rows(P, e)
    return x + wd * (b + sgn * _plain_rows(A, x))


def stage_lengths(H):
    """Σ_s (L_s + 3) over the stages: down, restrict, prolong, post per smoothed level, the coarse GEMV"""
    tot = H.sizes[-1] + 3
    for l in range(H.nlevels - 1):
        kA = int(np.diff(sp.csr_matrix(H.A[l]).indptr).max(initial=0))
        kP = int(np.diff(sp.csr_matrix(H.P[l]).indptr).max(initial=0))
        kR = int(np.diff(transposed(H.P[l]).indptr).max(initial=0))
        tot += 2 * (kA + 3) + (kP + 3) + (kR + 3)
    return tot


def bound(H, b):
    """entrywise bar of |cycle - cycle_ld| (module docstring)"""
    return np.asarray(2.0 * U * stage_lengths(H) * cycle_ld(H, b, absolute=True), dtype=np.float64)


# ------------------------------------------------------------------ values, patterns
def _vals(rng, shape):
    return rng.choice([-1.0, 1.0], size=shape) * 2.0 ** rng.uniform(-2.0, 2.0, size=shape)


def _refill(M, rng):
    M = sorted_csr(M)
    M.data = _vals(rng, M.indices.size)
    return M


def _ones(M):
    M = sp.csr_matrix(M)
    return sp.csr_matrix((np.ones(M.indices.size), M.indices.copy(), M.indptr.copy()), shape=M.shape)


def groups(n, w):
    """aggregates of w consecutive rows"""
    return np.arange(n, dtype=np.int64) // w


def p_pattern(S, agg):
    """the structural pattern of a smoothed prolongator: pattern(S T), T the tentative prolongator of `agg`; a row of S
    without entries is a row of P without entries"""
    n, nc = S.shape[0], int(agg.max()) + 1
    T = sp.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, nc))
    return sorted_csr(_ones(_ones(S) @ T))


LONGP_ROW, LONGP_EMPTY = 7, (100, 400)


def long_p(n=2100, nc=1100):
    """row LONGP_ROW holds the columns 0 .. 1024 (TILE + 1 entries), rows [100, 400) none, every other row one"""
    rows = np.arange(n)
    keep = (rows != LONGP_ROW) & ~((rows >= LONGP_EMPTY[0]) & (rows < LONGP_EMPTY[1]))
    I = np.concatenate([np.full(TILE + 1, LONGP_ROW), rows[keep]])
    J = np.concatenate([np.arange(TILE + 1), rows[keep] % nc])
    return sorted_csr(sp.coo_matrix((np.ones(I.size), (I, J)), shape=(n, nc)))


LEAD = 5


def lead_long():
    """LEAD rows (and columns) without entries, then arrow(2100, 1025): the first row block holds LEAD rows and no non-zero,
    the second the long row alone"""
    return sorted_csr(sp.block_diag([sp.csr_matrix((LEAD, LEAD)), ss.arrow(2100, TILE + 1)], format="csr"))


def odd_tail(m=1200):
    """Row 0: its diagonal; then m coupled pairs of rows, two entries each. Every row offset but the first is odd, so no
    row can be given back: the first block is paired (k0 = 0) and ends on an odd count (1023) before the end of the matrix,
    the next starts at an odd offset and fills the tile exactly."""
    return sorted_csr(sp.block_diag([sp.csr_matrix(np.ones((1, 1))), sp.kron(sp.identity(m), np.ones((2, 2)))], format="csr"))


def blocks_len(k):
    """the shortest tridiagonal whose row-block partition has k blocks (its last block holds one row); k = 1: 300 rows"""
    if k == 1:
        return 300
    lo, hi = 1, 400 * k                                       # the count grows with the length: bisection
    while lo < hi:
        mid = (lo + hi) // 2
        if row_blocks(ss.tridiag(mid).indptr).shape[0] >= k:
            hi = mid
        else:
            lo = mid + 1
    return lo


COARSE_N = (1, 3, 4, 5, 63, 64, 65, 130)
BLOCKS_K = (1, 7, 8, 9, 17)
ARROW_M = (1024, 1025, 2049)
NAMES = (("diag1025", "tridiag3000") + tuple(f"arrow_{m}" for m in ARROW_M) + ("odd_start", "holes", "longP", "lead_long", "giant", "three_tiny")
         + tuple(f"coarse1_{n}" for n in COARSE_N) + tuple(f"coarse2_{n}" for n in COARSE_N) + tuple(f"blocks_{k}" for k in BLOCKS_K) + ("odd_tail",))

_cache = {}


def _assemble(fem, As, Ps, rng):
    As = [_refill(A, rng) for A in As]
    Ps = [_refill(P, rng) for P in Ps]
    sizes = [A.shape[0] for A in As]
    assert all(P.shape == (a, c) for P, a, c in zip(Ps, sizes[:-1], sizes[1:]))
    wd = [rng.uniform(0.1, 1.0, size=n) for n in sizes[:-1]]
    nc = sizes[-1]
    G = _vals(rng, (nc, nc))
    Z = np.asfortranarray(np.triu(G) + np.triu(G, 1).T)
    nnz = [A.nnz for A in As]
    return fem.AmgHierarchy(As, Ps, [1.0] * len(Ps), wd, Z, sizes, float(sum(nnz)) / float(nnz[0]), None)


def _two_level(fem, A0, P0, rng):
    return _assemble(fem, [A0, ss.diag(P0.shape[1])], [P0], rng)


def hierarchy(fem, name, variant="full"):
    """the hierarchy `name` of NAMES in one of VARIANTS (one-level hierarchies: "full" alone)"""
    key = (name, variant)
    if key in _cache:
        return _cache[key]
    if variant != "full":
        H = hierarchy(fem, name)
        if H.nlevels == 1:
            raise KeyError(key)
        if variant == "pzp":
            H = dataclasses.replace(H, omega_over_d=[np.zeros_like(w) for w in H.omega_over_d])
        elif variant == "smooth":
            H = dataclasses.replace(H, coarse_inv=np.zeros_like(H.coarse_inv, order="F"))
        else:
            raise KeyError(key)
        _cache[key] = H
        return H
    rng = np.random.default_rng([17, NAMES.index(name)])
    kind, _, arg = name.partition("_")
    if name == "diag1025":
        A = ss.diag(1025)
        H = _two_level(fem, A, p_pattern(A, groups(1025, 2)), rng)
    elif name == "tridiag3000":
        A = ss.tridiag(3000)
        H = _two_level(fem, A, p_pattern(A, groups(3000, 4)), rng)
    elif kind == "arrow":
        A = ss.arrow(2100, int(arg))
        H = _two_level(fem, A, p_pattern(A, groups(2100, 2)), rng)
    elif name == "odd_start":
        A = ss.odd_start()
        H = _two_level(fem, A, p_pattern(A, groups(A.shape[0], 2)), rng)
    elif name == "holes":
        A = ss.holes()[0]
        H = _two_level(fem, A, p_pattern(A, groups(A.shape[0], 8)), rng)
    elif name == "longP":
        H = _two_level(fem, ss.tridiag(2100), long_p(), rng)
    elif name == "lead_long":
        A = lead_long()
        H = _two_level(fem, A, p_pattern(A, groups(A.shape[0], 2)), rng)
    elif name == "giant":
        import amg_ref as ar
        H = ar.giant_aggregate_hierarchy(fem)
    elif name == "three_tiny":
        A0, A1 = ss.tridiag(5), sp.csr_matrix(np.ones((2, 2)))
        H = _assemble(fem, [A0, A1, sp.csr_matrix(np.ones((1, 1)))], [p_pattern(A0, groups(5, 3)), sp.csr_matrix(np.ones((2, 1)))], rng)
    elif kind == "coarse1":
        H = _assemble(fem, [ss.diag(int(arg))], [], rng)
    elif kind == "coarse2":
        n = int(arg)
        A = ss.tridiag(2 * n + 3)
        H = _two_level(fem, A, p_pattern(A, (np.arange(2 * n + 3, dtype=np.int64) * n) // (2 * n + 3)), rng)
    elif name == "odd_tail":
        A = odd_tail()
        H = _two_level(fem, A, p_pattern(A, groups(A.shape[0], 2)), rng)
    elif kind == "blocks":
        A = ss.tridiag(blocks_len(int(arg)))
        H = _two_level(fem, A, p_pattern(A, groups(A.shape[0], 8)), rng)
    else:
        raise KeyError(name)
    _cache[key] = H
    return H


def variants(fem, name):
    return VARIANTS if hierarchy(fem, name).nlevels > 1 else ("full",)


def long_row(name, n):
    """the index of the row the case is named for (the long row; else a row in the middle)"""
    if name.startswith("arrow") or name == "giant":
        return 0
    return {"odd_start": 1, "longP": LONGP_ROW, "lead_long": LEAD}.get(name, n // 3)


def rhs(name, n):
    """a mixed-sign vector with about 20 % exact zeros, e_0, e_{n-1}, the unit vector of the long row"""
    rng = np.random.default_rng([23, NAMES.index(name) if name in NAMES else 999, n])
    v = _vals(rng, n)
    v[rng.random(n) < 0.2] = 0.0
    out = [v]
    for i in (0, n - 1, long_row(name, n)):
        e = np.zeros(n)
        e[i] = 1.0
        out.append(e)
    return out
