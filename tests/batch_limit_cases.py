"""Inputs of the batched and the multi-workgroup (GENERIC) Krylov loop at the sizes where their grids and buffers cap
(csrc/batch_solvers.hpp, csrc/csr_batch.hpp, the GENERIC kernels of csrc/kernels.hpp, the replay policy of csrc/solvers.hpp),
and the CPU restatements they are compared with. numpy / scipy only; not a conftest: tests/test_batch_limits_cpu.py holds
every input to the condition that makes it an edge, tests/test_gpu_batch_limits.py runs them on the device.

What caps, restated here as host arithmetic:

  vec_grid(n) = min(ceil(n / 1024), MAX_PARTS = 512)   workgroups of every vector kernel, four elements per thread and pass:
                                                       beyond n = 4 * 512 * 256 = 524 288 the kernels take a second pass
  CF_VEC_GRID = 256                                    workgroups of the vector half of the two-launch sparse form
  sum_partials(g)                                      8 lanes of 256 partials per pass: lanes 1 .. 7 for g > 256, a second
                                                       pass for g > 2048; the p'Ap partials have g = the SpMV's row blocks
  BATCH_RES_STAGE = 1024                               residual norms per system that travel through pinned memory
  first_graph(predicted, chunk, maxit)                 iterations of the set-up graph: at most 1024, a multiple of 32 past 64
  GRAPH_CAP = 48                                       graphs of one workspace size before the map is emptied

The systems:

  big_a, big_b   tridiagonal chains (`amg_setup_synth.chain`, `spd_values`) of 524 289 rows (the second pass holds exactly one
                 element; 1543 row blocks) and of the smallest odd length with at least 2049 row blocks; two slots, a right-hand
                 side per slot, a non-zero initial guess in column 1
  lap2049        tridiag(-1, 2, -1) + σ I, σ = 1e-2, 1e-3, 1e-4, 0 in the slots 0 .. 3: cg counts on both sides of 1024
  lap301         the unshifted Laplacian of 301 rows (slot 0) and its copy shifted by 1e-2 (slot 1): with maxit = n + 5 slot 0
                 reaches it = n + 1, where the reference's `res_norm[it] = ...` throws BoundsError
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

import amg_ref
import amg_setup_synth as asy
import amg_synth as ays

NT, MAX_PARTS, CF_VEC_GRID = 256, 512, 256
TILE = ays.TILE
LANE_SET, LANE_PASS = NT, 8 * NT                # partials one lane of sum_partials reads, partials of one pass
BATCH_RES_STAGE = 1024
FIRST_CAP = 1024
GRAPH_CAP = 48
EPS = 1e-7
TIGHT_PREFIX = 20                               # test_gpu_parity.assert_history: the tight branch needs it <= 20
LOW, HIGH = 0.95, 1.05                          # margins of a count that must not flip on summation order


def vec_grid(n):
    return int(max(1, min((n + 4 * NT - 1) // (4 * NT), MAX_PARTS)))


def passes(n, grid):
    """trips of a four-elements-per-thread kernel (k_update_xr, k_update_p, k_dot_partial) on a grid of `grid` workgroups"""
    return -(-n // (4 * grid * NT))


def first_graph(predicted, chunk, maxit):
    """iterations of the set-up graph (Krylov::solve, BatchKrylov::solve)"""
    first = predicted if predicted > 0 else chunk
    if first > 64:
        first -= first % 32
    return max(1, min(first, maxit, FIRST_CAP))


# ------------------------------------------------------------------ row blocks of a chain, in closed form
def _chain_ptr(i, n):
    """indptr[i] of the tridiagonal pattern of n rows"""
    return 0 if i == 0 else (3 * n - 2 if i == n else 3 * i - 1)


def chain_block_count(n):
    """`ays.row_blocks(asy.chain(n).indptr).shape[0]` without the pattern and without a step per row: the same greedy rule,
    the same back-off to an even offset, but every block starts its search where the tile is already nearly full"""
    r, nb = 0, 0
    while r < n:
        e = max(r + 1, min(n, r + TILE // 3 - 2))          # ptr[e] - ptr[r] <= 3 (e - r) + 1 <= TILE: every step up to e passes
        while e < n and _chain_ptr(e + 1, n) - _chain_ptr(r, n) <= TILE:
            e += 1
        if e < n and (_chain_ptr(e, n) & 1):
            for back in (1, 2, 3):
                if e - back <= r:
                    break
                if (_chain_ptr(e - back, n) & 1) == 0:
                    e -= back
                    break
        nb += 1
        r = e
    return nb


@functools.lru_cache(maxsize=None)
def smallest_odd_chain(k):
    """the smallest odd n whose chain has at least k row blocks: bisection around k rows-per-block, with `chain_block_count`"""
    per = TILE / 3.0                                       # a full block holds about 341 rows
    lo, hi = int(0.9 * k * per) | 1, int(1.1 * k * per) | 1
    assert chain_block_count(lo) < k <= chain_block_count(hi)
    while hi - lo > 2:                                     # odd lo, hi: count(lo) < k <= count(hi)
        mid = ((lo + hi) // 2) | 1
        if mid >= hi:
            mid -= 2
        if chain_block_count(mid) >= k:
            hi = mid
        else:
            lo = mid
    return hi


BIG_N = {"big_a": 4 * MAX_PARTS * NT + 1, "big_b": None}     # big_b: smallest_odd_chain(LANE_PASS + 1), see big_n
BIG_SEED = {"big_a": 11, "big_b": 24}
BIG_X0_SCALE = 1e-3                                        # the non-zero guess is small against the solution: it stays <= 20
BANK_P, BANK_W, BANK_STOP = 2, 8, 200


def big_n(name):
    return BIG_N[name] or smallest_odd_chain(LANE_PASS + 1)


@functools.lru_cache(maxsize=None)
def big(name):
    """(matrices of the two slots, right-hand sides, X0 [n x 2, column 0 zero, column 1 random]) """
    n = big_n(name)
    S = asy.chain(n)
    seed = BIG_SEED[name]
    rng = np.random.default_rng([seed, 7])
    mats = [asy.spd_values(S, [seed, p]) for p in range(2)]
    bs = [rng.standard_normal(n) for _ in range(2)]
    X0 = np.zeros((n, 2), order="F")
    X0[:, 1] = BIG_X0_SCALE * rng.standard_normal(n)
    return mats, bs, X0


def big_aggregates(name):
    return asy.chain_levels(big_n(name), BANK_W, BANK_STOP)


# ------------------------------------------------------------------ Laplacians
LAP_SIGMA = (1e-2, 1e-3, 1e-4, 0.0)
LAP_LONG_N, LAP_LONG_SEED = 2049, 5
LAP_OVER_N, LAP_OVER_SEED, LAP_OVER_SIGMA, LAP_OVER_EXTRA = 301, 9, 1e-2, 5


def laplacian(n, sigma=0.0):
    """tridiag(-1, 2, -1) + sigma I in sorted CSR; every sigma on the one pattern"""
    A = sp.diags([-np.ones(n - 1), np.full(n, 2.0 + sigma), -np.ones(n - 1)], [-1, 0, 1], format="csr")
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def lap2049():
    """(matrices of the slots 0 .. 3, the one right-hand side)"""
    return [laplacian(LAP_LONG_N, s) for s in LAP_SIGMA], np.random.default_rng(LAP_LONG_SEED).standard_normal(LAP_LONG_N)


@functools.lru_cache(maxsize=None)
def lap301():
    """(matrices: unshifted, shifted; right-hand side; maxit)"""
    n = LAP_OVER_N
    return [laplacian(n), laplacian(n, LAP_OVER_SIGMA)], np.random.default_rng(LAP_OVER_SEED).standard_normal(n), n + LAP_OVER_EXTRA


# ------------------------------------------------------------------ CPU restatements
def identity(r):
    return r.copy()


def cg_ref(A, b, x0=None, maxit=0, eps=EPS):
    """cg.jl:14-50 through the numpy pcg with M = identity (z is r): (x, it, res_norm[:it]). The restatement has no capacity:
    with maxit > n it counts on where the reference throws at it = n + 1."""
    return amg_ref.pcg(A, b, np.zeros(b.size) if x0 is None else x0, identity, maxit=maxit, eps=eps)


def bank_ref(fem, A, aggs, b, x0=None, eps=EPS):
    """pcg with the V-cycle of the host hierarchy that `fem.amg_refresh` builds for `A` on the aggregates `aggs`"""
    H = fem.amg_refresh(aggs, A)
    return amg_ref.pcg(A, b, np.zeros(b.size) if x0 is None else x0, lambda r: amg_ref.cycle(H, r), eps=eps)


def oracle_cg(orc, A, b, x0=None, maxit=0, eps=EPS):
    """cg.jl:14-50 by the C oracle on the stdlib CSC SpMV; raises the oracle's BoundsError where the reference does"""
    return orc.cg(orc.csc_operator(A), b, np.zeros(b.size) if x0 is None else x0, maxit=maxit, eps=eps)


_refs = {}


def big_cg_ref(orc, name, t):
    """the oracle's cg for system t of the big batch (slot t, its right-hand side, column t of X0), computed once"""
    if (name, t) not in _refs:
        mats, bs, X0 = big(name)
        _refs[name, t] = oracle_cg(orc, mats[t], bs[t], X0[:, t])
    return _refs[name, t]


def big_bank_ref(fem, name):
    """the restatement's pcg for slot 0 under member 0 (the hierarchy of slot 0's matrix), x0 = 0, computed once"""
    if (name, "bank") not in _refs:
        mats, bs, _ = big(name)
        _refs[name, "bank"] = bank_ref(fem, mats[0], big_aggregates(name), bs[0])
    return _refs[name, "bank"]


def margins(res, b, eps=EPS):
    """(res_norm[it] / tol, res_norm[it - 1] / tol): the stop must not sit on the tolerance"""
    tol = eps * np.linalg.norm(b)
    return float(res[-1] / tol), float(res[-2] / tol)


def tight(ref, b, eps=EPS):
    """the conditions of the REFERENCE bar: it <= TIGHT_PREFIX, the last residual at most LOW tol, the one before at least HIGH tol"""
    _, it, res = ref
    last, before = margins(res, b, eps)
    return it <= TIGHT_PREFIX and last <= LOW and before >= HIGH


# ------------------------------------------------------------------ poisoned systems of section 4
POISONS = ("A_nan", "A_zero", "x0_inf")


def poisoned_values(A, kind):
    """the CSR values of the poisoned matrix (None: the matrix stays clean and the poison sits in X0)"""
    v = np.array(A.data, dtype=np.float64, copy=True)
    if kind == "A_nan":
        v[v.size // 2] = np.nan
        return v
    if kind == "A_zero":
        return np.zeros_like(v)
    assert kind == "x0_inf"
    return None


def poison_x0(x0, kind):
    x0 = np.array(x0, dtype=np.float64, copy=True)
    if kind == "x0_inf":
        x0[x0.size // 3] = np.inf
    return x0
