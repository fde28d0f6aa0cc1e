"""Inputs and case tables for the edge suite of the Krylov loops (csrc/solvers.hpp; k_fused_*, k_defl_mu, k_multi_dot_view,
k_lu_solve, k_entry_zero, k_fold_start, k_update_xr / p in csrc/kernels.hpp).

Not a conftest: tests/test_krylov_edges_cpu.py and tests/test_gpu_krylov_edges.py import it. Everything here runs on the host.

  banded(n)        S T S with T the 5-diagonal stencil (-1/2, -1, 3 + SHIFT, -1, -1/2) (diagonally dominant, κ(T) < 1 + 6 / SHIFT)
                   and S² drawn from {1, 4, 25, 100}: a diagonal scaling of 1 ... 100, so Jacobi-PCG runs on T (6-8
                   iterations) and plain CG on κ ~ 1e2 in four clusters (35-46 iterations).
  Dense            blocks D + R (D uniform in [2, 20], R symmetric random with zero diagonal and absolute row sums <= 1, so
                   Gershgorin gives λ in [1, 21]: κ <= 21, no factorisation of a large matrix) on gather maps with an EXACT
                   number of Γ nodes and an exact largest multiplicity (exact_maps: gather_maps of the dense suite cannot hit
                   n_Γ = 1024 / 1025).
  SPARSE / DENSE   the problems by name; EPT (elements per thread of the single-workgroup loop) follows from n alone.
  Solve            one solver call as data; the lists at the end are what the GPU file runs, group by group, and what the
                   CPU file proves the conditions of the strict parity row for.

Chosen conditioning and stop: κ(T) < 1.2 (SHIFT = 30), scaling {1, 4, 25, 100}, dense κ_d <= 21; EPS = 1e-6, but EPS_DENSE_CG =
1e-2 for the unpreconditioned solves (cg, defcg) on the dense operators and EPS_SPARSE_DEFCG = 1e-4 for defcg on the sparse ones. With these every solve here ends within 50 iterations
and the oracle's history moves by < 1 % of the history bar under another summation order (tests/test_krylov_edges_cpu.py
asserts both, and that every stop is decided by >= 1e-4 relative). What did not hold, measured on the oracle against the
numpy solver below: a continuous scaling 10^U(0, 2) with SHIFT = 3 needs 82-106 CG iterations and its history moves by up to
5e6 x the bar once the outlying eigenvalues have converged (n = 2049, from iteration ~50); plain CG on the dense operators
(outliers at the nodes of multiplicity 4 - 6) moves by up to 1e7 x the bar at eps = 1e-5 (d1025w6), by <= 2e-4 of it at 1e-2."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

NTF = 1024                       # threads of the single-workgroup loop (csrc/kernels.hpp)
FUSED_MAX_N = 8 * NTF
GEMV_PANEL = 2048
EPS = 1e-6                       # stop threshold of the solves of this suite ...
EPS_DENSE_CG = 1e-2              # ... but cg / defcg on the dense operators
EPS_SPARSE_DEFCG = 1e-4          # ... and defcg on the sparse ones (random W does not help: 53 iterations to 1e-6 with 64 columns)
SHIFT = 30.0
SCALES = (1.0, 4.0, 25.0, 100.0)
RES_RTOL, RES_FLOOR, X_RTOL = 1e-8, 1e-12, 1e-6      # DESIGN §3, the strict row (test_gpu_parity)
STOP_GAP = 1e-4                  # |res - tol| / tol of the last two residuals: 1e4 x the history bar
ORDER_SHARE = 0.01               # oracle vs numpy (another summation order): share of the history bar
NVEC_ALL = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 20, 21, 32, 33, 36, 37, 64, 65)
NVEC_EPT8 = (3, 4, 5, 8, 9, 64)
NVEC_EPT2 = (7, 8, 9)


def ept(n):
    """template argument Krylov::with_ept picks; 0: n leaves the single-workgroup loop"""
    for e in (1, 2, 4, 8):
        if n <= e * NTF:
            return e
    return 0


# ------------------------------------------------------------------ sparse operators (view width 0)
SPARSE_N = (1023, 1024, 1025, 2048, 2049, 4096, 4097, 8191, 8192, 8193)


def banded(n):
    rng = np.random.default_rng(6100 + n)
    s = np.sqrt(np.array(SCALES)[rng.integers(0, len(SCALES), n)])
    T = sp.diags([np.full(n - 2, -0.5), np.full(n - 1, -1.0), np.full(n, 3.0 + SHIFT), np.full(n - 1, -1.0), np.full(n - 2, -0.5)],
                 [-2, -1, 0, 1, 2], format="csr")
    A = sp.csr_matrix(sp.diags(s) @ T @ sp.diags(s))
    A = sp.csr_matrix((A + A.T) / 2)
    A.sum_duplicates()
    A.sort_indices()
    return A


def rhs(n, seed=0):
    return np.random.default_rng(7700 + seed + n).standard_normal(n)


def x0_rand(n, seed=0):
    return np.random.default_rng(9900 + seed + n).standard_normal(n)


def random_W(n, nvec, seed=0):
    """orthonormalised random columns"""
    return np.asfortranarray(np.linalg.qr(np.random.default_rng(5300 + seed + 7 * nvec + n).standard_normal((n, nvec)))[0])


# ------------------------------------------------------------------ dense operators (slot views)
def exact_maps(sizes, n_nodes, width, rng):
    """Gather lists for blocks of `sizes` over exactly `n_nodes` Γ nodes, every node in 1 ... width blocks and node 0 in
    exactly `width` of them (the first `width` blocks). A block takes unused nodes first, then shared ones at random.
    Returns (gather lists, node_Γ_cnt, n_Γ)."""
    assert sum(sizes) >= n_nodes and len(sizes) >= width and max(sizes) <= n_nodes
    cnt = np.zeros(n_nodes, dtype=np.int64)
    g = []
    for d, n in enumerate(sizes):
        forced = np.zeros(1 if (width > 1 and d < width) else 0, dtype=np.int64)
        free = np.flatnonzero(cnt == 0)
        free = free[~np.isin(free, forced)]
        a = rng.choice(free, min(n - forced.size, free.size), replace=False)
        ok = np.flatnonzero((cnt > 0) & (cnt < width))
        ok = ok[~np.isin(ok, forced)]
        b = rng.choice(ok, n - forced.size - a.size, replace=False)
        pick = np.concatenate([forced, a, b]).astype(np.int64)
        rng.shuffle(pick)
        cnt[pick] += 1
        g.append(pick)
    assert cnt.min() >= 1 and cnt.max() == width
    return g, cnt, n_nodes


def dd_blocks(sizes, seed):
    """Strictly diagonally dominant symmetric blocks: λ in [1, 21] by Gershgorin."""
    out = []
    for k, n in enumerate(sizes):
        rng = np.random.default_rng(100 * seed + k)
        R = rng.standard_normal((n, n))
        R = (R + R.T) / 2
        np.fill_diagonal(R, 0.0)
        R /= max(np.abs(R).sum(axis=1).max(), 1.0)
        out.append(np.asfortranarray(R + np.diag(rng.uniform(2.0, 20.0, n))))
    return out


def gershgorin(S):
    d = np.diag(S)
    R = np.abs(S).sum(axis=1) - np.abs(d)
    return float((d - R).min()), float((d + R).max())


def split_sizes(total, nblk):
    """nblk unequal block sizes that add up to `total` (none a multiple of a tile on purpose: the remainder goes to block 0)"""
    w = np.array([1.0, 0.85, 0.7, 0.55, 0.4, 0.3, 0.25, 0.2][:nblk])
    s = np.floor(total * w / w.sum()).astype(int)
    s[0] += total - s.sum()
    return tuple(int(v) for v in s)


@dataclass(frozen=True)
class Dense:
    name: str
    n: int                       # n_Γ
    width: int                   # largest multiplicity (3 is widened to 4 slots by the operator)
    sizes: tuple
    seed: int
    tiling: tuple = None         # (MI355_GEMV_WAVES, MI355_GEMV_RPW) the GPU file forces while it builds the operators

    @property
    def nloc(self):
        return sum(self.sizes)

    @property
    def slot_width(self):
        return 4 if self.width == 3 else self.width

    @property
    def folds(self):
        return self.slot_width <= 4 and max(self.sizes) <= GEMV_PANEL

    def ntiles(self, waves=16, rpw=2):
        return sum(-(-n // (waves * rpw)) for n in self.sizes)


def _dense(name, n, width, seed, share=0.25, nblk=None, sizes=None, tiling=None):
    if sizes is None:
        total = n if width == 1 else int(n * (1 + share))
        nblk = nblk or max(width, 2, -(-total // 1400))
        sizes = split_sizes(total, nblk)
    return Dense(name, n, width, tuple(sizes), seed, tiling)


def _dense_table():
    t = []
    for k, n in enumerate((1024, 1025, 2048, 2049, 4096, 4097)):          # the last n of an EPT and the first of the next
        for w in (2, 4):
            t.append(_dense(f"d{n}w{w}", n, w, 10 * k + w))
    t.append(_dense("d2048w1", 2048, 1, 71))                               # generic view_load loop, EPT 2
    t.append(_dense("d1025w6", 1025, 6, 72))                               # generic loop, EPT 2; too wide to fold
    t.append(_dense("d4097w3", 4097, 3, 73))                               # 3 widened to 4, EPT 8
    # deflation: nloc (k_defl_mu's grid is ceil(nloc / 1024)) at 1023 / 1024 / 1025: three gather maps, EPT 1
    for k, last in enumerate((143, 144, 145)):
        t.append(_dense(f"nloc{880 + last}", 820, 4, 80 + k, sizes=(330, 300, 250, last)))
    # deflation: more than 256 / 512 tiles of the Neumann-Neumann operator when tiled 4 waves x 1 row
    t.append(_dense("tiles336", 1100, 4, 84, sizes=(600, 480, 203, 57), tiling=(4, 1)))
    t.append(_dense("tiles544", 1800, 4, 85, sizes=(900, 700, 450, 121), tiling=(4, 1)))
    # big-fold start-up: n_Γ in (8192, 8300], slot width 2, blocks of at most 1100 rows, 100 shared rows
    t.append(_dense("big8200", 8200, 2, 86, sizes=(1100,) * 7 + (600,)))
    return t


DENSE = {d.name: d for d in _dense_table()}
SPARSE = {f"sp{n}": n for n in SPARSE_N}


def size_of(prob):
    return SPARSE[prob] if prob in SPARSE else DENSE[prob].n


# ------------------------------------------------------------------ solver calls as data
@dataclass(frozen=True)
class Solve:
    prob: str
    kind: str                    # cg | pcg (Jacobi on sparse, Neumann-Neumann on dense) | pcg_id | defcg | defpcg
    nvec: int = 0
    x0: str = "zero"             # zero | rand
    maxit: int = 0
    eps_: float = 0.0            # 0: the default of the kind

    @property
    def eps(self):
        if self.eps_:
            return self.eps_
        if self.kind in ("cg", "defcg") and self.prob in DENSE:
            return EPS_DENSE_CG
        return EPS_SPARSE_DEFCG if self.kind == "defcg" else EPS

    @property
    def id(self):
        return f"{self.prob}-{self.kind}" + (f"-{self.nvec}" if self.nvec else "") + ("-x0" if self.x0 == "rand" else "") + \
            (f"-maxit{self.maxit}" if self.maxit else "") + (f"-eps{self.eps_:g}" if self.eps_ else "")


def sparse_solves(prob):
    """group 1: cg, Jacobi pcg, identity pcg from zero and from a random x0, maxit 0, 1, 2"""
    return [Solve(prob, kind, 0, x0, maxit) for kind in ("cg", "pcg", "pcg_id") for x0 in ("zero", "rand") for maxit in (0, 1, 2)]


def dense_solves(prob):
    """group 2: pcg from zero (the zero entry of the folded loop) and from a random x0, cg from zero"""
    return [Solve(prob, "pcg"), Solve(prob, "pcg", x0="rand"), Solve(prob, "cg")]


GROUP2 = [n for n in DENSE if n.startswith("d")]
# group 3: (problem, kinds, nvec values)
DEFLATED = [("nloc1023", ("defpcg",), NVEC_ALL), ("nloc1024", ("defpcg", "defcg"), NVEC_ALL), ("nloc1025", ("defpcg",), NVEC_ALL),
            ("tiles336", ("defpcg",), tuple(v for v in NVEC_ALL if v >= 32)),
            ("tiles544", ("defpcg",), tuple(v for v in NVEC_ALL if v >= 16)),
            ("d4097w4", ("defpcg",), NVEC_EPT8 + (65,)), ("d1025w4", ("defpcg", "defcg"), NVEC_EPT2),
            ("sp8192", ("defpcg", "defcg"), NVEC_EPT8 + (65,)), ("sp2048", ("defpcg", "defcg"), NVEC_EPT2)]
DEFLATED_SOLVES = [Solve(p, k, v) for p, kinds, nv in DEFLATED for k in kinds for v in nv]
BIG = "big8200"
BIG_SOLVES = [Solve(BIG, "pcg"), Solve(BIG, "pcg", x0="rand")]
# group 5: the solve whose chunking is varied, per problem; the sequence adds maxit = 2, a looser and a tighter eps, x0, b = 0
REPLAY = [Solve("sp8192", "pcg"), Solve("d4096w4", "pcg"), Solve("nloc1024", "defpcg", 5)]
EPS_LOOSE, EPS_TIGHT = 1e-3, 1e-8


def replay_sequence(s):
    """the eight solves of the sequence test as (Solve, b kind): b kind "b" or "zero" """
    def v(**kw):
        return Solve(s.prob, s.kind, s.nvec, kw.get("x0", "zero"), kw.get("maxit", 0), kw.get("eps", 0.0))
    return [(s, "b"), (v(maxit=2), "b"), (v(eps=EPS_LOOSE), "b"), (v(eps=EPS_TIGHT), "b"), (v(x0="rand"), "b"), (s, "b"),
            (s, "zero"), (s, "b")]


def all_solves():
    out = [s for p in SPARSE for s in sparse_solves(p)] + [s for p in GROUP2 for s in dense_solves(p)] + DEFLATED_SOLVES + BIG_SOLVES
    for s in REPLAY:
        out += [t for t, bk in replay_sequence(s) if bk == "b"]
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


# ------------------------------------------------------------------ realising problems and solves on the oracle
def exact_inverses(S):
    out = []
    for B in S:
        P = np.linalg.inv(B)
        out.append(np.asfortranarray((P + P.T) / 2))
    return out


class Problems:
    """Operators, vectors and oracle results per name, built once. `pinv(dense case, blocks) -> Π blocks`: the exact inverses
    on the host (default), mi_nn_pinv in the GPU file — the oracle then runs on the very Π the device uses."""

    def __init__(self, orc, pinv=None):
        self.orc, self.pinv = orc, pinv or (lambda d, S: exact_inverses(S))
        self._mat, self._maps, self._S, self._P, self._ops, self._res, self._W = {}, {}, {}, {}, {}, {}, {}

    # -- inputs
    def matrix(self, prob):
        if prob not in self._mat:
            self._mat[prob] = banded(SPARSE[prob])
        return self._mat[prob]

    def maps(self, prob):
        if prob not in self._maps:
            d = DENSE[prob]
            self._maps[prob] = exact_maps(d.sizes, d.n, d.width, np.random.default_rng(d.seed))
        return self._maps[prob]

    def blocks(self, prob):
        if prob not in self._S:
            self._S[prob] = dd_blocks(DENSE[prob].sizes, DENSE[prob].seed)
        return self._S[prob]

    def pi_blocks(self, prob):
        if prob not in self._P:
            self._P[prob] = self.pinv(DENSE[prob], self.blocks(prob))
        return self._P[prob]

    def b(self, prob, kind="b"):
        n = size_of(prob)
        return np.zeros(n) if kind == "zero" else rhs(n)

    def x0(self, s):
        n = size_of(s.prob)
        return x0_rand(n) if s.x0 == "rand" else np.zeros(n)

    def W(self, s):
        key = (s.prob, s.nvec)
        if s.nvec and key not in self._W:
            self._W[key] = random_W(size_of(s.prob), s.nvec)
        return self._W.get(key)

    # -- oracle operators
    def op(self, prob, which):
        """which: A | jacobi | identity | nn"""
        key = (prob, which)
        if key not in self._ops:
            orc = self.orc
            if prob in SPARSE:
                A = self.matrix(prob)
                self._ops[key] = {"A": lambda: orc.csc_operator(A), "jacobi": lambda: orc.jacobi_operator(A.diagonal()),
                                  "identity": lambda: orc.identity_operator(A.shape[0])}[which]()
            else:
                g, cnt, n = self.maps(prob)
                self._ops[key] = orc.apply_local_schurs_operator(self.blocks(prob), g, n) if which == "A" else \
                    orc.neumann_neumann_operator(self.pi_blocks(prob), g, cnt)
        return self._ops[key]

    def precond(self, s):
        if s.kind in ("cg", "defcg"):
            return None
        if s.prob in DENSE:
            return "nn"
        return "identity" if s.kind == "pcg_id" else "jacobi"

    def solve(self, s, bkind="b"):
        """the oracle's (x, it, res_norm) of a Solve, computed once"""
        key = (s, bkind)
        if key not in self._res:
            self._res[key] = run(self.orc, s, self.op(s.prob, "A"), self.op(s.prob, self.precond(s)) if self.precond(s) else None,
                                 self.b(s.prob, bkind), self.x0(s), self.W(s))
        return self._res[key]

    def drop(self, prob):
        """free the blocks and operators of a dense problem (the large ones hold hundreds of MB between them)"""
        for cache in (self._S, self._P, self._maps):
            cache.pop(prob, None)
        for key in [k for k in self._ops if k[0] == prob]:
            del self._ops[key]


def run(mod, s, A, M, b, x0, W):
    """a Solve on `mod` (the oracle module or the package's api: the same signatures)"""
    if s.kind == "cg":
        return mod.cg(A, b, x0, s.maxit, s.eps)
    if s.kind in ("pcg", "pcg_id"):
        return mod.pcg(A, b, x0, M, s.maxit, s.eps)
    if s.kind == "defcg":
        return mod.defcg(A, b, x0, W, s.maxit, s.eps)
    return mod.defpcg(A, b, x0, W, M, s.maxit, s.eps)


# ------------------------------------------------------------------ the same solvers in numpy, another summation order
def _psum(a, b):
    return np.sum(a * b)                 # pairwise; the oracle's orc_dot adds left to right. np.float64: x / 0 is IEEE's inf


def numpy_apply(probs, prob, which):
    if prob in SPARSE:
        A = probs.matrix(prob)
        if which == "A":
            return lambda v: A @ v
        if which == "identity":
            return lambda v: v.copy()
        dinv = 1.0 / A.diagonal()
        return lambda v: dinv * v
    g, cnt, n = probs.maps(prob)
    blocks = probs.blocks(prob) if which == "A" else probs.pi_blocks(prob)
    c = cnt.astype(np.float64)

    def f(v):
        y = np.zeros(n)
        for B, gd in zip(blocks, g):
            y[gd] += B @ v[gd] if which == "A" else (B @ (v[gd] / c[gd])) / c[gd]
        return y
    return f


def numpy_krylov(A, M, W, b, x0, eps, maxit=0):
    """cg.jl / defcg.jl with numpy's products and pairwise sums; M, W may be None"""
    n = b.size
    maxit = maxit or n
    x = x0.copy()
    if W is not None:
        AW = np.column_stack([A(W[:, v]) for v in range(W.shape[1])])
        WtAW = AW.T @ W
        x = x + W @ np.linalg.solve(WtAW, W.T @ (b - A(x)))
    r = b - A(x)
    z = M(r) if M else r
    rz = _psum(r, z)
    p = z - W @ np.linalg.solve(WtAW, AW.T @ z) if W is not None else z.copy()
    res = [np.sqrt(_psum(r, r))]
    tol = eps * np.sqrt(_psum(b, b))
    while len(res) < maxit and res[-1] > tol:
        Ap = A(p)
        alpha = rz / _psum(p, Ap)
        x = x + alpha * p
        r = r - alpha * Ap
        z = M(r) if M else r
        rz, old = _psum(r, z), rz
        p = (rz / old) * p + z
        if W is not None:
            p = p - W @ np.linalg.solve(WtAW, AW.T @ z)
        res.append(np.sqrt(_psum(r, r)))
    return x, len(res), np.array(res)


def numpy_solve(probs, s):
    pre = probs.precond(s)
    return numpy_krylov(numpy_apply(probs, s.prob, "A"), numpy_apply(probs, s.prob, pre) if pre else None, probs.W(s),
                        probs.b(s.prob), probs.x0(s), s.eps, s.maxit)


def history_margin(res, reso):
    """largest res_norm deviation over the common part in units of the strict bar 1e-8 res_k + 1e-12 res_1"""
    m = min(res.size, reso.size)
    return float(np.max(np.abs(res[:m] - reso[:m]) / (RES_RTOL * reso[:m] + RES_FLOOR * reso[0]))) if m and reso[0] else 0.0


def x_margin(x, xo):
    d = np.linalg.norm(xo)
    return float(np.linalg.norm(x - xo) / (X_RTOL * d)) if d else float(np.linalg.norm(x - xo))
