"""Cases, poisons and the expected-outcome table of the state-leak suite: a call that sees NaN / Inf, breaks down inside
the loop or returns an error must leave nothing behind in the device scratch of its handles (operators, context, Krylov
workspace, interior CG, eigCG window, preconditioner buffers). The reference carries nothing from one solve to the next.

Not a conftest: tests/test_poison_cpu.py and tests/test_gpu_poison.py import it. Everything here runs on the host. The
operators come from the generators of krylov_synth.py, sparse_synth.py and eig_synth.py; only the breakdown systems are new.

  POISONS          b_nan / b_inf (one entry of b), b_huge (b * 1e160: r'r overflows), x0_nan (one entry of x0), W_nan (one
                   entry of W), W_zero (W = 0: WtAW is singular).
  EXPECT           the oracle's outcome per (solver group, poison): (it, kind of res_norm[0]) or the exception.
  breakdown(n)     A = diag(+1 ... +1, -1 ... -1), b = 1, x0 = 0: p'Ap is a sum of n/2 (+1) and n/2 (-1), exactly 0 in ANY
                   summation order, so alpha = n / 0 = Inf in the first iteration of every implementation:
                   res_norm = [sqrt(n), inf, nan], it = 3. The only poison that turns non-finite inside the loop.
  breakdown_dense  the same operator as two dense blocks on identical maps (every node of multiplicity 2):
                   S_d = diag(+-1/2), Pi_d = I, so S = diag(+-1) and Pi = I / 2 exactly (every entry a power of two).
  Call             one solver call as data, for all ten solver kinds.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

import eig_synth as es
import krylov_synth as ks
import sparse_synth as ss

POISON_MAXIT = 20                # every poisoned solve is capped (the suite allows at most 50), so a missed stop cannot run long
POISONS_VEC = ("b_nan", "b_inf", "b_huge", "x0_nan")
POISONS_W = ("W_nan", "W_zero")
HUGE = 1e160

PLAIN = ("cg", "pcg", "pcg_id", "eigcg", "eigpcg")
DEFL = ("defcg", "defpcg", "eigdefcg", "initcg", "initpcg")
KINDS = PLAIN + DEFL + ("eigdefpcg",)
EIG_KINDS = ("eigcg", "eigpcg", "eigdefcg", "eigdefpcg", "initcg", "initpcg")     # "the six eigCG-family solvers"
UNPRECONDITIONED = ("cg", "defcg", "eigcg", "eigdefcg", "initcg")


def group_of(kind):
    return "plain" if kind in PLAIN else "defl" if kind in DEFL else "eigdefpcg"


def takes_W(kind):
    return kind not in PLAIN


# (group, poison) -> (it, what res_norm[0] is) | "singular" | "bounds" | None (not applicable)
EXPECT = {}
for _p, _a, _b in (("b_nan", "nan", "nan"), ("b_inf", "inf", "nan"), ("b_huge", "inf", "inf"), ("x0_nan", "nan", "nan")):
    EXPECT[("plain", _p)] = (1, _a)
    EXPECT[("defl", _p)] = (1, _b)
    EXPECT[("eigdefpcg", _p)] = "bounds"          # the final extraction at it = 1: eigvecs(...)[:, 1:nvec] of an empty matrix
EXPECT[("plain", "W_nan")] = EXPECT[("plain", "W_zero")] = None
EXPECT[("defl", "W_nan")] = (1, "nan")
EXPECT[("eigdefpcg", "W_nan")] = "bounds"
EXPECT[("defl", "W_zero")] = EXPECT[("eigdefpcg", "W_zero")] = "singular"


def poisons_of(kind):
    return POISONS_VEC + (POISONS_W if takes_W(kind) else ())


def poisoned(name, b, x0, W):
    """(b, x0, W) with the poison `name` in it; the inputs are left alone"""
    b, x0 = np.array(b, dtype=np.float64), np.array(x0, dtype=np.float64)
    W = None if W is None else np.array(W, dtype=np.float64, order="F")
    n = b.size
    if name == "b_nan":
        b[n // 2] = np.nan
    elif name == "b_inf":
        b[3] = np.inf
    elif name == "b_huge":
        b *= HUGE
    elif name == "x0_nan":
        x0[n // 3] = np.nan
    elif name == "W_nan":
        W[n // 2, W.shape[1] // 2] = np.nan
    elif name == "W_zero":
        W[:] = 0.0
    else:
        raise ValueError(name)
    return b, x0, W


def kind_of_value(v):
    return "nan" if np.isnan(v) else "inf" if np.isinf(v) else "finite"


# ------------------------------------------------------------------ the breakdown systems
BREAKDOWN_N = (1026, 4098, 9002)             # EPT 2, EPT 8, the two-launch sparse loop
BREAKDOWN_DENSE_N = 1026


def breakdown(n):
    assert n % 2 == 0
    return ss._csr(sp.diags(np.concatenate([np.ones(n // 2), -np.ones(n // 2)])))


def breakdown_dense(n=BREAKDOWN_DENSE_N):
    """(S blocks, Π blocks, gather lists, node_Γ_cnt, n_Γ)"""
    d = np.concatenate([np.full(n // 2, 0.5), np.full(n // 2, -0.5)])
    g = [np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64)]
    return ([np.asfortranarray(np.diag(d)) for _ in range(2)], [np.asfortranarray(np.eye(n)) for _ in range(2)], g,
            np.full(n, 2, dtype=np.int64), n)


def breakdown_history(n):
    with np.errstate(all="ignore"):
        return np.array([np.sqrt(float(n)), np.inf, np.nan])


# ------------------------------------------------------------------ problems beyond krylov_synth's tables
TRI = "tridiag9001"                         # sparse_synth's two-launch solver case
EIG = "synth1025"                           # eig_synth.matrix(1025), Jacobi
EIG_NVEC, EIG_SPDIM = 3, 8                  # the window of eig_synth's groups a, b, f; spdim > 3: the breakdown never restarts
EXTRA_SPARSE = {TRI: 9001, EIG: 1025, **{f"brk{n}": n for n in BREAKDOWN_N}}
BRK_DENSE = f"brkd{BREAKDOWN_DENSE_N}"
# The Krylov workspace of a context is keyed by n, so a breakdown leaves its Inf / NaN in the workspace of ITS size: the clean
# solves around a breakdown run at the same n (krylov_synth.banded / sparse_synth.tridiag / eig_synth.matrix accept any n), and
# the dense pair swaps its blocks on the same two operators (set_blocks) for diagonally dominant ones on the same maps.
BRK_CLEAN = {"brk1026": "band1026", "brk4098": "band4098", "brk9002": "tridiag9002", BRK_DENSE: "pair1026"}
EXTRA_SPARSE.update({"band1026": 1026, "band4098": 4098, "tridiag9002": 9002, "synth1026": 1026})
PAIR = "pair1026"
PAIR_SEED = 97


def is_breakdown(prob):
    return prob.startswith("brk")


@dataclass(frozen=True)
class Call:
    prob: str
    kind: str
    nvec: int = 0
    spdim: int = 0
    x0: str = "zero"             # zero | rand
    maxit: int = 0
    eps_: float = 0.0

    @property
    def eps(self):
        if self.eps_:
            return self.eps_
        if self.prob in ks.SPARSE or self.prob in ks.DENSE:
            return ks.Solve(self.prob, self.kind, self.nvec).eps
        return ks.EPS

    @property
    def id(self):
        return f"{self.prob}-{self.kind}" + (f"-{self.nvec}" if self.nvec else "") + ("-x0" if self.x0 == "rand" else "") + \
            (f"-maxit{self.maxit}" if self.maxit else "")

    def as_solve(self):
        return ks.Solve(self.prob, self.kind, self.nvec, self.x0, self.maxit, self.eps_)


def eig_call(kind, prob=EIG):
    """the clean call of an eigCG-family solver: the stop `after` of eig_synth (two iterations past the first restart, eps
    tiny: ends on maxit, a decided stop); initcg / initpcg at the same length as the deflated kinds"""
    deflated = kind not in ("eigcg", "eigpcg")
    maxit = es.stops(EIG_NVEC, EIG_SPDIM, deflated)["after"]
    return Call(prob, kind, EIG_NVEC, EIG_SPDIM, "zero", maxit, es.TINY)


def eig_start_call(kind, prob=EIG):
    """eigcg / eigpcg stopped at it = 1 (eig_synth's stop `start`): one Lanczos column, the other nvec - 1 returned columns zeros"""
    return Call(prob, kind, EIG_NVEC, EIG_SPDIM, "zero", es.stops(EIG_NVEC, EIG_SPDIM, False)["start"], es.TINY)


def run_call(mod, c, A, M, b, x0, W, maxit=None):
    """a Call on `mod` (the oracle module or the package's api: the same signatures); (x, it, res_norm[, V])"""
    maxit = c.maxit if maxit is None else maxit
    k = c.kind
    if k == "cg":
        return mod.cg(A, b, x0, maxit, c.eps)
    if k in ("pcg", "pcg_id"):
        return mod.pcg(A, b, x0, M, maxit, c.eps)
    if k == "defcg":
        return mod.defcg(A, b, x0, W, maxit, c.eps)
    if k == "defpcg":
        return mod.defpcg(A, b, x0, W, M, maxit, c.eps)
    if k == "initcg":
        return mod.initcg(A, b, x0, W, maxit, c.eps)
    if k == "initpcg":
        return mod.initpcg(A, b, x0, M, W, maxit, c.eps)
    return es.run(mod, k, A, M, b, x0, W, c.nvec, c.spdim, maxit, c.eps)


def outcome(mod, fn):
    """("ok", result) | ("singular", None) | ("bounds", None); anything else a call raises is not an accepted outcome"""
    try:
        with np.errstate(all="ignore"):
            return "ok", fn()
    except mod.SingularException:
        return "singular", None
    except mod.BoundsError:
        return "bounds", None


class Problems:
    """krylov_synth.Problems for its own names, plus tridiag(9001), eig_synth's matrix(1025) and the breakdown systems."""

    def __init__(self, orc, pinv=None):
        self.orc = orc
        self.ks = ks.Problems(orc, pinv)
        self._mat, self._ops, self._W, self._res, self._brk, self._pair = {}, {}, {}, {}, None, None

    def n(self, prob):
        if prob in EXTRA_SPARSE:
            return EXTRA_SPARSE[prob]
        return BREAKDOWN_DENSE_N if prob in (BRK_DENSE, PAIR) else ks.size_of(prob)

    def is_dense(self, prob):
        return prob in ks.DENSE or prob in (BRK_DENSE, PAIR)

    def matrix(self, prob):
        if prob in ks.SPARSE:
            return self.ks.matrix(prob)
        if prob not in self._mat:
            n = EXTRA_SPARSE[prob]
            self._mat[prob] = ss.tridiag(n) if prob.startswith("tridiag") else es.matrix(n) if prob.startswith("synth") else \
                ks.banded(n) if prob.startswith("band") else breakdown(n)
        return self._mat[prob]

    def dense(self, prob):
        """(S blocks, Π blocks, gather lists, node_Γ_cnt, n_Γ)"""
        if prob == BRK_DENSE:
            if self._brk is None:
                self._brk = breakdown_dense()
            return self._brk
        if prob == PAIR:
            if self._pair is None:
                _, _, g, cnt, n = self.dense(BRK_DENSE)
                S = ks.dd_blocks((n, n), PAIR_SEED)
                self._pair = (S, self.ks.pinv(ks.Dense(PAIR, n, 2, (n, n), PAIR_SEED), S), g, cnt, n)
            return self._pair
        g, cnt, n = self.ks.maps(prob)
        return self.ks.blocks(prob), self.ks.pi_blocks(prob), g, cnt, n

    def b(self, prob, kind=None):
        """the right-hand side; on the eigCG problem the deflated kinds get a second one, as in eig_synth (W comes from the first)"""
        n = self.n(prob)
        if is_breakdown(prob):
            return np.ones(n)
        if prob.startswith("synth"):
            return es.rhs(n, 1 if kind is not None and takes_W(kind) else 0)
        return ss.solver_rhs(n) if prob.startswith("tridiag") else ks.rhs(n)

    def x0(self, c):
        n = self.n(c.prob)
        return ks.x0_rand(n) if c.x0 == "rand" else np.zeros(n)

    def W(self, c):
        if not takes_W(c.kind):
            return None
        key = (c.prob, c.nvec)
        if c.prob.startswith("synth"):
            # eig_synth's "chain": the oracle's eigpcg / eigcg result on the first right-hand side (random columns leave a Ritz
            # gap of 6e-4 ... 9e-4 in eigdefpcg's extraction, below eig_synth.GAP_MIN)
            pre = c.kind not in UNPRECONDITIONED
            key = (c.prob, c.nvec, pre)
            if key not in self._W:
                A, n = self.op(c.prob, "A"), self.n(c.prob)
                with np.errstate(all="ignore"):
                    self._W[key] = self.orc.eigpcg(A, self.b(c.prob), np.zeros(n), self.op(c.prob, "jacobi"), c.nvec, EIG_SPDIM)[3] if pre \
                        else self.orc.eigcg(A, self.b(c.prob), np.zeros(n), c.nvec, EIG_SPDIM)[3]
        elif key not in self._W:
            self._W[key] = ks.random_W(self.n(c.prob), c.nvec)
        return self._W[key]

    def precond(self, c):
        if c.kind in UNPRECONDITIONED:
            return None
        if self.is_dense(c.prob):
            return "nn"
        # (the diagonal of a breakdown matrix is indefinite: its preconditioned kinds run with the identity)
        return "identity" if c.kind == "pcg_id" or is_breakdown(c.prob) else "jacobi"

    def op(self, prob, which):
        if prob in ks.SPARSE or prob in ks.DENSE:
            return self.ks.op(prob, which)
        key = (prob, which)
        if key not in self._ops:
            orc = self.orc
            if prob in (BRK_DENSE, PAIR):
                S, Pi, g, cnt, n = self.dense(prob)
                self._ops[key] = orc.apply_local_schurs_operator(S, g, n) if which == "A" else orc.neumann_neumann_operator(Pi, g, cnt)
            else:
                A = self.matrix(prob)
                self._ops[key] = {"A": lambda: orc.csc_operator(A), "jacobi": lambda: orc.jacobi_operator(A.diagonal()),
                                  "identity": lambda: orc.identity_operator(A.shape[0])}[which]()
        return self._ops[key]

    def solve(self, c, poison=None):
        """the oracle's outcome of a Call (with a poison: capped at POISON_MAXIT unless the call has a smaller cap), once"""
        key = (c, poison)
        if key not in self._res:
            pre = self.precond(c)
            A, M = self.op(c.prob, "A"), self.op(c.prob, pre) if pre else None
            b, x0, W = self.b(c.prob, c.kind), self.x0(c), self.W(c)
            maxit = c.maxit
            if poison:
                b, x0, W = poisoned(poison, b, x0, W)
                maxit = poison_maxit(c)
            self._res[key] = outcome(self.orc, lambda: run_call(self.orc, c, A, M, b, x0, W, maxit))
        return self._res[key]

    def drop(self, prob):
        if prob in ks.DENSE:
            self.ks.drop(prob)
        self._res = {k: v for k, v in self._res.items() if k[0].prob != prob}


def poison_maxit(c):
    return min(c.maxit, POISON_MAXIT) if c.maxit else POISON_MAXIT


def numpy_solve(probs, c, maxit):
    """the Call with numpy's products and pairwise sums (krylov_synth.numpy_krylov); cg / pcg / pcg_id only"""
    A = probs.matrix(c.prob) if not probs.is_dense(c.prob) else None
    if A is not None:
        apply_A = lambda v: A @ v                                          # noqa: E731
        M = None if c.kind == "cg" else (lambda v: v.copy()) if c.kind == "pcg_id" else (lambda v: v / A.diagonal())
    else:
        S, Pi, g, cnt, n = probs.dense(c.prob)
        cf = cnt.astype(np.float64)

        def apply_A(v):
            y = np.zeros(n)
            for B, gd in zip(S, g):
                y[gd] += B @ v[gd]
            return y

        def nn(v):
            y = np.zeros(n)
            for B, gd in zip(Pi, g):
                y[gd] += (B @ (v[gd] / cf[gd])) / cf[gd]
            return y
        M = None if c.kind == "cg" else nn
    with np.errstate(all="ignore"):
        return ks.numpy_krylov(apply_A, M, None, probs.b(c.prob, c.kind), probs.x0(c), c.eps, maxit)


# ------------------------------------------------------------------ what the GPU file runs, group by group
@dataclass(frozen=True)
class Form:
    name: str
    env: tuple = ()              # environment switches set to "1" around every solve


DEFAULT = Form("default")
SPARSE_FORMS = (DEFAULT, Form("MI355_NO_FUSED", ("MI355_NO_FUSED",)))
TRI_FORMS = (DEFAULT, Form("MI355_NO_CSRFOLD", ("MI355_NO_CSRFOLD",)))
DENSE_FORMS = (DEFAULT, Form("MI355_NO_FOLD", ("MI355_NO_FOLD",)))
BIG_FORMS = (DEFAULT, Form("MI355_NO_BIG_FOLD", ("MI355_NO_BIG_FOLD",)))
DEFL_FORMS = (DEFAULT, Form("MI355_NO_FOLD_DEFL", ("MI355_NO_FOLD_DEFL",)))


def _sparse_calls(prob):
    return [Call(prob, k, x0=x) for k in ("cg", "pcg", "pcg_id") for x in ("zero", "rand")]


# (problem, forms, clean calls)
SPARSE_GROUP = [("sp1025", SPARSE_FORMS, _sparse_calls("sp1025")), ("sp8192", SPARSE_FORMS, _sparse_calls("sp8192")),
                (TRI, TRI_FORMS, [Call(TRI, k) for k in ("cg", "pcg", "pcg_id")])]
DENSE_GROUP = [("d1025w4", DENSE_FORMS, [Call("d1025w4", "pcg"), Call("d1025w4", "pcg", x0="rand")]),
               ("d4097w4", DENSE_FORMS, [Call("d4097w4", "pcg"), Call("d4097w4", "pcg", x0="rand")]),
               ("d2048w1", DENSE_FORMS, [Call("d2048w1", "pcg"), Call("d2048w1", "cg")]),      # unfolded: view_load's generic loop
               ("big8200", BIG_FORMS, [Call("big8200", "pcg"), Call("big8200", "pcg", x0="rand")])]
F32_PROB = "d1025w4"
DEFL_PROB = "nloc1024"
DEFL_NVEC = (5, 21)
DEFL_GROUP = [(Call(DEFL_PROB, "defpcg", nv), DEFL_FORMS) for nv in DEFL_NVEC] + [(Call(DEFL_PROB, "defcg", nv), (DEFAULT,)) for nv in DEFL_NVEC]
EIG_GROUP = [eig_call(k) for k in EIG_KINDS]
BREAKDOWN_KINDS = ("cg", "pcg_id", "eigcg", "eigpcg")


def breakdown_call(prob, kind):
    if kind.startswith("eig"):
        return Call(prob, kind, 2, 8, "zero", POISON_MAXIT, ks.EPS)
    return Call(prob, "pcg" if prob == BRK_DENSE else kind, maxit=POISON_MAXIT, eps_=ks.EPS)


BREAKDOWN_CALLS = [breakdown_call(f"brk{n}", k) for n in BREAKDOWN_N for k in BREAKDOWN_KINDS] + [breakdown_call(BRK_DENSE, "pcg")]


def breakdown_pairs():
    """(clean call, breakdown call, forms): the clean solve runs before and after the breakdown, at the same n"""
    out = []
    for n, forms in zip(BREAKDOWN_N, (SPARSE_FORMS, SPARSE_FORMS, TRI_FORMS)):
        for kind in ("cg", "pcg_id"):
            out.append((Call(BRK_CLEAN[f"brk{n}"], kind), breakdown_call(f"brk{n}", kind), forms))
    out.append((Call(PAIR, "pcg"), breakdown_call(BRK_DENSE, "pcg"), DENSE_FORMS))
    return out


def eig_breakdown_pairs():
    """eigcg / eigpcg (identity) on the breakdown matrix of n = 1026, between clean calls on eig_synth.matrix(1026)"""
    return [(eig_call(k, "synth1026"), breakdown_call("brk1026", k)) for k in ("eigcg", "eigpcg")]


def clean_calls():
    """every clean solve of the suite that runs to its tolerance (the eigCG family ends on maxit)"""
    out = [c for _, _, calls in SPARSE_GROUP for c in calls] + [c for _, _, calls in DENSE_GROUP for c in calls] + \
        [c for c, _ in DEFL_GROUP] + [c for c, _, _ in breakdown_pairs()]
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


# ------------------------------------------------------------------ interior CG
ICG_MAX_ROWS = 300


def interior_sets():
    """`mixed` of sparse_synth with its 5000-row subdomain cut to 300 rows (every n_i <= 300: a stop rule that misses a NaN
    runs n_i iterations), and `capped`. name -> (set, the subdomain that is poisoned)"""
    wide_vals = np.linspace(1.0, 100.0, 12)
    blocks = [ss.diag(1), ss.tridiag(2, 1.0), ss.diag(300, wide_vals), ss.tridiag(300, 0.05), sp.csr_matrix((0, 0))]
    mixed = ss.interior_set(blocks, [1.0, 5.0, 100.0, 81.0, 1.0], 1e-9, zero_rhs=(ss.MIXED_ZERO_RHS,))
    return {"mixed": (mixed, 3), "capped": (ss.interior_sets(("capped",))["capped"], 0)}


def interior_rhs(s, dom=None, value=np.nan, zero=False):
    """the concatenated b_I; with `dom`: one entry of that subdomain set to `value`, or the whole subdomain zeroed"""
    parts = [np.array(v, dtype=np.float64) for v in s.b_I]
    if dom is not None:
        if zero:
            parts[dom][:] = 0.0
        else:
            parts[dom][parts[dom].size // 2] = value
    return np.concatenate(parts)
