"""Inputs and stop-table arithmetic for the edge suite of the eigCG family (csrc/eig_solvers.hpp, csrc/eig_kernels.hpp,
eig_record() in csrc/solvers.hpp).

Not a conftest: tests/test_eig_edges_cpu.py and tests/test_gpu_eig_edges.py import it. Everything here runs on the host.

  matrix(n)   tridiag(n, 0.01) + diag(linspace(0, 3, n)^2): SPD, eigenvalues from ~0.01 to ~13 with the low end well
              separated (the diagonal grows quadratically), so the Ritz values a short window sees have gaps.
  rhs / x0    seeded standard-normal vectors.
  stops()     the named `maxit` values at which a solve with eps = 1e-300 ends in a given state of the window.
  CASES       every (kind, nvec, spdim, stop) the GPU file runs, as data: the CPU file proves `it == maxit`, the state and
              the gap condition for each of them; the GPU file runs them on the device.

The window (eigcg.jl / defcg.jl; 1-based `ivec` as in the reference). L = maxit - 1 loop iterations are run. The first
Lanczos column is i0 = 1 (plain kinds) or nvec + 1 (deflated kinds: V[:, 1:nvec] = W). Iteration k enters with
ivec = i0 + k - 1, so the iteration R1 = spdim - i0 + 1 enters with ivec == spdim and restarts; it leaves ivec = nev + 1
(nev = 2 nvec kept columns) and just_restarted set. The second restart follows spdim - nev iterations later, at R2.
After the loop the preconditioned kinds extract Ritz vectors from the leading m = ivec - 1 columns unless the stop is
the restart itself (just_restarted) or ivec <= nvec; eigvecs(Tm[1:m-1, 1:m-1])[:, 1:nvec] needs m - 1 >= nvec.
"""
from __future__ import annotations

import re
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

import sparse_synth as ss

KINDS = ("eigcg", "eigpcg", "eigdefcg", "eigdefpcg")
PRE = {"eigcg": False, "eigpcg": True, "eigdefcg": False, "eigdefpcg": True}
DEFLATED = {"eigcg": False, "eigpcg": False, "eigdefcg": True, "eigdefpcg": True}
TINY = 1e-300          # eps of every stop case: the tolerance never ends the run
GAP_MIN = 1e-3         # relative gap between Ritz values nvec and nvec + 1 wherever subspaces are compared
POSED_TOL = 1e-8       # 1 % of test_gpu_eig.SUBSPACE_TOL: how far the oracle's own subspace may move under PERTURB
PERTURB = 1e-15        # relative, per entry of b: the size of a summation-order difference in one dot product


def matrix(n):
    return ss._csr(ss.tridiag(n, 0.01) + sp.diags(np.linspace(0.0, 3.0, n) ** 2))


def matrix_slow(n):
    """a weaker grading and a smaller shift: Jacobi-PCG and CG are both at a relative residual of ~5e-6 after 125 iterations
    (n = 257), so the long windows of group d are cut well before convergence"""
    return ss._csr(ss.tridiag(n, 0.001) + sp.diags(0.01 * np.linspace(0.0, 3.0, n) ** 2))


def matrix_mild(n):
    """κ ~ 50: CG converges in ~50 iterations (n = 257, ~20 restarts of an 8-column window). The convergence cases from a
    random x0 run on it: on matrix(n), unpreconditioned eigcg needs 85 iterations and its late Lanczos vectors r / |r| have
    lost so much orthogonality that the ORACLE's own returned subspace moves by 5e-4 when b is perturbed by 1e-15
    (test_eig_edges_cpu.test_subspace_is_well_posed measures this for every case; here 3e-13)."""
    return ss._csr(ss.tridiag(n, 0.1) + sp.diags(np.linspace(0.0, 1.0, n) ** 2))


def rhs(n, seed=0):
    return np.random.default_rng(7100 + seed + n).standard_normal(n)


def x0(n, seed=0):
    return np.random.default_rng(9300 + seed + n).standard_normal(n)


def random_W(n, nvec, seed=0):
    """orthonormalised random columns"""
    return np.asfortranarray(np.linalg.qr(np.random.default_rng(5200 + seed + nvec).standard_normal((n, nvec)))[0])


def diagonal_system(n):
    """(A, x*, b) with A x* == b exactly in floating point: powers of two times small integers."""
    rng = np.random.default_rng(n)
    d = 2.0 ** rng.integers(0, 3, n)
    xs = rng.integers(1, 9, n).astype(np.float64)
    return ss._csr(sp.diags(d)), xs, d * xs


# ------------------------------------------------------------------ the stop table
def stops(nvec, spdim, deflated):
    """name -> maxit. `few` exists for the plain kinds only; for the deflated kinds `start` and `bounds` coincide."""
    i0 = nvec + 1 if deflated else 1
    nev = 2 * nvec
    R1 = spdim - i0 + 1
    R2 = R1 + spdim - nev
    L = {"start": 0, "bounds": nvec + 1 - i0, "least": nvec + 2 - i0, "full": R1 - 1, "restart": R1, "after": R1 + 1,
         "full2": R2 - 1, "restart2": R2, "after2": R2 + 1}
    if not deflated:
        L["few"] = nvec - 1
    return {k: v + 1 for k, v in L.items()}


def expected_state(nvec, spdim, deflated, maxit):
    """(ivec 1-based, just_restarted, restarts) after maxit - 1 loop iterations with nev = 2 nvec at every restart"""
    i0 = nvec + 1 if deflated else 1
    nev = 2 * nvec
    L = maxit - 1
    R1 = spdim - i0 + 1
    if L < R1:
        return i0 + L, False, 0
    period = spdim - nev
    k, rem = divmod(L - R1, period)
    return nev + 1 + rem, rem == 0, k + 1


def extraction_m(kind, nvec, ivec, just_restarted):
    """m of the final extraction: None when none runs, -1 for the BoundsError"""
    if not PRE[kind] or just_restarted or ivec <= nvec:
        return None
    m = ivec - 1
    return -1 if m - 1 < nvec else m


def ritz_gap(T, nvec):
    """relative gap between Ritz values nvec and nvec + 1 (1-based) of the symmetric matrix held in T's upper triangle"""
    w = np.linalg.eigvalsh(np.triu(T) + np.triu(T, 1).T)
    return float((w[nvec] - w[nvec - 1]) / (w[-1] - w[0]))


def decisive_T(state):
    """The projected matrix whose lowest nvec Ritz vectors are the returned columns: the final extraction's Tm, else the
    last restart's; None when plain Lanczos vectors (or W) are returned."""
    if "extract_m" in state:
        m = state["extract_m"]
        return state["VtAV"][:m, :m]
    return state["restart_T"]


# ------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    group: str             # the section of the GPU file that runs it
    kind: str
    prob: str              # "synth<n>" / "slow<n>" / "mild<n>" (matrix / matrix_slow / matrix_mild, Jacobi) or "toy" (Schur, Neumann-Neumann)
    nvec: int
    spdim: int
    stop: str              # a name of stops(), or "conv": default eps, run to convergence
    shift: int = 0         # ±1 iteration under the gap rule (none needed: every case has shift 0)
    x0_seed: int = -1      # >= 0: a random initial guess
    W: str = "chain"       # deflated kinds: "chain" = the oracle's eigpcg / eigcg result on the first right-hand side, "rand"

    @property
    def id(self):
        return f"{self.group}-{self.kind}-{self.prob}-{self.nvec}-{self.spdim}-{self.stop}" + ("-x0" if self.x0_seed >= 0 else "")

    @property
    def maxit(self):
        return 0 if self.stop == "conv" else stops(self.nvec, self.spdim, DEFLATED[self.kind])[self.stop] + self.shift

    @property
    def eps(self):
        return 1e-7 if self.stop == "conv" else TINY


def stop_names(kind):
    names = ["start", "bounds", "least", "full", "restart", "after", "full2", "restart2", "after2"]
    if not DEFLATED[kind]:
        names.insert(1, "few")
    else:
        names.remove("bounds")        # == start
    return names


# rank(Y) at a restart is NOT 2 nvec for long windows: the lowest Ritz vectors of Tm and of Tm[1:m-1, 1:m-1] agree to
# rounding once they have converged inside the window, and the singular values of Y fall geometrically through the
# reference's rank threshold. Measured on the oracle (any of the matrices here): nev = nvec + 12..14. (33, 70) keeps 45
# columns (k_eig_coupling is launched over 66 rows, 21 of them idle); (60, 124) keeps 74, the first pair here whose rank
# decision is a factor > 3 away from the threshold on both sides: the second pass of k_eig_state's 64-thread stride loop.
LONG_WINDOWS = ((33, 70), (60, 124))
LONG_NEV = {(33, 70): 45, (60, 124): 74, (10, 24): 19}     # (10, 24): the large window of the regrowth test


def _cases():
    out = []
    for kind in KINDS:                                              # a. stop states
        for stop in stop_names(kind):
            out.append(Case("a", kind, "synth257", 3, 8, stop))
    for n in (255, 256, 257, 1025):                                 # b. n at the thread edge
        for kind in ("eigpcg", "eigcg"):
            out.append(Case("b", kind, f"synth{n}", 3, 8, "after"))
    for kind in ("eigdefcg", "eigdefpcg"):                          # c. deflated kinds, multi-workgroup loop, slot views
        for stop in ("after", "conv"):
            out.append(Case("c", kind, "toy", 3, 8, stop))
    for kind in ("eigcg", "eigpcg"):                                # d. long windows: 66 coupling rows; more than 64 kept columns
        for nvec, spdim in LONG_WINDOWS:
            for stop in ("restart", "after"):
                out.append(Case("d", kind, "slow257", nvec, spdim, stop))
    for nv in (12, 13, 20, 21):                                     # e. register LU edges
        for stop in ("least", "after"):
            out.append(Case("e", "eigdefcg", "synth257", nv, 2 * nv + 2, stop, W="rand"))
    for kind in KINDS:                                              # f. nonzero x0
        for stop in ("after", "conv"):
            out.append(Case("f", kind, "mild257" if stop == "conv" else "synth257", 3, 8, stop, x0_seed=1))
    out.append(Case("h", "eigpcg", "synth257", 10, 24, "after"))  # h. workspace regrowth: the large window in the middle
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def group(g):
    return [c for c in CASES if c.group == g]


# ------------------------------------------------------------------ realising a case on the oracle
class Problems:
    """Operators and vectors per problem name, built once. `toy` is the conftest fixture (or None while only synthetic
    problems are asked for)."""

    def __init__(self, orc, toy=None):
        self.orc, self.toy = orc, toy
        self._ops, self._W, self._res = {}, {}, {}

    def n(self, prob):
        return self.toy.sub.n_Γ if prob == "toy" else int(re.sub(r"\D", "", prob))

    def scipy_matrix(self, prob):
        return {"synth": matrix, "slow": matrix_slow, "mild": matrix_mild}[re.sub(r"\d", "", prob)](self.n(prob))

    def ops(self, prob):
        """(A, M) for the oracle"""
        if prob not in self._ops:
            orc = self.orc
            if prob == "toy":
                P = self.toy
                self._ops[prob] = (orc.apply_local_schurs_operator(P.Sd, P.sub.gather_idx, P.sub.n_Γ),
                                   orc.neumann_neumann_operator(P.ΠSd, P.sub.gather_idx, P.sub.node_Γ_cnt))
            else:
                A = self.scipy_matrix(prob)
                self._ops[prob] = (orc.csc_operator(A), orc.jacobi_operator(A.diagonal()))
        return self._ops[prob]

    def b_first(self, prob):
        return self.toy.b_schur if prob == "toy" else rhs(self.n(prob), 0)

    def b(self, case):
        """the right-hand side of the case: the first one for the plain kinds, a second one for the deflated kinds"""
        if not DEFLATED[case.kind]:
            return self.b_first(case.prob)
        if case.prob == "toy":
            return self.ops("toy")[0](np.random.default_rng(3).standard_normal(self.n("toy")))
        return rhs(self.n(case.prob), 1)

    def x0(self, case):
        n = self.n(case.prob)
        return x0(n, case.x0_seed) if case.x0_seed >= 0 else np.zeros(n)

    def W(self, case):
        if not DEFLATED[case.kind]:
            return None
        key = (case.prob, case.kind, case.nvec, case.spdim, case.W)
        if key not in self._W:
            n = self.n(case.prob)
            if case.W == "rand":
                self._W[key] = random_W(n, case.nvec)
            else:
                A, M = self.ops(case.prob)
                b = self.b_first(case.prob)
                if PRE[case.kind]:
                    self._W[key] = self.orc.eigpcg(A, b, np.zeros(n), M, case.nvec, case.spdim)[3]
                else:
                    self._W[key] = self.orc.eigcg(A, b, np.zeros(n), case.nvec, case.spdim)[3]
        return self._W[key]

    def solve(self, case, maxit=None, perturb=False):
        """The oracle's run of a case, computed once: (result or the BoundsError instance, state). perturb: b with a relative
        noise of PERTURB per entry."""
        key = (case.id, maxit, perturb)
        if key not in self._res:
            state = {}
            b = self.b(case)
            if perturb:
                b = b * (1.0 + PERTURB * np.random.default_rng(17).standard_normal(b.size))
            try:
                with np.errstate(all="ignore"):
                    res = run(self.orc, case.kind, *self.ops(case.prob), b, self.x0(case), self.W(case), case.nvec,
                              case.spdim, case.maxit if maxit is None else maxit, case.eps, state=state)
            except self.orc.BoundsError as e:
                res = e
            self._res[key] = (res, state)
        return self._res[key]


def run(mod, kind, A, M, b, x, W, nvec, spdim, maxit, eps, **kw):
    """kind on `mod` (the oracle module or the package's api: the same signatures)"""
    if kind == "eigcg":
        return mod.eigcg(A, b, x, nvec, spdim, maxit, eps, **kw)
    if kind == "eigpcg":
        return mod.eigpcg(A, b, x, M, nvec, spdim, maxit, eps, **kw)
    if kind == "eigdefcg":
        return mod.eigdefcg(A, b, x, W, spdim, maxit, eps, **kw)
    return mod.eigdefpcg(A, b, x, M, W, spdim, maxit, eps, **kw)
