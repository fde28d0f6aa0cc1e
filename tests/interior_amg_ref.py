"""numpy restatement of the device interior CG with `Pl` = AMG (`mi_schur_interior_amg`, DESIGN §6g "Interior `Pl`"), the reference of
tests/test_interior_amg_cpu.py and tests/test_gpu_interior_amg.py.

The `Pl` is ONE hierarchy of the stacked matrix blockdiag(A_IIdd): `fem.prepare_amg_precond` on it (or `fem.amg_refresh` on
its aggregates for a second set of values), applied by `amg_ref.cycle` to the whole stacked vector. The iteration is
`IterativeSolvers.cg(A, b; Pl, reltol)` per subdomain d, all subdomains side by side:

    x = 0, r = b, z = Pl \\ r, ρ = z'r, u = z, tol = reltol ‖b‖_d, maxiter = n_d
    while ‖r‖_d > tol and it < maxiter:
        c = A u; α = ρ / u'c; x += α u; r -= α c; z = Pl \\ r; ρ_new = z'r; u = z + (ρ_new / ρ) u; ρ = ρ_new; it += 1

A subdomain that has stopped is frozen. `Pl = "diagonal"` gives the diagonal `Pl` the counts are compared with.

The cases: what both test files run. Every right-hand side used for an iteration-count equality is listed here with its
seed, and test_interior_amg_cpu.py asserts for each that every subdomain stops with ‖r‖ <= 0.95 tol after a step with
‖r‖ >= 1.05 tol — a count that a rounding difference between numpy and the device cannot move."""
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import amg_ref as ar
import sparse_synth as ss
from conftest import f_m1, lognormal_coeff, one, u0734

RELTOL = 1e-9


def stack(blocks):
    """(sorted CSR of blockdiag(blocks), offsets[ndom + 1])"""
    blocks = [sp.csr_matrix(A) for A in blocks]
    offs = np.concatenate([[0], np.cumsum([A.shape[0] for A in blocks])]).astype(np.int64)
    A = sp.block_diag(blocks, format="csr") if offs[-1] else sp.csr_matrix((0, 0))
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A, offs


def csc_values(blocks):
    """the `ii_val` of `set_values`: the blocks' CSC nzval (sorted), concatenated"""
    out = []
    for A in blocks:
        A = sp.csc_matrix(A)
        A.sort_indices()
        out.append(np.asarray(A.data, dtype=np.float64))
    return np.concatenate(out) if out else np.zeros(0)


def pcg_domains(A, offs, b, Pl, reltol=RELTOL, rz=None):
    """The iteration above. Pl: a function on the stacked vector, or None. Returns (x, its[d], hist[d] = [‖r‖ after 0, 1,
    ... steps], tol[d]). `rz(r, z, s)`: a stand-in for the r'z of the rows s of one subdomain (`block_rz`: the sum of the
    per-row-block partials of k_amg_post_dot, with a seeded fault)."""
    rz = rz or (lambda r, z, s: r[s] @ z[s])
    nd = offs.size - 1
    sl = [slice(int(offs[d]), int(offs[d + 1])) for d in range(nd)]
    M = Pl if Pl is not None else (lambda r: r.copy())
    x, r = np.zeros_like(b), b.copy()
    z = M(r)
    u = z.copy()
    rho = np.array([rz(r, z, s) for s in sl])
    res = np.array([np.sqrt(r[s] @ r[s]) for s in sl])
    tol = reltol * res
    done = ~(res > tol)
    its = np.zeros(nd, dtype=np.int64)
    hist = [[float(v)] for v in res]
    while not done.all():
        c = A @ u
        for d in np.flatnonzero(~done):
            s = sl[d]
            alpha = rho[d] / (u[s] @ c[s])
            x[s] += alpha * u[s]
            r[s] -= alpha * c[s]
        z = M(r)
        for d in np.flatnonzero(~done):
            s = sl[d]
            res[d] = np.sqrt(r[s] @ r[s])
            rho_new = rz(r, z, s)
            u[s] = z[s] + (rho_new / rho[d]) * u[s]
            rho[d] = rho_new
            its[d] += 1
            hist[d].append(float(res[d]))
            done[d] = (not res[d] > tol[d]) or its[d] >= (s.stop - s.start)
    return x, its, hist, tol


def block_rz(blk, drop=None, rows_cap=None):
    """r'z of a subdomain as the sum of the partials of its row blocks `blk` ([nb, 4]: r0, r1, k0, k1, cut at the subdomain
    boundaries). Faults: `drop`: the partial of that block is left out; `rows_cap`: only the first rows_cap rows of every
    block are summed (a row pass that is lost)."""
    def rz(r, z, s):
        tot = 0.0
        for k, (r0, r1, _, _) in enumerate(blk):
            if r0 >= s.start and r1 <= s.stop and k != drop:
                r1 = r1 if rows_cap is None else min(r1, r0 + rows_cap)
                tot += r[r0:r1] @ z[r0:r1]
        return tot
    return rz


def solution_bars(C, fem, its):
    """Per subdomain, the bar of ‖u_device - u_restated‖ / ‖u_restated‖ for a solve of `its[d]` steps that both sides end at
    the same count. Both run the same recurrences and differ by rounding alone: a step applies A and one cycle, six chains
    of inner products (A, down, restrict, coarse, prolong, post) whose running error is at most (L + 3) u relative to the
    absolute-valued result, L the longest row of A_0, P_0 and R_0; a perturbation of the iterate reaches the solution
    amplified by at most κ_d (a Gershgorin bound, the matrices are diagonally dominant); 2 for the two sides:
    2 its_d 6 (L + 3) u κ_d. A first-order model, written before any device figure was seen; tests/test_amg_edges_cpu.py
    asserts that every seeded fault of the r'z partials that keeps the count moves the restated solution by more than it."""
    H = C.hierarchy(fem)
    L = max(int(np.diff(sp.csr_matrix(M).indptr).max(initial=0)) for M in (H.A[0], H.P[0], sp.csr_matrix(H.P[0].T)))
    kap = [ss.gershgorin_kappa(A) if A.shape[0] else 1.0 for A in C.A_II]
    return np.array([2.0 * max(int(i), 1) * 6 * (L + 3) * 2.0 ** -52 * k for i, k in zip(its, kap)])


def amg_pl(H):
    return lambda r: ar.cycle(H, r)


def diag_pl(A):
    dinv = 1.0 / A.diagonal()
    return lambda r: dinv * r


def margins(hist, tol):
    """per subdomain with at least one step: (stopping residual / tol, the one before it / tol)"""
    return [(h[-1] / t, h[-2] / t) for h, t in zip(hist, tol) if len(h) > 1]


@dataclass
class Case:
    """One operator: its blocks, interface wiring, the set-up keywords of the `Pl`, a second set of values on the same
    patterns, the seeds of the Γ vectors, and the dense S_d of both sets of values."""
    name: str
    A_II: list
    A_IΓ: list
    A_ΓΓ: list
    gather_idx: list
    node_Γ_cnt: np.ndarray
    kw: dict
    seed: int                       # x = default_rng(seed).standard_normal(n_Γ): the apply of the count equality
    A_II2: list = None              # second values (check 6)
    A_IΓ2: list = None
    A_ΓΓ2: list = None
    seed2: int = 0
    b_Id: list = None
    b_Γ: np.ndarray = None
    aggs: list = None               # frozen aggregates (one array per smoothed level, over the stacked rows) in place of `kw`
    cache: dict = field(default_factory=dict)

    @property
    def n_Γ(self):
        return int(np.size(self.node_Γ_cnt))

    def x(self, second=False):
        return np.random.default_rng(self.seed2 if second else self.seed).standard_normal(self.n_Γ)

    def b_I(self):
        return np.concatenate([np.asarray(b, dtype=np.float64) for b in self.b_Id])

    def host_solvers(self, second=False):
        """sparse direct A_IId^-1 per subdomain (the identity on an empty interior)"""
        return [spla.splu(sp.csc_matrix(A)).solve if A.shape[0] else (lambda r: r) for A in self.blocks(second)[0]]

    def blocks(self, second=False):
        return (self.A_II2, self.A_IΓ2, self.A_ΓΓ2) if second else (self.A_II, self.A_IΓ, self.A_ΓΓ)

    def stacked(self, second=False):
        return stack(self.blocks(second)[0])

    def hierarchy(self, fem, second=False):
        """prepare_amg_precond on the first values; amg_refresh on ITS aggregates for the second (with `aggs`: amg_refresh
        on them for both)"""
        key = ("H", second)
        if key not in self.cache:
            if self.aggs is not None:
                self.cache[key] = fem.amg_refresh(self.aggs, self.stacked(second)[0])
            elif second:
                self.cache[key] = fem.amg_refresh(self.hierarchy(fem), self.stacked(True)[0])
            else:
                self.cache[key] = fem.prepare_amg_precond(self.stacked()[0], **self.kw)
        return self.cache[key]

    def interior_rhs(self, x, second=False):
        _, A_IΓ, _ = self.blocks(second)
        return np.concatenate([sp.csr_matrix(A_IΓ[d]) @ x[self.gather_idx[d]] for d in range(len(A_IΓ))])

    def s_apply(self, x, v, second=False):
        """y = Σ_d R_d' (A_ΓΓdd x_d - A_IΓdd' v_d) with v the stacked interior solutions"""
        _, A_IΓ, A_ΓΓ = self.blocks(second)
        _, offs = self.stacked(second)
        y = np.zeros(self.n_Γ)
        for d in range(len(A_IΓ)):
            g = self.gather_idx[d]
            y[g] += sp.csr_matrix(A_ΓΓ[d]) @ x[g] - sp.csr_matrix(A_IΓ[d]).T @ v[offs[d]:offs[d + 1]]
        return y

    def Sd(self, second=False):
        """dense local Schur complements by a sparse direct solve, column-major"""
        key = ("Sd", second)
        if key not in self.cache:
            A_II, A_IΓ, A_ΓΓ = self.blocks(second)
            out = []
            for d in range(len(A_II)):
                G = sp.csc_matrix(A_IΓ[d]).toarray()
                S = sp.csc_matrix(A_ΓΓ[d]).toarray()
                if A_II[d].shape[0]:
                    S = S - G.T @ spla.splu(sp.csc_matrix(A_II[d])).solve(G)
                out.append(np.asfortranarray((S + S.T) * 0.5))
            self.cache[key] = out
        return self.cache[key]

    def exact_apply(self, x, second=False):
        y = np.zeros(self.n_Γ)
        for d, S in enumerate(self.Sd(second)):
            g = self.gather_idx[d]
            y[g] += S @ x[g]
        return y

    def solve_b(self, fem, rz=None):
        """the restated interior solve of `interior_solutions(0, b_I)`: data in every row of every block"""
        key = ("solve_b",)
        if rz is not None or key not in self.cache:
            A, offs = self.stacked()
            out = pcg_domains(A, offs, self.b_I(), amg_pl(self.hierarchy(fem)), rz=rz)
            if rz is not None:
                return out
            self.cache[key] = out
        return self.cache[key]

    def solve(self, fem, x, second=False, pl="amg"):
        """the restated interior solve of the apply to x: (v, its, hist, tol)"""
        key = ("solve", second, pl, x.tobytes())
        if key not in self.cache:
            A, offs = self.stacked(second)
            Pl = amg_pl(self.hierarchy(fem, second)) if pl == "amg" else diag_pl(A) if pl == "diagonal" else None
            self.cache[key] = pcg_domains(A, offs, self.interior_rhs(x, second), Pl)
        return self.cache[key]


# name -> (seed of the first apply, seed of the apply after set_values); chosen so that the margins hold (asserted in
# test_interior_amg_cpu.py::test_counts_are_not_marginal)
SEEDS = {"ragged": (22, 5), "n12_3": (1, 2), "n12_1": (1, 2), "blocks2": (1, 2), "empty": (1, 2)}
NAMES = tuple(SEEDS)
# the cases on row-block edges (tests/test_gpu_amg_edges.py), with hand-made aggregates: pairs of consecutive rows within
# each subdomain. Their right-hand sides are multiples of e_0 per subdomain, so the seed scales them and nothing else.
EDGE_SEEDS = {"edge_long": (1, 2), "edge_rows": (1, 2)}
EDGE_NAMES = tuple(EDGE_SEEDS)
_cases = {}


def _fem_case(fem, name, N, px, py, coeff_seeds, kw):
    mesh = fem.get_mesh(N)
    c1 = lognormal_coeff(fem, mesh.points, coeff_seeds[0]) if coeff_seeds[0] is not None else one
    P = fem.build_schur_problem(N, px, py, c1, f_m1, u0734, assemble=False, precond=False)
    c2 = lognormal_coeff(fem, mesh.points, coeff_seeds[1])
    A2, G2, S2, _, _ = fem.prepare_local_schurs(P.mesh.cells, P.mesh.points, P.epart, P.sub, c2, f_m1, u0734)
    s1, s2 = SEEDS[name]
    return Case(name, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd, P.sub.gather_idx, P.sub.node_Γ_cnt, kw, s1, A2, G2, S2, s2, P.b_Id, P.b_Γ)


def pair_aggregates(blocks):
    """aggregates of two consecutive rows, none across a subdomain boundary: (sizes, [agg]) of a two-level hierarchy"""
    agg, base = [], 0
    for A in blocks:
        n = A.shape[0]
        agg.append(base + np.arange(n, dtype=np.int64) // 2)
        base += (n + 1) // 2
    agg = np.concatenate(agg)
    return [int(agg.size), int(base)], [agg]


def _synthetic_case(name, blocks, kw, aggs=None):
    """sparse_synth's trivial interface wiring; the second values: every block scaled row- and column-wise by a smooth
    positive field (D A D, D = diag(1 + 0.3 sin(i / 17))): SPD on the same pattern. (These right-hand sides are a multiple
    of e_0 whatever the seed, so the margin of the count is a property of the values: amplitude and period were picked for it.)"""
    S = ss.interior_set(blocks, [1.0] * len(blocks), RELTOL)
    A2 = []
    for A in S.A_II:
        n = A.shape[0]
        D = sp.diags(1.0 + 0.3 * np.sin(np.arange(n) / 17.0)) if n else sp.csr_matrix((0, 0))
        A2.append(sp.csc_matrix(D @ sp.csr_matrix(A) @ D) if n else A)
    s1, s2 = SEEDS[name] if name in SEEDS else EDGE_SEEDS[name]
    return Case(name, S.A_II, S.A_IΓ, S.A_ΓΓ, S.gather_idx, S.node_Γ_cnt, kw, s1, A2, S.A_IΓ, S.A_ΓΓ, s2, S.b_I, np.zeros(S.n_Γ), aggs)


def case(fem, name):
    """ragged: N = 50, 3 x 2, lognormal (conftest's fixture), 2162 -> 400 -> 50. n12_3: N = 12, 2 x 2, max_coarse = 16:
    three levels, interiors smaller than a row block. n12_1: the same with the default max_coarse: the dense inverse alone.
    blocks2: grid_like blocks of 1023 and 1025 rows: a subdomain boundary beside a row-block boundary. empty: a subdomain
    without interior between two others. edge_long: arrow(1500, 1025) (a row longer than the tile, alone in its row block),
    a subdomain of one row, diag(1025) (stacked at an odd offset: 1023 rows in one block, then a block of two rows).
    edge_rows: tridiag(1023), an empty interior, tridiag(1025) (blocks of two and five rows before the subdomain boundaries).
    Both with pair_aggregates; tests/test_interior_amg_cpu.py asserts these block shapes with the host check."""
    if name not in _cases:
        if name == "ragged":
            _cases[name] = _fem_case(fem, name, 50, 3, 2, (7, 8), {})
        elif name == "n12_3":
            _cases[name] = _fem_case(fem, name, 12, 2, 2, (None, 8), dict(max_coarse=16))
        elif name == "n12_1":
            _cases[name] = _fem_case(fem, name, 12, 2, 2, (None, 8), {})
        elif name == "blocks2":
            _cases[name] = _synthetic_case(name, [ar.grid_like(1023, 0), ar.grid_like(1025, 1)], {})
        elif name == "empty":
            _cases[name] = _synthetic_case(name, [ar.grid_like(300, 2), sp.csr_matrix((0, 0)), ar.grid_like(500, 3)], dict(max_coarse=64))
        elif name in ("edge_long", "edge_rows"):
            blocks = ([ss.arrow(1500, 1025), ss.diag(1), ss.diag(1025)] if name == "edge_long" else
                      [ss.tridiag(1023), sp.csr_matrix((0, 0)), ss.tridiag(1025)])
            _cases[name] = _synthetic_case(name, blocks, {}, pair_aggregates(blocks)[1])
        else:
            raise KeyError(name)
    return _cases[name]


# ------------------------------------------------------------------ what the GPU suites share
def op(api, ctx, C, second=False, **kw):
    A_II, A_IΓ, A_ΓΓ = C.blocks(second)
    return api.MatrixFreeLocalSchurs(ctx, A_II, A_IΓ, A_ΓΓ, C.gather_idx, C.node_Γ_cnt, None, reltol=RELTOL, **kw)


def new_values(C):
    """set_values arguments for the case's second values (None where the case keeps the first ones)"""
    ig = None if C.A_IΓ2 is C.A_IΓ else csc_values(C.A_IΓ2)
    gg = None if C.A_ΓΓ2 is C.A_ΓΓ else csc_values(C.A_ΓΓ2)
    return csc_values(C.A_II2), ig, gg


def residuals(C, u, b, second=False, blocks=None):
    A, offs = C.stacked(second) if blocks is None else stack(blocks)
    r = b - A @ u
    return [(np.linalg.norm(r[offs[d]:offs[d + 1]]), np.linalg.norm(b[offs[d]:offs[d + 1]])) for d in range(offs.size - 1)]


def close(y, exact):
    err = np.abs(y - exact).max() / np.abs(exact).max()
    return err
