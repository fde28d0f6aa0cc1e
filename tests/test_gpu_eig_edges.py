"""GPU suite (-m gpu) of the eigCG family (csrc/eig_solvers.hpp, csrc/eig_kernels.hpp, eig_record() in csrc/solvers.hpp) at
the edges of its window, its restarts and its stop states, on the inputs of tests/eig_synth.py. tests/test_eig_edges_cpu.py
proves on the host that every case ends in the state it is named for (it == maxit, ivec, just_restarted, the m of the
final extraction) and that the gap condition holds wherever subspaces are compared.

Bars (none of them new):
  * (x, it, res_norm): test_gpu_parity.assert_history against the oracle.
  * Ritz output: test_gpu_eig.assert_space (sin θ_max <= SUBSPACE_TOL, Ritz values to RITZ_RTOL).
  * where the returned columns are plain Lanczos vectors (no restart and no extraction before the stop: `start`, `few`,
    every stop of eigcg / eigdefcg before the first restart), each column against the oracle's at X_RTOL; a column the
    oracle leaves at zero must be exactly zero.
  * segmentation and workspace regrowth: bit for bit (np.array_equal).
Every case prints its measured errors in units of its bar before it asserts.

Found by this suite and fixed in eig_solvers.hpp: V was not cleared at the start of a solve, so a stop before the window held
nvec columns returned whatever an earlier solve on the context had left in the columns behind the newest Lanczos vector
(NaN after a solve with nothing to iterate). The reference leaves those columns undefined (V = Array(undef, ...)); the oracle
defines them as zeros and the device now does the same. Shown by test_stop_states[a-eigcg-...-start], [a-eigpcg-...-start]
and both cases of test_nothing_to_iterate.

Measured on an MI355X (85 tests, 4 s in all; figures in units of the bar):
  * `it` equal to the oracle in every case, also in the long runs (71 / 72 / 125 / 126 iterations, 79 for initcg).
  * res_norm: <= 7.7e-5 of the tight bar in every solve of at most 50 iterations; the histories of eigcg / eigpcg at
    (33, 70) and (60, 124) are bit-identical to plain cg / pcg at the same maxit. initcg to convergence from a random x0
    (79 iterations, long-run bar): 6.9e3 of the tight bar in its last entries, x at 1.2e-3 of X_RTOL.
  * Lanczos columns: 4.3e-10 of X_RTOL; zero columns exactly zero.
  * subspaces: sin θ <= 2.3e-4 of SUBSPACE_TOL (eigcg (60, 124): 74 kept columns after 124 unpreconditioned iterations),
    2.1e-5 for eigpcg (60, 124) `after`, <= 1e-8 for every (3, 8) stop; Ritz values <= 6.4e-8 of RITZ_RTOL.
  * segmentation (4 kinds x 4 primings) and regrowth (4 calls): every bit equal.
Sensitivity, each defect seeded once into a scratch build and this file run against it: the coupling column of k_eig_state
zeroed: 18 tests fail; its 64-thread stride loop cut to one pass: d-eigpcg-slow257-60-124-after fails (the only case with
more than 64 kept columns AND an extraction that reads the coupling column); `predicted` ignored on every other solve
together with a reversed summation in k_eig_rotate: the four segmentation tests fail; e_spdim as T's leading dimension in
k_eig_state: 17 tests fail, test_workspace_regrowth among them; the parent of this change (V not cleared): the 4 tests above.
"""
import numpy as np
import pytest

import eig_synth as es
from test_gpu_eig import RITZ_RTOL, SUBSPACE_TOL, assert_space, ritz_values, sin_theta
from test_gpu_parity import RES_FLOOR, RES_RTOL, X_RTOL, assert_history, gpu_ops

pytestmark = pytest.mark.gpu

DEFAULT_CHUNK = 8


@pytest.fixture(scope="module")
def probs(orc, toy):
    return es.Problems(orc, toy)


class GpuOps:
    """(A, M) on a context per problem name, built once"""

    def __init__(self, pkg, ctx, probs):
        self.pkg, self.ctx, self.probs, self._ops = pkg, ctx, probs, {}

    def __call__(self, prob):
        if prob not in self._ops:
            api = self.pkg.api
            if prob == "toy":
                self._ops[prob] = gpu_ops(self.pkg, self.ctx, self.probs.toy)
            else:
                A = self.probs.scipy_matrix(prob)
                self._ops[prob] = (api.SparseMatrixCSC(self.ctx, A), api.JacobiPreconditioner(self.ctx, A.diagonal()))
        return self._ops[prob]

    def close(self):
        for A, M in self._ops.values():
            A.close()
            M.close()
        self._ops = {}


@pytest.fixture(scope="module")
def gops(pkg, ctx, probs):
    g = GpuOps(pkg, ctx, probs)
    yield g
    g.close()


def gpu_run(api, ops, probs, case, maxit=None):
    A, M = ops(case.prob)
    return es.run(api, case.kind, A, M, probs.b(case), probs.x0(case), probs.W(case), case.nvec, case.spdim,
                  case.maxit if maxit is None else maxit, case.eps)


def history_margin(got, want):
    """largest res_norm deviation in units of assert_history's tight bar 1e-8 res_k + 1e-12 res_1 (printed, not asserted)"""
    res, reso = got[2], want[2]
    m = min(res.size, reso.size)
    return float(np.max(np.abs(res[:m] - reso[:m]) / (RES_RTOL * reso[:m] + RES_FLOOR * reso[0]))) if m and reso[0] else 0.0


def x_margin(x, xo):
    d = np.linalg.norm(xo)
    return float(np.linalg.norm(x - xo) / (X_RTOL * d)) if d else float(np.linalg.norm(x - xo))


def assert_columns(V, Vo, tag):
    """plain Lanczos vectors: no sign freedom, column by column at X_RTOL; zero columns exactly zero"""
    assert V.shape == Vo.shape
    worst = 0.0
    for j in range(Vo.shape[1]):
        d, ref = np.linalg.norm(V[:, j] - Vo[:, j]), np.linalg.norm(Vo[:, j])
        worst = max(worst, d / (X_RTOL * ref) if ref else (0.0 if d == 0.0 else np.inf))
    print(f"  {tag}: columns, worst |v - v_o| / (X_RTOL |v_o|) = {worst:.3e} (bar 1)")
    assert np.all(np.isfinite(V)) and worst <= 1.0, f"{tag}: column error {worst:.3e} of the bar"


def space_report(apply, V, Vo, tag):
    s = sin_theta(V, Vo)
    r, ro = ritz_values(apply, V), ritz_values(apply, Vo)
    print(f"  {tag}: sin(theta) / SUBSPACE_TOL = {s / SUBSPACE_TOL:.3e}, Ritz rel. error / RITZ_RTOL = "
          f"{np.max(np.abs(r - ro) / np.abs(ro)) / RITZ_RTOL:.3e} (bars 1)")


def compare(case, got, probs, tag=None):
    """one device result against the oracle's run of the case"""
    tag = tag or case.id
    want, st = probs.solve(case)
    Ao = probs.ops(case.prob)[0]
    b = probs.b(case)
    print(f"  {tag}: it {got[1]} (oracle {want[1]}), res_norm / tight bar = {history_margin(got, want):.3e}, "
          f"|x - x_o| / (X_RTOL |x_o|) = {x_margin(got[0], want[0]):.3e}")
    assert_history(got[:3], want[:3], apply=Ao, b=b)
    if es.decisive_T(st) is None:
        assert_columns(got[3], want[3], tag)
    else:
        space_report(Ao, got[3], want[3], tag)
        assert_space(Ao, got[3], want[3])
    return want


# ------------------------------------------------------------------ a. stop states
@pytest.mark.parametrize("case", es.group("a"), ids=lambda c: c.id)
def test_stop_states(pkg, orc, probs, gops, case):
    api = pkg.api
    want, st = probs.solve(case)
    if case.stop in ("start", "few"):
        # the window of an earlier solve is still in the workspace: a full one, every column written
        gpu_run(api, gops, probs, es.BY_ID[f"a-{case.kind}-synth257-3-8-full"])
    if isinstance(want, orc.BoundsError):
        with pytest.raises(api.BoundsError):
            gpu_run(api, gops, probs, case)
        least = es.BY_ID[f"a-{case.kind}-synth257-3-8-least"]        # the context still solves
        compare(least, gpu_run(api, gops, probs, least), probs, tag=f"{least.id} after the BoundsError")
        return
    compare(case, gpu_run(api, gops, probs, case), probs)


# ------------------------------------------------------------------ b. n at the 256-thread edge, both loop forms
@pytest.mark.parametrize("case", es.group("b"), ids=lambda c: c.id)
def test_thread_edge(pkg, probs, gops, monkeypatch, case):
    api = pkg.api
    fused = gpu_run(api, gops, probs, case)
    compare(case, fused, probs, tag=f"{case.id} default")
    if probs.n(case.prob) in (257, 1025):
        monkeypatch.setenv("MI355_NO_FUSED", "1")
        try:
            multi = gpu_run(api, gops, probs, case)
        finally:
            monkeypatch.delenv("MI355_NO_FUSED")
        compare(case, multi, probs, tag=f"{case.id} multi-workgroup")
        assert multi[1] == fused[1]


# ------------------------------------------------------------------ c. deflated kinds, multi-workgroup loop, slot views
@pytest.mark.parametrize("case", es.group("c"), ids=lambda c: c.id)
def test_deflated_multi_workgroup_on_dense_operators(pkg, probs, gops, monkeypatch, case):
    api = pkg.api
    default = gpu_run(api, gops, probs, case)
    monkeypatch.setenv("MI355_NO_FUSED", "1")
    try:
        multi = gpu_run(api, gops, probs, case)
    finally:
        monkeypatch.delenv("MI355_NO_FUSED")
    compare(case, default, probs, tag=f"{case.id} default")
    compare(case, multi, probs, tag=f"{case.id} multi-workgroup")
    So = probs.ops("toy")[0]
    print(f"  {case.id} multi-workgroup vs default: res_norm / tight bar = {history_margin(multi, default):.3e}")
    assert multi[1] == default[1]
    assert_history(multi[:3], default[:3], apply=So, b=probs.b(case))
    space_report(So, multi[3], default[3], f"{case.id} multi-workgroup vs default")
    assert_space(So, multi[3], default[3])


# ------------------------------------------------------------------ d. long windows (66 coupling rows; nev > 64)
@pytest.mark.parametrize("case", es.group("d"), ids=lambda c: c.id)
def test_long_windows(pkg, probs, gops, case):
    api = pkg.api
    got = gpu_run(api, gops, probs, case)
    compare(case, got, probs)
    A, M = gops(case.prob)
    b, n = probs.b(case), probs.n(case.prob)
    plain = api.pcg(A, b, np.zeros(n), M, case.maxit, case.eps) if es.PRE[case.kind] else api.cg(A, b, np.zeros(n), case.maxit, case.eps)
    print(f"  {case.id} vs plain {'pcg' if es.PRE[case.kind] else 'cg'}: res_norm / tight bar = {history_margin(got, plain):.3e}")
    assert got[1] == plain[1] == case.maxit
    assert_history(got[:3], plain, apply=probs.ops(case.prob)[0], b=b)


# ------------------------------------------------------------------ e. register LU edges of the fused p-update
@pytest.mark.parametrize("case", es.group("e"), ids=lambda c: c.id)
def test_register_lu_edges_eigdefcg(pkg, probs, gops, case):
    compare(case, gpu_run(pkg.api, gops, probs, case), probs)


@pytest.mark.parametrize("nvec", [12, 13, 20, 21])
def test_register_lu_edges_defpcg(pkg, orc, probs, gops, nvec):
    api = pkg.api
    n = 257
    A, M = gops("synth257")
    Ao, Mo = probs.ops("synth257")
    b, W = es.rhs(n, 1), es.random_W(n, nvec)
    want = orc.defpcg(Ao, b, np.zeros(n), W, Mo)
    got = api.defpcg(A, b, np.zeros(n), W, M)
    print(f"  defpcg nvec {nvec}: it {got[1]} (oracle {want[1]}), res_norm / tight bar = {history_margin(got, want):.3e}, "
          f"|x - x_o| / (X_RTOL |x_o|) = {x_margin(got[0], want[0]):.3e}")
    assert_history(got, want, apply=Ao, b=b)


# ------------------------------------------------------------------ f. nonzero x0
@pytest.mark.parametrize("case", es.group("f"), ids=lambda c: c.id)
def test_nonzero_x0(pkg, probs, gops, case):
    compare(case, gpu_run(pkg.api, gops, probs, case), probs)


@pytest.mark.parametrize("maxit,eps", [(10, es.TINY), (0, 1e-7)], ids=["after", "conv"])
def test_nonzero_x0_initcg_initpcg(pkg, orc, probs, gops, maxit, eps):
    api = pkg.api
    n = 257
    A, M = gops("synth257")
    Ao, Mo = probs.ops("synth257")
    b, x0 = es.rhs(n, 1), es.x0(n, 1)
    Wp = probs.W(es.BY_ID["a-eigdefpcg-synth257-3-8-after"])
    Wc = probs.W(es.BY_ID["a-eigdefcg-synth257-3-8-after"])
    for name, got, want in (("initpcg", api.initpcg(A, b, x0, M, Wp, maxit, eps), orc.initpcg(Ao, b, x0, Mo, Wp, maxit, eps)),
                            ("initcg", api.initcg(A, b, x0, Wc, maxit, eps), orc.initcg(Ao, b, x0, Wc, maxit, eps))):
        print(f"  {name}: it {got[1]} (oracle {want[1]}), res_norm / tight bar = {history_margin(got, want):.3e}, "
              f"|x - x_o| / (X_RTOL |x_o|) = {x_margin(got[0], want[0]):.3e}")
        assert maxit == 0 or got[1] == want[1] == maxit
        assert_history(got, want, apply=Ao, b=b)


# ------------------------------------------------------------------ g. replay segmentation gives the same bits
def same_bits(got, ref, tag):
    print(f"  {tag}: it {got[1]} vs {ref[1]}, res_norm equal {np.array_equal(got[2], ref[2])}, x equal "
          f"{np.array_equal(got[0], ref[0])}, V equal {np.array_equal(got[3], ref[3])}")
    assert got[1] == ref[1], tag
    assert np.array_equal(got[2], ref[2]), tag
    assert np.array_equal(got[0], ref[0]), tag
    assert np.array_equal(got[3], ref[3]), tag


def run_quiet(api, ops, probs, case, maxit=None):
    """a priming solve: its BoundsError (eigdefpcg at `start`) is part of the plan"""
    try:
        return gpu_run(api, ops, probs, case, maxit)
    except api.BoundsError:
        return None


@pytest.mark.parametrize("kind", es.KINDS)
def test_segmentation_gives_the_same_bits(pkg, probs, kind):
    """solve() cuts a replay at the iteration count of the previous solve with the same operators and nvec. The solve at
    `after2` (12 / 9 iterations) after a shorter solve, after one that stopped on the first restart (the cut lands on the
    restart), after a converged one (the prediction overshoots) and with eager launches must give the bits of the same
    solve on a fresh context."""
    api = pkg.api
    target = es.BY_ID[f"a-{kind}-synth257-3-8-after2"]
    short = es.BY_ID[f"a-{kind}-synth257-3-8-" + ("start" if es.DEFLATED[kind] else "few")]
    restart = es.BY_ID[f"a-{kind}-synth257-3-8-restart"]
    c1 = api.Context(0)
    o1 = GpuOps(pkg, c1, probs)
    try:
        ref = gpu_run(api, o1, probs, target)
    finally:
        o1.close()
        c1.close()
    compare(target, ref, probs, tag=f"{target.id} fresh context")
    c2 = api.Context(0)
    o2 = GpuOps(pkg, c2, probs)
    try:
        run_quiet(api, o2, probs, short)
        same_bits(gpu_run(api, o2, probs, target), ref, f"{kind} after a solve that stopped at {short.stop}")
        run_quiet(api, o2, probs, restart)
        same_bits(gpu_run(api, o2, probs, target), ref, f"{kind} after a solve that stopped at restart")
        A, M = o2(target.prob)
        conv = es.run(api, kind, A, M, probs.b(target), probs.x0(target), probs.W(target), target.nvec, target.spdim, 0, 1e-7)
        assert conv[1] > target.maxit
        same_bits(gpu_run(api, o2, probs, target), ref, f"{kind} after a converged solve ({conv[1]} iterations)")
        c2.set_chunk(0)
        try:
            same_bits(gpu_run(api, o2, probs, target), ref, f"{kind} eager launches")
        finally:
            c2.set_chunk(DEFAULT_CHUNK)
    finally:
        o2.close()
        c2.close()


# ------------------------------------------------------------------ h. workspace regrowth
def test_workspace_regrowth(pkg, probs):
    """ensure_eig keeps the larger of the old and new sizes while T's leading dimension is the current spdim: small, large,
    small, then a deflated kind on one context, each equal bit for bit to the same call on a fresh context."""
    api = pkg.api
    n = 257
    b, b2 = es.rhs(n, 0), es.rhs(n, 1)
    W = probs.W(es.BY_ID["a-eigdefpcg-synth257-3-8-after2"])

    def calls(ops):
        A, M = ops("synth257")
        return [lambda: api.eigpcg(A, b, np.zeros(n), M, 3, 8, es.stops(3, 8, False)["after2"], es.TINY),
                lambda: api.eigpcg(A, b, np.zeros(n), M, 10, 24, es.stops(10, 24, False)["after"], es.TINY),
                lambda: api.eigpcg(A, b, np.zeros(n), M, 3, 8, es.stops(3, 8, False)["after2"], es.TINY),
                lambda: api.eigdefpcg(A, b2, np.zeros(n), M, W, 8, es.stops(3, 8, True)["after2"], es.TINY)]

    names = ["eigpcg(3, 8)", "eigpcg(10, 24)", "eigpcg(3, 8) again", "eigdefpcg(3 vectors, 8)"]
    fresh = []
    for i in range(4):
        c = api.Context(0)
        o = GpuOps(pkg, c, probs)
        try:
            fresh.append(calls(o)[i]())
        finally:
            o.close()
            c.close()
    c = api.Context(0)
    o = GpuOps(pkg, c, probs)
    try:
        for i, call in enumerate(calls(o)):
            same_bits(call(), fresh[i], f"{names[i]} on the shared context")
    finally:
        o.close()
        c.close()
    # and the fresh results are right: against the oracle
    compare(es.BY_ID["h-eigpcg-synth257-10-24-after"], fresh[1], probs, tag="eigpcg(10, 24) after fresh")
    compare(es.BY_ID["a-eigpcg-synth257-3-8-after2"], fresh[0], probs, tag="eigpcg(3, 8) after2 fresh")
    compare(es.BY_ID["a-eigdefpcg-synth257-3-8-after2"], fresh[3], probs, tag="eigdefpcg after2 fresh")


# ------------------------------------------------------------------ i. nothing to iterate
@pytest.mark.parametrize("which", ["zero_rhs", "exact_x0"])
def test_nothing_to_iterate(pkg, ctx, orc, probs, gops, which):
    """The loop never runs: it = 1, x = x0, V[:, 1] = z / sqrt(rTz) = 0 / 0 as in the reference (NaN), zeros behind it.
    eigdefpcg ends in the BoundsError of its `start` stop on both sides."""
    api = pkg.api
    n = 257
    D, xs, b = es.diagonal_system(n)
    if which == "zero_rhs":
        b, xs = np.zeros(n), np.zeros(n)
    A, M = api.SparseMatrixCSC(ctx, D), api.JacobiPreconditioner(ctx, D.diagonal())
    Ao, Mo = orc.csc_operator(D), orc.jacobi_operator(D.diagonal())
    W = es.random_W(n, 3)
    try:
        for kind in es.KINDS:
            if kind == "eigdefpcg":
                with pytest.raises(orc.BoundsError):
                    es.run(orc, kind, Ao, Mo, b, xs, W, 3, 8, 0, 1e-7)
                with pytest.raises(api.BoundsError):
                    es.run(api, kind, A, M, b, xs, W, 3, 8, 0, 1e-7)
                continue
            with np.errstate(all="ignore"):
                want = es.run(orc, kind, Ao, Mo, b, xs, W, 3, 8, 0, 1e-7)
            got = es.run(api, kind, A, M, b, xs, W, 3, 8, 0, 1e-7)
            dx = np.linalg.norm(got[0] - xs)
            print(f"  {which} {kind}: it {got[1]}, |x - x0| = {dx:.3e}, NaN pattern equal "
                  f"{np.array_equal(np.isfinite(got[3]), np.isfinite(want[3]))}")
            assert got[1] == want[1] == 1
            assert dx <= X_RTOL * np.linalg.norm(xs)
            assert np.allclose(got[2], want[2], rtol=RES_RTOL, atol=0.0)
            assert np.array_equal(np.isfinite(got[3]), np.isfinite(want[3]))
            fin = np.isfinite(want[3])
            assert np.allclose(got[3][fin], want[3][fin], rtol=X_RTOL, atol=0.0)
    finally:
        A.close()
        M.close()
    case = es.BY_ID["a-eigpcg-synth257-3-8-after"]                     # the context solves normally afterwards
    compare(case, gpu_run(api, gops, probs, case), probs, tag=f"{case.id} after the empty solves")
