"""GPU suite (-m gpu): a call that sees NaN / Inf, breaks down inside the loop or returns an error leaves no trace in the
device scratch of its handles. Every operator, the Krylov workspace of a context, the interior CG, the eigCG window and the
full-system preconditioners keep buffers between calls (contribution rows, slot tables, partial sums, p, V, T, u / z pairs,
f_I / y_I / part, the `done` flags, ws.predicted); the reference carries nothing from one solve to the next, so every one of
them has to be rewritten, or never multiplied by a stale value, at the start of the next call. Cases, poisons and the
expected outcomes: tests/poison_synth.py; tests/test_poison_cpu.py pins the outcomes on the oracle and proves that the clean
solves are short, decided and insensitive to the summation order, so a bit that differs here is state.

Every test, on ONE set of handles in a context of this file's own (`pctx`: nothing of the session's context changes):
  1. a clean call, against the oracle at the existing bar (test_gpu_krylov_edges.strict, test_gpu_eig_edges.compare,
     test_gpu_parity.assert_history, the apply bars of the preconditioner suites);
  2. the poisoned call (maxit <= 20): it returns; `it` equal to the oracle's, res_norm equal with inf / nan in the same
     positions and the finite entries at the usual bar; SingularException / BoundsError where the oracle raises them;
     x of a poisoned call is not compared;
  3. the clean call again: bit-identical to 1 in x, it, res_norm (and V);
  4. 1-3 with set_chunk(4) and set_chunk(0): the two agree bit for bit;
and step 3 once more on fresh handles in a fresh context, for one call per loop form and per preconditioner.

The Krylov workspace of a context is keyed by n, so the clean solves around a breakdown run at the breakdown's n
(krylov_synth.banded(1026 / 4098), sparse_synth.tridiag(9002), eig_synth.matrix(1026)); the dense pair swaps its blocks on
the same two operators (set_blocks). Not run: the deflated eigCG kinds on the breakdown matrix (the oracle outcomes pinned
for it are those of cg, identity pcg, eigcg and eigpcg), and pcg with the Neumann-Neumann induced preconditioner as written
on `micro` (CG does not converge with it, test_gpu_nn_induced.SOLVES: its applies are checked, its solves with the assembled
coupling).

Found and fixed:
  * csrc/kernels.hpp: k_icg_start / k_icg_direction, the three-launch interior CG, decided `done` with `res <= tol`; the
    two-launch form and the reference stop on `!(res > tol)`. With NaN in the right-hand side of one subdomain the
    three-launch form iterated on it up to n_i times and returned NaN where the reference returns x = 0 after 0 iterations
    (test_interior_cg_nan_stays_in_its_subdomain, both sets).
  * csrc/solvers.hpp: host_lu called a NaN or Inf pivot of WtAW (WtW) singular, so a NaN in W was MI_ERR_SINGULAR where the
    reference's `WtAW \\ mu` (getrf: info = 0) returns NaN and the solve ends at it = 1 with res_norm = [nan]; eigdefpcg:
    the BoundsError of its extraction. Shown by the W_nan step of the four deflated tests and of the four eigCG-family tests that take a W.
No stale buffer was found: every bitwise comparison held on the first run.

Measured on an MI355X (41 tests, 9 s for the file, no test above 0.2 s): 769 bitwise comparisons, all equal; 584 poisoned
calls, `it` and res_norm equal to the oracle's in all of them (every table outcome it = 1 with [nan] / [inf]; every breakdown
it = 3 with [sqrt(n), inf, nan]), 33 of them the oracle's exception; 68 clean calls against the oracle, res_norm <= 5.6e-4 of
the bar (d2048w1, pcg, folded), x <= 1.1e-8 of its bar. interior_iterations() at chunk 1: `mixed` 94 clean, 12 with the
slowest subdomain poisoned or zeroed, `capped` 8 and 0, the same in both forms.
Sensitivity, each defect seeded once into a scratch build and this file run against it:
  * k_gemv_pcg's operand without the `first1` case (r_0 - 0 * Ap with the contribution rows of the last solve): the dense
    breakdown test fails (pair1026 after brkd1026: x, it, res_norm all differ). The NaN / Inf poisons in b and x0 end at
    it = 1 before a folded launch has run, so only a breakdown leaves non-finite contribution rows;
  * the per-solve clear of V in eig_solvers.hpp removed: the eigcg and eigpcg tests fail (the it = 1 call returns the
    columns of the earlier window where fresh handles return zeros);
  * the interior-CG stop rule `res <= tol`: both interior tests fail;
  * LORASC's partial dots accumulated into `part` instead of stored: lorasc-micro and lorasc-ragged fail at the first
    apply after a NaN.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import block_jacobi_ref as bjr
import eig_synth as es
import krylov_synth as ks
import lorasc_ref as lr
import nn_induced_ref as nr
import poison_synth as ps
import sparse_synth as ss
import test_gpu_block_jacobi as tbj
import test_gpu_lorasc as tlo
import test_gpu_nn_induced as tni
from conftest import one
from test_gpu_dense_edges import concat, split
from test_gpu_eig_edges import compare as eig_compare
from test_gpu_krylov_edges import strict, with_env
from test_gpu_parity import RES_FLOOR, RES_RTOL, assert_history
from test_gpu_sparse_edges import make_op as make_interior_op
from test_gpu_spd_direct import _gg_problem

pytestmark = pytest.mark.gpu

CHUNKS = (4, 0)            # replayed graphs, eager launches


# ------------------------------------------------------------------ fixtures and helpers
@pytest.fixture(scope="module")
def pctx(pkg):
    c = pkg.api.Context(0)
    yield c
    c.close()


def device_pinv(api, ctx):
    return lambda d, S: split(api.nn_pinv(ctx, np.array(d.sizes, dtype=np.int64), concat(S)), d.sizes)


@pytest.fixture(scope="module")
def probs(pkg, pctx, orc):
    return ps.Problems(orc, device_pinv(pkg.api, pctx))


@pytest.fixture(scope="module")
def tally():
    t = {"bits": 0, "poisoned": 0, "errors": 0, "worst": {"res": (0.0, ""), "x": (0.0, ""), "n": 0}}
    yield t
    w = t["worst"]
    print(f"\n  poison suite: {t['bits']} bitwise comparisons, all equal; {t['poisoned']} poisoned calls with `it` and res_norm equal to "
          f"the oracle's, {t['errors']} of them the oracle's exception; {w['n']} clean calls against the oracle: res_norm <= "
          f"{w['res'][0]:.3e} of the bar ({w['res'][1]}), x <= {w['x'][0]:.3e} ({w['x'][1]})")


def make_ops(api, ctx, probs, prob, storage="f64"):
    if probs.is_dense(prob):
        S, Pi, g, cnt, n = probs.dense(prob)
        return {"A": api.LocalSchurs(ctx, S, g, cnt), "nn": api.NeumannNeumannSchurPreconditioner(ctx, Pi, g, cnt, storage=storage)}
    A = probs.matrix(prob)
    return {"A": api.SparseMatrixCSC(ctx, A), "jacobi": api.JacobiPreconditioner(ctx, A.diagonal()),
            "identity": api.IdentityPreconditioner(ctx, A.shape[0])}


def close_ops(ops):
    for op in ops.values():
        op.close()


def dev_call(api, ops, probs, c, poison=None):
    pre = probs.precond(c)
    b, x0, W = probs.b(c.prob, c.kind), probs.x0(c), probs.W(c)
    maxit = c.maxit
    if poison:
        b, x0, W = ps.poisoned(poison, b, x0, W)
        maxit = ps.poison_maxit(c)
    assert not poison or 0 < maxit <= 50
    return ps.run_call(api, c, ops["A"], ops[pre] if pre else None, b, x0, W, maxit)


def bits(got, ref, tag, tally):
    """bit for bit: x, it, res_norm and, for the eigCG family, V"""
    same = [np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got, ref)]
    print(f"  {tag}: it {got[1]} vs {ref[1]}; (x, it, res_norm[, V]) equal: {same}")
    tally["bits"] += 1
    assert len(got) == len(ref) and all(same), f"{tag}: {same}"


def same_outcome(got, want, tag, tally):
    """the outcome of a poisoned (or breaking-down) call against the oracle's"""
    desc = lambda o: o[0] if o[1] is None else (o[1][1], o[1][2])                       # noqa: E731
    print(f"  {tag}: device {desc(got)}, oracle {desc(want)}")
    tally["poisoned"] += 1
    assert got[0] == want[0], f"{tag}: device {desc(got)}, oracle {desc(want)}"
    if got[0] != "ok":
        tally["errors"] += 1
        return
    (_, it, res), (_, ito, reso) = got[1][:3], want[1][:3]
    assert it == ito and res.shape == reso.shape, f"{tag}: it {it} vs {ito}"
    assert np.array_equal(np.isnan(res), np.isnan(reso)) and np.array_equal(np.isposinf(res), np.isposinf(reso)) and \
        not np.isneginf(res).any(), f"{tag}: {res} vs {reso}"
    fin = np.isfinite(reso)
    if fin.any():
        assert np.all(np.abs(res[fin] - reso[fin]) <= RES_RTOL * reso[fin] + RES_FLOOR * reso[0]), f"{tag}: {res} vs {reso}"


def cycle(api, ctx, orc, probs, ops, c, poisons, tally, monkeypatch, form=ps.DEFAULT, bar=None, breakdown=None):
    """Steps 1-4 for one clean call: every poison (and the breakdown call, on its own operators `breakdown = (ops, call)`)
    between two clean calls, replayed and eager. Returns the clean result."""
    bar = bar or (lambda tag, got: strict(tag, got, probs.solve(c)[1], probs, c, tally["worst"]))
    run = lambda fn: with_env(monkeypatch, list(form.env), fn)                          # noqa: E731
    by_chunk = {}
    try:
        for chunk in CHUNKS:
            ctx.set_chunk(chunk)
            tag = f"{c.id} {form.name} chunk {chunk}"
            good = run(lambda: dev_call(api, ops, probs, c))
            if chunk == CHUNKS[0]:
                bar(tag, good)
            for p in poisons:
                got = ps.outcome(api, lambda: run(lambda: dev_call(api, ops, probs, c, p)))
                same_outcome(got, probs.solve(c, p), f"{tag} {p}", tally)
                bits(run(lambda: dev_call(api, ops, probs, c)), good, f"{tag} after {p}", tally)
            if breakdown:
                bops, bc = breakdown
                got = ps.outcome(api, lambda: run(lambda: dev_call(api, bops, probs, bc)))
                same_outcome(got, probs.solve(bc), f"{tag} {bc.id}", tally)
                bits(run(lambda: dev_call(api, ops, probs, c)), good, f"{tag} after {bc.id}", tally)
            by_chunk[chunk] = good
    finally:
        ctx.set_chunk(CHUNKS[0])
    bits(by_chunk[CHUNKS[1]], by_chunk[CHUNKS[0]], f"{c.id} {form.name} eager vs replayed", tally)
    return by_chunk[CHUNKS[0]]


def fresh_bits(api, probs, c, good, tally, monkeypatch, form=ps.DEFAULT, storage="f64", build=None):
    """the clean call on fresh handles in a fresh context against the one that followed the poisons"""
    ctx2 = api.Context(0)
    try:
        ctx2.set_chunk(CHUNKS[0])
        ops2 = build(ctx2) if build else make_ops(api, ctx2, probs, c.prob, storage)
        try:
            got = with_env(monkeypatch, list(form.env), lambda: dev_call(api, ops2, probs, c))
        finally:
            close_ops(ops2)
    finally:
        ctx2.close()
    bits(got, good, f"{c.id} {form.name} fresh handles vs the poisoned ones", tally)


# ------------------------------------------------------------------ 1. sparse operators: EPT 2 / 8, the two-launch loop
@pytest.mark.parametrize("prob,forms,calls", ps.SPARSE_GROUP, ids=[g[0] for g in ps.SPARSE_GROUP])
def test_sparse_loops_after_a_poisoned_solve(pkg, pctx, orc, probs, tally, monkeypatch, prob, forms, calls):
    """cg (k_fused_cg<EPT>), Jacobi and identity pcg (k_fused_residual / start / xr / p<EPT>; k_spmv_pcg / k_csrfold_start
    past FUSED_MAX_N) from zero (k_entry_zero<EPT>) and from a random x0 (the general entry), with NaN / Inf in b, b * 1e160
    and NaN in x0 between the clean solves; the default form and its environment switch."""
    api = pkg.api
    ops = make_ops(api, pctx, probs, prob)
    try:
        for form in forms:
            for k, c in enumerate(calls):
                good = cycle(api, pctx, orc, probs, ops, c, ps.POISONS_VEC, tally, monkeypatch, form)
                if k == 1:
                    fresh_bits(api, probs, c, good, tally, monkeypatch, form)
    finally:
        close_ops(ops)


# ------------------------------------------------------------------ 2. breakdown inside the loop
@pytest.mark.parametrize("clean,brk,forms", ps.breakdown_pairs(), ids=[b.id for _, b, _ in ps.breakdown_pairs()])
def test_breakdown_inside_the_loop_leaves_no_trace(pkg, pctx, orc, probs, tally, monkeypatch, clean, brk, forms):
    """A = diag(+1 ... -1 ...), b = 1: p'Ap == 0 exactly, alpha = Inf in the first iteration, res_norm = [sqrt(n), inf, nan],
    it = 3: p, Ap, the contribution rows and the partials hold Inf / NaN from real iterations. The clean solve before and
    after runs at the same n (the same Krylov workspace); the dense pair swaps blocks on the same two operators."""
    api = pkg.api
    assert brk.maxit <= 50
    if probs.is_dense(brk.prob):
        ops = make_ops(api, pctx, probs, clean.prob)
        S, Pi = probs.dense(clean.prob)[:2]
        Sb, Pib = probs.dense(brk.prob)[:2]

        def run_brk(form):                         # the same two handles hold the breakdown blocks while the breakdown call runs
            ops["A"].set_blocks(concat(Sb))
            ops["nn"].set_blocks(concat(Pib))
            try:
                return ps.outcome(api, lambda: with_env(monkeypatch, list(form.env), lambda: dev_call(api, ops, probs, brk)))
            finally:
                ops["A"].set_blocks(concat(S))
                ops["nn"].set_blocks(concat(Pi))
        try:
            for form in forms:
                by_chunk = {}
                for chunk in CHUNKS:
                    pctx.set_chunk(chunk)
                    tag = f"{clean.id} {form.name} chunk {chunk}"
                    good = with_env(monkeypatch, list(form.env), lambda: dev_call(api, ops, probs, clean))
                    if chunk == CHUNKS[0]:
                        strict(tag, good, probs.solve(clean)[1], probs, clean, tally["worst"])
                    same_outcome(run_brk(form), probs.solve(brk), f"{tag} {brk.id}", tally)
                    bits(with_env(monkeypatch, list(form.env), lambda: dev_call(api, ops, probs, clean)), good, f"{tag} after {brk.id}", tally)
                    by_chunk[chunk] = good
                bits(by_chunk[CHUNKS[1]], by_chunk[CHUNKS[0]], f"{clean.id} {form.name} eager vs replayed", tally)
            fresh_bits(api, probs, clean, by_chunk[CHUNKS[0]], tally, monkeypatch, forms[-1])
        finally:
            pctx.set_chunk(CHUNKS[0])
            close_ops(ops)
        return
    ops, bops = make_ops(api, pctx, probs, clean.prob), make_ops(api, pctx, probs, brk.prob)
    try:
        for form in forms:
            good = cycle(api, pctx, orc, probs, ops, clean, (), tally, monkeypatch, form, breakdown=(bops, brk))
        fresh_bits(api, probs, clean, good, tally, monkeypatch, forms[-1])
    finally:
        close_ops(ops)
        close_ops(bops)


# ------------------------------------------------------------------ 3. dense operators: folded, unfolded, generic, big fold, fp32 Π
@pytest.mark.parametrize("prob,forms,calls", ps.DENSE_GROUP, ids=[g[0] for g in ps.DENSE_GROUP])
def test_dense_loops_after_a_poisoned_solve(pkg, pctx, orc, probs, tally, monkeypatch, prob, forms, calls):
    """folded pcg at EPT 2 / 8 (k_gemv_pcg: `first1`), MI355_NO_FOLD=1, view_load's generic loop (d2048w1), k_residual +
    k_fold_start (big8200) against MI355_NO_BIG_FOLD=1"""
    api = pkg.api
    ops = make_ops(api, pctx, probs, prob)
    try:
        for form in forms:
            for k, c in enumerate(calls):
                good = cycle(api, pctx, orc, probs, ops, c, ps.POISONS_VEC, tally, monkeypatch, form)
                if k == 0:
                    fresh_bits(api, probs, c, good, tally, monkeypatch, form)
    finally:
        close_ops(ops)
        probs.drop(prob)


def test_fp32_stored_preconditioner_after_a_poisoned_solve(pkg, pctx, orc, tally, monkeypatch):
    """storage="f32": the oracle runs on the fp32-rounded Π blocks"""
    api = pkg.api
    pinv = device_pinv(api, pctx)
    p32 = ps.Problems(orc, lambda d, S: [np.asfortranarray(B.astype(np.float32).astype(np.float64)) for B in pinv(d, S)])
    ops = make_ops(api, pctx, p32, ps.F32_PROB, storage="f32")
    assert ops["nn"].storage == "f32"
    try:
        for c in (ps.Call(ps.F32_PROB, "pcg"), ps.Call(ps.F32_PROB, "pcg", x0="rand")):
            good = cycle(api, pctx, orc, p32, ops, c, ps.POISONS_VEC, tally, monkeypatch)
        fresh_bits(api, p32, c, good, tally, monkeypatch, storage="f32")
    finally:
        close_ops(ops)


# ------------------------------------------------------------------ 4. deflated solves
@pytest.fixture(scope="module")
def defl_ops(pkg, pctx, probs):
    ops = make_ops(pkg.api, pctx, probs, ps.DEFL_PROB)
    yield ops
    close_ops(ops)


@pytest.mark.parametrize("c,forms", ps.DEFL_GROUP, ids=[c.id for c, _ in ps.DEFL_GROUP])
def test_deflated_solves_after_a_poisoned_or_failed_solve(pkg, pctx, orc, probs, defl_ops, tally, monkeypatch, c, forms):
    """defpcg folded (k_defl_mu / k_fused_p; 21 columns: past the preloaded 20), MI355_NO_FOLD_DEFL=1 and defcg, with the
    poisons in b, x0 and W; W = 0 is MI_ERR_SINGULAR (SingularException), after which the same handles solve bit for bit"""
    api = pkg.api
    for form in forms:
        good = cycle(api, pctx, orc, probs, defl_ops, c, ps.poisons_of(c.kind), tally, monkeypatch, form)
    fresh_bits(api, probs, c, good, tally, monkeypatch, forms[-1])


# ------------------------------------------------------------------ 5. the eigCG family
@pytest.fixture(scope="module")
def eprobs(orc):
    return es.Problems(orc)


def eig_case(c):
    """the Call as eig_synth's Case (the same inputs: probs.W is eig_synth's chain)"""
    return es.Case("p", c.kind, c.prob, c.nvec, c.spdim, "after")


def eig_bar(orc, probs, eprobs, c):
    def bar(tag, got):
        if c.kind.startswith("eig"):
            case = eig_case(c)
            assert case.maxit == c.maxit and case.eps == c.eps
            assert np.array_equal(eprobs.b(case), probs.b(c.prob, c.kind))
            if probs.W(c) is not None:
                assert np.array_equal(eprobs.W(case), probs.W(c))
            eig_compare(case, got, eprobs, tag=tag)
        else:
            assert_history(got, probs.solve(c)[1], apply=probs.op(c.prob, "A"), b=probs.b(c.prob, c.kind))
    return bar


@pytest.mark.parametrize("c", ps.EIG_GROUP, ids=[c.id for c in ps.EIG_GROUP])
def test_eig_family_after_poisoned_and_failed_solves(pkg, pctx, orc, probs, eprobs, tally, monkeypatch, c):
    """good -> poisoned -> good -> poisoned (another kind) -> good ... on one window (nvec 3, spdim 8, n = 1025): x, it,
    res_norm and V bit for bit. eigdefpcg ends every poisoned call in the BoundsError of its final extraction, W = 0 is the
    SingularException; ws.predicted after an it = 1 solve cuts the next solve's replay segments, which must still equal the
    eager solve."""
    api = pkg.api
    ops = make_ops(api, pctx, probs, c.prob)
    try:
        good = cycle(api, pctx, orc, probs, ops, c, ps.poisons_of(c.kind), tally, monkeypatch, bar=eig_bar(orc, probs, eprobs, c))
        fresh_bits(api, probs, c, good, tally, monkeypatch)
        if c.kind in ("eigcg", "eigpcg"):
            # a stop at it = 1 after full windows and a poisoned call: the columns behind the only Lanczos vector are zeros,
            # as on fresh handles, not what those calls left in the window
            start = ps.eig_start_call(c.kind)
            same_outcome(ps.outcome(api, lambda: dev_call(api, ops, probs, c, "b_nan")), probs.solve(c, "b_nan"), f"{c.id} b_nan", tally)
            got = dev_call(api, ops, probs, start)
            eig_compare(es.Case("p", c.kind, c.prob, c.nvec, c.spdim, "start"), got, eprobs, tag=start.id)
            assert got[1] == 1 and not np.any(got[3][:, 1:])
            fresh_bits(api, probs, start, got, tally, monkeypatch)
    finally:
        close_ops(ops)


@pytest.mark.parametrize("clean,brk", ps.eig_breakdown_pairs(), ids=[b.id for _, b in ps.eig_breakdown_pairs()])
def test_eig_window_after_a_breakdown(pkg, pctx, orc, probs, eprobs, tally, monkeypatch, clean, brk):
    """eigcg ends the breakdown at it = 3 with [sqrt(n), inf, nan] and NaN columns in V; eigpcg (identity) in the BoundsError
    of its extraction; spdim = 8 > 3, so no restart is reached. Clean calls on eig_synth.matrix(1026): the same workspace."""
    api = pkg.api
    ops, bops = make_ops(api, pctx, probs, clean.prob), make_ops(api, pctx, probs, brk.prob)
    try:
        cycle(api, pctx, orc, probs, ops, clean, (), tally, monkeypatch, bar=eig_bar(orc, probs, eprobs, clean), breakdown=(bops, brk))
    finally:
        close_ops(ops)
        close_ops(bops)


# ------------------------------------------------------------------ 6. interior CG and the matrix-free operators
@pytest.fixture(scope="module")
def isets(orc):
    out = {}
    for name, (s, dom) in ps.interior_sets().items():
        ustar = [spla.splu(sp.csc_matrix(A)).solve(b) if A.shape[0] else np.zeros(0) for A, b in zip(s.A_II, s.b_I)]
        its = [orc.interior_cg(A, b, s.reltol)[1] if A.shape[0] else 0 for A, b in zip(s.A_II, s.b_I)]
        out[name] = (s, dom, ustar, its)
    return out


@pytest.mark.parametrize("name", ["mixed", "capped"])
def test_interior_cg_nan_stays_in_its_subdomain(pkg, pctx, orc, isets, tally, monkeypatch, name):
    """interior_solutions(u_Γ = 0, b_I) with NaN in the rows of ONE subdomain, both device forms, plain and diagonal Pl,
    MI355_ICG_CHUNK 1 and 7: the other subdomains bit-identical to the clean call; the poisoned one as the oracle's
    interior_cg leaves it (0 iterations, x = 0); interior_iterations() equal between the forms; the clean call again bit for
    bit. Bars of the clean call: tests/test_gpu_sparse_edges.py (2 κ_d reltol against SuperLU; the count to +-1)."""
    s, dom, ustar, its_o = isets[name]
    assert max(s.n_i) <= ps.ICG_MAX_ROWS
    off = np.concatenate([[0], np.cumsum(s.n_i)]).astype(int)
    u0 = np.zeros(s.n_Γ)
    b_clean, b_bad, b_zero = ps.interior_rhs(s), ps.interior_rhs(s, dom), ps.interior_rhs(s, dom, zero=True)
    others = np.ones(off[-1], dtype=bool)
    others[off[dom]:off[dom + 1]] = False
    want_bad = orc.interior_cg(s.A_II[dom], b_bad[off[dom]:off[dom + 1]], s.reltol)
    assert want_bad[1] == 0 and not np.any(want_bad[0])
    counts = {}
    for fused in (0, 1):
        for precond in (None, "diagonal"):
            for chunk in (1, 7):
                key = (fused, precond, chunk)
                S = make_interior_op(pkg, pctx, monkeypatch, s, fused, chunk, precond)
                try:
                    def solve(b):
                        before = S.interior_iterations()
                        u = S.interior_solutions(u0, b)
                        return u, S.interior_iterations() - before
                    u_clean, inc_clean = solve(b_clean)
                    for d in range(len(s.n_i)):
                        if s.b_I[d].any():
                            err = np.linalg.norm(u_clean[off[d]:off[d + 1]] - ustar[d]) / np.linalg.norm(ustar[d])
                            assert err <= 2.0 * s.kappa[d] * s.reltol, (key, d, err)
                    u_zero, inc_zero = solve(b_zero)
                    u_bad, inc_bad = solve(b_bad)
                    u_again, inc_again = solve(b_clean)
                    print(f"  {name} fused={fused} precond={precond} chunk={chunk}: interior_iterations clean {inc_clean}, subdomain {dom} "
                          f"zeroed {inc_zero}, poisoned {inc_bad} (oracle: 0 for it, {its_o} clean), again {inc_again}; NaN in the "
                          f"poisoned solution: {int(np.isnan(u_bad).sum())}")
                    tally["poisoned"] += 1
                    assert np.array_equal(u_bad[others], u_clean[others]), key            # the NaN does not cross a subdomain boundary
                    tally["bits"] += 1
                    assert np.array_equal(u_bad[~others], want_bad[0]), key               # x = 0 after 0 iterations
                    assert inc_bad == inc_zero, key                                       # ... and 0 iterations: a zero right-hand side's count
                    if chunk == 1 and precond is None:
                        rest = max([i for d, i in enumerate(its_o) if d != dom], default=0)
                        assert abs(inc_bad - rest) <= (1 if rest else 0), (key, inc_bad, its_o)
                        assert abs(inc_clean - max(its_o)) <= 1, (key, inc_clean, its_o)
                    assert np.array_equal(u_again, u_clean) and inc_again == inc_clean, key
                    tally["bits"] += 1
                    counts[key] = (inc_clean, inc_bad)
                finally:
                    S.close()
    for (fused, precond, chunk), v in counts.items():
        assert v == counts[(0, precond, chunk)], (fused, precond, chunk, v)               # both device forms: the same counts


@pytest.mark.parametrize("fused", [0, 1])
def test_matrix_free_operators_after_nan(pkg, pctx, isets, tally, monkeypatch, fused):
    """MatrixFreeLocalSchurs * v, schur_rhs and GlobalSchur * v with NaN in v / b_I, then the clean input again: bit for bit"""
    api = pkg.api
    s, dom, _, _ = isets["mixed"]
    rng = np.random.default_rng(31)
    v = rng.standard_normal(s.n_Γ)
    v_bad = v.copy()
    v_bad[s.gather_idx[dom][0]] = np.nan                                              # the node A_IΓ of the subdomain reads
    b_Γ = rng.standard_normal(s.n_Γ)
    S = make_interior_op(pkg, pctx, monkeypatch, s, fused, 7, None)
    try:
        y0 = S * v
        assert np.all(np.isfinite(y0))
        assert np.isnan(S * v_bad).any()
        assert np.array_equal(S * v, y0)
        r0 = S.schur_rhs(ps.interior_rhs(s), b_Γ)
        assert np.all(np.isfinite(r0))
        S.schur_rhs(ps.interior_rhs(s, dom), b_Γ)
        assert np.array_equal(S.schur_rhs(ps.interior_rhs(s), b_Γ), r0)
        assert np.array_equal(S * v, y0)
        tally["bits"] += 3
    finally:
        S.close()
    live = [d for d, n in enumerate(s.n_i) if n]
    A_IΓ = []
    for d in live:
        G = sp.lil_matrix((s.n_i[d], s.n_Γ))
        loc = sp.coo_matrix(s.A_IΓ[d])
        for i, j, a in zip(loc.row, loc.col, loc.data):
            G[i, s.gather_idx[d][j]] = a
        A_IΓ.append(sp.csc_matrix(G))
    monkeypatch.setenv("MI355_ICG_FUSED", str(fused))
    try:
        G = api.GlobalSchur(pctx, [s.A_II[d] for d in live], A_IΓ, sp.csc_matrix(ss.GAMMA_C * sp.identity(s.n_Γ)), None, reltol=s.reltol)
    finally:
        monkeypatch.delenv("MI355_ICG_FUSED")
    try:
        y0 = G * v
        assert np.all(np.isfinite(y0))
        assert np.isnan(G * v_bad).any()
        assert np.array_equal(G * v, y0)
        tally["bits"] += 1
    finally:
        G.close()


# ------------------------------------------------------------------ 7. full-system and Γ preconditioners
PRECONDS = ["spd_direct", "lorasc-micro", "lorasc-ragged", "nni-f64-reference", "nni-f64-assembled", "nni-f32-reference",
            "nni-f32-assembled", "bj-1", "bj-4"]
FRESH = {"spd_direct", "lorasc-micro", "nni-f64-assembled", "nni-f32-assembled", "bj-4"}


@pytest.fixture(scope="module")
def fcases(fem):
    return lr.gpu_cases(fem, which=("micro", "ragged"))


def precond_spec(name, pkg, orc, fem, fcases, micro):
    """name -> dict(n, b, A(ctx), Ao, M(ctx), Mo(), ref(r), bar, pcg: run a solve too)"""
    api = pkg.api
    dense_M = lambda Minv, n: orc.neumann_neumann_operator([np.asfortranarray(Minv)], [np.arange(n)], np.ones(n, dtype=np.int64))   # noqa: E731
    if name == "spd_direct":
        P = micro
        A_gg = sp.csc_matrix(_gg_problem(fem, P, one))
        n = P.sub.n_Γ
        lu = spla.splu(A_gg)
        return dict(n=n, b=P.b_schur, A=lambda ctx: api.LocalSchurs(ctx, P.Sd, P.sub.gather_idx, P.sub.node_Γ_cnt),
                    Ao=orc.apply_local_schurs_operator(P.Sd, P.sub.gather_idx, n), M=lambda ctx: api.SparseDirectPreconditioner(ctx, A_gg),
                    Mo=lambda: dense_M(np.linalg.inv(A_gg.toarray()), n), ref=lu.solve, bar=1e-12, pcg=True)
    if name.startswith("lorasc"):
        c = fcases[name.split("-")[1]]
        if c.name == "micro":
            E, coef = fem.prepare_lorasc_precond(lr.dense_schur(c), c.A_ΓΓ, nvec=25, ε=0.2)[0], None
            pE, pc = E, None
        else:
            # the applies with nev = 25 random columns and a coef (lorasc_ref.apply_inputs); the solves with the eigenvectors and
            # coef = Σ of test_gpu_lorasc.test_pcg_with_lorasc_against_oracle (random columns make no preconditioner: the
            # oracle's own history is then sensitive to the summation order from iteration ~8 on)
            _, E, coef = lr.apply_inputs(c, 25, True)
            assert E.shape[1] == 25 and coef is not None
            pE, pc = fem.prepare_lorasc_precond(lr.dense_schur(c), c.A_ΓΓ, nvec=25, ε=0.2)
        return dict(n=c.n, b=c.b, A=lambda ctx: api.SparseMatrixCSC(ctx, c.A), Ao=orc.csc_operator(c.A),
                    M=lambda ctx: tlo._device(pkg, ctx, c, E, coef), Mo=lambda: dense_M(lr.dense_minv(c, pE, pc), c.n),
                    ref=lambda r: lr.apply_lorasc(c, r, E, coef, refine=2), bar=tlo.APPLY_BAR, pcg=True, E=E, coef=coef,
                    pcg_correction=(pE, pc))
    c = fcases["micro"]
    if name.startswith("nni"):
        _, storage, cpl = name.split("-")
        blocks = tni._blocks_for(fem, c, storage)
        return dict(n=c.n, b=c.b, A=lambda ctx: api.SparseMatrixCSC(ctx, c.A), Ao=orc.csc_operator(c.A),
                    M=lambda ctx: tni._device(pkg, ctx, fem, c, storage, cpl), Mo=lambda: dense_M(nr.dense_minv(c, blocks, cpl), c.n),
                    ref=lambda r: nr.apply_neumann_neumann_induced(c, blocks, r, cpl, refine=2), bar=tni.APPLY_BAR,
                    pcg=cpl == "assembled")    # as written, CG does not converge on micro (test_gpu_nn_induced.SOLVES): applies only
    nb = int(name.split("-")[1])
    A = sp.csc_matrix(c.A)
    ref = bjr.Ref(A, nb, 2)
    return dict(n=c.n, b=c.b, A=lambda ctx: api.SparseMatrixCSC(ctx, A), Ao=orc.csc_operator(A),
                M=lambda ctx: api.BlockJacobiPreconditioner(ctx, nb, A), Mo=lambda: dense_M(ref.dense_minv(), c.n), ref=ref,
                bar=tbj.APPLY_BAR, pcg=True)


@pytest.mark.parametrize("name", PRECONDS)
def test_preconditioners_after_non_finite_input(pkg, pctx, orc, fem, fcases, micro, tally, name):
    """ldiv on a clean vector, on one with a NaN, on one with an Inf, on the clean one again: bit for bit (f_I / y_I / part and
    the level buffers are rewritten by every apply); pcg(A, b_nan, 0, M) between two clean solves, replayed and eager; LORASC:
    set_correction with a NaN in E, then the clean E again."""
    api = pkg.api
    sp_ = precond_spec(name, pkg, orc, fem, fcases, micro)
    n = sp_["n"]
    r = np.random.default_rng(41).standard_normal(n)
    A, M = sp_["A"](pctx), sp_["M"](pctx)
    try:
        z0 = M.ldiv(r)
        want = sp_["ref"](r)
        err = np.linalg.norm(z0 - want) / np.linalg.norm(want)
        print(f"  {name}: ldiv rel. error {err:.3e} (bar {sp_['bar']:.0e})")
        assert err <= sp_["bar"]
        for val, at in ((np.nan, n // 2), (np.inf, 3), (np.nan, n - 1), (-np.inf, 0)):
            rb = r.copy()
            rb[at] = val
            assert not np.all(np.isfinite(M.ldiv(rb)))
            assert np.array_equal(M.ldiv(r), z0), (name, val, at)
            tally["bits"] += 1
        if "E" in sp_:
            Eb = np.array(sp_["E"], copy=True)
            Eb[Eb.shape[0] // 2, Eb.shape[1] // 2] = np.nan
            M.set_correction(Eb, sp_["coef"])
            assert not np.all(np.isfinite(M.ldiv(r)))
            M.set_correction(sp_["E"], sp_["coef"])
            assert np.array_equal(M.ldiv(r), z0), name
            tally["bits"] += 1
        if not sp_["pcg"]:
            return
        if "pcg_correction" in sp_:
            M.set_correction(*sp_["pcg_correction"])
        x0, b = np.zeros(n), sp_["b"]
        b_bad = ps.poisoned("b_nan", b, x0, None)[0]
        Mo = sp_["Mo"]()
        want, want_bad = orc.pcg(sp_["Ao"], b, x0, Mo), ps.outcome(orc, lambda: orc.pcg(sp_["Ao"], b_bad, x0, Mo, ps.POISON_MAXIT))
        by_chunk = {}
        try:
            for chunk in CHUNKS:
                pctx.set_chunk(chunk)
                good = api.pcg(A, b, x0, M)
                if chunk == CHUNKS[0]:
                    tlo._assert_solve(good, want, sp_["Ao"], b)
                same_outcome(ps.outcome(api, lambda: api.pcg(A, b_bad, x0, M, ps.POISON_MAXIT)), want_bad, f"{name} chunk {chunk} b_nan", tally)
                bits(api.pcg(A, b, x0, M), good, f"{name} chunk {chunk} after b_nan", tally)
                by_chunk[chunk] = good
        finally:
            pctx.set_chunk(CHUNKS[0])
        bits(by_chunk[CHUNKS[1]], by_chunk[CHUNKS[0]], f"{name} eager vs replayed", tally)
        if name in FRESH:
            ctx2 = api.Context(0)
            try:
                ctx2.set_chunk(CHUNKS[0])
                A2, M2 = sp_["A"](ctx2), sp_["M"](ctx2)
                assert np.array_equal(M2.ldiv(r), z0)
                if "pcg_correction" in sp_:
                    M2.set_correction(*sp_["pcg_correction"])
                bits(api.pcg(A2, b, x0, M2), by_chunk[CHUNKS[0]], f"{name} fresh handles vs the poisoned ones", tally)
                M2.close(); A2.close()
            finally:
                ctx2.close()
    finally:
        M.close()
        A.close()


# ------------------------------------------------------------------ 8. set-up recovery
def test_setup_recovers_from_a_failed_run(pkg, pctx, fcases, tally):
    """SchurSetup.run with one NaN in the A_II values is MI_ERR_SINGULAR; the next run with the good values equals a fresh
    plan's output bit for bit, and a LORASC operator bound to the plan applies as before the failed run"""
    api = pkg.api
    c = fcases["micro"]
    P = c.P
    M = tlo._device(pkg, pctx, c)
    setup = M.setup
    x = np.random.default_rng(43).standard_normal(c.n)
    z0 = M.ldiv(x)
    Sd0, _ = setup.run()
    ii = tlo._csc_data(P.A_IIdd)
    bad = ii.copy()
    bad[bad.size // 2] = np.nan
    with pytest.raises(api.SingularException):
        setup.run(bad)
    Sd1, _ = setup.run(ii)
    fresh = api.SchurSetup(pctx, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd)
    fresh.keep_levels()
    Sd2, _ = fresh.run()
    assert np.all(np.isfinite(Sd1)) and np.array_equal(Sd1, Sd2) and np.array_equal(Sd1, Sd0)
    assert np.array_equal(M.ldiv(x), z0)
    tally["bits"] += 3
    tally["errors"] += 1
    M.close()
    fresh.close()
