"""GPU suite (-m gpu) of the Krylov loops (csrc/solvers.hpp; k_fused_xr / p / cg / start / residual, k_entry_zero,
k_multi_dot_view, k_defl_mu, k_lu_solve, k_fold_start in csrc/kernels.hpp) at the edges the FEM problems never reach: the
per-thread width of the single-workgroup loop (EPT 1 / 2 / 4 / 8 at n <= 1024 / 2048 / 4096 / 8192), view widths 0, 1, 2, 4
and 6 crossed with it, the deflation counts at which k_fused_p's column groups, k_defl_mu's shuffle tree, its second pass
over the partials, its columns past the 20 preloaded ones and the in-kernel LU change, the start-up forms, and replay.
Inputs and case tables: tests/krylov_synth.py. tests/test_krylov_edges_cpu.py proves on the oracle that every solve here
is short (<= 50 iterations), ends on a decided stop and is insensitive to the summation order, so DESIGN §3's strict row
applies to all of them.

Bar (not new): `it` equal to the oracle's, every res_norm entry within 1e-8 res_k + 1e-12 res_1, x within 1e-6 relative
(`strict`, which also calls test_gpu_parity.assert_history). Across loop forms `it` is equal; replay comparisons are bit for
bit. Every comparison prints its figures in units of the bar before it asserts. The oracle's Neumann-Neumann operator is
built on the very Π blocks the device uses (mi_nn_pinv).

No defect was found in the loops. Measured on an MI355X (153 tests, 9 s in all, no test above 0.4 s; figures in units of the
bar): 755 comparisons with the oracle, `it` equal in all of them and across the loop forms (46 iterations at most: cg on
sp4096 ... sp8193 from a random x0); res_norm <= 7.3e-4 (d2048w1, pcg from a random x0, folded), x <= 3.5e-7 (d1025w6, cg);
all 18 chunk comparisons and all 24 replayed-against-eager solves bit-identical.
Sensitivity, each defect seeded once into a scratch build and this file run against it:
  * `n <= 2 * NTF + 1` in the EPT dispatch (Krylov::with_ept): sp2049, d2049w2, d2049w4 fail. (`n < 2 * NTF` changes no bit: n = 2048 then runs
    the EPT 4 instantiation, whose guarded extra elements add +0.0 to every thread's sums in the same order.)
  * the partial column group of k_fused_p dropped (`q0 + QB <= nvec`): 87 tests fail — every nvec that is no multiple of 8
    (nloc*, tiles*, d1025w4 7 / 9) or of 4 at EPT 8 (d4097w4 and sp8192 with 3, 5, 9), and every nvec = 65;
  * the later passes of k_defl_mu over the partials skipped: tiles336 with 33, 36, 37, 64 and tiles544 with 17 ... 64 fail;
  * view_load's generic loop one slot short: d2048w1 and d1025w6 fail;
  * k_defl_mu's columns past the 20 preloaded ones ignored: the 30 folded cases with nvec 21 ... 64 fail (20 passes).
"""
import numpy as np
import pytest

import krylov_synth as ks
from test_gpu_dense_edges import concat, split
from test_gpu_parity import assert_history

pytestmark = pytest.mark.gpu

DEFAULT_CHUNK = 8


@pytest.fixture(scope="module")
def probs(pkg, ctx, orc):
    api = pkg.api

    def pinv(d, S):
        return split(api.nn_pinv(ctx, np.array(d.sizes, dtype=np.int64), concat(S)), d.sizes)
    return ks.Problems(orc, pinv)


@pytest.fixture(scope="module")
def worst():
    w = {"res": (0.0, ""), "x": (0.0, ""), "n": 0}
    yield w
    print(f"\n  krylov edges: {w['n']} comparisons with the oracle; largest res_norm deviation {w['res'][0]:.3e} of the bar "
          f"({w['res'][1]}), largest x deviation {w['x'][0]:.3e} of the bar ({w['x'][1]})")


def make_ops(api, ctx, probs, prob, monkeypatch):
    """device operators of a problem by role: A, and jacobi + identity (sparse) or nn (dense)"""
    if prob in ks.SPARSE:
        A = probs.matrix(prob)
        return {"A": api.SparseMatrixCSC(ctx, A), "jacobi": api.JacobiPreconditioner(ctx, A.diagonal()),
                "identity": api.IdentityPreconditioner(ctx, A.shape[0])}
    d = ks.DENSE[prob]
    g, cnt, n = probs.maps(prob)
    S, Pi = probs.blocks(prob), probs.pi_blocks(prob)
    if d.tiling:                                    # read when an operator is constructed
        monkeypatch.setenv("MI355_GEMV_WAVES", str(d.tiling[0]))
        monkeypatch.setenv("MI355_GEMV_RPW", str(d.tiling[1]))
    try:
        return {"A": api.LocalSchurs(ctx, S, g, cnt), "nn": api.NeumannNeumannSchurPreconditioner(ctx, Pi, g, cnt)}
    finally:
        if d.tiling:
            monkeypatch.delenv("MI355_GEMV_WAVES")
            monkeypatch.delenv("MI355_GEMV_RPW")


def close_ops(ops):
    for op in ops.values():
        op.close()


class GpuOps:
    """operators per problem, built once for the deflated solves (every (operators, nvec) pair is solved once per form)"""

    def __init__(self, api, ctx, probs):
        self.api, self.ctx, self.probs, self._ops = api, ctx, probs, {}

    def __call__(self, prob, monkeypatch):
        if prob not in self._ops:
            self._ops[prob] = make_ops(self.api, self.ctx, self.probs, prob, monkeypatch)
        return self._ops[prob]

    def close(self):
        for ops in self._ops.values():
            close_ops(ops)
        self._ops = {}


@pytest.fixture(scope="module")
def gops(pkg, ctx, probs):
    g = GpuOps(pkg.api, ctx, probs)
    yield g
    g.close()


def gpu_run(api, ops, probs, s, bkind="b"):
    pre = probs.precond(s)
    return ks.run(api, s, ops["A"], ops[pre] if pre else None, probs.b(s.prob, bkind), probs.x0(s), probs.W(s))


def with_env(monkeypatch, env, fn):
    for k in env:
        monkeypatch.setenv(k, "1")
    try:
        return fn()
    finally:
        for k in env:
            monkeypatch.delenv(k)


def strict(tag, got, want, probs, s, worst, bkind="b"):
    """DESIGN §3, the strict row, over the whole history"""
    x, it, res = got
    xo, ito, reso = want
    hm, xm = ks.history_margin(res, reso), ks.x_margin(x, xo)
    print(f"  {tag}: it {it} (oracle {ito}), res_norm / bar = {hm:.3e}, |x - x_o| / (1e-6 |x_o|) = {xm:.3e}")
    worst["n"] += 1
    if np.isfinite(hm) and hm > worst["res"][0]:
        worst["res"] = (hm, tag)
    if np.isfinite(xm) and xm > worst["x"][0]:
        worst["x"] = (xm, tag)
    assert it == ito, f"{tag}: iteration counts differ: {it} vs oracle {ito}"
    assert res.shape == reso.shape and np.all(np.isfinite(res)) and np.all(np.isfinite(x)), tag
    assert np.all(np.abs(res - reso) <= ks.RES_RTOL * reso + ks.RES_FLOOR * reso[0]), f"{tag}: res_norm {hm:.3e} of the bar"
    assert np.linalg.norm(x - xo) <= ks.X_RTOL * np.linalg.norm(xo), f"{tag}: x {xm:.3e} of the bar"
    if max(it, ito) <= 20:
        assert_history(got, want, apply=probs.op(s.prob, "A"), b=probs.b(s.prob, bkind))


def same_bits(got, ref, tag):
    print(f"  {tag}: it {got[1]} vs {ref[1]}, res_norm equal {np.array_equal(got[2], ref[2])}, x equal {np.array_equal(got[0], ref[0])}")
    assert got[1] == ref[1], tag
    assert np.array_equal(got[2], ref[2]), tag
    assert np.array_equal(got[0], ref[0]), tag


# ------------------------------------------------------------------ 1. sparse sizes: EPT 1 / 2 / 4 / 8 with plain vectors
@pytest.mark.parametrize("prob", list(ks.SPARSE))
def test_sparse_sizes_fused_and_multi_workgroup(pkg, ctx, probs, worst, monkeypatch, prob):
    """cg (k_fused_cg<EPT>), Jacobi pcg and identity pcg (k_fused_residual / start / xr / p<EPT>) from zero and from a random
    x0, maxit 0, 1, 2; n = 8193 leaves the single-workgroup loop. Each against the oracle, and against MI355_NO_FUSED=1."""
    api = pkg.api
    ops = make_ops(api, ctx, probs, prob, monkeypatch)
    try:
        for s in ks.sparse_solves(prob):
            want = probs.solve(s)
            fused = gpu_run(api, ops, probs, s)
            strict(f"{s.id} default (EPT {ks.ept(ks.SPARSE[prob])})", fused, want, probs, s, worst)
            multi = with_env(monkeypatch, ["MI355_NO_FUSED"], lambda: gpu_run(api, ops, probs, s))
            strict(f"{s.id} MI355_NO_FUSED", multi, want, probs, s, worst)
            assert multi[1] == fused[1]
    finally:
        close_ops(ops)


# ------------------------------------------------------------------ 2. dense sizes x slot widths, three loop forms
@pytest.mark.parametrize("prob", ks.GROUP2)
def test_dense_sizes_and_widths_in_three_loop_forms(pkg, ctx, probs, worst, monkeypatch, prob):
    """Folded (k_entry_zero<EPT> / k_fused_residual<EPT, true> start-up), MI355_NO_FOLD=1 (the single-workgroup loop over slot
    views: k_fused_residual<EPT, false>, k_fused_start, k_fused_xr, k_fused_p, and k_fused_cg for cg) and MI355_NO_FUSED=1.
    In the default form pcg from zero runs twice before the random x0: the second one takes the zero entry, the random x0
    then makes that entry report back (respec), and the last solve enters the general way again."""
    api = pkg.api
    d = ks.DENSE[prob]
    ops = make_ops(api, ctx, probs, prob, monkeypatch)
    pz, pr, cg = ks.dense_solves(prob)
    its = {}
    try:
        for form, env in (("default", []), ("MI355_NO_FOLD", ["MI355_NO_FOLD"]), ("MI355_NO_FUSED", ["MI355_NO_FUSED"])):
            order = [pz, pz, pr, pz] if form == "default" else [pz, pr]
            before = ctx.query("folded_pcg")
            for k, s in enumerate(order):
                got = with_env(monkeypatch, env, lambda: gpu_run(api, ops, probs, s))
                strict(f"{s.id} {form} #{k} (EPT {ks.ept(d.n)}, W {d.slot_width})", got, probs.solve(s), probs, s, worst)
                its.setdefault(s, set()).add(got[1])
            rose = ctx.query("folded_pcg") > before
            assert rose == (form == "default" and d.folds), f"{prob} {form}: folded launches issued: {rose}"
            before = ctx.query("folded_pcg")
            got = with_env(monkeypatch, env, lambda: gpu_run(api, ops, probs, cg))
            strict(f"{cg.id} {form}", got, probs.solve(cg), probs, cg, worst)
            its.setdefault(cg, set()).add(got[1])
            assert ctx.query("folded_pcg") == before                     # cg never folds
        assert all(len(v) == 1 for v in its.values()), its               # `it` equal across the forms
    finally:
        close_ops(ops)


# ------------------------------------------------------------------ 3. deflated solves
@pytest.mark.parametrize("s", ks.DEFLATED_SOLVES, ids=lambda s: s.id)
def test_deflated_solves_at_count_edges(pkg, ctx, probs, gops, worst, monkeypatch, s):
    """Dense operators: folded (k_defl_mu; its grid at nloc 1023 / 1024 / 1025, its tree widths, its second pass at more than
    256 / 512 tiles, its columns past 20) and MI355_NO_FOLD_DEFL=1 (k_multi_dot_view + k_fused_p with the in-kernel LU over
    slot views). Sparse operators and defcg: the single-workgroup loop. nvec = 65 takes the generic projection
    (k_multi_dot_partial + k_lu_solve's shared-memory loop) and does not fold."""
    api = pkg.api
    ops = gops(s.prob, monkeypatch)
    want = probs.solve(s)
    dense = s.prob in ks.DENSE
    folds = dense and ks.DENSE[s.prob].folds and s.kind == "defpcg" and s.nvec <= 64
    before = ctx.query("folded_pcg")
    got = gpu_run(api, ops, probs, s)
    rose = ctx.query("folded_pcg") > before
    strict(f"{s.id} default", got, want, probs, s, worst)
    assert rose == folds, f"{s.id}: folded launches issued: {rose}"
    if dense and s.kind == "defpcg":
        before = ctx.query("folded_pcg")
        unf = with_env(monkeypatch, ["MI355_NO_FOLD_DEFL"], lambda: gpu_run(api, ops, probs, s))
        strict(f"{s.id} MI355_NO_FOLD_DEFL", unf, want, probs, s, worst)
        assert ctx.query("folded_pcg") == before and unf[1] == got[1]


# ------------------------------------------------------------------ 4. big-fold start-up (n_Γ > 8192)
def test_big_fold_start_up(pkg, ctx, probs, worst, monkeypatch):
    """k_residual + k_fold_start in front of the folded launches, from zero and from a non-zero x0, against
    MI355_NO_BIG_FOLD=1 (the multi-workgroup loop) and the oracle."""
    api = pkg.api
    assert ks.DENSE[ks.BIG].n > ks.FUSED_MAX_N and ks.DENSE[ks.BIG].folds
    ops = make_ops(api, ctx, probs, ks.BIG, monkeypatch)
    try:
        # (the counter counts launches as they are issued: the second solve replays the first one's graph)
        before = ctx.query("folded_pcg")
        folded = {}
        for s in ks.BIG_SOLVES:
            folded[s] = gpu_run(api, ops, probs, s)
            strict(f"{s.id} default", folded[s], probs.solve(s), probs, s, worst)
        assert ctx.query("folded_pcg") > before
        before = ctx.query("folded_pcg")
        for s in ks.BIG_SOLVES:
            plain = with_env(monkeypatch, ["MI355_NO_BIG_FOLD"], lambda: gpu_run(api, ops, probs, s))
            strict(f"{s.id} MI355_NO_BIG_FOLD", plain, probs.solve(s), probs, s, worst)
            assert plain[1] == folded[s][1]
        assert ctx.query("folded_pcg") == before
    finally:
        close_ops(ops)
        probs.drop(ks.BIG)


# ------------------------------------------------------------------ 5. replay
@pytest.mark.parametrize("s", ks.REPLAY, ids=lambda s: s.id)
def test_chunk_sizes_around_the_iteration_count(pkg, ctx, probs, worst, monkeypatch, s):
    """Fresh operators have no prediction: the first replay holds the set-up and `chunk` iterations, `chunk`-sized replays
    follow. chunk = it - 1 is exactly the loop's length, it and it + 1 overshoot, 1 replays every iteration, 0 is eager."""
    api = pkg.api
    want = probs.solve(s)
    it = want[1]
    ref = None
    try:
        for chunk in (DEFAULT_CHUNK, 0, 1, it - 1, it, it + 1, 64):
            ops = make_ops(api, ctx, probs, s.prob, monkeypatch)
            try:
                ctx.set_chunk(chunk)
                got = gpu_run(api, ops, probs, s)
            finally:
                close_ops(ops)
            if ref is None:
                ref = got
                strict(f"{s.id} chunk {chunk}", ref, want, probs, s, worst)
            else:
                same_bits(got, ref, f"{s.id} chunk {chunk} vs chunk {DEFAULT_CHUNK}")
    finally:
        ctx.set_chunk(DEFAULT_CHUNK)


@pytest.mark.parametrize("s", ks.REPLAY, ids=lambda s: s.id)
def test_sequence_on_one_pair_of_operators(pkg, ctx, probs, worst, monkeypatch, s):
    """The solve, maxit = 2, a looser eps (shorter than predicted), a tighter eps (longer), a random x0 (the zero entry
    reports back), x0 = 0 again, b = 0, the first solve again — on one pair of operators with replayed graphs, against the
    same solves on fresh operators with eager launches (which consult neither graphs nor the prediction nor the zero-entry
    map): bit for bit. The eager results against the oracle."""
    api = pkg.api
    seq = ks.replay_sequence(s)
    ops = make_ops(api, ctx, probs, s.prob, monkeypatch)
    try:
        replayed = [gpu_run(api, ops, probs, t, bk) for t, bk in seq]
    finally:
        close_ops(ops)
    ops = make_ops(api, ctx, probs, s.prob, monkeypatch)
    try:
        ctx.set_chunk(0)
        eager = [gpu_run(api, ops, probs, t, bk) for t, bk in seq]
    finally:
        ctx.set_chunk(DEFAULT_CHUNK)
        close_ops(ops)
    for k, ((t, bk), got, ref) in enumerate(zip(seq, replayed, eager)):
        tag = f"{t.id} b={bk} (solve {k + 1} of the sequence)"
        strict(f"{tag} eager", ref, probs.solve(t, bk), probs, t, worst, bk)
        same_bits(got, ref, f"{tag} replayed vs eager")
