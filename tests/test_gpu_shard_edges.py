"""GPU suite (-m gpu): the SHARDED dense path — `DenseBlockOp` with reduce_over_ranks, the XCHG instantiations of k_gemv_pcg,
k_xchg_push, k_xchg_wait_advance and the generic k_xchg_stage / k_xchg_signal_wait / k_xchg_sum all-reduce — on the synthetic
cases of tests/shard_synth.py, with in-process ranks on one GPU (tests/test_gpu_multirank.py: run_ranks). The FEM problems
of the other sharded tests give every rank blocks of nearly equal size, one tiling, multiplicities 1-4 and no empty rank;
here: slices of unequal length, ranks without a streamed tile beside ranks with them, a different tiling on every rank,
blocks of 0 ... 7 rows, slot widths 1, 2, 4 (widened from 3) and 6, exchange sizes around the push chunk and the staging
sizes, and the parity of the exchange number across solves. tests/test_shard_edges_cpu.py asserts that every case has the
property it is named for. References: an np.longdouble apply (summation bound), the single-context operators (bit for
bit where the same kernels sum in the same order, 1e-9 where the per-tile partials are cut differently: the bar of
test_gpu_parity.py's sharded test) and the C oracle. The solves stop at eps = 1e-2 (shard_synth.Case: beyond
that, κ = 1e3 histories follow the order of the sums, not the code under test).
Measured on an MI355X: applies at most 0.026 of their bound, folded histories at most 2.3e-3 of the 1e-9 bar against the
single context, 1.6e-11 relative against the oracle; everything asserted bitwise was bitwise."""
import ctypes as C
import os
from contextlib import contextmanager

import numpy as np
import pytest

import shard_synth as ss
from shard_synth import assert_summation_bound, concat, ref_apply, split
from test_gpu_parity import assert_history

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

CASES = ss.cases()
NAMES = [c.name for c in CASES]


@contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(autouse=True)
def short_peer_timeout(monkeypatch):
    """Read when a context joins its group: a protocol error ends as MI_ERR_COMM in seconds instead of a minute."""
    monkeypatch.setenv("MI355_PEER_TIMEOUT_MS", "20000")


@pytest.fixture(scope="module")
def n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


class Prob:
    """One case with everything that is computed once: blocks, Π = mi_nn_pinv(S), vectors, the oracle's operators, and
    (lazily) the single-context operators and solves."""

    def __init__(self, api, ctx, orc, c):
        self.api, self.ctx, self.orc, self.c = api, ctx, orc, c
        self.g, self.cnt, self.n = c.maps()
        self.S = c.blocks()[0]
        nz = [d for d in range(c.ndom) if c.sizes[d] > 0]
        sz = [c.sizes[d] for d in nz]
        out = split(api.nn_pinv(ctx, np.array(sz, dtype=np.int64), concat([self.S[d] for d in nz])), sz)
        self.Pi = [np.zeros((0, 0), order="F") for _ in range(c.ndom)]
        for d, P in zip(nz, out):
            self.Pi[d] = np.asfortranarray(P)
        self.Pi32 = [P.astype(np.float32).astype(np.float64) for P in self.Pi]
        self.x, self.b, self.x0 = c.vectors()
        self.zero = np.zeros(self.n)
        self.W = c.width()
        self.Ao = orc.apply_local_schurs_operator(self.S, self.g, self.n)
        self.Mo = {"f64": orc.neumann_neumann_operator(self.Pi, self.g, self.cnt),
                   "f32": orc.neumann_neumann_operator(self.Pi32, self.g, self.cnt)}
        self._ops, self._ref, self._orc = {}, {}, {}

    def ops1(self, storage="f64"):
        if storage not in self._ops:
            A = self.api.LocalSchurs(self.ctx, self.S, self.g, self.cnt)
            M = self.api.NeumannNeumannSchurPreconditioner(self.ctx, self.Pi, self.g, self.cnt, storage=storage)
            self._ops[storage] = (A, M)
        return self._ops[storage]

    def solve1(self, fold, start="zero", maxit=0, storage="f64", b=None):
        """pcg on ONE context (default tiling 16 x 2), through the folded launches or with MI355_NO_FOLD=1."""
        key = (fold, start, maxit, storage, b is None)
        if key not in self._ref:
            A, M = self.ops1(storage)
            with env(**({} if fold else {"MI355_NO_FOLD": "1"})):
                self._ref[key] = self.api.pcg(A, self.b if b is None else b, self.x0 if start == "x0" else self.zero, M, maxit=maxit,
                                               eps=self.c.eps)
        return self._ref[key]

    def oracle(self, start="zero", maxit=0, storage="f64", b=None):
        key = (start, maxit, storage, b is None)
        if key not in self._orc:
            self._orc[key] = self.orc.pcg(self.Ao, self.b if b is None else b, self.x0 if start == "x0" else self.zero,
                                          self.Mo[storage], maxit=maxit, eps=self.c.eps)
        return self._orc[key]


_PROBS = {}


@pytest.fixture
def prob(pkg, ctx, orc, n_cu):
    def get(name):
        if name not in _PROBS:
            by = {c.name: c for c in ss.cases(n_cu) + ss.local_cases()}
            _PROBS[name] = Prob(pkg.api, ctx, orc, by[name])
        return _PROBS[name]
    return get


def run_case(api, p, shard_nn, body, group_mode=0, xmode=None, storage="f64", make_ops=None):
    def rank_main(ctx, r):
        A, M = (make_ops or ss.rank_ops)(api, ctx, p.c, r, p.S, p.Pi, shard_nn, storage)
        if xmode is not None:
            ctx.set_exchange(xmode)
        ctx.host_barrier.wait(timeout=120)
        return body(ctx, r, A, M)
    return ss.run_ranks(api, p.c.world, rank_main, mode=group_mode, timeout=300)


def same(a, b):
    return a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[0], b[0])


def assert_folded_bar(got, ref, what):
    """Differently tiled partial dot products: `it` equal, history rtol 1e-9 / atol 1e-13 res_0, x to 1e-9 (test_gpu_parity.py,
    the sharded folded loop against the single context)."""
    assert got[1] == ref[1], f"{what}: it {got[1]} vs single context {ref[1]}"
    dev = float(np.max(np.abs(got[2] - ref[2]) / np.maximum(ref[2], 1e-300))) if ref[2].size and ref[2][0] > 0 else 0.0
    bar = 1e-13 * ref[2][0] + 1e-9 * np.abs(ref[2])
    k = int(np.argmax(np.abs(got[2] - ref[2]) / np.maximum(bar, 1e-300))) if ref[2].size else 0
    print(f"SHARD_FIG {what}: history vs single context, max relative deviation {dev:.3e}; worst entry {k + 1} of {ref[1]}: "
          f"|diff| / (atol + rtol |ref|) = {float(np.abs(got[2][k] - ref[2][k]) / max(bar[k], 1e-300)):.3e}; "
          f"|x - x_ref| / |x_ref| = {float(np.linalg.norm(got[0] - ref[0]) / max(np.linalg.norm(ref[0]), 1e-300)):.3e}")
    assert np.allclose(got[2], ref[2], rtol=1e-9, atol=1e-13 * ref[2][0]), (what, dev)
    assert np.linalg.norm(got[0] - ref[0]) <= 1e-9 * np.linalg.norm(ref[0]), what


def assert_oracle(got, want, p, what):
    m = min(got[1], want[1])
    dev = float(np.max(np.abs(got[2][:m] - want[2][:m]) / want[2][:m])) if m and want[2][0] > 0 else 0.0
    print(f"SHARD_FIG {what}: history vs oracle, max relative deviation {dev:.3e} (it {got[1]} / {want[1]})")
    assert_history(got, want, p.Ao, p.b)


# ------------------------------------------------------------------ applies
@pytest.mark.parametrize("name", NAMES)
def test_sharded_applies(pkg, prob, name):
    """S * x and ΠS * x, both sharded: every rank holds the same bits, and they are the single-context operator's — a row is
    one wave's dot product in a fixed lane order whatever the tiling, and the ranks' slot tables are a disjoint union —
    within (m + 4) eps |A||x| of the long-double reference."""
    api, p = pkg.api, prob(name)

    def body(ctx, r, A, M):
        assert ctx.query("peer_exchange") >= 1
        return A * p.x, M * p.x

    out = run_case(api, p, True, body)
    for r in range(1, p.c.world):
        assert np.array_equal(out[r][0], out[0][0]) and np.array_equal(out[r][1], out[0][1]), r
    A1, M1 = p.ops1()
    assert np.array_equal(out[0][0], A1 * p.x) and np.array_equal(out[0][1], M1 * p.x)
    assert_summation_bound(out[0][0], ref_apply(p.S, p.g, p.cnt, p.x, nn=False), p.W, f"SHARD_FIG {name} S")
    assert_summation_bound(out[0][1], ref_apply(p.Pi, p.g, p.cnt, p.x, nn=True), p.W, f"SHARD_FIG {name} NN")


def test_sharded_fp32_apply(pkg, prob):
    """`tiny` with the Neumann-Neumann blocks held in fp32, sharded: the fp64 apply of double(float(Π))."""
    api, p = pkg.api, prob("tiny")
    out = run_case(api, p, True, lambda ctx, r, A, M: M * p.x, storage="f32")
    for r in range(1, p.c.world):
        assert np.array_equal(out[r], out[0])
    assert np.array_equal(out[0], p.ops1("f32")[1] * p.x)
    assert_summation_bound(out[0], ref_apply(p.Pi32, p.g, p.cnt, p.x, nn=True), p.W, "SHARD_FIG tiny NN fp32")


# ------------------------------------------------------------------ the folded loop across the ranks
FOLDED = [c.name for c in CASES if c.fold and not c.no_fold_env and not c.push]


def pcg_body(api, p, start="zero", maxit=0):
    def body(ctx, r, A, M):
        f0, e0 = ctx.query("folded_pcg"), ctx.query("exchanges")
        res = api.pcg(A, p.b, p.x0 if start == "x0" else p.zero, M, maxit=maxit, eps=p.c.eps)
        return res, ctx.query("exchanges") - e0, ctx.query("folded_pcg") - f0, ctx.query("peer_exchange")
    return body


def check_ranks(out):
    for r in range(1, len(out)):
        assert same(out[r][0], out[0][0]), f"rank {r} differs from rank 0"
        assert out[r][1] == out[0][1], f"exchange counters differ: {[o[1] for o in out]}"    # incl. a rank without a block


@pytest.mark.parametrize("shard_nn", [False, True], ids=["nn_replicated", "nn_sharded"])
@pytest.mark.parametrize("name", FOLDED)
def test_folded_pcg_across_ranks(pkg, prob, name, shard_nn):
    """pcg through the folded launches with S sharded and ΠS replicated (one exchange per iteration) or sharded too (two)."""
    api, p = pkg.api, prob(name)
    out = run_case(api, p, shard_nn, pcg_body(api, p))
    check_ranks(out)
    res, n_xchg, n_fold, _ = out[0]
    assert n_fold > 0, "the folded launches did not run"
    assert n_xchg >= (2 if shard_nn else 1) * (res[1] - 1), (n_xchg, res[1])
    tag = f"{name} {'nn_sharded' if shard_nn else 'nn_replicated'}"
    assert_folded_bar(res, p.solve1(True), tag)
    assert_oracle(res, p.oracle(), p, tag)


def test_folded_pcg_with_replicated_fp32_blocks(pkg, prob):
    """`tiny`, S sharded, ΠS replicated in fp32: still the folded loop (the fp32 launch has no exchange form, and needs none)."""
    api, p = pkg.api, prob("tiny")
    out = run_case(api, p, False, pcg_body(api, p), storage="f32")
    check_ranks(out)
    assert out[0][2] > 0
    assert_folded_bar(out[0][0], p.solve1(True, storage="f32"), "tiny fp32 replicated")
    assert_oracle(out[0][0], p.oracle(storage="f32"), p, "tiny fp32 replicated")


# ------------------------------------------------------------------ the unfolded loop: plain sharded applies + generic all-reduce
UNFOLDED = [("hub6", {}, "f64"), ("wide", {}, "f64"), ("tiny", {}, "f32"), ("tiny", {"MI355_NO_FOLD_SHARDED_NN": "1"}, "f64"),
            ("stage_16384", {"MI355_NO_FOLD": "1"}, "f64"), ("stage_16385", {"MI355_NO_FOLD": "1"}, "f64"),
            ("stage_65600", {"MI355_NO_FOLD": "1"}, "f64")]


@pytest.mark.parametrize("name,envs,storage", UNFOLDED, ids=[f"{n}-{s}{'-' + '+'.join(e) if e else ''}" for n, e, s in UNFOLDED])
def test_unfolded_pcg_across_ranks(pkg, prob, name, envs, storage):
    """Slot width 6, a block wider than the operand panel, a sharded fp32 ΠS, MI355_NO_FOLD_SHARDED_NN=1, and the stage-size
    cases: the 4-launch loop on plain sharded applies. Same kernels, union of slot tables: bit-identical to the single
    context under MI355_NO_FOLD=1."""
    api, p = pkg.api, prob(name)
    with env(**envs):
        out = run_case(api, p, True, pcg_body(api, p, maxit=p.c.maxit), storage=storage)
    check_ranks(out)
    res, n_xchg, n_fold, _ = out[0]
    assert n_fold == 0, "the folded launches ran"
    assert n_xchg >= 2 * (res[1] - 1)
    assert same(res, p.solve1(False, maxit=p.c.maxit, storage=storage)), name
    assert_oracle(res, p.oracle(maxit=p.c.maxit, storage=storage), p, f"{name} unfolded {storage}")


# ------------------------------------------------------------------ the table exchange in one, two and three chunks
@pytest.mark.parametrize("name", [c.name for c in CASES if c.push])
def test_push_kernel_chunks(pkg, prob, name, monkeypatch):
    """MI355_XCHG_PUSH_KERNEL=1 with n_own of rank 0 at 4096 (one full chunk), 4097 (a second chunk of one entry) and 8260
    (three): the same bits as the launches that store into the arenas themselves. Solves capped at 8 iterations."""
    api, p = pkg.api, prob(name)
    direct = run_case(api, p, True, pcg_body(api, p, maxit=p.c.maxit))
    monkeypatch.setenv("MI355_XCHG_PUSH_KERNEL", "1")
    pushed = run_case(api, p, True, pcg_body(api, p, maxit=p.c.maxit))
    check_ranks(direct)
    check_ranks(pushed)
    assert pushed[0][2] > 0 and same(pushed[0][0], direct[0][0]) and pushed[0][1] == direct[0][1]
    assert_folded_bar(pushed[0][0], p.solve1(True, maxit=p.c.maxit), f"{name} pushed")
    assert_oracle(pushed[0][0], p.oracle(maxit=p.c.maxit), p, f"{name} pushed")


# ------------------------------------------------------------------ producers and waits
@pytest.mark.parametrize("name", [c.name for c in CASES if c.modes])
def test_producers_and_waits(pkg, prob, name, n_cu, tmp_path):
    """One-wave wait kernels (mode 1), launches that wait themselves (mode 2), the push kernel, and the group's host
    rendezvous: same bits, same exchange counters. In the blockless cases rank 0 has no streamed tile: it alone produces
    through k_xchg_push (n_own == 0: signal and wait) and, in mode 2, waits in that kernel while its peers wait inside their
    launches and carry the exchange number in xep[] — the two must stay aligned, also after a stop by maxit."""
    api, p = pkg.api, prob(name)
    # mode 2 on one GPU: every rank's workgroups (and a push kernel's) must be resident at once
    lists = ss.tile_lists(ss.build_checker(tmp_path), [p.c], tmp_path, n_cu)[name]
    assert sum(len(R["tiles"]) for R in lists) + p.c.world <= n_cu

    def body(ctx, r, A, M):
        e0 = ctx.query("exchanges")
        res = api.pcg(A, p.b, p.zero, M, eps=p.c.eps)
        e1 = ctx.query("exchanges")
        res2 = api.pcg(A, p.b, p.zero, M, maxit=5, eps=p.c.eps)                # stopped by maxit
        y = A * p.x                                              # the generic all-reduce shares the counter
        return res, res2, y, (e1 - e0, ctx.query("exchanges") - e1), ctx.query("peer_exchange")

    runs = {"mode1": run_case(api, p, True, body, xmode=1), "mode2": run_case(api, p, True, body, xmode=2)}
    with env(MI355_XCHG_PUSH_KERNEL="1"):
        runs["push"] = run_case(api, p, True, body, xmode=1)
    runs["host"] = run_case(api, p, True, body, group_mode=1)
    q = runs["mode2"][0][4]
    print(f"{name}: peer_exchange in mode 2 = {q}" + ("" if q == 3 else " — no fine-grained arena: mode 2 ran as mode 1"))
    assert runs["mode1"][0][4] in (1, 2) and runs["host"][0][4] == 0
    want = runs["mode1"][0]
    for tag, out in runs.items():
        for r in range(p.c.world):
            assert same(out[r][0], want[0]) and same(out[r][1], want[1]) and np.array_equal(out[r][2], want[2]), (tag, r)
            if tag != "host":
                assert out[r][3] == want[3], (tag, r, out[r][3], want[3])
    assert want[1][1] == 5
    assert_folded_bar(want[0], p.solve1(True), f"{name} modes")


# ------------------------------------------------------------------ the exchange number across solves
@pytest.mark.parametrize("xmode", [1, 2])
@pytest.mark.parametrize("name", [c.name for c in CASES if c.sequence])
def test_counter_and_parity_sequence(pkg, prob, name, xmode):
    """One pair of sharded operators through: a solve to convergence; maxit = 1, 2, 3 (maxit = 0 is this API's "no cap": the
    first solve); a plain apply; a solve from a random x0; b = 0; the first solve again. The tables are double-buffered by
    the parity of the exchange number, and the generic sum shares the counter: every step must leave all ranks on the same
    number, whichever parity it ends on — the plain apply in the middle flips it, so solves end on odd and on even counts."""
    api, p = pkg.api, prob(name)

    def sequence(A, M, count):
        tol = p.c.eps
        steps = [lambda: api.pcg(A, p.b, p.zero, M, eps=tol)]
        steps += [lambda k=k: api.pcg(A, p.b, p.zero, M, maxit=k, eps=tol) for k in (1, 2, 3)]
        steps += [lambda: A * p.x, lambda: api.pcg(A, p.b, p.x0, M, eps=tol), lambda: api.pcg(A, p.zero, p.zero, M, eps=tol),
                  lambda: api.pcg(A, p.b, p.zero, M, eps=tol)]
        out, e = [], [count()]
        for f in steps:
            out.append(f())
            e.append(count())
        return out, [int(v) for v in np.diff(e)], [int(v) % 2 for v in e[1:]]

    out = run_case(api, p, True, lambda ctx, r, A, M: sequence(A, M, lambda: ctx.query("exchanges")), xmode=xmode)
    ref = sequence(*p.ops1(), lambda: 0)[0]
    steps0, counts0, parity0 = out[0]
    print(f"{name} mode {xmode}: exchanges per step {counts0}")
    for r in range(p.c.world):
        steps, counts, _ = out[r]
        assert counts == counts0, (r, counts, counts0)
        for k, (a, w) in enumerate(zip(steps, steps0)):
            assert np.array_equal(a, w) if k == 4 else same(a, w), (r, k)
    assert same(steps0[7], steps0[0])                            # the repeated first solve
    for k, (a, w) in enumerate(zip(steps0, ref)):
        if k == 4:
            assert np.array_equal(a, w)
        else:
            assert_folded_bar(a, w, f"{name} mode {xmode} step {k}")
    assert [s[1] for s in steps0[1:4]] == [1, 2, 3]
    # A solve makes 2 it exchanges (its set-up's residual apply included), the plain apply one: the solves before it end on
    # one parity of the exchange number, the solves after it on the other.
    assert all(c == 2 * s[1] for k, (c, s) in enumerate(zip(counts0, steps0)) if k != 4) and counts0[4] == 1, counts0
    assert {parity0[k] for k in (0, 1, 2, 3)} != {parity0[k] for k in (5, 6, 7)} and 1 in parity0, parity0
    assert_oracle(steps0[0], p.oracle(), p, f"{name} mode {xmode} first solve")
    assert_oracle(steps0[5], p.oracle("x0"), p, f"{name} mode {xmode} from x0")


# ------------------------------------------------------------------ one deflated case
def test_deflated_solver_on_uneven_slices(pkg, prob, orc):
    """defpcg (nvec = 3) on `uneven`, 3 ranks, S sharded and ΠS replicated: the 4-launch loop with an all-reduce of the slot
    table after every S-apply, also for A W. Same kernels as the single context under MI355_NO_FOLD=1: same bits."""
    api, p = pkg.api, prob("uneven_w3")
    W = np.asfortranarray(np.linalg.qr(np.random.default_rng(3).standard_normal((p.n, 3)))[0])
    out = run_case(api, p, False, lambda ctx, r, A, M: api.defpcg(A, p.b, p.zero, W, M, eps=p.c.eps))
    for r in range(1, p.c.world):
        assert same(out[r], out[0])
    A1, M1 = p.ops1()
    with env(MI355_NO_FOLD="1"):
        ref = api.defpcg(A1, p.b, p.zero, W, M1, eps=p.c.eps)
    assert same(out[0], ref)
    assert_oracle(out[0], orc.defpcg(p.Ao, p.b, p.zero, W, p.Mo["f64"], eps=p.c.eps), p, "uneven_w3 defpcg")


# ------------------------------------------------------------------ local-only maps (C ABI)
def local_ops(api, ctx, c, r, S, Pi, shard_nn, storage):
    """`mi_schur_assembled_create` / `mi_nn_create_stored` with NULL gather lists for the other ranks' subdomains."""
    from krylov_spdes_amd._lib import check, f64p, i64, i64p, vp
    g, cnt, n = c.maps()
    lo, hi = c.slices()[r]
    gl = [np.ascontiguousarray(g[d], dtype=np.int64) if lo <= d < hi else None for d in range(c.ndom)]
    nd = np.array(c.sizes, dtype=np.int64)
    cn = np.ascontiguousarray(cnt, dtype=np.int64)
    Sb = [np.asfortranarray(S[d]) if lo <= d < hi else None for d in range(c.ndom)]
    Pb = [np.asfortranarray(Pi[d]) if lo <= d < hi else None for d in range(c.ndom)]
    L = ctx._L
    hA, hM = vp(), vp()
    check(L.mi_schur_assembled_create(ctx._h, i64(c.ndom), i64(n), nd.ctypes.data_as(i64p), api._ptrs(gl, i64p), api._ptrs(Sb, f64p),
                                      C.c_int(0), i64(lo), i64(hi), C.byref(hA)))
    check(L.mi_nn_create_stored(ctx._h, i64(c.ndom), i64(n), nd.ctypes.data_as(i64p), api._ptrs(gl, i64p), api._ptrs(Pb, f64p),
                                cn.ctypes.data_as(i64p), C.c_int(0), i64(lo), i64(hi), C.c_int(0), C.byref(hM)))
    return api.Operator(ctx, hA, keep=(gl, nd, Sb)), api.Operator(ctx, hM, keep=(gl, nd, cn, Pb))


@pytest.mark.parametrize("name", ["local_equal", "local_unequal"])
def test_local_only_maps(pkg, prob, name):
    """A rank that was given only its own gather lists numbers the slots of a Γ node among its own subdomains: slot width
    and slot ranks are rank-local. The ranks then add their assembled Γ vectors (n_Γ entries on every rank) instead of
    the slot tables — whose sizes n_Γ W_r differ as soon as the widths do (`local_unequal`: 4 and 2; before this was
    fixed the ranks issued all-reduces of different counts from staging of different offsets). Not a bitwise comparison:
    per-rank partial sums are added (at most W + world terms per node)."""
    api, p = pkg.api, prob(name)

    def body(ctx, r, A, M):
        return A * p.x, M * p.x, api.pcg(A, p.b, p.zero, M, eps=p.c.eps)

    out = run_case(api, p, True, body, make_ops=local_ops)
    for r in range(1, p.c.world):
        assert np.array_equal(out[r][0], out[0][0]) and np.array_equal(out[r][1], out[0][1]) and same(out[r][2], out[0][2])
    width = max(ss.local_width(p.c, r) for r in range(p.c.world)) + p.c.world
    assert_summation_bound(out[0][0], ref_apply(p.S, p.g, p.cnt, p.x, nn=False), width, f"SHARD_FIG {name} S")
    assert_summation_bound(out[0][1], ref_apply(p.Pi, p.g, p.cnt, p.x, nn=True), width, f"SHARD_FIG {name} NN")
    assert_oracle(out[0][2], p.oracle(), p, f"{name} pcg")
