"""GPU suite of the batched PCG (`api.pcg_batch`, csrc/batch_solvers.hpp) and of the multi-workgroup (GENERIC) loop it repeats
(csrc/solvers.hpp, csrc/kernels.hpp) where their grids and buffers cap. Inputs and CPU restatements: tests/batch_limit_cases.py;
tests/test_batch_limits_cpu.py holds every input to the condition that makes it an edge.

Two bars:

  BITS        system t of a batch against its separate device solve in the GENERIC form (`World.check` of test_gpu_batch.py:
              `it` equal, res_norm[:it] and x equal under np.array_equal(..., equal_nan=True)); the separate solves run under
              `World.env` (MI355_NO_FUSED=1 for n <= 8192, MI355_NO_CSRFOLD=1)
  REFERENCE   a separate device solve against a CPU solve of the same recurrences (the C oracle's cg; for the bank the numpy pcg
              with `amg_ref.cycle` on the hierarchy `fem.amg_refresh` builds on the same aggregates), by the tight branch of
              `assert_history` (test_gpu_parity.py): `it` equal, RES_RTOL, RES_FLOOR, X_RTOL

1. the capped vector grid: n = 524 289 (second pass of one element, 1543 row blocks: lanes 1 .. 7 of sum_partials) and n = 696 323
   (2049 row blocks: a second pass of sum_partials), cg in the batch, in the GENERIC and in the two-launch sparse form; a bank of two
   members at 524 289 rows
2. solves past BATCH_RES_STAGE = 1024 iterations beside short ones: both copy paths of res_norm, the set-up graph capped at 1024
   iterations, a short batch frozen inside that graph
3. it = n + 1 on the device: BoundsError with x, it and res_norm[:n] of the separate solve
4. NaN / Inf that arise inside the loop of one system while its neighbours go on
5. more than 48 set-up graphs: the eviction of the map the single solvers of that size share"""
import ctypes as C
import time

import numpy as np
import pytest

import batch_limit_cases as blc
import test_gpu_batch as tgb
from test_gpu_parity import TIGHT_PREFIX, assert_history

pytestmark = pytest.mark.gpu

_worlds = {}


class LimitWorld(tgb.World):
    """`World` of test_gpu_batch.py on given matrices: slot s of the batch holds mats[s] (a matrix, or its CSR values), the bank
    (if there are aggregates) the hierarchies of mats[:members]"""

    def __init__(self, api, ctx, name, mats, bs, capacity, aggs=None, members=0, terms=16):
        self.api, self.ctx, self.name = api, ctx, name
        self.mats, self.bs, self.aggs = list(mats), list(bs), aggs
        self.n = self.mats[0].shape[0]
        self.batch = api.CsrBatch(ctx, self.mats[0], capacity)
        for s, A in enumerate(self.mats):
            self.batch.set_values(s, A)
        self.bank = self.view = None
        self.bank_seconds = 0.0
        if aggs is not None:
            ctx.synchronize()
            t0 = time.perf_counter()
            self.bank = api.AMGBank(ctx, self.mats[0], members, aggregates=aggs)
            for p in range(members):
                self.bank.set_values(p, self.mats[p])
            ctx.synchronize()
            self.bank_seconds = time.perf_counter() - t0
            self.view = self.bank.view(terms)
        self.A_op = api.SparseMatrixCSC(ctx, self.mats[0])
        self.in_op = 0
        self.refs = {}

    def operator(self, slot):
        """the one CsrOperator with the values of slot `slot`"""
        if self.in_op != slot:
            self.A_op.set_values(self.mats[slot])
            self.in_op = slot
        return self.A_op

    def close(self):
        if self.view is not None:
            self.view.close()
        self.A_op.close(); self.batch.close()
        if self.bank is not None:
            self.bank.close()


def make_world(pkg, ctx, fem, name) -> LimitWorld:
    if name in _worlds:
        return _worlds[name]
    api = pkg.api
    if name in blc.BIG_N:
        mats, bs, _ = blc.big(name)
        W = LimitWorld(api, ctx, name, mats, bs, 2)
    elif name == "big_a_bank":
        mats, bs, _ = blc.big("big_a")
        W = LimitWorld(api, ctx, name, mats, bs, 2, aggs=blc.big_aggregates("big_a"), members=blc.BANK_P, terms=3)
    elif name == "lap2049":
        mats, b = blc.lap2049()
        W = LimitWorld(api, ctx, name, mats, [b] * len(mats), len(mats))
    elif name == "lap301":
        mats, b, _ = blc.lap301()
        W = LimitWorld(api, ctx, name, mats, [b] * len(mats), len(mats))
    else:
        assert name == "N34"                                  # the N34 world of test_gpu_batch.py, and the poisoned slots 6, 7
        mats, bs, aggs = tgb.systems(fem, "N34")
        mats = mats + [blc.poisoned_values(mats[1], "A_nan"), blc.poisoned_values(mats[2], "A_zero")]
        W = LimitWorld(api, ctx, name, mats, bs + [bs[1], bs[2]], tgb.CAPACITY, aggs=aggs, members=tgb.P)
    _worlds[name] = W
    return W


@pytest.fixture(scope="module", autouse=True)
def _close_worlds():
    yield
    for w in _worlds.values():
        w.close()
    _worlds.clear()


@pytest.fixture(scope="module")
def bank_world(pkg, ctx, fem):
    """the bank of two members at 524 289 rows, built once (its set-up time is printed and is no part of a test's own time)"""
    W = make_world(pkg, ctx, fem, "big_a_bank")
    print(f"big_a: bank of {blc.BANK_P} members on {W.n} rows, {W.bank.n_levels} levels: set-up {W.bank_seconds:.2f} s")
    return W


def assert_reference(got, ref, tag):
    """REFERENCE: the tight branch of assert_history, which needs both counts at most TIGHT_PREFIX"""
    x, it, res = got
    print(f"{tag}: it = {it} (reference {ref[1]}), max |res - ref| / ref = {np.max(np.abs(res[:min(it, ref[1])] - ref[2][:min(it, ref[1])]) / ref[2][:min(it, ref[1])]):.2e}, "
          f"|x - ref| / |ref| = {np.linalg.norm(x - ref[0]) / np.linalg.norm(ref[0]):.2e}")
    assert ref[1] <= TIGHT_PREFIX and it == ref[1], f"{tag}: it = {it}, the reference {ref[1]}"
    assert_history(got, ref)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def same_batch(u, v):
    return same(np.asarray(u[0]), np.asarray(v[0])) and same(u[1], v[1]) and all(same(p, q) for p, q in zip(u[2], v[2]))


# ------------------------------------------------------------------ C entry points with a residual buffer of the caller's
def c_cg(pkg, ctx, A_op, b, x0, maxit, cap):
    """(rc, x, it, res[cap] filled with -1 before) of mi_cg on host arrays"""
    lib, L = pkg._lib.load(), pkg._lib
    pkg.api.check(lib.mi_ctx_set_pointer_mode(ctx._h, L.MI_PTR_HOST))
    b, x = np.ascontiguousarray(b, dtype=np.float64), np.array(x0, dtype=np.float64, copy=True)
    res, it = np.full(cap, -1.0), C.c_int64()
    rc = lib.mi_cg(A_op._h, C.c_void_p(b.ctypes.data), C.c_void_p(x.ctypes.data), maxit, 1e-7, res.ctypes.data_as(L.f64p), cap, C.byref(it))
    return rc, x, int(it.value), res


def c_pcg_batch(pkg, ctx, batch, slots, B, X0, maxit, ldres):
    """(rc, X, its, res[ldres x k] filled with -1 before) of mi_pcg_batch without a preconditioner on host arrays"""
    lib, L = pkg._lib.load(), pkg._lib
    pkg.api.check(lib.mi_ctx_set_pointer_mode(ctx._h, L.MI_PTR_HOST))
    k, n = len(slots), B.shape[0]
    B, X = np.asfortranarray(B, dtype=np.float64), np.array(X0, dtype=np.float64, order="F", copy=True)
    sl = np.array(slots, dtype=np.int64)
    res, it = np.full((ldres, k), -1.0, order="F"), np.zeros(k, dtype=np.int64)
    rc = lib.mi_pcg_batch(batch._h, k, sl.ctypes.data_as(L.i64p), None, None, C.c_void_p(B.ctypes.data), n, C.c_void_p(X.ctypes.data), n,
                          maxit, 1e-7, res.ctypes.data_as(L.f64p), ldres, it.ctypes.data_as(L.i64p))
    return rc, X, it, res


# ------------------------------------------------------------------ 1. the capped vector grid
@pytest.mark.parametrize("name", ["big_a", "big_b"])
def test_capped_grid_cg(pkg, ctx, fem, orc, monkeypatch, name):
    """vec_grid = 512 and a second pass in k_update_xr, k_update_p, k_dot_partial and their k_b* forms, a second trip of the plain
    grid-stride loops; the p'Ap partials: 1543 (big_a: lanes 1 .. 7 of sum_partials) and 2049 (big_b: its second pass)"""
    api = pkg.api
    W = make_world(pkg, ctx, fem, name)
    mats, bs, X0 = blc.big(name)
    assert W.n == blc.big_n(name) and blc.vec_grid(W.n) == blc.MAX_PARTS and blc.passes(W.n, blc.MAX_PARTS) == 2
    B = np.asfortranarray(np.column_stack(bs))
    refs = [blc.big_cg_ref(orc, name, t) for t in range(2)]
    for t in range(2):                                        # the default form: two launches per iteration, a vector grid of 256
        assert_reference(api.cg(W.operator(t), bs[t], X0[:, t]), refs[t], f"{name}, default form, system {t}")
    W.env(monkeypatch)
    got = api.pcg_batch(W.batch, [0, 1], B, X0, None)
    its = W.check([0, 1], None, B, X0, got)                   # BITS
    print(f"{name}: n = {W.n}, batch it = {its}")
    for t in range(2):
        assert_reference(W.separate(t, None, np.ascontiguousarray(B[:, t]), np.ascontiguousarray(X0[:, t])), refs[t], f"{name}, GENERIC form, system {t}")


def test_capped_grid_bank(pkg, ctx, fem, monkeypatch, bank_world):
    """k_update_xr with precond = 1 and the r'z partials at g = 512; slot 1 under the stale member 0 runs some thirty iterations"""
    W = bank_world
    W.env(monkeypatch)
    _, bs, X0 = blc.big("big_a")
    slots, members = [0, 1, 1], [0, 1, 0]
    B = np.asfortranarray(np.column_stack([bs[s] for s in slots]))
    X = np.zeros_like(B)
    X[:, 1] = X0[:, 1]
    got = pkg.api.pcg_batch(W.batch, slots, B, X, W.view, members)
    its = W.check(slots, members, B, X, got)                  # BITS
    print(f"big_a bank: batch it = {its}")
    assert its[2] > its[1], "slot 1 under the stale member 0 stops no later than under its own"
    assert_reference(W.separate(0, 0, np.ascontiguousarray(B[:, 0]), np.zeros(W.n)), blc.big_bank_ref(fem, "big_a"), "big_a bank, slot 0 under member 0")


# ------------------------------------------------------------------ 2. long solves
def _lap2049_columns(W, slots):
    B = np.asfortranarray(np.column_stack([W.bs[s] for s in slots]))
    return B, np.zeros_like(B)


def test_long_solves_and_the_capped_first_graph(pkg, ctx, fem, orc, monkeypatch):
    api = pkg.api
    W = make_world(pkg, ctx, fem, "lap2049")
    W.env(monkeypatch)
    n, allslots = W.n, [0, 1, 2, 3]
    B, X0 = _lap2049_columns(W, allslots)
    want = [W.separate(s, None, W.bs[s], np.zeros(n)) for s in allslots]       # before any counter is read: these capture too
    its = [w[1] for w in want]
    print(f"lap2049: the separate solves' it = {its}")
    assert its[0] <= blc.LOW * blc.BATCH_RES_STAGE and its[1] <= blc.LOW * blc.BATCH_RES_STAGE
    assert its[2] >= blc.HIGH * blc.BATCH_RES_STAGE and its[3] == n
    assert ctx.query("no_graph") == 0
    fresh = api.CsrBatch(ctx, W.mats[0], 4)                   # a (batch, None) that no solve has met
    try:
        for s in allslots:
            fresh.set_values(s, W.mats[s])
        counters = lambda: (ctx.query("graph_captures"), ctx.query("graph_replays"))
        c0, r0 = counters()
        a = api.pcg_batch(fresh, allslots, B, X0, None)       # (a) both copy paths of res_norm in one call
        c1, r1 = counters()
        W.check(allslots, None, B, X0, a, tag="(a)")
        assert c1 > c0
        bb = api.pcg_batch(fresh, allslots, B, X0, None)      # (b) predicted length 2048: the set-up graph of 1024 iterations
        c2, r2 = counters()
        W.check(allslots, None, B, X0, bb, tag="(b)")
        assert c2 - c1 <= 1, f"(b) captured {c2 - c1} graphs"
        chunk_replays = -(-(n - 1 - blc.FIRST_CAP) // 8)      # iterations left after the first graph, eight per replay
        assert 1 + chunk_replays <= r2 - r1 <= 1 + chunk_replays + 2, f"(b) replayed {r2 - r1} graphs: not one of {blc.FIRST_CAP} iterations and {chunk_replays} chunks"
        short = [0, 1]
        Bs, Xs = _lap2049_columns(W, short)
        c = api.pcg_batch(fresh, short, Bs, Xs, None)         # (c) both systems frozen inside the graph of 1024 iterations
        c3, r3 = counters()
        W.check(short, None, Bs, Xs, c, tag="(c)")
        assert c3 == c2 and r3 - r2 == 1, f"(c): {c3 - c2} captures, {r3 - r2} replays"
        assert blc.FIRST_CAP - max(c[1]) >= 500
        with pytest.raises(api.BoundsError) as e:             # (d) a capacity between the counts
            api.pcg_batch(fresh, allslots, B, X0, None, ldres=1100)
        c4, r4 = counters()
        assert "ldres = 1100" in str(e.value) and str(its[3]) in str(e.value)
        assert same(e.value.its, a[1]) and same(np.asarray(e.value.X), np.asarray(a[0])), "(d): its and X of the refused batch"
        print(f"lap2049: captures {c0} -> {c1} -> {c2} -> {c3} -> {c4}; replays {r1 - r0}, {r2 - r1}, {r3 - r2}, {r4 - r3}")
        rc, Xc, itc, res = c_pcg_batch(pkg, ctx, fresh, allslots, B, X0, 0, 1100)   # ... and what it left in the caller's res_norm
        assert rc == pkg._lib.MI_ERR_RES_CAPACITY and same(itc, a[1]) and same(Xc, np.asarray(a[0]))
        for t in allslots:
            m = min(its[t], 1100)
            assert same(res[:m, t], want[t][2][:m]) and np.all(res[m:, t] == -1.0), f"(d): res_norm of system {t}"
    finally:
        fresh.close()
    # REFERENCE, through the long branch of assert_history with the true residual
    A0 = W.mats[0]
    assert_history(want[0], blc.oracle_cg(orc, A0, W.bs[0]), apply=lambda x: A0 @ x, b=W.bs[0])


def test_long_solves_eager(pkg, ctx, fem, monkeypatch):
    W = make_world(pkg, ctx, fem, "lap2049")
    W.env(monkeypatch)
    slots = [0, 2]
    B, X0 = _lap2049_columns(W, slots)
    try:
        ctx.set_chunk(0)
        got = pkg.api.pcg_batch(W.batch, slots, B, X0, None)
    finally:
        ctx.set_chunk(8)
    its = W.check(slots, None, B, X0, got, tag="eager")
    assert its[0] < blc.BATCH_RES_STAGE < its[1]


# ------------------------------------------------------------------ 3. overflow on the device
def test_overflow_on_the_device(pkg, ctx, fem, monkeypatch):
    api, L = pkg.api, pkg._lib
    W = make_world(pkg, ctx, fem, "lap301")
    W.env(monkeypatch)
    _, b, maxit = blc.lap301()
    n = W.n
    slots = [0, 1, 0]
    B = np.asfortranarray(np.column_stack([b, b, np.zeros(n)]))
    X0 = np.zeros_like(B)
    Bc, Xc = np.asfortranarray(B[:, :2]), np.asfortranarray(X0[:, :2])
    before = api.pcg_batch(W.batch, [0, 1], Bc, Xc, None)
    W.check([0, 1], None, Bc, Xc, before, tag="clean, before")
    with pytest.raises(api.BoundsError) as e:
        api.pcg_batch(W.batch, slots, B, X0, None, maxit=maxit)
    its, X = e.value.its, np.asarray(e.value.X)
    print(f"lap301: maxit = {maxit}: it = {list(its)}")
    assert its[0] == n + 1 and its[2] == 1
    with pytest.raises(api.BoundsError) as es:                # the separate solve of the overflowing system
        api.cg(W.operator(0), b, np.zeros(n), maxit=maxit)
    assert es.value.it == n + 1 and same(X[:, 0], es.value.x), "x of the overflowing system"
    for t in (1, 2):
        x, it, _ = W.separate(slots[t], None, np.ascontiguousarray(B[:, t]), np.zeros(n), maxit)
        assert its[t] == it and same(X[:, t], x), f"system {t} beside the overflowing one"
    assert its[1] < blc.LOW * n and not X[:, 2].any()
    # res_norm through the C entry points: n entries of the overflowing system, nothing beyond
    rc, Xb, itb, res = c_pcg_batch(pkg, ctx, W.batch, slots, B, X0, maxit, n + 1)
    assert rc == L.MI_ERR_RES_CAPACITY and same(itb, its) and same(Xb, X)
    rc1, x1, it1, res1 = c_cg(pkg, ctx, W.operator(0), b, np.zeros(n), maxit, n + 1)
    assert rc1 == L.MI_ERR_RES_CAPACITY and it1 == n + 1 and same(x1, X[:, 0])
    assert same(res[:n, 0], res1[:n]) and np.isfinite(res1[:n]).all() and (res1[:n] > 0).all(), "res_norm[:n] of the overflowing system"
    assert res[n, 0] == -1.0 and res1[n] == -1.0, "res_norm[n + 1] was written"
    for t in (1, 2):
        rn = W.separate(slots[t], None, np.ascontiguousarray(B[:, t]), np.zeros(n), maxit)[2]
        assert same(res[:its[t], t], rn) and np.all(res[its[t]:, t] == -1.0)
    after = api.pcg_batch(W.batch, [0, 1], Bc, Xc, None)
    assert same_batch(after, before), "the batch after the overflow differs from the one before"


# ------------------------------------------------------------------ 4. non-finite values inside the loop
POISONED = {"A_nan": (6, 0), "A_zero": (7, 0), "x0_inf": (2, 0)}      # (slot, member) of the poisoned system
CLEAN_FOR = (1, 0)                                                    # what stands in its place in the clean batch
NEIGHBOURS = [(1, 0), (3, 0), (2, 2), (5, 0)]                         # under the stale member 0: 50+ iterations


def _layouts():
    """name -> list of (slot, member, poison or None)"""
    out = {}
    for kind, (s, m) in POISONED.items():
        nb = [(a, c, None) for a, c in NEIGHBOURS]
        out[f"{kind}_first"] = [(s, m, kind)] + nb
        out[f"{kind}_last"] = nb + [(s, m, kind)]
    sixteen = [(t % tgb.P, 0 if t % 3 else t % tgb.P, None) for t in range(16)]
    for t, kind in ((0, "A_zero"), (7, "x0_inf"), (15, "A_nan")):
        sixteen[t] = POISONED[kind] + (kind,)
    out["three_of_16"] = sixteen
    return out


LAYOUTS = _layouts()


@pytest.mark.parametrize("chunk", [8, 0])
def test_non_finite_inside_the_loop(pkg, ctx, fem, monkeypatch, chunk):
    """A slot with one NaN entry, an all-zero slot (p'Ap = 0) and +Inf in X0: the system stops at its own count, by one decrement of
    `active`; were it two, the host would stop the neighbours before their counts"""
    api = pkg.api
    W = make_world(pkg, ctx, fem, "N34")
    W.env(monkeypatch)
    n = W.n
    r = np.random.default_rng(4).standard_normal(n)
    try:
        ctx.set_chunk(chunk)
        for name, layout in LAYOUTS.items():
            slots, members = [s for s, _, _ in layout], [m for _, m, _ in layout]
            B = np.asfortranarray(np.column_stack([W.bs[s] for s in slots]))
            X0 = np.zeros_like(B)
            cslots, cmembers = list(slots), list(members)
            poisoned = [t for t, (_, _, kind) in enumerate(layout) if kind]
            for t in poisoned:
                X0[:, t] = blc.poison_x0(X0[:, t], layout[t][2])
                cslots[t], cmembers[t] = CLEAN_FOR
            Bc = np.asfortranarray(np.column_stack([W.bs[s] for s in cslots]))
            Xc = np.zeros_like(Bc)
            clean = api.pcg_batch(W.batch, cslots, Bc, Xc, W.view, cmembers)
            W.view.combine([1, 4], [0.25, 0.75])             # the view's own selection, of two terms
            z_before = W.view.ldiv(r)
            got = api.pcg_batch(W.batch, slots, B, X0, W.view, members)
            assert same(W.view.ldiv(r), z_before) and list(W.view.members) == [1, 4], f"{name}: the view's own selection changed"
            again = api.pcg_batch(W.batch, cslots, Bc, Xc, W.view, cmembers)
            assert same_batch(again, clean), f"{name}: the clean batch after the poisoned one differs from the one before"
            assert same(W.view.ldiv(r), z_before)
            W.check(cslots, cmembers, Bc, Xc, clean, tag=f"{name}, clean")
            its = W.check(slots, members, B, X0, got, tag=name)          # BITS, the poisoned systems under equal_nan
            for t in range(len(layout)):
                if t in poisoned:
                    assert got[1][t] <= 3, f"{name}: the poisoned system {t} ran to it = {got[1][t]}"
                    assert not (np.isfinite(got[2][t]).all() and np.isfinite(got[0][:, t]).all()), f"{name}: system {t} carries no NaN or Inf"
                else:
                    assert got[1][t] == clean[1][t], f"{name}: neighbour {t} stopped at {got[1][t]}, in the clean batch at {clean[1][t]}"
                    assert same(got[0][:, t], clean[0][:, t]) and same(got[2][t], clean[2][t]), f"{name}: neighbour {t} differs from the clean batch"
            rest = [its[t] for t in range(len(layout)) if t not in poisoned]
            assert max(rest) >= max(its[t] for t in poisoned) + 50, f"{name}: no neighbour runs 50 iterations past the poisoned stop: {its}"
            print(f"chunk {chunk}, {name}: it = {its}")
    finally:
        ctx.set_chunk(8)


# ------------------------------------------------------------------ 5. eviction
def test_eviction_of_the_shared_graph_map(pkg, ctx, fem, monkeypatch):
    """The prediction follows the last solve (its count less one), so the sweep runs downwards: maxit = 50 meets a predicted length
    near 300, every later maxit = m the prediction m left by the batch of maxit = m + 1, and `first` = maxit each time: 50 set-up
    graphs of the batch, and the separate solves' own between them, in the one map of this size. (Upwards, the prediction 1 left
    by maxit = 1 would serve every later batch with the graph of one iteration.)"""
    api = pkg.api
    W = make_world(pkg, ctx, fem, "lap301")
    W.env(monkeypatch)
    _, b, _ = blc.lap301()
    n = W.n
    B = np.asfortranarray(np.column_stack([b, b]))
    X0 = np.zeros_like(B)
    full = api.pcg_batch(W.batch, [0, 1], B, X0, None)
    W.check([0, 1], None, B, X0, full, tag="before the sweep")
    assert max(full[1]) > 64 + 50
    single = api.cg(W.operator(0), b, np.zeros(n))
    grew = 0
    for m in range(50, 0, -1):
        c0 = ctx.query("graph_captures")
        got = api.pcg_batch(W.batch, [0, 1], B, X0, None, maxit=m)
        grew += ctx.query("graph_captures") - c0
        its = W.check([0, 1], None, B, X0, got, maxit=m, tag=f"maxit = {m}")       # the separate solves capture between the batches
        assert its == [m, m]
    print(f"lap301: the batch captured {grew} graphs in the sweep")
    assert grew >= blc.GRAPH_CAP + 1
    last = api.pcg_batch(W.batch, [0, 1], B, X0, None)
    assert same_batch(last, full), "the default batch after the sweep differs from the one before"
    x, it, res = api.cg(W.operator(0), b, np.zeros(n))
    assert it == single[1] and same(x, single[0]) and same(res, single[2]), "the separate cg after the sweep differs from the one before"
