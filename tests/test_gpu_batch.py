"""GPU suite of the batched device PCG (`api.CsrBatch`, `api.pcg_batch`, `FullAssemblyPlan.update_batch`; csrc/csr_batch.hpp,
csrc/batch_solvers.hpp, `AmgBankView::apply_batch`): k realizations in one Krylov loop, system t as the grid's second dimension.

The bar is bit for bit (`np.array_equal`) against the device's own separate solves: for system t that is
`api.pcg(SparseMatrixCSC(ctx, A_t), b_t, x0_t, view.select(m_t))` in the multi-workgroup (GENERIC) form of the loop, whose
arithmetic and order the batched kernels repeat. For n <= 8192 the separate solve runs under MI355_NO_FUSED=1 (beyond, GENERIC
is the default); `api.cg`, the reference of `M = None`, also under MI355_NO_CSRFOLD=1, which is what keeps a cg on a sparse
matrix in that form. x, it and res_norm[:it] must all be equal; no tolerance anywhere.

Systems: the Example01 flow on the N x N mesh with lognormal coefficients of the seeds 481456 + p (as `mesh_members` of
test_gpu_amg_bank.py), and the tridiagonal chains of tests/amg_setup_synth.py with 1, 7, 8, 9 and 17 row blocks and an ODD count
of stored entries, so that an unpadded slot would start every second matrix at an odd offset."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import amg_setup_synth as asy
import amg_synth as ays
from conftest import f_m1, lognormal_coeff, u3

pytestmark = pytest.mark.gpu

MESH = {"N34": (34, {}), "N35": (35, {}), "N93": (93, {}), "N12_1": (12, dict(max_levels=1))}
CHAIN_BLOCKS = (1, 7, 8, 9, 17)
CASES = tuple(MESH) + tuple(f"chain_{k}" for k in CHAIN_BLOCKS)
P = 6                       # systems (and bank members) of every case
CAPACITY = 8                # slots of every batch

_worlds = {}


def chain_length(k):
    """an odd number of rows whose tridiagonal has k row blocks: 3 n - 2 stored entries, an odd count"""
    n = ays.blocks_len(k)
    return n if n & 1 else n + 1


def systems(fem, name):
    """(matrices in sorted CSR on one pattern, right-hand sides, aggregates)"""
    if name in MESH:
        N, kw = MESH[name]
        mesh = fem.get_mesh(N)
        d = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
        mats, bs = [], []
        for p in range(P):
            a = lognormal_coeff(fem, mesh.points, 481456 + p)
            A, b = fem.do_isotropic_elliptic_assembly(mesh.cells, mesh.points, d, mesh.point_marker, a, f_m1, u3)
            A = sp.csr_matrix(A)
            A.sum_duplicates(); A.sort_indices()
            assert not mats or (np.array_equal(A.indptr, mats[0].indptr) and np.array_equal(A.indices, mats[0].indices))
            mats.append(A); bs.append(np.asarray(b, dtype=np.float64))
        H = fem.prepare_amg_precond(mats[0], **kw)
        return mats, bs, [np.asarray(a, dtype=np.int64) for a in H.agg]
    k = int(name[6:])
    n = chain_length(k)
    S = asy.chain(n)
    assert ays.row_blocks(S.indptr).shape[0] == k and S.indices.size % 2 == 1, (k, n)
    rng = np.random.default_rng([77, k])
    return [asy.spd_values(S, [51 + p, k]) for p in range(P)], [rng.standard_normal(n) for _ in range(P)], asy.chain_levels(n, 8, 200)


class World:
    """One case on the device: P matrices in the slots 0 .. P - 1 of a batch, P members of a bank, a view of 16 terms, one
    CsrOperator that is refreshed in place for the separate solves, and the separate solves already made."""

    def __init__(self, api, ctx, fem, name):
        self.api, self.ctx, self.name = api, ctx, name
        self.mats, self.bs, self.aggs = systems(fem, name)
        self.n = self.mats[0].shape[0]
        self.bank = api.AMGBank(ctx, self.mats[0], P, aggregates=self.aggs)
        self.batch = api.CsrBatch(ctx, self.mats[0], CAPACITY)
        for p, A in enumerate(self.mats):
            self.bank.set_values(p, A)
            self.batch.set_values(p, A)
        self.view = self.bank.view(16)
        self.A_op = api.SparseMatrixCSC(ctx, self.mats[0])
        self.in_op = 0
        self.refs = {}

    def env(self, monkeypatch):
        """the separate solves take the multi-workgroup form"""
        if self.n <= 8192:
            monkeypatch.setenv("MI355_NO_FUSED", "1")
        monkeypatch.setenv("MI355_NO_CSRFOLD", "1")

    def separate(self, slot, member, b, x0, maxit=0):
        """(x, it, res_norm) of the separate solve; member None: cg. `env` must be in force."""
        key = (slot, member, b.tobytes(), x0.tobytes(), maxit)
        if key not in self.refs:
            if self.in_op != slot:
                self.A_op.set_values(self.mats[slot])
                self.in_op = slot
            if member is None:
                self.refs[key] = self.api.cg(self.A_op, b, x0, maxit=maxit)
            else:
                self.view.select(member)
                self.refs[key] = self.api.pcg(self.A_op, b, x0, self.view, maxit=maxit)
        return self.refs[key]

    def check(self, slots, members, B, X0, got, maxit=0, tag=""):
        X, its, res = got
        X = X.cpu().numpy() if hasattr(X, "cpu") else X
        want_its = []
        for t, s in enumerate(slots):
            m = None if members is None else members[t]
            x, it, rn = self.separate(s, m, np.ascontiguousarray(B[:, t]), np.ascontiguousarray(X0[:, t]), maxit)
            want_its.append(it)
            where = f"{self.name} {tag}: system {t} (slot {s}, member {m})"
            assert its[t] == it, f"{where}: it = {its[t]}, the separate solve {it}"
            assert np.array_equal(res[t], rn, equal_nan=True), f"{where}: res_norm differs"
            assert np.array_equal(X[:, t], x, equal_nan=True), f"{where}: x differs"
        return want_its

    def close(self):
        self.view.close(); self.A_op.close(); self.batch.close(); self.bank.close()


def world(pkg, ctx, fem, name) -> World:
    if name not in _worlds:
        _worlds[name] = World(pkg.api, ctx, fem, name)
    return _worlds[name]


@pytest.fixture(scope="module", autouse=True)
def _close_worlds():
    yield
    for w in _worlds.values():
        w.close()
    _worlds.clear()


def columns(W, slots, zero_x0=True, seed=3):
    """B (the systems' own right-hand sides) and X0 as Fortran arrays"""
    rng = np.random.default_rng(seed)
    B = np.asfortranarray(np.column_stack([W.bs[s] for s in slots]))
    X0 = np.zeros_like(B) if zero_x0 else np.asfortranarray(rng.standard_normal(B.shape))
    return B, X0


# ------------------------------------------------------------------ 1. sizes at the kernels' edges
@pytest.mark.parametrize("name", CASES)
def test_sizes_at_the_kernel_edges(pkg, ctx, fem, monkeypatch, name):
    """N = 34: n = 1024, one vector workgroup; N = 35: n = 1089, two; N = 93: n = 8281 > FUSED_MAX_N, 3 levels; the chains: 1, 7, 8, 9,
    17 row blocks (the SpMV's grid rounds to 8) and an odd nnz; N12_1: a coarse-only cycle"""
    W = world(pkg, ctx, fem, name)
    W.env(monkeypatch)
    if name == "N34":
        assert W.n == 1024
    if name == "N35":
        assert W.n == 1089
    if name == "N93":
        assert W.n == 8281 and W.bank.n_levels == 3
    if name == "N12_1":
        assert W.bank.n_levels == 1
    if name.startswith("chain_"):
        st = W.batch.stats()
        assert W.batch.nnz % 2 == 1 and st["bytes_per_slot"] == 8 * (W.batch.nnz + 1) == pkg.api.csr_batch_slot_bytes(W.batch.nnz)
    slots, members = [0, 1, 2], [0, 1, 2]
    B, X0 = columns(W, slots)
    got = pkg.api.pcg_batch(W.batch, slots, B, X0, W.view, members)
    its = W.check(slots, members, B, X0, got)
    print(f"{name}: n = {W.n}, it = {its}")
    rng = np.random.default_rng(8)
    Br, Xr = np.asfortranarray(rng.standard_normal((W.n, 2))), np.asfortranarray(rng.standard_normal((W.n, 2)))
    W.check([4, 5], [5, 4], Br, Xr, pkg.api.pcg_batch(W.batch, [4, 5], Br, Xr, W.view, [5, 4]), tag="random b, x0")


# ------------------------------------------------------------------ 2. batch shapes
def test_batch_shapes(pkg, ctx, fem, monkeypatch):
    api = pkg.api
    W = world(pkg, ctx, fem, "N34")
    W.env(monkeypatch)
    rng = np.random.default_rng(21)
    shapes = {
        "k = 1": ([2], [2]),
        "k = 16": ([t % P for t in range(16)], [(t * 5) % P for t in range(16)]),
        "k = 3 on a view of 16": ([0, 1, 2], [0, 1, 2]),
        "slots out of order": ([3, 0, 2], [3, 0, 2]),
        "one slot twice": ([1, 1], [1, 1]),
        "one member for all": ([0, 1, 2, 3], [0, 0, 0, 0]),
    }
    for tag, (slots, members) in shapes.items():
        B, X0 = columns(W, slots)
        if tag in ("one slot twice", "k = 16"):          # several right-hand sides for one matrix
            B = np.asfortranarray(B + 0.25 * rng.standard_normal(B.shape))
        its = W.check(slots, members, B, X0, api.pcg_batch(W.batch, slots, B, X0, W.view, members), tag=tag)
        print(f"{tag}: it = {its}")
    small = W.bank.view(3)                                # k = max_terms of a small view
    try:
        B, X0 = columns(W, [2, 1, 0])
        W.check([2, 1, 0], [0, 1, 2], B, X0, api.pcg_batch(W.batch, [2, 1, 0], B, X0, small, [0, 1, 2]), tag="view of 3")
    finally:
        small.close()


# ------------------------------------------------------------------ 3. different stopping iterations inside one batch
@pytest.mark.parametrize("name", ["N34", "N35", "N93"])
def test_systems_stop_at_different_iterations(pkg, ctx, fem, monkeypatch, name):
    """Systems under their own member (it = 7 .. 11) beside systems 1 .. 5 under the stale member 0 (53 .. 125 by the numpy
    restatement) and one system with b = 0, which stops at it = 1: every system freezes at its own count"""
    W = world(pkg, ctx, fem, name)
    W.env(monkeypatch)
    slots = [0, 1, 1, 2, 3, 4, 5, 2, 3]
    members = [0, 1, 0, 0, 0, 0, 0, 2, 3]
    B, X0 = columns(W, slots)
    B[:, 8] = 0.0
    its = [W.separate(s, m, np.ascontiguousarray(B[:, t]), np.ascontiguousarray(X0[:, t]))[1] for t, (s, m) in enumerate(zip(slots, members))]
    print(f"{name}: the separate solves' it = {its}")
    assert len(set(its)) > 1, "every system stops at the same iteration: nothing to freeze"
    assert its[8] == 1 and max(its) > 4 * min(its[:8])
    got = pkg.api.pcg_batch(W.batch, slots, B, X0, W.view, members)
    W.check(slots, members, B, X0, got)
    assert got[1][8] == 1 and np.array_equal(got[0][:, 8], np.zeros(W.n))


# ------------------------------------------------------------------ 4. mixed and limiting arguments
def test_mixed_and_limiting_arguments(pkg, ctx, fem, monkeypatch):
    import torch
    api = pkg.api
    W = world(pkg, ctx, fem, "N35")
    W.env(monkeypatch)
    n = W.n
    slots, members = [0, 1, 2, 3], [0, 1, 0, 3]
    B, X0 = columns(W, slots, zero_x0=False)
    X0[:, 0] = 0.0; X0[:, 2] = 0.0                           # zero for some systems, random for others
    for maxit in (1, 2, 0):
        got = api.pcg_batch(W.batch, slots, B, X0, W.view, members, maxit=maxit)
        its = W.check(slots, members, B, X0, got, maxit=maxit, tag=f"maxit = {maxit}")
        if maxit == 1:
            assert its == [1] * 4 and np.array_equal(got[0], X0)
        if maxit == 2:
            assert its == [2] * 4
    try:
        ctx.set_chunk(1)
        W.check(slots, members, B, X0, api.pcg_batch(W.batch, slots, B, X0, W.view, members), tag="chunk 1")
        ctx.set_chunk(0)
        W.check(slots, members, B, X0, api.pcg_batch(W.batch, slots, B, X0, W.view, members), tag="eager")
    finally:
        ctx.set_chunk(8)
    # leading dimensions above n, host arrays
    ld = n + 7
    Bw, Xw = np.full((ld, 4), np.nan, order="F"), np.full((ld, 4), np.nan, order="F")
    Bw[:n], Xw[:n] = B, X0
    lib, L = pkg._lib.load(), pkg._lib
    api.check(lib.mi_ctx_set_pointer_mode(ctx._h, L.MI_PTR_HOST))
    sl, mem = np.array(slots, dtype=np.int64), np.array(members, dtype=np.int64)
    ldres = n + 3
    res, it = np.full((ldres, 4), -1.0, order="F"), np.zeros(4, dtype=np.int64)
    api.check(lib.mi_pcg_batch(W.batch._h, 4, sl.ctypes.data_as(L.i64p), W.view._h, mem.ctypes.data_as(L.i64p), C.c_void_p(Bw.ctypes.data), ld,
                               C.c_void_p(Xw.ctypes.data), ld, 0, 1e-7, res.ctypes.data_as(L.f64p), ldres, it.ctypes.data_as(L.i64p)))
    assert np.all(np.isnan(Xw[n:])) and np.all(np.isnan(Bw[n:])), "rows beyond n were touched"
    W.check(slots, members, B, X0, (Xw[:n], it, [res[:it[t], t] for t in range(4)]), tag="ld > n")
    assert all(np.all(res[it[t]:, t] == -1.0) for t in range(4)), "res_norm beyond it was touched"
    # the same through views of larger arrays in the Python layer
    W.check(slots, members, B, X0, api.pcg_batch(W.batch, slots, Bw[:n], Xw[:n] * 0 + X0, W.view, members), tag="numpy view")
    # device tensors (column-major, column stride above n): X0 is mutated in place
    Bd = torch.full((4, ld), float("nan"), dtype=torch.float64, device="cuda")
    Xd = torch.full((4, ld), float("nan"), dtype=torch.float64, device="cuda")
    Bd[:, :n] = torch.from_numpy(np.ascontiguousarray(B.T)).cuda()
    Xd[:, :n] = torch.from_numpy(np.ascontiguousarray(X0.T)).cuda()
    got = api.pcg_batch(W.batch, slots, Bd.T[:n], Xd.T[:n], W.view, members)
    ctx.synchronize()
    assert got[0].data_ptr() == Xd.data_ptr() and bool(torch.isnan(Xd[:, n:]).all())
    W.check(slots, members, B, X0, got, tag="device tensors")
    # M = None: cg's recurrences
    for maxit in (0, 3):
        got = api.pcg_batch(W.batch, slots, B, X0, None, maxit=maxit)
        its = W.check(slots, None, B, X0, got, maxit=maxit, tag=f"cg, maxit = {maxit}")
    print(f"cg: it = {its}")


# ------------------------------------------------------------------ 5. isolation
def test_isolation(pkg, ctx, fem, monkeypatch):
    api = pkg.api
    W = world(pkg, ctx, fem, "N34")
    W.env(monkeypatch)
    slots, members = [0, 1, 2, 3], [0, 1, 0, 3]
    B, X0 = columns(W, slots)
    r = np.random.default_rng(4).standard_normal(W.n)
    W.view.combine([1, 4], [0.25, 0.75])                     # the view's own selection, of two terms
    z_before = W.view.ldiv(r)
    first = api.pcg_batch(W.batch, slots, B, X0, W.view, members)
    assert np.array_equal(W.view.ldiv(r), z_before), "a batched solve changed the view's own selection"
    assert list(W.view.members) == [1, 4]
    W.check(slots, members, B, X0, first)
    Bn = B.copy(order="F")
    Bn[W.n // 2, 1] = np.nan
    got = api.pcg_batch(W.batch, slots, Bn, X0, W.view, members)
    assert got[1][1] == 1 and len(got[2][1]) == 1 and np.isnan(got[2][1][0]), "the NaN system ends as the single solve does"
    W.check(slots, members, Bn, X0, got, tag="NaN in b of system 1")
    for t in (0, 2, 3):
        assert np.array_equal(got[0][:, t], first[0][:, t]) and got[1][t] == first[1][t] and np.array_equal(got[2][t], first[2][t])
    W.view.combine([1, 4], [0.25, 0.75])                     # (the separate solves of `check` select)
    again = api.pcg_batch(W.batch, slots, B, X0, W.view, members)
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])
    assert all(np.array_equal(u, v) for u, v in zip(again[2], first[2])), "the batch after the NaN one differs from the one before"
    assert np.array_equal(W.view.ldiv(r), z_before)


# ------------------------------------------------------------------ 6. one graph serves every selection
def test_one_graph_serves_every_selection(pkg, ctx, fem, monkeypatch):
    """The first solve on a (batch, view) captures the set-up graph of the default length and the chunk graph; the second one the
    set-up graph of the predicted length (the replay policy of the single solvers). From then on a permutation of the (slot,
    member) pairs, and a sub-batch that keeps the longest system, replay what is there."""
    api = pkg.api
    W = world(pkg, ctx, fem, "N34")
    W.env(monkeypatch)
    view = W.bank.view(16)                                   # a view of its own: no graph of another test
    try:
        slots, members = [0, 1, 2, 3, 5], [0, 0, 2, 0, 5]
        B, X0 = columns(W, slots)
        c0 = ctx.query("graph_captures")
        its = W.check(slots, members, B, X0, api.pcg_batch(W.batch, slots, B, X0, view, members))
        c1 = ctx.query("graph_captures")
        W.check(slots, members, B, X0, api.pcg_batch(W.batch, slots, B, X0, view, members))
        c2, r2 = ctx.query("graph_captures"), ctx.query("graph_replays")
        print(f"it = {its}; graph captures {c0} -> {c1} -> {c2}")
        assert c1 > c0 and c2 - c1 <= 1
        perm = [3, 0, 4, 2, 1]
        ps, pm = [slots[i] for i in perm], [members[i] for i in perm]
        Bp, Xp = np.asfortranarray(B[:, perm]), np.asfortranarray(X0[:, perm])
        W.check(ps, pm, Bp, Xp, api.pcg_batch(W.batch, ps, Bp, Xp, view, pm), tag="permutation")
        longest = int(np.argmax(its))
        keep = sorted({longest, 0, 2})
        ss, sm = [slots[i] for i in keep], [members[i] for i in keep]
        Bs, Xs = np.asfortranarray(B[:, keep]), np.asfortranarray(X0[:, keep])
        W.check(ss, sm, Bs, Xs, api.pcg_batch(W.batch, ss, Bs, Xs, view, sm), tag="sub-batch")
        assert ctx.query("graph_captures") == c2, "a later selection captured a graph again"
        assert ctx.query("graph_replays") > r2
    finally:
        view.close()
    # destroying the view dropped its graphs: a new view on the same batch captures its own and still matches
    view2 = W.bank.view(16)
    try:
        c3 = ctx.query("graph_captures")
        W.check(slots, members, B, X0, api.pcg_batch(W.batch, slots, B, X0, view2, members), tag="new view")
        assert ctx.query("graph_captures") > c3
    finally:
        view2.close()


# ------------------------------------------------------------------ 7. update_batch
def test_update_batch_writes_one_slot(pkg, ctx, fem):
    import full_assembly_cases as cases
    import torch
    api = pkg.api
    mesh = fem.get_mesh(34)
    plan = cases.make_plan(fem, mesh, f_m1, u3)
    dev = api.FullAssemblyPlan(ctx, plan)
    coeffs = [lognormal_coeff(fem, mesh.points, 481456 + p) for p in range(3)]
    pattern = sp.csr_matrix((np.ones(plan.nnz), plan.colidx, plan.rowptr), shape=(plan.n, plan.n))
    batch = api.CsrBatch(ctx, pattern, 5)
    other = api.CsrBatch(ctx, sp.identity(plan.n, format="csr"), 2)
    try:
        marks = [np.full(plan.nnz, float(s + 1)) for s in range(5)]
        for s in range(5):
            batch.set_values(s, marks[s])
        for p, s in ((0, 2), (1, 1), (2, 3)):
            vals, b = dev.run(coeffs[p])
            bb = dev.update_batch(coeffs[p], batch, s)
            assert cases.same_bits(bb, b) and cases.same_bits(batch.get_values(s), vals), (p, s)
            marks[s] = vals
            for q in (s - 1, s + 1):
                assert cases.same_bits(batch.get_values(q), marks[q]), f"slot {q} changed when slot {s} was written"
        bt = dev.update_batch(torch.from_numpy(coeffs[0]).cuda(), batch, 0)     # a device coefficient: no host copy
        ctx.synchronize()
        vals, b = dev.run(coeffs[0])
        assert bt.is_cuda and cases.same_bits(bt.cpu().numpy(), b) and cases.same_bits(batch.get_values(0), vals)
        assert batch.stats() == dict(capacity=5, slots_set=5, bytes_shared=batch.stats()["bytes_shared"], bytes_per_slot=api.csr_batch_slot_bytes(plan.nnz))
        with pytest.raises(api.MiError, match="stored entries"):
            dev.update_batch(coeffs[0], other, 0)
        with pytest.raises(api.MiError, match="slot = 5"):
            dev.update_batch(coeffs[0], batch, 5)
        A_op = api.SparseMatrixCSC(ctx, pattern)
        with pytest.raises(api.MiError, match="not a batch"):
            dev.update_batch(coeffs[0], A_op, 0)
        A_op.close()
    finally:
        batch.close(); other.close(); dev.close()


def test_update_batch_refuses_another_pattern(pkg, ctx, fem):
    """the same n and nnz, another pattern: found by the full comparison of the first meeting"""
    import full_assembly_cases as cases
    api = pkg.api
    mesh = fem.get_mesh(12)
    plan = cases.make_plan(fem, mesh, f_m1, u3)
    dev = api.FullAssemblyPlan(ctx, plan)
    S = sp.csr_matrix((np.ones(plan.nnz), plan.colidx, plan.rowptr), shape=(plan.n, plan.n)).tolil()
    i = next(r for r in range(plan.n) if S[r, (r + plan.n // 2) % plan.n] == 0 and S[r].nnz > 1)
    j = [c for c in S.rows[i] if c != i][0]
    S[i, j] = 0; S[i, (i + plan.n // 2) % plan.n] = 1
    S = sp.csr_matrix(S); S.eliminate_zeros(); S.sort_indices()
    assert S.nnz == plan.nnz
    batch = api.CsrBatch(ctx, S, 1)
    try:
        with pytest.raises(api.MiError, match="pattern"):
            dev.update_batch(np.ones(plan.n_node), batch, 0)
        assert batch.stats()["slots_set"] == 0
    finally:
        batch.close(); dev.close()


# ------------------------------------------------------------------ 8. refusals
def test_refusals(pkg, ctx, fem):
    api, L = pkg.api, pkg._lib
    lib = L.load()
    W = world(pkg, ctx, fem, "N34")
    n = W.n
    i64p, f64p = L.i64p, L.f64p
    api.check(lib.mi_ctx_set_pointer_mode(ctx._h, L.MI_PTR_HOST))

    def refused(rc, *words, code=L.MI_ERR_BAD_ARG):
        msg = lib.mi_last_error().decode()
        print("  refused:", msg)
        assert rc == code and len(msg) > 30 and all(w in msg for w in words), (rc, msg, words)

    arr = lambda *m: np.array(m, dtype=np.int64)
    B, X = np.asfortranarray(np.column_stack([W.bs[0]] * 16)), np.zeros((n, 16), order="F")
    res, it = np.zeros((n + 1, 16), order="F"), np.zeros(16, dtype=np.int64)

    def solve(A=W.batch._h, k=2, slots=arr(0, 1), M=W.view._h, members=arr(0, 1), ldb=n, ldx=n, ldres=n + 1, maxit=0):
        X[:] = 0.0                                           # X is the initial guess on entry
        it[:] = 0
        return lib.mi_pcg_batch(A, k, slots.ctypes.data_as(i64p), M, members.ctypes.data_as(i64p), C.c_void_p(B.ctypes.data), ldb,
                                C.c_void_p(X.ctypes.data), ldx, maxit, 1e-7, res.ctypes.data_as(f64p), ldres, it.ctypes.data_as(i64p))

    assert solve() == 0
    x_ok, it_ok = X[:, :2].copy(), it[:2].copy()
    refused(solve(k=0), "k = 0")
    refused(solve(k=17), "k = 17", "16")
    small = W.bank.view(2)
    refused(solve(k=3, slots=arr(0, 1, 2), M=small._h, members=arr(0, 1, 2)), "k = 3", "max_terms = 2")
    small.close()
    refused(solve(slots=arr(0, CAPACITY)), f"slot = {CAPACITY}", f"0 .. {CAPACITY - 1}")
    refused(solve(slots=arr(-1, 0)), "slot = -1")
    refused(solve(slots=arr(0, P)), f"slot {P}", "never set")
    refused(solve(members=arr(0, P)), f"member = {P}")
    refused(solve(ldb=n - 1), f"ldb = {n - 1}", f"n = {n}")
    refused(solve(ldx=n - 1), f"ldx = {n - 1}")
    refused(solve(A=W.A_op._h), "not a batch of sparse matrices")
    refused(solve(A=W.view._h), "not a batch of sparse matrices", "view")
    refused(solve(A=None), "NULL")
    refused(solve(M=W.A_op._h), "not a view of an AMG bank")
    refused(solve(M=W.bank._h), "not a view of an AMG bank", "AMG bank")
    refused(solve(M=W.batch._h), "not a view of an AMG bank", "batch")
    # an unset member
    bank2 = api.AMGBank(ctx, W.mats[0], 3, aggregates=W.aggs)
    bank2.set_values(0, W.mats[0])
    v2 = bank2.view(4)
    refused(solve(M=v2._h, members=arr(0, 2)), "member 2", "never set")
    v2.close(); bank2.close()
    # A and M of different size, and of different contexts
    Wo = world(pkg, ctx, fem, "N12_1")
    refused(solve(M=Wo.view._h), "differ in size or context", str(n), str(Wo.n))
    ctx2 = api.Context(0)
    bank3 = api.AMGBank(ctx2, W.mats[0], 1, aggregates=W.aggs)
    bank3.set_values(0, W.mats[0])
    v3 = bank3.view(2)
    refused(solve(M=v3._h, members=arr(0, 0)), "differ in size or context")
    v3.close(); bank3.close(); ctx2.close()
    # a context that is one rank of several
    grp = api.LoopbackGroup(2)
    grp.set_mode(1)
    rank0 = api.Context(0)
    rank0.loopback_init(grp, 0)
    b0 = api.CsrBatch(rank0, W.mats[0], 1)
    b0.set_values(0, W.mats[0])
    api.check(lib.mi_ctx_set_pointer_mode(rank0._h, L.MI_PTR_HOST))
    refused(solve(A=b0._h, k=1, slots=arr(0), M=None), "rank 0 of 2")
    b0.close(); rank0.close()
    api.check(lib.mi_ctx_set_pointer_mode(ctx._h, L.MI_PTR_HOST))
    # the refusals changed nothing; the capacity of res_norm comes after the solve, with it filled and X valid
    assert solve() == 0 and np.array_equal(X[:, :2], x_ok) and np.array_equal(it[:2], it_ok)
    refused(solve(ldres=3), "ldres = 3", code=L.MI_ERR_RES_CAPACITY)
    assert np.array_equal(it[:2], it_ok) and np.array_equal(X[:, :2], x_ok) and it_ok.min() > 3
    with pytest.raises(api.BoundsError) as e:
        api.pcg_batch(W.batch, [0, 1], B[:, :2], X[:, :2] * 0, W.view, [0, 1], ldres=3)
    assert np.array_equal(e.value.its, it_ok) and np.array_equal(e.value.X, x_ok)
    # the batch is no operator
    x, y = np.ones(n), np.zeros(n)
    xp, yp = C.c_void_p(x.ctypes.data), C.c_void_p(y.ctypes.data)
    one_it, r1 = C.c_int64(), np.zeros(n + 1)
    refused(lib.mi_op_apply(W.batch._h, xp, yp), "batch of sparse matrices", "mi_pcg_batch")
    refused(lib.mi_pcg(W.batch._h, W.view._h, xp, yp, 0, 1e-7, r1.ctypes.data_as(f64p), n + 1, C.byref(one_it)), "batch of sparse matrices")
    refused(lib.mi_pcg(W.A_op._h, W.batch._h, xp, yp, 0, 1e-7, r1.ctypes.data_as(f64p), n + 1, C.byref(one_it)), "batch of sparse matrices")
    refused(lib.mi_cg(W.batch._h, xp, yp, 0, 1e-7, r1.ctypes.data_as(f64p), n + 1, C.byref(one_it)), "batch of sparse matrices")
    kids = (C.c_void_p * 1)(W.batch._h)
    comb = C.c_void_p()
    refused(lib.mi_op_combine(ctx._h, 1, kids, np.ones(1).ctypes.data_as(f64p), C.byref(comb)), "batch of sparse matrices")
    size = C.c_int64()
    api.check(lib.mi_op_size(W.batch._h, C.byref(size)))
    assert size.value == n
    # slots
    vptr = C.c_void_p(np.ascontiguousarray(W.mats[0].data).ctypes.data)
    refused(lib.mi_csr_batch_set_values(W.batch._h, CAPACITY, vptr), f"slot = {CAPACITY}")
    refused(lib.mi_csr_batch_set_values(W.A_op._h, 0, vptr), "not a batch")
    refused(lib.mi_csr_batch_get_values(W.batch._h, P + 1, vptr), f"slot {P + 1}", "never set")
    refused(lib.mi_csr_batch_stats(W.view._h, None, None, None, None), "not a batch", "view")
    with pytest.raises(IndexError):
        W.batch.set_values(CAPACITY, W.mats[0])
    with pytest.raises(ValueError, match="stored entries"):
        W.batch.set_values(0, W.mats[0].data[:-1])
    with pytest.raises(ValueError, match="members"):
        api.pcg_batch(W.batch, [0, 1], B[:, :2], X[:, :2], W.view, [0])
    assert solve() == 0 and np.array_equal(X[:, :2], x_ok)
