"""GPU suite of the device AMG bank (`api.AMGBank`, `api.AMGBankView`; csrc/amg_bank.hpp, `mi_amg_bank_*`): P hierarchies on
one plan, one set of index arrays and one set-up engine, a member being one slot of numbers; the view runs the V(1,1) cycles
of the k members it selects in one sequence of launches.

Every comparison is bit for bit (`np.array_equal`): a member against a separate
`AMGPreconditioner(ctx, A0, device_setup=True, aggregates=aggs)` after `.set_values(A_p)` — the hierarchy read back, the
apply, the solves — against `amg_synth.cycle_bits` of the hierarchy read back, and a k-member view against
`InterpolatingPreconditioner(coef, separate operators)`.

Cases: the N = 12 mesh with 1, 2 and 3 levels and the N = 34 mesh, members from seeded lognormal coefficients; the synthetic
pairs of tests/amg_setup_synth.py (A0, A1 as two members); tridiagonal chains whose level 0 has 1, 7, 8, 9 and 17 row blocks
and an ODD count of stored entries, so that an unpadded slot would start every second member at an odd offset."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import amg_setup_synth as asy
import amg_synth as ays
from conftest import f_m1, lognormal_coeff, u3

pytestmark = pytest.mark.gpu

MESH = {"N12_1": (12, dict(max_levels=1)), "N12_2": (12, dict(max_levels=2, max_coarse=10)), "N12_3": (12, dict(max_levels=3, max_coarse=4)),
        "N34": (34, {})}
MESH_LEVELS = {"N12_1": 1, "N12_2": 2, "N12_3": 3}
SYNTH = ("giant", "arrow_1025", "arrow_2049", "one_1", "one_65", "segments")
CHAIN_BLOCKS = (1, 7, 8, 9, 17)
CASES = tuple(MESH) + SYNTH + tuple(f"chain_{k}" for k in CHAIN_BLOCKS)

_mesh, _cases = {}, {}


def mesh_members(fem, N, count):
    """(matrices, right-hand sides): `count` systems of the Example01 flow on the N x N mesh, lognormal coefficients of the
    seeds 481456 + p, in sorted CSR on one pattern"""
    got = _mesh.setdefault(N, ([], []))
    mesh = fem.get_mesh(N)
    d = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
    while len(got[0]) < count:
        a = lognormal_coeff(fem, mesh.points, 481456 + len(got[0]))
        A, b = fem.do_isotropic_elliptic_assembly(mesh.cells, mesh.points, d, mesh.point_marker, a, f_m1, u3)
        A = sp.csr_matrix(A)
        A.sum_duplicates(); A.sort_indices()
        assert not got[0] or (np.array_equal(A.indptr, got[0][0].indptr) and np.array_equal(A.indices, got[0][0].indices))
        got[0].append(A); got[1].append(b)
    return got[0][:count], got[1][:count]


def chain_length(k):
    """an odd number of rows whose tridiagonal has k row blocks: 3 n - 2 stored entries, an odd count"""
    n = ays.blocks_len(k)
    return n if n & 1 else n + 1


def case(fem, name):
    """(member matrices, aggregates)"""
    if name in _cases:
        return _cases[name]
    if name in MESH:
        N, kw = MESH[name]
        mats = mesh_members(fem, N, 3)[0]
        H = fem.prepare_amg_precond(mats[0], **kw)
        assert name not in MESH_LEVELS or H.nlevels == MESH_LEVELS[name]
        out = (mats, [np.asarray(a, dtype=np.int64) for a in H.agg])
    elif name.startswith("chain_"):
        k = int(name[6:])
        n = chain_length(k)
        S = asy.chain(n)
        assert ays.row_blocks(S.indptr).shape[0] == k and S.indices.size % 2 == 1, (k, n)
        out = ([asy.spd_values(S, [41, k]), asy.spd_values(S, [42, k]), asy.spd_values(S, [43, k])], asy.chain_levels(n, 8, 200))
    else:
        A0, A1, aggs = asy.case(name, fem)
        out = ([A0, A1], list(aggs))
    _cases[name] = out
    return out


def rhs(n, seed=5):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n), np.eye(n)[n // 3]]


def separate(api, ctx, mats, aggs, p):
    M = api.AMGPreconditioner(ctx, mats[0], device_setup=True, aggregates=aggs)
    M.set_values(mats[p])
    return M


def same_solve(a, b):
    return a[1] == b[1] and all(np.array_equal(np.asarray(u), np.asarray(v)) for u, v in zip(a, b) if not np.isscalar(u))


# ------------------------------------------------------------------ 1. a member is the separate operator
@pytest.mark.parametrize("name", CASES)
def test_member_equals_the_separate_operator(pkg, ctx, fem, name):
    import torch
    api = pkg.api
    mats, aggs = case(fem, name)
    n = mats[0].shape[0]
    bank = api.AMGBank(ctx, mats[0], len(mats), aggregates=aggs)
    bank1 = api.AMGBank(ctx, mats[0], len(mats), index_base=1, aggregates=aggs)
    view, view1 = bank.view(), bank1.view()
    try:
        for p, A in enumerate(mats):
            bank.set_values(p, A)
            bank1.set_values(p, A.data)
        for p in range(len(mats)):
            M = separate(api, ctx, mats, aggs, p)
            try:
                H, Hs = bank.device_hierarchy(p), M.device_hierarchy()
                assert asy.same_hierarchy(H, Hs), f"{name}: member {p} differs from the separate operator"
                assert asy.same_hierarchy(bank1.device_hierarchy(p), Hs), f"{name}: member {p} of the 1-based bank"
                assert np.array_equal(H.A[0].data, mats[p].data)
                view.select(p); view1.select(p)
                for r in rhs(n):
                    z = view.ldiv(r)
                    assert np.array_equal(z, M.ldiv(r)), f"{name}: apply of member {p}"
                    assert np.array_equal(z, ays.cycle_bits(H, r)), f"{name}: member {p} against the restatement"
                    assert np.array_equal(view.ldiv(r), z), "a second apply differs"
                    zd = view.apply(torch.from_numpy(r).cuda())
                    assert np.array_equal(zd.cpu().numpy(), z), "the apply through a device pointer differs"
                    assert np.array_equal(view1.ldiv(r), z), "the bank of 1-based arrays differs"
            finally:
                M.close()
    finally:
        bank.close(); bank1.close()


# ------------------------------------------------------------------ 2. slots do not overlap
@pytest.mark.parametrize("name", ["chain_7", "N12_3"])
@pytest.mark.parametrize("capacity", [1, 5])
def test_slots_do_not_overlap(pkg, ctx, fem, name, capacity):
    """member 0, then the last member with other values: member 0 reads back what a separate operator holds for the values
    it was given last (capacity 1: the last member IS member 0), the members in between stay unset. A slot that overlapped
    its neighbour would show here; a slot that merely started at an odd offset would not (an 8-byte aligned 16-byte load
    gives the same bits), so the padding itself is held by the assertion on `bytes_per_member`: with the odd nnz(A_0) of
    the chain an unpadded stride is odd"""
    api = pkg.api
    mats, aggs = case(fem, name)
    n = mats[0].shape[0]
    r = rhs(n)[0]
    last = capacity - 1
    bank = api.AMGBank(ctx, mats[0], capacity, aggregates=aggs)
    view = bank.view()
    try:
        assert bank.stats()["bytes_per_member"] % 16 == 0
        bank.set_values(0, mats[1])
        H0, z0 = bank.device_hierarchy(0), view.ldiv(r)
        bank.set_values(last, mats[2])
        want = {0: 1, last: 2}          # member -> the matrix it holds
        for p, q in want.items():
            M = separate(api, ctx, mats, aggs, q)
            try:
                view.select(p)
                assert asy.same_hierarchy(bank.device_hierarchy(p), M.device_hierarchy()), (name, capacity, p)
                assert np.array_equal(view.ldiv(r), M.ldiv(r)), (name, capacity, p)
            finally:
                M.close()
        if capacity > 1:
            view.select(0)
            assert asy.same_hierarchy(bank.device_hierarchy(0), H0) and np.array_equal(view.ldiv(r), z0)
        for p in range(1, last):
            with pytest.raises(api.MiError, match="never set"):
                bank.device_hierarchy(p)
        assert bank.stats()["members_set"] == len(want)
    finally:
        bank.close()


# ------------------------------------------------------------------ 3. combination
COMBOS = [([3], [1.0]), ([3], [0.37]), ([0, 5], [0.25, 0.75]), ([5, 0], [0.75, 0.25]), ([2, 2], [0.5, 0.5]), ([1, 4, 7], [0.6, 0.0, 0.4]),
          ([6, 9], [1.5, -0.5]), (list(range(16)), None), (list(range(15, -1, -1)), None)]


@pytest.mark.parametrize("name", ["N12_3", "chain_1"])
def test_combination_equals_the_interpolating_preconditioner(pkg, ctx, fem, name):
    api = pkg.api
    if name == "N12_3":
        mats, aggs = mesh_members(fem, 12, 16)[0], case(fem, name)[1]
    else:
        n = chain_length(1)
        S = asy.chain(n)
        mats, aggs = [asy.spd_values(S, [44, p]) for p in range(16)], asy.chain_levels(n, 8, 200)
    n = mats[0].shape[0]
    bank = api.AMGBank(ctx, mats[0], 16, aggregates=aggs)
    view = bank.view(16)
    small = bank.view(2)
    ops = [separate(api, ctx, mats, aggs, p) for p in range(16)]
    try:
        for p, A in enumerate(mats):
            bank.set_values(p, A)
        rng = np.random.default_rng(9)
        for members, coef in COMBOS:
            coef = rng.standard_normal(len(members)) if coef is None else np.asarray(coef)
            Pi = api.InterpolatingPreconditioner(ctx, coef, [ops[p] for p in members])
            try:
                view.combine(members, coef)
                for r in rhs(n):
                    assert np.array_equal(view.ldiv(r), Pi.ldiv(r)), (name, members)
                if len(members) <= 2:
                    small.combine(members, coef)
                    assert np.array_equal(small.ldiv(rhs(n)[0]), Pi.ldiv(rhs(n)[0])), (name, members, "max_terms = 2")
            finally:
                Pi.close()
    finally:
        for M in ops:
            M.close()
        bank.close()


# ------------------------------------------------------------------ 4. solves
def test_solves_and_graphs(pkg, ctx, fem):
    api = pkg.api
    mats, bs = mesh_members(fem, 34, 3)
    aggs = case(fem, "N34")[1]
    n = mats[0].shape[0]
    x0 = np.zeros(n)
    bank = api.AMGBank(ctx, mats[0], 3, aggregates=aggs)
    view = bank.view()
    As = [api.SparseMatrixCSC(ctx, A) for A in mats]
    ops = [separate(api, ctx, mats, aggs, p) for p in range(3)]
    try:
        for p, A in enumerate(mats):
            bank.set_values(p, A)
        want = [api.pcg(As[p], bs[p], x0, ops[p]) for p in range(3)]
        for p in (0, 1, 2, 1, 0):                           # ... to another member and back
            view.select(p)
            got = api.pcg(As[p], bs[p], x0, view)
            print(f"member {p}: it = {got[1]} (separate operator {want[p][1]})")
            assert got[1] == want[p][1] and np.array_equal(got[2], want[p][2]) and np.array_equal(got[0], want[p][0])
        # Graphs. The solvers size a solve's graph by the iteration count of the previous solve with the same (A, M), so
        # solves "of the same size" are solves of one count: maxit = 4, below every member's own count. One such solve
        # with each of the 3 members, then no selection captures anything: the (A, view) pair never changes.
        assert min(w[1] for w in want) > 4
        first = []
        for p in range(3):
            view.select(p)
            first.append(api.pcg(As[1], bs[1], x0, view, maxit=4))
        assert not np.array_equal(first[0][0], first[1][0]) and not np.array_equal(first[2][0], first[1][0])
        captures, replays = ctx.query("graph_captures"), ctx.query("graph_replays")
        assert captures > 0
        for _ in range(2):
            for p in (2, 0, 1):
                view.select(p)
                assert same_solve(api.pcg(As[1], bs[1], x0, view, maxit=4), first[p])
        print(f"graph captures {captures} -> {ctx.query('graph_captures')}, replays {replays} -> {ctx.query('graph_replays')}")
        assert ctx.query("graph_captures") == captures, "a later selection captured a graph again"
        assert ctx.query("graph_replays") > replays
        for p in (2, 0, 1):                                  # ... and the full solves still have the separate operators' bits
            view.select(p)
            assert same_solve(api.pcg(As[p], bs[p], x0, view), want[p])
        try:
            ctx.set_chunk(0)
            for p in range(3):
                view.select(p)
                assert same_solve(api.pcg(As[p], bs[p], x0, view), want[p]), "eager solve"
        finally:
            ctx.set_chunk(8)
        W = np.asfortranarray(np.random.default_rng(3).standard_normal((n, 4)))
        view.select(1)
        assert same_solve(api.defpcg(As[1], bs[1], x0, W, view), api.defpcg(As[1], bs[1], x0, W, ops[1]))
        assert same_solve(api.eigpcg(As[1], bs[1], x0, view, 4, 12), api.eigpcg(As[1], bs[1], x0, ops[1], 4, 12))
    finally:
        for o in ops + As:
            o.close()
        bank.close()


# ------------------------------------------------------------------ 5. refresh under a live view
def test_refresh_under_a_live_view(pkg, ctx, fem):
    api, L = pkg.api, pkg._lib
    mats, aggs = case(fem, "N34")
    n = mats[0].shape[0]
    r = rhs(n)[0]
    bank = api.AMGBank(ctx, mats[0], 3, aggregates=aggs)
    view = bank.view()
    ops = [separate(api, ctx, mats, aggs, p) for p in range(3)]
    try:
        bank.set_values(0, mats[0])
        assert np.array_equal(view.ldiv(r), ops[0].ldiv(r))
        bank.set_values(0, mats[1])                          # A': the next apply is that of an operator refreshed with A'
        z1, H1 = view.ldiv(r), bank.device_hierarchy(0)
        assert np.array_equal(z1, ops[1].ldiv(r)) and not np.array_equal(z1, ops[0].ldiv(r))
        neg = -mats[2]
        for p in (0, 2):                                     # a set member keeps its bits, an unset member stays unset
            with pytest.raises(api.MiError) as e:
                bank.set_values(p, neg)
            print("  refused:", e.value)
            assert e.value.code == L.MI_ERR_SINGULAR
        assert asy.same_hierarchy(bank.device_hierarchy(0), H1) and np.array_equal(view.ldiv(r), z1)
        assert bank.stats()["members_set"] == 1
        with pytest.raises(api.MiError, match="never set"):
            bank.device_hierarchy(2)
        with pytest.raises(api.MiError, match="never set"):
            view.select(2)
        assert np.array_equal(view.ldiv(r), z1)
        bank.set_values(2, mats[2])                          # the engine is not left in a bad state by the refusals
        view.select(2)
        assert np.array_equal(view.ldiv(r), ops[2].ldiv(r))
    finally:
        for o in ops:
            o.close()
        bank.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals(pkg, ctx, fem):
    api, L = pkg.api, pkg._lib
    lib = L.load()
    mats, aggs = case(fem, "N12_3")
    A = mats[0]
    n = A.shape[0]
    ptr, idx = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    n_l = np.array([n] + [int(a.max()) + 1 for a in aggs], dtype=np.int64)
    ag = api._ptrs(aggs, L.i64p)
    i64p, f64p = L.i64p, L.f64p

    def create(capacity=2, context=None, sizes=n_l):
        h = C.c_void_p()
        rc = lib.mi_amg_bank_create((context or ctx)._h, n, ptr.ctypes.data_as(i64p), idx.ctypes.data_as(i64p), len(sizes), sizes.ctypes.data_as(i64p),
                                    ag, capacity, 0, C.byref(h))
        return rc, h

    def refused(rc, *words):
        msg = lib.mi_last_error().decode()
        print("  refused:", msg)
        assert rc == L.MI_ERR_BAD_ARG and len(msg) > 40 and all(w in msg for w in words), (rc, msg, words)

    refused(create(capacity=0)[0], "capacity = 0")
    refused(create(capacity=-3)[0], "capacity = -3")
    bad = n_l.copy(); bad[1] = n + 5                         # what mi_amg_plan_create refuses: level sizes that do not chain
    refused(create(sizes=bad)[0], str(n + 5))
    grp = api.LoopbackGroup(2)
    grp.set_mode(1)
    rank0 = api.Context(0)
    rank0.loopback_init(grp, 0)
    refused(create(context=rank0)[0], "rank 0 of 2")
    rank0.close()

    rc, bank = create(capacity=2)
    assert rc == 0
    val = np.ascontiguousarray(A.data)
    vptr = C.c_void_p(val.ctypes.data)
    check = lambda rc: api.check(rc)
    check(lib.mi_ctx_set_pointer_mode(ctx._h, L.MI_PTR_HOST))
    size = C.c_int64()
    check(lib.mi_op_size(bank, C.byref(size)))
    assert size.value == n
    x, y = np.ones(n), np.zeros(n)
    xp, yp = C.c_void_p(x.ctypes.data), C.c_void_p(y.ctypes.data)
    Aop = api.SparseMatrixCSC(ctx, A)
    # the bank is not applicable
    refused(lib.mi_op_apply(bank, xp, yp), "AMG bank", "view")
    refused(lib.mi_op_apply_dominant(bank, xp, 1), "AMG bank", "view")
    res, it = np.zeros(n + 1), C.c_int64()
    refused(lib.mi_pcg(Aop._h, bank, xp, yp, 0, 1e-7, res.ctypes.data_as(f64p), n + 1, C.byref(it)), "AMG bank")
    refused(lib.mi_cg(bank, xp, yp, 0, 1e-7, res.ctypes.data_as(f64p), n + 1, C.byref(it)), "AMG bank")
    kids = (C.c_void_p * 1)(bank)
    one = np.ones(1)
    comb = C.c_void_p()
    refused(lib.mi_op_combine(ctx._h, 1, kids, one.ctypes.data_as(f64p), C.byref(comb)), "AMG bank")
    # members
    refused(lib.mi_amg_bank_set_values(bank, 2, vptr), "member = 2", "0 .. 1")
    refused(lib.mi_amg_bank_set_values(bank, -1, vptr), "member = -1")
    refused(lib.mi_amg_bank_set_values(Aop._h, 0, vptr), "not an AMG bank")
    refused(lib.mi_amg_bank_set_values(None, 0, vptr), "NULL")
    refused(lib.mi_amg_bank_coarse_inverse(bank, 1, y.ctypes.data_as(f64p)), "member 1", "never set")
    refused(lib.mi_amg_bank_level_get(bank, 0, 0, None, None, None, None, None, None, None, None), "member 0", "never set")
    # views
    view = C.c_void_p()
    refused(lib.mi_amg_bank_view(bank, 0, C.byref(view)), "max_terms = 0")
    refused(lib.mi_amg_bank_view(bank, 17, C.byref(view)), "max_terms = 17")
    refused(lib.mi_amg_bank_view(Aop._h, 1, C.byref(view)), "not an AMG bank")
    check(lib.mi_amg_bank_view(bank, 2, C.byref(view)))
    refused(lib.mi_amg_bank_view(view, 1, C.byref(comb)), "not an AMG bank", "view")
    # the default member 0 is unset: refused at apply and at solve entry
    refused(lib.mi_op_apply(view, xp, yp), "member 0", "never set")
    refused(lib.mi_op_apply_dominant(view, xp, 1), "member 0", "never set")
    refused(lib.mi_pcg(Aop._h, view, xp, yp, 0, 1e-7, res.ctypes.data_as(f64p), n + 1, C.byref(it)), "member 0", "never set")
    mem = lambda *m: np.array(m, dtype=np.int64).ctypes.data_as(i64p)
    cf = lambda *c: np.array(c, dtype=np.float64).ctypes.data_as(f64p)
    refused(lib.mi_amg_bank_select(view, 1, mem(0), cf(1.0)), "member 0", "never set")
    check(lib.mi_amg_bank_set_values(bank, 0, vptr))
    check(lib.mi_op_apply(view, xp, yp))
    z = y.copy()
    refused(lib.mi_amg_bank_select(view, 2, mem(0, 1), cf(0.5, 0.5)), "member 1", "never set")
    refused(lib.mi_amg_bank_select(view, 1, mem(2), cf(1.0)), "member = 2")
    refused(lib.mi_amg_bank_select(view, 0, mem(0), cf(1.0)), "k = 0")
    refused(lib.mi_amg_bank_select(view, 3, mem(0, 0, 0), cf(1.0, 1.0, 1.0)), "k = 3", "max_terms = 2")
    refused(lib.mi_amg_bank_select(view, 1, mem(0), cf(float("nan"))), "coef[0]", "finite")
    refused(lib.mi_amg_bank_select(view, 2, mem(0, 0), cf(1.0, float("inf"))), "coef[1]", "finite")
    refused(lib.mi_amg_bank_select(bank, 1, mem(0), cf(1.0)), "not a view", "AMG bank")
    refused(lib.mi_amg_bank_select(Aop._h, 1, mem(0), cf(1.0)), "not a view")
    refused(lib.mi_amg_bank_stats(view, None, None, None, None, None), "not an AMG bank", "view")
    check(lib.mi_op_apply(view, xp, yp))                     # the refused selections changed nothing
    assert np.array_equal(y, z)
    # lifetime: the bank under a live view; a view inside a combination
    nv = C.c_int64()
    check(lib.mi_amg_bank_stats(bank, None, None, None, None, C.byref(nv)))
    assert nv.value == 1
    refused(lib.mi_op_destroy(bank), "1 live view")
    kids = (C.c_void_p * 2)(view, view)
    check(lib.mi_op_combine(ctx._h, 2, kids, cf(0.25, 0.5), C.byref(comb)))
    check(lib.mi_op_apply(comb, xp, yp))
    assert np.array_equal(y, 0.25 * z + 0.5 * z)
    refused(lib.mi_op_destroy(view), "2 place(s)", "mi_op_combine")
    check(lib.mi_op_destroy(comb))
    check(lib.mi_op_destroy(view))
    check(lib.mi_amg_bank_stats(bank, None, None, None, None, C.byref(nv)))
    assert nv.value == 0
    check(lib.mi_op_destroy(bank))
    Aop.close()


def test_python_refusals_on_a_live_bank(pkg, ctx, fem):
    api = pkg.api
    mats, aggs = case(fem, "N12_2")
    bank = api.AMGBank(ctx, mats[0], 2, aggregates=aggs)
    try:
        with pytest.raises(IndexError):
            bank.set_values(2, mats[0])
        with pytest.raises(ValueError, match="stored entries"):
            bank.set_values(0, mats[0].data[:-1])
        with pytest.raises(ValueError, match="max_terms"):
            bank.view(17)
        view = bank.view(2)
        with pytest.raises(api.MiError, match="never set"):
            view.ldiv(np.ones(bank.n))
        bank.set_values(0, mats[0])
        with pytest.raises(ValueError, match="finite"):
            view.combine([0, 0], [1.0, np.inf])
        with pytest.raises(ValueError, match="k = 3"):
            view.combine([0, 0, 0], [1.0, 1.0, 1.0])
        with pytest.raises(api.MiError, match="live view"):
            api.check(ctx._L.mi_op_destroy(bank._h))
        assert bank.stats()["views"] == 1
        view.close()
        assert bank.stats()["views"] == 0
    finally:
        bank.close()


# ------------------------------------------------------------------ 7. stats
@pytest.mark.parametrize("name", ["N12_1", "N12_3", "N34", "chain_7", "one_65"])
def test_stats(pkg, ctx, fem, name):
    api = pkg.api
    mats, aggs = case(fem, name)
    bank = api.AMGBank(ctx, mats[0], 4, aggregates=aggs)
    try:
        st = bank.stats()
        assert st["capacity"] == 4 and st["members_set"] == 0 and st["views"] == 0
        bank.set_values(3, mats[1]); bank.set_values(1, mats[0]); bank.set_values(3, mats[0])
        v1, v2 = bank.view(), bank.view(3)
        st = bank.stats()
        assert st["members_set"] == 2 and st["views"] == 2
        H = bank.device_hierarchy(3)
        L, nc = H.nlevels, H.sizes[-1]
        counts = [a.indices.size for a in H.A] + 2 * [p.indices.size for p in H.P] + list(H.sizes[:-1]) + [nc * nc]
        formula = 8 * (sum(a.indices.size for a in H.A) + 2 * sum(p.indices.size for p in H.P) + sum(H.sizes[:-1]) + nc * nc + 2 * (L - 1))
        padding = 8 * sum(c % 2 for c in counts)
        print(f"{name}: bytes_per_member = {st['bytes_per_member']} = {formula} + {padding} of padding; bytes_shared = {st['bytes_shared']}")
        assert st["bytes_per_member"] == formula + padding == api.amg_bank_member_bytes(H)
        assert st["bytes_shared"] > 0
        v1.close()
        assert bank.stats()["views"] == 1
        v2.close()
    finally:
        bank.close()
