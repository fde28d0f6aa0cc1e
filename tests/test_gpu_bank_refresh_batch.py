"""GPU suite of the batched bank refresh (`AMGBank.set_values_batch`, `mi_amg_bank_set_values_batch`; csrc/amg_bank_setup.hpp):
the hierarchies of k <= 16 bank members from k slots of a `CsrBatch`, in one sequence of launches with the term as the grid's
second dimension.

Every comparison is bit for bit (`np.array_equal`), against the same bank type refreshed member by member with
`AMGBank.set_values` on the same values: the hierarchy read back (`device_hierarchy(p)`: every A_l, P_l, ω/d, ω and the coarse
inverse) and the view's apply on a random and a unit right-hand side, which covers R. The k coarse blocks are inverted in one
call of the routine that inverts the single block; its launches put the block on the grid's third dimension and the blocks of
one call share nb_max and n_max, so the inverse is held to the same bits, without a tolerance.

Cases, case builders and right-hand sides are those of tests/test_gpu_amg_bank.py (the N = 12 mesh with 1, 2 and 3 levels, the
N = 34 mesh, the synthetic pairs of tests/amg_setup_synth.py, the odd-nnz chains with 1, 7, 8, 9 and 17 row blocks); the failing
matrices are those of tests/test_gpu_amg_refresh.py and tests/test_gpu_amg_setup_edges.py."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import amg_setup_synth as asy
from conftest import f_m1, lognormal_coeff, u3
from test_gpu_amg_bank import CASES, case, mesh_members, rhs

pytestmark = pytest.mark.gpu


def filled_batch(api, ctx, mats, capacity=None, **kw):
    batch = api.CsrBatch(ctx, mats[0], capacity or len(mats), **kw)
    for s, A in enumerate(mats):
        batch.set_values(s, A)
    return batch


def single_bank(api, ctx, mats, aggs):
    """the reference: every member from a separate set_values call"""
    bank = api.AMGBank(ctx, mats[0], len(mats), aggregates=aggs)
    for p, A in enumerate(mats):
        bank.set_values(p, A)
    return bank


def assert_member(X, p, vx, Y, q, vy, tag):
    """member p of bank X is member q of bank Y: the hierarchy with its coarse inverse, and the apply"""
    Hx, Hy = X.device_hierarchy(p), Y.device_hierarchy(q)
    assert asy.same_hierarchy(Hx, Hy), f"{tag}: member {p} differs from the single refresh"
    vx.select(p); vy.select(q)
    for r in rhs(X.n):
        assert np.array_equal(vx.ldiv(r), vy.ldiv(r)), f"{tag}: apply of member {p}"


# ------------------------------------------------------------------ 1. a batched member is the singly refreshed one
@pytest.mark.parametrize("name", CASES)
def test_batched_member_equals_the_single_refresh(pkg, ctx, fem, name):
    api = pkg.api
    mats, aggs = case(fem, name)
    m = len(mats)
    X, Y = api.AMGBank(ctx, mats[0], m, aggregates=aggs), single_bank(api, ctx, mats, aggs)
    batch = filled_batch(api, ctx, mats)
    try:
        before = X.stats()["bytes_shared"]
        ok = X.set_values_batch(np.arange(m), batch, np.arange(m))
        assert ok.dtype == bool and ok.tolist() == [True] * m
        st = X.stats()
        assert st["members_set"] == m and st["bytes_shared"] > before == Y.stats()["bytes_shared"]
        vx, vy = X.view(), Y.view()
        for p in range(m):
            assert_member(X, p, vx, Y, p, vy, name)
            assert np.array_equal(X.device_hierarchy(p).A[0].data, mats[p].data)
    finally:
        batch.close(); X.close(); Y.close()


# ------------------------------------------------------------------ 2. shapes of the call
@pytest.fixture(scope="module")
def sixteen(pkg, ctx, fem):
    api = pkg.api
    mats, aggs = mesh_members(fem, 12, 16)[0], case(fem, "N12_3")[1]
    Y = single_bank(api, ctx, mats, aggs)
    batch = filled_batch(api, ctx, mats)
    yield mats, aggs, Y, Y.view(), batch
    batch.close(); Y.close()


@pytest.mark.parametrize("k", [1, 3, 16])
def test_k_terms(pkg, ctx, sixteen, k):
    mats, aggs, Y, vy, batch = sixteen
    X = pkg.api.AMGBank(ctx, mats[0], 16, aggregates=aggs)
    try:
        assert X.set_values_batch(np.arange(k), batch, np.arange(k)).all()
        assert X.stats()["members_set"] == k
        vx = X.view()
        for p in range(k):
            assert_member(X, p, vx, Y, p, vy, f"k = {k}")
        if k < 16:
            with pytest.raises(pkg.api.MiError, match="never set"):
                X.device_hierarchy(k)
    finally:
        X.close()


def test_permutations_shared_slots_and_a_reused_workspace(pkg, ctx, sixteen):
    mats, aggs, Y, vy, batch = sixteen
    X = pkg.api.AMGBank(ctx, mats[0], 16, aggregates=aggs)
    try:
        vx = X.view()
        holds = {}                                           # member of X -> the slot (= member of Y) it was built from

        def call(members, slots):
            assert X.set_values_batch(members, batch, slots).all()
            holds.update(zip(members, slots))
            for p, q in holds.items():
                assert_member(X, p, vx, Y, q, vy, f"members {members} from slots {slots}")

        perm = np.random.default_rng(4).permutation(16).tolist()
        call(perm[:5], [0, 1, 2, 3, 4])                      # members permuted against slots
        ws5 = X.stats()["bytes_shared"]
        call([0, 5, 9], [2, 2, 2])                           # one slot feeds several members
        assert X.stats()["bytes_shared"] == ws5              # a smaller k after a larger one: the same workspace
        call(perm, list(range(16)))                          # the largest k; overwrites every member set before
        ws16 = X.stats()["bytes_shared"]
        assert ws16 > ws5
        call([7, 3, 11], [15, 0, 8])                         # ... and a smaller k on the workspace of 16
        call([4], [9])
        assert X.stats()["bytes_shared"] == ws16 and X.stats()["members_set"] == 16
    finally:
        X.close()


def test_one_based_creation_gives_the_same_bits(pkg, ctx, sixteen):
    mats, aggs, Y, vy, _ = sixteen
    api = pkg.api
    X = api.AMGBank(ctx, mats[0], 4, index_base=1, aggregates=aggs)
    batch = filled_batch(api, ctx, mats[:4], index_base=1)
    try:
        assert X.set_values_batch([3, 0, 2, 1], batch, [0, 1, 2, 3]).all()
        vx = X.view()
        for p, q in zip([3, 0, 2, 1], [0, 1, 2, 3]):
            assert_member(X, p, vx, Y, q, vy, "1-based")
    finally:
        batch.close(); X.close()


# ------------------------------------------------------------------ 3. isolation
def test_a_failed_term_touches_nothing_but_itself(pkg, ctx):
    api, L = pkg.api, pkg._lib
    A0, bad, aggs = asy.breakdown(3)                         # positive diagonal, level-1 diagonal negative
    n = A0.shape[0]
    S = asy.chain(n)
    good = [asy.spd_values(S, [61, j]) for j in range(4)]
    neg = A0.copy()
    k = neg.indptr[n // 2] + int(np.flatnonzero(neg.indices[neg.indptr[n // 2]:neg.indptr[n // 2 + 1]] == n // 2)[0])
    neg.data[k] = -neg.data[k]                               # a non-positive level-0 diagonal
    nan = A0.copy()
    nan.data[nan.data.size // 2] = np.nan
    slots = [good[0], neg, good[1], bad, nan, good[2], good[3]]
    healthy = {0: 0, 2: 1, 5: 2, 6: 3}                       # slot -> index in `good`
    Y, vy = single_bank(api, ctx, good, aggs), None
    X = api.AMGBank(ctx, A0, 8, aggregates=aggs)
    batch = filled_batch(api, ctx, slots)
    Ag = api.SparseMatrixCSC(ctx, good[3])
    try:
        vy, vx = Y.view(), X.view()
        X.set_values(1, good[3]); X.set_values(3, good[3])   # set before the call: must keep these bits; member 4 stays unset
        H1 = X.device_hierarchy(1)
        b = rhs(n)[0]
        vx.select(1)
        first = api.pcg(Ag, b, np.zeros(n), vx)
        assert np.array_equal(api.pcg(Ag, b, np.zeros(n), vx)[0], first[0])            # (replayed)
        ok = X.set_values_batch([0, 1, 2, 3, 4, 5], batch, [0, 1, 2, 3, 4, 5], strict=False)
        msg = L.load().mi_last_error().decode()
        print("  failed terms:", msg)
        assert ok.tolist() == [True, False, True, False, False, True]
        assert "term 1" in msg and "term 3" in msg and "term 4" in msg and "diagonal" in msg and "finite" in msg and "3 of 6" in msg
        assert X.stats()["members_set"] == 5
        for p in (1, 3):
            assert asy.same_hierarchy(X.device_hierarchy(p), H1), f"member {p} lost its previous bits"
            assert_member(X, p, vx, Y, 3, vy, "kept")
        with pytest.raises(api.MiError, match="never set"):
            X.device_hierarchy(4)
        for p in (0, 2, 5):
            assert_member(X, p, vx, Y, healthy[p], vy, "healthy beside failed terms")
        vx.select(1)
        again = api.pcg(Ag, b, np.zeros(n), vx)                                         # the graph captured before the call
        assert again[1] == first[1] and np.array_equal(again[0], first[0]) and np.array_equal(again[2], first[2])
        # strict: the error comes after the commit of the healthy terms
        with pytest.raises(api.MiError) as e:
            X.set_values_batch([0, 1, 2], batch, [2, 3, 0])
        print("  raised:", e.value)
        assert e.value.code == L.MI_ERR_SINGULAR and "term 1 (member 1, slot 3)" in str(e.value) and "diagonal" in str(e.value)
        assert e.value.ok.tolist() == [True, False, True]
        assert_member(X, 0, vx, Y, healthy[2], vy, "strict"); assert_member(X, 2, vx, Y, healthy[0], vy, "strict")
        assert asy.same_hierarchy(X.device_hierarchy(1), H1)
        # without a status array the library returns MI_ERR_SINGULAR itself
        arr = lambda *v: np.array(v, dtype=np.int64)
        mem, sl = arr(6, 4), arr(6, 4)
        rc = L.load().mi_amg_bank_set_values_batch(X._h, 2, mem.ctypes.data_as(L.i64p), batch._h, sl.ctypes.data_as(L.i64p), None)
        assert rc == L.MI_ERR_SINGULAR and "term 1 (member 4, slot 4)" in L.load().mi_last_error().decode()
        assert_member(X, 6, vx, Y, 3, vy, "status == NULL")
        with pytest.raises(api.MiError, match="never set"):
            X.device_hierarchy(4)
        # the next all-healthy call
        assert X.set_values_batch([1, 3, 4], batch, [0, 2, 5]).all()
        for p, s in ((1, 0), (3, 2), (4, 5)):
            assert_member(X, p, vx, Y, healthy[s], vy, "after the failures")
        assert X.stats()["members_set"] == 7
    finally:
        Ag.close(); batch.close(); X.close(); Y.close()


# ------------------------------------------------------------------ 4. the flow
def test_update_batch_refresh_batch_pcg_batch(pkg, ctx, fem):
    import full_assembly_cases as cases
    api = pkg.api
    k = 4
    mesh = fem.get_mesh(34)
    plan = cases.make_plan(fem, mesh, f_m1, u3)
    dev = api.FullAssemblyPlan(ctx, plan)
    coeffs = [lognormal_coeff(fem, mesh.points, 481456 + p) for p in range(k)]
    csr = lambda v: sp.csr_matrix((v, plan.colidx, plan.rowptr), shape=(plan.n, plan.n))
    A_0 = csr(dev.run(np.ones(plan.n_node))[0])
    aggs = [np.asarray(a, dtype=np.int64) for a in fem.prepare_amg_precond(A_0).agg]
    n = plan.n
    batch = api.CsrBatch(ctx, A_0, k)
    X, Y = api.AMGBank(ctx, A_0, k, aggregates=aggs), api.AMGBank(ctx, A_0, k, aggregates=aggs)
    opened = []
    try:
        B = np.asfortranarray(np.column_stack([dev.update_batch(coeffs[t], batch, t) for t in range(k)]))
        assert X.set_values_batch(np.arange(k), batch, np.arange(k)).all()
        got = api.pcg_batch(batch, np.arange(k), B, np.zeros((n, k), order="F"), X.view(k), np.arange(k))
        vals = [batch.get_values(t) for t in range(k)]
        for t in range(k):
            Y.set_values(t, vals[t])
        want = api.pcg_batch(batch, np.arange(k), B, np.zeros((n, k), order="F"), Y.view(k), np.arange(k))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert all(np.array_equal(a, b) for a, b in zip(got[2], want[2]))
        for t in range(k):                                   # what the per-realization preconditioner promises
            A_t = csr(vals[t])
            M, Ag = api.AMGPreconditioner(ctx, fem.amg_refresh(aggs, A_t)), api.SparseMatrixCSC(ctx, A_t)
            opened += [M, Ag]
            it = api.pcg(Ag, B[:, t].copy(), np.zeros(n), M)[1]
            print(f"system {t}: it = {got[1][t]} batched, {it} with a fresh host hierarchy")
            assert got[1][t] == it
    finally:
        for o in opened:
            o.close()
        batch.close(); X.close(); Y.close(); dev.close()


# ------------------------------------------------------------------ 5. refusals
def test_refusals_leave_every_member_untouched(pkg, ctx, fem):
    api, L = pkg.api, pkg._lib
    lib = L.load()
    mats, aggs = case(fem, "N12_3")
    A = mats[0]
    n = A.shape[0]
    X = api.AMGBank(ctx, A, 4, aggregates=aggs)
    batch = filled_batch(api, ctx, mats[:2], capacity=4)     # slots 0, 1 set; 2, 3 never
    other_ctx = api.Context(0)
    made = []
    try:
        assert X.set_values_batch([0, 1], batch, [0, 1]).all()
        H = [X.device_hierarchy(p) for p in (0, 1)]
        arr = lambda v: np.array(v, dtype=np.int64)

        def call(members, slots, bank=X._h, A_batch=batch._h, k=None):
            mem, sl = arr(members), arr(slots)
            st = (C.c_int * 16)()
            return lib.mi_amg_bank_set_values_batch(bank, len(members) if k is None else k, mem.ctypes.data_as(L.i64p), A_batch, sl.ctypes.data_as(L.i64p), st)

        def refused(rc, *words):
            msg = lib.mi_last_error().decode()
            print("  refused:", msg)
            assert rc == L.MI_ERR_BAD_ARG and len(msg) > 40 and all(w in msg for w in words), (rc, msg, words)

        refused(call([0], [0], k=0), "k = 0")
        refused(call(list(range(17)), [0] * 17), "k = 17", "16")
        refused(call([0, 4], [0, 1]), "member = 4", "0 .. 3")
        refused(call([-1], [0]), "member = -1")
        refused(call([0, 1], [0, 4]), "slot = 4", "0 .. 3")
        refused(call([0, 1], [0, 2]), "slot 2", "never set")
        refused(call([2, 3, 2], [0, 1, 1]), "member 2", "twice", "terms 0 and 2")
        assert call([2, 3], [1, 1]) == 0                     # the same slot twice is allowed
        H += [X.device_hierarchy(p) for p in (2, 3)]
        view = X.view()
        A_op = api.SparseMatrixCSC(ctx, A); made.append(A_op)
        refused(call([0], [0], bank=batch._h), "not an AMG bank", "batch of sparse matrices")
        refused(call([0], [0], bank=view._h), "not an AMG bank", "view")
        refused(call([0], [0], bank=None), "NULL")
        refused(call([0], [0], A_batch=X._h), "not a batch", "AMG bank")
        refused(call([0], [0], A_batch=A_op._h), "not a batch")
        refused(call([0], [0], A_batch=None), "NULL")
        foreign = filled_batch(api, other_ctx, mats[:1]); made.append(foreign)
        refused(call([0], [0], A_batch=foreign._h), "different contexts")
        mats34 = mesh_members(fem, 34, 1)[0]
        big = filled_batch(api, ctx, mats34); made.append(big)
        refused(call([0], [0], A_batch=big._h), str(n), str(mats34[0].shape[0]), "stored entries")
        # the same n and nnz, another pattern: found by the full comparison of the first meeting
        S = sp.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape).tolil()
        i = next(r for r in range(n) if S[r, (r + n // 2) % n] == 0 and S[r].nnz > 1)
        j = [c for c in S.rows[i] if c != i][0]
        S[i, j] = 0; S[i, (i + n // 2) % n] = 1
        S = sp.csr_matrix(S); S.eliminate_zeros(); S.sort_indices()
        assert S.nnz == A.nnz
        moved = filled_batch(api, ctx, [S]); made.append(moved)
        refused(call([0], [0], A_batch=moved._h), "pattern")
        refused(call([0], [0], A_batch=moved._h), "pattern")  # ... and a refusal is not remembered as a match
        # a context that has become one rank of several
        rank_ctx = other_ctx
        bank_r = api.AMGBank(rank_ctx, A, 1, aggregates=aggs); made.append(bank_r)
        grp = api.LoopbackGroup(2)
        grp.set_mode(1)
        rank_ctx.loopback_init(grp, 0)
        refused(call([0], [0], bank=bank_r._h, A_batch=foreign._h), "rank 0 of 2")
        assert bank_r.stats()["members_set"] == 0
        assert X.stats()["members_set"] == 4
        for p in range(4):
            assert asy.same_hierarchy(X.device_hierarchy(p), H[p]), f"a refusal changed member {p}"
    finally:
        for o in reversed(made):
            o.close()
        batch.close(); X.close(); other_ctx.close()


# ------------------------------------------------------------------ 6. get_centroidal_bank(batch=4)
def test_centroidal_bank_in_batches(pkg, ctx, fem):
    import full_assembly_cases as cases
    api = pkg.api
    mesh = fem.get_mesh(12)
    plan = cases.make_plan(fem, mesh, f_m1, u3)
    dev = api.FullAssemblyPlan(ctx, plan)
    kl = fem.synthetic_kl(mesh.points, m_side=3)
    field = api.KLField(ctx, kl.Λ, kl.Ψ)
    centroids = np.random.default_rng(12).standard_normal((5, 6))          # 6 is no multiple of 4: the last call is short
    A_0 = sp.csr_matrix((dev.run(np.ones(plan.n_node))[0], plan.colidx, plan.rowptr), shape=(plan.n, plan.n))
    one = api.get_centroidal_bank(ctx, centroids, field, lambda a: dev.run(a)[0], A_0, max_levels=3, max_coarse=4)
    four = api.get_centroidal_bank(ctx, centroids, field, dev, A_0, batch=4, max_levels=3, max_coarse=4)
    try:
        assert one.n_levels == four.n_levels == 3 and four.stats()["members_set"] == 6
        v1, v4 = one.view(), four.view()
        for p in range(6):
            assert_member(four, p, v4, one, p, v1, "get_centroidal_bank(batch=4)")
        assert not asy.same_hierarchy(four.device_hierarchy(0), four.device_hierarchy(5))
    finally:
        one.close(); four.close(); dev.close()
