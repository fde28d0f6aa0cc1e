"""GPU suite (-m gpu): the fp32-stored Neumann-Neumann preconditioner (`mi_nn_create_stored(..., MI_STORE_F32)`,
`NeumannNeumannSchurPreconditioner(..., storage="f32")`), everything through the C ABI.

fp32 is a storage format of the ΠS_d blocks only: the apply must be the fp64 apply of `double(float(ΠS_d))` up to
summation order. So the oracle of every comparison is the existing fp64 oracle on the ROUNDED blocks
(`B.astype(float32).astype(float64)`), and the bars are the project's own (tests/test_gpu_parity.py): single applies
rel. 1e-13, `it` equal, res_norm to 1e-8 (+1e-12 res_1), solution 1e-6; synthetic blocks against the long-double row-sum
bound of tests/test_gpu_dense_edges.py. No bar here is new."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, f_m1, lognormal_coeff, lowest_eigvecs, u0734, unstructured_mesh
from test_gpu_dense_edges import assert_summation_bound, concat, gather_maps, ref_apply
from test_gpu_parity import assert_history

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
# both sides of a 4-column load, a 32-float line, a 256-column wave load, the 2 KiB-stride guard (512 floats) and GEMV_PANEL
F32_EDGE_SIZES = [1, 3, 4, 5, 31, 32, 33, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048]


def rounded(blocks):
    return [None if B is None else np.asfortranarray(B.astype(np.float32).astype(np.float64)) for B in blocks]


def nn(pkg, ctx, blocks, g, cnt, storage="f32", **kw):
    return pkg.api.NeumannNeumannSchurPreconditioner(ctx, blocks, g, cnt, storage=storage, **kw)


@pytest.fixture(scope="module")
def n200(fem):
    """N=200, 4x2 subdomains, lognormal coefficient (seed 481456): n_Γ = 789."""
    mesh = fem.get_mesh(200)
    return fem.build_schur_problem(200, 4, 2, lognormal_coeff(fem, mesh.points), f_m1, u0734)


@pytest.fixture(scope="module")
def edge_problem():
    rng = np.random.default_rng(20261016)
    g, cnt, n_Γ = gather_maps(F32_EDGE_SIZES, rng)
    blocks = [np.asfortranarray(rng.standard_normal((n, n))) for n in F32_EDGE_SIZES]   # non-symmetric on purpose
    plain = [B.copy(order="F") for B in blocks]
    for B in blocks:    # entries that round to fp32 subnormals (kept) and to zero, beside ordinary ones
        n = B.shape[0]
        if n > 3:
            B[0, n - 1] = 3.7e-41
            B[n - 1, 0] = -1.0e-46
            B[1, 2] = 1.0e-39
            B[2, 1] = 7.0e-46         # exactly half of the smallest subnormal: to even = 0
    x = rng.standard_normal(n_Γ)
    return g, cnt, n_Γ, blocks, x, plain


def slot_width(cnt):
    w = int(cnt.max())
    return 4 if w == 3 else w


# ------------------------------------------------------------------ applies
@pytest.mark.parametrize("case", ["micro", "toy", "ragged", "unstructured"])
def test_apply_matches_oracle_on_rounded_blocks(pkg, ctx, orc, fem, request, case):
    if case == "unstructured":
        mesh, epart, npart = unstructured_mesh(fem)
        coeff = lambda x, y: 1.0 + 0.5 * np.sin(5 * x) * np.cos(3 * y)      # noqa: E731
        P = fem.build_schur_problem(28, 0, 0, coeff, f_m1, u0734, mesh=mesh, partition=(epart, npart))
        assert P.sub.ndom == 6 and P.sub.node_Γ_cnt.max() >= 5
    else:
        P = request.getfixturevalue(case)
    sub = P.sub
    M = nn(pkg, ctx, P.ΠSd, sub.gather_idx, sub.node_Γ_cnt)
    Mo = orc.neumann_neumann_operator(rounded(P.ΠSd), sub.gather_idx, sub.node_Γ_cnt)
    assert M.storage == "f32"
    for seed in (8, 9):
        v = np.random.default_rng(seed).standard_normal(sub.n_Γ)
        y, yo = M.ldiv(v), Mo * v
        err = np.abs(y - yo).max() / np.abs(y).max()
        print(f"{case}: apply vs oracle(rounded) {err:.2e}")
        assert np.allclose(y, yo, rtol=0, atol=1e-13 * np.abs(y).max())
    M.close()


def test_apply_at_layout_edges(pkg, ctx, edge_problem):
    """Random non-symmetric blocks on random gather maps at the edges of the fp32 layout, against the long-double row sums
    of the rounded blocks; creation (host conversion) and set_blocks (device conversion, host and device pointers) must
    hold what numpy.astype(float32) gives, bit for bit."""
    import torch
    g, cnt, n_Γ, blocks, x, _ = edge_problem
    ref = ref_apply(rounded(blocks), g, cnt, x, nn=True)
    M = nn(pkg, ctx, blocks, g, cnt)
    y = M.apply(x)
    assert_summation_bound(y, ref, slot_width(cnt), "NN fp32")
    R = nn(pkg, ctx, rounded(blocks), g, cnt)
    assert np.array_equal(R.apply(x), y)                       # (float)B == (float)double(float(B)): host conversion = numpy's
    other = [np.asfortranarray(0.5 * b.T) for b in blocks]
    for src in (concat(blocks), torch.from_numpy(concat(blocks)).to("cuda")):
        U = nn(pkg, ctx, other, g, cnt)
        y_other = U.apply(x)
        U.set_blocks(src)
        ctx.synchronize()
        assert not np.array_equal(y_other, y)
        assert np.array_equal(U.apply(x), y), type(src).__name__
        U.close()
    M.close(); R.close()


@pytest.mark.parametrize("n", [5, 33, 300])
def test_subnormals_are_kept_not_flushed(pkg, ctx, n):
    """A block whose every entry rounds to an fp32 subnormal (or to zero): the products are ordinary fp64 numbers, so a
    conversion that flushed subnormals — on the host at creation, on the device in set_blocks, or when the kernel widens
    them — would return zeros and miss the bound by the whole result."""
    import torch
    rng = np.random.default_rng(n)
    B = np.asfortranarray(rng.standard_normal((n, n)) * 1e-41)
    B[rng.random((n, n)) < 0.2] *= 1e-6                         # some below half the smallest subnormal: zero
    Rn = rounded([B])[0]
    tiny = np.float64(np.finfo(np.float32).tiny)
    assert np.all(np.abs(Rn) < tiny) and np.count_nonzero(Rn) > n and np.count_nonzero(Rn == 0) > 0
    g, cnt = [np.arange(n, dtype=np.int64)], np.ones(n, dtype=np.int64)
    x = rng.standard_normal(n)
    ref = ref_apply([Rn], g, cnt, x, nn=True)
    M = nn(pkg, ctx, [B], g, cnt)
    y = M.apply(x)
    assert np.count_nonzero(y) == n
    assert_summation_bound(y, ref, 1, f"subnormal block n={n}")
    for src in (concat([B]), torch.from_numpy(concat([B])).to("cuda")):
        U = nn(pkg, ctx, [np.asfortranarray(np.eye(n))], g, cnt)
        U.set_blocks(src)
        ctx.synchronize()
        assert np.array_equal(U.apply(x), y), type(src).__name__
        U.close()
    M.close()


def test_storage_really_is_fp32(pkg, ctx, edge_problem):
    """(On the blocks without the tiny entries: 2^-24 is the relative rounding error of fp32's normal range.)"""
    g, cnt, n_Γ, _, x, blocks = edge_problem
    M32, M64 = nn(pkg, ctx, blocks, g, cnt), nn(pkg, ctx, blocks, g, cnt, storage="f64")
    R32 = nn(pkg, ctx, rounded(blocks), g, cnt, storage=np.float32)
    y32, y64 = M32.apply(x), M64.apply(x)
    assert np.array_equal(R32.apply(x), y32)                   # the blocks held are double(float(B)) ...
    assert not np.array_equal(y32, y64)                        # ... not B
    # every row within the rounding bound 2^-24 Σ_j |B_ij| |x_j| of the fp64-stored apply, plus both summation bounds
    _, mag, wid = ref_apply(blocks, g, cnt, x, nn=True)
    bar = (2.0 ** -24 + 2 * (wid + slot_width(cnt) + 4) * EPS) * mag
    err = np.abs(y32.astype(np.longdouble) - y64.astype(np.longdouble))
    print(f"fp32 vs fp64 storage: max err / bar = {float(np.max(err / np.maximum(bar, 1e-300))):.3e}")
    assert np.all(err <= bar)
    sizes = np.array(F32_EDGE_SIZES, dtype=np.int64)
    assert M32.bytes()[1] == int(np.sum(4 * sizes ** 2 + 20 * sizes))
    assert M64.bytes()[1] == int(np.sum(8 * sizes ** 2 + 20 * sizes))
    assert M32.bytes()[0] == M32.bytes()[1] + 8 * n_Γ
    assert (M32.storage, M64.storage, R32.storage) == ("f32", "f64", "f32")
    S = pkg.api.LocalSchurs(ctx, blocks, g, cnt)
    import ctypes as C
    s = C.c_int(-1)
    assert pkg._lib.load().mi_op_storage(S._h, C.byref(s)) == 0 and s.value == 0
    for op in (M32, M64, R32, S):
        op.close()


# ------------------------------------------------------------------ solvers
@pytest.mark.parametrize("case", ["micro", "toy", "ragged", "n200"])
def test_solvers_match_oracle_on_rounded_blocks(pkg, ctx, orc, request, monkeypatch, case):
    api = pkg.api
    P = request.getfixturevalue(case)
    sub = P.sub
    n, b, ndom = sub.n_Γ, P.b_schur, sub.ndom
    S = api.LocalSchurs(ctx, P.Sd, sub.gather_idx, sub.node_Γ_cnt)
    M = nn(pkg, ctx, P.ΠSd, sub.gather_idx, sub.node_Γ_cnt)
    So = orc.apply_local_schurs_operator(P.Sd, sub.gather_idx, n)
    Mo = orc.neumann_neumann_operator(rounded(P.ΠSd), sub.gather_idx, sub.node_Γ_cnt)
    Mo64 = orc.neumann_neumann_operator(P.ΠSd, sub.gather_idx, sub.node_Γ_cnt)
    x0 = np.zeros(n)
    want = orc.pcg(So, b, x0, Mo)
    assert want[1] == orc.pcg(So, b, x0, Mo64)[1]              # (the CPU suite pins this for micro, toy, ragged)
    W = lowest_eigvecs(So, n, ndom + 10)
    want_d = orc.defpcg(So, b, x0, W, Mo)
    nvec, spdim = (int(1.25 * ndom), 3 * ndom) if ndom > 4 else (3, 8)
    want_e = orc.eigpcg(So, b, x0, Mo, nvec, spdim)
    b2 = So(np.random.default_rng(3).standard_normal(n))
    want_e2 = orc.eigdefpcg(So, b2, x0, Mo, want_e[3], spdim)
    for no_fold in (False, True):
        if no_fold:
            monkeypatch.setenv("MI355_NO_FOLD", "1")
        else:
            monkeypatch.delenv("MI355_NO_FOLD", raising=False)
        f0 = ctx.query("folded_pcg")
        got = api.pcg(S, b, x0, M)
        f1 = ctx.query("folded_pcg")
        assert_history(got, want, So, b)
        assert got[1] == want[1]                                # = the fp64-preconditioned count
        got_d = api.defpcg(S, b, x0, W, M)
        f2 = ctx.query("folded_pcg")
        assert_history(got_d, want_d, So, b)
        assert (f1 > f0 and f2 > f1) if not no_fold else (f1 == f0 and f2 == f1), (no_fold, f0, f1, f2)
        got_e = api.eigpcg(S, b, x0, M, nvec, spdim)
        assert_history(got_e[:3], want_e[:3], So, b)
        got_e2 = api.eigdefpcg(S, b2, x0, M, want_e[3], spdim)
        assert_history(got_e2[:3], want_e2[:3], So, b2)
    S.close(); M.close()


def test_full_size_pcg(pkg, ctx, orc, full):
    """Config 3 (N=1000, 4x2, n_Γ = 3989): 15 iterations with the fp64 and with the fp32-stored preconditioner."""
    api, P = pkg.api, full
    sub = P.sub
    n, b = sub.n_Γ, P.b_schur
    S = api.LocalSchurs(ctx, P.Sd, sub.gather_idx, sub.node_Γ_cnt)
    M = nn(pkg, ctx, P.ΠSd, sub.gather_idx, sub.node_Γ_cnt)
    So = orc.apply_local_schurs_operator(P.Sd, sub.gather_idx, n)
    Mo = orc.neumann_neumann_operator(rounded(P.ΠSd), sub.gather_idx, sub.node_Γ_cnt)
    Mo64 = orc.neumann_neumann_operator(P.ΠSd, sub.gather_idx, sub.node_Γ_cnt)
    f0 = ctx.query("folded_pcg")
    got = api.pcg(S, b, np.zeros(n), M)
    assert ctx.query("folded_pcg") > f0
    want = orc.pcg(So, b, np.zeros(n), Mo)
    assert_history(got, want, So, b)
    it64 = orc.pcg(So, b, np.zeros(n), Mo64)[1]
    print(f"config 3: it fp32-stored {got[1]}, oracle rounded {want[1]}, oracle fp64 {it64}")
    assert got[1] == want[1] == it64
    nd = np.asarray(sub.n_Γd, dtype=np.int64)
    assert M.bytes()[1] == int(np.sum(4 * nd ** 2 + 20 * nd))
    S.close(); M.close()


def test_graph_replay_is_bitwise_reproducible(pkg, ctx, ragged):
    api, P = pkg.api, ragged
    sub = P.sub
    S = api.LocalSchurs(ctx, P.Sd, sub.gather_idx, sub.node_Γ_cnt)
    M = nn(pkg, ctx, P.ΠSd, sub.gather_idx, sub.node_Γ_cnt)
    r0 = ctx.query("graph_replays")
    runs = [api.pcg(S, P.b_schur, np.zeros(sub.n_Γ), M) for _ in range(3)]
    assert ctx.query("graph_replays") > r0 and ctx.query("no_graph") == 0
    for x, it, res in runs[1:]:
        assert it == runs[0][1] and np.array_equal(x, runs[0][0]) and np.array_equal(res, runs[0][2])
    S.close(); M.close()


# ------------------------------------------------------------------ set_blocks on the device flow of config 5
def test_device_setup_flow_into_fp32_preconditioner(pkg, ctx, orc, fem):
    """SchurSetup -> nn_pinv -> set_blocks, all on device tensors, into an fp32-stored preconditioner; against the oracle on
    the rounded host-route blocks at the bars tests/test_gpu_setup.py holds this flow to (apply 1e-7, `it` equal, x 1e-6)."""
    import torch
    api = pkg.api
    N, px, py = 60, 3, 2
    mesh = fem.get_mesh(N)
    a0, a1 = lognormal_coeff(fem, mesh.points, 1), lognormal_coeff(fem, mesh.points, 2)
    P0 = fem.build_schur_problem(N, px, py, a0, f_m1, u0734)
    P1 = fem.build_schur_problem(N, px, py, a1, f_m1, u0734)
    sub = P0.sub
    n = sub.n_Γ
    plan = fem.make_assembly_plan(mesh.cells, mesh.points, P0.epart, sub, f_m1, u0734)
    dev_plan = api.AssemblyPlan(ctx, plan)
    setup = api.SchurSetup(ctx, P0.A_IIdd, P0.A_IΓdd, P0.A_ΓΓdd)
    S = api.LocalSchurs(ctx, P0.Sd, sub.gather_idx, sub.node_Γ_cnt)
    M = nn(pkg, ctx, P0.ΠSd, sub.gather_idx, sub.node_Γ_cnt)
    vals = dev_plan.run(torch.from_numpy(a1).cuda())
    ii, ig, gg, bI, bΓ = dev_plan.block_values(vals)
    Sd, w = setup.run(ii, ig, gg, bI)
    S.set_blocks(Sd)
    Pi = api.nn_pinv(ctx, sub.n_Γd, Sd)
    M.set_blocks(Pi)
    ctx.synchronize()
    assert M.storage == "f32"
    So = orc.apply_local_schurs_operator(P1.Sd, sub.gather_idx, n)
    Mo = orc.neumann_neumann_operator(rounded(P1.ΠSd), sub.gather_idx, sub.node_Γ_cnt)
    v = np.random.default_rng(3).standard_normal(n)
    ym = M.ldiv(v)
    print(f"device flow, fp32 ΠS: apply vs oracle(rounded host blocks) {np.abs(ym - Mo * v).max() / np.abs(ym).max():.2e}")
    assert np.abs(ym - Mo * v).max() <= 1e-7 * np.abs(ym).max()
    got = api.pcg(S, P1.b_schur, np.zeros(n), M)
    want = orc.pcg(So, P1.b_schur, np.zeros(n), Mo)
    assert got[1] == want[1] and np.linalg.norm(got[0] - want[0]) <= 1e-6 * np.linalg.norm(want[0])
    # the update is a pure re-fill: equal to an operator created from the same device-made blocks
    blocks = [np.asfortranarray(B.cpu().numpy()) for B in setup.blocks(Pi)]
    M2 = nn(pkg, ctx, blocks, sub.gather_idx, sub.node_Γ_cnt)
    assert np.array_equal(M2.ldiv(v), ym)
    for op in (S, M, M2):
        op.close()


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan, 1e39, -1e39])
def test_unrepresentable_entries_are_refused(pkg, ctx, toy, bad):
    P = toy
    sub = P.sub
    blocks = [B.copy(order="F") for B in P.ΠSd]
    blocks[2][3, 1] = bad
    with pytest.raises(pkg._lib.MiError) as e:
        nn(pkg, ctx, blocks, sub.gather_idx, sub.node_Γ_cnt)
    assert e.value.code == pkg._lib.MI_ERR_BAD_ARG and "block 2" in str(e.value), str(e.value)
    # fp64 storage takes FLT_MAX-exceeding (finite) values as before; the context is still usable
    M = nn(pkg, ctx, P.ΠSd, sub.gather_idx, sub.node_Γ_cnt)
    with pytest.raises(pkg._lib.MiError) as e:
        M.set_blocks(concat(blocks))                            # host pointer: checked like creation
    assert e.value.code == pkg._lib.MI_ERR_BAD_ARG
    v = np.ones(sub.n_Γ)
    assert np.all(np.isfinite(M.ldiv(v)))
    M.close()


def test_unknown_storage_is_refused_and_creates_nothing(pkg, ctx, toy):
    import ctypes as C
    api, P = pkg.api, toy
    sub = P.sub
    g = [api._i64(a) for a in sub.gather_idx]
    nd = api._i64([a.size for a in g])
    cnt = api._i64(sub.node_Γ_cnt)
    Pb = api._blocks(P.ΠSd, 0, sub.ndom)
    i64, i64p, f64p = C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_double)
    for storage in (7, 2, -1):
        h = C.c_void_p(1)
        rc = ctx._L.mi_nn_create_stored(ctx._h, i64(sub.ndom), i64(cnt.size), nd.ctypes.data_as(i64p), api._ptrs(g, i64p),
                                        api._ptrs(Pb, f64p), cnt.ctypes.data_as(i64p), C.c_int(0), i64(0), i64(sub.ndom),
                                        C.c_int(storage), C.byref(h))
        assert rc == pkg._lib.MI_ERR_BAD_ARG and h.value is None
        assert b"storage" in ctx._L.mi_last_error()


# ------------------------------------------------------------------ multi-rank (in-process loopback)
@pytest.mark.timeout(900)
@pytest.mark.parametrize("world,shard_nn", [(2, False), (2, True), (4, False), (4, True)])
def test_in_process_ranks(pkg, orc, n200, world, shard_nn):
    """S sharded; fp32 ΠS replicated (a local operator: the folded loop, one exchange per iteration) or sharded (the
    unfolded loop: plain applies + all-reduce — DESIGN.md §6). `it` equal to the oracle, ranks bit-identical, and the
    folded-launch counter says which loop ran."""
    from test_gpu_multirank import run_ranks
    api, P = pkg.api, n200
    sub = P.sub
    n, b, ndom = sub.n_Γ, P.b_schur, sub.ndom
    gi, cnt = sub.gather_idx, sub.node_Γ_cnt

    def rank_main(ctx, r):
        lo, hi = api.shard_domains(ndom, r, world)
        S = api.LocalSchurs(ctx, [P.Sd[d] if lo <= d < hi else None for d in range(ndom)], gi, cnt, dom_slice=(lo, hi))
        if shard_nn:
            M = nn(pkg, ctx, [P.ΠSd[d] if lo <= d < hi else None for d in range(ndom)], gi, cnt, dom_slice=(lo, hi))
        else:
            M = nn(pkg, ctx, P.ΠSd, gi, cnt, dom_slice=(0, ndom))
        ctx.host_barrier.wait(timeout=300)
        f0 = ctx.query("folded_pcg")
        res = api.pcg(S, b, np.zeros(n), M)
        f1 = ctx.query("folded_pcg")
        z = M.ldiv(b)
        ctx.host_barrier.wait(timeout=300)
        return res, z, f1 - f0

    out = run_ranks(api, world, rank_main)
    for r in range(1, world):
        assert out[r][0][1] == out[0][0][1]
        assert np.array_equal(out[r][0][0], out[0][0][0]) and np.array_equal(out[r][0][2], out[0][0][2])
        assert np.array_equal(out[r][1], out[0][1])
    So = orc.apply_local_schurs_operator(P.Sd, gi, n)
    Mo = orc.neumann_neumann_operator(rounded(P.ΠSd), gi, cnt)
    assert_history(out[0][0], orc.pcg(So, b, np.zeros(n), Mo), So, b)
    z = out[0][1]
    assert np.allclose(z, Mo * b, rtol=0, atol=1e-13 * np.abs(z).max())
    for r in range(world):
        assert (out[r][2] == 0) if shard_nn else (out[r][2] > 0), (r, out[r][2])


# ------------------------------------------------------------------ tilings, each in a process of its own
_TILING_CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import __graft_entry__ as graft
from test_gpu_dense_edges import gather_maps
pkg = graft.load_package(); api = pkg.api
sizes = [1, 5, 33, 257, 513, 1025, 2048, 700]
rng = np.random.default_rng(5)
g, cnt, n = gather_maps(sizes, rng)
blocks = [np.asfortranarray(rng.standard_normal((m, m))) for m in sizes]
x = rng.standard_normal(n)
ctx = api.Context(0)
M = api.NeumannNeumannSchurPreconditioner(ctx, blocks, g, cnt, storage="f32")
print(M.apply(x).tobytes().hex())
"""


def test_tilings_give_the_same_bits():
    outs = []
    for env in ({"MI355_GEMV_RPW": "1", "MI355_GEMV_WAVES": "4"}, {"MI355_GEMV_RPW": "4", "MI355_GEMV_WAVES": "16"}, {}):
        base = {k: v for k, v in os.environ.items() if k not in ("MI355_GEMV_RPW", "MI355_GEMV_WAVES")}
        r = subprocess.run([sys.executable, "-c", _TILING_CHILD % (ROOT, os.path.join(ROOT, "tests"))], env={**base, **env},
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r.stdout.split()[-1])
    assert len(outs[0]) > 16 and outs[0] == outs[1] == outs[2]


@pytest.mark.parametrize("rpw,waves", [(1, 4), (4, 16), (4, 8)])
def test_solve_under_tiling_overrides(pkg, ctx, orc, ragged, monkeypatch, rpw, waves):
    api, P = pkg.api, ragged
    sub = P.sub
    monkeypatch.setenv("MI355_GEMV_RPW", str(rpw))
    monkeypatch.setenv("MI355_GEMV_WAVES", str(waves))
    S = api.LocalSchurs(ctx, P.Sd, sub.gather_idx, sub.node_Γ_cnt)
    M = nn(pkg, ctx, P.ΠSd, sub.gather_idx, sub.node_Γ_cnt)
    So = orc.apply_local_schurs_operator(P.Sd, sub.gather_idx, sub.n_Γ)
    Mo = orc.neumann_neumann_operator(rounded(P.ΠSd), sub.gather_idx, sub.node_Γ_cnt)
    f0 = ctx.query("folded_pcg")
    got = api.pcg(S, P.b_schur, np.zeros(sub.n_Γ), M)
    assert ctx.query("folded_pcg") > f0
    assert_history(got, orc.pcg(So, P.b_schur, np.zeros(sub.n_Γ), Mo), So, P.b_schur)
    S.close(); M.close()


# ------------------------------------------------------------------ the example
def test_example07_nn_f32(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "example07_stochastic.py"), "--nn-f32", "--N", "60",
                        "--nreals", "3", "--out", str(tmp_path / "its_{rank}.npz")], capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("nn-f32 ")]
    assert len(lines) == 2, r.stdout[-3000:]
    for ln in lines:                                              # "nn-f32 <label>: fp64 [..] fp32 [..]"
        a, b = ln.split("fp64")[1].split("fp32")
        va, vb = [int(t) for t in a.strip(" []:").split()], [int(t) for t in b.strip(" []:").split()]
        assert len(va) == len(vb) == 3
    saved = [f for _, _, fs in os.walk(tmp_path) for f in fs if "neumann-neumann-f32" in f]
    assert len(saved) == 2, saved
