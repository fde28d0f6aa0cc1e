"""GPU suite of the device Neumann-Neumann induced preconditioner `api.NeumannNeumannInducedPreconditioner`
(`mi_nn_induced_*`): the M of `defpcg(A, b, ϕ, M=ΠA_induced_nn_local_mat)` and `pcg(A, b, M=ΠA_induced_nn_local_mat)`
(Example03:300-319). Applies against the refined host restatement of `apply_neumann_neumann_induced`
(tests/nn_induced_ref.py) at the project's bar for the device's exact elimination against the host (relative 2-norm 1e-10,
DESIGN §3; the bar of §6c, not derived for this operator); the bits of the Neumann-Neumann stage against the existing
operator; determinism; index base and coupling switch; new realizations; the solvers against the oracle with the dense
restated M^-1 as its preconditioner; the error returns; the example's `--nn-induced` leg.

Measured margins of the apply test (MI355X, worst case over all inputs and variants): see DESIGN §6d."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, lognormal_coeff, lowest_eigvecs
from test_gpu_lorasc import _assert_solve, _csc_data
import nn_induced_ref as nr

pytestmark = pytest.mark.gpu

APPLY_BAR = 1e-10
STORAGES = ("f64", "f32")


@pytest.fixture(scope="module")
def cases(fem):
    return nr.nni_cases(fem)


def _setup(pkg, ctx, c):
    P = c.P
    setup = pkg.api.SchurSetup(ctx, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd)
    setup.keep_levels()
    setup.run()
    return setup


def _device(pkg, ctx, fem, c, storage="f64", coupling="reference", index_base=0, setup=None, ΠSd=None):
    P = c.P
    return pkg.api.NeumannNeumannInducedPreconditioner(
        ctx, P.A_IΓdd, (c.pos_I, c.pos_Γ), P.sub.gather_idx, P.sub.node_Γ_cnt, nr.prepare(fem, c) if ΠSd is None else ΠSd,
        setup or _setup(pkg, ctx, c), storage=storage, coupling=coupling, index_base=index_base)


def _blocks_for(fem, c, storage):
    ΠSd = nr.prepare(fem, c)
    return nr.rounded_f32(ΠSd) if storage == "f32" else ΠSd


@pytest.mark.parametrize("name", nr.GPU_CASES)
def test_apply_against_refined_restatement(pkg, ctx, fem, cases, name):
    """random r, both couplings, both storages: relative 2-norm error <= 1e-10 against the refined restatement (on the
    fp32-rounded blocks for f32 storage); two applies bit-identical; host and device pointers bit-identical. The inputs
    cover the kernels' edges: n_Γ mod 256 = 1, 0, 255, the empty hub column with multiplicity 5, the strip, a full and a
    one-row last GEMV tile."""
    import torch
    c = cases[name]
    r = nr.apply_input(c)
    setup = _setup(pkg, ctx, c)
    worst = 0.0
    for storage in STORAGES:
        M = _device(pkg, ctx, fem, c, storage, setup=setup)
        for cpl in nr.COUPLINGS:
            M.set_coupling(cpl)
            want = nr.apply_neumann_neumann_induced(c, _blocks_for(fem, c, storage), r, cpl, refine=2)
            got = M.ldiv(r)
            err = np.linalg.norm(got - want) / np.linalg.norm(want)
            worst = max(worst, err)
            print(f"nn-induced apply {name}: n = {c.n}, n_Γ = {c.n_Γ}, storage = {storage}, coupling = {cpl}: "
                  f"rel. error {err:.3e} (bar {APPLY_BAR:.0e}, margin {APPLY_BAR / max(err, 1e-300):.1f}x)")
            assert err <= APPLY_BAR, (name, storage, cpl, err)
            assert np.array_equal(M.ldiv(r), got), (name, storage, cpl)
            dev = pkg.api.apply_neumann_neumann_induced(M, torch.from_numpy(r).cuda()).cpu().numpy()
            assert np.array_equal(dev, got), (name, storage, cpl)
        M.close()
    print(f"nn-induced apply {name}: worst rel. error {worst:.3e}")


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("name", ["ragged", "unstructured", "tile_one"])
def test_nn_stage_bits(pkg, ctx, fem, cases, name, storage):
    """r_I = 0: every column sum is +0 and r_schur = r_Γ exactly, so z[pos_Γ] carries the bits of the existing
    Neumann-Neumann operator's ldiv(r_Γ) on the same ΠS_d and storage; z[pos_I] matches the restatement in the same run"""
    api = pkg.api
    c = cases[name]
    sub = c.P.sub
    r = np.zeros(c.n)
    r[c.pos_Γ] = np.random.default_rng(9).standard_normal(c.n_Γ)
    Πnn = api.NeumannNeumannSchurPreconditioner(ctx, nr.prepare(fem, c), sub.gather_idx, sub.node_Γ_cnt, storage=storage)
    want_Γ = Πnn.ldiv(r[c.pos_Γ])
    M = _device(pkg, ctx, fem, c, storage)
    for cpl in nr.COUPLINGS:
        M.set_coupling(cpl)
        z = M.ldiv(r)
        assert np.array_equal(z[c.pos_Γ], want_Γ), (name, storage, cpl)
        want = nr.apply_neumann_neumann_induced(c, _blocks_for(fem, c, storage), r, cpl, refine=2)
        for d, p in enumerate(c.pos_I):
            assert np.linalg.norm(z[p] - want[p]) <= APPLY_BAR * np.linalg.norm(want), (name, storage, cpl, d)


def test_index_base_one_and_coupling_switch(pkg, ctx, fem, cases):
    """index_base 1 == index_base 0; set_coupling == a create with that coupling; bit for bit. bytes(): the two level solves
    dominate"""
    c = cases["micro"]
    r = nr.apply_input(c, 1)
    setup = _setup(pkg, ctx, c)
    M0 = _device(pkg, ctx, fem, c, setup=setup)
    Mb = _device(pkg, ctx, fem, c, index_base=1, setup=setup)
    Ma = _device(pkg, ctx, fem, c, coupling="assembled", setup=setup)
    z_ref, z_asm = M0.ldiv(r), Ma.ldiv(r)
    assert not np.array_equal(z_ref, z_asm)
    assert np.array_equal(Mb.ldiv(r), z_ref)
    M0.set_coupling("assembled")
    assert M0.coupling == "assembled" and np.array_equal(M0.ldiv(r), z_asm)
    M0.set_coupling("reference")
    assert np.array_equal(M0.ldiv(r), z_ref)
    a, d = M0.bytes()
    assert a > 2 * d > 0


@pytest.mark.parametrize("storage", STORAGES)
def test_new_realization_equals_fresh_create(pkg, ctx, fem, cases, storage):
    """plan re-run + set_values + set_blocks == a fresh create on the second coefficient of `ragged`, bit for bit; and back
    again through device pointers"""
    import torch
    c1 = cases["ragged"]
    c2 = nr.make_case(fem, "ragged2", 50, 3, 2, lognormal_coeff(fem, c1.P.mesh.points, 8))
    r = nr.apply_input(c2)
    Π1, Π2 = nr.prepare(fem, c1), nr.prepare(fem, c2)
    fresh = _device(pkg, ctx, fem, c2, storage, "assembled").ldiv(r)
    want = nr.apply_neumann_neumann_induced(c2, _blocks_for(fem, c2, storage), r, "assembled", refine=2)
    assert np.linalg.norm(fresh - want) <= APPLY_BAR * np.linalg.norm(want)
    M = _device(pkg, ctx, fem, c1, storage, "assembled")
    before = M.ldiv(r)
    assert not np.array_equal(before, fresh)
    P1, P2 = c1.P, c2.P
    M.setup.run(_csc_data(P2.A_IIdd), _csc_data(P2.A_IΓdd), _csc_data(P2.A_ΓΓdd))
    M.set_values(_csc_data(P2.A_IΓdd))
    M.set_blocks(np.concatenate([B.ravel(order="F") for B in Π2]))
    assert np.array_equal(M.ldiv(r), fresh)
    M.setup.run(_csc_data(P1.A_IIdd), _csc_data(P1.A_IΓdd), _csc_data(P1.A_ΓΓdd))
    M.set_values(torch.from_numpy(_csc_data(P1.A_IΓdd)).cuda())
    M.set_blocks(torch.from_numpy(np.concatenate([B.ravel(order="F") for B in Π1])).cuda())
    assert np.array_equal(M.ldiv(r), before)


def _oracle_M(orc, c, ΠSd, cpl):
    Minv = nr.dense_minv(c, ΠSd, cpl)
    return orc.neumann_neumann_operator([Minv], [np.arange(c.n)], np.ones(c.n, dtype=np.int64))


# assembled coupling on the four solver inputs; as written on strip only: on the others CG with the as-written operator does
# not converge, or runs nonsymmetric for 40+ iterations, and iteration parity there would test rounding, not the code
SOLVES = [("micro", "assembled"), ("ragged", "assembled"), ("unstructured", "assembled"), ("strip", "assembled"),
          ("strip", "reference")]


@pytest.mark.parametrize("name,cpl", SOLVES)
def test_pcg_and_defpcg_against_oracle(pkg, ctx, orc, fem, cases, name, cpl):
    """pcg(A, b, 0, M) and defpcg(A, b, 0, ϕ, M), ϕ = the ndom + 10 least dominant eigenvectors of A (Example03:310-317),
    against the oracle with the dense restated M^-1; a solve replayed from graphs == the eager solve, bit for bit"""
    api = pkg.api
    c = cases[name]
    ΠSd = nr.prepare(fem, c)
    A, Ao = api.SparseMatrixCSC(ctx, c.A), orc.csc_operator(c.A)
    Mo = _oracle_M(orc, c, ΠSd, cpl)
    x0 = np.zeros(c.n)
    M = _device(pkg, ctx, fem, c, coupling=cpl)
    _assert_solve(api.pcg(A, c.b, x0, M), orc.pcg(Ao, c.b, x0, Mo), Ao, c.b)
    ϕ = lowest_eigvecs(Ao, c.n, len(c.A_IId) + 10)
    _assert_solve(api.defpcg(A, c.b, x0, ϕ, M), orc.defpcg(Ao, c.b, x0, ϕ, Mo), Ao, c.b)
    try:
        ctx.set_chunk(0)
        eager = api.pcg(A, c.b, x0, M)
        ctx.set_chunk(4)
        replay = api.pcg(A, c.b, x0, M)
        ctx.set_chunk(8)
        replay8 = api.pcg(A, c.b, x0, M)
    finally:
        ctx.set_chunk(0)
    for rep in (replay, replay8):
        assert eager[1] == rep[1] and np.array_equal(eager[0], rep[0]) and np.array_equal(eager[2], rep[2])


def test_pcg_f32_storage_against_oracle(pkg, ctx, orc, fem, cases):
    """f32 storage on micro, assembled: `it` equal to the oracle's with the fp32-rounded blocks"""
    api = pkg.api
    c = cases["micro"]
    A, Ao = api.SparseMatrixCSC(ctx, c.A), orc.csc_operator(c.A)
    x0 = np.zeros(c.n)
    M = _device(pkg, ctx, fem, c, "f32", "assembled")
    assert M.storage == "f32"
    want = orc.pcg(Ao, c.b, x0, _oracle_M(orc, c, _blocks_for(fem, c, "f32"), "assembled"))
    got = api.pcg(A, c.b, x0, M)
    print(f"f32 storage: it = {got[1]} (oracle {want[1]})")
    assert got[1] == want[1]


def test_errors_do_not_fault(pkg, ctx, fem, cases):
    """every MI_ERR_BAD_ARG of mi_nn_induced_create returns the code and a message; a bound plan cannot be destroyed or
    un-kept, and the operator still applies to the same bits; a LORASC operator and an induced operator on one plan"""
    api, L = pkg.api, pkg._lib
    c = cases["micro"]
    P, sub = c.P, c.P.sub
    ΠSd = nr.prepare(fem, c)
    M = _device(pkg, ctx, fem, c)
    setup = M.setup
    r = nr.apply_input(c, 2)
    z = M.ldiv(r)
    maps = (c.pos_I, c.pos_Γ)

    def refused(A_IΓdd=P.A_IΓdd, maps=maps, gather=sub.gather_idx, cnt=sub.node_Γ_cnt, blocks=ΠSd, plan=setup, ctx_=ctx, **kw):
        with pytest.raises(api.MiError) as e:
            api.NeumannNeumannInducedPreconditioner(ctx_, A_IΓdd, maps, gather, cnt, blocks, plan, **kw)
        assert e.value.code == L.MI_ERR_BAD_ARG and len(str(e.value)) > 40
        return str(e.value)

    dup = [p.copy() for p in c.pos_I]
    dup[1][0] = dup[0][0]
    assert "permutation" in refused(maps=(dup, c.pos_Γ))
    far = c.pos_Γ.copy()
    far[3] = c.n
    msg = refused(maps=(c.pos_I, far))
    assert "out of range" in msg and str(c.n) in msg
    # n != Σ n_i + n_gamma and an n_i that differs from the plan's: one interior node moved / dropped
    moved = [np.r_[c.pos_I[0], c.pos_I[1][:1]], c.pos_I[1][1:]] + list(c.pos_I[2:])
    assert "n_i" in refused(maps=(moved, c.pos_Γ))
    lib = L.load()
    assert "n_gamma" in _raw_create_with_n(pkg, ctx, c, ΠSd, setup, c.n + 1)
    # n_gamma_d that differs from the plan's: the last interface node of subdomain 0 dropped everywhere it shows
    g_short = [np.asarray(sub.gather_idx[0])[:-1]] + [np.asarray(g) for g in sub.gather_idx[1:]]
    b_short = [np.asfortranarray(ΠSd[0][:-1, :-1])] + list(ΠSd[1:])
    a_short = [P.A_IΓdd[0][:, :-1]] + list(P.A_IΓdd[1:])
    assert "n_gamma_d" in refused(A_IΓdd=a_short, gather=g_short, blocks=b_short)
    other = api.Context(0)
    assert "another context" in refused(ctx_=other)
    other.close()
    plain = api.SchurSetup(ctx, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd)
    assert "level" in refused(plan=plain)
    plain.keep_levels()                                   # kept, but no run after it
    assert "level" in refused(plan=plain)
    g_far = [np.asarray(g).copy() for g in sub.gather_idx]
    g_far[2][1] = c.n_Γ
    msg = refused(gather=g_far)
    assert "gather_idx" in msg and str(c.n_Γ) in msg
    cnt_bad = np.asarray(sub.node_Γ_cnt).copy()
    cnt_bad[5] += 1
    msg = refused(cnt=cnt_bad)
    assert "node_gamma_cnt[5]" in msg and str(int(cnt_bad[5])) in msg
    assert "storage 7" in refused(storage=7)
    assert "coupling 9" in refused(coupling=9)
    with pytest.raises(api.MiError) as e:
        M.set_coupling(9)
    assert e.value.code == L.MI_ERR_BAD_ARG and "coupling 9" in str(e.value)
    # the bound plan
    assert lib.mi_schur_setup_destroy(setup._h) == L.MI_ERR_BAD_ARG and b"Neumann-Neumann induced" in lib.mi_last_error()
    assert lib.mi_schur_setup_keep_levels(setup._h, 0) == L.MI_ERR_BAD_ARG and b"Neumann-Neumann induced" in lib.mi_last_error()
    assert np.array_equal(M.ldiv(r), z)
    # a LORASC operator on the same plan: the plan is free only after both are closed
    gg = api.SparseDirectPreconditioner(ctx, c.A_ΓΓ)
    Lo = api.LorascPreconditioner(ctx, c.A_IΓd, maps, setup, gg)
    assert lib.mi_schur_setup_destroy(setup._h) == L.MI_ERR_BAD_ARG and b"LORASC" in lib.mi_last_error()
    M.close()
    assert lib.mi_schur_setup_destroy(setup._h) == L.MI_ERR_BAD_ARG and b"LORASC" in lib.mi_last_error()
    M2 = _device(pkg, ctx, fem, c, setup=setup)
    Lo.close()
    assert lib.mi_schur_setup_destroy(setup._h) == L.MI_ERR_BAD_ARG and b"Neumann-Neumann induced" in lib.mi_last_error()
    assert np.array_equal(M2.ldiv(r), z)
    M2.close()
    assert lib.mi_schur_setup_destroy(setup._h) == 0
    setup._h = None


def _raw_create_with_n(pkg, ctx, c, ΠSd, setup, n):
    """mi_nn_induced_create through ctypes with an n that is not Σ n_i + n_gamma (the Python class computes n itself)"""
    import ctypes as C
    api, L = pkg.api, pkg._lib
    P, sub = c.P, c.P.sub
    ndom = len(P.A_IΓdd)
    n_i = api._i64([len(p) for p in c.pos_I])
    pI = [api._i64(p) for p in c.pos_I]
    pΓ = api._i64(c.pos_Γ)
    g = [api._i64(a) for a in sub.gather_idx]
    nd = api._i64([a.size for a in g])
    cnt = api._i64(sub.node_Γ_cnt)
    blocks = api._blocks(ΠSd, 0, ndom)
    igp, igi, igv = api._csc_parts(P.A_IΓdd, 0, ndom, 0)
    h = L.vp()
    rc = ctx._L.mi_nn_induced_create(
        ctx._h, L.i64(ndom), L.i64(n), L.i64(pΓ.size), nd.ctypes.data_as(L.i64p), n_i.ctypes.data_as(L.i64p),
        api._ptrs(pI, L.i64p), pΓ.ctypes.data_as(L.i64p), api._ptrs(g, L.i64p), cnt.ctypes.data_as(L.i64p),
        api._ptrs(igp, L.i64p), api._ptrs(igi, L.i64p), api._ptrs(igv, L.f64p), api._ptrs(blocks, L.f64p), C.c_int(0), setup._h,
        C.c_int(0), C.c_int(0), C.byref(h))
    msg = ctx._L.mi_last_error().decode()
    assert rc == L.MI_ERR_BAD_ARG and not h.value and len(msg) > 40 and str(n) in msg
    return msg


def test_multi_rank_context_is_refused(pkg, ctx, fem, cases):
    """a context that is one rank of several gets MI_ERR_BAD_ARG before anything else is looked at: the operator is
    replicated only (host-rendezvous loopback group: joining it needs no second rank)"""
    api, L = pkg.api, pkg._lib
    c = cases["strip"]
    grp = api.LoopbackGroup(2)
    grp.set_mode(1)
    rank0 = api.Context(0)
    rank0.loopback_init(grp, 0)
    setup = _setup(pkg, ctx, c)
    P = c.P
    with pytest.raises(api.MiError) as e:
        api.NeumannNeumannInducedPreconditioner(rank0, P.A_IΓdd, (c.pos_I, c.pos_Γ), P.sub.gather_idx, P.sub.node_Γ_cnt,
                                                nr.prepare(fem, c), setup)
    assert e.value.code == L.MI_ERR_BAD_ARG and "rank 0 of 2" in str(e.value) and len(str(e.value)) > 40
    setup.close()
    rank0.close()


def test_example03_nn_induced_leg(orc, fem, cases):
    """examples/example03_domain_decomposition.py --N 40 --nn-induced assembled: exit 0 and the printed `it` of pcg and
    defpcg equal the oracle's (5 and 5)"""
    c = cases["micro"]
    ΠSd = nr.prepare(fem, c)
    Ao = orc.csc_operator(c.A)
    Mo = _oracle_M(orc, c, ΠSd, "assembled")
    x0 = np.zeros(c.n)
    want_pcg = orc.pcg(Ao, c.b, x0, Mo)[1]
    want_def = orc.defpcg(Ao, c.b, x0, lowest_eigvecs(Ao, c.n, len(c.A_IId) + 10), Mo)[1]
    assert (want_pcg, want_def) == (5, 5)
    cmd = [sys.executable, os.path.join(ROOT, "examples", "example03_domain_decomposition.py"), "--N", "40",
           "--nn-induced", "assembled"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    m = re.search(r"nn-induced-pcg: n = (\d+), ndom = 4, coupling = assembled, iter = (\d+)", res.stdout)
    md = re.search(r"nn-induced-defpcg: n = (\d+), ndom = 4, .*coupling = assembled, iter = (\d+)", res.stdout)
    assert m and md, res.stdout[-2000:]
    assert int(m.group(1)) == c.n and int(m.group(2)) == want_pcg and int(md.group(2)) == want_def, (m.groups(), md.groups())
