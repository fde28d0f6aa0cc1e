"""GPU suite (-m gpu) of the sparse direct preconditioner (`api.SparseDirectPreconditioner`, csrc/spd_direct.hpp) at the edges
of its piece size P (MI355_SPD_PIECE, read at every create) and of its separator size |Σ|, on the cases of
spd_graphs.edge_cases() and the conditioning family spd_graphs.spd_kappa. tests/test_spd_direct_edges_cpu.py asserts on
the host that every case has the shape it is named for, so each case below reaches the branch it was written for:
|Σ| = 88 | 89 (k_sd_invert within | above the 64 KiB of LDS a kernel has without hipFuncSetAttribute), 90 | 91, 127 | 128 |
129 (one workgroup in LDS | one launch per Gauss-Jordan step), 253 (a dense-ish s on the step path), 2048 | 2049 (the
limit), P = 1 (single-node pieces), 100 (no multiple of the wave), 128 (132 KiB of LDS in k_sd_factor), an orphan Σ node
(the extra workgroup of k_sd_apply2), pieces without Σ neighbours, |Σ| = 0, n = 0 and n = 1.

Reference: SuperLU refined with long-double residuals (spd_graphs.reference = setup_synth.refined_solve, checked against
mpmath on the CPU). Right-hand sides: every unit vector for n <= 300 (the whole inverse, so that one wrong entry is not
averaged away) and one random vector; four random vectors above.

Bar (every comparison, per column): ||z - z_ref||_2 / ||z_ref||_2 <= 50 κ_2(A) m eps, m = max(P, |Σ|) the largest dense
block inverted; constant and form of test_gpu_setup_edges.py. Where the fp64 numpy copy of the algorithm
(spd_graphs.dissection_copy) itself exceeds the bar, the device may be up to 4 x the copy's error (the rule of the set-up
tests). On the host no case needs that rule: the copy stays below 1e-3 of the bar everywhere (CPU suite). The assembled
inverse is held to symmetry at the same bar, and two applies must be bit-identical.

κ ladder: κ_2 = 1e2 .. 1e10 (small margin, and D A D scaling) on grid(16) at P = 64, the |Σ| = 128 | 129 chains at P = 4,
a strip with a dense s at |Σ| = 128, the pattern of the `ragged` A_ΓΓ, and that A_ΓΓ itself with inclusions of contrast 1e6.
Create must succeed: n eps κ <= 2048 x 2.2e-16 x 1e10 < 1, so the pivot test cannot refuse these, and the copy's probe
residual is below 4 % of the certificate's bar.

Every test prints its figures (err, err / bar, asymmetry / bar) before it asserts. The device's margins are not recorded
here yet: no MI355X was available when this file was written; the host figures of the copy are in DESIGN.md §6b.
"""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT, f_m1, u0734
from test_gpu_parity import assert_history
import spd_graphs as sg

pytestmark = pytest.mark.gpu

C = 50.0
EDGES = sg.edge_cases()
SOLVED = [name for name, (A, P, shape) in EDGES.items() if shape["status"] == 0 and A.shape[0] > 0]
_REF = {}


def create(api, ctx, monkeypatch, A, P):
    """a create with MI355_SPD_PIECE = P (the variable is read at every create)"""
    monkeypatch.setenv("MI355_SPD_PIECE", str(P))
    try:
        return api.SparseDirectPreconditioner(ctx, A)
    finally:
        monkeypatch.delenv("MI355_SPD_PIECE")


def rhs(n):
    """the columns of the accuracy checks (+ one random vector behind the unit vectors)"""
    R = sg.rhs_of(n)
    return np.column_stack([R, np.random.default_rng(n).standard_normal(n)]) if n <= 300 else R


def reference(tag, A):
    """(columns, A^-1 columns, κ_2) of one matrix: computed once, shared by every test, never modified"""
    if tag not in _REF:
        R = rhs(A.shape[0])
        X = sg.reference(A, R)
        R.setflags(write=False)
        X.setflags(write=False)
        _REF[tag] = (R, X, sg.kappa2(A))
    return _REF[tag]


def col_err(Z, X):
    return np.linalg.norm(Z - X, axis=0) / np.linalg.norm(X, axis=0)


def copy_error(A, P, R, X, tmp_path):
    """largest column error of the numpy copy on the device's split (the host plan checker gives the split)"""
    import json
    exe, fn = str(tmp_path / "spd_direct_check"), str(tmp_path / "graph.txt")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "spd_direct_check.cpp")])
    sg.write_graph(fn, A)
    plan = json.loads(subprocess.run([exe, str(P), str(sg.SIGMA_MAX), fn], capture_output=True, text=True).stdout)
    return float(col_err(sg.dissection_copy(A, plan, R), X).max())


def check_accuracy(tag, M, A, P, tmp_path):
    """every column of rhs(n) through M.ldiv against the reference; symmetry of the assembled inverse; bit-identical repeats.
    Returns err / bar."""
    n = A.shape[0]
    R, X, kappa = reference(tag, A)
    Z = np.column_stack([M.ldiv(np.ascontiguousarray(R[:, j])) for j in range(R.shape[1])])
    assert np.all(np.isfinite(Z)), tag
    bar = C * kappa * max(P, M.stats[1]) * sg.EPS
    errs = col_err(Z, X)
    err = float(errs.max())
    print(f"{tag}: n {n}, (pieces, |Σ|) {M.stats}, κ {kappa:.2e}, err {err:.2e}, err / bar {err / bar:.2e} (column {int(errs.argmax())})")
    if err > bar:
        ce = copy_error(A, P, np.asarray(R), np.asarray(X), tmp_path)
        print(f"{tag}: above the bar; numpy copy err {ce:.2e}, copy / bar {ce / bar:.2e}, device / copy {err / ce:.2e}")
        assert ce > bar and err <= 4.0 * ce, (tag, err, bar, ce)
    if n <= 300:                                                            # the assembled inverse, symmetric to the same bar
        Zi = Z[:, :n]
        asym = float((np.linalg.norm(Zi - Zi.T, axis=0) / np.linalg.norm(X[:, :n], axis=0)).max())
        print(f"{tag}: asymmetry / bar {asym / bar:.2e}")
        assert asym <= bar, (tag, asym, bar)
    last = np.ascontiguousarray(R[:, -1])
    assert np.array_equal(M.ldiv(last), Z[:, -1]) and np.array_equal(M.ldiv(last), Z[:, -1]), tag
    return err / bar


# ------------------------------------------------------------------ applies at every edge
@pytest.mark.parametrize("name", SOLVED)
def test_edge_case_applies(pkg, ctx, monkeypatch, tmp_path, name):
    A, P, shape = EDGES[name]
    M = create(pkg.api, ctx, monkeypatch, A, P)
    assert M.stats == (shape["pieces"], shape["sigma"]), (name, M.stats)
    check_accuracy(name, M, A, P, tmp_path)


# ------------------------------------------------------------------ κ ladder
def _ladder(fem, gname, kind):
    if gname == "ragged":
        G, P = sg.ragged_gg(fem, f_m1, u0734, contrast=1.0), 64
    else:
        G, P = sg.LADDER_GRAPHS[gname]
    return [(f"{gname} {kind} κ={t:g}", sg.spd_kappa(G, t, seed=3, kind=kind), P) for t in sg.KAPPAS]


@pytest.mark.parametrize("kind", ["margin", "scaling"])
@pytest.mark.parametrize("gname", list(sg.LADDER_GRAPHS) + ["ragged"])
def test_kappa_ladder(pkg, ctx, fem, monkeypatch, tmp_path, gname, kind):
    """κ_2 = 1e2 .. 1e10: create succeeds (neither the pivot test nor the certificate refuses an SPD matrix of κ <= 1e10)
    and every solve is within the bar"""
    worst = 0.0
    for tag, A, P in _ladder(fem, gname, kind):
        try:
            M = create(pkg.api, ctx, monkeypatch, A, P)
        except pkg.api.MiError as e:
            raise AssertionError(f"{tag}: create refused an SPD matrix of κ {sg.kappa2(A):.2e}: {e}") from e
        worst = max(worst, check_accuracy(tag, M, A, P, tmp_path))
    print(f"κ ladder {gname} {kind}: largest err / bar {worst:.2e}")


def test_fem_contrast_1e6(pkg, ctx, fem, monkeypatch, tmp_path):
    """the `ragged` A_ΓΓ with inclusions of contrast 1e6 (κ_2 = 3.7e6), at the default P and at P = 8 (a larger Σ)"""
    A = sg.ragged_gg(fem, f_m1, u0734, contrast=1e6)
    for P in (64, 8):
        M = create(pkg.api, ctx, monkeypatch, A, P)
        check_accuracy("ragged contrast 1e6", M, A, P, tmp_path)


# ------------------------------------------------------------------ limits and refusals
def test_limits_are_bad_arg_and_leave_the_context_healthy(pkg, ctx, monkeypatch):
    """|Σ| = 2049 and MI355_SPD_PIECE = 0 | 129 are MI_ERR_BAD_ARG; an operator made before still answers bit-identically and
    a create after them works"""
    api, L = pkg.api, pkg._lib
    A, P, _ = EDGES["spider_P1"]
    M = create(api, ctx, monkeypatch, A, P)
    r = np.random.default_rng(1).standard_normal(A.shape[0])
    z = M.ldiv(r)
    big, Pb, shape = EDGES["chain4099_P1"]
    assert shape["sigma"] == sg.SIGMA_MAX + 1
    with pytest.raises(api.MiError) as e:
        create(api, ctx, monkeypatch, big, Pb)
    assert e.value.code == L.MI_ERR_BAD_ARG and "2049" in str(e.value) and "2048" in str(e.value)
    for bad in (0, 129):
        with pytest.raises(api.MiError) as e:
            create(api, ctx, monkeypatch, A, bad)
        assert e.value.code == L.MI_ERR_BAD_ARG, bad
    assert np.array_equal(M.ldiv(r), z)
    assert np.array_equal(create(api, ctx, monkeypatch, A, P).ldiv(r), z)


def test_n0(pkg, ctx, monkeypatch):
    """n = 0: create, set_values of an empty array and ldiv of an empty vector return without error"""
    A, P, _ = EDGES["n0_P64"]
    M = create(pkg.api, ctx, monkeypatch, A, P)
    assert M.n == 0 and M.stats == (0, 0)
    M.set_values(np.zeros(0))
    z = M.ldiv(np.zeros(0))
    assert z.shape == (0,)


def _rescaled(A, seed):
    """D A D with a positive diagonal D: still SPD, the same stored pattern"""
    A = sp.csc_matrix(A)
    d = 1.0 + 0.3 * np.random.default_rng(seed).random(A.shape[0])
    A2 = A.copy()
    A2.data = A.data * d[A.indices] * np.repeat(d, np.diff(A.indptr))
    return A2


@pytest.mark.parametrize("pair", ["sigma 128 then 100 at P 4", "P 128 then P 64 with sigma 102"])
def test_two_live_operators(pkg, ctx, monkeypatch, pair):
    """Operator A needs 132 KiB of dynamic LDS (k_sd_invert at |Σ| = 128, or k_sd_factor at P = 128); operator B, created
    later, needs less but more than 64 KiB, so its create lowers hipFuncAttributeMaxDynamicSharedMemorySize of the kernels
    (the attribute belongs to the function). A.set_values then launches with more than the last value set: it must give
    the bits of a fresh create on the same values, and so must B.set_values."""
    api = pkg.api
    if pair.startswith("sigma"):
        (A, PA, _), B, PB = EDGES["chain516_P4"], sg.spd_from_graph(sg.chain(404), 404), 4
        want_b = 100
    else:
        (A, PA, _), B, PB = EDGES["grid16_P128"], sg.spd_from_graph(sg.grid(26), 26), 64
        want_b = 102
    MA = create(api, ctx, monkeypatch, A, PA)
    MB = create(api, ctx, monkeypatch, B, PB)
    assert MB.stats[1] == want_b and 65536 < sg.sd_lds_bytes(want_b) < sg.sd_lds_bytes(max(PA, MA.stats[1])) == sg.sd_lds_bytes(sg.P_MAX)
    A2, B2 = _rescaled(A, 1), _rescaled(B, 2)
    ra, rb = np.random.default_rng(3).standard_normal(A.shape[0]), np.random.default_rng(4).standard_normal(B.shape[0])
    MA.set_values(A2.data)                                                  # B's create was the last to set the attribute
    za = MA.ldiv(ra)
    MB.set_values(B2.data)
    zb = MB.ldiv(rb)
    fresh_b = create(api, ctx, monkeypatch, B2, PB).ldiv(rb)
    fresh_a = create(api, ctx, monkeypatch, A2, PA).ldiv(ra)
    assert np.array_equal(za, fresh_a) and np.array_equal(zb, fresh_b)
    MB.set_values(B.data)                                                   # and after A's fresh create raised it again
    assert np.array_equal(MB.ldiv(rb), create(api, ctx, monkeypatch, B, PB).ldiv(rb))
    want = sg.reference(A2, ra)
    assert np.linalg.norm(za - want) <= C * sg.kappa2(A2) * max(PA, MA.stats[1]) * sg.EPS * np.linalg.norm(want)


@pytest.mark.parametrize("name", ["chain517_P4", "spider_P1"])
def test_refused_set_values_keeps_the_factor(pkg, ctx, monkeypatch, name):
    """an indefinite set_values (a diagonal entry negated: in a piece, in Σ, the orphan hub) raises SingularException on the
    step path of s^-1 and in the orphan case, and the previous factor still answers bit-identically"""
    api = pkg.api
    A, P, _ = EDGES[name]
    n = A.shape[0]
    M = create(api, ctx, monkeypatch, A, P)
    r = np.random.default_rng(5).standard_normal(n)
    z = M.ldiv(r)
    for node in sorted({0, 3, n // 2, n - 1}):
        bad = sp.csc_matrix(A).copy()
        dg = bad.diagonal()
        dg[node] = -dg[node]
        bad.setdiag(dg)
        assert np.array_equal(bad.indptr, A.indptr) and np.array_equal(bad.indices, A.indices)
        with pytest.raises(api.SingularException):
            M.set_values(bad.data)
        assert np.array_equal(M.ldiv(r), z), (name, node)
        with pytest.raises(api.SingularException):
            create(api, ctx, monkeypatch, bad, P)
    M.set_values(A.data)
    assert np.array_equal(M.ldiv(r), z)


# ------------------------------------------------------------------ one solve per new branch
@pytest.mark.parametrize("name", ["spider_P1", "chain517_P4"])
def test_pcg_on_the_new_branches(pkg, ctx, orc, monkeypatch, name):
    """pcg(S, b, 0, M) with S the matrix itself as SparseMatrixCSC and M its sparse direct factor (the orphan workgroup; the
    step path of s^-1) against the oracle under assert_history; a chunked (graph-replayed) run == an eager one, bit for bit"""
    api = pkg.api
    A, P, _ = EDGES[name]
    n = A.shape[0]
    S, So = api.SparseMatrixCSC(ctx, A), orc.csc_operator(A)
    M = create(api, ctx, monkeypatch, A, P)
    Mo = orc.neumann_neumann_operator([np.asfortranarray(np.linalg.inv(A.toarray()))], [np.arange(n)], np.ones(n, dtype=np.int64))
    b = np.random.default_rng(6).standard_normal(n)
    x0 = np.zeros(n)
    try:
        ctx.set_chunk(0)
        eager = api.pcg(S, b, x0, M)
        ctx.set_chunk(4)
        replay = api.pcg(S, b, x0, M)
    finally:
        ctx.set_chunk(8)
    want = orc.pcg(So, b, x0, Mo)
    print(f"{name}: it {eager[1]} (oracle {want[1]}), res {eager[2]}")
    assert_history(eager, want, apply=So, b=b)
    assert eager[1] == replay[1] and np.array_equal(eager[0], replay[0]) and np.array_equal(eager[2], replay[2])
