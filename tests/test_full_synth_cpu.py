"""Host assertions that tests/test_gpu_full_synth_edges.py relies on (no GPU): every case of tests/full_synth.py has the
shape it is named for, so the GPU file's parametrisation reaches the branch it was written for; the two restatements it
compares against are 100 x more accurate than its bar on these inputs; and the one solver case is SPD, short, decided and
insensitive to the summation order, so that `it` equal and the strict history row say something about the device code.

  * block sizes, slot width, `nwg`, n_Γ mod 256, the two maps a permutation, A_IΓd the scattered A_IΓdd;
  * the tile list of every RPW x WAVES tiling in both storages from csrc/dense_tiles.hpp through
    tests/cpp/dense_tiles_check.cpp: tile counts, one-row / one-short / full last tiles at every tile height, the row strides
    of `panels` and which of its blocks reach the second operand panel;
  * every ladder interior: two or three levels of 3 ... 40 nodes, κ(A_IId) <= 1e4; a block with level 0 >= 3 n_Γd and one with
    level 0 < n_Γd / 4 in every case;
  * the empty `gseg` range and the n_i = 0 subdomain of `bare`; one and six column segments (`w1`, `hub6`);
  * restatement noise (refine 2 against refine 3) < 1e-12;
  * `solve`: A SPD, the assembled dense M^-1 symmetric to 1e-13 and positive definite, oracle `pcg` / `defpcg` within 50
    iterations, the last two residuals >= 1e-4 from tol, the oracle within 1 % of the history bar of a numpy PCG with
    pairwise sums, `it` equal — on the fp64 blocks and on the fp32-rounded ones.
Measured: κ(A_IId) <= 54; restatement noise <= 4.8e-16; `solve`: n = 1242, κ(A) = 28, M^-1 symmetric to 2.0e-15 (3.1e-14 on
the rounded blocks) with smallest eigenvalue 0.067, 7 iterations for both solvers in both storages against 35 of plain CG,
residuals 0.86 / 0.90 tol and 7.7 / 9.9 tol at the stop, numpy against the oracle <= 2.7e-6 of the bar."""
import json
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import lowest_eigvecs
import full_synth as fs
import krylov_synth as ks
import lorasc_ref as lr
import nn_induced_ref as nr
import setup_synth as ssy
import shard_synth as ss

NOISE_BAR = 1e-12


@pytest.fixture(scope="module", autouse=True)
def forget_cases():
    yield
    fs.drop()                                                    # `panels` holds 130 MB of blocks


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return ss.build_checker(tmp_path_factory.mktemp("dense_tiles"))


def test_tables_cover_the_issue():
    assert fs.TILE_SIZES == (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
    assert fs.PANEL_SIZES[:4] == (2032, 2033, 2048, 2049) and len(fs.PANEL_SIZES) == 7 and max(fs.PANEL_SIZES[4:]) < 256
    assert fs.WG_REMAINDERS == (1, 63, 64, 65, 128, 192, 193, 255, 256)
    assert fs.NEV_ALL == (0, 1, 2, 3, 4, 5, 255, 256, 257, 1024) and fs.LO_MAX_NEV == 1024
    assert sorted(fs.TILINGS) == sorted((r, w) for r in (1, 2, 4) for w in (4, 8, 16))
    assert {r * w for r, w in fs.TILINGS} == {4, 8, 16, 32, 64}
    assert set(fs.ALL_CASES) == {"tiles", "panels", "w1", "w3", "hub6", "bare", "solve"} | {f"wg{r}" for r in fs.WG_REMAINDERS}


@pytest.mark.parametrize("name", fs.ALL_CASES)
def test_case_has_the_shape_it_is_named_for(name):
    c = fs.case(name)
    sub, P = c.P.sub, c.P
    sizes, n_Γ, width, _ = fs._TABLE[name]
    g, cnt = sub.gather_idx, np.asarray(sub.node_Γ_cnt)
    # maps: exact n_Γ, exact multiplicity (what mi_nn_induced_create checks), node 0 in `width` blocks
    assert c.sizes == list(sizes) and c.n_Γ == n_Γ == cnt.size and sub.ndom == len(sizes)
    assert all(np.unique(a).size == a.size and a.min() >= 0 and a.max() < n_Γ for a in g)
    assert np.array_equal(np.bincount(np.concatenate(g), minlength=n_Γ), cnt) and cnt.min() >= 1
    assert int(cnt.max()) == width == c.width and int(cnt[0]) == width
    assert c.slot_width == (4 if width == 3 else width)
    # the two maps: a random interleaved permutation of the rows
    both = np.concatenate(list(c.pos_I) + [c.pos_Γ])
    assert np.array_equal(np.sort(both), np.arange(c.n)) and c.n == sum(c.n_i) + n_Γ == c.A.shape[0] == c.b.size
    assert not np.array_equal(both, np.arange(c.n)) and np.any(np.diff(c.pos_Γ) < 0) and c.pos_Γ.min() < sum(c.n_i)
    # blocks: shapes, Γ-global columns = the local ones scattered through the gather list
    for d in range(sub.ndom):
        assert P.A_IIdd[d].shape == (c.n_i[d],) * 2 and P.A_IΓdd[d].shape == (c.n_i[d], sizes[d]) and P.A_ΓΓdd[d].shape == (sizes[d],) * 2
        assert c.A_IΓd[d].shape == (c.n_i[d], n_Γ) and c.A_IΓd[d].nnz == P.A_IΓdd[d].nnz
        assert abs(sp.csc_matrix(c.A_IΓd[d])[:, g[d]] - P.A_IΓdd[d]).sum() == 0.0
    assert c.A_ΓΓ.shape == (n_Γ, n_Γ) and abs(c.A_ΓΓ - c.A_ΓΓ.T).max() == 0.0
    # ladders: tiny interiors in the regime of §3's exact-elimination bar
    dense_cols = sparse_cols = False
    for d in range(sub.ndom):
        w = c.widths[d]
        if not w:
            assert c.n_i[d] == 0
            continue
        assert [len(l) for l in ssy.bfs_levels(P.A_IIdd[d], P.A_IΓdd[d])] == w and sum(w) == c.n_i[d]
        assert 2 <= len(w) <= 3 and all(3 <= v <= 40 for v in w)
        assert np.linalg.cond(P.A_IIdd[d].toarray()) <= 1e4
        if not (name == "bare" and g[d][-1] == fs.BARE_NODE):   # the interior sees the last row's z_loc: a tile-edge guard shows
            assert np.diff(sp.csc_matrix(P.A_IΓdd[d]).indptr)[-1] > 0
        dense_cols |= w[0] >= 3 * sizes[d]
        sparse_cols |= w[0] < sizes[d] / 4
    assert dense_cols and sparse_cols
    per_col = np.concatenate([np.diff(sp.csc_matrix(B).indptr) for B in P.A_IΓdd])
    assert per_col.max() >= 2 and np.count_nonzero(per_col == 0) > per_col.size / 2
    # the partial dots and the Γ loops: workgroups of 256
    assert c.nwg == -(-n_Γ // 256)
    seg = fs.column_segments(c)
    if name != "bare" and width > 1:
        assert seg[0] == width                                  # the hub's column holds an entry in every block that holds it
    if name.startswith("wg"):
        r = int(name[2:])
        assert n_Γ == 768 + r and n_Γ % 256 == r % 256 and c.nwg == 4
        lanes = [int(np.clip((n_Γ - 768) - 64 * j, 0, 64)) for j in range(4)]     # valid lanes of the last workgroup's four terms
        assert lanes == {1: [1, 0, 0, 0], 63: [63, 0, 0, 0], 64: [64, 0, 0, 0], 65: [64, 1, 0, 0], 128: [64, 64, 0, 0],
                         192: [64, 64, 64, 0], 193: [64, 64, 64, 1], 255: [64, 64, 64, 63], 256: [64, 64, 64, 64]}[r]
    if name == "w1":
        assert np.all(cnt == 1) and seg.max() == 1 and c.slot_width == 1
        assert sum(sizes) == n_Γ                                # disjoint gather lists
    if name == "w3":
        assert c.slot_width == 4 and np.count_nonzero(cnt == 3) >= 10
    if name == "hub6":
        assert c.slot_width == 6 and len(fs.holders(c, 0)) == 6 and seg[0] == 6 and c.nwg == 1
    if name == "bare":
        e, b = fs.BARE_EMPTY, fs.BARE_NODE
        assert seg[b] == 0 and cnt[b] == 2 and len(fs.holders(c, b)) == 2
        for d, l in fs.holders(c, b):
            assert c.n_i[d] > 0 and np.diff(sp.csc_matrix(P.A_IΓdd[d]).indptr)[l] == 0
            assert all(c.A_IΓd[k][:, b].nnz == 0 for k in range(sub.ndom))
        assert c.n_i[e] == 0 and c.pos_I[e].size == 0 and P.A_IΓdd[e].nnz == 0 and c.A_IΓd[e].nnz == 0 and sizes[e] > 0
        assert sum(1 for v in c.n_i if v == 0) == 1
    if name == "solve":
        assert sub.ndom == 6 and {33, 65} <= set(sizes) and 1000 <= c.n <= 1500 and c.consistent
        assert abs(fs.assemble_ΓΓ(P.A_ΓΓdd, g, n_Γ) - c.A_ΓΓ).max() == 0.0
    else:
        assert not c.consistent and [B.shape for B in nr.prepare(None, c)] == [(m, m) for m in sizes]
        assert all(np.linalg.norm(B - B.T) > 0.5 * np.linalg.norm(B) for B in nr.prepare(None, c) if B.shape[0] > 2)   # non-symmetric


@pytest.mark.parametrize("line", [16, 32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", fs.INDUCED_CASES)
def test_tile_lists_of_every_tiling(checker, tmp_path, name, line):
    """the tile list DenseBlockOp builds for the nine tilings (one `rank` each in the driver's input), 16 doubles or 32
    floats per line"""
    c = fs.case(name)
    sizes, ndom = c.sizes, len(c.sizes)
    words = [ndom, len(fs.TILINGS), ss.N_CU, line, 0, *sizes]
    for rpw, waves in fs.TILINGS:
        words += [0, ndom, waves, rpw]
    fn = tmp_path / f"{name}_{line}.txt"
    fn.write_text(" ".join(str(w) for w in words) + "\n")
    ranks = json.loads(subprocess.run([checker, str(fn)], capture_output=True, text=True, check=True).stdout)["ranks"]
    assert len(ranks) == 9
    for (rpw, waves), R in zip(fs.TILINGS, ranks):
        T = rpw * waves
        tiles = np.array(R["tiles"], dtype=np.int64).reshape(-1, 7)
        assert (R["waves"], R["rpw"]) == (waves, rpw)
        assert len(tiles) == R["part_total"] == sum(-(-n // T) for n in sizes)
        assert R["ld"] == [fs.padded_ld(n, line) for n in sizes] and R["max_nd"] == max(sizes)
        assert np.all(tiles[:, 5] > 0) and np.all(tiles[:, 4] % T == 0)            # all streamed here; row0 on a tile edge
        last = {int(t[1]): int(t[6]) for t in tiles}                               # block size -> rows of its last tile
        if name == "tiles":
            assert {T - 1, T, T + 1} <= set(sizes) and min(sizes) < T              # below, on and one past the tile height
            assert last[T - 1] == T - 1 and last[T] == T and last[T + 1] == 1
            assert sum(1 for n in sizes if n < T) >= 3                             # blocks below one tile
            assert {fs.padded_ld(n, 16) for n in (15, 16, 17)} == {16, 32} and {fs.padded_ld(n, 32) for n in (31, 32, 33)} == {32, 64}
        if name == "panels":
            want = {16: [2032, 2048, 2048, 2064], 32: [2048, 2048, 2048, 2080]}[line]
            assert R["ld"][:4] == want
            assert [-(-l // fs.GEMV_PANEL) for l in want] == [1, 1, 1, 2]          # only the 2049-row block reaches the second panel ...
            assert want[3] - fs.GEMV_PANEL == line                                 # ... of one line of columns
            assert -(-fs.GEMV_PANEL // (64 * waves)) == {4: 8, 8: 4, 16: 2}[waves]  # operand gather lanes q NTH + tid per thread
            assert np.count_nonzero(tiles[:, 1] == 2049) == -(-2049 // T)
    if name == "solve":
        assert {33, 65} <= set(sizes)


@pytest.mark.parametrize("name", fs.INDUCED_CASES)
def test_induced_restatement_noise(fem, name):
    """plain, refine = 2 and refine = 3 of the restatement agree to 1e-12 in both couplings and on both storages' blocks"""
    c = fs.case(name)
    ΠSd = nr.prepare(fem, c)
    r = nr.apply_input(c)
    worst = 0.0
    for blocks in (ΠSd, nr.rounded_f32(ΠSd)):
        for cpl in nr.COUPLINGS:
            z = [nr.apply_neumann_neumann_induced(c, blocks, r, cpl, refine=k) for k in (0, 2, 3)]
            assert np.all(np.isfinite(z[2])) and np.linalg.norm(z[2]) > 0
            for a in z[:2]:
                worst = max(worst, np.linalg.norm(a - z[2]) / np.linalg.norm(z[2]))
    print(f"induced restatement noise {name}: {worst:.2e}")
    assert worst < NOISE_BAR


@pytest.mark.parametrize("name", fs.LORASC_CASES)
def test_lorasc_restatement_noise(name):
    c = fs.case(name)
    worst = 0.0
    for nev, with_coef in ((0, False), (5, True), (257, False), (1024, True)):
        x, E, coef = lr.apply_inputs(c, nev, with_coef)
        z = [lr.apply_lorasc(c, x, E, coef, refine=k) for k in (0, 2, 3)]
        assert np.all(np.isfinite(z[2])) and np.linalg.norm(z[2]) > 0
        for a in z[:2]:
            worst = max(worst, np.linalg.norm(a - z[2]) / np.linalg.norm(z[2]))
    print(f"lorasc restatement noise {name}: {worst:.2e}")
    assert worst < NOISE_BAR


def test_restatement_on_the_empty_interior_and_the_bare_node(fem):
    """`bare`: the Γ part of z at the bare node sees no interior at all; the n_i = 0 subdomain contributes through ΠS_d only.
    Against dense algebra (the block formulas of the assembled form and of LORASC) at the 1e-11 of test_nn_induced_cpu.py."""
    c = fs.case("bare")
    ΠSd = nr.prepare(fem, c)
    want = nr.block_formula_minv(c, ΠSd)
    got = nr.dense_minv(c, ΠSd, "assembled", refine=2)
    assert np.linalg.norm(got - want) <= 1e-11 * np.linalg.norm(want)
    x, E, coef = lr.apply_inputs(c, 5, True)
    want = lr.block_formula_minv(c, E, coef)
    assert np.linalg.norm(lr.dense_minv(c, E, coef, refine=2) - want) <= 1e-11 * np.linalg.norm(want)
    # r supported on the bare node alone: r_schur = r_Γ there, whatever the interiors hold
    r = np.zeros(c.n)
    r[c.pos_Γ[fs.BARE_NODE]] = 1.0
    z = nr.apply_neumann_neumann_induced(c, ΠSd, r, "assembled")
    cnt = np.asarray(c.P.sub.node_Γ_cnt, dtype=np.float64)
    zΓ = np.zeros(c.n_Γ)
    for (d, l) in fs.holders(c, fs.BARE_NODE):
        gd = c.P.sub.gather_idx[d]
        zΓ[gd] += ΠSd[d][:, l] / cnt[fs.BARE_NODE] / cnt[gd]
    assert np.allclose(z[c.pos_Γ], zΓ, rtol=1e-13, atol=1e-15)


# ------------------------------------------------------------------ the solver case
@pytest.fixture(scope="module")
def solve(fem, orc):
    c = fs.case("solve")
    Ao = orc.csc_operator(c.A)
    out = {"c": c, "Ao": Ao, "ϕ": lowest_eigvecs(Ao, c.n, c.P.sub.ndom + 10)}
    for storage in ("f64", "f32"):
        ΠSd = nr.prepare(fem, c)
        out[storage] = nr.dense_minv(c, nr.rounded_f32(ΠSd) if storage == "f32" else ΠSd, "assembled")
    return out


def test_solve_system_is_spd_and_m_is_spd(solve):
    c = solve["c"]
    assert abs(c.A - c.A.T).max() == 0.0
    ev = np.linalg.eigvalsh(c.A.toarray())
    print(f"solve: n = {c.n}, κ(A) = {ev[-1] / ev[0]:.1f}")
    assert ev[0] > 0 and ev[-1] / ev[0] <= 1e3
    for storage in ("f64", "f32"):
        Minv = solve[storage]
        asym = np.linalg.norm(Minv - Minv.T) / np.linalg.norm(Minv)
        lo = np.linalg.eigvalsh((Minv + Minv.T) / 2).min()
        print(f"solve, {storage}: asymmetry of M^-1 {asym:.2e}, smallest eigenvalue {lo:.3e}")
        # (rounding to fp32 is entrywise: the blocks stay as symmetric as the pseudo-inverses are, the bar is the restatement's noise)
        assert asym <= (1e-13 if storage == "f64" else 1e-12) and lo > 0


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["pcg", "defpcg"])
def test_solve_is_short_decided_and_insensitive_to_summation_order(orc, solve, kind, storage):
    c, Ao, Minv = solve["c"], solve["Ao"], solve[storage]
    Mo = orc.neumann_neumann_operator([Minv], [np.arange(c.n)], np.ones(c.n, dtype=np.int64))
    x0 = np.zeros(c.n)
    W = solve["ϕ"] if kind == "defpcg" else None
    x, it, res = orc.pcg(Ao, c.b, x0, Mo, 0, fs.EPS) if W is None else orc.defpcg(Ao, c.b, x0, W, Mo, 0, fs.EPS)
    tol = fs.EPS * np.linalg.norm(c.b)
    assert 2 <= it <= 50
    assert res[-1] <= tol * (1 - ks.STOP_GAP) and res[-2] >= tol * (1 + ks.STOP_GAP)
    xn, itn, resn = ks.numpy_krylov(lambda v: c.A @ v, lambda r: Minv @ r, W, c.b, x0, fs.EPS)
    share = ks.history_margin(resn, res)
    print(f"solve {kind} {storage}: it {it}, res[-2] / tol {res[-2] / tol:.4g}, res[-1] / tol {res[-1] / tol:.4g}; numpy vs oracle: "
          f"|Δres| / bar {share:.2e}, |Δx| / (1e-6 |x|) {ks.x_margin(xn, x):.2e}")
    assert itn == it and share <= ks.ORDER_SHARE and ks.x_margin(xn, x) <= ks.ORDER_SHARE
    if kind == "pcg":
        plain = orc.cg(Ao, c.b, x0, 0, fs.EPS)[1]
        print(f"solve: unpreconditioned cg needs {plain} iterations")
        assert plain >= 3 * it                                   # the preconditioner is what makes it short
