"""CPU suite of tests/amg_synth.py, the inputs and the reference of tests/test_gpu_amg_edges.py: every synthetic hierarchy has
the row-block shape it is named for (the partition of csrc/spmv_blocks.hpp compiled for the host by
tests/cpp/spmv_blocks_check.cpp, which amg_synth.row_blocks must reproduce), the bit-exact restatement `cycle_bits` agrees
with an independent longdouble cycle and with tests/amg_ref.py, and every edge is visible: a restatement with the fault a
case is there for differs from `cycle_bits` in at least one bit on that case.

Measured here (printed by the tests):
  * |cycle_bits - cycle_ld| entrywise against amg_synth.bound, worst ratio over every hierarchy, variant and right-hand
    side: 0.030 (coarse1_4); arrow_2049 7.6e-5 (the bound grows with the longest row, the error does not).
  * cycle_bits against amg_ref.cycle in relative 2-norm on the mesh hierarchies: N = 40 lognormal at most 2.1e-16, N = 12 on
    three levels at most 4.7e-17 (bar 1e-13).
  * every (fault, hierarchy, variant) of SEEN_BY is seen; the faults of the long-row tail in A and of the pair tail are seen
    by one right-hand side each (the random one, resp. the unit vector that meets the entry), the others by two or more.
  * interior edge cases, interior_solutions(0, b_I): leaving out the partial of one row block moves the largest iteration
    count in 13 of 15 blocks (to 5 or 7 for the blocks of one, two and five rows, to the cap n_d otherwise); the other two —
    the subdomain of one row, and rows [1021, 1023) of edge_rows — move the solution by 1.0 and by 7.8e-11 (bar 5.6e-13). The
    smallest move of a solution whose count is kept or off by one: 4.7e-11 (bar 2.1e-11), rows [2524, 2526) of edge_long.
    A lost fourth row pass on edge_long sends its diag(1025) subdomain to the cap of 1025 iterations.
"""
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT
import amg_ref as ar
import amg_synth as az
import sparse_synth as ss

TILE, NT = az.TILE, az.NT


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("amgblk") / "spmv_blocks_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "spmv_blocks_check.cpp")])
    return exe


@pytest.fixture(scope="module")
def parts(checker, fem, tmp_path_factory):
    """(name, "A" | "P" | "R") -> blocks [nb, 4] of the level-0 matrices, from one run of the host driver; the Python port
    of the partition must give the same blocks"""
    tmp = tmp_path_factory.mktemp("amgptr")
    mats = {}
    for name in az.NAMES:
        H = az.hierarchy(fem, name)
        mats[(name, "A")] = az.sorted_csr(H.A[0])
        if H.nlevels > 1:
            mats[(name, "P")] = az.sorted_csr(H.P[0])
            mats[(name, "R")] = az.transposed(H.P[0])
    files = []
    for (name, which), M in mats.items():
        fn = str(tmp / f"{name}_{which}.bin")
        ss.write_rowptr(fn, M.indptr)
        files.append(fn)
    out = subprocess.run([checker] + files, capture_output=True, text=True, check=True)
    lines = out.stdout.splitlines()
    assert len(lines) == len(mats)
    res = {}
    for (key, M), line in zip(mats.items(), lines):
        r = json.loads(line)
        assert r["tile"] == TILE and r["n"] == M.shape[0]
        blk = np.array(r["blocks"], dtype=np.int64).reshape(-1, 4)
        assert np.array_equal(blk, az.row_blocks(M.indptr)), key
        res[key] = blk
    return res


def rows(blk):
    return blk[:, 1] - blk[:, 0]


def nnz(blk):
    return blk[:, 3] - blk[:, 2]


def odd(blk):
    return blk[:, 2] % 2 == 1


@pytest.fixture(scope="module")
def interior_blocks(checker, fem, tmp_path_factory):
    """name -> (offs, blocks [nb, 4]) of the stacked A_II of the interior edge cases, cut at the subdomain boundaries, from the
    host driver; the Python port with breaks must give the same"""
    import interior_amg_ref as ir
    out = {}
    for name in ir.EDGE_NAMES:
        A, offs = ir.case(fem, name).stacked()
        fn = str(tmp_path_factory.mktemp("icg") / f"{name}.bin")
        ss.write_rowptr(fn, A.indptr, offs[1:-1])
        r = json.loads(subprocess.run([checker, fn], capture_output=True, text=True, check=True).stdout)
        blk = np.array(r["blocks"], dtype=np.int64).reshape(-1, 4)
        assert np.array_equal(blk, az.row_blocks(A.indptr, offs[1:-1])), name
        out[name] = (offs, blk)
    return out


def test_interior_edge_cases_have_the_blocks_they_are_named_for(interior_blocks):
    """the row blocks k_amg_post_dot leaves its partials of r'z for: no block across a subdomain boundary, a block that
    ends at every boundary; edge_long: the long row alone, the subdomain of one row as a block of one row, a block of more
    than 768 rows (four row passes) at an odd offset and a block of two rows after it; edge_rows: blocks of more than NT
    rows, blocks of two and five rows before the boundaries, nothing for the empty interior"""
    offs, b = interior_blocks["edge_long"]
    assert offs.tolist() == [0, 1500, 1501, 2526]
    assert tuple(b[0]) == (0, 1, 0, TILE + 1)
    k = int(np.flatnonzero(b[:, 0] == 1500)[0])
    assert tuple(b[k, :2]) == (1500, 1501) and tuple(b[k + 1, :2]) == (1501, 2524) and odd(b)[k + 1] and rows(b)[k + 1] > 768
    assert tuple(b[k + 2, :2]) == (2524, 2526) and k + 3 == b.shape[0]
    offs, b = interior_blocks["edge_rows"]
    assert offs.tolist() == [0, 1023, 1023, 2048]
    assert rows(b).max() > NT and tuple(b[3, :2]) == (1021, 1023) and tuple(b[4, :1]) == (1023,) and tuple(b[-1, :2]) == (2043, 2048)
    for name, (offs, b) in interior_blocks.items():
        for cut in offs[1:-1]:
            assert not np.any((b[:, 0] < cut) & (b[:, 1] > cut)), (name, cut)
            assert cut in b[:, 1] and cut in b[:, 0], (name, cut)
        assert np.all(rows(b) > 0)


@pytest.mark.parametrize("name", ["edge_long", "edge_rows"])
def test_every_block_partial_of_the_interior_cases_is_visible(fem, interior_blocks, name):
    """The solve the GPU suite compares by iteration count on these cases, interior_solutions(0, b_I) with a random b_I, has
    data in every row. With r'z summed as the per-block partials (`block_rz`) the restatement keeps its history to rounding;
    with the partial of any one block left out, or with the rows past the first 256 of every block left out (and past the
    first 768 on edge_long, the fourth row pass), the iteration count or the residual history of that block's subdomain changes
    by more than 1e-6 relative (entries above the tolerance), or the solve ends above its tolerance (the subdomain of one
    row: ρ = 0 leaves x = 0) — far above the rounding between host and device."""
    import interior_amg_ref as ir
    C = ir.case(fem, name)
    offs, blk = interior_blocks[name]
    v, its, hist, tol = C.solve_b(fem)
    bars = ir.solution_bars(C, fem, its)
    dev = {}

    def moved(rz):
        with np.errstate(all="ignore"):
            v2, its2, hist2, _ = C.solve_b(fem, rz=rz)
        dev["its"] = int(its2.max())
        dev["u"] = [float(np.linalg.norm(v2[offs[d]:offs[d + 1]] - v[offs[d]:offs[d + 1]]) / max(np.linalg.norm(v[offs[d]:offs[d + 1]]), 1e-300))
                    for d in range(offs.size - 1)]
        out = []
        for d in range(offs.size - 1):
            m = min(len(hist[d]), len(hist2[d]))
            h, h2 = np.array(hist[d][:m]), np.array(hist2[d][:m])
            above = h > tol[d]                          # what lies below the tolerance is rounding (or zero: an empty interior)
            rel = np.max(np.abs(h2[above] - h[above]) / h[above], initial=0.0)
            missed = (hist2[d][-1] > tol[d]) != (hist[d][-1] > tol[d])      # ends above the tolerance (the GPU suite's residual cap)
            out.append(bool(its2[d] != its[d] or missed or not rel <= 1e-6))
        return out

    assert not any(moved(ir.block_rz(blk))), "the block partials alone move the history"
    assert all(u <= b for u, b in zip(dev["u"], bars)), (dev["u"], bars)
    print(f"{name}: bars of the solution {bars.tolist()}; block partials against numpy's dot move it by {dev['u']}")
    for k, (r0, r1, _, _) in enumerate(blk):
        d = int(np.searchsorted(offs, r0, side="right") - 1)
        while offs[d + 1] == offs[d]:
            d += 1
        seen = moved(ir.block_rz(blk, drop=k))
        print(f"{name}: without the partial of block {k} rows [{r0}, {r1}) of subdomain {d}: moved {seen}")
        assert seen[d], (name, k)
        # what the GPU suite sees of it: the largest count, or the solution against solution_bars
        print(f"    largest count {dev['its']} (clean {int(its.max())}), solution of subdomain {d} moved by {dev['u'][d]:.2e} (bar {bars[d]:.2e})")
        assert dev["its"] != int(its.max()) or dev["u"][d] > bars[d], (name, k)
    caps = (256, 768) if name == "edge_long" else (256,)
    for cap in caps:
        seen = moved(ir.block_rz(blk, rows_cap=cap))
        print(f"{name}: rows past the first {cap} of every block left out: moved {seen}")
        assert any(seen), (name, cap)
        assert dev["its"] != int(its.max()) or any(u > b for u, b in zip(dev["u"], bars)), (name, cap)
        if name == "edge_long" and cap == 768:
            assert seen[2] and not seen[1]


def test_hierarchies_have_the_shape_they_are_named_for(parts, fem):
    B = parts
    # diag1025: 1024 rows in one block (four row passes of NT threads), a second block of one row; P in pairs: the same
    for w in ("A", "P"):
        b = B[("diag1025", w)]
        assert b.shape[0] == 2 and rows(b).tolist() == [1024, 1] and rows(b).max() > 768
    # tridiag3000: more than NT rows per block, rows given back (a block below the greedy 1022 .. 1024). A_0 and P_0 (rows of
    # one and two entries, six per aggregate of four rows) have even offsets and even counts before the last block: the
    # paired path alone. R_0 (rows of four to six entries) carries both other paths: blocks at odd offsets (the unpaired
    # path) and a paired block of an odd count before the end of the matrix (the k + 1 < nnz tail).
    b = B[("tridiag3000", "A")]
    assert rows(b).max() > NT and np.any(nnz(b)[:-1] < TILE - 2) and b.shape[0] == 9
    for w in ("A", "P"):
        b = B[("tridiag3000", w)]
        assert not odd(b).any() and not np.any(nnz(b)[:-1] % 2 == 1), w
    b = B[("tridiag3000", "R")]
    assert odd(b).sum() >= 2 and np.any(~odd(b)[:-1] & (nnz(b)[:-1] % 2 == 1))
    # the same two paths in a P (k_amg_prolong): arrow_1024, whose P has a paired block of an odd count first and a block at
    # an odd offset after it
    b = B[("arrow_1024", "P")]
    assert odd(b).any() and np.any(~odd(b)[:-1] & (nnz(b)[:-1] % 2 == 1))
    # odd_tail: the same two paths in an A (k_amg_down, k_amg_post): a paired block of 1023 entries first, then a full tile
    # at an odd offset
    b = B[("odd_tail", "A")]
    assert tuple(b[0, 2:]) == (0, TILE - 1) and b.shape[0] > 2 and tuple(b[1, 2:]) == (TILE - 1, 2 * TILE - 1) and rows(b)[1] > NT
    # arrow_m: row 0 alone in its block with m entries: fills the tile exactly, one entry more, two tiles and one entry
    for m in az.ARROW_M:
        b = B[(f"arrow_{m}", "A")]
        assert tuple(b[0]) == (0, 1, 0, m), m
        assert tuple(B[(f"arrow_{m}", "R")][0]) == (0, 1, 0, m), m          # column 0 of P: every row that touches row 0
    assert (TILE, TILE + 1, 2 * TILE + 1) == az.ARROW_M
    b = B[("arrow_1025", "A")]
    assert odd(b)[1] and rows(b)[1] > NT and np.any(odd(b) & (rows(b) > 768))           # the unpaired path, two and four row passes
    b = B[("arrow_2049", "P")]                                              # row 0 of P: TILE + 1 entries, alone
    assert tuple(b[0]) == (0, 1, 0, TILE + 1)
    b = B[("arrow_1024", "P")]                                              # and a full tile at an odd offset in a P
    assert np.any(odd(b) & (nnz(b) == TILE))
    # odd_start: a block that fills the tile exactly at k0 = 1; then odd k0 with more than NT rows
    b = B[("odd_start", "A")]
    assert tuple(b[0]) == (0, 1, 0, 1) and tuple(b[1]) == (1, 2, 1, 1 + TILE) and odd(b)[2] and rows(b)[2] > NT
    # holes: empty rows first and last, a block that holds the run of 1500 empty rows, in A and in the rectangular P
    H = az.hierarchy(fem, "holes")
    for M, b in ((H.A[0], B[("holes", "A")]), (H.P[0], B[("holes", "P")])):
        rl = np.diff(M.indptr)
        assert np.all(rl[:ss.HOLES_LEAD] == 0) and np.all(rl[-ss.HOLES_TRAIL:] == 0) and rl[ss.HOLES_LEAD] > 0
        assert rows(b).max() > ss.HOLES_INNER > TILE
    assert H.P[0].shape[1] < H.P[0].shape[0] and (np.diff(az.transposed(H.P[0]).indptr) == 0).sum() > 100   # empty rows of R too
    # longP: a P row of TILE + 1 entries alone in its block, a run of empty rows in P; A and R without long rows
    b = B[("longP", "P")]
    k = int(np.flatnonzero(b[:, 0] == az.LONGP_ROW)[0])
    assert rows(b)[k] == 1 and nnz(b)[k] == TILE + 1
    rl = np.diff(az.hierarchy(fem, "longP").P[0].indptr)
    assert np.all(rl[az.LONGP_EMPTY[0]:az.LONGP_EMPTY[1]] == 0)
    assert nnz(B[("longP", "A")]).max() <= TILE and nnz(B[("longP", "R")]).max() <= TILE
    # lead_long: a block without any non-zero, then the long row alone — in A and in R
    for w in ("A", "R"):
        b = B[("lead_long", w)]
        assert nnz(b)[0] == 0 and rows(b)[0] > 0 and rows(b)[1] == 1 and nnz(b)[1] == TILE + 1, w
    # giant: the long row is R's alone
    assert nnz(B[("giant", "R")]).max() > TILE and nnz(B[("giant", "A")]).max() <= TILE and nnz(B[("giant", "P")]).max() <= TILE
    # three_tiny, coarse_n
    assert az.hierarchy(fem, "three_tiny").sizes == [5, 2, 1]
    for n in az.COARSE_N:
        assert az.hierarchy(fem, f"coarse1_{n}").sizes == [n]
        s = az.hierarchy(fem, f"coarse2_{n}").sizes
        assert len(s) == 2 and s[1] == n and s[0] > n
        assert np.diff(az.transposed(az.hierarchy(fem, f"coarse2_{n}").P[0]).indptr).min() > 0
    assert {n % 64 for n in az.COARSE_N} >= {0, 1, 63} and {n % 4 for n in az.COARSE_N} == {0, 1, 2, 3} and max(az.COARSE_N) > 128
    # blocks_k: exactly k row blocks; the dealing b = (bid & 7) * per + (bid >> 3) reaches every block once, and for
    # k = 1, 7, 9, 17 some of the 8 * per workgroups get none
    for k in az.BLOCKS_K:
        b = B[(f"blocks_{k}", "A")]
        assert b.shape[0] == k
        bid, blk = az.xcd_of_blocks(k)
        assert sorted(blk.tolist()) == list(range(k)) and (bid.size < 8 * ((k + 7) // 8)) == (k % 8 != 0)
    assert az.hierarchy(fem, "blocks_17").sizes[0] < 5600


def test_values_are_in_the_normal_range(fem):
    for name in az.NAMES:
        H = az.hierarchy(fem, name)
        for r in az.rhs(name, H.sizes[0]):
            assert np.all((r == 0.0) | (np.abs(r) > 1e-3))
        r = az.rhs(name, H.sizes[0])[0]
        if r.size >= 100:
            assert 0.1 < np.mean(r == 0.0) < 0.3 and (r > 0).any() and (r < 0).any()
        if name != "giant":
            for M in list(H.A) + list(H.P):
                assert np.all(np.abs(M.data) >= 0.25) and np.all(np.abs(M.data) <= 4.0)
            assert np.array_equal(H.coarse_inv, H.coarse_inv.T) and np.all(np.abs(H.coarse_inv) >= 0.25)
        assert np.all(az.hierarchy(fem, name, "pzp").omega_over_d[0] == 0.0) if H.nlevels > 1 else True
        assert not az.hierarchy(fem, name, "smooth").coarse_inv.any() if H.nlevels > 1 else True


def test_cycle_bits_within_the_bound_of_the_longdouble_cycle(fem):
    """entrywise |cycle_bits - cycle_ld| <= 2 u â Σ_s (L_s + 3) (amg_synth.bound) on every hierarchy, variant and right-hand side"""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    worst = {}
    for name in az.NAMES:
        for v in az.variants(fem, name):
            H = az.hierarchy(fem, name, v)
            for r in az.rhs(name, H.sizes[0]):
                d = np.abs(az.cycle_bits(H, r) - az.cycle_ld(H, r)).astype(np.float64)
                bd = az.bound(H, r)
                assert (d <= bd).all(), (name, v)
                worst[name] = max(worst.get(name, 0.0), float(np.max(np.divide(d, bd, out=np.zeros_like(d), where=bd > 0))))
    top = max(worst, key=worst.get)
    print(f"cycle_bits vs cycle_ld: worst error / bound {worst[top]:.3f} ({top}); arrow_2049 {worst['arrow_2049']:.2e}")


def mesh_hierarchies(fem):
    A12 = ar.system(fem, 12, "example01")[0]
    return {"N40 lognormal": ar.case(fem, 40, "lognormal")[2], "N12 three levels": fem.prepare_amg_precond(A12, max_levels=3, max_coarse=4)}


def test_cycle_bits_against_the_numpy_cycle_on_the_mesh_hierarchies(fem):
    for tag, H in mesh_hierarchies(fem).items():
        assert H.nlevels == (3 if "three" in tag else 2)
        for r in az.rhs(tag, H.sizes[0]):
            want, got = ar.cycle(H, r), az.cycle_bits(H, r)
            err = np.linalg.norm(got - want) / np.linalg.norm(want)
            print(f"{tag} {H.sizes}: cycle_bits vs amg_ref.cycle {err:.2e}")
            assert err <= 1e-13
            assert (np.abs(got - az.cycle_ld(H, r)).astype(np.float64) <= az.bound(H, r)).all()


# (defect, hierarchy, variant): the fault, a case that is there for it, and the variant that isolates the kernel
SEEN_BY = (
    [("block_last", n, v) for n in ("diag1025", "tridiag3000", "odd_start", "blocks_1", "blocks_9") for v in az.VARIANTS] +
    [("long_tail", "arrow_1025", "smooth"), ("long_tail", "arrow_2049", "smooth"), ("long_tail", "arrow_2049", "pzp"),
     ("long_tail", "longP", "pzp"), ("long_tail", "giant", "pzp"), ("long_tail", "lead_long", "full")] +
    [("pair_overrun", "tridiag3000", "pzp"), ("pair_overrun", "odd_start", "smooth"), ("pair_overrun", "tridiag3000", "full"),
     ("pair_overrun", "arrow_1024", "pzp"), ("pair_overrun", "odd_tail", "smooth"), ("pair_overrun", "odd_tail", "full"), ("block_last", "odd_tail", "smooth")] +
    [("skip_empty", "holes", "smooth"), ("skip_empty", "holes", "full"), ("skip_empty", "lead_long", "smooth")] +
    [("coarse_cols", f"coarse{k}_{n}", "full") for k in (1, 2) for n in az.COARSE_N if n % 64] +
    [("coarse_rows", f"coarse{k}_{n}", "full") for k in (1, 2) for n in az.COARSE_N if n % 4] +
    [("coarse_cols", "three_tiny", "pzp"), ("coarse_rows", "three_tiny", "pzp")])


@pytest.mark.parametrize("defect,name,variant", SEEN_BY)
def test_every_edge_is_visible(fem, defect, name, variant):
    """a restatement with the fault differs from cycle_bits in at least one bit, on the hierarchy named for the edge"""
    H = az.hierarchy(fem, name, variant)
    seen = [not np.array_equal(az.cycle_bits(H, r), az.cycle_bits(H, r, defect=defect)) for r in az.rhs(name, H.sizes[0])]
    print(f"{defect} on {name} ({variant}): seen by right-hand sides {np.flatnonzero(seen).tolist()}")
    assert any(seen), (defect, name, variant)


def test_defects_cover_the_list():
    assert {d for d, _, _ in SEEN_BY} == set(az.DEFECTS)


def test_a_defect_leaves_other_cases_alone(fem):
    """the variants are faults of the edge, not of the whole cycle: without the edge they change nothing"""
    H = az.hierarchy(fem, "coarse2_64")
    r = az.rhs("coarse2_64", H.sizes[0])[0]
    for d in ("long_tail", "skip_empty", "coarse_cols", "coarse_rows"):
        assert np.array_equal(az.cycle_bits(H, r), az.cycle_bits(H, r, defect=d)), d
