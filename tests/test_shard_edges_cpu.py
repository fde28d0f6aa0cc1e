"""CPU suite of the dense operators' tile list (csrc/dense_tiles.hpp, compiled for the host by
tests/cpp/dense_tiles_check.cpp) on the synthetic sharded cases of tests/shard_synth.py: the invariants the folded launches
and the exchange rely on — every rank derives the same partial-dot layout whatever tiling it chose — and for every case
the property it is named for, so that tests/test_gpu_shard_edges.py reaches the branches it was written to reach. Also the
oracle-side facts that suite's bars rest on (iteration counts, residuals well away from the stop threshold), and the same
driver under AddressSanitizer / UBSan."""
import subprocess

import numpy as np
import pytest

import shard_synth as ss

CASES = ss.cases()
BY_NAME = {c.name: c for c in CASES + ss.local_cases()}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return ss.build_checker(tmp_path_factory.mktemp("dense_tiles"))


@pytest.fixture(scope="module")
def lists(checker, tmp_path_factory):
    return ss.tile_lists(checker, CASES, tmp_path_factory.mktemp("cases"))


def padded_ld(n, line=16):
    l = -(-n // line) * line
    return l + line if (l % (16 * line) == 0 and l != ss.GEMV_PANEL) else l


def test_tile_list_invariants(lists):
    for c in CASES:
        ranks = lists[c.name]
        sizes = np.array(c.sizes)
        loc_off = np.concatenate([[0], np.cumsum(sizes)[:-1]])
        base = np.concatenate([[0], np.cumsum(-(-sizes // ss.PART_ROWS))])       # first partial-dot slot of every block
        block_of = {int(loc_off[d]): d for d in range(c.ndom) if sizes[d] > 0}
        seen = np.zeros(int(base[-1]), dtype=np.int64)
        assert sorted(c.slices()) == c.slices() and c.slices()[0][0] == 0 and c.slices()[-1][1] == c.ndom
        for r, (R, (lo, hi)) in enumerate(zip(ranks, c.slices())):
            step = R["waves"] * R["rpw"]
            assert R["waves"] in (4, 8, 16) and R["rpw"] in (1, 2, 4)
            # one layout on all ranks, derived from the maps alone
            assert R["part_total"] == base[-1] == ranks[0]["part_total"], (c.name, r)
            assert R["ld"] == [padded_ld(n) for n in c.sizes] and R["max_ld"] == max(R["ld"]) and R["max_nd"] == max(c.sizes)
            off = 0
            for d in range(c.ndom):
                own = lo <= d < hi
                assert R["moff"][d] == (off if own else 0)
                off += c.sizes[d] * R["ld"][d] if own else 0
            assert R["elems"] == off
            T = R["tiles"]
            cover = {d: [] for d in range(c.ndom)}
            for mat_off, n, ld, lo_t, row0, active, nrows in T:
                d = block_of[int(lo_t)]
                assert n == c.sizes[d] and ld == R["ld"][d]
                cover[d].append((int(row0), int(nrows)))
                if lo <= d < hi:
                    # a streamed tile: its slot follows from the block and the row alone
                    assert active - 1 == base[d] + row0 // ss.PART_ROWS and mat_off == R["moff"][d], (c.name, r, d)
                    assert 0 <= active - 1 < R["part_total"]
                    seen[active - 1] += 1
                else:
                    assert active == 0 and mat_off == 0, (c.name, r, d)
            for d in range(c.ndom):
                # the tiles of a block partition its rows, in order: waves x rpw rows where it is stored, 64 x waves elsewhere
                st = step if lo <= d < hi else 64 * R["waves"]
                want = [(r0, min(st, c.sizes[d] - r0)) for r0 in range(0, c.sizes[d], st)]
                assert cover[d] == want, (c.name, r, d)
        # the ranks' streamed tiles use pairwise disjoint slots
        assert seen.max(initial=0) <= 1, c.name


def test_single_context_list_is_the_tile_number(checker, tmp_path):
    """Not sharded: `active` = 1 + the tile number, part_total = the number of tiles (the layout of the one-GPU launches),
    for doubles (16 per line) and floats (32 per line: padding of the fp32-stored blocks)."""
    for line in (16, 32):
        one = [ss.Case(c.name, c.sizes, c.seed, 1, tilings=[tl]) for c in CASES[:8] for tl in [(16, 2), (4, 1), (8, 4)]]
        for k, c in enumerate(one):
            c.name += f"_{k}"
        for c in one:
            import json
            fn = tmp_path / f"{c.name}_{line}.txt"
            fn.write_text(ss.tile_input(c, line=line, sharded=False))
            R = json.loads(subprocess.run([checker, str(fn)], capture_output=True, text=True, check=True).stdout)["ranks"][0]
            T = np.array(R["tiles"]).reshape(-1, 7)
            assert R["part_total"] == T.shape[0]
            assert np.array_equal(T[:, 5], 1 + np.arange(T.shape[0]))
            assert R["ld"] == [padded_ld(n, line) for n in c.sizes]


def n_active(R):
    return int(np.count_nonzero(R["tiles"][:, 5])) if R["tiles"].size else 0


def folds(c, ranks):
    return c.width() <= 4 and all(R["max_ld"] <= ss.GEMV_PANEL and -(-R["max_ld"] // (64 * R["waves"])) <= 8 for R in ranks)


def test_every_case_has_the_property_it_is_named_for(lists):
    for c in CASES:
        ranks, sl = lists[c.name], c.slices()
        cnt = c.maps()[1]
        n_Γ = c.maps()[2]
        tilings = [(R["waves"], R["rpw"]) for R in ranks]
        assert c.world <= 8
        assert c.fold == folds(c, ranks), c.name
        if c.name.startswith("uneven"):
            assert len({hi - lo for lo, hi in sl}) > 1 and all(n_active(R) > 0 for R in ranks)
        if c.name == "blockless_world":
            assert c.world > c.ndom and sl[0] == (0, 0)
        if c.name == "blockless_empty":
            lo, hi = sl[0]
            assert hi > lo and all(c.sizes[d] == 0 for d in range(lo, hi))
        if c.name.startswith("blockless"):
            assert n_active(ranks[0]) == 0 and all(n_active(R) > 0 for R in ranks[1:])
            assert len(ranks[0]["tiles"]) > 0                       # ... but it has owner-duty tiles: its launches run
        else:
            assert all(n_active(R) > 0 for R in ranks), c.name
        if c.name == "empty_inside":
            for lo, hi in sl:
                z = [d for d in range(lo, hi) if c.sizes[d] == 0]
                assert lo in z and hi - 1 in z and any(lo < d < hi - 1 for d in z)
        if c.name == "tiny":
            assert {1, 2, 3, 5, 7} <= set(c.sizes)
            assert any(0 < c.sizes[d] < R["waves"] * R["rpw"] for R, (lo, hi) in zip(ranks, sl) for d in range(lo, hi))
            assert any(n % ss.PART_ROWS for n in c.sizes)
            assert any(c.sizes[d] % (R["waves"] * R["rpw"]) for R, (lo, hi) in zip(ranks, sl) for d in range(lo, hi))
        if c.name.startswith("mixed_tilings"):
            assert tilings == c.tilings and len(set(tilings)) == c.world
            assert len({w * r for w, r in tilings}) > 1 or c.name.endswith("_a")
            # an owner-duty tile list of more than one tile: a non-owned block longer than 64 waves rows
            assert any(c.sizes[d] > 64 * R["waves"] for R, (lo, hi) in zip(ranks, sl) for d in range(c.ndom) if not lo <= d < hi)
        if c.name.startswith("mixed_tilings") or c.name == "auto_big" or c.push:
            # ranks with different workgroup sizes AND more partials than summing threads: the sum of the partials is
            # only the same on all ranks if its association does not follow the workgroup size
            assert len({w for w, _ in tilings}) > 1 and ranks[0]["part_total"] > ss.PART_LANES, c.name
        if c.name == "auto_big":
            assert tilings[0] == (16, 2) and tilings[1] != tilings[0] and max(c.sizes) <= 2048
            lo, hi = sl[0]
            rows = sum(c.sizes[lo:hi])
            assert rows // ss.N_CU >= 24 and (rows - (hi - lo)) // ss.N_CU < 24     # as few rows as the threshold allows
        if c.name in ("w1", "w2", "w3", "hub6"):
            want = {"w1": (1, 1), "w2": (2, 2), "w3": (3, 4), "hub6": (6, 6)}[c.name]
            assert (int(cnt.max()), c.width()) == want
        if c.name == "w1":
            assert np.all(cnt == 1)
        if c.name == "wide":
            assert max(R["max_ld"] for R in ranks) > ss.GEMV_PANEL and c.width() <= 4
        if c.push:
            own_S, own_M = c.n_own(0, ranks[0]["tiles"], False), c.n_own(0, ranks[0]["tiles"], True)
            assert own_S == int(c.name.split("_")[1]), (c.name, own_S)
            chunks = {"push_4096": 1, "push_4097": 2, "push_8260": 3}[c.name]
            assert -(-own_S // ss.XCHG_PUSH_CHUNK) == chunks
            print(f"{c.name}: n_own S {own_S} ({chunks} chunks), ΠS {own_M} ({-(-own_M // ss.XCHG_PUSH_CHUNK)} chunks)")
        if c.name.startswith("stage"):
            count = n_Γ * c.width()
            want = int(c.name.split("_")[1])
            assert count + 4 == want or (want > 65536 and count == want), (c.name, count)
            if c.name == "stage_16384":
                assert count + 4 <= ss.LOOPBACK_STAGE
            if c.name == "stage_16385":
                assert count + 4 == ss.LOOPBACK_STAGE + 1
            if c.name == "stage_65600":
                assert count > 256 * 256                            # more entries than one pass of the 256 x 256 grid
            assert sum(c.sizes) * 64 * 8 < 64e6 and c.no_fold_env   # tens of MB; driven through the unfolded loop
        if c.modes:
            # launches that wait inside themselves: all ranks' workgroups must be resident on the chip at once
            assert sum(len(R["tiles"]) for R in ranks) <= ss.N_CU, c.name
    assert {c.name for c in CASES if c.push} == {n for n, _, _ in ss.PUSH_CASES}


def test_local_only_cases_have_the_widths_they_are_named_for():
    eq, uneq = ss.local_cases()
    assert ss.local_width(eq, 0) == ss.local_width(eq, 1) == 4
    assert ss.local_width(uneq, 0) == 4 and ss.local_width(uneq, 1) <= 2
    for c in (eq, uneq):                                        # ... and nodes shared ACROSS the ranks: colliding slots are added
        g = c.maps()[0]
        (lo0, hi0), (lo1, hi1) = c.slices()
        a = np.concatenate([g[d] for d in range(lo0, hi0)])
        b = np.concatenate([g[d] for d in range(lo1, hi1)])
        assert np.intersect1d(a, b).size > 0


SOLVER_CASES = [c.name for c in CASES + ss.local_cases() if c.maxit == 0]


def numpy_pcg(S, P, g, cnt, n, b, x0, eps):
    """cg.jl:67-109 with numpy's matrix-vector products and dots (pairwise / blocked sums: another order than the oracle's)."""
    def A(v):
        y = np.zeros(n)
        for Sd, gd in zip(S, g):
            if gd.size:
                y[gd] += Sd @ v[gd]
        return y

    def M(v):
        y = np.zeros(n)
        for Pd, gd in zip(P, g):
            if gd.size:
                y[gd] += (Pd @ (v[gd] / cnt[gd])) / cnt[gd]
        return y

    x = x0.copy()
    r = b - A(x)
    z = M(r)
    p = z.copy()
    rz = r @ z
    res = [np.sqrt(r @ r)]
    tol = eps * np.linalg.norm(b)
    while len(res) < n and res[-1] > tol:
        Ap = A(p)
        alpha = rz / (p @ Ap)
        x += alpha * p
        r -= alpha * Ap
        z = M(r)
        rz, old = r @ z, rz
        p = (rz / old) * p + z
        res.append(np.sqrt(r @ r))
    return x, len(res), np.array(res)


@pytest.mark.parametrize("name", SOLVER_CASES)
def test_oracle_solves_are_decided_and_insensitive_to_summation_order(orc, name):
    """The GPU suite asserts EQUAL iteration counts and holds the sharded histories to rtol 1e-9 / atol 1e-13 res_0 of the
    single context's, whose partial dot products are cut differently. Both are only meaningful where rounding cannot
    decide: on the oracle, with the exact inverses Q diag(1/λ) Q' for Π (mi_nn_pinv agrees with them to κ n eps ~ 1e-10),
    from x0 = 0 and from the non-zero x0 of the sequence test,
      - no solve takes more than 50 iterations;
      - the last residual above tol ‖b‖ and the first one below it both stay 1e-6 (relative) away from it;
      - a numpy PCG (another summation order in every product and dot) gives the same `it`, and history and x within a
        TENTH of that bar."""
    c = BY_NAME[name]
    g, cnt, n_Γ = c.maps()
    S, P = c.blocks()
    _, b, x0 = c.vectors()
    Ao = orc.apply_local_schurs_operator(S, g, n_Γ)
    Mo = orc.neumann_neumann_operator(P, g, cnt)
    for start in (np.zeros(n_Γ), x0):
        x, it, res = orc.pcg(Ao, b, start, Mo, eps=c.eps)
        tol = c.eps * np.linalg.norm(b)
        assert 1 <= it <= 50
        assert res[-1] <= tol * (1 - 1e-6)
        assert it == 1 or res[-2] >= tol * (1 + 1e-6)
        xn, itn, resn = numpy_pcg(S, P, g, cnt.astype(np.float64), n_Γ, b, start, c.eps)
        assert itn == it
        ratio = float(np.max(np.abs(resn - res) / (1e-13 * res[0] + 1e-9 * res)))
        xdev = float(np.linalg.norm(xn - x) / np.linalg.norm(x))
        print(f"{name}: it {it}, res[-2]/tol {res[-2] / tol if it > 1 else np.inf:.6g}, res[-1]/tol {res[-1] / tol:.6g}; "
              f"numpy vs oracle: |Δres| / bar {ratio:.2e}, |Δx|/|x| {xdev:.2e}")
        assert ratio <= 0.1 and xdev <= 1e-10


def test_driver_under_sanitizers(lists, tmp_path):
    """The header on every case under AddressSanitizer and UBSan (a stand-alone host program, nothing loaded into
    Python): clean exit, same lists."""
    exe = ss.build_checker(tmp_path, sanitize=True)
    again = ss.tile_lists(exe, CASES, tmp_path)
    for c in CASES:
        for R, Q in zip(lists[c.name], again[c.name]):
            assert np.array_equal(R["tiles"], Q["tiles"]) and R["moff"] == Q["moff"] and R["part_total"] == Q["part_total"]
