"""Synthetic SHARDED dense problems: blocks and gather maps drawn directly (fixed seeds) at the partition, tile and exchange
edges the FEM problems never produce. One table of named cases, shared by tests/test_shard_edges_cpu.py (the tile lists of
csrc/dense_tiles.hpp through tests/cpp/dense_tiles_check.cpp, and the oracle-side facts) and tests/test_gpu_shard_edges.py
(the in-process ranks on one GPU).

A case = block sizes, a seed, how the gather maps are drawn, `world`, the slice of every rank (default: api.shard_domains)
and per rank either "auto" or a forced (waves, rpw) tiling. Blocks: spd_blocks (κ = 1e3). Maps: gather_maps (dense sharing, multiplicities
1 ... 4) or cover_maps (exact multiplicity 1 or 2)."""
import json
import os
import subprocess
import threading

import numpy as np

from test_gpu_dense_edges import gather_maps, spd_blocks, split, concat, ref_apply, assert_summation_bound  # noqa: F401
from test_gpu_multirank import run_ranks  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PART_ROWS, GEMV_PANEL, XCHG_PUSH_CHUNK = 4, 2048, 4096      # csrc/dense_tiles.hpp, csrc/exchange.hpp
PART_LANES = 256                                             # csrc/kernels.hpp: threads that sum the partials of a sharded launch
LOOPBACK_STAGE = 16384                                       # doubles of staging the loopback self-test reserves
EPS = 1e-2                                                   # stop threshold of the solves (see Case)
N_CU = 256                                                   # MI355X; the GPU suite passes the device's own count


def shard_domains(ndom, rank, n_ranks):                      # api.shard_domains (the CPU suite has no package to ask)
    return ndom * rank // n_ranks, ndom * (rank + 1) // n_ranks


def cover_maps(sizes, n_nodes, rng):
    """Gather lists that lay the blocks end to end along a random cyclic order of `n_nodes` Γ nodes: every node lies in
    floor or ceil(sum(sizes) / n_nodes) blocks — exactly `share` of them when sum(sizes) == share * n_nodes (gather_maps
    cannot draw share 1 or 2: it has too few nodes). Returns (gather lists, node_Γ_cnt, n_Γ)."""
    assert max(sizes) <= n_nodes <= sum(sizes)
    order = rng.permutation(n_nodes)
    cnt = np.zeros(n_nodes, dtype=np.int64)
    g, off = [], 0
    for n in sizes:
        pick = order[(off + np.arange(n)) % n_nodes]
        rng.shuffle(pick)
        cnt[pick] += 1
        g.append(pick.astype(np.int64))
        off += n
    assert cnt.min() >= 1
    return g, cnt, n_nodes


class Case:
    def __init__(self, name, sizes, seed, world, tilings=None, hub=0, max_share=4, cover=None, slices=None, eps=None,
                 maxit=0, fold=True, no_fold_env=False, modes=False, sequence=False, push=False, big=False, branch=""):
        self.name, self.sizes, self.seed, self.world = name, list(sizes), seed, world
        self.tilings = list(tilings) if tilings else ["auto"] * world
        self.hub, self.max_share, self.cover = hub, max_share, cover
        # Stop threshold of the solves. κ = 1e3 blocks make PCG histories sensitive to the order of the dot-product sums:
        # at eps = 1e-7 two tilings on ONE context differ by up to 1e7 x the 1e-9 bar of the sharded comparisons (measured
        # on an MI355X), the C oracle and a numpy PCG likewise. Up to eps = 1e-2 (17-25 iterations), and with one block of
        # >= 300 rows in every case (small systems lose orthogonality sooner), they agree to a few percent of that bar:
        # tests/test_shard_edges_cpu.py asserts it for every case.
        self.eps = EPS if eps is None else eps
        self.no_fold_env = no_fold_env   # driven through the unfolded loop (MI355_NO_FOLD=1) whatever its shape
        self._slices = slices
        self.maxit = maxit            # > 0: solves are capped (the case is about sizes, not convergence)
        self.fold = fold              # the folded launches apply (slot width <= 4, max_ld <= GEMV_PANEL)
        self.modes = modes            # runs in the producers-and-waits test
        self.sequence = sequence      # runs in the counter-and-parity test
        self.push = push              # runs with MI355_XCHG_PUSH_KERNEL=1
        self.big = big                # applies and one folded solve only
        self.branch = branch          # what the case reaches
        self._maps = self._blocks = None
        assert len(self.tilings) == world

    @property
    def ndom(self):
        return len(self.sizes)

    def slices(self):
        return self._slices or [shard_domains(self.ndom, r, self.world) for r in range(self.world)]

    def maps(self):
        if self._maps is None:
            rng = np.random.default_rng(self.seed)
            if self.cover:
                self._maps = cover_maps(self.sizes, self.cover, rng)
            else:
                self._maps = gather_maps(self.sizes, rng, max_share=self.max_share, hub=self.hub)
        return self._maps

    def width(self):
        w = int(self.maps()[1].max())
        return 4 if w == 3 else w

    def blocks(self):
        """SPD blocks (κ = 1e3) and their exact inverses Q diag(1/λ) Q'."""
        if self._blocks is None:
            self._blocks = spd_blocks(self.sizes, 10 * self.seed, kappa=1e3)
        return self._blocks

    def vectors(self):
        rng = np.random.default_rng(self.seed + 1)
        n = self.maps()[2]
        # x (applies), b, and a non-zero start (small: ‖S x0‖ stays below ‖b‖, so the solve is no longer than from 0)
        return rng.standard_normal(n), rng.standard_normal(n), 1e-4 * rng.standard_normal(n)

    def n_own(self, rank, tiles, nn):
        """Entries of the exchanged table rank `rank` produces (operators.hpp): one per (owned row, contributor of its Γ
        node), plus one partial-dot slot per streamed tile — two for the Neumann-Neumann operator (r'r and r'z)."""
        g, cnt, _ = self.maps()
        lo, hi = self.slices()[rank]
        rows = sum(int(cnt[g[d]].sum()) for d in range(lo, hi))
        active = sum(1 for t in tiles if t[5])
        return rows + (2 if nn else 1) * active


def _auto_big(n_cu=N_CU):
    """The automatic rule itself gives two ranks different tilings, one of them 16x2 (owned rows per CU >= 24): as few rows
    as that threshold allows, in blocks of at most 2048 rows, on rank 0; a few dozen rows on rank 1 (4x1)."""
    need = 24 * n_cu
    nblk = -(-need // 2048)
    size = -(-need // nblk)
    sizes = [size] * nblk + [96, 65, 33]
    return Case("auto_big", sizes, 31, 2, slices=[(0, nblk), (nblk, nblk + 3)], big=True,
                branch="automatic rule: 16x2 on rank 0, 4x1 on rank 1")


def cases(n_cu=N_CU):
    t = []
    for w in (2, 3, 4):
        t.append(Case(f"uneven_w{w}", [130, 65, 96, 33, 47], 11, w, branch="5 blocks: slices of unequal length"))
    t.append(Case("blockless_world", [480, 65, 33], 12, 4, modes=True, sequence=True,
                  branch="world > ndom: rank 0 owns nothing, n_active == 0, k_xchg_push with n_own == 0 beside direct peers"))
    t.append(Case("blockless_empty", [0, 0, 0, 300, 65, 33], 13, 2, modes=True,
                  branch="every block of rank 0 has 0 rows: n_active == 0"))
    t.append(Case("empty_inside", [0, 48, 0, 33, 0, 0, 480, 0, 17, 0], 14, 2,
                  branch="0-row blocks first, in the middle and last within an owning slice"))
    t.append(Case("tiny", [1, 2, 3, 4, 5, 7, 31, 33, 63, 65, 480], 15, 3, modes=True, sequence=True,
                  branch="blocks below PART_ROWS and below one tile; last partial slot of a block covers < 4 rows"))
    sizes = [480, 300, 257, 129, 65, 33]     # 316 partial-dot slots: more than one per summing thread (PART_LANES = 256)
    t.append(Case("mixed_tilings_a", sizes, 16, 3, tilings=[(16, 2), (4, 1), (8, 4)], modes=True,
                  branch="ranks tiled 16x2 / 4x1 / 8x4; owner-duty tiles of a non-owned block longer than 64 waves"))
    t.append(Case("mixed_tilings_b", sizes, 16, 3, tilings=[(16, 1), (8, 1), (4, 4)], modes=True,
                  branch="ranks tiled 16x1 / 8x1 / 4x4"))
    t.append(_auto_big(n_cu))
    t.append(Case("w1", [96, 65, 33, 17], 17, 2, cover=96 + 65 + 33 + 17, branch="no shared node: W = 1, slot_sum's generic loop"))
    t.append(Case("w2", [96, 66, 34, 16], 18, 2, cover=190, branch="22 nodes in 2 blocks, the rest in 1: W = 2"))
    t.append(Case("w3", [300, 65, 33, 40, 20], 19, 2, max_share=3, branch="largest multiplicity 3, widened to W = 4"))
    t.append(Case("hub6", [300, 96, 65, 48, 33, 17], 20, 3, hub=6, fold=False, branch="W = 6: unfolded loop, all-reduce of the n_Γ W slot table"))
    t.append(Case("wide", [2049, 129, 33], 21, 2, fold=False, branch="max_ld > GEMV_PANEL: unfolded loop"))
    # push_chunks: n_own of rank 0's S on either side of XCHG_PUSH_CHUNK; sizes and seeds found by search (tests assert the value)
    for name, sz, seed in PUSH_CASES:
        t.append(Case(name, sz, seed, 2, tilings=[(16, 2), "auto"], slices=[(0, len(sz) - 1), (len(sz) - 1, len(sz))], push=True,
                      maxit=8,                  # the case is about the size of the exchange: the solves are capped
                      branch="k_xchg_push chunks"))
    # stage_sizes: n_Γ W + 4 on either side of the loopback self-test's 16384 doubles, and past the 65536 entries one
    # pass of the 256 x 256 grid of k_xchg_stage / k_xchg_sum covers; 64-row blocks laid end to end (cover_maps)
    t.append(Case("stage_16384", [64] * 255 + [60], 22, 2, cover=8190, maxit=6, no_fold_env=True,
                  branch="n_Γ W + 4 = 16384 (W = 2): the staging of the self-test just holds"))
    t.append(Case("stage_16385", [64] * 255 + [61], 23, 2, cover=16381, maxit=6, no_fold_env=True,
                  branch="n_Γ W + 4 = 16385 (W = 1): staging re-reserved by the operator's constructor"))
    t.append(Case("stage_65600", [64] * 1025, 24, 2, cover=32800, maxit=6, no_fold_env=True,
                  branch="n_Γ W = 65600 > 65536 (W = 2): stride loop of k_xchg_stage / k_xchg_sum"))
    return t


# (name, sizes, seed): rank 0 owns all blocks but the last. n_own of its S with tiling 16x2 is the number in the name.
PUSH_CASES = [("push_4096", [900, 927, 1, 1, 200], 102),      # one chunk, full
              ("push_4097", [900, 928, 1, 1, 200], 107),      # two chunks, the second holds one entry
              ("push_8260", [1950, 1930, 200], 100)]          # three chunks


def local_cases():
    """Local-only maps (C ABI: NULL gather lists for the other ranks' subdomains): the slot width is then each rank's own.
    `local_equal`: both ranks find width 4. `local_unequal`: rank 0's blocks share node 0 four ways, rank 1's two blocks at
    most two ways."""
    return [Case("local_equal", [300, 33, 48, 17, 40, 24], 49, 2, slices=[(0, 3), (3, 6)], fold=False,
                 branch="local-only maps, equal widths"),
            Case("local_unequal", [300, 33, 48, 17, 40, 24], 41, 2, hub=4, slices=[(0, 4), (4, 6)], fold=False,
                 branch="local-only maps, widths 4 and 2")]


def local_width(c, r):
    """Slot width rank r derives from the gather lists of its own slice alone (LocalMaps::build, 3 widened to 4)."""
    g, _, n = c.maps()
    lo, hi = c.slices()[r]
    w = int(np.bincount(np.concatenate([g[d] for d in range(lo, hi)]), minlength=n).max())
    return 4 if w == 3 else w


def case(name, n_cu=N_CU):
    return {c.name: c for c in cases(n_cu)}[name]


# ------------------------------------------------------------------ the host tile list (csrc/dense_tiles.hpp)
def build_checker(out_dir, sanitize=False):
    exe = os.path.join(str(out_dir), "dense_tiles_check" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Wextra", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "dense_tiles_check.cpp")])
    return exe


def tile_input(c, n_cu=N_CU, line=16, sharded=True):
    words = [c.ndom, c.world, n_cu, line, int(sharded)] + c.sizes
    for (lo, hi), tl in zip(c.slices(), c.tilings):
        words += [lo, hi] + ([0, 0] if tl == "auto" else list(tl))
    return " ".join(str(w) for w in words) + "\n"


def tile_lists(exe, cs, tmp, n_cu=N_CU, line=16):
    """name -> per rank dict(waves, rpw, part_total, max_nd, max_ld, elems, moff, ld, tiles [nt, 7]) from one run of the driver."""
    files = []
    for c in cs:
        fn = os.path.join(str(tmp), f"{c.name}_{line}.txt")
        with open(fn, "w") as f:
            f.write(tile_input(c, n_cu, line))
        files.append(fn)
    out = subprocess.run([exe] + files, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cs)
    res = {}
    for c, ln in zip(cs, lines):
        ranks = json.loads(ln)["ranks"]
        for r in ranks:
            r["tiles"] = np.array(r["tiles"], dtype=np.int64).reshape(-1, 7)
        res[c.name] = ranks
    return res


# ------------------------------------------------------------------ operators of one rank, with its own tiling
TILING_LOCK = threading.Lock()


def rank_ops(api, ctx, c, r, S, Pi, shard_nn, storage="f64"):
    """S sharded over the case's slices, ΠS sharded too or replicated. MI355_GEMV_WAVES / MI355_GEMV_RPW are read when an
    operator is constructed, and construction is not collective: a rank sets them, creates its operators and unsets them,
    under one lock shared by the ranks — so every rank has its own tiling."""
    g, cnt, _ = c.maps()
    lo, hi = c.slices()[r]
    tl = c.tilings[r]
    own = lambda blocks: [blocks[d] if lo <= d < hi else None for d in range(c.ndom)]
    with TILING_LOCK:
        try:
            if tl != "auto":
                os.environ["MI355_GEMV_WAVES"], os.environ["MI355_GEMV_RPW"] = str(tl[0]), str(tl[1])
            A = api.LocalSchurs(ctx, own(S), g, cnt, dom_slice=(lo, hi))
            if shard_nn:
                M = api.NeumannNeumannSchurPreconditioner(ctx, own(Pi), g, cnt, dom_slice=(lo, hi), storage=storage)
        finally:
            os.environ.pop("MI355_GEMV_WAVES", None)
            os.environ.pop("MI355_GEMV_RPW", None)
        if not shard_nn:   # a replicated operator has ONE tiling on all ranks (the default): its partials must add up alike everywhere
            M = api.NeumannNeumannSchurPreconditioner(ctx, Pi, g, cnt, dom_slice=(0, c.ndom), storage=storage)
    return A, M
