"""Synthetic partitioned full systems for the edge suite of the full-system preconditioners (csrc/nn_induced.hpp:
k_gemv_nni, k_nni_assemble; csrc/full_split.hpp: k_lo_zgamma, k_split_coupling; csrc/lorasc.hpp: k_lo_correct).

Not a conftest: tests/test_full_synth_cpu.py and tests/test_gpu_full_synth_edges.py import it. Everything here runs on the host.

A case is a `lorasc_ref.Case` whose `P` is a stand-in for `fem.SchurProblem` (`A_IIdd`, `A_IΓdd`, `A_ΓΓdd`, `sub.gather_idx`,
`sub.node_Γ_cnt`), so `nn_induced_ref.apply_neumann_neumann_induced` and `lorasc_ref.apply_lorasc` run on it unchanged.

  per subdomain   `setup_synth.ladder(widths, n_gamma = n_Γd, shift = 0.5)`: two or three BFS levels of 3 ... 40 nodes whatever
                  n_Γd is (κ(A_IId) < 1e2); level 0 holds 3 n_Γd nodes where n_Γd <= 13 (columns with several entries) and
                  fewer than n_Γd / 4 where n_Γd >= 128 (most columns empty).
  gather maps     `krylov_synth.exact_maps`: an exact n_Γ, an exact largest multiplicity, node 0 in that many blocks.
  pos_I / pos_Γ   a random permutation of 0 .. n-1 cut into the interiors (concatenated) and Γ.
  A_IΓd           the local columns scattered through the gather list (LORASC's Γ-global form).
  A_ΓΓ            apply-only cases: the 5-diagonal (-1/2, -1, 4 + U(0, 1), -1, -1/2), diagonally dominant; `solve`: Σ_d R_d' A_ΓΓdd R_d.
  ΠS_d            apply-only cases: NON-symmetric N(0, 1) / sqrt(n_Γd) (the apply is linear in them; symmetry would hide a
                  transposition); `solve`: left to `nn_induced_ref.prepare` (the pseudo-inverses of the ladder blocks' S_d).
  A, b            the assembled full matrix in the rows of pos_I / pos_Γ and a random right-hand side. Every subdomain's local
                  matrix is strictly diagonally dominant, so the A of `solve` is SPD; the apply-only cases never use theirs."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import scipy.sparse as sp

import krylov_synth as ks
import lorasc_ref as lr
import setup_synth as ssy

GEMV_PANEL = 2048
LO_MAX_NEV = 1024
RPWS, WAVES = (1, 2, 4), (4, 8, 16)
TILINGS = tuple((rpw, waves) for waves in WAVES for rpw in RPWS)
SHIFT = 0.5
EPS = 1e-6                                   # stop threshold of the `solve` case

TILE_SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
PANEL_SIZES = (2032, 2033, 2048, 2049, 5, 33, 64)
WG_REMAINDERS = (1, 63, 64, 65, 128, 192, 193, 255, 256)
WG_CASES = tuple(f"wg{r}" for r in WG_REMAINDERS)
NEV_ALL = (0, 1, 2, 3, 4, 5, 255, 256, 257, 1024)
WIDTH_CASES = ("w1", "w3", "hub6", "bare")
INDUCED_CASES = ("tiles", "panels") + WIDTH_CASES + ("solve",)
LORASC_CASES = WIDTH_CASES + WG_CASES
ALL_CASES = INDUCED_CASES + WG_CASES

# name -> (block sizes, n_Γ, largest multiplicity, seed)
_TABLE = {
    "tiles": (TILE_SIZES, 700, 4, 1),
    "panels": (PANEL_SIZES, 3600, 3, 2),
    "w1": ((130, 97, 64, 33, 9), 333, 1, 3),
    "w3": ((130, 97, 64, 33, 9), 200, 3, 4),
    "hub6": ((130, 97, 64, 33, 9, 17, 40), 250, 6, 5),
    "bare": ((130, 64, 33, 9, 12), 180, 2, 6),
    "solve": ((257, 129, 65, 33, 9, 256), 600, 3, 7),
}
for _r in WG_REMAINDERS:
    _TABLE[f"wg{_r}"] = (ks.split_sizes(int((768 + _r) * 1.15), 4) + (9,), 768 + _r, 2, 20 + _r)
BARE_NODE = 0                                # `bare`: the Γ node no subdomain couples to its interior (held by blocks 0 and 1)
BARE_EMPTY = 4                               # `bare`: the subdomain with n_i = 0
SOLVE_WIDTHS = ([40, 40, 40], [30, 40, 40], [40, 40, 30], [40, 40], [27, 40, 40], [40, 35, 40])


@dataclass
class Sub:
    gather_idx: list
    node_Γ_cnt: np.ndarray

    @property
    def ndom(self):
        return len(self.gather_idx)

    @property
    def n_Γ(self):
        return int(self.node_Γ_cnt.size)


@dataclass
class Plan:
    """what the set-up plan and the two operators take of a `fem.SchurProblem`"""
    A_IIdd: list
    A_IΓdd: list
    A_ΓΓdd: list
    sub: Sub


def _empty_solve(b):
    return np.zeros_like(np.asarray(b, dtype=np.float64))


@dataclass
class FullCase(lr.Case):
    widths: tuple = ()                       # per subdomain: the BFS level widths of its ladder ([] for n_i = 0)
    width: int = 0                           # largest multiplicity of the gather maps
    consistent: bool = False                 # A_ΓΓ assembled from the A_ΓΓdd, ΠS_d the pseudo-inverses: a system to solve

    @property
    def sizes(self):
        return [int(np.asarray(g).size) for g in self.P.sub.gather_idx]

    @property
    def n_i(self):
        return [int(np.asarray(p).size) for p in self.pos_I]

    @property
    def slot_width(self):
        return 4 if self.width == 3 else self.width

    @property
    def nwg(self):
        return -(-self.n_Γ // 256)

    def solves(self, refine: int):
        key = ("solves", refine)
        if key not in self.__dict__:
            self.__dict__[key] = ([lr.Solve(M, refine) if M.shape[0] else _empty_solve for M in self.A_IId],
                                  lr.Solve(self.A_ΓΓ, refine))
        return self.__dict__[key]


def level_widths(n_Γd, rng):
    """two or three levels of 3 ... 40 nodes; level 0: 3 n_Γd nodes for n_Γd <= 13, fewer than n_Γd / 4 for n_Γd >= 128"""
    if n_Γd <= 13:
        w0 = max(3, 3 * n_Γd)
    elif n_Γd >= 128:
        w0 = int(rng.integers(3, min(41, n_Γd // 4)))
    else:
        w0 = int(rng.integers(3, 41))
    return [w0] + [int(v) for v in rng.integers(3, 41, int(rng.integers(1, 3)))]


def banded_spd(n, rng):
    off1, off2 = np.full(max(n - 1, 0), -1.0), np.full(max(n - 2, 0), -0.5)
    A = sp.diags([off2, off1, 4.0 + rng.random(n), off1, off2], [-2, -1, 0, 1, 2], shape=(n, n), format="csc")
    A.sort_indices()
    return A


def scatter_columns(B, g, n_Γ):
    """the local columns of A_IΓdd scattered through the gather list: A_IΓd with Γ-global columns"""
    B = sp.coo_matrix(B)
    out = sp.csc_matrix((B.data, (B.row, np.asarray(g)[B.col])), shape=(B.shape[0], n_Γ))
    out.sort_indices()
    return out


def assemble_ΓΓ(A_ΓΓdd, g, n_Γ):
    out = sp.csc_matrix((n_Γ, n_Γ))
    for G, gd in zip(A_ΓΓdd, g):
        G = sp.coo_matrix(G)
        out = out + sp.csc_matrix((G.data, (np.asarray(gd)[G.row], np.asarray(gd)[G.col])), shape=(n_Γ, n_Γ))
    out.sum_duplicates()
    out.sort_indices()
    return out


def full_matrix(A_IId, A_IΓd, A_ΓΓ, pos_I, pos_Γ):
    """[A_II A_IΓ; A_IΓ' A_ΓΓ] in the (I_1, ..., I_ndom, Γ) ordering, moved to the rows of pos_I / pos_Γ"""
    A_IΓ = sp.vstack(A_IΓd, format="csr") if A_IΓd else sp.csr_matrix((0, A_ΓΓ.shape[0]))
    K = sp.coo_matrix(sp.bmat([[sp.block_diag(A_IId, format="csr"), A_IΓ], [A_IΓ.T, A_ΓΓ]]))
    perm = np.concatenate(list(pos_I) + [pos_Γ])
    A = sp.csr_matrix((K.data, (perm[K.row], perm[K.col])), shape=K.shape)
    A.sum_duplicates()
    A.sort_indices()
    return A


def couple_column(s, col):
    """Two local columns must hold an entry whatever the ladder drew. Γ node 0 lies in the first `width` blocks (exact_maps):
    without an entry in each of them the node never has `width` column segments. And the last column of every block: the
    interior sees z_loc only through non-empty columns, and the last row is the one a tile-edge guard gets wrong. An empty
    column gets a coupling of -1 to a level-0 node (the levels stay as they are) and both diagonals the same weight (the
    dominance stays as it is)."""
    B = sp.csc_matrix(s.A_IΓ)
    if B.indptr[col + 1] > B.indptr[col]:
        return
    row, (n_I, n_Γd) = int(B.indices[0]), B.shape
    s.A_IΓ = ssy._csc(B + sp.csc_matrix(([-1.0], ([row], [col])), shape=B.shape), n_I, n_Γd)
    s.A_II = ssy._csc(s.A_II + sp.csc_matrix(([1.0], ([row], [row])), shape=s.A_II.shape), n_I, n_I)
    s.A_ΓΓ = ssy._csc(s.A_ΓΓ + sp.csc_matrix(([1.0], ([col], [col])), shape=s.A_ΓΓ.shape), n_Γd, n_Γd)


def make_case(name):
    sizes, n_Γ, width, seed = _TABLE[name]
    rng = np.random.default_rng(7000 + seed)
    g, cnt, _ = ks.exact_maps(sizes, n_Γ, width, rng)
    consistent, bare = name == "solve", name == "bare"
    subs, widths = [], []
    for d, n_Γd in enumerate(sizes):
        if bare and d == BARE_EMPTY:
            subs.append(ssy.empty_interior(n_Γd))
            widths.append([])
            continue
        w = list(SOLVE_WIDTHS[d]) if consistent else level_widths(n_Γd, rng)
        # `bare` takes two Γ couplings per level-0 node, so that every one of them keeps one when a column is emptied
        s = ssy.ladder(w, degree=3, n_gamma=n_Γd, gamma_deg=2 if bare else 1, seed=100 * seed + d, shift=SHIFT)
        if bare and BARE_NODE in g[d]:
            B = sp.lil_matrix(s.A_IΓ)
            B[:, int(np.flatnonzero(g[d] == BARE_NODE)[0])] = 0.0
            s.A_IΓ = ssy._csc(sp.csc_matrix(B), *B.shape)
            s.A_IΓ.eliminate_zeros()
        elif width > 1 and d < width:
            couple_column(s, int(np.flatnonzero(g[d] == 0)[0]))
        if not (bare and g[d][-1] == BARE_NODE):
            couple_column(s, n_Γd - 1)
        subs.append(s)
        widths.append(w)
    n_i = [s.A_II.shape[0] for s in subs]
    n = sum(n_i) + n_Γ
    perm = rng.permutation(n).astype(np.int64)
    off = np.concatenate(([0], np.cumsum(n_i)))
    pos_I = [perm[off[d]:off[d + 1]] for d in range(len(sizes))]
    pos_Γ = perm[off[-1]:]
    P = Plan([s.A_II for s in subs], [s.A_IΓ for s in subs], [s.A_ΓΓ for s in subs], Sub(g, cnt))
    A_IΓd = [scatter_columns(s.A_IΓ, gd, n_Γ) for s, gd in zip(subs, g)]
    A_ΓΓ = assemble_ΓΓ(P.A_ΓΓdd, g, n_Γ) if consistent else banded_spd(n_Γ, rng)
    A = full_matrix(P.A_IIdd, A_IΓd, A_ΓΓ, pos_I, pos_Γ)
    c = FullCase(name, P, P.A_IIdd, A_IΓd, A_ΓΓ, A, rng.standard_normal(n), pos_I, pos_Γ, None, tuple(widths), width, consistent)
    if not consistent:
        c.__dict__["ΠSd"] = [np.asfortranarray(rng.standard_normal((m, m)) / np.sqrt(m)) for m in sizes]   # nn_induced_ref.prepare
    if 0 in n_i:                             # nn_induced_ref builds its interior solves itself: a 0 x 0 block has no LU
        for refine in (0, 2, 3):
            c.__dict__[("nni_solves", refine)] = [lr.Solve(M, refine) if M.shape[0] else _empty_solve for M in P.A_IIdd]
    return c


@lru_cache(maxsize=None)
def case(name):
    return make_case(name)


def drop():
    """forget the built cases (`panels` holds 130 MB of blocks)"""
    case.cache_clear()


def holders(c, node):
    """(subdomain, local column) of every block that holds a Γ node, ascending subdomain"""
    return [(d, int(np.flatnonzero(np.asarray(g) == node)[0])) for d, g in enumerate(c.P.sub.gather_idx) if node in g]


def column_segments(c):
    """per Γ node the number of subdomains with a non-empty A_IΓdd column there: the `gseg` range of k_lo_zgamma"""
    seg = np.zeros(c.n_Γ, dtype=np.int64)
    for B, g in zip(c.P.A_IΓdd, c.P.sub.gather_idx):
        seg[np.asarray(g)[np.diff(sp.csc_matrix(B).indptr) > 0]] += 1
    return seg


def padded_ld(n, line):
    """row stride of a block (csrc/dense_tiles.hpp): whole 128-byte lines, one more where the stride is a multiple of 2 KiB"""
    l = -(-n // line) * line
    return l + line if (l % (16 * line) == 0 and l != GEMV_PANEL) else l
