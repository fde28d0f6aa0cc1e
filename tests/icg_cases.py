"""Cases of tests/test_gpu_icg_bits.py, shared with the generator of its fixture (tests/golden/make_icg_golden.py): the
device interior CG (csrc/operators.hpp InteriorCg, the k_icg_* kernels of csrc/kernels.hpp) with every `Pl` — none,
Diagonal(A_II), the AMG hierarchy of the stacked A_II — on the interior sets of tests/sparse_synth.py and the cases of
tests/interior_amg_ref.py. Every operator is created under MI355_ICG_CHUNK=1 (one iteration per replay, so the increase of
`interior_iterations()` is the count of the slowest subdomain) and solves `u = interior_solutions(0, b_I)` once, between
two S-applies to a fixed x_Γ.

`wide` (300 000 rows, one subdomain) is created under MI355_ICG_PIECES=256: its pieces are longer than 4 NT = 1024 rows, so
the vector kernels load rows past the four they request ahead of the reduction (`pieces()` restates the cut;
tests/test_icg_cases_cpu.py asserts it). Its AMG hierarchy is hand-made: three consecutive rows per aggregate, the last
aggregate takes the remainder, 300 000 -> 100 000 -> ... -> 137.

`run_all(api, ctx)` returns {"case/pl": (u, iterations, y = S x_Γ)}; `input_digests()` the SHA-256 of every case's inputs
(values of A_II, b_I, x_Γ, aggregates), which the fixture stores next to the results: where they differ, numpy / LAPACK made
other inputs and the bits of the results say nothing about the kernels. `run_sequence(api, ctx)` walks ONE operator through
none -> diagonal -> AMG -> none -> AMG -> diagonal -> set_values -> diagonal -> AMG and names the entry of `run_all` (a
fresh operator each) that every step has to reproduce."""
import hashlib
import importlib
import os
from contextlib import contextmanager

import numpy as np
import scipy.sparse as sp

import interior_amg_ref as ir
import sparse_synth as ss

SYNTH = ("mixed", "capped", "longrow")                   # none, diagonal
AMG_CASES = ("n12_3", "empty", "blocks2", "edge_rows")   # none, diagonal, AMG
SECOND = "blocks2"                                       # ... and its second values, as `blocks2_2`
WIDE_PIECES = 256
PLS = ("none", "diagonal", "amg")
NAMES = tuple([f"{c}/{p}" for c in SYNTH for p in PLS[:2]] +
              [f"{c}/{p}" for c in ("wide",) + AMG_CASES + (SECOND + "_2",) for p in PLS])
SEQUENCE = (("none", "blocks2/none"), ("diagonal", "blocks2/diagonal"), ("amg", "blocks2/amg"), ("none", "blocks2/none"),
            ("amg", "blocks2/amg"), ("diagonal", "blocks2/diagonal"), ("set_values", None), ("diagonal", "blocks2_2/diagonal"),
            ("amg", "blocks2_2/amg"))


@contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def triple_aggregates(n, coarsest=256):
    """(sizes, aggs): three consecutive rows per aggregate, the last one also takes the n mod 3 rows left over"""
    sizes, aggs = [n], []
    while sizes[-1] > coarsest:
        m = sizes[-1]
        aggs.append(np.minimum(np.arange(m, dtype=np.int64) // 3, m // 3 - 1))
        sizes.append(m // 3)
    return sizes, aggs


class Inputs:
    """what one operator is made from, and the `Pl`s it is solved with"""

    def __init__(self, A_II, A_IΓ, A_ΓΓ, gather_idx, node_Γ_cnt, b_I, reltol, pls, amg=None, environ=None):
        self.A_II, self.A_IΓ, self.A_ΓΓ, self.gather_idx, self.node_Γ_cnt = A_II, A_IΓ, A_ΓΓ, gather_idx, node_Γ_cnt
        self.b_I, self.reltol, self.pls, self.amg = np.asarray(b_I, dtype=np.float64), reltol, pls, amg
        self.environ = dict(MI355_ICG_CHUNK=1, MI355_ICG_FUSED=0, **(environ or {}))
        self.x_Γ = np.random.default_rng(7).standard_normal(np.size(node_Γ_cnt))

    def digest(self):
        h = hashlib.sha256()
        for A in self.A_II:
            A = sp.csc_matrix(A)
            A.sort_indices()
            for a in (A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.astype(np.float64)):
                h.update(a.tobytes())
        h.update(self.b_I.tobytes())
        h.update(self.x_Γ.tobytes())
        if self.amg is not None:
            for a in [np.asarray(self.amg[0], dtype=np.int64)] + [np.asarray(a, dtype=np.int64) for a in self.amg[1]]:
                h.update(a.tobytes())
        return h.hexdigest()

    def op(self, api, ctx):
        with env(**self.environ):
            return api.MatrixFreeLocalSchurs(ctx, self.A_II, self.A_IΓ, self.A_ΓΓ, self.gather_idx, self.node_Γ_cnt, None,
                                             reltol=self.reltol)

    def select(self, S, pl):
        if pl == "amg":
            S.interior_amg(sizes=self.amg[0], aggregates=self.amg[1])
        else:
            S.interior_precond(None if pl == "none" else pl)

    def solve(self, S):
        """(u, iterations of the solve for u, y = S x_Γ). The apply comes first and last: it solves into the operator's own
        vector, so it replays the graph the apply before it captured — after a change of `Pl`, the graph of the `Pl` before
        if `select` kept it — while interior_solutions solves into another vector and captures anew."""
        y = S * self.x_Γ
        it0 = S.interior_iterations()
        u = S.interior_solutions(np.zeros(self.x_Γ.size), self.b_I)
        it = S.interior_iterations() - it0
        assert np.array_equal(S * self.x_Γ, y, equal_nan=True)
        return u, it, y


_inputs = {}


def inputs(fem):
    if not _inputs:
        sets = ss.interior_sets(SYNTH + ("wide",))
        for name in SYNTH + ("wide",):
            s = sets[name]
            wide = name == "wide"
            _inputs[name] = Inputs(s.A_II, s.A_IΓ, s.A_ΓΓ, s.gather_idx, s.node_Γ_cnt, np.concatenate(s.b_I), s.reltol,
                                   PLS if wide else PLS[:2], triple_aggregates(s.n_i[0]) if wide else None,
                                   dict(MI355_ICG_PIECES=WIDE_PIECES) if wide else None)
        for name in AMG_CASES:
            C = ir.case(fem, name)
            amg = ir.pair_aggregates(C.A_II) if C.aggs is not None else fem.prepare_interior_amg(C.A_II, **C.kw)
            _inputs[name] = Inputs(C.A_II, C.A_IΓ, C.A_ΓΓ, C.gather_idx, C.node_Γ_cnt, C.b_I(), ir.RELTOL, PLS, amg)
            if name == SECOND:
                _inputs[name + "_2"] = Inputs(C.A_II2, C.A_IΓ2, C.A_ΓΓ2, C.gather_idx, C.node_Γ_cnt, C.b_I(), ir.RELTOL, PLS, amg)
    return _inputs


def _fem(api):
    return importlib.import_module(api.__package__ + ".fem")


def input_digests(fem):
    return {name: I.digest() for name, I in inputs(fem).items()}


def run_all(api, ctx):
    out = {}
    for name, I in inputs(_fem(api)).items():
        for pl in I.pls:
            S = I.op(api, ctx)          # a fresh operator for every `Pl`
            try:
                I.select(S, pl)
                out[f"{name}/{pl}"] = I.solve(S)
            finally:
                S.close()
    return out


def run_sequence(api, ctx):
    """[(step, entry of run_all it has to equal, u, iterations, y)] on one operator of `blocks2`"""
    fem = _fem(api)
    I = inputs(fem)[SECOND]
    C = ir.case(fem, SECOND)
    out = []
    S = I.op(api, ctx)
    try:
        for step, (pl, want) in enumerate(SEQUENCE):
            if pl == "set_values":
                S.set_values(*ir.new_values(C))
                continue
            I.select(S, pl)
            out.append((f"{step}:{pl}", want) + I.solve(S))
    finally:
        S.close()
    return out


def pack(results, digests):
    """the arrays of the fixture: u, y and the count per entry (of `wide`: the SHA-256 of u.tobytes() and the count), and the
    digest of every case's inputs"""
    out = {}
    for name, (u, it, y) in results.items():
        out[name + "/y"] = y
        if name.startswith("wide/"):
            out[name + "/sha256"] = np.array(hashlib.sha256(np.ascontiguousarray(u).tobytes()).hexdigest())
        else:
            out[name + "/u"] = u
        out[name + "/it"] = np.int64(it)
    for name, h in digests.items():
        out["inputs/" + name] = np.array(h)
    return out


# ------------------------------------------------------------------ the pieces of the vector kernels, restated
def row_blocks(indptr, breaks=()):
    """csrc/spmv_blocks.hpp spmv_row_blocks: [(r0, r1)]"""
    n, out, r, nb = len(indptr) - 1, [], 0, 0
    breaks = list(breaks)
    while r < n:
        while nb < len(breaks) and breaks[nb] <= r:
            nb += 1
        limit = min(breaks[nb], n) if nb < len(breaks) else n
        e = r + 1
        while e < limit and indptr[e + 1] - indptr[r] <= ss.SPMV_TILE:
            e += 1
        if e < limit and indptr[e] & 1:
            for back in (1, 2, 3):
                if e - back > r and indptr[e - back] & 1 == 0:
                    e -= back
                    break
        out.append((r, e))
        r = e
    return out


def pieces(indptr, offs, target):
    """InteriorCg::build_fold: the row ranges [(lo, hi)] of the pieces of subdomains with the offsets `offs` (ndom + 1),
    MI355_ICG_PIECES = target. rows_per = max(256, ceil(n / max(256, target))); a subdomain is cut at the first rows of the
    eight XCD shares of the row blocks (spmv_xcd_rows), every part into ceil(rows / rows_per) equal runs."""
    n = len(indptr) - 1
    blocks = row_blocks(indptr, list(offs[:-1]))
    per = (len(blocks) + 7) >> 3
    xr = [blocks[x * per][0] if x * per < len(blocks) else n for x in range(8)] + [n]
    target = max(256, target)
    rows_per = max(ss.NT, (n + target - 1) // target)
    out = []
    for d in range(len(offs) - 1):
        for x in range(8):
            lo, hi = max(int(offs[d]), xr[x]), min(int(offs[d + 1]), xr[x + 1])
            if hi <= lo:
                continue
            cnt = (hi - lo + rows_per - 1) // rows_per
            out += [(lo + (hi - lo) * k // cnt, lo + (hi - lo) * (k + 1) // cnt) for k in range(cnt)]
    return out
