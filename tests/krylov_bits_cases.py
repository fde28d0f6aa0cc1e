"""Cases of tests/test_gpu_krylov_bits.py and tests/golden/make_krylov_golden.py: the smallest solves of tests/krylov_synth.py
and tests/eig_synth.py that reach each loop form of csrc/solvers.hpp (Loop::GENERIC, FUSED, FOLD, FOLD_BIG, CSRFOLD), its start-up
and entry variants, eager launches (chunk 0) and one-iteration replays (chunk 1).

Not a conftest. A GROUP is one problem with fresh device operators and the runs made on them, in order; a run is (label,
environment switches, chunk or None for the default, solves). The order matters in one place: on d1025w2 pcg from zero runs
twice before the random x0, so that the second takes k_entry_zero, the random x0 makes that entry report back (respec) and is
replayed through the general entry. A result is (x, it, res_norm) and, for the eigCG family, the returned vectors."""
from __future__ import annotations

import hashlib
import os

import numpy as np

import eig_synth as es
import krylov_synth as ks
from krylov_synth import Solve

HASH_ABOVE = 4096            # x of a longer vector is held by its SHA-256
DEFAULT_CHUNK = 8
NO_FUSED, NO_CSRFOLD, NO_FOLD, NO_FOLD_DEFL = "MI355_NO_FUSED", "MI355_NO_CSRFOLD", "MI355_NO_FOLD", "MI355_NO_FOLD_DEFL"


def _fused_solves(prob):
    return [Solve(prob, kind, 0, x0, maxit) for kind in ("cg", "pcg") for maxit in (0, 1, 2) for x0 in ("zero", "rand")]


def _chunks(label, env, s):
    return [(f"{label}-chunk{c}", env, c, [s]) for c in (0, 1)]


PZ, PR = Solve("d1025w2", "pcg"), Solve("d1025w2", "pcg", x0="rand")
GROUPS = [
    ("sp1025", [("csrfold", (NO_FUSED,), None, [Solve("sp1025", "cg"), Solve("sp1025", "pcg")]),
                ("generic", (NO_FUSED, NO_CSRFOLD), None, [Solve("sp1025", k) for k in ("cg", "pcg", "pcg_id")])]
     + _chunks("csrfold", (NO_FUSED,), Solve("sp1025", "pcg")) + _chunks("generic", (NO_FUSED, NO_CSRFOLD), Solve("sp1025", "pcg"))),
    ("sp8193", [("csrfold", (), None, [Solve("sp8193", "pcg")])]),
    ("sp2048", [("generic", (NO_FUSED,), None, [Solve("sp2048", "defcg", 5), Solve("sp2048", "defpcg", 5)])]),
    ("sp1023", [("fused", (), None, _fused_solves("sp1023"))] + _chunks("fused", (), Solve("sp1023", "pcg"))),
    ("sp2049", [("fused", (), None, _fused_solves("sp2049"))]),
    ("d1025w2", [("fold", (), None, [PZ, PZ, PR, PZ]), ("fused", (NO_FOLD,), None, [PZ]), ("generic", (NO_FUSED,), None, [PZ])]
     + _chunks("fold", (), PZ)),
    ("nloc1024", [("fold", (), None, [Solve("nloc1024", "defpcg", 5), Solve("nloc1024", "defpcg", 21)]),
                  ("fused", (NO_FOLD_DEFL,), None, [Solve("nloc1024", "defpcg", 5), Solve("nloc1024", "defpcg", 65)])]),
    ("big8200", [("foldbig", (), None, list(ks.BIG_SOLVES))] + _chunks("foldbig", (), ks.BIG_SOLVES[0])),
]
# the eigCG family: eigcg on a sparse matrix runs the single-workgroup loop, eigdefpcg always the generic one
EIG = [es.BY_ID["b-eigcg-synth255-3-8-after"], es.BY_ID["a-eigdefpcg-synth257-3-8-after"]]


def _names():
    out = []
    for prob, runs in GROUPS:
        for label, env, chunk, solves in runs:
            out += [f"{prob}/{label}/{k}:{s.id}" for k, s in enumerate(solves)]
    return out + ["eig/" + c.id for c in EIG]


NAMES = _names()
assert len(set(NAMES)) == len(NAMES)


def probs_of(api, ctx, orc):
    """krylov_synth's problems with Π from mi_nn_pinv, as tests/test_gpu_krylov_edges.py builds them, and eig_synth's"""
    def pinv(d, S):
        sizes = np.array(d.sizes, dtype=np.int64)
        flat = api.nn_pinv(ctx, sizes, np.concatenate([np.asarray(B, order="F").ravel(order="F") for B in S]))
        off = np.concatenate([[0], np.cumsum(sizes * sizes)])
        return [np.asfortranarray(flat[off[k]:off[k + 1]].reshape(n, n, order="F")) for k, n in enumerate(d.sizes)]
    return ks.Problems(orc, pinv), es.Problems(orc)


def _make_ops(api, ctx, probs, prob):
    if prob in ks.SPARSE:
        A = probs.matrix(prob)
        return {"A": api.SparseMatrixCSC(ctx, A), "jacobi": api.JacobiPreconditioner(ctx, A.diagonal()),
                "identity": api.IdentityPreconditioner(ctx, A.shape[0])}
    g, cnt, n = probs.maps(prob)
    return {"A": api.LocalSchurs(ctx, probs.blocks(prob), g, cnt),
            "nn": api.NeumannNeumannSchurPreconditioner(ctx, probs.pi_blocks(prob), g, cnt)}


def _sha(h, *arrays):
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())


def input_digests(probs, eprobs):
    """SHA-256 of everything a group's solves read: the matrix or the blocks, Π and the gather maps, b, both x0 and every W"""
    out = {}
    for prob, runs in GROUPS:
        h = hashlib.sha256()
        if prob in ks.SPARSE:
            A = probs.matrix(prob)
            _sha(h, A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data)
        else:
            g, cnt, n = probs.maps(prob)
            _sha(h, *[np.asarray(a, dtype=np.int64) for a in g], np.asarray(cnt, dtype=np.int64),
                 *[np.asarray(B, order="F").ravel(order="F") for B in probs.blocks(prob) + probs.pi_blocks(prob)])
        n = ks.size_of(prob)
        _sha(h, probs.b(prob), ks.x0_rand(n))
        for nvec in sorted({s.nvec for _, _, _, solves in runs for s in solves if s.nvec}):
            _sha(h, np.asarray(ks.random_W(n, nvec), order="F").ravel(order="F"))
        out[prob] = h.hexdigest()
    for c in EIG:
        h = hashlib.sha256()
        A = eprobs.scipy_matrix(c.prob)
        _sha(h, A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data, eprobs.b(c), eprobs.x0(c))
        if eprobs.W(c) is not None:
            _sha(h, np.asarray(eprobs.W(c), order="F").ravel(order="F"))
        out["eig/" + c.id] = h.hexdigest()
    return out


def run_all(api, ctx, probs, eprobs):
    """name -> result for every entry of NAMES. Environment switches are set around each solve (read when the solver is
    constructed); the chunk of the context is put back to the default."""
    out = {}
    for prob, runs in GROUPS:
        ops = _make_ops(api, ctx, probs, prob)
        try:
            for label, env, chunk, solves in runs:
                saved = {k: os.environ.get(k) for k in env}
                os.environ.update({k: "1" for k in env})
                try:
                    ctx.set_chunk(DEFAULT_CHUNK if chunk is None else chunk)
                    for k, s in enumerate(solves):
                        pre = probs.precond(s)
                        out[f"{prob}/{label}/{k}:{s.id}"] = ks.run(api, s, ops["A"], ops[pre] if pre else None, probs.b(prob),
                                                                  probs.x0(s), probs.W(s))
                finally:
                    ctx.set_chunk(DEFAULT_CHUNK)
                    for k, v in saved.items():
                        if v is None:
                            del os.environ[k]
                        else:
                            os.environ[k] = v
        finally:
            for op in ops.values():
                op.close()
            if prob in ks.DENSE:
                probs.drop(prob)
    for c in EIG:
        M = eprobs.scipy_matrix(c.prob)
        A, J = api.SparseMatrixCSC(ctx, M), api.JacobiPreconditioner(ctx, M.diagonal())
        try:
            out["eig/" + c.id] = es.run(api, c.kind, A, J, eprobs.b(c), eprobs.x0(c), eprobs.W(c), c.nvec, c.spdim, c.maxit, c.eps)
        finally:
            A.close()
            J.close()
    return out


def pack(results, digests):
    """the arrays of the fixture: it, res_norm and x (its SHA-256 above HASH_ABOVE entries) per name, V of the eigCG family,
    and the digest of every group's inputs"""
    out = {}
    for name, r in results.items():
        x, it, res = r[:3]
        out[name + "/it"] = np.int64(it)
        out[name + "/res"] = np.asarray(res, dtype=np.float64)
        if x.size > HASH_ABOVE:
            out[name + "/sha256"] = np.array(hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest())
        else:
            out[name + "/x"] = x
        if len(r) > 3:
            out[name + "/V"] = np.asarray(r[3])
    for name, h in digests.items():
        out["inputs/" + name] = np.array(h)
    return out
