"""Cases of tests/test_gpu_setup_bits.py and tests/golden/make_setup_golden.py: the smallest inputs that reach every part of the
level elimination of csrc/setup_gj.hpp from each of its callers — `mi_schur_setup_run` with and without b_I, with kept levels
and with a second realization on the same plan (gj_run, both graphs); `mi_nn_pinv` on full-rank and on exactly floating
blocks (both batches of pinv_blocks_fast); one block-Jacobi operator (gj_run and pinv_blocks_fast(spd_only)) and one AMG
coarse inverse (pinv_blocks_fast(spd_only)).

Not a conftest. The inputs come from the generators of the existing GPU tests (tests/test_gpu_setup_edges.py,
tests/test_gpu_dense_edges.py, tests/block_jacobi_ref.py, tests/amg_refresh_ref.py). A case's result is a dict name -> array;
`pack` keeps arrays of more than HASH_ABOVE entries by their SHA-256."""
from __future__ import annotations

import hashlib

import numpy as np
import scipy.sparse as sp

import amg_refresh_ref as rr
import block_jacobi_ref as bjr
import setup_synth as ss
import test_gpu_dense_edges as de
import test_gpu_setup_edges as se

HASH_ABOVE = 4096
VALUE_SEED = 1234
OLD_HEAD = [(n0, k) for n0 in (33, 64, 65, 129, 257) for k in (1e4, 1e8)]
# plan -> (the cases of the first realization, those of the second: other values on the same sparsity)
PLANS = {
    "ladders": lambda: (se.ladders(), se.ladders(value_seed=VALUE_SEED)),
    "direct-1e6": lambda: ([ss.direct_inverse(n0, 1e6) for n0 in se.N0S], [ss.direct_inverse(n0, 1e6, seed=VALUE_SEED + n0) for n0 in se.N0S]),
    "direct-1e4-1e8": lambda: ([ss.direct_inverse(n0, k) for n0, k in OLD_HEAD], [ss.direct_inverse(n0, k, seed=VALUE_SEED + n0) for n0, k in OLD_HEAD]),
}
PINV_SIZES = [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 193, 1000, 2049]
PINV_KAPPA = 1e4
NAMES = ["plan/" + p for p in PLANS] + ["pinv/full-rank", "pinv/floating", "block-jacobi", "amg-coarse-inverse"]

_memo = {}


def _once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def plan_cases(plan):
    return _once("plan/" + plan, PLANS[plan])


def pinv_blocks(kind):
    """the blocks of test_pinv_full_rank_is_the_inverse / test_pinv_floating_blocks_take_the_shift at κ = 1e4, one mixed batch"""
    def make():
        out = []
        for n in PINV_SIZES:
            if kind == "full-rank":
                out.append(de.sym_from(de.orthogonal(n, n), np.geomspace(1.0, PINV_KAPPA, n) if n > 1 else np.array([PINV_KAPPA])))
            elif n >= 2:
                Q = de.orthogonal(n, n, first=np.ones(n) / np.sqrt(n))
                out.append(de.sym_from(Q, np.concatenate([[0.0], np.geomspace(1.0, PINV_KAPPA, n - 1)])))
        return out
    return _once("pinv/" + kind, make)


def block_jacobi_case():
    """test_unequal_depth_and_single_level_blocks: a block whose only level is level 0 beside a block of 5 levels"""
    def make():
        A1, s1 = bjr.ladder_matrix([10], n_gamma=6, seed=1)
        A2, s2 = bjr.ladder_matrix([2, 2, 2, 2, 2], n_gamma=6, seed=2, degree=1)
        A = sp.block_diag([A1, A2], format="csc")
        return A, [s1, s2], np.random.default_rng(VALUE_SEED).standard_normal(A.shape[0])
    return _once("block-jacobi", make)


def amg_case(fem):
    """test_mesh_pairs_bit_for_bit's N12_1: one level, the whole 12 x 12 mesh matrix is the coarsest one"""
    return _once("amg", lambda: rr.pair(fem, 12)[0])


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _csc_arrays(M):
    M = sp.csc_matrix(M)
    return [M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data]


def input_digests(fem):
    """SHA-256 of everything a case reads"""
    out = {}
    for plan in PLANS:
        arrs = []
        for cs in plan_cases(plan):
            for c in cs:
                arrs += _csc_arrays(c.A_II) + _csc_arrays(c.A_IΓ) + _csc_arrays(c.A_ΓΓ) + [c.b_I, c.f]
        out["plan/" + plan] = _sha(*arrs)
    for kind in ("full-rank", "floating"):
        out["pinv/" + kind] = _sha(*[b.ravel(order="F") for b in pinv_blocks(kind)])
    A, seeds, r = block_jacobi_case()
    out["block-jacobi"] = _sha(*_csc_arrays(A), *[np.asarray(s, dtype=np.int64) for s in seeds], r)
    M = sp.csr_matrix(amg_case(fem))
    out["amg-coarse-inverse"] = _sha(M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data)
    return out


def _values(cases):
    return (np.concatenate([c.A_II.data for c in cases]), np.concatenate([c.A_IΓ.data for c in cases]),
            np.concatenate([c.A_ΓΓ.data for c in cases]))


def run_plan(api, ctx, plan):
    """run with b_I; run without (the other graph); keep_levels(True): run and interior_solve; the second realization"""
    A, B = plan_cases(plan)
    ng, ni = [c.A_ΓΓ.shape[0] for c in A], [c.A_II.shape[0] for c in A]
    out = {}

    def put(run, S, w=None, u=None):
        for k, blk in enumerate(ss.split_blocks(S, ng)):
            out[f"{run}/S/{k}"] = np.array(blk)
        for what, v, sizes in (("w", w, ng), ("u", u, ni)):
            if v is not None:
                for k, piece in enumerate(ss.split_vec(v, sizes)):
                    out[f"{run}/{what}/{k}"] = np.array(piece)

    setup = se.make_setup(api, ctx, A)
    try:
        b = np.concatenate([c.b_I for c in A])
        put("rhs", *setup.run(b_I=b))
        put("no-rhs", setup.run()[0])
        setup.keep_levels(True)
        S, w = setup.run(b_I=b)
        put("kept", S, w, setup.interior_solve(np.concatenate([c.f for c in A])))
        put("second", *setup.run(*_values(B), b_I=np.concatenate([c.b_I for c in B])))
    finally:
        setup.close()
    return out


def run_pinv(api, ctx, kind):
    """one mixed batch; rocSOLVER's route is not under test: the spectral counter must not move"""
    blocks = pinv_blocks(kind)
    sizes = [b.shape[0] for b in blocks]
    before = ctx.query("spectral_pinv")
    flat = api.nn_pinv(ctx, np.array(sizes, dtype=np.int64), de.concat(blocks), de.RTOL if kind == "full-rank" else 0.0)
    moved = ctx.query("spectral_pinv") - before
    assert moved == 0, f"pinv/{kind}: {moved} blocks went to the eigen-decomposition"
    return {f"P/{n}": np.array(P) for n, P in zip(sizes, de.split(flat, sizes))}


def run_block_jacobi(api, ctx):
    A, seeds, r = block_jacobi_case()
    M = api.BlockJacobiPreconditioner(ctx, 2, A, seeds=seeds)
    try:
        return {"z": M.ldiv(r)}
    finally:
        M.close()


def run_amg(api, ctx, fem):
    M = api.AMGPreconditioner(ctx, amg_case(fem), device_setup=True, max_levels=1)
    try:
        return {"coarse_inv": np.array(M.device_hierarchy().coarse_inv)}
    finally:
        M.close()


def run_case(api, ctx, fem, name):
    if name.startswith("plan/"):
        return run_plan(api, ctx, name[5:])
    if name.startswith("pinv/"):
        return run_pinv(api, ctx, name[5:])
    return run_block_jacobi(api, ctx) if name == "block-jacobi" else run_amg(api, ctx, fem)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def pack(results, digests):
    """the arrays of the fixture: `<case>/<array>` (or `<case>/<array>/sha256` above HASH_ABOVE entries) and `inputs/<case>`"""
    out = {}
    for name, arrays in results.items():
        for key, a in arrays.items():
            if a.size > HASH_ABOVE:
                assert np.all(np.isfinite(a)), (name, key)
                out[f"{name}/{key}/sha256"] = np.array(digest(a))
            else:
                out[f"{name}/{key}"] = a
    for name, h in digests.items():
        out["inputs/" + name] = np.array(h)
    return out
