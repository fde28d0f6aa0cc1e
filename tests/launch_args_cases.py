"""Cases of tests/test_gpu_launch_args.py, shared with the generator of its fixture (tests/golden/make_launch_args_golden.py).

Every launch of the loop kernels is run once with inputs that are the same bits on every machine: blocks, right-hand sides
and CSR values are integers from `default_rng(seed).integers`, scaled by powers of two and combined elementwise (no BLAS or
LAPACK call), the gather maps are `gather_maps` of tests/test_gpu_dense_edges.py (integer draws). A block is
`(5 + n/16) I + (R + R') / 32` with R uniform on -16 ... 16: symmetric, and positive definite because the spectral radius of
the random part stays near 0.85 sqrt(n) < 5 + n/16 - 1 for every n (checked in numpy for the sizes used here). ΠS_d is a
second block of the same kind (another seed), not an inverse: the kernels do not care, and PCG with any SPD M converges.

`run_all(api, ctx)` returns {case: (x, it, res_norm)}; an apply is stored as (y, 0, []).
"""
import os
from contextlib import contextmanager

import numpy as np

import shard_synth as ss
from test_gpu_dense_edges import gather_maps


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


def int_blocks(sizes, seed):
    out = []
    rng = np.random.default_rng(seed)
    for n in sizes:
        R = rng.integers(-16, 17, size=(n, n)).astype(np.float64)
        B = (R + R.T) * 2.0 ** -5
        B[np.arange(n), np.arange(n)] += 5.0 + n / 16.0
        out.append(np.asfortranarray(B))
    return out


def int_vec(n, seed, shift=6):
    return np.random.default_rng(seed).integers(-64, 65, size=n).astype(np.float64) * 2.0 ** -shift


def dense_problem(sizes, seed, hub=0):
    g, cnt, n = gather_maps(sizes, np.random.default_rng(seed), hub=hub)
    return dict(sizes=sizes, g=g, cnt=cnt, n=n, S=int_blocks(sizes, seed + 1), Pi=int_blocks(sizes, seed + 2),
                b=int_vec(n, seed + 3), x0=int_vec(n, seed + 4, shift=10))


def banded_csr(n, seed, offsets=(1, 7, 57)):
    """Symmetric, strictly diagonally dominant: off-diagonals -k/8 (k = 1 ... 8) on three bands, diagonal = 1 + Σ|row|.
    Returns CSR arrays with sorted columns (= CSC of the same matrix) as (ptr, idx, val, n)."""
    rng = np.random.default_rng(seed)
    band = {o: -rng.integers(1, 9, size=n - o).astype(np.float64) / 8.0 for o in offsets}
    diag = np.ones(n)
    for o, v in band.items():
        diag[:n - o] += -v
        diag[o:] += -v
    rows, cols, vals = [np.arange(n)], [np.arange(n)], [diag]
    for o, v in band.items():
        rows += [np.arange(n - o), np.arange(o, n)]
        cols += [np.arange(o, n), np.arange(n - o)]
        vals += [v, v]
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(ptr, rows + 1, 1)
    return np.cumsum(ptr), cols[order].astype(np.int64), vals[order], n, diag


def solve(t):
    return np.asarray(t[0]), int(t[1]), np.asarray(t[2])


# (a), (c), (d), (h): blocks of 33 / 17 / 64 rows (33 twice, node 0 in all four blocks), default tiling 16 waves x 2 rows:
# 32-row tiles -> a tile with one row (33), a partial only tile (17) and two full ones (64)
SMALL = [33, 17, 64, 33]
# (b): a 700-row block (row stride 704: FOLD_CPT 3 with 4 waves), then 8 waves x 4 rows
TILINGS = [("b_w4r1_n700", 4, 1, [700, 33, 17, 64]), ("b_w8r4", 8, 4, [130, 33, 17, 64])]
XCHG_SIZES = [130, 65, 96, 33, 47]      # `uneven_w2` of tests/shard_synth.py, the smallest sharded case, on integer blocks
WIDE = [2049, 130]


def run_all(api, ctx):
    out = {}
    zero = lambda p: np.zeros(p["n"])

    p = dense_problem(SMALL, 4100, hub=4)
    assert int(p["cnt"].max()) == 4
    A = api.LocalSchurs(ctx, p["S"], p["g"], p["cnt"])
    M = api.NeumannNeumannSchurPreconditioner(ctx, p["Pi"], p["g"], p["cnt"])
    f0 = ctx.query("folded_pcg")
    out["a_folded"] = solve(api.pcg(A, p["b"], zero(p), M))
    assert ctx.query("folded_pcg") > f0
    out["h_x0"] = solve(api.pcg(A, p["b"], p["x0"], M))
    out["h_maxit"] = solve(api.pcg(A, p["b"], zero(p), M, maxit=3))
    assert out["h_maxit"][1] == 3 < out["a_folded"][1]
    W = np.asfortranarray(np.random.default_rng(4107).integers(-8, 9, size=(p["n"], 3)).astype(np.float64) / 8.0)
    f0 = ctx.query("folded_pcg")
    out["c_defpcg"] = solve(api.defpcg(A, p["b"], zero(p), W, M))
    assert ctx.query("folded_pcg") > f0
    M32 = api.NeumannNeumannSchurPreconditioner(ctx, p["Pi"], p["g"], p["cnt"], storage="f32")
    f0 = ctx.query("folded_pcg")
    out["d_f32"] = solve(api.pcg(A, p["b"], zero(p), M32))
    assert ctx.query("folded_pcg") > f0
    for op in (A, M, M32):
        op.close()

    for name, waves, rpw, sizes in TILINGS:
        q = dense_problem(sizes, 4200 + waves)
        with env(MI355_GEMV_WAVES=waves, MI355_GEMV_RPW=rpw):       # read when an operator is constructed
            A = api.LocalSchurs(ctx, q["S"], q["g"], q["cnt"])
            M = api.NeumannNeumannSchurPreconditioner(ctx, q["Pi"], q["g"], q["cnt"])
        f0 = ctx.query("folded_pcg")
        out[name] = solve(api.pcg(A, q["b"], zero(q), M))
        assert ctx.query("folded_pcg") > f0
        A.close(); M.close()

    # (e) both operators sharded over two in-process ranks: the XCHG = true instantiations
    c = ss.Case("launch_args_xchg", XCHG_SIZES, 4300, 2)
    g, cnt, n = c.maps()
    S, Pi = int_blocks(XCHG_SIZES, 4301), int_blocks(XCHG_SIZES, 4302)
    b = int_vec(n, 4303)

    def rank_main(rctx, r):
        Ar, Mr = ss.rank_ops(api, rctx, c, r, S, Pi, True)
        rctx.host_barrier.wait(timeout=120)
        f0 = rctx.query("folded_pcg")
        res = solve(api.pcg(Ar, b, np.zeros(n), Mr))
        return res, rctx.query("folded_pcg") - f0, rctx.query("peer_exchange")
    with env(MI355_PEER_TIMEOUT_MS=20000):
        ranks = ss.run_ranks(api, 2, rank_main, timeout=300)
    for res, folded, peer in ranks:
        assert folded > 0 and peer >= 1
        assert res[1] == ranks[0][0][1] and np.array_equal(res[0], ranks[0][0][0]) and np.array_equal(res[2], ranks[0][0][2])
    out["e_xchg"] = ranks[0][0]

    # (f) plain applies (fp64 and fp32 storage) and apply_multi (the deflated solver's A W, nvec = 5: a pass of 4 and one of 1)
    w = dense_problem(WIDE, 4400)
    A = api.LocalSchurs(ctx, w["S"], w["g"], w["cnt"])
    M = api.NeumannNeumannSchurPreconditioner(ctx, w["Pi"], w["g"], w["cnt"])
    M32 = api.NeumannNeumannSchurPreconditioner(ctx, w["Pi"], w["g"], w["cnt"], storage="f32")
    none = np.zeros(0)
    out["f_apply_S"] = (np.asarray(A * w["b"]), 0, none)
    out["f_apply_NN"] = (np.asarray(M * w["b"]), 0, none)
    out["f_apply_NN32"] = (np.asarray(M32 * w["b"]), 0, none)
    W = np.asfortranarray(np.random.default_rng(4407).integers(-8, 9, size=(w["n"], 5)).astype(np.float64) / 8.0)
    out["f_multi_defpcg"] = solve(api.defpcg(A, w["b"], zero(w), W, M))
    for op in (A, M, M32):
        op.close()

    # (g) the sparse 2-launch loop with a diagonal M. Up to 8192 rows the single-workgroup loop would take the solve:
    # MI355_NO_FUSED=1 hands it to k_spmv_pcg / k_update_xr_blk; 9001 rows get there by themselves
    for name, nrows, envs in (("g_csr3001", 3001, {"MI355_NO_FUSED": 1}), ("g_csr9001", 9001, {})):
        ptr, idx, val, n, diag = banded_csr(nrows, 4500 + nrows)
        Ag = api.SparseMatrixCSC(ctx, (ptr, idx, val, n))
        Mj = api.JacobiPreconditioner(ctx, diag)
        with env(**envs):
            out[name] = solve(api.pcg(Ag, int_vec(n, 4501), np.zeros(n), Mj))
        Ag.close(); Mj.close()
    return out


def pack(results):
    flat = {}
    for name, (x, it, res) in results.items():
        flat[name + "/x"], flat[name + "/it"], flat[name + "/res_norm"] = x, np.int64(it), res
    return flat
