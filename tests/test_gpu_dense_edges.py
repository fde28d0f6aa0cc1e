"""GPU suite (-m gpu): the dense-block kernels on synthetic blocks at the shapes the FEM problems never produce.

Every block of the parity suite comes out of `fem.build_schur_problem`: symmetric, at most 1249 rows, Γ nodes shared by at
most 4 subdomains. Here the blocks and gather maps are drawn directly (fixed seeds):
  (a) `LocalSchurs` / `NeumannNeumannSchurPreconditioner` applies on NON-symmetric blocks of 0 ... 4097 rows (the
      multi-panel loop of k_gemv_batched past GEMV_PANEL = 2048, the unpadded stride of exactly 2048, the 16-row tails),
      against an np.longdouble reference, for every RPW x WAVES tiling, and `set_blocks` against creation;
  (b) k_gemv_multi (the deflated solvers' A W) on a block wider than one panel, against the per-column applies;
  (c) the folded PCG launches for every FOLD_CPT template, and the unfolded path they give way to;
  (d) `mi_nn_pinv`'s three routes against numpy's pinv, including eigenvalues on either side of the cut-off.
"""
import numpy as np
import pytest

from test_gpu_parity import assert_history

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
RTOL = float(np.sqrt(EPS))          # mi_nn_pinv's default cut-off (the reference's)


# ------------------------------------------------------------------ synthetic maps and blocks
def gather_maps(sizes, rng, max_share=4, hub=0):
    """Random gather lists for blocks of `sizes`: every Γ node lies in 1..max_share blocks (`hub` > 0: node 0 in the first
    `hub` non-empty blocks on top of that). Returns (gather lists, node_Γ_cnt, n_Γ) with cnt = the true multiplicity."""
    n_Γ0 = max(max(sizes), int(np.ceil(sum(sizes) / 2.5)))
    cnt = np.zeros(n_Γ0, dtype=np.int64)
    g = [None] * len(sizes)
    hubs = [d for d in range(len(sizes)) if sizes[d] > 0][:hub]
    for d in sorted(range(len(sizes)), key=lambda d: -sizes[d]):
        n = sizes[d]
        ok = np.flatnonzero(cnt < max_share)
        if d in hubs:
            ok = ok[ok != 0]
            pick = np.concatenate([[0], rng.choice(ok, n - 1, replace=False)])
            rng.shuffle(pick)
        else:
            pick = rng.choice(ok, n, replace=False)
        cnt[pick] += 1
        g[d] = pick.astype(np.int64)
    used = np.flatnonzero(cnt > 0)
    new = np.full(n_Γ0, -1, dtype=np.int64)
    new[used] = np.arange(used.size)
    return [new[a] for a in g], cnt[used], int(used.size)


_Q = {}


def orthogonal(n, seed, first=None):
    """A random orthogonal n x n matrix (fixed seed); `first`: its first column (up to sign) is this unit vector."""
    key = (n, seed, first is not None)
    if key not in _Q:
        A = np.random.default_rng(seed).standard_normal((n, n))
        if first is not None:
            A[:, 0] = first
        _Q[key] = np.linalg.qr(A)[0]
    return _Q[key]


def sym_from(Q, lam):
    """Q diag(lam) Q' with bitwise-symmetric storage (x + y = y + x)."""
    S = (Q * lam) @ Q.T
    return np.asfortranarray((S + S.T) / 2)


def spd_blocks(sizes, seed, kappa=1e3):
    """SPD blocks Q diag Q' with a geometric spectrum on [1, kappa], and their inverses."""
    S, P = [], []
    for k, n in enumerate(sizes):
        Q = orthogonal(n, seed + k)
        lam = np.geomspace(1.0, kappa, n)
        S.append(sym_from(Q, lam))
        P.append(sym_from(Q, 1.0 / lam))
    return S, P


def concat(blocks):
    return np.concatenate([b.ravel(order="F") for b in blocks]) if blocks else np.zeros(0)


def split(v, sizes):
    out, off = [], 0
    for n in sizes:
        out.append(np.asarray(v[off:off + n * n]).reshape(n, n, order="F"))
        off += n * n
    return out


# ------------------------------------------------------------------ (a) applies against a long-double reference
EDGE_SIZES = [0, 1, 2, 15, 16, 17, 127, 128, 129, 255, 256, 257, 1023, 1024, 2032, 2033, 2047, 2048, 2049, 2300, 4097]


@pytest.fixture(scope="module")
def edge_problem():
    rng = np.random.default_rng(20261016)
    g, cnt, n_Γ = gather_maps(EDGE_SIZES, rng)
    blocks = [np.asfortranarray(rng.standard_normal((n, n))) for n in EDGE_SIZES]   # non-symmetric on purpose
    x = rng.standard_normal(n_Γ)
    return g, cnt, n_Γ, blocks, x


def ref_apply(blocks, g, cnt, x, nn):
    """y = Σ_d R_d' (D_d^-1) B_d (D_d^-1) R_d x in long double (D = diag(cnt) for the Neumann-Neumann operator, I for S),
    the same sum with |B_d|, |x| (the summation bound's scale), and per row the widest block it lies in."""
    n_Γ = x.size
    y = np.zeros(n_Γ, dtype=np.longdouble)
    mag = np.zeros(n_Γ, dtype=np.longdouble)
    wid = np.zeros(n_Γ, dtype=np.int64)
    xl = x.astype(np.longdouble)
    cl = cnt.astype(np.longdouble)
    for B, gd in zip(blocks, g):
        if gd.size == 0:
            continue
        Bl = B.astype(np.longdouble)
        xd = xl[gd] / cl[gd] if nn else xl[gd]
        yd, md = Bl @ xd, np.abs(Bl) @ np.abs(xd)
        if nn:
            yd, md = yd / cl[gd], md / cl[gd]
        y[gd] += yd                      # (a block's gather list has no repeats)
        mag[gd] += md
        np.maximum.at(wid, gd, gd.size)
    return y, mag, wid


def assert_summation_bound(y, ref, slot_width, what):
    yr, mag, wid = ref
    err = np.abs(y.astype(np.longdouble) - yr)
    bar = (wid + slot_width + 4) * EPS * mag            # (m + 4) eps |A||x|, m = block size + slot width
    worst = int(np.argmax(err / np.maximum(bar, np.finfo(np.float64).tiny)))
    assert np.all(err <= bar), f"{what}: row {worst} err {float(err[worst]):.3e} > bar {float(bar[worst]):.3e}"
    print(f"{what}: max err / bar = {float(np.max(err / np.maximum(bar, 1e-300))):.3e}")


def test_dense_applies_at_tile_edges_every_tiling(pkg, ctx, edge_problem, monkeypatch):
    """Every row of a dense block is one wave's dot product in a fixed lane order (GemvRows / gemv_fma_group: lane l sums
    columns c0 + cb + 128 u + 2 l, + 1 of every panel, then wave_sum): the tiling (rows per wave RPW, waves per workgroup)
    only decides which wave does a row, so all nine tilings must give the same bits. The 0-row block is accepted and
    contributes nothing."""
    api = pkg.api
    g, cnt, n_Γ, blocks, x = edge_problem
    width = int(cnt.max())
    width = 4 if width == 3 else width
    refS = ref_apply(blocks, g, cnt, x, nn=False)
    refM = ref_apply(blocks, g, cnt, x, nn=True)
    first = None
    for rpw in (1, 2, 4):
        for waves in (4, 8, 16):
            monkeypatch.setenv("MI355_GEMV_RPW", str(rpw))
            monkeypatch.setenv("MI355_GEMV_WAVES", str(waves))
            S = api.LocalSchurs(ctx, blocks, g, cnt)
            M = api.NeumannNeumannSchurPreconditioner(ctx, blocks, g, cnt)
            yS, yM = S.apply(x), M.apply(x)
            S.close(); M.close()
            if first is None:
                assert_summation_bound(yS, refS, width, "S")
                assert_summation_bound(yM, refM, width, "NN")
                first = (yS, yM)
            else:
                assert np.array_equal(yS, first[0]) and np.array_equal(yM, first[1]), (rpw, waves)


def test_set_blocks_matches_creation(pkg, ctx, edge_problem):
    """`mi_dense_set_blocks` (device tensor, column-major concatenation -> k_block_to_rowmajor) fills the same padded
    row-major storage as the host copy at creation: same bits. The operators are created from other blocks first."""
    import torch
    api = pkg.api
    g, cnt, n_Γ, blocks, x = edge_problem
    other = [np.asfortranarray(0.5 * b.T) for b in blocks]
    dev = torch.from_numpy(concat(blocks)).to("cuda")
    for cls in (api.LocalSchurs, api.NeumannNeumannSchurPreconditioner):
        want = cls(ctx, blocks, g, cnt)
        got = cls(ctx, other, g, cnt)
        y_other = got.apply(x)
        got.set_blocks(dev)
        ctx.synchronize()
        y_want, y_got = want.apply(x), got.apply(x)
        assert not np.array_equal(y_other, y_want)
        assert np.array_equal(y_got, y_want), cls.__name__
        want.close(); got.close()


# ------------------------------------------------------------------ (b) k_gemv_multi: the deflated solvers' A W
@pytest.fixture(scope="module")
def wide_spd():
    sizes = [2100, 300, 130, 17]
    rng = np.random.default_rng(77)
    g, cnt, n_Γ = gather_maps(sizes, rng)
    S, P = spd_blocks(sizes, 700, kappa=1e2)
    b = rng.standard_normal(n_Γ)
    return sizes, g, cnt, n_Γ, S, P, b, rng


@pytest.mark.parametrize("kind", ["defcg", "defpcg"])
@pytest.mark.parametrize("nvec", [1, 3, 4, 5, 9])
def test_gemv_multi_matches_single_applies(pkg, ctx, orc, wide_spd, kind, nvec, monkeypatch):
    """A block of 2100 rows (two operand panels) and nvec = 1, 3, 4, 5, 9 (KV = 4 columns per pass, remainders kv < KV):
    k_gemv_multi accumulates every (row, vector) in k_gemv_batched's order (kernels.hpp), so MI355_NO_MULTI=1 (one apply
    per column) must give the same bits; both against the oracle."""
    api = pkg.api
    sizes, g, cnt, n_Γ, S, P, b, _ = wide_spd
    W = np.asfortranarray(np.random.default_rng(nvec).standard_normal((n_Γ, nvec)))
    x0 = np.zeros(n_Γ)
    A = api.LocalSchurs(ctx, S, g, cnt)
    M = api.NeumannNeumannSchurPreconditioner(ctx, P, g, cnt)
    Ao = orc.apply_local_schurs_operator(S, g, n_Γ)
    Mo = orc.neumann_neumann_operator(P, g, cnt)
    if kind == "defcg":
        run = lambda: api.defcg(A, b, x0, W)
        want = orc.defcg(Ao, b, x0, W)
    else:
        run = lambda: api.defpcg(A, b, x0, W, M)
        want = orc.defpcg(Ao, b, x0, W, Mo)
    monkeypatch.delenv("MI355_NO_MULTI", raising=False)
    multi = run()
    monkeypatch.setenv("MI355_NO_MULTI", "1")
    single = run()
    assert multi[1] == single[1]
    assert np.array_equal(multi[0], single[0]) and np.array_equal(multi[2], single[2])
    for got in (multi, single):
        assert_history(got, want, Ao, b)
    A.close(); M.close()


# ------------------------------------------------------------------ (c) folded PCG launches, every FOLD_CPT
# (waves, rpw, largest block, hub multiplicity). FOLD_CPT = ceil(max_ld / (64 WAVES)), max_ld the padded row stride:
# round n up to 16, and + 16 if that is a multiple of 256 other than GEMV_PANEL (operators.hpp).
FOLD_CASES = [
    (4, 1, 480, 0),     # ld 480:  FOLD_CPT 2
    (4, 1, 700, 0),     # ld 704:  3
    (4, 1, 1000, 0),    # ld 1008: 4
    (4, 1, 1200, 0),    # ld 1200: 5
    (4, 1, 1500, 0),    # ld 1504: 6
    (4, 1, 1700, 0),    # ld 1712: 7 -> the 8 template
    (4, 1, 2048, 0),    # ld 2048 (left unpadded): 8
    (8, 4, 1500, 0),    # ld 1504 / 512: 3
    (16, 2, 2000, 0),   # ld 2000 / 1024: 2
    (16, 2, 2049, 0),   # ld 2064 > GEMV_PANEL: unfolded
    (16, 2, 300, 6),    # a node in 6 subdomains: slot width 6 > 4, unfolded
]


@pytest.mark.parametrize("waves,rpw,nmax,hub", FOLD_CASES, ids=[f"w{c[0]}r{c[1]}n{c[2]}h{c[3]}" for c in FOLD_CASES])
def test_folded_pcg_variants(pkg, ctx, orc, waves, rpw, nmax, hub, monkeypatch):
    """pcg(S, b, x0, ΠS) on SPD blocks (κ = 1e3) with Π from mi_nn_pinv, against the oracle pcg on the same Π, from x0 = 0
    and from a random x0. The partial dot products follow the tiling, so the variants are not compared bit for bit."""
    api = pkg.api
    sizes = [nmax, 200, 150, 100, 64, 33] if hub else [nmax, 256, 129, 17]
    rng = np.random.default_rng(1000 * waves + nmax)
    g, cnt, n_Γ = gather_maps(sizes, rng, hub=hub)
    if hub:
        assert cnt.max() == hub
    S, _ = spd_blocks(sizes, nmax, kappa=1e3)
    nd = np.array(sizes, dtype=np.int64)
    Pi = split(api.nn_pinv(ctx, nd, concat(S)), sizes)
    monkeypatch.setenv("MI355_GEMV_WAVES", str(waves))
    monkeypatch.setenv("MI355_GEMV_RPW", str(rpw))
    A = api.LocalSchurs(ctx, S, g, cnt)
    M = api.NeumannNeumannSchurPreconditioner(ctx, Pi, g, cnt)
    Ao = orc.apply_local_schurs_operator(S, g, n_Γ)
    Mo = orc.neumann_neumann_operator(Pi, g, cnt)
    b = rng.standard_normal(n_Γ)
    folded = ctx.query("folded_pcg")
    for x0 in (np.zeros(n_Γ), rng.standard_normal(n_Γ)):
        got = api.pcg(A, b, x0, M)
        want = orc.pcg(Ao, b, x0, Mo)
        assert_history(got, want, Ao, b)
        x, it, res = got
        assert np.linalg.norm(b - Ao(x)) <= 2.0 * max(res[-1], 1e-7 * np.linalg.norm(b))   # the true residual
    # the folded launches ran exactly where they apply: max_ld <= GEMV_PANEL and slot width <= 4 (solvers.hpp)
    assert (ctx.query("folded_pcg") > folded) == (nmax <= 2048 and not hub)
    A.close(); M.close()


# ------------------------------------------------------------------ (d) mi_nn_pinv: the three routes
PINV_SIZES = [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 193, 1000, 2047, 2048, 2049]
# Bars: error <= C_PINV κ n eps (relative to max |pinv|, for the asymmetry, ‖I - ΠS‖_max and the Penrose conditions).
# Every case prints its ratio err / (κ n eps). Measured on an MI355X: at most 21.1 (Penrose, floating, κ = 1e6, n = 32),
# 11.3 (‖I - ΠS‖ at κ = 1e4, n = 65: a trailing pivot block of one row), 7.2 for the error against pinv (floating,
# κ = 1e6), every non-floating error against pinv below 3.7. C_PINV = 50 leaves a margin of 2.4 over the largest.
C_PINV = 50.0


def run_pinv(api, ctx, blocks, rtol=0.0):
    sizes = [b.shape[0] for b in blocks]
    before = ctx.query("spectral_pinv")
    out = api.nn_pinv(ctx, np.array(sizes, dtype=np.int64), concat(blocks), rtol)
    return split(out, sizes), ctx.query("spectral_pinv") - before


def np_pinv(S, rtol):
    return np.linalg.pinv(S, rcond=rtol, hermitian=True)


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), np.finfo(np.float64).tiny))


def check_pinv(tag, S, P, ref, kappa, rtol):
    """P against the pseudo-inverse `ref`, within C_PINV κ n eps (κ: of the kept spectrum). Returns the ratio."""
    n = S.shape[0]
    bar = kappa * n * EPS
    r = rel(P, ref) / bar
    print(f"pinv {tag} n={n}: err/(κ n eps) = {r:.3e}")
    assert r <= C_PINV, f"{tag} n={n}: |Π - pinv| / |pinv| = {r * bar:.3e} > {C_PINV * bar:.3e}"
    return r


@pytest.mark.parametrize("kappa", [10.0, 1e4, 1e5, 1e6, 1e7, 1e8])
def test_pinv_full_rank_is_the_inverse(pkg, ctx, kappa):
    """Full rank, alone and in a mixed-size batch. κ <= 1e4 -> route 1 (block Gauss-Jordan): no block reaches the
    eigen-decomposition. Beyond, the Gauss-Jordan inverse without pivoting loses accuracy faster than κ eps (41 % at
    κ = 1e8, n = 65, a one-row trailing pivot block) although its certificate holds; the probe residual must send such
    blocks on, so here only the result is checked, whatever the route. κ = 1e8 lies below the default cut-off
    sqrt(eps) = 1.5e-8 (pinv would drop λ_min), so it runs with rtol = 1e-12; κ = 1e5 ... 1e7 use the default.
    Symmetry is NOT bitwise beyond one 64-wide pivot block: k_gj_update stores each off-diagonal tile's mirror image from
    the same registers, but inside a diagonal tile (i, j) = M_ij - Σ A_iK (P A_Kj) and (j, i) = M_ji - Σ A_jK (P A_Ki) apply
    the pivot block P to different panels (R = P A[K, J] first): different products, equal only up to rounding. One pivot
    block (n <= 64) is mirrored to the last bit. So the asymmetry is held to the same bar as the error."""
    api = pkg.api
    rtol = 1e-12 if kappa > 1e6 else RTOL
    blocks, exact = [], []
    for n in PINV_SIZES:
        Q = orthogonal(n, n)
        lam = np.geomspace(1.0, kappa, n) if n > 1 else np.array([kappa])
        blocks.append(sym_from(Q, lam))
        exact.append(sym_from(Q, 1.0 / lam))
    gj = kappa <= 1e4
    mixed, spec = run_pinv(api, ctx, blocks, rtol)
    print(f"pinv κ={kappa:g}: {spec} of {len(blocks)} blocks to the eigen-decomposition")
    assert spec == 0 or not gj
    for S, E, P in zip(blocks, exact, mixed):
        single, spec = run_pinv(api, ctx, [S], rtol)
        assert spec == 0 or not gj
        assert np.array_equal(single[0], P)                 # a block's result does not depend on its batch
        n = S.shape[0]
        if n <= 64 and gj:
            assert np.array_equal(P, P.T)
        check_pinv(f"κ={kappa:g} asymmetry", S, P, P.T, kappa, rtol)
        check_pinv(f"κ={kappa:g} vs Q diag(1/λ) Q'", S, P, E, kappa, rtol)
        check_pinv(f"κ={kappa:g} vs numpy", S, P, np_pinv(S, rtol), kappa, rtol)
        # ‖I - ΠS‖ = ‖(Π - S^-1) S‖ <= κ x the relative error of Π, i.e. up to κ² n eps under the bar above; held to
        # κ n eps where that was measured to hold (κ <= 1e4)
        kr = kappa if gj else kappa ** 2
        r = float(np.max(np.abs(np.eye(n) - P @ S))) / (kr * n * EPS)
        print(f"pinv κ={kappa:g} n={n}: ‖I - ΠS‖_max/({'κ' if kr == kappa else 'κ²'} n eps) = {r:.3e}")
        assert r <= C_PINV


def penrose(S, P, kappa):
    """Moore-Penrose conditions, each relative, divided by κ n eps."""
    n = S.shape[0]
    bar = kappa * n * EPS
    nS, nP = np.max(np.abs(S)), np.max(np.abs(P))
    SP = S @ P
    return (np.max(np.abs(SP @ S - S)) / nS / bar, np.max(np.abs(P @ S @ P - P)) / nP / bar,
            np.max(np.abs(SP - SP.T)) / bar)


@pytest.mark.parametrize("kappa", [10.0, 1e4, 1e6])
def test_pinv_floating_blocks_take_the_shift(pkg, ctx, kappa):
    """Exactly floating (S 1 = 0 to rounding, rank n - 1) -> route 2, (S + α u u')^-1 - u u'/α, for κ <= 1e4; against
    numpy's pinv and the Penrose conditions. At κ = 1e6 the shifted inversion may fail its probe residual: any route."""
    api = pkg.api
    sizes = [n for n in PINV_SIZES if n >= 2]
    blocks = []
    for n in sizes:
        Q = orthogonal(n, n, first=np.ones(n) / np.sqrt(n))
        blocks.append(sym_from(Q, np.concatenate([[0.0], np.geomspace(1.0, kappa, n - 1)])))
    mixed, spec = run_pinv(api, ctx, blocks)
    print(f"pinv floating κ={kappa:g}: {spec} of {len(blocks)} blocks to the eigen-decomposition")
    assert spec == 0 or kappa > 1e4
    for S, P in zip(blocks, mixed):
        single, spec = run_pinv(api, ctx, [S])
        assert (spec == 0 or kappa > 1e4) and np.array_equal(single[0], P)
        check_pinv(f"floating κ={kappa:g} asymmetry", S, P, P.T, kappa, RTOL)     # (route 1's kernels: see above)
        check_pinv(f"floating κ={kappa:g}", S, P, np_pinv(S, RTOL), kappa, RTOL)
        p = penrose(S, P, kappa)
        print(f"pinv floating κ={kappa:g} n={S.shape[0]}: Penrose/(κ n eps) = {p[0]:.3e} {p[1]:.3e} {p[2]:.3e}")
        assert max(p) <= C_PINV


@pytest.mark.parametrize("kappa", [10.0, 1e4])
def test_pinv_rank_deficiency_two_goes_spectral(pkg, ctx, kappa):
    """Two zero eigenvalues -> route 3 (rocSOLVER dsyevd): the spectral counter moves by one per block."""
    api = pkg.api
    sizes = [n for n in PINV_SIZES if n >= 3 and n <= 1000]
    blocks = []
    for n in sizes:
        Q = orthogonal(n, n)
        blocks.append(sym_from(Q, np.concatenate([[0.0, 0.0], np.geomspace(1.0, kappa, n - 2)])))
    mixed, spec = run_pinv(api, ctx, blocks)
    assert spec == len(blocks)
    for S, P in zip(blocks, mixed):
        check_pinv(f"rank-2-deficient κ={kappa:g}", S, P, np_pinv(S, RTOL), kappa, RTOL)
        p = penrose(S, P, kappa)
        print(f"pinv deficient κ={kappa:g} n={S.shape[0]}: Penrose/(κ n eps) = {p[0]:.3e} {p[1]:.3e} {p[2]:.3e}")
        assert max(p) <= C_PINV


STRADDLE_SIZES = [3, 33, 64, 129, 400, 1000, 1500]


@pytest.mark.parametrize("along_u", [True, False], ids=["along_u", "random_dir"])
@pytest.mark.parametrize("f", [0.5, 2.0, 5.0, 20.0])
def test_pinv_eigenvalue_near_the_cutoff(pkg, ctx, f, along_u):
    """One eigenvalue λ0 = f rtol σ_max (spectrum otherwise geomspace(1, 100)), on the constants u = 1/sqrt(n) or on a
    random direction: whichever route a block takes, the result is pinv's. f stays a factor 2 from 1 (pinv is discontinuous
    at the cut-off). κ of the bar: σ_max over the smallest KEPT eigenvalue."""
    api = pkg.api
    blocks, kappas = [], []
    for n in STRADDLE_SIZES:
        Q = orthogonal(n, 3 * n, first=np.ones(n) / np.sqrt(n) if along_u else None)
        lam = np.geomspace(1.0, 100.0, n)
        lam[0] = f * RTOL * 100.0
        blocks.append(sym_from(Q, lam))
        kappas.append(100.0 / (lam[0] if f > 1 else lam[1]))
    mixed, _ = run_pinv(api, ctx, blocks)
    for S, P, k in zip(blocks, mixed, kappas):
        single, _ = run_pinv(api, ctx, [S])
        assert np.array_equal(single[0], P)
        check_pinv(f"λ0={f:g} rtol σ_max {'on u' if along_u else 'random'}", S, P, np_pinv(S, RTOL), k, RTOL)


def test_pinv_nan_block_is_singular(pkg, ctx):
    """A block with a NaN (a set-up that met a singular interior block) -> MI_ERR_SINGULAR, next to a good block."""
    api = pkg.api
    good = sym_from(orthogonal(65, 65), np.geomspace(1.0, 10.0, 65))
    bad = good.copy()
    bad[3, 7] = bad[7, 3] = np.nan
    with pytest.raises(pkg._lib.SingularException) as e:
        run_pinv(api, ctx, [good, bad])
    assert e.value.code == pkg._lib.MI_ERR_SINGULAR
    P, _ = run_pinv(api, ctx, [good])                      # the context is still usable
    assert np.all(np.isfinite(P[0]))
