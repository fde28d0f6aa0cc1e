"""numpy restatement of the reference's realization layer, for tests/test_kl_field_cpu.py and tests/test_gpu_kl_field.py:

  set_field           `set!(Λ, Ψ, ξ, g)` (Fem/KarhunenLoeveDomainDecomposition.jl = "KLDD.jl" :1150-1164), the loop of `draw!`
                      (KLDD.jl:1037-1040) and of the samplers (Fem/Samplers.jl:64-67), accumulated from zero as fem.draw does
  dd_field            the nest of `draw(mesh, Λ, Φ, Φd, inds_l2gd)` (KLDD.jl:870-881), node by node, for a given ξ
  kl_coordinates      `get_kl_coordinates` (KLDD.jl:1109-1124)
  mc / mcmc / hybrid  the samplers of Fem/Samplers.jl:33-199 (hybrid: the evident intent of :287-322) as plain functions that
                      return the whole chain, driven by a scripted generator
  dd_bound, coords_bound, EXP_RTOL   the derived tolerances of the device forms

Nothing here calls the package."""
import numpy as np

EPS = 2.0 ** -52
# A = exp(G) on equal bits of G: the device's exp and the host's are each within 1 ulp of the true value; doubled
EXP_RTOL = 4 * EPS


def set_field(Λ, Ψ, ξ):
    Λ, Ψ, ξ = np.asarray(Λ, float), np.asarray(Ψ, float), np.asarray(ξ, float)
    g = np.zeros(Ψ.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for α in range(Λ.size):
            c_α = np.sqrt(Λ[α]) * ξ[α]
            g = g + c_α * Ψ[:, α]
    return g


def dd_field(nnode, Λ, Φ, Φd, inds_l2gd, ξ):
    """KLDD.jl:870-881 as written: scalar loops over (idom, i, α, γ)"""
    Λ, Φ, ξ = np.asarray(Λ, float), np.asarray(Φ, float), np.asarray(ξ, float)
    md = [np.asarray(P).shape[1] for P in Φd]
    g = np.zeros(nnode)
    cnt = np.zeros(nnode, dtype=np.int64)
    for idom in range(len(Φd)):
        P = np.asarray(Φd[idom], float)
        for i, inode in enumerate(inds_l2gd[idom]):
            cnt[inode] += 1
            for α in range(md[idom]):
                ind_α_idom = α if idom == 0 else sum(md[:idom]) + α
                for γ in range(Λ.size):
                    g[inode] += np.sqrt(Λ[γ]) * ξ[γ] * Φ[ind_α_idom, γ] * P[i, α]
    return g / cnt


def dd_bound(nnode, Λ, Φ, Φd, inds_l2gd, ξ):
    """|g_device - dd_field|_i <= 2 (m + md_max + cnt_i + 4) eps (1 / cnt_i) Σ_{d ∋ i} Σ_α |Φd[l, α]| Σ_γ |Φ[α, γ]| |c_γ|:
    every term of either nest is a product of three factors and c_γ itself a product (4 roundings); the sums have m, md_d and
    cnt_i terms in either order; one division; 2 for the two sides."""
    Λ, Φ, ξ = np.asarray(Λ, float), np.asarray(Φ, float), np.asarray(ξ, float)
    c = np.abs(np.sqrt(Λ) * ξ)
    yabs = np.abs(Φ) @ c
    s = np.zeros(nnode)
    cnt = np.zeros(nnode, dtype=np.int64)
    off = 0
    md_max = 0
    for P, l2g in zip(Φd, inds_l2gd):
        P = np.asarray(P, float)
        md_max = max(md_max, P.shape[1])
        s[l2g] += np.abs(P) @ yabs[off:off + P.shape[1]]
        cnt[l2g] += 1
        off += P.shape[1]
    return 2 * (Λ.size + md_max + cnt + 4) * EPS * s / cnt


def kl_coordinates(g, Λ, Φ, M):
    Λ, Φ = np.asarray(Λ, float), np.asarray(Φ, float)
    w = M @ np.asarray(g, float)
    ξ = np.zeros(Λ.size)
    for α, λ_α in enumerate(Λ):
        sqrt_λ_α = np.sqrt(λ_α)
        for i in range(Φ.shape[0]):
            ξ[α] += Φ[i, α] * w[i] / sqrt_λ_α
    return ξ


def kl_coordinates_blas(g, Λ, Ψ, M):
    """The same column sums in numpy's own order, divided once: for sizes where the scalar loop above takes too long. Any order
    of the n terms is within one side's share of coords_bound, which is all a comparison against it uses."""
    return (np.asarray(Ψ, float).T @ (M @ np.asarray(g, float))) / np.sqrt(np.asarray(Λ, float))


def coords_bound(g, Λ, Ψ, M):
    """|ξ_device - kl_coordinates|_α <= 2 (n + row_nnz_max + 6) eps Σ_i |Ψ_iα| (|M| |g|)_i / sqrt(Λ_α): a row of M g has at most
    row_nnz_max terms, the column sum n, plus the products and the division (once per term or once per sum); 2 for the two sides"""
    Ψ = np.asarray(Ψ, float)
    Mabs = abs(M)
    nnz_max = int(np.diff(Mabs.tocsr().indptr).max())
    return 2 * (Ψ.shape[0] + nnz_max + 6) * EPS * (np.abs(Ψ).T @ (Mabs @ np.abs(g))) / np.sqrt(np.asarray(Λ, float))


# ------------------------------------------------------------------ samplers
class ScriptedRng:
    """Stands in for numpy.random.Generator: `standard_normal(k)` and `random()` hand out the scripted numbers in order and
    fail when the script and the caller disagree about the next call."""

    def __init__(self, script):
        self.script, self.pos = list(script), 0

    def _next(self, kind):
        assert self.pos < len(self.script), "the script is exhausted"
        k, v = self.script[self.pos]
        assert k == kind, f"call {self.pos}: the script has '{k}', the sampler asked for '{kind}'"
        self.pos += 1
        return v

    def standard_normal(self, size):
        v = np.array(self._next("normal"), dtype=float)
        assert v.shape == (size,), f"call {self.pos - 1}: {size} normals asked for, {v.shape} scripted"
        return v

    def random(self):
        return float(self._next("uniform"))

    def exhausted(self):
        return self.pos == len(self.script)


def _metropolis(ξ, σ2, ϑ2, rng, trace):
    """Samplers.jl:167-191 -> (χ, cnt); `trace` collects (‖ξ‖² < ‖χ‖², α, u) per proposal"""
    sq_norm_of_ξ = ξ @ ξ
    χ = ξ + np.sqrt(ϑ2) * rng.standard_normal(ξ.size)
    sq_norm_of_χ = χ @ χ
    cnt = 1
    α = np.exp((sq_norm_of_ξ - sq_norm_of_χ) / 2 / σ2) if sq_norm_of_ξ < sq_norm_of_χ else 1.
    u = rng.random()
    trace.append((bool(sq_norm_of_ξ < sq_norm_of_χ), float(α), u))
    while u > α:
        χ = ξ + np.sqrt(ϑ2) * rng.standard_normal(ξ.size)
        sq_norm_of_χ = χ @ χ
        α = np.exp((sq_norm_of_ξ - sq_norm_of_χ) / 2 / σ2) if sq_norm_of_ξ < sq_norm_of_χ else 1.
        u = rng.random()
        trace.append((bool(sq_norm_of_ξ < sq_norm_of_χ), float(α), u))
        cnt += 1
    return χ, cnt


def mc_chain(Λ, Ψ, rng, ndraw):
    """prepare_mc_sampler + ndraw draw! -> [(ξ, g)], the first entry is the state after construction"""
    m = len(Λ)
    out = []
    for _ in range(ndraw + 1):
        ξ = rng.standard_normal(m)
        out.append((ξ.copy(), set_field(Λ, Ψ, ξ)))
    return out


def mcmc_chain(Λ, Ψ, rng, ndraw):
    """prepare_mcmc_sampler + ndraw draw! -> ([(ξ, g, cnt)], trace); entry 0 is the state after construction (cnt 0)"""
    m = len(Λ)
    σ2 = 1.
    ξ = np.sqrt(σ2) * rng.standard_normal(m)
    ϑ2 = 2.38 ** 2 * σ2 / m
    χ = ξ + np.sqrt(ϑ2) * rng.standard_normal(m)                  # noqa: F841  (the reference draws it and never uses it)
    out, trace = [(ξ.copy(), set_field(Λ, Ψ, ξ), 0)], []
    for _ in range(ndraw):
        steps = []
        χ, cnt = _metropolis(ξ, σ2, ϑ2, rng, steps)
        ξ = χ.copy()
        out.append((ξ.copy(), set_field(Λ, Ψ, ξ), cnt))
        trace.append(steps)
    return out, trace


def hybrid_chain(Λ, Ψ, m_mcmc, rng, ndraw):
    m = len(Λ)
    σ2 = 1.
    ξ = np.empty(m)
    ξ[:m_mcmc] = np.sqrt(σ2) * rng.standard_normal(m_mcmc)
    ξ[m_mcmc:] = rng.standard_normal(m - m_mcmc)
    ϑ2 = 2.38 ** 2 * σ2 / m_mcmc
    rng.standard_normal(m_mcmc)                                   # χ of the constructor
    out = [(ξ.copy(), set_field(Λ, Ψ, ξ), 0)]
    for _ in range(ndraw):
        χ, cnt = _metropolis(ξ[:m_mcmc].copy(), σ2, ϑ2, rng, [])
        ξ[:m_mcmc] = χ
        ξ[m_mcmc:] = rng.standard_normal(m - m_mcmc)
        out.append((ξ.copy(), set_field(Λ, Ψ, ξ), cnt))
    return out


def mcmc_script():
    """m = 3, three draws: (1) the first proposal is accepted with ‖χ‖² > ‖ξ‖² (α = 0.88 >= u = 0.5); (2) two rejections
    (α = 5e-7 < u = 0.3, α = 0.009 < u = 0.9), then an acceptance; (3) ‖χ‖² <= ‖ξ‖²: α = 1 whatever u. tests assert that the
    trace of the restatement shows exactly these events."""
    N, U = "normal", "uniform"
    return [(N, [1.0, -0.5, 0.25]), (N, [0.3, 0.3, -0.3]),
            (N, [0.1, 0.1, 0.1]), (U, 0.5),
            (N, [2.0, 2.0, 2.0]), (U, 0.3), (N, [-2.0, 1.5, -2.0]), (U, 0.9), (N, [0.3, -0.2, 0.1]), (U, 0.2),
            (N, [-0.5, 0.2, -0.2]), (U, 0.999)]


def hybrid_script():
    """m = 4, m_mcmc = 2, two draws; the second has one rejection"""
    N, U = "normal", "uniform"
    return [(N, [0.8, -0.4]), (N, [0.7, -1.1]), (N, [0.2, 0.2]),
            (N, [0.1, 0.05]), (U, 0.4), (N, [-0.9, 0.6]),
            (N, [3.0, 3.0]), (U, 0.5), (N, [-0.2, 0.1]), (U, 0.6), (N, [1.3, 0.4])]


def split_problem(fem, N=24, cut=15, md=(1, 3, 7, 2), m=5, seed=1):
    """A structured mesh of N x N nodes split 2 x 2 at cell `cut` in x and y, with one triangle of the right-hand neighbour
    moved into box 0: box 0 then has (cut + 1)² + 1 nodes — with the defaults 257, one row past a row tile of 256 — the others
    144, 144 and 81 (below a row tile), and cnt takes the values 1, 2 and 4. Index sets from fem.kl_set_subdomain; random
    local factors Φd (n_d x md_d), reduced factors Φ (Σ md x m) and Λ. -> (mesh, l2gd, elemsd, Φd, Φ, Λ, rng)"""
    rng = np.random.default_rng(seed)
    mesh = fem.get_mesh(N)
    h = 1.0 / (N - 1)
    cen = mesh.points[:, mesh.cells].mean(axis=1)
    ix, iy = np.floor(cen[0] / h).astype(int), np.floor(cen[1] / h).astype(int)
    epart = (ix >= cut).astype(np.int64) + 2 * (iy >= cut)
    box0 = set(np.unique(mesh.cells[:, epart == 0]))
    cand = [el for el in np.flatnonzero((ix == cut) & (iy == 0)) if sum(int(v) not in box0 for v in mesh.cells[:, el]) == 1]
    assert len(cand) == 1
    epart[cand[0]] = 0
    subs = [fem.kl_set_subdomain(mesh.cells, mesh.points, epart, d) for d in range(4)]
    l2gd, elemsd = [s[0] for s in subs], [s[2] for s in subs]
    assert l2gd[0].size == (cut + 1) ** 2 + 1
    Φd = [rng.standard_normal((l2g.size, k)) for l2g, k in zip(l2gd, md)]
    Φ = rng.standard_normal((sum(md), m))
    Λ = np.sort(rng.random(m) + 0.1)[::-1]
    return mesh, l2gd, elemsd, Φd, Φ, Λ, rng


def small_modes(rng, n, m):
    """(Λ, Ψ) of a test: decaying positive Λ, mixed-sign Ψ with exact zeros"""
    Λ = np.sort(rng.random(m) + 0.05)[::-1] / (1 + np.arange(m))
    Ψ = rng.standard_normal((n, m))
    Ψ[rng.random((n, m)) < 0.1] = 0.0
    return Λ, Ψ
