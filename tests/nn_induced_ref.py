"""Host reference of the Neumann-Neumann induced preconditioner for tests/test_nn_induced_cpu.py and
tests/test_gpu_nn_induced.py.

`apply_neumann_neumann_induced` restates the reference's function (EPDD.jl:2363-2423) statement by statement in numpy /
scipy; `lorasc_ref.Solve` (SuperLU, optionally refined on long-double residuals) stands in for the CHOLMOD factors of
`chol_A_IId`. `coupling="reference"` is :2411 as written (the interior sees the local, unweighted, unassembled z_Γd),
`coupling="assembled"` replaces it by z_Γ[gather_d]. ΠS_d is taken as given: for fp32 storage the caller passes
`ΠS_d.astype(float32).astype(float64)`. `dense_minv` is M^-1 column by column from it."""
import numpy as np
import scipy.sparse as sp

from lorasc_ref import ALL_CASES, Case, Solve, gpu_cases, make_case  # noqa: F401  (re-exported for the two suites)

COUPLINGS = ("reference", "assembled")

# (N, px, py) of two more box partitions, found by a host search over N in 20..70 and px, py in 1..4 (px py >= 2) for the
# smallest number of free nodes (test_nn_induced_cpu.py asserts the property): a subdomain block whose n_Γd is a multiple
# of the 32-row GEMV tile (n_Γd = 32 in the middle box of 3 x 3 on N = 24: a full last tile) and one with n_Γd = 1 (mod 32)
# (n_Γd = 33 in a box of 2 x 3 on N = 26: a last tile of one row).
TILE_EDGE_PARTITIONS = {"tile_full": (24, 3, 3), "tile_one": (26, 2, 3)}
GPU_CASES = ALL_CASES + tuple(TILE_EDGE_PARTITIONS)


def nni_cases(fem, which=None):
    """`lorasc_ref.gpu_cases` plus the two tile-edge partitions, by name."""
    names = list(which or GPU_CASES)
    out = gpu_cases(fem, [k for k in names if k in ALL_CASES]) if any(k in ALL_CASES for k in names) else {}
    for k in names:
        if k in TILE_EDGE_PARTITIONS:
            N, px, py = TILE_EDGE_PARTITIONS[k]
            out[k] = make_case(fem, k, N, px, py)
    return {k: out[k] for k in names}


def prepare(fem, case: Case):
    """ΠS_d of `prepare_neumann_neumann_induced_precond` (EPDD.jl:2305-2353) for a case; computed once per case."""
    if "ΠSd" not in case.__dict__:
        P = case.P
        case.__dict__["ΠSd"] = fem.prepare_neumann_neumann_induced_precond(P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd)
    return case.__dict__["ΠSd"]


def rounded_f32(ΠSd):
    return [np.asfortranarray(B.astype(np.float32).astype(np.float64)) for B in ΠSd]


def _interior_solves(case: Case, refine: int):
    key = ("nni_solves", refine)
    if key not in case.__dict__:
        case.__dict__[key] = [Solve(M, refine) for M in case.P.A_IIdd]
    return case.__dict__[key]


def apply_neumann_neumann_induced(case: Case, ΠSd, r, coupling: str = "reference", refine: int = 0):
    """EPDD.jl:2363-2423 on a vector or on the columns of a matrix."""
    assert coupling in COUPLINGS
    r = np.asarray(r, dtype=np.float64)
    P = case.P
    A_IΓdd = [sp.csc_matrix(a) for a in P.A_IΓdd]
    chol_A_IId = _interior_solves(case, refine)
    gather, cnt = P.sub.gather_idx, np.asarray(P.sub.node_Γ_cnt, dtype=np.float64)
    ndom = len(A_IΓdd)
    col = (lambda v: v) if r.ndim == 1 else (lambda v: v[:, None])
    r_Id = [r[case.pos_I[d]] for d in range(ndom)]                                # :2383-2387
    r_Γ = r[case.pos_Γ]                                                           # :2389-2391
    r_schur = r_Γ.copy()                                                          # :2393
    z_Id = [None] * ndom
    for d in range(ndom):                                                         # :2394-2400
        z_Id[d] = chol_A_IId[d](r_Id[d])
        r_Γd = A_IΓdd[d].T @ z_Id[d]
        r_schur[gather[d]] -= r_Γd
    z_Γ = np.zeros_like(r_Γ)                                                      # :2380
    z_Γd = [None] * ndom
    for d in range(ndom):                                                         # :2402-2410
        r_Γd = r_schur[gather[d]] / col(cnt[gather[d]])
        z_Γd[d] = ΠSd[d] @ r_Γd
        z_Γ[gather[d]] += z_Γd[d] / col(cnt[gather[d]])
    z = np.empty_like(r)
    for d in range(ndom):                                                         # :2411-2415
        v = z_Γd[d] if coupling == "reference" else z_Γ[gather[d]]
        z[case.pos_I[d]] = chol_A_IId[d](r_Id[d] - A_IΓdd[d] @ v)
    z[case.pos_Γ] = z_Γ                                                           # :2418-2420
    return z


def dense_minv(case: Case, ΠSd, coupling: str = "reference", refine: int = 0):
    """M^-1 as a dense matrix: the apply on the columns of the identity."""
    return np.asfortranarray(apply_neumann_neumann_induced(case, ΠSd, np.eye(case.n), coupling, refine))


def block_formula_minv(case: Case, ΠSd):
    """[I -A_II^-1 A_IΓ; 0 I] diag(A_II^-1, M_NN) [I 0; -A_ΓI A_II^-1 I] with M_NN = Σ_d R_d' D_d ΠS_d D_d R_d, dense algebra
    in the (I_1, ..., I_ndom, Γ) ordering, then permuted to the rows of A."""
    n_I = [a.shape[0] for a in case.A_IId]
    nI, nΓ = sum(n_I), case.n_Γ
    iA = np.linalg.inv(sp.block_diag(case.A_IId).toarray())
    A_IΓ = sp.vstack(case.A_IΓd).toarray()
    cnt = np.asarray(case.P.sub.node_Γ_cnt, dtype=np.float64)
    M_NN = np.zeros((nΓ, nΓ))
    for g, B in zip(case.P.sub.gather_idx, ΠSd):
        M_NN[np.ix_(g, g)] += B / cnt[g][:, None] / cnt[g][None, :]
    U = np.block([[np.eye(nI), -iA @ A_IΓ], [np.zeros((nΓ, nI)), np.eye(nΓ)]])
    D = np.block([[iA, np.zeros((nI, nΓ))], [np.zeros((nΓ, nI)), M_NN]])
    L = np.block([[np.eye(nI), np.zeros((nI, nΓ))], [-A_IΓ.T @ iA, np.eye(nΓ)]])
    perm = np.concatenate(list(case.pos_I) + [case.pos_Γ])
    out = np.empty((nI + nΓ, nI + nΓ))
    out[np.ix_(perm, perm)] = U @ D @ L
    return out


def apply_input(case: Case, salt: int = 0):
    """The random r of one apply test."""
    return np.random.default_rng(sum(case.name.encode()) * 1000 + 77 + salt).standard_normal(case.n)
