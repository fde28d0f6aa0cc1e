"""Inputs and helpers of tests/test_gpu_handle_lifetime.py: state that outlives one call and belongs to two handles at once
(DESIGN.md "Who remembers whom").

Every input is one the suite already builds: the full system of `fem.get_mesh(N)`, N in {20, 24}, with three nodal
coefficients (constant 1 and two lognormal draws: one sparsity pattern, three sets of values), the Schur blocks of the 2 x 2
partition of N = 24, the `micro` case of lorasc_ref / nn_induced_ref, and the two amg_synth hierarchies of test_gpu_vq.py's
`kids` fixture. Comparisons are return codes, error texts and `np.array_equal`: no tolerance lives here.

"Fresh" is `fresh_context(api)`: the same inputs through handles created in a new `Context`, which shares no workspace,
graph, prediction or plan with the context under test."""
import contextlib
import ctypes as C

import numpy as np
import scipy.sparse as sp

import full_assembly_cases as fa
from conftest import f_m1, lognormal_coeff, u0734

vp, i64 = C.c_void_p, C.c_int64
NVEC, SPDIM = 3, 10            # of the deflated and eigCG solves
SEEDS = (None, 1, 2)           # coefficient of system k: constant 1, lognormal draws 1 and 2


def grid_systems(fem, N):
    """(mesh, plan, [a_k], [(A_k, b_k)]) for the three coefficients: the assembly plan of Example06's f and uexact, the nodal
    coefficients and the host systems (sorted CSR, one pattern). n = (N - 2)^2."""
    mesh = fem.get_mesh(N)
    plan = fa.make_plan(fem, mesh, f_m1, u0734)
    coeffs = [np.ones(mesh.points.shape[1]) if s is None else lognormal_coeff(fem, mesh.points, s) for s in SEEDS]
    systems = []
    for a in coeffs:
        _, A, b = fa.host_system(fem, mesh, a, f_m1, u0734)
        A = sp.csr_matrix(A)
        A.sort_indices()
        systems.append((A, b))
    assert all(np.array_equal(A.indices, systems[0][0].indices) and np.array_equal(A.indptr, systems[0][0].indptr) for A, _ in systems)
    return mesh, plan, coeffs, systems


def moved_pattern(A):
    """(indptr, indices, data, n) of A with one column index moved: same rows, same count (test_gpu_full_assembly's refusal)"""
    idx = A.indices.copy()
    idx[A.indptr[1] - 1] += 1
    return A.indptr, idx, A.data, A.shape[0]


def scipy_of(parts):
    ptr, idx, val, n = parts
    return sp.csr_matrix((val, idx, ptr), shape=(n, n))


def deflation_vectors(n, seed=5, k=NVEC):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((n, k)))


@contextlib.contextmanager
def fresh_context(api):
    c = api.Context(0)
    try:
        yield c
    finally:
        c.close()          # the operators of a closed context are abandoned by their wrappers (api.Operator.close)


def same_solve(got, want):
    """x, it, res_norm (and V of the eigCG family) bit for bit"""
    return (len(got) == len(want) and got[1] == want[1] and np.array_equal(got[2], want[2]) and np.array_equal(got[0], want[0])
            and all(np.array_equal(g, w) for g, w in zip(got[3:], want[3:])))


def trio(api, A, M, b, W):
    """pcg, defpcg with W and eigpcg, each twice (the second run replays the graphs and uses the prediction of the first):
    [pcg, pcg, defpcg, defpcg, eigpcg, eigpcg]"""
    x0 = np.zeros(b.size)
    out = []
    for _ in range(2):
        out.append(api.pcg(A, b, x0, M))
    for _ in range(2):
        out.append(api.defpcg(A, b, x0, W, M))
    for _ in range(2):
        out.append(api.eigpcg(A, b, x0, M, NVEC, SPDIM))
    return out


def fresh_trio(api, A, diag, b, W):
    """`trio` on (SparseMatrixCSC(A), JacobiPreconditioner(diag)) in a new context"""
    with fresh_context(api) as c:
        Ao, Mo = api.SparseMatrixCSC(c, A), api.JacobiPreconditioner(c, diag)
        out = trio(api, Ao, Mo, b, W)
        Mo.close(); Ao.close()
    return out


# ------------------------------------------------------------------ raw handles (mi_op_combine, mi_op_destroy)
def steal(op):
    """The raw handle of an api operator; the wrapper forgets it, so that no close() or finalizer can reach it"""
    h, op._h = op._h, None
    return h


def raw_combine(pkg, ctx, handles, coef):
    Lb = pkg._lib.load()
    arr = (vp * len(handles))(*handles)
    cf = np.ascontiguousarray(coef, dtype=np.float64)
    h = vp()
    rc = Lb.mi_op_combine(ctx._h, i64(len(handles)), arr, cf.ctypes.data_as(pkg._lib.f64p), C.byref(h))
    return rc, h


def raw_destroy(pkg, h):
    Lb = pkg._lib.load()
    rc = Lb.mi_op_destroy(h)
    return rc, (Lb.mi_last_error().decode() if rc else "")


def raw_apply(pkg, ctx, h, r):
    Lb = pkg._lib.load()
    ctx._mode_for(r)
    y = np.empty_like(r)
    rc = Lb.mi_op_apply(h, vp(r.ctypes.data), vp(y.ctypes.data))
    assert rc == 0, Lb.mi_last_error()
    return y


def host_expression(coef, ts):
    z = np.zeros_like(ts[0])
    for c, t in zip(coef, ts):
        z = z + c * t
    return z


# ------------------------------------------------------------------ Schur blocks of N = 24, 2 x 2
def schur_problems(fem, N=24):
    """two realizations of the 2 x 2 partition of get_mesh(N) on one set of patterns"""
    mesh = fem.get_mesh(N)
    return [fem.build_schur_problem(N, 2, 2, lognormal_coeff(fem, mesh.points, s), f_m1, u0734) for s in (1, 2)]


def csc_data(mats):
    out = []
    for m in mats:
        m = sp.csc_matrix(m)
        m.sort_indices()
        out.append(m.data)
    return np.concatenate(out)
