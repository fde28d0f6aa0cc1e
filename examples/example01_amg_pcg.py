#!/usr/bin/env python3
"""Example01_EllipticPde.jl:33-61 on the MI355X drop-in: the full Galerkin system of -∇·(a ∇u) = f with
a = 0.1 + 1e-4 x y, solved by `pcg(A, b, zeros(n), Π_amg)` with the smoothed-aggregation AMG preconditioner.

    Π_amg = AMGPreconditioner{SmoothedAggregation}(A)        (:49-53)   -> api.AMGPreconditioner(ctx, A)
    u, it, _ = pcg(A, b, zeros(A.n), Π_amg)                  (:58)      -> api.pcg(A_op, b, x0, Π_amg)

The hierarchy is built on the host once (`fem.prepare_amg_precond`), the V(1,1) cycle and the whole solve run on the
device. The smoother is damped Jacobi where the reference's is symmetric Gauss-Seidel, so `it` is this
library's own; it is compared here with a numpy restatement of the same cycle and of cg.jl:67-109, and with Jacobi-PCG.

    python examples/example01_amg_pcg.py [--N 100]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402


def cycle(H, b, l=0):
    """the V(1,1) cycle in numpy (tests/amg_ref.py)"""
    if l == H.nlevels - 1:
        return H.coarse_inv @ b
    A, P, wd = H.A[l], H.P[l], H.omega_over_d[l]
    x = wd * b
    e = cycle(H, P.T @ (b - A @ x), l + 1)
    x = x + P @ e
    return x + wd * (b - A @ x)


def pcg_numpy(A, b, M, eps=1e-7):
    """cg.jl:67-109"""
    x = np.zeros(b.size)
    r = b.copy()
    z = M(r)
    p, rTz, it = z.copy(), r @ z, 1
    res = [np.linalg.norm(r)]
    while it < b.size and res[-1] > eps * np.linalg.norm(b):
        Ap = A @ p
        α = rTz / (p @ Ap)
        β = 1.0 / rTz
        x += α * p
        r -= α * Ap
        z = M(r)
        rTz = r @ z
        β *= rTz
        p = z + β * p
        it += 1
        res.append(np.linalg.norm(r))
    return x, it, np.asarray(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100, help="nodes per side (Example01 uses a 1 M DoF mesh: --N 1000)")
    ap.add_argument("--no-check", action="store_true", help="skip the numpy restatement")
    args = ap.parse_args()
    pkg = graft.load_package()
    fem, api = pkg.fem, pkg.api
    mesh = fem.get_mesh(args.N)
    dinds = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
    A, b = fem.do_isotropic_elliptic_assembly(mesh.cells, mesh.points, dinds, mesh.point_marker,
                                              lambda x, y: 0.1 + 0.0001 * x * y,          # Example01:33-35
                                              lambda x, y: -1.0 + 0 * x, lambda x, y: 3.0 + 0 * x)
    n = b.size
    print(f"nnode = {mesh.points.shape[1]}\nnel = {mesh.cells.shape[1]}\nn = {n}")
    t = time.time()
    H = fem.prepare_amg_precond(A)
    print(f"AMG set-up (host) {time.time() - t:.2f}s: levels {H.sizes}, operator complexity {H.operator_complexity:.3f}")

    ctx = api.Context(int(os.environ.get("LOCAL_RANK", "0")))
    A_op = api.SparseMatrixCSC(ctx, A)
    Π_amg = api.AMGPreconditioner(ctx, H)
    x0 = np.zeros(n)
    api.pcg(A_op, b, x0, Π_amg)                                                          # first call: graphs are captured
    t = time.perf_counter()
    u, it, res = api.pcg(A_op, b, x0, Π_amg)
    dt = time.perf_counter() - t
    print(f"pcg(A, b, 0, Π_amg): it = {it}, |r| / |b| = {res[it - 1] / np.linalg.norm(b):.3e}, "
          f"|b - A u| / |b| = {np.linalg.norm(b - A @ u) / np.linalg.norm(b):.3e}, {1e3 * dt:.2f} ms")
    Π_j = api.JacobiPreconditioner(ctx, A.diagonal())
    api.pcg(A_op, b, x0, Π_j)
    t = time.perf_counter()
    uj, itj, _ = api.pcg(A_op, b, x0, Π_j)
    print(f"pcg(A, b, 0, Jacobi): it = {itj}, {1e3 * (time.perf_counter() - t):.2f} ms, |u - u_jacobi| / |u| = "
          f"{np.linalg.norm(u - uj) / np.linalg.norm(u):.3e}")
    if not args.no_check:
        ur, itr, resr = pcg_numpy(A, b, lambda r: cycle(H, r))
        print(f"numpy restatement: it = {itr}, max rel. history difference {np.max(np.abs(res - resr[:it]) / resr[:it]):.3e}, "
              f"|u - u_ref| / |u_ref| = {np.linalg.norm(u - ur) / np.linalg.norm(ur):.3e}")
        assert it == itr, (it, itr)
    u_full = fem.append_bc(dinds, u, mesh.points, lambda x, y: 3.0 + 0 * x)               # Example01:60
    print(f"u in [{u_full.min():.6f}, {u_full.max():.6f}]")


if __name__ == "__main__":
    main()
