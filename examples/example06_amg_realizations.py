#!/usr/bin/env python3
"""The AMG loop of Example06_PcgStochasticEllipticPde.jl:160-200 on the full matrix, on the MI355X drop-in: per realization
of the lognormal coefficient, `pcg(A_t, b_t, 0, Π)` with

    Π_amg_0 = AMGPreconditioner{SmoothedAggregation}(A_0)       (:167, ξ = 0: a = 1)   -> api.AMGPreconditioner(ctx, A_0)
    Π_amg_t = AMGPreconditioner{SmoothedAggregation}(A_t)       (:182, per realization) -> Π_amg_t.set_values(A_t)

The reference rebuilds Π_amg_t on the host for every realization. Here one operator is created with `device_setup=True`
— the aggregation runs once, on A_0 — and `set_values` redoes the numbers of the hierarchy on the device (DESIGN §6g,
"Refresh"). Both iteration counts are printed per realization, with the time of the refresh beside the time of the host
set-up it replaces (`--host-setup` measures that too).

    python examples/example06_amg_realizations.py [--N 100] [--nreals 3] [--host-setup]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100, help="nodes per side")
    ap.add_argument("--nreals", type=int, default=3)
    ap.add_argument("--seed", type=int, default=481456)
    ap.add_argument("--host-setup", action="store_true", help="also time fem.prepare_amg_precond(A_t) per realization")
    args = ap.parse_args()
    pkg = graft.load_package()
    fem, api = pkg.fem, pkg.api
    mesh = fem.get_mesh(args.N)
    dinds = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
    f, uexact = (lambda x, y: -1.0 + 0 * x), (lambda x, y: 0.734 + 0 * x)                 # Example06:68-74
    assemble = lambda a: fem.do_isotropic_elliptic_assembly(mesh.cells, mesh.points, dinds, mesh.point_marker, a, f, uexact)
    kl = fem.synthetic_kl(mesh.points)
    rng = np.random.default_rng(args.seed)
    gs = [fem.draw(kl, rng)[1] for _ in range(args.nreals)]                               # :158-162
    A_0, _ = assemble(np.ones(mesh.points.shape[1]))                                      # :96-103, exp.(g_0) with g_0 = 0
    n = A_0.shape[0]
    print(f"nnode = {mesh.points.shape[1]}\nnel = {mesh.cells.shape[1]}\nn = {n}")

    ctx = api.Context(int(os.environ.get("LOCAL_RANK", "0")))
    t = time.time()
    Π_amg_0 = api.AMGPreconditioner(ctx, A_0)                                             # :167
    print(f"Π_amg_0: host set-up and create {time.time() - t:.2f} s, levels {Π_amg_0.hierarchy.sizes}")
    t = time.time()
    Π_amg_t = api.AMGPreconditioner(ctx, A_0, device_setup=True)
    print(f"Π_amg_t: aggregation on A_0, plan and first numeric phase {time.time() - t:.2f} s")
    x0 = np.zeros(n)
    iters_0, iters_t = [], []
    for ireal, g in enumerate(gs, 1):
        A, b = assemble(np.exp(g))                                                        # :175-179
        A_op = api.SparseMatrixCSC(ctx, A)
        t = time.perf_counter()
        Π_amg_t.set_values(A)                                                             # :182
        dt = time.perf_counter() - t
        line = f"realization {ireal}: set_values {1e3 * dt:.2f} ms"
        if args.host_setup:
            t = time.perf_counter()
            fem.prepare_amg_precond(A)
            line += f", fem.prepare_amg_precond {time.perf_counter() - t:.2f} s"
        _, it_0, res_0 = api.pcg(A_op, b, x0, Π_amg_0)
        u, it_t, res_t = api.pcg(A_op, b, x0, Π_amg_t)
        iters_0.append(int(it_0)); iters_t.append(int(it_t))
        print(f"{line}; pcg it = {it_0} with Π_amg_0, {it_t} with Π_amg_t, |b - A u| / |b| = "
              f"{np.linalg.norm(b - A @ u) / np.linalg.norm(b):.3e}")
        A_op.close()
    print(f"iters_0 = {iters_0}\niters_t = {iters_t}")
    Π_amg_t.close(); Π_amg_0.close()
    ctx.close()


if __name__ == "__main__":
    main()
