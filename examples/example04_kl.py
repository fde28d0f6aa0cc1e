#!/usr/bin/env python3
"""Example02_KarhunenLoeve.jl and Example04_KarhunenLoeveDomainDecomposition.jl on the MI355X drop-in: from mesh and covariance
model to the KL modes (Λ, Ψ) of a Gaussian field, with every covariance evaluation on the device.

  global (Example02:36-46)   Λ, Φ = solve_kl(cells, points, cov, nev): the dominant pairs of C ϕ = λ M ϕ, C = M K M applied
                             matrix-free (api.CovarianceOperator) inside the device Lanczos eigensolver; draw; files.
  dd     (Example04:56-100)  solve_local_kl per subdomain, do_global_mass_covariance_reduced_assembly (panel products
                             Φ_d' M_d K(P_d, P_d') M_d' Φ_d' on the device), solve_global_reduced_kl, project_on_mesh, draw.

Files, named as the reference names them, under --out (with --flow both: under <out>/example02 and <out>/example04):
  <root>.kl-eigvals.npz, <root>.kl-eigvecs.npz, <root>.greal.npz,  <root> = get_root_filename(model, sig2, L, N²)
examples/example07_stochastic.py --kl <root> --kl-dir <dir> draws its coefficient fields from them.

The mesh is the structured N x N triangulation and the partition element boxes (fem.get_mesh / fem.mesh_partition stand in
for Triangle and METIS, as everywhere in this repository).

    python examples/example04_kl.py [--N 63 --px 5 --py 4 --nev 100 --nev-local 25 --model SExp --L 0.1 --forget 1e-6]
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
    ap.add_argument("--N", type=int, default=63, help="nodes per side (63² ≈ Example02's tentative_nnode = 4000)")
    ap.add_argument("--px", type=int, default=5)
    ap.add_argument("--py", type=int, default=4, help="px · py subdomains (Example04: ndom = 20)")
    ap.add_argument("--nev", type=int, default=100, help="global flow: wanted pairs (Example02: 500)")
    ap.add_argument("--nev-local", type=int, default=25, help="dd flow: wanted pairs per subdomain (Example04: 70)")
    ap.add_argument("--model", default="SExp", choices=["SExp", "Exp"])
    ap.add_argument("--sig2", type=float, default=1.0)
    ap.add_argument("--L", type=float, default=0.1)
    ap.add_argument("--forget", type=float, default=1e-6)
    ap.add_argument("--tol", type=float, default=1e-12)
    ap.add_argument("--flow", default="both", choices=["global", "dd", "both"])
    ap.add_argument("--seed", type=int, default=481456)
    ap.add_argument("--out", default="data")
    args = ap.parse_args()
    pkg = graft.load_package()
    fem, api, io = pkg.fem, pkg.api, pkg.io
    mesh = fem.get_mesh(args.N)
    cells, points = mesh.cells, mesh.points
    nnode = points.shape[1]
    root = io.get_root_filename(args.model, args.sig2, args.L, nnode)
    cov = dict(model=args.model, sig2=args.sig2, L=args.L)
    print(f"nnode = {nnode}\nnel = {cells.shape[1]}")
    ctx = api.Context(0)
    rng = np.random.default_rng(args.seed)

    def finish(Λ, Ψ, out):
        io.save_kl(Λ, Ψ, root, out)
        ξ, g = fem.draw(fem.SyntheticKL(Λ, Ψ), rng)
        print(f"sample: {Λ.size} modes, g in [{g.min():.3f}, {g.max():.3f}] -> {io.save_greal(g, root, out)}")

    if args.flow in ("global", "both"):
        print("solve_kl ...")
        t0 = time.time()
        Λ, Φ = api.solve_kl(ctx, cells, points, min(args.nev, nnode), relative=0.99, tol=args.tol, **cov)
        print(f"... done with solve_kl in {time.time() - t0:.2f} s")
        finish(Λ, Φ, os.path.join(args.out, "example02") if args.flow == "both" else args.out)

    if args.flow in ("dd", "both"):
        epart, _ = fem.mesh_partition(mesh, args.px, args.py)
        ndom = args.px * args.py
        relative_local, relative_global = fem.suggest_parameters(nnode)
        print("solve_local_kl ...")
        t0 = time.time()
        subs = []
        for idom in range(ndom):
            n_d = fem.kl_set_subdomain(cells, points, epart, idom)[0].size
            subs.append(api.solve_local_kl(ctx, cells, points, epart, min(args.nev_local, n_d), idom, relative=relative_local, tol=args.tol, **cov))
        print(f"... done with solve_local_kl in {time.time() - t0:.2f} s")
        Φd, centerd = [s.Φ for s in subs], [s.center for s in subs]
        energy_expected = sum(s.energy for s in subs)
        print("do_global_mass_covariance_reduced_assembly ...")
        t0 = time.time()
        K = api.do_global_mass_covariance_reduced_assembly(ctx, points, subs, Φd, centerd, forget=args.forget, **cov)
        print(f"... done with do_global_mass_covariance_reduced_assembly in {time.time() - t0:.2f} s: K is {K.shape[0]} x {K.shape[1]}")
        print("solve_global_reduced_kl ...")
        Λ, Ψ = fem.solve_global_reduced_kl(nnode, K, energy_expected, [s.elems for s in subs], [s.inds_l2g for s in subs], Φd,
                                           relative=relative_global)
        finish(Λ, Ψ, os.path.join(args.out, "example04") if args.flow == "both" else args.out)
    ctx.close()


if __name__ == "__main__":
    main()
