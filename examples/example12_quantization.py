#!/usr/bin/env python3
"""The flows of Example12_Quantization.jl, Example14_QuantizationAndShepardLocalInterpolation.jl and
Example20_QuantizedPreconditioner.jl in one driver, at small default sizes, on the MI355X drop-in:

    X, centroids, ... = get_quantizer(ns, P, Λ; distance)              (Example12_Quantization_Functions.jl:29-59)
                                                                        -> api.get_quantizer: k-means++ and Lloyd on the device
    Π = get_centroidal_preconds(centroids, Λ, Ψ)                       (:85-113) -> api.get_centroidal_preconds: per centroid,
                                                                        KLField.coefficient, assembly, AMGPreconditioner.set_values
    per fresh realization ξ: p = find_precond(ξ, centroids)            (Example20_…_Functions.jl:39-54) -> api.find_precond
                             pcg(A, b, 0, Π[p])                        (Example12_…_Functions.jl:147-160)
    --interpolate k:         pcg(A, b, 0, InterpolatingPreconditioner(shepard coefficients of the k nearest, their Π))
                                                                        (Example14_…_Functions.jl:73-113, 174-206)

The iteration counts are printed beside those of the constant preconditioner of ξ = 0 (Example06's Π_amg_0).

`--bank`: the same flow on ONE `api.AMGBank` (`api.get_centroidal_bank`): the P hierarchies share one plan and
one set of index arrays, `view.select(p)` / `view.combine(near, coef)` stand for `Π[p]` / `InterpolatingPreconditioner`, and
one captured solve graph serves every selection. The iteration counts are those of the default flow.

`--device-assembly`: every system, the centroids' and the realizations', is assembled on the device
(`api.FullAssemblyPlan`, bit-identical to the host assembly), and ONE `A_op` is refreshed in place per realization.

`--bank --batch k`: the realizations are solved k at a time in ONE Krylov loop. k values of ξ are drawn and their
coefficients come from one `KLField` pass; k calls of `FullAssemblyPlan.update_batch` fill k slots of an `api.CsrBatch`, one
`vq_assign` gives the k members, and one `api.pcg_batch` solves the k systems. `iters_quantized` is that of the unbatched flow.

    python examples/example12_quantization.py [--N 60] [--ns 2000] [--P 8] [--nreals 5] [--distance L2-full] [--interpolate 4]
                                              [--device-assembly] [--bank] [--batch 4]
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
    ap.add_argument("--N", type=int, default=60, help="nodes per side")
    ap.add_argument("--m-side", type=int, default=4, help="fem.synthetic_kl: m_side² modes")
    ap.add_argument("--ns", type=int, default=2000, help="draws of ξ that are clustered")
    ap.add_argument("--P", type=int, default=8, help="centroids")
    ap.add_argument("--nreals", type=int, default=5, help="fresh realizations that are solved")
    ap.add_argument("--distance", default="L2-full", choices=["L2", "L2-full", "L2-10%", "cdf", "cdf-full"])
    ap.add_argument("--interpolate", type=int, default=0, help="k > 0: Shepard combination of the k nearest centroids' preconditioners")
    ap.add_argument("--seed", type=int, default=987654321)
    ap.add_argument("--device-assembly", action="store_true", help="assemble on the device and refresh one A_op in place")
    ap.add_argument("--bank", action="store_true", help="hold the centroidal hierarchies in one AMGBank and select through a view")
    ap.add_argument("--batch", type=int, default=0, help="k > 0 (with --bank): solve the realizations k at a time with pcg_batch")
    args = ap.parse_args()
    if args.batch and (not args.bank or args.interpolate > 0 or not 1 <= args.batch <= 16):
        ap.error("--batch k: 1 <= k <= 16, with --bank and without --interpolate (one member per system)")
    if args.bank and min(args.interpolate, args.P) > 16:
        ap.error(f"--bank: a view combines at most 16 members, --interpolate {args.interpolate} with --P {args.P} asks for {min(args.interpolate, args.P)}")
    pkg = graft.load_package()
    fem, api = pkg.fem, pkg.api
    mesh = fem.get_mesh(args.N)
    dinds = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
    f, uexact = (lambda x, y: -1.0 + 0 * x), (lambda x, y: 0.734 + 0 * x)
    system = lambda a: fem.do_isotropic_elliptic_assembly(mesh.cells, mesh.points, dinds, mesh.point_marker, a, f, uexact)
    kl = fem.synthetic_kl(mesh.points, m_side=args.m_side)
    rng = np.random.default_rng(args.seed)
    ctx = api.Context(int(os.environ.get("LOCAL_RANK", "0")))
    field = api.KLField(ctx, kl.Λ, kl.Ψ)

    t = time.perf_counter()
    X, centroids, assignments, costs = api.get_quantizer(ctx, args.ns, args.P, kl.Λ, args.distance, rng=rng)
    sizes = np.bincount(np.asarray(assignments), minlength=args.P)
    print(f"quantizer: {args.ns} draws of {kl.Λ.size} coordinates into P = {args.P} cells ({args.distance}) in {time.perf_counter() - t:.3f} s; "
          f"cell sizes {sizes.tolist()}, distortion {float(np.sum(costs)) / args.ns:.4e}")

    A_0, _ = system(np.ones(mesh.points.shape[1]))
    plan = A_t = None
    if args.device_assembly or args.batch:
        plan = api.FullAssemblyPlan(ctx, fem.make_full_assembly_plan(mesh.cells, mesh.points, dinds, mesh.point_marker, f, uexact))
        A_t = api.SparseMatrixCSC(ctx, A_0)
    t = time.perf_counter()
    assemble = (lambda a: plan.run(a)[0]) if plan else (lambda a: system(a)[0])
    bank = view = None
    if args.bank:
        bank = api.get_centroidal_bank(ctx, centroids, field, assemble, A_0)
        view = bank.view(max(1, min(args.interpolate, args.P)))
        st = bank.stats()
        print(f"{args.P} centroidal AMG hierarchies (n = {A_0.shape[0]}) on one bank in {time.perf_counter() - t:.2f} s: "
              f"{st['bytes_shared']} bytes shared, {st['bytes_per_member']} per member")
    else:
        Π = api.get_centroidal_preconds(ctx, centroids, field, assemble, A_0)
        print(f"{args.P} centroidal AMG preconditioners (n = {A_0.shape[0]}) in {time.perf_counter() - t:.2f} s")
    Π_0 = api.AMGPreconditioner(ctx, A_0)

    scaled_centroids = fem.scale_data(centroids, kl.Λ, args.distance)
    rows = centroids.shape[0]
    iters_0, iters_q = [], []
    if args.batch:
        batched_flow(args, api, fem, ctx, rng, kl, field, plan, A_0, bank, scaled_centroids)
        bank.close()
        return
    for ireal in range(1, args.nreals + 1):
        ξ = rng.standard_normal(kl.Λ.size)
        if plan:
            b = plan.update(field.coefficient(ξ), A_t)
            A_op = A_t
        else:
            A, b = system(field.coefficient(ξ))
            A_op = api.SparseMatrixCSC(ctx, A)
        x0 = np.zeros(b.size)
        η = fem.scale_data(ξ, kl.Λ, args.distance)
        if args.interpolate > 0:
            _, dist2, _ = api.vq_assign(ctx, η.reshape(-1, 1), scaled_centroids, want_assign=False, want_objv=False)
            d2 = fem.vq_dist2(η[:, None], scaled_centroids)[0]
            near = np.argsort(d2, kind="stable")[:min(args.interpolate, args.P)]
            full = np.zeros((kl.Λ.size, near.size))
            full[:rows] = centroids[:, near]
            coef = fem.shepard_coefficients(ξ, full, kl.Λ)
            if bank:
                view.combine(near, coef)
                M = view
            else:
                M = api.InterpolatingPreconditioner(ctx, coef, [Π[p] for p in near])
            what = f"Shepard combination of centroids {near.tolist()} (nearest at squared distance {float(dist2[0]):.3e})"
        else:
            p = api.find_precond(ctx, η, scaled_centroids)
            if bank:
                view.select(p)
                M = view
            else:
                M = Π[p]
            what = f"centroid {p}"
        u, it_q, _ = api.pcg(A_op, b, x0, M)
        _, it_0, _ = api.pcg(A_op, b, x0, Π_0)
        iters_q.append(int(it_q)); iters_0.append(int(it_0))
        print(f"realization {ireal}: {what}: pcg it = {it_q} (ξ = 0 preconditioner: {it_0}), |b - A u| / |b| = "
              f"{np.linalg.norm(b - A_op * u) / np.linalg.norm(b):.3e}")
        if args.interpolate > 0 and not bank:
            M.close()
        if not plan:
            A_op.close()
    print(f"iters_quantized = {iters_q}\niters_xi_0 = {iters_0}")
    if bank:
        bank.close()


def batched_flow(args, api, fem, ctx, rng, kl, field, plan, A_0, bank, scaled_centroids):
    """k realizations per Krylov loop: the draws, the members and the solves of the loop above, k at a time"""
    kmax = args.batch
    batch = api.CsrBatch(ctx, A_0, kmax)
    view = bank.view(kmax)
    padded = np.zeros((kl.Λ.size, scaled_centroids.shape[1]), order="F")     # as find_precond pads the centroids
    padded[:scaled_centroids.shape[0]] = scaled_centroids
    iters_q, done = [], 0
    while done < args.nreals:
        k = min(kmax, args.nreals - done)
        Ξ = np.column_stack([rng.standard_normal(kl.Λ.size) for _ in range(k)])
        a = field.coefficient(Ξ)                                             # one pass over the modes for the k coefficients
        B = np.empty((plan.n, k), order="F")
        for t in range(k):
            B[:, t] = plan.update_batch(np.ascontiguousarray(a[:, t]), batch, t)
        H = np.asfortranarray(np.column_stack([fem.scale_data(Ξ[:, t], kl.Λ, args.distance) for t in range(k)]))
        members = np.asarray(api.vq_assign(ctx, H, padded, want_dist2=False, want_objv=False)[0], dtype=np.int64)
        t0 = time.perf_counter()
        X, its, _ = api.pcg_batch(batch, np.arange(k), B, np.zeros((plan.n, k), order="F"), view, members)
        dt = time.perf_counter() - t0
        print(f"realizations {done + 1} .. {done + k}: centroids {members.tolist()}: pcg_batch it = {its.tolist()} in {dt * 1e3:.2f} ms")
        iters_q += [int(i) for i in its]
        done += k
    print(f"iters_quantized = {iters_q}")
    view.close()
    batch.close()


if __name__ == "__main__":
    main()
