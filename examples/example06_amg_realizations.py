#!/usr/bin/env python3
"""The AMG loop of Example06_PcgStochasticEllipticPde.jl:160-200 on the full matrix, on the MI355X drop-in: per realization
of the lognormal coefficient, `pcg(A_t, b_t, 0, Π)` with

    Π_amg_0 = AMGPreconditioner{SmoothedAggregation}(A_0)       (:167, ξ = 0: a = 1)   -> api.AMGPreconditioner(ctx, A_0)
    Π_amg_t = AMGPreconditioner{SmoothedAggregation}(A_t)       (:182, per realization) -> Π_amg_t.set_values(A_t)

The reference rebuilds Π_amg_t on the host for every realization. Here one operator is created with `device_setup=True`
— the aggregation runs once, on A_0 — and `set_values` redoes the numbers of the hierarchy on the device (DESIGN §6g,
"Refresh"). Both iteration counts are printed per realization, with the time of the refresh beside the time of the host
set-up it replaces (`--host-setup` measures that too).

`--device-assembly` keeps the whole realization on the device: ONE `A_op` is created once, and per realization
ξ -> `KLField.coefficient` -> `FullAssemblyPlan.run` -> `A_op.set_values(values)` and `Π_amg_t.set_values(values)` ->
`pcg(A_op, b, x0, Π)` with device tensors throughout; only ξ is uploaded. The device assembly has the bits of the host
assembly (`update_isotropic_elliptic_assembly!`, EllipticPde.jl:291-377) of the same coefficient, so the iteration counts
are those of the default path; its time is printed beside the host assembly's.

`--device-assembly --batch k` then runs the same k = `--nreals` realizations as ONE batch: the k values of ξ go
through one `KLField` pass, k `FullAssemblyPlan.update_batch` calls fill k slots of a `CsrBatch`, one
`AMGBank.set_values_batch` builds the k hierarchies into the members 0 .. k - 1 of a bank on the same aggregates, and one
`pcg_batch` solves every system under its own member. Its iteration counts are printed beside those of the loop above; they
must be equal.

    python examples/example06_amg_realizations.py [--N 100] [--nreals 3] [--host-setup] [--device-assembly [--batch 3]]
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
    ap.add_argument("--device-assembly", action="store_true", help="assemble A_t, b_t on the device and refresh one A_op in place")
    ap.add_argument("--batch", type=int, default=0, metavar="k",
                    help="with --device-assembly: also run k realizations (1 .. 16; --nreals is set to k) as one batch")
    args = ap.parse_args()
    if args.batch:
        if not args.device_assembly or not 1 <= args.batch <= 16:
            ap.error("--batch k needs --device-assembly and 1 <= k <= 16")
        args.nreals = args.batch
    pkg = graft.load_package()
    fem, api = pkg.fem, pkg.api
    mesh = fem.get_mesh(args.N)
    dinds = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
    f, uexact = (lambda x, y: -1.0 + 0 * x), (lambda x, y: 0.734 + 0 * x)                 # Example06:68-74
    assemble = lambda a: fem.do_isotropic_elliptic_assembly(mesh.cells, mesh.points, dinds, mesh.point_marker, a, f, uexact)
    kl = fem.synthetic_kl(mesh.points)
    rng = np.random.default_rng(args.seed)
    draws = [fem.draw(kl, rng) for _ in range(args.nreals)]                               # :158-162
    gs = [g for _, g in draws]
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
    if args.device_assembly:
        device_loop(args, fem, api, ctx, mesh, dinds, f, uexact, kl, [ξ for ξ, _ in draws], assemble, A_0, Π_amg_0, Π_amg_t)
        Π_amg_t.close(); Π_amg_0.close()
        ctx.close()
        return
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


def device_loop(args, fem, api, ctx, mesh, dinds, f, uexact, kl, ξs, assemble, A_0, Π_amg_0, Π_amg_t):
    import torch
    plan = api.FullAssemblyPlan(ctx, fem.make_full_assembly_plan(mesh.cells, mesh.points, dinds, mesh.point_marker, f, uexact))
    field = api.KLField(ctx, kl.Λ, kl.Ψ)
    A_op = api.SparseMatrixCSC(ctx, A_0)                                                  # once: refreshed in place below
    n = A_0.shape[0]
    iters_0, iters_t = [], []
    for ireal, ξ in enumerate(ξs, 1):
        a = field.coefficient(torch.from_numpy(ξ).cuda())                                 # :175, exp.(g) on the device
        ctx.synchronize()
        t = time.perf_counter()
        values, b = plan.run(a)                                                           # :176-179
        ctx.synchronize()
        dt_dev = time.perf_counter() - t
        t = time.perf_counter()
        assemble(a.cpu().numpy())
        dt_host = time.perf_counter() - t
        A_op.set_values(values)
        t = time.perf_counter()
        Π_amg_t.set_values(values)                                                        # :182
        dt = time.perf_counter() - t
        x0 = torch.zeros(n, dtype=torch.float64, device=a.device)
        _, it_0, _ = api.pcg(A_op, b, x0.clone(), Π_amg_0)
        u, it_t, _ = api.pcg(A_op, b, x0, Π_amg_t)
        iters_0.append(int(it_0)); iters_t.append(int(it_t))
        r = b - A_op * u
        print(f"realization {ireal}: assembly {1e3 * dt_dev:.3f} ms on the device (host: {dt_host:.2f} s), set_values {1e3 * dt:.2f} ms; "
              f"pcg it = {it_0} with Π_amg_0, {it_t} with Π_amg_t, |b - A u| / |b| = {float(torch.linalg.norm(r) / torch.linalg.norm(b)):.3e}")
    print(f"iters_0 = {iters_0}\niters_t = {iters_t}")
    if args.batch:
        batched(args.batch, api, ctx, plan, field, ξs, A_0, Π_amg_t.aggregates, iters_t)
    A_op.close(); plan.close()


def batched(k, api, ctx, plan, field, ξs, A_0, aggregates, iters_t):
    """the k realizations of the loop above as one batch: every system under the hierarchy of its own matrix"""
    import torch
    n = A_0.shape[0]
    batch, bank = api.CsrBatch(ctx, A_0, k), api.AMGBank(ctx, A_0, k, aggregates=aggregates)
    view = bank.view(k)
    ctx.synchronize()
    t = time.perf_counter()
    a = field.coefficient(torch.from_numpy(np.column_stack(ξs)).cuda())                   # one pass: column t is exp.(g_t)
    B = torch.stack([plan.update_batch(a[:, s].contiguous(), batch, s) for s in range(k)]).T
    ctx.synchronize()
    dt_asm = time.perf_counter() - t
    t = time.perf_counter()
    bank.set_values_batch(np.arange(k), batch, np.arange(k))                              # :182, k at a time
    dt_set = time.perf_counter() - t
    t = time.perf_counter()
    X = torch.zeros((k, n), dtype=torch.float64, device="cuda").T
    _, its, _ = api.pcg_batch(batch, np.arange(k), B, X, view, np.arange(k))
    ctx.synchronize()
    dt_solve = time.perf_counter() - t
    print(f"batch of {k}: field + assembly {1e3 * dt_asm:.3f} ms, set_values_batch {1e3 * dt_set:.2f} ms, pcg_batch {1e3 * dt_solve:.2f} ms")
    print(f"iters_t = {iters_t} (one realization at a time)\niters_b = {[int(i) for i in its]} (one batch)")
    assert [int(i) for i in its] == iters_t, "the batched flow and the loop disagree"
    batch.close(); bank.close()


if __name__ == "__main__":
    main()
