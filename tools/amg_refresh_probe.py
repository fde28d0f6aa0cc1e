#!/usr/bin/env python3
"""Measures the device refresh of the AMG hierarchy (`AMGPreconditioner(ctx, A, device_setup=True).set_values`)
against the only route there was before it, in one run, at config 2 (N = 500) and at N = 1000. A0 is the Example01 matrix
(a = 0.1 + 1e-4 x y), A1 the lognormal one of the same mesh:

  - `set_values(A1)` on a device tensor: HIP events around every call, median of `--repeats` calls after warm-up, with
    (max - min) / median beside it; and on a host array (adds the upload);
  - the host route for the same matrix: `fem.prepare_amg_precond(A1)` plus `AMGPreconditioner(ctx, H)`, wall clock;
  - the share of every kernel group of one refresh (`refresh_profile`, events between the groups);
  - what is paid once: aggregation + plan + first numeric phase (the constructor), and the bytes kept;
  - `it` of `pcg(A1, b, 0, Π)` with the refreshed hierarchy and with the stale one (the hierarchy of A0).

    python tools/amg_refresh_probe.py --out profiles/amg_refresh_probe.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

WARMUP = 2


def measure(N, args, pkg, torch):
    fem, api = pkg.fem, pkg.api
    mesh = fem.get_mesh(N)
    d = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
    f, u = (lambda x, y: -1.0 + 0 * x), (lambda x, y: 3.0 + 0 * x)
    asm = lambda a: fem.do_isotropic_elliptic_assembly(mesh.cells, mesh.points, d, mesh.point_marker, a, f, u)
    A0, _ = asm(lambda x, y: 0.1 + 0.0001 * x * y)
    g = fem.draw(fem.synthetic_kl(mesh.points), np.random.default_rng(481456))[1]
    A1, b1 = asm(np.exp(g))
    for M in (A0, A1):
        M.sum_duplicates(); M.sort_indices()
    n = b1.size
    print(f"N = {N}: n = {n}, nnz = {A0.nnz}", flush=True)
    ctx = api.Context(0)
    t0 = time.perf_counter()
    M = api.AMGPreconditioner(ctx, A0, device_setup=True)
    once_s = time.perf_counter() - t0
    doc = dict(config=f"N={N} full matrix; A0: a = 0.1 + 1e-4 x y, A1: lognormal (synthetic KL, seed 481456)", n=n, nnz=int(A0.nnz),
               levels=M.hierarchy.sizes, once_aggregation_plan_first_refresh_s=round(once_s, 2), stats=M.stats())
    v_dev = torch.from_numpy(np.ascontiguousarray(A1.data)).cuda()
    torch.cuda.synchronize()
    ms = []
    for k in range(WARMUP + args.repeats):
        e0 = api.Event(ctx).record()
        M.set_values(v_dev)
        e1 = api.Event(ctx).record()
        ctx.synchronize()
        if k >= WARMUP:
            ms.append(e0.elapsed_ms(e1))
    med = float(np.median(ms))
    doc["set_values_device_ms"] = dict(median=round(med, 3), spread=round((max(ms) - min(ms)) / med, 4), repeats=args.repeats, warmup=WARMUP)
    ts = []
    for k in range(WARMUP + 3):
        t0 = time.perf_counter()
        M.set_values(A1.data)
        ts.append(1e3 * (time.perf_counter() - t0))
    doc["set_values_host_array_wall_ms"] = round(float(np.median(ts[WARMUP:])), 3)
    prof = M.refresh_profile()
    tot = sum(prof.values())
    doc["refresh_profile_ms"] = {k: round(v, 3) for k, v in prof.items()}
    doc["refresh_profile_share"] = {k: round(v / tot, 3) for k, v in prof.items()}
    hs = []
    for _ in range(args.host_repeats):
        t0 = time.perf_counter()
        H1 = fem.prepare_amg_precond(A1)
        t1 = time.perf_counter()
        Mh = api.AMGPreconditioner(ctx, H1)
        ctx.synchronize()
        hs.append((t1 - t0, time.perf_counter() - t1))
        if _ < args.host_repeats - 1:
            Mh.close()
    doc["host_route_s"] = dict(prepare_amg_precond=round(float(np.median([a for a, _ in hs])), 3),
                               create=round(float(np.median([b for _, b in hs])), 3), repeats=args.host_repeats)
    host_ms = 1e3 * (doc["host_route_s"]["prepare_amg_precond"] + doc["host_route_s"]["create"])
    doc["host_route_over_set_values"] = round(host_ms / med, 1)
    print(f"  set_values {doc['set_values_device_ms']} ms; host route {doc['host_route_s']} s; ratio {doc['host_route_over_set_values']}\n"
          f"  shares {doc['refresh_profile_share']}", flush=True)
    Aop = api.SparseMatrixCSC(ctx, A1)
    x0 = np.zeros(n)
    Ms = api.AMGPreconditioner(ctx, A0)
    it_f, it_h, it_s = (int(api.pcg(Aop, b1, x0, P)[1]) for P in (M, Mh, Ms))
    doc["pcg_it"] = dict(refreshed=it_f, fresh_host_hierarchy=it_h, stale_hierarchy_of_A0=it_s)
    print(f"  pcg it: {doc['pcg_it']}", flush=True)
    for op in (Ms, Mh, Aop, M):
        op.close()
    ctx.close()
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[500, 1000])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    pkg = graft.load_package()
    doc = {}
    for N in args.N:
        doc[f"N{N}"] = measure(N, args, pkg, torch)
        if args.out:                                  # after every size: a run that is cut short leaves what it has measured
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            open(args.out, "w").write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
