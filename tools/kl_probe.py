#!/usr/bin/env python3
"""Measures the Karhunen-Loève layer on the device at Example02's sizes, n ≈ 4 000 and 40 000 nodes:

  - one covariance launch at m = 1 (`time_dominant` of api.CovarianceOperator: graph replay, HIP events) and at m = col_block
    (HIP events around `mi_cov_apply` on device pointers), with the pair rate n² / t each;
  - one apply of C = M K M (SpMV, covariance, SpMV);
  - a whole `api.solve_kl` (wall time, restarts, applies);
  - the domain-decomposition flow: `solve_local_kl` over all subdomains and `do_global_mass_covariance_reduced_assembly`.
Every time is the mean of `--repeats` repeats with (max - min) / mean beside it.

    python tools/kl_probe.py --out profiles/kl_probe.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

WARMUP = 2


def stats(ts, unit):
    mean = float(np.mean(ts))
    return {f"mean_{unit}": round(mean, 3), "spread": round((max(ts) - min(ts)) / mean, 4), "repeats": len(ts)}


def events(ctx, api, fn, repeats):
    for _ in range(WARMUP):
        fn()
    ctx.synchronize()
    ms = []
    for _ in range(repeats):
        e0 = api.Event(ctx).record()
        fn()
        e1 = api.Event(ctx).record()
        ctx.synchronize()
        ms.append(e0.elapsed_ms(e1))
    return ms


def measure(N, args, pkg, torch):
    fem, api, L = pkg.fem, pkg.api, pkg._lib.load()
    mesh = fem.get_mesh(N)
    cells, points = mesh.cells, mesh.points
    n = points.shape[1]
    M = fem.get_mass_matrix(cells, points)
    ctx = api.Context(0)
    rt, sc, cb, splits1 = api.cov_tiling(n, n, 1)
    doc = dict(config=f"N={N} unit square, SExp, sig2 = 1, L = {args.L}", n=n, row_tile=rt, src_chunk=sc, col_block=cb,
               splits_m1=splits1, splits_mcb=api.cov_tiling(n, n, cb)[3])
    print(f"N = {N}: n = {n}, tiling {rt} x {sc} x {cb}, splits {splits1}", flush=True)
    op = api.CovarianceOperator(ctx, points, M, "SExp", 1.0, args.L)
    x = torch.from_numpy(np.random.default_rng(0).standard_normal(n)).cuda()
    us = [op.time_dominant(x, 20) for _ in range(args.repeats)]
    doc["cov_m1"] = dict(stats(us, "us"), Gpairs_per_s=round(n * n / float(np.mean(us)) / 1e3, 1))
    # m = col_block: mi_cov_apply on device pointers
    pts = torch.from_numpy(np.ascontiguousarray(points.T)).cuda()
    X = torch.from_numpy(np.random.default_rng(1).standard_normal((cb, n))).cuda()
    Y = torch.empty_like(X)
    torch.cuda.synchronize()

    def panel():
        rc = L.mi_cov_apply(ctx._h, C.c_int(0), C.c_double(1.0), C.c_double(args.L), C.c_int64(n), C.c_void_p(pts.data_ptr()), C.c_int64(n),
                            C.c_void_p(pts.data_ptr()), C.c_int64(cb), C.c_void_p(X.data_ptr()), C.c_int64(n), C.c_void_p(Y.data_ptr()), C.c_int64(n))
        assert rc == 0, L.mi_last_error()
    L.mi_ctx_set_pointer_mode(ctx._h, 1)
    ms = events(ctx, api, panel, args.repeats)
    L.mi_ctx_set_pointer_mode(ctx._h, 0)
    doc["cov_mcb"] = dict(stats([1e3 * t for t in ms], "us"), columns=cb, Gpairs_per_s=round(n * n / (1e3 * float(np.mean(ms))) / 1e3, 1),
                          note="includes the call's workspace hand-out and its closing synchronisation")
    y = torch.empty_like(x)
    ms = events(ctx, api, lambda: op.apply(x, y), args.repeats)
    doc["C_apply"] = stats([1e3 * t for t in ms], "us")
    op.close()
    print(f"  cov m=1 {doc['cov_m1']}\n  cov m={cb} {doc['cov_mcb']}\n  C apply {doc['C_apply']}", flush=True)
    ts, info = [], None
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        Λ, Φ = api.solve_kl(ctx, cells, points, args.nev, "SExp", 1.0, args.L, tol=args.tol, verbose=False)
        ts.append(time.perf_counter() - t0)
    doc["solve_kl"] = dict(stats(ts, "s"), nev=args.nev, kept=int(Λ.size), tol=args.tol, lambda_1=float(Λ[0]), includes="host mass matrix, operator creates")
    print(f"  solve_kl {doc['solve_kl']}", flush=True)
    px, py = args.px, args.py
    epart, _ = fem.mesh_partition(mesh, px, py)
    rel_local, _ = fem.suggest_parameters(n)
    t0 = time.perf_counter()
    subs = [api.solve_local_kl(ctx, cells, points, epart, args.nev_local, d, "SExp", 1.0, args.L, relative=rel_local, tol=args.tol, verbose=False)
            for d in range(px * py)]
    t_local = time.perf_counter() - t0
    Φd, cen = [s.Φ for s in subs], [s.center for s in subs]
    ts = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        K = api.do_global_mass_covariance_reduced_assembly(ctx, points, subs, Φd, cen, "SExp", 1.0, args.L, forget=1e-6)
        ts.append(time.perf_counter() - t0)
    off = np.concatenate([[0], np.cumsum([p.shape[1] for p in Φd])])
    nd = px * py
    computed = sum(1 for i in range(nd) for j in range(i, nd) if np.any(K[off[i]:off[i + 1], off[j]:off[j + 1]]))
    doc["dd"] = dict(ndom=nd, nev_local=args.nev_local, local_nodes=int(np.mean([s.inds_l2g.size for s in subs])),
                     solve_local_kl_all_s=round(t_local, 3), reduced_size=int(K.shape[0]), reduced_assembly=stats(ts, "s"),
                     blocks_computed=int(computed), blocks_upper=nd * (nd + 1) // 2)
    print(f"  dd {doc['dd']}", flush=True)
    ctx.close()
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[63, 200], help="nodes per side: 63² ≈ 4 000, 200² = 40 000 (Example02:11)")
    ap.add_argument("--L", type=float, default=0.1)
    ap.add_argument("--nev", type=int, default=50)
    ap.add_argument("--nev-local", type=int, default=25)
    ap.add_argument("--px", type=int, default=5)
    ap.add_argument("--py", type=int, default=4)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--repeats", type=int, default=3)
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
