#!/usr/bin/env python3
"""Measures the device smoothed-aggregation AMG preconditioner (`api.AMGPreconditioner`) on the Example01 system
(a = 0.1 + 1e-4 x y) at config 2 (N = 500) and at N = 1000:

  - the host set-up (`fem.prepare_amg_precond`) and the device create;
  - one V-cycle (HIP events around eager applies on device pointers);
  - the fine-level k_amg_down by `time_dominant` (graph replay), beside the bare k_spmv_csr of the same matrix, each against
    its algorithmic bytes;
  - `it` and wall time of `pcg(A, b, 0, Π_amg)` and of the Jacobi-PCG it replaces, on the same system.
Every time is the mean of `--repeats` repeats with (max - min) / mean beside it.

    python tools/amg_probe.py --out profiles/amg_probe.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o amg -- python tools/amg_probe.py --N 1000 --trace-applies 5
    python tools/amg_probe.py --N 1000 --kernel-trace DIR/.../amg_kernel_trace.csv --trace-applies 5 --merge profiles/amg_probe.json

The traced run does applies only (no counters, a run of its own); its summary lists every launch of the cycle per level."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

WARMUP = 2


def timed(ctx, api, fn, repeats, inner=1):
    for _ in range(WARMUP):
        fn()
    ctx.synchronize()
    ms = []
    for _ in range(repeats):
        e0 = api.Event(ctx).record()
        for _ in range(inner):
            fn()
        e1 = api.Event(ctx).record()
        ctx.synchronize()
        ms.append(e0.elapsed_ms(e1) / inner)
    mean = float(np.mean(ms))
    return dict(mean_us=round(1e3 * mean, 2), spread=round((max(ms) - min(ms)) / mean, 4), repeats=repeats, applies_per_repeat=inner)


def wall(ctx, fn, repeats):
    out, ts = None, []
    for _ in range(WARMUP + repeats):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = ts[WARMUP:]
    mean = float(np.mean(ts))
    return out, dict(mean_ms=round(mean, 3), spread=round((max(ts) - min(ts)) / mean, 4), repeats=repeats)


def summarize(path, applies, nlevels):
    """per kernel name, the launches of one apply in order of appearance: level 0 first for down / restrict, last for
    prolong / post"""
    rows = {}
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"]
        if "k_amg_" in name:
            rows.setdefault(name.replace("void ", "").split("(")[0].split("::")[-1], []).append(
                (int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    out = {}
    total = applies + WARMUP
    for k, d in rows.items():
        d.sort()
        per = len(d) // total
        us = np.array([t for _, t in d[:per * total]]).reshape(total, per)[WARMUP:]
        order = list(range(per)) if k in ("k_amg_down", "k_amg_restrict", "k_amg_coarse") else list(range(per - 1, -1, -1))
        out[k] = dict(launches_per_apply=per, us_by_level=[round(float(us[:, j].mean()), 2) for j in order],
                      us_min_by_level=[round(float(us[:, j].min()), 2) for j in order], us_per_apply=round(float(us.sum(axis=1).mean()), 1))
    return dict(applies=applies, warmup=WARMUP, nlevels=nlevels, per_kernel=out,
                us_per_apply_all_kernels=round(sum(v["us_per_apply"] for v in out.values()), 1))


def measure(N, args, pkg, torch):
    fem, api = pkg.fem, pkg.api
    t0 = time.time()
    mesh = fem.get_mesh(N)
    d = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
    A, b = fem.do_isotropic_elliptic_assembly(mesh.cells, mesh.points, d, mesh.point_marker, lambda x, y: 0.1 + 0.0001 * x * y,
                                              lambda x, y: -1.0 + 0 * x, lambda x, y: 3.0 + 0 * x)
    n = b.size
    print(f"N = {N}: assembled n = {n} in {time.time() - t0:.1f} s", flush=True)
    t0 = time.time()
    H = fem.prepare_amg_precond(A)
    setup_s = time.time() - t0
    ctx = api.Context(0)
    t0 = time.time()
    M = api.AMGPreconditioner(ctx, H)
    create_s = time.time() - t0
    alg, dom = M.bytes()
    doc = dict(config=f"N={N} full matrix, a = 0.1 + 1e-4 x y (Example01)", n=n, nnz=int(A.nnz), levels=H.sizes,
               operator_complexity=round(H.operator_complexity, 4), host_setup_s=round(setup_s, 2), create_s=round(create_s, 2),
               launches_per_cycle=4 * (H.nlevels - 1) + 1, bytes_per_cycle=alg, bytes_fine_down=dom, bytes_fine_post=dom,
               stats=M.stats())
    print(f"  levels {H.sizes}, complexity {H.operator_complexity:.3f}, host set-up {setup_s:.1f} s, create {create_s:.2f} s", flush=True)
    r = torch.from_numpy(np.random.default_rng(0).standard_normal(n)).cuda()
    z = torch.empty_like(r)
    if args.trace_applies:
        for _ in range(WARMUP + args.trace_applies):
            M.apply(r, z)
        ctx.synchronize()
        return None
    doc["v_cycle"] = timed(ctx, api, lambda: M.apply(r, z), args.repeats, inner=20)
    doc["v_cycle"]["GBps"] = round(alg / doc["v_cycle"]["mean_us"] / 1e3, 1)
    Aop = api.SparseMatrixCSC(ctx, A)
    downs = [M.time_dominant(r, 200) for _ in range(args.repeats)]
    spmvs = [Aop.time_dominant(r, 200) for _ in range(args.repeats)]
    sb = Aop.bytes()[1]
    doc["k_amg_down_fine"] = dict(us=round(float(np.mean(downs)), 2), spread=round((max(downs) - min(downs)) / float(np.mean(downs)), 4),
                                  bytes=dom, GBps=round(dom / float(np.mean(downs)) / 1e3, 1))
    doc["k_spmv_csr_same_matrix"] = dict(us=round(float(np.mean(spmvs)), 2), spread=round((max(spmvs) - min(spmvs)) / float(np.mean(spmvs)), 4),
                                         bytes=sb, GBps=round(sb / float(np.mean(spmvs)) / 1e3, 1))
    print(f"  V-cycle {doc['v_cycle']}\n  k_amg_down {doc['k_amg_down_fine']}\n  k_spmv_csr {doc['k_spmv_csr_same_matrix']}", flush=True)
    x0 = np.zeros(n)
    (x, it, res), t_amg = wall(ctx, lambda: api.pcg(Aop, b, x0, M)[:3], args.repeats)
    doc["pcg_amg"] = dict(it=int(it), wall=t_amg, final_res_over_b=float(res[it - 1] / np.linalg.norm(b)))
    Mj = api.JacobiPreconditioner(ctx, A.diagonal())
    (xj, itj, resj), t_j = wall(ctx, lambda: api.pcg(Aop, b, x0, Mj)[:3], args.repeats)
    doc["pcg_jacobi"] = dict(it=int(itj), wall=t_j, final_res_over_b=float(resj[itj - 1] / np.linalg.norm(b)))
    doc["x_amg_vs_x_jacobi_rel_diff"] = float(np.linalg.norm(x - xj) / np.linalg.norm(xj))
    doc["wall_jacobi_over_amg"] = round(t_j["mean_ms"] / t_amg["mean_ms"], 2)
    print(f"  pcg AMG {doc['pcg_amg']}\n  pcg Jacobi {doc['pcg_jacobi']}\n  Jacobi / AMG wall {doc['wall_jacobi_over_amg']}", flush=True)
    for op in (Mj, Aop, M):
        op.close()
    ctx.close()
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[500, 1000])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace-applies", type=int, default=0, help="only this many applies (the program of a rocprofv3 run)")
    ap.add_argument("--kernel-trace", default="", help="per-dispatch CSV of the traced run: summarize it")
    ap.add_argument("--nlevels", type=int, default=0, help="levels of the traced hierarchy (for the summary's header)")
    ap.add_argument("--merge", default="", help="JSON file of an earlier run that receives the trace summary")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.kernel_trace:
        doc = json.load(open(args.merge)) if args.merge and os.path.exists(args.merge) else {}
        doc[f"rocprofv3_kernel_trace_N{args.N[0]}"] = summarize(args.kernel_trace, args.trace_applies, args.nlevels)
        text = json.dumps(doc, indent=1)
        print(text)
        if args.merge:
            open(args.merge, "w").write(text + "\n")
        return
    import torch
    pkg = graft.load_package()
    doc = {}
    for N in args.N:
        out = measure(N, args, pkg, torch)
        if out is not None:
            doc[f"N{N}"] = out
            if args.out:                              # after every size: a run that is cut short leaves what it has measured
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                open(args.out, "w").write(json.dumps(doc, indent=1) + "\n")
    if doc:
        print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
