#!/usr/bin/env python3
"""Measures the device eigensolver (`api.eigsolve` / `api.geneigsolve`, csrc/lanczos.hpp) at config 3 (N = 1000, 4x2 boxes,
lognormal a = exp(g), seed 481456) against today's host path, in one run:
  - S (assembled local Schur complements), :SR, nev = 18, krylovdim = 36, tol = 1e-10: wall time, restarts, applies;
  - the host path for the same pairs: S densified by n_Γ applies against the identity, then numpy.linalg.eigh;
  - the LORASC pencil (S, A_ΓΓ), nvec = 25, krylovdim = 50, against densify + scipy.linalg.eigh(S, A_ΓΓ);
  - the largest differences between the device and the host eigenvalues;
  - with --kernel-stats CSV: µs per launch of the k_lz_* kernels from one `rocprofv3 --kernel-trace --stats` run of
    `--trace` (the standard problem only), and the achieved bytes/s of the three sweeps from their algorithmic bytes (n 8-byte rows per column):
        k_lz_project         (c + 1) columns read                      c = active columns of the step
        k_lz_update_project  (2 c + 1) read (V twice, the second time from cache where the slice fits) + 1 written
        k_lz_update_norm     (c + 1) read + 1 written

    python tools/eigsolve_probe.py --cache /tmp/eigsolve.pkl --out profiles/eigsolve_probe.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o eig -- python tools/eigsolve_probe.py --cache /tmp/eigsolve.pkl --trace
    python tools/eigsolve_probe.py --merge profiles/eigsolve_probe.json --kernel-stats DIR/.../eig_kernel_stats.csv

`--cache` keeps the host-built blocks between the runs."""
import argparse
import csv
import json
import os
import pickle
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402


def build(args, fem, api, ctx):
    f = lambda x, y: -1.0 + 0 * x          # noqa: E731
    uex = lambda x, y: 0.734 + 0 * x       # noqa: E731
    mesh = fem.get_mesh(args.N)
    _, g = fem.draw(fem.synthetic_kl(mesh.points), np.random.default_rng(args.seed))
    a = np.exp(g)
    P = fem.build_schur_problem(args.N, args.px, args.py, a, f, uex, mesh=mesh, assemble=False)
    A_ΓΓ = fem.prepare_global_schur(mesh.cells, mesh.points, P.epart, P.sub, a, f, uex)[2]
    setup = api.SchurSetup(ctx, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd)          # S_d by the device's exact elimination
    Sd, _ = setup.run()
    blocks = [np.asfortranarray(b) for b in setup.blocks(Sd)]
    setup.close()
    return dict(Sd=blocks, gather_idx=P.sub.gather_idx, cnt=P.sub.node_Γ_cnt, A_ΓΓ=sp.csc_matrix(A_ΓΓ), n_Γ=P.sub.n_Γ)


def column_steps(nev, m, restarts):
    """active columns c = j + 1 of every step of a run without break-down"""
    k = min(nev + (m - nev) // 2, m - 1)
    return list(range(1, m + 1)) + restarts * list(range(k + 1, m + 1))


def kernel_rows(path, doc):
    rows = {r["Name"].split("(")[0].replace("void ", "").replace("mi::", ""): r for r in csv.DictReader(open(path)) if "k_lz_" in r["Name"] or "k_eig_rotate" in r["Name"]}
    n = doc["n_gamma"]
    cols = column_steps(18, 36, doc["standard"]["restarts"])           # --trace runs the standard problem only
    reads = {"k_lz_project": sum(c + 1 for c in cols), "k_lz_update_project": sum(2 * c + 2 for c in cols),
             "k_lz_update_norm": sum(c + 2 for c in cols)}
    out = {}
    for name, r in rows.items():
        us = float(r["TotalDurationNs"]) / 1e3
        out[name] = dict(calls=int(r["Calls"]), us_avg=round(float(r["AverageNs"]) / 1e3, 2), us_total=round(us, 1))
        if name in reads:
            per_launch = 8.0 * n * reads[name] / len(cols)
            out[name]["algorithmic_bytes_per_launch_mean"] = int(per_launch)
            out[name]["GB_per_s"] = round(per_launch / (float(r["AverageNs"]) * 1e-9) / 1e9, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1000)
    ap.add_argument("--px", type=int, default=4)
    ap.add_argument("--py", type=int, default=2)
    ap.add_argument("--seed", type=int, default=481456)
    ap.add_argument("--cache", default="")
    ap.add_argument("--trace", action="store_true", help="only the standard device eigensolve, twice (the run rocprofv3 traces)")
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--merge", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.merge:
        doc = json.load(open(args.merge))
        doc["per_launch_rocprofv3_kernel_trace"] = kernel_rows(args.kernel_stats, doc)
        with open(args.merge, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")
        return
    pkg = graft.load_package()
    fem, api = pkg.fem, pkg.api
    ctx = api.Context(0)
    t0 = time.perf_counter()
    if args.cache and os.path.exists(args.cache):
        D = pickle.load(open(args.cache, "rb"))
    else:
        D = build(args, fem, api, ctx)
        if args.cache:
            pickle.dump(D, open(args.cache, "wb"), protocol=4)
    t_build = time.perf_counter() - t0
    n = int(D["n_Γ"])
    S = api.LocalSchurs(ctx, D["Sd"], D["gather_idx"], D["cnt"])
    B = api.SparseMatrixCSC(ctx, D["A_ΓΓ"])
    Binv = api.SparseDirectPreconditioner(ctx, D["A_ΓΓ"])
    v0 = np.random.default_rng(0).standard_normal(n)
    out = dict(config=f"N={args.N} {args.px}x{args.py} boxes, lognormal a=exp(g) seed {args.seed}", n_gamma=n, host_build_s=round(t_build, 2))

    def timed(fn):
        fn()                                                    # warm-up (allocations)
        ctx.synchronize()
        t = time.perf_counter()
        r = fn()
        ctx.synchronize()
        return r, time.perf_counter() - t
    (vals, X, info), t_std = timed(lambda: api.eigsolve(S, 18, "SR", krylovdim=36, tol=1e-10, maxiter=2000, v0=v0))
    out["standard"] = dict(nev=18, krylovdim=36, tol=1e-10, wall_s=round(t_std, 4), restarts=info.numiter, applies=info.numops,
                           converged=info.converged, bytes_per_apply=S.bytes()[0])
    print(json.dumps(out["standard"]), flush=True)
    if args.trace:
        return
    (gvals, E, ginfo), t_gen = timed(lambda: api.geneigsolve(S, B, Binv, 25, "SR", krylovdim=50, tol=1e-10, maxiter=2000, v0=v0))
    out["pencil"] = dict(nvec=25, krylovdim=50, tol=1e-10, wall_s=round(t_gen, 4), restarts=ginfo.numiter, applies=ginfo.numops,
                         converged=ginfo.converged)
    print(json.dumps(out["pencil"]), flush=True)
    t = time.perf_counter()
    Sdense = np.column_stack([S * col for col in np.eye(n)])
    t_dense = time.perf_counter() - t
    t = time.perf_counter()
    lam = np.linalg.eigh((Sdense + Sdense.T) / 2)[0]
    t_eigh = time.perf_counter() - t
    import scipy.linalg as sla
    t = time.perf_counter()
    A = D["A_ΓΓ"].toarray()
    glam = sla.eigh((Sdense + Sdense.T) / 2, (A + A.T) / 2, subset_by_index=[0, 24])[0]
    t_geigh = time.perf_counter() - t
    out["host_path"] = dict(densify_s=round(t_dense, 3), applies=n, eigh_s=round(t_eigh, 3), generalized_eigh_s=round(t_geigh, 3))
    out["standard"]["max_abs_value_difference_to_eigh"] = float(np.max(np.abs(vals - lam[:18])))
    out["pencil"]["max_abs_value_difference_to_eigh"] = float(np.max(np.abs(gvals - glam)))
    out["standard"]["speedup_over_host_path"] = round((t_dense + t_eigh) / t_std, 1)
    out["pencil"]["speedup_over_host_path"] = round((t_dense + t_geigh) / t_gen, 1)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
