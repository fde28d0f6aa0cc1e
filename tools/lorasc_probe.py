#!/usr/bin/env python3
"""Measures the device LORASC preconditioner (`api.LorascPreconditioner`, Example03:245-256) at config 3 (N = 1000, 4x2
boxes, lognormal a = exp(g), seed 481456):
  - µs per apply, eager (HIP events around eager applies) and replayed (inside the solve graphs: µs per pcg iteration);
  - `it` and µs per iteration of pcg(A, b, 0, ΠA_lorasc) with nev = 0 and nev = 25 (E from fem.prepare_lorasc_precond,
    nvec = 25, the reference's default ε = 0.01, applied as the reference does: coef = 1);
  - with --kernel-stats CSV: the per-launch times of one `rocprofv3 --kernel-trace --stats` run of `--trace-applies K`:

    python tools/lorasc_probe.py --cache /tmp/lorasc.pkl --out profiles/lorasc_probe.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o lorasc -- \\
        python tools/lorasc_probe.py --cache /tmp/lorasc.pkl --trace-applies 5
    python tools/lorasc_probe.py --merge profiles/lorasc_probe.json --kernel-stats DIR/.../lorasc_kernel_stats.csv --trace-applies 5

`--cache` keeps the host-built problem (blocks, maps, E) between the runs."""
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
    A_IId, A_IΓd, A_ΓΓ, _, _ = fem.prepare_global_schur(mesh.cells, mesh.points, P.epart, P.sub, a, f, uex)
    A, b = fem.do_isotropic_elliptic_assembly(mesh.cells, mesh.points, P.dinds, mesh.point_marker, a, f, uex)
    pos_I, pos_Γ = fem.lorasc_maps(P.sub, P.dinds)
    # S dense from the device's exact elimination (the plan is needed anyway), then the host eigenpairs
    setup = api.SchurSetup(ctx, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd)
    Sd, _ = setup.run()
    n_Γ = P.sub.n_Γ
    S = np.zeros((n_Γ, n_Γ))
    for blk, gi in zip(setup.blocks(Sd), P.sub.gather_idx):
        S[np.ix_(gi, gi)] += blk
    setup.close()
    t = time.perf_counter()
    E, Σ = fem.prepare_lorasc_precond(S, A_ΓΓ, nvec=25, ε=0.01)
    return dict(blocks=(P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd), A_IΓd=A_IΓd, A_ΓΓ=sp.csc_matrix(A_ΓΓ), A=sp.csr_matrix(A), b=b,
                pos_I=pos_I, pos_Γ=pos_Γ, E=E, Σ=Σ, eig_s=time.perf_counter() - t)


def kernel_rows(path, applies):
    rows = [r for r in csv.DictReader(open(path)) if "mi::" in r["Name"]]
    out = {}
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        name = r["Name"].split("(")[0].replace("void ", "")
        out[name] = dict(calls_per_apply=round(int(r["Calls"]) / applies, 2), us_avg=round(float(r["AverageNs"]) / 1e3, 2),
                         us_per_apply=round(float(r["TotalDurationNs"]) / 1e3 / applies, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1000)
    ap.add_argument("--px", type=int, default=4)
    ap.add_argument("--py", type=int, default=2)
    ap.add_argument("--seed", type=int, default=481456)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cache", default="")
    ap.add_argument("--trace-applies", type=int, default=0)
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--merge", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.merge:                                      # fold a rocprofv3 kernel-stats CSV into an existing result
        doc = json.load(open(args.merge))
        doc["per_launch_rocprofv3_kernel_trace"] = dict(
            applies=args.trace_applies, note="set-up launches (plan run, A_ΓΓ factorization) are in the same trace: "
            "calls_per_apply of the k_lo_*, k_lv_* and k_sd_apply* rows is exact, other rows are set-up",
            kernels=kernel_rows(args.kernel_stats, args.trace_applies))
        with open(args.merge, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")
        return
    import torch
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
    n, n_Γ = D["A"].shape[0], D["pos_Γ"].size
    t = time.perf_counter()
    setup = api.SchurSetup(ctx, *D["blocks"])
    setup.keep_levels()
    setup.run()
    gg = api.SparseDirectPreconditioner(ctx, D["A_ΓΓ"])
    M = api.LorascPreconditioner(ctx, D["A_IΓd"], (D["pos_I"], D["pos_Γ"]), setup, gg)
    ctx.synchronize()
    t_setup = time.perf_counter() - t
    r = torch.from_numpy(np.random.default_rng(0).standard_normal(n)).cuda()
    z = torch.empty_like(r)
    if args.trace_applies:                              # the run that rocprofv3 traces
        M.set_correction(D["E"])
        for _ in range(args.trace_applies):
            M.apply(r, z)
        ctx.synchronize()
        return
    A = api.SparseMatrixCSC(ctx, D["A"])
    b = torch.from_numpy(D["b"]).cuda()
    out = dict(config=f"N={args.N} {args.px}x{args.py} boxes, lognormal a=exp(g) seed {args.seed}", n=n, n_gamma=int(n_Γ),
               host_build_s=round(t_build, 2), generalized_eig_s=round(D["eig_s"], 2), device_setup_s=round(t_setup, 2),
               bytes_per_apply=M.bytes()[0], bytes_one_level_solve=M.bytes()[1], spd_direct_stats=gg.stats, by_nev={})
    for nev in (0, D["E"].shape[1]):
        M.set_correction(D["E"] if nev else None)
        for _ in range(2):
            M.apply(r, z)
        e0, e1 = api.Event(ctx), api.Event(ctx)
        e0.record()
        for _ in range(10):
            M.apply(r, z)
        e1.record()
        us_apply = e0.elapsed_ms(e1) * 1e3 / 10
        x = torch.zeros(n, dtype=torch.float64, device="cuda")
        api.pcg(A, b, x, M)                             # warm-up: graph capture
        best, it = float("inf"), 0
        for _ in range(args.reps):
            x = torch.zeros(n, dtype=torch.float64, device="cuda")
            ctx.synchronize()
            t = time.perf_counter()
            _, it, res = api.pcg(A, b, x, M)
            ctx.synchronize()
            best = min(best, time.perf_counter() - t)
        out["by_nev"][str(nev)] = dict(us_apply_eager=round(us_apply, 1), pcg_it=int(it),
                                       pcg_us_per_it_replayed=round(best * 1e6 / max(it, 1), 1),
                                       final_res=float(np.asarray(res)[-1]))
        print(json.dumps({nev: out["by_nev"][str(nev)]}), flush=True)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
