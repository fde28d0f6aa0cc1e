#!/usr/bin/env python3
"""fp32-stored vs fp64-stored Neumann-Neumann blocks at config 3 (N=1000, 4x2, lognormal): kernel-only time of the plain
ΠS apply (mi_op_time_dominant), bytes per launch, and wall time per iteration and `it` of pcg(S, b, 0, ΠSnn), both
storages in one process, alternating. Writes profiles/nn_f32_probe.json (or --out).

    python tools/nn_f32_probe.py [--N 1000 --px 4 --py 2 --reps 200 --solves 30 --out profiles/nn_f32_probe.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o nn_f64 -- python tools/nn_f32_probe.py --trace-storage f64
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o nn_f32 -- python tools/nn_f32_probe.py --trace-storage f32
  then DIR/nn_<storage>_kernel_stats.csv -> profiles/nn_f32_kernel_stats_<storage>.csv
(the per-launch device time of k_gemv_pcg<..., float> beside k_gemv_pcg<..., double>: profiles/nn_f32_kernel_stats_*.csv)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1000)
    ap.add_argument("--px", type=int, default=4)
    ap.add_argument("--py", type=int, default=2)
    ap.add_argument("--seed", type=int, default=481456)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--solves", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nn_f32_probe.json"))
    ap.add_argument("--trace-storage", choices=["f64", "f32"], default=None,
                    help="only --solves solves with this storage and nothing else: the run to put under "
                         "`rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/nn_f32_probe.py --trace-storage f32`")
    args = ap.parse_args()
    pkg = graft.load_package()
    fem, api = pkg.fem, pkg.api
    mesh = fem.get_mesh(args.N)
    kl = fem.synthetic_kl(mesh.points)
    a = np.exp(fem.draw(kl, np.random.default_rng(args.seed))[1])
    P = fem.build_schur_problem(args.N, args.px, args.py, a, lambda x, y: -1.0 + 0 * x, lambda x, y: 0.734 + 0 * x)
    sub = P.sub
    n, b = sub.n_Γ, P.b_schur
    ctx = api.Context(0)
    S = api.LocalSchurs(ctx, P.Sd, sub.gather_idx, sub.node_Γ_cnt)
    M = {st: api.NeumannNeumannSchurPreconditioner(ctx, P.ΠSd, sub.gather_idx, sub.node_Γ_cnt, storage=st) for st in ("f64", "f32")}
    x0 = np.zeros(n)
    if args.trace_storage:
        for _ in range(args.solves):
            x, it, _ = api.pcg(S, b, x0, M[args.trace_storage])
        ctx.synchronize()
        print(f"{args.trace_storage}: {args.solves} solves, it={it}")
        return
    out = {"N": args.N, "n_gamma": int(n), "ndom": int(sub.ndom), "reps": args.reps, "solves": args.solves,
           "S_bytes_dominant": S.bytes()[1], "S_apply_us": [], "storages": {}}
    for st in M:
        out["storages"][st] = {"bytes_dominant": M[st].bytes()[1], "apply_us": [], "pcg_us_per_it": [], "it": None}
        M[st].time_dominant(b, 20)                       # warm-up
        out["storages"][st]["it"] = int(api.pcg(S, b, x0, M[st])[1])
    S.time_dominant(b, 20)
    for _ in range(args.rounds):                         # alternating: both storages see the same drift
        out["S_apply_us"].append(S.time_dominant(b, args.reps))
        for st in M:
            r = out["storages"][st]
            r["apply_us"].append(M[st].time_dominant(b, args.reps))
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.solves):
                api.pcg(S, b, x0, M[st])
            ctx.synchronize()
            r["pcg_us_per_it"].append((time.perf_counter() - t0) / args.solves / r["it"] * 1e6)
    for st, r in out["storages"].items():
        us = float(np.median(r["apply_us"]))
        r["apply_us_median"] = us
        r["apply_GBps"] = r["bytes_dominant"] / us * 1e-3
        r["pcg_us_per_it_median"] = float(np.median(r["pcg_us_per_it"]))
        print(f"{st}: ΠS kernel {us:.2f} us ({r['bytes_dominant'] / 1e6:.1f} MB, {r['apply_GBps']:.0f} GB/s)  "
              f"pcg {r['pcg_us_per_it_median']:.2f} us/it (whole solve / it, host included)  it={r['it']}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
