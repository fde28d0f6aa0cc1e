#!/usr/bin/env python3
"""Measures the device Neumann-Neumann induced preconditioner (`api.NeumannNeumannInducedPreconditioner`, Example03:300-319)
at config 3 (N = 1000, 4x2 boxes, lognormal a = exp(g), seed 481456) from ONE `rocprofv3 --kernel-trace --stats` run of
`--trace-applies 5` (the program goes after `--`; no counters in that run):
  - the per-launch times of one apply;
  - in the same run, `k_gemv_nni` beside the existing Neumann-Neumann apply's `k_gemv_batched<…, true, …>` on the same
    blocks, for both storages: the second output adds 8 Σ n_Γd bytes to the blocks' ~68 MB, so the two should be equal
    within the run-to-run spread — the spread of the five launches is recorded next to the ratio.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o nni -- \\
        python tools/nn_induced_probe.py --cache /tmp/nni.pkl --trace-applies 5
    python tools/nn_induced_probe.py --kernel-trace DIR/.../nni_kernel_trace.csv --trace-applies 5 --out profiles/nn_induced_probe.json

`--cache` keeps the host-built problem (blocks, maps) between runs."""
import argparse
import csv
import json
import os
import pickle
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

WARMUP = 2


def build(args, fem):
    f = lambda x, y: -1.0 + 0 * x          # noqa: E731
    uex = lambda x, y: 0.734 + 0 * x       # noqa: E731
    mesh = fem.get_mesh(args.N)
    _, g = fem.draw(fem.synthetic_kl(mesh.points), np.random.default_rng(args.seed))
    P = fem.build_schur_problem(args.N, args.px, args.py, np.exp(g), f, uex, mesh=mesh, assemble=False)
    pos_I, pos_Γ = fem.lorasc_maps(P.sub, P.dinds)
    return dict(blocks=(P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd), pos_I=pos_I, pos_Γ=pos_Γ, gather=P.sub.gather_idx,
                cnt=np.asarray(P.sub.node_Γ_cnt))


def summarize(path, applies):
    """Per kernel name: the durations (µs) of its last `applies` x calls-per-apply dispatches, from the per-dispatch trace."""
    rows = {}
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"]
        if "mi::" not in name:
            continue
        rows.setdefault(name.replace("void ", "").split("(")[0], []).append(
            (int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))

    def five(name_has):
        hit = [k for k in rows if all(t in k for t in name_has)]
        assert len(hit) == 1, (name_has, hit)
        d = [us for _, us in sorted(rows[hit[0]])][-applies:]
        med = statistics.median(d)
        return dict(kernel=hit[0], us=[round(x, 2) for x in d], median_us=round(med, 2), spread=round((max(d) - min(d)) / med, 4))

    gemv = {}
    for sto, ty in (("f64", "double>"), ("f32", "float>")):
        nni, nn = five(("k_gemv_nni<", ty)), five(("k_gemv_batched<", "true", ty))
        gemv[sto] = dict(k_gemv_nni=nni, k_gemv_batched=nn, ratio_nni_over_batched=round(nni["median_us"] / nn["median_us"], 4),
                         within_spread=abs(nni["median_us"] / nn["median_us"] - 1.0) <= max(nni["spread"], nn["spread"]))
    per_launch = {}
    for k, v in rows.items():
        if any(t in k for t in ("k_lo_gather", "k_lo_zgamma", "k_gemv_nni", "k_nni_", "k_split_", "k_lv_")):
            d = [us for _, us in v]
            per_launch[k] = dict(calls=len(d), calls_per_apply=round(len(d) / (2 * (applies + WARMUP)), 2),
                                 us_avg=round(sum(d) / len(d), 2), us_min=round(min(d), 2), us_max=round(max(d), 2))
    return dict(applies=applies, warmup=WARMUP, gemv=gemv, per_launch=per_launch,
                note="both storages in one trace: calls_per_apply counts warm-up applies too; k_lv_* are the two level solves")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1000)
    ap.add_argument("--px", type=int, default=4)
    ap.add_argument("--py", type=int, default=2)
    ap.add_argument("--seed", type=int, default=481456)
    ap.add_argument("--cache", default="")
    ap.add_argument("--trace-applies", type=int, default=5)
    ap.add_argument("--kernel-trace", default="", help="per-dispatch CSV of the traced run: summarize it into --out")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.kernel_trace:
        doc = dict(config=f"N={args.N} {args.px}x{args.py} boxes, lognormal a=exp(g) seed {args.seed}",
                   rocprofv3_kernel_trace=summarize(args.kernel_trace, args.trace_applies))
        text = json.dumps(doc, indent=1)
        print(text)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(text + "\n")
        return
    import torch
    pkg = graft.load_package()
    fem, api = pkg.fem, pkg.api
    ctx = api.Context(0)
    if args.cache and os.path.exists(args.cache):
        D = pickle.load(open(args.cache, "rb"))
    else:
        D = build(args, fem)
        if args.cache:
            pickle.dump(D, open(args.cache, "wb"), protocol=4)
    setup = api.SchurSetup(ctx, *D["blocks"])
    setup.keep_levels()
    Sd, _ = setup.run()
    ΠSd = [np.asfortranarray(B) for B in setup.blocks(api.nn_pinv(ctx, setup.n_Γd, Sd))]
    n = int(sum(len(p) for p in D["pos_I"]) + D["pos_Γ"].size)
    rng = np.random.default_rng(0)
    r = torch.from_numpy(rng.standard_normal(n)).cuda()
    r_Γ = torch.from_numpy(rng.standard_normal(D["pos_Γ"].size)).cuda()
    z, z_Γ = torch.empty_like(r), torch.empty_like(r_Γ)
    for storage in ("f64", "f32"):
        M = api.NeumannNeumannInducedPreconditioner(ctx, D["blocks"][1], (D["pos_I"], D["pos_Γ"]), D["gather"], D["cnt"], ΠSd,
                                                    setup, storage=storage)
        Πnn = api.NeumannNeumannSchurPreconditioner(ctx, ΠSd, D["gather"], D["cnt"], storage=storage)
        for _ in range(WARMUP + args.trace_applies):      # interleaved: both kernels see the same machine state
            M.apply(r, z)
            Πnn.apply(r_Γ, z_Γ)
        ctx.synchronize()
        print(json.dumps(dict(storage=storage, bytes_per_apply=M.bytes()[0], bytes_one_level_solve=M.bytes()[1],
                              bytes_nn_blocks=Πnn.bytes()[1])), flush=True)
        M.close()
        Πnn.close()


if __name__ == "__main__":
    main()
