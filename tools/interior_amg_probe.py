#!/usr/bin/env python3
"""Measures the AMG `Pl` of the device interior CG (`MatrixFreeLocalSchurs.interior_amg`, DESIGN §6g "Interior `Pl`") at config 3
(N = 1000, 4 x 2 boxes, lognormal coefficient), in one run:

  - one matrix-free S-apply with `Pl` = none, diagonal and AMG (device vectors, wall clock around apply + synchronise: the
    apply waits for the host between graph replays, so that is its cost), mean of `--repeats` after 2 warm-ups with
    (max - min) / mean beside it; the same through the exact level solves of a set-up plan (`use_level_solver`);
  - the AMG apply for every `--chunks` value of MI355_ICG_CHUNK (iterations per graph replay) and for the default;
  - iterations of the slowest subdomain (MI355_ICG_CHUNK=1: exact) for the three `Pl`;
  - one `set_values(ii_val)` with the AMG selected (the device refresh of the hierarchy) and without;
  - levels, coarse rows and bytes kept.

`--host-counts` needs no GPU: the numpy restatement (tests/interior_amg_ref.py) for the iterations of every subdomain.
`--trace-applies K` only applies the AMG operator K times (the run `rocprofv3 --kernel-trace --stats` traces);
`--merge FILE --kernel-stats CSV --trace-applies K` folds that trace's kernel statistics into a result file.

    python tools/interior_amg_probe.py --out profiles/interior_amg_probe.json
"""
import argparse
import csv
import json
import os
import pickle
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

WARMUP = 2
RELTOL = 1e-9


def build(args, fem):
    if args.cache and os.path.exists(args.cache):
        return pickle.load(open(args.cache, "rb"))
    mesh = fem.get_mesh(args.N)
    _, g = fem.draw(fem.synthetic_kl(mesh.points), np.random.default_rng(args.seed))
    P = fem.build_schur_problem(args.N, args.px, args.py, np.exp(g), lambda x, y: -1.0 + 0 * x, lambda x, y: 0.734 + 0 * x,
                                assemble=False, precond=False)
    t0 = time.perf_counter()
    sizes, aggs = fem.prepare_interior_amg(P.A_IIdd)
    D = dict(A_II=P.A_IIdd, A_IG=P.A_IΓdd, A_GG=P.A_ΓΓdd, gi=P.sub.gather_idx, cnt=P.sub.node_Γ_cnt, sizes=sizes, aggs=aggs,
             aggregation_s=time.perf_counter() - t0)
    if args.cache:
        pickle.dump(D, open(args.cache, "wb"), protocol=4)
    return D


def kernel_rows(path, applies):
    groups = {"spmv": ("k_spmv_csr",), "vector": ("k_icg_",), "cycle": ("k_amg_",)}
    out = {k: dict(us_per_apply=0.0, calls_per_apply=0.0) for k in groups}
    rows = {}
    for r in csv.DictReader(open(path)):
        name = r["Name"].split("(")[0].replace("void mi::", "").strip()
        rows[name] = dict(calls_per_apply=round(int(r["Calls"]) / applies, 2), us_avg=round(float(r["AverageNs"]) / 1e3, 2),
                          us_per_apply=round(float(r["TotalDurationNs"]) / 1e3 / applies, 1))
        for k, pre in groups.items():
            if any(p in name for p in pre):
                out[k]["us_per_apply"] = round(out[k]["us_per_apply"] + rows[name]["us_per_apply"], 1)
                out[k]["calls_per_apply"] = round(out[k]["calls_per_apply"] + rows[name]["calls_per_apply"], 2)
    return dict(groups=out, kernels={k: v for k, v in rows.items() if any(p in k for pre in groups.values() for p in pre)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1000)
    ap.add_argument("--px", type=int, default=4)
    ap.add_argument("--py", type=int, default=2)
    ap.add_argument("--seed", type=int, default=481456)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunks", default="2,4,8,16,32")
    ap.add_argument("--cache", default="")
    ap.add_argument("--host-counts", action="store_true")
    ap.add_argument("--trace-applies", type=int, default=0)
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--merge", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.merge:
        doc = json.load(open(args.merge))
        doc["per_iteration_rocprofv3_kernel_trace"] = dict(
            applies=args.trace_applies, note="a run of its own; the k_spmv_csr rows include the three products around the interior solve, "
            "k_amg_* one cycle per iteration plus the first one of every solve", **kernel_rows(args.kernel_stats, args.trace_applies))
        open(args.merge, "w").write(json.dumps(doc, indent=1) + "\n")
        return
    pkg = graft.load_package()
    fem = pkg.fem
    D = build(args, fem)
    n_Γ = int(np.size(D["cnt"]))
    x = np.random.default_rng(0).standard_normal(n_Γ)
    if args.host_counts:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import interior_amg_ref as ir
        C = ir.Case("probe", D["A_II"], D["A_IG"], D["A_GG"], D["gi"], D["cnt"], {}, 0)
        out = {}
        for pl in ("amg", "diagonal"):
            _, its, hist, tol = C.solve(fem, x, pl=pl)
            out[pl] = [int(v) for v in its]
            print(pl, out[pl], flush=True)
        doc = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
        doc["restatement_iterations_per_subdomain"] = dict(note="numpy restatement, x = default_rng(0)", **out)
        if args.out:
            open(args.out, "w").write(json.dumps(doc, indent=1) + "\n")
        return
    import torch
    api = pkg.api
    ctx = api.Context(0)
    blocks = (D["A_II"], D["A_IG"], D["A_GG"])
    xd = torch.from_numpy(x).cuda()
    yd = torch.empty_like(xd)

    def make(chunk=None, amg=False, diag=False):
        if chunk is not None:
            os.environ["MI355_ICG_CHUNK"] = str(chunk)
        S = api.MatrixFreeLocalSchurs(ctx, *blocks, D["gi"], D["cnt"], None, reltol=RELTOL)
        os.environ.pop("MI355_ICG_CHUNK", None)
        if amg:
            S.interior_amg(sizes=D["sizes"], aggregates=D["aggs"])
        if diag:
            S.interior_precond("diagonal")
        return S

    def timed(fn, reps=None):
        ms = []
        for k in range(WARMUP + (reps or args.repeats)):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            if k >= WARMUP:
                ms.append(1e3 * (time.perf_counter() - t0))
        m = float(np.mean(ms))
        return dict(mean_ms=round(m, 3), spread=round((max(ms) - min(ms)) / m, 4), repeats=len(ms), warmup=WARMUP)

    if args.trace_applies:
        S = make(amg=True)
        for _ in range(args.trace_applies):
            S.apply(xd, yd)
        ctx.synchronize()
        return

    doc = dict(config=f"N={args.N} {args.px}x{args.py} boxes, lognormal a=exp(g) seed {args.seed}, reltol {RELTOL}", n_gamma=n_Γ,
               n_interior=int(sum(A.shape[0] for A in D["A_II"])), host_aggregation_s=round(D["aggregation_s"], 2))

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            open(args.out, "w").write(json.dumps(doc, indent=1) + "\n")

    def csc_values(mats):                       # the layout of set_values / SchurSetup.run: sorted CSC nzval, concatenated
        out = []
        for A in mats:
            A = A.tocsc()
            A.sort_indices()
            out.append(np.asarray(A.data, dtype=np.float64))
        return torch.from_numpy(np.concatenate(out)).cuda()

    ii, ig, gg = (csc_values(b) for b in blocks)
    # the exact answer and its time: the level solves of a set-up plan
    setup = api.SchurSetup(ctx, *blocks)
    setup.keep_levels()
    ctx.synchronize()
    t0 = time.perf_counter()
    setup.run(ii, ig, gg)
    ctx.synchronize()
    doc["level_setup_s"] = round(time.perf_counter() - t0, 3)
    Sl = make()
    Sl.use_level_solver(setup)
    doc["s_apply_level_solves"] = timed(lambda: Sl.apply(xd, yd))
    exact = yd.cpu().numpy().copy()
    print("level solves:", doc["s_apply_level_solves"], flush=True)
    Sl.close(); setup.close()
    save()

    def err():
        return float(np.abs(yd.cpu().numpy() - exact).max() / np.abs(exact).max())

    # iterations of the slowest subdomain, one iteration per replay
    its = {}
    for label, kw in (("none", {}), ("diagonal", dict(diag=True)), ("amg", dict(amg=True))):
        S = make(chunk=1, **kw)
        i0 = S.interior_iterations()
        S.apply(xd, yd)
        ctx.synchronize()
        its[label] = S.interior_iterations() - i0
        S.close()
    doc["iterations_slowest_subdomain"] = its
    print("iterations:", its, flush=True)
    save()

    S = make()
    doc["s_apply_pl_none"] = dict(timed(lambda: S.apply(xd, yd)), error_vs_level_solves=err())
    S.interior_precond("diagonal")
    doc["s_apply_pl_diagonal"] = dict(timed(lambda: S.apply(xd, yd)), error_vs_level_solves=err())
    print("none:", doc["s_apply_pl_none"], "\ndiagonal:", doc["s_apply_pl_diagonal"], flush=True)
    doc["set_values_ii_diagonal_only"] = timed(lambda: S.set_values(ii, None, None))
    S.close()
    save()

    Sa = make(amg=True)
    doc["amg"] = Sa.interior_amg_stats()
    doc["s_apply_pl_amg_default_chunk"] = dict(timed(lambda: Sa.apply(xd, yd)), error_vs_level_solves=err())
    print("amg:", doc["amg"], doc["s_apply_pl_amg_default_chunk"], flush=True)
    doc["set_values_ii_with_amg_refresh"] = timed(lambda: Sa.set_values(ii, None, None))
    print("refresh:", doc["set_values_ii_with_amg_refresh"], "diagonal only:", doc["set_values_ii_diagonal_only"], flush=True)
    Sa.close()
    save()
    doc["s_apply_pl_amg_by_chunk"] = {}      # MI355_ICG_CHUNK; s_apply_pl_amg_default_chunk above is the library's default
    for ch in [int(c) for c in args.chunks.split(",") if c]:
        Sc = make(chunk=ch, amg=True)
        doc["s_apply_pl_amg_by_chunk"][str(ch)] = timed(lambda: Sc.apply(xd, yd))
        print(f"chunk {ch}:", doc["s_apply_pl_amg_by_chunk"][str(ch)], flush=True)
        Sc.close()
        save()
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
