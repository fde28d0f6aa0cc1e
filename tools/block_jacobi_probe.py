#!/usr/bin/env python3
"""Measures the device block-Jacobi preconditioner (`api.BlockJacobiPreconditioner`) on the full matrix of
config 3 (N = 1000, lognormal a = exp(g), seed 481456) with nb = 8:

  - the numeric set-up (`set_values`: gather, elimination with kept levels, S_G^-1, checks);
  - one apply (HIP events around eager launches on device pointers);
  - the floor: `mi_schur_setup_interior_solve` on a set-up plan of the same split (ONE level solve);
  - the composed form: `NeumannNeumannInducedPreconditioner`, coupling "assembled", cnt = 1, ΠS_d = S_G^-1 on the same
    split (TWO level solves — what the operator avoids);
  - `it` and µs per iteration of `pcg(A, b, 0, Π_bj)` (graph-replayed chunks).
Every time is the mean of `--repeats` repeats with (max - min) / mean beside it.

    python tools/block_jacobi_probe.py --out profiles/block_jacobi_probe.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o bj -- python tools/block_jacobi_probe.py --trace-applies 5
    python tools/block_jacobi_probe.py --kernel-trace DIR/.../bj_kernel_trace.csv --trace-applies 5 --merge profiles/block_jacobi_probe.json

The traced run does applies only (no counters, a run of its own)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import scipy.sparse.csgraph as csgraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

WARMUP = 2


def default_split(A, nb):
    """The default seed rule of csrc/block_jacobi.hpp, vectorised: per block (lo, hi, G, I) with block-local indices."""
    A = sp.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    bsize = n // nb
    first, last = A.indices[A.indptr[:-1]], A.indices[A.indptr[1:] - 1]      # lowest / highest column of every row
    out = []
    for d in range(nb):
        lo, hi = d * bsize, (d + 1) * bsize if d + 1 < nb else n
        B = A[lo:hi, lo:hi]
        ncomp, lab = csgraph.connected_components(B, directed=False)
        low, high = first[lo:hi] < lo, last[lo:hi] >= hi
        c_low, c_high = np.zeros(ncomp, bool), np.zeros(ncomp, bool)
        c_low[lab[low]] = True
        c_high[lab[high]] = True
        seed = (low & c_low[lab]) | (high & ~c_low[lab] & c_high[lab])
        lowest = np.full(ncomp, hi - lo)
        np.minimum.at(lowest, lab, np.arange(hi - lo))
        lone = ~c_low & ~c_high
        seed[lowest[lone]] = True
        G = np.flatnonzero(seed)
        out.append((lo, hi, G, np.flatnonzero(~seed)))
    return out


def composed_inputs(A, split):
    A = sp.csc_matrix(A)
    ii, ig, gg, pos_I, gather = [], [], [], [], []
    off = 0
    for lo, hi, G, I in split:
        B = A[lo:hi, lo:hi]
        ii.append(sp.csc_matrix(B[I][:, I])); ig.append(sp.csc_matrix(B[I][:, G])); gg.append(sp.csc_matrix(B[G][:, G]))
        pos_I.append(lo + I)
        gather.append(np.arange(off, off + G.size))
        off += G.size
    pos_Γ = np.concatenate([lo + G for lo, _, G, _ in split])
    return ii, ig, gg, pos_I, pos_Γ, gather


def timed(ctx, api, fn, repeats):
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
    mean = float(np.mean(ms))
    return dict(mean_ms=round(mean, 4), spread=round((max(ms) - min(ms)) / mean, 4), repeats=repeats)


def summarize(path, applies):
    rows = {}
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"]
        if "mi::" in name:
            rows.setdefault(name.replace("void ", "").split("(")[0], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {}
    for k, d in rows.items():
        if any(t in k for t in ("k_bj_zg0", "k_bj_gamma", "k_bj_back0", "k_bj_scatter", "k_lv_")):
            out[k] = dict(calls=len(d), calls_per_apply=round(len(d) / (applies + WARMUP), 2), us_avg=round(sum(d) / len(d), 2),
                          us_min=round(min(d), 2), us_max=round(max(d), 2), us_per_apply=round(sum(d) / (applies + WARMUP), 1))
    return dict(applies=applies, warmup=WARMUP, per_launch=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1000)
    ap.add_argument("--nb", type=int, default=8)
    ap.add_argument("--seed", type=int, default=481456)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace-applies", type=int, default=0, help="only this many applies (the program of a rocprofv3 run)")
    ap.add_argument("--kernel-trace", default="", help="per-dispatch CSV of the traced run: summarize it")
    ap.add_argument("--merge", default="", help="JSON file of an earlier run that receives the trace summary")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.kernel_trace:
        doc = json.load(open(args.merge)) if args.merge and os.path.exists(args.merge) else {}
        doc["rocprofv3_kernel_trace"] = summarize(args.kernel_trace, args.trace_applies)
        text = json.dumps(doc, indent=1)
        print(text)
        if args.merge:
            open(args.merge, "w").write(text + "\n")
        return
    import torch
    pkg = graft.load_package()
    fem, api = pkg.fem, pkg.api
    f = lambda x, y: -1.0 + 0 * x          # noqa: E731
    uex = lambda x, y: 0.734 + 0 * x       # noqa: E731
    t0 = time.time()
    mesh = fem.get_mesh(args.N)
    _, g = fem.draw(fem.synthetic_kl(mesh.points), np.random.default_rng(args.seed))
    dinds = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
    A, b = fem.do_isotropic_elliptic_assembly(mesh.cells, mesh.points, dinds, mesh.point_marker, np.exp(g), f, uex)
    A = sp.csc_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    print(f"assembled n = {n} in {time.time() - t0:.1f} s", flush=True)
    ctx = api.Context(0)
    t0 = time.time()
    M = api.BlockJacobiPreconditioner(ctx, args.nb, A)
    st = M.stats()
    doc = dict(config=f"N={args.N} full matrix, lognormal a=exp(g) seed {args.seed}, nb={args.nb}", n=n, create_s=round(time.time() - t0, 2),
               n_g=[int(v) for v in st["n_g"]], n_levels=[int(v) for v in st["n_levels"]], max_level=[int(v) for v in st["max_level"]],
               kept_bytes=st["kept_bytes"], bytes_per_apply=M.bytes()[0], bytes_dominant=M.bytes()[1])
    def save():                                   # after every stage: a run that is cut short leaves what it has measured
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            open(args.out, "w").write(json.dumps(doc, indent=1) + "\n")

    print(f"created in {doc['create_s']} s: n_g {doc['n_g']}, levels {doc['n_levels']}, kept {st['kept_bytes'] / 1e9:.2f} GB", flush=True)
    r = torch.from_numpy(np.random.default_rng(0).standard_normal(n)).cuda()
    z = torch.empty_like(r)
    if args.trace_applies:
        for _ in range(WARMUP + args.trace_applies):
            M.apply(r, z)
        ctx.synchronize()
        return
    vals = torch.from_numpy(A.data.copy()).cuda()
    doc["set_values"] = timed(ctx, api, lambda: M.set_values(vals), args.repeats)
    doc["apply"] = timed(ctx, api, lambda: M.apply(r, z), args.repeats)
    doc["apply"]["GBps"] = round(M.bytes()[0] / doc["apply"]["mean_ms"] / 1e6, 1)
    print(f"set_values {doc['set_values']}, apply {doc['apply']}", flush=True)
    save()
    Ag = api.SparseMatrixCSC(ctx, A)
    x0 = np.zeros(n)
    its, us = [], []
    for _ in range(WARMUP + args.repeats):
        ctx.synchronize()
        t0 = time.perf_counter()
        _, it, _ = api.pcg(Ag, b, x0, M)
        ctx.synchronize()
        its.append(it); us.append((time.perf_counter() - t0) * 1e6 / max(it, 1))
    us = us[WARMUP:]
    doc["pcg"] = dict(it=its[-1], us_per_iteration=round(float(np.mean(us)), 1), spread=round((max(us) - min(us)) / float(np.mean(us)), 4),
                      note="host wall clock of the whole solve (host vectors in and out) over it")
    print(f"pcg {doc['pcg']}", flush=True)
    save()
    # the floor and the composed form on the same split
    split = default_split(A, args.nb)
    assert [len(s[2]) for s in split] == doc["n_g"], "the tool's split differs from the library's"
    ii, ig, gg, pos_I, pos_Γ, gather = composed_inputs(A, split)
    print("split blocks extracted", flush=True)
    setup = api.SchurSetup(ctx, ii, ig, gg)
    setup.keep_levels()
    Sd, _ = setup.run()
    fI = torch.from_numpy(np.random.default_rng(1).standard_normal(int(sum(setup.n_Id)))).cuda()
    doc["one_level_solve"] = timed(ctx, api, lambda: setup.interior_solve(fI), args.repeats)
    print(f"one level solve {doc['one_level_solve']}", flush=True)
    save()
    ΠSd = [np.asfortranarray(B) for B in setup.blocks(api.nn_pinv(ctx, setup.n_Γd, Sd))]
    C = api.NeumannNeumannInducedPreconditioner(ctx, ig, (pos_I, pos_Γ), gather, np.ones(pos_Γ.size, dtype=np.int64), ΠSd, setup,
                                                coupling="assembled")
    zc = torch.empty_like(r)
    doc["composed_apply"] = timed(ctx, api, lambda: C.apply(r, zc), args.repeats)
    M.apply(r, z)
    ctx.synchronize()
    doc["composed_vs_operator_rel_diff"] = float((z - zc).norm() / z.norm())
    a, c = doc["apply"], doc["composed_apply"]
    doc["apply_over_composed"] = round(a["mean_ms"] / c["mean_ms"], 4)
    doc["below_composed_by_more_than_the_spread"] = bool(c["mean_ms"] - a["mean_ms"] > a["spread"] * a["mean_ms"] + c["spread"] * c["mean_ms"])
    print(json.dumps(doc, indent=1))
    save()


if __name__ == "__main__":
    main()
