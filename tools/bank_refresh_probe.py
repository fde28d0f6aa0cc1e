#!/usr/bin/env python3
"""Measures the batched bank refresh (`AMGBank.set_values_batch`) against the k `AMGBank.set_values` calls it
replaces, in one run, at N = 317 and N = 1000, for k = 1, 4, 8, 16. Every figure is the mean of `--repeats` samples after 2
warm-ups, with (max - min) / mean beside it.

The k matrices are those of k lognormal realizations (synthetic KL, ξ from the seeds 481456 + t), assembled on the device.
Per (N, k), wall time (host clock around the calls, the stream idle before and after; both refreshes are synchronous):

  batch_ms    : one `set_values_batch` of k members from k device-resident slots of a `CsrBatch`;
  single_ms   : k `set_values` calls on the same values as device tensors;
  ratio       : batch_ms / single_ms (below 1: the batched call is faster);
  step_batch_ms  : the whole per-batch step, k `update_batch` + `set_values_batch` + `pcg_batch` with every system under its
                   own member;
  step_single_ms : the same step on the path without the batched refresh: k x (`FullAssemblyPlan.run`, `CsrBatch.set_values`,
                   `AMGBank.set_values`) + the same `pcg_batch`;
  workspace_bytes : what the batched set-up adds to the bank's `bytes_shared` (k candidate slots and the per-term work);
  apply_equal : the last member's V-cycle on a random vector has the same bits in both banks.

    python tools/bank_refresh_probe.py --out profiles/bank_refresh_probe.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

WARMUP = 2


def stat(samples, digits=4):
    mean = float(np.mean(samples))
    return dict(mean=round(mean, digits), spread=round((max(samples) - min(samples)) / mean, 4), samples=len(samples))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[317, 1000])
    ap.add_argument("--k", type=int, nargs="+", default=[1, 4, 8, 16])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    pkg = graft.load_package()
    fem, api = pkg.fem, pkg.api
    ctx = api.Context(0)
    R = WARMUP + args.repeats
    doc = dict(config="full matrix, k lognormal realizations (synthetic KL, ξ from the seeds 481456 + t) assembled on the device, member t from slot t",
               repeats=args.repeats, warmup=WARMUP, cases=[])
    f, u = (lambda x, y: -1.0 + 0 * x), (lambda x, y: 3.0 + 0 * x)
    kmax = max(args.k)
    for N in args.N:
        mesh = fem.get_mesh(N)
        d = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
        host_plan = fem.make_full_assembly_plan(mesh.cells, mesh.points, d, mesh.point_marker, f, u)
        plan = api.FullAssemblyPlan(ctx, host_plan)
        kl = fem.synthetic_kl(mesh.points)
        field = api.KLField(ctx, kl.Λ, kl.Ψ)
        n = host_plan.n
        v0 = plan.run(np.ones(host_plan.n_node))[0]
        A_0 = sp.csr_matrix((np.asarray(v0), host_plan.colidx, host_plan.rowptr), shape=(n, n))
        aggs = fem.prepare_amg_precond(A_0).agg
        coeffs = [field.coefficient(torch.from_numpy(np.random.default_rng(481456 + t).standard_normal(kl.Λ.size)).cuda()) for t in range(kmax)]
        batch = api.CsrBatch(ctx, A_0, kmax)
        vals, bs = [], []
        for t in range(kmax):
            v, b = plan.run(coeffs[t])
            vals.append(v.clone()); bs.append(b.clone())
            plan.update_batch(coeffs[t], batch, t)
        X_bank, Y_bank = api.AMGBank(ctx, A_0, kmax, aggregates=aggs), api.AMGBank(ctx, A_0, kmax, aggregates=aggs)
        shared0 = X_bank.stats()["bytes_shared"]
        vx, vy = X_bank.view(kmax), Y_bank.view(kmax)
        v1x, v1y = X_bank.view(1), Y_bank.view(1)
        r = torch.from_numpy(np.random.default_rng(5).standard_normal(n)).cuda()
        torch.cuda.synchronize(); ctx.synchronize()
        for k in sorted(args.k):
            ks = list(range(k))
            B = torch.stack(bs[:k]).T
            X = torch.zeros((k, n), dtype=torch.float64, device="cuda").T
            t_b, t_s, s_b, s_s = [], [], [], []
            its_b = its_s = None
            for rep in range(R):
                torch.cuda.synchronize(); ctx.synchronize()
                t0 = time.perf_counter()
                X_bank.set_values_batch(ks, batch, ks)
                tb = time.perf_counter() - t0
                t0 = time.perf_counter()
                for t in ks:
                    Y_bank.set_values(t, vals[t])
                ts = time.perf_counter() - t0
                # the whole step, both ways
                X.zero_()
                torch.cuda.synchronize(); ctx.synchronize()
                t0 = time.perf_counter()
                for t in ks:
                    plan.update_batch(coeffs[t], batch, t)
                X_bank.set_values_batch(ks, batch, ks)
                _, its_b, _ = api.pcg_batch(batch, ks, B, X, vx, ks)
                ctx.synchronize()
                sb = time.perf_counter() - t0
                X.zero_()
                torch.cuda.synchronize(); ctx.synchronize()
                t0 = time.perf_counter()
                for t in ks:
                    v, _ = plan.run(coeffs[t])
                    batch.set_values(t, v)
                    Y_bank.set_values(t, v)
                _, its_s, _ = api.pcg_batch(batch, ks, B, X, vy, ks)
                ctx.synchronize()
                ss = time.perf_counter() - t0
                if rep >= WARMUP:
                    t_b.append(1e3 * tb); t_s.append(1e3 * ts); s_b.append(1e3 * sb); s_s.append(1e3 * ss)
            assert [int(i) for i in its_b] == [int(i) for i in its_s], (its_b, its_s)
            v1x.select(k - 1); v1y.select(k - 1)
            same = bool(torch.equal(v1x.apply(r), v1y.apply(r)))
            row = dict(N=N, n=n, k=k, batch_ms=stat(t_b), single_ms=stat(t_s), step_batch_ms=stat(s_b), step_single_ms=stat(s_s),
                       it=[int(i) for i in its_b], workspace_bytes=X_bank.stats()["bytes_shared"] - shared0,
                       bytes_per_member=X_bank.stats()["bytes_per_member"], apply_equal=same)
            row["ratio"] = round(row["batch_ms"]["mean"] / row["single_ms"]["mean"], 3)
            row["step_ratio"] = round(row["step_batch_ms"]["mean"] / row["step_single_ms"]["mean"], 3)
            doc["cases"].append(row)
            print(json.dumps(row), flush=True)
        X_bank.close(); Y_bank.close(); batch.close(); plan.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(json.dumps(doc, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
