#!/usr/bin/env python3
"""Measures the batched device PCG (`api.pcg_batch`) against the k separate solves it replaces, in one run, at
N = 317 (the bank probe's size) and N = 1000, for k = 1, 4, 8, 16. Every figure is the mean of `--repeats` samples after 2
warm-ups, with (max - min) / mean beside it.

Four lognormal matrices (seeds 481456 + p) are assembled on the host and make the four members of one `AMGBank`; system t of
a batch is matrix t mod 4 in slot t. Two mixes of members:

  own   : system t under member t mod 4, its own — every system stops after about the same number of iterations;
  stale : every system under member 0 — three of four systems need several times the iterations of the first.

Per (N, k, mix), wall time (host clock around the calls, device tensors in and out, the stream idle before and after):

  batch_ms    : one `pcg_batch` of the k systems;
  separate_ms : the k separate solves, the path without the batch: ONE `SparseMatrixCSC` operator refreshed in place
                (`set_values` of a device tensor, outside the timed region — in the flow the assembly writes there), then
                `view.select(m)` and `pcg(A, b, 0, view)`, both timed;
  ratio       : batch_ms / separate_ms (below 1: the batch is faster);
  it          : the iteration counts (the same in both), per-iteration times (batch: over the longest system; separate: over
                the sum), and the bytes a slot keeps.

    python tools/batch_probe.py --out profiles/batch_probe.json
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
MEMBERS = 4


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
    doc = dict(config="full matrix, lognormal members (synthetic KL, seeds 481456 + p), system t = matrix t mod 4; own: member t mod 4, stale: member 0",
               repeats=args.repeats, warmup=WARMUP, cases=[])
    f, u = (lambda x, y: -1.0 + 0 * x), (lambda x, y: 3.0 + 0 * x)
    for N in args.N:
        mesh = fem.get_mesh(N)
        d = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
        kl = fem.synthetic_kl(mesh.points)
        mats, bs = [], []
        for s in range(MEMBERS):
            g = fem.draw(kl, np.random.default_rng(481456 + s))[1]
            A, b = fem.do_isotropic_elliptic_assembly(mesh.cells, mesh.points, d, mesh.point_marker, np.exp(g), f, u)
            A = sp.csr_matrix(A)
            A.sum_duplicates(); A.sort_indices()
            mats.append(A); bs.append(b)
        n = bs[0].size
        aggs = fem.prepare_amg_precond(mats[0]).agg
        bank = api.AMGBank(ctx, mats[0], MEMBERS, aggregates=aggs)
        kmax = max(args.k)
        batch = api.CsrBatch(ctx, mats[0], kmax)
        vals = [torch.from_numpy(np.ascontiguousarray(A.data)).cuda() for A in mats]
        for p in range(MEMBERS):
            bank.set_values(p, vals[p])
        for t in range(kmax):
            batch.set_values(t, vals[t % MEMBERS])
        view, view1 = bank.view(kmax), bank.view(1)
        A_op = api.SparseMatrixCSC(ctx, mats[0])
        bcols = [torch.from_numpy(b).cuda() for b in bs]
        torch.cuda.synchronize()
        st = batch.stats()
        for k in args.k:
            for mix in ("own", "stale"):
                members = [t % MEMBERS if mix == "own" else 0 for t in range(k)]
                B = torch.stack([bcols[t % MEMBERS] for t in range(k)]).T          # (n, k), column-major
                X = torch.zeros((k, n), dtype=torch.float64, device="cuda").T
                xs = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(k)]
                t_batch, t_sep, t_refresh = [], [], []
                its_b = its_s = None
                for r in range(R):
                    X.zero_()
                    torch.cuda.synchronize(); ctx.synchronize()
                    t0 = time.perf_counter()
                    _, its_b, _ = api.pcg_batch(batch, list(range(k)), B, X, view, members)
                    ctx.synchronize()
                    tb = time.perf_counter() - t0
                    ts, tr, its_s = 0.0, 0.0, []
                    for t in range(k):
                        xs[t].zero_()
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        A_op.set_values(vals[t % MEMBERS])
                        ctx.synchronize()
                        tr += time.perf_counter() - t0
                        t0 = time.perf_counter()
                        view1.select(members[t])
                        its_s.append(int(api.pcg(A_op, bcols[t % MEMBERS], xs[t], view1)[1]))
                        ctx.synchronize()
                        ts += time.perf_counter() - t0
                    if r >= WARMUP:
                        t_batch.append(1e3 * tb); t_sep.append(1e3 * ts); t_refresh.append(1e3 * tr)
                assert [int(i) for i in its_b] == its_s, (its_b, its_s)
                same = all(torch.equal(X[:, t], xs[t]) for t in range(k))
                row = dict(N=N, n=n, k=k, mix=mix, batch_ms=stat(t_batch), separate_ms=stat(t_sep), csr_refresh_ms=stat(t_refresh),
                           it_min=min(its_s), it_max=max(its_s), it_sum=sum(its_s), bytes_per_slot=st["bytes_per_slot"],
                           x_equal_to_default_separate_solves=bool(same))
                row["ratio"] = round(row["batch_ms"]["mean"] / row["separate_ms"]["mean"], 3)
                row["batch_us_per_iteration"] = round(1e3 * row["batch_ms"]["mean"] / max(its_s), 2)
                row["separate_us_per_iteration"] = round(1e3 * row["separate_ms"]["mean"] / sum(its_s), 2)
                doc["cases"].append(row)
                print(json.dumps(row), flush=True)
        view.close(); view1.close(); A_op.close(); batch.close(); bank.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(json.dumps(doc, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
