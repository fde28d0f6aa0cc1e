#!/usr/bin/env python3
"""Measures the device AMG bank (`api.AMGBank`) against separate `AMGPreconditioner(ctx, A0, device_setup=True)`
objects in one run, at N = 317 (99 225 rows) with 64 members. Every figure is the median of `--repeats` samples after 2
warm-ups, with (max - min) / median beside it:

  - bytes_shared, bytes_per_member, what 10 000 members would take, and `bytes_kept` of one separate operator;
  - `set_values` per member (device tensor, HIP events), bank and separate operator;
  - creation: the bank (plan + slab), against creating 64 separate operators (plan + first numeric phase each, all 64 alive
    at the end of a sample), and one separate operator alone;
  - one cycle of a k = 1 view against the separate operator's cycle (samples of `--applies` applies between two events);
  - a k = 4 view against `InterpolatingPreconditioner` of four separate operators;
  - `pcg(A, b, 0, M)` with each of the four (device tensors, events around the solve).

Four lognormal matrices (seeds 481456 ...) are assembled on the host; member p holds matrix p mod 4 (the set-up's time does
not depend on the values).

    python tools/amg_bank_probe.py --out profiles/amg_bank_probe.json
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
    med = float(np.median(samples))
    return dict(median=round(med, digits), spread=round((max(samples) - min(samples)) / med, 4), samples=len(samples))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=317)
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--applies", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    pkg = graft.load_package()
    fem, api = pkg.fem, pkg.api
    mesh = fem.get_mesh(args.N)
    d = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
    f, u = (lambda x, y: -1.0 + 0 * x), (lambda x, y: 3.0 + 0 * x)
    kl = fem.synthetic_kl(mesh.points)
    mats, bs = [], []
    for s in range(4):
        g = fem.draw(kl, np.random.default_rng(481456 + s))[1]
        A, b = fem.do_isotropic_elliptic_assembly(mesh.cells, mesh.points, d, mesh.point_marker, np.exp(g), f, u)
        A = sp.csr_matrix(A)
        A.sum_duplicates(); A.sort_indices()
        mats.append(A); bs.append(b)
    n, P, R = bs[0].size, args.members, WARMUP + args.repeats
    aggs = fem.prepare_amg_precond(mats[0]).agg
    ctx = api.Context(0)
    doc = dict(config=f"N={args.N} full matrix, lognormal members (synthetic KL, seeds 481456 + p mod 4), {P} members", n=n, nnz=int(mats[0].nnz),
               repeats=args.repeats, warmup=WARMUP)

    def timed(fn, reps=1):
        out = []
        for k in range(R):
            e0 = api.Event(ctx).record()
            for _ in range(reps):
                fn()
            e1 = api.Event(ctx).record()
            ctx.synchronize()
            if k >= WARMUP:
                out.append(e0.elapsed_ms(e1) / reps)
        return stat(out)

    def wall(fn, after=lambda r: None):
        out = []
        for k in range(R):
            t0 = time.perf_counter()
            r = fn()
            ctx.synchronize()
            t = time.perf_counter() - t0
            after(r)
            if k >= WARMUP:
                out.append(1e3 * t)
        return stat(out)

    # creation
    doc["create_bank_ms"] = wall(lambda: api.AMGBank(ctx, mats[0], P, aggregates=aggs), lambda b: b.close())
    one = wall(lambda: api.AMGPreconditioner(ctx, mats[0], device_setup=True, aggregates=aggs), lambda m: m.close())
    doc["create_one_separate_operator_ms"] = one
    many = lambda: [api.AMGPreconditioner(ctx, mats[0], device_setup=True, aggregates=aggs) for _ in range(P)]
    doc["create_separate_operators_ms"] = wall(many, lambda ms: [m.close() for m in ms])
    doc["create_separate_over_bank"] = round(doc["create_separate_operators_ms"]["median"] / doc["create_bank_ms"]["median"], 1)
    print(json.dumps({k: v for k, v in doc.items() if k.startswith("create")}), flush=True)
    bank = api.AMGBank(ctx, mats[0], P, aggregates=aggs)
    ops = [api.AMGPreconditioner(ctx, mats[0], device_setup=True, aggregates=aggs) for _ in range(4)]
    st, so = bank.stats(), ops[0].stats()
    doc["levels"] = bank.n_levels
    doc["bytes"] = dict(shared=st["bytes_shared"], per_member=st["bytes_per_member"], members_10000=st["bytes_shared"] + 10000 * st["bytes_per_member"],
                        separate_operator_kept=so["bytes_kept"], separate_operators_10000=10000 * so["bytes_kept"])
    print(json.dumps(doc["bytes"]), flush=True)
    # set_values
    vals = [torch.from_numpy(np.ascontiguousarray(A.data)).cuda() for A in mats]
    torch.cuda.synchronize()
    for p in range(P):
        bank.set_values(p, vals[p % 4])
    for p in range(4):
        ops[p].set_values(vals[p])
    doc["set_values_member_ms"] = timed(lambda: bank.set_values(5, vals[1]))
    doc["set_values_separate_ms"] = timed(lambda: ops[1].set_values(vals[1]))
    # cycles
    r = torch.from_numpy(np.random.default_rng(1).standard_normal(n)).cuda()
    z = torch.empty_like(r)
    v1, v4 = bank.view(1), bank.view(4)
    v1.select(1)
    coef = np.array([0.4, 0.3, 0.2, 0.1])
    v4.combine([0, 1, 2, 3], coef)
    Pi = api.InterpolatingPreconditioner(ctx, coef, ops)
    assert torch.equal(v1.apply(r), ops[1].apply(r)) and torch.equal(v4.apply(r), Pi.apply(r))
    for name, M in (("separate_operator", ops[1]), ("view_k1", v1), ("interpolating_4_separate", Pi), ("view_k4", v4)):
        doc[f"cycle_{name}_ms"] = timed(lambda: M.apply(r, out=z), args.applies)
    doc["cycle_view_k1_over_separate"] = round(doc["cycle_view_k1_ms"]["median"] / doc["cycle_separate_operator_ms"]["median"], 3)
    doc["cycle_view_k4_over_interpolating"] = round(doc["cycle_view_k4_ms"]["median"] / doc["cycle_interpolating_4_separate_ms"]["median"], 3)
    # solves
    Aop = api.SparseMatrixCSC(ctx, mats[1])
    b = torch.from_numpy(bs[1]).cuda()
    its = {}
    for name, M in (("separate_operator", ops[1]), ("view_k1", v1), ("interpolating_4_separate", Pi), ("view_k4", v4)):
        def solve():
            its[name] = int(api.pcg(Aop, b, torch.zeros_like(b), M)[1])
        doc[f"pcg_{name}_ms"] = timed(solve)
    doc["pcg_it"] = its
    print(json.dumps(doc, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(json.dumps(doc, indent=1) + "\n")
    Pi.close(); Aop.close()
    for m in ops:
        m.close()
    bank.close()
    ctx.close()


if __name__ == "__main__":
    main()
