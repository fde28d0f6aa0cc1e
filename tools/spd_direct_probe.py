#!/usr/bin/env python3
"""Measures the sparse direct preconditioner (`api.SparseDirectPreconditioner`, `M \\ r` with M = A_ΓΓ, Example07:412/416)
at config 3 (N = 1000, 4x2 boxes, lognormal a = exp(g), seed 481456) for piece sizes P = 32, 64, 128:
  - µs of the dominant launch (mi_op_time_dominant: graph replay) and of a whole apply (HIP events around eager applies);
  - µs per iteration and iteration count of pcg(S, b_schur, 0, A_ΓΓ_t) and pcg(S, b_schur, 0, A_ΓΓ_0) (and of the
    Neumann-Neumann pcg beside it);
  - numeric set-up ms (set_values, host values; synchronous), pieces, |Σ|, bytes per apply.
Prints one JSON document and writes it to --out.

    python tools/spd_direct_probe.py [--N 1000 --px 4 --py 2 --out profiles/spd_direct_probe.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1000)
    ap.add_argument("--px", type=int, default=4)
    ap.add_argument("--py", type=int, default=2)
    ap.add_argument("--seed", type=int, default=481456)
    ap.add_argument("--pieces", default="32,64,128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    pkg = graft.load_package()
    fem, api = pkg.fem, pkg.api
    f = lambda x, y: -1.0 + 0 * x          # noqa: E731
    uex = lambda x, y: 0.734 + 0 * x       # noqa: E731
    ctx = api.Context(0)
    mesh = fem.get_mesh(args.N)
    _, g = fem.draw(fem.synthetic_kl(mesh.points), np.random.default_rng(args.seed))
    a = np.exp(g)
    t0 = time.perf_counter()
    P = fem.build_schur_problem(args.N, args.px, args.py, a, f, uex, mesh=mesh, dense_setup=api.device_dense_setup(ctx))
    t_build = time.perf_counter() - t0
    sub = P.sub
    n = sub.n_Γ
    gg = {}
    for tag, coeff in (("t", a), ("0", np.ones_like(a))):
        A = sp.csc_matrix(fem.prepare_global_schur(mesh.cells, mesh.points, P.epart, sub, coeff, f, uex)[2])
        A.sort_indices()
        gg[tag] = A
    S = api.LocalSchurs(ctx, P.Sd, sub.gather_idx, sub.node_Γ_cnt)
    NN = api.NeumannNeumannSchurPreconditioner(ctx, P.ΠSd, sub.gather_idx, sub.node_Γ_cnt)
    b = torch.from_numpy(P.b_schur).cuda()
    x0 = torch.zeros(n, dtype=torch.float64, device="cuda")

    def time_pcg(M):
        api.pcg(S, b, x0.clone(), M)               # warm-up (graph capture); x is overwritten with the solution
        torch.cuda.synchronize()
        best, it = float("inf"), 0
        for _ in range(args.reps):
            x = x0.clone()
            ctx.synchronize()
            t = time.perf_counter()
            _, it, _ = api.pcg(S, b, x, M)
            ctx.synchronize()
            best = min(best, time.perf_counter() - t)
        return it, best * 1e6 / max(it, 1)

    it_nn, us_nn = time_pcg(NN)
    out = dict(config=f"N={args.N} {args.px}x{args.py} boxes, lognormal a=exp(g) seed {args.seed}", n_gamma=n,
               nnz_A_GG=int(gg["t"].nnz), host_build_s=round(t_build, 2),
               pcg_nn=dict(it=it_nn, us_per_it=round(us_nn, 2)), schur_bytes_per_apply=S.bytes()[0], by_piece_size={})
    r = torch.from_numpy(np.random.default_rng(0).standard_normal(n)).cuda()
    z = torch.empty_like(r)
    for Ps in [int(v) for v in args.pieces.split(",")]:
        os.environ["MI355_SPD_PIECE"] = str(Ps)
        t = time.perf_counter()
        M = api.SparseDirectPreconditioner(ctx, gg["t"])
        t_create = time.perf_counter() - t
        ts = []
        for _ in range(args.reps):
            t = time.perf_counter()
            M.set_values(gg["t"].data)
            ts.append(time.perf_counter() - t)
        dom = min(M.time_dominant(r, 200) for _ in range(3))
        for _ in range(10):
            M.apply(r, z)
        e0, e1 = api.Event(ctx), api.Event(ctx)
        e0.record()
        for _ in range(200):
            M.apply(r, z)
        e1.record()
        us_apply = e0.elapsed_ms(e1) * 1e3 / 200
        it_t, us_t = time_pcg(M)
        M0 = api.SparseDirectPreconditioner(ctx, gg["0"])
        it_0, us_0 = time_pcg(M0)
        pieces, sigma = M.stats
        ab, db = M.bytes()
        out["by_piece_size"][Ps] = dict(
            pieces=pieces, sigma=sigma, bytes_per_apply=ab, bytes_dominant=db,
            us_dominant_replayed=round(dom, 2), us_apply_eager=round(us_apply, 2),
            create_ms=round(t_create * 1e3, 2), numeric_setup_ms=round(min(ts) * 1e3, 3),
            pcg_A_GG_t=dict(it=it_t, us_per_it=round(us_t, 2)), pcg_A_GG_0=dict(it=it_0, us_per_it=round(us_0, 2)))
        print(json.dumps({Ps: out["by_piece_size"][Ps]}), flush=True)
        del M, M0
    os.environ.pop("MI355_SPD_PIECE", None)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
