#!/usr/bin/env python3
"""Measures the quantizer at Example20's size: d = 170 coordinates, ns = 100 000 draws.

  - `mi_vq_assign` (device pointers, assignments and distances written) at P in {10, 100, 1 000, 10 000}, and the same at
    ns = 1 (the shape of find_precond): mean over `--repeats` calls between two HIP events after three warm-up calls, with
    (max - min) / mean beside it, and the 3 d ns P fp64 operations of the distance per second;
  - that rate beside the fp64 vector rate a plain loop of independent subtract / multiply / add chains reaches in the same run
    (tools/probes/fp64_rate.hip, built like the library): the code's own ceiling, not a data-sheet number;
  - one full `kmeans` at P = 1 000 from the first P draws as centres (tol = 1e-8, maxiter = 1 000): iterations, seconds;
  - the k-means++ seeding at P = 100;
  - fem.vq_assign and fem.kmeans on the host of the same machine, for the sizes that finish in a minute.
Every step runs in a child process of its own under `timeout`; a step that fails or runs out of time ends the probe.

    python tools/vq_probe.py --out profiles/vq_probe.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

D, NS = 170, 100_000
WARMUP = 3
RATE_SRC = os.path.join(ROOT, "tools", "probes", "fp64_rate.hip")
RATE_BIN = os.path.join(ROOT, "tools", "probes", "fp64_rate")


def draws(ns):
    return np.random.default_rng(987654321).standard_normal((D, ns))


def step_assign(args, ns):
    import torch
    pkg = graft.load_package()
    api = pkg.api
    ctx = api.Context(0)
    X = torch.from_numpy(np.ascontiguousarray(draws(max(ns, 10_000)).T)).cuda()
    out = {}
    for P in (10, 100, 1000, 10000):
        Xs, Cn = X[:ns].t(), X[:P].t()
        for _ in range(WARMUP):
            api.vq_assign(ctx, Xs, Cn, want_objv=False)
        ctx.synchronize()
        ms = []
        for _ in range(args.repeats):
            e0 = api.Event(ctx).record()
            api.vq_assign(ctx, Xs, Cn, want_objv=False)
            e1 = api.Event(ctx).record()
            ctx.synchronize()
            ms.append(e0.elapsed_ms(e1))
        mean = float(np.mean(ms))
        out[f"P={P}"] = {"mean_ms": round(mean, 4), "spread": round((max(ms) - min(ms)) / mean, 4), "repeats": len(ms),
                         "cent_splits": api.vq_tiling(D, ns, P)[3], "fp64_ops": 3 * D * ns * P,
                         "fp64_ops_per_s": float(f"{3 * D * ns * P / (mean * 1e-3):.4e}")}
    return out


def step_kmeans(args):
    pkg = graft.load_package()
    api = pkg.api
    ctx = api.Context(0)
    X = np.asfortranarray(draws(NS))
    t = time.perf_counter()
    res = api.kmeans(ctx, X, 1000, init=np.arange(1000), tol=1e-8, maxiter=1000)
    dt = time.perf_counter() - t
    return {"P": 1000, "iterations": res.iterations, "converged": res.converged, "seconds_with_host_copies": round(dt, 3),
            "ms_per_iteration": round(1e3 * dt / max(res.iterations, 1), 3), "totalcost": res.totalcost, "empty_clusters": int(np.sum(res.counts == 0))}


def step_seed(args):
    pkg = graft.load_package()
    api = pkg.api
    ctx = api.Context(0)
    X = np.asfortranarray(draws(NS))
    u = np.random.default_rng(1).random(100)
    t = time.perf_counter()
    picked, _ = api.kmpp_seed(ctx, X, 100, u)
    dt = time.perf_counter() - t
    return {"P": 100, "seconds_with_host_copies": round(dt, 3), "ms_per_centre": round(1e3 * dt / 100, 3), "distinct": int(len(set(picked.tolist())))}


def step_host(args):
    fem = graft.load_package().fem
    X = draws(NS)
    out = {}
    for P in (10, 100):
        t = time.perf_counter()
        fem.vq_assign(X, X[:, :P])
        dt = time.perf_counter() - t
        out[f"vq_assign ns={NS} P={P}"] = {"seconds": round(dt, 3), "fp64_ops_per_s": float(f"{3 * D * NS * P / dt:.4e}")}
    t = time.perf_counter()
    r = fem.kmeans(X[:, :10_000], X[:, :10], maxiter=5)
    out["kmeans ns=10000 P=10 maxiter=5"] = {"seconds": round(time.perf_counter() - t, 3), "iterations": r.iterations}
    return out


STEPS = {"assign": (lambda a: step_assign(a, NS), 240), "assign_ns1": (lambda a: step_assign(a, 1), 120), "kmeans": (step_kmeans, 400),
         "seed": (step_seed, 200), "host": (step_host, 200)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vq_probe.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step", default=None, help="internal: run one step and print its JSON")
    args = ap.parse_args()
    if args.step:
        print("VQ_PROBE_JSON " + json.dumps(STEPS[args.step][0](args)))
        return 0
    doc = {"d": D, "ns": NS, "tiling (point_tile, cent_tile, k_chunk, cent_splits, sum_chunk) at P = 10000": graft.load_package().api.vq_tiling(D, NS, 10000)}
    if not os.path.exists(RATE_BIN):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-o", RATE_BIN, RATE_SRC])
    r = subprocess.run(["timeout", "-k", "10", "60", RATE_BIN], capture_output=True, text=True)
    if r.returncode != 0:
        print(f"fp64_rate ended with status {r.returncode}: {r.stderr}", file=sys.stderr)
        return 1
    doc["plain_loop"] = json.loads(r.stdout.strip().splitlines()[-1])
    for name, (_, limit) in STEPS.items():
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, "--repeats", str(args.repeats)],
                           capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("VQ_PROBE_JSON ")]
        if r.returncode != 0 or not lines:
            print(f"step {name} ended with status {r.returncode}; nothing more is started\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", file=sys.stderr)
            doc[name] = {"failed": r.returncode}
            break
        doc[name] = json.loads(lines[-1][len("VQ_PROBE_JSON "):])
        print(name, json.dumps(doc[name]), flush=True)
    ceiling = doc["plain_loop"]["fp64_ops_per_s_mean"]
    for key in ("assign", "assign_ns1"):
        for v in doc.get(key, {}).values():
            if isinstance(v, dict) and "fp64_ops_per_s" in v:
                v["of_plain_loop"] = round(v["fp64_ops_per_s"] / ceiling, 4)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))
    return 1 if any(isinstance(v, dict) and "failed" in v for v in doc.values()) else 0


if __name__ == "__main__":
    sys.exit(main())
