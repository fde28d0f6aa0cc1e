#!/usr/bin/env python3
"""Measures the full-system assembly on the device at N = 500 and N = 1000, in one process run:

  (a) `k_assemble_full` through `mi_full_assembly_run` (row-owned plan);
  (b) `k_elem_coeff` + `k_assemble_plan` on `plan.as_block_plan()` through `mi_assembly_run`: the generic plan, same numbers;
  (c) a plain device copy of (a)'s algorithmic bytes (index arrays, cells, points, ue, be and a read once; values and b written);
  (d) `fem.do_isotropic_elliptic_assembly` on the host;
  (e) the device bytes each plan keeps;
  (f) the `--device-assembly` realization of Example06 step by step: ξ -> coefficient -> assembly -> A_op.set_values ->
      Π_amg_t.set_values -> pcg, everything as device tensors (wall clock around a synchronised step).
Device times of (a)-(c) are the mean over `--repeats` windows of `--launches` calls between two HIP events on the context's
stream (device pointers: a call only enqueues), with (max - min) / mean beside it. (a) and (b) are also compared bit for bit.

    python tools/full_assembly_probe.py --out profiles/full_assembly_probe.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

WARMUP = 3


def stats(ms, launches):
    us = [1e3 * t / launches for t in ms]
    mean = float(np.mean(us))
    return {"mean_us": round(mean, 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "spread": round((max(us) - min(us)) / mean, 4),
            "repeats": len(us), "launches_per_window": launches}


def windows(ctx, api, fn, repeats, launches):
    for _ in range(WARMUP):
        fn()
    ctx.synchronize()
    ms = []
    for _ in range(repeats):
        e0 = api.Event(ctx).record()
        for _ in range(launches):
            fn()
        e1 = api.Event(ctx).record()
        ctx.synchronize()
        ms.append(e0.elapsed_ms(e1))
    return ms


def measure(N, args, pkg, ctx, torch):
    fem, api, L = pkg.fem, pkg.api, pkg._lib.load()
    vp = C.c_void_p
    f, uexact = (lambda x, y: -1.0 + 0 * x), (lambda x, y: 0.734 + 0 * x)                 # Example06:68-74
    mesh = fem.get_mesh(N)
    dinds = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
    kl = fem.synthetic_kl(mesh.points)
    a = np.exp(fem.draw(kl, np.random.default_rng(481456))[1])
    doc = dict(N=N, n_node=int(mesh.points.shape[1]), nel=int(mesh.cells.shape[1]))
    # ---- (d) the host assembly
    ts = []
    for _ in range(args.host_repeats):
        t = time.perf_counter()
        A, b = fem.do_isotropic_elliptic_assembly(mesh.cells, mesh.points, dinds, mesh.point_marker, a, f, uexact)
        ts.append(time.perf_counter() - t)
    doc.update(n=int(A.shape[0]), nnz=int(A.nnz))
    doc["d_host_assembly_s"] = dict(mean=round(float(np.mean(ts)), 3), min=round(min(ts), 3), repeats=len(ts))
    print(f"N = {N}: n = {A.shape[0]}, nnz = {A.nnz}; (d) host assembly {doc['d_host_assembly_s']}", flush=True)
    # ---- the plans
    t = time.perf_counter()
    plan = fem.make_full_assembly_plan(mesh.cells, mesh.points, dinds, mesh.point_marker, f, uexact)
    t1 = time.perf_counter()
    block = plan.as_block_plan()
    t2 = time.perf_counter()
    dev, gen = api.FullAssemblyPlan(ctx, plan), api.AssemblyPlan(ctx, block)
    doc["plan_setup_s"] = dict(make_full_assembly_plan=round(t1 - t, 2), as_block_plan=round(t2 - t1, 2), device_create_both=round(time.perf_counter() - t2, 2))
    st = dev.stats()
    nel, ncontrib = block.cells.shape[1], int(block.ccode.size)
    generic_bytes = 4 * 3 * nel + 4 * ncontrib + 8 * (block.n_entries + 1) + 8 * (9 + 1 + 3 + 3 + 1) * nel
    doc["e_bytes_kept"] = dict(row_owned=st["bytes_kept"], generic=int(generic_bytes), ratio_generic_over_row_owned=round(generic_bytes / st["bytes_kept"], 2),
                               incidences=st["incidences"], contributions=ncontrib, row_blocks=st["row_blocks"])
    print("(e) bytes kept:", doc["e_bytes_kept"], flush=True)
    a_t = torch.from_numpy(a).cuda()
    vals, rhs = torch.empty(plan.nnz, dtype=torch.float64, device="cuda"), torch.empty(plan.n, dtype=torch.float64, device="cuda")
    out = torch.empty(block.n_entries, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def run_a():
        rc = L.mi_full_assembly_run(dev._h, vp(a_t.data_ptr()), vp(vals.data_ptr()), vp(rhs.data_ptr()))
        assert rc == 0, L.mi_last_error()

    def run_b():
        rc = L.mi_assembly_run(gen._h, vp(a_t.data_ptr()), vp(out.data_ptr()))
        assert rc == 0, L.mi_last_error()
    L.mi_ctx_set_pointer_mode(ctx._h, 1)
    # interleaved, so that neither side owns the warmer half of the run
    ms_a, ms_b = [], []
    for _ in range(2):
        ms_a += windows(ctx, api, run_a, args.repeats, args.launches)
        ms_b += windows(ctx, api, run_b, args.repeats, args.launches)
    L.mi_ctx_set_pointer_mode(ctx._h, 0)
    doc["a_k_assemble_full"], doc["b_k_assemble_plan"] = stats(ms_a, args.launches), stats(ms_b, args.launches)
    va, ba, ob = vals.cpu().numpy(), rhs.cpu().numpy(), out.cpu().numpy()

    def same(u, v):
        return bool(np.array_equal(u, v) and np.array_equal(np.signbit(u), np.signbit(v)))
    doc["bits"] = dict(a_equals_host=same(va, A.data) and same(ba, b), b_equals_host=same(ob[:plan.nnz], A.data) and same(ob[plan.nnz:], b))
    doc["a_faster_than_b_beyond_spread"] = bool(doc["a_k_assemble_full"]["max_us"] < doc["b_k_assemble_plan"]["min_us"])
    doc["b_over_a"] = round(doc["b_k_assemble_plan"]["mean_us"] / doc["a_k_assemble_full"]["mean_us"], 2)
    print("(a)", doc["a_k_assemble_full"], "\n(b)", doc["b_k_assemble_plan"], "\nbits", doc["bits"], "b/a", doc["b_over_a"], flush=True)
    # ---- (c) a plain copy of (a)'s algorithmic bytes
    algo = st["bytes_kept"] + 8 * plan.n_node + 8 * (plan.nnz + plan.n)
    src = torch.empty(algo // 16, dtype=torch.float64, device="cuda").normal_()
    dst = torch.empty_like(src)
    for _ in range(WARMUP):
        dst.copy_(src)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    doc["c_device_copy_of_a_bytes"] = dict(stats(ms, args.launches), bytes=int(algo))
    doc["a_over_copy"] = round(doc["a_k_assemble_full"]["mean_us"] / doc["c_device_copy_of_a_bytes"]["mean_us"], 2)
    print("(c)", doc["c_device_copy_of_a_bytes"], "a / copy", doc["a_over_copy"], flush=True)
    del src, dst, out
    gen.close()
    # ---- (f) the realization of Example06 --device-assembly, step by step
    t = time.perf_counter()
    A_0, _ = dev.plan.system(*dev.run(np.ones(plan.n_node)))
    Π = api.AMGPreconditioner(ctx, A_0, device_setup=True)
    doc["f_amg_plan_s"] = round(time.perf_counter() - t, 2)
    print(f"(f) aggregation on A_0 and plan: {doc['f_amg_plan_s']} s", flush=True)
    field = api.KLField(ctx, kl.Λ, kl.Ψ)
    A_op = api.SparseMatrixCSC(ctx, A_0)
    rng = np.random.default_rng(1)
    steps = []
    for _ in range(args.nreals + 1):                                    # the first one warms up (graph capture) and is dropped
        ξ = torch.from_numpy(rng.standard_normal(kl.Λ.size)).cuda()
        x0 = torch.zeros(plan.n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize(); ctx.synchronize()
        row, t = {}, time.perf_counter()

        def lap(name):
            nonlocal t
            ctx.synchronize(); torch.cuda.synchronize()
            now = time.perf_counter()
            row[name] = round(1e3 * (now - t), 3)
            t = now
        a_r = field.coefficient(ξ); lap("coefficient_ms")
        values, b_r = dev.run(a_r); lap("assembly_ms")
        A_op.set_values(values); lap("A_set_values_ms")
        Π.set_values(values); lap("amg_set_values_ms")
        _, it, _ = api.pcg(A_op, b_r, x0, Π); lap("pcg_ms")
        row["it"] = int(it)
        row["total_ms"] = round(sum(v for k, v in row.items() if k.endswith("_ms")), 3)
        steps.append(row)
    doc["f_example06_realization"] = dict(first_dropped=steps[0], realizations=steps[1:],
                                          mean_ms={k: round(float(np.mean([s[k] for s in steps[1:]])), 3) for k in steps[0] if k.endswith("_ms")})
    print("(f)", doc["f_example06_realization"]["mean_ms"], flush=True)
    for h in (A_op, Π, field, dev):
        h.close()
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[500, 1000])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--nreals", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    pkg = graft.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("full_assembly_probe measures on the device: no GPU is visible")
    ctx = pkg.api.Context(0)
    doc = dict(method="HIP events around windows of launches on the context's stream; (a) and (b) interleaved, 2 x repeats windows each",
               fa_rows=pkg.fem.FA_ROWS, fa_seg=pkg.fem.FA_SEG, sizes=[])
    for N in args.N:
        doc["sizes"].append(measure(N, args, pkg, ctx, torch))
        if args.out:                                                    # after every size: a run cut short keeps what it has
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fp:
                json.dump(doc, fp, indent=1, ensure_ascii=False)
                fp.write("\n")
    print(json.dumps(doc, ensure_ascii=False))


if __name__ == "__main__":
    main()
