#!/usr/bin/env python3
"""Measures the realization sampler at config 3's size: N = 1000 (10^6 nodes), fem.synthetic_kl's 64 modes.

  - the dense launch `mi_kl_field_set` at nreal = 1 and nreal = real_block, field and coefficient written;
  - the factored launches at the same nreal: 20 subdomains (5 x 4 boxes), 25 local modes each, random orthonormal factors
    (no eigensolve: the bytes and the access pattern are those of a real decomposition, the numbers are not);
  - the coordinates launch `mi_kl_field_coords` (SpMV with the mass matrix, column sums, reduction);
  - the host path they replace: fem.draw, np.exp, upload of the coefficient;
  - a plain device copy of Ψ's size in the same run, beside the copy ceiling recorded in profiles/NOTES.md.
Every device time is the mean over `--repeats` windows of `--launches` calls between two HIP events on the context's stream
(device pointers: a call only enqueues), with (max - min) / mean beside it; rates are the bytes `mi_kl_field_stats` counts
for a set (plus the extra outputs) over that time.

    python tools/kl_field_probe.py --out profiles/kl_field_probe.json
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
COPY_CEILING_TBS = 6.3          # profiles/NOTES.md: the measured copy ceiling of this device
PEAK_TBS = 8.0


def stats(ms, launches):
    us = [1e3 * t / launches for t in ms]
    mean = float(np.mean(us))
    return {"mean_us": round(mean, 2), "spread": round((max(us) - min(us)) / mean, 4), "repeats": len(us), "launches_per_window": launches}


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


def rate(doc, nbytes):
    tbs = nbytes / (doc["mean_us"] * 1e-6) / 1e12
    doc.update(bytes=int(nbytes), TB_per_s=round(tbs, 3), of_peak=round(tbs / PEAK_TBS, 3), of_copy_ceiling=round(tbs / COPY_CEILING_TBS, 3))
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1000)
    ap.add_argument("--px", type=int, default=5)
    ap.add_argument("--py", type=int, default=4)
    ap.add_argument("--md", type=int, default=25)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    pkg = graft.load_package()
    fem, api, L = pkg.fem, pkg.api, pkg._lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("kl_field_probe measures on the device: no GPU is visible")
    ctx = api.Context(0)
    vp, i64 = C.c_void_p, C.c_int64
    mesh = fem.get_mesh(args.N)
    n = mesh.points.shape[1]
    kl = fem.synthetic_kl(mesh.points)
    m = kl.Λ.size
    rt, mc, rb, splits = api.kl_field_tiling(n, m, 1)
    doc = dict(config=f"N={args.N} unit square, fem.synthetic_kl", n=n, m=m, row_tile=rt, mode_chunk=mc, real_block=rb, coord_splits=splits,
               copy_ceiling_TB_per_s=COPY_CEILING_TBS, peak_TB_per_s=PEAK_TBS)
    print(f"n = {n}, m = {m}, tiling {rt} x {mc} x {rb}, coordinate splits {splits}", flush=True)
    rng = np.random.default_rng(0)

    # ---- host path: fem.draw, np.exp, upload
    ts = []
    for k in range(3):
        t = time.perf_counter()
        ξ, g = fem.draw(kl, np.random.default_rng(k))
        t1 = time.perf_counter()
        a = np.exp(g)
        t2 = time.perf_counter()
        a_t = torch.from_numpy(a).cuda()
        torch.cuda.synchronize()
        ts.append((t1 - t, t2 - t1, time.perf_counter() - t2))
    doc["host_path_ms"] = dict(draw=round(1e3 * float(np.mean([t[0] for t in ts])), 2), exp=round(1e3 * float(np.mean([t[1] for t in ts])), 2),
                               upload=round(1e3 * float(np.mean([t[2] for t in ts])), 3), total=round(1e3 * float(np.mean([sum(t) for t in ts])), 2), repeats=3)
    print("host path (ms):", doc["host_path_ms"], flush=True)

    def set_fn(field, nreal):
        Ξ = torch.from_numpy(rng.standard_normal((nreal, m))).cuda()
        G = torch.empty((nreal, n), dtype=torch.float64, device="cuda")
        A = torch.empty_like(G)
        torch.cuda.synchronize()

        def go():
            rc = L.mi_kl_field_set(field._h, i64(nreal), vp(Ξ.data_ptr()), i64(m), vp(G.data_ptr()), i64(n), vp(A.data_ptr()), i64(n))
            assert rc == 0, L.mi_last_error()
        return go, (Ξ, G, A)

    def measure_sets(field, name, per_real=0):
        """`per_real`: bytes of intermediates every further realization of a pass writes and reads"""
        st = field.stats()
        doc[name] = dict(bytes_kept=st["bytes_kept"], bytes_per_set=st["bytes_per_set"])
        for nreal in (1, rb):
            go, keep = set_fn(field, nreal)
            L.mi_ctx_set_pointer_mode(ctx._h, 1)
            ms = windows(ctx, api, go, args.repeats, args.launches)
            L.mi_ctx_set_pointer_mode(ctx._h, 0)
            # one pass over the kept factors; per realization ξ in and two outputs (bytes_per_set counts one output of one realization)
            nbytes = st["bytes_per_set"] + 8 * n + (nreal - 1) * (16 * n + 8 * m + per_real)
            doc[name][f"nreal_{nreal}"] = rate(stats(ms, args.launches), nbytes)
            doc[name][f"nreal_{nreal}"]["us_per_realization"] = round(doc[name][f"nreal_{nreal}"]["mean_us"] / nreal, 2)
            print(f"{name} nreal = {nreal}:", doc[name][f"nreal_{nreal}"], flush=True)
            del keep

    # ---- dense form
    dense = api.KLField(ctx, kl.Λ, kl.Ψ)
    measure_sets(dense, "dense")
    # the same bits as the host loop, at this size
    ξ, g = fem.draw(kl, np.random.default_rng(7))
    doc["dense"]["bit_equal_to_fem_draw"] = bool(np.array_equal(dense.set(ξ), g))
    # a plain copy of Ψ's bytes (read + write)
    src = torch.empty(n * m, dtype=torch.float64, device="cuda").normal_()
    dst = torch.empty_like(src)
    for _ in range(WARMUP):
        dst.copy_(src)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.repeats):                                  # torch's own stream and events: the copy is torch's kernel
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    doc["device_copy_of_psi_bytes"] = rate(stats(ms, 20), 16 * n * m)
    print("device copy:", doc["device_copy_of_psi_bytes"], flush=True)
    del src, dst

    # ---- coordinates
    M = fem.get_mass_matrix(mesh.cells, mesh.points)
    Mop = api.SparseMatrixCSC(ctx, M)
    g_t, ξ_t = torch.from_numpy(g).cuda(), torch.empty(m, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def coords():
        rc = L.mi_kl_field_coords(dense._h, Mop._h, vp(g_t.data_ptr()), vp(ξ_t.data_ptr()))
        assert rc == 0, L.mi_last_error()
    L.mi_ctx_set_pointer_mode(ctx._h, 1)
    ms = windows(ctx, api, coords, args.repeats, args.launches)
    L.mi_ctx_set_pointer_mode(ctx._h, 0)
    cb = -(-m // rb)
    doc["coords"] = rate(stats(ms, args.launches), 8 * n * m + 8 * n * cb + Mop.bytes()[0] + 16 * splits * m)
    doc["coords"]["note"] = "SpMV with the mass matrix, column sums (Ψ once, M g once per column block), reduction"
    print("coords:", doc["coords"], flush=True)
    Mop.close(); dense.close()
    del g_t, ξ_t

    # ---- factored form: 20 subdomains, 25 local modes, random orthonormal factors
    epart, _ = fem.mesh_partition(mesh, args.px, args.py)
    ndom = args.px * args.py
    l2gd = [fem.kl_set_subdomain(mesh.cells, mesh.points, epart, d)[0] for d in range(ndom)]
    Φd = [np.linalg.qr(rng.standard_normal((l.size, args.md)))[0] for l in l2gd]
    Φ = np.linalg.qr(rng.standard_normal((ndom * args.md, m)))[0]
    dd = api.KLField.from_dd(ctx, n, kl.Λ, Φ, Φd, l2gd)
    doc["factored_config"] = dict(ndom=ndom, md=args.md, nloc=int(sum(l.size for l in l2gd)), nred=ndom * args.md)
    nloc, nred = int(sum(l.size for l in l2gd)), ndom * args.md
    measure_sets(dd, "factored", per_real=16 * (nloc + nred))          # y and t, written and read
    doc["factored"]["note"] = "nreal_8 bytes include y and t of every realization (16 B per reduced and local row each)"
    doc["factored"]["kept_bytes_ratio_dense_over_factored"] = round(doc["dense"]["bytes_kept"] / doc["factored"]["bytes_kept"], 2)
    dd.close()
    if args.out:
        with open(args.out, "w") as fp:
            json.dump(doc, fp, indent=1, ensure_ascii=False)
            fp.write("\n")
    print(json.dumps(doc, ensure_ascii=False))


if __name__ == "__main__":
    main()
