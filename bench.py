#!/usr/bin/env python3
"""Headline benchmark: Neumann-Neumann Schur-PCG on the 1 M-DoF / 8-subdomain problem
(BASELINE.json configs[2] at N=1; configs[3] sharding at N>1).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

One "step" = one complete `pcg(S, b_schur, 0, ΠSnn)` solve (Example03:193) with the assembled
local Schur complements resident in HBM. `value` = PCG loop iterations per second over the whole
job (every iteration = one S-apply + one NN-apply + the BLAS-1 updates; `it` of the reference
counts from 1, so a solve that returns `it` ran it-1 iterations). Inputs (S_d, ΠS_d, b_schur) are on the
device before the timed region starts; the timed region is K solves bracketed by barrier + sync.

At N>1 the 8 subdomains are split across ranks (8/N each), Γ-vectors are replicated and the two
Γ-sums of every iteration are captured inside the iteration graph: the one-shot peer exchange (peer stores over
xGMI + flags, csrc/exchange.hpp) when every rank can map its peers' arenas, RCCL all-reduces otherwise (`--exchange`);
total work is fixed, so scaling is "strong".

A plain run sets up, warms up, times the K solves and prints the line; `roofline`, `cpu_baseline` and
`secondary` are null in it. `--full` adds them: `roofline` for the dominant kernel (batched dense GEMV of the
S-apply, HIP events on the library's stream), `cpu_baseline` (the C oracle, OpenMP over the host cores, also the
parity check of the run; rank 0 at N=1 only) and `secondary` (the other loops, config 2, set-up, config 5).

`--dump-outputs DIR` writes what the last timed solve returned (x, it, res_norm) as DIR/<name>.npy in float64.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: HBM3E peak 8.0 TB/s (spec)


def log(rank, *a):
    if rank == 0:
        print("[bench]", *a, file=sys.stderr, flush=True)


def kernel_us(api, ctx, op, x, reps):
    """Average duration of the operator's dominant kernel: HIP events on the library's stream around `reps`
    launches replayed from one graph (mi_op_time_dominant)."""
    return min(op.time_dominant(x, reps) for _ in range(3))


def profiled_kernel_us(csv_name, kernel):
    """Average duration (us) of `kernel` in a committed rocprofv3 kernel-stats summary (profiles/), or None."""
    try:
        import csv
        with open(os.path.join(ROOT, "profiles", csv_name)) as fh:
            for r in csv.DictReader(fh):
                if kernel in r["Name"]:
                    return float(r["AverageNs"]) / 1e3
    except Exception:
        pass
    return None


def spmv_traffic():
    """PMC HBM-side bytes per launch of the CSR SpMV at config 2, if a profile has been committed."""
    try:
        t = json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json")))
        return next((v["bytes_per_launch"] for k, v in t.items()
                     if isinstance(v, dict) and "k_spmv_csr<0, true>" in k and v["bytes_per_launch"] < 60e6), None)
    except Exception:
        return None


def bench_full_system(args):
    """configs[1]: 250k-DoF 2D elliptic (Example01 coefficients), 1 subdomain, `pcg(A, b, 0, M)` on the full
    matrix with M = Jacobi (AMG is out of scope). One step = one complete solve; CSR SpMV + BLAS-1 kernels only."""
    import torch
    torch.cuda.set_device(0)
    pkg = graft.load_package()
    fem, api = pkg.fem, pkg.api
    N = 500 if args.N == 1000 else args.N
    mesh = fem.get_mesh(N)
    d = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
    A, b = fem.do_isotropic_elliptic_assembly(mesh.cells, mesh.points, d, mesh.point_marker,
                                              lambda x, y: 0.1 + 0.0001 * x * y, lambda x, y: -1.0 + 0 * x,
                                              lambda x, y: 3.0 + 0 * x)
    n = b.size
    ctx = api.Context(0)
    Aop = api.SparseMatrixCSC(ctx, A)
    M = api.JacobiPreconditioner(ctx, A.diagonal())
    bd = torch.from_numpy(b).cuda()
    steps, warm = args.steps, args.warmup
    xs = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(steps + warm)]
    for w in range(warm):
        _, its, res = api.pcg(Aop, bd, xs[w], M, eps=args.eps)
    torch.cuda.synchronize(); ctx.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        _, it, res = api.pcg(Aop, bd, xs[warm + k], M, eps=args.eps)
    ctx.synchronize()
    el = time.perf_counter() - t0
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, x=xs[warm + steps - 1], it=it, res_norm=res)
    out = {"metric": "full-A Jacobi-PCG iterations/sec, 250k DoF (configs[1])", "value": round(steps * (it - 1) / el, 1),
           "unit": "iterations/s", "n_gpus": 1, "steps": steps, "warmup": warm, "ms_per_step": round(el / steps * 1e3, 3),
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
           "config": {"workload": f"configs[1]: N={N}, n={n}, nnz={A.nnz}, a=0.1+1e-4xy, pcg(A,b,0,Jacobi)", "it": it,
                      "final_relres": float(res[-1] / np.linalg.norm(b))},
           "roofline": None, "cpu_baseline": None}
    if not args.full:
        OUT.emit(json.dumps(out))
        return
    _, nb = Aop.bytes()
    e0, e1 = api.Event(ctx), api.Event(ctx)
    if args.kernel_reps <= 0:      # profiling passes (PMC): only the solves
        OUT.emit(json.dumps({"value": round(steps * (it - 1) / el, 1), "ms_per_step": round(el / steps * 1e3, 3), "it": it}))
        return
    Aop.apply_dominant(bd, reps=20); ctx.synchronize()
    reps = max(args.kernel_reps, 50)
    us = kernel_us(api, ctx, Aop, bd, reps)
    cpu = None
    if not args.no_cpu_baseline:
        from oracle import oracle as orc
        cores = orc.set_threads(min(len(os.sched_getaffinity(0)), 16))
        Ao, Mo = orc.csc_operator(A, gather=True), orc.jacobi_operator(A.diagonal())
        xo, ito, reso = orc.pcg(Ao, b, np.zeros(n), Mo, eps=args.eps)
        assert abs(ito - it) <= max(2, it // 100), f"GPU it={it}, oracle it={ito}"   # ~900-iteration CG: see DESIGN.md §3
        nsolve, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < 10.0:
            orc.pcg(Ao, b, np.zeros(n), Mo, eps=args.eps)
            nsolve += 1
        tc = time.perf_counter() - t0
        cpu = {"value": round(nsolve * (ito - 1) / tc, 1), "unit": "iterations/s", "cores": cores, "kind": "port",
               "sample": f"{nsolve} full Jacobi-PCG solves of the same system in {tc:.1f}s (C restatement, OpenMP row-gather SpMV; not Julia)"}
    out["roofline"] = {"bound": "hbm", "kernel": "k_spmv_csr", "achieved": round(nb / us / 1e3, 1), "peak": HBM_PEAK_GBS,
                       "unit": "GB/s", "frac": round(nb / us / 1e3 / HBM_PEAK_GBS, 4), "traffic": spmv_traffic(),
                       "bytes_per_launch": int(nb), "us_per_launch": round(us, 3)}
    out["cpu_baseline"] = cpu
    OUT.emit(json.dumps(out))


def secondary_measurements(args, api, fem, ctx, S, M, b_dev, n_Γ, ndom, bytes_iter, e0, e1):
    """The other loops of the path on the SAME device-resident operators, each timed like the headline (complete solves
    from x0 = 0, HIP events on the library's stream, median): `defpcg(S, b, 0, W, ΠSnn)` with the nvec = ndom + 10
    least-dominant eigenvectors of S (Example03:206-214), the recycling pair `eigpcg -> eigdefpcg` with nvec = 1.25 ndom,
    spdim = 3 ndom (Example09:39-40, _Functions.jl:345,364), unpreconditioned `cg(S, b, 0)`; and config 2. Each entry:
    loop iterations/s, time per loop iteration (difference of full and maxit-capped solves) and that iteration's HBM
    roofline fraction = algorithmic bytes of one iteration / time / 8 TB/s."""
    import torch
    out = {}
    t_all = time.perf_counter()

    def timed(solve, reps=12):
        ts, last = [], None
        for k in range(reps + 2):
            torch.cuda.synchronize()
            e0.record()
            last = solve()
            e1.record()
            if k >= 2:
                ts.append(e0.elapsed_ms(e1))
        return float(np.median(ts)), last

    def entry(name, solve_full, solve_short, short_it, bytes_per_iter, extra=None):
        try:    # a side measurement must not take the headline line down
            _entry(name, solve_full, solve_short, short_it, bytes_per_iter, extra)
        except Exception as e:   # noqa: BLE001
            out[name] = {"error": f"{type(e).__name__}: {e}"}

    def _entry(name, solve_full, solve_short, short_it, bytes_per_iter, extra=None):
        t_full, r = timed(solve_full)
        it = r[1]
        e = {"it": it, "iterations_per_s": round((it - 1) / (t_full * 1e-3), 1), "ms_per_solve": round(t_full, 4)}
        if it > short_it + 2:
            t_short, _ = timed(solve_short)
            us_it = (t_full - t_short) * 1e3 / (it - short_it)
            e.update({"us_per_iteration": round(us_it, 2), "bytes_per_iteration": int(bytes_per_iter),
                      "roofline_frac_iteration": round(bytes_per_iter / (us_it * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)})
        if extra:
            e.update(extra)
        out[name] = e

    z = lambda: torch.zeros(n_Γ, dtype=torch.float64, device="cuda")   # noqa: E731
    # W: least-dominant eigenvectors of the assembled S (a dense symmetric eigensolver stands in for KrylovKit, Example03:209).
    # On the HOST (LAPACK, untimed set-up): the device route went through rocSOLVER's dsyevd, which faults under
    # `rocprofv3 --pmc` (profiles/r02_pmc_crash_stack.txt) — the default command issues no rocSOLVER call any more.
    nvec_def = ndom + 10
    vec_bytes = lambda nv: 2 * nv * n_Γ * 8                                       # noqa: E731  WtA*z and W*mu streams
    try:
        from scipy.linalg import eigh as host_eigh
        eye = torch.eye(n_Γ, dtype=torch.float64, device="cuda")
        Sd = torch.stack([S.apply(eye[k].contiguous()) for k in range(n_Γ)], dim=1)
        ctx.synchronize()
        Sh = Sd.cpu().numpy()
        del Sd, eye
        Wh = host_eigh((Sh + Sh.T) / 2, subset_by_index=[0, nvec_def - 1])[1]
        W = torch.from_numpy(np.ascontiguousarray(Wh.T)).cuda().T                  # n x nvec, column-major
        entry(f"defpcg_nvec{nvec_def}", lambda: api.defpcg(S, b_dev, z(), W, M, eps=args.eps),
              lambda: api.defpcg(S, b_dev, z(), W, M, maxit=3, eps=args.eps), 3, bytes_iter + vec_bytes(nvec_def))
    except Exception as e:   # noqa: BLE001
        out[f"defpcg_nvec{nvec_def}"] = {"error": f"{type(e).__name__}: {e}"}
    nvec, spdim = int(1.25 * ndom), 3 * ndom
    entry(f"eigpcg_nvec{nvec}_spdim{spdim}", lambda: api.eigpcg(S, b_dev, z(), M, nvec, spdim, eps=args.eps),
          lambda: api.eigpcg(S, b_dev, z(), M, nvec, spdim, maxit=3, eps=args.eps), 3, bytes_iter)
    try:
        Wrec = api.eigpcg(S, b_dev, z(), M, nvec, spdim, eps=args.eps)[3]
        entry(f"eigdefpcg_nvec{nvec}_spdim{spdim}", lambda: api.eigdefpcg(S, b_dev, z(), M, Wrec, spdim, eps=args.eps),
              lambda: api.eigdefpcg(S, b_dev, z(), M, Wrec, spdim, maxit=3, eps=args.eps), 3, bytes_iter + vec_bytes(nvec) * 2)
    except Exception as e:   # noqa: BLE001
        out[f"eigdefpcg_nvec{nvec}_spdim{spdim}"] = {"error": f"{type(e).__name__}: {e}"}
    entry("cg_unpreconditioned", lambda: api.cg(S, b_dev, z(), eps=args.eps),
          lambda: api.cg(S, b_dev, z(), maxit=20, eps=args.eps), 20, bytes_iter // 2)
    try:
        config2_entry(args, api, fem, ctx, entry, torch)
    except Exception as e:   # noqa: BLE001
        out["config2_fullA_jacobi_pcg_250k"] = {"error": f"{type(e).__name__}: {e}"}
    return many_subdomains_entry(args, api, fem, ctx, entry, torch, out, t_all)


def config2_entry(args, api, fem, ctx, entry, torch):
    # ---- config 2: N = 500, full A, Jacobi-PCG (Example01:33-61 with Jacobi for AMG)
    mesh = fem.get_mesh(500)
    d = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
    A, b = fem.do_isotropic_elliptic_assembly(mesh.cells, mesh.points, d, mesh.point_marker,
                                              lambda x, y: 0.1 + 0.0001 * x * y, lambda x, y: -1.0 + 0 * x,
                                              lambda x, y: 3.0 + 0 * x)
    n = b.size
    Aop, Mj = api.SparseMatrixCSC(ctx, A), api.JacobiPreconditioner(ctx, A.diagonal())
    bd = torch.from_numpy(b).cuda()
    zf = lambda: torch.zeros(n, dtype=torch.float64, device="cuda")             # noqa: E731
    _, spmv_bytes = Aop.bytes()
    Aop.apply_dominant(bd, reps=20); ctx.synchronize()
    us = kernel_us(api, ctx, Aop, bd, 200)
    entry("config2_fullA_jacobi_pcg_250k", lambda: api.pcg(Aop, bd, zf(), Mj, eps=args.eps),
          lambda: api.pcg(Aop, bd, zf(), Mj, maxit=100, eps=args.eps), 100, spmv_bytes + 120 * n,
          {"workload": f"configs[1]: N=500, n={n}, nnz={A.nnz}, pcg(A,b,0,Jacobi)",
           "spmv_replayed_us": round(us, 3), "spmv_bytes": int(spmv_bytes),
           "spmv_replayed_frac": round(spmv_bytes / us / 1e3 / HBM_PEAK_GBS, 4),
           # what the SOLVER runs is k_spmv_pcg (SpMV of the direction formed on the fly + beta, stop rule, p, p'Ap), not the bare
           # replayed SpMV above: its own kernel time from the committed rocprofv3 summary of this workload
           "spmv_in_loop": (lambda t: None if t is None else {"kernel": "k_spmv_pcg", "us": round(t, 2),
                                                              "frac_of_spmv_bytes": round(spmv_bytes / t / 1e3 / HBM_PEAK_GBS, 4),
                                                              "source": "profiles/r03_kernel_stats_fullA.csv (rocprofv3 --kernel-trace --stats of `bench.py --workload fullA`)"})(
               profiled_kernel_us("r03_kernel_stats_fullA.csv", "k_spmv_pcg"))})


def many_subdomains_entry(args, api, fem, ctx, entry, torch, out, t_all):
    # ---- the reference's own partition sizes (80-500 subdomains, KarhunenLoeveDomainDecompositionHelper.jl:14-32): 160
    # subdomains of an N = 400 mesh, n_Γ = 9417 > 8192: the generic multi-workgroup loop (tests/test_gpu_manydomains.py)
    if not getattr(args, "many_subdomains", False):
        out["wall_s"] = round(time.perf_counter() - t_all, 1)
        return out
    try:
        mesh = fem.get_mesh(400)
        gm = fem.draw(fem.synthetic_kl(mesh.points), np.random.default_rng(481456))[1]
        Pm = fem.build_schur_problem(400, 16, 10, np.exp(gm), lambda x, y: -1.0 + 0 * x, lambda x, y: 0.734 + 0 * x, mesh=mesh)
        Sm = api.LocalSchurs(ctx, Pm.Sd, Pm.sub.gather_idx, Pm.sub.node_Γ_cnt)
        Mm = api.NeumannNeumannSchurPreconditioner(ctx, Pm.ΠSd, Pm.sub.gather_idx, Pm.sub.node_Γ_cnt)
        bm = torch.from_numpy(Pm.b_schur).cuda()
        zm = lambda: torch.zeros(Pm.sub.n_Γ, dtype=torch.float64, device="cuda")      # noqa: E731
        bs, _ = Sm.bytes()
        bn, _ = Mm.bytes()
        entry("pcg_160_subdomains_generic_loop", lambda: api.pcg(Sm, bm, zm(), Mm, eps=args.eps),
              lambda: api.pcg(Sm, bm, zm(), Mm, maxit=50, eps=args.eps), 50, int(bs + bn),
              {"workload": f"N=400, 16x10 boxes, n_Γ={Pm.sub.n_Γ}, max n_Γd={max(len(a) for a in Pm.sub.gather_idx)}: "
                           "pcg(S, b_schur, 0, ΠSnn) on the multi-workgroup loop (n_Γ > 8192)"})
    except Exception as e:   # a side measurement must not take the headline line down
        out["pcg_160_subdomains_generic_loop"] = {"error": f"{type(e).__name__}: {e}"}
    out["wall_s"] = round(time.perf_counter() - t_all, 1)
    return out


def setup_measurement(api, ctx, P, S, M):
    """Set-up of the assembled mode on the device for one realization of config 3 (Example07:180-199): S_d and the condensed
    right-hand sides by exact level elimination (mi_schur_setup_run: hand-written kernels, one graph replay), ΠS_d = pinv(S_d) (mi_nn_pinv), operator refill
    (mi_dense_set_blocks); block values already on the device. Wall clock, synchronised."""
    import torch
    sub = P.sub
    t0 = time.perf_counter()
    setup = api.SchurSetup(ctx, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd)
    t_plan = time.perf_counter() - t0
    vals = [torch.from_numpy(v).cuda() for v in setup._vals]
    bI = torch.from_numpy(np.concatenate(P.b_Id)).cuda()
    setup.run(*vals, bI); ctx.synchronize()          # first call: library handles, work space
    t0 = time.perf_counter()
    Sd, w = setup.run(*vals, bI)
    ctx.synchronize()
    t_S = time.perf_counter() - t0
    t0 = time.perf_counter()
    Pi = api.nn_pinv(ctx, sub.n_Γd, Sd)
    ctx.synchronize()
    t_pinv = time.perf_counter() - t0
    t0 = time.perf_counter()
    S.set_blocks(Sd); M.set_blocks(Pi)
    ctx.synchronize()
    t_set = time.perf_counter() - t0
    out = {"plan_once_s": round(t_plan, 3), "assemble_local_schurs_ms": round(t_S * 1e3, 1), "pinv_ms": round(t_pinv * 1e3, 1),
           "set_blocks_ms": round(t_set * 1e3, 2),
           "note": "S_d: block Gauss-Jordan level elimination (fp64 MFMA, upper-triangular tiles), all subdomains batched, one hipGraph replay; "
                   "look-ahead pivots; pinv: the same inversion behind a norm certificate (floating blocks: rank-one shift), eigen-decomposition only beyond"}
    # the matrix-free S-apply (apply_local_schurs, EPDD.jl:711-747) with the EXACT interior solve of the kept level inverses
    # (mi_schur_setup_keep_levels) against the reference's own interior iteration on the device (IterativeSolvers.cg, reltol 1e-9)
    try:
        setup.keep_levels(True)
        t0 = time.perf_counter()
        Sd2, _ = setup.run(*vals, bI)
        ctx.synchronize()
        t_keep = time.perf_counter() - t0
        Smf = api.MatrixFreeLocalSchurs(ctx, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd, sub.gather_idx, sub.node_Γ_cnt, None, reltol=1e-9)
        v = torch.from_numpy(np.random.default_rng(0).standard_normal(sub.n_Γ)).cuda()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y_cg = Smf.apply(v)
        ctx.synchronize()
        t_cg = time.perf_counter() - t0
        Smf.use_level_solver(setup)
        Smf.apply(v); ctx.synchronize()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            y_lv = Smf.apply(v)
            ctx.synchronize()
            ts.append(time.perf_counter() - t0)
        y_as = S.apply(v)
        ctx.synchronize()
        scale = float(y_as.abs().max())
        out["matrix_free_apply"] = {"interior_cg_reltol1e-9_ms": round(t_cg * 1e3, 1), "level_solves_ms": round(min(ts) * 1e3, 2),
                                    "setup_with_kept_levels_ms": round(t_keep * 1e3, 1),
                                    "rel_diff_level_vs_assembled": float((y_lv - y_as).abs().max()) / scale,
                                    "rel_diff_cg_vs_assembled": float((y_cg - y_as).abs().max()) / scale}
        setup.keep_levels(False)
    except Exception as e:   # noqa: BLE001
        out["matrix_free_apply"] = {"error": f"{type(e).__name__}: {e}"}
    return out


def config5_measurement(args, api, fem, ctx, mesh, P, f, uex, nreals=50, check_first=3):
    """BASELINE.json configs[4] end to end on ONE GPU (it is "replicas only": every GPU of a node runs this same chain on
    its own realizations): `nreals` consecutive realizations of the lognormal coefficient, each ENTIRELY on the device —
    coefficient a = exp(Ψ (√Λ ξ_t)) -> element loop (mi_assembly_run; `prepare_local_schurs`, Example07:162-171) -> S_d and
    the condensed right-hand side (mi_schur_setup_run; Example07:180-187, EPDD.jl:667-695, 853-861) -> operator refill
    (mi_dense_set_blocks) -> b_schur -> the recycling pair of Example09_..._Functions.jl:345,364 with the ξ = 0
    preconditioner ΠSnn_0 fixed (Example07:152-154, 273): `eigpcg` for the first system, `eigdefpcg` with the W the previous
    solve returned for every later one (nvec = 1.25 ndom, spdim = 3 ndom, Example09:39-40). Reports realizations/s, the time
    split, the histogram of `it`; for the first `check_first` realizations `it` is ASSERTED against the C / numpy oracle on
    the same blocks, right-hand side and incoming W (rank 0, outside the timed figure)."""
    import torch
    # torch kernels (coefficient, b_schur) and the library's launches interleave: one stream for both — a torch stream of
    # its own, not the legacy default stream (the solvers capture graphs)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx.use_torch_stream()
        try:
            return _config5_chain(args, api, fem, ctx, mesh, P, f, uex, nreals, check_first)
        finally:
            ctx.synchronize()
            ctx.use_own_stream()


def _config5_chain(args, api, fem, ctx, mesh, P, f, uex, nreals, check_first):
    import torch
    sub = P.sub
    n, ndom = sub.n_Γ, sub.ndom
    t_once = time.perf_counter()
    plan = fem.make_assembly_plan(mesh.cells, mesh.points, P.epart, sub, f, uex)
    dev_plan = api.AssemblyPlan(ctx, plan)
    setup = api.SchurSetup(ctx, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd)
    kl = fem.synthetic_kl(mesh.points)
    Psi = torch.from_numpy(kl.Ψ).cuda()
    sqrtL = np.sqrt(kl.Λ)
    gidx = [torch.from_numpy(np.asarray(g, dtype=np.int64)).cuda() for g in sub.gather_idx]

    def realize(a_dev):   # everything of a realization's set-up on the stream; returns (S_d blocks on the device, b_schur)
        vals = dev_plan.run(a_dev)
        ii, ig, gg, bI, bΓ = dev_plan.block_values(vals)
        Sd, w = setup.run(ii, ig, gg, bI)
        b = bΓ.clone()
        off = 0
        for d in range(ndom):                      # get_schur_rhs, EPDD.jl:853-861: subdomains in ascending order
            b[gidx[d]] -= w[off:off + sub.n_Γd[d]]
            off += sub.n_Γd[d]
        return Sd, b

    # ξ = 0: the reference operator and its Neumann-Neumann preconditioner, built once (Example07:88-154)
    Sd0, _ = realize(torch.ones(plan.n_node, dtype=torch.float64, device="cuda"))
    S5 = api.LocalSchurs(ctx, P.Sd, sub.gather_idx, sub.node_Γ_cnt)
    M0 = api.NeumannNeumannSchurPreconditioner(ctx, P.ΠSd, sub.gather_idx, sub.node_Γ_cnt)
    Pi0 = api.nn_pinv(ctx, sub.n_Γd, Sd0)
    M0.set_blocks(Pi0)
    ctx.synchronize()
    t_once = time.perf_counter() - t_once
    rng = np.random.default_rng(args.seed)
    xis = [rng.standard_normal(kl.Λ.size) for _ in range(nreals)]    # consecutive draws of the same generator
    nvec, spdim = int(1.25 * ndom), 3 * ndom
    its, split = [], {"coefficient_and_assembly": 0.0, "assemble_local_schurs_and_rhs": 0.0, "set_blocks": 0.0, "solve": 0.0}
    checks = []
    W = None
    x0 = torch.zeros(n, dtype=torch.float64, device="cuda")

    def lap(key, t):
        ctx.synchronize(); torch.cuda.synchronize()
        now = time.perf_counter()
        split[key] += now - t
        return now

    # warm-up realization (graphs, work space), not counted
    Sdw, bw = realize(torch.exp(Psi @ torch.from_numpy(sqrtL * xis[0]).cuda()))
    S5.set_blocks(Sdw)
    api.eigpcg(S5, bw, x0.clone(), M0, nvec, spdim)
    ctx.synchronize(); torch.cuda.synchronize()
    t_all = time.perf_counter()
    for t in range(nreals):
        t0 = time.perf_counter()
        a = torch.exp(Psi @ torch.from_numpy(sqrtL * xis[t]).cuda())
        vals = dev_plan.run(a)
        ii, ig, gg, bI, bΓ = dev_plan.block_values(vals)
        t0 = lap("coefficient_and_assembly", t0)
        Sd, w = setup.run(ii, ig, gg, bI)
        b = bΓ.clone()
        off = 0
        for d in range(ndom):
            b[gidx[d]] -= w[off:off + sub.n_Γd[d]]
            off += sub.n_Γd[d]
        t0 = lap("assemble_local_schurs_and_rhs", t0)
        S5.set_blocks(Sd)
        t0 = lap("set_blocks", t0)
        W_in = W
        if W is None:
            x, it, res, W = api.eigpcg(S5, b, x0.clone(), M0, nvec, spdim)
        else:
            x, it, res, W = api.eigdefpcg(S5, b, x0.clone(), M0, W, spdim)
        t0 = lap("solve", t0)
        its.append(int(it))
        if t < check_first:      # inputs of this solve, for the oracle check after the timed loop
            to_host = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)   # noqa: E731
            checks.append(([np.asfortranarray(to_host(blk)) for blk in setup.blocks(Sd)], to_host(b),
                           None if W_in is None else np.asfortranarray(to_host(W_in)), int(it), np.array(to_host(res), copy=True)))
            t_all += time.perf_counter() - t0     # (the copies for the check are not part of the chain)
    elapsed = time.perf_counter() - t_all
    out = {"realizations": nreals, "realizations_per_s": round(nreals / elapsed, 3), "ms_per_realization": round(elapsed / nreals * 1e3, 1),
           "split_ms_per_realization": {k: round(v / nreals * 1e3, 2) for k, v in split.items()},
           "it_histogram": {str(k): int(v) for k, v in sorted(zip(*np.unique(its, return_counts=True)))},
           "it_first": its[:8], "nvec": nvec, "spdim": spdim, "once_s": round(t_once, 2),
           "chain": "a=exp(Ψ√Λξ_t) -> mi_assembly_run -> mi_schur_setup_run -> mi_dense_set_blocks -> eigpcg (t=0) / eigdefpcg(W recycled), ΠSnn_0 fixed; "
                    "one GPU (config 5 is replicas only: N GPUs run N such chains)"}
    if not args.no_cpu_baseline and checks:
        from oracle import oracle as orc
        Pi0_h = [np.asfortranarray(blk.cpu().numpy()) for blk in setup.blocks(Pi0)]
        Mo = orc.neumann_neumann_operator(Pi0_h, sub.gather_idx, sub.node_Γ_cnt)
        ito, dev_max = [], 0.0
        for blocks, bh, Wh, it_dev, res_dev in checks:
            So = orc.apply_local_schurs_operator(blocks, sub.gather_idx, n)
            r = orc.eigpcg(So, bh, np.zeros(n), Mo, nvec, spdim) if Wh is None else orc.eigdefpcg(So, bh, np.zeros(n), Mo, np.asfortranarray(Wh), spdim)
            ito.append(int(r[1]))
            # With ΠSnn_0 fixed over the realizations PCG's recurrence is sensitive to rounding: two correct fp64 summation
            # orders separate by ~10x per iteration after a dozen iterations (measured) and may stop one
            # iteration apart. The calibrated bar (two CPU orders; `it` equal wherever they agree) is tests/test_gpu_config5.py;
            # here: at most one iteration apart, both counts reported.
            assert abs(int(r[1]) - it_dev) <= 1, f"config 5: device it={it_dev}, oracle it={r[1]}"
            k = min(int(r[1]), it_dev)
            dev_max = max(dev_max, max(abs(float(res_dev[i]) - float(r[2][i])) / float(r[2][i]) for i in range(k)))
        out["max_rel_deviation_of_residual_histories"] = dev_max
        out["it_oracle_first"] = ito
    return out


class StdoutToStderr:
    """Everything written to fd 1 while this is active goes to stderr (RCCL prints a version banner on stdout when a
    communicator is created); `emit` writes one line to the real stdout — the ONE JSON line of the contract."""

    def __init__(self):
        sys.stdout.flush()
        self._saved = os.dup(1)
        os.dup2(2, 1)

    def emit(self, line: str) -> None:
        sys.stdout.flush()
        os.write(self._saved, (line + "\n").encode())


OUT = None


def dump_outputs(out_dir: str, **arrays) -> None:
    """--dump-outputs: what the caller of the timed solve received in the last step (x on the device, `it`, the residual
    history), one float64 DIR/<name>.npy each, so that two builds can be compared output for output."""
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        a = a.detach().cpu().numpy() if hasattr(a, "detach") else a
        np.save(os.path.join(out_dir, f"{name}.npy"), np.asarray(a, dtype=np.float64))


def spawn_ranks(n: int) -> None:
    """Run this same command line as n rank processes (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set the way
    torch.distributed.run sets them) and wait for them. Rank 0 prints the JSON line on the inherited stdout."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=OUT._saved))   # the real stdout (this process's fd 1 points at stderr by now)
    codes = [p.wait() for p in procs]
    if any(codes):
        raise SystemExit(f"rank exit codes {codes}")


def launcher_selftest(rank: int, world: int) -> None:
    """--launcher-selftest: what the spawned ranks do instead of the benchmark — a gloo rendezvous and one all-reduce
    on the CPU (tests/test_multirank_cpu.py checks the launcher with it; no GPU involved)."""
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo")
    t = torch.tensor([float(rank + 1)], dtype=torch.float64)
    dist.all_reduce(t)
    assert dist.get_rank() == rank and dist.get_world_size() == world
    if rank == 0:
        OUT.emit(json.dumps({"launcher": "ok", "n_gpus": world, "sum": t.item(), "master": os.environ["MASTER_ADDR"]}))
    dist.destroy_process_group()


def main():
    global OUT
    OUT = StdoutToStderr()
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--N", type=int, default=1000, help="nodes per side (1000 -> 996 004 free DoF)")
    ap.add_argument("--px", type=int, default=4)
    ap.add_argument("--py", type=int, default=2)
    ap.add_argument("--seed", type=int, default=481456)
    ap.add_argument("--chunk", type=int, default=-1, help="iterations per captured graph (-1: library default)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--kernel-reps", type=int, default=200)
    ap.add_argument("--force-dist", action="store_true",
                    help="take the multi-GPU code path (process group, RCCL communicator, all-reduces) even with one rank")
    ap.add_argument("--exchange", choices=["auto", "peer", "peer-inlaunch", "rccl"], default="auto",
                    help="multi-GPU Γ-sum: the one-shot peer exchange when every rank can map its peers' arenas (auto / peer: "
                         "one-wave wait kernels between the launches; peer-inlaunch: the launches wait for the flags themselves — "
                         "only when every rank has a GPU of its own; measured equal on one GPU), or RCCL all-reduces")
    ap.add_argument("--shard-precond", action="store_true",
                    help="multi-GPU: shard the Neumann-Neumann blocks like S (two all-reduces per iteration) instead of replicating them")
    ap.add_argument("--workload", choices=["schur", "fullA"], default="schur",
                    help="schur: configs[2] (headline, default). fullA: configs[1], pcg on the full matrix (CSR SpMV + BLAS-1)")
    ap.add_argument("--eps", type=float, default=1e-7, help="stop tolerance (reference constant 1e-7; other values for analysis only)")
    ap.add_argument("--no-secondary", action="store_true", help="skip the `secondary` object (deflated / recycling loops, config 2)")
    ap.add_argument("--config5-reals", type=int, default=50, help="realizations of the config-5 chain in `secondary.config5`")
    ap.add_argument("--many-subdomains", action="store_true",
                    help="add the 160-subdomain problem (n_Γ = 9417) to `secondary`; off by default so that the kernel statistics of the "
                         "default command contain the headline's launches of k_gemv_pcg only")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: `roofline` (--kernel-reps), `cpu_baseline` with the oracle's "
                         "parity check (--no-cpu-baseline), `secondary` (--no-secondary, --config5-reals, --many-subdomains)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write x, it and res_norm of the last timed solve as DIR/<name>.npy (float64)")
    ap.add_argument("--launcher-selftest", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the N ranks ourselves, as fresh children, BEFORE this
        # process touches the GPU (it never does: it only waits), one rank per GPU, rendezvous on 127.0.0.1
        return spawn_ranks(args.gpus)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run")
    if args.launcher_selftest:
        return launcher_selftest(rank, world)

    if args.workload == "fullA":
        return bench_full_system(args)
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(local_rank)
    multi = world > 1 or args.force_dist
    peer_on = False
    peer_inwait = False
    if multi:
        if "RANK" not in os.environ:      # --force-dist from a plain `python bench.py`: a one-rank rendezvous on the loopback
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                port = sk.getsockname()[1]
            os.environ.update({"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    pkg = graft.load_package()
    fem, api = pkg.fem, pkg.api
    ndom = args.px * args.py
    lo, hi = api.shard_domains(ndom, rank, world)

    # ---------------- problem set-up on the host (not timed; the reference does this in Julia)
    t0 = time.time()
    mesh = fem.get_mesh(args.N)
    kl = fem.synthetic_kl(mesh.points)
    _, g = fem.draw(kl, np.random.default_rng(args.seed))       # config 3: a = exp(g)
    coeff = np.exp(g)
    f = lambda x, y: -1.0 + 0 * x
    uex = lambda x, y: 0.734 + 0 * x
    # S_d, the condensed right-hand side and ΠS_d = pinv(S_d) through the library's own device set-up (mi_schur_setup_run,
    # mi_nn_pinv): the default command dispatches no kernel of another library (rocSOLVER / rocBLAS through torch faulted
    # under `rocprofv3 --pmc`, profiles/r02_pmc_crash_stack.txt); MI355_SETUP_ON_HOST=1 keeps fem.py's host elimination
    ctx = api.Context(local_rank)
    hook = None if os.environ.get("MI355_SETUP_ON_HOST") else api.device_dense_setup(ctx)
    P = fem.build_schur_problem(args.N, args.px, args.py, coeff, f, uex, dom_slice=(lo, hi), dense_setup=hook)
    n_Γ = P.sub.n_Γ
    n_free = int((mesh.point_marker == 0).sum())
    log(rank, f"set-up {time.time() - t0:.1f}s: free DoF={n_free} n_Γ={n_Γ} n_Γd={P.sub.n_Γd} local subdomains {lo}..{hi - 1}")

    # ---------------- device residents
    if args.chunk >= 0:
        ctx.set_chunk(args.chunk)
    if multi:
        uid = torch.zeros(128, dtype=torch.uint8, device="cuda")
        if rank == 0:
            uid = torch.frombuffer(bytearray(ctx.unique_id()), dtype=torch.uint8).cuda()
        dist.broadcast(uid, 0)
        ctx.comm_init(bytes(uid.cpu().numpy().tobytes()), rank, world)
        # The one-shot peer exchange (include/mi355schur.h) carries the tables of the folded launches when every rank can
        # map every other rank's arena (same node, peer access over xGMI): IPC handles travel through torch.distributed.
        # All ranks take the same decision; otherwise RCCL carries everything.
        if args.exchange != "rccl":
            ok, handle = 1, None
            try:
                ctx.peer_init(rank, world)
                handle, _ = ctx.peer_export()
            except Exception as e:                               # noqa: BLE001
                ok = 0
                log(rank, f"peer exchange unavailable on rank {rank}: {e}")
            handles = [None] * world
            dist.all_gather_object(handles, handle)
            if ok and all(h is not None for h in handles):
                try:
                    for q, h in enumerate(handles):
                        if q != rank:
                            ctx.peer_import(q, h)
                except Exception as e:                           # noqa: BLE001
                    ok = 0
                    log(rank, f"peer exchange: cannot map a peer's arena from rank {rank}: {e}")
            else:
                ok = 0
            flag = torch.tensor([ok], dtype=torch.int32, device="cuda")
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            peer_on = bool(flag.item())
            if peer_on:
                os.environ.setdefault("MI355_PEER_TIMEOUT_MS", "20000")     # (the self-check below must not sit out the library's 60 s)
                ctx.peer_ready()
                # a launch that waits for its peers' flags keeps its compute units: only when no two ranks share a GPU
                ident = (os.environ.get("HIP_VISIBLE_DEVICES"), os.environ.get("ROCR_VISIBLE_DEVICES"),
                         os.environ.get("CUDA_VISIBLE_DEVICES"), torch.cuda.current_device())
                idents = [None] * world
                dist.all_gather_object(idents, ident)
                peer_inwait = args.exchange == "peer-inlaunch" and len(set(idents)) == world
                ctx.set_exchange(2 if peer_inwait else 1)
                peer_inwait = ctx.query("peer_exchange") == 3          # (needs a fine-grained arena: mode 1 otherwise)
            elif args.exchange in ("peer", "peer-inlaunch"):
                raise SystemExit("--exchange peer: the peer exchange could not be set up on every rank")
        if peer_on and (world > 1 or args.force_dist):
            args.shard_precond = True      # both operators sharded: two cheap exchanges per iteration instead of a replicated ΠS stream
                                           # (--force-dist on one GPU: the whole sharded machinery with every tile active — what the
                                           # two exchanges of an iteration cost when the arenas are local memory)
        bs = torch.from_numpy(P.b_schur).cuda()
        dist.all_reduce(bs)                                     # b_schur = Σ_ranks (set-up plumbing)
        b_host = bs.cpu().numpy()
    else:
        b_host = P.b_schur
    if args.force_dist and world == 1:
        os.environ["MI355_FORCE_REDUCE"] = "1"   # one-rank rehearsal: keep the collectives of the sharded S
    S = api.LocalSchurs(ctx, P.Sd, P.sub.gather_idx, P.sub.node_Γ_cnt, dom_slice=(lo, hi))
    if not args.shard_precond:
        os.environ.pop("MI355_FORCE_REDUCE", None)        # (kept for the Neumann-Neumann blocks when they are "sharded" too)
    def replicated_nn():
        # S is sharded (subdomain d on GPU d, one all-reduce per S-apply). The Neumann-Neumann blocks are replicated
        # on every rank instead (68 MB): the NN-apply is then purely local and an iteration needs ONE all-reduce.
        Pi_all = list(P.ΠSd)
        for d in range(ndom):
            owner = next(r for r in range(world) if api.shard_domains(ndom, r, world)[0] <= d < api.shard_domains(ndom, r, world)[1])
            nd = P.sub.n_Γd[d]
            t = torch.from_numpy(np.ascontiguousarray(Pi_all[d])).cuda() if rank == owner else \
                torch.empty((nd, nd), dtype=torch.float64, device="cuda")
            dist.broadcast(t, owner)
            Pi_all[d] = np.asfortranarray(t.cpu().numpy()) if rank != owner else Pi_all[d]
        return api.NeumannNeumannSchurPreconditioner(ctx, Pi_all, P.sub.gather_idx, P.sub.node_Γ_cnt, dom_slice=(0, ndom))

    if multi and not args.shard_precond:
        M = replicated_nn()
    else:
        M = api.NeumannNeumannSchurPreconditioner(ctx, P.ΠSd, P.sub.gather_idx, P.sub.node_Γ_cnt, dom_slice=(lo, hi))
    os.environ.pop("MI355_FORCE_REDUCE", None)
    b_dev = torch.from_numpy(b_host).cuda()
    xs = [torch.zeros(n_Γ, dtype=torch.float64, device="cuda") for _ in range(args.warmup + args.steps)]
    torch.cuda.synchronize()

    def barrier():
        torch.cuda.synchronize()
        ctx.synchronize()
        if multi:
            dist.barrier()

    # ---------------- the peer exchange is checked on THIS machine before anything is timed: one solve through it against the
    # same solve through RCCL's all-reduces (it was developed without a multi-GPU box). A rank that fails or
    # disagrees sends every rank back to RCCL — a wrong or hanging exchange must never reach the timed region.
    if multi and peer_on:
        ok = 1
        x_peer = torch.zeros(n_Γ, dtype=torch.float64, device="cuda")
        x_rccl = torch.zeros(n_Γ, dtype=torch.float64, device="cuda")
        it_p = -1
        try:
            _, it_p, _ = api.pcg(S, b_dev, x_peer, M, eps=args.eps)
        except Exception as e:                                   # noqa: BLE001  (MI_ERR_COMM: a wait expired)
            ok = 0
            log(rank, f"peer exchange failed on rank {rank}: {e}")
        ctx.set_exchange(0)
        _, it_r, _ = api.pcg(S, b_dev, x_rccl, M, eps=args.eps)
        if ok:
            dx = float((x_peer - x_rccl).abs().max()) / max(float(x_rccl.abs().max()), 1e-300)
            ok = int(it_p == it_r and dx <= 1e-9)
            if not ok:
                log(rank, f"peer exchange disagrees with RCCL on rank {rank}: it {it_p} vs {it_r}, |dx|/|x| = {dx:.2e}")
        flag = torch.tensor([ok], dtype=torch.int32, device="cuda")
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag.item()):
            ctx.set_exchange(2 if peer_inwait else 1)
        else:
            peer_on = peer_inwait = False
            log(rank, "peer exchange rejected by its self-check: RCCL all-reduces carry the Γ-sums of this run")

    # ---------------- `--exchange auto`: which of the two multi-GPU layouts is faster HERE — both operators sharded over the
    # peer exchange, or S sharded + Neumann-Neumann blocks replicated with one RCCL all-reduce per iteration — is measured
    # (3 solves each, maximum over the ranks), not assumed: the peer exchange has never met real xGMI.
    layout_times = None
    if multi and peer_on and args.exchange == "auto":
        try:
            M_rep = replicated_nn()
            xq = torch.zeros(n_Γ, dtype=torch.float64, device="cuda")

            def timed(Mx, mode):
                ctx.set_exchange(mode)
                xq.zero_(); api.pcg(S, b_dev, xq, Mx, eps=args.eps)           # graphs of this layout
                barrier()
                t0 = time.perf_counter()
                for _ in range(3):
                    xq.zero_(); api.pcg(S, b_dev, xq, Mx, eps=args.eps)
                barrier()
                return time.perf_counter() - t0
            tt = torch.tensor([timed(M, 2 if peer_inwait else 1), timed(M_rep, 0)], dtype=torch.float64, device="cuda")
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            layout_times = {"peer_both_sharded_ms_per_solve": round(float(tt[0]) / 3 * 1e3, 4), "rccl_nn_replicated_ms_per_solve": round(float(tt[1]) / 3 * 1e3, 4)}
            if float(tt[1]) < 0.97 * float(tt[0]):
                M, peer_on, peer_inwait, args.shard_precond = M_rep, False, False, False
                ctx.set_exchange(0)
                log(rank, f"layout: RCCL with replicated Neumann-Neumann blocks is faster here {layout_times}")
            else:
                ctx.set_exchange(2 if peer_inwait else 1)
                log(rank, f"layout: both operators sharded over the peer exchange {layout_times}")
        except Exception as e:                                       # noqa: BLE001
            ctx.set_exchange(2 if peer_inwait else 1)
            log(rank, f"layout comparison skipped: {e}")

    # ---------------- warm-up, then the timed region: EXACTLY K solves
    its = None
    for w in range(args.warmup):
        _, it, res = api.pcg(S, b_dev, xs[w], M, eps=args.eps)
        its = it if its is None else its
        assert it == its
    if its is None:
        _, its, res = api.pcg(S, b_dev, torch.zeros_like(b_dev), M, eps=args.eps)
    barrier()
    t0 = time.perf_counter()
    for k in range(args.steps):
        _, it, res = api.pcg(S, b_dev, xs[args.warmup + k], M, eps=args.eps)
    barrier()
    elapsed = time.perf_counter() - t0
    assert it == its, "iteration count changed between solves"
    if multi:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    loop_its = its - 1
    value = args.steps * loop_its / elapsed
    relres = float(res[-1] / np.linalg.norm(b_host))
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, x=xs[args.warmup + args.steps - 1], it=it, res_norm=res)
    short = max(2, min(5, its - 2))
    folded = its > short + 2   # every layout runs the folded loop (sharded launches are followed by an exchange: peer stores or an RCCL all-reduce of the launch's table)

    # ---------------- --full: roofline, secondary workloads and the CPU baseline (with the oracle's parity check)
    roofline = cpu = secondary = None
    if args.full:
        full = full_measurements(args, rank, world, multi, api, fem, ctx, mesh, P, f, uex, S, M, b_dev, b_host, n_Γ, ndom,
                                 its, res, short, folded, value, elapsed)
        if full is None:
            return
        roofline, secondary, cpu = full

    if rank == 0:
        out = {
            "metric": "Schur-PCG iterations/sec (NN-preconditioned, assembled local Schurs), 1M DoF",
            "value": round(value, 1), "unit": "iterations/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": f"configs[2]: N={args.N} structured P1 mesh, {n_free} free DoF, {ndom} subdomains "
                                   f"({args.px}x{args.py} boxes), lognormal a=exp(g) seed {args.seed}, n_Γ={n_Γ}; "
                                   f"pcg(S, b_schur, 0, ΠSnn), eps={args.eps:g}",
                       "subdomains_per_gpu": hi - lo,
                       "parallelism": ("single GPU" if not multi else
                                       f"S sharded {hi - lo} subdomain(s)/GPU; NN blocks "
                                       + ("sharded: folded loop, two peer exchanges per iteration (the launches store into every rank's arena over xGMI and signal; "
                                          + ("the next launch waits for the flags itself" if peer_inwait else "a one-wave kernel waits for the flags") + ", csrc/exchange.hpp)"
                                          if args.shard_precond and peer_on else
                                          "sharded: folded loop, an RCCL all-reduce of the launch's table behind each of the two launches" if args.shard_precond
                                          else "replicated: folded loop, 1 exchange of the S launch's contribution table per iteration ("
                                               + ("peer stores" if peer_on else "RCCL all-reduce") + ")")),
                       "exchange": (("peer-inlaunch" if peer_inwait else "peer") if peer_on else "rccl") if multi else None,
                       "layouts_measured": layout_times,
                       "it": its, "loop_iterations_per_solve": loop_its,
                       "final_relres": relres, "launches_per_iteration": 2 if folded else 4},
            "roofline": roofline,
            "cpu_baseline": cpu,
            "secondary": secondary,
        }
        OUT.emit(json.dumps(out))
    if multi:
        dist.destroy_process_group()


def full_measurements(args, rank, world, multi, api, fem, ctx, mesh, P, f, uex, S, M, b_dev, b_host, n_Γ, ndom,
                      its, res, short, folded, value, elapsed):
    """What `--full` adds to the headline run, on the same device-resident operators after the timed region:
    (roofline, secondary, cpu_baseline); None after a profiling run's reduced line (--kernel-reps 0)."""
    import torch
    # ---------------- roofline of the dominant kernel, HIP events on the library's stream
    # In the timed region every iteration is two launches of k_gemv_pcg (the S-apply and the NN-apply GEMV with
    # the PCG vector work folded in). Their average duration is measured live as the GPU-time difference between
    # full solves and solves cut at maxit = 5, divided by the number of extra launches (set-up and copies cancel).
    _, bytes_dom = S.bytes()
    _, bytes_nn = M.bytes()
    e0, e1 = api.Event(ctx), api.Event(ctx)
    if args.kernel_reps <= 0:      # profiling runs: leave only the solves in the trace
        if rank == 0:
            OUT.emit(json.dumps({"value": round(value, 1), "ms_per_step": round(elapsed / args.steps * 1e3, 4), "it": its}))
        return None

    def gpu_ms(maxit, reps=30):
        ts = []
        xz = torch.zeros(n_Γ, dtype=torch.float64, device="cuda")
        for k in range(reps + 3):
            xz.zero_(); torch.cuda.synchronize()
            e0.record()
            api.pcg(S, b_dev, xz, M, maxit=maxit, eps=args.eps)
            e1.record()
            if k >= 3:
                ts.append(e0.elapsed_ms(e1))
        return float(np.median(ts))

    k_us = None
    if folded:
        t_short = gpu_ms(short)
        t_full = gpu_ms(0)
        k_us = (t_full - t_short) * 1e3 / (2 * (its - short))
    # the GEMV kernels alone (no PCG work folded in): `reps` back-to-back launches each
    S.apply_dominant(b_dev, reps=20)
    M.apply_dominant(b_dev, reps=20)
    k_ms = kernel_us(api, ctx, S, b_dev, args.kernel_reps) * 1e-3
    nn_ms = kernel_us(api, ctx, M, b_dev, args.kernel_reps) * 1e-3
    pmc_table = {}
    pmc = os.path.join(ROOT, "profiles", "hbm_traffic.json")  # written by tools/hbm_traffic.py from rocprofv3 --pmc passes
    if os.path.exists(pmc):
        try:
            pmc_table = json.load(open(pmc))
        except Exception:
            pmc_table = {}
    bytes_launch = (bytes_dom + bytes_nn) / 2
    if k_us is None:               # N>1: the unfolded launches run; report the plain S-apply GEMV
        k_us, kname = k_ms * 1e3, "k_gemv_batched<S-apply>"
        bytes_launch = bytes_dom
    else:
        kname = "k_gemv_pcg (S-apply / NN-apply GEMV with the PCG update folded in; average of both phases)"
        if multi:
            kname += "; N>1: half an iteration, i.e. including half of the all-reduce that follows the sharded S launch"
    if kname.startswith("k_gemv_pcg"):
        traffic = pmc_table.get("dominant_kernel_bytes_per_launch")
    else:
        traffic = next((v["bytes_per_launch"] for k, v in pmc_table.items()
                        if isinstance(v, dict) and "k_gemv_batched" in k and "false" in k), None)
    achieved = bytes_launch / (k_us * 1e-6) / 1e9
    roofline = {"bound": "hbm", "kernel": kname, "achieved": round(achieved, 1),
                "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                "traffic": traffic, "traffic_source": "profiles/hbm_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, tools/pmc_pass.sh); not re-measured in this run",
                "bytes_per_launch": int(bytes_launch), "us_per_launch": round(k_us, 3),
                "plain_gemv": {"S_apply_us": round(k_ms * 1e3, 3), "S_apply_GBs": round(bytes_dom / (k_ms * 1e-3) / 1e9, 1),
                               "NN_apply_us": round(nn_ms * 1e3, 3), "NN_apply_GBs": round(bytes_nn / (nn_ms * 1e-3) / 1e9, 1)}}

    # ---------------- secondary workloads, measured in the same run (rank 0, N=1): the deflated / recycling loops of
    # config 5 on the same 1M-DoF operators, and config 2 (full-A Jacobi-PCG at 250k DoF)
    secondary = None
    if rank == 0 and world == 1 and not args.no_secondary:
        secondary = secondary_measurements(args, api, fem, ctx, S, M, b_dev, n_Γ, ndom, bytes_dom + bytes_nn, e0, e1)
        try:
            secondary["device_setup_per_realization"] = setup_measurement(api, ctx, P, S, M)
        except Exception as e:   # noqa: BLE001
            secondary["device_setup_per_realization"] = {"error": f"{type(e).__name__}: {e}"}
        try:
            secondary["config5"] = config5_measurement(args, api, fem, ctx, mesh, P, f, uex, nreals=args.config5_reals)
        except Exception as e:   # noqa: BLE001
            secondary["config5"] = {"error": f"{type(e).__name__}: {e}"}

    # ---------------- CPU baseline: the oracle (C restatement) on this box's host cores, rank 0, N=1 only
    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        from oracle import oracle as orc
        # the box shows every logical CPU of the host but a 1-GPU job owns a 16-core share
        cores = orc.set_threads(min(len(os.sched_getaffinity(0)), 16))
        So = orc.apply_local_schurs_operator(P.Sd, P.sub.gather_idx, n_Γ)
        Mo = orc.neumann_neumann_operator(P.ΠSd, P.sub.gather_idx, P.sub.node_Γ_cnt)
        xo, ito, reso = orc.pcg(So, b_host, np.zeros(n_Γ), Mo, eps=args.eps)   # also the parity check of this run
        assert ito == its, f"GPU it={its} but oracle it={ito}"
        assert np.allclose(res, reso, rtol=1e-8, atol=1e-12 * reso[0])
        nsolve, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < 10.0:
            orc.pcg(So, b_host, np.zeros(n_Γ), Mo, eps=args.eps)
            nsolve += 1
        tc = time.perf_counter() - t0
        cpu = {"value": round(nsolve * (ito - 1) / tc, 2), "unit": "iterations/s", "cores": cores, "kind": "port",
               "sample": f"{nsolve} full NN-PCG solves of the same 1M-DoF Schur system in {tc:.1f}s "
                         "(C restatement of cg.jl/EPDD.jl, OpenMP row-parallel GEMV; not Julia)"}

    return roofline, secondary, cpu


if __name__ == "__main__":
    main()
