#!/usr/bin/env python3
"""Example07_PcgSchurStochasticEllipticPde.jl (lines 56-285; with --gg also the second loop, 290-424) on the MI355X
drop-in — BASELINE config 5.

For every realization ξ_t of the lognormal coefficient: rebuild the local blocks, b_schur, the assembled
S_d and NN_t on the host (as the reference does), then on the GPU
    pcg(S, b_schur, 0, ΠSnn_0)        (Example07:273)   preconditioner of the ξ = 0 operator, built once
    pcg(S, b_schur, 0, ΠSnn_t)        (Example07:277)   preconditioner of this realization
    defpcg(S, b_schur, 0, W_0, ΠSnn_0)                  deflation with the nev least-dominant eigenvectors of
                                                        S_0 (the `defpcg` variant that Example07 keeps in its
                                                        trailing comment block, with W fixed instead of recycled)
    eigpcg / eigdefpcg(S, b_schur, 0, ΠSnn_0, W, spdim)   (--recycle) BASELINE config 5's "deflated Schur-PCG with
                                                        recycled W": the first system runs eigpcg, every later one
                                                        eigdefpcg with the W the previous solve returned
                                                        (Example09_..._Functions.jl:345, 364; nvec = 1.25 ndom,
                                                        spdim = 3 ndom), the chain being per rank
and record the iteration counts. With --gg, also the second loop's solves preconditioned by the interface block itself
    pcg(S, b_schur, 0, A_ΓΓ_0)        (Example07:412)   A_ΓΓ of the ξ = 0 operator
    pcg(S, b_schur, 0, A_ΓΓ_t)        (Example07:416)   A_ΓΓ of this realization
with `M \\ r` by the device sparse direct solve (api.SparseDirectPreconditioner, refilled per realization by set_values:
from `prepare_global_schur` on the host, or with --device-setup from the device assembly through fem.gamma_gather_map).
With --matrix-free-amg, also
    pcg(S_t, b_schur, 0, ΠSnn_0)      S_t matrix-free: apply_local_schurs with `cg(A_IId, rhs; Pl = Π_IId, reltol)` inside
                                      (EPDD.jl:648-650), Π_IId the AMG preconditioner Example07:174 rebuilds per
                                      realization — here one hierarchy of blockdiag(A_IIdd) on the device
                                      (MatrixFreeLocalSchurs.interior_amg), its numbers redone by set_values
Realizations are independent: under torch.distributed.run each rank takes
realizations rank, rank+world, ... on its own GPU (replicas only, no collective in the solve).

With --device-assembly the element loop of `prepare_local_schurs` (Example07:162-171, redone per realization by the
reference) runs on the GPU: the index half is prepared once (`fem.make_assembly_plan`), each realization is one
`mi_assembly_run` (0.2 ms at 1 M DoF vs ~1-3 s for the host loop); the block values come back for the dense
elimination that builds S_d.

With --device-setup the dense elimination, the condensed rhs and NN_t run on the device too, and with --device-field the
coefficient itself: one api.KLField keeps Ψ on the device, per realization only the latent vector ξ is uploaded and
a = exp(g(ξ)) goes straight into the assembly (g has the bits of fem.draw's loop, so the iteration counts do not change).

    python examples/example07_stochastic.py [--N 200 --px 4 --py 2 --nreals 20 --device-assembly --device-setup --device-field]
"""
import argparse
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--px", type=int, default=4)
    ap.add_argument("--py", type=int, default=2)
    ap.add_argument("--nreals", type=int, default=20)   # Example07:29 nreals = 1000
    ap.add_argument("--seed", type=int, default=481456)
    ap.add_argument("--out", default="")
    ap.add_argument("--device-assembly", action="store_true")
    ap.add_argument("--device-setup", action="store_true",
                    help="with --device-assembly: S_d, the condensed rhs and NN_t on the device too (mi_schur_setup_run, mi_nn_pinv, "
                         "mi_dense_set_blocks): nothing of a realization's set-up runs on the host")
    ap.add_argument("--device-field", action="store_true",
                    help="with --device-setup: the coefficient itself on the device too (api.KLField): per realization only the latent "
                         "vector ξ (m numbers) is uploaded, a = exp(g(ξ)) goes straight into the device assembly")
    ap.add_argument("--recycle", action="store_true")
    ap.add_argument("--nn-f32", action="store_true",
                    help="run the two solves of Example07:273-277 also with fp32-STORED Neumann-Neumann blocks (storage=\"f32\": "
                         "half the preconditioner's bytes, all arithmetic fp64) and print both count vectors side by side")
    ap.add_argument("--kl", default="", help="root file name of KL modes written by examples/example04_kl.py (Example07:124-125 reads "
                                             "data/$root_fname.kl-eigvals.npz / .kl-eigvecs.npz); default: fem.synthetic_kl")
    ap.add_argument("--kl-dir", default="data")
    ap.add_argument("--matrix-free-amg", action="store_true",
                    help="also pcg(S_t, b_schur, 0, ΠSnn_0) with S_t matrix-free, its interior CG preconditioned by the AMG `Pl` "
                         "(interior_amg; set_values refreshes the hierarchy on the device every realization)")
    ap.add_argument("--gg", action="store_true", help="also pcg(S, b_schur, 0, A_ΓΓ_0) and pcg(S, b_schur, 0, A_ΓΓ_t) (Example07:412, 416)")
    args = ap.parse_args()
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    pkg = graft.load_package()
    fem, api = pkg.fem, pkg.api
    f = lambda x, y: -1.0 + 0 * x
    uexact = lambda x, y: 0.734 + 0 * x
    mesh = fem.get_mesh(args.N)
    if args.kl:
        kl = fem.SyntheticKL(*pkg.io.load_kl(args.kl, args.kl_dir))
        if kl.Ψ.shape[0] != mesh.points.shape[1]:
            raise SystemExit(f"--kl: modes on {kl.Ψ.shape[0]} nodes, the mesh has {mesh.points.shape[1]} (run example04_kl.py with --N {args.N})")
    else:
        kl = fem.synthetic_kl(mesh.points)
    rng = np.random.default_rng(args.seed)
    draws = [fem.draw(kl, rng) for _ in range(args.nreals)]          # Example07:140-144: all draws up front
    ξs, gs = [d[0] for d in draws], [d[1] for d in draws]

    ctx = api.Context(int(os.environ.get("LOCAL_RANK", "0")))
    P0 = fem.build_schur_problem(args.N, args.px, args.py, np.exp(0 * gs[0]), f, uexact)   # ξ = 0 operator (:88-137)
    sub = P0.sub
    n_Γ, ndom = sub.n_Γ, sub.ndom
    ΠSnn_0 = api.NeumannNeumannSchurPreconditioner(ctx, P0.ΠSd, sub.gather_idx, sub.node_Γ_cnt)      # :152-154
    S_0 = api.LocalSchurs(ctx, P0.Sd, sub.gather_idx, sub.node_Γ_cnt)
    S0d = np.column_stack([S_0 * e for e in np.eye(n_Γ)])
    W_0 = np.asfortranarray(np.linalg.eigh((S0d + S0d.T) / 2)[1][:, :ndom + 10])

    plan = dev_plan = None
    if args.device_assembly:
        plan = fem.make_assembly_plan(mesh.cells, mesh.points, P0.epart, sub, f, uexact)
        dev_plan = api.AssemblyPlan(ctx, plan)
    setup = S_dev = NN_dev = None
    if args.device_setup:
        if not args.device_assembly:
            raise SystemExit("--device-setup needs --device-assembly")
        import torch
        setup = api.SchurSetup(ctx, P0.A_IIdd, P0.A_IΓdd, P0.A_ΓΓdd)
        S_dev = api.LocalSchurs(ctx, P0.Sd, sub.gather_idx, sub.node_Γ_cnt)
        NN_dev = api.NeumannNeumannSchurPreconditioner(ctx, P0.ΠSd, sub.gather_idx, sub.node_Γ_cnt)
    field = None
    if args.device_field:
        if not args.device_setup:
            raise SystemExit("--device-field needs --device-assembly --device-setup")
        field = api.KLField(ctx, kl.Λ, kl.Ψ)                 # Ψ crosses once; `set!(Λ, Ψ, ξ, g)` and exp.(g) per realization on the device
    ΠSnn_0_f32 = NN_dev_f32 = None
    if args.nn_f32:
        ΠSnn_0_f32 = api.NeumannNeumannSchurPreconditioner(ctx, P0.ΠSd, sub.gather_idx, sub.node_Γ_cnt, storage="f32")
        if args.device_setup:
            NN_dev_f32 = api.NeumannNeumannSchurPreconditioner(ctx, P0.ΠSd, sub.gather_idx, sub.node_Γ_cnt, storage="f32")
    iters_0_f32, iters_t_f32 = [], []
    M_gg0 = M_ggt = gmap = None
    if args.gg:   # Example07:290-300: A_ΓΓ_0 of the ξ = 0 operator; A_ΓΓ_t on the same pattern, refilled per realization
        A_gg0 = sp.csc_matrix(fem.prepare_global_schur(mesh.cells, mesh.points, P0.epart, sub, np.exp(0 * gs[0]), f, uexact)[2])
        A_gg0.sort_indices()
        M_gg0 = api.SparseDirectPreconditioner(ctx, A_gg0)
        M_ggt = api.SparseDirectPreconditioner(ctx, A_gg0)
        if args.device_setup:
            gmap = fem.gamma_gather_map(plan.patterns["ΓΓ"], sub.gather_idx, n_Γ, offsets=[o for o, _ in plan.layout["ΓΓ"]])
            assert np.array_equal(gmap.indptr, A_gg0.indptr) and np.array_equal(gmap.indices, A_gg0.indices)
    S_mf, iters_mf = None, []
    if args.matrix_free_amg:
        S_mf = api.MatrixFreeLocalSchurs(ctx, P0.A_IIdd, P0.A_IΓdd, P0.A_ΓΓdd, sub.gather_idx, sub.node_Γ_cnt, None, reltol=1e-9)
        print(f"[rank {rank}] interior AMG: {S_mf.interior_amg(P0.A_IIdd)}", flush=True)

    def csc_values(mats):
        return np.concatenate([np.asarray(sp.csc_matrix(A).sorted_indices().data, dtype=np.float64) for A in mats])

    iters_0, iters_t, iters_def, iters_rec, iters_gg0, iters_ggt = [], [], [], [], [], []
    W_rec, nvec, spdim = None, int(1.25 * ndom), 3 * ndom
    for ireal in range(rank, args.nreals, world):
        if setup is not None:
            # the whole realization on the device: element loop -> block values -> S_d, w_d -> operators refilled
            a_t = field.coefficient(torch.from_numpy(ξs[ireal]).cuda()) if field is not None else torch.from_numpy(np.exp(gs[ireal])).cuda()
            vals = dev_plan.run(a_t)
            ii, ig, gg, bI, bΓ = dev_plan.block_values(vals)
            Sd, w = setup.run(ii, ig, gg, bI)                                                          # :180-187
            S_dev.set_blocks(Sd)
            Πd = api.nn_pinv(ctx, sub.n_Γd, Sd)                                                        # :190-199
            NN_dev.set_blocks(Πd)
            if NN_dev_f32 is not None:
                NN_dev_f32.set_blocks(Πd)                                                              # (rounded to fp32 on the way in)
            ctx.synchronize()
            b_schur, wh, off = bΓ.cpu().numpy().copy(), w.cpu().numpy(), 0
            for d in range(ndom):                                                                      # get_schur_rhs, EPDD.jl:853-861
                b_schur[sub.gather_idx[d]] -= wh[off:off + sub.n_Γd[d]]
                off += sub.n_Γd[d]
            S, ΠSnn_t, ΠSnn_t_f32 = S_dev, NN_dev, NN_dev_f32
            if M_ggt is not None:
                M_ggt.set_values(gmap.values(vals))                                                    # A_ΓΓ_t = Σ_d R_d' A_ΓΓdd R_d
            if S_mf is not None:
                S_mf.set_values(ii, ig, gg)                                                            # :162-174 without a host trip
        else:
            blocks = plan.blocks(dev_plan.run(np.exp(gs[ireal]))) if plan else None                   # :162-171 on the GPU
            P = fem.build_schur_problem(args.N, args.px, args.py, np.exp(gs[ireal]), f, uexact, mesh=mesh,
                                        partition=(P0.epart, None), blocks=blocks, sub=sub)      # :162-199
            S = api.LocalSchurs(ctx, P.Sd, sub.gather_idx, sub.node_Γ_cnt)
            ΠSnn_t = api.NeumannNeumannSchurPreconditioner(ctx, P.ΠSd, sub.gather_idx, sub.node_Γ_cnt)
            ΠSnn_t_f32 = (api.NeumannNeumannSchurPreconditioner(ctx, P.ΠSd, sub.gather_idx, sub.node_Γ_cnt, storage="f32")
                          if args.nn_f32 else None)
            b_schur = P.b_schur
            if M_ggt is not None:
                A_ggt = sp.csc_matrix(fem.prepare_global_schur(mesh.cells, mesh.points, P0.epart, sub, np.exp(gs[ireal]), f, uexact)[2])
                A_ggt.sort_indices()
                M_ggt.set_values(A_ggt.data)
            if S_mf is not None:
                S_mf.set_values(csc_values(P.A_IIdd), csc_values(P.A_IΓdd), csc_values(P.A_ΓΓdd))
        x0 = np.zeros(n_Γ)
        iters_0.append(api.pcg(S, b_schur, x0, ΠSnn_0)[1])                                            # :273
        iters_t.append(api.pcg(S, b_schur, x0, ΠSnn_t)[1])                                            # :277
        iters_def.append(api.defpcg(S, b_schur, x0, W_0, ΠSnn_0)[1])
        mf = ""
        if S_mf is not None:
            i0 = S_mf.interior_iterations()
            iters_mf.append(api.pcg(S_mf, b_schur, x0, ΠSnn_0)[1])
            mf = f"  matrix-free S_t, AMG Pl: pcg(NN_0) it={iters_mf[-1]} ({S_mf.interior_iterations() - i0} interior iterations)"
        f32 = ""
        if args.nn_f32:
            iters_0_f32.append(api.pcg(S, b_schur, x0, ΠSnn_0_f32)[1])
            iters_t_f32.append(api.pcg(S, b_schur, x0, ΠSnn_t_f32)[1])
            f32 = f"  fp32-stored: pcg(NN_0) it={iters_0_f32[-1]}  pcg(NN_t) it={iters_t_f32[-1]}"
            if ΠSnn_t_f32 is not NN_dev_f32:
                ΠSnn_t_f32.close()                       # host route: one operator per realization
        rec = ""
        if args.recycle:
            try:
                if W_rec is None:
                    _, it, _, W_rec = api.eigpcg(S, b_schur, x0, ΠSnn_0, nvec, spdim)
                else:
                    _, it, _, W_rec = api.eigdefpcg(S, b_schur, x0, ΠSnn_0, W_rec, spdim)
                iters_rec.append(it)
                rec = f"  eig(def)pcg(W recycled, NN_0) it={it}"
            except (api.BoundsError, api.SingularException) as e:          # Example09:355-375: status = -1
                rec = f"  recycling stopped: {type(e).__name__}"
                W_rec = None
        gg = ""
        if M_gg0 is not None:
            iters_gg0.append(api.pcg(S, b_schur, x0, M_gg0)[1])                                       # :412
            iters_ggt.append(api.pcg(S, b_schur, x0, M_ggt)[1])                                       # :416
            gg = f"  pcg(A_GG_0) it={iters_gg0[-1]}  pcg(A_GG_t) it={iters_ggt[-1]}"
        print(f"[rank {rank}] realization {ireal}: pcg(NN_0) it={iters_0[-1]}  pcg(NN_t) it={iters_t[-1]}  "
              f"defpcg(W_0, NN_0) it={iters_def[-1]}{mf}{f32}{rec}{gg}", flush=True)
    if args.out:                                                                                       # :281-285 npz of iteration counts
        np.savez(args.out.format(rank=rank), iters_0=iters_0, iters_t=iters_t, iters_def=iters_def, iters_rec=iters_rec,
                 iters_gg0=iters_gg0, iters_ggt=iters_ggt, iters_mf=iters_mf)                                          # (:423-424: io.save_pcg_iters(..., precond="A_GG"))
    if args.nn_f32:
        for tag, i64_, i32_ in (("NN_0", iters_0, iters_0_f32), ("NN_t", iters_t, iters_t_f32)):
            print(f"nn-f32 {tag}: fp64 [{' '.join(map(str, i64_))}] fp32 [{' '.join(map(str, i32_))}]")
            if args.out:
                pkg.io.save_pcg_iters(i32_, f"example07_N{args.N}_rank{rank}", ndom, tag, len(i32_),
                                      data_dir=os.path.dirname(args.out.format(rank=rank)) or ".", precond="neumann-neumann-f32")
    print(f"[rank {rank}] mean its: NN_0 {np.mean(iters_0):.1f}  NN_t {np.mean(iters_t):.1f}  def {np.mean(iters_def):.1f}"
          + (f"  A_GG_0 {np.mean(iters_gg0):.1f}  A_GG_t {np.mean(iters_ggt):.1f}" if iters_gg0 else ""))


if __name__ == "__main__":
    main()
