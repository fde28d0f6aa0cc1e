#!/usr/bin/env python3
"""Example03_EllipticPdeDomainDecomposition.jl (lines 45-225) on the MI355X drop-in.

Same flow and prints as the reference script; only the operator construction goes through the
device library. Mesh/partition are the structured substitutes (no Triangle / METIS here), the
interior solves of the set-up are direct, the least-dominant eigenvectors come from a dense `eigh`
on the host instead of KrylovKit (Example03:209).

    python examples/example03_domain_decomposition.py [--N 100 --px 2 --py 2] [--lorasc] [--nn-induced {reference,assembled}]
                                                      [--device-eigs]

`--lorasc` adds Example03:245-256: `prepare_lorasc_precond` (host, dense generalized eigenpairs of (S, A_ΓΓ)) and
`pcg(A, b, zeros, ΠA_lorasc)` with the device LORASC preconditioner.

`--device-eigs` takes every eigenpair from the device eigensolver instead (thick-restart Lanczos, `api.eigsolve` /
`api.geneigsolve`): the `ld` / `md` bases of Example03:209/219 from `S_local_mat`, the LORASC pairs of EPDD.jl:1546-1549 from
the pencil `(S_local_mat, A_ΓΓ)` with `chol_A_ΓΓ` as the inverse, and `Arpack.eigs(A, nev, :SM)` (Example03:311) as the
largest eigenvalues θ of `A \\ b` (`BlockJacobiPreconditioner(ctx, 1, A)`), λ = 1/θ. The printed iteration counts are those
of the default path.

`--nn-induced` adds Example03:300-319: `prepare_neumann_neumann_induced_precond`, then `defpcg(A, b, ϕ, M=ΠA_induced_nn)`
with the least dominant eigenvectors of A and `pcg(A, b, M=ΠA_induced_nn)` on the full system. `reference` is the
preconditioner as the reference applies it (EPDD.jl:2411: neither symmetric nor positive definite, "only seems to work with
deflation"), `assembled` its symmetric positive definite form. ϕ is `lowest_eigvecs(A, ndom + 10)`: where the cut at
ndom + 10 falls inside a repeated eigenvalue (the x <-> y symmetry of a square box partition gives pairs), the whole
eigenspace is taken, so that the deflation space, and with it the printed `iter`, does not depend on the basis the
eigensolver happens to return inside that eigenspace.
"""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100)      # tentative_nnode = N*N (Example03:16: 40_000)
    ap.add_argument("--px", type=int, default=2)
    ap.add_argument("--py", type=int, default=2)       # ndom = px*py (Example03:19: 20)
    ap.add_argument("--lorasc", action="store_true", help="also run the LORASC leg, Example03:245-256")
    ap.add_argument("--nn-induced", choices=("reference", "assembled"), default=None,
                    help="also run the Neumann-Neumann induced leg, Example03:300-319, with this coupling (EPDD.jl:2411)")
    ap.add_argument("--device-eigs", action="store_true",
                    help="eigenpairs from the device eigensolver (api.eigsolve / api.geneigsolve) instead of the dense host detour")
    return ap.parse_args(argv)


def lowest_eigvecs(A, nev, extra=6, rtol=1e-8):
    """The eigenvectors of the `nev` smallest eigenvalues of the SPD matrix A (Arpack.eigs(A, nev, :SM), Example03:311),
    by shift-invert Lanczos at 0. An eigenvalue equal (to `rtol`) to the `nev`-th brings its eigenvectors along, up to
    `extra` more: cutting through an eigenspace would leave the span of ϕ to the solver's choice of basis in it."""
    lam, V = spla.eigsh(sp.csc_matrix(A), k=min(nev + extra, A.shape[0] - 1), sigma=0.0, which="LM")
    order = np.argsort(lam)
    lam, V = lam[order], V[:, order]
    m = nev
    while m < lam.size and lam[m] - lam[nev - 1] <= rtol * lam[nev - 1]:
        m += 1
    return np.asfortranarray(V[:, :m])


def lowest_eigvecs_device(api, ctx, A, nev, extra=6, rtol=1e-8, tol=1e-8):
    """The same space from the device: Arpack.eigs(A, nev, :SM) as the nev + extra LARGEST eigenvalues θ of A^-1, applied
    exactly by the block-Jacobi preconditioner with one block (`A \\ b`); λ = 1/θ. The cut follows lowest_eigvecs."""
    Ainv = api.BlockJacobiPreconditioner(ctx, 1, sp.csc_matrix(A))
    k = min(nev + extra, A.shape[0] - 1)
    θ, V, info = api.eigsolve(Ainv, k, "LR", krylovdim=2 * k, tol=tol, maxiter=200)   # tol is absolute: θ = 1/λ is O(1e2 .. 1e3) here
    Ainv.close()
    lam = 1.0 / θ                                       # ascending, as θ is descending
    print(f"device eigsolve(A^-1, {k}, LR): converged {info.converged}, restarts {info.numiter}, applies {info.numops}")
    m = nev
    while m < lam.size and lam[m] - lam[nev - 1] <= rtol * lam[nev - 1]:
        m += 1
    return np.asfortranarray(V[:, :m])


def main(argv=None):
    args = parse_args(argv)
    pkg = graft.load_package()
    fem, api = pkg.fem, pkg.api
    a = lambda x, y: 1.0 + 0 * x                        # Example03:63-65
    f = lambda x, y: -1.0 + 0 * x                       # Example03:67-69
    uexact = lambda x, y: 0.734 + 0 * x                 # Example03:71-73

    t = time.time()
    P = fem.build_schur_problem(args.N, args.px, args.py, a, f, uexact)
    sub, mesh = P.sub, P.mesh
    n_Γ, ndom = sub.n_Γ, sub.ndom
    print(f"nnode = {mesh.points.shape[1]}\nnel = {mesh.cells.shape[1]}\nset-up {time.time() - t:.2f}s, n_Γ = {n_Γ}")

    ctx = api.Context(0)
    A, b = fem.do_isotropic_elliptic_assembly(mesh.cells, mesh.points, P.dinds, mesh.point_marker, a, f, uexact)
    A_IId, A_IΓd, A_ΓΓ, b_Id, b_Γ = fem.prepare_global_schur(mesh.cells, mesh.points, P.epart, sub, a, f, uexact)
    S_global = api.GlobalSchur(ctx, A_IId, A_IΓd, A_ΓΓ, P.solvers)                                     # Example03:101
    S_local_mat = api.LocalSchurs(ctx, P.Sd, sub.gather_idx, sub.node_Γ_cnt)                          # Example03:131-135
    ΠSnn_local_mat = api.NeumannNeumannSchurPreconditioner(ctx, P.ΠSd, sub.gather_idx, sub.node_Γ_cnt)  # :139-141
    S_local = api.MatrixFreeLocalSchurs(ctx, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd, sub.gather_idx, sub.node_Γ_cnt, P.solvers)  # :143-150
    b_schur = P.b_schur

    d = S_global * b_schur - S_local_mat * b_schur                                                    # Example03:175
    print(f"extrema(S_global * b_schur - S_local_mat * b_schur) = ({d.min():.3e}, {d.max():.3e})")
    for name, op in (("S * b_schur (matrix-free)", S_global), ("S_local * b_schur (matrix-free)", S_local),
                     ("S_local_mat * b_schur", S_local_mat)):
        t = time.time(); op * b_schur; print(f"{name} ... {time.time() - t:.6f} seconds")            # :178-183

    u_Γ, it, _ = api.pcg(S_local_mat, b_schur, np.zeros(n_Γ), ΠSnn_local_mat)                         # Example03:193
    print(f"neumann-neumann-pcg: n = {S_local_mat.N}, iter = {it}")
    u_Id = fem.get_subdomain_solutions(u_Γ, A_IId, A_IΓd, b_Id, P.solvers)                            # :197
    u_with_dd = fem.merge_subdomain_solutions(u_Γ, u_Id, sub, P.dinds, uexact, mesh.points)           # :200
    u_no_dd = fem.append_bc(P.dinds, spla.spsolve(sp.csc_matrix(A), b), mesh.points, uexact)          # :111-117 (direct, no AMG)
    e = u_with_dd - u_no_dd
    print(f"extrema(u_with_dd - u_no_dd) = ({e.min():.3e}, {e.max():.3e})")                            # :204

    nev = ndom + 10                                                                                    # :206
    if args.device_eigs:
        t = time.time()
        bases = []
        for which in ("SR", "LR"):                                                                     # Example03:209, :219
            _, ϕ, info = api.eigsolve(S_local_mat, nev, which, krylovdim=2 * nev, tol=1e-10, maxiter=500)
            print(f"device eigsolve(S_local_mat, {nev}, {which}): converged {info.converged}, restarts {info.numiter}, applies {info.numops}")
            bases.append(ϕ)
        print(f"eigsolve (device) ... {time.time() - t:.2f} seconds")
        Sdense = None
    else:
        Sdense = np.column_stack([S_local_mat * col for col in np.eye(n_Γ)])
        lam, V = np.linalg.eigh((Sdense + Sdense.T) / 2)
        bases = [V[:, :nev], V[:, -nev:]]
    for tag, ϕ in zip(("ld", "md"), bases):
        u_Γ, it, _ = api.defpcg(S_local_mat, b_schur, np.zeros(n_Γ), np.asfortranarray(ϕ), ΠSnn_local_mat)  # :214, :224
        print(f"{tag}-def-neumann-neumann-pcg: n = {S_local_mat.N}, ndom = {ndom}, nev = {nev} ({tag}), iter = {it}")

    if args.lorasc:
        t = time.time()
        chol_A_ΓΓ = api.SparseDirectPreconditioner(ctx, A_ΓΓ)                                         # cholesky(A_ΓΓ), EPDD.jl:1525
        if args.device_eigs:                                                                           # EPDD.jl:1546-1549
            A_ΓΓ_dev = api.SparseMatrixCSC(ctx, A_ΓΓ)
            E, Σ = fem.prepare_lorasc_precond(None, A_ΓΓ, eigs=lambda k: api.geneigsolve(
                S_local_mat, A_ΓΓ_dev, chol_A_ΓΓ, k, "SR", krylovdim=2 * k, tol=1e-10, maxiter=500)[:2])
        else:
            E, Σ = fem.prepare_lorasc_precond(Sdense, A_ΓΓ)                                            # Example03:246-252
        setup = api.SchurSetup(ctx, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd)                                      # cholesky(A_IId), EPDD.jl:1535-1537
        setup.keep_levels()
        setup.run()
        ΠA_lorasc = api.LorascPreconditioner(ctx, A_IΓd, (sub, P.dinds), setup, chol_A_ΓΓ, E)
        print(f"prepare_lorasc_precond ... {time.time() - t:.2f} seconds, nev = {E.shape[1]}")
        A_dev = api.SparseMatrixCSC(ctx, A)
        u, it, _ = api.pcg(A_dev, b, np.zeros(b.size), ΠA_lorasc)                                      # Example03:255
        print(f"lorasc-pcg: n = {A.shape[0]}, ndom = {ndom}, iter = {it}")                             # :256
        e = fem.append_bc(P.dinds, u, mesh.points, uexact) - u_no_dd
        print(f"extrema(u_lorasc - u_no_dd) = ({e.min():.3e}, {e.max():.3e})")

    if args.nn_induced:
        t = time.time()
        ΠSd = fem.prepare_neumann_neumann_induced_precond(P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd)                # Example03:299-308
        setup = api.SchurSetup(ctx, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd)                                      # cholesky(A_IIdd), EPDD.jl:2340
        setup.keep_levels()
        setup.run()
        ΠA_induced_nn = api.NeumannNeumannInducedPreconditioner(ctx, P.A_IΓdd, (sub, P.dinds), sub.gather_idx, sub.node_Γ_cnt,
                                                                ΠSd, setup, coupling=args.nn_induced)
        print(f"prepare_neumann_neumann_induced_precond ... {time.time() - t:.2f} seconds")
        A_dev = api.SparseMatrixCSC(ctx, A)
        ϕ = lowest_eigvecs_device(api, ctx, A, nev) if args.device_eigs else lowest_eigvecs(A, nev)    # Example03:311
        u, it, _ = api.defpcg(A_dev, b, np.zeros(b.size), ϕ, ΠA_induced_nn)                            # Example03:313
        print(f"nn-induced-defpcg: n = {A.shape[0]}, ndom = {ndom}, nev = {ϕ.shape[1]}, coupling = {args.nn_induced}, iter = {it}")
        u, it, _ = api.pcg(A_dev, b, np.zeros(b.size), ΠA_induced_nn)                                  # Example03:317
        print(f"nn-induced-pcg: n = {A.shape[0]}, ndom = {ndom}, coupling = {args.nn_induced}, iter = {it}")   # :318
        e = fem.append_bc(P.dinds, u, mesh.points, uexact) - u_no_dd
        print(f"extrema(u_nn_induced - u_no_dd) = ({e.min():.3e}, {e.max():.3e})")


if __name__ == "__main__":
    main()
