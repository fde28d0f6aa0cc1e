#!/usr/bin/env python3
"""Example16_McmcRealizations.jl:63-88 on the MI355X drop-in: one Metropolis chain on the latent vector of the lognormal
coefficient (`prepare_mcmc_sampler`, `draw!`, Fem/Samplers.jl:130-199), keeping the coefficient `exp.(sampler.g)` at the
start and the first time the number of proposals reaches each entry of `--nsmp` (the reference's nsmp = (0, 10, 100, 1000)).

The chain itself — m numbers per proposal — stays on the host; the field g(ξ) = Σ_α sqrt(Λ_α) ξ_α Ψ[:, α] and the coefficient
exp(g) of every accepted state come from the device (`api.KLField`): Ψ crosses once, then only ξ. `--host` runs the same
chain with the host loop (`fem.set_field`) instead; equal seeds give equal chains and bit-equal fields. Also printed: the
acceptance ratio n_kept / Σ cnt, accepted states over proposals made.

    python examples/example16_mcmc_realizations.py [--N 100] [--nsmp 0 10 100 1000] [--kl ROOT] [--out DIR] [--host]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402


def sample_chain(sampler, nsmp):
    """Example16:63-82 -> (reals, draws, proposals)"""
    cnt_reals, n_draws = 0, 0
    reals = {0: sampler.a.copy()}
    while nsmp[-1] not in reals:
        cnt_reals += sampler.draw()
        n_draws += 1
        for m in nsmp:
            if m not in reals and cnt_reals >= m:
                reals[m] = sampler.a.copy()
    return reals, n_draws, cnt_reals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100, help="nodes per side")
    ap.add_argument("--nsmp", type=int, nargs="+", default=[0, 10, 100, 1000])
    ap.add_argument("--seed", type=int, default=481456)
    ap.add_argument("--kl", default="", help="root file name of KL modes written by examples/example04_kl.py; default: fem.synthetic_kl")
    ap.add_argument("--kl-dir", default="data")
    ap.add_argument("--out", default="", help="directory for real_mcmc_<m>.npy (Example16:86-88); default: nothing is written")
    ap.add_argument("--host", action="store_true", help="the field on the host (fem.set_field) instead of the device")
    args = ap.parse_args()
    nsmp = sorted(set(args.nsmp) | {0})
    pkg = graft.load_package()
    fem, api = pkg.fem, pkg.api
    mesh = fem.get_mesh(args.N)
    if args.kl:
        Λ, Ψ = pkg.io.load_kl(args.kl, args.kl_dir)
    else:
        kl = fem.synthetic_kl(mesh.points)
        Λ, Ψ = kl.Λ, kl.Ψ
    field = None
    if not args.host:
        ctx = api.Context(int(os.environ.get("LOCAL_RANK", "0")))
        field = api.KLField(ctx, Λ, Ψ)
        print(f"KLField: n = {field.n}, m = {field.m}, {field.stats()['bytes_kept'] / 1e6:.1f} MB kept on the device")
    sampler = api.McmcSampler(Λ, Ψ, np.random.default_rng(args.seed), field=field)
    reals, n_draws, proposals = sample_chain(sampler, nsmp)
    for m in nsmp:
        a = reals[m]
        print(f"real_mcmc_{m}: min {a.min():.4e}  mean {a.mean():.4e}  max {a.max():.4e}")
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            np.save(os.path.join(args.out, f"real_mcmc_{m}.npy"), a)
    print(f"{n_draws} states kept of {proposals} proposals: acceptance ratio n_kept / Σ cnt = {n_draws / proposals:.3f}")


if __name__ == "__main__":
    main()
