"""The cases of tests/test_gpu_full_split.py and tests/golden/make_full_split_golden.py: applies and one solve of the LORASC and
the Neumann-Neumann induced preconditioner on the synthetic partitions of tests/full_synth.py, small on purpose.

Not a conftest. `inputs()` is host only; `run_all(api, fem, ctx)` needs the GPU and goes through the Python API alone, so it
runs unchanged on the commit before the two operators were given one interior/Γ split and on every commit after it.

  lorasc/<case>/nev<k>            ldiv on w1, w3, hub6, bare (nev 0, 3) and wg1, wg256 (nev 0, 3, 257); hub6 with index base 1
  induced/<case>/<storage>/<cpl>  ldiv on w3, hub6, bare, both storages, both couplings; hub6 with index base 1
  solve/lorasc, solve/induced     pcg(A, b, 0, M) on `solve` at the default chunk: x, it, res_norm
  in/<case>, sha/<case>           the input vector of every apply and a SHA-256 of the case's matrices and maps"""
import hashlib

import numpy as np
import scipy.sparse as sp

import full_synth as fs
import lorasc_ref as lr
import nn_induced_ref as nr

LORASC = tuple((name, nev) for name in fs.WIDTH_CASES for nev in (0, 3)) + tuple((name, nev) for name in ("wg1", "wg256") for nev in (0, 3, 257))
INDUCED = tuple((name, sto, cpl) for name in ("w3", "hub6", "bare") for sto in ("f64", "f32") for cpl in nr.COUPLINGS)
BASE1 = "hub6"
SOLVE = "solve"
SOLVE_NEV = 3
GRID_BITS = 20


def on_grid(B):
    """the symmetric part of B rounded to multiples of 2^-GRID_BITS of its largest entry: the pseudo-inverses of `solve` come
    from LAPACK, whose last bits may differ between two hosts; on the grid they are the same matrix on both"""
    B = (np.asarray(B) + np.asarray(B).T) / 2
    q = 2.0 ** (np.floor(np.log2(np.max(np.abs(B)))) - GRID_BITS)
    return np.asfortranarray(np.round(B / q) * q)


def blocks(fem, c):
    ΠSd = nr.prepare(fem, c)
    return [on_grid(B) for B in ΠSd] if c.name == SOLVE else ΠSd


def digest(fem, c):
    h = hashlib.sha256()

    def add(a, dtype):
        h.update(np.ascontiguousarray(np.asarray(a, dtype=dtype)).tobytes())
    for M in list(c.P.A_IIdd) + list(c.P.A_IΓdd) + list(c.P.A_ΓΓdd) + list(c.A_IΓd) + [c.A_ΓΓ, sp.csc_matrix(c.A)]:
        M = sp.csc_matrix(M)
        M.sort_indices()
        add(M.shape, np.int64); add(M.indptr, np.int64); add(M.indices, np.int64); add(M.data, np.float64)
    for p in list(c.pos_I) + [c.pos_Γ] + list(c.P.sub.gather_idx) + [c.P.sub.node_Γ_cnt]:
        add(p, np.int64)
    for B in blocks(fem, c):
        add(B, np.float64)
    add(c.b, np.float64)
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def case_names():
    return tuple(dict.fromkeys([n for n, _ in LORASC] + [n for n, _, _ in INDUCED] + [SOLVE]))


def inputs(fem):
    """in/<case> and sha/<case> of every case: what the device results depend on, computed on the host"""
    out = {}
    for name in case_names():
        c = fs.case(name)
        out[f"sha/{name}"] = digest(fem, c)
        if name != SOLVE:
            out[f"in/{name}"] = nr.apply_input(c)
    return out


def correction(c, nev):
    return lr.apply_inputs(c, nev, False)[1]


def run_all(api, fem, ctx):
    out, setups = {}, {}

    def setup(name):
        if name not in setups:
            P = fs.case(name).P
            s = api.SchurSetup(ctx, P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd)
            s.keep_levels()
            s.run()
            setups[name] = s
        return setups[name]

    def lorasc(c, nev):
        gg = api.SparseDirectPreconditioner(ctx, c.A_ΓΓ)
        return api.LorascPreconditioner(ctx, c.A_IΓd, (c.pos_I, c.pos_Γ), setup(c.name), gg, correction(c, nev),
                                        index_base=int(c.name == BASE1))

    def induced(c, sto, cpl):
        sub = c.P.sub
        return api.NeumannNeumannInducedPreconditioner(ctx, c.P.A_IΓdd, (c.pos_I, c.pos_Γ), sub.gather_idx, sub.node_Γ_cnt,
                                                       blocks(fem, c), setup(c.name), storage=sto, coupling=cpl,
                                                       index_base=int(c.name == BASE1))
    for name, nev in LORASC:
        c = fs.case(name)
        M = lorasc(c, nev)
        out[f"lorasc/{name}/nev{nev}"] = M.ldiv(nr.apply_input(c))
        M.close()
    for name, sto, cpl in INDUCED:
        c = fs.case(name)
        M = induced(c, sto, cpl)
        out[f"induced/{name}/{sto}/{cpl}"] = M.ldiv(nr.apply_input(c))
        M.close()
    c = fs.case(SOLVE)
    A = api.SparseMatrixCSC(ctx, c.A)
    for kind, M in (("lorasc", lorasc(c, SOLVE_NEV)), ("induced", induced(c, "f64", "assembled"))):
        x, it, res = api.pcg(A, c.b, np.zeros(c.n), M, 0, fs.EPS)
        out[f"solve/{kind}/x"], out[f"solve/{kind}/it"], out[f"solve/{kind}/res_norm"] = np.asarray(x), np.int64(it), np.asarray(res)
        M.close()
    A.close()
    for s in setups.values():
        s.close()
    return out
