"""GPU suite (-m gpu) of the numeric set-up chain of the smoothed-aggregation hierarchy (csrc/amg_setup.hpp: k_as_gersh,
k_as_omega, k_as_prolong, k_as_gather, k_as_product, k_as_sym, k_as_dense, k_as_sym_dense, driven by AmgPlanOp::refresh
through mi_amg_plan_create and mi_amg_set_values), bit for bit against `amg_setup_synth.setup_bits`, the chain restated on
the host in the device's order of operations. The cases, their matrices and their aggregates are those of
tests/amg_setup_synth.py; tests/test_amg_setup_edges_cpu.py asserts on the host that each has the shape it is named for,
that the restatement lies within the level bounds of a longdouble chain, and that the fault each case is there for changes
at least one bit of what is read back here.

Bars, for every case: created on A0 with the frozen aggregates, then `set_values(A1)`, then `set_values(A0)`:
  * `device_hierarchy()` after each step equals `setup_bits` under np.array_equal — the values of every A_l and P_l on equal
    indptr and indices, every (ω/d)_l, ω_l as a float — and every A_{l+1} is exactly symmetric; the third step restores the
    bits of the first, the coarse inverse included; an operator created from 1-based arrays reads back the same bits.
  * R is not read back: `M.ldiv(r)` equals `amg_synth.cycle_bits(hierarchy read back, r)` bit for bit for the right-hand
    sides of tests/test_gpu_amg_edges.py (a wrong k_as_gather shows in A_{l+1} and here).
  * the coarse inverse (the blocked Gauss-Jordan of setup_gj.hpp, not restated) keeps the bar of amg_refresh_ref.check_coarse
    against numpy on the device's own A_L, and is exactly symmetric.
The mesh pairs of tests/test_gpu_amg_refresh.py (N = 12 with 1, 2 and 3 levels, 34, 100) are held to the same bits. A failure
that arises on level 1 (tests/amg_setup_synth.breakdown) raises MI_ERR_SINGULAR and leaves the hierarchy, the apply and a solve
replayed from the graphs captured before it with their previous bits.

Measured on an MI355X (printed by the tests before they assert): 860 comparisons (arrays of the hierarchies read back and
applies) over the 32 synthetic cases and the five mesh cases, all bit-identical; no quantity needed a bound and no kernel was
changed. Coarse inverse: condition numbers 1 to 4.6e4, ||I - Z A||_F 0.87 to 2.47 times numpy's (bar 8). The file takes 5.1 s,
its slowest case (search) 0.55 s. DESIGN §6g "Refresh" has the sensitivity runs.
"""
import numpy as np
import pytest

import amg_refresh_ref as rr
import amg_setup_synth as sz
import amg_synth as az

pytestmark = pytest.mark.gpu


def _held(M, B, tag, aggs, A):
    """the hierarchy read back now against the restatement B, the apply against cycle_bits of what was read back; returns
    (the hierarchy, the applies, the number of comparisons)"""
    H = M.device_hierarchy()
    n, bad = sz.compare(H, B, tag)
    if bad and aggs:                                         # how far off, in units of the level bounds
        try:
            print(f"{tag}: against the longdouble chain:", sz.check_ld(H, aggs, sz.setup_ld(A, aggs, B), tag))
        except AssertionError as e:
            print(f"{tag}: outside the level bounds: {e}")
    assert not bad, f"{tag}: the device set-up is not the host order bit for bit: {bad} (see the lines printed above)"
    outs = []
    for k, r in enumerate(az.rhs(tag.split()[0], H.sizes[0])):
        got, want = M.ldiv(r), az.cycle_bits(H, r)
        n += 1
        assert np.isfinite(got).all() and np.array_equal(got, want), (tag, "apply", k, int((got != want).sum()))
        outs.append(got)
    return H, outs, n


@pytest.mark.parametrize("name", sz.NAMES)
def test_setup_bit_for_bit(pkg, ctx, fem, name):
    api = pkg.api
    A0, A1, aggs = sz.case(name, fem)
    M = api.AMGPreconditioner(ctx, A0, device_setup=True, aggregates=aggs)
    M1 = None
    try:
        assert [int(a.max()) + 1 for a in aggs] == sz.bits(name, 0, fem=fem).sizes[1:]
        H0, z0, n = _held(M, sz.bits(name, 0, fem=fem), f"{name} (create)", aggs, A0)
        M.set_values(A1)
        H1, z1, m = _held(M, sz.bits(name, 1, fem=fem), f"{name} (set_values)", aggs, A1)
        n += m
        with np.errstate(invalid="ignore", divide="ignore"):     # n_c = 1: both residuals are exactly zero, the printed ratio 0 / 0
            rr.check_coarse(H1, name)
        assert not sz.same_hierarchy(H0, H1)
        M.set_values(A0)
        assert sz.same_hierarchy(M.device_hierarchy(), H0), "set_values(A0) does not restore the first bits"
        assert all(np.array_equal(M.ldiv(r), z) for r, z in zip(az.rhs(name, A0.shape[0]), z0))
        M1 = api.AMGPreconditioner(ctx, A0, index_base=1, device_setup=True, aggregates=aggs)
        assert sz.same_hierarchy(M1.device_hierarchy(), H0), "1-based arrays give other bits"
        print(f"{name} {H0.sizes}: {n} comparisons bit-identical to setup_bits and cycle_bits (create, set_values); restored; 1-based equal")
    finally:
        M.close()
        if M1 is not None:
            M1.close()


MESH = {"N12_1": (12, dict(max_levels=1)), "N12_2": (12, dict(max_levels=2, max_coarse=10)), "N12_3": (12, dict(max_levels=3, max_coarse=4)),
        "N34": (34, {}), "N100": (100, {})}


@pytest.mark.parametrize("case", list(MESH))
def test_mesh_pairs_bit_for_bit(pkg, ctx, fem, case):
    """the pairs of tests/test_gpu_amg_refresh.py (A0 = example01, A1 = lognormal) on the aggregates of the host set-up"""
    N, kw = MESH[case]
    A0, A1, _ = rr.pair(fem, N)
    M = pkg.api.AMGPreconditioner(ctx, A0, device_setup=True, **kw)
    try:
        aggs = M.aggregates
        assert len(aggs) + 1 == {"N12_1": 1, "N12_2": 2, "N12_3": 3, "N34": 2, "N100": 3}[case]
        _, _, n = _held(M, sz.setup_bits(A0, aggs), f"{case} (create)", aggs, A0)
        M.set_values(A1)
        H1, _, m = _held(M, sz.setup_bits(A1, aggs), f"{case} (set_values)", aggs, A1)
        rr.check_coarse(H1, case)
        print(f"{case} {H1.sizes}: {n + m} comparisons bit-identical")
    finally:
        M.close()


@pytest.mark.parametrize("levels", [2, 3])
def test_a_failure_below_level_0_leaves_everything_as_it_was(pkg, ctx, levels):
    """a matrix with a positive diagonal whose level 1 has a negative diagonal entry (asserted on the host by
    tests/test_amg_setup_edges_cpu.py): MI_ERR_SINGULAR naming the diagonal; the hierarchy, the apply and a solve replayed from
    the graphs captured before the call keep their bits; at create the same matrix is refused"""
    api, L = pkg.api, pkg._lib
    A0, bad, aggs = sz.breakdown(levels)
    B = sz.setup_bits(bad, aggs)
    assert (bad.diagonal() > 0).all() and B.A[1].diagonal().min() < 0 and all(np.isfinite(v).all() for v in B.values())
    n = A0.shape[0]
    b = az.rhs("breakdown", n)[0]
    M, Ag = api.AMGPreconditioner(ctx, A0, device_setup=True, aggregates=aggs), api.SparseMatrixCSC(ctx, A0)
    try:
        H0, z0, _ = _held(M, sz.setup_bits(A0, aggs), f"breakdown_{levels} (create)", aggs, A0)
        first = api.pcg(Ag, b, np.zeros(n), M)
        assert np.array_equal(api.pcg(Ag, b, np.zeros(n), M)[0], first[0])       # (replayed)
        with pytest.raises(api.MiError) as e:
            M.set_values(bad)
        print("  refused:", e.value)
        assert e.value.code == L.MI_ERR_SINGULAR and "diagonal" in str(e.value)
        assert sz.same_hierarchy(M.device_hierarchy(), H0)
        assert all(np.array_equal(M.ldiv(r), z) for r, z in zip(az.rhs(f"breakdown_{levels}", n), z0))
        again = api.pcg(Ag, b, np.zeros(n), M)
        assert again[1] == first[1] and np.array_equal(again[0], first[0]) and np.array_equal(again[2], first[2])
        M.set_values(A0)                                          # and the operator still takes good values
        assert sz.same_hierarchy(M.device_hierarchy(), H0)
    finally:
        M.close(); Ag.close()
    with pytest.raises(api.MiError) as e:
        api.AMGPreconditioner(ctx, bad, device_setup=True, aggregates=aggs)
    assert e.value.code == L.MI_ERR_SINGULAR and "diagonal" in str(e.value)
