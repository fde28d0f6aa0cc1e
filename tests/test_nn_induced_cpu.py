"""CPU suite of the Neumann-Neumann induced preconditioner: the host restatement of `apply_neumann_neumann_induced`
(tests/nn_induced_ref.py) — its own noise, the symmetry and definiteness of its two couplings (DESIGN §6d's table), the
block formula of the assembled form, the oracle's iteration counts with the dense restated M^-1 — and the properties of
the inputs that tests/test_gpu_nn_induced.py relies on: the workgroup-edge and GEMV-tile-edge partitions, the hub of the
unstructured mesh. The example's argument parsing."""
import importlib.util
import os

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT, lowest_eigvecs
import nn_induced_ref as nr

SOLVER_CASES = ("micro", "ragged", "unstructured", "strip")
# ||M^-1 - M^-T|| / ||M^-1|| (Frobenius) and the smallest eigenvalue of the symmetric part, coupling as written
AS_WRITTEN = {"micro": (0.23, -3.0e-2), "ragged": (0.48, -4.9), "unstructured": (0.29, -0.37), "strip": (6.9e-3, 0.125)}
# oracle `it` of pcg / defpcg (ϕ = the ndom + 10 lowest eigenvectors of A) with the dense M^-1 as preconditioner
IT_ASSEMBLED = {"micro": (5, 5), "ragged": (10, 10), "unstructured": (17, 17), "strip": (3, 3)}
IT_AS_WRITTEN = {"strip": (5, 4)}


@pytest.fixture(scope="module")
def cases(fem):
    return nr.nni_cases(fem)


@pytest.fixture(scope="module")
def minv(fem, cases):
    """dense M^-1 of the four solver inputs in both couplings, computed once"""
    return {(k, cpl): nr.dense_minv(cases[k], nr.prepare(fem, cases[k]), cpl) for k in SOLVER_CASES for cpl in nr.COUPLINGS}


def test_checker_noise_is_100x_below_the_gpu_bar(fem, cases):
    """on every input of the GPU suite, in both couplings and both storages' blocks, the plain and the refined restatement
    differ by less than 1e-12 ||z||"""
    for c in cases.values():
        ΠSd = nr.prepare(fem, c)
        r = nr.apply_input(c)
        for blocks in (ΠSd, nr.rounded_f32(ΠSd)):
            for cpl in nr.COUPLINGS:
                plain = nr.apply_neumann_neumann_induced(c, blocks, r, cpl, refine=0)
                fine = nr.apply_neumann_neumann_induced(c, blocks, r, cpl, refine=2)
                assert np.linalg.norm(plain - fine) < 1e-12 * np.linalg.norm(fine), (c.name, cpl)


def test_assembled_is_spd_and_as_written_is_not(minv):
    """the assembled M^-1 is symmetric to 1e-12 and positive definite on all four inputs; as written it is neither on
    micro, ragged and unstructured, and nonsymmetric on strip — the figures of DESIGN §6d's table"""
    for k in SOLVER_CASES:
        Ma = minv[k, "assembled"]
        assert np.linalg.norm(Ma - Ma.T) <= 1e-12 * np.linalg.norm(Ma), k
        assert np.linalg.eigvalsh((Ma + Ma.T) / 2).min() > 0, k
        Mw = minv[k, "reference"]
        asym = np.linalg.norm(Mw - Mw.T) / np.linalg.norm(Mw)
        lo = np.linalg.eigvalsh((Mw + Mw.T) / 2).min()
        print(f"as written, {k}: asymmetry {asym:.3e}, smallest eigenvalue of the symmetric part {lo:.3e}")
        want_asym, want_lo = AS_WRITTEN[k]
        assert abs(asym - want_asym) <= 0.05 * want_asym, (k, asym)
        assert abs(lo - want_lo) <= 0.05 * abs(want_lo), (k, lo)
    assert np.linalg.norm(minv["micro", "reference"] - minv["micro", "reference"].T) > 0.1 * np.linalg.norm(minv["micro", "reference"])


def test_assembled_equals_block_formula(fem, cases, minv):
    """dense M^-1 from the statement-by-statement apply, assembled coupling == [I -A_II^-1 A_IΓ; 0 I] diag(A_II^-1, M_NN)
    [I 0; -A_ΓI A_II^-1 I]"""
    for k in ("micro", "strip"):
        want = nr.block_formula_minv(cases[k], nr.prepare(fem, cases[k]))
        got = minv[k, "assembled"]
        assert np.linalg.norm(got - want) <= 1e-11 * np.linalg.norm(want), k


def _oracle_its(orc, c, Minv):
    Ao = orc.csc_operator(c.A)
    M = orc.neumann_neumann_operator([Minv], [np.arange(c.n)], np.ones(c.n, dtype=np.int64))
    ϕ = lowest_eigvecs(Ao, c.n, len(c.A_IId) + 10)
    x0 = np.zeros(c.n)
    return orc.pcg(Ao, c.b, x0, M)[1], orc.defpcg(Ao, c.b, x0, ϕ, M)[1]


@pytest.mark.parametrize("name", SOLVER_CASES)
def test_oracle_iteration_counts(orc, cases, minv, name):
    """the oracle's pcg / defpcg with the dense restated M^-1: the counts the GPU suite's inputs were chosen by"""
    c = cases[name]
    assert _oracle_its(orc, c, minv[name, "assembled"]) == IT_ASSEMBLED[name]
    if name in IT_AS_WRITTEN:
        assert _oracle_its(orc, c, minv[name, "reference"]) == IT_AS_WRITTEN[name]


def test_edge_inputs_have_the_shapes_the_gpu_suite_needs(cases):
    """n_Γ mod 256 of the three workgroup-edge partitions; the hub of the unstructured mesh: the highest multiplicity of
    all inputs (5 of the 6 slices hold it — box partitions stop at 4) and an empty A_IΓdd column in every subdomain that
    holds it; a block with n_Γd = 0 (mod 32) and one with n_Γd = 1 (mod 32): a full
    last tile and a one-row last tile of the 32-row GEMV tile"""
    assert cases["tail1"].n_Γ % 256 == 1 and cases["full"].n_Γ % 256 == 0 and cases["short1"].n_Γ % 256 == 255
    sub = cases["unstructured"].P.sub
    cnt = np.asarray(sub.node_Γ_cnt)
    hub = int(np.argmax(cnt))
    assert int(cnt[hub]) == 5 and sub.ndom == 6
    holders = 0
    for d, g in enumerate(sub.gather_idx):
        l = np.flatnonzero(np.asarray(g) == hub)
        if l.size == 0:
            continue
        holders += 1
        per = np.diff(sp.csc_matrix(cases["unstructured"].P.A_IΓdd[d]).indptr)
        assert l.size == 1 and per[l[0]] == 0                      # an empty column: all the hub's neighbours are Γ nodes
    assert holders == 5
    nd_full = [len(g) for g in cases["tile_full"].P.sub.gather_idx]
    nd_one = [len(g) for g in cases["tile_one"].P.sub.gather_idx]
    assert any(n > 0 and n % 32 == 0 for n in nd_full), nd_full
    assert any(n % 32 == 1 for n in nd_one), nd_one
    for c in cases.values():                                       # what mi_nn_induced_create checks
        mult = np.zeros(c.n_Γ, dtype=np.int64)
        for g in c.P.sub.gather_idx:
            mult[np.asarray(g)] += 1
        assert np.array_equal(mult, np.asarray(c.P.sub.node_Γ_cnt)), c.name
        assert [a.shape for a in c.P.A_IΓdd] == [(len(p), len(g)) for p, g in zip(c.pos_I, c.P.sub.gather_idx)], c.name


def test_prepare_returns_the_pseudo_inverses(fem, cases):
    """fem.prepare_neumann_neumann_induced_precond: ΠS_d S_d ΠS_d = ΠS_d and S_d ΠS_d S_d = S_d with the dense S_d"""
    c = cases["micro"]
    P = c.P
    Sd = fem.assemble_local_schurs(P.A_IIdd, P.A_IΓdd, P.A_ΓΓdd)
    for S, B in zip(Sd, nr.prepare(fem, c)):
        assert B.shape == S.shape
        assert np.linalg.norm(B @ S @ B - B) <= 1e-7 * np.linalg.norm(B)
        assert np.linalg.norm(S @ B @ S - S) <= 1e-7 * np.linalg.norm(S)


def test_example_argument_parsing():
    """--nn-induced takes `reference` or `assembled`, is off by default, and refuses anything else; no GPU needed"""
    spec = importlib.util.spec_from_file_location("example03", os.path.join(ROOT, "examples", "example03_domain_decomposition.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    assert ex.parse_args([]).nn_induced is None and not ex.parse_args([]).lorasc
    assert ex.parse_args(["--nn-induced", "assembled", "--N", "40"]).nn_induced == "assembled"
    assert ex.parse_args(["--nn-induced", "reference"]).nn_induced == "reference"
    with pytest.raises(SystemExit):
        ex.parse_args(["--nn-induced", "textbook"])
