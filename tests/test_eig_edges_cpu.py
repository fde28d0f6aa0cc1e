"""Host assertions that tests/test_gpu_eig_edges.py relies on (no GPU): for every case of tests/eig_synth.py the oracle
really ends in the state the case is named for, so that the GPU file's parametrisation reaches the branch of
final_extraction() / restart() / eig_record() it was written for.

  * it == maxit for every stop case (eps = 1e-300: no case is ended by its tolerance); BoundsError exactly at `bounds`
    (preconditioned kinds) and nowhere else; V finite everywhere else.
  * ivec, just_restarted and the number of restarts recomputed from the stop table. The column count kept by a restart is
    rank(Y), which is 2 nvec for the short windows of the plain kinds only:
      - the deflated kinds have no coupling column, so after their first restart VtAV is block diagonal (kept Ritz values |
        new Lanczos block), the lowest eigenvectors of Tm and Tm[1:m-1, 1:m-1] are the same unit vectors and their second
        restart keeps 3 of 6 columns for (3, 8);
      - long windows keep nvec + 12..14 columns (eig_synth.LONG_NEV), and random W of 20 / 21 columns keep 2 nvec - 6.
    ivec is therefore checked as len(kept) + 1 + (iterations since the restart), and len(kept) against the table where
    the table knows it.
  * the gap condition wherever the GPU file compares subspaces: (θ_{nvec+1} - θ_nvec) / (θ_max - θ_min) >= 1e-3 on the
    projected matrix that decides the returned columns. Smallest gaps measured: c-eigdefpcg-toy 6.3e-3, e-eigdefcg-12-26-after
    3.7e-3, every stop of group a >= 7e-2. No stop had to be moved.
  * well-posedness of every compared subspace under a rounding-level perturbation of b (test_subspace_is_well_posed).
  * the oracle itself at `after` for eigcg: V'AV of the returned columns equals the Ritz values kept by the restart.
"""
import numpy as np
import pytest

import eig_synth as es


@pytest.fixture(scope="module")
def probs(orc, toy):
    return es.Problems(orc, toy)


STOP_CASES = [c for c in es.CASES if c.stop != "conv"]
CONV_CASES = [c for c in es.CASES if c.stop == "conv"]


def test_stop_table_against_the_issue_figures():
    # eigpcg(3, 8): bounds at maxit = 4; eigdefpcg with 3 vectors: at maxit = 1; (33, 70): restart 71, after 72
    assert es.stops(3, 8, False) == {"start": 1, "few": 3, "bounds": 4, "least": 5, "full": 8, "restart": 9, "after": 10,
                                     "full2": 10, "restart2": 11, "after2": 12}
    d = es.stops(3, 8, True)
    assert d["start"] == d["bounds"] == 1 and d["least"] == 2 and d["full"] == 5 and d["restart"] == 6 and d["after"] == 7
    assert (d["full2"], d["restart2"], d["after2"]) == (7, 8, 9) and "few" not in d
    long = es.stops(33, 70, False)
    assert long["restart"] == 71 and long["after"] == 72
    assert all(c.shift == 0 for c in es.CASES)                         # no stop was moved under the gap rule


def test_bounds_error_at_no_other_maxit(orc, probs):
    """eigpcg(3, 8) raises at maxit = 4 and at no other maxit in 1..16; eigdefpcg with 3 vectors at maxit = 1 only."""
    for kind, bad in (("eigpcg", 4), ("eigdefpcg", 1)):
        c = es.BY_ID[f"a-{kind}-synth257-3-8-least"]
        raised = [m for m in range(1, 17) if isinstance(probs.solve(c, maxit=m)[0], orc.BoundsError)]
        assert raised == [bad]


@pytest.mark.parametrize("case", STOP_CASES, ids=lambda c: c.id)
def test_oracle_state_at_the_stop(orc, probs, case):
    res, st = probs.solve(case)
    deflated = es.DEFLATED[case.kind]
    ivec, jr, restarts = es.expected_state(case.nvec, case.spdim, deflated, case.maxit)
    assert (st["just_restarted"], st["restarts"]) == (jr, restarts)
    if restarts == 0:
        assert st["ivec"] == ivec and st["kept"] is None
    else:
        nev = len(st["kept"])
        since = ivec - (2 * case.nvec + 1)                              # iterations since the restart
        assert st["ivec"] == nev + 1 + since
        if (case.nvec, case.spdim) in es.LONG_NEV:
            assert nev == es.LONG_NEV[(case.nvec, case.spdim)]
            assert (nev > 64) == ((case.nvec, case.spdim) == (60, 124))
        elif case.group != "e" and not (deflated and restarts > 1):
            assert nev == 2 * case.nvec
        assert nev + 1 + since <= case.spdim
    m = es.extraction_m(case.kind, case.nvec, st["ivec"], st["just_restarted"])
    want_bounds = es.PRE[case.kind] and case.stop in ("bounds", "start" if deflated else "bounds")
    if want_bounds:
        assert m == -1 and isinstance(res, orc.BoundsError)
        return
    assert not isinstance(res, Exception), res
    assert st.get("extract_m") == m
    x, it, resn, V = res
    assert it == case.maxit and resn[-1] > 0.0
    assert np.all(np.isfinite(V)) and np.all(np.isfinite(x))
    if case.stop in ("start", "few") and not deflated:
        assert int(np.count_nonzero(np.abs(V).sum(axis=0))) == case.maxit   # L + 1 Lanczos columns, zeros behind them
    if case.stop == "least" and es.PRE[case.kind]:
        assert m - 1 == case.nvec
    if case.stop in ("full", "full2") and es.PRE[case.kind] and not (deflated and restarts > 1):
        assert m == case.spdim - 1
    if case.stop == "after" and es.PRE[case.kind] and case.group == "a":
        assert m == 2 * case.nvec + 1


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: c.id)
def test_convergence_cases_end_on_their_tolerance(probs, case):
    (x, it, resn, V), st = probs.solve(case)
    n = probs.n(case.prob)
    assert it < n and resn[-1] <= 1e-7 * np.linalg.norm(probs.b(case)) and np.all(np.isfinite(V))


@pytest.mark.parametrize("case", es.CASES, ids=lambda c: c.id)
def test_gap_condition(orc, probs, case):
    res, st = probs.solve(case)
    if isinstance(res, orc.BoundsError):
        return
    T = es.decisive_T(st)
    if T is None:                                                   # Lanczos vectors (or W) come back: compared column by column
        assert st["restarts"] == 0 and "extract_m" not in st
        return
    gap = es.ritz_gap(T, case.nvec)
    print(f"{case.id}: gap {gap:.3e}")
    assert gap >= es.GAP_MIN


@pytest.mark.parametrize("case", es.CASES, ids=lambda c: c.id)
def test_subspace_is_well_posed(orc, probs, case):
    """The oracle's own returned subspace under a perturbation of b at rounding level (what a different summation order does
    to one dot product) moves by at most 1 % of the GPU file's subspace bar; `it` does not move. A case that failed this
    would measure the conditioning of its cut, not the code: unpreconditioned eigcg to convergence on matrix(257) from a
    random x0 (85 iterations, 39 restarts) moves by 5e-4 — the same case on the device differs from the oracle by 5.0e-4 —
    and is therefore run on matrix_mild(257) (3e-13)."""
    res, st = probs.solve(case)
    if isinstance(res, orc.BoundsError) or es.decisive_T(st) is None:
        return
    pert, _ = probs.solve(case, perturb=True)
    assert pert[1] == res[1]
    Q1, Q2 = np.linalg.qr(res[3])[0], np.linalg.qr(pert[3])[0]
    moved = np.linalg.norm(Q2 - Q1 @ (Q1.T @ Q2), 2)
    print(f"{case.id}: subspace moves by {moved:.3e}")
    assert moved <= es.POSED_TOL


def test_oracle_ritz_values_at_after(orc, probs):
    """eigcg stops one iteration after its first restart: the returned columns are the restart's Ritz vectors, untouched
    by that iteration. Dense numpy: V'AV = diag(kept Ritz values), V'V = I."""
    case = es.BY_ID["a-eigcg-synth257-3-8-after"]
    (x, it, resn, V), st = probs.solve(case)
    A = probs.scipy_matrix(case.prob).toarray()
    H = V.T @ A @ V
    kept = st["kept"][:case.nvec]
    assert np.allclose(np.diag(H), kept, rtol=1e-8, atol=0.0)
    assert np.abs(H - np.diag(np.diag(H))).max() <= 1e-8 * np.abs(kept).max()
    assert np.allclose(V.T @ V, np.eye(case.nvec), rtol=0, atol=1e-8)
    # and they are the lowest Ritz values of A on the Krylov space of 8 vectors: above A's own lowest eigenvalues
    assert np.all(kept >= np.linalg.eigvalsh(A)[:case.nvec] * (1 - 1e-12))


def test_nothing_to_iterate_on_the_oracle(orc):
    """b = 0, and x0 = the exact solution of a diagonal system: it = 1, x = x0, V[:, 1] = 0 / 0."""
    A, xs, b = es.diagonal_system(257)
    assert np.array_equal(A @ xs, b)
    Ao, Mo = orc.csc_operator(A), orc.jacobi_operator(A.diagonal())
    W = es.random_W(257, 3)
    for bb, xx in ((np.zeros(257), np.zeros(257)), (b, xs)):
        for kind in es.KINDS:
            try:
                with np.errstate(all="ignore"):
                    x, it, resn, V = es.run(orc, kind, Ao, Mo, bb, xx, W, 3, 8, 0, 1e-7)
            except orc.BoundsError:
                assert kind == "eigdefpcg"
                continue
            assert kind != "eigdefpcg" and it == 1 and np.array_equal(x, xx)
            col = 3 if es.DEFLATED[kind] else 0
            assert np.all(np.isfinite(V)) if es.DEFLATED[kind] else (np.all(np.isnan(V[:, col])) and np.all(V[:, 1:] == 0.0))
