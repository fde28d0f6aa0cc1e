"""CPU check of what tests/icg_cases.py claims about its `wide` case: under MI355_ICG_PIECES=256 the vector kernels of the
interior CG get pieces longer than 4 NT = 1024 rows (a thread then loads rows past the four it requests ahead of the
reduction), and under the default 512 they do not. `icg_cases.pieces` restates InteriorCg::build_fold
(csrc/operators.hpp): rows_per = max(256, ceil(n / max(256, PIECES))) on the eight XCD shares of the SpMV row blocks."""
import numpy as np

import icg_cases as cases
import sparse_synth as ss


def test_wide_has_a_piece_longer_than_four_rows_per_thread():
    s = ss.interior_sets(("wide",))["wide"]
    n = s.n_i[0]
    indptr = s.stacked().indptr
    for target, longer in ((cases.WIDE_PIECES, True), (512, False)):
        pc = cases.pieces(indptr, [0, n], target)
        rows = np.array([hi - lo for lo, hi in pc])
        print(f"MI355_ICG_PIECES={target}: {rows.size} pieces of {rows.min()} .. {rows.max()} rows")
        assert pc[0][0] == 0 and pc[-1][1] == n and all(a[1] == b[0] for a, b in zip(pc, pc[1:]))   # a partition of the rows
        assert rows.max() <= max(ss.NT, -(-n // max(256, target)))
        assert (rows.max() > 4 * ss.NT) == longer
        if longer:
            assert rows.min() > 4 * ss.NT            # every workgroup takes the path


def test_hand_made_aggregates_of_wide():
    sizes, aggs = cases.triple_aggregates(300000)
    assert sizes == [300000, 100000, 33333, 11111, 3703, 1234, 411, 137] and len(aggs) == 7
    for a, n, nc in zip(aggs, sizes, sizes[1:]):
        assert a.size == n and a[0] == 0 and a.max() == nc - 1 and np.all(np.diff(a) >= 0)
        assert np.bincount(a).min() == 3 and np.bincount(a).max() <= 5
