"""GPU suite (-m gpu): the device interior CG computes, with every `Pl`, the bits it computed before its kernels became
the four templates k_icg_init / k_icg_start / k_icg_update / k_icg_direction<IcgPl> and InteriorCg got its one `select`.
u = interior_solutions(0, b_I), its iteration count and one S-apply of every case of tests/icg_cases.py are compared BIT
FOR BIT with tests/golden/icg_parent.npz, recorded on an MI355X with the build of the commit before that change
(tests/golden/make_icg_golden.py). The fixture also holds a SHA-256 of every case's inputs, asserted first: a mismatch
there means numpy / LAPACK built other matrices, not that a kernel changed.

The cases reach lead and non-lead pieces, a zero right-hand side, an empty interior, subdomains frozen at three different
iterations (`mixed`), the stop by maxiter (`capped`), the long-row SpMV block (`longrow`), pieces longer than 4 NT rows
(`wide` under MI355_ICG_PIECES=256: the loads past the four rows a thread requests ahead of the reduction), and the AMG
`Pl` on three levels below one row block, next to an empty interior, and at row-block edges. The sequence walks one
operator through every change of `Pl` and a set_values; each step has to give what a fresh operator gave."""
import hashlib
import os

import numpy as np
import pytest

import icg_cases as cases
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(fem):
    g = np.load(os.path.join(GOLDEN, "icg_parent.npz"))
    for name, h in cases.input_digests(fem).items():
        assert str(g["inputs/" + name]) == h, f"{name}: inputs differ from those of the fixture (numpy / LAPACK, not a kernel)"
    return g


@pytest.fixture(scope="module")
def results(pkg, ctx, golden):
    out = cases.run_all(pkg.api, ctx)
    assert sorted(out) == sorted(cases.NAMES)
    return out


def same_bits(golden, name, u, it, y):
    git = int(golden[name + "/it"])
    print(f"{name}: it {it} (parent {git})")
    assert it == git
    assert np.array_equal(y, golden[name + "/y"])
    if name.startswith("wide/"):
        assert u.size == 300000 and np.all(np.isfinite(u))
        assert hashlib.sha256(np.ascontiguousarray(u).tobytes()).hexdigest() == str(golden[name + "/sha256"])
    else:
        gu = golden[name + "/u"]
        print(f"{name}: u differs in {int(np.sum(u != gu)) if u.shape == gu.shape else -1} entries of {gu.size}")
        assert u.shape == gu.shape and np.array_equal(u, gu)


@pytest.mark.parametrize("name", cases.NAMES)
def test_bitwise_equal_to_parent_build(results, golden, name):
    same_bits(golden, name, *results[name])


def test_one_operator_through_every_selection(pkg, ctx, golden):
    steps = cases.run_sequence(pkg.api, ctx)
    assert len(steps) == len(cases.SEQUENCE) - 1
    for step, want, u, it, y in steps:
        print("step", step)
        same_bits(golden, want, u, it, y)
