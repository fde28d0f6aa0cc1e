"""GPU suite (-m gpu): the LORASC and the Neumann-Neumann induced operator, built on one shared interior/Γ split
(csrc/full_split_plan.hpp, csrc/full_split.hpp), must compute what they computed as two separate copies: every apply and
solve of tests/full_split_cases.py is compared BIT FOR BIT with tests/golden/full_split_parent.npz, recorded on an MI355X
with the build of the commit before the merge (tests/golden/make_full_split_golden.py). The host inputs are asserted first
(the input vectors and a SHA-256 of every case's matrices and maps), so a host that builds other inputs says so instead of
blaming the device code."""
import os

import numpy as np
import pytest

import full_split_cases as cases
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

APPLIES = [f"lorasc/{n}/nev{k}" for n, k in cases.LORASC] + [f"induced/{n}/{s}/{c}" for n, s, c in cases.INDUCED]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "full_split_parent.npz"))


@pytest.fixture(scope="module")
def host_inputs(fem, golden):
    got = cases.inputs(fem)
    assert sorted(got) == sorted(k for k in golden.files if k.startswith(("in/", "sha/")))
    for k, v in got.items():
        assert np.array_equal(v, golden[k]), f"host input {k} differs from the recorded one: the device results cannot be compared"
    return got


@pytest.fixture(scope="module")
def results(pkg, fem, ctx, host_inputs):
    return cases.run_all(pkg.api, fem, ctx)


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = got != want
    print(f"{what}: {int(np.count_nonzero(diff))} of {got.size} entries differ, max |Δ| {np.max(np.abs(got - want), initial=0.0):.3e}")
    assert np.array_equal(got, want), what
    assert np.all(np.isfinite(got))


def test_every_recorded_result_is_computed(results, golden, host_inputs):
    assert sorted(list(results) + list(host_inputs)) == sorted(golden.files)
    assert len(APPLIES) == 8 + 6 + 12


@pytest.mark.parametrize("key", APPLIES)
def test_apply_bitwise_equal_to_parent_build(results, golden, key):
    same_bits(results[key], golden[key], key)


@pytest.mark.parametrize("kind", ["lorasc", "induced"])
def test_solve_bitwise_equal_to_parent_build(results, golden, kind):
    it, git = int(results[f"solve/{kind}/it"]), int(golden[f"solve/{kind}/it"])
    print(f"solve/{kind}: it {it} (parent {git})")
    assert it == git and it > 0
    same_bits(results[f"solve/{kind}/res_norm"], golden[f"solve/{kind}/res_norm"], f"solve/{kind}/res_norm")
    same_bits(results[f"solve/{kind}/x"], golden[f"solve/{kind}/x"], f"solve/{kind}/x")
