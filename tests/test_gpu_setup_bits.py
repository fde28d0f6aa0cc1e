"""GPU suite (-m gpu): the level elimination of csrc/setup_gj.hpp computes the bits it computed before it was cut down to its
one form (64-wide pivot blocks inverted by gj_invert_block64, the first pivot of a level in k_gj_pivot, every later one by
look-ahead in k_gj_update; one block-step loop for gj_enqueue and pinv_blocks_fast; one graph capture). Every array of every
case of tests/setup_bits_cases.py is compared BIT FOR BIT (np.array_equal; by SHA-256 plus a finiteness check above 4 096
entries) with tests/golden/setup_parent.npz, recorded on an MI355X with the build of the commit before that change
(tests/golden/make_setup_golden.py). The fixture also holds a SHA-256 of every case's inputs, asserted first: a mismatch there
means numpy or scipy built other inputs, not that a kernel changed.

The cases:
  plan/ladders          test_gpu_setup_edges.ladders() with empty_interior(5), one plan
  plan/direct-1e6       direct_inverse(n0, 1e6) for every n0 of N0S, one plan: 1, 2, 31..33 inside one pivot block, 63..65 and
                        127..129 at the block edge with a one-row trailing block, 193 and 257
  plan/direct-1e4-1e8   direct_inverse(n0, κ), n0 in (33, 64, 65, 129, 257), κ in (1e4, 1e8), one plan
      per plan and subdomain: S_d and w_d of a run with b_I; S_d of a run without (the other graph); after keep_levels(True)
      S_d, w_d and interior_solve(f); S_d and w_d of a second realization (other values) on the same plan
  pinv/full-rank, pinv/floating   mi_nn_pinv on the blocks of test_gpu_dense_edges.py at κ = 1e4, sizes 1, 2, 3, 31..33, 63..65,
                        127..129, 191, 193, 1000, 2049 as one mixed batch each (both batches of pinv_blocks_fast); the spectral
                        counter must not move
  block-jacobi          one apply of the operator of test_unequal_depth_and_single_level_blocks
  amg-coarse-inverse    mi_amg_coarse_inverse of the one-level hierarchy of the 12 x 12 mesh"""
import os

import numpy as np
import pytest

import setup_bits_cases as cases
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(fem):
    g = np.load(os.path.join(GOLDEN, "setup_parent.npz"))
    for name, h in cases.input_digests(fem).items():
        assert str(g["inputs/" + name]) == h, f"{name}: inputs differ from those of the fixture (numpy / scipy, not a kernel)"
    return g


@pytest.mark.parametrize("name", cases.NAMES)
def test_bitwise_equal_to_parent_build(pkg, ctx, fem, golden, name):
    got = cases.run_case(pkg.api, ctx, fem, name)
    want = sorted(k[len(name) + 1:].removesuffix("/sha256") for k in golden.files if k.startswith(name + "/"))
    assert sorted(got) == want
    bad = []
    for key, a in got.items():
        if a.size > cases.HASH_ABOVE:
            same = bool(np.all(np.isfinite(a))) and cases.digest(a) == str(golden[f"{name}/{key}/sha256"])
            print(f"{name}/{key}: {a.size} entries, SHA-256 {'equal' if same else 'DIFFERS (or not finite)'}")
        else:
            g = golden[f"{name}/{key}"]
            same = a.shape == g.shape and np.array_equal(a, g)
            print(f"{name}/{key}: differs in {int(np.sum(a != g)) if a.shape == g.shape else -1} entries of {g.size}")
        if not same:
            bad.append(key)
    assert not bad, f"{name}: {len(bad)} of {len(got)} arrays differ from the parent build's: {bad[:8]}"
