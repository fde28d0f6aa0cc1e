"""GPU suite (-m gpu): the outer Krylov loop computes, in every form, the bits it computed before `struct Krylov` got its one
`Loop form` (csrc/solvers.hpp select_form) and the stop rule, beta, the two start-ups, the SolveArgs entry and the publish
tail became helpers next to SolverState (csrc/kernels.hpp; k_spmv_pcg and k_gemv_pcg keep the rule written out). `it`, the whole res_norm history and x of every case of
tests/krylov_bits_cases.py (x by its SHA-256 for n > 4096; the returned vectors too for the eigCG family) are compared BIT
FOR BIT with tests/golden/krylov_parent.npz, recorded on an MI355X with the build of the commit before that change
(tests/golden/make_krylov_golden.py). The fixture also holds a SHA-256 of every case's inputs, asserted first: a mismatch
there means numpy, scipy or mi_nn_pinv built other inputs, not that a loop kernel changed.

The cases, all from tests/krylov_synth.py and tests/eig_synth.py:
  CSRFOLD   sp1025 cg and Jacobi pcg under MI355_NO_FUSED; sp8193 pcg by default
  GENERIC   sp1025 cg, Jacobi pcg and identity pcg under MI355_NO_FUSED + MI355_NO_CSRFOLD; d1025w2 pcg under MI355_NO_FUSED
            (M not diagonal); sp2048 defcg and defpcg with 5 vectors under MI355_NO_FUSED
  FUSED     sp1023 and sp2049 cg (k_fused_cg) and Jacobi pcg with maxit 0 / 1 / 2 from zero and from a random x0; d1025w2 pcg
            under MI355_NO_FOLD; nloc1024 defpcg with 5 and 65 vectors under MI355_NO_FOLD_DEFL
  FOLD      d1025w2 pcg from zero twice (the second takes k_entry_zero), from a random x0 (respec, then the general entry)
            and from zero again; nloc1024 defpcg with 5 and 21 vectors
  FOLD_BIG  big8200 pcg from zero and from a random x0
  eigCG     eigcg on synth255 (FUSED) and eigdefpcg on synth257 (always GENERIC), both one iteration past the first restart
  chunks    one pcg per form with eager launches (chunk 0) and with one-iteration replays (chunk 1)."""
import hashlib
import os

import numpy as np
import pytest

import krylov_bits_cases as cases
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def all_probs(pkg, ctx, orc):
    return cases.probs_of(pkg.api, ctx, orc)


@pytest.fixture(scope="module")
def golden(all_probs):
    g = np.load(os.path.join(GOLDEN, "krylov_parent.npz"))
    for name, h in cases.input_digests(*all_probs).items():
        assert str(g["inputs/" + name]) == h, f"{name}: inputs differ from those of the fixture (numpy / scipy / mi_nn_pinv, not a loop kernel)"
    return g


@pytest.fixture(scope="module")
def results(pkg, ctx, all_probs, golden):
    out = cases.run_all(pkg.api, ctx, *all_probs)
    assert sorted(out) == sorted(cases.NAMES)
    return out


@pytest.mark.parametrize("name", cases.NAMES)
def test_bitwise_equal_to_parent_build(results, golden, name):
    r = results[name]
    x, it, res = r[:3]
    git, gres = int(golden[name + "/it"]), golden[name + "/res"]
    print(f"{name}: it {it} (parent {git}); res_norm differs in {int(np.sum(res != gres)) if res.shape == gres.shape else -1} entries of {gres.size}")
    assert it == git
    assert res.shape == gres.shape and np.array_equal(res, gres)
    if x.size > cases.HASH_ABOVE:
        assert np.all(np.isfinite(x))
        assert hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest() == str(golden[name + "/sha256"])
    else:
        gx = golden[name + "/x"]
        print(f"{name}: x differs in {int(np.sum(x != gx)) if x.shape == gx.shape else -1} entries of {gx.size}")
        assert x.shape == gx.shape and np.array_equal(x, gx)
    if len(r) > 3:
        gV = golden[name + "/V"]
        print(f"{name}: V differs in {int(np.sum(r[3] != gV)) if r[3].shape == gV.shape else -1} entries of {gV.size}")
        assert r[3].shape == gV.shape and np.array_equal(r[3], gV)
