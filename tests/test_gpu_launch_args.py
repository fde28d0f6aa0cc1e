"""GPU suite (-m gpu): every loop kernel whose argument list was rearranged for kernel-argument preload (k_gemv_pcg in
its default, non-default, fp32, deflated and XCHG instantiations; k_gemv_batched; k_gemv_multi; k_spmv_pcg;
k_update_xr_blk; k_defl_mu; the entry and exit kernels) must compute what it computed before: x, it and res_norm are
compared BIT FOR BIT with tests/golden/launch_args_parent.npz, recorded on an MI355X with the build of the commit before
the rearrangement (tests/golden/make_launch_args_golden.py). The inputs (tests/launch_args_cases.py) are integers scaled by
powers of two, so they are the same bits wherever the test runs. A mis-wired pointer or count shows as a different
history, a fault, or a solve that does not stop; the cases are the smallest that reach every branch that reads an argument:
partial tiles and a one-row tile, W = 4, FOLD_CPT 3, nvec > 0, fp32 storage, peer exchange, a second operand panel,
x0 != 0 and the stop by maxit."""
import os

import numpy as np
import pytest

import launch_args_cases as cases
from conftest import GOLDEN

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

NAMES = ["a_folded", "b_w4r1_n700", "b_w8r4", "c_defpcg", "d_f32", "e_xchg", "f_apply_S", "f_apply_NN", "f_apply_NN32",
         "f_multi_defpcg", "g_csr3001", "g_csr9001", "h_x0", "h_maxit"]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "launch_args_parent.npz"))


@pytest.fixture(scope="module")
def results(pkg, ctx):
    out = cases.run_all(pkg.api, ctx)
    assert sorted(out) == sorted(NAMES)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_bitwise_equal_to_parent_build(results, golden, name):
    x, it, res = results[name]
    gx, git, gres = golden[name + "/x"], int(golden[name + "/it"]), golden[name + "/res_norm"]
    print(f"{name}: it {it} (parent {git}); x differs in {int(np.sum(x != gx)) if x.shape == gx.shape else -1} entries")
    assert it == git
    assert res.shape == gres.shape and np.array_equal(res, gres)
    assert x.shape == gx.shape and np.array_equal(x, gx)
    assert np.all(np.isfinite(x))
