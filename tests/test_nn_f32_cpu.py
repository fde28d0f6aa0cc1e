"""CPU suite: the fp32-stored Neumann-Neumann preconditioner (`mi_nn_create_stored`, MI_STORE_F32) as far as it can be
checked without a GPU: the ABI surface, the refusals that need no device, the Python keyword, the file name of the
iteration counts, and — with the oracle alone — that on the problems the GPU suite uses the *semantics* (blocks rounded
once to fp32, everything else fp64) keep the iteration count of the fp64 preconditioner."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def rounded(blocks):
    return [np.asfortranarray(B.astype(np.float32).astype(np.float64)) for B in blocks]


def test_symbols_declared_bound_and_exported(pkg):
    text = open(os.path.join(ROOT, "include", "mi355schur.h")).read()
    assert re.search(r"#define\s+MI_STORE_F64\s+0\b", text) and re.search(r"#define\s+MI_STORE_F32\s+1\b", text)
    decl = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    import __graft_entry__ as graft
    graft.build()
    L = C.CDLL(pkg._lib.LIB_PATH)
    for name in ("mi_nn_create_stored", "mi_op_storage"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", decl), name
        assert name in pkg._lib.SIGNATURES and hasattr(L, name), name
    # mi_nn_create's arguments, then `int storage`, then the result
    assert pkg._lib.SIGNATURES["mi_nn_create_stored"][:-2] == pkg._lib.SIGNATURES["mi_nn_create"][:-1]
    assert pkg._lib.SIGNATURES["mi_nn_create_stored"][-2] is C.c_int
    # the comment names the precedent and says how this differs from it
    assert "CholPreconditioners.jl:32-56" in text and "EPDD.jl:1111-1137" in text


def test_bad_arguments_without_a_gpu(pkg):
    L = pkg._lib.load()
    BAD = pkg._lib.MI_ERR_BAD_ARG
    h = C.c_void_p(1)
    for storage in (0, 1):
        assert L.mi_nn_create_stored(None, 1, 1, None, None, None, None, 0, 0, 1, storage, C.byref(h)) == BAD
        assert h.value is None                                   # no operator
        assert L.mi_nn_create_stored(None, 1, 1, None, None, None, None, 0, 0, 1, storage, None) == BAD
    for storage in (7, -1, 2):
        h = C.c_void_p(1)
        assert L.mi_nn_create_stored(None, 1, 1, None, None, None, None, 0, 0, 1, storage, C.byref(h)) == BAD
        assert h.value is None and b"storage" in L.mi_last_error()
    s = C.c_int(-5)
    assert L.mi_op_storage(None, C.byref(s)) == BAD and L.mi_op_storage(None, None) == BAD
    assert s.value == -5


def test_python_keyword_is_validated_before_any_device_call(pkg):
    api = pkg.api
    import inspect
    sig = inspect.signature(api.NeumannNeumannSchurPreconditioner.__init__)
    assert sig.parameters["storage"].default == "f64"
    assert isinstance(api.NeumannNeumannSchurPreconditioner.storage, property)
    for bad in ("f16", np.float16, 32, None):
        with pytest.raises(ValueError):
            api.NeumannNeumannSchurPreconditioner(None, [], [], [], storage=bad)
    assert "storage" not in inspect.signature(api.LocalSchurs.__init__).parameters    # S_d stays fp64: not expressible


def test_pcg_iters_file_name(pkg, tmp_path):
    io = pkg.io
    path = io.save_pcg_iters([5, 6, 7], "cov", 8, "static", 3, data_dir=str(tmp_path), precond="neumann-neumann-f32")
    assert os.path.basename(path) == "cov.neumann-neumann-f32_ndom8_static.pcg-iters.nreals3.npz"
    assert os.path.exists(path)
    # the existing names are unchanged
    assert os.path.basename(io.save_pcg_iters([5], "cov", 8, "static", 1, data_dir=str(tmp_path))) == \
        "cov.neumann-neumann_ndom8_static.pcg-iters.nreals1.npz"


@pytest.mark.parametrize("case,it_want", [("micro", 5), ("toy", 6), ("ragged", 10)])
def test_oracle_rounded_blocks_keep_the_iteration_count(orc, request, case, it_want):
    """The reference semantics alone: pcg with ΠS_d rounded through float32 (handed back as fp64) takes as many iterations
    as with the fp64 blocks, and arrives at the same solution. These are the inputs of tests/test_gpu_nn_f32.py."""
    P = request.getfixturevalue(case)
    sub = P.sub
    So = orc.apply_local_schurs_operator(P.Sd, sub.gather_idx, sub.n_Γ)
    M64 = orc.neumann_neumann_operator(P.ΠSd, sub.gather_idx, sub.node_Γ_cnt)
    M32 = orc.neumann_neumann_operator(rounded(P.ΠSd), sub.gather_idx, sub.node_Γ_cnt)
    x0 = np.zeros(sub.n_Γ)
    x64, it64, _ = orc.pcg(So, P.b_schur, x0, M64)
    x32, it32, _ = orc.pcg(So, P.b_schur, x0, M32)
    print(f"{case}: n_Γ={sub.n_Γ} it64={it64} it32={it32} |x32-x64|/|x64|={np.linalg.norm(x32 - x64) / np.linalg.norm(x64):.1e}")
    assert it64 == it_want and it32 == it64
    assert np.linalg.norm(x32 - x64) <= 1e-6 * np.linalg.norm(x64)
    # rounding a symmetric block element-wise keeps it symmetric, and fp32's range is nowhere near
    for B, R in zip(P.ΠSd, rounded(P.ΠSd)):
        assert np.array_equal(R, R.T) or not np.array_equal(B, B.T)
        assert np.all(np.isfinite(R)) and np.abs(B).max() < 1e30
