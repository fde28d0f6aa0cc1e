"""CPU checks of the batched PCG's entry points (`mi_csr_batch_*`, `mi_full_assembly_update_batch`, `mi_pcg_batch`): NULL or
invalid arguments are refused with MI_ERR_BAD_ARG before any device is touched, in the style of
tests/test_abi_cpu.py::test_null_arguments_return_bad_arg, and the slot stride is the padded one."""
import ctypes as C

import numpy as np
import pytest

NEW = ("mi_csr_batch_create", "mi_csr_batch_set_values", "mi_csr_batch_get_values", "mi_csr_batch_stats", "mi_csr_batch_stride",
       "mi_full_assembly_update_batch", "mi_pcg_batch")


def test_new_symbols_are_declared_bound_and_exported(pkg):
    import test_abi_cpu as abi
    L = pkg._lib.load()
    declared = set(abi._declared_symbols())
    for sym in NEW:
        assert sym in pkg._lib.SIGNATURES, sym
        assert hasattr(L, sym), sym
        assert sym in declared, sym
    for name in ("CsrBatch", "pcg_batch", "csr_batch_slot_bytes", "CSR_BATCH_MAX"):
        assert hasattr(pkg.api, name), name
    assert hasattr(pkg.api.FullAssemblyPlan, "update_batch")
    assert pkg.api.CSR_BATCH_MAX == pkg.api.AMG_BANK_MAX_TERMS == 16


def test_null_and_invalid_arguments_return_bad_arg(pkg):
    L = pkg._lib.load()
    BAD = pkg._lib.MI_ERR_BAD_ARG
    i64p, f64p = pkg._lib.i64p, pkg._lib.f64p
    h = C.c_void_p()
    ptr = np.array([0, 1, 2], dtype=np.int64).ctypes.data_as(i64p)
    idx = np.array([0, 1], dtype=np.int64).ctypes.data_as(i64p)
    val = np.ones(2)
    vp = C.c_void_p(val.ctypes.data)
    fake_ctx = C.c_void_p(1)             # never dereferenced: every call below is refused on an argument checked before the context is used
    assert L.mi_csr_batch_create(None, 2, ptr, idx, 1, 0, C.byref(h)) == BAD and b"NULL" in L.mi_last_error()
    assert L.mi_csr_batch_create(fake_ctx, 2, ptr, idx, 1, 0, None) == BAD
    assert L.mi_csr_batch_create(fake_ctx, 2, None, idx, 1, 0, C.byref(h)) == BAD
    assert L.mi_csr_batch_create(fake_ctx, 2, ptr, None, 1, 0, C.byref(h)) == BAD
    assert L.mi_csr_batch_create(fake_ctx, 0, ptr, idx, 1, 0, C.byref(h)) == BAD and b"n = 0" in L.mi_last_error()
    assert L.mi_csr_batch_create(fake_ctx, 2, ptr, idx, 0, 0, C.byref(h)) == BAD and b"capacity = 0" in L.mi_last_error()
    assert L.mi_csr_batch_create(fake_ctx, 2, ptr, idx, -2, 0, C.byref(h)) == BAD and b"capacity = -2" in L.mi_last_error()
    assert L.mi_csr_batch_create(fake_ctx, 2, ptr, idx, 1, 2, C.byref(h)) == BAD and b"index_base = 2" in L.mi_last_error()
    assert not h.value
    assert L.mi_csr_batch_set_values(None, 0, vp) == BAD and b"NULL" in L.mi_last_error()
    assert L.mi_csr_batch_get_values(None, 0, vp) == BAD and b"NULL" in L.mi_last_error()
    assert L.mi_csr_batch_stats(None, None, None, None, None) == BAD and b"NULL" in L.mi_last_error()
    assert L.mi_full_assembly_update_batch(None, vp, None, 0, vp) == BAD and b"NULL" in L.mi_last_error()
    it = np.zeros(2, dtype=np.int64)
    sl = np.zeros(2, dtype=np.int64)
    assert L.mi_pcg_batch(None, 2, sl.ctypes.data_as(i64p), None, None, vp, 2, vp, 2, 0, 1e-7, None, 0, it.ctypes.data_as(i64p)) == BAD
    assert b"NULL" in L.mi_last_error() and b"mi_pcg_batch" in L.mi_last_error()
    d = C.c_int64()
    assert L.mi_csr_batch_stride(-1, C.byref(d)) == BAD and L.mi_csr_batch_stride(3, None) == BAD


@pytest.mark.parametrize("nnz", [0, 1, 2, 3, 4, 1023, 1024, 7 * 1024 + 1, 2 ** 31 - 2, 2 ** 31 - 1])
def test_padded_stride(pkg, nnz):
    """bytes_per_slot = 8 (nnz + nnz mod 2): every slot starts on a 16-byte boundary"""
    L = pkg._lib.load()
    d = C.c_int64(-1)
    assert L.mi_csr_batch_stride(nnz, C.byref(d)) == 0
    assert d.value == nnz + nnz % 2 and d.value % 2 == 0 and 0 <= d.value - nnz <= 1
    assert pkg.api.csr_batch_slot_bytes(nnz) == 8 * (nnz + nnz % 2) and pkg.api.csr_batch_slot_bytes(nnz) % 16 == 0


def test_python_layer_refuses_before_the_library(pkg):
    api = pkg.api
    with pytest.raises(ValueError, match="capacity = 0"):
        api.CsrBatch(None, np.eye(3), 0)
    with pytest.raises(ValueError, match="index_base"):
        api.CsrBatch(None, np.eye(3), 1, index_base=2)
    with pytest.raises(TypeError):
        api.CsrBatch(None, [[1.0]], 1)
    with pytest.raises(ValueError, match="square"):
        api.CsrBatch(None, np.ones((2, 3)), 1)
