"""CPU checks of the batched bank refresh's entry point (`mi_amg_bank_set_values_batch`, `AMGBank.set_values_batch`,
`get_centroidal_bank(batch=)`), in the manner of tests/test_batch_cpu.py: the symbol is declared, bound and exported, and NULL
handles or a k outside 1 .. 16 are refused with MI_ERR_BAD_ARG, the number in the message, before any handle or context is
dereferenced."""
import ctypes as C
import inspect

import numpy as np
import pytest

NEW = "mi_amg_bank_set_values_batch"


def test_new_symbol_is_declared_bound_and_exported(pkg):
    import test_abi_cpu as abi
    L = pkg._lib.load()
    assert NEW in set(abi._declared_symbols())
    assert NEW in pkg._lib.SIGNATURES and len(pkg._lib.SIGNATURES[NEW]) == 6
    assert hasattr(L, NEW)
    assert callable(getattr(pkg.api.AMGBank, "set_values_batch", None))
    sig = inspect.signature(pkg.api.AMGBank.set_values_batch)
    assert list(sig.parameters)[1:] == ["members", "batch", "slots", "strict"] and sig.parameters["strict"].default is True
    sig = inspect.signature(pkg.api.get_centroidal_bank)
    assert "batch" in sig.parameters and sig.parameters["batch"].default == 0


def test_null_handles_and_k_out_of_range_return_bad_arg(pkg):
    L = pkg._lib.load()
    BAD = pkg._lib.MI_ERR_BAD_ARG
    i64p = pkg._lib.i64p
    idx = np.zeros(17, dtype=np.int64)
    ip = idx.ctypes.data_as(i64p)
    status = (C.c_int * 17)(*([7] * 17))
    fake = C.c_void_p(1)                 # never dereferenced: k is checked before the handles are looked at
    for k in (0, 17, -3):
        for bank, batch in ((None, None), (fake, fake)):
            assert L.mi_amg_bank_set_values_batch(bank, k, ip, batch, ip, status) == BAD
            msg = L.mi_last_error()
            assert f"k = {k}".encode() in msg and b"16" in msg and b"mi_amg_bank_set_values_batch" in msg, msg
    assert L.mi_amg_bank_set_values_batch(None, 2, ip, None, ip, status) == BAD
    assert b"NULL" in L.mi_last_error() and b"mi_amg_bank_set_values_batch" in L.mi_last_error()
    assert L.mi_amg_bank_set_values_batch(None, 2, ip, None, ip, None) == BAD and b"NULL" in L.mi_last_error()
    assert list(status) == [7] * 17, "a refused call wrote a status"


def test_julia_shim_binds_the_call_with_one_based_members_and_slots():
    """in the manner of tests/test_julia_shim_batch_cpu.py"""
    import re

    import test_julia_shim_cpu as shim
    protos = shim._prototypes()
    calls = [c for c in shim._ccalls(shim._src()) if c[0] == NEW]
    assert len(calls) == 1
    sym, ret, jtypes, args = calls[0]
    ctypes_, names = protos[sym]
    assert ret == "Cint" and len(jtypes) == len(ctypes_) == len(args) == 6
    for k, (ct, jt) in enumerate(zip(ctypes_, jtypes)):
        ok = next((allowed for pat, allowed in shim.C2J if re.match(pat, ct)), None)
        assert ok is not None and jt in ok, f"parameter {k} ({names[k]}): C '{ct}' bound as Julia '{jt}'"
    by = dict(zip(names, args))
    assert by == dict(bank="bank.op.h", k="k", members="m0", A_batch="batch.op.h", slots="s0", status="status")
    s = shim._strip_comments_and_docstrings(shim._src())
    assert "m0 = Int64[member0(bank, p) for p in members]" in s and "s0 = Int64[slot0(batch, s) for s in slots]" in s
    assert re.search(r"^function set_values!\(bank::MiAMGBank, members::Vector\{Int\}, batch::MiCsrBatch, slots::Vector\{Int\}; strict::Bool=true\)",
                     s, flags=re.M)


def test_python_layer_refuses_before_the_library(pkg):
    api = pkg.api
    with pytest.raises(ValueError, match="batch = 17"):
        api.get_centroidal_bank(None, np.zeros((2, 3)), None, None, None, batch=17)
    with pytest.raises(ValueError, match="batch = -1"):
        api.get_centroidal_bank(None, np.zeros((2, 3)), None, None, None, batch=-1)
    with pytest.raises(TypeError, match="FullAssemblyPlan"):
        api.get_centroidal_bank(None, np.zeros((2, 3)), None, lambda a: a, None, batch=4)
