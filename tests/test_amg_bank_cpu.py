"""Host checks (no GPU) of the device AMG bank (`mi_amg_bank_*`, `api.AMGBank`, `api.AMGBankView`): the symbols resolve and
refuse NULL handles; the Python classes check their arguments before the library is called (a stand-in library records
every call); `bytes_per_member`'s formula of include/mi355schur.h, evaluated on `fem.prepare_amg_precond` at N = 34, against a
count done by hand here."""
import ctypes as C

import numpy as np
import pytest

import amg_refresh_ref as rr

SYMBOLS = ("mi_amg_bank_create", "mi_amg_bank_set_values", "mi_amg_bank_view", "mi_amg_bank_select", "mi_amg_bank_stats",
           "mi_amg_bank_level_get", "mi_amg_bank_coarse_inverse")


def test_symbols_exist_and_refuse_null_handles(pkg):
    L = pkg._lib
    lib = L.load()
    for name in SYMBOLS + ("mi_amg_bank_level_sizes",):
        assert getattr(lib, name) is not None and name in L.SIGNATURES
    h = C.c_void_p()
    one, v = np.zeros(1, dtype=np.int64), np.ones(1)
    ip, fp = one.ctypes.data_as(L.i64p), v.ctypes.data_as(L.f64p)
    calls = [lib.mi_amg_bank_create(None, 1, ip, ip, 1, ip, None, 1, 0, C.byref(h)),
             lib.mi_amg_bank_set_values(None, 0, C.c_void_p(v.ctypes.data)),
             lib.mi_amg_bank_view(None, 1, C.byref(h)),
             lib.mi_amg_bank_select(None, 1, ip, fp),
             lib.mi_amg_bank_stats(None, None, None, None, None, None),
             lib.mi_amg_bank_level_sizes(None, 0, None, None, None, None),
             lib.mi_amg_bank_level_get(None, 0, 0, None, None, None, None, None, None, None, None),
             lib.mi_amg_bank_coarse_inverse(None, 0, fp)]
    assert calls == [L.MI_ERR_BAD_ARG] * len(calls)
    assert len(lib.mi_last_error().decode()) > 10 and h.value is None
    assert lib.mi_amg_bank_create(None, 1, ip, ip, 1, ip, None, 0, 0, C.byref(h)) == L.MI_ERR_BAD_ARG
    assert "capacity = 0" in lib.mi_last_error().decode()


class _Recorder:
    """stands in for the loaded library: every function returns 0 and is recorded; mi_op_size answers 7"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append(name)
            if name == "mi_op_size":
                args[1]._obj.value = 7
            if name.endswith("_create") or name == "mi_amg_bank_view":
                args[-1]._obj.value = 1 + len(self.calls)
            return 0
        return f


class _Ctx:
    def __init__(self):
        self._L, self._h = _Recorder(), C.c_void_p(1)

    def _mode_for(self, *v):
        return 0

    def _order(self, *a, **k):
        pass

    _ptr = staticmethod(lambda v, n=None, writable=False: (v, C.c_void_p(v.ctypes.data)))


def test_python_checks_come_before_the_library(pkg):
    import scipy.sparse as sp
    api = pkg.api
    A = sp.diags([np.full(6, -1.0), np.full(7, 4.0), np.full(6, -1.0)], [-1, 0, 1], format="csr")
    agg = [np.array([0, 0, 0, 1, 1, 2, 2])]
    ctx = _Ctx()
    for bad in (0, -1):
        with pytest.raises(ValueError, match="capacity"):
            api.AMGBank(ctx, A, bad, aggregates=agg)
    with pytest.raises(ValueError, match="index_base"):
        api.AMGBank(ctx, A, 2, index_base=2, aggregates=agg)
    with pytest.raises(TypeError, match="aggregates"):
        api.AMGBank(ctx, A, 2, aggregates=agg, max_levels=2)
    with pytest.raises(TypeError):
        api.AMGBank(ctx, "A", 2, aggregates=agg)
    with pytest.raises(ValueError, match="square"):
        api.AMGBank(ctx, sp.csr_matrix(np.ones((2, 3))), 2, aggregates=agg)
    assert ctx._L.calls == []
    bank = api.AMGBank(ctx, A, 3, aggregates=agg)
    assert ctx._L.calls == ["mi_amg_bank_create"] and bank.capacity == 3 and bank.nnz == A.nnz and bank.n_levels == 2
    for p in (3, -1, 0.5):
        with pytest.raises(IndexError):
            bank.set_values(p, A)
    with pytest.raises(ValueError, match="stored entries"):
        bank.set_values(0, A.data[:-1])
    for bad in (0, 17, 1.5):
        with pytest.raises(ValueError, match="max_terms"):
            bank.view(bad)
    assert ctx._L.calls == ["mi_amg_bank_create"]
    view = bank.view(2)
    assert ctx._L.calls == ["mi_amg_bank_create", "mi_amg_bank_view", "mi_op_size"] and view.n == 7 and view.max_terms == 2
    seen = len(ctx._L.calls)
    with pytest.raises(ValueError, match="k = 3"):
        view.combine([0, 1, 2], [1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="k = 0"):
        view.combine([], [])
    with pytest.raises(ValueError, match="coefficients"):
        view.combine([0, 1], [1.0])
    with pytest.raises(ValueError, match="finite"):
        view.combine([0, 1], [1.0, np.nan])
    with pytest.raises(IndexError):
        view.select(3)
    with pytest.raises(IndexError):
        view.combine([0, -1], [0.5, 0.5])
    assert len(ctx._L.calls) == seen
    view.combine([2, 2], [0.5, 0.5])
    assert ctx._L.calls[seen:] == ["mi_amg_bank_select"] and list(view.members) == [2, 2]
    bank.close()                                             # the view first, then the bank
    assert ctx._L.calls[-2:] == ["mi_op_destroy", "mi_op_destroy"] and view._h is None and bank._h is None


def test_bytes_per_member_formula_matches_a_hand_count(pkg, fem):
    A0 = rr.pair(fem, 34)[0]
    H = fem.prepare_amg_precond(A0)
    assert H.nlevels >= 2
    doubles = pads = 0
    for l in range(H.nlevels):
        a = int(H.A[l].nnz)
        doubles += a; pads += a % 2                          # the values of A_l, the coarsest included
        if l < H.nlevels - 1:
            p, n = int(H.P[l].nnz), int(H.A[l].shape[0])
            doubles += p + p + n                             # P_l, R_l = P_l', ω_l / d
            pads += 2 * (p % 2) + n % 2
            doubles += 2                                     # (ω_l, g_l)
    nc = int(H.A[-1].shape[0])
    doubles += nc * nc
    pads += (nc * nc) % 2
    print(f"N = 34: levels {H.sizes}, {doubles} doubles + {pads} of padding per member = {8 * (doubles + pads)} bytes")
    assert pkg.api.amg_bank_member_bytes(H) == 8 * (doubles + pads)
    assert 8 * (doubles + pads) % 16 == 0
    # every array padded to an even count: an odd count costs exactly one double
    S = fem.amg_refresh(H.agg, A0)
    assert pkg.api.amg_bank_member_bytes(S) >= pkg.api.amg_bank_member_bytes(H)   # the structural patterns drop no entry
