"""Mechanical review of the AMG bank section of julia/MI355Schur.jl, on top of tests/test_julia_shim_cpu.py: the new entry
points are bound by `ccall((:sym, lib), ...)` with Julia argument types that match the prototypes of include/mi355schur.h,
`index_base` is the literal 1, members go to C 0-based through `member0`, the new names are exported and shadow nothing of
Fem, and the view has the `\\`, `ldiv!` and solver methods of `MiAMGPreconditioner`."""
import re

import test_julia_shim_cpu as shim

NEW = {"mi_amg_bank_create", "mi_amg_bank_set_values", "mi_amg_bank_view", "mi_amg_bank_select", "mi_amg_bank_stats"}


def test_bank_ccalls_match_the_header():
    protos = shim._prototypes()
    for sym in NEW | {"mi_amg_bank_level_sizes", "mi_amg_bank_level_get", "mi_amg_bank_coarse_inverse"}:
        assert sym in protos, f"{sym} is not declared in mi355schur.h"
    calls = [c for c in shim._ccalls(shim._src()) if c[0] in NEW]
    assert {c[0] for c in calls} == NEW
    for sym, ret, jtypes, args in calls:
        ctypes_, names = protos[sym]
        assert ret == "Cint" and len(jtypes) == len(ctypes_) == len(args), f"{sym}: {len(jtypes)} Julia types, {len(args)} arguments, {len(ctypes_)} C parameters"
        for k, (ct, jt) in enumerate(zip(ctypes_, jtypes)):
            ok = next((allowed for pat, allowed in shim.C2J if re.match(pat, ct)), None)
            assert ok is not None, f"{sym}: no rule for C type '{ct}'"
            assert jt in ok, f"{sym} parameter {k} ({names[k]}): C '{ct}' bound as Julia '{jt}'"
    by = {c[0]: dict(zip(protos[c[0]][1], c[3])) for c in calls}
    create = by["mi_amg_bank_create"]
    assert create["index_base"] == "1"                                   # Julia arrays: colptr, rowval and the aggregates are 1-based
    assert create["rowptr"] == "cp" and create["colidx"] == "rv" and create["n"] == "A.n" and create["capacity"] == "capacity"
    # members are 1-based on the Julia side and 0-based in C
    assert by["mi_amg_bank_set_values"]["member"] == "member0(bank, p)"
    assert by["mi_amg_bank_select"]["members"] == "m0" and by["mi_amg_bank_select"]["view"] == "Π.op.h"
    s = shim._strip_comments_and_docstrings(shim._src())
    assert re.search(r"^member0\(bank::MiAMGBank, p::Integer\) = 1 <= p <= bank\.capacity \? Int64\(p - 1\) : throw\(BoundsError", s, flags=re.M)
    assert "m0 = Int64[member0(Π.bank, p) for p in members]" in s
    assert by["mi_amg_bank_view"]["bank"] == "bank.op.h"


def test_bank_names_and_methods():
    s = shim._strip_comments_and_docstrings(shim._src())
    defined = shim._defined_functions(s)
    new = {"MiAMGBank", "MiAMGBankView", "select!", "combine!", "amg_bank_stats"}
    assert new <= shim._exports(s) and not shim._exports(s) & shim.FEM_EXPORTS
    assert {"select!", "combine!", "set_values!", "MiAMGBank", "MiAMGBankView"} <= defined
    assert not new & shim.FEM_EXPORTS
    for kind in ("struct", "mutable struct"):
        for mm in re.finditer(rf"^{kind}\s+([A-Za-z_]\w*!?)", s, flags=re.M):
            assert mm.group(1) not in shim.FEM_EXPORTS
    assert re.search(r"^mutable struct MiAMGBank\b", s, flags=re.M) and re.search(r"^mutable struct MiAMGBankView\b", s, flags=re.M)
    assert re.search(r"^set_values!\(bank::MiAMGBank, p::Integer, A::SparseMatrixCSC\{Float64,Int\}\)", s, flags=re.M)
    # the view roots its bank: the operator's `keep`
    assert "MiAMGBankView(wrap(bank.op.ctx, r, bank), bank, max_terms)" in s
    # `\`, ldiv! and every preconditioned solver, as for MiAMGPreconditioner
    assert re.search(r"^\\\(Π::MiAMGBankView, r::Vector\{Float64\}\) = Π\.op \* r", s, flags=re.M)
    assert len(re.findall(r"^ldiv!\((?:z::Vector\{Float64\}, )?Π::MiAMGBankView", s, flags=re.M)) == 2
    for solver in ("pcg", "defpcg", "eigpcg", "eigdefpcg", "initpcg"):
        amg = re.search(rf"^{solver}\(([^)]*M::MiAMGPreconditioner[^)]*)\)", s, flags=re.M)
        bank = re.search(rf"^{solver}\(([^)]*M::MiAMGBankView[^)]*)\)", s, flags=re.M)
        assert amg and bank, solver
        assert bank.group(1) == amg.group(1).replace("MiAMGPreconditioner", "MiAMGBankView"), solver
