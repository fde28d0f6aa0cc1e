"""Mechanical review of the batched-solve section of julia/MI355Schur.jl, on top of tests/test_julia_shim_cpu.py: the new entry
points are bound by `ccall((:sym, lib), ...)` with Julia argument types that match the prototypes of include/mi355schur.h,
`index_base` is the literal 1, slots and members go to C 0-based through `slot0` / `member0`, the new names are exported and
shadow nothing of Fem."""
import re

import test_julia_shim_cpu as shim

NEW = {"mi_csr_batch_create", "mi_csr_batch_set_values", "mi_csr_batch_stats", "mi_pcg_batch"}


def test_batch_ccalls_match_the_header():
    protos = shim._prototypes()
    for sym in NEW | {"mi_csr_batch_get_values", "mi_csr_batch_stride", "mi_full_assembly_update_batch"}:
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
    create = by["mi_csr_batch_create"]
    assert create["index_base"] == "1"                                   # Julia arrays: colptr and rowval are 1-based
    assert create["rowptr"] == "cp" and create["colidx"] == "rv" and create["n"] == "A.n" and create["capacity"] == "capacity"
    # slots and members are 1-based on the Julia side and 0-based in C
    assert by["mi_csr_batch_set_values"]["slot"] == "slot0(batch, s)" and by["mi_csr_batch_set_values"]["val"] == "A.nzval"
    solve = by["mi_pcg_batch"]
    assert solve["slots"] == "s0" and solve["members"] == "m0" and solve["A_batch"] == "A.op.h" and solve["M_view"] == "M.op.h"
    assert solve["k"] == "k" and solve["ldb"] == solve["ldx"] == solve["ldres"] == "n" and solve["B"] == "B" and solve["X"] == "X"
    assert solve["it"] == "its" and solve["res_norm"] == "res" and solve["eps"] == "1e-7" and solve["maxit"] == "maxit"
    s = shim._strip_comments_and_docstrings(shim._src())
    assert re.search(r"^slot0\(batch::MiCsrBatch, s::Integer\) = 1 <= s <= batch\.capacity \? Int64\(s - 1\) : throw\(BoundsError", s, flags=re.M)
    assert "s0 = Int64[slot0(A, s) for s in slots]" in s
    assert "m0 = Int64[member0(M.bank, p) for p in members]" in s
    assert "res = Matrix{Float64}(undef, n, k)" in s and "its = zeros(Int64, k)" in s


def test_batch_names_and_methods():
    s = shim._strip_comments_and_docstrings(shim._src())
    defined = shim._defined_functions(s)
    new = {"MiCsrBatch", "pcg_batch", "csr_batch_stats"}
    assert new <= shim._exports(s) and not shim._exports(s) & shim.FEM_EXPORTS
    assert {"MiCsrBatch", "pcg_batch", "set_values!", "csr_batch_stats"} <= defined
    assert not new & shim.FEM_EXPORTS
    for kind in ("struct", "mutable struct"):
        for mm in re.finditer(rf"^{kind}\s+([A-Za-z_]\w*!?)", s, flags=re.M):
            assert mm.group(1) not in shim.FEM_EXPORTS
    assert re.search(r"^mutable struct MiCsrBatch\b", s, flags=re.M)
    assert re.search(r"^function set_values!\(batch::MiCsrBatch, s::Integer, A::SparseMatrixCSC\{Float64,Int\}\)", s, flags=re.M)
    assert re.search(r"^function pcg_batch\(A::MiCsrBatch, slots::Vector\{Int\}, B::Matrix\{Float64\}, X::Matrix\{Float64\}, M::MiAMGBankView, "
                     r"members::Vector\{Int\}; maxit=0\)", s, flags=re.M)
    # the solve returns X, the counts and one residual history per system, 1-based slices
    assert "return X, Vector{Int}(its), [res[1:its[t], t] for t in 1:k]" in s
