"""Mechanical review of the full-system assembly entry of julia/MI355Schur.jl, on top of tests/test_julia_shim_cpu.py: the shim
ADDS a method to `Fem.update_isotropic_elliptic_assembly!` by its qualified name — the device operator and the plan first, so
that it cannot collide with the reference's (A_mat::SparseMatrixCSC, b_vec, cells, ...) — defines and exports no name that Fem
exports, and its calls of the new entry points, written `ccall((:sym, lib), ...)` with the C types the shim test's table knows
(the plan handle is the library's `mi_plan_t`), match the prototypes of include/mi355schur.h."""
import re

import test_julia_shim_cpu as shim

NEW = {"mi_full_assembly_plan_create", "mi_full_assembly_run", "mi_full_assembly_update", "mi_csr_set_values", "mi_diag_set_from_csr"}


def test_full_assembly_extends_fem_and_never_shadows_it():
    s = shim._strip_comments_and_docstrings(shim._src())
    defined = shim._defined_functions(s)
    assert "Fem.update_isotropic_elliptic_assembly!" in defined
    assert "update_isotropic_elliptic_assembly!" in shim.FEM_EXPORTS
    assert "update_isotropic_elliptic_assembly!" not in defined or "update_isotropic_elliptic_assembly!" in shim._imports(s).get("Fem", set())
    m = re.search(r"^function Fem\.update_isotropic_elliptic_assembly!\(([^)]*)\)", s, flags=re.M)
    assert [a.strip() for a in shim._split_top(m.group(1))][:2] == ["A_op::MiOperator", "p::MiFullAssembly"]
    assert re.search(r"^mutable struct MiFullAssembly\b", s, flags=re.M)
    assert {"MiFullAssembly", "jacobi_refresh!"} <= shim._exports(s) and not shim._exports(s) & shim.FEM_EXPORTS
    for kind in ("struct", "mutable struct", "const", "abstract type"):
        for mm in re.finditer(rf"^{kind}\s+([A-Za-z_]\w*!?)", s, flags=re.M):
            assert mm.group(1) not in shim.FEM_EXPORTS, f"{kind} {mm.group(1)} shadows Fem's export"
    # the handle dies through the plan destructor both kinds of plan share
    body = s[s.index("function MiFullAssembly(ctx::MiContext"):]
    body = body[:body.index("\nend")]
    assert "mi_assembly_plan_destroy" in body and "finalizer" in body


def test_full_assembly_ccalls_match_the_header():
    protos = shim._prototypes()
    calls = [c for c in shim._ccalls(shim._src()) if c[0] in NEW]
    assert {c[0] for c in calls} == NEW
    assert not re.search(r"@ccall[ (]\s*lib\.(%s)\(" % "|".join(NEW), shim._src())            # one spelling per section
    for sym, ret, jtypes, args in calls:
        ctypes_, names = protos[sym]
        assert ret == "Cint" and len(jtypes) == len(ctypes_) == len(args), f"{sym}: {len(jtypes)} Julia types, {len(args)} arguments, {len(ctypes_)} C parameters"
        for k, (ct, jt) in enumerate(zip(ctypes_, jtypes)):
            ok = next((allowed for pat, allowed in shim.C2J if re.match(pat, ct)), None)
            assert ok is not None, f"{sym}: no rule for C type '{ct}'"
            assert jt in ok, f"{sym} parameter {k} ({names[k]}): C '{ct}' bound as Julia '{jt}'"
    create = next(c for c in calls if c[0] == "mi_full_assembly_plan_create")
    names = protos["mi_full_assembly_plan_create"][1]
    arg = dict(zip(names, create[3]))
    assert arg["index_base"] == "1"                                     # Julia arrays: cells, colptr and rowval are 1-based
    # layouts: vertex i of every element contiguous, x row then y row; the CSC arrays of the symmetric A_mat as CSR arrays
    assert arg["cells"] == "permutedims(cells)" and arg["points"] == "permutedims(points)"
    assert arg["rowptr"] == "Vector{Int64}(A_mat.colptr)" and arg["colidx"] == "Vector{Int64}(A_mat.rowval)" and arg["n"] == "A_mat.n"
    update = next(c for c in calls if c[0] == "mi_full_assembly_update")
    arg = dict(zip(protos["mi_full_assembly_update"][1], update[3]))
    assert arg["plan"] == "p.h" and arg["A"] == "A_op.h" and arg["b"] == "b_vec"
