"""Mechanical review of the block-Jacobi entry of julia/MI355Schur.jl, on top of tests/test_julia_shim_cpu.py (whose export
lists know RecyclingKrylovSolvers and Fem only): the shim ADDS a method to `MyPreconditioners.BJPreconditioner`, neither
defines nor exports a name that MyPreconditioners exports, and its ccalls match the prototypes of include/mi355schur.h.

The export list is data taken from the reference (MyPreconditioners/MyPreconditioners.jl:8-11)."""
import re

import test_julia_shim_cpu as shim

MYPRECOND_EXPORTS = {"BJPreconditioner", "Cholesky16", "get_cholesky16", "Cholesky32", "get_cholesky32"}


def test_block_jacobi_extends_mypreconditioners_and_never_shadows_it():
    s = shim._strip_comments_and_docstrings(shim._src())
    assert re.search(r"^import MyPreconditioners\s*$", s, flags=re.M), "`import MyPreconditioners` is missing"
    imported = shim._imports(s).get("MyPreconditioners", set())
    assert imported <= MYPRECOND_EXPORTS
    defined = shim._defined_functions(s)
    assert "MyPreconditioners.BJPreconditioner" in defined                 # the qualified extension
    for name in defined:
        if "." not in name and name in MYPRECOND_EXPORTS:
            assert name in imported, f"{name} is defined without `import MyPreconditioners: {name}` (would shadow it)"
    for kind in ("struct", "mutable struct", "const", "abstract type"):
        for m in re.finditer(rf"^{kind}\s+([A-Za-z_]\w*)", s, flags=re.M):
            assert m.group(1) not in MYPRECOND_EXPORTS, f"{kind} {m.group(1)} shadows MyPreconditioners' export"
    clash = shim._exports(s) & MYPRECOND_EXPORTS
    assert not clash, f"the shim exports names MyPreconditioners exports too: {sorted(clash)}"
    # the added method takes a context first: it cannot collide with the reference's (nb::Int, A::SparseMatrixCSC)
    m = re.search(r"^function MyPreconditioners\.BJPreconditioner\(([^)]*)\)", s, flags=re.M)
    args = shim._split_top(m.group(1))
    assert args[0] == "ctx::MiContext" and args[1] == "nb::Int" and args[2].startswith("A::SparseMatrixCSC{Float64,Int}")


def test_block_jacobi_ccalls_match_the_header():
    protos = shim._prototypes()
    calls = {c[0]: c for c in shim._ccalls(shim._src()) if c[0].startswith("mi_block_jacobi_")}
    assert {"mi_block_jacobi_create", "mi_block_jacobi_set_values"} <= set(calls)
    for sym, (_, ret, jtypes, args) in calls.items():
        ctypes_, names = protos[sym]
        assert ret == "Cint" and len(jtypes) == len(ctypes_) == len(args), sym
        for k, (ct, jt) in enumerate(zip(ctypes_, jtypes)):
            ok = next((allowed for pat, allowed in shim.C2J if re.match(pat, ct)), None)
            assert ok is not None and jt in ok, f"{sym} parameter {k} ({names[k]}): C '{ct}' bound as Julia '{jt}'"
    _, _, _, args = calls["mi_block_jacobi_create"]
    names = protos["mi_block_jacobi_create"][1]
    assert args[names.index("index_base")] == "1" and args[names.index("nb")] == "nb"
    assert args[names.index("seed_ptr")] == args[names.index("seed_idx")] == "C_NULL"      # the default seed rule
