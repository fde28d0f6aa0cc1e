"""Mechanical review of the realization-sampler entry of julia/MI355Schur.jl, on top of tests/test_julia_shim_cpu.py (whose
export list stops before Fem's KL and sampler names and whose type table does not know `mi_kl_field_t`): the shim ADDS methods
to `Fem.set!`, `Fem.draw!` and `Fem.get_kl_coordinates` by their qualified names, neither defines nor exports a name that Fem
exports there, and its calls of `mi_kl_field_*` — written with `@ccall`, argument and type side by side — match the
prototypes of include/mi355schur.h.

The export names are data taken from the reference (Fem/Fem.jl:101-125)."""
import re

import test_julia_shim_cpu as shim

FEM_KL_EXPORTS = {"get_kl_coordinates", "draw", "draw!", "set!", "pll_do_global_mass_covariance_reduced_assembly", "pll_solve_local_kl",
                  "pll_compute_kl", "pll_draw", "suggest_parameters", "get_root_filename", "cov_sexp", "McSampler", "prepare_mc_sampler",
                  "McmcSampler", "prepare_mcmc_sampler", "HybridSampler", "prepare_hybrid_sampler"}

C2J = shim.C2J + [(r"^mi_kl_field_t$", {"Ptr{Cvoid}"}), (r"^mi_kl_field_t \*$", {"Ref{Ptr{Cvoid}}", "Ptr{Ptr{Cvoid}}"})]


def _at_ccalls(s):
    """(symbol, return type, [julia arg types], [arg expressions]) of every `@ccall lib.mi_...(...)::T` in the shim"""
    out = []
    for m in re.finditer(r"@ccall[ (]\s*lib\.(mi_[a-z0-9_]+)\(", s):
        i = m.end()
        depth, j = 1, i
        while depth:
            depth += {"(": 1, ")": -1}.get(s[j], 0)
            j += 1
        ret = re.match(r"::([A-Za-z]+)", s[j:])
        assert ret, f"@ccall of {m.group(1)}: no return type"
        types, args = [], []
        for part in shim._split_top(" ".join(s[i:j - 1].split())):
            expr, _, typ = part.rpartition("::")
            assert expr, f"@ccall of {m.group(1)}: argument '{part}' has no type"
            types.append(typ.strip()); args.append(expr.strip())
        out.append((m.group(1), ret.group(1), types, args))
    return out


def test_klfield_extends_fem_and_never_shadows_it():
    s = shim._strip_comments_and_docstrings(shim._src())
    assert re.search(r"^import Fem\s*$", s, flags=re.M), "`import Fem` is missing"
    imported = shim._imports(s).get("Fem", set())
    defined = shim._defined_functions(s)
    for need in ("Fem.set!", "Fem.draw!", "Fem.get_kl_coordinates"):
        assert need in defined, f"{need} gets no method"
    for name in defined:
        if "." not in name and name in FEM_KL_EXPORTS:
            assert name in imported, f"{name} is defined without `import Fem: {name}` (would shadow it)"
    for kind in ("struct", "mutable struct", "const", "abstract type"):
        for m in re.finditer(rf"^{kind}\s+([A-Za-z_]\w*!?)", s, flags=re.M):
            assert m.group(1) not in FEM_KL_EXPORTS, f"{kind} {m.group(1)} shadows Fem's export"
    clash = shim._exports(s) & FEM_KL_EXPORTS
    assert not clash, f"the shim exports names Fem exports too: {sorted(clash)}"
    assert {"MiKlField", "MiMcmcSampler"} <= shim._exports(s)
    assert re.search(r"^mutable struct MiKlField\b", s, flags=re.M) and re.search(r"^mutable struct MiMcmcSampler\b", s, flags=re.M)
    # every added method takes the handle type first: it cannot collide with the reference's (Λ, Ψ, ξ, g) / (smp::McmcSampler)
    firsts = {}
    for m in re.finditer(r"^function (Fem\.(?:set!|draw!|get_kl_coordinates))\(([^)]*)\)", s, flags=re.M):
        firsts.setdefault(m.group(1), []).append(shim._split_top(m.group(2))[0])
    assert firsts == {"Fem.set!": ["f::MiKlField", "smp::MiMcmcSampler"], "Fem.draw!": ["f::MiKlField", "smp::MiMcmcSampler"],
                      "Fem.get_kl_coordinates": ["f::MiKlField"]}
    # the sampler's draw! returns cnt
    body = s[s.index("function Fem.draw!(smp::MiMcmcSampler)"):]
    body = body[:body.index("\nend")]
    assert re.search(r"^\s*return cnt\s*$", body, flags=re.M) and "cnt += 1" in body


def test_klfield_ccalls_match_the_header():
    protos = shim._prototypes()
    calls = _at_ccalls(shim._src())
    assert {c[0] for c in calls} == {"mi_kl_field_create", "mi_kl_field_create_dd", "mi_kl_field_set", "mi_kl_field_coords", "mi_kl_field_stats",
                                     "mi_kl_field_destroy"}
    assert not [c for c in shim._ccalls(shim._src()) if c[0].startswith("mi_kl_field_")]      # one spelling per section
    for sym, ret, jtypes, args in calls:
        ctypes_, names = protos[sym]
        assert ret == "Cint" and len(jtypes) == len(ctypes_), f"{sym}: {len(jtypes)} Julia arguments for {len(ctypes_)} C parameters"
        for k, (ct, jt) in enumerate(zip(ctypes_, jtypes)):
            ok = next((allowed for pat, allowed in C2J if re.match(pat, ct)), None)
            assert ok is not None, f"{sym}: no rule for C type '{ct}'"
            assert jt in ok, f"{sym} parameter {k} ({names[k]}): C '{ct}' bound as Julia '{jt}'"
        if "index_base" in names:
            assert args[names.index("index_base")] == "1", f"{sym}: index_base must be the literal 1 for Julia arrays"
    sets = [c for c in calls if c[0] == "mi_kl_field_set"]
    names = protos["mi_kl_field_set"][1]
    assert len(sets) == 2
    nulls = sorted((c[3][names.index("G")] == "C_NULL", c[3][names.index("A")] == "C_NULL") for c in sets)
    assert nulls == [(False, True), (True, False)]                     # set! writes G only, coefficient! A only; never both NULL
    for c in sets:
        assert c[3][names.index("nreal")] == "1" and c[3][names.index("ldxi")] == "f.m" and c[3][names.index("ldg")] == "f.n"
