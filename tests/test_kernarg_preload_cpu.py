"""Kernel-argument preload (csrc/Makefile PRELOAD, gfx950): the loop kernels must take what the head of a launch
dereferences as leading plain parameters, so that the kernel descriptor asks for them in SGPRs at wave start. A struct
passed by value is never preloaded: a kernel that goes back to `DenseMeta m` as its first parameter reports 0 here.
Read from the built library by tools/kernarg_report.py (kernel descriptors only); no GPU.

A PRELOAD=0 BUILD of the library (three minutes of compilation) is not made here: the test asserts on make's dry run that
PRELOAD=0 drops the option and that the default, also under an environment CXXFLAGS, keeps it."""
import importlib.util
import os
import re
import subprocess

import pytest

from conftest import ROOT, graft

CSRC = os.path.join(ROOT, "julia-phd-krylov-spdes_amd", "csrc")
OPTION = "-amdgpu-kernarg-preload-count="


@pytest.fixture(scope="module")
def rep():
    graft.build()
    spec = importlib.util.spec_from_file_location("kernarg_report", os.path.join(ROOT, "tools", "kernarg_report.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.report()
    assert len(out) > 300 and all(size is not None for size, _ in out.values())
    return out


def pick(rep, pattern):
    return {k: v for k, v in rep.items() if re.search(pattern, k)}


def test_dense_kernels_preload_their_head(rep):
    """Every instantiation the dispatch macros of operators.hpp can select (the library holds no other):
    k_gemv_pcg: RPW 1, 2, 4 x WAVES 4, 8, 16 x FOLD_CPT 2, 3, 4, 5, 6, 8 x (PHASE 0, 1 x XCHG false, true; fp32 PHASE 1) = 270;
    k_gemv_batched: RPW x WAVES x (SCALE false, true; fp32) = 27; k_gemv_multi: SCALE false, true."""
    pcg = pick(rep, r"^_ZN2mi10k_gemv_pcgI")
    batched = pick(rep, r"^_ZN2mi14k_gemv_batchedI")
    multi = pick(rep, r"^_ZN2mi12k_gemv_multiI")
    assert (len(pcg), len(batched), len(multi)) == (270, 27, 2)
    assert sum(1 for k in pcg if re.search(r"Lb1EdE", k)) == 108 and sum(1 for k in pcg if re.search(r"Lb0EfE", k)) == 54
    for name, (size, pre) in {**pcg, **batched, **multi}.items():
        assert pre >= 4, (name, size, pre)
    # all of the 14 dwords, in fact: seven pointers (k_gemv_pcg, k_gemv_batched), five pointers, a long long and an int (multi)
    assert {pre for _, pre in pcg.values()} == {14} and {pre for _, pre in batched.values()} == {14}
    assert {pre for _, pre in multi.values()} == {13}


@pytest.mark.parametrize("kernel", ["10k_spmv_pcgE", "15k_update_xr_blkE", "9k_defl_muE", "12k_entry_zeroI", "13k_solve_end_gE"])
def test_flat_argument_loop_kernels_preload(rep, kernel):
    found = pick(rep, r"^_ZN2mi" + kernel)
    assert found, kernel
    for name, (size, pre) in found.items():
        assert pre > 0, (name, size, pre)


def make_dry_run(*args, env=None):
    e = dict(os.environ)
    e.pop("CXXFLAGS", None)
    e.update(env or {})
    return subprocess.run(["make", "-n", "-B", "-C", CSRC, *args], check=True, capture_output=True, text=True, env=e).stdout


def test_preload_variable_of_the_makefile():
    for target in ((), ("resource-usage",)):
        assert OPTION + "14" in make_dry_run(*target)
        assert OPTION not in make_dry_run("PRELOAD=0", *target)
        assert OPTION + "8" in make_dry_run("PRELOAD=8", *target)
    out = make_dry_run(env={"CXXFLAGS": "-O2 -fPIC"})
    assert OPTION + "14" in out and "-O2 -fPIC" in out
